"""Extension terms of the trajectory-terms pass (qc_terms_create_ext): smoothness, pairwise and linear slack cost.
CPU: the numpy restatement (terms_ext_reference.py) certified by complex step and finite differences, descriptor validation and
Hessian structure without a device, the ctypes / C / Julia mirrors of qc_terms_ext.  GPU: every output of the kernel against
the restatement, NaN-poisoned buffers with a guard block, bit-identical repeats and host / device entries, and an empty
extension equal to qc_terms_create bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import terms_ext_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_case(qc, T=9, free=True, dt_scaled=True, global_dim=0, baseline=False, seed=0):
    """A trajectory with components u, v, w (4 entries each: u is in a regulariser, a smoothness term and two edges at once),
    controls a (2), slacks s1_u / s2_u (3) and an optional free timestep; the terms both as a spec and as the restatement."""
    rng = np.random.default_rng(seed)
    comps = {"u": rng.standard_normal((4, T)), "v": rng.standard_normal((4, T)), "w": rng.standard_normal((4, T)),
             "a": rng.standard_normal((2, T)), "s1_u": rng.uniform(0, 1, (3, T)), "s2_u": rng.uniform(0, 1, (3, T))}
    if free:
        comps["Δt"] = rng.uniform(0.1, 0.3, (1, T))
    gd = {"g": rng.standard_normal(global_dim)} if global_dim else None
    traj = qc.NamedTrajectory(comps, controls=("a", "s1_u", "s2_u"), timestep="Δt" if free else 0.17, global_data=gd)
    Ra = rng.uniform(0.5, 2.0, 2)
    base = rng.standard_normal((2, T)) if baseline else None
    Su = rng.uniform(0.5, 3.0, 4)
    Q = [1.5, 0.7]
    spec = (qc.QuadraticRegularizer("a", traj, Ra, baseline=base) + qc.QuadraticRegularizer("u", traj, 0.3)
            + qc.QuadraticSmoothnessRegularizer("u", traj, Su) + qc.QuadraticSmoothnessRegularizer("a", traj, 0.4)
            + qc.PairwiseQuadraticRegularizer(traj, Q, [("u", "v"), ("w", "u")]) + qc.L1Regularizer("u", traj, 0.1))
    if free:
        spec = spec + qc.MinimumTimeObjective(traj, 0.8)
    c = traj.components
    ua, aa = np.asarray(c["u"]), np.asarray(c["a"])
    reg = np.concatenate([ua, aa])
    R = np.concatenate([np.full(4, 0.3), Ra])
    o = np.argsort(reg)
    bl = None
    if baseline:
        bl = np.zeros((T, 6))
        bl[:, 4:] = base.T
        bl = bl[:, o]
    sidx = np.concatenate([ua, aa])
    sR = np.concatenate([Su, np.full(2, 0.4)])
    so = np.argsort(sidx)
    lidx = np.concatenate([np.asarray(c["s1_u"]), np.asarray(c["s2_u"])])
    tm = ref.TermsExt(T=T, zdim=traj.dim, off_dt=traj.offset("Δt") if free else -1, dt_fixed=0.0 if free else 0.17, global_dim=global_dim,
                      dt_scaled=dt_scaled, reg_index=reg[o], reg_R=R[o], baseline=bl, D=0.8 if free else 0.0, n_mt=T - 1 if free else 0,
                      s_index=sidx[so], s_R=sR[so], p_a=np.concatenate([ua, np.asarray(c["w"])]),
                      p_b=np.concatenate([np.asarray(c["v"]), ua]), p_Q=np.repeat(Q, 4), l_index=lidx, l_w=np.full(6, 0.1))
    Z = np.concatenate([traj.datavec[:T * traj.dim], rng.standard_normal(global_dim)])
    return traj, spec, tm, Z


def ext_struct(qc, tm, keep, baseline=False):
    """qc_terms_desc + qc_terms_ext of the restatement (arrays kept alive in `keep`).  `baseline=True` also passes
    tm.baseline as reg_baseline; by default the descriptor carries none."""
    L = qc._lib
    arr = lambda a, dt: keep.append(np.ascontiguousarray(a, dtype=dt)) or keep[-1]
    d = L.qc_terms_desc()
    d.T, d.zdim, d.off_dt, d.global_dim, d.dt_fixed = tm.T, tm.zdim, tm.off_dt, tm.global_dim, tm.dt_fixed
    ri, rR = arr(tm.reg_index, np.int32), arr(tm.reg_R, np.float64)
    d.n_reg = ri.size
    d.weighting = L.QC_REG_DT_SCALED if tm.dt_scaled else L.QC_REG_PLAIN
    d.reg_index = ri.ctypes.data_as(C.POINTER(C.c_int32))
    d.reg_R = L.dptr(rR)
    if baseline and tm.baseline is not None:
        d.reg_baseline = L.dptr(arr(tm.baseline, np.float64))      # (T, n_reg), entry-fastest
    d.min_time_D, d.min_time_knots = tm.D, tm.n_mt
    x = L.qc_terms_ext()
    ip = lambda a: arr(a, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    x.n_smooth, x.n_pair, x.n_lin = len(tm.s_index), len(tm.p_a), len(tm.l_index)
    x.smooth_index, x.smooth_R = ip(tm.s_index), L.dptr(arr(tm.s_R, np.float64))
    x.pair_a, x.pair_b, x.pair_Q = ip(tm.p_a), ip(tm.p_b), L.dptr(arr(tm.p_Q, np.float64))
    x.lin_index, x.lin_w = ip(tm.l_index), L.dptr(arr(tm.l_w, np.float64))
    return d, x


# ---------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("T,free,dt_scaled,global_dim,baseline", [(1, True, True, 0, False), (2, True, True, 2, True), (3, False, True, 0, False),
                                                                  (4, True, False, 1, False), (3, False, False, 0, True)])
def test_reference_derivatives(qc, T, free, dt_scaled, global_dim, baseline):
    traj, spec, tm, Z = make_case(qc, T=T, free=free, dt_scaled=dt_scaled, global_dim=global_dim, baseline=baseline, seed=T)
    g = ref.grad(tm, Z)
    eps = 1e-30
    gcs = np.array([np.imag(ref.value(tm, Z.astype(complex) + 1j * eps * e)) / eps for e in np.eye(Z.size)])
    np.testing.assert_allclose(g, gcs, rtol=1e-13, atol=1e-14)
    H = ref.hess_dense(tm, Z)
    h = 1e-6
    Hfd = np.array([(ref.grad(tm, Z + h * e) - ref.grad(tm, Z - h * e)) / (2 * h) for e in np.eye(Z.size)])
    np.testing.assert_allclose(H, Hfd, rtol=1e-7, atol=1e-7)
    r, c = ref.hess_structure(tm)
    assert np.all(r <= c) and r.size == ref.hess_nnz(tm)


def test_smoothness_known_answers(qc):
    traj, spec, tm, Z = make_case(qc, T=5)
    only = ref.TermsExt(T=5, zdim=tm.zdim, s_index=tm.s_index[:1], s_R=np.array([2.0]))
    X = np.zeros((5, tm.zdim))
    X[:, tm.s_index[0]] = [0.0, 1.0, 3.0, 3.0, 2.0]           # differences 1, 2, 0, -1
    assert ref.value(only, X.ravel()) == 0.5 * 2.0 * (1 + 4 + 0 + 1)
    assert ref.value(ref.TermsExt(T=1, zdim=tm.zdim, s_index=tm.s_index, s_R=tm.s_R), Z[:tm.zdim]) == 0.0


def test_structure_host_entry_points(qc):
    """No device: nnz and structure of the extended descriptor equal the restatement, and the regulariser layout is a prefix."""
    L = qc._lib
    for T, free, dt_scaled in ((1, True, True), (4, True, True), (3, False, True), (5, True, False)):
        traj, spec, tm, Z = make_case(qc, T=T, free=free, dt_scaled=dt_scaled)
        keep = []
        d, x = ext_struct(qc, tm, keep)
        nnz, nnz0 = C.c_int64(), C.c_int64()
        assert L.lib.qc_terms_desc_ext_hess_nnz(C.byref(d), C.byref(x), C.byref(nnz)) == 0
        assert L.lib.qc_terms_desc_hess_nnz(C.byref(d), C.byref(nnz0)) == 0
        assert nnz.value == ref.hess_nnz(tm) > nnz0.value
        r0, c0 = ref.hess_structure(tm)
        for one_based in (0, 1):
            r = np.full(nnz.value, -7, dtype=np.int64)
            c = np.full(nnz.value, -7, dtype=np.int64)
            assert L.lib.qc_terms_desc_ext_hess_structure(C.byref(d), C.byref(x), L.iptr(r), L.iptr(c), one_based) == 0
            np.testing.assert_array_equal(r, r0 + one_based)
            np.testing.assert_array_equal(c, c0 + one_based)
            assert np.all(r <= c)
            rp = np.empty(nnz0.value, dtype=np.int64)
            cp = np.empty(nnz0.value, dtype=np.int64)
            L.lib.qc_terms_desc_hess_structure(C.byref(d), L.iptr(rp), L.iptr(cp), one_based)
            np.testing.assert_array_equal(r[:nnz0.value], rp)
            np.testing.assert_array_equal(c[:nnz0.value], cp)
        # NULL and all-empty extensions: the plain descriptor
        for xe in (None, C.byref(L.qc_terms_ext())):
            assert L.lib.qc_terms_desc_ext_hess_nnz(C.byref(d), xe, C.byref(nnz)) == 0 and nnz.value == nnz0.value


def test_validation_without_a_device(qc):
    L = qc._lib
    traj, spec, tm, Z = make_case(qc, T=4)
    nnz = C.c_int64()
    h = C.c_void_p()

    def refused(mutate):
        keep = []
        d, x = ext_struct(qc, tm, keep)
        mutate(x, keep)
        assert L.lib.qc_terms_desc_ext_hess_nnz(C.byref(d), C.byref(x), C.byref(nnz)) == L.QC_ERR_INVALID
        msg = L.lib.qc_terms_last_error(None).decode()
        assert msg.startswith("qc_terms_ext"), msg
        assert L.lib.qc_terms_create_ext(C.byref(d), C.byref(x), C.byref(h)) == L.QC_ERR_INVALID and not h.value
        return msg

    def set_idx(field, k, v):
        def m(x, keep):
            a = np.ctypeslib.as_array(getattr(x, field), shape=(k + 1,))
            a[k] = v
        return m
    off_dt, zdim = tm.off_dt, tm.zdim
    for field in ("smooth_index", "lin_index", "pair_a", "pair_b"):
        assert "outside" in refused(set_idx(field, 1, zdim))
        assert "outside" in refused(set_idx(field, 0, -1))
        assert "outside" in refused(set_idx(field, 2, off_dt))
    assert "pair_a[p] == pair_b[p]" in refused(set_idx("pair_b", 3, int(tm.p_a[3])))
    assert "repeated" in refused(set_idx("smooth_index", 1, int(tm.s_index[0])))
    assert "repeated" in refused(set_idx("lin_index", 4, int(tm.l_index[2])))
    for cnt in ("n_smooth", "n_pair", "n_lin"):
        assert "negative" in refused(lambda x, keep, cnt=cnt: setattr(x, cnt, -1))
    for arr in ("smooth_index", "smooth_R", "pair_a", "pair_b", "pair_Q", "lin_index", "lin_w"):
        assert "NULL" in refused(lambda x, keep, arr=arr: setattr(x, arr, None))
    # NULL arrays behind zero counts are fine
    keep = []
    d, x = ext_struct(qc, tm, keep)
    x.n_lin, x.lin_index, x.lin_w = 0, None, None
    assert L.lib.qc_terms_desc_ext_hess_nnz(C.byref(d), C.byref(x), C.byref(nnz)) == 0


def test_host_layer_terms(qc):
    """Slack names, the edges flattened into pairs, and the host-side errors of the description classes."""
    traj, spec, tm, Z = make_case(qc, T=3)
    assert qc.slack_names("Ũ⃗") == ("s1_Ũ⃗", "s2_Ũ⃗")
    pw = qc.PairwiseQuadraticRegularizer(traj, [1.5, 0.7], [("u", "v"), ("w", "u")])
    a, b, Q = pw.pairs(traj)
    np.testing.assert_array_equal(a, tm.p_a)
    np.testing.assert_array_equal(b, tm.p_b)
    np.testing.assert_array_equal(Q, tm.p_Q)
    with pytest.raises(ValueError):
        qc.PairwiseQuadraticRegularizer(traj, 1.0, [("u", "a")])          # lengths differ
    with pytest.raises(ValueError):
        qc.PairwiseQuadraticRegularizer(traj, [1.0, 2.0], [("u", "v")])   # one Q per edge
    with pytest.raises(ValueError):
        qc.QuadraticSmoothnessRegularizer("u", traj, [1.0, 2.0])


def test_mirrors_of_the_extension_struct(qc, tmp_path):
    """qc_terms_ext: ctypes size = the library's qc_sizeof_terms_ext = C's sizeof, offsets agree, and the Julia mirror lists the
    same fields in the same order with the same types."""
    L = qc._lib
    assert L.lib.qc_sizeof_terms_ext() == C.sizeof(L.qc_terms_ext) == 88
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "qcolloc.h"\n'
                   'int main(){printf("%zu %zu %zu %zu\\n", sizeof(qc_terms_ext), offsetof(qc_terms_ext, smooth_index), '
                   'offsetof(qc_terms_ext, lin_w), offsetof(qc_terms_ext, reserved1));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    X = L.qc_terms_ext
    assert got == [C.sizeof(X), X.smooth_index.offset, X.lin_w.offset, X.reserved1.offset]
    txt = open(os.path.join(ROOT, "julia", "QCollocHIP.jl"), encoding="utf-8").read()
    body = re.search(r"^struct QCTermsExt\n(.*?)^end", txt, flags=re.S | re.M).group(1)
    body = re.sub(r"#[^\n]*", "", body)
    jf = [tuple(x.strip() for x in decl.split("::")) for decl in re.split(r"[;\n]", body) if decl.strip()]
    assert [f for f, _ in jf] == [f for f, _ in X._fields_]
    tmap = {"Int32": C.c_int32, "Int64": C.c_int64, "Float64": C.c_double}
    for (fname, jt), (_, ct) in zip(jf, X._fields_):
        if jt.startswith("Ptr{"):
            assert issubclass(ct, C._Pointer), fname
        elif jt.startswith("NTuple{"):
            n, e = jt[len("NTuple{"):-1].split(",")
            assert C.sizeof(ct) == int(n) * C.sizeof(tmap[e.strip()]), fname
        else:
            assert tmap[jt] is ct, fname


# ---------------------------------------------------------------------------------------------------------------- GPU
GPU_CASES = [(1, True, True, 0, False), (1, False, False, 3, False), (2, True, True, 2, True), (2, False, True, 0, False),
             (3, True, False, 0, False), (3, False, True, 1, True), (257, True, True, 5, False), (257, False, False, 0, True),
             (1000, True, True, 2, True), (1000, False, True, 0, False), (1000, True, False, 1, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("T,free,dt_scaled,global_dim,baseline", GPU_CASES)
def test_kernel_matches_reference(qc, T, free, dt_scaled, global_dim, baseline):
    import torch
    traj, spec, tm, Z = make_case(qc, T=T, free=free, dt_scaled=dt_scaled, global_dim=global_dim, baseline=baseline, seed=T + 7)
    obj = qc.TrajectoryObjective(spec, traj, dt_scaled=dt_scaled)
    assert obj.has_ext and obj.hess_nnz == ref.hess_nnz(tm)
    r0, c0 = ref.hess_structure(tm)
    np.testing.assert_array_equal(obj.hess_structure[0], r0)
    np.testing.assert_array_equal(obj.hess_structure[1], c0)
    J, g, H = obj.L_grad_hess(Z)
    Jr = ref.value(tm, Z)
    assert abs(J - Jr) <= 1e-12 * max(1.0, abs(Jr))
    gr = ref.grad(tm, Z)
    np.testing.assert_allclose(g, gr, rtol=1e-12, atol=1e-13)          # every entry: zeros and the global tail included
    assert np.all(g[T * tm.zdim:] == 0.0) and np.all(g[gr == 0.0] == 0.0)
    np.testing.assert_allclose(H, ref.hess_values(tm, Z), rtol=1e-12, atol=1e-13)
    if T <= 50:
        np.testing.assert_allclose(qc_dense(obj, H, Z.size), ref.hess_dense(tm, Z), rtol=1e-12, atol=1e-13)
    # repeated calls and the device entry are bit-identical; NaN-poisoned outputs are written in range, the guard stays NaN
    J2, g2, H2 = obj.L_grad_hess(Z)
    assert J2 == J and g2.tobytes() == g.tobytes() and H2.tobytes() == H.tobytes()
    guard = 64
    dZ = torch.from_numpy(Z).cuda()
    dJ = torch.full((1 + guard,), float("nan"), dtype=torch.float64, device="cuda")
    dg = torch.full((Z.size + guard,), float("nan"), dtype=torch.float64, device="cuda")
    dH = torch.full((obj.hess_nnz + guard,), float("nan"), dtype=torch.float64, device="cuda")
    obj.eval_device(dZ, dJ, dg, dH)
    torch.cuda.synchronize()
    hJ, hg, hH = dJ.cpu().numpy(), dg.cpu().numpy(), dH.cpu().numpy()
    assert hJ[0] == J and np.isnan(hJ[1:]).all()
    assert hg[:Z.size].tobytes() == g.tobytes() and np.isnan(hg[Z.size:]).all()
    assert hH[:obj.hess_nnz].tobytes() == H.tobytes() and np.isnan(hH[obj.hess_nnz:]).all()
    obj.close()


def qc_dense(obj, vals, n):
    r, c = obj.hess_structure
    M = np.zeros((n, n))
    np.add.at(M, (r, c), vals)
    return np.triu(M) + np.triu(M, 1).T


@pytest.mark.gpu
@pytest.mark.parametrize("free,dt_scaled", [(True, True), (False, False)])
def test_empty_extension_equals_plain_handle(qc, free, dt_scaled):
    """NULL and all-empty extensions make the handle qc_terms_create makes: same structure, bit-identical J, gradient, Hessian."""
    L = qc._lib
    traj, spec, tm, Z = make_case(qc, T=300, free=free, dt_scaled=dt_scaled, global_dim=2, seed=3)
    plain = ref.TermsExt(**{**tm.__dict__, "s_index": ref._i(None), "s_R": ref._f(None), "p_a": ref._i(None), "p_b": ref._i(None),
                            "p_Q": ref._f(None), "l_index": ref._i(None), "l_w": ref._f(None)})
    keep = []
    d, _ = ext_struct(qc, plain, keep)
    outs = []
    for mode in ("plain", "null", "empty"):
        h = C.c_void_p()
        if mode == "plain":
            rc = L.lib.qc_terms_create(C.byref(d), C.byref(h))
        else:
            rc = L.lib.qc_terms_create_ext(C.byref(d), None if mode == "null" else C.byref(L.qc_terms_ext()), C.byref(h))
        assert rc == 0, L.lib.qc_terms_last_error(None)
        nnz = C.c_int64()
        L.lib.qc_terms_hess_nnz(h, C.byref(nnz))
        r = np.empty(nnz.value, dtype=np.int64)
        c = np.empty(nnz.value, dtype=np.int64)
        L.lib.qc_terms_hess_structure(h, L.iptr(r), L.iptr(c), 0)
        J = C.c_double()
        g = np.empty(Z.size)
        H = np.empty(nnz.value)
        assert L.lib.qc_terms_eval(h, L.dptr(Z), C.byref(J), L.dptr(g), L.dptr(H)) == 0
        outs.append((r.tobytes(), c.tobytes(), J.value, g.tobytes(), H.tobytes()))
        L.lib.qc_terms_destroy(h)
    assert outs[0] == outs[1] == outs[2]
    assert abs(outs[0][2] - ref.value(plain, Z)) <= 1e-12 * abs(outs[0][2])


@pytest.mark.gpu
def test_regulariser_only_objective_is_unchanged(qc):
    """A TrajectoryObjective without extension terms still goes through qc_terms_create and matches the restatement."""
    traj, spec, tm, Z = make_case(qc, T=64, global_dim=1, seed=11)
    obj = qc.TrajectoryObjective(qc.QuadraticRegularizer("a", traj, 0.5) + qc.MinimumTimeObjective(traj, 0.8), traj)
    assert not obj.has_ext
    only = ref.TermsExt(T=64, zdim=tm.zdim, off_dt=tm.off_dt, global_dim=1, reg_index=np.asarray(traj.components["a"]),
                        reg_R=np.full(2, 0.5), D=0.8, n_mt=63)
    J, g, H = obj.L_grad_hess(Z)
    assert abs(J - ref.value(only, Z)) <= 1e-12 * abs(J)
    np.testing.assert_allclose(g, ref.grad(only, Z), rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(H, ref.hess_values(only, Z), rtol=1e-13, atol=1e-15)
    obj.close()


@pytest.mark.gpu
def test_one_handle_alternating_outputs_and_many_handles(qc):
    """The extension handle (two more device tables) through the same use as the plain one: calls with and without gradient / Hessian
    in turn return the bits of the first call and of a fresh handle; the last of 20 handles created and destroyed in a row (the
    smallest shape, T = 1) still evaluates."""
    same = lambda a, b: all((x is None and y is None) or np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))
    traj, spec, tm, Z = make_case(qc, T=2, global_dim=2, baseline=True, seed=9)
    obj = qc.TrajectoryObjective(spec, traj)
    assert obj.has_ext
    full = obj._eval(Z, True, True)
    bare = obj._eval(Z, False, False)
    assert bare[0] == full[0] and bare[1] is None and bare[2] is None
    assert same(obj._eval(Z, True, True), full)
    fresh = qc.TrajectoryObjective(spec, traj)
    assert same(fresh._eval(Z, False, False), bare) and same(fresh._eval(Z, True, True), full)
    fresh.close()
    obj.close()
    traj, spec, tm, Z = make_case(qc, T=1, seed=8)
    for k in range(20):
        obj = qc.TrajectoryObjective(spec, traj)
        if k < 19:
            obj.close()
    J, g, H = obj._eval(Z, True, True)
    assert abs(J - ref.value(tm, Z)) <= 1e-12 * max(1.0, abs(ref.value(tm, Z)))
    np.testing.assert_allclose(g, ref.grad(tm, Z), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(H, ref.hess_values(tm, Z), rtol=1e-12, atol=1e-13)
    obj.close()
