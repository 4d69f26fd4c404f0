"""UnitaryRobustnessObjective (reference unitary_robustness_problem.jl:46-49) through `qc_robust_*`: the numpy restatement
(tests/robust_reference.py) is certified on the CPU by the complex step and central differences; the device-free entry points
are checked on the CPU; the GPU values (L, the dense gradient, the dense Hessian) are checked against the restatement."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import robust_reference as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _herm(rng, n):
    X = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    return (X + X.conj().T) / 2


def _spec_and_Z(rng, T, N, sub, free, K=None, global_dim=0, state_first=True, H=None):
    n = N if sub is None else len(sub)
    H = _herm(rng, n) if H is None else H
    lead = 0 if state_first else 3
    off_state = lead
    zdim = lead + 2 * N * N + 2 + (1 if free else 0)
    off_dt = zdim - 1 if free else -1
    s = rr.RobustSpec(T=T, zdim=zdim, off_state=off_state, N=N, H=H, subspace=sub, off_dt=off_dt, dt_fixed=0.2, K=K,
                      global_dim=global_dim)
    Z = rng.standard_normal(T * zdim + global_dim) / np.sqrt(N)
    if free:
        Z[off_dt:T * zdim:zdim] = rng.uniform(0.1, 0.3, T)
    return s, Z


def _desc(qc, s: rr.RobustSpec, hessian=1, keep=None):
    L = qc._lib
    d = L.qc_robust_desc()
    keep = [] if keep is None else keep
    Hre = np.ascontiguousarray(np.asarray(s.H).real.reshape(-1, order="F"))
    Him = np.ascontiguousarray(np.asarray(s.H).imag.reshape(-1, order="F"))
    keep += [Hre, Him]
    d.T, d.zdim, d.off_state, d.N = s.T, s.zdim, s.off_state, s.N
    if s.subspace is not None:
        sub = np.ascontiguousarray(s.subspace, dtype=np.int32)
        keep.append(sub)
        d.subspace = sub.ctypes.data_as(C.POINTER(C.c_int32))
        d.n_sub = sub.size
    d.H_re, d.H_im = L.dptr(Hre), L.dptr(Him)
    d.off_dt, d.dt_fixed, d.global_dim = s.off_dt, s.dt_fixed, s.global_dim
    d.n_knots = s.nK
    d.hessian = hessian
    return d, keep


# ---------------------------------------------------------------------------------------------------- CPU ----
@pytest.mark.parametrize("N,sub,free,K", [(2, None, True, None), (3, [0, 1], False, None), (4, [3, 0, 2], True, 4), (3, [1, 2], True, 3)])
def test_restatement_against_complex_step_and_central_differences(N, sub, free, K):
    rng = np.random.default_rng(N * 7 + (K or 0))
    n = N if sub is None else len(sub)
    H = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))      # not Hermitian: the formulas do not assume it
    s, Z = _spec_and_Z(rng, 5, N, sub, free, K=K, global_dim=2, state_first=False, H=H)
    g = rr.grad(Z, s)
    gc = rr.complex_step_grad(Z, s)
    assert np.abs(g - gc).max() <= 1e-15 * max(1.0, np.abs(g).max()) * 4
    eps = 1e-6
    for i in rr.variables(s)[::3]:
        Zp, Zm = Z.copy(), Z.copy()
        Zp[i] += eps
        Zm[i] -= eps
        assert abs((rr.loss(Zp, s) - rr.loss(Zm, s)) / (2 * eps) - g[i]) < 1e-8 * max(1.0, np.abs(g).max())
    outside = np.setdiff1d(np.arange(Z.size), rr.variables(s))
    assert not g[outside].any()
    Hm = rr.hessian(Z, s)
    assert np.abs(Hm - Hm.T).max() < 1e-12 * np.abs(Hm).max()
    vs = rr.variables(s)
    fd = np.empty_like(Hm)
    for c, i in enumerate(vs):
        Zp, Zm = Z.copy(), Z.copy()
        Zp[i] += eps
        Zm[i] -= eps
        fd[:, c] = (rr.grad(Zp, s)[vs] - rr.grad(Zm, s)[vs]) / (2 * eps)
    assert np.abs(Hm - fd).max() < 1e-8 * np.abs(Hm).max()


def test_robust_desc_layout_matches_c(qc, tmp_path):
    src = tmp_path / "rsz.c"
    fields = ["T", "zdim", "off_state", "N", "n_sub", "subspace", "H_re", "H_im", "off_dt", "dt_fixed", "global_dim", "n_knots",
              "hessian", "device", "reserved1"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "qcolloc.h"\nint main(){printf("%zu'
                   + " %zu" * len(fields) + '\\n", sizeof(qc_robust_desc)'
                   + "".join(f", offsetof(qc_robust_desc, {f})" for f in fields) + ");return 0;}\n")
    exe = tmp_path / "rsz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    m = qc._lib.qc_robust_desc
    assert got == [C.sizeof(m)] + [getattr(m, f).offset for f in fields]
    assert qc._lib.lib.qc_sizeof_robust_desc() == C.sizeof(m)


@pytest.mark.parametrize("N,sub,free,K,state_first", [(2, None, True, None, True), (3, [0, 1], False, 4, False),
                                                      (8, [6, 1, 4], True, 3, False), (4, None, False, None, True)])
def test_desc_variables_and_hessian_structure_match_the_restatement(qc, N, sub, free, K, state_first):
    rng = np.random.default_rng(3)
    s, _ = _spec_and_Z(rng, 5, N, sub, free, K=K, global_dim=2, state_first=state_first)
    lib = qc._lib.lib
    d, keep = _desc(qc, s)
    nv, nnz = C.c_int64(), C.c_int64()
    assert lib.qc_robust_desc_n_vars(C.byref(d), C.byref(nv)) == 0
    vs = rr.variables(s)
    assert nv.value == vs.size
    got = np.empty(nv.value, dtype=np.int64)
    assert lib.qc_robust_desc_vars(C.byref(d), qc._lib.iptr(got)) == 0
    assert np.array_equal(got, vs)
    assert lib.qc_robust_desc_hess_nnz(C.byref(d), C.byref(nnz)) == 0
    assert nnz.value == vs.size * (vs.size + 1) // 2
    rows, cols = np.empty(nnz.value, dtype=np.int64), np.empty(nnz.value, dtype=np.int64)
    assert lib.qc_robust_desc_hess_structure(C.byref(d), qc._lib.iptr(rows), qc._lib.iptr(cols), 1) == 0
    r, c = np.triu_indices(vs.size)
    order = np.lexsort((r, c))                      # column-major upper triangle
    assert np.array_equal(rows, vs[r[order]] + 1) and np.array_equal(cols, vs[c[order]] + 1)
    d.hessian = 0
    assert lib.qc_robust_desc_hess_nnz(C.byref(d), C.byref(nnz)) == 0 and nnz.value == 0
    del keep


def test_invalid_descriptors_are_refused_with_a_message(qc):
    L = qc._lib
    rng = np.random.default_rng(5)
    s, _ = _spec_and_Z(rng, 6, 3, [0, 1], True)
    nnz = C.c_int64()

    def rc_of(mut):
        d, keep = _desc(qc, s)
        keep.append(mut(d))
        rc = L.lib.qc_robust_desc_hess_nnz(C.byref(d), C.byref(nnz))
        return rc, L.lib.qc_robust_last_error(None).decode()

    assert rc_of(lambda d: None)[0] == 0
    bad_sub = np.array([0, 3], dtype=np.int32)
    dup_sub = np.array([1, 1], dtype=np.int32)

    def set_sub(a):
        def f(d):
            d.subspace = a.ctypes.data_as(C.POINTER(C.c_int32))
            d.n_sub = a.size
            return a
        return f

    for mut, word in ((set_sub(bad_sub), "subspace"), (set_sub(dup_sub), "subspace"),
                      (lambda d: setattr(d, "n_knots", 0), "n_knots"), (lambda d: setattr(d, "n_knots", s.T + 1), "n_knots"),
                      (lambda d: setattr(d, "off_state", s.zdim - 2 * s.N * s.N + 1), "state"),
                      (lambda d: setattr(d, "hessian", 2), "hessian"), (lambda d: setattr(d, "off_dt", s.zdim), "off_dt"),
                      (lambda d: setattr(d, "H_re", None), "H_re")):
        rc, msg = rc_of(mut)
        assert rc == L.QC_ERR_INVALID and word in msg, (word, rc, msg)
    assert L.lib.qc_robust_desc_hess_nnz(None, C.byref(nnz)) == L.QC_ERR_INVALID


def test_unsupported_sizes_are_refused(qc):
    L = qc._lib
    nnz = C.c_int64()
    rng = np.random.default_rng(6)
    s, _ = _spec_and_Z(rng, 2, 33, [0, 1], False)            # 2N = 66
    d, keep = _desc(qc, s)
    assert L.lib.qc_robust_desc_hess_nnz(C.byref(d), C.byref(nnz)) == L.QC_ERR_UNSUPPORTED
    assert "64" in L.lib.qc_robust_last_error(None).decode()
    # N = 3, n = 2, free timestep: V = 9 K;  K = 1500 is under the cap (V = 13 500), K = 2000 is over it
    s, _ = _spec_and_Z(rng, 2000, 3, [0, 1], True, K=1500)
    d, keep = _desc(qc, s)
    assert L.lib.qc_robust_desc_hess_nnz(C.byref(d), C.byref(nnz)) == 0 and nnz.value == 13500 * 13501 // 2
    d.n_knots = 2000
    assert L.lib.qc_robust_desc_hess_nnz(C.byref(d), C.byref(nnz)) == L.QC_ERR_UNSUPPORTED
    msg = L.lib.qc_robust_last_error(None).decode()
    assert "18000" in msg and str(18000 * 18001 // 2) in msg
    d.hessian = 0                                            # without the Hessian the same term is fine
    assert L.lib.qc_robust_desc_hess_nnz(C.byref(d), C.byref(nnz)) == 0 and nnz.value == 0
    del keep


@pytest.mark.skipif(torch.cuda.is_available(), reason="this box has a GPU")
def test_create_without_a_gpu_fails_loudly(qc):
    L = qc._lib
    s, _ = _spec_and_Z(np.random.default_rng(7), 4, 2, None, True)
    d, keep = _desc(qc, s)
    h = C.c_void_p()
    assert L.lib.qc_robust_create(C.byref(d), C.byref(h)) == L.QC_ERR_NO_DEVICE
    traj = qc.NamedTrajectory({"Ũ⃗": np.zeros((8, 4)), "Δt": np.full((1, 4), 0.2)}, timestep="Δt")
    with pytest.raises(qc.QCollocError) as e:
        qc.UnitaryRobustnessObjective(traj, H_error=np.diag([1.0, -1.0]))
    assert e.value.code == L.QC_ERR_NO_DEVICE
    del keep


# ---------------------------------------------------------------------------------------------------- GPU ----
SIZES = [(2, None), (3, [0, 1]), (8, None), (8, [1, 4, 6]), (16, None), (32, [0, 9, 20, 31])]
TS = [1, 2, 51, 257, 1000, 4097]
HESS_MAX_V = 2000            # the restatement's complex-stepped Hessian stays quick below this


def _traj(qc, s: rr.RobustSpec, Z):
    """A NamedTrajectory with the restatement's knot layout: [lead (3) ; Ũ⃗ ; a (2) ; Δt?] and a global phase block."""
    N, T = s.N, s.T
    data = Z[:T * s.zdim].reshape(T, s.zdim).T
    comps = {}
    if s.off_state:
        comps["lead"] = data[:s.off_state]
    comps["Ũ⃗"] = data[s.off_state:s.off_state + 2 * N * N]
    comps["a"] = data[s.off_state + 2 * N * N:s.off_state + 2 * N * N + 2]
    if s.off_dt >= 0:
        comps["Δt"] = data[s.off_dt:s.off_dt + 1]
    g = {"ϕ": Z[T * s.zdim:]} if s.global_dim else None
    traj = qc.NamedTrajectory(comps, controls=("a",), timestep="Δt" if s.off_dt >= 0 else s.dt_fixed, global_data=g)
    assert np.array_equal(traj.datavec, Z)
    return traj


def _cases():
    out = []
    i = 0
    for N, sub in SIZES:
        for T in TS:
            out.append(pytest.param(N, sub, T, i % 2 == 0, i % 3 == 1 and T > 1, 3 if i % 4 == 2 else 0, i % 5 != 3, i % 7 == 0,
                                    id=f"N{N}-n{N if sub is None else len(sub)}-T{T}-{i}"))
            i += 1
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("N,sub,T,free,last_knot_out,global_dim,state_first,nonherm", _cases())
def test_gpu_matches_the_restatement(qc, N, sub, T, free, last_knot_out, global_dim, state_first, nonherm):
    rng = np.random.default_rng(N * 10007 + T)
    n = N if sub is None else len(sub)
    H = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)) if nonherm else None
    s, Z = _spec_and_Z(rng, T, N, sub, free, K=T - 1 if last_knot_out else None, global_dim=global_dim, state_first=state_first, H=H)
    traj = _traj(qc, s, Z)
    V = rr.variables(s).size
    want_h = V <= HESS_MAX_V
    obj = qc.UnitaryRobustnessObjective(traj, H_error=s.H, subspace=sub, knots=s.nK, eval_hessian=want_h)
    try:
        assert np.array_equal(obj.variables, rr.variables(s))
        L, g, Hv = obj.L_grad_hess(Z)
        L_ref, g_ref = rr.loss(Z, s), rr.grad(Z, s)
        assert abs(L - L_ref) <= 1e-12 * abs(L_ref)
        assert g.shape == Z.shape
        assert np.abs(g - g_ref).max() <= 1e-12 * np.abs(g_ref).max()
        if global_dim:
            assert not g[T * s.zdim:].any()
        if want_h:
            H_ref = rr.packed_upper(rr.hessian(Z, s))
            assert Hv.shape == H_ref.shape
            assert np.abs(Hv - H_ref).max() <= 1e-10 * np.abs(H_ref).max()
    finally:
        obj.close()


@pytest.mark.gpu
def test_values_are_bit_identical_across_calls_and_entry_points(qc):
    rng = np.random.default_rng(11)
    s, Z = _spec_and_Z(rng, 257, 3, [0, 1], True, global_dim=2, state_first=False)
    traj = _traj(qc, s, Z)
    obj = qc.UnitaryRobustnessObjective(traj, H_error=qc.EmbeddedOperator(np.diag([1.0, -1.0]), [0, 1], 3))
    try:
        L1, g1, H1 = obj.L_grad_hess(Z)
        L2, g2, H2 = obj.L_grad_hess(Z)
        assert L1 == L2 and np.array_equal(g1, g2) and np.array_equal(H1, H2)
        dZ = torch.from_numpy(Z).cuda()
        dL = torch.empty(1, dtype=torch.float64, device="cuda")
        dg = torch.full((Z.size,), np.nan, dtype=torch.float64, device="cuda")      # every entry is written, zeros included
        dH = torch.empty(obj.hess_nnz, dtype=torch.float64, device="cuda")
        for _ in range(2):
            obj.eval_device(dZ, dL, dg, dH)
            torch.cuda.synchronize()
            assert dL.item() == L1 and np.array_equal(dg.cpu().numpy(), g1) and np.array_equal(dH.cpu().numpy(), H1)
        obj.eval_device(dZ, dL)              # L alone
        torch.cuda.synchronize()
        assert dL.item() == L1
        r, c = obj.hess_structure
        vs = rr.variables(s)
        ri, ci = np.triu_indices(vs.size)
        order = np.lexsort((ri, ci))
        assert np.array_equal(r, vs[ri[order]]) and np.array_equal(c, vs[ci[order]])
        assert np.array_equal(getattr(obj, "∂²L_structure")[0], r) and np.array_equal(getattr(obj, "∇L")(Z), g1)
    finally:
        obj.close()


@pytest.mark.gpu
def test_without_the_hessian_the_structure_is_empty(qc):
    rng = np.random.default_rng(12)
    s, Z = _spec_and_Z(rng, 51, 2, None, True)
    obj = qc.UnitaryRobustnessObjective(_traj(qc, s, Z), H_error=s.H, eval_hessian=False)
    try:
        r, c = obj.hess_structure
        assert obj.hess_nnz == 0 and r.size == 0 and c.size == 0
        assert abs(obj.L(Z) - rr.loss(Z, s)) <= 1e-12 * rr.loss(Z, s)
        assert np.abs(obj.grad_L(Z) - rr.grad(Z, s)).max() <= 1e-12 * np.abs(rr.grad(Z, s)).max()
        with pytest.raises(RuntimeError):
            obj.hess_L(Z)
    finally:
        obj.close()


@pytest.mark.gpu
def test_evaluator_with_the_term_is_the_sum_of_its_parts(qc):
    inp = qc.config_inputs(1, T=20)
    traj = inp.traj
    dyn = qc.QuantumDynamics(inp.integrators, traj)
    reg = qc.TrajectoryObjective(qc.QuadraticRegularizer("a", traj, 1e-2) + qc.QuadraticRegularizer("dda", traj, 1e-2), traj)
    rob = qc.UnitaryRobustnessObjective(traj, H_error=qc.PAULIS["Z"])
    ev = qc.QuantumControlEvaluator(dyn, [reg, rob])
    try:
        Z = traj.datavec
        g = np.empty(ev.n_variables)
        ev.eval_objective_gradient(g, Z)
        assert np.array_equal(g, reg.grad_L(Z) + rob.grad_L(Z))
        assert ev.eval_objective(Z) == reg.L(Z) + rob.L(Z)
        rng = np.random.default_rng(13)
        mu = rng.standard_normal(ev.n_constraints)
        Hv = np.empty(ev.hess_nnz)
        ev.eval_hessian_lagrangian(Hv, Z, 0.7, mu)
        hr, hc = ev.hessian_lagrangian_structure()
        r_reg, c_reg = reg.hess_structure
        n_reg, n_rob = r_reg.size, rob.hess_nnz
        assert np.array_equal(Hv[:n_reg], 0.7 * reg.hess_L(Z))
        assert np.array_equal(Hv[n_reg:n_reg + n_rob], 0.7 * rob.hess_L(Z))
        assert np.array_equal(hr[n_reg:n_reg + n_rob], rob.hess_structure[0]) and np.array_equal(hc[n_reg:n_reg + n_rob], rob.hess_structure[1])
        assert np.allclose(Hv[n_reg + n_rob:], dyn.mu_d2F(Z, mu), rtol=1e-13, atol=0)
        # the assembled matrix: the robustness block against the restatement
        s = rr.RobustSpec(T=traj.T, zdim=traj.dim, off_state=traj.offset("Ũ⃗"), N=2, H=qc.PAULIS["Z"], off_dt=traj.offset("Δt"),
                          global_dim=traj.global_dim)
        W = ev.hessian_lagrangian_matrix(Z, 1.0, np.zeros(ev.n_constraints)).toarray()
        vs = rr.variables(s)
        reg_full = np.zeros((ev.n_variables, ev.n_variables))
        np.add.at(reg_full, (r_reg, c_reg), reg.hess_L(Z))
        reg_full = reg_full + np.triu(reg_full, 1).T
        H_ref = rr.hessian(Z, s)
        assert np.abs(W[np.ix_(vs, vs)] - reg_full[np.ix_(vs, vs)] - H_ref).max() <= 1e-10 * np.abs(H_ref).max()
    finally:
        for o in (dyn, reg, rob):
            o.close()


# ---------------------------------------------------------------------------------------------- launch forms ----
# The host rule of qc_robust_create (qc_robust.hip:539-547, the opt-in at :581-586) restated: knots per group, passes of the
# per-knot loops (load_v, mul_nn / mul_cn, the G loop: kp n^2 items strided by 256 threads), the two LDS sizes, V.
HESS_CAP = 1 << 27          # V (V + 1) / 2 packed values (kRobHessCap, qc_robust.hip:47, checked at :455)


def robust_launch(N, sub, free, K):
    n = N if sub is None else len(sub)
    nn, m2 = n * n, 2 * n * n
    kp = max(1, min(64, 256 // nn))                                   # :540
    V = K * (m2 + (1 if free else 0))                                 # robust_layout, :454
    return dict(n=n, kp=kp, passes=-(-kp * nn // 256),
                lds_partial=(m2 + kp * (2 * m2 + m2 + 1)) * 8,        # :546
                lds_grad=(2 * m2 + kp * 5 * m2 + 2 * kp) * 8,         # :547
                V=V)


def hessian_check(V):
    """How a case's Hessian is compared: 'full' (dense restatement), 'columns' (whole columns + HVPs), None (over the cap)."""
    if V <= HESS_MAX_V:
        return "full"
    return "columns" if V * (V + 1) // 2 <= HESS_CAP else None


SUB20 = [0, 2, 3, 5, 6, 7, 8, 9, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 23]
# N, sub, T, K (None: every knot), free dt, state first (else a lead of 3 entries), global_dim
FORM_CASES = [
    (1, None, 2, None, False, True, 0),            # n = 1: kp = 64, m2 = 2 padded to 4
    (3, [2], 257, 256, False, False, 2),
    (3, [1], 1000, None, True, False, 2),          # n = 1, V = 3000
    (17, None, 1, None, True, False, 2),           # n = 17: two passes, no opt-in
    (17, None, 257, None, False, True, 0),
    (24, SUB20, 2, None, True, False, 3),          # n = 20: two passes
    (20, None, 1000, 999, True, True, 0),
    (25, None, 1, None, True, False, 2),           # n = 25: opt-in on the gradient kernel
    (25, None, 257, None, False, True, 0),
    (32, None, 1, None, False, True, 2),           # n = 32: opt-in on both kernels (fixed dt: one knot's L does not depend on dt)
    (32, None, 2, None, True, False, 0),
    (32, None, 1000, 999, True, False, 2),
]
# the Hessian above V = 2000: N, sub, T, K, free, state first, global_dim
HESS_BIG_CASES = [
    (2, None, 700, 667, True, False, 2),           # V = 6003
    (3, [0, 1], 1500, None, True, True, 0),        # V = 13 500, the size profiles/robust_summary.txt times
    (32, None, 8, 7, True, False, 0),              # V = 14 343, near the cap
]


def _form_id(c):
    N, sub, T, K, free, sf, gd = c
    return f"N{N}-n{N if sub is None else len(sub)}-T{T}-K{K or T}-{'free' if free else 'fixed'}"


def test_launch_form_coverage():
    """The GPU cases below reach every launch form of qc_robust_create and every way the Hessian is compared."""
    def forms(cases):
        return [dict(robust_launch(N, sub, free, K or T), check=hessian_check(robust_launch(N, sub, free, K or T)["V"]))
                for N, sub, T, K, free, _, _ in cases]
    new = forms(FORM_CASES)
    big = forms(HESS_BIG_CASES)
    assert any(f["passes"] == 1 for f in new)
    assert any(f["passes"] > 1 and f["lds_grad"] <= 65536 for f in new)
    assert any(f["lds_grad"] > 65536 and f["lds_partial"] <= 65536 for f in new)
    assert any(f["lds_partial"] > 65536 for f in new)
    assert robust_launch(32, None, True, 1)["lds_partial"] == 65544 and robust_launch(24, None, True, 1)["lds_grad"] < 65536
    assert any(f["n"] == 1 and f["kp"] == 64 for f in new)
    assert any(f["check"] == "full" and f["passes"] > 1 for f in new) and any(f["check"] == "full" and f["lds_grad"] > 65536 for f in new)
    assert any(f["check"] == "columns" for f in new) and any(f["check"] is None for f in new)
    assert [f["check"] for f in big] == ["columns"] * 3 and 5000 < big[0]["V"] < 7000 and big[1]["V"] == 13500
    assert big[2]["V"] == 14343 and big[2]["lds_partial"] > 65536


def test_hessian_cap_at_32_levels(qc):
    """n = 32 with a free timestep: V = 2049 K.  K = 7 is under the 2^27 cap, K = 8 over it; without the Hessian K = 8 is fine."""
    L = qc._lib
    nnz = C.c_int64()
    s, _ = _spec_and_Z(np.random.default_rng(8), 8, 32, None, True, K=7)
    d, keep = _desc(qc, s)
    assert L.lib.qc_robust_desc_hess_nnz(C.byref(d), C.byref(nnz)) == 0 and nnz.value == 14343 * 14344 // 2
    d.n_knots = 8
    assert L.lib.qc_robust_desc_hess_nnz(C.byref(d), C.byref(nnz)) == L.QC_ERR_UNSUPPORTED
    assert str(2049 * 8) in L.lib.qc_robust_last_error(None).decode()
    d.hessian = 0
    assert L.lib.qc_robust_desc_hess_nnz(C.byref(d), C.byref(nnz)) == 0 and nnz.value == 0
    nv = C.c_int64()
    assert L.lib.qc_robust_desc_n_vars(C.byref(d), C.byref(nv)) == 0 and nv.value == 2049 * 8
    del keep


def _column_picks(s: rr.RobustSpec, V, seed, count=48):
    """Columns to compare whole: the first and last variable of knots 0, 1, K-2, K-1, some dt columns, columns 16J-1, 16J,
    16J+15 of a low, a middle and the last tile row, the rest at random (fixed seed)."""
    P, K = V // s.nK, s.nK
    pick = set()
    for t in (0, 1, K - 2, K - 1):
        if 0 <= t < K:
            pick.update((t * P, t * P + P - 1))
    if s.off_dt >= 0:
        dtpos = int(np.flatnonzero(rr.variables(s)[:P] == s.off_dt)[0])
        pick.update(t * P + dtpos for t in {0, K // 2, K - 1})
    last = (V - 1) // 16
    for J in (1, last // 2, last):
        pick.update(c for c in (16 * J - 1, 16 * J, 16 * J + 15) if 0 <= c < V)
    rng = np.random.default_rng(seed)
    while len(pick) < min(count, V):
        pick.add(int(rng.integers(V)))
    return sorted(pick)


def _check_packed_hessian(Hp, Z, s: rr.RobustSpec, seed, n_hvp=2):
    """(a) whole columns against the complex-stepped columns at 1e-10 of each column's max; (b) H v from every packed value
    against the complex step of the gradient along v, entry by entry within 1e-10 of (|H| |v|)_i."""
    V = rr.variables(s).size
    assert Hp.shape == (V * (V + 1) // 2,) and np.isfinite(Hp).all()
    cols = _column_picks(s, V, seed)
    assert len(cols) >= min(48, V)
    ref = rr.hessian_columns(Z, s, cols)
    for c, k in enumerate(cols):
        got = rr.packed_column(Hp, k)
        assert np.abs(got - ref[:, c]).max() <= 1e-10 * np.abs(ref[:, c]).max(), k
    X = np.random.default_rng(seed + 1).standard_normal((V, n_hvp))
    HX, AX = rr.packed_matvec(Hp, X)
    for q in range(n_hvp):
        want = rr.hessian_vector_product(Z, s, X[:, q])
        assert (np.abs(HX[:, q] - want) <= 1e-10 * AX[:, q]).all(), q


def test_column_helpers_against_the_dense_hessian():
    """hessian_columns / hessian_vector_product / packed_column / packed_matvec restate the dense Hessian, and the packed check
    rejects one wrong stored value."""
    rng = np.random.default_rng(9)
    s, Z = _spec_and_Z(rng, 6, 3, [0, 2], True, K=5, global_dim=2, state_first=False)
    Hm = rr.hessian(Z, s)
    V = Hm.shape[0]
    cols = [0, 7, V - 1]
    assert np.abs(rr.hessian_columns(Z, s, cols) - Hm[:, cols]).max() <= 1e-14 * np.abs(Hm).max()
    Hp = rr.packed_upper(Hm)
    Hs = np.triu(Hm) + np.triu(Hm, 1).T                              # the matrix the packed triangle holds
    for k in range(V):
        assert np.array_equal(rr.packed_column(Hp, k), Hs[:, k])
    X = rng.standard_normal((V, 2))
    HX, AX = rr.packed_matvec(Hp, X)
    assert np.abs(HX - Hs @ X).max() <= 1e-13 * np.abs(Hm).max() and np.allclose(AX, np.abs(Hs) @ np.abs(X), rtol=1e-14)
    assert np.abs(rr.hessian_vector_product(Z, s, X[:, 0]) - Hm @ X[:, 0]).max() <= 1e-12 * AX[:, 0].max()
    _check_packed_hessian(Hp, Z, s, seed=1)
    bad = Hp.copy()
    bad[bad.size // 2] *= 1 + 1e-7
    with pytest.raises(AssertionError):
        _check_packed_hessian(bad, Z, s, seed=1)


@pytest.mark.gpu
@pytest.mark.parametrize("N,sub,T,K,free,state_first,global_dim", FORM_CASES, ids=[_form_id(c) for c in FORM_CASES])
def test_gpu_launch_forms_match_the_restatement(qc, N, sub, T, K, free, state_first, global_dim):
    """More than one pass of the per-knot loops (n = 17, 20), the LDS opt-in of one kernel (n = 25) and of both (n = 32),
    kp = 64 (n = 1): L and the gradient against the restatement, the Hessian wherever V allows."""
    rng = np.random.default_rng(N * 1009 + T)
    s, Z = _spec_and_Z(rng, T, N, sub, free, K=K, global_dim=global_dim, state_first=state_first)
    form = robust_launch(N, sub, free, s.nK)
    check = hessian_check(form["V"])
    obj = qc.UnitaryRobustnessObjective(_traj(qc, s, Z), H_error=s.H, subspace=sub, knots=s.nK, eval_hessian=check is not None)
    try:
        assert np.array_equal(obj.variables, rr.variables(s))
        if check is None:
            L, g = obj.L(Z), obj.grad_L(Z)
        else:
            L, g, Hv = obj.L_grad_hess(Z)
        L_ref, g_ref = rr.loss(Z, s), rr.grad(Z, s)
        assert abs(L - L_ref) <= 1e-12 * abs(L_ref)
        assert g.shape == Z.shape and np.abs(g - g_ref).max() <= 1e-12 * np.abs(g_ref).max()
        if global_dim:
            assert not g[T * s.zdim:].any()
        if check == "full":
            H_ref = rr.packed_upper(rr.hessian(Z, s))
            assert Hv.shape == H_ref.shape and np.abs(Hv - H_ref).max() <= 1e-10 * np.abs(H_ref).max()
        elif check == "columns":
            _check_packed_hessian(Hv, Z, s, seed=N + T)
    finally:
        obj.close()


@pytest.mark.gpu
@pytest.mark.parametrize("N,sub,T,K,free,state_first,global_dim", HESS_BIG_CASES, ids=[_form_id(c) for c in HESS_BIG_CASES])
def test_gpu_hessian_above_the_dense_check(qc, N, sub, T, K, free, state_first, global_dim):
    """2000 < V <= the cap: whole columns and Hessian-vector products over every packed value; the largest size twice, bit for bit."""
    import gc
    rng = np.random.default_rng(N * 31 + T)
    s, Z = _spec_and_Z(rng, T, N, sub, free, K=K, global_dim=global_dim, state_first=state_first)
    obj = qc.UnitaryRobustnessObjective(_traj(qc, s, Z), H_error=s.H, subspace=sub, knots=s.nK)
    try:
        L, g, Hv = obj.L_grad_hess(Z)
        assert abs(L - rr.loss(Z, s)) <= 1e-12 * abs(rr.loss(Z, s))
        g_ref = rr.grad(Z, s)
        assert np.abs(g - g_ref).max() <= 1e-12 * np.abs(g_ref).max()
        _check_packed_hessian(Hv, Z, s, seed=N + T, n_hvp=3 if N == 2 else 2)
        if N == 32:
            L2, g2, H2 = obj.L_grad_hess(Z)
            assert L2 == L and np.array_equal(g2, g) and np.array_equal(H2, Hv)
            del H2
    finally:
        obj.close()
        Hv = None
        gc.collect()


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 2])
def test_hessian_staging_arrives_with_the_first_call_that_asks(qc, T):
    """A handle with the exact Hessian, host-buffer calls without Hessian values, then with, then without: the staging of the values is
    allocated by the second call.  Every result carries the bits of fresh handles' (one whose first call asks for the values, one that
    never does)."""
    rng = np.random.default_rng(31 + T)
    s, Z = _spec_and_Z(rng, T, 2, None, True)
    traj = _traj(qc, s, Z)
    make = lambda: qc.UnitaryRobustnessObjective(traj, H_error=s.H, eval_hessian=True)
    obj, with_h, without_h = make(), make(), make()
    try:
        L0, g0, _ = without_h._eval(Z, True, False)
        L1, g1, H1 = with_h._eval(Z, True, True)
        assert L0 == L1 and np.array_equal(g0, g1)
        for want_h in (False, True, False):
            L, g, H = obj._eval(Z, True, want_h)
            assert L == L0 and np.array_equal(g, g0)
            assert (H is None) if not want_h else np.array_equal(H, H1)
        assert abs(L0 - rr.loss(Z, s)) <= 1e-12 * abs(rr.loss(Z, s))
        assert np.abs(H1 - rr.packed_upper(rr.hessian(Z, s))).max() <= 1e-10 * np.abs(H1).max()
    finally:
        for o in (obj, with_h, without_h):
            o.close()
