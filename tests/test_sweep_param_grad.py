"""Sweep parameter gradients (`qc_sweep_grad_params*`, `RolloutSweep.param_grad`, `rollout_sweep_parameter_gradient`): dF_s/dtheta[s, j]
and dF_s/dc[s, k] of every sample of a rollout sweep, the derivatives with respect to the parameters the sample's system is made of.
CPU: the two routes of tests/sweep_param_grad_reference.py against each other, the Euler identity between that reference and the control
gradient's, prototypes, header, the NULL handle, argument validation that needs no handle.  GPU: every value against the forward-mode
reference, the squarings, two identities on device outputs, bit-level properties, the device entry point, refused handles and
arguments, the example.

Tolerance (GPU against the reference), per sample s: |got - want| <= 1e-9 max(1, A_s), A_s = max over the parameters of
sum_t |term_{s,t}| from the forward-mode reference: the per-interval bound of tests/test_sweep_grad.py (states to 1e-10, truncation
1.7e-12 relative per term) carried through a sum, so it scales with the sum of magnitudes, not with T.  The identities between
outputs of one call hold to 1e-12 max(1, A_s).  Measured worst ratios: profiles/sweep_param_grad_summary.txt.
Every sample of mid-size and filled launches (S = 97 .. 2049) against the reference: tests/test_sweep_every_sample.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import sweep_grad_reference as gref
import sweep_param_grad_reference as pref
import sweep_reference as ref
import test_sweep as ts
import test_sweep_grad as tg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAR_RTOL, ID_RTOL = 1e-9, 1e-12
_herm, _unitary = ts._herm, ts._unitary

PARAM_CASES = ["qubit", "qutrit", "levels4-5drives", "qubits3-6drives", "qubits3-8drives", "ket", "one-interval", "one-chunk", "long-trajectory"]
_REF = {}          # case name -> (terms, sums): computed once, shared, never written to


def reference(c):
    if c["name"] not in _REF:
        out = pref.param_terms_forward(c["G0"], c["Gd"], c["Gp"], c["controls"], c["dts"], c["init"], c["theta"], c["scale"], c["samples"], c["kind"],
                                       c["goal"], c["L"], c["subspace"], c["form"])
        for a in out:
            a.setflags(write=False)
        _REF[c["name"]] = out
    return _REF[c["name"]]


def magnitudes(terms):
    """A_s: the largest sum of magnitudes over the intervals among a sample's parameters."""
    return np.abs(terms).sum(axis=1).max(axis=1) if terms.shape[2] else np.zeros(terms.shape[0])


def custom(qc, name, N, m, p, T, S, free, use_scale, seed, fid=("unitary", None, "abs"), perts=None):
    """A case of the shape `tg.build` returns, for shapes GRAD_CASES does not have."""
    rng = np.random.default_rng(seed)
    H0 = _herm(rng, N)
    Hd = [_herm(rng, N, (N * max(m, 1)) ** -0.5) for _ in range(m)]
    perts = [_herm(rng, N) for _ in range(p)] if perts is None else perts(Hd)
    kind, subspace, form = fid
    return dict(name=name, L=N, m=m, p=p, S=S, T=T, system=qc.QuantumSystem(H0, Hd) if qc is not None else None, perts=perts,
                G0=ref.iso_generator(H0), Gd=[ref.iso_generator(H) for H in Hd], Gp=[ref.iso_generator(P) for P in perts],
                init=ref.operator_to_iso_vec(_unitary(rng, N)), cols=N, goal=ref.operator_to_iso_vec(_unitary(rng, N)), kind=kind,
                subspace=subspace, form=form, controls=rng.uniform(-1, 1, (m, T)), dts=rng.uniform(0.1, 0.3, T) if free else 0.2,
                theta=rng.uniform(-0.3, 0.3, (S, p)), scale=rng.uniform(0.9, 1.1, (S, m)) if use_scale else None, samples=list(range(S)))


# ---------------------------------------------------------------------------------------------------------------------------------
#  CPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_scale", [True, False], ids=["scale", "no-scale"])
@pytest.mark.parametrize("free", [True, False], ids=["free-dt", "fixed-dt"])
@pytest.mark.parametrize("fid", [("unitary", None, "abs"), ("unitary", [0, 1], "abs2"), ("ket", None, "abs")], ids=["abs", "abs2-subspace", "ket"])
@pytest.mark.parametrize("N", [2, 3, 8])
def test_reference_routes_agree(N, fid, free, use_scale):
    """Forward mode (expm_frechet) against central differences of the sweep reference: finite-difference accuracy, 1e-6 relative."""
    kind, subspace, form = fid
    rng = np.random.default_rng(10 * N + len(form) + free + 2 * use_scale)
    m, p, T, S = 2, 2, 5, 2
    G0, Gd = ref.iso_generator(_herm(rng, N)), [ref.iso_generator(_herm(rng, N, 0.4)) for _ in range(m)]
    Gp = [ref.iso_generator(_herm(rng, N)) for _ in range(p)]
    controls = rng.uniform(-1, 1, (m, T))
    dts = rng.uniform(0.1, 0.3, T) if free else 0.2
    theta, scale = rng.uniform(-0.3, 0.3, (S, p)), (rng.uniform(0.9, 1.1, (S, m)) if use_scale else None)
    if kind == "unitary":
        init, goal = ref.operator_to_iso_vec(_unitary(rng, N)), ref.operator_to_iso_vec(_unitary(rng, N))
    else:
        v = _unitary(rng, N)
        init, goal = ref.operator_to_iso_vec(v[:, :1]), np.concatenate([v[:, 1].real, v[:, 1].imag])
    args = (G0, Gd, Gp, controls, dts, init, theta, scale, [0, 1], kind, goal, N, subspace, form)
    (terms, a), b = pref.param_terms_forward(*args), pref.param_grad_fd(*args)
    assert terms.shape == (2, T - 1, p + m) and a.shape == b.shape == (2, p + m)
    err = np.abs(a - b).max() / max(1.0, np.abs(a).max())
    print(f"N={N} {fid} free={free} scale={use_scale}: forward vs central differences {err:.2e}, max |g| {np.abs(a).max():.3f}")
    assert err < 1e-6 and np.abs(a).max() > 1e-3


@pytest.mark.parametrize("name", ["qubit", "qutrit", "levels4-3drives", "levels4-5drives", "ket", "one-interval", "qubits3-6drives"])
def test_reference_euler_identity(name):
    """c[s, k] dF_s/dc[s, k] = sum_t a_{t,k} dF_s/da_{t,k}, between this reference and the control gradient's, to 1e-13."""
    c = tg.build(None, name)
    _, sums = reference(c)
    gs = tg.reference(c)
    m, p = c["m"], c["p"]
    scale = np.ones((c["S"], m)) if c["scale"] is None else c["scale"]
    lhs = scale[c["samples"]] * sums[:, p:]
    rhs = np.einsum("kt,stk->sk", c["controls"][:, :c["T"] - 1], gs[:, :, :m])
    err = np.abs(lhs - rhs).max()
    print(f"{name}: Euler identity between the references {err:.2e}")
    assert err <= 1e-13


def test_prototypes_and_header(qc):
    L = qc._lib
    for name, nargs in (("qc_sweep_grad_params", 13), ("qc_sweep_grad_params_dev", 14)):
        assert name in L.SYMBOLS and len(L.SYMBOLS[name][1]) == nargs
        assert getattr(L.lib, name).argtypes is not None
    header = open(os.path.join(ROOT, "include", "qcolloc.h")).read()
    for decl in ("int qc_sweep_grad_params_dev(qc_sweep* h,", "int qc_sweep_grad_params(qc_sweep* h,"):
        assert decl in header
    assert "open-system gradients" in header and "derivatives with respect to theta and\n * `scale`, second" not in header
    assert L.lib.qc_abi_version() == 6      # additive: the ABI stays 0.6
    for what in ("param_grad", "param_grad_device"):
        assert hasattr(qc.RolloutSweep, what)
    assert callable(qc.rollout_sweep_parameter_gradient) and "rollout_sweep_parameter_gradient" in qc.__all__
    julia = open(os.path.join(ROOT, "julia", "QCollocHIP.jl"), encoding="utf-8").read()
    assert "function rollout_sweep_parameter_gradient(" in julia and ":qc_sweep_grad_params, LIB[]" in julia


def test_null_handle_and_python_arguments(qc):
    L = qc._lib
    x = np.zeros(4)
    rc = L.lib.qc_sweep_grad_params(None, L.dptr(x), L.dptr(x), 1, None, None, None, L.dptr(x), None, None, None, None, None)
    assert rc == L.QC_ERR_INVALID and b"qc_sweep_grad_params: NULL handle" in L.lib.qc_sweep_last_error(None)
    rc = L.lib.qc_sweep_grad_params_dev(None, None, None, 1, None, None, None, None, None, None, None, None, None, None)
    assert rc == L.QC_ERR_INVALID and b"qc_sweep_grad_params_dev: NULL handle" in L.lib.qc_sweep_last_error(None)
    rng = np.random.default_rng(0)
    sys2 = qc.QuantumSystem(_herm(rng, 2), [_herm(rng, 2), _herm(rng, 2)])
    init, goal = ref.operator_to_iso_vec(np.eye(2)), ref.operator_to_iso_vec(_unitary(rng, 2))
    with pytest.raises(ValueError, match="controls"):
        qc.rollout_sweep_parameter_gradient(init, np.zeros((3, 5)), 0.2, sys2, [qc.GATES["Z"]], np.zeros((2, 1)), goal=goal)
    with pytest.raises(ValueError, match="controls"):
        qc.rollout_sweep_parameter_gradient(init, np.zeros(5), 0.2, sys2, [qc.GATES["Z"]], np.zeros((2, 1)), goal=goal)
    if not torch.cuda.is_available():       # the arguments are fine: what is missing is the device
        with pytest.raises(qc.QCollocError) as e:
            qc.rollout_sweep_parameter_gradient(init, np.zeros((2, 5)), 0.2, sys2, [qc.GATES["Z"]], np.zeros((2, 1)), goal=goal)
        assert e.value.code == L.QC_ERR_NO_DEVICE


# ---------------------------------------------------------------------------------------------------------------------------------
#  GPU
# ---------------------------------------------------------------------------------------------------------------------------------
def _raw(qc, sw, Z, init, theta, scale, weights=None, want=("fids", "J", "grad", "gs", "gth", "gsc")):
    """One `qc_sweep_grad_params` call with exactly the outputs named in `want`; returns a dict of them."""
    L = qc._lib
    S, theta, scale = sw._samples(theta, scale)
    Z, init = np.ascontiguousarray(Z, dtype=np.float64), np.ascontiguousarray(init, dtype=np.float64)
    out = dict(fids=np.full(S, -7.0), grad=np.full(sw.Z_len, -7.0), gs=np.full((S, sw.T - 1, sw.n_deriv), -7.0), gth=np.full((S, sw.p), -7.0),
               gsc=np.full((S, sw.m), -7.0))
    J = C.c_double(-7.0)
    opt = lambda a: L.dptr(a) if (a is not None and a.size) else None
    get = lambda k: opt(out[k]) if k in want else None
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    rc = L.lib.qc_sweep_grad_params(sw._h, L.dptr(Z), L.dptr(init), S, opt(theta), opt(scale), opt(w), get("fids"), C.byref(J) if "J" in want else None,
                                    get("grad"), get("gs"), get("gth"), get("gsc"))
    if rc != L.QC_OK:
        raise L.QCollocError(rc, L.lib.qc_sweep_last_error(sw._h).decode())
    out["J"] = J.value
    return {k: v for k, v in out.items() if k in want}


def _assert_params(gth, gsc, c, what):
    """Per sample: |got - want| <= 1e-9 max(1, A_s) against the forward-mode reference, on the case's `samples`."""
    terms, sums = reference(c)
    got = np.concatenate([gth, gsc], axis=1)[c["samples"]]
    bound = PAR_RTOL * np.maximum(1.0, magnitudes(terms))
    ratio = (np.abs(got - sums).max(axis=1) / bound).max()
    print(f"SWEEP-PARAM-GRAD {what}: worst |d g| / bound = {ratio:.4f} (max |d g| = {np.abs(got - sums).max():.3e}, max |g| = {np.abs(sums).max():.3e}, "
          f"max A_s = {magnitudes(terms).max():.3f})")
    assert ratio <= 1.0, what
    assert not np.isnan(got).any()


def _check_case(qc, c, sw=None):
    own = sw is None
    sw = ts.make_sweep(qc, c) if own else sw
    try:
        assert sw.kernel_name == "mfma16-sweep" and sw.grad_supported
        Z = sw.pack(c["controls"], c["dts"])
        fids, gth, gsc = sw.param_grad(Z, c["init"], c["theta"], c["scale"])
        assert fids.shape == (c["S"],) and gth.shape == (c["S"], c["p"]) and gsc.shape == (c["S"], c["m"])
        _assert_params(gth, gsc, c, c["name"])
        np.testing.assert_array_equal(fids, sw.eval(Z, c["init"], c["theta"], c["scale"], finals=False)[1])
        return Z, fids, gth, gsc
    finally:
        if own:
            sw.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", PARAM_CASES)
def test_param_grad_matches_the_reference(qc, name):
    c = tg.build(qc, name)
    want = ts.sweep_launch(2 * c["L"], c["m"], c["S"], c["T"])
    if name == "qubit":
        assert (want["chunk"], want["n_chunks"], want["last"]) == (3, 4, 1)
    if name in ("one-chunk", "one-interval"):
        assert want["n_chunks"] == 1
    if name == "long-trajectory":
        assert (want["chunk"], want["n_chunks"], want["last"]) == (32, 32, 7)
        assert magnitudes(reference(c)[0]).max() > 5.0       # the bound's magnitude term is in play here
    _check_case(qc, c)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["no-drives", "sixteen-outputs", "no-perturbations", "no-perturbations-scale", "zeros-in-scale"])
def test_param_grad_new_shapes(qc, shape):
    """Shapes GRAD_CASES does not have: m = 0 with a fixed timestep (no control derivative exists: the control gradient launches no
    walk there, this call must), n_pert = m = 8, no perturbation at all (theta = None), exact zeros in `scale`."""
    if shape == "no-drives":
        c = custom(qc, shape, N=2, m=0, p=2, T=7, S=5, free=False, use_scale=False, seed=41)
    elif shape == "sixteen-outputs":
        c = custom(qc, shape, N=8, m=8, p=8, T=6, S=3, free=True, use_scale=True, seed=42)
    elif shape.startswith("no-perturbations"):
        c = custom(qc, shape, N=2, m=2, p=0, T=7, S=5, free=True, use_scale=shape.endswith("scale"), seed=43)
        if c["scale"] is None:
            c["theta"] = np.zeros((c["S"], 0))
    else:
        c = custom(qc, shape, N=3, m=2, p=1, T=9, S=6, free=True, use_scale=True, seed=44)
        c["scale"][1, 0] = c["scale"][3, 1] = 0.0
        c["scale"][4, :] = 0.0
    sw = ts.make_sweep(qc, c)
    try:
        if shape == "no-drives":
            assert sw.n_deriv == 0
        theta = c["theta"] if (c["p"] or c["scale"] is None) else None        # theta = None: `scale` gives the number of samples
        Z = sw.pack(c["controls"], c["dts"])
        fids, gth, gsc = sw.param_grad(Z, c["init"], theta, c["scale"])
        _assert_params(gth, gsc, c, shape)
        np.testing.assert_array_equal(fids, sw.eval(Z, c["init"], theta, c["scale"], finals=False)[1])
        if shape == "zeros-in-scale":
            assert np.all(np.isfinite(gsc)) and np.all(np.abs(gsc[4]) > 1e-6)      # defined and not zero where c = 0
        if shape == "no-drives":
            J, f2, grad, gth2, gsc2 = sw.param_grad(Z, c["init"], theta, None, with_controls=True)
            np.testing.assert_array_equal(gth2, gth)
            assert np.array_equal(grad.view(np.uint64), np.zeros(grad.size, dtype=np.uint64)) and abs(J - f2.mean()) <= 1e-14
    finally:
        sw.close()


@pytest.mark.gpu
def test_param_grad_through_the_squarings(qc):
    """One case per number of squarings 0 .. 6, built as test_sweep_grad.test_grad_through_the_squarings builds them: the strong theta
    that makes the samples of one call need different numbers is the very parameter being differentiated."""
    rng = np.random.default_rng(17)
    N, m, T, S = 4, 2, 12, 5
    H0, Hd, P = _herm(rng, N), [_herm(rng, N, 0.25) for _ in range(m)], _herm(rng, N)
    controls = rng.uniform(-1, 1, (m, T))
    init, goal = ref.operator_to_iso_vec(_unitary(rng, N)), ref.operator_to_iso_vec(_unitary(rng, N))
    theta = np.array([[0.0], [0.5], [1.5], [4.0], [-9.0]])
    dt = 0.2
    base = max(np.abs(dt * ref.sample_generator(ref.iso_generator(H0), [ref.iso_generator(H) for H in Hd], [], controls[:, t], (), np.ones(m))).sum(axis=0).max()
               for t in range(T - 1))
    seen = set()
    for k in range(7):
        f = 0.09 * 2.0 ** k / base
        sys_ = qc.QuantumSystem(f * H0, [f * H for H in Hd])
        G0, Gd, Gp = ref.iso_generator(f * H0), [ref.iso_generator(f * H) for H in Hd], [ref.iso_generator(f * P)]
        per_sample = [max(ts._squarings(np.abs(dt * ref.sample_generator(G0, Gd, Gp, controls[:, t], theta[s], np.ones(m))).sum(axis=0).max())
                          for t in range(T - 1)) for s in range(S)]
        assert per_sample[0] == k
        seen |= set(per_sample)
        sw = qc.RolloutSweep(sys_, [f * P], T, goal=goal, fid_kind="unitary", dt_fixed=dt)
        c = dict(name=f"squarings {per_sample}", L=N, m=m, p=1, S=S, T=T, G0=G0, Gd=Gd, Gp=Gp, init=init, goal=goal, kind="unitary", subspace=None,
                 form="abs", controls=controls, dts=dt, theta=theta, scale=None, samples=list(range(S)))
        try:
            _check_case(qc, c, sw)
        finally:
            sw.close()
    assert set(range(7)) <= seen


@pytest.mark.gpu
def test_param_grad_identities_on_device_outputs(qc):
    """Between the outputs of ONE call, within 1e-12 max(1, A_s):
    Euler, c[s, k] grad_scale[s, k] = sum_t a_{t,k} grad_samples[s, t, k];
    a perturbation that is a drive's own operator, P_0 = H_drive[0]: c[s, 0] grad_theta[s, 0] = sum_t grad_samples[s, t, 0]."""
    for name in ("qutrit", "qubits3-6drives", "same-as-drive"):
        c = tg.build(qc, name) if name != "same-as-drive" else \
            custom(qc, name, N=4, m=3, p=2, T=10, S=4, free=True, use_scale=True, seed=45, perts=lambda Hd: [Hd[0], _herm(np.random.default_rng(46), 4)])
        sw = ts.make_sweep(qc, c)
        try:
            o = _raw(qc, sw, sw.pack(c["controls"], c["dts"]), c["init"], c["theta"], c["scale"])
        finally:
            sw.close()
        m, T, sel = c["m"], c["T"], c["samples"]
        bound = ID_RTOL * np.maximum(1.0, magnitudes(reference(c)[0]))[:, None]
        scale = np.ones((c["S"], m)) if c["scale"] is None else c["scale"]
        lhs = (scale * o["gsc"])[sel]
        rhs = np.einsum("kt,stk->sk", c["controls"][:, :T - 1], o["gs"][sel][:, :, :m])
        euler = (np.abs(lhs - rhs) / bound).max()
        print(f"SWEEP-PARAM-GRAD {name}: Euler identity, worst |difference| / bound = {euler:.4f}")
        assert euler <= 1.0
        if name == "same-as-drive":
            lhs = (scale[:, 0] * o["gth"][:, 0])[sel]
            rhs = o["gs"][sel][:, :, 0].sum(axis=1)
            same = (np.abs(lhs - rhs) / bound[:, 0]).max()
            print(f"SWEEP-PARAM-GRAD {name}: P_0 = H_drive[0], worst |difference| / bound = {same:.4f}")
            assert same <= 1.0 and np.abs(rhs).max() > 1e-3


@pytest.mark.gpu
def test_param_grad_bits(qc):
    """Repeated calls return the same bits; grad_theta / grad_scale do not depend on which other outputs are requested; fids carry
    the bits of the sweep, J / grad / grad_samples those of the control gradient.  Several chunks (S = 5) and one (S = 2048)."""
    rng = np.random.default_rng(9)
    N, m, p, T = 4, 3, 2, 14
    sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, 0.3) for _ in range(m)])
    goal, init = ref.operator_to_iso_vec(_unitary(rng, N)), ref.operator_to_iso_vec(_unitary(rng, N))
    sw = qc.RolloutSweep(sys_, [_herm(rng, N) for _ in range(p)], T, goal=goal, fid_kind="unitary")
    try:
        Z = sw.pack(rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T))
        for S in (5, 2048):
            theta, scale, w = rng.uniform(-0.3, 0.3, (S, p)), rng.uniform(0.9, 1.1, (S, m)), rng.uniform(0.5, 1.5, S)
            assert (sw.launch(S)[2] == 1) == (S == 2048)
            full = _raw(qc, sw, Z, init, theta, scale, w)
            for _ in range(3):
                again = _raw(qc, sw, Z, init, theta, scale, w)
                assert again["J"] == full["J"]
                for k in ("fids", "grad", "gs", "gth", "gsc"):
                    np.testing.assert_array_equal(again[k], full[k])
            for want in (("gth", "gsc"), ("gth",), ("gsc",), ("fids", "gsc"), ("grad", "gth"), ("gs", "gth", "gsc")):
                part = _raw(qc, sw, Z, init, theta, scale, w, want=want)
                for k in want:
                    np.testing.assert_array_equal(part[k], full[k], err_msg=f"{k} of {want}")
            fids, gth, gsc = sw.param_grad(Z, init, theta, scale)
            np.testing.assert_array_equal(gth, full["gth"])
            np.testing.assert_array_equal(gsc, full["gsc"])
            np.testing.assert_array_equal(fids, sw.eval(Z, init, theta, scale, finals=False)[1])
            np.testing.assert_array_equal(fids, full["fids"])
            J, f, g, gs = sw.grad(Z, init, theta, scale, weights=w, per_sample=True)
            assert J == full["J"]
            for a, b in ((f, full["fids"]), (g, full["grad"]), (gs, full["gs"])):
                np.testing.assert_array_equal(a, b)
            Jc, fc, gc, gthc, gscc = sw.param_grad(Z, init, theta, scale, weights=w, with_controls=True)
            assert Jc == J and np.array_equal(gc, g) and np.array_equal(gthc, gth) and np.array_equal(gscc, gsc)
    finally:
        sw.close()


@pytest.mark.gpu
def test_param_grad_nan_in_one_sample(qc):
    """A NaN in one sample's theta does not raise: that sample's outputs are NaN, every other sample's bits are those of the clean call."""
    rng = np.random.default_rng(10)
    N, m, T, S = 2, 2, 11, 5           # 4 chunks
    sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, 0.5) for _ in range(m)])
    goal, init = ref.operator_to_iso_vec(_unitary(rng, N)), ref.operator_to_iso_vec(_unitary(rng, N))
    sw = qc.RolloutSweep(sys_, [_herm(rng, N)], T, goal=goal, fid_kind="unitary")
    try:
        Z = sw.pack(rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T))
        theta, scale = rng.uniform(-0.3, 0.3, (S, 1)), rng.uniform(0.9, 1.1, (S, m))
        good = sw.param_grad(Z, init, theta, scale)
        assert all(np.isfinite(a).all() for a in good)
        bad = theta.copy()
        bad[2, 0] = np.nan
        got = sw.param_grad(Z, init, bad, scale)
        others = [0, 1, 3, 4]
        for a, b in zip(got, good):
            assert np.isnan(a[2]).all()
            np.testing.assert_array_equal(a[others], b[others])
        for a, b in zip(sw.param_grad(Z, init, theta, scale), good):
            np.testing.assert_array_equal(a, b)
    finally:
        sw.close()


@pytest.mark.gpu
def test_param_grad_device_entry_layout_and_side_stream(qc):
    """`param_grad_device` on torch tensors on a side stream, the layout of test_sweep_grad.test_grad_layout_and_weights (controls at a
    non-zero offset inside a wider knot, global variables behind the knots): the bits of the host entry point and of the minimal
    layout; outputs optional one at a time."""
    rng = np.random.default_rng(5)
    N, m, p, T, S = 2, 2, 1, 9, 6
    sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, 0.5) for _ in range(m)])
    perts = [_herm(rng, N)]
    init, goal = ref.operator_to_iso_vec(_unitary(rng, N)), ref.operator_to_iso_vec(_unitary(rng, N))
    controls, dts = rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T)
    theta, scale, w = rng.uniform(-0.3, 0.3, (S, p)), rng.uniform(0.9, 1.1, (S, m)), rng.uniform(0.5, 1.5, S)
    zdim, off_a, off_dt, gdim = 9, 3, 7, 4
    sw = qc.RolloutSweep(sys_, perts, T, goal=goal, fid_kind="unitary", zdim=zdim, off_a=off_a, off_dt=off_dt, global_dim=gdim)
    plain = qc.RolloutSweep(sys_, perts, T, goal=goal, fid_kind="unitary")
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    mk = lambda *shape: torch.full(shape, -7.0, dtype=torch.float64, device=dev)
    side = torch.cuda.Stream(device=dev)
    try:
        Z = sw.pack(controls, dts)
        Z[Z == 0] = rng.standard_normal(np.count_nonzero(Z == 0))       # what the call does not read is noise, not zeros
        host = _raw(qc, sw, Z, init, theta, scale, w)
        fp, gthp, gscp = plain.param_grad(plain.pack(controls, dts), init, theta, scale)
        for a, b in ((fp, host["fids"]), (gthp, host["gth"]), (gscp, host["gsc"])):
            np.testing.assert_array_equal(a, b)
        dZ, dinit, dth, dsc, dw = t(Z), t(init), t(theta), t(scale), t(w)
        dfid, dJ, dg, dgs, dgth, dgsc = mk(S), mk(1), mk(sw.Z_len), mk(S, T - 1, sw.n_deriv), mk(S, p), mk(S, m)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            sw.param_grad_device(dZ, dinit, S, dth, dsc, dw, dfid, dJ, dg, dgs, dgth, dgsc, stream=side)
        side.synchronize()
        assert dJ.item() == host["J"]
        for a, k in ((dfid, "fids"), (dg, "grad"), (dgs, "gs"), (dgth, "gth"), (dgsc, "gsc")):
            np.testing.assert_array_equal(a.cpu().numpy(), host[k])
        only = mk(S, m)
        sw.param_grad_device(dZ, dinit, S, dth, dsc, dgrad_scale=only, stream=side)
        side.synchronize()
        np.testing.assert_array_equal(only.cpu().numpy(), host["gsc"])
        with pytest.raises(ValueError, match="every output"):
            sw.param_grad_device(dZ, dinit, S, dth, dsc)
        with pytest.raises(ValueError, match="dgrad_theta"):
            sw.param_grad_device(dZ, dinit, S, dth, dsc, dgrad_theta=mk(S, p + 1))
        with pytest.raises(ValueError, match="dtheta"):
            sw.param_grad_device(dZ, dinit, S, None, dsc, dgrad_scale=only)
    finally:
        sw.close()
        plain.close()


@pytest.mark.gpu
def test_param_grad_refused_arguments(qc):
    """All outputs NULL, grad_theta on a handle without perturbations and grad_scale on one without drives are QC_ERR_INVALID with a
    message that says so; the Python layer's own checks."""
    L = qc._lib
    rng = np.random.default_rng(3)
    goal, init = ref.operator_to_iso_vec(_unitary(rng, 2)), ref.operator_to_iso_vec(_unitary(rng, 2))
    no_pert = qc.RolloutSweep(qc.QuantumSystem(_herm(rng, 2), [_herm(rng, 2)]), [], 5, goal=goal, fid_kind="unitary")
    no_drive = qc.RolloutSweep(qc.QuantumSystem(_herm(rng, 2), []), [_herm(rng, 2)], 5, goal=goal, fid_kind="unitary", dt_fixed=0.2)
    try:
        Zp, Zd = no_pert.pack(rng.uniform(-1, 1, (1, 5)), 0.2), no_drive.pack(np.zeros((0, 5)))
        x = np.zeros(8)
        args = lambda Z: (L.dptr(Z), L.dptr(init), 2)
        rc = L.lib.qc_sweep_grad_params(no_pert._h, *args(Zp), None, None, None, None, None, None, None, None, None)
        assert rc == L.QC_ERR_INVALID and b"every output is NULL" in L.lib.qc_sweep_last_error(no_pert._h)
        rc = L.lib.qc_sweep_grad_params(no_pert._h, *args(Zp), None, None, None, None, None, None, None, L.dptr(x), None)
        assert rc == L.QC_ERR_INVALID and b"grad_theta" in L.lib.qc_sweep_last_error(no_pert._h) and b"n_pert = 0" in L.lib.qc_sweep_last_error(no_pert._h)
        rc = L.lib.qc_sweep_grad_params(no_drive._h, *args(Zd), L.dptr(x), None, None, None, None, None, None, None, L.dptr(x))
        assert rc == L.QC_ERR_INVALID and b"grad_scale" in L.lib.qc_sweep_last_error(no_drive._h) and b"m = 0" in L.lib.qc_sweep_last_error(no_drive._h)
        rc = L.lib.qc_sweep_grad_params(no_drive._h, *args(Zd), None, None, None, None, None, None, None, L.dptr(x), None)
        assert rc == L.QC_ERR_INVALID and b"theta is NULL" in L.lib.qc_sweep_last_error(no_drive._h)
        with pytest.raises(ValueError, match="Z has length"):
            no_pert.param_grad(Zp[:-1], init, None, np.ones((2, 1)))
        with pytest.raises(ValueError, match="initial state"):
            no_pert.param_grad(Zp, init[:-1], None, np.ones((2, 1)))
        with pytest.raises(ValueError, match="theta"):
            no_drive.param_grad(Zd, init, np.zeros((2, 2)))
        with pytest.raises(ValueError, match="weights"):
            no_drive.param_grad(Zd, init, np.zeros((2, 1)), weights=np.ones(3))
        # and both handles serve what they have
        f, gth, gsc = no_pert.param_grad(Zp, init, None, np.ones((2, 1)))
        assert gth.shape == (2, 0) and gsc.shape == (2, 1) and np.isfinite(gsc).all()
        f, gth, gsc = no_drive.param_grad(Zd, init, np.array([[0.1], [-0.2]]))
        assert gth.shape == (2, 1) and gsc.shape == (2, 0) and np.isfinite(gth).all()
    finally:
        no_pert.close()
        no_drive.close()


@pytest.mark.gpu
def test_param_grad_refused_handles(qc):
    """The handles the control gradient refuses (test_sweep_grad.test_grad_refused_handles) are refused here with the gradient's own
    reason, while the sweep itself still serves them."""
    L = qc._lib
    made = []
    for name, word in (("open2-S11-T2", "antisymmetric"), ("levels12-S11-T50", "2N = 24"), ("qubit-9drives-S11-T50", "9 drives")):
        c = ts.build_case(qc, name)
        made.append((name, word, ts.make_sweep(qc, c), c))
    rng = np.random.default_rng(2)
    c4 = dict(controls=rng.uniform(-1, 1, (1, 5)), dts=0.2, init=rng.standard_normal(8), theta=np.zeros((2, 0)), scale=None)
    sys4 = qc.QuantumSystem(_herm(rng, 4), [_herm(rng, 4)])
    made.append(("density", "density", qc.RolloutSweep(sys4, [], 5, cols=1, goal=np.array([1.0, 0, 0, 0]), fid_kind="density", dt_fixed=0.2), c4))
    for name, word, sw, c in made:
        try:
            Z = sw.pack(c["controls"], c["dts"])
            with pytest.raises(qc.QCollocError) as e:
                sw.param_grad(Z, c["init"], c["theta"], c["scale"])
            assert e.value.code == L.QC_ERR_UNSUPPORTED and str(e.value).count("qc_sweep gradients: ") == 1 and word in str(e.value), name
            assert sw.grad_unsupported_reason in str(e.value)
            finals, _ = sw.eval(Z, c["init"], c["theta"], c["scale"], fids=False)
            assert np.isfinite(finals).all()
        finally:
            sw.close()


@pytest.mark.gpu
def test_free_function(qc):
    c = tg.build(qc, "qutrit")
    form = qc._lib.QC_FID_FORM_ABS2
    fids, gth, gsc = qc.rollout_sweep_parameter_gradient(c["init"], c["controls"], c["dts"], c["system"], c["perts"], c["theta"], c["scale"],
                                                         goal=c["goal"], fid_kind="unitary", subspace=c["subspace"], fid_form=form)
    _assert_params(gth, gsc, c, "qutrit through rollout_sweep_parameter_gradient")
    _, want = qc.rollout_sweep(c["init"], c["controls"], c["dts"], c["system"], c["perts"], c["theta"], c["scale"], goal=c["goal"],
                               fid_kind="unitary", subspace=c["subspace"], fid_form=form)
    np.testing.assert_array_equal(fids, want)


@pytest.mark.gpu
def test_worst_case_search_example(qc):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import worst_case_search
    grid_worst, found_worst, history = worst_case_search.worst_case(T=20, starts=16, iters=15, verbose=False)
    H = np.array(history)
    assert H.shape == (16, 16)
    print(f"worst infidelity: 9^3 grid {grid_worst:.6e}, 16 ascents {found_worst:.6e}; starts at the grid's worst or better: "
          f"{int(np.sum(H[-1] >= grid_worst - 1e-9))}")
    assert np.all(np.diff(H, axis=0) >= 0)                # no start's infidelity ever decreases
    assert found_worst >= grid_worst - 1e-9
