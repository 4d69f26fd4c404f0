"""Noise-trajectory sweeps (`qc_sweep_noise_*`, `RolloutSweep.noise_eval` / `noise_grad`, `SweepNoiseInfidelityObjective`): S samples of
one pulse whose perturbation amplitudes change from interval to interval, theta[s, j] + noise[s, t, j] in interval t, and the
time-resolved sensitivities dF_s/dnoise[s, t, j].  CPU: the two routes of tests/sweep_noise_reference.py against each other, constant
noise against the sweep reference, the device-free scope query, prototypes, argument validation.  GPU: every output against the
reference, the squarings, exact equalities at zero noise, the resolution identity against the parameter gradient, additive control
noise against single-sample calls, a Lindblad handle, bit-level properties, a NaN, the refusals, the objective and the example.

Tolerances (GPU against the reference) are those of the neighbouring files: states rtol 1e-10 / atol 1e-11 and fidelities 1e-9
(test_sweep.py); every gradient output, `grad_noise` included, per sample |got - want| <= 1e-9 max(1, max |.|) (test_sweep_grad.py: a
gradient entry is a bounded bilinear form in the state x and the adjoint lambda, and grad_noise is the same form against P_j)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import sweep_noise_reference as nref
import sweep_reference as ref
import test_sweep as ts
import test_sweep_grad as tg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAD_RTOL = 1e-9
_herm, _unitary = ts._herm, ts._unitary

# name: (state, levels, m, p, scale given, free timestep, S, T, (kind, subspace, form))
NOISE_CASES = {
    "qubit-S3": ("unitary", 2, 2, 1, False, True, 3, 6, ("unitary", None, "abs")),               # 3 chunks of 2, 2, 1; template M = 4
    "qubit-S40": ("unitary", 2, 2, 1, False, True, 40, 6, ("unitary", None, "abs")),
    "qutrit-ket": ("ket", 3, 1, 2, False, False, 5, 9, ("ket", None, "abs")),                    # padded tile, fixed timestep, M = 4 with a zero slot
    "qubits3-full": ("unitary", 8, 6, 2, True, False, 4, 5, ("unitary", [0, 1, 2], "abs")),      # full tile, M = 8, every slot taken
    "no-drives": ("unitary", 2, 0, 1, False, True, 3, 5, ("unitary", None, "abs")),              # m = 0: every lane reads noise; M = 1
}


def build(qc, name):
    state, L, m, p, use_scale, free, S, T, fid = NOISE_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    H0 = _herm(rng, L)
    Hd = [_herm(rng, L, (L * max(m, 1)) ** -0.5) for _ in range(m)]
    system = qc.QuantumSystem(H0, Hd) if qc is not None else None
    perts = [_herm(rng, L) for _ in range(p)]
    G0, Gd, Gp = ref.iso_generator(H0), [ref.iso_generator(H) for H in Hd], [ref.iso_generator(P) for P in perts]
    kind, subspace, form = fid
    if state == "unitary":
        init, cols, goal = ref.operator_to_iso_vec(_unitary(rng, L)), L, ref.operator_to_iso_vec(_unitary(rng, L))
    else:
        v = _unitary(rng, L)
        init, cols, goal = ref.operator_to_iso_vec(v[:, :1]), 1, np.concatenate([v[:, 1].real, v[:, 1].imag])
    controls = rng.uniform(-1, 1, (m, T))
    dts = rng.uniform(0.1, 0.3, T) if free else 0.2
    theta = rng.uniform(-0.3, 0.3, (S, p))
    scale = rng.uniform(0.9, 1.1, (S, m)) if use_scale else None
    noise = rng.uniform(-0.3, 0.3, (S, T - 1, p))
    return dict(name=name, L=L, m=m, p=p, S=S, T=T, system=system, perts=perts, G0=G0, Gd=Gd, Gp=Gp, init=init, cols=cols, goal=goal, kind=kind,
                subspace=subspace, form=form, controls=controls, dts=dts, theta=theta, scale=scale, noise=noise)


_REFERENCE = {}


def reference(c):
    """(finals, fids, grad_samples, grad_noise) of a case, computed once and shared."""
    key = c["name"]
    if key not in _REFERENCE:
        a = (c["G0"], c["Gd"], c["Gp"], c["controls"], c["dts"], c["init"], c["theta"], c["scale"], c["noise"])
        finals = nref.noise_finals(*a)
        fids = ref.fidelities(finals, c["kind"], c["goal"], c["L"], c["subspace"], c["form"])
        gs, gn = nref.noise_grads_forward(*a, list(range(c["S"])), c["kind"], c["goal"], c["L"], c["subspace"], c["form"])
        for x in (finals, fids, gs, gn):
            x.setflags(write=False)
        _REFERENCE[key] = (finals, fids, gs, gn)
    return _REFERENCE[key]


# ---------------------------------------------------------------------------------------------------------------------------------
#  CPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("free", [True, False], ids=["free-dt", "fixed-dt"])
@pytest.mark.parametrize("fid", [("unitary", None, "abs"), ("unitary", [0, 1], "abs2"), ("ket", None, "abs")], ids=["abs", "abs2-subspace", "ket"])
@pytest.mark.parametrize("N", [2, 3])
def test_reference_routes_agree(N, fid, free):
    """Forward mode (expm_frechet) against central differences of the chain: finite-difference accuracy, 1e-6 relative."""
    kind, subspace, form = fid
    rng = np.random.default_rng(100 * N + len(form) + free)
    m, p, T, S = 2, 2, 5, 2
    G0, Gd = ref.iso_generator(_herm(rng, N)), [ref.iso_generator(_herm(rng, N, 0.4)) for _ in range(m)]
    Gp = [ref.iso_generator(_herm(rng, N)) for _ in range(p)]
    controls = rng.uniform(-1, 1, (m, T))
    dts = rng.uniform(0.1, 0.3, T) if free else 0.2
    theta, scale, noise = rng.uniform(-0.3, 0.3, (S, p)), rng.uniform(0.9, 1.1, (S, m)), rng.uniform(-0.3, 0.3, (S, T - 1, p))
    if kind == "unitary":
        init, goal = ref.operator_to_iso_vec(_unitary(rng, N)), ref.operator_to_iso_vec(_unitary(rng, N))
    else:
        v = _unitary(rng, N)
        init, goal = ref.operator_to_iso_vec(v[:, :1]), np.concatenate([v[:, 1].real, v[:, 1].imag])
    args = (G0, Gd, Gp, controls, dts, init, theta, scale, noise, [0, 1], kind, goal, N, subspace, form)
    (a, an), (b, bn) = nref.noise_grads_forward(*args), nref.noise_grads_fd(*args)
    assert a.shape == b.shape == (2, T - 1, m + free) and an.shape == bn.shape == (2, T - 1, p)
    for what, x, y in (("controls", a, b), ("noise", an, bn)):
        err = np.abs(x - y).max() / max(1.0, np.abs(x).max())
        print(f"N={N} {fid} free={free} {what}: forward vs central differences {err:.2e}, max |grad| {np.abs(x).max():.3f}")
        assert err < 1e-6 and np.abs(x).max() > 1e-3


@pytest.mark.parametrize("name", ["qubit-S3", "qutrit-ket"])
def test_constant_noise_is_a_shifted_theta(name):
    """noise[s, t, j] = delta[s, j] for every t is the sweep at theta + delta: the two references agree to 1e-12.  And the noise
    derivatives summed over t are then the derivative with respect to theta (central differences of the sweep reference)."""
    c = build(None, name)
    rng = np.random.default_rng(3)
    delta = rng.uniform(-0.3, 0.3, (c["S"], c["p"]))
    const = np.repeat(delta[:, None, :], c["T"] - 1, axis=1)
    got = nref.noise_finals(c["G0"], c["Gd"], c["Gp"], c["controls"], c["dts"], c["init"], c["theta"], c["scale"], const)
    want = ref.sweep_finals(c["G0"], c["Gd"], c["Gp"], c["controls"], c["dts"], c["init"], c["theta"] + delta, c["scale"])
    print(f"{name}: constant noise vs shifted theta {np.abs(got - want).max():.2e}")
    assert np.abs(got - want).max() <= 1e-12
    zeros = nref.noise_finals(c["G0"], c["Gd"], c["Gp"], c["controls"], c["dts"], c["init"], None, c["scale"], np.zeros_like(const))
    want0 = ref.sweep_finals(c["G0"], c["Gd"], c["Gp"], c["controls"], c["dts"], c["init"], np.zeros_like(delta), c["scale"])
    assert np.abs(zeros - want0).max() <= 1e-12        # theta = None means zeros
    _, gn = nref.noise_grads_forward(c["G0"], c["Gd"], c["Gp"], c["controls"], c["dts"], c["init"], c["theta"], c["scale"], const, [0], c["kind"],
                                     c["goal"], c["L"], c["subspace"], c["form"])
    F = lambda th: ref.fidelities(ref.sweep_finals(c["G0"], c["Gd"], c["Gp"], c["controls"], c["dts"], c["init"], th, c["scale"]), c["kind"],
                                  c["goal"], c["L"], c["subspace"], c["form"])[0]
    for j in range(c["p"]):
        e = np.zeros_like(delta)
        e[0, j] = 1e-5
        fd = (F(c["theta"] + delta + e) - F(c["theta"] + delta - e)) / 2e-5
        assert abs(gn[0, :, j].sum() - fd) < 1e-6 * max(1.0, abs(fd))


def test_reference_without_drives():
    """m = 0: the noise alone moves the generator.  The two routes agree there too, and the chain is the product of the exponentials."""
    import scipy.linalg as sla
    c = build(None, "no-drives")
    args = (c["G0"], c["Gd"], c["Gp"], c["controls"], c["dts"], c["init"], c["theta"], c["scale"], c["noise"])
    finals = nref.noise_finals(*args)
    X = c["init"].reshape(4, -1, order="F")
    for t in range(c["T"] - 1):
        X = sla.expm(c["dts"][t] * (c["G0"] + (c["theta"][1, 0] + c["noise"][1, t, 0]) * c["Gp"][0])) @ X
    assert np.abs(finals[:, 1] - X.reshape(-1, order="F")).max() <= 1e-14
    tail = ([0, 2], c["kind"], c["goal"], c["L"], c["subspace"], c["form"])
    (a, an), (b, bn) = nref.noise_grads_forward(*args, *tail), nref.noise_grads_fd(*args, *tail)
    assert a.shape == (2, c["T"] - 1, 1) and an.shape == (2, c["T"] - 1, 1)
    assert np.abs(a - b).max() < 1e-6 * max(1.0, np.abs(a).max()) and np.abs(an - bn).max() < 1e-6 * max(1.0, np.abs(an).max())


def _supported(qc, D):
    ok = C.c_int32(-1)
    rc = qc._lib.lib.qc_sweep_desc_noise_supported(C.byref(D.d), C.byref(ok))
    return rc, ok.value, qc._lib.lib.qc_sweep_last_error(None).decode()


def _wide(D):
    D.d.wide = 1
    return D


def test_noise_scope_without_a_device(qc):
    L = qc._lib
    U = L.QC_FID_UNITARY
    open2 = tg._GDesc(qc, N=4, m=2, cols=1, fid_kind=L.QC_FID_DENSITY)        # a Lindblad generator: served, antisymmetric or not
    open2.G0[:] = np.random.default_rng(0).standard_normal(64)
    served = {
        "qubit": tg._GDesc(qc, N=2, m=2, fid_kind=U),
        "m + n_pert = 8": tg._GDesc(qc, N=8, m=6, p=2, fid_kind=U),
        "no drives, 8 perturbations": tg._GDesc(qc, N=2, m=0, p=8, fid_kind=U),
        "7 drives": tg._GDesc(qc, N=4, m=7, p=1),
        "ket": tg._GDesc(qc, N=4, m=2, cols=1, fid_kind=L.QC_FID_KET),
        "open system": open2,
        "17 columns, no fidelity": tg._GDesc(qc, N=2, m=2, cols=17),
        "wide, but 2N <= 16": _wide(tg._GDesc(qc, N=8, m=2, fid_kind=U)),
    }
    for what, D in served.items():
        assert _supported(qc, D)[:2] == (L.QC_OK, 1), what
    refused = {
        "wide": (_wide(tg._GDesc(qc, N=12, m=2, fid_kind=U)), "not served in the mfma32-sweep form"),
        "N = 12": (tg._GDesc(qc, N=12, m=2, fid_kind=U), "rollout-per-sample form (2N = 24 > 16)"),
        "9 drives": (tg._GDesc(qc, N=2, m=9, fid_kind=U), "rollout-per-sample form (9 drives > 8)"),
        "no perturbations": (tg._GDesc(qc, N=2, m=2, p=0, fid_kind=U), "n_pert = 0"),
        "m + n_pert = 9": (tg._GDesc(qc, N=2, m=6, p=3, fid_kind=U), "m + n_pert = 6 + 3"),
        "m + n_pert = 16": (tg._GDesc(qc, N=2, m=8, p=8, fid_kind=U), "m + n_pert = 8 + 8"),
    }
    for what, (D, word) in refused.items():
        rc, ok, msg = _supported(qc, D)
        assert (rc, ok) == (L.QC_OK, 0), what
        assert msg.startswith("qc_sweep noise: ") and word in msg, (what, msg)
    assert _supported(qc, tg._GDesc(qc, T=1))[0] == L.QC_ERR_INVALID       # an invalid descriptor is its own error
    assert L.lib.qc_sweep_desc_noise_supported(C.byref(served["qubit"].d), None) == L.QC_ERR_INVALID


def test_noise_prototypes_and_header(qc):
    L = qc._lib
    for name, nargs in (("qc_sweep_desc_noise_supported", 2), ("qc_sweep_noise_eval", 9), ("qc_sweep_noise_eval_dev", 10),
                        ("qc_sweep_noise_grad", 13), ("qc_sweep_noise_grad_dev", 14)):
        assert name in L.SYMBOLS and len(L.SYMBOLS[name][1]) == nargs
        assert getattr(L.lib, name).argtypes is not None
    header = open(os.path.join(ROOT, "include", "qcolloc.h")).read()
    for decl in ("int qc_sweep_desc_noise_supported(const qc_sweep_desc* d, int32_t* supported);", "int qc_sweep_noise_eval(qc_sweep* h,",
                 "int qc_sweep_noise_eval_dev(qc_sweep* h,", "int qc_sweep_noise_grad(qc_sweep* h,", "int qc_sweep_noise_grad_dev(qc_sweep* h,"):
        assert decl in header
    assert "pullbacks, pushforwards and Hessian products with noise" in header
    assert L.lib.qc_abi_version() == 6      # additive: the ABI stays 0.6
    assert C.sizeof(L.qc_sweep_desc) == L.lib.qc_sizeof_sweep_desc()
    for attr in ("noise_eval", "noise_eval_device", "noise_grad", "noise_grad_device", "noise_supported"):
        assert hasattr(qc.RolloutSweep, attr)
    assert callable(qc.rollout_noise_sweep) and issubclass(qc.SweepNoiseInfidelityObjective, qc.SweepInfidelityObjective)


def test_noise_argument_validation(qc):
    rng = np.random.default_rng(1)
    traj = tg._traj(qc, rng)      # T = 6, two drives
    sys2 = qc.QuantumSystem(_herm(rng, 2), [_herm(rng, 2), _herm(rng, 2)])
    Zop = qc.GATES["Z"]
    mk = lambda **kw: qc.SweepNoiseInfidelityObjective(**{**dict(traj=traj, system=sys2, perturbations=[Zop], noise=np.zeros((3, 5))), **kw})
    with pytest.raises(ValueError, match="noise"):
        mk(noise=None)
    with pytest.raises(ValueError, match="noise must be S x 5 x 1"):
        mk(noise=np.zeros((3, 6)))
    with pytest.raises(ValueError, match="noise must be S x 5 x 2"):
        mk(perturbations=[Zop, Zop], noise=np.zeros((3, 5)))
    with pytest.raises(ValueError, match="theta"):
        mk(theta=np.zeros((3, 2)))
    with pytest.raises(ValueError, match="scale"):
        mk(scale=np.ones((2, 2)))
    with pytest.raises(ValueError, match="weights"):
        mk(weights=np.ones(4))
    with pytest.raises(ValueError, match="no component"):
        mk(state_name="nope")
    with pytest.raises(ValueError, match="n_drives x T"):
        qc.rollout_noise_sweep(np.zeros(8), np.zeros((3, 6)), 0.2, sys2, [Zop], np.zeros((3, 5)))
    # the handle's own normalisation of (noise, theta, scale), which needs no device
    sw = object.__new__(qc.RolloutSweep)
    sw._h, sw.T, sw.p, sw.m = None, 6, 1, 2
    S, noise, theta, scale = sw._noise_samples(np.ones((4, 5)), None, None)
    assert S == 4 and noise.shape == (4, 5, 1) and theta.shape == (4, 1) and not theta.any() and scale is None
    for bad in (None, np.zeros((4, 4)), np.zeros((4, 5, 2)), np.zeros(5), np.zeros((0, 5, 1))):
        with pytest.raises(ValueError, match="noise"):
            sw._noise_samples(bad, None, None)
    with pytest.raises(ValueError, match="samples"):
        sw._noise_samples(np.zeros((4, 5)), np.zeros((3, 1)), None)
    with pytest.raises(ValueError, match="scale"):
        sw._noise_samples(np.zeros((4, 5)), None, np.ones((4, 3)))
    if not torch.cuda.is_available():       # the arguments are fine: what is missing is the device
        with pytest.raises(qc.QCollocError) as e:
            mk()
        assert e.value.code == qc._lib.QC_ERR_NO_DEVICE


# ---------------------------------------------------------------------------------------------------------------------------------
#  GPU
# ---------------------------------------------------------------------------------------------------------------------------------
def _assert_samples(got, want, what):
    """Per sample: |got - want| <= 1e-9 max(1, max |.|)."""
    worst = 0.0
    for q in range(want.shape[0]):
        if want[q].size:
            bound = GRAD_RTOL * max(1.0, np.abs(want[q]).max())
            worst = max(worst, np.abs(got[q] - want[q]).max() / bound)
    mx = np.abs(want).max() if want.size else 0.0
    print(f"SWEEP-NOISE {what}: worst error / bound = {worst:.2e} (max |.| = {mx:.3e})")
    assert worst <= 1.0, what
    assert not np.isnan(got).any()


def _make(qc, c, **kw):
    form = qc._lib.QC_FID_FORM_ABS2 if c["form"] == "abs2" else qc._lib.QC_FID_FORM_ABS
    return qc.RolloutSweep(c["system"], c["perts"], c["T"], cols=c["cols"], goal=c["goal"], fid_kind=c["kind"], subspace=c["subspace"], fid_form=form,
                           dt_fixed=None if np.ndim(c["dts"]) else float(c["dts"]), **kw)


def _check_call(sw, Z, c, weights=None):
    """One evaluation and one gradient call against the reference and against each other."""
    S, T = c["S"], c["T"]
    rf, rfid, rgs, rgn = reference(c)
    finals, fids = sw.noise_eval(Z, c["init"], c["noise"], c["theta"], c["scale"])
    assert finals.shape == rf.shape and fids.shape == (S,)
    ts._assert_states(finals, rf, c["name"])
    ts._assert_fids(fids, rfid, c["name"])
    J, f2, grad, gn, gs = sw.noise_grad(Z, c["init"], c["noise"], c["theta"], c["scale"], weights=weights, per_sample=True)
    assert gs.shape == (S, T - 1, sw.n_deriv) and gn.shape == (S, T - 1, c["p"]) and grad.shape == (sw.Z_len,)
    np.testing.assert_array_equal(f2, fids)             # the seed chains the totals as the final-state launch does
    _assert_samples(gs, rgs, c["name"] + " grad_samples")
    _assert_samples(gn, rgn, c["name"] + " grad_noise")
    assert np.abs(rgn).max() > 1e-3
    w = np.full(S, 1.0 / S) if weights is None else np.asarray(weights)
    assert abs(J - np.dot(w, fids)) <= 1e-14 * max(1.0, np.abs(w).sum())
    want = tg._weighted(gs, w, sw)
    np.testing.assert_allclose(grad, want, rtol=0, atol=1e-12 * max(1.0, np.abs(gs).max() if gs.size else 0.0) * max(1.0, np.abs(w).sum()))
    np.testing.assert_array_equal(grad[want == 0], 0.0)
    # without the per-sample output the handle's own scratch takes its place: the same bits
    J3, f3, g3, gn3 = sw.noise_grad(Z, c["init"], c["noise"], c["theta"], c["scale"], weights=weights)
    assert J3 == J and np.array_equal(f3, fids) and np.array_equal(g3, grad) and np.array_equal(gn3, gn)
    return finals, fids, J, grad, gn, gs


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(NOISE_CASES))
def test_noise_matches_the_reference(qc, name):
    c = build(qc, name)
    sw = _make(qc, c)
    try:
        assert sw.kernel_name == "mfma16-sweep" and sw.noise_supported and sw.noise_unsupported_reason is None and sw.grad_supported
        want = ts.sweep_launch(2 * c["L"], c["m"], c["S"], c["T"])
        assert sw.launch(c["S"]) == (True, want["chunk"], want["n_chunks"])
        if name in ("qubit-S3", "qubit-S40"):
            assert (want["chunk"], want["n_chunks"], want["last"]) == (2, 3, 1)      # several chunks, the last one shorter
        assert want["n_chunks"] > 1
        Z = sw.pack(c["controls"], c["dts"])
        finals, fids = _check_call(sw, Z, c)[:2]
        if name == "qubit-S3":
            _check_call(sw, Z, c, weights=np.array([0.2, 1.5, 0.7]))
            # the one-call form: the same launch
            f3, fid3 = qc.rollout_noise_sweep(c["init"], c["controls"], c["dts"], c["system"], c["perts"], c["noise"], c["theta"], cols=c["cols"],
                                              goal=c["goal"], fid_kind="unitary")
            np.testing.assert_array_equal(f3, finals)
            np.testing.assert_array_equal(fid3, fids)
    finally:
        sw.close()


@pytest.mark.gpu
def test_noise_through_the_squarings(qc):
    """Noise strong enough that the intervals of ONE chunk need 0 .. 7 squarings, differently in every sample: the count is taken per
    wavefront and interval from the generator the noise has entered."""
    rng = np.random.default_rng(23)
    N, m, p, T, S, dt = 2, 1, 1, 8, 4, 0.2
    H0, Hd, P = _herm(rng, N, 0.02), [_herm(rng, N, 0.02)], np.array([[1.0, 0.0], [0.0, -1.0]], dtype=complex)
    system = qc.QuantumSystem(H0, Hd)
    G0, Gd, Gp = ref.iso_generator(H0), [ref.iso_generator(Hd[0])], [ref.iso_generator(P)]
    controls = rng.uniform(-1, 1, (m, T))
    init, goal = ref.operator_to_iso_vec(_unitary(rng, N)), ref.operator_to_iso_vec(_unitary(rng, N))
    # |dt xi| = 0.08 2^k: about k squarings; chunks are intervals 0-2, 3-5, 6
    k = np.array([[0, 3, 6, 1, 2, 4, 5], [6, 0, 7, 2, 2, 2, 2], [1, 1, 1, 5, 0, 6, 3], [0, 0, 0, 0, 0, 0, 4]], dtype=np.float64)
    noise = (0.4 * 2.0 ** k * rng.choice([-1.0, 1.0], (S, T - 1)))[:, :, None]
    theta = np.zeros((S, 1))
    sq = np.array([[ts._squarings(np.abs(dt * nref.interval_generator(G0, Gd, Gp, controls[:, t], theta[s], np.ones(m), noise[s, t])).sum(axis=0).max())
                    for t in range(T - 1)] for s in range(S)])
    launch = ts.sweep_launch(2 * N, m, S, T)
    assert (launch["chunk"], launch["n_chunks"]) == (3, 3)
    print("squarings per sample and interval:\n", sq)
    first = sq[:, :3]                                       # the first chunk of every sample
    assert first[0].min() == 0 and first[0].max() >= 6      # 0 .. at least 6 inside one chunk
    assert len({tuple(r) for r in sq}) == S and len({r.max() for r in first}) >= 3      # and different from sample to sample
    c = dict(name="squarings", L=N, m=m, p=p, S=S, T=T, system=system, perts=[P], G0=G0, Gd=Gd, Gp=Gp, init=init, cols=N, goal=goal, kind="unitary",
             subspace=None, form="abs", controls=controls, dts=dt, theta=theta, scale=None, noise=noise)
    sw = _make(qc, c)
    try:
        assert sw.launch(S) == (True, 3, 3)
        _check_call(sw, sw.pack(controls), c)
    finally:
        sw.close()


@pytest.mark.gpu
def test_zero_noise_is_the_sweep(qc):
    """An explicit +0.0 noise array: finals and fids equal `eval`'s, fids / J / grad / grad_samples equal `grad`'s, value for value
    (np.array_equal: fma(0, P, Ga) may turn a -0 into +0, nothing else).  And the noise derivatives resolve the parameter gradient in
    time: sum_t grad_noise[s, t, j] = grad_theta[s, j] of `param_grad` on the same handle."""
    for name in ("qubit-S3", "qutrit-ket"):
        c = build(qc, name)
        sw = _make(qc, c)
        try:
            Z = sw.pack(c["controls"], c["dts"])
            zero = np.zeros((c["S"], c["T"] - 1, c["p"]))
            assert not np.signbit(zero).any()
            w = np.linspace(0.5, 1.5, c["S"])
            finals, fids = sw.noise_eval(Z, c["init"], zero, c["theta"], c["scale"])
            f0, fid0 = sw.eval(Z, c["init"], c["theta"], c["scale"])
            assert np.array_equal(finals, f0) and np.array_equal(fids, fid0)
            J, f2, grad, gn, gs = sw.noise_grad(Z, c["init"], zero, c["theta"], c["scale"], weights=w, per_sample=True)
            J0, f20, grad0, gs0 = sw.grad(Z, c["init"], c["theta"], c["scale"], weights=w, per_sample=True)
            assert J == J0 and np.array_equal(f2, f20) and np.array_equal(grad, grad0) and np.array_equal(gs, gs0)
            assert np.abs(gs0).max() > 1e-3
            # the resolution identity
            _, gth, _ = sw.param_grad(Z, c["init"], c["theta"], c["scale"])
            tot, mag = gn.sum(axis=1), np.abs(gn).sum(axis=1)
            worst = (np.abs(tot - gth) / (1e-9 * np.maximum(1.0, mag))).max()
            print(f"SWEEP-NOISE {name} resolution identity: worst |sum_t grad_noise - grad_theta| / bound = {worst:.2e}, max |grad_theta| = {np.abs(gth).max():.3e}")
            assert worst <= 1.0 and np.abs(gth).max() > 1e-3
        finally:
            sw.close()


@pytest.mark.gpu
def test_additive_control_noise_against_single_sample_calls(qc):
    """P_0 = G_0: the noise is additive on drive line 0.  One noise sweep against S single-sample sweeps that each carry a_{t,0} + xi[s, t]
    in a trajectory vector of their own -- the loop the entry point replaces."""
    rng = np.random.default_rng(31)
    N, m, T, S = 4, 2, 9, 5
    H0, Hd = _herm(rng, N), [_herm(rng, N, 0.3) for _ in range(m)]
    system = qc.QuantumSystem(H0, Hd)
    init = ref.operator_to_iso_vec(_unitary(rng, N))
    controls, dts = rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T)
    noise = rng.uniform(-0.2, 0.2, (S, T - 1))
    sw = qc.RolloutSweep(system, [Hd[0]], T)
    plain = qc.RolloutSweep(system, [], T)
    try:
        finals, fids = sw.noise_eval(sw.pack(controls, dts), init, noise)
        assert fids is None and finals.shape == (2 * N * N, S)
        for s in range(S):
            cs = controls.copy()
            cs[0, :T - 1] += noise[s]
            one, _ = plain.eval(plain.pack(cs, dts), init, np.zeros((1, 0)))
            ts._assert_states(finals[:, s], one[:, 0], f"additive control noise, sample {s}")
    finally:
        sw.close()
        plain.close()


def _open_case(qc):
    rng = np.random.default_rng(41)
    L, m, T, S = 2, 2, 5, 3
    H0, Hd = _herm(rng, L), [_herm(rng, L, 0.4) for _ in range(m)]
    diss = [0.3 * (rng.standard_normal((L, L)) + 1j * rng.standard_normal((L, L))) / L ** 0.5]
    system = qc.OpenQuantumSystem(H0, Hd, diss)
    Lx = (rng.standard_normal((L, L)) + 1j * rng.standard_normal((L, L))) / L ** 0.5
    perts = [np.asarray(qc.iso_operator(qc.OpenQuantumSystem.dissipator_superoperator(Lx)))]      # a decay channel whose rate fluctuates
    psi = rng.standard_normal(L) + 1j * rng.standard_normal(L)
    psi /= np.linalg.norm(psi)
    g = rng.standard_normal(L) + 1j * rng.standard_normal(L)
    g /= np.linalg.norm(g)
    return dict(name="open2", L=L, m=m, p=1, S=S, T=T, system=system, perts=perts, G0=np.asarray(system.G_drift),
                Gd=[np.asarray(G) for G in system.G_drives], Gp=perts, init=qc.density_to_iso_vec(np.outer(psi, psi.conj())), cols=1,
                goal=np.concatenate([g.real, g.imag]), kind="density", subspace=None, form="abs", controls=rng.uniform(-1, 1, (m, T)),
                dts=rng.uniform(0.1, 0.3, T), theta=rng.uniform(0.1, 0.3, (S, 1)), scale=None, noise=rng.uniform(0.0, 0.2, (S, T - 1, 1)))


@pytest.mark.gpu
def test_noise_on_a_lindblad_handle(qc):
    """N = 4 = 2^2, the density-operator fidelity: the evaluation serves generators that are not antisymmetric; the gradient is refused
    with the gradient's own reason."""
    c = _open_case(qc)
    sw = _make(qc, c)
    try:
        assert sw.N == 4 and sw.kernel_name == "mfma16-sweep" and sw.noise_supported and not sw.grad_supported
        Z = sw.pack(c["controls"], c["dts"])
        finals, fids = sw.noise_eval(Z, c["init"], c["noise"], c["theta"])
        want = nref.noise_finals(c["G0"], c["Gd"], c["Gp"], c["controls"], c["dts"], c["init"], c["theta"], None, c["noise"])
        ts._assert_states(finals, want, "open2 with noise")
        ts._assert_fids(fids, ref.fidelities(want, "density", c["goal"], c["L"]), "open2 with noise")
        with pytest.raises(qc.QCollocError) as e:
            sw.noise_grad(Z, c["init"], c["noise"], c["theta"])
        assert e.value.code == qc._lib.QC_ERR_UNSUPPORTED and "is not antisymmetric" in str(e.value) and "qc_sweep noise: " in str(e.value)
    finally:
        sw.close()


@pytest.mark.gpu
def test_noise_bits_host_device_and_side_stream(qc):
    """Host entry = device entry = device entry on a side stream; repeated calls identical; every output's bits independent of which
    others were requested; S growing, then shrinking, on one handle."""
    c = build(qc, "qubit-S40")
    rng = np.random.default_rng(8)
    sw = _make(qc, c)
    T, m, p = c["T"], c["m"], c["p"]
    Z, init = sw.pack(c["controls"], c["dts"]), c["init"]
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    mk = lambda *shape: torch.full(shape, -7.0, dtype=torch.float64, device=dev)
    side = torch.cuda.Stream(device=dev)
    try:
        for i, S in enumerate((3, 40, 5)):
            theta, scale, w = rng.uniform(-0.3, 0.3, (S, p)), rng.uniform(0.9, 1.1, (S, m)), rng.uniform(0.5, 1.5, S)
            noise = rng.uniform(-0.3, 0.3, (S, T - 1, p))
            finals, fids = sw.noise_eval(Z, init, noise, theta, scale)
            first = sw.noise_grad(Z, init, noise, theta, scale, weights=w, per_sample=True)      # J, fids, grad, grad_noise, grad_samples
            np.testing.assert_array_equal(first[1], fids)
            if i == 1:
                for _ in range(4):
                    again = sw.noise_grad(Z, init, noise, theta, scale, weights=w, per_sample=True)
                    assert again[0] == first[0]
                    for a, b in zip(again[1:], first[1:]):
                        np.testing.assert_array_equal(a, b)
                    f2, fid2 = sw.noise_eval(Z, init, noise, theta, scale)
                    assert np.array_equal(f2, finals) and np.array_equal(fid2, fids)
            dZ, dinit, dth, dsc, dw, dn = t(Z), t(init), t(theta), t(scale), t(w), t(noise)
            torch.cuda.synchronize()
            for stream in (None, side):
                dfin, dfid = mk(S, sw.ns), mk(S)
                dfid2, dJ, dg, dgs, dgn = mk(S), mk(1), mk(sw.Z_len), mk(S, T - 1, sw.n_deriv), mk(S, T - 1, p)
                with torch.cuda.stream(side if stream is not None else torch.cuda.current_stream()):
                    sw.noise_eval_device(dZ, dinit, dn, dth, dsc, dfin, dfid, stream=stream)
                    sw.noise_grad_device(dZ, dinit, dn, dth, dsc, dw, dfid2, dJ, dg, dgs, dgn, stream=stream)
                (side if stream is not None else torch.cuda.current_stream()).synchronize()
                np.testing.assert_array_equal(dfin.cpu().numpy().T, finals)
                np.testing.assert_array_equal(dfid.cpu().numpy(), fids)
                assert dJ.item() == first[0]
                for a, b in zip((dfid2, dg, dgn, dgs), first[1:]):
                    np.testing.assert_array_equal(a.cpu().numpy(), b)
            # outputs are optional one at a time, and none depends on the others
            for k, (key, shape) in enumerate((("dJ", (1,)), ("dfids", (S,)), ("dgrad", (sw.Z_len,)), ("dgrad_noise", (S, T - 1, p)),
                                              ("dgrad_samples", (S, T - 1, sw.n_deriv)))):
                out = mk(*shape)
                sw.noise_grad_device(dZ, dinit, dn, dth, dsc, dw, **{key: out})
                torch.cuda.synchronize()
                np.testing.assert_array_equal(out.cpu().numpy().reshape(np.shape(first[k])), first[k])
            only_f, only_fid = mk(S, sw.ns), mk(S)
            sw.noise_eval_device(dZ, dinit, dn, dth, dsc, dfinals=only_f)
            sw.noise_eval_device(dZ, dinit, dn, dth, dsc, dfids=only_fid)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(only_f.cpu().numpy().T, finals)
            np.testing.assert_array_equal(only_fid.cpu().numpy(), fids)
        # theta = None means zeros on the device entry too
        S = 5
        a = mk(S)
        sw.noise_eval_device(dZ, dinit, dn, None, dsc, dfids=a)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(a.cpu().numpy(), sw.noise_eval(Z, init, noise, None, scale, finals=False)[1])
        with pytest.raises(ValueError):
            sw.noise_eval_device(dZ, dinit, dn[:, :-1].contiguous(), dth, dsc, dfids=a)
        with pytest.raises(ValueError):
            sw.noise_grad_device(dZ, dinit, dn, dth, dsc)
    finally:
        sw.close()


@pytest.mark.gpu
def test_noise_non_finite_input(qc):
    """A NaN at noise[1, 2, 0] of three samples does not raise: samples 0 and 2 carry the bits of the clean run in every per-sample
    output, sample 1 and the sums over the samples are not finite, and the handle then serves a clean call as if nothing had happened."""
    c = build(qc, "qubit-S3")
    sw = _make(qc, c)
    try:
        Z = sw.pack(c["controls"], c["dts"])
        call = lambda noise: sw.noise_eval(Z, c["init"], noise, c["theta"]) + sw.noise_grad(Z, c["init"], noise, c["theta"], per_sample=True)
        good = call(c["noise"])            # finals, fids, J, fids, grad, grad_noise, grad_samples
        assert all(np.isfinite(x).all() for x in good)
        bad = c["noise"].copy()
        bad[1, 2, 0] = np.nan
        finals, fids, J, f2, grad, gn, gs = call(bad)
        for s in (0, 2):
            assert np.array_equal(finals[:, s], good[0][:, s]) and fids[s] == good[1][s] and f2[s] == good[3][s]
            assert np.array_equal(gn[s], good[5][s]) and np.array_equal(gs[s], good[6][s])
        assert np.isnan(finals[:, 1]).all() and np.isnan(fids[1]) and np.isnan(f2[1]) and np.isnan(gn[1]).all() and np.isnan(gs[1]).all()
        assert np.isnan(J) and not np.isfinite(grad).all()
        after = call(c["noise"])
        for a, b in zip(after, good):
            np.testing.assert_array_equal(a, b)
    finally:
        sw.close()


@pytest.mark.gpu
def test_noise_refusals(qc):
    """Handles outside the scope say so with the words of the device-free query, through both entry points, while the sweep itself still
    serves them; and the QC_ERR_INVALID rows of the header."""
    L = qc._lib
    rng = np.random.default_rng(2)
    made = []
    sys12 = qc.QuantumSystem(_herm(rng, 12), [_herm(rng, 12, 0.2)])
    goal12 = ref.operator_to_iso_vec(_unitary(rng, 12))
    sys2 = qc.QuantumSystem(_herm(rng, 2), [_herm(rng, 2, 0.3) for _ in range(6)])
    sys9 = qc.QuantumSystem(_herm(rng, 2), [_herm(rng, 2, 0.3) for _ in range(9)])
    goal2 = ref.operator_to_iso_vec(_unitary(rng, 2))
    T = 5
    made.append(("wide", "not served in the mfma32-sweep form", qc.RolloutSweep(sys12, [_herm(rng, 12)], T, goal=goal12, fid_kind="unitary", wide=True)))
    made.append(("per-sample: size", "rollout-per-sample form (2N = 24 > 16)", qc.RolloutSweep(sys12, [_herm(rng, 12)], T, goal=goal12, fid_kind="unitary")))
    made.append(("per-sample: drives", "rollout-per-sample form (9 drives > 8)", qc.RolloutSweep(sys9, [_herm(rng, 2)], T, goal=goal2, fid_kind="unitary")))
    made.append(("no perturbations", "n_pert = 0", qc.RolloutSweep(sys2, [], T, goal=goal2, fid_kind="unitary")))
    made.append(("nine tiles", "m + n_pert = 6 + 3", qc.RolloutSweep(sys2, [_herm(rng, 2) for _ in range(3)], T, goal=goal2, fid_kind="unitary")))
    for name, word, sw in made:
        try:
            assert not sw.noise_supported and word in sw.noise_unsupported_reason and sw.noise_unsupported_reason.startswith("qc_sweep noise: "), name
            S = 2
            Z = sw.pack(rng.uniform(-1, 1, (sw.m, T)), 0.2)
            init = ref.operator_to_iso_vec(np.eye(sw.N))
            noise, theta = np.zeros((S, T - 1, sw.p)), np.zeros((S, sw.p))
            for call in (sw.noise_eval, sw.noise_grad):
                with pytest.raises(qc.QCollocError) as e:
                    call(Z, init, noise, theta)
                assert e.value.code == L.QC_ERR_UNSUPPORTED and word in str(e.value) and "qc_sweep noise: " in str(e.value), name
            finals, _ = sw.eval(Z, init, theta, fids=False)
            assert np.isfinite(finals).all()
        finally:
            sw.close()
    # QC_ERR_INVALID, on a handle inside the scope and one without a fidelity
    sysq = qc.QuantumSystem(_herm(rng, 2), [_herm(rng, 2), _herm(rng, 2)])
    sw = qc.RolloutSweep(sysq, [qc.GATES["Z"]], T, goal=goal2, fid_kind="unitary")
    bare = qc.RolloutSweep(sysq, [qc.GATES["Z"]], T)
    try:
        S = 3
        Z, init = sw.pack(rng.uniform(-1, 1, (2, T)), 0.2), ref.operator_to_iso_vec(np.eye(2))
        theta, noise = np.zeros((S, 1)), np.zeros(max(S * (T - 1), S * sw.ns, sw.Z_len))
        fin, fid, J = np.empty(S * sw.ns), np.empty(S), C.c_double()
        P = L.dptr
        ev = lambda h, n, a, b: L.lib.qc_sweep_noise_eval(h._h, P(Z), P(init), S, P(theta), None, n, a, b)
        gr = lambda h, n, f=None, j=None, g=None, gs=None, gn=None: L.lib.qc_sweep_noise_grad(h._h, P(Z), P(init), S, P(theta), None, n, None, f, j, g, gs, gn)
        err = lambda h: L.lib.qc_sweep_last_error(h._h).decode()
        assert ev(sw, None, P(fin), P(fid)) == L.QC_ERR_INVALID and "noise is NULL" in err(sw)
        assert gr(sw, None, f=P(fid)) == L.QC_ERR_INVALID and "noise is NULL" in err(sw)
        assert ev(sw, P(noise), P(noise), P(fid)) == L.QC_ERR_INVALID and "noise overlaps an output" in err(sw)
        assert ev(sw, P(noise), P(fin), P(noise[1:])) == L.QC_ERR_INVALID and "noise overlaps an output" in err(sw)
        for kw in (dict(f=P(noise)), dict(g=P(noise[2:])), dict(gn=P(noise)), dict(gs=P(noise[S * (T - 1) - 1:]))):
            assert gr(sw, P(noise), **kw) == L.QC_ERR_INVALID and "noise overlaps an output" in err(sw), list(kw)
        assert gr(sw, P(noise), j=P(noise[3:])) == L.QC_ERR_INVALID and "noise overlaps an output" in err(sw)
        assert ev(sw, P(noise), None, None) == L.QC_ERR_INVALID and "both NULL" in err(sw)
        assert gr(sw, P(noise)) == L.QC_ERR_INVALID and "every output is NULL" in err(sw)
        assert ev(bare, P(noise), P(fin), P(fid)) == L.QC_ERR_INVALID and "created without one" in err(bare)
        assert ev(bare, P(noise), P(fin), None) == L.QC_OK and np.isfinite(fin).all()
        assert L.lib.qc_sweep_noise_eval(sw._h, P(Z), P(init), 0, P(theta), None, P(noise), P(fin), None) == L.QC_ERR_INVALID
        assert L.lib.qc_sweep_noise_eval(sw._h, P(Z), P(init), S, None, None, P(noise), P(fin), None) == L.QC_ERR_INVALID and "theta is NULL" in err(sw)
        assert L.lib.qc_sweep_noise_eval(None, P(Z), P(init), S, P(theta), None, P(noise), P(fin), None) == L.QC_ERR_INVALID
        # a buffer that ends where the noise begins does not overlap it
        both = np.zeros(S * (T - 1) + S)
        assert L.lib.qc_sweep_noise_eval(sw._h, P(Z), P(init), S, P(theta), None, P(both[S:]), None, P(both[:S])) == L.QC_OK
    finally:
        sw.close()
        bare.close()


@pytest.mark.gpu
def test_noise_objective_in_an_evaluator(qc):
    """`SweepNoiseInfidelityObjective` from a trajectory's own layout: L = 1 - w . fids, grad_L = -grad against the handle called by hand and
    against central differences of L itself, and the term inside a first-order `QuantumControlEvaluator`."""
    rng = np.random.default_rng(14)
    N, m, T, S = 2, 2, 8, 5
    traj = tg._traj(qc, rng, N=N, m=m, T=T)
    sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, 0.5) for _ in range(m)])
    noise, scale, w = rng.uniform(-0.2, 0.2, (S, T - 1)), rng.uniform(0.9, 1.1, (S, m)), rng.uniform(0.1, 0.3, S)
    obj = qc.SweepNoiseInfidelityObjective(traj, sys_, [qc.GATES["Z"]], noise, scale=scale, weights=w)
    Z = traj.datavec
    assert obj.hess_structure[0].size == 0 == obj.hess_structure[1].size and obj.S == S
    with pytest.raises(RuntimeError):
        obj.hess_L(Z)
    sw = qc.RolloutSweep(sys_, [qc.GATES["Z"]], T, goal=traj.goal["Ũ⃗"], fid_kind="unitary", zdim=traj.dim, off_a=traj.offset("a"),
                         off_dt=traj.offset("Δt"), global_dim=traj.global_dim)
    try:
        J, fids, grad, gn = sw.noise_grad(Z, traj.initial["Ũ⃗"], noise, None, scale, weights=w)
        assert obj.L(Z) == 1.0 - float(np.dot(w, fids)) and abs(obj.L(Z) - (1.0 - J)) < 1e-14
        np.testing.assert_array_equal(obj.grad_L(Z), -grad)
        np.testing.assert_array_equal(getattr(obj, "∇L")(Z), -grad)
        np.testing.assert_array_equal(obj.noise_sensitivity(Z), gn)
        plain = sw.grad(Z, traj.initial["Ũ⃗"], np.zeros((S, 1)), scale, weights=w)
        assert abs(plain[0] - J) > 1e-6          # the noise is felt
        for k in (2 * traj.dim + traj.offset("a"), 5 * traj.dim + traj.offset("a") + 1, 3 * traj.dim + traj.offset("Δt")):
            e = np.zeros(Z.size)
            e[k] = 1e-5
            fd = (obj.L(Z + e) - obj.L(Z - e)) / 2e-5
            assert abs(fd - obj.grad_L(Z)[k]) < 1e-7, k
    finally:
        sw.close()

    class _Dyn:      # the evaluator reads the dimensions and structures of its dynamics at construction, nothing else here
        class dims:
            Z_len, n_rows, jac_nnz, hess_nnz = Z.size, 0, 0, 0
        dF_structure = (np.empty(0, dtype=np.int64), np.empty(0, dtype=np.int64))
        mu_d2F_structure = (np.empty(0, dtype=np.int64), np.empty(0, dtype=np.int64))

    reg = qc.TrajectoryObjective(qc.QuadraticRegularizer("a", traj, 1e-2) + qc.QuadraticRegularizer("da", traj, 1e-2), traj)
    ev = qc.QuantumControlEvaluator(_Dyn(), [reg, obj], eval_hessian=False)
    g = np.empty(Z.size)
    ev.eval_objective_gradient(g, Z)
    np.testing.assert_array_equal(g, (np.zeros(Z.size) + reg.grad_L(Z)) + obj.grad_L(Z))
    assert ev.eval_objective(Z) == float(reg.L(Z) + obj.L(Z))
    obj.close()


@pytest.mark.gpu
def test_noise_robust_polish_example(qc):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import noise_robust_polish
    before, after, profile = noise_robust_polish.polish(T=8, S=6, max_iter=25, steps=3, verbose=False)
    print(f"mean infidelity over the realisations {before:.3e} -> {after:.3e}; profile {np.array2string(profile, precision=3)}")
    assert after < before
    assert profile.shape == (7,) and np.isfinite(profile).all() and profile.max() > 0
