"""Sweep gradients (`qc_sweep_grad*`, `RolloutSweep.grad`, `SweepInfidelityObjective`): dF_s/da_{t,k} and dF_s/ddt_t of every sample of a
rollout sweep and their weighted sum as a dense gradient over the trajectory vector.  CPU: the two routes of
tests/sweep_grad_reference.py against each other, the device-free scope query, prototypes, header, argument validation.  GPU: every value
of `grad_samples` for a subset of samples against the forward-mode reference, `grad` and `J` against the weighted sum, bit-level
properties, the refused handles, non-finite input, the objective inside an evaluator, the example.

Tolerance (GPU against the reference), per sample: |got - want| <= 1e-9 max(1, max |grad F_s|).  The argument is test_sweep.py's for the
fidelities: the states agree to 1e-10, and a gradient entry is a bounded bilinear form in the state x and the adjoint lambda.
Measured worst errors: profiles/sweep_grad_summary.txt.
Every sample of mid-size and filled launches (S = 97 .. 2049) against the reference: tests/test_sweep_every_sample.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import sweep_grad_reference as gref
import sweep_reference as ref
import test_sweep as ts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAD_RTOL = 1e-9
_herm, _unitary = ts._herm, ts._unitary

# name: (state, levels, m, p, scale given, free timestep, S, T, (kind, subspace, form), samples checked against the reference)
GRAD_CASES = {
    "qubit": ("unitary", 2, 2, 1, False, True, 5, 11, ("unitary", None, "abs"), None),                 # 4 chunks of 3, 3, 3, 1
    "qutrit": ("unitary", 3, 1, 3, True, False, 7, 10, ("unitary", [0, 1], "abs2"), None),             # padded tile
    "qubits3-6drives": ("unitary", 8, 6, 1, True, True, 3, 12, ("unitary", None, "abs"), None),         # full tile, template M = 6
    "qubits3-8drives": ("unitary", 8, 8, 1, False, True, 3, 12, ("unitary", None, "abs2"), None),       # template M = 8
    "levels4-3drives": ("unitary", 4, 3, 1, True, True, 3, 8, ("unitary", None, "abs"), None),          # zero-padded slot of M = 4
    "levels4-5drives": ("unitary", 4, 5, 2, False, False, 3, 8, ("unitary", [0, 1], "abs"), None),      # zero-padded slot of M = 6
    "ket": ("ket", 4, 2, 1, True, True, 11, 6, ("ket", None, "abs"), None),
    "one-interval": ("unitary", 2, 2, 1, False, True, 3, 2, ("unitary", None, "abs"), None),            # T = 2
    "one-chunk": ("unitary", 2, 2, 1, True, True, 2048, 4, ("unitary", None, "abs"), (0, 1000, 2047)),  # n_chunks = 1
    "long-chunk": ("unitary", 2, 2, 1, False, True, 2048, 200, ("unitary", None, "abs"), (0, 1000, 2047)),   # one chunk of 199
    "long-trajectory": ("unitary", 8, 2, 1, True, True, 2, 1000, ("unitary", None, "abs"), None),      # 32 chunks of 32, the last 7
}


def build(qc, name):
    state, L, m, p, use_scale, free, S, T, fid, samples = GRAD_CASES[name]
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
        K = rng.standard_normal((L, 1)) + 1j * rng.standard_normal((L, 1))
        init, cols = ref.operator_to_iso_vec(K / np.linalg.norm(K)), 1
        gk = rng.standard_normal(L) + 1j * rng.standard_normal(L)
        gk /= np.linalg.norm(gk)
        goal = np.concatenate([gk.real, gk.imag])
    controls = rng.uniform(-1, 1, (m, T))
    dts = rng.uniform(0.1, 0.3, T) if free else 0.2
    theta = rng.uniform(-0.3, 0.3, (S, p))
    scale = rng.uniform(0.9, 1.1, (S, m)) if use_scale else None
    return dict(name=name, L=L, m=m, p=p, S=S, T=T, system=system, perts=perts, G0=G0, Gd=Gd, Gp=Gp, init=init, cols=cols, goal=goal, kind=kind,
                subspace=subspace, form=form, controls=controls, dts=dts, theta=theta, scale=scale,
                samples=list(range(S)) if samples is None else list(samples))


def reference(c):
    return gref.grad_samples_forward(c["G0"], c["Gd"], c["Gp"], c["controls"], c["dts"], c["init"], c["theta"], c["scale"], c["samples"], c["kind"],
                                     c["goal"], c["L"], c["subspace"], c["form"])


# ---------------------------------------------------------------------------------------------------------------------------------
#  CPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("free", [True, False], ids=["free-dt", "fixed-dt"])
@pytest.mark.parametrize("fid", [("unitary", None, "abs"), ("unitary", [0, 1], "abs2"), ("ket", None, "abs")], ids=["abs", "abs2-subspace", "ket"])
@pytest.mark.parametrize("N", [2, 3, 8])
def test_reference_routes_agree(N, fid, free):
    """Forward mode (expm_frechet) against central differences of the sweep reference: finite-difference accuracy, 1e-6 relative."""
    kind, subspace, form = fid
    rng = np.random.default_rng(10 * N + len(form) + free)
    m, p, T, S = 2, 1, 5, 2
    G0, Gd, Gp = ref.iso_generator(_herm(rng, N)), [ref.iso_generator(_herm(rng, N, 0.4)) for _ in range(m)], [ref.iso_generator(_herm(rng, N))]
    controls = rng.uniform(-1, 1, (m, T))
    dts = rng.uniform(0.1, 0.3, T) if free else 0.2
    theta, scale = rng.uniform(-0.3, 0.3, (S, p)), rng.uniform(0.9, 1.1, (S, m))
    if kind == "unitary":
        init, goal = ref.operator_to_iso_vec(_unitary(rng, N)), ref.operator_to_iso_vec(_unitary(rng, N))
    else:
        v = _unitary(rng, N)
        init, goal = ref.operator_to_iso_vec(v[:, :1]), np.concatenate([v[:, 1].real, v[:, 1].imag])
    args = (G0, Gd, Gp, controls, dts, init, theta, scale, [0, 1], kind, goal, N, subspace, form)
    a, b = gref.grad_samples_forward(*args), gref.grad_samples_fd(*args)
    assert a.shape == b.shape == (2, T - 1, m + free)
    err = np.abs(a - b).max() / max(1.0, np.abs(a).max())
    print(f"N={N} {fid} free={free}: forward vs central differences {err:.2e}, max |grad| {np.abs(a).max():.3f}")
    assert err < 1e-6 and np.abs(a).max() > 1e-3


class _GDesc(ts._Desc):
    """ts._Desc (zero matrices: antisymmetric) with a goal long enough for every kind."""

    def __init__(self, qc, **kw):
        super().__init__(qc, **kw)
        self.goal = np.zeros(2 * self.d.N * self.d.N + 2)
        self.d.goal_iso = qc._lib.dptr(self.goal)


def _supported(qc, D):
    ok = C.c_int32(-1)
    rc = qc._lib.lib.qc_sweep_desc_grad_supported(C.byref(D.d), C.byref(ok))
    return rc, ok.value, qc._lib.lib.qc_sweep_last_error(None).decode()


def test_grad_scope_without_a_device(qc):
    L = qc._lib
    U = L.QC_FID_UNITARY
    served = {
        "qubit": _GDesc(qc, N=2, m=2, fid_kind=U),
        "qutrit with subspace": _GDesc(qc, N=3, m=1, p=3, fid_kind=U, fid_form=L.QC_FID_FORM_ABS2, subspace=[0, 1]),
        "3 qubits, 8 drives": _GDesc(qc, N=8, m=8, fid_kind=U),
        "ket": _GDesc(qc, N=4, m=2, cols=1, fid_kind=L.QC_FID_KET),
    }
    for what, D in served.items():
        assert _supported(qc, D)[:2] == (L.QC_OK, 1), what
    # iso generators of Hermitian operators pass the antisymmetry test; a symmetric part of 1e-12 does not
    rng = np.random.default_rng(0)
    D = _GDesc(qc, N=3, m=1, fid_kind=U)
    D.G0[:] = ref.iso_generator(_herm(rng, 3)).reshape(-1, order="F")
    D.Gd[:] = ref.iso_generator(_herm(rng, 3)).reshape(-1, order="F")
    assert _supported(qc, D)[:2] == (L.QC_OK, 1)
    D.Gd[1] += 1e-12
    rc, ok, msg = _supported(qc, D)
    assert (rc, ok) == (L.QC_OK, 0) and "antisymmetric" in msg and "drive" in msg
    open2 = _GDesc(qc, N=4, m=2, cols=1, fid_kind=L.QC_FID_DENSITY)        # a Lindblad generator: n = 8, not antisymmetric
    open2.G0[:] = rng.standard_normal(64)
    refused = {
        "open2": (open2, "antisymmetric"),
        "N = 12": (_GDesc(qc, N=12, m=2, fid_kind=U), "2N = 24"),
        "9 drives": (_GDesc(qc, N=2, m=9, fid_kind=U), "9 drives"),
        "no fidelity": (_GDesc(qc, N=2, m=2), "no fidelity"),
        "density": (_GDesc(qc, N=4, m=2, cols=1, fid_kind=L.QC_FID_DENSITY), "density"),
        "17 columns": (_GDesc(qc, N=2, m=2, cols=17), "16 columns"),
    }
    for what, (D, word) in refused.items():
        rc, ok, msg = _supported(qc, D)
        assert (rc, ok) == (L.QC_OK, 0), what
        assert msg.startswith("qc_sweep gradients:") and word in msg, (what, msg)
    # an invalid descriptor is its own error
    assert _supported(qc, _GDesc(qc, T=1))[0] == L.QC_ERR_INVALID
    assert L.lib.qc_sweep_desc_grad_supported(C.byref(served["qubit"].d), None) == L.QC_ERR_INVALID


def test_grad_prototypes_and_header(qc):
    L = qc._lib
    for name, nargs in (("qc_sweep_desc_grad_supported", 2), ("qc_sweep_grad", 11), ("qc_sweep_grad_dev", 12)):
        assert name in L.SYMBOLS and len(L.SYMBOLS[name][1]) == nargs
        assert getattr(L.lib, name).argtypes is not None
    header = open(os.path.join(ROOT, "include", "qcolloc.h")).read()
    for decl in ("int qc_sweep_desc_grad_supported(const qc_sweep_desc* d, int32_t* supported);", "int qc_sweep_grad_dev(qc_sweep* h,",
                 "int qc_sweep_grad(qc_sweep* h,"):
        assert decl in header
    assert "open-system gradients" in header and "Out of scope: per-knot outputs, gradients" not in header
    assert L.lib.qc_abi_version() == 6      # additive: the ABI stays 0.6
    assert C.sizeof(L.qc_sweep_desc) == L.lib.qc_sizeof_sweep_desc()
    assert hasattr(qc.RolloutSweep, "grad") and hasattr(qc.RolloutSweep, "grad_device") and hasattr(qc.RolloutSweep, "grad_supported")


def _traj(qc, rng, N=2, m=2, T=6, free=True, ket=False, extra=2):
    comps = {}
    if ket:
        v = _unitary(rng, N)
        comps["ψ̃"] = np.repeat(np.concatenate([v[:, 0].real, v[:, 0].imag])[:, None], T, axis=1)
        goal = {"ψ̃": np.concatenate([v[:, 1].real, v[:, 1].imag])}
        initial = {"ψ̃": comps["ψ̃"][:, 0].copy()}
    else:
        comps["Ũ⃗"] = np.repeat(ref.operator_to_iso_vec(np.eye(N))[:, None], T, axis=1)
        goal = {"Ũ⃗": ref.operator_to_iso_vec(_unitary(rng, N))}
        initial = {"Ũ⃗": comps["Ũ⃗"][:, 0].copy()}
    if extra:
        comps["pad"] = rng.standard_normal((extra, T))
    comps["a"] = rng.uniform(-1, 1, (m, T))
    comps["da"] = rng.standard_normal((m, T))
    if free:
        comps["Δt"] = rng.uniform(0.1, 0.3, (1, T))
    return qc.NamedTrajectory(comps, controls=("da",), timestep="Δt" if free else 0.2, initial=initial, goal=goal,
                              global_data={"φ": np.array([0.3, -0.2, 0.1])})


def test_objective_argument_validation(qc):
    rng = np.random.default_rng(1)
    traj = _traj(qc, rng)
    sys2 = qc.QuantumSystem(_herm(rng, 2), [_herm(rng, 2), _herm(rng, 2)])
    Zop = qc.GATES["Z"]
    mk = lambda **kw: qc.SweepInfidelityObjective(**{**dict(traj=traj, system=sys2, perturbations=[Zop], theta=np.zeros((3, 1))), **kw})
    with pytest.raises(ValueError, match="no component"):
        mk(state_name="nope")
    with pytest.raises(ValueError, match="no component"):
        mk(control_name="nope")
    with pytest.raises(ValueError, match="drives"):
        mk(system=qc.QuantumSystem(_herm(rng, 2), [_herm(rng, 2)]))
    with pytest.raises(ValueError, match="neither"):
        mk(system=qc.QuantumSystem(_herm(rng, 3), [_herm(rng, 3), _herm(rng, 3)]))
    with pytest.raises(ValueError, match="theta"):
        mk(theta=np.zeros((3, 2)))
    with pytest.raises(ValueError, match="scale"):
        mk(scale=np.ones((2, 2)))
    with pytest.raises(ValueError, match="weights"):
        mk(weights=np.ones(4))
    with pytest.raises(ValueError, match="form"):
        mk(form="abs3")
    with pytest.raises(ValueError, match="unitary component only"):
        qc.SweepInfidelityObjective(_traj(qc, rng, ket=True), sys2, [Zop], np.zeros((3, 1)), state_name="ψ̃", subspace=[0])
    if not torch.cuda.is_available():       # the arguments are fine: what is missing is the device
        with pytest.raises(qc.QCollocError) as e:
            mk()
        assert e.value.code == qc._lib.QC_ERR_NO_DEVICE


# ---------------------------------------------------------------------------------------------------------------------------------
#  GPU
# ---------------------------------------------------------------------------------------------------------------------------------
def _assert_samples(got, want, what):
    """Per sample: |got - want| <= 1e-9 max(1, max |grad F_s|)."""
    worst = 0.0
    for q in range(want.shape[0]):
        bound = GRAD_RTOL * max(1.0, np.abs(want[q]).max())
        worst = max(worst, np.abs(got[q] - want[q]).max() / bound)
    print(f"SWEEP-GRAD {what}: worst |d grad| / bound = {worst:.4f} (max |d grad| = {np.abs(got - want).max():.3e}, max |grad| = {np.abs(want).max():.3e})")
    assert worst <= 1.0, what
    assert not np.isnan(got).any()


def _weighted(gs, w, sw):
    """The dense gradient a weighted sum of per-sample derivatives gives, in the handle's layout."""
    T = sw.T
    out = np.zeros(sw.Z_len)
    K = out[:T * sw.zdim].reshape(T, sw.zdim)
    tot = np.tensordot(w, gs, axes=(0, 0))
    K[:T - 1, sw.off_a:sw.off_a + sw.m] = tot[:, :sw.m]
    if sw.off_dt >= 0:
        K[:T - 1, sw.off_dt] = tot[:, sw.m]
    return out


def _check_call(sw, Z, c, weights=None):
    """One gradient call against the reference and against itself: per-sample values, fidelities (the bits of the sweep), J, grad."""
    J, fids, grad, gs = sw.grad(Z, c["init"], c["theta"], c["scale"], weights=weights, per_sample=True)
    S = c["S"]
    assert gs.shape == (S, c["T"] - 1, sw.n_deriv) and grad.shape == (sw.Z_len,) and fids.shape == (S,)
    _assert_samples(gs[c["samples"]], reference(c), c["name"])
    np.testing.assert_array_equal(fids, sw.eval(Z, c["init"], c["theta"], c["scale"], finals=False)[1])
    w = np.full(S, 1.0 / S) if weights is None else np.asarray(weights)
    assert abs(J - np.dot(w, fids)) <= 1e-14 * max(1.0, np.abs(w).sum())
    want = _weighted(gs, w, sw)
    np.testing.assert_allclose(grad, want, rtol=0, atol=1e-12 * max(1.0, np.abs(gs).max()) * max(1.0, np.abs(w).sum()))
    np.testing.assert_array_equal(grad[want == 0], 0.0)
    assert not np.signbit(grad[want == 0]).any()
    # without the per-sample output the handle's own scratch takes its place: the same bits
    J2, f2, g2 = sw.grad(Z, c["init"], c["theta"], c["scale"], weights=weights)
    assert J2 == J and np.array_equal(f2, fids) and np.array_equal(g2, grad)
    return J, fids, grad, gs


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GRAD_CASES))
def test_grad_matches_the_reference(qc, name):
    c = build(qc, name)
    sw = ts.make_sweep(qc, c)
    try:
        assert sw.kernel_name == "mfma16-sweep" and sw.grad_supported and sw.grad_unsupported_reason is None
        want = ts.sweep_launch(2 * c["L"], c["m"], c["S"], c["T"])
        assert sw.launch(c["S"]) == (True, want["chunk"], want["n_chunks"])
        if name == "qubit":
            assert (want["chunk"], want["n_chunks"], want["last"]) == (3, 4, 1)
        if name in ("one-chunk", "long-chunk", "one-interval"):
            assert want["n_chunks"] == 1
        if name == "long-trajectory":
            assert (want["chunk"], want["n_chunks"], want["last"]) == (32, 32, 7)
        _check_call(sw, sw.pack(c["controls"], c["dts"]), c)
    finally:
        sw.close()


@pytest.mark.gpu
def test_grad_through_the_squarings(qc):
    """One case per number of squarings 0 .. 6, the system scaled as test_sweep_generator_norms scales it: a strong perturbation makes
    the samples of one call need different numbers."""
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
        c = dict(name=f"squarings {per_sample}", L=N, m=m, S=S, T=T, G0=G0, Gd=Gd, Gp=Gp, init=init, goal=goal, kind="unitary", subspace=None, form="abs",
                 controls=controls, dts=dt, theta=theta, scale=None, samples=list(range(S)))
        try:
            _check_call(sw, sw.pack(controls), c)
        finally:
            sw.close()
    assert set(range(7)) <= seen


@pytest.mark.gpu
def test_grad_layout_and_weights(qc):
    """Controls at a non-zero offset inside a wider knot, the timestep elsewhere, global variables behind the knots: every entry of
    `grad` that is not a control or a timestep of knots 0 .. T-2 is +0.0 bit for bit.  Non-uniform weights; weights = None against
    1/S written out."""
    rng = np.random.default_rng(5)
    N, m, p, T, S = 2, 2, 1, 9, 6
    sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, 0.5) for _ in range(m)])
    perts = [_herm(rng, N)]
    init, goal = ref.operator_to_iso_vec(_unitary(rng, N)), ref.operator_to_iso_vec(_unitary(rng, N))
    controls, dts = rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T)
    theta, scale = rng.uniform(-0.3, 0.3, (S, p)), rng.uniform(0.9, 1.1, (S, m))
    c = dict(name="layout", L=N, m=m, S=S, T=T, G0=np.asarray(sys_.G_drift),
             Gd=[np.asarray(G) for G in sys_.G_drives], Gp=[ref.iso_generator(perts[0])], init=init, goal=goal, kind="unitary", subspace=None,
             form="abs", controls=controls, dts=dts, theta=theta, scale=scale, samples=list(range(S)))
    zdim, off_a, off_dt, gdim = 9, 3, 7, 4
    sw = qc.RolloutSweep(sys_, perts, T, goal=goal, fid_kind="unitary", zdim=zdim, off_a=off_a, off_dt=off_dt, global_dim=gdim)
    plain = qc.RolloutSweep(sys_, perts, T, goal=goal, fid_kind="unitary")
    try:
        Z = sw.pack(controls, dts)
        Z[Z == 0] = rng.standard_normal(np.count_nonzero(Z == 0))       # what the gradient does not read is noise, not zeros
        assert Z.size == T * zdim + gdim
        J, fids, grad, gs = _check_call(sw, Z, c)
        K = grad[:T * zdim].reshape(T, zdim)
        mask = np.ones((T, zdim), dtype=bool)
        mask[:T - 1, off_a:off_a + m] = False
        mask[:T - 1, off_dt] = False
        for zero in (K[mask], grad[T * zdim:], K[T - 1]):
            assert np.array_equal(zero.view(np.uint64), np.zeros(zero.size, dtype=np.uint64))
        assert np.all(K[~mask] != 0)
        # the minimal layout gives the same per-sample bits
        Jp, fp, gp, gsp = plain.grad(plain.pack(controls, dts), init, theta, scale, per_sample=True)
        np.testing.assert_array_equal(gsp, gs)
        np.testing.assert_array_equal(fp, fids)
        # weights
        w = rng.uniform(0.0, 2.0, S)
        Jw, fw, gw, gsw = _check_call(sw, Z, c, weights=w)
        np.testing.assert_array_equal(gsw, gs)
        assert abs(Jw - J) > 1e-6
        Ju, fu, gu = sw.grad(Z, init, theta, scale, weights=np.full(S, 1.0 / S))
        assert Ju == J and np.array_equal(gu, grad)
    finally:
        sw.close()
        plain.close()


@pytest.mark.gpu
def test_grad_bits_host_device_and_side_stream(qc):
    """Six repeated calls return identical bits; the host and device entry points return identical bits; one handle on a side stream
    with growing S."""
    rng = np.random.default_rng(8)
    N, m, T = 8, 6, 120
    sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, (N * m) ** -0.5) for _ in range(m)])
    goal = ref.operator_to_iso_vec(_unitary(rng, N))
    sw = qc.RolloutSweep(sys_, [_herm(rng, N)], T, goal=goal, fid_kind="unitary")
    Z = sw.pack(rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T))
    init = ref.operator_to_iso_vec(_unitary(rng, N))
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    side = torch.cuda.Stream(device=dev)
    try:
        for i, S in enumerate((5, 300, 40)):          # growing S reallocates the handle's scratch; a smaller S afterwards reuses it
            theta, scale, w = rng.uniform(-0.3, 0.3, (S, 1)), rng.uniform(0.9, 1.1, (S, m)), rng.uniform(0.5, 1.5, S)
            first = sw.grad(Z, init, theta, scale, weights=w, per_sample=True)
            if i == 1:
                for _ in range(6):
                    again = sw.grad(Z, init, theta, scale, weights=w, per_sample=True)
                    assert again[0] == first[0]
                    for a, b in zip(again[1:], first[1:]):
                        np.testing.assert_array_equal(a, b)
            dZ, dinit, dth, dsc, dw = t(Z), t(init), t(theta), t(scale), t(w)
            mk = lambda *shape: torch.full(shape, -7.0, dtype=torch.float64, device=dev)
            dfid, dJ, dg, dgs = mk(S), mk(1), mk(sw.Z_len), mk(S, T - 1, sw.n_deriv)
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                sw.grad_device(dZ, dinit, S, dth, dsc, dw, dfid, dJ, dg, dgs, stream=side)
            side.synchronize()
            assert dJ.item() == first[0]
            for a, b in zip((dfid, dg, dgs), first[1:]):
                np.testing.assert_array_equal(a.cpu().numpy(), b)
            # outputs are optional one at a time
            dg2 = mk(sw.Z_len)
            sw.grad_device(dZ, dinit, S, dth, dsc, dw, dgrad=dg2, stream=side)
            side.synchronize()
            np.testing.assert_array_equal(dg2.cpu().numpy(), first[2])
        with pytest.raises(ValueError):
            sw.grad_device(t(Z), t(init), 3, t(np.zeros((3, 1))))
    finally:
        sw.close()


@pytest.mark.gpu
def test_grad_refused_handles(qc):
    """Every handle outside the scope says so: `grad_supported` is False with a reason, and the gradient call returns
    QC_ERR_UNSUPPORTED with that reason, while the sweep itself still serves the handle."""
    L = qc._lib
    made = []
    for name, word in (("open2-S11-T2", "antisymmetric"), ("levels12-S11-T50", "2N = 24"), ("qubit-9drives-S11-T50", "9 drives"),
                       ("kets3-S11-T102", "no fidelity")):
        c = ts.build_case(qc, name)
        made.append((name, word, ts.make_sweep(qc, c), c))
    rng = np.random.default_rng(2)
    sys2 = qc.QuantumSystem(_herm(rng, 2), [_herm(rng, 2)])
    c17 = dict(controls=rng.uniform(-1, 1, (1, 5)), dts=0.2, init=rng.standard_normal(4 * 17), theta=np.zeros((2, 0)), scale=None)
    made.append(("17 columns", "16 columns", qc.RolloutSweep(sys2, [], 5, cols=17, dt_fixed=0.2), c17))
    # a closed system with the density fidelity: an antisymmetric generator of N = 4 = 2^2 "levels"
    c4 = dict(controls=rng.uniform(-1, 1, (1, 5)), dts=0.2, init=rng.standard_normal(8), theta=np.zeros((2, 0)), scale=None)
    sys4 = qc.QuantumSystem(_herm(rng, 4), [_herm(rng, 4)])
    made.append(("density", "density", qc.RolloutSweep(sys4, [], 5, cols=1, goal=np.array([1.0, 0, 0, 0]), fid_kind="density", dt_fixed=0.2), c4))
    for name, word, sw, c in made:
        try:
            assert not sw.grad_supported and word in sw.grad_unsupported_reason, name
            Z = sw.pack(c["controls"], c["dts"])
            with pytest.raises(qc.QCollocError) as e:
                sw.grad(Z, c["init"], c["theta"], c["scale"])
            assert e.value.code == L.QC_ERR_UNSUPPORTED and word in str(e.value), name
            finals, _ = sw.eval(Z, c["init"], c["theta"], c["scale"], fids=False)
            assert np.isfinite(finals).all()
        finally:
            sw.close()


@pytest.mark.gpu
def test_grad_non_finite_input(qc):
    """One NaN control does not raise.  In the last knot it reaches nothing: the bits of the clean call.  Inside the trajectory it reaches
    every sample (the controls are shared): fidelities and derivatives are NaN, the entries that are no derivative stay +0.0, and the
    handle then serves a finite call as if nothing had happened."""
    rng = np.random.default_rng(4)
    N, m, T, S = 4, 2, 30, 6
    sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, 0.3) for _ in range(m)])
    goal = ref.operator_to_iso_vec(_unitary(rng, N))
    zdim = m + 3
    sw = qc.RolloutSweep(sys_, [_herm(rng, N)], T, goal=goal, fid_kind="unitary", zdim=zdim, off_a=1, off_dt=m + 2, global_dim=2)
    try:
        controls, dts = rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T)
        init, theta = ref.operator_to_iso_vec(_unitary(rng, N)), rng.uniform(-0.3, 0.3, (S, 1))
        good = sw.grad(sw.pack(controls, dts), init, theta, per_sample=True)
        assert np.isfinite(good[2]).all() and np.isfinite(good[3]).all()
        bad = controls.copy()
        bad[0, T - 1] = np.nan
        again = sw.grad(sw.pack(bad, dts), init, theta, per_sample=True)
        assert again[0] == good[0]
        for a, b in zip(again[1:], good[1:]):
            np.testing.assert_array_equal(a, b)
        bad = controls.copy()
        bad[1, 7] = np.nan
        J, fids, grad, gs = sw.grad(sw.pack(bad, dts), init, theta, per_sample=True)
        assert np.isnan(J) and np.isnan(fids).all() and np.isnan(gs).all()
        K = grad[:T * zdim].reshape(T, zdim)
        assert np.isnan(K[:T - 1, 1:1 + m]).all() and np.isnan(K[:T - 1, m + 2]).all()
        for zero in (K[:, 0], K[:, m + 1], K[T - 1], grad[T * zdim:]):
            assert np.array_equal(zero.view(np.uint64), np.zeros(zero.size, dtype=np.uint64))
        after = sw.grad(sw.pack(controls, dts), init, theta, per_sample=True)
        for a, b in zip(after[1:], good[1:]):
            np.testing.assert_array_equal(a, b)
    finally:
        sw.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ket", [False, True], ids=["unitary", "ket"])
def test_objective_in_an_evaluator(qc, ket):
    """`SweepInfidelityObjective` from a trajectory's own layout: L = 1 - J, grad_L = -grad against the sweep handle called by hand, and
    inside a first-order `QuantumControlEvaluator` the objective gradient is the other terms' plus this term's."""
    rng = np.random.default_rng(12 + ket)
    N, m, T, S = 2, 2, 8, 5
    traj = _traj(qc, rng, N=N, m=m, T=T, ket=ket)
    name = "ψ̃" if ket else "Ũ⃗"
    sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, 0.5) for _ in range(m)])
    theta, scale, w = rng.uniform(-0.2, 0.2, (S, 1)), rng.uniform(0.9, 1.1, (S, m)), rng.uniform(0.1, 0.3, S)
    obj = qc.SweepInfidelityObjective(traj, sys_, [qc.GATES["Z"]], theta, scale, w, state_name=name)
    Z = traj.datavec
    assert obj.hess_structure[0].size == 0 == obj.hess_structure[1].size
    with pytest.raises(RuntimeError):
        obj.hess_L(Z)
    sw = qc.RolloutSweep(sys_, [qc.GATES["Z"]], T, cols=1 if ket else N, goal=traj.goal[name], fid_kind="ket" if ket else "unitary",
                         zdim=traj.dim, off_a=traj.offset("a"), off_dt=traj.offset("Δt"), global_dim=traj.global_dim)
    try:
        J, fids, grad = sw.grad(Z, traj.initial[name], theta, scale, weights=w)
        assert obj.L(Z) == 1.0 - float(np.dot(w, fids)) and abs(obj.L(Z) - (1.0 - J)) < 1e-14
        np.testing.assert_array_equal(obj.grad_L(Z), -grad)
        np.testing.assert_array_equal(getattr(obj, "∇L")(Z), -grad)
        # against central differences of the objective itself
        k = 2 * traj.dim + traj.offset("a")
        e = np.zeros(Z.size)
        e[k] = 1e-5
        fd = (obj.L(Z + e) - obj.L(Z - e)) / 2e-5
        assert abs(fd - obj.grad_L(Z)[k]) < 1e-7
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
    with pytest.raises(RuntimeError):
        ev.eval_hessian_lagrangian(np.empty(ev.hess_nnz), Z, 1.0, np.empty(0))
    obj.close()


@pytest.mark.gpu
def test_robust_polish_example(qc):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import robust_polish
    before, after = robust_polish.polish(T=20, grid=5, max_iter=25, steps=20, verbose=False)
    print(f"mean infidelity over the grid {before:.3e} -> {after:.3e}")
    assert after < before
