"""Open-system sweep gradients: reverse mode by the stored-state walk (`qc_sweep_desc.reserved1[0] = QC_SWEEP_STORED_STATES`,
`RolloutSweep(stored_states=True)`, qc_sweep_open_grad.hip).  `qc_sweep_grad*`, `qc_sweep_grad_params*` and `qc_sweep_vjp*` on Lindblad
generators (density fidelity) and on non-Hermitian effective Hamiltonians (unitary / ket fidelities), which the closed walk refuses.

CPU: the flag through `qc_sweep_desc_validate` and the scope queries, the keyword's default, the restated generators against the
package's, and the self-check of the reference (forward mode against central differences, 1e-6) on the systems the GPU cases use.
GPU: every value against the forward-mode reference (tests/sweep_open_reference.py: scipy.linalg.expm_frechet per interval).

Tolerance, the project's own (tests/test_sweep_grad.py): per sample |got - want| <= 1e-9 max(1, max |want of that sample|).  `fids` and
`finals` are compared with `qc_sweep_eval` bit for bit.  Measured worst errors: profiles/sweep_open_summary.txt."""
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest
import torch

import sweep_open_reference as oref
import sweep_reference as ref
import sweep_vjp_reference as vref
import test_sweep as ts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-9
_herm, _unitary = ts._herm, ts._unitary
SX = np.array([[0, 1], [1, 0]], dtype=complex)
SY = np.array([[0, -1j], [1j, 0]], dtype=complex)
SZ = np.array([[1, 0], [0, -1]], dtype=complex)
SM = np.array([[0, 1], [0, 0]], dtype=complex)      # |0><1|: decay into level 0


def lindblad_case(qc, name, S, T, free=True, gamma1=0.15, gamma2=0.1, dt=(0.1, 0.3), m=2, samples=None):
    """One qubit with T1 (rate gamma1) and pure dephasing (rate gamma2): N = 4, 2N = 8, one detuning perturbation, density fidelity."""
    rng = np.random.default_rng(sum(map(ord, name)))
    H0 = 0.4 * SZ + 0.1 * SX
    Hd = [0.5 * SX, 0.5 * SY][:m]
    Ls = [np.sqrt(gamma1) * SM, np.sqrt(gamma2 / 2) * SZ]
    Pz = oref.lindblad_generator(0.5 * SZ)              # a detuning: the commutator superoperator, a generator matrix
    v = _unitary(rng, 2)
    psi0, g = v[:, 0], v[:, 1]
    init = oref.density_iso(np.outer(psi0, psi0.conj()))
    goal = np.concatenate([g.real, g.imag])
    c = dict(name=name, L=2, N=4, m=m, p=1, S=S, T=T, G0=oref.lindblad_generator(H0, Ls), Gd=[oref.lindblad_generator(H) for H in Hd], Gp=[Pz],
             init=init, cols=1, goal=goal, kind="density", subspace=None, form="abs", controls=rng.uniform(-1, 1, (m, T)),
             dts=rng.uniform(dt[0], dt[1], T) if free else 0.5 * (dt[0] + dt[1]), theta=rng.uniform(-0.3, 0.3, (S, 1)),
             scale=rng.uniform(0.9, 1.1, (S, m)), samples=list(range(S)) if samples is None else list(samples))
    c["system"] = qc.OpenQuantumSystem(H0, Hd, Ls) if qc is not None else None
    c["perts"] = [Pz]
    return c


def nonherm_case(qc, name, L, m, p, S, T, free, fid, use_scale=True, decay=0.3, samples=None, cols=None):
    """H_eff = H - i Gamma / 2 with Gamma >= 0 diagonal (loss out of every level at its own rate): iso generators that are not
    antisymmetric.  fid = (kind, subspace, form) or None; cols: several kets without a fidelity."""
    rng = np.random.default_rng(sum(map(ord, name)))
    H0 = _herm(rng, L) - 0.5j * np.diag(rng.uniform(0.0, decay, L))
    Hd = [_herm(rng, L, (L * max(m, 1)) ** -0.5) for _ in range(m)]
    perts = [_herm(rng, L) - 0.5j * np.diag(rng.uniform(0.0, 0.2, L)) for _ in range(p)]      # a detuning that also moves the loss rates
    kind, subspace, form = fid if fid is not None else (None, None, "abs")
    if kind == "unitary":
        init, ncol, goal = ref.operator_to_iso_vec(_unitary(rng, L)), L, ref.operator_to_iso_vec(_unitary(rng, L))
    else:
        ncol = cols or 1
        K = rng.standard_normal((L, ncol)) + 1j * rng.standard_normal((L, ncol))
        init = ref.operator_to_iso_vec(K / np.linalg.norm(K, axis=0))
        gk = rng.standard_normal(L) + 1j * rng.standard_normal(L)
        gk /= np.linalg.norm(gk)
        goal = np.concatenate([gk.real, gk.imag]) if kind else None
    c = dict(name=name, L=L, N=L, m=m, p=p, S=S, T=T, G0=ref.iso_generator(H0), Gd=[ref.iso_generator(H) for H in Hd],
             Gp=[ref.iso_generator(P) for P in perts], init=init, cols=ncol, goal=goal, kind=kind, subspace=subspace, form=form,
             controls=rng.uniform(-1, 1, (m, T)), dts=rng.uniform(0.1, 0.3, T) if free else 0.2, theta=rng.uniform(-0.3, 0.3, (S, p)),
             scale=rng.uniform(0.9, 1.1, (S, m)) if use_scale else None, samples=list(range(S)) if samples is None else list(samples))
    c["system"] = qc.QuantumSystem(H0, Hd) if qc is not None else None
    c["perts"] = perts
    return c


# the GPU cases of the issue, by letter
CASES = {
    "a-qubit-lindblad": lambda qc: lindblad_case(qc, "a-qubit-lindblad", S=5, T=9),                                   # chunks 3, 3, 2; 15 items
    "b-nonherm-m8": lambda qc: nonherm_case(qc, "b-nonherm-m8", 8, 8, 1, 3, 6, False, ("unitary", [0, 1, 2, 5], "abs")),
    "b-nonherm-m1": lambda qc: nonherm_case(qc, "b-nonherm-m1", 8, 1, 1, 2, 3, False, ("unitary", [0, 1, 2, 5], "abs2")),
    "b-nonherm-m2": lambda qc: nonherm_case(qc, "b-nonherm-m2", 8, 2, 1, 2, 3, False, ("unitary", None, "abs")),
    "b-nonherm-m4": lambda qc: nonherm_case(qc, "b-nonherm-m4", 8, 4, 2, 2, 3, False, ("unitary", [0, 1, 2, 5], "abs")),
    "b-nonherm-m6": lambda qc: nonherm_case(qc, "b-nonherm-m6", 8, 6, 1, 2, 3, False, ("unitary", None, "abs2"), use_scale=False),
    "c-qutrit-one-interval": lambda qc: nonherm_case(qc, "c-qutrit-one-interval", 3, 1, 1, 1, 2, True, ("ket", None, "abs")),
    "d-one-chunk": lambda qc: lindblad_case(qc, "d-one-chunk", S=2049, T=3, samples=(0, 1, 1024, 2047, 2048)),
    "e-sq0": lambda qc: lindblad_case(qc, "e-sq0", S=3, T=5, dt=(0.01, 0.02)),
    "e-sq3": lambda qc: lindblad_case(qc, "e-sq3", S=3, T=5, dt=(0.9, 1.4)),
    "f-strong-dissipation": lambda qc: lindblad_case(qc, "f-strong-dissipation", S=3, T=9, gamma1=10.0, gamma2=2.0, dt=(0.4, 0.6)),
}


def squarings(c):
    """The rule of the kernels: the smallest sq with ||dt G||_1 / 2^sq <= 1/8, over every sample and interval."""
    out = []
    h = np.full(c["T"], c["dts"]) if np.ndim(c["dts"]) == 0 else c["dts"]
    sc = np.ones((c["S"], c["m"])) if c["scale"] is None else c["scale"]
    for s in c["samples"]:
        for t in range(c["T"] - 1):
            nrm = np.abs(h[t] * ref.sample_generator(c["G0"], c["Gd"], c["Gp"], c["controls"][:, t], c["theta"][s], sc[s])).sum(axis=0).max()
            out.append(0 if nrm <= 0.125 else int(np.ceil(np.log2(nrm / 0.125))))
    return min(out), max(out)


# ---------------------------------------------------------------------------------------------------------------------------------
#  CPU
# ---------------------------------------------------------------------------------------------------------------------------------
class _ODesc(ts._Desc):
    """ts._Desc with a goal long enough for every kind and the flag of reserved1[0]."""

    def __init__(self, qc, flag=0, wide=0, **kw):
        super().__init__(qc, **kw)
        self.goal = np.zeros(2 * self.d.N * self.d.N + 2)
        self.d.goal_iso = qc._lib.dptr(self.goal)
        self.d.reserved1[0] = flag
        self.d.wide = wide


def _query(qc, fn, D):
    ok = C.c_int32(-1)
    rc = getattr(qc._lib.lib, fn)(C.byref(D.d), C.byref(ok))
    return rc, ok.value, qc._lib.lib.qc_sweep_last_error(None).decode()


def test_flag_values_through_validate(qc):
    L = qc._lib
    assert L.QC_SWEEP_STORED_STATES == 1
    val = lambda D: L.lib.qc_sweep_desc_validate(C.byref(D.d))
    assert val(_ODesc(qc, flag=0)) == L.QC_OK
    assert val(_ODesc(qc, flag=1)) == L.QC_OK
    for bad in (2, -1, 1 << 40):
        assert val(_ODesc(qc, flag=bad)) == L.QC_ERR_INVALID
        assert "reserved1[0]" in L.lib.qc_sweep_last_error(None).decode()
    D = _ODesc(qc, flag=1)
    D.d.reserved1[1] = 12345        # ignored
    assert val(D) == L.QC_OK
    header = open(os.path.join(ROOT, "include", "qcolloc.h")).read()
    assert "#define QC_SWEEP_STORED_STATES 1" in header and "int64_t reserved1[2];" in header
    assert L.lib.qc_abi_version() == 6 and C.sizeof(L.qc_sweep_desc) == L.lib.qc_sizeof_sweep_desc()


def test_scope_queries_follow_the_flag(qc):
    L = qc._lib
    rng = np.random.default_rng(0)

    def lind(flag, **kw):
        D = _ODesc(qc, flag=flag, **{**dict(N=4, m=2, cols=1, fid_kind=L.QC_FID_DENSITY), **kw})
        D.G0[:] = rng.standard_normal(D.G0.size)       # not antisymmetric
        return D

    for fn, pre in (("qc_sweep_desc_grad_supported", "qc_sweep gradients: "), ("qc_sweep_desc_vjp_supported", "qc_sweep pullback: ")):
        rc, ok, msg = _query(qc, fn, lind(0))
        assert (rc, ok) == (L.QC_OK, 0) and msg.startswith(pre), msg
        assert "G_drift is not antisymmetric (open-system generators are not served: their gradients need stored forward states)" in msg
        assert _query(qc, fn, lind(1))[:2] == (L.QC_OK, 1)
        # a wide descriptor in the mfma32-sweep form: the new reason; wide at 2N <= 16 stays mfma16-sweep and is served
        rc, ok, msg = _query(qc, fn, lind(1, N=12, cols=0, fid_kind=L.QC_FID_UNITARY, wide=L.QC_SWEEP_WIDE))
        assert (rc, ok) == (L.QC_OK, 0) and msg == pre + "stored-state gradients are not served in the mfma32-sweep form"
        assert _query(qc, fn, lind(1, wide=L.QC_SWEEP_WIDE))[:2] == (L.QC_OK, 1)
        # the per-sample form keeps its own reasons; more than 16 state columns likewise
        rc, ok, msg = _query(qc, fn, lind(1, N=12, cols=0, fid_kind=L.QC_FID_UNITARY))
        assert (rc, ok) == (L.QC_OK, 0) and "rollout-per-sample form (2N = 24 > 16)" in msg
        rc, ok, msg = _query(qc, fn, lind(1, N=2, m=9, cols=0, fid_kind=L.QC_FID_UNITARY))
        assert (rc, ok) == (L.QC_OK, 0) and "9 drives > 8" in msg
        rc, ok, msg = _query(qc, fn, _ODesc(qc, flag=1, N=2, m=2, cols=17))
        assert (rc, ok) == (L.QC_OK, 0) and "16 columns" in msg
    # the gradient needs a fidelity, the pullback does not; flag off, an antisymmetric density handle is refused as before
    rc, ok, msg = _query(qc, "qc_sweep_desc_grad_supported", _ODesc(qc, flag=1, N=2, m=2))
    assert (rc, ok) == (L.QC_OK, 0) and "no fidelity" in msg
    assert _query(qc, "qc_sweep_desc_vjp_supported", _ODesc(qc, flag=1, N=2, m=2))[:2] == (L.QC_OK, 1)
    rc, ok, msg = _query(qc, "qc_sweep_desc_grad_supported", _ODesc(qc, flag=0, N=4, m=2, cols=1, fid_kind=L.QC_FID_DENSITY))
    assert (rc, ok) == (L.QC_OK, 0) and "density-operator fidelity is not served" in msg
    assert _query(qc, "qc_sweep_desc_grad_supported", _ODesc(qc, flag=1, N=4, m=2, cols=1, fid_kind=L.QC_FID_DENSITY))[:2] == (L.QC_OK, 1)
    # Hessian products and the noise sweep do not look at the flag
    for flag in (0, 1):
        rc, ok, msg = _query(qc, "qc_sweep_desc_hvp_supported", lind(flag))
        assert (rc, ok) == (L.QC_OK, 0) and "is not antisymmetric" in msg
        assert _query(qc, "qc_sweep_desc_jvp_supported", lind(flag))[:2] == (L.QC_OK, 1)


def test_python_keyword_defaults_to_false(qc):
    for f in (qc.RolloutSweep.__init__, qc.rollout_sweep, qc.rollout_sweep_parameter_gradient, qc.SweepInfidelityObjective.__init__,
              qc.SweepFinalStateObjective.__init__):
        par = inspect.signature(f).parameters
        assert "stored_states" in par and par["stored_states"].default is False, f
    julia = open(os.path.join(ROOT, "julia", "QCollocHIP.jl")).read()
    assert julia.count("stored_states::Bool=false") == 4 and "device::Int32; wide::Int32; reserved1::NTuple{2,Int64}" in julia


def test_restated_generators_match_the_package(qc):
    c = lindblad_case(qc, "a-qubit-lindblad", S=2, T=3)
    assert np.array_equal(c["G0"], c["system"].G_drift) and all(np.array_equal(a, b) for a, b in zip(c["Gd"], c["system"].G_drives))
    assert np.abs(c["G0"] + c["G0"].T).max() > 0.05          # a Lindblad generator is not antisymmetric
    c = nonherm_case(qc, "b-nonherm-m2", 8, 2, 1, 2, 3, False, ("unitary", None, "abs"))
    assert np.array_equal(c["G0"], c["system"].G_drift) and np.abs(c["G0"] + c["G0"].T).max() > 0.05
    # the density fidelity is <c, x>
    rng = np.random.default_rng(3)
    A = rng.standard_normal((2, 2)) + 1j * rng.standard_normal((2, 2))
    g = rng.standard_normal(4)
    x = oref.density_iso(A @ A.conj().T)
    assert abs(ref.density_fidelity(x, g) - oref.density_cotangent(g) @ x) < 1e-13 * abs(ref.density_fidelity(x, g))


@pytest.mark.parametrize("name", ["a-qubit-lindblad", "b-nonherm-m2", "c-qutrit-one-interval", "e-sq3", "f-strong-dissipation"])
def test_reference_routes_agree(name):
    """Forward mode (expm_frechet) against central differences on the systems, rates and steps the GPU cases use: 1e-6 relative."""
    c = CASES[name](None)
    err, big = oref.forward_vs_fd(c, c["samples"][:2])
    print(f"{name}: forward vs central differences {err:.2e}, max |grad| {big:.3e}")
    assert err < 1e-6 and big > 1e-6


# ---------------------------------------------------------------------------------------------------------------------------------
#  GPU
# ---------------------------------------------------------------------------------------------------------------------------------
def _handle(qc, c, stored=True, fid=True, **kw):
    free = np.ndim(c["dts"]) != 0
    return qc.RolloutSweep(c["system"], c["perts"], c["T"], cols=c["cols"], goal=c["goal"] if fid else None, fid_kind=c["kind"] if fid else None,
                           subspace=c["subspace"], fid_form=qc._lib.QC_FID_FORM_ABS2 if c["form"] == "abs2" else qc._lib.QC_FID_FORM_ABS,
                           dt_fixed=None if free else float(c["dts"]), stored_states=stored, **kw)


def _Z(sw, c):
    return sw.pack(c["controls"], c["dts"] if np.ndim(c["dts"]) else None)


def _worst(got, want, what):
    """Per sample: |got - want| <= 1e-9 max(1, max |want of the sample|); returns the worst error as a share of its bound."""
    worst = 0.0
    for q in range(want.shape[0]):
        bound = RTOL * max(1.0, np.abs(want[q]).max(initial=0.0))
        worst = max(worst, np.abs(got[q] - want[q]).max(initial=0.0) / bound)
    print(f"    {what}: worst error {worst:.3e} of its bound")
    assert worst <= 1.0, what
    return worst


def _check_grad_outputs(qc, c):
    """grad_samples, grad (weighted), J, fids, grad_theta, grad_scale of a stored-state handle against the reference."""
    sw = _handle(qc, c)
    assert sw.stored_states and sw.grad_supported and sw.kernel_name == "mfma16-sweep"
    Z = _Z(sw, c)
    S, sel = c["S"], c["samples"]
    w = np.random.default_rng(5).uniform(0.5, 1.5, S)
    w /= w.sum()
    want = oref.grad_forward(c)
    J, f, g, gs = sw.grad(Z, c["init"], c["theta"], c["scale"], w, per_sample=True)
    f_eval = sw.eval(Z, c["init"], c["theta"], c["scale"], finals=False)[1]
    assert np.array_equal(f, f_eval), "fids must carry the bits of qc_sweep_eval"
    f_ref = oref.fidelities(c) if S <= 16 else None
    if f_ref is not None:
        assert np.abs(f - f_ref).max() < 1e-9
    print(f"{c['name']}: squarings {squarings(c)}, max |grad| {np.abs(want['grad_samples']).max():.3e}")
    worst = _worst(gs[sel], want["grad_samples"], "grad_samples")
    assert abs(J - w @ f) < 1e-12
    if len(sel) == S:
        dense = np.zeros(sw.Z_len)
        K = dense[:sw.T * sw.zdim].reshape(sw.T, sw.zdim)
        acc = np.einsum("s,stk->tk", w, want["grad_samples"])
        K[:sw.T - 1, sw.off_a:sw.off_a + sw.m] = acc[:, :sw.m]
        if sw.off_dt >= 0:
            K[:sw.T - 1, sw.off_dt] = acc[:, sw.m]
        worst = max(worst, _worst(g[None], dense[None], "grad"))
    f2, gth, gsc = sw.param_grad(Z, c["init"], c["theta"], c["scale"])
    assert np.array_equal(f2, f)
    worst = max(worst, _worst(gth[sel], want["grad_theta"], "grad_theta"), _worst(gsc[sel], want["grad_scale"], "grad_scale"))
    sw.close()
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_stored_state_gradients_against_reference(qc, name):
    c = CASES[name](qc)
    lo, hi = squarings(c)
    if name == "e-sq0":
        assert hi == 0
    if name == "e-sq3":
        assert lo >= 3
    if name == "f-strong-dissipation":
        h = c["dts"][:c["T"] - 1].sum()
        assert 35.0 < 10.0 * h < 50.0      # gamma sum h ~ 40: reversing the step would amplify rounding by about e^40
    worst = _check_grad_outputs(qc, c)
    print(f"SUMMARY {name}: worst error {worst:.3e} of its bound")


@pytest.mark.gpu
def test_closed_system_cross_check(qc):
    """(g) One antisymmetric system, flag on against flag off: every output of grad, grad_params and vjp within the 1e-9 rule, fids bit-equal."""
    import test_sweep_grad as tg
    c = tg.build(qc, "levels4-3drives")
    mk = lambda stored: qc.RolloutSweep(c["system"], c["perts"], c["T"], cols=c["cols"], goal=c["goal"], fid_kind=c["kind"], stored_states=stored)
    outs = []
    cot = np.random.default_rng(7).standard_normal((c["S"], 2 * c["L"] * c["cols"]))
    for stored in (False, True):
        sw = mk(stored)
        assert sw.grad_supported and sw.hvp_supported
        Z = sw.pack(c["controls"], c["dts"])
        J, f, g, gs = sw.grad(Z, c["init"], c["theta"], c["scale"], per_sample=True)
        f2, gth, gsc = sw.param_grad(Z, c["init"], c["theta"], c["scale"])
        vg, vgs, vgi, vgth, vgsc = sw.vjp(Z, c["init"], cot, c["theta"], c["scale"], per_sample=True, init_grad=True, params=True)
        outs.append(dict(fids=f, J=np.array([J]), grad=g[None], grad_samples=gs, grad_theta=gth, grad_scale=gsc, vjp_grad=vg[None], vjp_samples=vgs,
                         vjp_init=vgi, vjp_theta=vgth, vjp_scale=vgsc))
        sw.close()
    off, on = outs
    assert np.array_equal(off["fids"], on["fids"]) and off["J"][0] == on["J"][0]
    worst = max(_worst(on[k], off[k], k) for k in off if k not in ("fids", "J"))
    print(f"SUMMARY g-closed-cross-check: worst difference flag on / off {worst:.3e} of the bound")


def _pullback_case(qc, which):
    if which == "lindblad":
        return lindblad_case(qc, "h-lindblad", S=4, T=7), True
    if which == "no-fidelity":
        c = nonherm_case(qc, "h-nofid", 4, 3, 2, 3, 6, True, ("unitary", None, "abs"))
        c["scale"][1, 0] = 0.0           # one c[s, k] = 0: the derivative with respect to it is still defined
        return c, False
    return nonherm_case(qc, "h-kets3", 5, 2, 1, 3, 5, False, None, use_scale=False, cols=3), False      # scale = NULL


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["lindblad", "no-fidelity", "kets3"])
def test_pullback_against_reference(qc, which):
    c, fid = _pullback_case(qc, which)
    sw = _handle(qc, c, fid=fid)
    assert sw.vjp_supported and (fid or not sw.grad_supported)
    Z = _Z(sw, c)
    cot = np.random.default_rng(11).standard_normal((c["S"], sw.ns))
    want = vref.pullback_forward(c["G0"], c["Gd"], c["Gp"], c["controls"], c["dts"], c["init"], c["theta"], c["scale"], c["samples"], cot)
    g, gs, gi, gth, gsc = sw.vjp(Z, c["init"], cot, c["theta"], c["scale"], per_sample=True, init_grad=True, params=True)
    worst = max(_worst(gs, want["grad_samples"], "grad_samples"), _worst(gi, want["grad_init"], "grad_init"),
                _worst(gth, want["grad_theta"], "grad_theta"), _worst(gsc, want["grad_scale"], "grad_scale"))
    acc = np.zeros_like(gs[0])          # grad: the plain sum in ascending s, +0.0 everywhere else
    for q in range(c["S"]):
        acc = acc + gs[q]
    K = g[:sw.T * sw.zdim].reshape(sw.T, sw.zdim).copy()
    assert np.array_equal(K[:sw.T - 1, :sw.n_deriv], acc)
    K[:sw.T - 1, :sw.n_deriv] = 0.0
    assert not K.any() and not np.signbit(K).any()
    # the final states of the pullback carry the bits of qc_sweep_eval
    fin = np.empty((c["S"], sw.ns))
    gz = np.empty(sw.Z_len)
    L = qc._lib
    opt = lambda a: L.dptr(np.ascontiguousarray(a)) if a is not None else None
    th, sc = np.ascontiguousarray(c["theta"]), (None if c["scale"] is None else np.ascontiguousarray(c["scale"]))
    rc = L.lib.qc_sweep_vjp(sw._h, L.dptr(Z), L.dptr(np.ascontiguousarray(c["init"])), c["S"], L.dptr(th), None if sc is None else L.dptr(sc),
                            L.dptr(cot), L.dptr(fin), L.dptr(gz), None, None, None, None)
    assert rc == L.QC_OK and np.array_equal(gz, g)
    assert np.array_equal(fin.T, sw.eval(Z, c["init"], c["theta"], c["scale"], fids=False)[0])
    sw.close()
    print(f"SUMMARY h-pullback-{which}: worst error {worst:.3e} of its bound")


def _raw_grad_params(qc, sw, Z, init, theta, scale, w, want):
    """qc_sweep_grad_params with exactly the outputs named in `want`."""
    L = qc._lib
    S = theta.shape[0]
    bufs = dict(fids=np.empty(S), J=np.empty(1), grad=np.empty(sw.Z_len), grad_samples=np.empty((S, sw.T - 1, sw.n_deriv)),
                grad_theta=np.empty((S, sw.p)), grad_scale=np.empty((S, sw.m)))
    ptr = lambda k: L.dptr(bufs[k]) if k in want else None
    rc = L.lib.qc_sweep_grad_params(sw._h, L.dptr(Z), L.dptr(init), S, L.dptr(theta), L.dptr(scale), L.dptr(w), ptr("fids"),
                                    bufs["J"].ctypes.data_as(C.POINTER(C.c_double)) if "J" in want else None, ptr("grad"), ptr("grad_samples"),
                                    ptr("grad_theta"), ptr("grad_scale"))
    assert rc == L.QC_OK, L.lib.qc_sweep_last_error(sw._h).decode()
    return {k: bufs[k] for k in want}


@pytest.mark.gpu
def test_bit_level_properties(qc):
    c = lindblad_case(qc, "i-bits", S=6, T=8)
    sw = _handle(qc, c)
    Z = _Z(sw, c)
    init, theta, scale = (np.ascontiguousarray(c[k]) for k in ("init", "theta", "scale"))
    w = np.full(c["S"], 1.0 / c["S"])
    names = ("fids", "J", "grad", "grad_samples", "grad_theta", "grad_scale")
    a = _raw_grad_params(qc, sw, Z, init, theta, scale, w, names)
    b = _raw_grad_params(qc, sw, Z, init, theta, scale, w, names)
    for k in names:
        assert np.array_equal(a[k], b[k]), f"repeated calls: {k}"
        alone = _raw_grad_params(qc, sw, Z, init, theta, scale, w, (k,))[k]
        assert np.array_equal(alone, a[k]), f"{k} alone against {k} with every other output"
    # grad: +0.0 outside the controls and timesteps of knots 0 .. T-2
    K = a["grad"][:sw.T * sw.zdim].reshape(sw.T, sw.zdim).copy()
    assert np.abs(K[:sw.T - 1, :sw.n_deriv]).min() > 0.0
    K[:sw.T - 1, :sw.n_deriv] = 0.0
    rest = np.concatenate([K.ravel(), a["grad"][sw.T * sw.zdim:]])
    assert not rest.any() and not np.signbit(rest).any()
    # the gradient entry point gives the same bits as the parameter flavour
    J, f, g, gs = sw.grad(Z, init, theta, scale, w, per_sample=True)
    assert np.array_equal(gs, a["grad_samples"]) and np.array_equal(g, a["grad"]) and np.array_equal(f, a["fids"])
    # a NaN in one sample's theta reaches that sample's outputs and grad, nothing else
    bad = theta.copy()
    bad[2, 0] = np.nan
    n = _raw_grad_params(qc, sw, Z, init, bad, scale, w, names)
    keep = [s for s in range(c["S"]) if s != 2]
    for k in ("fids", "grad_samples", "grad_theta", "grad_scale"):
        assert np.isnan(n[k][2]).all(), k
        assert np.array_equal(n[k][keep], a[k][keep]), k
    assert np.isnan(n["J"]).all() and np.isnan(n["grad"][:(sw.T - 1) * sw.zdim].reshape(sw.T - 1, sw.zdim)[:, :sw.n_deriv]).all()
    sw.close()


@pytest.mark.gpu
def test_refusals_with_the_flag_on(qc):
    L = qc._lib
    c = lindblad_case(qc, "j-refusals", S=3, T=5)
    sw = _handle(qc, c)
    Z = _Z(sw, c)
    assert sw.grad_supported and sw.vjp_supported and sw.jvp_supported and not sw.hvp_supported
    assert "is not antisymmetric" in sw.hvp_unsupported_reason
    cot = np.ones((c["S"], sw.ns))
    with pytest.raises(qc.QCollocError) as e:
        sw.hvp(Z, c["init"], cot, c["theta"], c["scale"], vZ=np.ones(sw.Z_len))
    assert e.value.code == L.QC_ERR_UNSUPPORTED and "is not antisymmetric" in str(e.value)
    with pytest.raises(qc.QCollocError) as e:
        sw.noise_grad(Z, c["init"], np.zeros((c["S"], c["T"] - 1, 1)), c["theta"], c["scale"])
    assert e.value.code == L.QC_ERR_UNSUPPORTED and "is not antisymmetric" in str(e.value)
    # the forward entries do not look at the flag: the bits of a handle without it
    sw0 = _handle(qc, c, stored=False)
    assert not sw0.grad_supported and "stored forward states" in sw0.grad_unsupported_reason
    for a, b in zip(sw.eval(Z, c["init"], c["theta"], c["scale"]), sw0.eval(Z, c["init"], c["theta"], c["scale"])):
        assert np.array_equal(a, b)
    with pytest.raises(qc.QCollocError) as e:
        sw0.grad(Z, c["init"], c["theta"], c["scale"])
    assert e.value.code == L.QC_ERR_UNSUPPORTED and "is not antisymmetric" in str(e.value)
    sw.close()
    sw0.close()
    # a wide handle in the mfma32-sweep form
    rng = np.random.default_rng(2)
    sysw = qc.QuantumSystem(_herm(rng, 12), [_herm(rng, 12)])
    sww = qc.RolloutSweep(sysw, [], 4, goal=ref.operator_to_iso_vec(np.eye(12)), fid_kind="unitary", wide=True, stored_states=True)
    assert sww.kernel_name == "mfma32-sweep" and not sww.grad_supported and not sww.vjp_supported
    with pytest.raises(qc.QCollocError) as e:
        sww.grad(sww.pack(np.zeros((1, 4)), 0.1), ref.operator_to_iso_vec(np.eye(12)), np.zeros((2, 0)))
    assert e.value.code == L.QC_ERR_UNSUPPORTED and "stored-state gradients are not served in the mfma32-sweep form" in str(e.value)
    sww.close()


def _open_traj(qc, c):
    T = c["T"]
    comps = {"ρ̃⃗": np.repeat(c["init"][:, None], T, axis=1), "a": c["controls"], "Δt": np.asarray(c["dts"]).reshape(1, T)}
    return qc.NamedTrajectory(comps, controls=("a",), timestep="Δt", initial={"ρ̃⃗": c["init"].copy()}, goal={})


@pytest.mark.gpu
def test_objective_and_autograd_on_a_lindblad_system(qc):
    c = lindblad_case(qc, "k-objective", S=4, T=6)
    traj = _open_traj(qc, c)
    with pytest.raises(qc.QCollocError) as e:
        qc.SweepInfidelityObjective(traj, c["system"], c["perts"], c["theta"], scale=c["scale"], state_name="ρ̃⃗", goal_ket=c["goal"])
    assert e.value.code == qc._lib.QC_ERR_UNSUPPORTED and "is not antisymmetric" in str(e.value)
    obj = qc.SweepInfidelityObjective(traj, c["system"], c["perts"], c["theta"], scale=c["scale"], state_name="ρ̃⃗", goal_ket=c["goal"],
                                      stored_states=True)
    assert obj.stored_states
    Z = np.array(traj.datavec, dtype=np.float64)
    g = obj.grad_L(Z)
    idx = np.flatnonzero(g)
    assert idx.size == (c["T"] - 1) * 3
    fd = np.zeros_like(g)
    for i in idx:
        zp, zm = Z.copy(), Z.copy()
        zp[i] += 1e-5
        zm[i] -= 1e-5
        fd[i] = (obj.L(zp) - obj.L(zm)) / 2e-5
    print(f"grad_L against central differences: {np.abs(g - fd).max():.2e}")
    assert np.abs(g - fd).max() < 1e-7
    # finals_autograd on the same handle: backward through vjp, forward through jvp
    sw = obj._sweep
    dev = torch.device("cuda", 0)
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cvec = put(oref.density_cotangent(c["goal"]))
    dZ = put(Z).requires_grad_(True)
    X = sw.finals_autograd(dZ, put(c["init"]), put(c["theta"]), put(c["scale"]))
    loss = 1.0 - (X @ cvec).mean()
    assert abs(loss.item() - obj.L(Z)) < 1e-13
    loss.backward()
    ga = dZ.grad.cpu().numpy()
    assert np.abs(ga - fd).max() < 1e-7 and np.abs(ga - g).max() <= 1e-9 * max(1.0, np.abs(g).max())
    import torch.autograd.forward_ad as fwAD
    v = np.random.default_rng(4).standard_normal(Z.size)
    with fwAD.dual_level():
        Xd = sw.finals_autograd(fwAD.make_dual(put(Z), put(v)), put(c["init"]), put(c["theta"]), put(c["scale"]))
        tan = fwAD.unpack_dual(1.0 - (Xd @ cvec).mean()).tangent
    assert abs(tan.item() - g @ v) <= 1e-9 * max(1.0, np.abs(g).max() * np.abs(v).sum())
    obj.close()


@pytest.mark.gpu
def test_open_system_polish_example(qc):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import open_system_polish
    before, after, closed = open_system_polish.polish(T=12, S=5, steps=25, verbose=False)
    print(f"mean infidelity over the detunings {before:.4e} -> {after:.4e}; the pulse polished on the closed model {closed:.4e}")
    assert after < before
