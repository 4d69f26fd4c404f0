"""Sweep pullbacks (`qc_sweep_vjp*`, `RolloutSweep.vjp` / `vjp_device` / `finals_autograd`, `SweepFinalStateObjective`): the derivatives of
phi_s = <cot[s], x_final[s]> for cotangents the caller chooses, on "mfma16-sweep" handles (wide handles: test_sweep_vjp_wide.py).  CPU: the
two routes of tests/sweep_vjp_reference.py against each other, the device-free scope query, prototypes.  GPU: every requested output
against the forward-mode reference, `finals` against `eval` (bits), `grad` against the plain sum, bit-level properties, consistency
with the fidelity gradient, isolation of a non-finite cotangent, refusals, autograd, the objective, the example.

Tolerance (GPU against the reference).  The cotangents have Frobenius norm 1, so lambda has norm 1 along the whole walk (the
propagators are orthogonal), as the fidelity seeds have; test_sweep_grad.py's argument carries over: per sample
|got - want| <= 1e-9 max(1, max |want_s|) for grad_samples, grad_theta and grad_scale.  grad_init = W^T C_s is an orthogonal image of a
unit vector: the state tolerance of test_sweep.py (rtol 1e-10, atol 1e-11).  Measured worst errors: profiles/sweep_vjp_summary.txt.
Every sample of mid-size and filled launches (S = 97 .. 2049) against the reference: tests/test_sweep_every_sample.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import sweep_grad_reference as gref
import sweep_reference as ref
import sweep_vjp_reference as vref
import test_sweep as ts
import test_sweep_grad as tg
import test_sweep_wide as tw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VJP_RTOL = 1e-9
_herm, _unitary = ts._herm, ts._unitary

# name: (state, levels, m, p, scale given, free timestep, S, T, fidelity, samples checked against the reference)
VJP_CASES = {
    "qubit": ("unitary", 2, 2, 1, False, True, 5, 11, ("unitary", None, "abs"), None),                # chunks of 3, 3, 3, 1
    "qutrit": ("unitary", 3, 1, 3, True, False, 7, 10, ("unitary", [0, 1], "abs2"), None),            # padded tile, parameter flavour
    "qubits3-6drives": ("unitary", 8, 6, 1, True, True, 3, 12, ("unitary", None, "abs"), None),        # full tile, M = 6
    "kets3": ("kets3", 4, 2, 1, True, True, 3, 8, None, None),                                        # a handle `grad` refuses
    "no-drives": ("unitary", 2, 0, 1, False, False, 3, 6, ("unitary", None, "abs"), None),            # no control walk
    "one-interval": ("unitary", 2, 2, 1, False, True, 3, 2, ("unitary", None, "abs"), None),          # n_chunks = 1, T = 2
    "one-chunk": ("unitary", 2, 2, 1, True, True, 2048, 4, ("unitary", None, "abs"), (0, 1000, 2047)),
}
_REF = {}          # (form, case name) -> reference dict: computed once, shared, never written to


def unit_cotangents(rng, S, ns):
    cot = rng.standard_normal((S, ns))
    return cot / np.linalg.norm(cot, axis=1, keepdims=True)


def build(qc, name, cases=VJP_CASES):
    c = tw.build(qc, name, cases[name])
    c["cot"] = unit_cotangents(np.random.default_rng(7 + sum(map(ord, name))), c["S"], c["init"].size)
    return c


def reference(c, form="16"):
    key = (form, c["name"])
    if key not in _REF:
        out = vref.pullback_forward(c["G0"], c["Gd"], c["Gp"], c["controls"], c["dts"], c["init"], c["theta"], c["scale"], c["samples"], c["cot"])
        for a in out.values():
            a.setflags(write=False)
        _REF[key] = out
    return _REF[key]


# ---------------------------------------------------------------------------------------------------------------------------------
#  CPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("free", [True, False], ids=["free-dt", "fixed-dt"])
@pytest.mark.parametrize("state", ["unitary", "ket", "kets3"])
@pytest.mark.parametrize("N", [2, 3, 8])
def test_reference_routes_agree(N, state, free):
    """Forward mode (expm_frechet) against central differences of the sweep reference: finite-difference accuracy, 1e-6 relative."""
    rng = np.random.default_rng(10 * N + len(state) + free)
    m, p, T, S = 2, 1, 5, 2
    G0, Gd, Gp = ref.iso_generator(_herm(rng, N)), [ref.iso_generator(_herm(rng, N, 0.4)) for _ in range(m)], [ref.iso_generator(_herm(rng, N))]
    controls = rng.uniform(-1, 1, (m, T))
    dts = rng.uniform(0.1, 0.3, T) if free else 0.2
    theta, scale = rng.uniform(-0.3, 0.3, (S, p)), rng.uniform(0.9, 1.1, (S, m))
    cols = {"unitary": N, "ket": 1, "kets3": 3}[state]
    K = rng.standard_normal((N, cols)) + 1j * rng.standard_normal((N, cols))
    init = ref.operator_to_iso_vec(_unitary(rng, N) if state == "unitary" else K / np.linalg.norm(K, axis=0))
    cot = unit_cotangents(rng, S, init.size)
    args = (G0, Gd, Gp, controls, dts, init, theta, scale, [0, 1], cot)
    a, b = vref.pullback_forward(*args), vref.pullback_fd(*args)
    assert a["grad_samples"].shape == (2, T - 1, m + free) and a["grad_init"].shape == (2, init.size)
    assert a["grad_theta"].shape == (2, p) and a["grad_scale"].shape == (2, m)
    for key in ("grad_samples", "grad_init", "grad_theta", "grad_scale"):
        assert a[key].shape == b[key].shape
        err = np.abs(a[key] - b[key]).max() / max(1.0, np.abs(a[key]).max())
        print(f"N={N} {state} free={free} {key}: forward vs central differences {err:.2e}, max |value| {np.abs(a[key]).max():.3f}")
        assert err < 1e-6 and np.abs(a[key]).max() > 1e-3, key


def _supported(qc, D, fn="qc_sweep_desc_vjp_supported"):
    ok = C.c_int32(-1)
    rc = getattr(qc._lib.lib, fn)(C.byref(D.d), C.byref(ok))
    return rc, ok.value, qc._lib.lib.qc_sweep_last_error(None).decode()


def _wide(D):
    D.d.wide = 1
    return D


def test_vjp_scope_without_a_device(qc):
    L = qc._lib
    U = L.QC_FID_UNITARY
    served = {
        "qubit": tg._GDesc(qc, N=2, m=2, fid_kind=U),
        "qutrit with subspace": tg._GDesc(qc, N=3, m=1, p=3, fid_kind=U, fid_form=L.QC_FID_FORM_ABS2, subspace=[0, 1]),
        "3 qubits, 8 drives": tg._GDesc(qc, N=8, m=8, fid_kind=U),
        "ket": tg._GDesc(qc, N=4, m=2, cols=1, fid_kind=L.QC_FID_KET),
        "three kets, no fidelity": tg._GDesc(qc, N=4, m=2, cols=3),
        "wide, N = 12": _wide(tg._GDesc(qc, N=12, m=2, fid_kind=U)),
        "density fidelity, closed": tg._GDesc(qc, N=4, m=2, cols=1, fid_kind=L.QC_FID_DENSITY),
    }
    for what, D in served.items():
        assert _supported(qc, D)[:2] == (L.QC_OK, 1), what
    rng = np.random.default_rng(0)
    D = tg._GDesc(qc, N=3, m=1, fid_kind=U)
    D.G0[:] = ref.iso_generator(_herm(rng, 3)).reshape(-1, order="F")
    assert _supported(qc, D)[:2] == (L.QC_OK, 1)
    D.G0[1] += 1e-12
    refused = {
        "drift": (D, "antisymmetric"),
        "9 drives": (tg._GDesc(qc, N=2, m=9), "9 drives"),
        "2N = 18": (tg._GDesc(qc, N=9, m=2, fid_kind=U), "2N = 18"),
        "17 columns": (tg._GDesc(qc, N=2, m=2, cols=17), "16 columns"),
    }
    for what, (D, word) in refused.items():
        rc, ok, msg = _supported(qc, D)
        assert (rc, ok) == (L.QC_OK, 0), what
        assert msg.startswith("qc_sweep pullback: ") and word in msg, (what, msg)
    assert "G_drift" in _supported(qc, refused["drift"][0])[2]
    # an invalid descriptor is its own error; NULL `supported`
    assert _supported(qc, tg._GDesc(qc, T=1))[0] == L.QC_ERR_INVALID
    assert L.lib.qc_sweep_desc_vjp_supported(C.byref(served["qubit"].d), None) == L.QC_ERR_INVALID
    assert "qc_sweep_desc_vjp_supported" in L.lib.qc_sweep_last_error(None).decode()
    # the gradient's own query is unchanged
    rc, ok, msg = _supported(qc, served["three kets, no fidelity"], "qc_sweep_desc_grad_supported")
    assert (rc, ok) == (L.QC_OK, 0) and msg == "qc_sweep gradients: the handle has no fidelity (QC_SWEEP_FID_NONE)"
    assert _supported(qc, served["qubit"], "qc_sweep_desc_grad_supported")[:2] == (L.QC_OK, 1)


def test_vjp_prototypes_and_header(qc):
    L = qc._lib
    for name, nargs in (("qc_sweep_desc_vjp_supported", 2), ("qc_sweep_vjp", 13), ("qc_sweep_vjp_dev", 14)):
        assert name in L.SYMBOLS and len(L.SYMBOLS[name][1]) == nargs
        assert getattr(L.lib, name).argtypes is not None
    header = open(os.path.join(ROOT, "include", "qcolloc.h")).read()
    for decl in ("int qc_sweep_desc_vjp_supported(const qc_sweep_desc* d, int32_t* supported);", "int qc_sweep_vjp_dev(qc_sweep* h,",
                 "int qc_sweep_vjp(qc_sweep* h,"):
        assert decl in header
    assert "second derivatives, derivatives of the\n * final states" not in header
    x = np.zeros(8)
    p = L.dptr(x)
    assert L.lib.qc_sweep_vjp(None, p, p, 1, p, None, p, None, p, None, None, None, None) == L.QC_ERR_INVALID
    assert L.lib.qc_sweep_last_error(None).decode() == "qc_sweep_vjp: NULL handle"
    assert L.lib.qc_sweep_vjp_dev(None, None, None, 1, None, None, None, None, None, None, None, None, None, None) == L.QC_ERR_INVALID
    assert L.lib.qc_sweep_last_error(None).decode() == "qc_sweep_vjp_dev: NULL handle"
    assert L.lib.qc_abi_version() == 6      # additive: the ABI stays 0.6
    for attr in ("vjp", "vjp_device", "vjp_supported", "vjp_unsupported_reason", "finals_autograd"):
        assert hasattr(qc.RolloutSweep, attr)
    assert hasattr(qc, "SweepFinalStateObjective")


# ---------------------------------------------------------------------------------------------------------------------------------
#  GPU
# ---------------------------------------------------------------------------------------------------------------------------------
OUTPUTS = ("finals", "grad", "grad_samples", "grad_init", "grad_theta", "grad_scale")
WORST = {}         # what -> worst error / bound seen in this session (printed by the tests; profiles/sweep_vjp_summary.txt)


def device_call(sw, Z, c, want, cot=None, stream=None):
    """One `vjp_device` call for the outputs named in `want`; returns them as numpy arrays (buffers prefilled with -7)."""
    dev = torch.device("cuda:0")
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    S = c["S"]
    shapes = dict(finals=(S, sw.ns), grad=(sw.Z_len,), grad_samples=(S, sw.T - 1, sw.n_deriv), grad_init=(S, sw.ns), grad_theta=(S, sw.p),
                  grad_scale=(S, sw.m))
    bufs = {k: torch.full(shapes[k], -7.0, dtype=torch.float64, device=dev) for k in want}
    args = (t(Z), t(c["init"]), S, t(c["cot"] if cot is None else cot), t(c["theta"]) if sw.p else None, t(c["scale"]))
    torch.cuda.synchronize()
    sw.vjp_device(*args, **{"d" + k: v for k, v in bufs.items()}, stream=stream)
    (stream.synchronize() if stream is not None else torch.cuda.synchronize())
    return {k: v.cpu().numpy() for k, v in bufs.items()}


def assert_samples(got, want, what):
    """Per sample: |got - want| <= 1e-9 max(1, max |want_s|)."""
    worst = 0.0
    for q in range(want.shape[0]):
        if want[q].size:
            worst = max(worst, np.abs(got[q] - want[q]).max() / (VJP_RTOL * max(1.0, np.abs(want[q]).max())))
    WORST[what] = worst
    print(f"SWEEP-VJP {what}: worst error / bound = {worst:.3e} (max |value| = {np.abs(want).max() if want.size else 0.0:.3e})")
    assert worst <= 1.0, what
    assert not np.isnan(got).any()


def assert_init(got, want, what):
    err = np.abs(got - want)
    worst = (err / (ts.STATE_ATOL + ts.STATE_RTOL * np.abs(want))).max()
    WORST[what] = worst
    print(f"SWEEP-VJP {what}: worst error / (atol + rtol |want|) = {worst:.3e} (max error {err.max():.3e})")
    np.testing.assert_allclose(got, want, rtol=ts.STATE_RTOL, atol=ts.STATE_ATOL)


def plain_sum(gs, sw):
    """The dense gradient the plain sum of per-sample derivatives gives, in the handle's layout, and the mask of its derivative entries."""
    T = sw.T
    out, mask = np.zeros(sw.Z_len), np.zeros(sw.Z_len, dtype=bool)
    K, M = out[:T * sw.zdim].reshape(T, sw.zdim), mask[:T * sw.zdim].reshape(T, sw.zdim)
    tot = gs.sum(axis=0)
    K[:T - 1, sw.off_a:sw.off_a + sw.m] = tot[:, :sw.m]
    M[:T - 1, sw.off_a:sw.off_a + sw.m] = True
    if sw.off_dt >= 0:
        K[:T - 1, sw.off_dt] = tot[:, sw.m]
        M[:T - 1, sw.off_dt] = True
    return out, mask


def check_case(sw, c, form="16", params=True):
    """Every output of one call against the reference and against the call's other shapes."""
    Z = sw.pack(c["controls"], c["dts"])
    S, samples, name = c["S"], c["samples"], f"{form}/{c['name']}"
    want = [k for k in OUTPUTS if not (k == "grad_theta" and not (params and sw.p)) and not (k == "grad_scale" and not (params and sw.m))]
    if c["name"] == "no-drives":
        assert sw.n_deriv == 0
        want = ["finals", "grad_init", "grad_theta"]
    out = device_call(sw, Z, c, want)
    r = reference(c, form)
    if "grad_samples" in want:
        assert_samples(out["grad_samples"][samples], r["grad_samples"], f"{name} grad_samples")
    if "grad_theta" in want:
        assert_samples(out["grad_theta"][samples], r["grad_theta"], f"{name} grad_theta")
    if "grad_scale" in want:
        assert_samples(out["grad_scale"][samples], r["grad_scale"], f"{name} grad_scale")
    assert_init(out["grad_init"][samples], r["grad_init"], f"{name} grad_init")
    np.testing.assert_array_equal(out["finals"], sw.eval(Z, c["init"], c["theta"], c["scale"], fids=False)[0].T)
    if "grad" in want:
        gs = out["grad_samples"]
        dense, mask = plain_sum(gs, sw)
        np.testing.assert_allclose(out["grad"], dense, rtol=0, atol=1e-12 * max(1.0, np.abs(gs).max()) * S)
        zero = out["grad"][~mask]
        assert np.array_equal(zero, np.zeros(zero.size)) and not np.signbit(zero).any()
        assert np.all(out["grad"][mask] != 0)
        # without grad_samples the handle's own scratch takes its place: the same bits
        np.testing.assert_array_equal(device_call(sw, Z, c, ["grad"])["grad"], out["grad"])
    else:
        g = device_call(sw, Z, c, ["grad"])["grad"]
        assert np.array_equal(g.view(np.uint64), np.zeros(g.size, dtype=np.uint64))
    # outputs requested one at a time: the bits of all together
    for k in want:
        np.testing.assert_array_equal(device_call(sw, Z, c, [k])[k], out[k], err_msg=k)
    # the host-buffer entry point
    if "grad" in want:
        par = "grad_theta" in want or "grad_scale" in want
        host = sw.vjp(Z, c["init"], c["cot"], c["theta"], c["scale"], per_sample=True, init_grad=True, params=par)
        for a, k in zip(host, ["grad", "grad_samples", "grad_init"] + (["grad_theta", "grad_scale"] if par else [])):
            if k in out:
                np.testing.assert_array_equal(a, out[k], err_msg=k)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(VJP_CASES))
def test_vjp_matches_the_reference(qc, name):
    c = build(qc, name)
    sw = ts.make_sweep(qc, c)
    try:
        assert sw.kernel_name == "mfma16-sweep" and sw.vjp_supported and sw.vjp_unsupported_reason is None
        want = ts.sweep_launch(2 * c["L"], c["m"], c["S"], c["T"])
        assert sw.launch(c["S"]) == (True, want["chunk"], want["n_chunks"])
        if name == "qubit":
            assert (want["chunk"], want["n_chunks"], want["last"]) == (3, 4, 1)
        if name in ("one-chunk", "one-interval"):
            assert want["n_chunks"] == 1
        if name == "kets3":
            assert not sw.grad_supported
        check_case(sw, c)
    finally:
        sw.close()


def fidelity_seed(x, c):
    """dF/dx at the final state x by the seed formulas (sweep_grad_reference.fidelity_differential, one unit direction at a time)."""
    E = np.eye(x.size)
    return np.array([gref.fidelity_differential(x, E[i], c["kind"], c["goal"], c["L"], c["subspace"], c["form"]) for i in range(x.size)])


def check_against_the_fidelity_gradient(sw, c, what):
    Z = sw.pack(c["controls"], c["dts"])
    finals = sw.eval(Z, c["init"], c["theta"], c["scale"], fids=False)[0]
    cot = np.stack([fidelity_seed(finals[:, s], c) for s in range(c["S"])])
    gs = sw.vjp(Z, c["init"], cot, c["theta"], c["scale"], per_sample=True)[1]
    want = sw.grad(Z, c["init"], c["theta"], c["scale"], per_sample=True)[3]
    assert_samples(gs, want, f"{what} vs qc_sweep_grad")


@pytest.mark.gpu
@pytest.mark.parametrize("name,form", [("qubit", "abs"), ("qubit", "abs2"), ("ket", "abs")])
def test_vjp_consistent_with_the_fidelity_gradient(qc, name, form):
    """With C_s = dF_s/dx formed on the host the pullback's per-sample derivatives are the fidelity gradient's, to the same 1e-9 bound
    (not bit for bit: the host forms the seed in another order)."""
    c = tg.build(qc, name)
    c["form"] = form
    sw = ts.make_sweep(qc, c)
    try:
        check_against_the_fidelity_gradient(sw, c, f"16/{name}-{form}")
    finally:
        sw.close()


def check_bits(qc, make, Z, init, m, ns, T):
    """Six repeated calls; host against device on a side stream; S grows, then shrinks: the bits of a fresh handle."""
    rng = np.random.default_rng(8)
    sw = make()
    side = torch.cuda.Stream(device=torch.device("cuda:0"))
    try:
        for i, S in enumerate((3, 150, 7)):
            c = dict(S=S, init=init, theta=rng.uniform(-0.3, 0.3, (S, 1)), scale=rng.uniform(0.9, 1.1, (S, m)), cot=unit_cotangents(rng, S, ns))
            fresh = make()
            first = fresh.vjp(Z, init, c["cot"], c["theta"], c["scale"], per_sample=True, init_grad=True)
            fresh.close()
            got = sw.vjp(Z, init, c["cot"], c["theta"], c["scale"], per_sample=True, init_grad=True)
            for a, b in zip(got, first):
                np.testing.assert_array_equal(a, b)
            if i == 1:
                for _ in range(6):
                    for a, b in zip(sw.vjp(Z, init, c["cot"], c["theta"], c["scale"], per_sample=True, init_grad=True), first):
                        np.testing.assert_array_equal(a, b)
            with torch.cuda.stream(side):
                out = device_call(sw, Z, c, ["grad", "grad_samples", "grad_init"], stream=side)
            for k, b in zip(("grad", "grad_samples", "grad_init"), first):
                np.testing.assert_array_equal(out[k], b, err_msg=k)
    finally:
        sw.close()


@pytest.mark.gpu
def test_vjp_bits_host_device_and_side_stream(qc):
    rng = np.random.default_rng(9)
    N, m, T = 3, 2, 20
    sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, (N * m) ** -0.5) for _ in range(m)])
    perts = [_herm(rng, N)]
    make = lambda: qc.RolloutSweep(sys_, perts, T, cols=2)
    sw = make()
    Z = sw.pack(rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T))
    sw.close()
    check_bits(qc, make, Z, rng.standard_normal(2 * N * 2), m, 2 * N * 2, T)


def check_isolation(sw, c):
    """A NaN in cot[1] reaches sample 1's outputs and `grad`, nothing else; the handle then serves a finite call; a zero cotangent."""
    Z = sw.pack(c["controls"], c["dts"])
    want = [k for k in OUTPUTS if not (k == "grad_theta" and (sw.kernel_name != "mfma16-sweep" or not sw.p))
            and not (k == "grad_scale" and (sw.kernel_name != "mfma16-sweep" or not sw.m))]
    per_sample = [k for k in want if k not in ("finals", "grad")]
    clean = device_call(sw, Z, c, want)
    assert all(np.isfinite(v).all() for v in clean.values())
    bad = c["cot"].copy()
    col = 1
    bad[1, col * sw.n + 1] = np.nan
    out = device_call(sw, Z, c, want, cot=bad)
    np.testing.assert_array_equal(out["finals"], clean["finals"])
    others = [s for s in range(c["S"]) if s != 1]
    for k in per_sample:
        np.testing.assert_array_equal(out[k][others], clean[k][others], err_msg=k)
        if k != "grad_init":
            assert np.isnan(out[k][1]).all(), k
    # lambda_0 = W^T C: the NaN stays in its own column of the state, the other columns carry the clean bits
    gi, gc = out["grad_init"][1].reshape(-1, sw.n), clean["grad_init"][1].reshape(-1, sw.n)
    assert np.isnan(gi[col]).all()
    np.testing.assert_array_equal(np.delete(gi, col, axis=0), np.delete(gc, col, axis=0))
    _, mask = plain_sum(clean["grad_samples"], sw)
    assert np.isnan(out["grad"][mask]).all()
    zero = out["grad"][~mask]
    assert np.array_equal(zero.view(np.uint64), np.zeros(zero.size, dtype=np.uint64))
    after = device_call(sw, Z, c, want)
    for k in want:
        np.testing.assert_array_equal(after[k], clean[k], err_msg=k)
    nought = device_call(sw, Z, c, want, cot=np.zeros_like(c["cot"]))
    for k in want:
        if k != "finals":
            assert np.all(nought[k] == 0.0), k


@pytest.mark.gpu
def test_vjp_isolation_of_a_non_finite_cotangent(qc):
    c = build(qc, "qubit")
    sw = ts.make_sweep(qc, c)
    try:
        check_isolation(sw, c)
    finally:
        sw.close()


def _raw(qc, sw, fn="qc_sweep_vjp", **null):
    """The host entry point called through ctypes with valid arrays everywhere but where `null` says None / a given array."""
    L = qc._lib
    S = 2
    a = dict(Z=np.zeros(sw.Z_len), init=np.zeros(sw.ns), theta=np.zeros((S, max(sw.p, 1))), scale=None, cot=np.zeros((S, sw.ns)), finals=None,
             grad=np.zeros(sw.Z_len), grad_samples=None, grad_init=None, grad_theta=None, grad_scale=None)
    S = null.pop("S", S)
    a.update(null)
    p = lambda k: None if a[k] is None else L.dptr(a[k])
    rc = L.lib.qc_sweep_vjp(sw._h, p("Z"), p("init"), S, p("theta"), p("scale"), p("cot"), p("finals"), p("grad"), p("grad_samples"), p("grad_init"),
                            p("grad_theta"), p("grad_scale"))
    return rc, L.lib.qc_sweep_last_error(sw._h).decode()


@pytest.mark.gpu
def test_vjp_refusals(qc):
    L = qc._lib
    INV, UNS = L.QC_ERR_INVALID, L.QC_ERR_UNSUPPORTED
    rng = np.random.default_rng(3)
    sys2 = qc.QuantumSystem(_herm(rng, 2), [_herm(rng, 2), _herm(rng, 2)])
    sw = qc.RolloutSweep(sys2, [qc.GATES["Z"]], 5)
    no_pert = qc.RolloutSweep(sys2, [], 5)
    no_drive = qc.RolloutSweep(qc.QuantumSystem(_herm(rng, 2), []), [qc.GATES["Z"]], 5, dt_fixed=0.2)
    sys9 = qc.QuantumSystem(_herm(rng, 9), [_herm(rng, 9)])
    wide = qc.RolloutSweep(sys9, [_herm(rng, 9)], 5, wide=True)
    narrow = qc.RolloutSweep(sys9, [_herm(rng, 9)], 5)
    c_open = ts.build_case(qc, "open2-S11-T2")
    opened = ts.make_sweep(qc, c_open)
    try:
        assert _raw(qc, sw)[0] == L.QC_OK
        for kw, code, word in ((dict(Z=None), INV, "qc_sweep_vjp: NULL input"), (dict(init=None), INV, "qc_sweep_vjp: NULL input"),
                               (dict(cot=None), INV, "qc_sweep_vjp: cot is NULL"), (dict(grad=None), INV, "qc_sweep_vjp: every output is NULL"),
                               (dict(S=0), INV, "qc_sweep_vjp: S must be in 1 .. 2^24"), (dict(S=(1 << 24) + 1), INV, "S must be in 1 .. 2^24"),
                               (dict(theta=None), INV, "qc_sweep_vjp: theta is NULL but the handle has perturbations")):
            rc, msg = _raw(qc, sw, **kw)
            assert rc == code and word in msg, (kw, rc, msg)
        rc, msg = _raw(qc, no_pert, grad_theta=np.zeros((2, 1)))
        assert rc == INV and "grad_theta" in msg and "n_pert = 0" in msg
        rc, msg = _raw(qc, no_drive, grad_scale=np.zeros((2, 1)))
        assert rc == INV and "grad_scale" in msg and "m = 0" in msg
        par_msg = "qc_sweep pullback: parameter cotangents are not served in the mfma32-sweep form"
        assert wide.kernel_name == "mfma32-sweep" and wide.vjp_supported
        for kw in (dict(grad_theta=np.zeros((2, 1))), dict(grad_scale=np.zeros((2, 1)))):
            assert _raw(qc, wide, **kw) == (UNS, par_msg)
        assert _raw(qc, wide)[0] == L.QC_OK
        # the device entry point says the same under its own name
        dev = torch.device("cuda:0")
        z = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)
        with pytest.raises(qc.QCollocError) as e:
            wide.vjp_device(z(wide.Z_len), z(wide.ns), 2, z(2, wide.ns), z(2, 1), dgrad_theta=z(2, 1))
        assert e.value.code == UNS and par_msg in str(e.value)
        rc = L.lib.qc_sweep_vjp_dev(sw._h, z(sw.Z_len).data_ptr(), z(sw.ns).data_ptr(), 2, z(2, 1).data_ptr(), None, None, None, z(sw.Z_len).data_ptr(),
                                    None, None, None, None, None)
        assert rc == INV and L.lib.qc_sweep_last_error(sw._h).decode() == "qc_sweep_vjp_dev: cot is NULL"
        with pytest.raises(ValueError):
            sw.vjp_device(z(sw.Z_len), z(sw.ns), 2, z(2, sw.ns), z(2, 1))
        with pytest.raises(ValueError):
            sw.vjp_device(z(sw.Z_len), z(sw.ns), 2, z(3, sw.ns), z(2, 1), dgrad=z(sw.Z_len))
        # handles out of scope: an open system, the per-sample form
        for h, word in ((opened, "antisymmetric"), (narrow, "2N = 18")):
            assert not h.vjp_supported and word in h.vjp_unsupported_reason and h.vjp_unsupported_reason.startswith("qc_sweep pullback: ")
            rc, msg = _raw(qc, h)
            assert rc == UNS and msg.startswith("qc_sweep pullback: ") and word in msg
        assert narrow.kernel_name == "rollout-per-sample"
        with pytest.raises(qc.QCollocError) as e:
            opened.vjp(opened.pack(c_open["controls"], c_open["dts"]), c_open["init"], np.zeros((11, opened.ns)), c_open["theta"], c_open["scale"])
        assert e.value.code == UNS and "antisymmetric" in str(e.value)
    finally:
        for h in (sw, no_pert, no_drive, wide, narrow, opened):
            h.close()


@pytest.mark.gpu
def test_finals_autograd_gradcheck(qc):
    """torch.autograd.gradcheck of `finals_autograd` composed with a fixed random linear functional, over Z, init, theta and scale
    (eps and atol: the project's finite-difference bound)."""
    rng = np.random.default_rng(31)
    N, m, T, S = 2, 2, 3, 2
    sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, 0.5) for _ in range(m)])
    sw = qc.RolloutSweep(sys_, [_herm(rng, N)], T)
    dev = torch.device("cuda:0")
    t = lambda a, g=True: torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(g)
    try:
        Z = t(sw.pack(rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T)))
        init, theta, scale = t(ref.operator_to_iso_vec(_unitary(rng, N))), t(rng.uniform(-0.3, 0.3, (S, 1))), t(rng.uniform(0.9, 1.1, (S, m)))
        W = t(rng.standard_normal((S, sw.ns)), False)
        X = sw.finals_autograd(Z, init, theta, scale)
        assert X.shape == (S, sw.ns) and X.grad_fn is not None
        fin = torch.empty((S, sw.ns), dtype=torch.float64, device=dev)
        sw.eval_device(Z.detach(), init.detach(), theta.detach(), scale.detach(), fin, None)
        assert torch.equal(X.detach(), fin)
        fn = lambda Z_, i_, th_, sc_: (sw.finals_autograd(Z_, i_, th_, sc_) * W).sum()
        assert torch.autograd.gradcheck(fn, (Z, init, theta, scale), eps=1e-6, atol=1e-6)
        # only what needs a gradient receives one
        Z2, th2 = Z.detach().clone().requires_grad_(True), theta.detach().clone()
        fn(Z2, init.detach(), th2, scale.detach()).backward()
        assert Z2.grad is not None and th2.grad is None
        last = Z2.grad[(T - 1) * sw.zdim:]
        assert torch.equal(last, torch.zeros_like(last))
    finally:
        sw.close()


def _traj3(qc, rng, N, m, T, kets=0):
    """A trajectory with a unitary component (or `kets` ket components), padding, controls and a free timestep."""
    comps, initial, goal = {}, {}, {}
    if kets:
        v = _unitary(rng, N)
        for k in range(kets):
            x = np.concatenate([v[:, k].real, v[:, k].imag])
            comps[f"ψ̃{k}"] = np.repeat(x[:, None], T, axis=1)
            initial[f"ψ̃{k}"] = x.copy()
    else:
        comps["Ũ⃗"] = np.repeat(ref.operator_to_iso_vec(np.eye(N))[:, None], T, axis=1)
        initial["Ũ⃗"] = comps["Ũ⃗"][:, 0].copy()
        goal["Ũ⃗"] = ref.operator_to_iso_vec(_unitary(rng, N))
    comps["pad"] = rng.standard_normal((2, T))
    comps["a"] = rng.uniform(-1, 1, (m, T))
    comps["Δt"] = rng.uniform(0.1, 0.3, (1, T))
    return qc.NamedTrajectory(comps, controls=("a",), timestep="Δt", initial=initial, goal=goal, global_data={"φ": np.array([0.3, -0.2])})


def complex_finals(X, N, cols):
    """S x cols x N complex: entry [s, j, i] = column j, level i of sample s's final state."""
    V = X.reshape(X.shape[0], cols, 2 * N)
    return torch.complex(V[:, :, :N], V[:, :, N:])


@pytest.mark.gpu
def test_final_state_objective_in_an_evaluator(qc):
    """`SweepFinalStateObjective` at N = 3: mean subspace infidelity + 0.5 x leakage against central differences of L (1e-6 relative:
    the finite-difference bound); with the handle's own infidelity as the loss, `SweepInfidelityObjective.grad_L` within the 1e-9 bound."""
    rng = np.random.default_rng(23)
    N, m, T, S = 3, 2, 5, 3
    traj = _traj3(qc, rng, N, m, T)
    sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, 0.5) for _ in range(m)])
    P = np.diag([0.0, 1.0, 2.0]).astype(complex)
    theta, scale = rng.uniform(-0.2, 0.2, (S, 1)), rng.uniform(0.9, 1.1, (S, m))
    G = torch.from_numpy(ref.iso_vec_to_operator(traj.goal["Ũ⃗"], N)).cuda()
    sub = [0, 1]

    def leaky(X):
        U = complex_finals(X, N, N).transpose(1, 2)                   # [s, row, col]
        tr = (G[sub][:, sub].conj() * U[:, sub][:, :, sub]).sum(dim=(1, 2))
        leak = (U[:, 2:, :][:, :, sub].abs() ** 2).sum(dim=(1, 2))
        return (1.0 - tr.abs() / len(sub)).mean() + 0.5 * leak.mean()

    def own(X):
        U = complex_finals(X, N, N).transpose(1, 2)
        return 1.0 - ((G.conj() * U).sum(dim=(1, 2)).abs() / N).mean()

    obj = qc.SweepFinalStateObjective(traj, sys_, [P], theta, leaky, scale=scale)
    Z = traj.datavec

    class _Dyn:      # the evaluator reads the dimensions and structures of its dynamics at construction, nothing else here
        class dims:
            Z_len, n_rows, jac_nnz, hess_nnz = Z.size, 0, 0, 0
        dF_structure = (np.empty(0, dtype=np.int64), np.empty(0, dtype=np.int64))
        mu_d2F_structure = (np.empty(0, dtype=np.int64), np.empty(0, dtype=np.int64))

    try:
        assert obj.hess_structure[0].size == 0 == obj.hess_structure[1].size
        with pytest.raises(RuntimeError):
            obj.hess_L(Z)
        ev = qc.QuantumControlEvaluator(_Dyn(), [obj], eval_hessian=False)
        g = np.empty(Z.size)
        ev.eval_objective_gradient(g, Z)
        np.testing.assert_array_equal(g, np.zeros(Z.size) + obj.grad_L(Z))
        np.testing.assert_array_equal(getattr(obj, "∇L")(Z), obj.grad_L(Z))
        assert ev.eval_objective(Z) == obj.L(Z)
        idx = [t * traj.dim + o for t in range(T - 1) for o in list(range(traj.offset("a"), traj.offset("a") + m)) + [traj.offset("Δt")]]
        fd = np.zeros(Z.size)
        for k in idx:
            e_k = np.zeros(Z.size)
            e_k[k] = 1e-5
            fd[k] = (obj.L(Z + e_k) - obj.L(Z - e_k)) / 2e-5
        err = np.abs(fd - g).max() / max(1.0, np.abs(g).max())
        print(f"SWEEP-VJP objective: central differences vs grad_L {err:.2e} (bound 1e-6), max |grad| {np.abs(g).max():.3f}")
        assert err < 1e-6 and np.abs(g[idx]).min() > 0 and np.count_nonzero(g) == len(idx)
    finally:
        obj.close()
    a = qc.SweepFinalStateObjective(traj, sys_, [P], theta, own, scale=scale)
    b = qc.SweepInfidelityObjective(traj, sys_, [P], theta, scale)
    try:
        assert abs(a.L(Z) - b.L(Z)) <= 1e-13
        ga, gb = a.grad_L(Z), b.grad_L(Z)
        worst = np.abs(ga - gb).max() / (VJP_RTOL * max(1.0, np.abs(gb).max()))
        WORST["objective vs SweepInfidelityObjective"] = worst
        print(f"SWEEP-VJP objective vs SweepInfidelityObjective: worst error / bound = {worst:.3e}")
        assert worst <= 1.0
    finally:
        a.close()
        b.close()


@pytest.mark.gpu
def test_final_state_objective_states_and_refusal(qc):
    """K kets in one component or as a list of ket components: the same final states, columns in the order given.  Construction raises the
    scope's reason when the pullback does not serve the handle."""
    rng = np.random.default_rng(29)
    N, m, T, S = 4, 2, 5, 3
    traj = _traj3(qc, rng, N, m, T, kets=3)
    sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, 0.5) for _ in range(m)])
    theta = rng.uniform(-0.2, 0.2, (S, 1))
    names = ["ψ̃2", "ψ̃0", "ψ̃1"]
    seen = []
    loss = lambda X: (seen.append(tuple(X.shape)), (X ** 2).sum() + X[:, 3].sum())[1]
    P = np.diag(np.arange(N)).astype(complex)
    obj = qc.SweepFinalStateObjective(traj, sys_, [P], theta, loss, state_name=names)
    one = qc.SweepFinalStateObjective(traj, sys_, [P], theta, loss, state_name="ψ̃0")
    try:
        Z = traj.datavec
        X = obj.finals(Z)
        assert X.shape == (S, 2 * N * 3)
        np.testing.assert_array_equal(X[:, 2 * N:4 * N], one.finals(Z))          # the second column is ψ̃0
        assert np.isfinite(obj.L(Z)) and seen[-1] == (S, 2 * N * 3)
        g = obj.grad_L(Z)
        assert g.shape == Z.shape and np.count_nonzero(g) == (T - 1) * (m + 1)
    finally:
        obj.close()
        one.close()
    with pytest.raises(ValueError, match="no component"):
        qc.SweepFinalStateObjective(traj, sys_, [], theta, loss, state_name="nope")
    with pytest.raises(ValueError, match="callable"):
        qc.SweepFinalStateObjective(traj, sys_, [], theta, None, state_name=names)
    sys9 = qc.QuantumSystem(_herm(rng, 9), [_herm(rng, 9), _herm(rng, 9)])
    traj9 = _traj3(qc, rng, 9, m, T)
    with pytest.raises(qc.QCollocError) as e:
        qc.SweepFinalStateObjective(traj9, sys9, [_herm(rng, 9)], theta, loss)
    assert e.value.code == qc._lib.QC_ERR_UNSUPPORTED and "qc_sweep pullback: " in str(e.value) and "2N = 18" in str(e.value)


@pytest.mark.gpu
def test_leakage_robust_polish_example(qc):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import leakage_robust_polish
    out = leakage_robust_polish.main(T=6, grid=3, steps=3, verbose=False)
    print(f"loss {out['loss_before']:.4e} -> {out['loss_after']:.4e}, leakage {out['leakage_before']:.4e} -> {out['leakage_after']:.4e}")
    assert out["kernel"] == "mfma16-sweep"
    assert out["loss_after"] <= out["loss_before"] and out["leakage_after"] < out["leakage_before"]
