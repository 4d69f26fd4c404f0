"""Sweep pushforwards (`qc_sweep_jvp*`, `RolloutSweep.jvp` / `jvp_device`, the forward-mode rule of `finals_autograd`,
`SweepFinalStateObjective.gauss_newton_times`): the tangent of the final states and fidelities along one direction, on "mfma16-sweep"
handles with any generators.  CPU: the two routes of tests/sweep_jvp_reference.py against each other, the device-free scope query,
prototypes and mirrors.  GPU: every requested value against the Frechet route, bit-level properties, the adjoint identity against the
pullback, the fidelity tangents against the gradient, isolation of a non-finite direction, refusals, autograd in both modes, the
Gauss-Newton product, the example.

Tolerance (GPU against the reference).  The two reference routes agree to 1e-13 or better at every size used here (the CPU test
holds them to 1e-11).  The kernels hold the states to 1e-10 (test_sweep.py), and a tangent is a bounded bilinear form of states and
direction -- the argument of GRAD_RTOL in tests/test_sweep_grad.py: per sample |got - want| <= 1e-9 max(1, max |want_s|) for tfinals
and tfids.  finals: the state tolerance of test_sweep.py.  The adjoint identity compares two quantities that are each within 1e-9 of the
truth: 2e-9.
Every sample of mid-size and filled launches, the scratch `dTotJ`: tests/test_sweep_jvp_every_sample.py; states of up to 4096 entries:
tests/test_sweep_many_columns.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import sweep_jvp_reference as jref
import sweep_reference as ref
import test_sweep as ts
import test_sweep_grad as tg
import test_sweep_wide as tw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JVP_RTOL = 1e-9
_herm, _unitary = ts._herm, ts._unitary
U_ABS = ("unitary", None, "abs")

# name: (state, levels, m, p, scale given, free timestep, S, T, fidelity, samples checked against the reference)
JVP_CASES = {
    "qubit": ("unitary", 2, 2, 1, False, True, 5, 11, U_ABS, None),                                   # chunks of 3, 3, 3, 1
    "qutrit": ("unitary", 3, 1, 3, True, False, 7, 10, ("unitary", [0, 1], "abs2"), None),            # padded tile, vtheta and vscale
    "levels8-6drives": ("unitary", 8, 6, 1, True, True, 3, 6, U_ABS, None),                           # full tile, M = 6
    "levels8-8drives": ("unitary", 8, 8, 1, True, True, 3, 6, U_ABS, None),                           # M = 8
    "levels4-3drives": ("unitary", 4, 3, 1, True, True, 3, 6, U_ABS, None),                           # a zero-padded slot of M = 4
    "levels4-5drives": ("unitary", 4, 5, 1, True, True, 3, 6, U_ABS, None),                           # ... of M = 6
    "ket": ("ket", 4, 2, 1, True, True, 11, 6, ("ket", None, "abs"), None),
    "kets3": ("kets3", 4, 2, 1, True, True, 3, 8, None, None),                                        # no fidelity
    "density": ("density", 2, 2, 1, True, True, 5, 9, ("density", None, "abs"), None),                # Lindblad: `grad` / `vjp` refuse it
    "no-drives": ("unitary", 2, 0, 1, False, False, 3, 6, U_ABS, None),                               # only vtheta and vinit act
    "one-interval": ("unitary", 2, 2, 1, False, True, 3, 2, U_ABS, None),
    "one-chunk": ("unitary", 2, 2, 1, True, True, 2048, 4, U_ABS, (0, 1000, 2047)),
    "squarings": ("unitary", 8, 2, 1, False, True, 3, 8, U_ABS, None),                                # timesteps log-uniform in [1e-3, 40]
    "long": ("unitary", 8, 2, 1, False, True, 2, 1000, U_ABS, None),                                  # 32 chunks of 32, the last 7
}
CLOSED = [k for k in JVP_CASES if k != "density"]
_REF = {}          # case name -> reference dict: computed once, shared, never written to


def build(qc, name):
    """The case of test_sweep_wide.build plus a direction with every part that exists non-zero."""
    c = tw.build(qc, name, JVP_CASES[name])
    rng = np.random.default_rng(11 + sum(map(ord, name)))
    S, T, m, p, ns = c["S"], c["T"], c["m"], c["p"], c["init"].size
    if name == "squarings":
        c["dts"] = np.exp(rng.uniform(np.log(1e-3), np.log(40.0), T))
        c["dts"][0], c["dts"][1] = 1e-3, 40.0
    free = np.ndim(c["dts"]) != 0
    c["vcontrols"] = rng.standard_normal((m, T))
    c["vdts"] = None
    if free:
        c["vdts"] = rng.standard_normal(T) * c["dts"] if name == "squarings" else 0.1 * rng.standard_normal(T)
    c["vinit"] = rng.standard_normal(ns) / np.sqrt(ns)
    c["vtheta"] = rng.standard_normal((S, p)) if p else None
    c["vscale"] = rng.standard_normal((S, m)) if m else None
    c["fid"] = None if c["kind"] is None else (c["kind"], c["goal"], c["L"], c["subspace"], c["form"])
    return c


def reference(c):
    if c["name"] not in _REF:
        out = jref.pushforward_frechet(c["G0"], c["Gd"], c["Gp"], c["controls"], c["dts"], c["init"], c["theta"], c["scale"], c["samples"],
                                       c["vcontrols"], c["vdts"], c["vinit"], c["vtheta"], c["vscale"], c["fid"])
        for a in out.values():
            if a is not None:
                a.setflags(write=False)
        _REF[c["name"]] = out
    return _REF[c["name"]]


# ---------------------------------------------------------------------------------------------------------------------------------
#  CPU
# ---------------------------------------------------------------------------------------------------------------------------------
_STATES = {"unitary": U_ABS, "ket": ("ket", None, "abs"), "kets3": None, "density": ("density", None, "abs")}


@pytest.mark.parametrize("free", [True, False], ids=["free-dt", "fixed-dt"])
@pytest.mark.parametrize("state", list(_STATES))
@pytest.mark.parametrize("N", [2, 3, 8])
def test_reference_routes_agree(qc, N, state, free):
    """expm_frechet along the recurrence against the complex step through expm: 1e-11 max(1, max |want|)."""
    name = f"routes-{N}-{state}-{free}"
    c = tw.build(qc, name, (state, N, 2, 1, True, free, 2, 5, _STATES[state], None))
    rng = np.random.default_rng(5 + sum(map(ord, name)))
    ns, T = c["init"].size, c["T"]
    fid = None if c["kind"] is None else (c["kind"], c["goal"], c["L"], c["subspace"], c["form"])
    args = (c["G0"], c["Gd"], c["Gp"], c["controls"], c["dts"], c["init"], c["theta"], c["scale"], [0, 1])
    kw = dict(vcontrols=rng.standard_normal((2, T)), vdts=0.1 * rng.standard_normal(T) if free else None, vinit=rng.standard_normal(ns) / np.sqrt(ns),
              vtheta=rng.standard_normal((2, 1)), vscale=rng.standard_normal((2, 2)), fid=fid)
    a, b = jref.pushforward_frechet(*args, **kw), jref.pushforward_complex_step(*args, **kw)
    assert a["tfinals"].shape == b["tfinals"].shape == (2, ns)
    for key in ("finals", "tfinals", "tfids"):
        if a[key] is None:
            assert fid is None and b[key] is None
            continue
        err = np.abs(a[key] - b[key]).max() / max(1.0, np.abs(a[key]).max())
        print(f"SWEEP-JVP reference n={c['n']} {state} free={free} {key}: frechet vs complex step {err:.2e}, max |value| {np.abs(a[key]).max():.3f}")
        assert err <= 1e-11 and np.abs(a[key]).max() > 1e-3, key


def _supported(qc, D):
    ok = C.c_int32(-1)
    rc = qc._lib.lib.qc_sweep_desc_jvp_supported(C.byref(D.d), C.byref(ok))
    return rc, ok.value, qc._lib.lib.qc_sweep_last_error(None).decode()


def test_jvp_scope_without_a_device(qc):
    L = qc._lib
    U = L.QC_FID_UNITARY
    open2 = tg._GDesc(qc, N=4, m=2, cols=1, fid_kind=L.QC_FID_DENSITY)        # a Lindblad generator: n = 8, not antisymmetric
    open2.G0[:] = np.random.default_rng(0).standard_normal(64)
    served = {"closed": tg._GDesc(qc, N=2, m=2, fid_kind=U), "open": open2, "no fidelity": tg._GDesc(qc, N=4, m=2, cols=3),
              "8 drives, 17 columns": tg._GDesc(qc, N=8, m=8, cols=17)}
    for what, D in served.items():
        assert _supported(qc, D)[:2] == (L.QC_OK, 1), what
    wide12 = tg._GDesc(qc, N=12, m=2, fid_kind=U)
    wide12.d.wide = 1
    refused = {"N = 12": (tg._GDesc(qc, N=12, m=2, fid_kind=U), "rollout-per-sample form (2N = 24 > 16)"),
               "N = 12, wide": (wide12, "not served in the mfma32-sweep form"),
               "9 drives": (tg._GDesc(qc, N=2, m=9), "rollout-per-sample form (9 drives > 8)")}
    for what, (D, word) in refused.items():
        rc, ok, msg = _supported(qc, D)
        assert (rc, ok) == (L.QC_OK, 0), what
        assert msg.startswith("qc_sweep pushforward: ") and word in msg, (what, msg)
    assert _supported(qc, tg._GDesc(qc, T=1))[0] == L.QC_ERR_INVALID
    assert "T must be >= 2" in L.lib.qc_sweep_last_error(None).decode()
    assert L.lib.qc_sweep_desc_jvp_supported(C.byref(served["closed"].d), None) == L.QC_ERR_INVALID
    assert "qc_sweep_desc_jvp_supported" in L.lib.qc_sweep_last_error(None).decode()


def test_jvp_prototypes_header_and_mirrors(qc):
    L = qc._lib
    for name, nargs in (("qc_sweep_desc_jvp_supported", 2), ("qc_sweep_jvp", 14), ("qc_sweep_jvp_dev", 15)):
        assert name in L.SYMBOLS and len(L.SYMBOLS[name][1]) == nargs
        assert getattr(L.lib, name).argtypes is not None
    header = open(os.path.join(ROOT, "include", "qcolloc.h")).read()
    for decl in ("int qc_sweep_desc_jvp_supported(const qc_sweep_desc* d, int32_t* supported);", "int qc_sweep_jvp_dev(qc_sweep* h,",
                 "int qc_sweep_jvp(qc_sweep* h,", "const double* dvZ, const double* dvinit, const double* dvtheta, const double* dvscale,",
                 "double* dfinals, double* dfids, double* dtfinals, double* dtfids, void* stream);"):
        assert decl in header, decl
    assert "pushforwards on \"mfma32-sweep\" and \"rollout-per-sample\" handles" in header
    assert "(they need stored forward states), second derivatives, several devices" not in header
    x = np.zeros(8)
    p = L.dptr(x)
    assert L.lib.qc_sweep_jvp(None, p, p, 1, p, None, p, None, None, None, None, None, p, None) == L.QC_ERR_INVALID
    assert L.lib.qc_sweep_last_error(None).decode() == "qc_sweep_jvp: NULL handle"
    assert L.lib.qc_sweep_jvp_dev(None, None, None, 1, None, None, None, None, None, None, None, None, None, None, None) == L.QC_ERR_INVALID
    assert L.lib.qc_sweep_last_error(None).decode() == "qc_sweep_jvp_dev: NULL handle"
    assert L.lib.qc_abi_version() == 6      # additive: the ABI stays 0.6
    julia = open(os.path.join(ROOT, "julia", "QCollocHIP.jl"), encoding="utf-8").read()
    assert "function rollout_sweep_pushforward(" in julia and "(:qc_sweep_jvp, LIB[])" in julia and "(:qc_sweep_desc_jvp_supported, LIB[])" in julia
    for kw in ("vZ=nothing", "vinit=nothing", "vtheta=nothing", "vscale=nothing"):
        assert kw in julia
    import inspect
    for attr in ("jvp", "jvp_device", "jvp_supported", "jvp_unsupported_reason"):
        assert hasattr(qc.RolloutSweep, attr)
    assert list(inspect.signature(qc.RolloutSweep.jvp).parameters)[1:] == ["Z", "init", "vZ", "theta", "scale", "vinit", "vtheta", "vscale", "fids"]
    assert hasattr(qc.SweepFinalStateObjective, "gauss_newton_times")
    from qcolloc_amd.rollouts import _SweepFinals
    assert _SweepFinals.jvp is not torch.autograd.Function.jvp


# ---------------------------------------------------------------------------------------------------------------------------------
#  GPU
# ---------------------------------------------------------------------------------------------------------------------------------
OUTPUTS = ("finals", "fids", "tfinals", "tfids")
DIRS = ("vZ", "vinit", "vtheta", "vscale")
WORST = {}


def direction(sw, c):
    """The four directions in the handle's layouts (None where the handle has none)."""
    return dict(vZ=sw.pack(c["vcontrols"], c["vdts"]), vinit=c["vinit"], vtheta=c["vtheta"], vscale=c["vscale"])


def device_call(sw, Z, c, want, dirs, stream=None):
    """One `jvp_device` call for the outputs named in `want` along `dirs`; numpy arrays back (buffers prefilled with -7)."""
    dev = torch.device("cuda:0")
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    S = c["S"]
    shapes = dict(finals=(S, sw.ns), fids=(S,), tfinals=(S, sw.ns), tfids=(S,))
    bufs = {k: torch.full(shapes[k], -7.0, dtype=torch.float64, device=dev) for k in want}
    torch.cuda.synchronize()
    sw.jvp_device(t(Z), t(c["init"]), S, t(c["theta"]) if sw.p else None, t(c["scale"]), **{"d" + k: t(v) for k, v in dirs.items()},
                  **{"d" + k: v for k, v in bufs.items()}, stream=stream)
    (stream.synchronize() if stream is not None else torch.cuda.synchronize())
    return {k: v.cpu().numpy() for k, v in bufs.items()}


def assert_samples(got, want, what):
    """Per sample: |got - want| <= 1e-9 max(1, max |want_s|)."""
    worst = 0.0
    for q in range(want.shape[0]):
        worst = max(worst, np.abs(got[q] - want[q]).max() / (JVP_RTOL * max(1.0, np.abs(want[q]).max())))
    WORST[what] = worst
    print(f"SWEEP-JVP {what}: worst error / bound = {worst:.3e} (max |value| = {np.abs(want).max():.3e})")
    assert worst <= 1.0, what
    assert not np.isnan(got).any()


def outputs_of(sw):
    return [k for k in OUTPUTS if sw.fid_kind != -1 or k in ("finals", "tfinals")]


def check_case(sw, c):
    Z = sw.pack(c["controls"], c["dts"])
    samples, name = c["samples"], c["name"]
    want = outputs_of(sw)
    dirs = {k: v for k, v in direction(sw, c).items() if v is not None}
    out = device_call(sw, Z, c, want, dirs)
    r = reference(c)
    # values
    assert_samples(out["tfinals"][samples], r["tfinals"], f"{name} tfinals")
    err = np.abs(out["finals"][samples] - r["finals"])
    print(f"SWEEP-JVP {name} finals: worst error / (atol + rtol |want|) = {(err / (ts.STATE_ATOL + ts.STATE_RTOL * np.abs(r['finals']))).max():.3e}")
    np.testing.assert_allclose(out["finals"][samples], r["finals"], rtol=ts.STATE_RTOL, atol=ts.STATE_ATOL)
    if "tfids" in want:
        assert_samples(out["tfids"][samples, None], r["tfids"][:, None], f"{name} tfids")
    # bits: the sweep's own finals / fids
    finals, fids = sw.eval(Z, c["init"], c["theta"], c["scale"], fids="fids" in want)
    np.testing.assert_array_equal(out["finals"], finals.T)
    if "fids" in want:
        np.testing.assert_array_equal(out["fids"], fids)
    # a second call; each output alone
    again = device_call(sw, Z, c, want, dirs)
    for k in want:
        np.testing.assert_array_equal(again[k], out[k], err_msg=k)
        np.testing.assert_array_equal(device_call(sw, Z, c, [k], dirs)[k], out[k], err_msg=k + " alone")
    # a NULL direction is an explicit zero array, one direction at a time
    for k in dirs:
        some = {q: v for q, v in dirs.items() if q != k}
        if not some:
            continue
        a = device_call(sw, Z, c, want, some)
        b = device_call(sw, Z, c, want, dict(some, **{k: np.zeros_like(dirs[k])}))
        for o in want:
            np.testing.assert_array_equal(a[o], b[o], err_msg=f"{o} without {k}")
    # an all-zero direction through non-NULL arrays
    nought = device_call(sw, Z, c, want, {k: np.zeros_like(v) for k, v in dirs.items()})
    assert np.all(nought["tfinals"] == 0.0)
    np.testing.assert_array_equal(nought["finals"], out["finals"])
    # the host-buffer entry point; the device entry point on a side stream
    host = sw.jvp(Z, c["init"], dirs.get("vZ"), c["theta"], c["scale"], vinit=dirs.get("vinit"), vtheta=dirs.get("vtheta"), vscale=dirs.get("vscale"),
                  fids="tfids" in want)
    np.testing.assert_array_equal(host[0] if "tfids" in want else host, out["tfinals"])
    if "tfids" in want:
        np.testing.assert_array_equal(host[1], out["tfids"])
    side = torch.cuda.Stream(device=torch.device("cuda:0"))
    with torch.cuda.stream(side):
        other = device_call(sw, Z, c, want, dirs, stream=side)
    for k in want:
        np.testing.assert_array_equal(other[k], out[k], err_msg=k + " on a side stream")
    # only the controls and timesteps of knots 0 .. T-2 of vZ are read
    if "vZ" in dirs:
        K = np.zeros(sw.Z_len, dtype=bool)
        Kt = K[:sw.T * sw.zdim].reshape(sw.T, sw.zdim)
        Kt[:sw.T - 1, sw.off_a:sw.off_a + sw.m] = True
        if sw.off_dt >= 0:
            Kt[:sw.T - 1, sw.off_dt] = True
        poisoned = dirs["vZ"].copy()
        poisoned[~K] = np.nan
        assert np.isnan(poisoned).sum() >= sw.zdim
        bad = device_call(sw, Z, c, want, dict(dirs, vZ=poisoned))
        for k in want:
            np.testing.assert_array_equal(bad[k], out[k], err_msg=k + " with NaNs in the unread entries of vZ")
    return out, dirs


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(JVP_CASES))
def test_jvp_matches_the_reference(qc, name):
    c = build(qc, name)
    sw = ts.make_sweep(qc, c)
    try:
        assert sw.kernel_name == "mfma16-sweep" and sw.jvp_supported and sw.jvp_unsupported_reason is None
        want = ts.sweep_launch(c["n"], c["m"], c["S"], c["T"])
        assert sw.launch(c["S"]) == (True, want["chunk"], want["n_chunks"])
        if name == "qubit":
            assert (want["chunk"], want["n_chunks"], want["last"]) == (3, 4, 1)
        if name in ("one-chunk", "one-interval"):
            assert want["n_chunks"] == 1
        if name == "long":
            assert (want["chunk"], want["n_chunks"], want["last"]) == (32, 32, 7)
        if name == "density":
            assert c["n"] == 8 and not sw.grad_supported and not sw.vjp_supported
        if name == "squarings":
            th = c["theta"]
            sq = [ts._squarings(np.abs(c["dts"][t] * ref.sample_generator(c["G0"], c["Gd"], c["Gp"], c["controls"][:, t], th[s], np.ones(c["m"]))).sum(axis=0).max())
                  for s in range(c["S"]) for t in range(c["T"] - 1)]
            assert min(sq) == 0 and max(sq) >= 8, sq
        check_case(sw, c)
    finally:
        sw.close()


def pairing(sw, c, dirs, pull):
    """grad_samples[s] . v + grad_init[s] . vinit + grad_theta[s] . vtheta[s] + grad_scale[s] . vscale[s] of every sample, from the pullback's
    outputs `pull` = (grad, grad_samples, grad_init[, grad_theta, grad_scale])."""
    gs, gi = pull[1], pull[2]
    S, T = c["S"], sw.T
    V = dirs["vZ"][:T * sw.zdim].reshape(T, sw.zdim)[:T - 1]
    v = np.concatenate([V[:, sw.off_a:sw.off_a + sw.m]] + ([V[:, sw.off_dt:sw.off_dt + 1]] if sw.off_dt >= 0 else []), axis=1)
    out = np.einsum("stk,tk->s", gs, v) + gi @ dirs["vinit"]
    if len(pull) > 3:
        if sw.p:
            out += np.einsum("sj,sj->s", pull[3], dirs["vtheta"])
        if sw.m:
            out += np.einsum("sk,sk->s", pull[4], dirs["vscale"])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", CLOSED)
def test_jvp_adjoint_identity_with_the_pullback(qc, name):
    """<C_s, tfinals[s]> is the pullback's derivative paired with the direction, for unit cotangents C, on every closed case and every
    sample of it: 2e-9 max(1, .)."""
    c = build(qc, name)
    sw = ts.make_sweep(qc, c)
    try:
        assert sw.vjp_supported
        Z = sw.pack(c["controls"], c["dts"])
        dirs = direction(sw, c)
        rng = np.random.default_rng(3)
        cot = rng.standard_normal((c["S"], sw.ns))
        cot /= np.linalg.norm(cot, axis=1, keepdims=True)
        tf = sw.jvp(Z, c["init"], dirs["vZ"], c["theta"], c["scale"], vinit=dirs["vinit"], vtheta=dirs["vtheta"], vscale=dirs["vscale"])
        lhs = np.einsum("sn,sn->s", cot, tf)
        rhs = pairing(sw, c, dirs, sw.vjp(Z, c["init"], cot, c["theta"], c["scale"], per_sample=True, init_grad=True, params=True))
        worst = (np.abs(lhs - rhs) / (2 * JVP_RTOL * np.maximum(1.0, np.abs(rhs)))).max()
        print(f"SWEEP-JVP {name} adjoint identity: worst error / bound = {worst:.3e} (max |value| = {np.abs(rhs).max():.3e})")
        assert worst <= 1.0 and np.abs(rhs).max() > 1e-3
    finally:
        sw.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["qubit", "qutrit", "ket"])
def test_jvp_fidelity_tangents_against_the_gradient(qc, name):
    """tfids[s] along vZ alone is `grad`'s grad_samples[s] . v, to the bound of the adjoint identity."""
    c = build(qc, name)
    sw = ts.make_sweep(qc, c)
    try:
        assert sw.grad_supported
        Z = sw.pack(c["controls"], c["dts"])
        dirs = direction(sw, c)
        _, tfids = sw.jvp(Z, c["init"], dirs["vZ"], c["theta"], c["scale"], fids=True)
        gs = sw.grad(Z, c["init"], c["theta"], c["scale"], per_sample=True)[3]
        rhs = pairing(sw, c, dict(dirs, vinit=np.zeros(sw.ns)), (None, gs, np.zeros((c["S"], sw.ns))))
        worst = (np.abs(tfids - rhs) / (2 * JVP_RTOL * np.maximum(1.0, np.abs(rhs)))).max()
        print(f"SWEEP-JVP {name} tfids vs qc_sweep_grad: worst error / bound = {worst:.3e} (max |value| = {np.abs(rhs).max():.3e})")
        assert worst <= 1.0 and np.abs(rhs).max() > 1e-3
    finally:
        sw.close()


@pytest.mark.gpu
def test_jvp_isolation_of_a_non_finite_direction(qc):
    """A NaN in vtheta[1] makes sample 1's tangents non-finite and leaves every other sample's bits as they were."""
    c = build(qc, "qutrit")
    sw = ts.make_sweep(qc, c)
    try:
        Z = sw.pack(c["controls"], c["dts"])
        dirs = direction(sw, c)
        want = outputs_of(sw)
        clean = device_call(sw, Z, c, want, dirs)
        for which in ("vtheta", "vscale"):
            bad = dirs[which].copy()
            bad[1, 0] = np.nan
            out = device_call(sw, Z, c, want, dict(dirs, **{which: bad}))
            others = [s for s in range(c["S"]) if s != 1]
            for k in want:
                np.testing.assert_array_equal(out[k][others], clean[k][others], err_msg=k)
            np.testing.assert_array_equal(out["finals"], clean["finals"])
            np.testing.assert_array_equal(out["fids"], clean["fids"])
            assert not np.isfinite(out["tfinals"][1]).any() and not np.isfinite(out["tfids"][1])
        after = device_call(sw, Z, c, want, dirs)
        for k in want:
            np.testing.assert_array_equal(after[k], clean[k], err_msg=k)
    finally:
        sw.close()


def _raw(qc, sw, **null):
    """The host entry point called through ctypes with valid arrays everywhere but where `null` says None / a given array."""
    L = qc._lib
    S = 2
    a = dict(Z=np.zeros(sw.Z_len), init=np.zeros(sw.ns), theta=np.zeros((S, max(sw.p, 1))), scale=None, vZ=np.zeros(sw.Z_len), vinit=None, vtheta=None,
             vscale=None, finals=None, fids=None, tfinals=np.zeros((S, sw.ns)), tfids=None)
    S = null.pop("S", S)
    a.update(null)
    p = lambda k: None if a[k] is None else L.dptr(a[k])
    rc = L.lib.qc_sweep_jvp(sw._h, *(p(k) for k in ("Z", "init")), S, *(p(k) for k in ("theta", "scale", "vZ", "vinit", "vtheta", "vscale", "finals", "fids",
                                                                                          "tfinals", "tfids")))
    return rc, L.lib.qc_sweep_last_error(sw._h).decode()


@pytest.mark.gpu
def test_jvp_refusals(qc):
    L = qc._lib
    INV, UNS = L.QC_ERR_INVALID, L.QC_ERR_UNSUPPORTED
    rng = np.random.default_rng(3)
    sys2 = qc.QuantumSystem(_herm(rng, 2), [_herm(rng, 2), _herm(rng, 2)])
    sw = qc.RolloutSweep(sys2, [qc.GATES["Z"]], 5)
    no_pert = qc.RolloutSweep(sys2, [], 5)
    no_drive = qc.RolloutSweep(qc.QuantumSystem(_herm(rng, 2), []), [qc.GATES["Z"]], 5, dt_fixed=0.2)
    cw = tw.build(qc, "transmons9-S11-T50", tw.WIDE_CASES["transmons9-S11-T50"])
    wide = ts.make_sweep(qc, cw, wide=True)
    c9 = ts.build_case(qc, "qubit-9drives-S11-T50")
    nine = ts.make_sweep(qc, c9)
    try:
        assert _raw(qc, sw)[0] == L.QC_OK
        for kw, word in ((dict(Z=None), "qc_sweep_jvp: NULL input"), (dict(init=None), "qc_sweep_jvp: NULL input"),
                         (dict(vZ=None), "qc_sweep_jvp: every direction is NULL"), (dict(tfinals=None), "qc_sweep_jvp: every output is NULL"),
                         (dict(S=0), "qc_sweep_jvp: S must be in 1 .. 2^24"), (dict(S=(1 << 24) + 1), "qc_sweep_jvp: S must be in 1 .. 2^24"),
                         (dict(theta=None), "qc_sweep_jvp: theta is NULL but the handle has perturbations"),
                         (dict(fids=np.zeros(2)), "qc_sweep_jvp: fidelities or their tangents requested from a handle created without one"),
                         (dict(tfids=np.zeros(2)), "qc_sweep_jvp: fidelities or their tangents requested from a handle created without one")):
            rc, msg = _raw(qc, sw, **kw)
            assert rc == INV and msg == word, (kw, rc, msg)
        rc, msg = _raw(qc, no_pert, vtheta=np.zeros((2, 1)))
        assert rc == INV and msg.startswith("qc_sweep_jvp: vtheta") and "n_pert = 0" in msg
        rc, msg = _raw(qc, no_drive, vscale=np.zeros((2, 1)))
        assert rc == INV and msg.startswith("qc_sweep_jvp: vscale") and "m = 0" in msg
        # vscale with scale = NULL is valid
        assert _raw(qc, sw, vscale=np.ones((2, 2)))[0] == L.QC_OK
        # the device entry point says the same under its own name
        dev = torch.device("cuda:0")
        z = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)
        rc = L.lib.qc_sweep_jvp_dev(sw._h, z(sw.Z_len).data_ptr(), z(sw.ns).data_ptr(), 2, z(2, 1).data_ptr(), None, None, None, None, None, None, None,
                                    z(2, sw.ns).data_ptr(), None, None)
        assert rc == INV and L.lib.qc_sweep_last_error(sw._h).decode() == "qc_sweep_jvp_dev: every direction is NULL"
        with pytest.raises(ValueError):
            sw.jvp_device(z(sw.Z_len), z(sw.ns), 2, z(2, 1), dtfinals=z(2, sw.ns))
        with pytest.raises(ValueError):
            sw.jvp_device(z(sw.Z_len), z(sw.ns), 2, z(2, 1), dvZ=z(sw.Z_len))
        with pytest.raises(ValueError):
            sw.jvp_device(z(sw.Z_len), z(sw.ns), 2, z(2, 1), dvZ=z(sw.Z_len + 1), dtfinals=z(2, sw.ns))
        # handles out of scope still serve eval
        for h, c, word in ((wide, cw, "not served in the mfma32-sweep form"), (nine, c9, "9 drives")):
            assert not h.jvp_supported and word in h.jvp_unsupported_reason and h.jvp_unsupported_reason.startswith("qc_sweep pushforward: ")
            rc, msg = _raw(qc, h)
            assert rc == UNS and msg == h.jvp_unsupported_reason
            Zc = h.pack(c["controls"], c["dts"])
            with pytest.raises(qc.QCollocError) as e:
                h.jvp(Zc, c["init"], np.zeros(h.Z_len), c["theta"], c["scale"])
            assert e.value.code == UNS and word in str(e.value)
            finals, _ = h.eval(Zc, c["init"], c["theta"], c["scale"], fids=False)
            assert np.isfinite(finals).all()
        assert wide.kernel_name == "mfma32-sweep" and nine.kernel_name == "rollout-per-sample"
    finally:
        for h in (sw, no_pert, no_drive, wide, nine):
            h.close()


@pytest.mark.gpu
def test_finals_autograd_forward_mode(qc):
    """Under forward_ad the tangent of `finals_autograd` is `jvp_device`'s tfinals, bit for bit, for tangents on Z, init and theta;
    reverse mode on the same inputs gives the bits of `vjp_device`."""
    import torch.autograd.forward_ad as fwAD
    rng = np.random.default_rng(37)
    N, m, T, S = 2, 2, 5, 3
    sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, 0.5) for _ in range(m)])
    sw = qc.RolloutSweep(sys_, [_herm(rng, N)], T)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    try:
        Z, init = t(sw.pack(rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T))), t(ref.operator_to_iso_vec(_unitary(rng, N)))
        theta, scale = t(rng.uniform(-0.3, 0.3, (S, 1))), t(rng.uniform(0.9, 1.1, (S, m)))
        vZ, vinit, vtheta = t(rng.standard_normal(sw.Z_len)), t(rng.standard_normal(sw.ns)), t(rng.standard_normal((S, 1)))
        fin = torch.empty((S, sw.ns), dtype=torch.float64, device=dev)
        sw.eval_device(Z, init, theta, scale, fin, None)
        for which in ("Z", "init", "theta", "all"):
            use = dict(Z=which in ("Z", "all"), init=which in ("init", "all"), theta=which in ("theta", "all"))
            want = torch.empty((S, sw.ns), dtype=torch.float64, device=dev)
            sw.jvp_device(Z, init, S, theta, scale, dvZ=vZ if use["Z"] else None, dvinit=vinit if use["init"] else None,
                          dvtheta=vtheta if use["theta"] else None, dtfinals=want)
            with fwAD.dual_level():
                dual = lambda x, v, on: fwAD.make_dual(x, v) if on else x
                X = sw.finals_autograd(dual(Z, vZ, use["Z"]), dual(init, vinit, use["init"]), dual(theta, vtheta, use["theta"]), scale)
                primal, tangent = fwAD.unpack_dual(X)
                assert tangent is not None, which
                assert torch.equal(primal, fin) and torch.equal(tangent, want), which
        # reverse mode is what it was: the bits of one vjp_device call
        cot = t(rng.standard_normal((S, sw.ns)))
        Zr, ir, thr = Z.clone().requires_grad_(True), init.clone().requires_grad_(True), theta.clone().requires_grad_(True)
        Xr = sw.finals_autograd(Zr, ir, thr, scale)
        assert torch.equal(Xr.detach(), fin)
        (Xr * cot).sum().backward()
        gZ, gI, gT = torch.empty(sw.Z_len, dtype=torch.float64, device=dev), torch.empty((S, sw.ns), dtype=torch.float64, device=dev), torch.empty(
            (S, 1), dtype=torch.float64, device=dev)
        sw.vjp_device(Z, init, S, cot, theta, scale, dgrad=gZ, dgrad_init=gI, dgrad_theta=gT)
        assert torch.equal(Zr.grad, gZ) and torch.equal(ir.grad, gI.sum(0)) and torch.equal(thr.grad, gT)
    finally:
        sw.close()


@pytest.mark.gpu
def test_gauss_newton_product(qc):
    """`gauss_newton_times` on a qubit (T = 4) with loss = sum ||X - G||^2 / (2 S) against J^T J v / S assembled on the CPU from the Frechet
    route over the unit directions; symmetry and the quadratic form; a linear loss; a wide handle."""
    import test_sweep_vjp as tv
    rng = np.random.default_rng(41)
    N, m, T, S = 2, 2, 4, 3
    traj = tv._traj3(qc, rng, N, m, T)
    H0, Hd, P = _herm(rng, N), [_herm(rng, N, 0.5) for _ in range(m)], np.diag([0.0, 1.0]).astype(complex)
    sys_ = qc.QuantumSystem(H0, Hd)
    theta, scale = rng.uniform(-0.2, 0.2, (S, 1)), rng.uniform(0.9, 1.1, (S, m))
    goal = torch.from_numpy(np.ascontiguousarray(traj.goal["Ũ⃗"])).cuda()
    obj = qc.SweepFinalStateObjective(traj, sys_, [P], theta, lambda X: ((X - goal) ** 2).sum() / (2 * S), scale=scale)
    lin = qc.SweepFinalStateObjective(traj, sys_, [P], theta, lambda X: (X * goal).sum() + 3.0, scale=scale)
    Z = traj.datavec
    nZ = Z.size
    try:
        # J of every sample, (ns x Z_len), by the reference along the unit directions of the controls and timesteps
        G0, Gd, Gp = ref.iso_generator(H0), [ref.iso_generator(H) for H in Hd], [ref.iso_generator(P)]
        a0, dt0 = traj.offset("a"), traj.offset("Δt")
        K = Z[:T * traj.dim].reshape(T, traj.dim)
        controls, dts, init = K[:, a0:a0 + m].T.copy(), K[:, dt0].copy(), traj.initial["Ũ⃗"]
        J = np.zeros((S, init.size, nZ))
        for t in range(T - 1):
            for o in list(range(a0, a0 + m)) + [dt0]:
                va, vh = np.zeros((m, T)), np.zeros(T)
                if o == dt0:
                    vh[t] = 1.0
                else:
                    va[o - a0, t] = 1.0
                J[:, :, t * traj.dim + o] = jref.pushforward_frechet(G0, Gd, Gp, controls, dts, init, theta, scale, range(S), va, vh)["tfinals"]
        u, v = rng.standard_normal(nZ), rng.standard_normal(nZ)
        want = np.einsum("snz,sn->z", J, np.einsum("snz,z->sn", J, v)) / S
        got = obj.gauss_newton_times(Z, v)
        assert got.shape == (nZ,)
        err = np.abs(got - want).max() / max(1.0, np.abs(want).max())
        print(f"SWEEP-JVP gauss_newton_times vs J^T J v / S: {err:.3e} (bound 1e-9), max |value| {np.abs(want).max():.3f}")
        assert err <= 1e-9 and np.abs(want).max() > 1e-3
        gu = obj.gauss_newton_times(Z, u)
        assert abs(u @ got - v @ gu) <= 1e-9 * abs(u @ got)
        sw = obj._sweep
        tf = sw.jvp(Z, init, v, theta, scale)
        assert abs(v @ got - (tf ** 2).sum() / S) <= 1e-9 * abs(v @ got)
        # tensors in, a tensor out: the same bits
        dgot = obj.gauss_newton_times(torch.from_numpy(Z).cuda(), torch.from_numpy(v).cuda())
        assert torch.is_tensor(dgot) and dgot.is_cuda
        np.testing.assert_array_equal(dgot.cpu().numpy(), got)
        zero = lin.gauss_newton_times(Z, v)
        assert np.array_equal(zero, np.zeros(nZ))
        with pytest.raises(RuntimeError):
            obj.hess_L(Z)
        assert obj.hess_structure[0].size == 0
    finally:
        obj.close()
        lin.close()
    sys9 = qc.QuantumSystem(_herm(rng, 9), [_herm(rng, 9), _herm(rng, 9)])
    traj9 = tv._traj3(qc, rng, 9, m, T)
    wide = qc.SweepFinalStateObjective(traj9, sys9, [_herm(rng, 9)], theta, lambda X: (X ** 2).sum(), wide=True)
    try:
        with pytest.raises(qc.QCollocError) as e:
            wide.gauss_newton_times(traj9.datavec, np.ones(traj9.datavec.size))
        assert e.value.code == qc._lib.QC_ERR_UNSUPPORTED
        assert str(e.value).count("qc_sweep pushforward: ") == 1 and "not served in the mfma32-sweep form" in str(e.value)
    finally:
        wide.close()


@pytest.mark.gpu
def test_robust_gauss_newton_example(qc):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import robust_gauss_newton
    out = robust_gauss_newton.main(T=6, grid=3, steps=4, verbose=False)
    hist = out["loss_history"]
    print(f"SWEEP-JVP example: loss {hist[0]:.6e} -> {hist[-1]:.6e} in {out['accepted']} accepted steps, {out['gn_products']} Gauss-Newton products")
    assert out["kernel"] == "mfma16-sweep"
    assert len(hist) == out["accepted"] + 1 >= 2
    assert all(b <= a for a, b in zip(hist, hist[1:])) and hist[-1] < hist[0]
