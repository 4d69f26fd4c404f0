"""Sweep Hessian products (`qc_sweep_hvp*`, `RolloutSweep.hvp` / `hvp_device`, `SweepFinalStateObjective.hessian_times`): the tangent of
the sweep pullback along one direction, on closed "mfma16-sweep" handles.  CPU: the two routes of tests/sweep_hvp_reference.py against
each other, the symmetry of the reference, the device-free scope query, prototypes and mirrors.  GPU: every requested value against
the recurrence route, the linear part against the pullback, symmetry, bit-level properties, isolation of non-finite entries, refusals,
`hessian_times`, the example.

Tolerance (GPU against the reference).  The two reference routes agree to 1e-12 or better at every size used here (the CPU test holds
them to 1e-11).  The new walk is the products of the gradient walk and the pushforward differentiated once more, at a series whose
twice-differentiated truncation is 2e-14 (degree 10 at ||Y||_1 <= 1/8), so the project's tangent tolerance carries over (JVP_RTOL of
tests/test_sweep_jvp.py, argued in tests/test_sweep_grad.py): per sample |got - want| <= 1e-9 max(1, max |want_s|) for tgrad_samples and
tgrad_init, the same with the whole vector for tgrad.  Two quantities that are each within 1e-9 of the truth are compared at 2e-9."""
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest
import torch

import sweep_hvp_reference as href
import sweep_jvp_reference as jref
import sweep_reference as ref
import test_sweep as ts
import test_sweep_grad as tg
import test_sweep_jvp as tj
import test_sweep_wide as tw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HVP_RTOL = tj.JVP_RTOL
assert HVP_RTOL == 1e-9
_herm, _unitary = ts._herm, ts._unitary

# the closed cases of the pushforward's table, plus a launch whose items do not fill its last workgroup
HVP_CASES = {k: tj.JVP_CASES[k] for k in tj.CLOSED}
HVP_CASES["filled"] = ("unitary", 2, 2, 1, True, True, 37, 20, tj.U_ABS, None)       # 5 chunks of 4, 4, 4, 4, 3: 185 items
_REF = {}          # case name -> reference dict: computed once, shared, never written to


def build(qc, name):
    """test_sweep_wide.build, the direction of test_sweep_jvp.build (every part that exists non-zero), a cotangent and its direction."""
    c = tw.build(qc, name, HVP_CASES[name])
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
    c["cot"] = rng.standard_normal((S, ns)) / np.sqrt(ns)
    c["vcot"] = rng.standard_normal((S, ns)) / np.sqrt(ns)
    return c


def reference(c):
    if c["name"] not in _REF:
        out = href.hessian_product_frechet(c["G0"], c["Gd"], c["Gp"], c["controls"], c["dts"], c["init"], c["theta"], c["scale"], c["samples"], c["cot"],
                                           c["vcontrols"], c["vdts"], c["vinit"], c["vtheta"], c["vscale"], c["vcot"])
        for a in out.values():
            a.setflags(write=False)
        _REF[c["name"]] = out
    return _REF[c["name"]]


def scatter(lay, per_interval):
    """The plain sum over the leading axis of S x (T-1) x nd values, in ascending order, in the layout of the trajectory vector."""
    T, zdim, off_a, off_dt, m, Z_len = lay
    Z = np.zeros(Z_len)
    K = Z[:T * zdim].reshape(T, zdim)
    acc = np.zeros(per_interval.shape[1:])
    for s in range(per_interval.shape[0]):
        acc = acc + per_interval[s]
    K[:T - 1, off_a:off_a + m] = acc[:, :m]
    if off_dt >= 0:
        K[:T - 1, off_dt] = acc[:, m]
    return Z


def layout(sw):
    return (sw.T, sw.zdim, sw.off_a, sw.off_dt, sw.m, sw.Z_len)


# ---------------------------------------------------------------------------------------------------------------------------------
#  CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def _small(qc, N, state, free, tag):
    name = f"{tag}-{N}-{state}-{free}"
    c = tw.build(qc, name, (state, N, 2, 1, True, free, 2, 5, None, None))
    rng = np.random.default_rng(5 + sum(map(ord, name)))
    ns, T = c["init"].size, c["T"]
    args = (c["G0"], c["Gd"], c["Gp"], c["controls"], c["dts"], c["init"], c["theta"], c["scale"], [0, 1])
    kw = dict(vcontrols=rng.standard_normal((2, T)), vdts=0.1 * rng.standard_normal(T) if free else None, vinit=rng.standard_normal(ns) / np.sqrt(ns),
              vtheta=rng.standard_normal((2, 1)), vscale=rng.standard_normal((2, 2)), vcot=rng.standard_normal((2, ns)) / np.sqrt(ns))
    return c, rng, args, rng.standard_normal((2, ns)) / np.sqrt(ns), kw


@pytest.mark.parametrize("free", [True, False], ids=["free-dt", "fixed-dt"])
@pytest.mark.parametrize("state", ["unitary", "ket", "kets3"])
@pytest.mark.parametrize("N", [2, 3, 8])
def test_reference_routes_agree(qc, N, state, free):
    """The recurrences (expm_frechet and the 4n x 4n block exponential) against the complex step through the pullback: 1e-11 max(1, max |want|),
    with every direction non-zero."""
    c, _, args, cot, kw = _small(qc, N, state, free, "hvp-routes")
    a, b = href.hessian_product_frechet(*args, cot, **kw), href.hessian_product_complex_step(*args, cot, **kw)
    assert a["tgrad_samples"].shape == b["tgrad_samples"].shape == (2, 4, 3 if free else 2)
    assert a["tgrad_init"].shape == b["tgrad_init"].shape == (2, c["init"].size)
    for key in ("tgrad_samples", "tgrad_init"):
        err = np.abs(a[key] - b[key]).max() / max(1.0, np.abs(a[key]).max())
        print(f"SWEEP-HVP reference n={c['n']} {state} free={free} {key}: recurrences vs complex step {err:.2e}, max |value| {np.abs(a[key]).max():.3f}")
        assert err <= 1e-11 and np.abs(a[key]).max() > 1e-3, key


@pytest.mark.parametrize("N", [2, 3])
def test_reference_is_symmetric(qc, N):
    """With vcot = 0 the product is that of a symmetric matrix: <w, tgrad(v)> = <v, tgrad(w)> over the controls and timesteps."""
    c, rng, args, cot, _ = _small(qc, N, "unitary", True, "hvp-symmetry")
    T = c["T"]
    v, w = (dict(vcontrols=rng.standard_normal((2, T)), vdts=0.1 * rng.standard_normal(T)) for _ in range(2))
    pair = lambda tgs, d: float(np.sum(tgs[:, :, :2].sum(axis=0) * d["vcontrols"][:, :T - 1].T) + np.sum(tgs[:, :, 2].sum(axis=0) * d["vdts"][:T - 1]))
    lhs = pair(href.hessian_product_frechet(*args, cot, **v)["tgrad_samples"], w)
    rhs = pair(href.hessian_product_frechet(*args, cot, **w)["tgrad_samples"], v)
    print(f"SWEEP-HVP reference symmetry n={c['n']}: {lhs:.12e} vs {rhs:.12e}")
    assert abs(lhs - rhs) <= 1e-11 * max(1.0, abs(lhs)) and abs(lhs) > 1e-3


def _supported(qc, D):
    ok = C.c_int32(-1)
    rc = qc._lib.lib.qc_sweep_desc_hvp_supported(C.byref(D.d), C.byref(ok))
    return rc, ok.value, qc._lib.lib.qc_sweep_last_error(None).decode()


def test_hvp_scope_without_a_device(qc):
    L = qc._lib
    U = L.QC_FID_UNITARY
    served = {"closed": tg._GDesc(qc, N=2, m=2, fid_kind=U), "no fidelity": tg._GDesc(qc, N=4, m=2, cols=3), "8 drives, 16 columns": tg._GDesc(qc, N=8, m=8, cols=16),
              "ket": tg._GDesc(qc, N=4, m=2, cols=1, fid_kind=L.QC_FID_KET)}
    for what, D in served.items():
        assert _supported(qc, D)[:2] == (L.QC_OK, 1), what
    open2 = tg._GDesc(qc, N=4, m=2, cols=1, fid_kind=L.QC_FID_DENSITY)        # a Lindblad generator: n = 8, not antisymmetric
    open2.G0[:] = np.random.default_rng(0).standard_normal(64)
    wide12 = tg._GDesc(qc, N=12, m=2, fid_kind=U)
    wide12.d.wide = 1
    refused = {"Lindblad": (open2, "G_drift is not antisymmetric"),
               "N = 12, wide": (wide12, "not served in the mfma32-sweep form"),
               "N = 12": (tg._GDesc(qc, N=12, m=2, fid_kind=U), "rollout-per-sample form (2N = 24 > 16)"),
               "9 drives": (tg._GDesc(qc, N=2, m=9), "rollout-per-sample form (9 drives > 8)"),
               "17 columns": (tg._GDesc(qc, N=8, m=2, cols=17), "more than 16 columns")}
    for what, (D, word) in refused.items():
        rc, ok, msg = _supported(qc, D)
        assert (rc, ok) == (L.QC_OK, 0), what
        assert msg.startswith("qc_sweep Hessian product: ") and msg.count("qc_sweep Hessian product: ") == 1 and word in msg, (what, msg)
    # the pullback's reasons, word for word
    for D in (open2, refused["17 columns"][0], refused["9 drives"][0]):
        msg = _supported(qc, D)[2]
        ok = C.c_int32(-1)
        assert L.lib.qc_sweep_desc_vjp_supported(C.byref(D.d), C.byref(ok)) == L.QC_OK and ok.value == 0
        assert L.lib.qc_sweep_last_error(None).decode() == msg.replace("qc_sweep Hessian product: ", "qc_sweep pullback: ")
    assert _supported(qc, tg._GDesc(qc, T=1))[0] == L.QC_ERR_INVALID
    assert "T must be >= 2" in L.lib.qc_sweep_last_error(None).decode()
    assert L.lib.qc_sweep_desc_hvp_supported(C.byref(served["closed"].d), None) == L.QC_ERR_INVALID
    assert "qc_sweep_desc_hvp_supported" in L.lib.qc_sweep_last_error(None).decode()


def test_hvp_prototypes_header_and_mirrors(qc):
    L = qc._lib
    for name, nargs in (("qc_sweep_desc_hvp_supported", 2), ("qc_sweep_hvp", 15), ("qc_sweep_hvp_dev", 16)):
        assert name in L.SYMBOLS and len(L.SYMBOLS[name][1]) == nargs
        assert getattr(L.lib, name).argtypes is not None
    header = open(os.path.join(ROOT, "include", "qcolloc.h")).read()
    for decl in ("int qc_sweep_desc_hvp_supported(const qc_sweep_desc* d, int32_t* supported);", "int qc_sweep_hvp_dev(qc_sweep* h,",
                 "int qc_sweep_hvp(qc_sweep* h,", "const double* dcot, const double* dvZ, const double* dvinit, const double* dvtheta, const double* dvscale,",
                 "const double* dvcot, double* dtgrad, double* dtgrad_samples, double* dtgrad_init, void* stream);",
                 "const double* vcot, double* tgrad, double* tgrad_samples, double* tgrad_init);"):
        assert decl in header, decl
    assert header.index("int qc_sweep_jvp(qc_sweep* h,") < header.index("int qc_sweep_desc_hvp_supported(") < header.index("qc_debug_read_stamps")
    x = np.zeros(8)
    p = L.dptr(x)
    assert L.lib.qc_sweep_hvp(None, p, p, 1, p, None, p, p, None, None, None, None, p, None, None) == L.QC_ERR_INVALID
    assert L.lib.qc_sweep_last_error(None).decode() == "qc_sweep_hvp: NULL handle"
    assert L.lib.qc_sweep_hvp_dev(None, None, None, 1, None, None, None, None, None, None, None, None, None, None, None, None) == L.QC_ERR_INVALID
    assert L.lib.qc_sweep_last_error(None).decode() == "qc_sweep_hvp_dev: NULL handle"
    assert L.lib.qc_abi_version() == 6      # additive: the ABI stays 0.6
    julia = open(os.path.join(ROOT, "julia", "QCollocHIP.jl"), encoding="utf-8").read()
    assert "function rollout_sweep_hessian_product(" in julia and "(:qc_sweep_hvp, LIB[])" in julia and "(:qc_sweep_desc_hvp_supported, LIB[])" in julia
    for kw in ("vZ=nothing", "vinit=nothing", "vtheta=nothing", "vscale=nothing", "vcot=nothing"):
        assert kw in julia[julia.index("function rollout_sweep_hessian_product("):]
    for attr in ("hvp", "hvp_device", "hvp_supported", "hvp_unsupported_reason"):
        assert hasattr(qc.RolloutSweep, attr)
    assert list(inspect.signature(qc.RolloutSweep.hvp).parameters)[1:] == ["Z", "init", "cot", "theta", "scale", "vZ", "vinit", "vtheta", "vscale", "vcot",
                                                                           "per_sample", "init_grad"]
    assert list(inspect.signature(qc.RolloutSweep.hvp_device).parameters)[1:] == ["dZ", "dinit", "S", "dcot", "dtheta", "dscale", "dvZ", "dvinit", "dvtheta",
                                                                                  "dvscale", "dvcot", "dtgrad", "dtgrad_samples", "dtgrad_init", "stream"]
    assert hasattr(qc.SweepFinalStateObjective, "hessian_times") and hasattr(qc.SweepFinalStateObjective, "gauss_newton_times")


# ---------------------------------------------------------------------------------------------------------------------------------
#  GPU
# ---------------------------------------------------------------------------------------------------------------------------------
OUTPUTS = ("tgrad", "tgrad_samples", "tgrad_init")


def direction(sw, c):
    """The five directions in the handle's layouts (None where the handle has none)."""
    return dict(vZ=sw.pack(c["vcontrols"], c["vdts"]), vinit=c["vinit"], vtheta=c["vtheta"], vscale=c["vscale"], vcot=c["vcot"])


def outputs_of(sw):
    return [k for k in OUTPUTS if k != "tgrad_samples" or sw.n_deriv > 0]


def device_call(sw, Z, c, want, dirs, cot=None, stream=None):
    """One `hvp_device` call for the outputs named in `want` along `dirs`; numpy arrays back (buffers prefilled with -7)."""
    dev = torch.device("cuda:0")
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    S = c["S"]
    shapes = dict(tgrad=(sw.Z_len,), tgrad_samples=(S, sw.T - 1, sw.n_deriv), tgrad_init=(S, sw.ns))
    bufs = {k: torch.full(shapes[k], -7.0, dtype=torch.float64, device=dev) for k in want}
    torch.cuda.synchronize()
    sw.hvp_device(t(Z), t(c["init"]), S, t(c["cot"] if cot is None else cot), t(c["theta"]) if sw.p else None, t(c["scale"]),
                  **{"d" + k: t(v) for k, v in dirs.items()}, **{"d" + k: v for k, v in bufs.items()}, stream=stream)
    (stream.synchronize() if stream is not None else torch.cuda.synchronize())
    return {k: v.cpu().numpy() for k, v in bufs.items()}


def ratio(got, want):
    """max |got - want| / (1e-9 max(1, max |want|))"""
    return float(np.abs(got - want).max() / (HVP_RTOL * max(1.0, np.abs(want).max()))) if want.size else 0.0


def assert_samples(got, want, what):
    """Per sample: |got - want| <= 1e-9 max(1, max |want_s|)."""
    worst = max([ratio(got[q], want[q]) for q in range(want.shape[0])] + [0.0])
    print(f"SWEEP-HVP {what}: worst error / bound = {worst:.3e} (max |value| = {np.abs(want).max() if want.size else 0.0:.3e})")
    assert worst <= 1.0, what
    assert not np.isnan(got).any()


def control_mask(sw):
    K = np.zeros(sw.Z_len, dtype=bool)
    Kt = K[:sw.T * sw.zdim].reshape(sw.T, sw.zdim)
    Kt[:sw.T - 1, sw.off_a:sw.off_a + sw.m] = True
    if sw.off_dt >= 0:
        Kt[:sw.T - 1, sw.off_dt] = True
    return K


def check_case(sw, c):
    Z = sw.pack(c["controls"], c["dts"])
    samples, name = c["samples"], c["name"]
    want = outputs_of(sw)
    dirs = {k: v for k, v in direction(sw, c).items() if v is not None}
    out = device_call(sw, Z, c, want, dirs)
    r = reference(c)
    # values, per sample; nothing passes on zeros
    assert max(np.abs(a).max() for a in r.values() if a.size) > 1e-3
    if "tgrad_samples" in want:
        assert np.abs(r["tgrad_samples"]).max() > 1e-3
        assert_samples(out["tgrad_samples"][samples], r["tgrad_samples"], f"{name} tgrad_samples")
    assert np.abs(r["tgrad_init"]).max() > 1e-3
    assert_samples(out["tgrad_init"][samples], r["tgrad_init"], f"{name} tgrad_init")
    K = control_mask(sw)
    if "tgrad_samples" in want:
        # tgrad is the plain sum in ascending s of the per-sample values: the same additions, the same bits
        np.testing.assert_array_equal(out["tgrad"], scatter(layout(sw), out["tgrad_samples"]))
        if len(samples) == c["S"]:
            whole = scatter(layout(sw), r["tgrad_samples"])
            worst = ratio(out["tgrad"], whole)
            print(f"SWEEP-HVP {name} tgrad: worst error / bound = {worst:.3e} (max |value| = {np.abs(whole).max():.3e})")
            assert worst <= 1.0 and np.abs(whole).max() > 1e-3
    # every entry that is not a control or timestep of knots 0 .. T-2 is +0.0
    assert np.all(out["tgrad"][~K] == 0.0) and not np.signbit(out["tgrad"][~K]).any()
    # a second call; each output alone
    again = device_call(sw, Z, c, want, dirs)
    for k in want:
        np.testing.assert_array_equal(again[k], out[k], err_msg=k)
        np.testing.assert_array_equal(device_call(sw, Z, c, [k], dirs)[k], out[k], err_msg=k + " alone")
    # a NULL direction is an explicit zero array, one direction at a time
    for k in dirs:
        some = {q: v for q, v in dirs.items() if q != k}
        a = device_call(sw, Z, c, want, some)
        b = device_call(sw, Z, c, want, dict(some, **{k: np.zeros_like(dirs[k])}))
        for o in want:
            np.testing.assert_array_equal(a[o], b[o], err_msg=f"{o} without {k}")
    # the host-buffer entry point; the device entry point on a side stream
    host = sw.hvp(Z, c["init"], c["cot"], c["theta"], c["scale"], vZ=dirs.get("vZ"), vinit=dirs.get("vinit"), vtheta=dirs.get("vtheta"),
                  vscale=dirs.get("vscale"), vcot=dirs.get("vcot"), per_sample="tgrad_samples" in want, init_grad=True)
    np.testing.assert_array_equal(host[0], out["tgrad"])
    np.testing.assert_array_equal(host[-1], out["tgrad_init"])
    if "tgrad_samples" in want:
        np.testing.assert_array_equal(host[1], out["tgrad_samples"])
    side = torch.cuda.Stream(device=torch.device("cuda:0"))
    with torch.cuda.stream(side):
        other = device_call(sw, Z, c, want, dirs, stream=side)
    for k in want:
        np.testing.assert_array_equal(other[k], out[k], err_msg=k + " on a side stream")
    # only the controls and timesteps of knots 0 .. T-2 of vZ are read
    poisoned = dirs["vZ"].copy()
    poisoned[~K] = np.nan
    assert np.isnan(poisoned).sum() >= sw.zdim
    bad = device_call(sw, Z, c, want, dict(dirs, vZ=poisoned))
    for k in want:
        np.testing.assert_array_equal(bad[k], out[k], err_msg=k + " with NaNs in the unread entries of vZ")
    return out, dirs


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(HVP_CASES))
def test_hvp_matches_the_reference(qc, name):
    c = build(qc, name)
    sw = ts.make_sweep(qc, c)
    try:
        assert sw.kernel_name == "mfma16-sweep" and sw.hvp_supported and sw.hvp_unsupported_reason is None
        want = ts.sweep_launch(c["n"], c["m"], c["S"], c["T"])
        assert sw.launch(c["S"]) == (True, want["chunk"], want["n_chunks"])
        if name == "qubit":
            assert (want["chunk"], want["n_chunks"], want["last"]) == (3, 4, 1)
        if name in ("one-chunk", "one-interval"):
            assert want["n_chunks"] == 1
        if name == "long":
            assert (want["chunk"], want["n_chunks"], want["last"]) == (32, 32, 7)
        if name == "filled":
            assert (want["chunk"], want["n_chunks"], want["last"]) == (4, 5, 3) and (c["S"] * want["n_chunks"]) % 4 == 1
            assert c["samples"] == list(range(c["S"]))
        if name == "kets3":
            assert sw.fid_kind == -1
        if name == "squarings":
            th = c["theta"]
            sq = [ts._squarings(np.abs(c["dts"][t] * ref.sample_generator(c["G0"], c["Gd"], c["Gp"], c["controls"][:, t], th[s], np.ones(c["m"]))).sum(axis=0).max())
                  for s in range(c["S"]) for t in range(c["T"] - 1)]
            assert min(sq) == 0 and max(sq) >= 8, sq
        check_case(sw, c)
    finally:
        sw.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["qubit", "qutrit", "levels8-8drives", "kets3", "no-drives", "filled"])
def test_hvp_linear_part_is_the_pullback(qc, name):
    """With only vcot non-NULL the product is linear in it: tgrad_samples and tgrad_init are the pullback's grad_samples and grad_init with
    cot = vcot.  Both sides are within 1e-9 of the truth: 2e-9 max(1, max |.|)."""
    c = build(qc, name)
    sw = ts.make_sweep(qc, c)
    try:
        Z = sw.pack(c["controls"], c["dts"])
        want = outputs_of(sw)
        out = device_call(sw, Z, c, want, dict(vcot=c["vcot"]))
        pull = sw.vjp(Z, c["init"], c["vcot"], c["theta"], c["scale"], per_sample=True, init_grad=True)
        pairs = [("tgrad_init", pull[2])] + ([("tgrad_samples", pull[1]), ("tgrad", pull[0])] if "tgrad_samples" in want else [])
        for key, other in pairs:
            worst = ratio(out[key], other) / 2
            print(f"SWEEP-HVP {name} {key} along vcot alone vs qc_sweep_vjp: worst error / bound = {worst:.3e} (max |value| = {np.abs(other).max():.3e})")
            assert worst <= 1.0 and np.abs(other).max() > 1e-3, key
    finally:
        sw.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["qubit", "qutrit", "levels8-6drives", "ket", "squarings", "filled"])
def test_hvp_symmetry(qc, name):
    """With vcot = 0 the product is that of the symmetric matrix sum_s <cot_s, d2 x_s / dZ2>: <w, tgrad(v)> = <v, tgrad(w)> for two random
    directions over the trajectory vector.  Normalised as the adjoint identity of test_sweep_jvp.py: unit cotangents, and v, w of unit
    1-norm, so that each side is within 1e-9 max(1, max |tgrad|) of the truth: 2e-9 max(1, |<w, tgrad(v)>|, max |tgrad(v)|, max |tgrad(w)|)."""
    c = build(qc, name)
    sw = ts.make_sweep(qc, c)
    try:
        Z = sw.pack(c["controls"], c["dts"])
        rng = np.random.default_rng(3)
        cot = rng.standard_normal((c["S"], sw.ns))
        cot /= np.linalg.norm(cot, axis=1, keepdims=True)
        v, w = rng.standard_normal(sw.Z_len), rng.standard_normal(sw.Z_len)
        K = control_mask(sw)
        if name == "squarings":      # timestep directions in proportion to the timesteps, as in the value test
            dt_at = np.arange(sw.T) * sw.zdim + sw.off_dt
            v[dt_at] *= c["dts"]
            w[dt_at] *= c["dts"]
        v /= np.abs(v[K]).sum()
        w /= np.abs(w[K]).sum()
        tv = device_call(sw, Z, c, ["tgrad"], dict(vZ=v), cot=cot)["tgrad"]
        tw_ = device_call(sw, Z, c, ["tgrad"], dict(vZ=w), cot=cot)["tgrad"]
        lhs, rhs = float(w @ tv), float(v @ tw_)
        bound = 2 * HVP_RTOL * max(1.0, abs(lhs), np.abs(tv).max(), np.abs(tw_).max())
        print(f"SWEEP-HVP {name} symmetry: <w, tgrad(v)> = {lhs:.12e}, <v, tgrad(w)> = {rhs:.12e}, |difference| / bound = {abs(lhs - rhs) / bound:.3e}")
        assert abs(lhs - rhs) <= bound and abs(lhs) > 1e-3 * max(np.abs(tv).max(), 1e-3)
    finally:
        sw.close()


@pytest.mark.gpu
def test_hvp_isolation_of_non_finite_entries(qc):
    """A NaN in cot[1], vcot[1], vtheta[1] or vscale[1] reaches sample 1's outputs and tgrad, and leaves every other sample's bits as they
    were; a following evaluation on the handle is unaffected."""
    c = build(qc, "qutrit")
    sw = ts.make_sweep(qc, c)
    try:
        Z = sw.pack(c["controls"], c["dts"])
        dirs = direction(sw, c)
        want = outputs_of(sw)
        finals0, fids0 = sw.eval(Z, c["init"], c["theta"], c["scale"])
        clean = device_call(sw, Z, c, want, dirs)
        others = [s for s in range(c["S"]) if s != 1]
        for which in ("cot", "vcot", "vtheta", "vscale"):
            bad = (c["cot"] if which == "cot" else dirs[which]).copy()
            bad[1, 0] = np.nan
            out = device_call(sw, Z, c, want, dirs if which == "cot" else dict(dirs, **{which: bad}), cot=bad if which == "cot" else None)
            for k in ("tgrad_samples", "tgrad_init"):
                np.testing.assert_array_equal(out[k][others], clean[k][others], err_msg=f"{k} with a NaN in {which}[1]")
                assert np.isnan(out[k][1]).any(), (k, which)
            assert np.isnan(out["tgrad"]).any()
        after = device_call(sw, Z, c, want, dirs)
        for k in want:
            np.testing.assert_array_equal(after[k], clean[k], err_msg=k)
        finals1, fids1 = sw.eval(Z, c["init"], c["theta"], c["scale"])
        np.testing.assert_array_equal(finals1, finals0)
        np.testing.assert_array_equal(fids1, fids0)
    finally:
        sw.close()


def _raw(qc, sw, **null):
    """The host entry point called through ctypes with valid arrays everywhere but where `null` says None / a given array."""
    L = qc._lib
    S = 2
    a = dict(Z=np.zeros(sw.Z_len), init=np.zeros(sw.ns), theta=np.zeros((S, max(sw.p, 1))), scale=None, cot=np.zeros((S, sw.ns)), vZ=np.zeros(sw.Z_len),
             vinit=None, vtheta=None, vscale=None, vcot=None, tgrad=np.zeros(sw.Z_len), tgrad_samples=None, tgrad_init=None)
    S = null.pop("S", S)
    a.update(null)
    p = lambda k: None if a[k] is None else L.dptr(a[k])
    rc = L.lib.qc_sweep_hvp(sw._h, *(p(k) for k in ("Z", "init")), S, *(p(k) for k in ("theta", "scale", "cot", "vZ", "vinit", "vtheta", "vscale", "vcot",
                                                                                          "tgrad", "tgrad_samples", "tgrad_init")))
    return rc, L.lib.qc_sweep_last_error(sw._h).decode()


@pytest.mark.gpu
def test_hvp_refusals(qc):
    L = qc._lib
    INV, UNS = L.QC_ERR_INVALID, L.QC_ERR_UNSUPPORTED
    PRE = "qc_sweep Hessian product: "
    rng = np.random.default_rng(3)
    sys2 = qc.QuantumSystem(_herm(rng, 2), [_herm(rng, 2), _herm(rng, 2)])
    sw = qc.RolloutSweep(sys2, [qc.GATES["Z"]], 5)
    no_pert = qc.RolloutSweep(sys2, [], 5)
    no_drive = qc.RolloutSweep(qc.QuantumSystem(_herm(rng, 2), []), [qc.GATES["Z"]], 5, dt_fixed=0.2)
    cols17 = qc.RolloutSweep(sys2, [qc.GATES["Z"]], 5, cols=17)
    cw = tw.build(qc, "transmons9-S11-T50", tw.WIDE_CASES["transmons9-S11-T50"])
    wide = ts.make_sweep(qc, cw, wide=True)
    c9 = ts.build_case(qc, "qubit-9drives-S11-T50")
    nine = ts.make_sweep(qc, c9)
    co = tj.build(qc, "density")
    lindblad = ts.make_sweep(qc, co)
    try:
        assert _raw(qc, sw)[0] == L.QC_OK
        for kw, word in ((dict(Z=None), "qc_sweep_hvp: NULL input"), (dict(init=None), "qc_sweep_hvp: NULL input"),
                         (dict(vZ=None), "qc_sweep_hvp: every direction is NULL"), (dict(tgrad=None), "qc_sweep_hvp: every output is NULL"),
                         (dict(S=0), "qc_sweep_hvp: S must be in 1 .. 2^24"), (dict(S=(1 << 24) + 1), "qc_sweep_hvp: S must be in 1 .. 2^24"),
                         (dict(theta=None), "qc_sweep_hvp: theta is NULL but the handle has perturbations")):
            rc, msg = _raw(qc, sw, **kw)
            assert rc == INV and msg == word, (kw, rc, msg)
        rc, msg = _raw(qc, sw, cot=None)
        assert rc == INV and msg.startswith("qc_sweep_hvp: ") and "cot" in msg, msg
        rc, msg = _raw(qc, no_pert, vtheta=np.zeros((2, 1)))
        assert rc == INV and msg.startswith("qc_sweep_hvp: vtheta") and "n_pert = 0" in msg
        rc, msg = _raw(qc, no_drive, vscale=np.zeros((2, 1)))
        assert rc == INV and msg.startswith("qc_sweep_hvp: vscale") and "m = 0" in msg
        # vscale with scale = NULL is valid, and vcot alone is a direction
        assert _raw(qc, sw, vscale=np.ones((2, 2)))[0] == L.QC_OK
        assert _raw(qc, sw, vZ=None, vcot=np.ones((2, sw.ns)))[0] == L.QC_OK
        # the device entry point says the same under its own name
        dev = torch.device("cuda:0")
        z = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)
        rc = L.lib.qc_sweep_hvp_dev(sw._h, z(sw.Z_len).data_ptr(), z(sw.ns).data_ptr(), 2, z(2, 1).data_ptr(), None, z(2, sw.ns).data_ptr(), None, None, None,
                                    None, None, z(sw.Z_len).data_ptr(), None, None, None)
        assert rc == INV and L.lib.qc_sweep_last_error(sw._h).decode() == "qc_sweep_hvp_dev: every direction is NULL"
        with pytest.raises(ValueError):
            sw.hvp_device(z(sw.Z_len), z(sw.ns), 2, z(2, sw.ns), z(2, 1), dtgrad=z(sw.Z_len))
        with pytest.raises(ValueError):
            sw.hvp_device(z(sw.Z_len), z(sw.ns), 2, z(2, sw.ns), z(2, 1), dvZ=z(sw.Z_len))
        with pytest.raises(ValueError):
            sw.hvp_device(z(sw.Z_len), z(sw.ns), 2, None, z(2, 1), dvZ=z(sw.Z_len), dtgrad=z(sw.Z_len))
        with pytest.raises(ValueError):
            sw.hvp_device(z(sw.Z_len), z(sw.ns), 2, z(2, sw.ns), z(2, 1), dvZ=z(sw.Z_len + 1), dtgrad=z(sw.Z_len))
        # handles out of scope still serve eval
        for h, c, word in ((wide, cw, "not served in the mfma32-sweep form"), (nine, c9, "9 drives"), (lindblad, co, "is not antisymmetric"),
                           (cols17, None, "more than 16 columns")):
            why = h.hvp_unsupported_reason
            assert not h.hvp_supported and word in why and why.startswith(PRE) and why.count(PRE) == 1, why
            rc, msg = _raw(qc, h)
            assert rc == UNS and msg == why
            if c is None:
                continue
            Zc = h.pack(c["controls"], c["dts"])
            with pytest.raises(qc.QCollocError) as e:
                h.hvp(Zc, c["init"], np.zeros((c["S"], h.ns)), c["theta"], c["scale"], vZ=np.zeros(h.Z_len))
            assert e.value.code == UNS and word in str(e.value) and str(e.value).count(PRE) == 1
            finals, _ = h.eval(Zc, c["init"], c["theta"], c["scale"], fids=False)
            assert np.isfinite(finals).all()
        assert wide.kernel_name == "mfma32-sweep" and nine.kernel_name == "rollout-per-sample" and lindblad.jvp_supported
    finally:
        for h in (sw, no_pert, no_drive, cols17, wide, nine, lindblad):
            h.close()


@pytest.mark.gpu
def test_hessian_times(qc):
    """`hessian_times` on a qubit with l(X) = mean_s (1/2 ||X_s - G||^2 + 1/4 ||X_s||^4) against the reference built from the recurrence
    route and the pushforward reference, with the loss's derivatives in closed form; numpy and tensors; the difference to
    `gauss_newton_times` is the product with vcot = 0; a linear loss has a non-zero product where the Gauss-Newton one is exactly zero."""
    import test_sweep_vjp as tv
    rng = np.random.default_rng(43)
    N, m, T, S = 2, 2, 6, 3
    traj = tv._traj3(qc, rng, N, m, T)
    H0, Hd, P = _herm(rng, N), [_herm(rng, N, 0.5) for _ in range(m)], np.diag([0.0, 1.0]).astype(complex)
    sys_ = qc.QuantumSystem(H0, Hd)
    theta, scale = rng.uniform(-0.2, 0.2, (S, 1)), rng.uniform(0.9, 1.1, (S, m))
    Gnp = np.ascontiguousarray(traj.goal["Ũ⃗"])
    goal = torch.from_numpy(Gnp).cuda()
    loss = lambda X: (0.5 * ((X - goal) ** 2).sum(dim=1) + 0.25 * (X ** 2).sum(dim=1) ** 2).mean()
    obj = qc.SweepFinalStateObjective(traj, sys_, [P], theta, loss, scale=scale)
    lin = qc.SweepFinalStateObjective(traj, sys_, [P], theta, lambda X: (X * goal).sum() + 3.0, scale=scale)
    Z = traj.datavec
    nZ = Z.size
    try:
        G0, Gd, Gp = ref.iso_generator(H0), [ref.iso_generator(H) for H in Hd], [ref.iso_generator(P)]
        a0, dt0 = traj.offset("a"), traj.offset("Δt")
        lay = (T, traj.dim, a0, dt0, m, nZ)
        K = Z[:T * traj.dim].reshape(T, traj.dim)
        controls, dts, init = K[:, a0:a0 + m].T.copy(), K[:, dt0].copy(), traj.initial["Ũ⃗"]
        v = rng.standard_normal(nZ)
        V = v[:T * traj.dim].reshape(T, traj.dim)
        va, vh = V[:, a0:a0 + m].T.copy(), V[:, dt0].copy()
        args = (G0, Gd, Gp, controls, dts, init, theta, scale, range(S))
        push = jref.pushforward_frechet(*args, va, vh)
        grad, hess_times = href.pullback_loss_terms(push["finals"], Gnp)
        vcot = hess_times(push["tfinals"])
        want = scatter(lay, href.hessian_product_frechet(*args, grad, va, vh, vcot=vcot)["tgrad_samples"])
        got = obj.hessian_times(Z, v)
        assert isinstance(got, np.ndarray) and got.shape == (nZ,)
        worst = ratio(got, want)
        print(f"SWEEP-HVP hessian_times vs the reference: worst error / bound = {worst:.3e} (max |value| = {np.abs(want).max():.3e})")
        assert worst <= 1.0 and np.abs(want).max() > 1e-3
        # tensors in, a device tensor out.  Not compared bit for bit: vcot is torch's double backward through the loss, whose last bits
        # differ between the first evaluation of a graph in a process and the later ones (the library's part is bit-stable: test_hvp_matches_the_reference)
        dgot = obj.hessian_times(torch.from_numpy(Z).cuda(), torch.from_numpy(v).cuda())
        assert torch.is_tensor(dgot) and dgot.is_cuda and dgot.dtype == torch.float64 and dgot.shape == (nZ,)
        assert ratio(dgot.cpu().numpy(), want) <= 1.0 and ratio(dgot.cpu().numpy(), got) <= 1e-3
        # exact = Gauss-Newton + the curvature of the sweep map
        sw = obj._sweep
        curv = sw.hvp(Z, init, grad, theta, scale, vZ=v)[0]
        gn = obj.gauss_newton_times(Z, v)
        worst = ratio(got - gn, curv) / 2
        print(f"SWEEP-HVP hessian_times - gauss_newton_times vs hvp(vcot = 0): worst error / bound = {worst:.3e} (max |value| = {np.abs(curv).max():.3e})")
        assert worst <= 1.0 and np.abs(curv).max() > 1e-3
        # symmetric
        u = rng.standard_normal(nZ)
        gu = obj.hessian_times(Z, u)
        Km = np.zeros(nZ, dtype=bool)
        Km[:T * traj.dim].reshape(T, traj.dim)[:T - 1, list(range(a0, a0 + m)) + [dt0]] = True
        lhs, rhs = float(u @ got), float(v @ gu)
        assert abs(lhs - rhs) <= 2 * HVP_RTOL * max(1.0, np.abs(got).max() * np.abs(u[Km]).sum(), np.abs(gu).max() * np.abs(v[Km]).sum())
        # a linear loss: the Gauss-Newton product is exactly zero, the exact product is the whole Hessian
        assert np.array_equal(lin.gauss_newton_times(Z, v), np.zeros(nZ))
        got_lin = lin.hessian_times(Z, v)
        want_lin = scatter(lay, href.hessian_product_frechet(*args, np.tile(Gnp, (S, 1)), va, vh)["tgrad_samples"])
        worst = ratio(got_lin, want_lin)
        print(f"SWEEP-HVP hessian_times of a linear loss: worst error / bound = {worst:.3e} (max |value| = {np.abs(want_lin).max():.3e})")
        assert worst <= 1.0 and np.abs(want_lin).max() > 1e-3 and np.abs(got_lin).max() > 1e-3
        with pytest.raises(RuntimeError):
            obj.hess_L(Z)
        assert obj.hess_structure[0].size == 0
    finally:
        obj.close()
        lin.close()
    sys9 = qc.QuantumSystem(_herm(rng, 9), [_herm(rng, 9), _herm(rng, 9)])
    traj9 = tv._traj3(qc, rng, 9, m, 4)
    wide = qc.SweepFinalStateObjective(traj9, sys9, [_herm(rng, 9)], theta, lambda X: (X ** 2).sum(), wide=True)
    try:
        with pytest.raises(qc.QCollocError) as e:
            wide.hessian_times(traj9.datavec, np.ones(traj9.datavec.size))
        assert e.value.code == qc._lib.QC_ERR_UNSUPPORTED
        assert str(e.value).count("qc_sweep Hessian product: ") == 1 and "not served in the mfma32-sweep form" in str(e.value)
    finally:
        wide.close()


@pytest.mark.gpu
def test_robust_newton_cg_example(qc):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import robust_newton_cg
    out = robust_newton_cg.main(T=6, grid=3, steps=4, verbose=False)
    hist = out["loss_history"]
    print(f"SWEEP-HVP example: loss {hist[0]:.6e} -> {hist[-1]:.6e} in {out['accepted']} accepted steps, {out['exact_products']} exact Hessian products, "
          f"{out['gn_products']} Gauss-Newton products")
    print("SWEEP-HVP example: " + out["summary"])
    assert out["kernel"] == "mfma16-sweep" and out["T"] <= 20 and out["S"] <= 8
    assert out["exact_products"] > 0 and "exact Hessian products" in out["summary"]
    assert len(hist) == out["accepted"] + 1 >= 2
    assert all(b <= a for a, b in zip(hist, hist[1:])) and hist[-1] < hist[0]
