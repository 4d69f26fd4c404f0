"""Wide sweep Hessian products (`qc_sweep_desc.wide` bit 8, QC_SWEEP_WIDE_HESSIAN; `RolloutSweep(..., wide=True, wide_hessian=True)`):
`qc_sweep_hvp*` on "mfma32-sweep" handles (csrc/qc_sweep32_hvp.hip, the ld = 32 seed kernel of csrc/qc_sweep_hvp.hip).  CPU: the valid
values of `wide`, the device-free scope query, the launch query, constants, Python keywords, the Julia text, the two reference routes of
tests/sweep_hvp_reference.py against each other at wide sizes.  GPU: every requested value against the recurrence route and the
bit-level properties of tests/test_sweep_hvp.py (its `check_case`, unchanged), the linear part against the wide pullback, symmetry, the
bits of handles made with further bits and of the other entry points, isolation of non-finite entries, refusals, `hessian_times`, the
example.

Tolerance (GPU against the reference): that of tests/test_sweep_hvp.py, HVP_RTOL = 1e-9 -- per sample
|got - want| <= 1e-9 max(1, max |want_s|) for tgrad_samples and tgrad_init, the same with the whole vector for tgrad.  The walk is the
narrow one on 2 x 2 tiles with the same degree-10 series (twice-differentiated truncation 2e-14 at ||Y||_1 <= 1/8); its inner products
have 32 terms where the narrow ones have 16, which moves rounding by a factor of two at 1e-16, far below the bound.  Two quantities that
are each within 1e-9 of the truth are compared at 2e-9.  The helpers are those of the existing files, imported, not copied; the direction,
the cotangent and their draws follow test_sweep_hvp.build.  Every sample of mid-size and filled launches:
tests/test_sweep_wide_hvp_every_sample.py."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

import sweep_hvp_reference as href
import sweep_reference as ref
import test_sweep as ts
import test_sweep_hvp as thv
import test_sweep_open_grad as too
import test_sweep_vjp as tv
import test_sweep_wide as tw
import test_sweep_wide_jvp as twj
import test_sweep_wide_open_grad as two

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HVP_RTOL = thv.HVP_RTOL
_herm = ts._herm
HESSIAN = 256
PRE = "qc_sweep Hessian product: "
OLD = PRE + "Hessian products are not served in the mfma32-sweep form"

# the closed rows of the wide pushforward's table
CASES = ["n9-S5-T11", "n10-S3-T10", "n16-m8", "n16-no-perturbations", "n12-no-drives", "n10-kets3", "n12-ket", "squarings", "one-interval",
         "one-chunk", "long"]
SPECS = {k: twj.SPECS[k] for k in CASES}


def build(qc, name):
    """test_sweep_wide.build under the name wide-hvp/<name>, then the draws of test_sweep_hvp.build: a direction with every part that exists
    non-zero, a cotangent and its direction."""
    c = tw.build(qc, "wide-hvp/" + name, SPECS[name])
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


def handle(qc, c, **kw):
    return ts.make_sweep(qc, c, wide=True, wide_hessian=True, **kw)


# ---------------------------------------------------------------------------------------------------------------------------------
#  CPU
# ---------------------------------------------------------------------------------------------------------------------------------
ODD = (1, 3, 9, 11, 17, 19, 25, 27)


def test_wide_values_with_the_hessian_bit(qc):
    L = qc._lib
    val = lambda D: L.lib.qc_sweep_desc_validate(C.byref(D.d))
    assert L.QC_SWEEP_WIDE_HESSIAN == HESSIAN
    for N in (12, 16, 2):
        assert val(tw._wdesc(qc, 257, N=N)) == L.QC_OK, N              # refused before the bit existed
        assert val(tw._wdesc(qc, 256 | 27 | 64, N=N)) == L.QC_OK, N
        for odd in ODD:
            for good in (odd, odd | 64, odd | 256, odd | 64 | 256):
                assert val(tw._wdesc(qc, good, N=N)) == L.QC_OK, (N, good)
        assert val(tw._wdesc(qc, 0, N=N)) == L.QC_OK
        for bad in (256, 258, 128 | 1, 33, 5, 512 | 1, 256 | 2, 256 | 64, 256 | 4 | 1, 256 | 128 | 1, (1 << 20) | 257, -1):
            assert val(tw._wdesc(qc, bad, N=N)) == L.QC_ERR_INVALID, (N, bad)
            msg = L.lib.qc_sweep_last_error(None).decode()
            assert msg.startswith("qc_sweep: wide"), msg
            for word in ("17, 19, 25 or 27", "QC_SWEEP_WIDE_TANGENT (16)", "QC_SWEEP_WIDE_NOISE (64)", "QC_SWEEP_WIDE_HESSIAN (256)"):
                assert word in msg, (N, bad, word, msg)


def _lindblad_desc(qc, wide, N=16, **kw):
    D = too._ODesc(qc, wide=wide, **{**dict(N=N, m=2, cols=1, fid_kind=qc._lib.QC_FID_DENSITY), **kw})
    D.G0[:] = np.random.default_rng(0).standard_normal(D.G0.size)       # not antisymmetric
    return D


def test_hvp_scope_follows_the_bit(qc):
    L = qc._lib
    U = L.QC_FID_UNITARY
    q = lambda D: too._query(qc, "qc_sweep_desc_hvp_supported", D)
    for N in (9, 12, 16):
        assert q(tw._wdesc(qc, 257, N=N, fid_kind=U))[:2] == (L.QC_OK, 1), N            # zero matrices: antisymmetric
        assert q(tw._wdesc(qc, 257, N=N, cols=3))[:2] == (L.QC_OK, 1), N                # no fidelity
        assert q(tw._wdesc(qc, 257, N=N, cols=16))[:2] == (L.QC_OK, 1), N
        assert q(tw._wdesc(qc, 257, N=N, m=8, fid_kind=U))[:2] == (L.QC_OK, 1), N
        for other in (2, 8, 16, 64, 2 | 8 | 16 | 64):
            assert q(tw._wdesc(qc, 257 | other, N=N, fid_kind=U))[:2] == (L.QC_OK, 1), (N, other)
    # without the bit: the old message, verbatim
    for wide in (1, 3, 17, 27, 65):
        for N in (9, 12, 16):
            assert q(tw._wdesc(qc, wide, N=N, fid_kind=U)) == (L.QC_OK, 0, OLD), (wide, N)
    # the order of the reasons: the closed scope first, then the form
    for wide in (257, 1):
        rc, ok, msg = q(_lindblad_desc(qc, wide))
        assert (rc, ok) == (L.QC_OK, 0) and msg.startswith(PRE) and "is not antisymmetric" in msg and "mfma32-sweep form" not in msg, (wide, msg)
    assert q(_lindblad_desc(qc, 257)) == q(_lindblad_desc(qc, 1))
    rc, ok, msg = q(tw._wdesc(qc, 257, N=12, cols=17))
    assert (rc, ok) == (L.QC_OK, 0) and "more than 16 columns" in msg
    rc, ok, msg = q(tw._wdesc(qc, 257, N=12, m=9, fid_kind=U))
    assert (rc, ok) == (L.QC_OK, 0) and msg == PRE + "the handle takes the rollout-per-sample form (9 drives > 8)"
    rc, ok, msg = q(tw._wdesc(qc, 257, N=17, fid_kind=U))
    assert (rc, ok) == (L.QC_OK, 0) and msg == PRE + "the handle takes the rollout-per-sample form (2N = 34 > 32)"
    for N in (2, 8):                                                                     # the narrow form does not look at the bit
        for D in (lambda w: tw._wdesc(qc, w, N=N, fid_kind=U), lambda w: _lindblad_desc(qc, w, N=4), lambda w: tw._wdesc(qc, w, N=N, cols=17)):
            assert q(D(257)) == q(D(1)) == q(D(0)), N
        assert q(tw._wdesc(qc, 257, N=N, fid_kind=U))[:2] == (L.QC_OK, 1)
    assert q(tw._wdesc(qc, 256, N=12))[0] == L.QC_ERR_INVALID
    # every other scope answers what it answered without the bit
    for fn in ("qc_sweep_desc_grad_supported", "qc_sweep_desc_vjp_supported", "qc_sweep_desc_jvp_supported", "qc_sweep_desc_noise_supported"):
        for base in ODD + (65, 91):
            for D in (lambda w: tw._wdesc(qc, w, N=12, fid_kind=U), lambda w: _lindblad_desc(qc, w), lambda w: _lindblad_desc(qc, w, flag=1)):
                assert too._query(qc, fn, D(base)) == too._query(qc, fn, D(base | HESSIAN)), (fn, base)


def test_launch_query_does_not_see_the_hessian_bit(qc):
    L = qc._lib
    for n in (16, 18, 24, 32, 34):
        for m in (1, 8, 9):
            for S, T in ((1, 2), (2, 102), (5, 12), (11, 50), (2047, 50), (2048, 3), (8192, 1000)):
                got = []
                for wide in (1, 257, 257 | 16, 257 | 2 | 8 | 16 | 64):
                    D = tw._wdesc(qc, wide, N=n // 2, m=m, T=T, cols=1)
                    mf, ch, nch = C.c_int32(), C.c_int64(), C.c_int64()
                    assert L.lib.qc_sweep_desc_launch(C.byref(D.d), S, C.byref(mf), C.byref(ch), C.byref(nch)) == L.QC_OK
                    got.append((bool(mf.value), ch.value, nch.value))
                want = tw.wide_launch(n, m, S, T)
                assert set(got) == {(want["mfma"], want["chunk"], want["n_chunks"])}, (n, m, S, T)
    for name in CASES:
        if name in twj.ITEMS:
            _, L_, m, _, _, _, S, T, _, _ = SPECS[name]
            w = tw.wide_launch(2 * L_, m, S, T)
            assert (w["chunk"], w["n_chunks"], w["last"], S * w["n_chunks"]) == twj.ITEMS[name], name
    assert twj.ITEMS["n10-S3-T10"][3] % 2 == 1      # whichever the waves per workgroup, 2 or 4: the last workgroup is not full


def test_constants_keywords_and_texts(qc):
    L = qc._lib
    assert (L.QC_SWEEP_WIDE, L.QC_SWEEP_WIDE_PARAMS, L.QC_SWEEP_WIDE_STORED, L.QC_SWEEP_WIDE_TANGENT, L.QC_SWEEP_WIDE_NOISE, L.QC_SWEEP_WIDE_HESSIAN) == (1, 2, 8, 16, 64, 256)
    header = open(os.path.join(ROOT, "include", "qcolloc.h")).read()
    assert re.search(r"^#define QC_SWEEP_WIDE_HESSIAN 256\b", header, re.M)
    assert L.lib.qc_abi_version() == 6 and L.lib.qc_sizeof_sweep_desc() == 128      # additive: the ABI stays 0.6
    for name, nargs in (("qc_sweep_desc_hvp_supported", 2), ("qc_sweep_hvp", 15), ("qc_sweep_hvp_dev", 16)):
        assert name in L.SYMBOLS and len(L.SYMBOLS[name][1]) == nargs
    assert not any("sweep32" in name for name in L.SYMBOLS)                          # no new exported symbol
    for f in (qc.RolloutSweep.__init__, qc.SweepFinalStateObjective.__init__):
        par = inspect.signature(f).parameters
        assert "wide_hessian" in par and par["wide_hessian"].default is False, f
    rng = np.random.default_rng(0)
    sys9 = qc.QuantumSystem(_herm(rng, 9), [_herm(rng, 9)])
    for kw in (dict(), dict(wide_tangent=False), dict(stored_states=True)):        # before the library is touched: no device is needed to be told so
        with pytest.raises(ValueError, match="wide_hessian=True needs wide=True"):
            qc.RolloutSweep(sys9, [], 5, wide_hessian=True, **kw)
    assert "wide_hessian" in qc.RolloutSweep.__doc__ and "wide_hessian" in qc.RolloutSweep.hvp_supported.__doc__
    assert "wide_hessian" in qc.SweepFinalStateObjective.hessian_times.__doc__ and "wide_tangent" in qc.SweepFinalStateObjective.hessian_times.__doc__
    julia = open(os.path.join(ROOT, "julia", "QCollocHIP.jl"), encoding="utf-8").read()
    assert re.search(r"^const QC_SWEEP_WIDE_HESSIAN = 256\b", julia, re.M)
    fn = julia[julia.index("function rollout_sweep_hessian_product("):]
    fn = fn[:fn.index("\nend\n")]
    assert "wide::Bool=false" in fn and "wide ? (QC_SWEEP_WIDE | QC_SWEEP_WIDE_HESSIAN) : 0" in fn
    makefile = open(os.path.join(ROOT, "quantumcollocation.jl_amd", "csrc", "Makefile")).read()
    assert "qc_sweep32_hvp.hip" in makefile and "qc_sweep32_hvp.o" in makefile
    design = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    assert "5.8.10" in design and "3120 + 288" in design
    assert "qc_sweep32_hvp.hip" in open(os.path.join(ROOT, "README.md"), encoding="utf-8").read()


@pytest.mark.parametrize("free", [True, False], ids=["free-dt", "fixed-dt"])
@pytest.mark.parametrize("state", ["unitary", "ket", "kets3"])
@pytest.mark.parametrize("N", [9, 12, 16])
def test_reference_routes_agree_at_wide_sizes(qc, N, state, free):
    """The recurrences (expm_frechet and the 4n x 4n block exponential) against the complex step through the pullback at 2N = 18, 24, 32,
    S = 2, T = 4, every direction non-zero: 1e-11 max(1, max |want|), and values that a zero could not pass for."""
    name = f"wide-hvp-routes-{N}-{state}-{free}"
    S, T, m, p = 2, 4, 2, 1
    c = tw.build(qc, name, (state, N, m, p, True, free, S, T, None, None))
    rng = np.random.default_rng(5 + sum(map(ord, name)))
    ns = c["init"].size
    args = (c["G0"], c["Gd"], c["Gp"], c["controls"], c["dts"], c["init"], c["theta"], c["scale"], [0, 1])
    kw = dict(vcontrols=rng.standard_normal((m, T)), vdts=0.1 * rng.standard_normal(T) if free else None, vinit=rng.standard_normal(ns) / np.sqrt(ns),
              vtheta=rng.standard_normal((S, p)), vscale=rng.standard_normal((S, m)), vcot=rng.standard_normal((S, ns)) / np.sqrt(ns))
    cot = rng.standard_normal((S, ns)) / np.sqrt(ns)
    a, b = href.hessian_product_frechet(*args, cot, **kw), href.hessian_product_complex_step(*args, cot, **kw)
    assert a["tgrad_samples"].shape == b["tgrad_samples"].shape == (S, T - 1, m + 1 if free else m)
    assert a["tgrad_init"].shape == b["tgrad_init"].shape == (S, ns)
    for key in ("tgrad_samples", "tgrad_init"):
        err = np.abs(a[key] - b[key]).max() / max(1.0, np.abs(a[key]).max())
        print(f"SWEEP-WIDE-HVP reference n={c['n']} {state} free={free} {key}: recurrences vs complex step {err:.2e}, max |value| {np.abs(a[key]).max():.3f}")
        assert err <= 1e-11 and np.abs(a[key]).max() > 1e-3, key


# ---------------------------------------------------------------------------------------------------------------------------------
#  GPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_wide_hvp_matches_the_reference(qc, name):
    """Every requested value against the recurrence route along the full direction, and the bit-level properties of
    test_sweep_hvp.check_case: tgrad is the plain sum of tgrad_samples, +0.0 outside the controls and timesteps, a second call, each output
    alone, a NULL direction against zeros, the host entry point, a side stream, NaNs in the unread entries of vZ."""
    c = build(qc, name)
    sw = handle(qc, c)
    try:
        assert sw.kernel_name == "mfma32-sweep" and sw.wide_hessian and sw._desc.wide == 257
        assert sw.hvp_supported and sw.hvp_unsupported_reason is None and not sw.jvp_supported      # the product does not need the tangent bit
        want = tw.wide_launch(c["n"], c["m"], c["S"], c["T"])
        assert sw.launch(c["S"]) == (True, want["chunk"], want["n_chunks"])
        if name in twj.ITEMS:
            assert (want["chunk"], want["n_chunks"], want["last"], c["S"] * want["n_chunks"]) == twj.ITEMS[name]
        if name == "squarings":
            sq = [ts._squarings(np.abs(c["dts"][t] * ref.sample_generator(c["G0"], c["Gd"], c["Gp"], c["controls"][:, t], c["theta"][s], np.ones(c["m"]))).sum(axis=0).max())
                  for s in range(c["S"]) for t in range(c["T"] - 1)]
            assert min(sq) == 0 and max(sq) >= 10, sq
        if name == "n12-no-drives":
            assert sw.n_deriv == 0 and thv.outputs_of(sw) == ["tgrad", "tgrad_init"]
        out, _ = thv.check_case(sw, c)
        if name == "n12-no-drives":      # nd = 0: the walk is skipped, tgrad_init is served, tgrad is +0.0 everywhere
            assert np.all(out["tgrad"] == 0.0) and not np.signbit(out["tgrad"]).any()
    finally:
        sw.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n9-S5-T11", "n16-m8", "n12-no-drives", "n10-kets3", "n12-ket"])
def test_linear_part_is_the_wide_pullback(qc, name):
    """With only vcot given, tgrad, tgrad_samples and tgrad_init are the wide pullback's grad, grad_samples and grad_init with cot = vcot on
    the same handle.  Both sides are within 1e-9 of the truth: 2e-9 max(1, max |.|)."""
    c = build(qc, name)
    sw = handle(qc, c)
    try:
        Z = sw.pack(c["controls"], c["dts"])
        want = thv.outputs_of(sw)
        out = thv.device_call(sw, Z, c, want, dict(vcot=c["vcot"]))
        pull = sw.vjp(Z, c["init"], c["vcot"], c["theta"], c["scale"], per_sample=True, init_grad=True)
        pairs = [("tgrad_init", pull[2])] + ([("tgrad_samples", pull[1]), ("tgrad", pull[0])] if "tgrad_samples" in want else [])
        for key, other in pairs:
            worst = thv.ratio(out[key], other) / 2
            print(f"SWEEP-WIDE-HVP {name} {key} along vcot alone vs qc_sweep_vjp: worst error / bound = {worst:.3e} (max |value| = {np.abs(other).max():.3e})")
            assert worst <= 1.0 and np.abs(other).max() > 1e-3, key
    finally:
        sw.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n9-S5-T11", "n16-m8"])
def test_symmetry(qc, name):
    """With vcot = 0 the product is that of the symmetric matrix sum_s <cot_s, d2 x_s / dZ2>: <w, tgrad(v)> = <v, tgrad(w)> for two random
    directions over the trajectory vector, at 1e-9 relative, both sides above 1e-3."""
    c = build(qc, name)
    sw = handle(qc, c)
    try:
        Z = sw.pack(c["controls"], c["dts"])
        rng = np.random.default_rng(3)
        cot = rng.standard_normal((c["S"], sw.ns))
        cot /= np.linalg.norm(cot, axis=1, keepdims=True)
        v, w = rng.standard_normal(sw.Z_len), rng.standard_normal(sw.Z_len)
        tv_ = thv.device_call(sw, Z, c, ["tgrad"], dict(vZ=v), cot=cot)["tgrad"]
        tw_ = thv.device_call(sw, Z, c, ["tgrad"], dict(vZ=w), cot=cot)["tgrad"]
        lhs, rhs = float(w @ tv_), float(v @ tw_)
        rel = abs(lhs - rhs) / max(abs(lhs), abs(rhs))
        print(f"SWEEP-WIDE-HVP {name} symmetry: <w, tgrad(v)> = {lhs:.12e}, <v, tgrad(w)> = {rhs:.12e}, relative difference {rel:.3e} (bound 1e-9)")
        assert min(abs(lhs), abs(rhs)) > 1e-3
        assert rel <= 1e-9
    finally:
        sw.close()


def _reverse_outputs(sw, Z, c):
    """eval, grad and vjp (every output) of one handle, as a flat list of arrays."""
    out = list(sw.eval(Z, c["init"], c["theta"], c["scale"], fids=c["kind"] is not None))
    if c["kind"] is not None:
        out += list(sw.grad(Z, c["init"], c["theta"], c["scale"]))
    out += list(sw.vjp(Z, c["init"], c["cot"], c["theta"], c["scale"], per_sample=True, init_grad=True))
    return [np.asarray(a) for a in out if a is not None]


@pytest.mark.gpu
def test_bits_do_not_depend_on_the_other_bits_or_on_shared_scratch(qc):
    """A handle with 257 | every other bit gives the product's bits of 257 (also with reserved1[0] = 1: the product keeps the closed walk);
    eval, grad and vjp of a 257 handle are those of a wide = 1 handle, before and after a Hessian-product call on the shared scratch."""
    c = build(qc, "n9-S5-T11")
    sw = handle(qc, c)
    full = handle(qc, c, wide_params=True, wide_tangent=True, wide_noise=True)
    stored = handle(qc, c, wide_params=True, wide_tangent=True, wide_noise=True, stored_states=True, wide_stored=True)
    plain = ts.make_sweep(qc, c, wide=True)
    try:
        assert (sw._desc.wide, full._desc.wide, stored._desc.wide, plain._desc.wide) == (257, 257 | 2 | 16 | 64, 257 | 2 | 8 | 16 | 64, 1)
        assert stored._desc.reserved1[0] == 1 and stored.hvp_supported
        assert sw.kernel_name == full.kernel_name == stored.kernel_name == plain.kernel_name == "mfma32-sweep"
        assert sw.launch(c["S"]) == full.launch(c["S"]) == plain.launch(c["S"])
        Z = sw.pack(c["controls"], c["dts"])
        dirs = {k: v for k, v in thv.direction(sw, c).items() if v is not None}
        before = _reverse_outputs(sw, Z, c)
        for a, b in zip(before, _reverse_outputs(plain, Z, c)):
            np.testing.assert_array_equal(a, b)
        out = thv.device_call(sw, Z, c, thv.OUTPUTS, dirs)
        assert np.abs(out["tgrad"]).max() > 1e-3
        for other in (full, stored):
            got = thv.device_call(other, Z, c, thv.OUTPUTS, dirs)
            for k in thv.OUTPUTS:
                np.testing.assert_array_equal(got[k], out[k], err_msg=f"{k} with wide = {other._desc.wide}")
        after = _reverse_outputs(sw, Z, c)
        assert len(after) == len(before) >= 6
        for a, b in zip(after, before):
            np.testing.assert_array_equal(a, b)
        # and the product after them
        again = thv.device_call(sw, Z, c, thv.OUTPUTS, dirs)
        for k in thv.OUTPUTS:
            np.testing.assert_array_equal(again[k], out[k], err_msg=k)
    finally:
        for h in (sw, full, stored, plain):
            h.close()


@pytest.mark.gpu
def test_isolation_of_non_finite_entries(qc):
    """A NaN in cot[1], vcot[1], vtheta[1] or vscale[1] reaches sample 1's outputs and tgrad, and leaves every other sample's
    tgrad_samples and tgrad_init bit-equal to the clean call; a following call on the handle is unaffected."""
    c = build(qc, "n9-S5-T11")
    sw = handle(qc, c)
    try:
        Z = sw.pack(c["controls"], c["dts"])
        dirs = thv.direction(sw, c)
        want = thv.outputs_of(sw)
        clean = thv.device_call(sw, Z, c, want, dirs)
        others = [s for s in range(c["S"]) if s != 1]
        for which in ("cot", "vcot", "vtheta", "vscale"):
            bad = (c["cot"] if which == "cot" else dirs[which]).copy()
            bad[1, 0] = np.nan
            out = thv.device_call(sw, Z, c, want, dirs if which == "cot" else dict(dirs, **{which: bad}), cot=bad if which == "cot" else None)
            for k in ("tgrad_samples", "tgrad_init"):
                np.testing.assert_array_equal(out[k][others], clean[k][others], err_msg=f"{k} with a NaN in {which}[1]")
                assert np.isnan(out[k][1]).any(), (k, which)
            assert np.isnan(out["tgrad"]).any()
        after = thv.device_call(sw, Z, c, want, dirs)
        for k in want:
            np.testing.assert_array_equal(after[k], clean[k], err_msg=k)
    finally:
        sw.close()


@pytest.mark.gpu
def test_refusals(qc):
    """Without the bit a wide handle keeps the old message and code; a Lindblad wide handle with the bit is refused for its generators."""
    L = qc._lib
    UNS = L.QC_ERR_UNSUPPORTED
    c = build(qc, "one-interval")
    plain = ts.make_sweep(qc, c, wide=True)
    tangent = ts.make_sweep(qc, c, wide=True, wide_tangent=True)
    co = two.two_qubit_case(qc, "wide-hvp/two-qubit-lindblad", S=3, T=4)
    lindblad = ts.make_sweep(qc, co, wide=True, wide_hessian=True)
    try:
        Z = plain.pack(c["controls"], c["dts"])
        for h in (plain, tangent):
            assert not h.hvp_supported and h.hvp_unsupported_reason == OLD and not h.wide_hessian
            with pytest.raises(qc.QCollocError) as e:
                h.hvp(Z, c["init"], c["cot"], c["theta"], c["scale"], vZ=np.zeros(h.Z_len))
            assert e.value.code == UNS and OLD in str(e.value) and str(e.value).count(PRE) == 1
            assert thv._raw(qc, h) == (UNS, OLD)
        assert lindblad.kernel_name == "mfma32-sweep" and lindblad.wide_hessian and not lindblad.hvp_supported
        why = lindblad.hvp_unsupported_reason
        assert why.startswith(PRE) and "is not antisymmetric" in why and "mfma32-sweep form" not in why
        assert thv._raw(qc, lindblad) == (UNS, why)
        Zo = lindblad.pack(co["controls"], co["dts"])
        with pytest.raises(qc.QCollocError) as e:
            lindblad.hvp(Zo, co["init"], np.zeros((co["S"], lindblad.ns)), co["theta"], co["scale"], vZ=np.zeros(lindblad.Z_len))
        assert e.value.code == UNS and "is not antisymmetric" in str(e.value)
        finals, _ = lindblad.eval(Zo, co["init"], co["theta"], co["scale"], fids=False)      # the handle still serves the sweep
        assert np.isfinite(finals).all()
    finally:
        for h in (plain, tangent, lindblad):
            h.close()


@pytest.mark.gpu
def test_hessian_times_on_a_wide_handle(qc):
    """`hessian_times` on 9 levels (S = 3, T = 6) with l(X) = mean_s (1/2 ||X_s - G||^2 + 1/4 ||X_s||^4): against the central difference
    of the objective's own gradient along v (step 1e-5: 1e-6 max |want|), and against `gauss_newton_times` plus the product with vcot = 0
    (2e-9); with only one of the two bits it raises QC_ERR_UNSUPPORTED with the handle's reason."""
    rng = np.random.default_rng(47)
    N, m, T, S = 9, 2, 6, 3
    traj = tv._traj3(qc, rng, N, m, T)
    H0, Hd, P = _herm(rng, N), [_herm(rng, N, 0.5) for _ in range(m)], _herm(rng, N)
    sys_ = qc.QuantumSystem(H0, Hd)
    theta, scale = rng.uniform(-0.2, 0.2, (S, 1)), rng.uniform(0.9, 1.1, (S, m))
    Gnp = np.ascontiguousarray(traj.goal["Ũ⃗"])
    goal = torch.from_numpy(Gnp).cuda()
    loss = lambda X: (0.5 * ((X - goal) ** 2).sum(dim=1) + 0.25 * (X ** 2).sum(dim=1) ** 2).mean()
    obj = qc.SweepFinalStateObjective(traj, sys_, [P], theta, loss, scale=scale, wide=True, wide_tangent=True, wide_hessian=True)
    Z = np.array(traj.datavec, dtype=np.float64)
    nZ = Z.size
    try:
        sw = obj._sweep
        assert obj.wide_hessian and obj.wide_tangent and sw.kernel_name == "mfma32-sweep" and sw._desc.wide == 257 | 16
        a0, dt0 = traj.offset("a"), traj.offset("Δt")
        Km = np.zeros(nZ, dtype=bool)
        Km[:T * traj.dim].reshape(T, traj.dim)[:T - 1, list(range(a0, a0 + m)) + [dt0]] = True
        v = rng.standard_normal(nZ)
        v /= np.linalg.norm(v[Km])
        got = obj.hessian_times(Z, v)
        assert isinstance(got, np.ndarray) and got.shape == (nZ,) and np.all(got[~Km] == 0.0)
        eps = 1e-5
        cd = (obj.grad_L(Z + eps * v) - obj.grad_L(Z - eps * v)) / (2 * eps)
        err = np.abs(got - cd).max() / np.abs(cd).max()
        print(f"SWEEP-WIDE-HVP hessian_times vs the central difference of grad_L (step 1e-5): {err:.3e} of max |want| = {np.abs(cd).max():.3e} (bound 1e-6)")
        assert np.abs(cd).max() > 1e-3 and err <= 1e-6
        # exact = Gauss-Newton + the curvature of the sweep map
        X = obj.finals(Z)
        assert X.shape == (S, sw.ns)
        cot, _ = href.pullback_loss_terms(X, Gnp)
        curv = sw.hvp(Z, traj.initial["Ũ⃗"], cot, theta, scale, vZ=v)[0]
        gn = obj.gauss_newton_times(Z, v)
        worst = thv.ratio(got - gn, curv) / 2
        print(f"SWEEP-WIDE-HVP hessian_times - gauss_newton_times vs hvp(vcot = 0): worst error / bound = {worst:.3e} (max |value| = {np.abs(curv).max():.3e})")
        assert worst <= 1.0 and np.abs(curv).max() > 1e-3
        dgot = obj.hessian_times(torch.from_numpy(Z).cuda(), torch.from_numpy(v).cuda())
        assert torch.is_tensor(dgot) and dgot.is_cuda and thv.ratio(dgot.cpu().numpy(), got) <= 1e-3
    finally:
        obj.close()
    for kw, word in ((dict(wide_tangent=True), OLD), (dict(wide_hessian=True), "qc_sweep pushforward: pushforwards are not served in the mfma32-sweep form")):
        one = qc.SweepFinalStateObjective(traj, sys_, [P], theta, loss, scale=scale, wide=True, **kw)
        try:
            with pytest.raises(qc.QCollocError) as e:
                one.hessian_times(Z, np.ones(nZ))
            assert e.value.code == qc._lib.QC_ERR_UNSUPPORTED and word in str(e.value), (kw, str(e.value))
        finally:
            one.close()


@pytest.mark.gpu
def test_transmon_newton_cg_example(qc):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import transmon_newton_cg
    out = transmon_newton_cg.main(T=12, grid=3, steps=2, cg_iter=8, verbose=False)
    hist = out["loss_history"]
    print(f"SWEEP-WIDE-HVP example: loss {hist[0]:.6e} -> {hist[-1]:.6e} in {out['accepted']} accepted steps, {out['exact_products']} exact Hessian products, "
          f"{out['gn_products']} Gauss-Newton products")
    print("SWEEP-WIDE-HVP example: " + out["summary"])
    assert out["kernel"] == "mfma32-sweep" and out["T"] == 12 and out["S"] == 3
    assert out["exact_products"] > 0 and "exact Hessian products" in out["summary"]
    assert len(hist) == out["accepted"] + 1 >= 2
    assert all(b <= a for a, b in zip(hist, hist[1:])) and hist[-1] < hist[0]
