"""Wide sweep pushforwards (`qc_sweep_desc.wide` bit 4, QC_SWEEP_WIDE_TANGENT; `RolloutSweep(..., wide=True, wide_tangent=True)`):
`qc_sweep_jvp*` on "mfma32-sweep" handles (csrc/qc_sweep32_jvp.hip, the ld = 32 finish kernel of csrc/qc_sweep_jvp.hip).  CPU: the valid
values of `wide`, the device-free scope queries, the launch query, constants, Python keywords, the Julia text, the two reference routes
of tests/sweep_jvp_reference.py against each other on every GPU case.  GPU: every requested value against the Frechet route, the
bit-level properties of tests/test_sweep_jvp.py (its `check_case`, unchanged), isolation of a non-finite direction, the adjoint identity
against the wide pullback (closed, and the stored-state walk of a two-qubit Lindblad model), a state of 4096 entries (the 144 KiB
launch of the finish kernel), forward-mode autograd, the Gauss-Newton product, refusals without the bit, the example.

Tolerance (GPU against the reference): that of tests/test_sweep_jvp.py, JVP_RTOL = 1e-9 -- per sample
|got - want| <= 1e-9 max(1, max |want_s|) for tfinals and tfids (the kernels hold states to 1e-10, a tangent is a bounded bilinear
form of states and direction); finals: the state tolerance of test_sweep.py.  The adjoint identity: 1e-9 relative, both sides above
1e-3.  The helpers are those of the existing files, imported, not copied.
Every sample of mid-size and filled launches, the scratch `dTotJ`, the one-slot branch of the finish kernel:
tests/test_sweep_wide_jvp_every_sample.py."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

import sweep_jvp_reference as jref
import sweep_reference as ref
import test_sweep as ts
import test_sweep_grad as tg
import test_sweep_jvp as tj
import test_sweep_open_grad as too
import test_sweep_vjp as tv
import test_sweep_wide as tw
import test_sweep_wide_open_grad as two

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_herm, _unitary = ts._herm, ts._unitary
U_ABS = ("unitary", None, "abs")
TANGENT = 16

# name: (state, levels, m, p, scale given, free timestep, S, T, fidelity, samples checked against the reference), the tuple of
# test_sweep_wide.build; the two Lindblad models come from test_sweep_wide_open_grad
SPECS = {
    "n9-S5-T11": ("unitary", 9, 2, 1, True, True, 5, 11, ("unitary", [0, 1, 3, 4], "abs"), None),      # chunks 3, 3, 3, 1: 20 work items
    "n9-S3-T11": ("unitary", 9, 2, 1, True, True, 3, 11, U_ABS, None),                                 # 12 work items
    "n10-S3-T10": ("unitary", 10, 1, 1, False, True, 3, 10, U_ABS, None),                              # 9 work items: the last workgroup's last wave exits
    "n16-m8": ("unitary", 16, 8, 2, True, False, 3, 6, ("unitary", None, "abs2"), None),               # full tiles, 8 drives, fixed timestep
    "n12-no-drives": ("unitary", 12, 0, 1, False, False, 3, 6, U_ABS, None),                           # only vtheta and vinit act
    "n10-kets3": ("kets3", 10, 1, 3, True, False, 4, 7, None, None),                                   # no fidelity
    "n12-ket": ("ket", 12, 2, 1, True, True, 11, 5, ("ket", None, "abs"), None),
    "squarings": ("unitary", 9, 2, 1, False, True, 3, 8, U_ABS, None),                                 # timesteps log-uniform in [1e-3, 40]
    "one-chunk": ("unitary", 9, 2, 1, True, True, 2048, 3, U_ABS, (0, 1000, 2047)),
    "one-interval": ("unitary", 9, 2, 1, False, True, 3, 2, U_ABS, None),                              # T = 2: the prefetch reads tn = t
    "n16-no-perturbations": ("unitary", 16, 2, 0, True, True, 3, 6, U_ABS, None),                      # p = 0: theta empty, no vtheta, Bdot stays zero
    "long": ("unitary", 9, 2, 1, False, True, 2, 1000, U_ABS, None),                                   # 32 chunks of 32, the last 7: the finish kernel chains 32 totals
}
LINDBLAD = {
    "two-qubit-lindblad": lambda qc: two.two_qubit_case(qc, "wide-jvp/two-qubit-lindblad", S=5, T=9),  # N = 16 = 4^2, density fidelity
    "qutrit-lindblad": lambda qc: two.qutrit_case(qc, "wide-jvp/qutrit-lindblad", S=3, T=6, free=False),
}
CASES = list(SPECS) + list(LINDBLAD)
ITEMS = {"n9-S5-T11": (3, 4, 1, 20), "n9-S3-T11": (3, 4, 1, 12), "n10-S3-T10": (3, 3, 3, 9), "one-chunk": (2, 1, 2, 2048),
         "one-interval": (1, 1, 1, 3), "n16-no-perturbations": (2, 3, 1, 9), "long": (32, 32, 7, 64)}


def build(qc, name):
    """The case plus a direction with every part that exists non-zero (the draws of test_sweep_jvp.build)."""
    if name in LINDBLAD:
        c = LINDBLAD[name](qc)
        c["n"] = 2 * c["N"]
    else:
        c = tw.build(qc, "wide-jvp/" + name, SPECS[name])
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


def handle(qc, c, **kw):
    return ts.make_sweep(qc, c, wide=True, wide_tangent=True, **kw)


# ---------------------------------------------------------------------------------------------------------------------------------
#  CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_wide_values_with_the_tangent_bit(qc):
    L = qc._lib
    val = lambda D: L.lib.qc_sweep_desc_validate(C.byref(D.d))
    assert L.QC_SWEEP_WIDE_TANGENT == TANGENT
    for N in (12, 16, 2):
        for good in (0, 1, 3, 9, 11, 17, 19, 25, 27):
            assert val(tw._wdesc(qc, good, N=N)) == L.QC_OK, (N, good)
        for bad in (16, 18, 20, 21, 24, 32 | 1, 2, 4, 5, 7, 8, 10, 12, 13, 15, -1, (1 << 20) | 1):
            assert val(tw._wdesc(qc, bad, N=N)) == L.QC_ERR_INVALID, (N, bad)
            msg = L.lib.qc_sweep_last_error(None).decode()
            assert msg.startswith("qc_sweep: wide") and "17, 19, 25 or 27" in msg and "QC_SWEEP_WIDE_TANGENT (16)" in msg, (N, bad, msg)


def _lindblad_desc(qc, wide, N=16, **kw):
    D = too._ODesc(qc, wide=wide, **{**dict(N=N, m=2, cols=1, fid_kind=qc._lib.QC_FID_DENSITY), **kw})
    D.G0[:] = np.random.default_rng(0).standard_normal(D.G0.size)       # not antisymmetric
    return D


def test_jvp_scope_follows_the_bit(qc):
    L = qc._lib
    U = L.QC_FID_UNITARY
    q = lambda D: too._query(qc, "qc_sweep_desc_jvp_supported", D)
    for N in (9, 12, 16):
        for wide in (17, 19, 25, 27):
            assert q(tw._wdesc(qc, wide, N=N, fid_kind=U))[:2] == (L.QC_OK, 1), (N, wide)            # zero matrices: antisymmetric
        assert q(tw._wdesc(qc, 17, N=N, cols=3))[:2] == (L.QC_OK, 1)                                   # no fidelity
        assert q(tw._wdesc(qc, 17, N=N, cols=17))[:2] == (L.QC_OK, 1)                                  # more columns than reverse mode takes
    assert q(_lindblad_desc(qc, 17, N=16))[:2] == (L.QC_OK, 1) and q(_lindblad_desc(qc, 17, N=9))[:2] == (L.QC_OK, 1)
    assert q(_lindblad_desc(qc, 27, N=16, flag=1))[:2] == (L.QC_OK, 1)
    old = "qc_sweep pushforward: pushforwards are not served in the mfma32-sweep form"
    for wide in (1, 3, 9, 11):
        assert q(tw._wdesc(qc, wide, N=12, fid_kind=U)) == (L.QC_OK, 0, old)
        assert q(_lindblad_desc(qc, wide)) == (L.QC_OK, 0, old)
    rc, ok, msg = q(tw._wdesc(qc, 17, N=12, m=9, fid_kind=U))
    assert (rc, ok) == (L.QC_OK, 0) and msg == "qc_sweep pushforward: the handle takes the rollout-per-sample form (9 drives > 8)"
    rc, ok, msg = q(tw._wdesc(qc, 17, N=17, fid_kind=U))
    assert (rc, ok) == (L.QC_OK, 0) and msg == "qc_sweep pushforward: the handle takes the rollout-per-sample form (2N = 34 > 32)"
    for N in (2, 8):                                                                                   # the narrow form does not look at the bit
        assert q(tw._wdesc(qc, 17, N=N, fid_kind=U))[:2] == (L.QC_OK, 1) and q(tw._wdesc(qc, 0, N=N, fid_kind=U))[:2] == (L.QC_OK, 1)
    assert q(tw._wdesc(qc, 16, N=12))[0] == L.QC_ERR_INVALID
    # Hessian products and noise sweeps keep refusing the form, in their old words
    for wide in (1, 17, 27):
        rc, ok, msg = too._query(qc, "qc_sweep_desc_hvp_supported", tw._wdesc(qc, wide, N=12, fid_kind=U))
        assert (rc, ok) == (L.QC_OK, 0) and msg == "qc_sweep Hessian product: Hessian products are not served in the mfma32-sweep form", msg
        rc, ok, msg = too._query(qc, "qc_sweep_desc_noise_supported", tw._wdesc(qc, wide, N=12, fid_kind=U))
        assert (rc, ok) == (L.QC_OK, 0) and msg == "qc_sweep noise: noise trajectories are not served in the mfma32-sweep form", msg
    # reverse mode answers what it answered without the bit
    for fn in ("qc_sweep_desc_grad_supported", "qc_sweep_desc_vjp_supported"):
        for base in (1, 3, 9, 11):
            for D in (lambda w: tw._wdesc(qc, w, N=12, fid_kind=U), lambda w: _lindblad_desc(qc, w), lambda w: _lindblad_desc(qc, w, flag=1)):
                assert too._query(qc, fn, D(base)) == too._query(qc, fn, D(base | TANGENT)), (fn, base)


def test_launch_query_does_not_see_the_tangent_bit(qc):
    L = qc._lib
    for n in (16, 18, 24, 32, 34):
        for m in (1, 8, 9):
            for S, T in ((1, 2), (2, 102), (5, 12), (11, 50), (2047, 50), (2048, 3), (8192, 1000)):
                got = []
                for wide in (1, 17, 19, 25, 27):
                    D = tw._wdesc(qc, wide, N=n // 2, m=m, T=T, cols=1)
                    mf, ch, nch = C.c_int32(), C.c_int64(), C.c_int64()
                    assert L.lib.qc_sweep_desc_launch(C.byref(D.d), S, C.byref(mf), C.byref(ch), C.byref(nch)) == L.QC_OK
                    got.append((bool(mf.value), ch.value, nch.value))
                want = tw.wide_launch(n, m, S, T)
                assert set(got) == {(want["mfma"], want["chunk"], want["n_chunks"])}, (n, m, S, T)
    for name, (chunk, n_chunks, last, items) in ITEMS.items():
        _, L_, m, _, _, _, S, T, _, _ = SPECS[name]
        w = tw.wide_launch(2 * L_, m, S, T)
        assert (w["chunk"], w["n_chunks"], w["last"], S * w["n_chunks"]) == (chunk, n_chunks, last, items), name
    assert ITEMS["n10-S3-T10"][3] % 2 == 1 and ITEMS["n10-S3-T10"][3] % 4 != 0      # whichever the waves per workgroup: a wave exits


def test_constants_abi_and_texts(qc, tmp_path):
    import subprocess
    L = qc._lib
    assert (L.QC_SWEEP_WIDE, L.QC_SWEEP_WIDE_PARAMS, L.QC_SWEEP_WIDE_STORED, L.QC_SWEEP_WIDE_TANGENT) == (1, 2, 8, 16)
    header = open(os.path.join(ROOT, "include", "qcolloc.h")).read()
    assert re.search(r"^#define QC_SWEEP_WIDE_TANGENT 16\b", header, re.M)
    assert "0, 1, 3, 9, 11, 17, 19, 25 and 27" in header
    assert L.lib.qc_abi_version() == 6
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "qcolloc.h"\nint main(){printf("%zu %d\\n", sizeof(qc_sweep_desc), QC_SWEEP_WIDE_TANGENT);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [128, 16] and L.lib.qc_sizeof_sweep_desc() == 128
    # no new exported symbol: the wide pushforward is reached through the entry points that were there
    assert not any("sweep32" in name for name in L.SYMBOLS)
    julia = open(os.path.join(ROOT, "julia", "QCollocHIP.jl"), encoding="utf-8").read()
    assert re.search(r"^const QC_SWEEP_WIDE_TANGENT = 16\b", julia, re.M)
    push = julia[julia.index("function rollout_sweep_pushforward("):]
    push = push[:push.index("\nend\n")]
    assert "wide::Bool=false" in push and "wide ? (QC_SWEEP_WIDE | QC_SWEEP_WIDE_TANGENT) : 0" in push
    makefile = open(os.path.join(ROOT, "quantumcollocation.jl_amd", "csrc", "Makefile")).read()
    assert "qc_sweep32_jvp.hip" in makefile and "qc_sweep32_jvp.o" in makefile
    design = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    assert "Wide sweep pushforwards" in design and "864 + 96" in design
    assert "qc_sweep32_jvp.hip" in open(os.path.join(ROOT, "README.md"), encoding="utf-8").read()


def test_python_keywords(qc):
    for f in (qc.RolloutSweep.__init__, qc.rollout_sweep, qc.SweepFinalStateObjective.__init__):
        par = inspect.signature(f).parameters
        assert "wide_tangent" in par and par["wide_tangent"].default is False, f
    rng = np.random.default_rng(0)
    sys9 = qc.QuantumSystem(_herm(rng, 9), [_herm(rng, 9)])
    for kw in (dict(), dict(stored_states=True)):      # before the library is touched: no device is needed to be told so
        with pytest.raises(ValueError, match="wide_tangent"):
            qc.RolloutSweep(sys9, [], 5, wide_tangent=True, **kw)


# `long` (T = 1000) is left out, as tests/test_sweep_jvp.py leaves its own out: the 1e-11 bound between the two routes was not written
# for a thousand steps
@pytest.mark.parametrize("name", [k for k in CASES if k not in ("one-chunk", "long")] + ["one-chunk", "many-columns"])
def test_reference_routes_agree(qc, name):
    """expm_frechet along the recurrence against the complex step through expm on every case the GPU tests use but `long` (two samples
    of each): 1e-11 max(1, max |want|), and tangents that a zero could not pass for."""
    c = many_columns(qc) if name == "many-columns" else build(qc, name)
    samples = sorted({0, c["S"] - 1})
    args = (c["G0"], c["Gd"], c["Gp"], c["controls"], c["dts"], c["init"], c["theta"], c["scale"], samples)
    kw = dict(vcontrols=c["vcontrols"], vdts=c["vdts"], vinit=c["vinit"], vtheta=c["vtheta"], vscale=c["vscale"], fid=c["fid"])
    a, b = jref.pushforward_frechet(*args, **kw), jref.pushforward_complex_step(*args, **kw)
    for key in ("finals", "tfinals", "tfids"):
        if a[key] is None:
            assert c["fid"] is None and b[key] is None
            continue
        err = np.abs(a[key] - b[key]).max() / max(1.0, np.abs(a[key]).max())
        print(f"SWEEP-WIDE-JVP reference {name} {key}: frechet vs complex step {err:.2e}, max |value| {np.abs(a[key]).max():.3e}")
        assert err <= 1e-11 and np.abs(a[key]).max() > 1e-3, key


# ---------------------------------------------------------------------------------------------------------------------------------
#  GPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_wide_jvp_matches_the_reference(qc, name):
    """Every requested value against the Frechet route along the full direction, and the bit-level properties of
    test_sweep_jvp.check_case: finals / fids are `eval`'s, a second call, each output alone, a NULL direction against zeros, the host
    entry point, a side stream, NaNs in the unread entries of vZ."""
    c = build(qc, name)
    sw = handle(qc, c)
    try:
        assert sw.kernel_name == "mfma32-sweep" and sw.wide_tangent and sw.jvp_supported and sw.jvp_unsupported_reason is None
        assert not sw.hvp_supported
        want = tw.wide_launch(c["n"], c["m"], c["S"], c["T"])
        assert sw.launch(c["S"]) == (True, want["chunk"], want["n_chunks"])
        if name in ITEMS:
            assert (want["chunk"], want["n_chunks"], want["last"], c["S"] * want["n_chunks"]) == ITEMS[name]
        if name in LINDBLAD:
            assert np.abs(c["G0"] + c["G0"].T).max() > 0.05 and not sw.vjp_supported and not sw.stored_states
        if name == "squarings":
            sq = [ts._squarings(np.abs(c["dts"][t] * ref.sample_generator(c["G0"], c["Gd"], c["Gp"], c["controls"][:, t], c["theta"][s], np.ones(c["m"]))).sum(axis=0).max())
                  for s in range(c["S"]) for t in range(c["T"] - 1)]
            assert min(sq) == 0 and max(sq) >= 10, sq
        tj.check_case(sw, c)
    finally:
        sw.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["vZ", "vinit", "vtheta", "vscale"])
def test_each_direction_alone(qc, which):
    """tfinals and tfids along one of the four directions at a time, on the 20-item case and on the two-qubit Lindblad model."""
    for name in ("n9-S5-T11", "two-qubit-lindblad"):
        c = build(qc, name)
        only = dict(vcontrols=None, vdts=None, vinit=None, vtheta=None, vscale=None)
        for k in {"vZ": ("vcontrols", "vdts"), "vinit": ("vinit",), "vtheta": ("vtheta",), "vscale": ("vscale",)}[which]:
            only[k] = c[k]
        if which == "vZ":
            only["vcontrols"] = c["vcontrols"]
        r = jref.pushforward_frechet(c["G0"], c["Gd"], c["Gp"], c["controls"], c["dts"], c["init"], c["theta"], c["scale"], c["samples"], fid=c["fid"], **only)
        sw = handle(qc, c)
        try:
            Z = sw.pack(c["controls"], c["dts"])
            out = tj.device_call(sw, Z, c, tj.OUTPUTS, {which: tj.direction(sw, c)[which]})
        finally:
            sw.close()
        assert np.abs(r["tfinals"]).max() > 1e-3
        tj.assert_samples(out["tfinals"], r["tfinals"], f"wide {name} tfinals along {which}")
        tj.assert_samples(out["tfids"][:, None], r["tfids"][:, None], f"wide {name} tfids along {which}")


@pytest.mark.gpu
def test_isolation_of_a_non_finite_direction(qc):
    """A NaN in vtheta[1] (then in vscale[1]) makes only sample 1's tangents non-finite and leaves every other sample's bits as they were."""
    c = build(qc, "n9-S5-T11")
    sw = handle(qc, c)
    try:
        Z = sw.pack(c["controls"], c["dts"])
        dirs = tj.direction(sw, c)
        clean = tj.device_call(sw, Z, c, tj.OUTPUTS, dirs)
        others = [s for s in range(c["S"]) if s != 1]
        for which in ("vtheta", "vscale"):
            bad = dirs[which].copy()
            bad[1, 0] = np.nan
            out = tj.device_call(sw, Z, c, tj.OUTPUTS, dict(dirs, **{which: bad}))
            for k in tj.OUTPUTS:
                np.testing.assert_array_equal(out[k][others], clean[k][others], err_msg=k)
            np.testing.assert_array_equal(out["finals"], clean["finals"])
            np.testing.assert_array_equal(out["fids"], clean["fids"])
            assert not np.isfinite(out["tfinals"][1]).any() and not np.isfinite(out["tfids"][1])
        after = tj.device_call(sw, Z, c, tj.OUTPUTS, dirs)
        for k in tj.OUTPUTS:
            np.testing.assert_array_equal(after[k], clean[k], err_msg=k)
    finally:
        sw.close()


def _adjoint_identity(sw, c, what):
    Z = sw.pack(c["controls"], c["dts"])
    dirs = tj.direction(sw, c)
    rng = np.random.default_rng(3)
    cot = rng.standard_normal((c["S"], sw.ns))
    cot /= np.linalg.norm(cot, axis=1, keepdims=True)
    tf = sw.jvp(Z, c["init"], dirs["vZ"], c["theta"], c["scale"], vinit=dirs["vinit"], vtheta=dirs["vtheta"], vscale=dirs["vscale"])
    lhs = np.einsum("sn,sn->s", cot, tf)
    rhs = tj.pairing(sw, c, dirs, sw.vjp(Z, c["init"], cot, c["theta"], c["scale"], per_sample=True, init_grad=True, params=True))
    rel = np.abs(lhs - rhs) / np.maximum(np.abs(lhs), np.abs(rhs))
    print(f"SWEEP-WIDE-JVP {what} adjoint identity: worst relative difference {rel.max():.3e} (bound 1e-9), |value| in "
          f"[{np.minimum(np.abs(lhs), np.abs(rhs)).min():.3e}, {np.abs(rhs).max():.3e}]")
    assert np.minimum(np.abs(lhs), np.abs(rhs)).min() > 1e-3
    assert rel.max() <= 1e-9


@pytest.mark.gpu
def test_adjoint_identity_with_the_wide_pullback(qc):
    """<cot_s, tfinals[s]> = <vjp(cot)_s, v> for every sample, on a closed handle with wide = 19."""
    c = build(qc, "n9-S5-T11")
    sw = handle(qc, c, wide_params=True)
    try:
        assert sw._desc.wide == 19 and sw.vjp_supported and sw.jvp_supported
        _adjoint_identity(sw, c, "closed, wide = 19")
    finally:
        sw.close()


@pytest.mark.gpu
def test_adjoint_identity_with_the_stored_state_pullback(qc):
    """The same on the two-qubit Lindblad model: wide = 27 and reserved1[0] = 1, the pullback by the stored-state walk."""
    c = build(qc, "two-qubit-lindblad")
    sw = handle(qc, c, wide_params=True, wide_stored=True, stored_states=True)
    try:
        assert sw._desc.wide == 27 and sw._desc.reserved1[0] == 1 and sw.vjp_supported and sw.jvp_supported
        _adjoint_identity(sw, c, "two-qubit Lindblad, wide = 27, stored states")
    finally:
        sw.close()


def many_columns(qc):
    """N = 16 with 128 ket columns (ns = 4096), T = 3, S = 2: the finish kernel's largest launch, 4 ns + 2048 doubles = 144 KiB."""
    name = "many-columns"
    N, cols, S, T, m, p = 16, 128, 2, 3, 2, 1
    c = tw.build(qc, "wide-jvp/" + name, ("kets3", N, m, p, True, True, S, T, None, None))
    rng = np.random.default_rng(23 + sum(map(ord, name)))
    K = rng.standard_normal((N, cols)) + 1j * rng.standard_normal((N, cols))
    K /= np.linalg.norm(K, axis=0)
    c["init"], c["cols"] = ref.operator_to_iso_vec(K), cols
    ns = c["init"].size
    assert ns == 4096 and (4 * ns + 2048) * 8 == 144 * 1024
    c.update(vcontrols=rng.standard_normal((m, T)), vdts=0.1 * rng.standard_normal(T), vinit=rng.standard_normal(ns) / np.sqrt(ns),
             vtheta=rng.standard_normal((S, p)), vscale=rng.standard_normal((S, m)), fid=None)
    return c


@pytest.mark.gpu
def test_many_columns(qc):
    c = many_columns(qc)
    sw = handle(qc, c)
    try:
        assert sw.kernel_name == "mfma32-sweep" and sw.ns == 4096 and sw.jvp_supported
        Z = sw.pack(c["controls"], c["dts"])
        finals, _ = sw.eval(Z, c["init"], c["theta"], c["scale"])
        dirs = tj.direction(sw, c)
        out = tj.device_call(sw, Z, c, ("finals", "tfinals"), dirs)
        again = tj.device_call(sw, Z, c, ("finals", "tfinals"), dirs)
    finally:
        sw.close()
    r = tj.reference(c)
    ts._assert_states(out["finals"], r["finals"], "SWEEP-WIDE-JVP many columns finals")
    tj.assert_samples(out["tfinals"], r["tfinals"], "wide many columns tfinals")
    np.testing.assert_array_equal(out["finals"], finals.T, err_msg="finals of jvp_device against eval")
    for k in out:
        np.testing.assert_array_equal(again[k], out[k], err_msg=k + ", second call")


@pytest.mark.gpu
def test_finals_autograd_forward_mode_on_a_wide_handle(qc):
    """Under forward_ad the tangent of `finals_autograd` is `jvp_device`'s tfinals, bit for bit, for tangents on Z, init and theta."""
    import torch.autograd.forward_ad as fwAD
    rng = np.random.default_rng(37)
    N, m, T, S = 9, 2, 5, 3
    sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, 0.5) for _ in range(m)])
    sw = qc.RolloutSweep(sys_, [_herm(rng, N)], T, wide=True, wide_tangent=True)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    try:
        assert sw.kernel_name == "mfma32-sweep"
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
                assert torch.equal(primal, fin) and torch.equal(tangent, want) and float(tangent.abs().max()) > 1e-3, which
    finally:
        sw.close()


@pytest.mark.gpu
def test_gauss_newton_product_on_a_wide_handle(qc):
    """`gauss_newton_times` on 9 levels (T = 4, S = 3) with loss = sum ||X - G||^2 / (2 S) against J^T J v / S assembled on the CPU from the
    Frechet route over the unit directions: 1e-9; symmetry; `hessian_times` keeps refusing."""
    rng = np.random.default_rng(41)
    N, m, T, S = 9, 2, 4, 3
    traj = tv._traj3(qc, rng, N, m, T)
    H0, Hd, P = _herm(rng, N), [_herm(rng, N, 0.5) for _ in range(m)], _herm(rng, N)
    sys_ = qc.QuantumSystem(H0, Hd)
    theta, scale = rng.uniform(-0.2, 0.2, (S, 1)), rng.uniform(0.9, 1.1, (S, m))
    goal = torch.from_numpy(np.ascontiguousarray(traj.goal["Ũ⃗"])).cuda()
    obj = qc.SweepFinalStateObjective(traj, sys_, [P], theta, lambda X: ((X - goal) ** 2).sum() / (2 * S), scale=scale, wide=True, wide_tangent=True)
    Z = traj.datavec
    nZ = Z.size
    try:
        assert obj.wide_tangent and obj._sweep.kernel_name == "mfma32-sweep"
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
        print(f"SWEEP-WIDE-JVP gauss_newton_times vs J^T J v / S: {err:.3e} (bound 1e-9), max |value| {np.abs(want).max():.3f}")
        assert err <= 1e-9 and np.abs(want).max() > 1e-3
        gu = obj.gauss_newton_times(Z, u)
        assert abs(u @ got - v @ gu) <= 1e-9 * abs(u @ got) and abs(u @ got) > 1e-3
        dgot = obj.gauss_newton_times(torch.from_numpy(Z).cuda(), torch.from_numpy(v).cuda())
        assert torch.is_tensor(dgot) and dgot.is_cuda
        np.testing.assert_array_equal(dgot.cpu().numpy(), got)
        with pytest.raises(qc.QCollocError) as e:
            obj.hessian_times(Z, v)
        assert e.value.code == qc._lib.QC_ERR_UNSUPPORTED and "Hessian products are not served in the mfma32-sweep form" in str(e.value)
    finally:
        obj.close()


@pytest.mark.gpu
def test_refusals_are_unchanged(qc):
    """Without the bit a wide handle refuses the pushforward in its old words; with it, Hessian products and noise sweeps keep refusing."""
    L = qc._lib
    UNS = L.QC_ERR_UNSUPPORTED
    c = build(qc, "n9-S3-T11")
    plain = ts.make_sweep(qc, c, wide=True)
    tan = handle(qc, c)
    try:
        Z = plain.pack(c["controls"], c["dts"])
        old = "qc_sweep pushforward: pushforwards are not served in the mfma32-sweep form"
        assert not plain.jvp_supported and plain.jvp_unsupported_reason == old and not plain.wide_tangent
        with pytest.raises(qc.QCollocError) as e:
            plain.jvp(Z, c["init"], np.zeros(plain.Z_len), c["theta"], c["scale"])
        assert e.value.code == UNS and old in str(e.value)
        rc, msg = tj._raw(qc, plain)
        assert rc == UNS and msg == old
        assert tj._raw(qc, tan)[0] == L.QC_OK
        with pytest.raises(qc.QCollocError) as e:
            tan.hvp(Z, c["init"], np.zeros((c["S"], tan.ns)), c["theta"], c["scale"], vZ=np.zeros(tan.Z_len))
        assert e.value.code == UNS and "qc_sweep Hessian product: Hessian products are not served in the mfma32-sweep form" in str(e.value)
        with pytest.raises(qc.QCollocError) as e:
            tan.noise_eval(Z, c["init"], np.zeros((c["S"], c["T"] - 1, 1)), c["theta"], c["scale"])
        assert e.value.code == UNS and "qc_sweep noise: noise trajectories are not served in the mfma32-sweep form" in str(e.value)
        # the forward sweep and the gradient of the two handles: the same bits
        fa, fb = plain.eval(Z, c["init"], c["theta"], c["scale"]), tan.eval(Z, c["init"], c["theta"], c["scale"])
        np.testing.assert_array_equal(fa[0], fb[0])
        np.testing.assert_array_equal(fa[1], fb[1])
        ga, gb = plain.grad(Z, c["init"], c["theta"], c["scale"]), tan.grad(Z, c["init"], c["theta"], c["scale"])
        for x, y in zip(ga, gb):
            np.testing.assert_array_equal(x, y)
        assert plain.kernel_name == tan.kernel_name == "mfma32-sweep"
    finally:
        plain.close()
        tan.close()


@pytest.mark.gpu
def test_transmon_gauss_newton_example(qc):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import transmon_gauss_newton
    out = transmon_gauss_newton.main(T=10, grid=3, steps=3, cg_iter=8, verbose=False)
    hist = out["loss_history"]
    print(f"SWEEP-WIDE-JVP example: loss {hist[0]:.6e} -> {hist[-1]:.6e} in {out['accepted']} accepted steps, {out['gn_products']} Gauss-Newton products")
    assert out["kernel"] == "mfma32-sweep"
    assert len(hist) == out["accepted"] + 1 >= 2
    assert all(b <= a for a, b in zip(hist, hist[1:])) and hist[-1] < hist[0]
