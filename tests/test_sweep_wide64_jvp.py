"""Sweep pushforwards in the "mfma64-sweep" form (`qc_sweep_desc.wide` bit 14, QC_SWEEP_WIDE_64_TANGENT;
`RolloutSweep(..., wide=True, wide64=True, wide64_tangent=True)`): `qc_sweep_jvp*` on handles of 32 < 2N <= 64
(csrc/qc_sweep64_jvp.hip, the ld = 64 finish kernel of csrc/qc_sweep_jvp.hip).  CPU: the valid values of `wide`, the launch rule and the
scope queries with and without the bit, the pushforward's own scope (the bound ns <= 2048), constants, keywords, texts, the two routes of
tests/sweep_jvp_reference.py against each other at 17 levels.  GPU: every requested value against the Frechet route with the bit-level
properties of tests/test_sweep_jvp.py (its `check_case`, unchanged), the squaring counts, exact cases, scratch that grows and shrinks,
isolation of a non-finite direction, the adjoint identity against the 4 x 4-tile pullback, forward-mode autograd, the Gauss-Newton
product, refusals, the example.

Tolerances are the project's (tests/test_sweep_jvp.py): per sample |got - want| <= 1e-9 max(1, max |want_s|) for tfinals and tfids
against `pushforward_frechet`; finals / fids: the state and fidelity tolerances of tests/test_sweep.py; the adjoint identity: 1e-9
relative, both sides above 1e-3.  The helpers are those of the existing files, imported, not copied.  Every GPU test prints its worst
error as a share of its bound.  Every sample of launches of 250 .. 510 workgroups: tests/test_sweep_wide64_jvp_every_sample.py."""
import ctypes as C
import inspect
import os
import re
import subprocess
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
import test_sweep_wide64 as t64
import test_sweep_wide_jvp as twj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_herm, _unitary = ts._herm, ts._unitary
U_ABS = ("unitary", None, "abs")
W64, GRAD64, PARAMS64, TAN64 = 1024, 2048, 8192, 16384
NS_MAX = 2048
QUERIES = ("grad", "vjp", "hvp", "noise")          # every *_supported query but the pushforward's

# name: (state, levels, m, p, scale given, free timestep, S, T, fidelity, samples checked against the reference), the tuple of
# test_sweep_wide.build
SPECS = {
    "n17-S3-T26": ("unitary", 17, 2, 1, True, True, 3, 26, ("unitary", [0, 1, 3, 4], "abs"), None),   # third tile row almost empty; five chunks of five
    "n17-S3-T12": ("unitary", 17, 2, 1, True, True, 3, 12, U_ABS, None),                              # chunks 3, 3, 3, 2
    "n17-S5-T3": ("unitary", 17, 2, 1, False, True, 5, 3, U_ABS, None),                               # one-interval chunks
    "n17-T2": ("unitary", 17, 2, 1, True, True, 3, 2, U_ABS, None),                                   # T = 2: the prefetch reads its own knot
    "n24-m6-p8": ("unitary", 24, 6, 8, True, True, 3, 4, U_ABS, None),                                # exactly three tiles, every perturbation slot
    "n27-fixed-abs2": ("unitary", 27, 6, 1, True, False, 3, 5, ("unitary", None, "abs2"), None),      # three transmons, fixed timestep, |t|^2 / n^2
    "n32-S2-T102": ("unitary", 32, 10, 3, True, True, 2, 102, U_ABS, None),                           # ns = 2048: the 128 KiB finish launch; eleven sqrt-capped chunks
    "n32-m16": ("unitary", 32, 16, 0, True, False, 3, 5, None, None),                                 # the drive limit; no fidelity, no perturbation
    "n20-no-drives": ("unitary", 20, 0, 1, False, False, 3, 6, U_ABS, None),                          # only vtheta and vinit act
    "ket20-S256-T3": ("ket", 20, 2, 1, True, True, 256, 3, ("ket", None, "abs"), (0, 100, 255)),      # one chunk at the fill constant
    "kets3-n18": ("kets3", 18, 1, 3, True, False, 4, 7, None, None),                                  # few columns, no fidelity
    "n17-cols33": ("kets3", 17, 2, 1, True, True, 3, 6, None, None),                                  # 33 columns: more than reverse mode takes
    "lindblad25": ("density", 5, 2, 1, True, True, 4, 9, ("density", None, "abs"), None),             # N = 25: generators not antisymmetric
    "squarings": ("unitary", 17, 2, 1, False, True, 3, 8, U_ABS, None),                               # timesteps log-uniform in [1e-3, 40]
}
# name: (chunk, n_chunks, intervals of the last chunk, workgroups)
ITEMS = {"n17-S3-T26": (5, 5, 5, 15), "n17-S3-T12": (3, 4, 2, 12), "n17-S5-T3": (1, 2, 1, 10), "n17-T2": (1, 1, 1, 3),
         "n32-S2-T102": (10, 11, 1, 22), "ket20-S256-T3": (2, 1, 2, 256)}


def build(qc, name):
    """The case plus a direction with every part that exists non-zero (the draws of test_sweep_jvp.build)."""
    c = tw.build(qc, "wide64-jvp/" + name, SPECS[name])
    rng = np.random.default_rng(11 + sum(map(ord, name)))
    if name == "n17-cols33":
        K = rng.standard_normal((17, 33)) + 1j * rng.standard_normal((17, 33))
        K /= np.linalg.norm(K, axis=0)
        c["init"], c["cols"] = ref.operator_to_iso_vec(K), 33
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
    return ts.make_sweep(qc, c, wide=True, wide64=True, wide64_tangent=True, **kw)


def _squaring_counts(c):
    return [ts._squarings(np.abs(c["dts"][t] * ref.sample_generator(c["G0"], c["Gd"], c["Gp"], c["controls"][:, t], c["theta"][s], np.ones(c["m"]))).sum(axis=0).max())
            for s in range(c["S"]) for t in range(c["T"] - 1)]


# ---------------------------------------------------------------------------------------------------------------------------------
#  CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def _valid_without_the_bit():
    """Every value valid before bit 14: those of test_sweep_wide64._valid_today, the odd ones | 1024, those | 2048, those | 8192."""
    out = set()
    for v in t64._valid_today():
        out.add(v)
        if v:
            out |= {v | W64, v | W64 | GRAD64, v | W64 | GRAD64 | PARAMS64}
    return out


def test_wide_values_with_the_tangent64_bit(qc):
    L = qc._lib
    val = lambda D: L.lib.qc_sweep_desc_validate(C.byref(D.d))
    msg = lambda: L.lib.qc_sweep_last_error(None).decode()
    assert L.QC_SWEEP_WIDE_64_TANGENT == TAN64 == 1 << 14
    before = _valid_without_the_bit()
    assert len(before) == 33 + 3 * 32
    for N in (20, 12, 2):
        for v in t64._valid_today():
            for extra in (0, W64, W64 | GRAD64, W64 | GRAD64 | PARAMS64, GRAD64, PARAMS64, W64 | PARAMS64, GRAD64 | PARAMS64):
                for tan in (0, TAN64):
                    value = v | extra | tan
                    # valid: a value valid before, alone or -- when it has bits 0 and 10 -- with bit 14
                    want = (v | extra) in before and (not tan or bool(value & 1 and value & W64))
                    assert (val(tw._wdesc(qc, value, N=N)) == L.QC_OK) == want, (N, value)
                    if not want:
                        assert val(tw._wdesc(qc, value, N=N)) == L.QC_ERR_INVALID, (N, value)
        for bad in (TAN64, TAN64 | 1, TAN64 | W64, TAN64 | 1 | GRAD64, TAN64 | 1 | W64 | 4, TAN64 | 1 | W64 | 32, TAN64 | 1 | W64 | 128,
                    TAN64 | 1 | W64 | 512, TAN64 | 1 | W64 | 4096, TAN64 | 1 | W64 | (1 << 20), 1 | W64 | 4096, 1 | W64 | (1 << 15), -1):
            assert val(tw._wdesc(qc, bad, N=N)) == L.QC_ERR_INVALID, (N, bad)
            text = msg()
            assert text.startswith("qc_sweep: wide"), text
            for words in ("17, 19, 25 or 27", "QC_SWEEP_WIDE_TANGENT (16)", "QC_SWEEP_WIDE_NOISE (64)", "QC_SWEEP_WIDE_HESSIAN (256)",
                          "QC_SWEEP_WIDE_64 (1024)", "QC_SWEEP_WIDE_64_GRAD (2048)", "QC_SWEEP_WIDE_64_PARAMS (8192)",
                          "QC_SWEEP_WIDE_64_TANGENT (16384)"):
                assert words in text, (words, text)
        for good in (1 | W64 | TAN64, 27 | W64 | TAN64, 347 | W64 | TAN64, 1 | W64 | GRAD64 | TAN64, 3 | W64 | GRAD64 | PARAMS64 | TAN64):
            assert val(tw._wdesc(qc, good, N=N)) == L.QC_OK, (N, good)


def _launch(qc, n, m, S, T, wide):
    L = qc._lib
    D = tw._wdesc(qc, wide, N=n // 2, m=m, T=T, cols=1)
    mf, ch, nch = C.c_int32(), C.c_int64(), C.c_int64()
    assert L.lib.qc_sweep_desc_launch(C.byref(D.d), S, C.byref(mf), C.byref(ch), C.byref(nch)) == L.QC_OK, (n, m, S, T, wide)
    return bool(mf.value), ch.value, nch.value


def test_launch_rule_does_not_see_the_bit(qc):
    for n in (16, 32, 34, 48, 54, 64):
        for m in (1, 10, 16, 17):
            for S, T in ((1, 2), (2, 102), (3, 26), (5, 12), (255, 50), (256, 50), (300, 2), (8192, 1000)):
                for base in (1 | W64, 27 | W64, 1 | W64 | GRAD64, 3 | W64 | GRAD64 | PARAMS64):
                    got = _launch(qc, n, m, S, T, base | TAN64)
                    assert got == _launch(qc, n, m, S, T, base), (n, m, S, T, base)
                    want = t64.launch64(n, m, S, T, base)
                    assert got == (want["mfma"], want["chunk"], want["n_chunks"]), (n, m, S, T, base)
    for name, (chunk, n_chunks, last, items) in ITEMS.items():
        state, lv, m, _, _, _, S, T, _, _ = SPECS[name]
        w = t64.launch64(2 * lv, m, S, T, 1 | W64 | TAN64)
        assert w["mfma"] and (w["chunk"], w["n_chunks"], w["last"], S * w["n_chunks"]) == (chunk, n_chunks, last, items), name
    assert t64.launch64(64, 10, 2, 102, 1 | W64)["by_sqrt"]
    for name, spec in SPECS.items():          # the GPU cases are all inside the form
        n = 2 * spec[1] ** 2 if spec[0] == "density" else 2 * spec[1]
        assert 32 < n <= 64 and t64.launch64(n, spec[2], spec[6], spec[7], 1 | W64)["mfma"], name


def _lindblad(qc, wide, N=25, **kw):
    D = too._ODesc(qc, wide=wide, **{**dict(N=N, m=2, cols=1, fid_kind=qc._lib.QC_FID_DENSITY), **kw})
    D.G0[:] = np.random.default_rng(0).standard_normal(D.G0.size)       # not antisymmetric
    return D


def test_other_scope_queries_do_not_see_the_bit(qc):
    """grad, vjp, hvp and noise answer with the bit what they answer without it, text for text: closed, Lindblad and stored-flag
    descriptors, in the form and below it."""
    L = qc._lib
    U = L.QC_FID_UNITARY
    makers = [lambda w, N=N: too._ODesc(qc, wide=w, N=N, m=2, fid_kind=U) for N in (17, 27, 32, 12, 4)]
    makers += [lambda w: too._ODesc(qc, wide=w, N=17, m=2, cols=1, fid_kind=L.QC_FID_KET), lambda w: _lindblad(qc, w), lambda w: _lindblad(qc, w, flag=1),
               lambda w: too._ODesc(qc, wide=w, N=27, m=6, fid_kind=U, flag=1), lambda w: _lindblad(qc, w, N=16), lambda w: too._ODesc(qc, wide=w, N=27, m=17, fid_kind=U)]
    seen = set()
    for make in makers:
        for base in (1 | W64, 347 | W64, 1 | W64 | GRAD64, 1 | W64 | GRAD64 | PARAMS64, 27 | W64 | GRAD64 | PARAMS64):
            for which in QUERIES:
                fn = f"qc_sweep_desc_{which}_supported"
                a, b = too._query(qc, fn, make(base)), too._query(qc, fn, make(base | TAN64))
                assert a[0] == b[0] == L.QC_OK and a[1] == b[1], (which, base)
                if a[1] == 0:
                    assert a[2] == b[2], (which, base, a[2], b[2])
                    seen.add(a[2])
    assert any("which serves the forward sweep only" in s for s in seen) and any("which does not serve" in s for s in seen)
    # today's refusals of what stays refused, word for word, on a descriptor with every mfma64 bit
    D = too._ODesc(qc, wide=1 | W64 | GRAD64 | PARAMS64 | TAN64, N=27, m=6, fid_kind=U)
    assert too._query(qc, "qc_sweep_desc_hvp_supported", D) == (L.QC_OK, 0, "qc_sweep Hessian product: the handle takes the mfma64-sweep form (2N = 54), which does not serve Hessian products")
    assert too._query(qc, "qc_sweep_desc_noise_supported", D) == (L.QC_OK, 0, "qc_sweep noise: the handle takes the mfma64-sweep form (2N = 54), which does not serve noise trajectories")
    D = too._ODesc(qc, wide=1 | W64 | GRAD64 | TAN64, N=27, m=6, fid_kind=U, flag=1)
    rc, ok, text = too._query(qc, "qc_sweep_desc_grad_supported", D)
    assert (rc, ok) == (L.QC_OK, 0) and "the mfma64-sweep form (2N = 54), which does not serve stored-state gradients" in text
    D = too._ODesc(qc, wide=1 | W64 | TAN64, N=27, m=6, fid_kind=U)
    assert too._query(qc, "qc_sweep_desc_grad_supported", D)[2].endswith("the handle takes the mfma64-sweep form (2N = 54), which serves the forward sweep only")


def test_jvp_scope_follows_the_bit(qc):
    L = qc._lib
    U = L.QC_FID_UNITARY
    q = lambda D: too._query(qc, "qc_sweep_desc_jvp_supported", D)
    for base in (1 | W64, 27 | W64, 1 | W64 | GRAD64, 3 | W64 | GRAD64 | PARAMS64):
        for N in (17, 27, 32):
            assert q(too._ODesc(qc, wide=base | TAN64, N=N, m=2, fid_kind=U))[:2] == (L.QC_OK, 1), (base, N)
        assert q(_lindblad(qc, base | TAN64))[:2] == (L.QC_OK, 1)                                         # N = 25 Lindblad, density fidelity
        assert q(_lindblad(qc, base | TAN64, flag=1))[:2] == (L.QC_OK, 1)                                 # the flag is not looked at
        assert q(too._ODesc(qc, wide=base | TAN64, N=17, m=2, cols=33))[:2] == (L.QC_OK, 1)               # more columns than reverse mode's 32
        assert q(too._ODesc(qc, wide=base | TAN64, N=18, m=1, cols=3))[:2] == (L.QC_OK, 1)                # no fidelity
        assert q(too._ODesc(qc, wide=base | TAN64, N=32, m=16, fid_kind=U))[:2] == (L.QC_OK, 1)           # ns = 2048 exactly, the drive limit
        assert q(too._ODesc(qc, wide=base | TAN64, N=32, m=2, cols=32))[:2] == (L.QC_OK, 1)
        assert q(too._ODesc(qc, wide=base | TAN64, N=17, m=2, cols=60))[:2] == (L.QC_OK, 1)               # ns = 2040
        rc, ok, text = q(too._ODesc(qc, wide=base | TAN64, N=17, m=2, cols=61))                           # ns = 2074
        assert (rc, ok) == (L.QC_OK, 0), base
        assert text.startswith("qc_sweep pushforward: the handle takes the mfma64-sweep form (2N = 34)") and "2048" in text and "ns = 2N x state_cols = 2074" in text, text
        rc, ok, text = q(too._ODesc(qc, wide=base | TAN64, N=32, m=2, cols=33))                           # ns = 2112
        assert (rc, ok) == (L.QC_OK, 0) and "2N = 64" in text and "= 2112" in text, text
    # without the bit: today's two texts
    for N in (17, 27):
        for cols in (0, 61):
            fwd = f"qc_sweep pushforward: the handle takes the mfma64-sweep form (2N = {2 * N}), which serves the forward sweep only"
            uns = f"qc_sweep pushforward: the handle takes the mfma64-sweep form (2N = {2 * N}), which does not serve pushforwards"
            for base in (1 | W64, 27 | W64, 347 | W64):
                assert q(too._ODesc(qc, wide=base, N=N, m=2, cols=cols)) == (L.QC_OK, 0, fwd), (N, base)
            for base in (1 | W64 | GRAD64, 17 | W64 | GRAD64 | PARAMS64):
                assert q(too._ODesc(qc, wide=base, N=N, m=2, cols=cols)) == (L.QC_OK, 0, uns), (N, base)
    # more than 16 drives: the per-sample form, whatever the bit
    rc, ok, text = q(too._ODesc(qc, wide=1 | W64 | TAN64, N=27, m=17, fid_kind=U))
    assert (rc, ok) == (L.QC_OK, 0) and text == "qc_sweep pushforward: the handle takes the rollout-per-sample form (17 drives > 16)"
    # 2N <= 32 never looks at the bit
    for N, cols in ((12, 0), (16, 128), (4, 0), (8, 17)):
        for base in (1 | W64, 17 | W64, 27 | W64 | GRAD64):
            assert q(too._ODesc(qc, wide=base, N=N, m=2, cols=cols)) == q(too._ODesc(qc, wide=base | TAN64, N=N, m=2, cols=cols)), (N, base)
    assert q(too._ODesc(qc, wide=1 | W64 | TAN64, N=12, m=2))[:2] == (L.QC_OK, 0) and q(too._ODesc(qc, wide=17 | W64 | TAN64, N=12, m=2))[:2] == (L.QC_OK, 1)
    assert q(too._ODesc(qc, wide=TAN64 | 1, N=17, m=2))[0] == L.QC_ERR_INVALID


def test_constants_abi_keywords_and_texts(qc, tmp_path):
    L = qc._lib
    header = open(os.path.join(ROOT, "include", "qcolloc.h")).read()
    assert re.search(r"^#define QC_SWEEP_WIDE_64_TANGENT 16384\b", header, re.M)
    assert "Bit 14, QC_SWEEP_WIDE_64_TANGENT" in header and "qc_sweep64_jvp.hip" in header
    src = tmp_path / "t64.c"
    src.write_text('#include <stdio.h>\n#include "qcolloc.h"\nint main(){printf("%zu %d\\n", sizeof(qc_sweep_desc), QC_SWEEP_WIDE_64_TANGENT);return 0;}\n')
    exe = tmp_path / "t64"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [128, 16384]
    assert L.lib.qc_sizeof_sweep_desc() == C.sizeof(L.qc_sweep_desc) == 128 and L.lib.qc_abi_version() == 6
    # no new entry point, no exported symbol of the form
    names = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "qc_sweep_jvp" in names and "sweep64" not in names
    assert not any("sweep64" in name for name in L.SYMBOLS)
    makefile = open(os.path.join(ROOT, "quantumcollocation.jl_amd", "csrc", "Makefile")).read()
    assert "qc_sweep64_jvp.hip" in makefile and "qc_sweep64_jvp.o" in makefile
    julia = open(os.path.join(ROOT, "julia", "QCollocHIP.jl"), encoding="utf-8").read()
    assert re.search(r"^const QC_SWEEP_WIDE_64_TANGENT = 16384\b", julia, re.M)
    push = julia[julia.index("function rollout_sweep_pushforward("):]
    push = push[:push.index("\nend\n")]
    assert "wide64::Bool=false" in push and "wide64_tangent::Bool=false" in push and "QC_SWEEP_WIDE_64_TANGENT" in push
    assert "wide64_tangent = true needs wide64 = true" in push and "wide ? (QC_SWEEP_WIDE | QC_SWEEP_WIDE_TANGENT) : 0" in push
    assert "the `wide64_tangent` path was not run" in julia
    design = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    assert "5.8.14" in design and "qc_sweep64_jvp.hip" in design and "qc_sweep64_jvp_finish_kernel" in design and "QC_SWEEP_WIDE_64_TANGENT" in design
    readme = open(os.path.join(ROOT, "README.md"), encoding="utf-8").read()
    assert "qc_sweep64_jvp.hip" in readme and "wide64_tangent" in readme
    kernel = open(os.path.join(ROOT, "quantumcollocation.jl_amd", "csrc", "qc_sweep64_jvp.hip")).read()
    assert "Barriers of one interval" in kernel and "qc_sweep64_jvp_kernel" in kernel


def test_python_keywords(qc):
    for f in (qc.RolloutSweep.__init__, qc.SweepFinalStateObjective.__init__):
        names = list(inspect.signature(f).parameters)
        par = inspect.signature(f).parameters
        assert par["wide64_tangent"].default is False, f
        assert names[-2:] == ["wide64_tangent", "wide64_params"] and names[-3] == "wide64_grad", (f, names[-4:])
    for word in ("wide64_tangent", "2048"):
        assert word in qc.RolloutSweep.__doc__
    assert "wide64_tangent" in qc.SweepFinalStateObjective.__doc__
    # refused before the library is touched: no system is looked at
    for kw in (dict(), dict(wide=True), dict(wide=True, wide_tangent=True)):
        with pytest.raises(ValueError, match="wide64_tangent=True needs wide64=True"):
            qc.RolloutSweep(None, [], 5, wide64_tangent=True, **kw)
    with pytest.raises(ValueError, match="wide64=True needs wide=True"):
        qc.RolloutSweep(None, [], 5, wide64=True, wide64_tangent=True)


def test_reference_routes_agree_at_17_levels(qc):
    """expm_frechet along the recurrence against the complex step through expm on the 17-level case of five chunks (two samples):
    1e-11 max(1, max |want|), and tangents that a zero could not pass for."""
    c = build(qc, "n17-S3-T26")
    samples = [0, c["S"] - 1]
    args = (c["G0"], c["Gd"], c["Gp"], c["controls"], c["dts"], c["init"], c["theta"], c["scale"], samples)
    kw = dict(vcontrols=c["vcontrols"], vdts=c["vdts"], vinit=c["vinit"], vtheta=c["vtheta"], vscale=c["vscale"], fid=c["fid"])
    a, b = jref.pushforward_frechet(*args, **kw), jref.pushforward_complex_step(*args, **kw)
    for key in ("finals", "tfinals", "tfids"):
        err = np.abs(a[key] - b[key]).max() / max(1.0, np.abs(a[key]).max())
        print(f"SWEEP-WIDE64-JVP reference n17-S3-T26 {key}: frechet vs complex step {err:.2e}, max |value| {np.abs(a[key]).max():.3e}")
        assert err <= 1e-11 and np.abs(a[key]).max() > 1e-3, key


# ---------------------------------------------------------------------------------------------------------------------------------
#  GPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SPECS))
def test_wide64_jvp_matches_the_reference(qc, name):
    """Every requested value of every sample against the Frechet route along the full direction, and the bit-level properties of
    test_sweep_jvp.check_case: finals / fids are `eval`'s, a second call, each output alone, a NULL direction against zeros, the host
    entry point, a side stream, NaNs in the unread entries of vZ."""
    c = build(qc, name)
    sw = handle(qc, c)
    try:
        assert sw.kernel_name == "mfma64-sweep" and sw.wide64_tangent and sw.jvp_supported and sw.jvp_unsupported_reason is None
        assert not sw.hvp_supported and not sw.grad_supported and 32 < c["n"] <= 64 and sw.ns <= NS_MAX
        want = t64.launch64(c["n"], c["m"], c["S"], c["T"], 1 | W64)
        assert sw.launch(c["S"]) == (True, want["chunk"], want["n_chunks"])
        if name in ITEMS:
            assert (want["chunk"], want["n_chunks"], want["last"], c["S"] * want["n_chunks"]) == ITEMS[name]
        if name == "n32-S2-T102":
            assert want["by_sqrt"] and sw.ns == NS_MAX and (4 * sw.ns + 8192) * 8 == 128 * 1024
        if name == "n17-cols33":
            assert sw.cols == 33 and sw.ns == 34 * 33
        if name == "lindblad25":
            assert c["n"] == 50 and np.abs(c["G0"] + c["G0"].T).max() > 0.05
        if name == "squarings":
            sq = _squaring_counts(c)
            print(f"SWEEP-WIDE64-JVP squarings: counts {sorted(set(sq))}")
            assert min(sq) == 0 and max(sq) >= 8 and len(set(sq)) >= 5, sq
        out, dirs = tj.check_case(sw, c)
        assert set(dirs) == {k for k, v in (("vZ", 1), ("vinit", 1), ("vtheta", c["p"]), ("vscale", c["m"])) if v}
        # a handle made without the bit: the same finals / fids, bit for bit
        plain = ts.make_sweep(qc, c, wide=True, wide64=True)
        try:
            finals, fids = plain.eval(sw.pack(c["controls"], c["dts"]), c["init"], c["theta"], c["scale"], fids=c["kind"] is not None)
        finally:
            plain.close()
        np.testing.assert_array_equal(out["finals"], finals.T)
        if c["kind"] is not None:
            np.testing.assert_array_equal(out["fids"], fids)
            r = tj.reference(c)
            rfid = ref.fidelities(r["finals"].T, c["kind"], c["goal"], c["L"], c["subspace"], c["form"])
            print(f"SWEEP-WIDE64-JVP {name} fids: worst error / bound = {np.abs(out['fids'][c['samples']] - rfid).max() / ts.FID_ATOL:.3e}")
            ts._assert_fids(out["fids"][c["samples"]], rfid, name)
    finally:
        sw.close()


@pytest.mark.gpu
def test_zero_generators_give_vinit(qc):
    """Zero drift, drives and perturbation: E = I and Edot = 0 exactly, so finals are init and tfinals are vinit, bit for bit, whatever
    the direction."""
    N, T, S, m = 20, 9, 5, 2
    rng = np.random.default_rng(N)
    zsys = qc.QuantumSystem(np.zeros((N, N)), [np.zeros((N, N))] * m)
    sw = qc.RolloutSweep(zsys, [np.zeros((N, N))], T, wide=True, wide64=True, wide64_tangent=True)
    try:
        assert sw.kernel_name == "mfma64-sweep"
        init, vinit = ref.operator_to_iso_vec(_unitary(rng, N)), rng.standard_normal(sw.ns)
        Z, vZ = sw.pack(rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T)), rng.standard_normal(sw.Z_len)
        theta = rng.uniform(-1, 1, (S, 1))
        c = dict(S=S, init=init, theta=theta, scale=None)
        out = tj.device_call(sw, Z, c, ("finals", "tfinals"), dict(vZ=vZ, vinit=vinit, vtheta=rng.standard_normal((S, 1)), vscale=rng.standard_normal((S, m))))
    finally:
        sw.close()
    np.testing.assert_array_equal(out["finals"], np.repeat(init[None], S, axis=0))
    np.testing.assert_array_equal(out["tfinals"], np.repeat(vinit[None], S, axis=0))
    print("SWEEP-WIDE64-JVP zero generators: finals = init and tfinals = vinit (bound: 0 differing bits)")


@pytest.mark.gpu
def test_bits_with_scratch_that_grows_and_shrinks(qc):
    """A handle whose S goes 3 -> 100 -> 7 returns the bits of a fresh handle at every S (`dTotJ`: S x n_chunks x 8192 doubles, grown
    on demand, with other chunk counts and strides), six repeated calls included."""
    c = build(qc, "n17-S3-T12")
    rng = np.random.default_rng(8)
    sw = handle(qc, c)
    try:
        Z = sw.pack(c["controls"], c["dts"])
        vZ = sw.pack(c["vcontrols"], c["vdts"])
        for i, S in enumerate((3, 100, 7)):
            cs = dict(S=S, init=c["init"], theta=rng.uniform(-0.3, 0.3, (S, 1)), scale=rng.uniform(0.9, 1.1, (S, c["m"])))
            dirs = dict(vZ=vZ, vinit=c["vinit"], vtheta=rng.standard_normal((S, 1)), vscale=rng.standard_normal((S, c["m"])))
            fresh = handle(qc, c)
            try:
                want = tj.device_call(fresh, Z, cs, tj.OUTPUTS, dirs)
            finally:
                fresh.close()
            for _ in range(6 if i == 1 else 1):
                got = tj.device_call(sw, Z, cs, tj.OUTPUTS, dirs)
                for k in tj.OUTPUTS:
                    np.testing.assert_array_equal(got[k], want[k], err_msg=f"{k} at S = {S}")
            assert np.isfinite(want["tfinals"]).all() and np.abs(want["tfinals"][0] - want["tfinals"][-1]).max() > 1e-6
        print("SWEEP-WIDE64-JVP bits: S = 3 -> 100 -> 7 on one handle against fresh handles, six repeated calls (bound: 0 differing bits)")
    finally:
        sw.close()


@pytest.mark.gpu
def test_isolation_of_a_non_finite_direction(qc):
    """A NaN in vtheta[1] (then in vscale[1]) makes only sample 1's tangents non-finite; no finals / fids bit changes anywhere and no
    tangent of another sample."""
    c = build(qc, "n17-S3-T12")
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
        print("SWEEP-WIDE64-JVP isolation: a NaN in one sample's vtheta / vscale reaches that sample's tangents only (bound: 0 differing bits elsewhere)")
    finally:
        sw.close()


def _columns_case(qc, cols):
    """17 levels, S = 3, T = 12 (chunks 3, 3, 3, 2) with `cols` ket columns and no fidelity."""
    c = build(qc, "n17-S3-T12")
    rng = np.random.default_rng(70 + cols)
    if cols != 17:
        K = rng.standard_normal((17, cols)) + 1j * rng.standard_normal((17, cols))
        K /= np.linalg.norm(K, axis=0)
        c["init"], c["cols"] = ref.operator_to_iso_vec(K), cols
        c["vinit"] = rng.standard_normal(c["init"].size) / np.sqrt(c["init"].size)
        c["goal"] = c["kind"] = c["subspace"] = c["form"] = c["fid"] = None
    return c


@pytest.mark.gpu
@pytest.mark.parametrize("cols", [1, 8, 17])
def test_adjoint_identity_with_the_wide64_pullback(qc, cols):
    """<cot_s, tfinals[s]> = <vjp(cot)_s, v> over all four direction parts for every sample, on a closed handle with bits 11, 13 and 14."""
    c = _columns_case(qc, cols)
    sw = handle(qc, c, wide64_grad=True, wide64_params=True)
    try:
        assert sw._desc.wide == 1 | W64 | GRAD64 | PARAMS64 | TAN64 and sw.vjp_supported and sw.jvp_supported and sw.cols == cols
        twj._adjoint_identity(sw, c, f"mfma64-sweep, {cols} columns")
    finally:
        sw.close()


@pytest.mark.gpu
def test_finals_autograd_forward_mode_on_a_wide64_handle(qc):
    """Under forward_ad the tangent of `finals_autograd` is `jvp_device`'s tfinals, bit for bit, for tangents on Z, init and theta, and
    the full tangent is the Frechet reference's to 1e-9."""
    import torch.autograd.forward_ad as fwAD
    c = build(qc, "n17-S3-T12")
    sw = handle(qc, c)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    S = c["S"]
    try:
        Z, init, theta, scale = t(sw.pack(c["controls"], c["dts"])), t(c["init"]), t(c["theta"]), t(c["scale"])
        vZ, vinit, vtheta = t(sw.pack(c["vcontrols"], c["vdts"])), t(c["vinit"]), t(c["vtheta"])
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
        r = jref.pushforward_frechet(c["G0"], c["Gd"], c["Gp"], c["controls"], c["dts"], c["init"], c["theta"], c["scale"], range(S),
                                     vcontrols=c["vcontrols"], vdts=c["vdts"], vinit=c["vinit"], vtheta=c["vtheta"])
        tj.assert_samples(tangent.cpu().numpy(), r["tfinals"], "wide64 forward-mode tangent of finals_autograd")
    finally:
        sw.close()


@pytest.mark.gpu
def test_gauss_newton_product_on_a_wide64_handle(qc):
    """`gauss_newton_times` on 17 levels (T = 3, S = 2) with loss = sum ||X - G||^2 / (2 S) against J^T J v / S assembled on the CPU from
    the Frechet route over the unit directions: 1e-9; symmetry; `hessian_times` raises the handle's `hvp` reason."""
    rng = np.random.default_rng(41)
    N, m, T, S = 17, 2, 3, 2
    traj = tv._traj3(qc, rng, N, m, T)
    H0, Hd, P = _herm(rng, N), [_herm(rng, N, 0.5) for _ in range(m)], _herm(rng, N)
    sys_ = qc.QuantumSystem(H0, Hd)
    theta, scale = rng.uniform(-0.2, 0.2, (S, 1)), rng.uniform(0.9, 1.1, (S, m))
    goal = torch.from_numpy(np.ascontiguousarray(traj.goal["Ũ⃗"])).cuda()
    loss = lambda X: ((X - goal) ** 2).sum() / (2 * S)
    obj = qc.SweepFinalStateObjective(traj, sys_, [P], theta, loss, scale=scale, wide=True, wide64=True, wide64_grad=True, wide64_tangent=True)
    Z = traj.datavec
    nZ = Z.size
    try:
        assert obj._sweep.wide64_tangent and obj._sweep.kernel_name == "mfma64-sweep"
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
        print(f"SWEEP-WIDE64-JVP gauss_newton_times vs J^T J v / S: error / bound = {err / 1e-9:.3e} (bound 1e-9), max |value| {np.abs(want).max():.3f}")
        assert err <= 1e-9 and np.abs(want).max() > 1e-3
        gu = obj.gauss_newton_times(Z, u)
        assert abs(u @ got - v @ gu) <= 1e-9 * abs(u @ got) and abs(u @ got) > 1e-3
        dgot = obj.gauss_newton_times(torch.from_numpy(Z).cuda(), torch.from_numpy(v).cuda())
        assert torch.is_tensor(dgot) and dgot.is_cuda
        np.testing.assert_array_equal(dgot.cpu().numpy(), got)
        with pytest.raises(qc.QCollocError) as e:
            obj.hessian_times(Z, v)
        assert e.value.code == qc._lib.QC_ERR_UNSUPPORTED and "the mfma64-sweep form (2N = 34), which does not serve Hessian products" in str(e.value)
    finally:
        obj.close()
    # without the tangent bit the product raises the pushforward's reason, as it did
    obj = qc.SweepFinalStateObjective(traj, sys_, [P], theta, loss, scale=scale, wide=True, wide64=True, wide64_grad=True)
    try:
        with pytest.raises(qc.QCollocError) as e:
            obj.gauss_newton_times(Z, np.ones(nZ))
        assert e.value.code == qc._lib.QC_ERR_UNSUPPORTED and "the mfma64-sweep form (2N = 34), which does not serve pushforwards" in str(e.value)
    finally:
        obj.close()


@pytest.mark.gpu
def test_refusals_are_unchanged(qc):
    """Without the bit an "mfma64-sweep" handle refuses the pushforward in its two old texts; with it, Hessian products, noise sweeps and
    (without bit 11) gradients keep refusing, above ns = 2048 the pushforward refuses with the new reason, and `eval` returns the same bits."""
    L = qc._lib
    UNS = L.QC_ERR_UNSUPPORTED
    c = build(qc, "n17-S3-T12")
    plain = ts.make_sweep(qc, c, wide=True, wide64=True)
    grad = ts.make_sweep(qc, c, wide=True, wide64=True, wide64_grad=True)
    tan = handle(qc, c)
    try:
        Z = plain.pack(c["controls"], c["dts"])
        for h, old in ((plain, "qc_sweep pushforward: the handle takes the mfma64-sweep form (2N = 34), which serves the forward sweep only"),
                       (grad, "qc_sweep pushforward: the handle takes the mfma64-sweep form (2N = 34), which does not serve pushforwards")):
            assert not h.jvp_supported and h.jvp_unsupported_reason == old and not h.wide64_tangent
            with pytest.raises(qc.QCollocError) as e:
                h.jvp(Z, c["init"], np.zeros(h.Z_len), c["theta"], c["scale"])
            assert e.value.code == UNS and old in str(e.value)
            rc, msg = tj._raw(qc, h)
            assert rc == UNS and msg == old
        assert tj._raw(qc, tan)[0] == L.QC_OK
        with pytest.raises(qc.QCollocError) as e:
            tan.hvp(Z, c["init"], np.zeros((c["S"], tan.ns)), c["theta"], c["scale"], vZ=np.zeros(tan.Z_len))
        assert e.value.code == UNS and "mfma64-sweep form (2N = 34), which serves the forward sweep only" in str(e.value)
        with pytest.raises(qc.QCollocError) as e:
            tan.noise_eval(Z, c["init"], np.zeros((c["S"], c["T"] - 1, 1)), c["theta"], c["scale"])
        assert e.value.code == UNS and "mfma64-sweep form (2N = 34), which serves the forward sweep only" in str(e.value)
        with pytest.raises(qc.QCollocError) as e:
            tan.grad(Z, c["init"], c["theta"], c["scale"])
        assert e.value.code == UNS and "mfma64-sweep form (2N = 34), which serves the forward sweep only" in str(e.value)
        fa, fb = plain.eval(Z, c["init"], c["theta"], c["scale"]), tan.eval(Z, c["init"], c["theta"], c["scale"])
        np.testing.assert_array_equal(fa[0], fb[0])
        np.testing.assert_array_equal(fa[1], fb[1])
        assert plain.kernel_name == tan.kernel_name == "mfma64-sweep" and plain.launch(c["S"]) == tan.launch(c["S"])
    finally:
        for h in (plain, grad, tan):
            h.close()
    # 17 levels with 61 ket columns: ns = 2074, past the finish kernel's bound; the forward sweep is served
    big = _columns_case(qc, 61)
    sw = handle(qc, big)
    try:
        why = sw.jvp_unsupported_reason
        assert not sw.jvp_supported and "mfma64-sweep form (2N = 34)" in why and "ns = 2N x state_cols = 2074" in why
        rc, msg = tj._raw(qc, sw)
        assert rc == UNS and msg == why
        finals, _ = sw.eval(sw.pack(big["controls"], big["dts"]), big["init"], big["theta"], big["scale"], fids=False)
        assert np.isfinite(finals).all()
    finally:
        sw.close()


@pytest.mark.gpu
def test_three_transmon_gauss_newton_example(qc):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import three_transmon_gauss_newton
    out = three_transmon_gauss_newton.main(verbose=False)
    hist = out["loss_history"]
    print(f"SWEEP-WIDE64-JVP example: loss {hist[0]:.6e} -> {hist[-1]:.6e} in {out['accepted']} accepted steps, {out['gn_products']} Gauss-Newton products")
    assert out["kernel"] == "mfma64-sweep"
    assert len(hist) == out["accepted"] + 1 >= 2
    assert all(b <= a for a, b in zip(hist, hist[1:])) and hist[-1] < hist[0]
