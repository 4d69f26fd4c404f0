"""Sweep gradients and pullbacks in the "mfma64-sweep" form (32 < 2N <= 64): `qc_sweep_desc.wide = QC_SWEEP_WIDE | QC_SWEEP_WIDE_64 |
QC_SWEEP_WIDE_64_GRAD` (3073), `RolloutSweep(..., wide=True, wide64=True, wide64_grad=True)`, the closed adjoint walk of
csrc/qc_sweep64_grad.hip behind the seeds at ld = 64.  CPU: the descriptor field, the device-free scope queries, the unchanged launch rule,
keywords and texts.  GPU: every value of `grad_samples` against `sweep_grad_reference.grad_samples_forward` (pullbacks:
`sweep_vjp_reference.pullback_forward`) at the smallest shapes at which tiling, padding, the column tiles, chunking and squaring can go
wrong; fidelities and final states bit for bit against `eval`; bits; refusals; non-finite input; the example.

Tolerances are the project's: per sample |got - want| <= 1e-9 max(1, max |grad F_s|) (test_sweep_grad._assert_samples,
test_sweep_vjp.assert_samples), states rtol 1e-10 / atol 1e-11.  The truncation bound of the once-differentiated series (1.7e-12, header
of csrc/qc_sweep_grad.hip) does not depend on the size.  Every sample of launches of 250 .. 300 workgroups:
tests/test_sweep_wide64_grad_every_sample.py.  Measured values: profiles/sweep_wide64_grad_summary.txt.

Two cases cannot be put to the fidelity reference as named: a unitary fidelity needs all N columns and a ket fidelity one, so
  * "transmons27-sub8" is the full 27-column unitary with the fidelity on the 8 computational levels (the 8-column state is the pullback's
    case of the same name), and
  * "levels20-nc17" (17 of 20 columns: no fidelity is defined) is checked through the pullback against `pullback_forward`; 17 live columns
    under a fidelity are the N = 17 unitaries of the squaring cases.
"no-drives-p0": `grad_samples_forward` cannot reshape an empty control matrix, so its reference is taken with one zero drive generator at
zero amplitude, whose column is dropped (it changes no generator)."""
import ctypes as C
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sweep_reference as ref
import sweep_vjp_reference as vref
import test_sweep as ts
import test_sweep_grad as tg
import test_sweep_vjp as tv
import test_sweep_wide as tw
import test_sweep_wide64 as t64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_herm, _unitary = ts._herm, ts._unitary
W64, WG = t64.W64, 2048
WIDE = 1 | W64 | WG          # 3073
HANDLE = dict(wide=True, wide64=True, wide64_grad=True)
QUERIES = t64.QUERIES
SUB8 = [9 * a + 3 * b + c for a in (0, 1) for b in (0, 1) for c in (0, 1)]      # the computational levels of three three-level transmons
U, KET = ("unitary", None, "abs"), ("ket", None, "abs")

# name: (state, levels, m, p, scale given, free timestep, S, T, fidelity, samples) -- the tuple test_sweep_wide.build reads
GRAD_CASES64 = {
    "levels17-ket": ("ket", 17, 2, 1, False, True, 11, 6, KET, None),                                  # heaviest padding, one column
    "transmons27-sub8": ("unitary", 27, 6, 1, True, True, 5, 12, ("unitary", SUB8, "abs"), None),      # several chunks, second column tile partly live
    "levels32-unitary": ("unitary", 32, 3, 1, True, False, 3, 5, ("unitary", None, "abs2"), None),     # full tiles, full column count, fixed timestep
    "levels32-m16": ("unitary", 32, 16, 0, True, True, 2, 3, U, None),                                 # the drive limit
    "no-drives-p0": ("unitary", 17, 0, 0, False, True, 3, 4, U, None),                                 # only the timestep's derivative
    "one-interval": ("ket", 17, 2, 1, True, True, 3, 2, KET, None),                                    # T = 2
    "one-chunk": ("ket", 17, 2, 1, True, True, 256, 3, KET, (0, 100, 255)),                            # S at the fill constant
    "sqrt-capped": ("ket", 17, 2, 1, True, True, 2, 102, KET, None),                                   # 11 chunks of 10, the last of 1
}
# the pullback's cases: (the tuple above with a three-ket state, the number of state columns it is rebuilt with)
VJP_CASES64 = {
    "transmons27-sub8": (("kets3", 27, 6, 1, True, True, 5, 12, None, None), 8),
    "levels17-ket": (("kets3", 17, 2, 1, False, True, 11, 6, None, None), 1),
    "levels20-nc17": (("kets3", 20, 2, 1, True, True, 3, 5, None, None), 17),                          # the second column tile holds one live column
}
_CASES, _REF = {}, {}


def _case(qc, name):
    if name not in _CASES:
        _CASES[name] = tw.build(qc, name, GRAD_CASES64[name])
    return _CASES[name]


def _reference(c):
    """`grad_samples_forward` of the case's checked samples: computed once, shared, never written to."""
    if c["name"] not in _REF:
        r = c
        if c["m"] == 0:      # see the header: one zero drive at zero amplitude, its column dropped
            r = dict(c, Gd=[np.zeros_like(c["G0"])], controls=np.zeros((1, c["T"])))
        want = tg.reference(r)
        want = want[:, :, 1:] if c["m"] == 0 else want
        want.setflags(write=False)
        _REF[c["name"]] = want
    return _REF[c["name"]]


def _vjp_case(qc, name):
    """A case without a fidelity whose state has `cols` columns (test_sweep_wide.build makes one or three), with unit cotangents."""
    key = "vjp/" + name
    if key not in _CASES:
        spec, cols = VJP_CASES64[name]
        c = tw.build(qc, key, spec)
        rng = np.random.default_rng(11 + sum(map(ord, name)))
        K = rng.standard_normal((c["L"], cols)) + 1j * rng.standard_normal((c["L"], cols))
        c["init"], c["cols"] = ref.operator_to_iso_vec(K / np.linalg.norm(K, axis=0)), cols
        c["cot"] = tv.unit_cotangents(rng, c["S"], c["init"].size)
        _CASES[key] = c
    return _CASES[key]


def _vjp_reference(c):
    if c["name"] not in _REF:
        out = vref.pullback_forward(c["G0"], c["Gd"], c["Gp"], c["controls"], c["dts"], c["init"], c["theta"], c["scale"], c["samples"], c["cot"])
        for a in out.values():
            a.setflags(write=False)
        _REF[c["name"]] = out
    return _REF[c["name"]]


# ---------------------------------------------------------------------------------------------------------------------------------
#  CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_wide64_grad_field_is_validated(qc):
    L = qc._lib
    val = lambda D: L.lib.qc_sweep_desc_validate(C.byref(D.d))
    today = t64._valid_today()
    assert len(today) == 33 and L.QC_SWEEP_WIDE_64_GRAD == WG == 1 << 11
    for N in (20, 12, 2):
        for v in today:
            assert val(tw._wdesc(qc, v, N=N)) == L.QC_OK, (N, v)
            if v:
                assert val(tw._wdesc(qc, v | W64, N=N)) == L.QC_OK, (N, v | W64)
                assert val(tw._wdesc(qc, v | W64 | WG, N=N)) == L.QC_OK, (N, v | W64 | WG)
                assert val(tw._wdesc(qc, v | WG, N=N)) == L.QC_ERR_INVALID, (N, v | WG)          # bit 11 without bit 10
        for bad in (2048, 2049, 2050, 3072, (1 << 20) | 3073, 1024, 4096 | 3073, 512 | 3073):
            assert val(tw._wdesc(qc, bad, N=N)) == L.QC_ERR_INVALID, (N, bad)
            text = L.lib.qc_sweep_last_error(None).decode()
            assert text.startswith("qc_sweep: wide"), text
            for words in ("17, 19, 25 or 27", "QC_SWEEP_WIDE_TANGENT (16)", "QC_SWEEP_WIDE_NOISE (64)", "QC_SWEEP_WIDE_HESSIAN (256)",
                          "QC_SWEEP_WIDE_64 (1024)", "QC_SWEEP_WIDE_64_GRAD (2048)"):
                assert words in text, (words, text)
    ok = C.c_int32(-1)
    assert L.lib.qc_sweep_desc_grad_supported(C.byref(tw._wdesc(qc, 2049, N=20).d), C.byref(ok)) == L.QC_ERR_INVALID
    assert L.lib.qc_sweep_desc_launch(C.byref(tw._wdesc(qc, 3072, N=20).d), 5, None, None, None) == L.QC_ERR_INVALID


def _desc(qc, wide, stored=0, lindblad=False, **kw):
    D = tg._GDesc(qc, **kw)
    if lindblad:
        D.G0[:] = np.random.default_rng(0).standard_normal(D.G0.size)
    D.d.wide = wide
    D.d.reserved1[0] = stored
    return D


def test_wide64_grad_scope_queries(qc):
    L = qc._lib
    Uk = L.QC_FID_UNITARY
    served = (dict(N=27, m=6, fid_kind=Uk), dict(N=17, m=2, cols=1, fid_kind=L.QC_FID_KET), dict(N=32, m=16, fid_kind=Uk))
    for wide in (WIDE, WIDE | 346):          # the other bits are the mfma32-sweep form's: nothing here reads them
        for kw in served:
            for which in ("grad", "vjp"):
                assert t64._query(qc, which, _desc(qc, wide, **kw)) == (L.QC_OK, 1, None), (which, wide, kw)
            for which, word in (("jvp", "pushforwards"), ("hvp", "Hessian products"), ("noise", "noise trajectories")):
                rc, ok, text = t64._query(qc, which, _desc(qc, wide, **kw))
                assert (rc, ok) == (L.QC_OK, 0), (which, kw)
                assert "mfma64-sweep" in text and f"2N = {2 * kw['N']}" in text and word in text and "forward sweep only" not in text, text
            # the stored-state flag: refused, naming the form
            for which in ("grad", "vjp"):
                rc, ok, text = t64._query(qc, which, _desc(qc, wide, stored=1, **kw))
                assert (rc, ok) == (L.QC_OK, 0) and "mfma64-sweep" in text and f"2N = {2 * kw['N']}" in text and "stored-state" in text, text
    # the pullback asks for no fidelity; the gradient does
    D = _desc(qc, WIDE, N=20, m=2, cols=17)
    assert t64._query(qc, "vjp", D)[:2] == (L.QC_OK, 1)
    rc, ok, text = t64._query(qc, "grad", D)
    assert (rc, ok) == (L.QC_OK, 0) and "no fidelity" in text
    D = _desc(qc, WIDE, N=17, m=2, cols=33)
    rc, ok, text = t64._query(qc, "vjp", D)
    assert (rc, ok) == (L.QC_OK, 0) and "32 columns" in text and "mfma64-sweep" in text and "2N = 34" in text
    assert t64._query(qc, "vjp", _desc(qc, WIDE, N=17, m=2, cols=32))[:2] == (L.QC_OK, 1)
    # a Lindblad generator of five levels: not antisymmetric, with the reason of the smaller forms
    for which in ("grad", "vjp"):
        rc, ok, text = t64._query(qc, which, _desc(qc, WIDE, lindblad=True, N=25, m=2, cols=1, fid_kind=L.QC_FID_DENSITY))
        assert (rc, ok) == (L.QC_OK, 0) and "G_drift is not antisymmetric" in text, text
    # more than 16 drives: the per-sample form, and said so
    for which in QUERIES:
        rc, ok, text = t64._query(qc, which, _desc(qc, WIDE, N=27, m=17, fid_kind=Uk))
        assert (rc, ok) == (L.QC_OK, 0) and "rollout-per-sample" in text and "17 drives" in text, (which, text)
    # without bit 11: today's answers and texts
    for which in QUERIES:
        rc, ok, text = t64._query(qc, which, _desc(qc, 1 | W64, N=27, m=6, fid_kind=Uk))
        assert (rc, ok) == (L.QC_OK, 0) and "which serves the forward sweep only" in text, (which, text)
    # 2N <= 32: every answer and every text is that of the descriptor without bit 11
    variants = [(kw, False, 0) for kw in (dict(N=12, m=2, fid_kind=Uk), dict(N=4, m=2, p=2, fid_kind=Uk), dict(N=16, m=8, p=1, cols=1, fid_kind=L.QC_FID_KET),
                                          dict(N=12, m=9, fid_kind=Uk), dict(N=12, m=2), dict(N=12, m=2, cols=17))]
    for kw in (dict(N=16, m=2, cols=1, fid_kind=L.QC_FID_DENSITY), dict(N=4, m=2, cols=1, fid_kind=L.QC_FID_DENSITY)):
        variants += [(kw, True, 0), (kw, True, 1)]
    variants.append((dict(N=12, m=2, fid_kind=Uk), False, 1))
    for kw, lindblad, stored in variants:
        for wide in (1, 3, 9, 11, 17, 65, 257, 347):
            answers = [[t64._query(qc, which, _desc(qc, wide | W64 | bit, stored, lindblad, **kw)) for which in QUERIES] for bit in (0, WG)]
            assert answers[0] == answers[1], (kw, lindblad, stored, wide)
            assert all(rc == L.QC_OK for rc, _, _ in answers[0])


def test_wide64_grad_launch_rule_is_unchanged(qc):
    L = qc._lib

    def launch(n, m, S, T, wide):
        D = tw._wdesc(qc, wide, N=n // 2, m=m, T=T, cols=1)
        mf, ch, nch = C.c_int32(), C.c_int64(), C.c_int64()
        assert L.lib.qc_sweep_desc_launch(C.byref(D.d), S, C.byref(mf), C.byref(ch), C.byref(nch)) == L.QC_OK
        return bool(mf.value), ch.value, nch.value

    for n in (16, 24, 32, 34, 54, 64):
        for m in (1, 8, 16, 17):
            for S, T in ((1, 2), (2, 102), (5, 12), (50, 26), (255, 5), (256, 3), (257, 5), (300, 3), (8192, 1000)):
                want = t64.launch64(n, m, S, T, 1 | W64)
                assert launch(n, m, S, T, WIDE) == launch(n, m, S, T, 1 | W64) == (want["mfma"], want["chunk"], want["n_chunks"]), (n, m, S, T)
    f = t64.launch64(34, 2, 2, 102, WIDE)          # the sqrt-capped GPU case
    assert f["by_sqrt"] and (f["chunk"], f["n_chunks"], f["last"]) == (10, 11, 1)
    for name, spec in GRAD_CASES64.items():
        assert 32 < 2 * spec[1] <= 64 and t64.launch64(2 * spec[1], spec[2], spec[6], spec[7], WIDE)["mfma"], name
    assert t64.launch64(54, 6, 5, 12, WIDE)["n_chunks"] == 4 and t64.launch64(34, 2, 256, 3, WIDE)["n_chunks"] == 1


def test_wide64_grad_constants_keywords_and_texts(qc, tmp_path):
    L = qc._lib
    src = tmp_path / "w64g.c"
    src.write_text('#include <stdio.h>\n#include "qcolloc.h"\nint main(){printf("%zu %d %d\\n", sizeof(qc_sweep_desc), QC_SWEEP_WIDE_64_GRAD, '
                   'QC_SWEEP_WIDE | QC_SWEEP_WIDE_64 | QC_SWEEP_WIDE_64_GRAD);return 0;}\n')
    exe = tmp_path / "w64g"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [128, 2048, 3073]
    assert L.lib.qc_sizeof_sweep_desc() == C.sizeof(L.qc_sweep_desc) == 128 and L.lib.qc_abi_version() == 6
    julia = open(os.path.join(ROOT, "julia", "QCollocHIP.jl"), encoding="utf-8").read()
    assert "const QC_SWEEP_WIDE_64_GRAD = 2048" in julia and julia.count("wide64_grad::Bool=false") == 2
    assert julia.count("(wide64_grad ? QC_SWEEP_WIDE_64_GRAD : 0)") == 2
    for f in (qc.RolloutSweep.__init__, qc.SweepInfidelityObjective.__init__, qc.SweepFinalStateObjective.__init__):
        p = inspect.signature(f).parameters
        assert p["wide64_grad"].default is False and p["wide64"].default is False, f
    assert "wide64_grad" in qc.RolloutSweep.__doc__
    # refused before the library is touched: no system is looked at
    with pytest.raises(ValueError, match="wide64_grad=True needs wide64=True"):
        qc.RolloutSweep(None, [], 5, wide=True, wide64_grad=True)
    with pytest.raises(ValueError, match="wide64=True needs wide=True"):
        qc.RolloutSweep(None, [], 5, wide64=True, wide64_grad=True)
    # no new exported symbol; the new file is built
    names = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "qc_sweep_grad" in names and "sweep64" not in names
    makefile = open(os.path.join(ROOT, "quantumcollocation.jl_amd", "csrc", "Makefile")).read()
    assert "qc_sweep64_grad.hip" in makefile and "qc_sweep64_grad.o" in makefile
    for doc in ("DESIGN.md", "README.md"):
        text = open(os.path.join(ROOT, doc), encoding="utf-8").read()
        assert "qc_sweep64_grad.hip" in text and "have no sweep gradient yet" not in text, doc


# ---------------------------------------------------------------------------------------------------------------------------------
#  GPU
# ---------------------------------------------------------------------------------------------------------------------------------
def _check_call(sw, Z, c, weights=None):
    """test_sweep_grad._check_call with the shared reference: per-sample values, fidelities (the bits of `eval`), J and grad against the
    weighted sum, +0.0 outside the derivatives, and the handle's own scratch in place of the per-sample output."""
    J, fids, grad, gs = sw.grad(Z, c["init"], c["theta"], c["scale"], weights=weights, per_sample=True)
    S = c["S"]
    assert gs.shape == (S, c["T"] - 1, sw.n_deriv) and grad.shape == (sw.Z_len,) and fids.shape == (S,)
    tg._assert_samples(gs[c["samples"]], _reference(c), "wide64/" + c["name"])
    np.testing.assert_array_equal(fids, sw.eval(Z, c["init"], c["theta"], c["scale"], finals=False)[1])
    w = np.full(S, 1.0 / S) if weights is None else np.asarray(weights)
    assert abs(J - np.dot(w, fids)) <= 1e-14 * max(1.0, np.abs(w).sum())
    want = tg._weighted(gs, w, sw)
    np.testing.assert_allclose(grad, want, rtol=0, atol=1e-12 * max(1.0, np.abs(gs).max()) * max(1.0, np.abs(w).sum()))
    np.testing.assert_array_equal(grad[want == 0], 0.0)
    assert not np.signbit(grad[want == 0]).any()
    J2, f2, g2 = sw.grad(Z, c["init"], c["theta"], c["scale"], weights=weights)
    assert J2 == J and np.array_equal(f2, fids) and np.array_equal(g2, grad)
    return J, fids, grad, gs


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GRAD_CASES64))
def test_wide64_grad_matches_the_reference(qc, name):
    c = _case(qc, name)
    want = t64.launch64(c["n"], c["m"], c["S"], c["T"], WIDE)
    sw = ts.make_sweep(qc, c, **HANDLE)
    try:
        assert sw.kernel_name == "mfma64-sweep" and sw.wide64_grad and sw._desc.wide == WIDE
        assert sw.grad_supported and sw.grad_unsupported_reason is None and sw.vjp_supported
        assert sw.launch(c["S"]) == (True, want["chunk"], want["n_chunks"])
        if name == "sqrt-capped":
            assert want["by_sqrt"] and (want["chunk"], want["n_chunks"], want["last"]) == (10, 11, 1)
        if name in ("one-chunk", "one-interval"):
            assert want["n_chunks"] == 1
        if name == "transmons27-sub8":
            assert want["n_chunks"] == 4 and sw.cols == 27
        if name == "levels32-unitary":
            assert sw.ns == 2048 and sw.off_dt < 0
        if name == "no-drives-p0":
            assert sw.n_deriv == 1 and sw.p == 0
        _check_call(sw, sw.pack(c["controls"], c["dts"]), c, weights=np.linspace(0.5, 1.5, c["S"]) if name == "levels17-ket" else None)
    finally:
        sw.close()


@pytest.mark.gpu
def test_wide64_grad_through_the_squarings(qc):
    """One system per number of squarings 0 .. 6 (test_sweep_wide.squaring_cases at N = 17: a unitary of 17 columns, so the second
    column tile holds one live column); the samples of one call differ in it."""
    seen = set()
    for k, per_sample, c in tw.squaring_cases(qc, N=17, m=2, T=12):
        seen |= set(per_sample)
        c["name"] = f"N17 {c['name']}"
        sw = ts.make_sweep(qc, c, **HANDLE)
        try:
            assert sw.kernel_name == "mfma64-sweep"
            _check_call(sw, sw.pack(c["controls"]), c)
        finally:
            sw.close()
    assert set(range(7)) <= seen


@pytest.mark.gpu
def test_wide64_grad_zero_generators(qc):
    """Zero drift and drives: every propagator is the identity, bit for bit, so x and lambda keep the bits of the seed through the walk
    and the derivative of the identity walk, dF/da_k = h <lambda, G_k x>, is checked against the reference.  A zero drive as well."""
    N, T, S, m = 17, 5, 3, 2
    rng = np.random.default_rng(64)
    Hd = [_herm(rng, N, 0.3), np.zeros((N, N))]
    system = qc.QuantumSystem(np.zeros((N, N)), Hd)
    init, goal = ref.operator_to_iso_vec(_unitary(rng, N)), ref.operator_to_iso_vec(_unitary(rng, N))
    c = dict(name="zero generators", L=N, m=m, S=S, T=T, system=system, perts=[np.zeros((N, N))], G0=np.zeros((2 * N, 2 * N)),
             Gd=[ref.iso_generator(H) for H in Hd], Gp=[np.zeros((2 * N, 2 * N))], init=init, cols=N, goal=goal, kind="unitary", subspace=None,
             form="abs", controls=np.zeros((m, T)), dts=rng.uniform(0.1, 0.3, T), theta=rng.uniform(-1, 1, (S, 1)), scale=None, samples=list(range(S)))
    sw = ts.make_sweep(qc, c, **HANDLE)
    try:
        Z = sw.pack(c["controls"], c["dts"])
        J, fids, grad, gs = _check_call(sw, Z, c)
        finals = sw.eval(Z, init, c["theta"], fids=False)[0]
        np.testing.assert_array_equal(finals, np.repeat(init[:, None], S, axis=1))          # the identity's bits
        assert np.all(gs[:, :, 1] == 0.0) and np.all(gs[:, :, 2] == 0.0) and np.abs(gs[:, :, 0]).max() > 1e-3
        np.testing.assert_array_equal(gs, np.repeat(gs[:1], S, axis=0))                     # theta multiplies a zero matrix
        out = tv.device_call(sw, Z, dict(c, cot=tv.unit_cotangents(rng, S, init.size)), ["finals", "grad_init", "grad_samples"])
        np.testing.assert_array_equal(out["finals"], np.repeat(init[None, :], S, axis=0))
    finally:
        sw.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(VJP_CASES64))
def test_wide64_vjp_matches_the_reference(qc, name):
    """Random unit cotangents on handles without a fidelity: per-sample derivatives, `grad_init` and the plain sum against the
    reference, finals against `eval` bit for bit, outputs one at a time, the host entry."""
    c = _vjp_case(qc, name)
    sw = ts.make_sweep(qc, c, **HANDLE)
    try:
        assert sw.kernel_name == "mfma64-sweep" and sw.vjp_supported and not sw.grad_supported and "no fidelity" in sw.grad_unsupported_reason
        assert sw.cols == VJP_CASES64[name][1] and sw.fid_kind == qc._lib.QC_SWEEP_FID_NONE
        Z = sw.pack(c["controls"], c["dts"])
        want = ["finals", "grad", "grad_samples", "grad_init"]
        out = tv.device_call(sw, Z, c, want)
        r = _vjp_reference(c)
        tv.assert_samples(out["grad_samples"][c["samples"]], r["grad_samples"], f"64/{name} grad_samples")
        tv.assert_init(out["grad_init"][c["samples"]], r["grad_init"], f"64/{name} grad_init")
        np.testing.assert_array_equal(out["finals"], sw.eval(Z, c["init"], c["theta"], c["scale"], fids=False)[0].T)
        dense, mask = tv.plain_sum(out["grad_samples"], sw)
        np.testing.assert_allclose(out["grad"], dense, rtol=0, atol=1e-12 * max(1.0, np.abs(out["grad_samples"]).max()) * c["S"])
        ref_dense = tv.plain_sum(r["grad_samples"], sw)[0]
        assert np.abs(out["grad"] - ref_dense).max() <= tv.VJP_RTOL * c["S"] * max(1.0, np.abs(r["grad_samples"]).max())
        zero = out["grad"][~mask]
        assert np.array_equal(zero.view(np.uint64), np.zeros(zero.size, dtype=np.uint64)) and np.all(out["grad"][mask] != 0)
        for k in want:
            np.testing.assert_array_equal(tv.device_call(sw, Z, c, [k])[k], out[k], err_msg=k)
        host = sw.vjp(Z, c["init"], c["cot"], c["theta"], c["scale"], per_sample=True, init_grad=True)
        for a, k in zip(host, ("grad", "grad_samples", "grad_init")):
            np.testing.assert_array_equal(a, out[k], err_msg=k)
    finally:
        sw.close()


@pytest.mark.gpu
def test_wide64_vjp_consistent_with_the_fidelity_gradient(qc):
    c = _case(qc, "transmons27-sub8")
    sw = ts.make_sweep(qc, c, **HANDLE)
    try:
        tv.check_against_the_fidelity_gradient(sw, c, "64/transmons27-sub8")
    finally:
        sw.close()


@pytest.mark.gpu
def test_wide64_finals_autograd_backward(qc):
    """One backward pass of a torch loss on `finals_autograd` against central differences of the forward sweep (the step and tolerance of
    test_sweep_vjp.test_finals_autograd_gradcheck: eps 1e-6, atol 1e-6)."""
    rng = np.random.default_rng(31)
    N, m, T, S = 17, 2, 3, 2
    sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, 0.3) for _ in range(m)])
    sw = qc.RolloutSweep(sys_, [_herm(rng, N)], T, cols=2, **HANDLE)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    try:
        Z0 = sw.pack(rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T))
        init, theta, scale = t(rng.standard_normal(sw.ns)), t(rng.uniform(-0.3, 0.3, (S, 1))), t(rng.uniform(0.9, 1.1, (S, m)))
        Wt = t(rng.standard_normal((S, sw.ns)))
        loss = lambda Z_: ((sw.finals_autograd(Z_, init, theta, scale) * Wt).sum() + 0.5 * (sw.finals_autograd(Z_, init, theta, scale) ** 2 * Wt).sum())
        Z = t(Z0).requires_grad_(True)
        X = sw.finals_autograd(Z, init, theta, scale)
        fin = torch.empty((S, sw.ns), dtype=torch.float64, device=dev)
        sw.eval_device(Z.detach(), init, theta, scale, fin, None)
        assert torch.equal(X.detach(), fin)
        loss(Z).backward()
        got = Z.grad.cpu().numpy()
        eps, fd = 1e-6, np.zeros(sw.Z_len)
        with torch.no_grad():
            for i in range((T - 1) * sw.zdim):
                e = np.zeros(sw.Z_len)
                e[i] = eps
                fd[i] = (loss(t(Z0 + e)).item() - loss(t(Z0 - e)).item()) / (2 * eps)
        print(f"SWEEP-WIDE64-GRAD finals_autograd: max |backward - central differences| = {np.abs(got - fd).max():.3e} (bound 1e-6)")
        np.testing.assert_allclose(got, fd, rtol=0, atol=1e-6)
        assert np.abs(fd).max() > 1e-2 and np.all(got[(T - 1) * sw.zdim:] == 0.0)
        th = theta.clone().requires_grad_(True)          # a parameter cotangent: refused in backward, naming the form
        with pytest.raises(qc.QCollocError) as e:
            (sw.finals_autograd(t(Z0), init, th, scale) * Wt).sum().backward()
        assert e.value.code == qc._lib.QC_ERR_UNSUPPORTED and "mfma64-sweep" in str(e.value) and "2N = 34" in str(e.value)
    finally:
        sw.close()


@pytest.mark.gpu
def test_wide64_grad_bits_host_device_side_stream_and_scratch(qc):
    """Two repeated calls return identical bits; the host and device entry points agree bit for bit, on a side stream; a handle whose
    S grows (3, then 7) and is then reused (5) returns the bits of a fresh handle at every S, for `grad` and `vjp`."""
    rng = np.random.default_rng(8)
    N, m, T = 17, 2, 8
    sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, (N * m) ** -0.5) for _ in range(m)])
    perts = [_herm(rng, N)]
    goal = ref.operator_to_iso_vec(_unitary(rng, N))
    make = lambda: qc.RolloutSweep(sys_, perts, T, goal=goal, fid_kind="unitary", subspace=[0, 1, 3, 4], **HANDLE)
    sw = make()
    Z = sw.pack(rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T))
    init = ref.operator_to_iso_vec(_unitary(rng, N))
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    side = torch.cuda.Stream(device=dev)
    try:
        for S in (3, 7, 5):
            theta, scale, w = rng.uniform(-0.3, 0.3, (S, 1)), rng.uniform(0.9, 1.1, (S, m)), rng.uniform(0.5, 1.5, S)
            cot = tv.unit_cotangents(rng, S, sw.ns)
            fresh = make()
            first = fresh.grad(Z, init, theta, scale, weights=w, per_sample=True)
            first_v = fresh.vjp(Z, init, cot, theta, scale, per_sample=True, init_grad=True)
            fresh.close()
            for _ in range(2):
                again = sw.grad(Z, init, theta, scale, weights=w, per_sample=True)
                assert again[0] == first[0]
                for a, b in zip(again[1:], first[1:]):
                    np.testing.assert_array_equal(a, b)
                for a, b in zip(sw.vjp(Z, init, cot, theta, scale, per_sample=True, init_grad=True), first_v):
                    np.testing.assert_array_equal(a, b)
            assert np.isfinite(first[3]).all() and np.abs(first[3]).max() > 1e-3
            mk = lambda *shape: torch.full(shape, -7.0, dtype=torch.float64, device=dev)
            dfid, dJ, dg, dgs = mk(S), mk(1), mk(sw.Z_len), mk(S, T - 1, sw.n_deriv)
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                sw.grad_device(t(Z), t(init), S, t(theta), t(scale), t(w), dfid, dJ, dg, dgs, stream=side)
            side.synchronize()
            assert dJ.item() == first[0]
            for a, b in zip((dfid, dg, dgs), first[1:]):
                np.testing.assert_array_equal(a.cpu().numpy(), b)
            with torch.cuda.stream(side):
                out = tv.device_call(sw, Z, dict(S=S, init=init, theta=theta, scale=scale, cot=cot), ["grad", "grad_samples", "grad_init"], stream=side)
            for k, b in zip(("grad", "grad_samples", "grad_init"), first_v):
                np.testing.assert_array_equal(out[k], b, err_msg=k)
        print("SWEEP-WIDE64-GRAD bits: repeated calls, host / device / side stream and S = 3 -> 7 -> 5 identical (bound: 0 differing bits)")
    finally:
        sw.close()


@pytest.mark.gpu
def test_wide64_grad_refusals_on_a_live_handle(qc):
    L = qc._lib
    UNS = L.QC_ERR_UNSUPPORTED
    rng = np.random.default_rng(3)
    N, m, T, S = 20, 2, 6, 3
    sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, 0.3) for _ in range(m)])
    goal, P = ref.operator_to_iso_vec(_unitary(rng, N)), _herm(rng, N)
    init, theta = ref.operator_to_iso_vec(_unitary(rng, N)), rng.uniform(-0.3, 0.3, (S, 1))
    sw = qc.RolloutSweep(sys_, [P], T, goal=goal, fid_kind="unitary", **HANDLE)
    plain = qc.RolloutSweep(sys_, [P], T, goal=goal, fid_kind="unitary", wide=True, wide64=True)
    try:
        Z = sw.pack(rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T))
        assert sw.grad_supported and sw.vjp_supported and np.isfinite(sw.grad(Z, init, theta)[2]).all()
        named = lambda e: e.value.code == UNS and "mfma64-sweep" in str(e.value) and "2N = 40" in str(e.value) and "rollout-per-sample" not in str(e.value)
        with pytest.raises(qc.QCollocError) as e:
            sw.param_grad(Z, init, theta)
        assert named(e) and "parameter gradients" in str(e.value)
        with pytest.raises(qc.QCollocError) as e:
            sw.vjp(Z, init, np.zeros((S, sw.ns)), theta, params=True)
        assert named(e) and "parameter cotangents" in str(e.value)
        for which, call in (("jvp", lambda: sw.jvp(Z, init, np.ones_like(Z), theta)),
                            ("hvp", lambda: sw.hvp(Z, init, np.zeros((S, sw.ns)), theta, vZ=np.ones_like(Z))),
                            ("noise", lambda: sw.noise_eval(Z, init, np.zeros((S, T - 1, 1))))):
            assert not getattr(sw, which + "_supported") and "mfma64-sweep" in getattr(sw, which + "_unsupported_reason")
            with pytest.raises(qc.QCollocError) as e:
                call()
            assert named(e), which
        # a handle made without the bit refuses `grad` with the text it always had
        assert plain.kernel_name == "mfma64-sweep" and not plain.wide64_grad and not plain.grad_supported
        with pytest.raises(qc.QCollocError) as e:
            plain.grad(Z, init, theta)
        assert named(e) and "which serves the forward sweep only" in str(e.value)
        # and the two handles' forward sweeps carry the same bits
        for a, b in zip(sw.eval(Z, init, theta), plain.eval(Z, init, theta)):
            np.testing.assert_array_equal(a, b)
    finally:
        sw.close()
        plain.close()
    stored = qc.RolloutSweep(sys_, [P], T, goal=goal, fid_kind="unitary", stored_states=True, **HANDLE)          # the stored-state flag
    try:
        assert not stored.grad_supported and not stored.vjp_supported
        with pytest.raises(qc.QCollocError) as e:
            stored.grad(Z, init, theta)
        assert e.value.code == UNS and "mfma64-sweep" in str(e.value) and "stored-state" in str(e.value)
        assert np.isfinite(stored.eval(Z, init, theta)[0]).all()
    finally:
        stored.close()


@pytest.mark.gpu
def test_wide64_grad_non_finite_input(qc):
    """One NaN control does not raise.  In the last knot it reaches nothing.  Inside the trajectory it reaches every sample (the controls
    are shared); a NaN in one sample's theta reaches that sample alone and the others carry their bits; the handle then serves a finite
    call as if nothing had happened."""
    rng = np.random.default_rng(12)
    N, m, T, S = 17, 2, 8, 4
    sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, 0.3) for _ in range(m)])
    goal = ref.operator_to_iso_vec(_unitary(rng, N))
    sw = qc.RolloutSweep(sys_, [_herm(rng, N)], T, goal=goal, fid_kind="unitary", **HANDLE)
    try:
        controls, dts = rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T)
        init, theta = ref.operator_to_iso_vec(_unitary(rng, N)), rng.uniform(-0.3, 0.3, (S, 1))
        good = sw.grad(sw.pack(controls, dts), init, theta, per_sample=True)
        assert np.isfinite(good[2]).all() and np.isfinite(good[3]).all()
        bad = controls.copy()
        bad[0, T - 1] = np.nan          # the last knot's controls drive no interval
        again = sw.grad(sw.pack(bad, dts), init, theta, per_sample=True)
        assert again[0] == good[0]
        for a, b in zip(again[1:], good[1:]):
            np.testing.assert_array_equal(a, b)
        bad = controls.copy()
        bad[1, 3] = np.nan
        J, fids, grad, gs = sw.grad(sw.pack(bad, dts), init, theta, per_sample=True)
        assert np.isnan(J) and np.isnan(fids).all() and np.isnan(gs).all()
        K = grad[:T * sw.zdim].reshape(T, sw.zdim)
        assert np.isnan(K[:T - 1]).all() and np.array_equal(K[T - 1].view(np.uint64), np.zeros(sw.zdim, dtype=np.uint64))
        th = theta.copy()
        th[2, 0] = np.nan
        J, fids, grad, gs = sw.grad(sw.pack(controls, dts), init, th, per_sample=True)
        others = [0, 1, 3]
        assert np.isnan(fids[2]) and np.isnan(gs[2]).all() and np.isnan(J)
        np.testing.assert_array_equal(fids[others], good[1][others])
        np.testing.assert_array_equal(gs[others], good[3][others])
        after = sw.grad(sw.pack(controls, dts), init, theta, per_sample=True)
        for a, b in zip(after[1:], good[1:]):
            np.testing.assert_array_equal(a, b)
        print("SWEEP-WIDE64-GRAD non-finite: a NaN control reaches every sample, a NaN theta its own sample alone (bound: 0 differing bits elsewhere)")
    finally:
        sw.close()


@pytest.mark.gpu
def test_three_transmon_polish_example(qc):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import three_transmon_polish as ex
        out = ex.run(T=6, grid=3, steps=2, verbose=False)
    finally:
        sys.path.pop(0)
    assert out["kernel"] == "mfma64-sweep" and out["columns"] == 8 and out["levels"] == 27
    assert np.isfinite(out["before"]) and out["after"] < out["before"] and out["grad_norm"] > 0.0 and out["iterations"] >= 1
