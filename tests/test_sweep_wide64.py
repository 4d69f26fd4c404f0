"""Matrix-core rollout sweeps for 32 < 2N <= 64 (`qc_sweep_desc.wide = QC_SWEEP_WIDE | QC_SWEEP_WIDE_64`,
`RolloutSweep(..., wide=True, wide64=True)`): the form "mfma64-sweep" with up to 16 drives (csrc/qc_sweep64.hip), the forward sweep only.
CPU: the descriptor field, the restated launch rule with and without the bit, the scope queries, constants / keywords / texts.  GPU: parity
with the scipy reference of tests/sweep_reference.py at the smallest shapes at which tiling, padding, chunking and squaring can go wrong,
generator norms, exact cases, bits, non-finite input, the unchanged default.

Tolerances are test_sweep.py's (states rtol 1e-10 / atol 1e-11, fidelities 1e-9 absolute; its argument |dF| <= sqrt(N) max|dU| is
stated for N <= 32, which is exactly this range).  Every GPU test prints its worst error against the bound; measured values:
profiles/sweep_wide64_summary.txt.  Every sample of launches of 200 .. 510 workgroups: tests/test_sweep_wide64_every_sample.py."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest
import torch

import sweep_reference as ref
import test_sweep as ts
import test_sweep_wide as tw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_herm, _unitary = ts._herm, ts._unitary
W64 = 1024
FILL64 = 256            # one workgroup per compute unit: 256 CUs x 1
QUERIES = ("grad", "vjp", "jvp", "hvp", "noise")


def launch64(n, m, S, T, wide):
    """The launch rule restated.  With bits 0 and 10, 32 < 2N <= 64 and m <= 16 is the MFMA form whose item is a workgroup: one chunk once
    S >= 256, else ceil(256 / S) chunks, at most ceil(sqrt(T - 1)).  2N <= 32 does not look at bit 10: test_sweep_wide.wide_launch."""
    if n <= 32:
        return tw.wide_launch(n, m, S, T, bool(wide & 1))
    if not ((wide & 1) and (wide & W64)) or n > 64 or m > 16:
        return dict(mfma=False, chunk=T - 1, n_chunks=0, last=0)
    n_int = T - 1
    want = 1 if S >= FILL64 else -(-FILL64 // S)
    r = 1
    while r * r < n_int:
        r += 1
    nch = min(want, r)
    chunk = -(-n_int // nch)
    n_chunks = -(-n_int // chunk)
    return dict(mfma=True, chunk=chunk, n_chunks=n_chunks, last=n_int - (n_chunks - 1) * chunk, by_sqrt=want > r)


# name: (state, levels, m, p, scale given, free timestep, S, T, fidelity, samples) -- the tuple test_sweep_wide.build reads
CASES64 = {
    "levels17-S11-T50": ("unitary", 17, 2, 1, False, True, 11, 50, ("unitary", [0, 1, 3, 4], "abs"), None),   # third tile row / column almost empty
    "levels24-S300-T2": ("unitary", 24, 6, 8, False, True, 300, 2, ("unitary", None, "abs"), None),         # exactly three tiles, one interval, one chunk, every perturbation slot
    "transmons27-S5-T12": ("unitary", 27, 6, 1, True, False, 5, 12, ("unitary", None, "abs2"), None),       # the example's size
    "levels32-S2-T102": ("unitary", 32, 10, 3, True, True, 2, 102, ("unitary", None, "abs"), None),         # full tiles, 5-qubit drive count, sqrt-capped chunks, short last chunk
    "levels32-m16": ("unitary", 32, 16, 0, True, False, 3, 5, None, None),                                  # the drive limit; final states only
    "ket20-S256-T3": ("ket", 20, 2, 1, True, True, 256, 3, ("ket", None, "abs"), None),                     # S at the fill boundary: one chunk
    "kets3-levels18": ("kets3", 18, 1, 3, True, False, 11, 20, None, None),                                 # few columns
    "open5-S7-T20": ("density", 5, 2, 1, True, True, 7, 20, ("density", None, "abs"), None),                # N = 25: Lindblad generators, not antisymmetric
}


def _valid_today():
    """0, and bit 0 with any of bits 1, 3, 4, 6, 8: the thirty-three values valid before bit 10."""
    out = [0]
    for mask in range(32):
        v = 1
        for i, bit in enumerate((2, 8, 16, 64, 256)):
            if mask >> i & 1:
                v |= bit
        out.append(v)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
#  CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_wide64_field_is_validated(qc):
    L = qc._lib
    val = lambda D: L.lib.qc_sweep_desc_validate(C.byref(D.d))
    msg = lambda: L.lib.qc_sweep_last_error(None).decode()
    today = _valid_today()
    assert len(today) == 33 and {0, 1, 3, 9, 11, 17, 19, 25, 27, 65, 91, 257, 347} <= set(today)
    for N in (20, 12, 2):
        for v in today:
            assert val(tw._wdesc(qc, v, N=N)) == L.QC_OK, (N, v)
            if v:
                assert val(tw._wdesc(qc, v | W64, N=N)) == L.QC_OK, (N, v | W64)
        for bad in (1024, 1026, 513, 2049, (1 << 20) | 1025, -1):
            assert val(tw._wdesc(qc, bad, N=N)) == L.QC_ERR_INVALID, (N, bad)
            text = msg()
            assert text.startswith("qc_sweep: wide"), text
            for words in ("17, 19, 25 or 27", "QC_SWEEP_WIDE_TANGENT (16)", "QC_SWEEP_WIDE_NOISE (64)", "QC_SWEEP_WIDE_HESSIAN (256)",
                          "QC_SWEEP_WIDE_64 (1024)"):
                assert words in text, (words, text)
    ok = C.c_int32(-1)
    assert L.lib.qc_sweep_desc_grad_supported(C.byref(tw._wdesc(qc, 1024, N=20).d), C.byref(ok)) == L.QC_ERR_INVALID
    assert L.lib.qc_sweep_desc_launch(C.byref(tw._wdesc(qc, 1024, N=20).d), 5, None, None, None) == L.QC_ERR_INVALID


def test_wide64_form_and_launch_rule(qc):
    """`qc_sweep_desc_launch` against the restated rule: above 2N = 32 the MFMA form iff both bits are set, 2N <= 64 and m <= 16; at
    2N <= 32 the answer without bit 10."""
    L = qc._lib

    def launch(n, m, S, T, wide):
        D = tw._wdesc(qc, wide, N=n // 2, m=m, T=T, cols=1)
        mf, ch, nch = C.c_int32(), C.c_int64(), C.c_int64()
        assert L.lib.qc_sweep_desc_launch(C.byref(D.d), S, C.byref(mf), C.byref(ch), C.byref(nch)) == L.QC_OK, (n, m, S, T, wide)
        return bool(mf.value), ch.value, nch.value

    seen = set()
    for n in (32, 34, 48, 54, 64):
        for m in (1, 10, 16, 17):
            for S, T in ((1, 2), (2, 102), (5, 12), (255, 50), (256, 50), (300, 2), (8192, 1000)):
                for wide in (0, 1, 1 | W64, 27 | W64):
                    got = launch(n, m, S, T, wide)
                    want = launch64(n, m, S, T, wide)
                    assert got == (want["mfma"], want["chunk"], want["n_chunks"]), (n, m, S, T, wide)
                    assert want["mfma"] == ((n <= 32 and m <= 8 and bool(wide & 1)) or (n > 32 and bool(wide & W64) and m <= 16)), (n, m, wide)
                    if want["mfma"]:
                        assert (got[2] - 1) * got[1] < T - 1 <= got[2] * got[1]
                    if n <= 32 and wide & W64:      # the bit is ignored
                        assert got == launch(n, m, S, T, wide & ~W64)
                    seen.add((n, m, wide, want["mfma"]))
    assert (54, 10, 1025, True) in seen and (54, 10, 1, False) in seen and (64, 16, 1025, True) in seen and (64, 17, 1025, False) in seen
    assert (34, 1, 0, False) in seen and (32, 1, 1025, True) in seen and (32, 10, 1025, False) in seen
    D = tw._wdesc(qc, 1 | W64, N=33, m=1, T=10, cols=1)
    assert L.lib.qc_sweep_desc_launch(C.byref(D.d), 5, None, None, None) == L.QC_ERR_UNSUPPORTED
    assert "2N = 66" in L.lib.qc_sweep_last_error(None).decode()
    f = launch64(64, 10, 2, 102, 1025)          # the sqrt-capped GPU case: 11 chunks of 10, the last of 1
    assert f["by_sqrt"] and (f["chunk"], f["n_chunks"], f["last"]) == (10, 11, 1)
    assert launch64(54, 6, 255, 50, 1025)["n_chunks"] == 2 and launch64(54, 6, 256, 50, 1025)["n_chunks"] == 1
    for name, spec in CASES64.items():          # the GPU cases are all inside the form
        n = 2 * spec[1] ** 2 if spec[0] == "density" else 2 * spec[1]
        assert 32 < n <= 64 and launch64(n, spec[2], spec[6], spec[7], 1025)["mfma"], name
    assert launch64(40, 2, 256, 3, 1025)["n_chunks"] == 1 and launch64(64, 1, 300, 2, 1025)["n_chunks"] == 1


def _query(qc, which, D):
    L = qc._lib
    ok = C.c_int32(-1)
    rc = getattr(L.lib, f"qc_sweep_desc_{which}_supported")(C.byref(D.d), C.byref(ok))
    return rc, ok.value, L.lib.qc_sweep_last_error(None).decode() if ok.value == 0 else None      # the reason is written only with a 0


def test_wide64_scope_queries(qc):
    """In the new form every other family answers 0 and names the form and the size; at 2N <= 32 the bit changes no answer and no text."""
    import test_sweep_grad as tg
    L = qc._lib
    U = L.QC_FID_UNITARY
    for wide in (1 | W64, 3 | W64, 347 | W64):
        for kw in (dict(N=27, m=6, fid_kind=U), dict(N=17, m=2, cols=1, fid_kind=L.QC_FID_KET), dict(N=32, m=16, fid_kind=U),
                   dict(N=25, m=2, cols=1, fid_kind=L.QC_FID_DENSITY)):
            for stored in (0, 1):
                D = tg._GDesc(qc, **kw)
                D.d.wide = wide
                D.d.reserved1[0] = stored
                for which in QUERIES:
                    rc, ok, text = _query(qc, which, D)
                    assert (rc, ok) == (L.QC_OK, 0), (which, wide, kw, stored)
                    assert "mfma64-sweep" in text and f"2N = {2 * kw['N']}" in text and "rollout-per-sample" not in text, (which, text)
    # more than 16 drives: the per-sample form, and said so
    D = tg._GDesc(qc, N=27, m=17, fid_kind=U)
    D.d.wide = 1 | W64
    rc, ok, text = _query(qc, "grad", D)
    assert (rc, ok) == (L.QC_OK, 0) and "rollout-per-sample" in text and "17 drives" in text
    # without the bit: today's texts
    D = tg._GDesc(qc, N=27, m=6, fid_kind=U)
    D.d.wide = 1
    rc, ok, text = _query(qc, "grad", D)
    assert (rc, ok) == (L.QC_OK, 0) and "rollout-per-sample form (2N = 54 > 32)" in text
    D.d.wide = 0
    assert "rollout-per-sample form (2N = 54 > 16)" in _query(qc, "jvp", D)[2]
    # 2N <= 32: closed, Lindblad and stored-flag variants answer what they answer without the bit
    variants = []
    for kw in (dict(N=12, m=2, fid_kind=U), dict(N=4, m=2, p=2, fid_kind=U), dict(N=16, m=8, p=1, cols=1, fid_kind=L.QC_FID_KET),
               dict(N=12, m=9, fid_kind=U), dict(N=12, m=2), dict(N=12, m=2, p=0, fid_kind=U)):
        variants.append((kw, False, 0))
    for kw in (dict(N=16, m=2, cols=1, fid_kind=L.QC_FID_DENSITY), dict(N=4, m=2, cols=1, fid_kind=L.QC_FID_DENSITY)):
        variants += [(kw, True, 0), (kw, True, 1)]
    variants.append((dict(N=12, m=2, fid_kind=U), False, 1))
    for kw, lindblad, stored in variants:
        for wide in (1, 3, 9, 11, 17, 65, 257, 347):
            answers = []
            for bit in (0, W64):
                D = tg._GDesc(qc, **kw)
                if lindblad:
                    D.G0[:] = np.random.default_rng(0).standard_normal(D.G0.size)
                D.d.wide = wide | bit
                D.d.reserved1[0] = stored
                answers.append([_query(qc, which, D) for which in QUERIES])
            assert answers[0] == answers[1], (kw, lindblad, stored, wide)
            assert all(rc == L.QC_OK for rc, _, _ in answers[0])
    assert _query(qc, "grad", _with_wide(tg._GDesc(qc, N=12, m=2, fid_kind=U), 1 | W64))[:2] == (L.QC_OK, 1)


def _with_wide(D, wide):
    D.d.wide = wide
    return D


def test_wide64_constants_keywords_and_texts(qc, tmp_path):
    L = qc._lib
    assert L.QC_SWEEP_WIDE_64 == W64 == 1 << 10
    src = tmp_path / "w64.c"
    src.write_text('#include <stdio.h>\n#include "qcolloc.h"\nint main(){printf("%zu %d %d\\n", sizeof(qc_sweep_desc), QC_SWEEP_WIDE_64, '
                   'QC_SWEEP_WIDE);return 0;}\n')
    exe = tmp_path / "w64"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [128, 1024, 1]
    assert L.lib.qc_sizeof_sweep_desc() == C.sizeof(L.qc_sweep_desc) == 128 and L.lib.qc_abi_version() == 6
    julia = open(os.path.join(ROOT, "julia", "QCollocHIP.jl"), encoding="utf-8").read()
    assert "const QC_SWEEP_WIDE_64 = 1024" in julia and "wide64::Bool=false" in julia
    assert "device::Int32; wide::Int32; reserved1::NTuple{2,Int64}" in julia          # the struct does not change
    for f in (qc.RolloutSweep.__init__, qc.rollout_sweep, qc.unitary_rollout_fidelity_sweep, qc.rollout_fidelity_sweep):
        p = inspect.signature(f).parameters
        assert p["wide64"].default is False and p["wide"].default is False, f
    assert "wide64" in qc.RolloutSweep.__doc__ and "mfma64-sweep" in qc.RolloutSweep.kernel_name.__doc__
    # refused before the library is touched: no system is looked at
    with pytest.raises(ValueError, match="wide64=True needs wide=True"):
        qc.RolloutSweep(None, [], 5, wide64=True)
    # no new exported symbol
    names = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "qc_sweep_eval" in names and "sweep64" not in names
    makefile = open(os.path.join(ROOT, "quantumcollocation.jl_amd", "csrc", "Makefile")).read()
    assert "qc_sweep64.hip" in makefile and "qc_sweep64.o" in makefile and "qc_sweep64_common.h" in makefile
    for doc in ("DESIGN.md", "README.md"):
        assert "qc_sweep64.hip" in open(os.path.join(ROOT, doc), encoding="utf-8").read(), doc


# ---------------------------------------------------------------------------------------------------------------------------------
#  GPU
# ---------------------------------------------------------------------------------------------------------------------------------
def _report(what, got, want, fids=None, rfids=None):
    err = np.abs(got - want)
    worst = (err / (ts.STATE_ATOL + ts.STATE_RTOL * np.abs(want))).max()
    line = f"SWEEP-WIDE64 {what}: max |d state| = {err.max():.3e}, worst / tolerance = {worst:.4f}"
    if fids is not None:
        line += f", max |d fidelity| = {np.abs(fids - rfids).max():.3e} (bound {ts.FID_ATOL:.0e})"
    print(line)


_REFERENCE = {}


def _case(qc, name):
    """The case and its reference, computed once and left unchanged."""
    if name not in _REFERENCE:
        c = tw.build(qc, name, CASES64[name])
        _REFERENCE[name] = (c, ts.reference(c))
    return _REFERENCE[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES64))
def test_wide64_sweep_matches_the_reference(qc, name):
    c, (rf, rfid) = _case(qc, name)
    want = launch64(c["n"], c["m"], c["S"], c["T"], 1 | W64)
    assert want["mfma"] and 32 < c["n"] <= 64
    sw = ts.make_sweep(qc, c, wide=True, wide64=True)
    try:
        assert sw.kernel_name == "mfma64-sweep" and sw.wide and sw.wide64
        assert sw.launch(c["S"]) == (True, want["chunk"], want["n_chunks"])
        if name == "levels32-S2-T102":
            assert want["by_sqrt"] and (want["chunk"], want["n_chunks"], want["last"]) == (10, 11, 1)
        if name in ("ket20-S256-T3", "levels24-S300-T2"):
            assert want["n_chunks"] == 1
        Z = sw.pack(c["controls"], c["dts"])
        finals, fids = sw.eval(Z, c["init"], c["theta"], c["scale"])
        if c["kind"] is not None:   # fidelities alone: the same bits
            np.testing.assert_array_equal(sw.eval(Z, c["init"], c["theta"], c["scale"], finals=False)[1], fids)
    finally:
        sw.close()
    assert finals.shape == rf.shape == (c["n"] * c["cols"], c["S"])
    _report(name, finals, rf, fids, rfid)
    ts._assert_states(finals, rf, name)
    if c["kind"] is None:
        assert fids is None
    else:
        ts._assert_fids(fids, rfid, name)
    # The one-call form returns the same bits in every case.  It reads its timesteps from the trajectory vector; for a fixed timestep
    # that is the same double the handle above takes from dt_fixed, and nothing else in the kernel depends on where it came from.
    form = qc._lib.QC_FID_FORM_ABS2 if c["form"] == "abs2" else qc._lib.QC_FID_FORM_ABS
    f3, fid3 = qc.rollout_sweep(c["init"], c["controls"], c["dts"], c["system"], c["perts"], c["theta"], c["scale"], cols=c["cols"],
                                goal=c["goal"], fid_kind=c["kind"], subspace=c["subspace"], fid_form=form, wide=True, wide64=True)
    np.testing.assert_array_equal(f3, finals)
    if fids is None:
        assert fid3 is None
    else:
        np.testing.assert_array_equal(fid3, fids)


@pytest.mark.gpu
def test_wide64_sweep_generator_norms(qc):
    """One system per number of squarings 0 .. 6, samples of one call that differ in it, through the new form."""
    seen = set()
    for k, per_sample, c in tw.squaring_cases(qc, N=17, m=2, T=12):
        seen |= set(per_sample)
        sw = ts.make_sweep(qc, c, wide=True, wide64=True)
        try:
            assert sw.kernel_name == "mfma64-sweep"
            finals, fids = sw.eval(sw.pack(c["controls"], c["dts"]), c["init"], c["theta"], c["scale"])
        finally:
            sw.close()
        rf, rfid = ts.reference(c)
        _report(c["name"], finals, rf, fids, rfid)
        ts._assert_states(finals, rf, c["name"])
        ts._assert_fids(fids, rfid, c["name"])
    assert set(range(7)) <= seen


@pytest.mark.gpu
def test_wide64_sweep_exact_cases(qc):
    """A zero generator gives the identity bits: finals are init.  theta = 0, scale = 1 on an N = 20 handle: the bits of the handle
    without perturbations, the per-sample form of the same descriptor without the bit to the tolerances, and `unitary_rollout`."""
    N, T, S, m = 20, 14, 7, 2
    rng = np.random.default_rng(N)
    init = ref.operator_to_iso_vec(_unitary(rng, N))
    kw = dict(wide=True, wide64=True)
    zsys = qc.QuantumSystem(np.zeros((N, N)), [np.zeros((N, N))] * m)
    finals, _ = qc.rollout_sweep(init, rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T), zsys, [np.zeros((N, N))], rng.uniform(-1, 1, (S, 1)), **kw)
    np.testing.assert_array_equal(finals, np.repeat(init[:, None], S, axis=1))
    sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, 0.3) for _ in range(m)])
    controls, dts = rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T)
    goal = ref.operator_to_iso_vec(_unitary(rng, N))
    perts = [_herm(rng, N), _herm(rng, N)]
    a = qc.rollout_sweep(init, controls, dts, sys_, perts, np.zeros((S, 2)), np.ones((S, m)), goal=goal, fid_kind="unitary", **kw)
    b = qc.rollout_sweep(init, controls, dts, sys_, [], np.zeros((S, 0)), None, goal=goal, fid_kind="unitary", **kw)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    assert np.all(a[0] == a[0][:, :1]) and np.abs(a[0][:, 0] - init).max() > 1e-3
    narrow = qc.rollout_sweep(init, controls, dts, sys_, perts, np.zeros((S, 2)), np.ones((S, m)), goal=goal, fid_kind="unitary", wide=True)
    _report("mfma64-sweep against the per-sample form", a[0], narrow[0], a[1], narrow[1])
    ts._assert_states(a[0], narrow[0], "mfma64-sweep against the per-sample form")
    ts._assert_fids(a[1], narrow[1], "mfma64-sweep against the per-sample form")
    roll = qc.unitary_rollout(init, controls, dts, sys_)[:, -1]
    _report("mfma64-sweep against unitary_rollout", a[0][:, 0], roll)
    ts._assert_states(a[0][:, 0], roll, "mfma64-sweep against unitary_rollout")


@pytest.mark.gpu
def test_wide64_sweep_bits_host_device_side_stream_and_scratch(qc):
    """Six repeated calls return identical bits; the host and device entry points agree bit for bit, on a side stream too; a handle whose
    S grows and then shrinks returns the bits of a fresh handle at every S (the S x n_chunks x 4096 totals are grown on demand)."""
    rng = np.random.default_rng(8)
    N, m, T = 17, 2, 20
    sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, (N * m) ** -0.5) for _ in range(m)])
    perts = [_herm(rng, N)]
    goal = ref.operator_to_iso_vec(_unitary(rng, N))
    make = lambda: qc.RolloutSweep(sys_, perts, T, goal=goal, fid_kind="unitary", subspace=[0, 1, 3, 4], wide=True, wide64=True)
    sw = make()
    assert sw.kernel_name == "mfma64-sweep"
    Z = sw.pack(rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T))
    init = ref.operator_to_iso_vec(_unitary(rng, N))
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    side = torch.cuda.Stream(device=dev)
    try:
        for i, S in enumerate((3, 150, 7)):
            theta, scale = rng.uniform(-0.3, 0.3, (S, 1)), rng.uniform(0.9, 1.1, (S, m))
            fresh = make()
            want = fresh.eval(Z, init, theta, scale)
            fresh.close()
            got = sw.eval(Z, init, theta, scale)
            np.testing.assert_array_equal(got[0], want[0])
            np.testing.assert_array_equal(got[1], want[1])
            assert np.isfinite(want[0]).all() and np.abs(want[0][:, 0] - want[0][:, -1]).max() > 1e-6
            if i == 1:
                for _ in range(6):
                    again = sw.eval(Z, init, theta, scale)
                    np.testing.assert_array_equal(again[0], want[0])
                    np.testing.assert_array_equal(again[1], want[1])
            dZ, dinit, dth, dsc = t(Z), t(init), t(theta), t(scale)
            dfin, dfid = torch.full((S, sw.ns), -7.0, dtype=torch.float64, device=dev), torch.full((S,), -7.0, dtype=torch.float64, device=dev)
            sw.eval_device(dZ, dinit, dth, dsc, dfin, dfid)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(dfin.cpu().numpy().T, want[0])
            np.testing.assert_array_equal(dfid.cpu().numpy(), want[1])
            dfin2, dfid2 = torch.full_like(dfin, -7.0), torch.full_like(dfid, -7.0)
            with torch.cuda.stream(side):
                sw.eval_device(dZ, dinit, dth, dsc, dfin2, dfid2, stream=side)
            side.synchronize()
            np.testing.assert_array_equal(dfin2.cpu().numpy().T, want[0])
            np.testing.assert_array_equal(dfid2.cpu().numpy(), want[1])
        print("SWEEP-WIDE64 bits: six repeated calls, host / device / side stream and S = 3 -> 150 -> 7 identical (bound: 0 differing bits)")
    finally:
        sw.close()


@pytest.mark.gpu
def test_wide64_sweep_non_finite_input(qc):
    rng = np.random.default_rng(12)
    N, m, T, S = 20, 2, 14, 6
    sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, 0.3) for _ in range(m)])
    goal = ref.operator_to_iso_vec(_unitary(rng, N))
    sw = qc.RolloutSweep(sys_, [_herm(rng, N)], T, goal=goal, fid_kind="unitary", wide=True, wide64=True)
    try:
        assert sw.kernel_name == "mfma64-sweep"
        controls, dts = rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T)
        init = ref.operator_to_iso_vec(_unitary(rng, N))
        theta = rng.uniform(-0.3, 0.3, (S, 1))
        good = sw.eval(sw.pack(controls, dts), init, theta)
        assert np.isfinite(good[0]).all()
        bad = controls.copy()
        bad[1, 7] = np.nan
        finals, fids = sw.eval(sw.pack(bad, dts), init, theta)
        assert np.isnan(finals).all() and np.isnan(fids).all()
        bad = controls.copy()
        bad[0, T - 1] = np.nan          # the last knot's controls drive no interval
        again = sw.eval(sw.pack(bad, dts), init, theta)
        np.testing.assert_array_equal(again[0], good[0])
        np.testing.assert_array_equal(again[1], good[1])
        print("SWEEP-WIDE64 non-finite: a NaN control reaches every output; a NaN in the last knot changes no bit (bound: 0 differing bits)")
    finally:
        sw.close()


@pytest.mark.gpu
def test_wide64_default_is_unchanged(qc):
    """Without the bit, N = 20 is still the per-sample form with today's refusal texts; with it, N = 12 is still "mfma32-sweep" and N = 4
    still "mfma16-sweep", each with the bits of the handle without the bit; `grad` on an "mfma64-sweep" handle refuses, naming the form."""
    rng = np.random.default_rng(3)
    N, m, T, S = 20, 2, 6, 3
    sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, 0.3) for _ in range(m)])
    goal, P = ref.operator_to_iso_vec(_unitary(rng, N)), _herm(rng, N)
    init, theta = ref.operator_to_iso_vec(_unitary(rng, N)), rng.uniform(-0.3, 0.3, (S, 1))
    for wide, top in ((False, 16), (True, 32)):
        sw = qc.RolloutSweep(sys_, [P], T, goal=goal, fid_kind="unitary", wide=wide)
        try:
            assert sw.kernel_name == "rollout-per-sample" and not sw.wide64 and sw.launch(S) == (False, T - 1, 0)
            why = f"the handle takes the rollout-per-sample form (2N = 40 > {top})"
            assert not sw.grad_supported and why in sw.grad_unsupported_reason and why in sw.jvp_unsupported_reason
            Z = sw.pack(rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T))
            with pytest.raises(qc.QCollocError) as e:
                sw.grad(Z, init, theta)
            assert e.value.code == qc._lib.QC_ERR_UNSUPPORTED and why in str(e.value)
            assert np.isfinite(sw.eval(Z, init, theta)[0]).all()
        finally:
            sw.close()
    sw = qc.RolloutSweep(sys_, [P], T, goal=goal, fid_kind="unitary", wide=True, wide64=True)
    try:
        assert sw.kernel_name == "mfma64-sweep"
        for which in QUERIES:
            assert not getattr(sw, which + "_supported")
            assert "mfma64-sweep" in getattr(sw, which + "_unsupported_reason") and "2N = 40" in getattr(sw, which + "_unsupported_reason")
        with pytest.raises(qc.QCollocError) as e:
            sw.grad(Z, init, theta)
        assert e.value.code == qc._lib.QC_ERR_UNSUPPORTED and "mfma64-sweep" in str(e.value) and "rollout-per-sample" not in str(e.value)
        with pytest.raises(qc.QCollocError) as e:
            sw.jvp(Z, init, np.ones_like(Z), theta)
        assert e.value.code == qc._lib.QC_ERR_UNSUPPORTED and "mfma64-sweep" in str(e.value)
        assert np.isfinite(sw.eval(Z, init, theta)[0]).all()
    finally:
        sw.close()
    for N, name in ((12, "mfma32-sweep"), (4, "mfma16-sweep")):
        sysn = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, 0.3) for _ in range(m)])
        goal, init, P = ref.operator_to_iso_vec(_unitary(rng, N)), ref.operator_to_iso_vec(_unitary(rng, N)), _herm(rng, N)
        a, b = (qc.RolloutSweep(sysn, [P], T, goal=goal, fid_kind="unitary", wide=True, wide64=w) for w in (False, True))
        try:
            assert a.kernel_name == b.kernel_name == name and a.launch(S) == b.launch(S)
            Z = a.pack(rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T))
            for u, v in zip(a.eval(Z, init, theta), b.eval(Z, init, theta)):
                np.testing.assert_array_equal(u, v)
            assert a.grad_supported and b.grad_supported
            ra, rb = a.grad(Z, init, theta, per_sample=True), b.grad(Z, init, theta, per_sample=True)
            assert ra[0] == rb[0]
            for u, v in zip(ra[1:], rb[1:]):
                np.testing.assert_array_equal(u, v)
        finally:
            a.close()
            b.close()
    print("SWEEP-WIDE64 default: 2N <= 32 handles with and without the bit return identical bits for eval and grad (bound: 0 differing bits)")
