"""Matrix-core rollout sweeps for 32 < 2N <= 64 ("mfma64-sweep", `qc_sweep_mfma64_kernel` of csrc/qc_sweep64.hip and
`qc_sweep_finish_kernel` at ld = 64: `RolloutSweep(..., wide=True, wide64=True)`, `wide` = 1025) at launches of 40 .. 300 samples, EVERY
sample against the CPU reference: the method of tests/test_sweep_every_sample.py (read its header: R = 8 rows of (theta, scale), sample s
carries row cls[s], `test_sweep.reference` once for the R rows), its helpers imported.  tests/test_sweep_wide64.py compares this form with
the reference at 77, 22, 35, 12 and 220 items in launches of several chunks, at S = 300 and 256 in one chunk of one or two intervals, and
its growth test compares the kernel with itself.  What is checked here is what this form has of its own:
  * the work item is a whole workgroup of 16 waves, item = blockIdx.x, s = item / n_chunks, and the fill constant is 256: the regime
    where ceil(256 / S) sets the chunk count (3 chunks at S = 97, 2 at S = 129 and 255), just below and just above the fill constant
    (S = 255, 257), and the sqrt-capped regime at S = 40;
  * the chunk total at tot + item * 4096 and the finish kernel's read at tot + s * n_chunks * 4096, with 16, 1 and 3 state columns; at
    ns = 2048 (32 levels) the finish kernel's dynamic LDS is exactly 64 KiB, the largest it takes without the opt-in;
  * the drive limit m = 16 (lane u of a wave carries drive u's amplitude), eight perturbations over several intervals, a fixed timestep,
    Lindblad generators at n = 50, a third tile row that is almost empty (n = 34), long chunks (13 intervals) and a last chunk of 1;
  * the scratch S x n_chunks x 4096: 200 slots, grown to 300, reused as 291 at another stride.
This form is forward only: one `eval_device` call with `finals` and `fids`, then `eval`.
  1. finals[s], fids[s] of every sample against `test_sweep.reference` of the R rows, by `test_sweep._assert_states` (rtol 1e-10 / atol
     1e-11) and `test_sweep._assert_fids` (1e-9 absolute) through `every_sample`;
  2. every row of both outputs carries the bits of the first sample of its class;
  3. `eval`, `eval` with finals=False and the host entry return the device call's bits;
  4. both output buffers are prefilled with -7, so an unwritten sample fails 1.
No tolerance is new.

Why a wrong mapping fails.  Neighbouring samples belong to different classes in 7 of 8 places and any two classes' final states lie
>= 1e-3 apart (the non-vacuity test: 10^7 times the state tolerance), so a chunk total written or read at another item's slot -- a wrong
stride (4096 doubles an item), s or the chunk index formed with another launch's n_chunks, a workgroup that takes blockIdx.x for a
sample -- gives most samples a product that contains another class's propagator and fails 1, the samples named.  A slot nobody writes
holds what the allocation held; a sample nobody finishes keeps -7.  On the grown handle a slot that still holds the S = 300 launch's
total is another sample's and another interval range's: 1 fails at S = 97, and so does the comparison with a fresh handle.  The controls'
and the timestep's look-ahead read is clamped at the chunk's end; a wrong clamp makes the last interval of a chunk use the next knot's
controls, which are independent draws from [-1, 1]: 1 fails in every class.
CPU: the launch table by `test_sweep_wide64.launch64` and `qc_sweep_desc_launch` with `wide` = 1025, the class map at the new S, the
soundness of sharing references at n = 34, that no two classes look alike, that checks 1 and 2 fail on a shifted, an unwritten and a
last-bit-off sample made from the reference.  Measured worst ratios and times:
profiles/sweep_wide_every_sample_summary.txt."""
import ctypes as C
import itertools
import time

import numpy as np
import pytest
import torch

import test_sweep as ts
import test_sweep_every_sample as te
import test_sweep_wide as tw
import test_sweep_wide64 as t64
from test_sweep_every_sample import KET, R, U, assert_class_bits, assert_launch, classes, every_sample, expand

W64 = t64.W64
U0134, DENSITY = te.CASES["wide-sqrt-301"][0][8], ("density", None, "abs")
HANDLE = dict(wide=True, wide64=True)                                   # wide = 1025
# name: ((state, levels, m, p, scale given, free timestep, S, T, fidelity), wide, (chunk, n_chunks, last chunk), chunk count capped by sqrt(T - 1))
TABLE = {
    "w64-byS-97": (("unitary", 17, 2, 1, False, True, 97, 38, U0134), W64, (13, 3, 11), False),          # 291 workgroups: S sets the chunk count; long chunks; n = 34
    "w64-sqrt-40": (("unitary", 27, 6, 1, True, False, 40, 24, ("unitary", None, "abs2")), W64, (5, 5, 3), True),     # sqrt-capped; fixed timestep
    "w64-two-255": (("unitary", 24, 3, 8, True, True, 255, 8, U), W64, (4, 2, 3), False),                # just below the fill constant; eight perturbations
    "w64-one-257": (("ket", 20, 2, 1, True, True, 257, 8, KET), W64, (7, 1, 7), False),                  # just above it: one chunk
    "w64-byS-129-m16": (("unitary", 32, 16, 1, True, True, 129, 12, U), W64, (6, 2, 5), False),          # full tiles, the drive limit, ns = 2048
    "w64-lindblad-97": (("density", 5, 2, 1, True, True, 97, 24, DENSITY), W64, (8, 3, 7), False),       # n = 50; generators not antisymmetric
    "w64-kets3-97": (("kets3", 18, 1, 3, True, False, 97, 8, None), W64, (3, 3, 1), False),              # a last chunk of 1; no fidelity
}
ITEMS = {"w64-byS-97": 291, "w64-sqrt-40": 200, "w64-two-255": 510, "w64-one-257": 257, "w64-byS-129-m16": 258, "w64-lindblad-97": 291, "w64-kets3-97": 291}
GROWTH64 = (40, 300, 97)          # on one "w64-sqrt-40" handle at T = 24: 5 chunks, 1, 3 -- 200, 300, 291 slots of 4096 doubles
NEW_S = (40, 129, 255, 257, 300)  # the S whose class map test_sweep_every_sample.test_classes_reach_both_ends does not see


def _N(spec):
    return spec[1] * spec[1] if spec[0] == "density" else spec[1]


def rule64(spec, S):
    """`test_sweep_wide64.launch64` on a case tuple: what `assert_launch` takes as its rule."""
    return t64.launch64(2 * _N(spec), spec[2], S, spec[7], 1 | W64)


def timed_reference(rows):
    """`te.ref_finals(rows)` (computed once, shared, frozen), with the CPU time of its first build on the record."""
    t0 = time.process_time()
    fresh = ("finals", rows["name"]) not in te._REF
    r = te.ref_finals(rows)
    if fresh:
        print(f"SWEEP-WIDE64-EVERY reference {rows['name']}: final states of {R} rows built in {time.process_time() - t0:.2f} s of CPU time")
    return r


# ---------------------------------------------------------------------------------------------------------------------------------
#  CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_wide64_launch_table(qc):
    """The shapes sit on the edges they are named for, by `launch64` (the rule with fill 256) and by `qc_sweep_desc_launch` with
    `wide` = 1025."""
    L = qc._lib
    assert L.QC_SWEEP_WIDE | L.QC_SWEEP_WIDE_64 == 1025 == 1 | W64 and t64.FILL64 == 256
    assert set(ITEMS) == set(TABLE) and len(TABLE) == 7
    for name, (spec, wide, (chunk, n_chunks, last), by_sqrt) in TABLE.items():
        _, _, m, _, _, _, S, T, _ = spec
        N = _N(spec)
        assert wide == W64 and 32 < 2 * N <= 64 and m <= 16, name
        assert rule64(spec, S) == dict(mfma=True, chunk=chunk, n_chunks=n_chunks, last=last, by_sqrt=by_sqrt), name
        assert (n_chunks - 1) * chunk + last == T - 1 and S * n_chunks == ITEMS[name]
        D = tw._wdesc(qc, 1025, N=N, m=m, T=T, cols=1)
        mf, ch, nch = C.c_int32(), C.c_int64(), C.c_int64()
        assert L.lib.qc_sweep_desc_launch(C.byref(D.d), S, C.byref(mf), C.byref(ch), C.byref(nch)) == L.QC_OK
        assert (bool(mf.value), ch.value, nch.value) == (True, chunk, n_chunks), name
        D = tw._wdesc(qc, 1, N=N, m=m, T=T, cols=1)                                        # without bit 10: the per-sample form
        assert L.lib.qc_sweep_desc_launch(C.byref(D.d), S, C.byref(mf), C.byref(ch), C.byref(nch)) == L.QC_OK and not mf.value
    f = {k: TABLE[k][2] for k in TABLE}
    # the regime where S sets the chunk count: ceil(256 / S) below the sqrt cap
    for name in ("w64-byS-97", "w64-byS-129-m16", "w64-two-255", "w64-lindblad-97", "w64-kets3-97"):
        S, T = TABLE[name][0][6], TABLE[name][0][7]
        cap = next(r for r in range(1, T) if r * r >= T - 1)
        assert f[name][1] == -(-t64.FILL64 // S) > 1 and f[name][1] <= cap and not TABLE[name][3], name
    assert TABLE["w64-sqrt-40"][3] and -(-t64.FILL64 // 40) == 7 > f["w64-sqrt-40"][1] == 5          # sqrt-capped: ceil(sqrt(23)) = 5
    assert f["w64-two-255"][1] == 2 and f["w64-one-257"][1] == 1 and 255 < t64.FILL64 < 257          # both sides of the fill constant
    assert f["w64-kets3-97"] == (3, 3, 1) and f["w64-byS-97"][0] == 13                               # a last chunk of 1; long chunks
    assert 97 % 3 != 0 and all(f[k][1] % 2 == 1 for k in ("w64-byS-97", "w64-sqrt-40", "w64-lindblad-97"))
    sp = TABLE["w64-byS-129-m16"][0]
    assert 2 * sp[1] == 64 and sp[2] == 16 and (2 * (2 * sp[1] * sp[1]) + 64 * 64) * 8 == 64 * 1024  # ns = 2048: the finish kernel's LDS is 64 KiB
    assert 2 * TABLE["w64-byS-97"][0][1] == 34 and 2 * _N(TABLE["w64-lindblad-97"][0]) == 50
    assert TABLE["w64-two-255"][0][3] == 8 and TABLE["w64-two-255"][0][7] - 1 > 1                    # eight perturbations, several intervals
    assert not TABLE["w64-sqrt-40"][0][5] and not TABLE["w64-kets3-97"][0][5] and TABLE["w64-kets3-97"][0][8] is None
    # the scratch-growth sequence on one handle at T = 24: grown, then reused at another stride
    sp = TABLE["w64-sqrt-40"][0]
    seq = [rule64(sp, S)["n_chunks"] for S in GROWTH64]
    assert sp[7] == 24 and seq == [5, 1, 3] and [S * n for S, n in zip(GROWTH64, seq)] == [200, 300, 291]
    assert {TABLE[k][0][6] for k in TABLE} | set(GROWTH64) <= set(NEW_S) | {97}


def test_classes_reach_both_ends_at_the_new_sizes():
    """`test_sweep_every_sample.test_classes_reach_both_ends` at S = 40, 129, 255, 257, 300; S = 97 is checked there."""
    assert 97 in te.GROWTH and not set(NEW_S) & ({te.CASES[k][0][6] for k in te.CASES} | set(te.GROWTH))
    te.assert_classes_reach_both_ends(NEW_S)


def test_wide64_reference_reuse_is_sound(qc):
    """Two samples with equal rows have equal final states and fidelities, bit for bit, and distinct rows differ, at n = 34:
    `sweep_reference.sweep_finals` treats a sample by its own row (theta, scale) alone."""
    table = {"w64-reuse": (("unitary", 17, 2, 1, True, True, R, 5, U0134), W64, None, None)}
    rows = te.build_rows(qc, "w64-reuse", table)
    c = expand(rows, 2 * R + 3)
    S, cls = c["S"], c["cls"]
    pairs = [(r, S - 1 - r) for r in (0, 3, R - 1)]
    assert rows["n"] == 34 and all(cls[a] == cls[b] for a, b in pairs)
    picked = [s for pair in pairs for s in pair]
    finals, fids = ts.reference(c)
    own = ts.reference(rows)
    for what, a, b in (("finals", finals.T[picked], own[0].T[[0, 3, R - 1]]), ("fids", fids[picked][:, None], own[1][[0, 3, R - 1]][:, None])):
        a = np.ascontiguousarray(a)
        assert a.shape[0] == 6 and np.abs(a).max() > 1e-3, what
        np.testing.assert_array_equal(a[0::2].view(np.uint64), a[1::2].view(np.uint64), err_msg=what)
        assert not np.array_equal(a[0], a[2]), what                                         # and distinct rows differ
        np.testing.assert_array_equal(a[0::2], b, err_msg=what)                             # and they are the rows' own references


@pytest.mark.parametrize("name", list(TABLE))
def test_wide64_rows_are_not_vacuous(qc, name):
    """No class passes for another: any two classes' final states differ by >= 1e-3 in max-norm, 10^7 times the state tolerance; no final
    state is the initial one."""
    rows = te.build_rows(qc, name, TABLE)
    finals, fids = timed_reference(rows)
    a = finals.T
    assert a.shape == (R, rows["init"].size) and (fids is None) == (TABLE[name][0][8] is None)
    apart = min(np.abs(a[i] - a[j]).max() for i, j in itertools.combinations(range(R), 2))
    moved = np.abs(a - rows["init"]).max(axis=1).min()
    print(f"SWEEP-WIDE64-EVERY every/{name} finals: smallest distance between two classes {apart:.3e}, smallest distance from the initial state {moved:.3e}")
    assert apart >= 1e-3 and moved >= 1e-3, name
    assert ts.STATE_ATOL + ts.STATE_RTOL * np.abs(a).max() <= 2e-10 <= 1e-6 * apart


def test_the_checks_see_a_shifted_or_an_unwritten_sample(qc):
    """Checks 1 and 2 on arrays made here from the reference at S = 97: they pass on ref[cls], and fail when every sample holds its
    neighbour's value (a slot one item off), when one sample keeps the prefill, and when one sample differs from its class in the last bit."""
    name = "w64-kets3-97"
    rows = te.build_rows(qc, name, TABLE)
    c = expand(rows, TABLE[name][0][6])
    good = np.ascontiguousarray(timed_reference(rows)[0].T[c["cls"]])
    check_values(good, None, rows, c, "made up")
    unwritten, last_bit = good.copy(), good.copy()
    unwritten[50] = -7.0
    last_bit[50, 3] = np.nextafter(last_bit[50, 3], 2.0)
    for what, bad in (("shifted", np.roll(good, 1, axis=0)), ("unwritten", unwritten), ("last bit", last_bit)):
        with pytest.raises(AssertionError):
            check_values(bad, None, rows, c, what)
    with pytest.raises(AssertionError, match="largest errors at"):
        check_values(np.roll(good, 1, axis=0), None, rows, c, "shifted")


# ---------------------------------------------------------------------------------------------------------------------------------
#  GPU
# ---------------------------------------------------------------------------------------------------------------------------------
def eval_call(sw, Z, c):
    """One `eval_device` call with every output the handle has, the buffers prefilled with -7: (finals S x ns, fids S or None)."""
    dev = torch.device("cuda:0")
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    S = c["S"]
    dfin = torch.full((S, sw.ns), -7.0, dtype=torch.float64, device=dev)
    dfid = torch.full((S,), -7.0, dtype=torch.float64, device=dev) if c["kind"] is not None else None
    torch.cuda.synchronize()
    sw.eval_device(t(Z), t(c["init"]), t(c["theta"]), t(c["scale"]), dfin, dfid)
    torch.cuda.synchronize()
    return dfin.cpu().numpy(), None if dfid is None else dfid.cpu().numpy()


def check_values(finals, fids, rows, c, what):
    """Checks 1 and 2: every sample against the reference of its class, and the bits of the first sample of its class."""
    cls = c["cls"]
    rfin, rfid = timed_reference(rows)
    assert finals.shape == (c["S"], rows["init"].size)
    every_sample(ts._assert_states, finals, rfin.T[cls], cls, f"SWEEP-WIDE64-EVERY {what} finals")
    assert_class_bits(finals, cls, f"{what} finals")
    if rfid is None:
        assert fids is None
    else:
        every_sample(ts._assert_fids, fids, rfid[cls], cls, f"SWEEP-WIDE64-EVERY {what} fids")
        assert_class_bits(fids, cls, f"{what} fids")


def check_eval(sw, rows, c, what):
    Z = sw.pack(c["controls"], c["dts"])
    finals, fids = eval_call(sw, Z, c)
    check_values(finals, fids, rows, c, what)
    # 3: the host entry, and fidelities alone
    hfin, hfid = sw.eval(Z, c["init"], c["theta"], c["scale"])
    np.testing.assert_array_equal(hfin, finals.T, err_msg=f"{what}: host finals")
    if fids is None:
        assert hfid is None
    else:
        np.testing.assert_array_equal(hfid, fids, err_msg=f"{what}: host fids")
        np.testing.assert_array_equal(sw.eval(Z, c["init"], c["theta"], c["scale"], finals=False)[1], fids, err_msg=f"{what}: fids alone")
    return finals, fids


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TABLE))
def test_wide64_every_sample(qc, name):
    t_wall = time.perf_counter()
    rows = te.build_rows(qc, name, TABLE)
    spec = TABLE[name][0]
    c = expand(rows, spec[6])
    timed_reference(rows)
    sw = ts.make_sweep(qc, rows, **HANDLE)
    try:
        want = assert_launch(sw, name, table=TABLE, rule=rule64, kernel="mfma64-sweep")
        assert sw._desc.wide == 1025 and sw.wide64 and c["S"] * want["n_chunks"] == ITEMS[name] and rows["n"] == 2 * _N(spec)
        assert sw.m == spec[2] and sw.p == spec[3] and (c["scale"] is None) == (not spec[4]) and (np.ndim(c["dts"]) == 1) == spec[5]
        if name == "w64-byS-129-m16":
            assert sw.ns == 2048 and sw.m == 16
        if name == "w64-lindblad-97":
            assert rows["n"] == 50 and np.abs(rows["G0"] + rows["G0"].T).max() > 0.05
        check_eval(sw, rows, c, f"w64-every/{name}")
    finally:
        sw.close()
    print(f"SWEEP-WIDE64-EVERY w64-every/{name}: {time.perf_counter() - t_wall:.2f} s of wall time")


@pytest.mark.gpu
def test_wide64_scratch_growth_every_sample(qc):
    """One handle at S = 40, then 300, then 97 with T = 24: 5 chunks, 1, 3, so the totals are 200 slots of 4096 doubles, grown to 300, then
    reused as 291 at another stride.  At every S the outputs pass checks 1 and 2 and carry the bits of a fresh handle's."""
    t_wall = time.perf_counter()
    name = "w64-sqrt-40"
    rows = te.build_rows(qc, name, TABLE)
    timed_reference(rows)
    sw = ts.make_sweep(qc, rows, **HANDLE)
    try:
        seen = []
        for S in GROWTH64:
            c = expand(rows, S)
            seen.append(assert_launch(sw, name, S, table=TABLE, rule=rule64, kernel="mfma64-sweep")["n_chunks"])
            what = f"w64-every/{name} grown to S = {S}"
            Z = sw.pack(c["controls"], c["dts"])
            finals, fids = eval_call(sw, Z, c)
            fresh = ts.make_sweep(qc, rows, **HANDLE)
            try:
                finals2, fids2 = eval_call(fresh, Z, c)
            finally:
                fresh.close()
            check_values(finals, fids, rows, c, what)
            np.testing.assert_array_equal(finals, finals2, err_msg=f"{what}: finals of a fresh handle")
            np.testing.assert_array_equal(fids, fids2, err_msg=f"{what}: fids of a fresh handle")
        assert seen == [5, 1, 3] and [S * n for S, n in zip(GROWTH64, seen)] == [200, 300, 291]
    finally:
        sw.close()
    print(f"SWEEP-WIDE64-EVERY w64-every/{name} growth: {time.perf_counter() - t_wall:.2f} s of wall time")
