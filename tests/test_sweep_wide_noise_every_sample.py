"""Wide noise-trajectory sweeps (`qc_sweep32_noise_kernel`, `qc_sweep32_noise_grad_kernel` of csrc/qc_sweep32_noise.hip: `qc_sweep_noise_eval*`
and `qc_sweep_noise_grad*` on "mfma32-sweep" handles made with `wide=True, wide_noise=True`, `wide` = 65) at mid-size and filled launches,
EVERY sample against the CPU reference: the method of tests/test_sweep_noise_every_sample.py (read its header and that of
tests/test_sweep_every_sample.py: R = 8 rows of (theta, scale, noise trajectory), sample s carries row cls[s], the references of
tests/sweep_noise_reference.py once for the R rows) applied to wide handles, its helpers imported.  The largest launch of
tests/test_sweep_wide_noise.py is four distinct samples tiled to S = 2048 at T = 3, its longest chunk has 3 intervals and its largest
m + p is 9.  What is checked here:
  * the mapping from a sample to a wave, a workgroup and a scratch slot -- item = 4 blockIdx + wave, s = item / n_chunks, the partly
    filled last workgroup (1505, 2049, 2049, 679 items: 1, 1, 1, 3 mod 4), workgroups whose waves straddle two samples (5, 3, 7 chunks)
    -- and the sample's own noise at noise + s (T-1) p, with 8 different trajectories in the launch;
  * the per-lane pointers: the read one interval ahead (backwards: one behind) and its clamp at the chunk's end, on chunks of 4 .. 20
    intervals, on 3 .. 20 chunks and on a last chunk of 1;
  * the documented limit of 16 generators: at m + p = 16 with a free timestep the timestep's value sits in lane 16, the first lane of the
    second 16-lane row, at m + p = 15 in lane 15, the last lane of the first; a filled launch at m + p = 16 (fixed timestep: grad_samples
    has m columns), and two cases at S = 3 with one row per sample that tell a failure of the lane map from one of the sample mapping;
  * `sNoise`, `sGnoise` and the scratch shared with `eval` and `grad`: growth and reuse at a smaller stride, host and device entries.

Checks 1 to 6 of tests/test_sweep_noise_every_sample.py, unchanged (`check_values`, `assert_same_bits`, `check_zero_noise`,
`scratch_growth`):
  1. finals[s], fids[s], grad_samples[s], grad_noise[s] against the reference of cls[s] by the assertions of test_sweep.py (states rtol
     1e-10 / atol 1e-11, fidelities 1e-9) and test_sweep_noise.py (1e-9 max(1, max |want_s|));
  2. every per-sample output row carries the bits of the first sample of its class; the gradient's fids carry the evaluation's;
  3. |J - w . F_ref[cls]| <= 1e-9 sum |w|, and `grad` against the reference's own weighted sum by `assert_dense`;
  4. the host-buffer entry points return the bits of the device calls;
  5. with noise = +0.0 finals, fids, J, grad and grad_samples equal `eval` and `grad` on the same handle, whole arrays, by np.array_equal,
     the comparison of test_sweep_wide_noise.test_wide_zero_noise_is_the_sweep;
  6. every output buffer is prefilled with -7.
No tolerance is new.

Why a wrong mapping fails.  Neighbouring samples belong to different classes in 7 of 8 places, and any two classes lie >= 1e-3 apart in
finals, grad_samples and grad_noise (the non-vacuity test: 10^6 bounds), so noise read at another sample's offset -- a wrong stride
(T-1) p, s taken from another launch's n_chunks -- or a chunk-end state at another item's slot gives most samples another class's value:
1 fails and names the samples; the tiled launch of the older file passes a read four samples away, this map does not.  A row nobody writes
keeps -7.  A wrong clamp of the look-ahead read makes the last (backwards: the first) interval of every chunk but the run's last use a
neighbouring interval's noise, or lets the step leave the sample's trajectory at its end: the noise values are independent draws from
[-0.3, 0.3] and every class has max |d F / d xi| >= 1e-2, so finals and grad_noise move by about 1e-3; with 20 chunks of 20 intervals
("wide-long") and a last chunk of 1 ("wide-sqrt-97", "small-mt*") every position of the clamp occurs.  A timestep taken from the wrong
lane at 16 generators puts a drive's or a perturbation's derivative, or nothing, into column m of grad_samples: "small-mt16" fails 1 in
that column with one row per sample and "small-mt15" passes, which separates it from the sample mapping; a lane map that loses
generator 15 gives another final state at both m + p = 16 cases.
CPU: the launch table against the restated rule and `qc_sweep_desc_launch` with `wide` = 65, the generator counts and the scope query,
the soundness of sharing references at a wide shape, that no check passes on zeros or on rows that look alike, and that checks 1 to 3
fail on arrays made from the references as a wrong lane, a clamp one interval early and a read one sample off would leave them (no faulty
kernel is run on a device).  Measured worst ratios and times: profiles/sweep_wide_every_sample_summary.txt."""
import ctypes as C
import time
import types

import numpy as np
import pytest

import test_sweep as ts
import test_sweep_every_sample as te
import test_sweep_grad as tg
import test_sweep_noise as tn
import test_sweep_noise_every_sample as tne
import test_sweep_wide as tw
from test_sweep_every_sample import GROWTH, KET, R, U, assert_launch

U0134 = te.CASES["wide-sqrt-301"][0][8]                                 # the subspace fidelity of that case
NOISE = dict(wide=True, wide_noise=True)                                # wide = 65
# name: ((state, levels, m, p, scale given, free timestep, S, T, fidelity), wide, (chunk, n_chunks, last chunk), chunk count capped by sqrt(T - 1))
TABLE = {
    "wide-sqrt-301": (("unitary", 9, 2, 1, True, True, 301, 24, U0134), True, (5, 5, 3), True),          # 1505 items: odd n_chunks, partial last workgroup
    "wide-byS-683-mt16": (("unitary", 16, 8, 8, True, False, 683, 12, U), True, (4, 3, 3), False),       # 2049 items, full tiles, sixteen generators
    # "-n": the name seeds the draw; under "wide-one-2049" two classes' grad_noise lie 6.2e-4 apart, below the 1e-3 floor (here 2.8e-3)
    "wide-one-2049-n": (("ket", 10, 2, 1, True, True, 2049, 6, KET), True, (5, 1, 5), False),            # past the fill threshold: one chunk of 5
    "wide-sqrt-97": (("unitary", 12, 3, 2, False, True, 97, 38, U), True, (6, 7, 1), True),              # 679 items, 7 chunks, a last chunk of 1
    "wide-long": (("unitary", 9, 2, 1, False, True, 2, 400, U), True, (20, 20, 19), True),               # 20 chunks of 20 intervals
    "small-mt16": (("unitary", 9, 8, 8, True, True, 3, 6, U), True, (2, 3, 1), True),                    # the timestep in lane 16, without the mapping
    "small-mt15": (("unitary", 9, 7, 8, True, True, 3, 6, U), True, (2, 3, 1), True),                    # the timestep in lane 15
}
ITEMS_MOD_4 = {"wide-sqrt-301": 1, "wide-byS-683-mt16": 1, "wide-one-2049-n": 1, "wide-sqrt-97": 3, "wide-long": 0, "small-mt16": 1, "small-mt15": 1}
ONE_ROW_PER_SAMPLE = ("wide-long", "small-mt16", "small-mt15")


def rows_of(qc, name):
    """The case with its distinct rows as the samples, and their number: R, or S where every sample has a row of its own."""
    Rn = tne.n_rows(name, TABLE, ONE_ROW_PER_SAMPLE)
    return tne.build_rows(qc, name, TABLE, rows=Rn), Rn


def timed_reference(rows):
    """`reference(rows)` of the narrow file (computed once, shared, frozen), with the CPU time of its first build on the record."""
    t0 = time.process_time()
    fresh = rows["name"] not in tne._REF
    r = tne.reference(rows)
    if fresh:
        print(f"SWEEP-WIDE-NOISE-EVERY reference {rows['name']}: noise references over {rows['S']} rows built in {time.process_time() - t0:.2f} s of CPU time")
    return r


# ---------------------------------------------------------------------------------------------------------------------------------
#  CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_wide_noise_launch_table(qc):
    """The shapes sit on the edges they are named for, by the restated rule and by `qc_sweep_desc_launch` with `wide` = 65."""
    L = qc._lib
    assert L.QC_SWEEP_WIDE | L.QC_SWEEP_WIDE_NOISE == 65
    assert set(ITEMS_MOD_4) == set(TABLE) and len(TABLE) == 7
    for name, (spec, wide, (chunk, n_chunks, last), by_sqrt) in TABLE.items():
        state, levels, m, p, _, _, S, T, _ = spec
        assert wide and state in ("unitary", "ket") and 16 < 2 * levels <= 32 and 1 <= p <= 8 and m <= 8
        want = ts.sweep_launch(16, m, S, T)                                                # the rule with fill 2048, whatever the size
        assert want == tw.wide_launch(2 * levels, m, S, T, True) == dict(mfma=True, chunk=chunk, n_chunks=n_chunks, last=last, by_sqrt=by_sqrt), name
        assert (n_chunks - 1) * chunk + last == T - 1
        assert (S * n_chunks) % 4 == ITEMS_MOD_4[name], name
        D = tw._wdesc(qc, 65, N=levels, m=m, p=p, T=T, cols=1)
        mf, ch, nch = C.c_int32(), C.c_int64(), C.c_int64()
        assert L.lib.qc_sweep_desc_launch(C.byref(D.d), S, C.byref(mf), C.byref(ch), C.byref(nch)) == L.QC_OK
        assert (bool(mf.value), ch.value, nch.value) == (True, chunk, n_chunks), name
    f = {k: TABLE[k][2] for k in TABLE}
    assert all(f[k][1] % 2 == 1 and f[k][1] > 1 for k in ("wide-sqrt-301", "wide-byS-683-mt16", "wide-sqrt-97"))      # workgroups straddle samples
    assert {ITEMS_MOD_4[k] for k in ("wide-sqrt-301", "wide-byS-683-mt16", "wide-one-2049-n", "wide-sqrt-97")} == {1, 3}   # a partly filled last workgroup
    assert -(-ts.SWEEP_FILL // 683) == 3 == f["wide-byS-683-mt16"][1] and f["wide-byS-683-mt16"][1] < 4               # set by S, not by sqrt(11)
    assert f["wide-one-2049-n"][1] == 1 and 683 < ts.SWEEP_FILL < 2049                                                  # both sides of the fill threshold
    assert f["wide-sqrt-97"] == (6, 7, 1) and f["small-mt16"] == f["small-mt15"] == (2, 3, 1)                         # a last chunk of one interval
    assert f["wide-long"] == (20, 20, 19) and max(v[0] for v in f.values()) == 20                                     # long chunks, many of them
    assert 2 * TABLE["wide-byS-683-mt16"][0][1] == 32                                                                 # full tiles
    # the class map of every mapped S is checked by test_sweep_every_sample.test_classes_reach_both_ends
    mapped = {TABLE[k][0][6] for k in TABLE if k not in ONE_ROW_PER_SAMPLE}
    assert mapped | set(GROWTH) <= {te.CASES[k][0][6] for k in te.CASES} | set(te.GROWTH)
    for k in ONE_ROW_PER_SAMPLE:
        n = tne.n_rows(k, TABLE, ONE_ROW_PER_SAMPLE)
        assert n == TABLE[k][0][6] <= R and tne.class_map(k, n, ONE_ROW_PER_SAMPLE).tolist() == list(range(n))
    assert tne.n_rows("wide-sqrt-97", TABLE, ONE_ROW_PER_SAMPLE) == R
    # the scratch-growth sequence on one handle at T = 24
    sp = TABLE["wide-sqrt-301"][0]
    assert sp[7] == 24 and [tw.wide_launch(2 * sp[1], sp[2], S, 24)["n_chunks"] for S in GROWTH] == [5, 1, 5]
    assert GROWTH[1] > GROWTH[0] > GROWTH[2]                                               # sNoise, sGnoise: grown twice, then reused smaller


def test_generator_counts_reach_the_limit(qc):
    """m + p of the cases covers 3, 5, 15 and 16, the documented limit; at 16 and 15 with a free timestep its lane is lane 16 resp. 15, on
    both sides of the boundary between the first two 16-lane rows; `qc_sweep_desc_noise_supported` answers 1 for every case."""
    L = qc._lib
    count = {name: spec[2] + spec[3] for name, (spec, *_) in TABLE.items()}
    assert set(count.values()) == {3, 5, 15, 16}
    assert count["small-mt16"] == count["wide-byS-683-mt16"] == 16 == 8 + L.QC_MAX_PERT and count["small-mt15"] == 15
    assert TABLE["small-mt16"][0][5] and TABLE["small-mt15"][0][5] and not TABLE["wide-byS-683-mt16"][0][5]
    assert count["small-mt16"] // 16 == 1 and count["small-mt16"] % 16 == 0 and count["small-mt15"] // 16 == 0 and count["small-mt15"] % 16 == 15
    assert TABLE["small-mt16"][0][:2] + TABLE["small-mt16"][0][3:] == TABLE["small-mt15"][0][:2] + TABLE["small-mt15"][0][3:]      # "the same with m = 7"
    for name, (spec, *_) in TABLE.items():
        state, levels, m, p, _, _, _, T, _ = spec
        D = tg._GDesc(qc, N=levels, m=m, p=p, T=T, fid_kind=L.QC_FID_KET if state == "ket" else L.QC_FID_UNITARY, **(dict(cols=1) if state == "ket" else {}))
        D.d.wide = 65
        assert tn._supported(qc, D)[:2] == (L.QC_OK, 1), name
        D.d.wide = 1                                                                       # and without the bit it is the bit that is missing
        assert tn._supported(qc, D)[:2] == (L.QC_OK, 0), name
    # every lane role: drives with and without a scale, a timestep lane or none
    assert {TABLE[k][0][4] for k in TABLE} == {True, False} == {TABLE[k][0][5] for k in TABLE}


def test_wide_noise_reference_reuse_is_sound(qc):
    """The narrow file's check on one wide shape (9 levels, a subspace fidelity, two noise lanes)."""
    tne.assert_reference_reuse_is_sound(qc, "wide-reuse", ("unitary", 9, 2, 2, True, True, R, 5, U0134))


@pytest.mark.parametrize("name", list(TABLE))
def test_wide_noise_rows_are_not_vacuous(qc, name):
    """The narrow file's floors on the wide rows: every class has max |grad_noise| >= 1e-2, any two classes differ by >= 1e-3 in finals,
    grad_samples and grad_noise."""
    tne.assert_rows_are_not_vacuous(qc, name, TABLE, ONE_ROW_PER_SAMPLE)


def made_up_outputs(rows, c, sw):
    """What a faultless kernel returns for the launch `c`, from the reference of the rows: the dictionary `check_values` reads."""
    cls, w = c["cls"], c["weights"]
    rfin, rfid, rgs, rgn = tne.reference(rows)
    return dict(finals=rfin[cls].copy(), fids=rfid[cls].copy(), gfids=rfid[cls].copy(), J=float(np.dot(w, rfid[cls])), grad=tg._weighted(rgs[cls], w, sw),
                grad_samples=rgs[cls].copy(), grad_noise=rgn[cls].copy())


def layout_of(rows):
    """The attributes of a handle that `check_values` reads, without a device: the layout `RolloutSweep.pack` gives the case."""
    T, m, free = rows["T"], rows["m"], np.ndim(rows["dts"]) == 1
    zdim = m + (1 if free else 0)
    return types.SimpleNamespace(T=T, m=m, p=rows["p"], ns=rows["init"].size, n_deriv=zdim, zdim=zdim, off_a=0, off_dt=m if free else -1, Z_len=T * zdim)


def test_the_checks_see_a_wrong_lane_a_wrong_clamp_and_a_shifted_sample(qc):
    """Checks 1 to 3 on arrays made here from the references, no device: they pass on the reference itself and fail on what three faulty
    kernels would return.  (a) "small-mt16", the timestep's derivative taken from lane 15: column m of grad_samples holds the last
    perturbation's derivative.  (b) "small-mt16", the look-ahead read clamped one interval early: the last interval of every chunk of two
    uses the noise of the interval before it; the final states are the reference's under that noise.  (c) "wide-one-2049-n", the noise read
    one sample off: every sample holds its neighbour's outputs."""
    name = "small-mt16"
    rows, Rn = rows_of(qc, name)
    c = tne.launch_of(rows, Rn, tne.class_map(name, Rn, ONE_ROW_PER_SAMPLE))
    sw = layout_of(rows)
    assert (sw.m, sw.p, sw.n_deriv, sw.off_dt) == (8, 8, 9, 8) and TABLE[name][2] == (2, 3, 1)
    good = made_up_outputs(rows, c, sw)
    tne.check_values(sw, good, rows, c, "made up")
    lane = dict(good, grad_samples=good["grad_samples"].copy())
    lane["grad_samples"][:, :, sw.m] = good["grad_noise"][:, :, sw.p - 1]
    with pytest.raises(AssertionError):
        tne.check_values(sw, lane, rows, c, "wrong lane")
    early = rows["noise"].copy()
    early[:, 1], early[:, 3] = rows["noise"][:, 0], rows["noise"][:, 2]                     # chunks [0, 1], [2, 3], [4]
    moved = tne.compute_reference(dict(rows, noise=early), range(Rn))
    clamp = dict(good, finals=moved[0], fids=moved[1], gfids=moved[1])
    print(f"SWEEP-WIDE-NOISE-EVERY a clamp one interval early moves the final states by {np.abs(moved[0] - good['finals']).max():.3e}")
    with pytest.raises(AssertionError):
        tne.check_values(sw, clamp, rows, c, "wrong clamp")
    name = "wide-one-2049-n"
    rows, Rn = rows_of(qc, name)
    S = TABLE[name][0][6]
    c = tne.launch_of(rows, S, tne.class_map(name, S, ONE_ROW_PER_SAMPLE))
    sw = layout_of(rows)
    good = made_up_outputs(rows, c, sw)
    tne.check_values(sw, good, rows, c, "made up")
    shifted = {k: (np.roll(v, 1, axis=0) if k in ("finals", "fids", "gfids", "grad_samples", "grad_noise") else v) for k, v in good.items()}
    with pytest.raises(AssertionError, match="largest errors at"):
        tne.check_values(sw, shifted, rows, c, "shifted")


# ---------------------------------------------------------------------------------------------------------------------------------
#  GPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TABLE))
def test_wide_noise_every_sample(qc, name):
    t_wall = time.perf_counter()
    rows, Rn = rows_of(qc, name)
    spec = TABLE[name][0]
    S = spec[6]
    c = tne.launch_of(rows, S, tne.class_map(name, S, ONE_ROW_PER_SAMPLE))
    timed_reference(rows)
    sw = ts.make_sweep(qc, rows, **NOISE)
    try:
        want = assert_launch(sw, name, table=TABLE)
        assert (want["chunk"], want["n_chunks"], want["last"]) == TABLE[name][2] and (S * want["n_chunks"]) % 4 == ITEMS_MOD_4[name]
        assert sw._desc.wide == 65 and sw.wide_noise and sw.noise_supported and sw.noise_unsupported_reason is None and sw.grad_supported
        assert sw.m + sw.p == spec[2] + spec[3] and sw.n_deriv == spec[2] + (1 if spec[5] else 0)
        what = f"wide-every/{name}"
        Z = sw.pack(c["controls"], c["dts"])
        out = tne.device_calls(sw, Z, c)
        tne.check_values(sw, out, rows, c, what)
        tne.assert_same_bits(tne.host_calls(sw, Z, c), out, f"{what}: the host entries against the device calls")
        tne.check_zero_noise(sw, Z, c, what)
    finally:
        sw.close()
    print(f"SWEEP-WIDE-NOISE-EVERY wide-every/{name}: {time.perf_counter() - t_wall:.2f} s of wall time")


@pytest.mark.gpu
def test_wide_noise_scratch_growth_every_sample(qc):
    """One `wide` = 65 handle at S = 301 (host buffers), then 2049 (device tensors), then 97 (host buffers) with T = 24: 5 chunks, 1, 5
    again, so dTot / dXs / dLs grow and are then reused at a smaller stride, and so do the staging buffers `sNoise` and `sGnoise`.  At
    every S both noise entries carry the bits of a fresh handle's and pass checks 1 to 3."""
    t_wall = time.perf_counter()
    name = "wide-sqrt-301"
    timed_reference(rows_of(qc, name)[0])
    tne.scratch_growth(qc, name, TABLE, **NOISE)
    print(f"SWEEP-WIDE-NOISE-EVERY wide-every/{name} growth: {time.perf_counter() - t_wall:.2f} s of wall time")
