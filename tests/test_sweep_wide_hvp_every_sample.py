"""Wide sweep Hessian products (`qc_sweep32_hvp_kernel` with the launches around it in csrc/qc_sweep32_hvp.hip: `qc_sweep_hvp*` on
"mfma32-sweep" handles made with `wide=True, wide_hessian=True`, `wide` = 257) at mid-size and filled launches, EVERY sample against the
CPU reference: the method of tests/test_sweep_hvp_every_sample.py (read its header and that of tests/test_sweep_every_sample.py: R = 8 rows,
sample s carries row cls[s], the recurrence reference once for the R rows) applied to wide handles, its helpers imported.
tests/test_sweep_wide_hvp.py checks the arithmetic at up to 20 work items and three samples of one S = 2048 launch with one chunk; what is
checked here is what one call has of its own, four launches over the same item space with different shapes:
  * `qc_sweep32_jvp_kernel`, two waves a workgroup: item = 2 blockIdx + wave, 2048 doubles an item in `dTotJ`; every item count here is
    odd, so the last workgroup's second wave exits;
  * the ld = 32 seed kernel, one workgroup a sample, reading `dTotJ + s * n_chunks * 2048`;
  * `qc_sweep32_hvp_kernel`, four waves a workgroup: item = 4 blockIdx + wave, s = item / n_chunks, chunk-end states, adjoints and both
    tangents at item * ns; item counts 1 and 3 mod 4, workgroups that straddle two samples (n_chunks 5, 3, 7);
  * the plain-sum reduction over the samples;
at 5, 3, 7 chunks and at one, on both sides of the fill threshold, with 1 and 16 state columns, padded and full tiles; and the scratch
`dXsT` / `dLsT` / `dTGsamp` / `dTotJ` next to the `dTot` / `dXs` / `dLs` that `grad` and `vjp` use on the same handle: growth, reuse
at a smaller stride, a call of the other entries before and after.

Checks 1 to 6 of tests/test_sweep_hvp_every_sample.py, unchanged (`check_values`, `check_hvp`, `linear_part`, `scratch_growth`):
  1. tgrad_samples[s], tgrad_init[s] against `sweep_hvp_reference.hessian_product_frechet` of cls[s] by `test_sweep_hvp.assert_samples`
     (HVP_RTOL = 1e-9: |got - want| <= 1e-9 max(1, max |want_s|));
  2. every per-sample output row carries the bits of the first sample of its class;
  3. tgrad is, bit for bit, the plain ascending sum of the kernel's own rows (`test_sweep_hvp.scatter`), and is compared with the
     reference's sum by `assert_dense` with unit weights (1e-9 S max(1, max |ref|), +0.0 elsewhere);
  4. the host-buffer entry point returns the bits of the device call;
  5. along vcot alone the product is the wide pullback of vcot on the same handle, every sample: 2e-9 max(1, max |.|_s);
  6. every output buffer is prefilled with -7.
No tolerance is new.  The growth test's handle carries `wide_params` as well (`wide` = 259): `vjp_device` is asked for every output.

Why a wrong mapping fails.  Two neighbouring samples s, s + 1 belong to different classes in 7 of 8 places (`classes` is pseudo-random, and
any two classes' references lie >= 1e-3 apart, 10^6 bounds: the non-vacuity test), so a kernel that reads the chunk totals, the chunk-end
state or a tangent of another sample -- a wrong stride of `dTotJ` (2048 an item), of `dXs` / `dXsT` (ns an item), n_chunks taken for
another launch's -- gives most samples another class's value and fails 1 with the samples named; a read inside the right class would have
to hit the same class by chance at every one of 301 .. 2049 samples.  A sample nobody writes keeps -7 (6), which fails 1; a slot of the
grown scratch that still holds the S = 2049 launch's data is another sample's and fails 1 at S = 97 and the comparison with a fresh
handle.  An item dropped by the odd second wave or by the last workgroup of 1 or 3 waves leaves its chunk out of the sample: 1 fails.
CPU: the launch table (items mod 2 and mod 4) against the restated rule and `qc_sweep_desc_launch` with `wide` = 257, the soundness of
sharing references at a wide shape, that no check passes on zeros or on rows that look alike, and that checks 1 to 3 fail on arrays made
from the reference with a shifted, a stale or an unwritten sample (no faulty kernel is run on a device).  Measured worst ratios and times:
profiles/sweep_wide_every_sample_summary.txt."""
import ctypes as C
import time

import numpy as np
import pytest

import test_sweep as ts
import test_sweep_every_sample as te
import test_sweep_hvp as th
import test_sweep_hvp_every_sample as thes
import test_sweep_wide as tw
from test_sweep_every_sample import GROWTH, R, assert_launch
from test_sweep_hvp_every_sample import build_rows, check_hvp, launch_of, reference
from test_sweep_wide_noise_every_sample import layout_of

U = te.U
HESSIAN = dict(wide=True, wide_hessian=True)                            # wide = 257
# the tuple layout of test_sweep_every_sample.CASES
TABLE = {"wide-sqrt-301": te.CASES["wide-sqrt-301"],                    # 1505 items: 1 mod 2, 1 mod 4; scale = None with vscale given
         "wide-byS-683": te.CASES["wide-byS-683"],                      # 2049 items: the chunk count set by S; levels 12; fixed timestep
         "wide-one-2049": te.CASES["wide-one-2049"],                    # past the fill threshold, one chunk; a ket with a fidelity
         "wide-one-2049-kets3": te.KETS3["wide-one-2049-kets3"],        # the same without a fidelity
         "wide-sqrt-97": (("unitary", 16, 1, 1, False, True, 97, 38, U), True, (6, 7, 1), True)}      # full tiles, 16 columns, 679 items, a last chunk of 1
ITEMS = {"wide-sqrt-301": 1505, "wide-byS-683": 2049, "wide-one-2049": 2049, "wide-one-2049-kets3": 2049, "wide-sqrt-97": 679}
ITEMS_MOD_4 = {"wide-sqrt-301": 1, "wide-byS-683": 1, "wide-one-2049": 1, "wide-one-2049-kets3": 1, "wide-sqrt-97": 3}
LINEAR = ["wide-sqrt-301", "wide-one-2049-kets3"]


def timed_reference(rows):
    """`reference(rows)` of the narrow file (computed once, shared, frozen), with the CPU time of its first build on the record."""
    t0 = time.process_time()
    fresh = rows["name"] not in thes._REF
    r = reference(rows)
    if fresh:
        print(f"SWEEP-WIDE-HVP-EVERY reference {rows['name']}: recurrence route over {R} rows built in {time.process_time() - t0:.2f} s of CPU time")
    return r


# ---------------------------------------------------------------------------------------------------------------------------------
#  CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_wide_hvp_launch_table(qc):
    """Every case sits on the edge it is named for, by the restated rule and by `qc_sweep_desc_launch` with `wide` = 257: odd item counts
    for the two-wave totals kernel, counts that are no multiple of 4 for the four-wave walk, both sides of the fill threshold, a last
    chunk of 1, the growth sequence; no S whose class map nobody checks."""
    L = qc._lib
    assert L.QC_SWEEP_WIDE | L.QC_SWEEP_WIDE_HESSIAN == 257
    want = {"wide-sqrt-301": (301, (5, 5, 3), True), "wide-byS-683": (683, (4, 3, 3), False), "wide-one-2049": (2049, (5, 1, 5), False),
            "wide-one-2049-kets3": (2049, (5, 1, 5), False), "wide-sqrt-97": (97, (6, 7, 1), True)}
    assert list(TABLE) == list(want) == list(ITEMS) == list(ITEMS_MOD_4)
    for name, (spec, wide, (chunk, n_chunks, last), by_sqrt) in TABLE.items():
        _, levels, m, _, _, _, S, T, _ = spec
        assert wide and 16 < 2 * levels <= 32 and (S, (chunk, n_chunks, last), by_sqrt) == want[name], name
        assert tw.wide_launch(2 * levels, m, S, T, True) == dict(mfma=True, chunk=chunk, n_chunks=n_chunks, last=last, by_sqrt=by_sqrt), name
        assert ts.sweep_launch(16, m, S, T) == tw.wide_launch(2 * levels, m, S, T, True)       # the rule with fill 2048, whatever the size
        assert (n_chunks - 1) * chunk + last == T - 1
        assert S * n_chunks == ITEMS[name] and ITEMS[name] % 2 == 1 and ITEMS[name] % 4 == ITEMS_MOD_4[name] != 0, name
        D = tw._wdesc(qc, 257, N=levels, m=m, T=T, cols=1)
        mf, ch, nch = C.c_int32(), C.c_int64(), C.c_int64()
        assert L.lib.qc_sweep_desc_launch(C.byref(D.d), S, C.byref(mf), C.byref(ch), C.byref(nch)) == L.QC_OK
        assert (bool(mf.value), ch.value, nch.value) == (True, chunk, n_chunks), name
    f = {k: TABLE[k][2] for k in TABLE}
    assert all(f[k][1] % 2 == 1 and f[k][1] > 1 for k in ("wide-sqrt-301", "wide-byS-683", "wide-sqrt-97"))      # workgroups straddle samples
    assert -(-ts.SWEEP_FILL // 683) == 3 == f["wide-byS-683"][1] and f["wide-byS-683"][1] < 4                    # set by S, not by sqrt(11)
    assert f["wide-one-2049"][1] == 1 and 683 < ts.SWEEP_FILL < 2049                                             # both sides of the fill threshold
    assert f["wide-sqrt-97"] == (6, 7, 1) and {ITEMS_MOD_4[k] for k in TABLE} == {1, 3}                          # a last chunk of 1
    sp = TABLE["wide-sqrt-97"][0]
    assert 2 * sp[1] == 32 and sp[0] == "unitary" and sp[4] is False                                             # full 2 x 2 tiles, 16 state columns
    assert TABLE["wide-sqrt-301"][0][4] is False and TABLE["wide-byS-683"][0][5] is False and TABLE["wide-byS-683"][0][1] == 12
    assert TABLE["wide-one-2049"][0][8] is not None and TABLE["wide-one-2049-kets3"][0][8] is None
    # no S here whose class map test_sweep_every_sample.test_classes_reach_both_ends leaves unchecked
    assert {TABLE[k][0][6] for k in TABLE} | set(GROWTH) <= {te.CASES[k][0][6] for k in te.CASES} | set(te.GROWTH)
    # the scratch-growth sequence on one handle at T = 24: grown twice, then reused at a smaller size
    sp = TABLE["wide-sqrt-301"][0]
    assert sp[7] == 24 and [tw.wide_launch(2 * sp[1], sp[2], S, 24)["n_chunks"] for S in GROWTH] == [5, 1, 5]
    assert GROWTH[0] * 5 < GROWTH[1] * 1 and GROWTH[2] * 5 < GROWTH[0] * 5
    assert set(LINEAR) <= set(TABLE)


def test_wide_hvp_reference_reuse_is_sound(qc):
    """The narrow file's check on one wide shape (9 levels, a subspace fidelity): equal rows give bit-equal recurrence references,
    distinct rows differ, the cotangent's direction matters on its own."""
    thes.assert_reference_reuse_is_sound(qc, "wide-hvp-reuse", ("unitary", 9, 2, 1, True, True, R, 5, ("unitary", [0, 1, 3, 4], "abs")))


@pytest.mark.parametrize("name", list(TABLE))
def test_wide_hvp_rows_are_not_vacuous(qc, name):
    """The narrow file's floors on the wide rows: class maxima >= 1e-2 (tgrad_samples) and >= 1e-1 (tgrad_init), classes >= 1e-3 apart."""
    thes.assert_rows_are_not_vacuous(qc, name, TABLE)


def test_the_checks_see_a_shifted_a_stale_and_an_unwritten_sample(qc):
    """Checks 1 to 3 on arrays made here from the reference at S = 2049, no device: they pass on ref[cls] with its own plain sum, and fail
    when every sample holds its neighbour's rows (a scratch slot one sample off), when one sample holds the rows of the sample 301 places
    before it (a slot left from an earlier, smaller launch), when one sample keeps the prefill, and when tgrad is a sum in another order."""
    name = "wide-one-2049-kets3"
    rows = build_rows(qc, name, TABLE)
    c = launch_of(rows, TABLE[name][0][6])
    cls, r = c["cls"], timed_reference(rows)
    sw = layout_of(rows)
    good = {k: np.ascontiguousarray(r[k][cls]) for k in ("tgrad_samples", "tgrad_init")}
    good["tgrad"] = th.scatter(th.layout(sw), good["tgrad_samples"])
    thes.check_values(sw, good, rows, c, "made up")
    assert cls[1000] != cls[1000 - 301]
    for what in ("shifted", "stale", "unwritten"):
        bad = {k: v.copy() for k, v in good.items()}
        for k in ("tgrad_samples", "tgrad_init"):
            if what == "shifted":
                bad[k] = np.roll(good[k], 1, axis=0)
            else:
                bad[k][1000] = good[k][1000 - 301] if what == "stale" else -7.0
        bad["tgrad"] = th.scatter(th.layout(sw), bad["tgrad_samples"])
        with pytest.raises(AssertionError, match="largest errors at"):
            thes.check_values(sw, bad, rows, c, what)
    order = dict(good, tgrad=th.scatter(th.layout(sw), good["tgrad_samples"][::-1]))
    assert not np.array_equal(order["tgrad"], good["tgrad"])
    with pytest.raises(AssertionError, match="plain sum"):
        thes.check_values(sw, order, rows, c, "another order")


# ---------------------------------------------------------------------------------------------------------------------------------
#  GPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TABLE))
def test_wide_hvp_every_sample(qc, name):
    t_wall = time.perf_counter()
    rows = build_rows(qc, name, TABLE)
    spec = TABLE[name][0]
    c = launch_of(rows, spec[6])
    timed_reference(rows)
    sw = ts.make_sweep(qc, rows, **HESSIAN)
    try:
        want = assert_launch(sw, name, table=TABLE)
        items = c["S"] * want["n_chunks"]
        assert items == ITEMS[name] and items % 2 == 1 and items % 4 == ITEMS_MOD_4[name]
        assert sw._desc.wide == 257 and sw.hvp_supported and sw.hvp_unsupported_reason is None and sw.vjp_supported and not sw.jvp_supported
        if not spec[4]:
            assert c["scale"] is None and (c["vscale"] != 0).all()              # the cl = 1, vcl != 0 path
        if not spec[5]:
            assert c["vdts"] is None and sw.n_deriv == spec[2]                  # the h_n = h path
        check_hvp(sw, rows, c, f"wide-every/{name}")
    finally:
        sw.close()
    print(f"SWEEP-WIDE-HVP-EVERY wide-every/{name}: {time.perf_counter() - t_wall:.2f} s of wall time")


@pytest.mark.gpu
@pytest.mark.parametrize("name", LINEAR)
def test_wide_hvp_linear_part_every_sample(qc, name):
    """5: with only vcot given, tgrad_samples[s] and tgrad_init[s] are the wide pullback's grad_samples[s] and grad_init[s] with
    cot = vcot on the same handle, every sample, at 2e-9 max(1, max |.|_s)."""
    t_wall = time.perf_counter()
    thes.linear_part(qc, name, TABLE, **HESSIAN)
    print(f"SWEEP-WIDE-HVP-EVERY wide-every/{name} linear part: {time.perf_counter() - t_wall:.2f} s of wall time")


@pytest.mark.gpu
def test_wide_hvp_scratch_growth_every_sample(qc):
    """One `wide` = 259 handle at S = 301, then 2049, then 97 with T = 24: 5 chunks, 1, 5 again, so dTot / dXs / dLs (shared with `grad`
    and `vjp`), dTotJ (2048 doubles an item) and dXsT / dLsT / dTGsamp grow twice and are then reused at a smaller size.  At every S, in
    this order: `grad_device`, `hvp_device`, `vjp_device`.  The Hessian product passes checks 1 to 3, and it and the calls around it carry
    the bits of fresh handles."""
    t_wall = time.perf_counter()
    name = "wide-sqrt-301"
    timed_reference(build_rows(qc, name, TABLE))
    thes.scratch_growth(qc, name, TABLE, wide_params=True, **HESSIAN)
    print(f"SWEEP-WIDE-HVP-EVERY wide-every/{name} growth: {time.perf_counter() - t_wall:.2f} s of wall time")
