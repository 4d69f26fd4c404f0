"""Parameter gradients and parameter cotangents in the "mfma64-sweep" form (`qc_sweep64_grad_kernel<true>` of csrc/qc_sweep64_grad.hip:
`RolloutSweep(..., wide=True, wide64=True, wide64_grad=True, wide64_params=True)`, `wide` = 11265) at launches of 250 .. 510 workgroups,
EVERY sample against the CPU reference: the method of tests/test_sweep_every_sample.py (read its header: R = 8 rows of (theta, scale,
cotangent), sample s carries row classes(S)[s], the forward-mode references once for the R rows, every output buffer prefilled with -7),
its helpers and those of test_sweep_wide64_grad_every_sample.py and test_sweep_wide_params_every_sample.py imported.
tests/test_sweep_wide64_param_grad.py checks the arithmetic at S <= 5 and, with m = p = 1 and T = 3, at S = 255 .. 257; what is checked
here is the mapping from a (sample, chunk) workgroup to its share par[item][p + m] (item = blockIdx.x = s n_chunks + c; perturbations,
then drives: lane k < m stores at p + k, lane nd + q at q) and from there through `qc_sweep_par_reduce_kernel` to row s of grad_theta /
grad_scale, with several chunks of several intervals over many samples, on both sides of the fill constant 256:
  * S = 50, T = 26: five chunks of five intervals (capped by sqrt(25)), 250 workgroups; nd = m + 1;
  * S = 100, T = 27: chunks of 9, 9 and 8 (set by S), 300 workgroups: more than there are compute units, a ragged last chunk;
  * S = 255, T = 26, fixed timestep: chunks of 13 and 12, 510 workgroups; nd = m, the perturbation lanes directly behind the drives;
  * S = 257, T = 26, m = 3, p = 1, `scale = NULL`: one chunk of 25 intervals.
All at N = 17 (2N = 34).  p = m = 2 where it can be: a share written or reduced as [drives | perturbations] has the right shape and is
caught by its values alone.  One state column with the ket fidelity for `qc_sweep_grad_params`; each case's "-kets2" twin (two columns,
no fidelity: `grad` refuses) for the pullback's grad_theta / grad_scale.
  1. every row of grad_theta, grad_scale and grad_samples (pullback: also grad_init and finals) against the reference of its class, by
     the assertion and tolerance the output has in its own test file (`tp._assert_params`: 1e-9 max(1, A_s); `tv.assert_samples`,
     `tg._assert_samples`, `tv.assert_init`, `ts._assert_states`);
  2. every row carries the bits of the first sample of its class;
  3. fids, J and the dense gradients against the reference; `param_grad` and a call for grad_theta / grad_scale alone (the walk's
     gs == NULL path) return the bits of the full call;
  4. one handle at S = 50, 300, 255 (250, 300, 510 shares at other strides) passes 1 - 3 at every S and carries a fresh handle's bits.
No tolerance is new.  CPU: the launch table with and without bit 13, the class map at S = 100, that every class's grad_theta / grad_scale
reach 1e-2 and any two classes lie >= 1e-3 apart (the floors of the other every-sample files: 10^6 bounds), and that the checks fail on
a shifted, a stale, an unwritten and a last-bit-off sample, on grad_theta and grad_scale exchanged, and on a sample whose last chunk's
share is left out, all made from the reference.  Measured worst ratios: profiles/sweep_wide64_params_every_sample_summary.txt."""
import ctypes as C
import itertools
import time

import numpy as np
import pytest

import test_sweep as ts
import test_sweep_every_sample as tes
import test_sweep_grad as tg
import test_sweep_param_grad as tp
import test_sweep_vjp as tv
import test_sweep_wide as tw
import test_sweep_wide64 as t64
import test_sweep_wide64_grad_every_sample as tge
import test_sweep_wide_params_every_sample as twp
from test_sweep_every_sample import KET, R, assert_class_bits, assert_launch, every_sample, expand

WIDE_G = tge.WIDE                  # 3073
WIDE = WIDE_G | 8192               # 11265
HANDLE = dict(wide=True, wide64=True, wide64_grad=True, wide64_params=True)
FORM = "64par-every"               # the key of test_sweep_vjp.reference's cache for this file's rows
# The name seeds the draw ("-a", "-c": under the plain names a class's largest grad_theta / grad_scale or two classes' distance misses the floor).
# name: ((state, levels, m, p, scale given, free timestep, S, T, fidelity), wide, (chunk, n_chunks, last chunk), chunk count capped by sqrt(T - 1))
TABLE = {
    "p64-sqrt-50": (("ket", 17, 2, 2, True, True, 50, 26, KET), WIDE, (5, 5, 5), True),
    "p64-byS-100-a": (("ket", 17, 2, 2, True, True, 100, 27, KET), WIDE, (9, 3, 8), False),
    "p64-two-255-c": (("ket", 17, 2, 2, True, False, 255, 26, KET), WIDE, (13, 2, 12), False),
    "p64-one-257-a": (("ket", 17, 3, 1, False, True, 257, 26, KET), WIDE, (25, 1, 25), False),
}
KETS2 = {k + "-kets2": (("kets3",) + v[0][1:8] + (None,),) + v[1:] for k, v in TABLE.items()}
ITEMS = {"p64-sqrt-50": 250, "p64-byS-100-a": 300, "p64-two-255-c": 510, "p64-one-257-a": 257}
GROWTH = tge.GROWTH64              # (50, 300, 255) on one handle at T = 26: 5 chunks, 1, 2 -- 250, 300 and 510 shares
NEW_S = (100,)                     # the S whose class map no other file checks
GROWN = "p64-sqrt-50"


def rule64(spec, S):
    return t64.launch64(2 * spec[1], spec[2], S, spec[7], WIDE)


def build_rows(qc, name):
    return tge.build_rows(qc, name, TABLE, KETS2)


def table_of(name):
    return TABLE if name in TABLE else KETS2


def param_sums(rows):
    """(grad_theta, grad_scale) of the R rows from `tp.reference` (perturbations, then drives)."""
    sums = tp.reference(rows)[1]
    return sums[:, :rows["p"]], sums[:, rows["p"]:]


# ---------------------------------------------------------------------------------------------------------------------------------
#  CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_wide64_params_launch_table(qc):
    """The shapes sit where they are named for, by the restated rule and by `qc_sweep_desc_launch`, with and without bit 13."""
    L = qc._lib
    assert WIDE == 11265 and WIDE_G == 3073 and set(ITEMS) == set(TABLE) and len(KETS2) == len(TABLE)
    for name, (spec, wide, (chunk, n_chunks, last), by_sqrt) in {**TABLE, **KETS2}.items():
        _, N, m, p, _, free, S, T, _ = spec
        assert wide == WIDE and 2 * N == 34
        assert rule64(spec, S) == dict(mfma=True, chunk=chunk, n_chunks=n_chunks, last=last, by_sqrt=by_sqrt), name
        assert t64.launch64(2 * N, m, S, T, WIDE_G) == rule64(spec, S), name
        assert (n_chunks - 1) * chunk + last == T - 1 and S * n_chunks == ITEMS[name.replace("-kets2", "")]
        for w in (WIDE, WIDE_G):               # the bit does not touch the launch rule
            D = tw._wdesc(qc, w, N=N, m=m, T=T, cols=1)
            mf, ch, nch = C.c_int32(), C.c_int64(), C.c_int64()
            assert L.lib.qc_sweep_desc_launch(C.byref(D.d), S, C.byref(mf), C.byref(ch), C.byref(nch)) == L.QC_OK
            assert (bool(mf.value), ch.value, nch.value) == (True, chunk, n_chunks), (name, w)
    f = {k: TABLE[k][2] for k in TABLE}
    sp = {k: TABLE[k][0] for k in TABLE}
    assert -(-t64.FILL64 // 50) == 6 > f["p64-sqrt-50"][1] == 5 and TABLE["p64-sqrt-50"][3]                      # capped by sqrt(25)
    assert -(-t64.FILL64 // 100) == 3 == f["p64-byS-100-a"][1] < 6 and f["p64-byS-100-a"][2] < f["p64-byS-100-a"][0]   # set by S, ragged
    assert ITEMS["p64-byS-100-a"] > 256                                                                          # more workgroups than CUs
    assert f["p64-two-255-c"][1] == 2 and f["p64-one-257-a"][1] == 1 and 255 < t64.FILL64 < 257
    assert all(c[0] > 1 for c in f.values())                                                                     # several intervals a chunk
    assert not sp["p64-two-255-c"][5] and all(sp[k][5] for k in TABLE if k != "p64-two-255-c")                   # nd = m once, m + 1 else
    assert not sp["p64-one-257-a"][4] and (sp["p64-one-257-a"][2], sp["p64-one-257-a"][3]) == (3, 1)             # scale = NULL, m != p
    assert all(sp[k][2] == sp[k][3] == 2 for k in TABLE if k != "p64-one-257-a")                                 # the halves of a share exchange
    seq = [rule64(sp[GROWN], S)["n_chunks"] for S in GROWTH]
    assert seq == [5, 1, 2] and [S * n for S, n in zip(GROWTH, seq)] == [250, 300, 510]
    tes.assert_classes_reach_both_ends(NEW_S)


@pytest.mark.parametrize("name", list(TABLE))
def test_wide64_params_rows_are_not_vacuous(qc, name):
    """No class passes for another and no output is all but zero: for grad_theta and grad_scale, of `param_grad` and of the pullback
    separately, every class's largest value is >= 1e-2 and any two classes' references differ by >= 1e-3 in max-norm, 10^6 times the
    bound of a derivative of size one."""
    t0 = time.process_time()
    rows = build_rows(qc, name)
    gth, gsc = param_sums(rows)
    print(f"SWEEP-WIDE64-PARAMS-EVERY reference of every/{name} (param_terms_forward, 8 rows): {time.process_time() - t0:.2f} s of CPU time")
    t0 = time.process_time()
    rows2 = build_rows(qc, name + "-kets2")
    r2 = tv.reference(rows2, FORM)
    print(f"SWEEP-WIDE64-PARAMS-EVERY reference of every/{name}-kets2 (pullback_forward, 8 rows): {time.process_time() - t0:.2f} s of CPU time")
    assert gth.shape == (R, rows["p"]) and gsc.shape == (R, rows["m"]) and r2["grad_theta"].shape == gth.shape and r2["grad_scale"].shape == gsc.shape
    # the outputs that ride along (checked by the same class map) hold the same floors
    along = dict(grad_samples=tes.ref_grad(rows), vjp_grad_samples=r2["grad_samples"], vjp_grad_init=r2["grad_init"],
                 finals=np.ascontiguousarray(tes.ref_finals(rows2)[0].T))
    for key, a in dict(grad_theta=gth, grad_scale=gsc, vjp_grad_theta=r2["grad_theta"], vjp_grad_scale=r2["grad_scale"], **along).items():
        a = a.reshape(R, -1)
        small = np.abs(a).max(axis=1).min()
        apart = min(np.abs(a[i] - a[j]).max() for i, j in itertools.combinations(range(R), 2))
        print(f"SWEEP-WIDE64-PARAMS-EVERY every/{name} {key}: smallest class maximum {small:.3e}, smallest distance between two classes {apart:.3e}")
        assert small >= 1e-2 and apart >= 1e-3, (name, key)


def test_the_checks_see_a_wrong_share_a_dropped_chunk_or_a_misplaced_sample(qc):
    """Checks 1 and 2 on arrays made here from the reference of p64-sqrt-50 (S = 50, five chunks of five intervals, p = m = 2).  They pass
    on ref[cls].  They fail when every sample holds its neighbour's value (a share one item off), when one sample holds another launch's
    value for that slot (stale dPart: the class map of S = 300), when one sample keeps the prefill, when one sample differs from its class
    in the last bit (by the bits alone), when grad_theta and grad_scale are exchanged (the share laid out [drives | perturbations]: by
    the values alone), and when one sample's sums leave out the last chunk's share, or any other chunk's (by the values)."""
    name = GROWN
    rows, rows2 = build_rows(qc, name), build_rows(qc, name + "-kets2")
    spec, _, (chunk, n_chunks, last), _ = TABLE[name]
    S, p, m = spec[6], spec[3], spec[2]
    c = expand(rows, S)
    cls = c["cls"]
    case = tes.params_case(rows, c)
    terms = tp.reference(rows)[0]
    assert p == m == 2 and terms.shape == (R, n_chunks * chunk, p + m) and last == chunk
    ref_th, ref_sc = param_sums(rows)
    r2 = tv.reference(rows2, FORM)

    def values(gth, gsc, what):
        tp._assert_params(gth, gsc, case, what)

    def values_vjp(gth, gsc, what):
        every_sample(tv.assert_samples, gth, r2["grad_theta"][cls], cls, what + " grad_theta")
        every_sample(tv.assert_samples, gsc, r2["grad_scale"][cls], cls, what + " grad_scale")

    def bits(gth, gsc, what):
        assert_class_bits(gth, cls, what + " grad_theta")
        assert_class_bits(gsc, cls, what + " grad_scale")

    def fails(check, *args):
        try:
            check(*args)
        except AssertionError:
            return True
        return False

    other = tes.classes(300)[:S]
    s0 = int(np.flatnonzero(other != cls)[0])
    for route, (rth, rsc), by_values in (("param_grad", (ref_th, ref_sc), values), ("pullback", (r2["grad_theta"], r2["grad_scale"]), values_vjp)):
        good = np.ascontiguousarray(rth[cls]), np.ascontiguousarray(rsc[cls])
        by_values(*good, f"made up {route}")
        bits(*good, f"made up {route}")
        stale, unwritten, last_bit = [a.copy() for a in good], [a.copy() for a in good], [a.copy() for a in good]
        stale[0][s0], stale[1][s0] = rth[other[s0]], rsc[other[s0]]
        unwritten[0][20] = unwritten[1][20] = -7.0
        last_bit[1][20, 1] = np.nextafter(last_bit[1][20, 1], 2.0)
        wrong = dict(shifted=[np.roll(a, 1, axis=0) for a in good], stale=stale, unwritten=unwritten, exchanged=[good[1], good[0]])
        for what, bad in wrong.items():
            assert fails(by_values, *bad, f"{what} {route}"), (route, what)
        # exchanged halves keep every sample at its class's bits, one last bit keeps every value inside its bound: each needs its own check
        assert not fails(bits, *wrong["exchanged"], f"exchanged {route}") and all(fails(bits, *wrong[k], f"{k} {route}") for k in ("shifted", "stale", "unwritten"))
        assert fails(bits, *last_bit, f"last bit {route}") and not fails(by_values, *last_bit, f"last bit {route}")
    with pytest.raises(AssertionError, match="largest errors at"):
        values_vjp(*[np.roll(a, 1, axis=0) for a in (r2["grad_theta"][cls], r2["grad_scale"][cls])], "shifted")
    # a chunk's share left out of one sample's sums: every chunk of every class carries >= 1e-6 in some parameter, a thousand bounds
    shares = terms.reshape(R, n_chunks, chunk, p + m).sum(axis=2)
    print(f"SWEEP-WIDE64-PARAMS-EVERY every/{name}: smallest over (class, chunk) of the largest share among the parameters {np.abs(shares).max(axis=2).min():.3e}")
    assert np.abs(shares).max(axis=2).min() >= 1e-6 and tp.magnitudes(terms).max() < 1e3
    np.testing.assert_allclose(shares.sum(axis=1), np.concatenate([ref_th, ref_sc], axis=1), rtol=0, atol=1e-13)
    for s in (20, 0, S - 1):
        for drop in range(n_chunks - 1, -1, -1):
            kept = np.delete(shares[cls[s]], drop, axis=0).sum(axis=0)
            gth, gsc = ref_th[cls].copy(), ref_sc[cls].copy()
            gth[s], gsc[s] = kept[:p], kept[p:]
            assert fails(values, gth, gsc, f"sample {s} without chunk {drop}"), (s, drop)


# ---------------------------------------------------------------------------------------------------------------------------------
#  GPU
# ---------------------------------------------------------------------------------------------------------------------------------
def check_params(qc, sw, rows, c, what):
    """`twp.check_params` (one `qc_sweep_grad_params` call with every output, `param_grad` as callers use it), then a call for grad_theta
    and grad_scale alone -- the walk's gs == NULL path at this launch: the bits of the full call."""
    o = twp.check_params(qc, sw, rows, c, what)
    assert o["gth"].shape == (c["S"], rows["p"]) and o["gsc"].shape == (c["S"], rows["m"]) and o["gs"].shape == (c["S"], c["T"] - 1, sw.n_deriv)
    part = tp._raw(qc, sw, sw.pack(c["controls"], c["dts"]), c["init"], c["theta"], c["scale"], c["weights"], want=("gth", "gsc"))
    for k in ("gth", "gsc"):
        np.testing.assert_array_equal(part[k], o[k], err_msg=f"{what}: {k} asked for alone")
    return o


def check_vjp_params(sw, rows, c, what):
    """`twp.check_vjp_params` and the `finals` check of `tes.check_vjp`."""
    out = twp.check_vjp_params(sw, rows, c, what, form=FORM)
    every_sample(ts._assert_states, out["finals"], tes.ref_finals(rows)[0].T[c["cls"]], c["cls"], f"SWEEP-EVERY {what} finals")
    return out


def make(qc, rows, name, S=None):
    sw = ts.make_sweep(qc, rows, **HANDLE)
    try:
        want = assert_launch(sw, name, S, table=table_of(name), rule=rule64, kernel="mfma64-sweep")
        assert sw._desc.wide == WIDE and sw.wide64_params and sw.vjp_supported and rows["n"] == 34
        if S is None:
            assert table_of(name)[name][0][6] * want["n_chunks"] == ITEMS[name.replace("-kets2", "")]
    except BaseException:
        sw.close()
        raise
    return sw


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TABLE))
def test_wide64_param_grad_every_sample(qc, name):
    t_wall = time.perf_counter()
    rows = build_rows(qc, name)
    spec = TABLE[name][0]
    c = expand(rows, spec[6])
    sw = make(qc, rows, name)
    try:
        assert sw.grad_supported and sw.cols == 1 and (sw.m, sw.p) == (spec[2], spec[3]) and sw.n_deriv == spec[2] + spec[5]
        assert (c["scale"] is None) == (not spec[4]) and (np.ndim(c["dts"]) == 1) == spec[5]
        check_params(qc, sw, rows, c, f"64/every/{name} params")
    finally:
        sw.close()
    print(f"SWEEP-WIDE64-PARAMS-EVERY 64/every/{name} params: {time.perf_counter() - t_wall:.2f} s of wall time")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(KETS2))
def test_wide64_vjp_params_every_sample(qc, name):
    t_wall = time.perf_counter()
    rows = build_rows(qc, name)
    c = expand(rows, KETS2[name][0][6])
    sw = make(qc, rows, name)
    try:
        assert not sw.grad_supported and "no fidelity" in sw.grad_unsupported_reason and sw.cols == 2 and sw.ns == 68
        check_vjp_params(sw, rows, c, f"64/every/{name} pullback")
    finally:
        sw.close()
    print(f"SWEEP-WIDE64-PARAMS-EVERY 64/every/{name} pullback: {time.perf_counter() - t_wall:.2f} s of wall time")


@pytest.mark.gpu
def test_wide64_params_scratch_growth_every_sample(qc):
    """One handle at S = 50, then 300, then 255 with T = 26: 5 chunks, 1, 2, so dPart holds 250 shares, is grown to 300 and to 510 at
    other strides (and dXs / dLs / dTot / dGsamp with it).  At every S the outputs of `qc_sweep_grad_params` and, on a "-kets2" handle
    grown the same way, of the pullback pass checks 1 - 3 against the reference and carry the bits of a fresh handle's."""
    t_wall = time.perf_counter()
    name = GROWN
    rows, rows2 = build_rows(qc, name), build_rows(qc, name + "-kets2")
    sw, sw2 = make(qc, rows, name), None
    try:
        sw2 = make(qc, rows2, name + "-kets2")
        seen = []
        for S in GROWTH:
            c, c2 = expand(rows, S), expand(rows2, S)
            seen.append(assert_launch(sw, name, S, table=TABLE, rule=rule64, kernel="mfma64-sweep")["n_chunks"])
            assert assert_launch(sw2, name + "-kets2", S, table=KETS2, rule=rule64, kernel="mfma64-sweep")["n_chunks"] == seen[-1]
            what = f"64/every/{name} grown to S = {S}"
            o = check_params(qc, sw, rows, c, what + " params")
            out = check_vjp_params(sw2, rows2, c2, what + " pullback")
            fresh, fresh2 = ts.make_sweep(qc, rows, **HANDLE), ts.make_sweep(qc, rows2, **HANDLE)
            try:
                o2 = tp._raw(qc, fresh, fresh.pack(c["controls"], c["dts"]), c["init"], c["theta"], c["scale"], c["weights"])
                out2 = tv.device_call(fresh2, fresh2.pack(c2["controls"], c2["dts"]), c2, list(out))
            finally:
                fresh.close()
                fresh2.close()
            assert o["J"] == o2["J"]
            for k in ("fids", "grad", "gs", "gth", "gsc"):
                np.testing.assert_array_equal(o[k], o2[k], err_msg=f"S = {S}: {k}")
            for k in out:
                np.testing.assert_array_equal(out[k], out2[k], err_msg=f"S = {S}: pullback {k}")
        assert seen == [5, 1, 2]
    finally:
        sw.close()
        if sw2 is not None:
            sw2.close()
    print(f"SWEEP-WIDE64-PARAMS-EVERY 64/every/{name} growth: {time.perf_counter() - t_wall:.2f} s of wall time")
