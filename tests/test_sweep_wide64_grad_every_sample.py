"""Sweep gradients and pullbacks in the "mfma64-sweep" form (`qc_sweep64_grad_kernel` of csrc/qc_sweep64_grad.hip behind the seeds at ld = 64:
`RolloutSweep(..., wide=True, wide64=True, wide64_grad=True)`, `wide` = 3073) at launches of 250 .. 510 workgroups, EVERY sample against the
CPU reference: the method of tests/test_sweep_every_sample.py (read its header: R = 8 rows of (theta, scale, cotangent), sample s carries
row classes(S)[s], the forward-mode references once for the R rows), its helpers imported.  tests/test_sweep_wide64_grad.py checks the
arithmetic at S <= 11 and three samples of S = 256; what is checked here is the mapping from a sample to a workgroup and to its slots:
item = blockIdx.x, s = item / n_chunks, x and lambda of the chunk's end at (s n_chunks + c) ns in dXs / dLs, the chunk total at
(s n_chunks + c) 4096, the per-interval store at gs[s][t][.], on both sides of the fill constant 256:
  * S = 300, T = 3: one chunk of two intervals;
  * S = 255 and S = 257, T = 5: two chunks of two intervals, and one chunk of four;
  * S = 50, T = 26: ceil(256 / S) = 6 chunks are wanted and ceil(sqrt(25)) = 5 are taken, five chunks of five intervals, 250 workgroups.
All at N = 17 (2N = 34: the third tile row almost empty), so that the CPU reference of eight rows stays short: one state column with the
ket fidelity for `grad`, two columns without a fidelity for `vjp` (test_sweep_wide.build makes one or three: the first two are kept).
  1. every row of grad_samples (vjp: grad_samples, grad_init, finals) against the reference of its class, by the assertion and tolerance
     the output has in its own test file (`check_grad` / `check_vjp` of test_sweep_every_sample.py);
  2. every row carries the bits of the first sample of its class;
  3. fids, J and the dense gradients against the reference; +0.0 outside the derivatives; the host entries return the device call's bits;
  4. every output buffer is prefilled with -7, so an unwritten sample fails 1.
No tolerance is new.  CPU: the launch table, the class map at the new S, that any two classes' references lie >= 1e-3 apart (the floor of
the other every-sample files: 10^6 bounds), and that checks 1 and 2 fail on a shifted, a stale, an unwritten and a last-bit-off sample
made from the reference."""
import ctypes as C
import itertools
import time

import numpy as np
import pytest

import test_sweep as ts
import test_sweep_every_sample as te
import test_sweep_grad as tg
import test_sweep_vjp as tv
import test_sweep_wide as tw
import test_sweep_wide64 as t64
from test_sweep_every_sample import KET, R, assert_class_bits, assert_launch, every_sample, expand

WIDE = 1 | t64.W64 | 2048
HANDLE = dict(wide=True, wide64=True, wide64_grad=True)
# The name seeds the draw ("-c", "-h": under the plain names two classes' grad_samples lie 3e-4 .. 8e-4 apart, below the 1e-3 floor).
# name: ((state, levels, m, p, scale given, free timestep, S, T, fidelity), wide, (chunk, n_chunks, last chunk), chunk count capped by sqrt(T - 1))
TABLE = {
    "g64-one-300-c": (("ket", 17, 2, 1, True, True, 300, 3, KET), WIDE, (2, 1, 2), False),
    "g64-two-255-c": (("ket", 17, 2, 1, False, True, 255, 5, KET), WIDE, (2, 2, 2), False),
    "g64-one-257-h": (("ket", 17, 2, 1, True, False, 257, 5, KET), WIDE, (4, 1, 4), False),
    "g64-sqrt-50": (("ket", 17, 2, 1, True, True, 50, 26, KET), WIDE, (5, 5, 5), True),
}
KETS2 = {k + "-kets2": (("kets3",) + v[0][1:8] + (None,),) + v[1:] for k, v in TABLE.items()}
ITEMS = {"g64-one-300-c": 300, "g64-two-255-c": 510, "g64-one-257-h": 257, "g64-sqrt-50": 250}
GROWTH64 = (50, 300, 255)   # on one handle at T = 26: 5 chunks, 1, 2 -- 250, 300 and 510 slots
NEW_S = (50,)               # the S whose class map no other file checks (255, 257, 300: test_sweep_wide64_every_sample.py)


def rule64(spec, S):
    return t64.launch64(2 * spec[1], spec[2], S, spec[7], WIDE)


def build_rows(qc, name, table=None, kets2=None):
    """`te.build_rows`; the two-column rows keep the first two of the three kets and draw cotangents of that size.  `table`, `kets2`:
    another file's cases and their twins."""
    table, kets2 = TABLE if table is None else table, KETS2 if kets2 is None else kets2
    if name in table:
        return te.build_rows(qc, name, table)
    rows = te.build_rows(qc, name, kets2)
    n = rows["n"]
    rows["init"], rows["cols"] = np.ascontiguousarray(rows["init"][:2 * n]), 2
    rows["cot"] = tv.unit_cotangents(np.random.default_rng(7 + sum(map(ord, name))), R, 2 * n)
    return rows


# ---------------------------------------------------------------------------------------------------------------------------------
#  CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_wide64_grad_launch_table(qc):
    L = qc._lib
    assert set(ITEMS) == set(TABLE) and len(KETS2) == len(TABLE)
    for name, (spec, wide, (chunk, n_chunks, last), by_sqrt) in {**TABLE, **KETS2}.items():
        _, N, m, _, _, _, S, T, _ = spec
        assert wide == WIDE == 3073 and 2 * N == 34
        assert rule64(spec, S) == dict(mfma=True, chunk=chunk, n_chunks=n_chunks, last=last, by_sqrt=by_sqrt), name
        assert (n_chunks - 1) * chunk + last == T - 1 and S * n_chunks == ITEMS[name.replace("-kets2", "")]
        for w in (WIDE, 1 | t64.W64):          # the bit does not touch the launch rule
            D = tw._wdesc(qc, w, N=N, m=m, T=T, cols=1)
            mf, ch, nch = C.c_int32(), C.c_int64(), C.c_int64()
            assert L.lib.qc_sweep_desc_launch(C.byref(D.d), S, C.byref(mf), C.byref(ch), C.byref(nch)) == L.QC_OK
            assert (bool(mf.value), ch.value, nch.value) == (True, chunk, n_chunks), name
    f = {k: TABLE[k][2] for k in TABLE}
    assert f["g64-one-300-c"][1] == 1 and f["g64-two-255-c"][1] == 2 and f["g64-one-257-h"][1] == 1 and 255 < t64.FILL64 < 257
    assert -(-t64.FILL64 // 50) == 6 > f["g64-sqrt-50"][1] == 5 and TABLE["g64-sqrt-50"][3]
    sp = TABLE["g64-sqrt-50"][0]
    seq = [rule64(sp, S)["n_chunks"] for S in GROWTH64]
    assert seq == [5, 1, 2] and [S * n for S, n in zip(GROWTH64, seq)] == [250, 300, 510]
    te.assert_classes_reach_both_ends(NEW_S)


@pytest.mark.parametrize("name", list(TABLE))
def test_wide64_grad_rows_are_not_vacuous(qc, name):
    """No class passes for another: any two classes' references differ by >= 1e-3 in max-norm, 10^6 times the bound of a derivative of
    size one; every class has derivatives of at least 1e-2."""
    t0 = time.process_time()
    rows, rows2 = build_rows(qc, name), build_rows(qc, name + "-kets2")
    r2 = tv.reference(rows2, "64")
    refs = dict(grad_samples=te.ref_grad(rows), vjp_grad_samples=r2["grad_samples"], vjp_grad_init=r2["grad_init"],
                finals=np.ascontiguousarray(te.ref_finals(rows2)[0].T))
    print(f"SWEEP-WIDE64-GRAD-EVERY references of every/{name}: {time.process_time() - t0:.2f} s of CPU time")
    for key, a in refs.items():
        a = a.reshape(R, -1)
        small = np.abs(a).max(axis=1).min()
        apart = min(np.abs(a[i] - a[j]).max() for i, j in itertools.combinations(range(R), 2))
        print(f"SWEEP-WIDE64-GRAD-EVERY every/{name} {key}: smallest class maximum {small:.3e}, smallest distance between two classes {apart:.3e}")
        assert small >= 1e-2 and apart >= 1e-3, (name, key)


def test_the_checks_see_a_shifted_a_stale_or_an_unwritten_sample(qc):
    """Checks 1 and 2 on arrays made here from the reference at S = 50: they pass on ref[cls], and fail when every sample holds its
    neighbour's value (a slot one item off), when one sample holds another launch's value for that slot (stale scratch: the class map of
    another S), when one sample keeps the prefill, and when one sample differs from its class in the last bit."""
    name = "g64-sqrt-50"
    rows = build_rows(qc, name)
    c = expand(rows, 50)
    cls = c["cls"]
    good = np.ascontiguousarray(te.ref_grad(rows)[cls])

    def check(gs, what):
        every_sample(tg._assert_samples, gs, te.ref_grad(rows)[cls], cls, what)
        assert_class_bits(gs, cls, what)

    check(good, "made up")
    stale, unwritten, last_bit = good.copy(), good.copy(), good.copy()
    other = te.classes(300)[:50]
    s0 = int(np.flatnonzero(other != cls)[0])
    stale[s0] = te.ref_grad(rows)[other[s0]]
    unwritten[20] = -7.0
    last_bit[20, 3, 1] = np.nextafter(last_bit[20, 3, 1], 2.0)
    for what, bad in (("shifted", np.roll(good, 1, axis=0)), ("stale", stale), ("unwritten", unwritten), ("last bit", last_bit)):
        with pytest.raises(AssertionError):
            check(bad, what)
    with pytest.raises(AssertionError, match="largest errors at"):
        check(np.roll(good, 1, axis=0), "shifted")


# ---------------------------------------------------------------------------------------------------------------------------------
#  GPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TABLE))
def test_wide64_grad_every_sample(qc, name):
    t_wall = time.perf_counter()
    rows = build_rows(qc, name)
    spec = TABLE[name][0]
    c = expand(rows, spec[6])
    sw = ts.make_sweep(qc, rows, **HANDLE)
    try:
        want = assert_launch(sw, name, table=TABLE, rule=rule64, kernel="mfma64-sweep")
        assert sw._desc.wide == WIDE and sw.grad_supported and c["S"] * want["n_chunks"] == ITEMS[name] and rows["n"] == 34 and sw.cols == 1
        assert (c["scale"] is None) == (not spec[4]) and (np.ndim(c["dts"]) == 1) == spec[5]
        te.check_grad(sw, rows, c, f"64/every/{name}")
    finally:
        sw.close()
    print(f"SWEEP-WIDE64-GRAD-EVERY 64/every/{name} grad: {time.perf_counter() - t_wall:.2f} s of wall time")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(KETS2))
def test_wide64_vjp_every_sample(qc, name):
    t_wall = time.perf_counter()
    rows = build_rows(qc, name)
    c = expand(rows, KETS2[name][0][6])
    sw = ts.make_sweep(qc, rows, **HANDLE)
    try:
        assert_launch(sw, name, table=KETS2, rule=rule64, kernel="mfma64-sweep")
        assert sw.vjp_supported and not sw.grad_supported and sw.cols == 2 and sw.ns == 68
        te.check_vjp(sw, rows, c, f"64/every/{name}", "64")
    finally:
        sw.close()
    print(f"SWEEP-WIDE64-GRAD-EVERY 64/every/{name} vjp: {time.perf_counter() - t_wall:.2f} s of wall time")


@pytest.mark.gpu
def test_wide64_grad_scratch_growth_every_sample(qc):
    """One handle at S = 50, then 300, then 255 with T = 26: 5 chunks, 1, 2, so dTot / dXs / dLs / dGsamp hold 250 slots, are grown to 300
    and to 510 at other strides.  At every S the outputs pass checks 1 - 3 and carry the bits of a fresh handle's."""
    name = "g64-sqrt-50"
    rows = build_rows(qc, name)
    sw = ts.make_sweep(qc, rows, **HANDLE)
    try:
        seen = []
        for S in GROWTH64:
            c = expand(rows, S)
            seen.append(assert_launch(sw, name, S, table=TABLE, rule=rule64, kernel="mfma64-sweep")["n_chunks"])
            fids, gs = te.check_grad(sw, rows, c, f"64/every/{name} grown to S = {S}")
            fresh = ts.make_sweep(qc, rows, **HANDLE)
            try:
                J2, fids2, grad2, gs2 = te.grad_call(fresh, fresh.pack(c["controls"], c["dts"]), c)
            finally:
                fresh.close()
            np.testing.assert_array_equal(fids, fids2)
            np.testing.assert_array_equal(gs, gs2)
        assert seen == [5, 1, 2]
    finally:
        sw.close()
