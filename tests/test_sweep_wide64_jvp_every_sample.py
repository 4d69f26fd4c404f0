"""Sweep pushforwards in the "mfma64-sweep" form (`qc_sweep64_jvp_kernel` of csrc/qc_sweep64_jvp.hip and `qc_sweep64_jvp_finish_kernel`,
the ld = 64 instantiation of `jvp_finish`: `RolloutSweep(..., wide=True, wide64=True, wide64_tangent=True)`, `wide` = 17409) at launches
of 250 .. 510 workgroups, EVERY sample against the CPU reference: the method of tests/test_sweep_wide64_every_sample.py and
tests/test_sweep_jvp_every_sample.py (read their headers: R = 8 distinct classes of (theta, scale, vtheta, vscale), sample s carries row
`classes(S)[s]`, the Frechet reference once for the R rows, every buffer prefilled with -7), their helpers imported.
tests/test_sweep_wide64_jvp.py checks the arithmetic at up to 22 workgroups and three samples of one S = 256 launch; what is checked here is
what the kernel has of its own at full launches:
  * the work item is a whole workgroup, item = blockIdx.x, s = item / n_chunks: five sqrt-capped chunks at S = 50 (250 workgroups), the
    chunk count set by S at S = 100 (chunks of 9, 9, 8: 300 workgroups), both sides of the fill constant (S = 255 with a fixed timestep:
    510 workgroups; S = 257: one chunk);
  * the two totals of an item at tot + item * 8192 (W, then Wdot) stored from registers, and the finish kernel's read at
    tot + s * n_chunks * 8192;
  * the scratch `dTotJ`: 250 slots of 8192 doubles, grown to 300, then to 510 at another stride, with `eval` and `vjp` (whose totals live
    in `dTot`, 4096 doubles an item) in between.
All cases are 17 levels (n = 34: a third tile row that is almost empty) with two ket columns; a two-column state has no fidelity, so one
further case with a single ket and the ket fidelity (S = 100) checks `fids` and `tfids` in the same way.
  1. finals[s], tfinals[s] (fids[s], tfids[s]) of every sample against the reference of its class (`check_values` of
     tests/test_sweep_jvp_every_sample.py: JVP_RTOL for tangents, the state and fidelity tolerances of tests/test_sweep.py);
  2. every row of every output carries the bits of the first sample of its class;
  3. `eval` and the host entry point return the device call's bits (`check_jvp`).
No tolerance is new.

Why a wrong mapping fails.  Neighbouring samples belong to different classes in 7 of 8 places, any two classes' final states lie >= 1e-3
apart and any two classes' tangents >= 1e-3 of the tangents' scale (the floor tests: 10^6 times the bound), so a total written or read at
another item's slot fails 1 with the samples named; so does a slot that holds an earlier launch's total (stale), a slot nobody wrote, W and
Wdot exchanged in a slot, a Wdot that is missing.  CPU: the launch table, the class map at S = 50 and 100, the floors, and that the checks
fail on arrays made from the reference with each of these defects (the last two through a restatement of the finish kernel's chain over
chunk totals made with scipy)."""
import ctypes as C
import itertools
import time

import numpy as np
import pytest
import scipy.linalg as sla

import sweep_reference as ref
import test_sweep as ts
import test_sweep_every_sample as te
import test_sweep_jvp as tj
import test_sweep_jvp_every_sample as tje
import test_sweep_vjp as tv
import test_sweep_wide as tw
import test_sweep_wide64 as t64
from test_sweep_every_sample import R, assert_launch, classes
from test_sweep_jvp_every_sample import check_adjoint, check_jvp, check_values, jvp_call, launch_of, reference

W64, GRAD64, PARAMS64, TAN64 = 1024, 2048, 8192, 16384
KET = ("ket", None, "abs")
TANGENT = dict(wide=True, wide64=True, wide64_tangent=True)                                   # wide = 17409
PULLBACK = dict(TANGENT, wide64_grad=True, wide64_params=True)                                # wide = 27649
COLS = 2
# name: ((state, levels, m, p, scale given, free timestep, S, T, fidelity), wide, (chunk, n_chunks, last chunk), chunk count capped by sqrt(T - 1))
TABLE = {
    "w64j-five-50": (("kets3", 17, 2, 1, True, True, 50, 26, None), W64, (5, 5, 5), True),           # five chunks of five, 250 workgroups
    "w64j-byS-100": (("kets3", 17, 2, 1, False, True, 100, 27, None), W64, (9, 3, 8), False),        # chunks of 9, 9, 8; scale = None with vscale given
    "w64j-two-255": (("kets3", 17, 2, 1, True, False, 255, 26, None), W64, (13, 2, 12), False),      # just below the fill constant; fixed timestep
    "w64j-one-257": (("kets3", 17, 2, 1, True, True, 257, 6, None), W64, (5, 1, 5), False),          # just above it: one chunk
    "w64j-ket-100": (("ket", 17, 2, 1, True, True, 100, 27, KET), W64, (9, 3, 8), False),            # one ket with its fidelity: fids and tfids
}
ITEMS = {"w64j-five-50": 250, "w64j-byS-100": 300, "w64j-two-255": 510, "w64j-one-257": 257, "w64j-ket-100": 300}
GROWTH64 = (50, 300, 255)          # on one "w64j-five-50" handle at T = 26: 5 chunks, 1, 2 -- 250, 300, 510 slots of 8192 doubles
NEW_S = (50, 100)                  # the S whose class map no other file checks


def rule64(spec, S):
    return t64.launch64(2 * spec[1], spec[2], S, spec[7], 1 | W64 | TAN64)


def build_rows(qc, name):
    """The R rows of test_sweep_jvp_every_sample.build_rows; the two-column cases get a state of two kets (and cotangents and a `vinit` of
    its size) in place of the three of the "kets3" tuple."""
    rows = tje.build_rows(qc, name, TABLE)
    if TABLE[name][0][0] == "kets3":
        rng = np.random.default_rng(29 + sum(map(ord, name)))
        K = rng.standard_normal((17, COLS)) + 1j * rng.standard_normal((17, COLS))
        K /= np.linalg.norm(K, axis=0)
        rows["init"], rows["cols"] = ref.operator_to_iso_vec(K), COLS
        ns = rows["init"].size
        rows["cot"] = tv.unit_cotangents(rng, R, ns)
        rows["vinit"] = rng.standard_normal(ns) / np.sqrt(ns)
    return rows


def timed_reference(rows):
    """`reference(rows)` (computed once, shared, frozen), with the CPU time of its first build on the record."""
    t0 = time.process_time()
    fresh = rows["name"] not in tje._REF
    r = reference(rows)
    te.ref_finals(rows)
    if fresh:
        print(f"SWEEP-WIDE64-JVP-EVERY reference {rows['name']}: Frechet route over {R} rows built in {time.process_time() - t0:.2f} s of CPU time")
    return r


def reference_arrays(rows, c):
    """What a faultless launch returns, made from the reference: every output of the handle, sample s the row of its class."""
    cls, r = c["cls"], timed_reference(rows)
    out = dict(finals=np.ascontiguousarray(r["finals"][cls]), tfinals=np.ascontiguousarray(r["tfinals"][cls]))
    if rows["kind"] is not None:
        out.update(fids=np.ascontiguousarray(te.ref_finals(rows)[1][cls]), tfids=np.ascontiguousarray(r["tfids"][cls]))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
#  CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_wide64_jvp_launch_table(qc):
    L = qc._lib
    assert L.QC_SWEEP_WIDE | L.QC_SWEEP_WIDE_64 | L.QC_SWEEP_WIDE_64_TANGENT == 17409 and t64.FILL64 == 256
    assert set(ITEMS) == set(TABLE)
    for name, (spec, wide, (chunk, n_chunks, last), by_sqrt) in TABLE.items():
        _, levels, m, _, _, _, S, T, _ = spec
        assert wide == W64 and levels == 17, name
        assert rule64(spec, S) == dict(mfma=True, chunk=chunk, n_chunks=n_chunks, last=last, by_sqrt=by_sqrt), name
        assert (n_chunks - 1) * chunk + last == T - 1 and S * n_chunks == ITEMS[name]
        for bits in (17409, 27649):
            D = tw._wdesc(qc, bits, N=levels, m=m, T=T, cols=COLS)
            mf, ch, nch = C.c_int32(), C.c_int64(), C.c_int64()
            assert L.lib.qc_sweep_desc_launch(C.byref(D.d), S, C.byref(mf), C.byref(ch), C.byref(nch)) == L.QC_OK
            assert (bool(mf.value), ch.value, nch.value) == (True, chunk, n_chunks), name
    f = {k: TABLE[k][2] for k in TABLE}
    assert f["w64j-five-50"] == (5, 5, 5) and TABLE["w64j-five-50"][3] and -(-256 // 50) == 6 > 5          # sqrt-capped: ceil(sqrt(25)) = 5
    assert f["w64j-byS-100"] == (9, 3, 8) and -(-256 // 100) == 3                                          # S sets the chunk count
    assert f["w64j-two-255"][1] == 2 and f["w64j-one-257"][1] == 1 and not TABLE["w64j-two-255"][0][5]     # both sides of the fill constant
    assert not TABLE["w64j-byS-100"][0][4]                                                                 # scale = None there
    sp = TABLE["w64j-five-50"][0]
    seq = [rule64(sp, S)["n_chunks"] for S in GROWTH64]
    assert sp[7] == 26 and seq == [5, 1, 2] and [S * n for S, n in zip(GROWTH64, seq)] == [250, 300, 510]


def test_classes_reach_both_ends_at_the_new_sizes():
    te.assert_classes_reach_both_ends(set(NEW_S) | {TABLE[k][0][6] for k in TABLE} | set(GROWTH64))


@pytest.mark.parametrize("name", list(TABLE))
def test_floors_keep_the_classes_apart(qc, name):
    """No class passes for another: any two classes' final states differ by >= 1e-3 and any two classes' tangents by >= 1e-3 of the
    tangents' scale (10^6 times the bound of check 1); no final state is the initial one and no tangent is `vinit`."""
    rows = build_rows(qc, name)
    r = timed_reference(rows)
    pairs = list(itertools.combinations(range(R), 2))
    scale = max(1.0, np.abs(r["tfinals"]).max())
    apart = min(np.abs(r["finals"][i] - r["finals"][j]).max() for i, j in pairs)
    tapart = min(np.abs(r["tfinals"][i] - r["tfinals"][j]).max() for i, j in pairs) / scale
    moved = min(np.abs(r["finals"] - rows["init"]).max(axis=1).min(), np.abs(r["tfinals"] - rows["vinit"]).max(axis=1).min())
    print(f"SWEEP-WIDE64-JVP-EVERY {name}: smallest distance between two classes, finals {apart:.3e}, tangents {tapart:.3e} of their scale "
          f"{scale:.3e}; smallest distance from init / vinit {moved:.3e}")
    assert apart >= 1e-3 and tapart >= 1e-3 and moved >= 1e-3, name
    assert tj.JVP_RTOL * scale <= 1e-6 * tapart * scale
    if rows["kind"] is not None:
        fapart = min(abs(r["tfids"][i] - r["tfids"][j]) for i, j in pairs)
        print(f"SWEEP-WIDE64-JVP-EVERY {name}: smallest distance between two classes' fidelity tangents {fapart:.3e}")
        assert fapart >= 1e-6, name


def chunk_totals(rows, n_chunks, chunk):
    """(W_c, Wdot_c) of every class and chunk by scipy: R x n_chunks x n x n each, W = E_last ... E_first over the chunk's intervals."""
    n, T, m = rows["n"], rows["T"], rows["m"]
    h = rows["dts"] if np.ndim(rows["dts"]) else np.full(T, float(rows["dts"]))
    vh = np.zeros(T) if rows["vdts"] is None else rows["vdts"]
    sc = np.ones((R, m)) if rows["scale"] is None else rows["scale"]
    W, Wd = np.zeros((R, n_chunks, n, n)), np.zeros((R, n_chunks, n, n))
    for r in range(R):
        for c in range(n_chunks):
            Q, Qd = np.eye(n), np.zeros((n, n))
            for t in range(c * chunk, min((c + 1) * chunk, T - 1)):
                a, va = rows["controls"][:, t], rows["vcontrols"][:, t]
                G = ref.sample_generator(rows["G0"], rows["Gd"], rows["Gp"], a, rows["theta"][r], sc[r])
                D = sum(rows["vtheta"][r][j] * P for j, P in enumerate(rows["Gp"])) + sum((rows["vscale"][r][k] * a[k] + sc[r][k] * va[k]) * Gk
                                                                                         for k, Gk in enumerate(rows["Gd"]))
                E, Ed = sla.expm_frechet(h[t] * G, vh[t] * G + h[t] * D)
                Q, Qd = E @ Q, E @ Qd + Ed @ Q
            W[r, c], Wd[r, c] = Q, Qd
    return W, Wd


def finish_chain(rows, W, Wd):
    """The finish kernel's chain restated: x <- init, xdot <- vinit; per chunk xdot <- W xdot + Wdot x, then x <- W x."""
    n = rows["n"]
    fin, tfin = [], []
    for r in range(R):
        x, xd = rows["init"].reshape(n, -1, order="F"), rows["vinit"].reshape(n, -1, order="F")
        for c in range(W.shape[1]):
            x, xd = W[r, c] @ x, W[r, c] @ xd + Wd[r, c] @ x
        fin.append(x.reshape(-1, order="F"))
        tfin.append(xd.reshape(-1, order="F"))
    return np.array(fin), np.array(tfin)


def test_the_checks_see_each_defect(qc):
    """Checks 1 and 2 on arrays made here from the reference at S = 100 (chunks of 9, 9, 8): they pass on the faultless arrays, and fail
    when every sample holds its neighbour's value (a slot one item off), when one sample holds the value an S = 300 launch left in its slot
    (stale), when one sample keeps the prefill, when one sample differs from its class in the last bit, when W and Wdot are exchanged in
    one chunk's slot, and when one chunk's Wdot is left out."""
    name = "w64j-byS-100"
    rows = build_rows(qc, name)
    c = launch_of(rows, TABLE[name][0][6])
    good = reference_arrays(rows, c)
    check_values(good, rows, c, "made up")
    cls = c["cls"]

    def fails(bad, what, match=None):
        with pytest.raises(AssertionError, match=match):
            check_values(bad, rows, c, what)

    shifted = {k: np.roll(v, 1, axis=0) for k, v in good.items()}
    fails(shifted, "shifted", "largest errors at")
    r = timed_reference(rows)
    other = classes(300)[:c["S"]]
    s = int(np.flatnonzero(other != cls)[R])                     # a sample that another launch gave another class
    for key in ("tfinals", "finals"):
        stale, unwritten, last_bit = (dict(good, **{key: good[key].copy()}) for _ in range(3))
        stale[key][s] = r[key][other[s]]
        unwritten[key][s] = -7.0
        last_bit[key][s, 3] = np.nextafter(last_bit[key][s, 3], 2.0)
        for what, bad in (("stale", stale), ("unwritten", unwritten), ("last bit", last_bit)):
            fails(bad, f"{what} {key}")
    # the two totals of a slot: the restated chain reproduces the reference, and fails with either defect in one chunk
    chunk, n_chunks, _ = TABLE[name][2]
    W, Wd = chunk_totals(rows, n_chunks, chunk)
    fin, tfin = finish_chain(rows, W, Wd)
    assert np.abs(fin - r["finals"]).max() <= 1e-12 and np.abs(tfin - r["tfinals"]).max() <= 1e-12 * max(1.0, np.abs(r["tfinals"]).max())
    check_values(dict(finals=np.ascontiguousarray(fin[cls]), tfinals=np.ascontiguousarray(tfin[cls])), rows, c, "restated chain")
    for k in range(n_chunks):
        Ws, Wds = W.copy(), Wd.copy()
        Ws[:, k], Wds[:, k] = Wd[:, k], W[:, k]
        fin2, tfin2 = finish_chain(rows, Ws, Wds)
        fails(dict(finals=np.ascontiguousarray(fin2[cls]), tfinals=np.ascontiguousarray(tfin2[cls])), f"W and Wdot exchanged in chunk {k}")
        Wz = Wd.copy()
        Wz[:, k] = 0.0
        fin3, tfin3 = finish_chain(rows, W, Wz)
        np.testing.assert_array_equal(fin3, fin)
        fails(dict(finals=np.ascontiguousarray(fin3[cls]), tfinals=np.ascontiguousarray(tfin3[cls])), f"Wdot of chunk {k} left out")


# ---------------------------------------------------------------------------------------------------------------------------------
#  GPU
# ---------------------------------------------------------------------------------------------------------------------------------
def same_bits(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        np.testing.assert_array_equal(a[k].view(np.uint64), b[k].view(np.uint64), err_msg=f"{what}: {k}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TABLE))
def test_wide64_jvp_every_sample(qc, name):
    t_wall = time.perf_counter()
    rows = build_rows(qc, name)
    spec = TABLE[name][0]
    c = launch_of(rows, spec[6])
    what = f"w64-every/{name}"
    timed_reference(rows)
    sw = ts.make_sweep(qc, rows, **TANGENT)
    back = None
    try:
        want = assert_launch(sw, name, table=TABLE, rule=rule64, kernel="mfma64-sweep")
        assert sw._desc.wide == 17409 and sw.wide64_tangent and sw.jvp_supported and c["S"] * want["n_chunks"] == ITEMS[name]
        assert not sw.vjp_supported and rows["n"] == 34 and sw.cols == (1 if spec[0] == "ket" else COLS)
        if not spec[4]:
            assert c["scale"] is None and np.all(c["vscale"] != 0)              # the cl = 1, vcl != 0 path
        if not spec[5]:
            assert np.ndim(c["dts"]) == 0 and c["vdts"] is None                 # the h_n = h path
        Z, dirs, out = check_jvp(sw, rows, c, what)
        # the adjoint identity against the pullback of a handle that serves one; its pushforward carries the bits of `sw`'s
        back = ts.make_sweep(qc, rows, **PULLBACK)
        assert back._desc.wide == 27649 and back.kernel_name == "mfma64-sweep" and back.vjp_supported and back.jvp_supported
        _, _, again = jvp_call(back, c)
        same_bits(again, out, f"{what}: the wide = 27649 handle against the wide = 17409 handle")
        check_adjoint(back, c, Z, dirs, again, what)
    finally:
        sw.close()
        if back is not None:
            back.close()
    print(f"SWEEP-WIDE64-JVP-EVERY {what}: {time.perf_counter() - t_wall:.2f} s of wall time")


@pytest.mark.gpu
def test_wide64_jvp_scratch_growth_every_sample(qc):
    """One handle (`wide` = 27649) at S = 50, then 300, then 255 with T = 26: 5 chunks, 1, 2, so `dTotJ` holds 250 slots of 8192 doubles,
    grows to 300, then to 510 at another stride.  At every S, in this order: `eval`, `jvp_device`, `vjp` with the adjoint check,
    `jvp_device`, `eval`.  The two pushforwards are bit-equal, each carries the bits of a fresh handle's and passes checks 1 and 2, and
    `eval` afterwards returns the bits of `eval` before: `dTotJ` and the `dTot` of the other entry points do not touch each other."""
    t_wall = time.perf_counter()
    name = "w64j-five-50"
    rows = build_rows(qc, name)
    timed_reference(rows)
    sw = ts.make_sweep(qc, rows, **PULLBACK)
    try:
        seen = []
        for S in GROWTH64:
            c = launch_of(rows, S)
            seen.append(assert_launch(sw, name, S, table=TABLE, rule=rule64, kernel="mfma64-sweep")["n_chunks"])
            what = f"w64-every/{name} grown to S = {S}"
            Z = sw.pack(c["controls"], c["dts"])
            before = sw.eval(Z, c["init"], c["theta"], c["scale"])
            _, dirs, first = jvp_call(sw, c)
            check_adjoint(sw, c, Z, dirs, first, what)
            _, _, second = jvp_call(sw, c)
            after = sw.eval(Z, c["init"], c["theta"], c["scale"])
            fresh = ts.make_sweep(qc, rows, **TANGENT)
            try:
                _, _, third = jvp_call(fresh, c)
            finally:
                fresh.close()
            same_bits(second, first, f"{what}: the second call")
            same_bits(third, first, f"{what}: a fresh handle")
            check_values(first, rows, c, what)
            check_values(second, rows, c, what + ", second call")
            np.testing.assert_array_equal(after[0], before[0], err_msg=f"{what}: finals of eval after the pushforward")
            np.testing.assert_array_equal(first["finals"], before[0].T)
        assert seen == [5, 1, 2] and [S * n for S, n in zip(GROWTH64, seen)] == [250, 300, 510]
    finally:
        sw.close()
    print(f"SWEEP-WIDE64-JVP-EVERY w64-every/{name} growth: {time.perf_counter() - t_wall:.2f} s of wall time")
