"""Open-system sweep gradients (the stored-state walks of qc_sweep_open_grad.hip and qc_sweep32_open_grad.hip: `qc_sweep_grad*`,
`qc_sweep_grad_params*`, `qc_sweep_vjp*` on handles made with `stored_states=True`, wide ones with `wide_stored=True`) at mid-size and
filled launches, EVERY sample against the CPU reference: the method of tests/test_sweep_every_sample.py (read its header; R = 8 rows,
sample s carries row cls[s], references once for the R rows, checks 1 to 4).  tests/test_sweep_open_grad.py and
tests/test_sweep_wide_open_grad.py check the arithmetic at S <= 6 and five samples of one S = 2049 launch; what is checked here is the
mapping the stored-state path adds to the closed walk's:
  * two launches (store, walk) that must agree on item = kWaves blockIdx + wave, s = item / n_chunks, c = item - s n_chunks; on wide handles
    with parameters the store kernel runs four waves a workgroup and the walk two, so one item sits in different workgroups;
  * h->dXall, S x (T-1) x ns, written by (s n_int + t) ns and read back through a transposed index pattern by a pointer walking down;
  * the chunk-start state at xs + (item - 1) ns, also for items whose workgroup straddles two samples;
  * a last chunk of ONE interval (the store kernel writes one knot and leaves; the walk starts with t1 - 1 == t0);
  * waves of one workgroup running different squaring counts (theta rows -2 .. 2, timesteps 0.05 .. 1.2: the "spread" rows);
  * dXall reused across calls: one handle called twice at the same size with different controls, so a knot that is not rewritten is read
    from the other call; a pullback that asks for `finals` only (dXall is not grown) ahead of the first gradient.

Tolerances, none new: per-sample outputs |got - want| <= 1e-9 max(1, max |want of that sample|) (`too.RTOL`, the rule of both open test
files); `fids` and `finals` bit-equal to `qc_sweep_eval` on the same handle; `fids`, `J` and the dense `grad` by `tes.assert_fidelities`
and `tes.assert_dense` with `ts.FID_ATOL`, `tg.GRAD_RTOL`, `tv.VJP_RTOL`.
CPU: the launch table against the restated rule and `qc_sweep_desc_launch`, the squaring spread, the soundness of sharing references on
the open routes, the reference's self-check on the spread rows.  Measured worst ratios, the squaring ranges per case and the mapping
each case is there for: profiles/sweep_open_every_sample_summary.txt."""
import ctypes as C

import numpy as np
import pytest

import sweep_open_reference as oref
import sweep_vjp_reference as vref
import test_sweep as ts
import test_sweep_every_sample as tes
import test_sweep_grad as tg
import test_sweep_open_grad as too
import test_sweep_param_grad as tp
import test_sweep_vjp as tv
import test_sweep_wide as tw
import test_sweep_wide_open_grad as two

R = tes.R
SPREAD_DT = (0.05, 1.2)          # free timesteps of the spread rows
GROWTH = tes.GROWTH              # (301, 2049, 97) on one handle at T = 24: 5 chunks, 1 chunk, 5 chunks
U0125 = ("unitary", [0, 1, 2, 5], "abs")


def _spread(c):
    """theta rows -2 .. 2 in every perturbation column (the scale rows stay in 0.9 .. 1.1): the rows' squaring counts differ."""
    c["theta"] = np.ascontiguousarray(np.repeat(np.linspace(-2.0, 2.0, R)[:, None], c["p"], axis=1))
    return c


# the R rows of a system as a case of S = R samples; the name seeds the draws (the suffix -1: a seed whose draws meet
# test_spread_rows_make_waves_diverge)
SYSTEMS = {
    "lindblad-spread": lambda qc, T: _spread(too.lindblad_case(qc, "open-every/lindblad-spread", R, T, dt=SPREAD_DT)),
    "lindblad": lambda qc, T: too.lindblad_case(qc, "open-every/lindblad", R, T),
    "nonherm8-m6": lambda qc, T: too.nonherm_case(qc, "open-every/nonherm8-m6", 8, 6, 1, R, T, False, U0125, use_scale=False),
    "qutrit-ket": lambda qc, T: too.nonherm_case(qc, "open-every/qutrit-ket", 3, 1, 1, R, T, True, ("ket", None, "abs")),
    "kets3-levels5": lambda qc, T: too.nonherm_case(qc, "open-every/kets3-levels5", 5, 2, 1, R, T, True, None, use_scale=False, cols=3),
    "wide-qutrit-spread": lambda qc, T: _spread(two.qutrit_case(qc, "open-every/wide-qutrit-spread-1", R, T, dt=SPREAD_DT)),
    "wide-nonherm12-m3": lambda qc, T: too.nonherm_case(qc, "open-every/wide-nonherm12-m3", 12, 3, 1, R, T, False, ("unitary", two.SUB12, "abs")),
    "wide-two-qubit-spread": lambda qc, T: _spread(two.two_qubit_case(qc, "open-every/wide-two-qubit-spread-1", R, T, dt=SPREAD_DT)),
    "wide-kets3-levels10": lambda qc, T: too.nonherm_case(qc, "open-every/wide-kets3-levels10", 10, 2, 1, R, T, True, None, cols=3),
}
# name: (system, N of the descriptor, m, S, T, (chunk, n_chunks, last chunk), the `wide` values served: 0 = "mfma16-sweep")
CASES = {
    "open-sqrt-301": ("lindblad-spread", 4, 2, 301, 24, (5, 5, 3), (0,)),                # odd n_chunks: workgroups straddle samples, diverging sq
    "open-byS-683": ("nonherm8-m6", 8, 6, 683, 14, (5, 3, 3), (0,)),                     # M = 6, the tight-register flavour, 8 state columns
    "open-two-2047": ("qutrit-ket", 3, 1, 2047, 8, (4, 2, 3), (0,)),                     # just under the fill threshold, ns = 6
    "open-one-2049": ("qutrit-ket", 3, 1, 2049, 8, (7, 1, 7), (0,)),                     # one chunk, odd S
    "open-sqrt-97": ("lindblad", 4, 2, 97, 102, (10, 11, 1), (0,)),                      # a last chunk of ONE interval
    "open-kets3-301": ("kets3-levels5", 5, 2, 301, 24, (5, 5, 3), (0,)),                 # pullback only: nc = 3, ns = 30, grad_init
    "wide-open-sqrt-301": ("wide-qutrit-spread", 9, 2, 301, 24, (5, 5, 3), (9, 11)),     # 11: store in 4-wave groups, walk in 2-wave groups
    "wide-open-byS-683": ("wide-nonherm12-m3", 12, 3, 683, 12, (4, 3, 3), (9,)),         # 12 state columns, ns = 288
    "wide-open-one-2049": ("wide-two-qubit-spread", 16, 2, 2049, 4, (3, 1, 3), (11,)),   # filled; the last 2-wave workgroup holds one wave
    "wide-open-kets3-301": ("wide-kets3-levels10", 10, 2, 301, 12, (3, 4, 2), (11,)),    # pullback with parameter cotangents, even item count
}
ITEMS_MOD_4 = {"open-sqrt-301": 1, "open-byS-683": 1, "open-two-2047": 2, "open-one-2049": 1, "open-sqrt-97": 3, "open-kets3-301": 1}
SPREAD = ("open-sqrt-301", "wide-open-sqrt-301", "wide-open-one-2049")
NO_FIDELITY = ("open-kets3-301", "wide-open-kets3-301")
GPU_CASES = [(name, wide) for name in CASES for wide in CASES[name][6]]
_ROWS, _REF = {}, {}     # built once, shared, never written to
WORST = {}               # what -> worst error as a share of the 1e-9 rule's bound, this session


def rows_of(qc, name, T=None):
    """The R rows of a case's system (what the references are computed for), with one unit cotangent per row."""
    system, T = CASES[name][0], CASES[name][4] if T is None else T
    if (system, T) not in _ROWS:
        rows = SYSTEMS[system](qc, T)
        rows["name"] = f"{rows['name']}/T{T}"
        rows["cot"] = tv.unit_cotangents(np.random.default_rng(7 + sum(map(ord, rows["name"]))), R, rows["init"].size)
        _ROWS[(system, T)] = rows
    return _ROWS[(system, T)]


def second_draw(rows):
    """The same system, rows and cotangents under other controls and timesteps."""
    name = rows["name"] + "/draw2"
    if name not in _ROWS:
        rng = np.random.default_rng(sum(map(ord, name)))
        assert np.ndim(rows["dts"]) == 1
        r2 = dict(rows, name=name, controls=rng.uniform(-1, 1, rows["controls"].shape), dts=rng.uniform(*SPREAD_DT, rows["T"]))
        _ROWS[name] = r2
    return _ROWS[name]


def ref_grad(rows):
    """oref.grad_forward on the R rows: grad_samples, grad_theta, grad_scale of the case's fidelity."""
    key = ("grad", rows["name"])
    if key not in _REF:
        _REF[key] = tes._frozen(oref.grad_forward(rows))
    return _REF[key]


def ref_vjp(rows):
    """vref.pullback_forward on the R rows with the rows' cotangents."""
    key = ("vjp", rows["name"])
    if key not in _REF:
        _REF[key] = tes._frozen(vref.pullback_forward(*oref._args(rows), rows["samples"], rows["cot"]))
    return _REF[key]


def interval_squarings(c):
    """R x (T-1) squaring counts, `too.squarings` (the kernels' rule restated) on every interval of every row by itself."""
    free = np.ndim(c["dts"]) != 0
    out = np.zeros((R, c["T"] - 1), dtype=int)
    for r in range(R):
        for t in range(c["T"] - 1):
            lo, hi = too.squarings(dict(c, T=2, samples=[r], controls=c["controls"][:, t:t + 2], dts=c["dts"][t:t + 2] if free else c["dts"]))
            assert lo == hi
            out[r, t] = lo
    return out


def rule(got, want, what):
    """Check 1 of every per-sample output: `too._worst`, |got - want| <= 1e-9 max(1, max |want of the sample|)."""
    assert got.shape == want.shape and not np.isnan(got).any(), what
    WORST[what] = too._worst(got, want, what)


def case_line(what, extra=""):
    mine = {k: v for k, v in WORST.items() if k.startswith(what + " ")}
    k = max(mine, key=mine.get)
    print(f"SWEEP-EVERY {what}: worst error / bound = {mine[k]:.3e} ({k[len(what) + 1:]}; {len(mine)} outputs, every sample){extra}")


def launch_of(name, S=None, T=None):
    _, N, m, S0, T0, _, wides = CASES[name]
    return tw.wide_launch(2 * N, m, S0 if S is None else S, T0 if T is None else T, wide=bool(wides[0]))


# ---------------------------------------------------------------------------------------------------------------------------------
#  CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_launch_table(qc):
    """The shapes sit on the edges they are named for, by the restated rule and by `qc_sweep_desc_launch` (which sees neither
    reserved1[0] nor the bits 1 and 3 of `wide`)."""
    L = qc._lib
    for name, (system, N, m, S, T, (chunk, n_chunks, last), wides) in CASES.items():
        rows = rows_of(qc, name)
        assert (rows["N"], rows["m"], rows["T"], rows["S"]) == (N, m, T, R), name
        want = launch_of(name)
        assert (want["mfma"], want["chunk"], want["n_chunks"], want["last"]) == (True, chunk, n_chunks, last), name
        assert (n_chunks - 1) * chunk + last == T - 1
        assert (2 * N > 16) == (wides[0] != 0), name
        if name in ITEMS_MOD_4:
            assert (S * n_chunks) % 4 == ITEMS_MOD_4[name], name
        for flag in (0, 1):
            for wide in ((0, 1) if not wides[0] else (0, 1, 9, 11)):
                D = too._ODesc(qc, flag=flag, wide=wide, N=N, m=m, T=T, cols=1)
                mf, ch, nch = C.c_int32(), C.c_int64(), C.c_int64()
                assert L.lib.qc_sweep_desc_launch(C.byref(D.d), S, C.byref(mf), C.byref(ch), C.byref(nch)) == L.QC_OK
                if wides[0] and not wide:
                    assert (bool(mf.value), ch.value, nch.value) == (False, T - 1, 0), name
                else:
                    assert (bool(mf.value), ch.value, nch.value) == (True, chunk, n_chunks), name
    f = {k: launch_of(k) for k in CASES}
    assert all(f[k]["n_chunks"] % 2 == 1 for k in ("open-sqrt-301", "open-sqrt-97", "wide-open-sqrt-301", "open-byS-683"))      # straddling
    assert f["open-sqrt-97"]["last"] == 1 and f["open-sqrt-97"]["chunk"] > 1                          # the store kernel's early `break`
    assert -(-ts.SWEEP_FILL // 683) == 3 == f["open-byS-683"]["n_chunks"] == f["wide-open-byS-683"]["n_chunks"]      # set by S, not by sqrt
    assert f["open-two-2047"]["n_chunks"] == 2 and f["open-one-2049"]["n_chunks"] == 1 and 2047 < ts.SWEEP_FILL < 2049
    # wide = 11: the store kernel takes items four a workgroup, the walk two; an odd count leaves the last walk workgroup one wave
    assert 301 * f["wide-open-sqrt-301"]["n_chunks"] == 1505 and 2049 * f["wide-open-one-2049"]["n_chunks"] % 2 == 1
    assert 301 * f["wide-open-kets3-301"]["n_chunks"] % 2 == 0 and 301 * f["wide-open-kets3-301"]["n_chunks"] % 4 == 0
    # the growth sequence on one handle at T = 24, narrow and wide
    for name in ("open-sqrt-301", "wide-open-sqrt-301"):
        assert [launch_of(name, S, 24)["n_chunks"] for S in GROWTH] == [5, 1, 5]
    assert GROWTH[1] * 1 > GROWTH[2] * 5 and GROWTH[0] * 5 > GROWTH[2] * 5 and GROWTH[1] * 23 > GROWTH[0] * 23      # dXs and dXall grow, then are reused


@pytest.mark.parametrize("name", SPREAD)
def test_spread_rows_make_waves_diverge(qc, name):
    """Over the R rows both the per-row minimum and the per-row maximum of the squaring counts take at least two values; the intervals of
    one chunk of one row see at least three counts; and in the launch most workgroups hold waves whose count sequences differ."""
    rows = rows_of(qc, name)
    S, T = CASES[name][3], CASES[name][4]
    sq = interval_squarings(rows)
    lo, hi = sq.min(axis=1), sq.max(axis=1)
    for r in range(R):
        assert (lo[r], hi[r]) == too.squarings(dict(rows, samples=[r]))
    print(f"SWEEP-EVERY open/{name}: squarings per row (min, max) from {(int(lo.min()), int(hi.min()))} to {(int(lo.max()), int(hi.max()))}")
    assert len(set(lo.tolist())) >= 2 and len(set(hi.tolist())) >= 2
    want = launch_of(name)
    chunk, n_chunks = want["chunk"], want["n_chunks"]
    spans = [(t0, min(T - 1, t0 + chunk)) for t0 in range(0, T - 1, chunk)]
    assert len(spans) == n_chunks
    assert max(len(set(sq[r, a:b].tolist())) for r in range(R) for a, b in spans) >= 3
    # the walk's workgroups: the counts of their waves, step by step from the chunk's end.  4 restates kWaves (qc_sweep_common.h, both
    # forms); 2 restates kOW<true> of qc_sweep32_open_grad.hip, the parameter flavour of the wide walk (wide = 11)
    cls = tes.classes(S)
    for waves in ((2, 4) if 11 in CASES[name][6] else (4,)):
        seq = [tuple(sq[cls[item // n_chunks], spans[item % n_chunks][0]:spans[item % n_chunks][1]][::-1]) for item in range(S * n_chunks)]
        groups = [seq[i:i + waves] for i in range(0, len(seq), waves)]
        differ = sum(len(set(g)) > 1 for g in groups)
        assert 2 * differ > len(groups), (name, waves, differ, len(groups))


@pytest.mark.parametrize("which", ["density", "nonherm-unitary"])
def test_reference_reuse_is_sound(qc, which):
    """Two samples with equal rows have equal references, bit for bit, on the routes the open cases take; distinct rows differ; the rows'
    references are their own."""
    if which == "density":
        rows = _spread(too.lindblad_case(None, "open-every/reuse-density", R, 5, dt=SPREAD_DT))
    else:
        rows = too.nonherm_case(None, "open-every/reuse-nonherm", 3, 2, 1, R, 5, True, ("unitary", [0, 1], "abs2"))
    rows["cot"] = tv.unit_cotangents(np.random.default_rng(3), R, rows["init"].size)
    c = tes.expand(rows, 2 * R + 3)
    S, cls = c["S"], c["cls"]
    pairs = [(r, S - 1 - r) for r in (0, 3, R - 1)]
    assert all(cls[a] == cls[b] for a, b in pairs)
    c["samples"] = [s for pair in pairs for s in pair]
    g = oref.grad_forward(c)
    pb = vref.pullback_forward(*oref._args(c), c["samples"], c["cot"])
    for what, a in dict(**g, **{"vjp " + k: v for k, v in pb.items()}).items():
        assert a.shape[0] == 6 and np.abs(a).max() > 1e-3, what
        np.testing.assert_array_equal(a[0::2].view(np.uint64), a[1::2].view(np.uint64), err_msg=what)
        assert not np.array_equal(a[0], a[2]), what
    own = oref.grad_forward(rows)
    for k in g:
        np.testing.assert_array_equal(g[k][0::2], own[k][[0, 3, R - 1]], err_msg=k)


@pytest.mark.parametrize("name", SPREAD)
def test_reference_routes_agree_on_the_spread_rows(qc, name):
    """Forward mode (expm_frechet) against central differences at theta = -2 and 2 and timesteps up to 1.2, outside what the open test
    files' own self-checks cover: the project's 1e-6."""
    rows = rows_of(qc, name)
    err, big = oref.forward_vs_fd(rows, [0, R - 1])
    print(f"SWEEP-EVERY open/{name}: forward vs central differences {err:.2e}, max |grad| {big:.3e}")
    assert err < 1e-6 and big > 1e-6


# ---------------------------------------------------------------------------------------------------------------------------------
#  GPU
# ---------------------------------------------------------------------------------------------------------------------------------
def make(qc, rows, wide):
    fid = rows["kind"] is not None
    if not wide:
        sw = too._handle(qc, rows, fid=fid)
        assert sw.kernel_name == "mfma16-sweep" and sw.stored_states
    else:
        sw = two._handle(qc, rows, params=wide == 11, fid=fid)
        assert sw.kernel_name == "mfma32-sweep" and sw.stored_states and sw.wide_stored and sw.wide_params == (wide == 11)
        assert sw._desc.wide == wide
    assert sw.vjp_supported and sw.grad_supported == fid
    return sw


def assert_launch(sw, name, S=None, T=None):
    want = launch_of(name, S, T)
    assert sw.launch(CASES[name][3] if S is None else S) == (True, want["chunk"], want["n_chunks"])
    return want


def grad_outputs(qc, sw, c, params):
    """The bare calls: `grad_device` with every output and, on handles that serve it, `qc_sweep_grad_params` with every output; every
    buffer prefilled with -7."""
    Z = too._Z(sw, c)
    J, fids, grad, gs = tes.grad_call(sw, Z, c)
    out = dict(J=np.array([J]), fids=fids, grad=grad, gs=gs)
    if params:
        o = tp._raw(qc, sw, Z, c["init"], c["theta"], c["scale"], c["weights"])
        out.update({"par " + k: (np.array([v]) if k == "J" else v) for k, v in o.items()})
    return out


def check_grad(qc, sw, rows, c, what, params):
    """Checks 1 to 4 on the outputs of `grad_outputs`, then the host entries bit-equal."""
    Z, cls, want = too._Z(sw, c), c["cls"], ref_grad(rows)
    out = grad_outputs(qc, sw, c, params)
    f_eval = sw.eval(Z, c["init"], c["theta"], c["scale"], finals=False)[1]
    flavours = [("", "gs", "fids", "J", "grad")] + ([("par ", "par gs", "par fids", "par J", "par grad")] if params else [])
    for pre, gs, fids, J, grad in flavours:
        tes.every_sample(rule, out[gs], want["grad_samples"][cls], cls, f"{what} {pre}grad_samples")
        tes.assert_class_bits(out[gs], cls, f"{what} {pre}grad_samples")
        np.testing.assert_array_equal(out[fids], f_eval, err_msg=f"{what} {pre}fids: the bits of qc_sweep_eval")
        tes.assert_fidelities(out[fids], out[J][0], rows, c, f"{what} {pre}".strip())
        tes.assert_dense(out[grad], want["grad_samples"], cls, c["weights"], sw, tg.GRAD_RTOL, f"{what} {pre}".strip())
    host = sw.grad(Z, c["init"], c["theta"], c["scale"], weights=c["weights"], per_sample=True)
    for a, k in zip(host, ("J", "fids", "grad", "gs")):
        np.testing.assert_array_equal(np.asarray(a).reshape(out[k].shape), out[k], err_msg=f"{what} host {k}")
    if params:
        for k, r in (("par gth", "grad_theta"), ("par gsc", "grad_scale")):
            tes.every_sample(rule, out[k], want[r][cls], cls, f"{what} {r}")
            tes.assert_class_bits(out[k], cls, f"{what} {r}")
        for k in ("gs", "grad", "fids", "J"):      # the per-interval values do not depend on the flavour
            np.testing.assert_array_equal(out["par " + k], out[k], err_msg=f"{what} parameter flavour {k}")
        fids, gth, gsc = sw.param_grad(Z, c["init"], c["theta"], c["scale"])
        for a, k in ((fids, "fids"), (gth, "par gth"), (gsc, "par gsc")):
            np.testing.assert_array_equal(a, out[k], err_msg=f"{what} param_grad {k}")
    return out


def vjp_outputs(sw, c, params):
    want = [k for k in tv.OUTPUTS if params or k not in ("grad_theta", "grad_scale")]
    return tv.device_call(sw, too._Z(sw, c), c, want)


def check_vjp(sw, rows, c, what, params):
    """One `vjp_device` call with every output the form serves (buffers prefilled with -7): checks 1 to 4, `finals` bit-equal to
    `qc_sweep_eval`."""
    cls, S = c["cls"], c["S"]
    out = vjp_outputs(sw, c, params)
    r = ref_vjp(rows)
    assert set(out) - {"finals", "grad"} <= set(r)      # every per-sample output has its reference: none is skipped below
    for k in out:
        if k in r:
            tes.every_sample(rule, out[k], r[k][cls], cls, f"{what} pullback {k}")
        if k != "grad":
            tes.assert_class_bits(out[k], cls, f"{what} pullback {k}")
    fin = sw.eval(too._Z(sw, c), c["init"], c["theta"], c["scale"], fids=False)[0]
    np.testing.assert_array_equal(out["finals"].T, fin, err_msg=f"{what} finals: the bits of qc_sweep_eval")
    tes.every_sample(rule, out["finals"], tes.ref_finals(rows)[0].T[cls], cls, f"{what} pullback finals")
    tes.assert_dense(out["grad"], r["grad_samples"], cls, np.ones(S), sw, tv.VJP_RTOL, what + " pullback")
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,wide", GPU_CASES, ids=[f"{n}-wide{w}" if w else n for n, w in GPU_CASES])
def test_open_every_sample(qc, name, wide):
    rows = rows_of(qc, name)
    c = tes.expand(rows, CASES[name][3])
    what = f"open/{name}" + (f" wide {wide}" if wide else "")
    params = wide in (0, 11)
    sw = make(qc, rows, wide)
    try:
        assert_launch(sw, name)
        if name not in NO_FIDELITY:
            check_grad(qc, sw, rows, c, what, params)
        check_vjp(sw, rows, c, what, params)
    finally:
        sw.close()
    case_line(what, f"; squarings of the rows {too.squarings(rows)}")


@pytest.mark.gpu
@pytest.mark.parametrize("name,wide", [("open-sqrt-301", 0), ("wide-open-sqrt-301", 11)], ids=["narrow", "wide11"])
def test_open_scratch_growth_and_stale_states(qc, name, wide):
    """One handle at T = 24 through S = 301, 2049 and 97 (5 chunks, 1, 5: dXs, dLs, dXall and dPart grow and are reused at a smaller
    stride), the last under a second draw of controls and timesteps, then at S = 97 once more under the first draw: dXall holds the other
    draw's states at the same offsets, so a knot the store kernel does not rewrite fails check 1 there.  Before anything else the handle
    serves a pullback that asks for `finals` only, which grows no dXall.  At every visit the outputs pass checks 1 to 4 and carry the
    bits of a fresh handle's, which never made the first call."""
    rows = rows_of(qc, name, T=24)
    draws = (rows, rows, second_draw(rows), rows)
    sw = make(qc, rows, wide)
    try:
        c = tes.expand(rows, GROWTH[0])
        first = tv.device_call(sw, too._Z(sw, c), c, ["finals"])["finals"]
        np.testing.assert_array_equal(first.T, sw.eval(too._Z(sw, c), c["init"], c["theta"], c["scale"], fids=False)[0])
        seen = []
        for visit, (S, r) in enumerate(zip(GROWTH + GROWTH[-1:], draws)):
            c = tes.expand(r, S)
            n_chunks = assert_launch(sw, name, S, 24)["n_chunks"]
            if visit < len(GROWTH):
                seen.append(n_chunks)
            what = f"open/growth/{name} visit {visit} S = {S}" + (" second draw" if r is not rows else "")
            g = check_grad(qc, sw, r, c, what, True)
            v = check_vjp(sw, r, c, what, True)
            fresh = make(qc, rows, wide)
            try:
                g2, v2 = grad_outputs(qc, fresh, c, True), vjp_outputs(fresh, c, True)
            finally:
                fresh.close()
            for k in g:
                np.testing.assert_array_equal(g[k], g2[k], err_msg=f"{what}: {k} against a fresh handle")
            for k in v:
                np.testing.assert_array_equal(v[k], v2[k], err_msg=f"{what}: pullback {k} against a fresh handle")
            case_line(what)
        assert seen == [5, 1, 5]
        assert not np.array_equal(ref_grad(rows)["grad_samples"], ref_grad(draws[2])["grad_samples"])
    finally:
        sw.close()
