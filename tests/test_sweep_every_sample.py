"""Sweep derivatives (`qc_sweep_grad*`, `qc_sweep_grad_params*`, `qc_sweep_vjp*`, both MFMA forms) at mid-size and filled launches, EVERY
sample against the CPU reference.  The other sweep tests check the arithmetic at S <= 11 and three samples of S = 2048; what is checked
here is the mapping from a sample to a wave, a workgroup and a scratch slot: item = 4 blockIdx + wave, s = item / n_chunks, the partly
filled last workgroup, workgroups whose waves straddle two samples, the per-sample scratch and its growth, at S = 97 .. 2049 on both
sides of the fill threshold and in the regime where ceil(2048 / S) sets the chunk count.

The method: a launch of S samples is made of R = 8 distinct parameter rows (theta, scale, cotangent), the classes; sample s carries row
cls[s], a fixed pseudo-random map with every class in the first and in the last R samples.  The forward-mode references of
tests/sweep_*_reference.py are computed once for the R rows; a sample with identical inputs has the identical reference, so
  1. every output row got[s] is compared with ref[cls[s]] by the assertion and tolerance the output has in its own test file;
  2. got[s] carries the bits of got[cls[s]], the first sample of its class: one wave per item, no atomics, reductions in a fixed order;
  3. the reduced outputs are compared with the reference, not with the kernel's own rows:
     |grad - sum_s w_s ref[cls[s]]| <= rtol sum_s |w_s| max(1, max |ref|) entrywise (the per-sample bound through the triangle inequality),
     |J - w . F_ref[cls]| <= FID_ATOL sum |w|; entries that are no control or timestep of knots 0 .. T-2 are +0.0 bit for bit;
  4. every output buffer is prefilled with -7, so an unwritten row fails 1.
No tolerance is new.  CPU: the class map, the launch table against `qc_sweep_desc_launch`, the soundness of sharing references.
Measured worst ratios: profiles/sweep_every_sample_summary.txt."""
import ctypes as C

import numpy as np
import pytest
import torch

import sweep_param_grad_reference as pref
import sweep_vjp_reference as vref
import test_sweep as ts
import test_sweep_grad as tg
import test_sweep_param_grad as tp
import test_sweep_vjp as tv
import test_sweep_wide as tw

R = 8              # distinct parameter rows of a launch

U, U01A2, KET = ("unitary", None, "abs"), ("unitary", [0, 1], "abs2"), ("ket", None, "abs")
# name: ((state, levels, m, p, scale given, free timestep, S, T, fidelity), wide, (chunk, n_chunks, last chunk), chunk count capped by sqrt(T - 1))
CASES = {
    "sqrt-301": (("unitary", 2, 2, 1, True, True, 301, 24, U), False, (5, 5, 3), True),                  # 1505 items: odd n_chunks, partial last workgroup
    "byS-683": (("unitary", 8, 6, 1, False, True, 683, 50, U), False, (17, 3, 15), False),               # 2049 items: n_chunks = ceil(2048 / S), M = 6
    "two-2047": (("unitary", 3, 1, 3, True, False, 2047, 8, U01A2), False, (4, 2, 3), False),            # 4094 items: just below the fill threshold
    "one-2049": (("ket", 4, 2, 1, True, True, 2049, 8, KET), False, (7, 1, 7), False),                   # 2049 items: just above it, one chunk, odd S
    "sqrt-97": (("unitary", 2, 2, 1, False, True, 97, 102, U), False, (10, 11, 1), True),                # 1067 items: many chunks, a last chunk of 1
    "wide-sqrt-301": (("unitary", 9, 2, 1, False, True, 301, 24, ("unitary", [0, 1, 3, 4], "abs")), True, (5, 5, 3), True),
    "wide-byS-683": (("unitary", 12, 3, 1, True, False, 683, 12, ("unitary", None, "abs2")), True, (4, 3, 3), False),
    "wide-one-2049": (("ket", 10, 2, 1, True, True, 2049, 6, KET), True, (5, 1, 5), False),
}
ITEMS_MOD_4 = {"sqrt-301": 1, "byS-683": 1, "two-2047": 2, "one-2049": 1, "sqrt-97": 3, "wide-sqrt-301": 1, "wide-byS-683": 1, "wide-one-2049": 1}
# the ket rows once more as three kets without a fidelity: the handle `grad` refuses, served by the pullback alone
KETS3 = {
    "one-2049-kets3": (("kets3", 4, 2, 1, True, True, 2049, 8, None), False, (7, 1, 7), False),
    "wide-one-2049-kets3": (("kets3", 10, 2, 1, True, True, 2049, 6, None), True, (5, 1, 5), False),
}
NARROW = [k for k in CASES if not CASES[k][1]]
GROWTH = (301, 2049, 97)          # on one handle at T = 24: 5 chunks, 1 chunk, 5 chunks at a smaller stride
_REF = {}          # (what, case name) -> the reference of the R rows: computed once, shared, never written to


def classes(S):
    """Sample -> parameter row: pseudo-random, every class among the first R samples (in order: class r first occurs at s = r) and among
    the last R, so in the first and in the last workgroup."""
    cls = np.random.default_rng(4000 + S).integers(0, R, S)
    cls[:R] = np.arange(R)
    cls[-R:] = np.arange(R)[::-1]
    return cls


def weights(S):
    """Non-uniform, positive, per sample (not per class), summing to about 1."""
    return np.random.default_rng(5000 + S).uniform(0.5, 1.5, S) / S


def build_rows(qc, name, table=CASES):
    """The case with its R distinct rows as the samples (what the references are computed for)."""
    spec = table[name][0]
    rows = tw.build(qc, "every/" + name, spec[:6] + (R,) + spec[7:] + (None,))
    rows["cot"] = tv.unit_cotangents(np.random.default_rng(7 + sum(map(ord, name))), R, rows["init"].size)
    return rows


def expand(rows, S):
    """The launch of S samples: sample s carries row cls[s]."""
    cls = classes(S)
    c = dict(rows)
    c.update(S=S, cls=cls, samples=list(range(S)), theta=np.ascontiguousarray(rows["theta"][cls]), cot=np.ascontiguousarray(rows["cot"][cls]),
             scale=None if rows["scale"] is None else np.ascontiguousarray(rows["scale"][cls]),
             weights=weights(S))
    return c


def _frozen(out):
    for a in (out.values() if isinstance(out, dict) else out):
        if a is not None:
            a.setflags(write=False)
    return out


def ref_grad(rows):
    key = ("grad", rows["name"])
    if key not in _REF:
        _REF[key] = _frozen((tg.reference(rows),))[0]
    return _REF[key]


def ref_finals(rows):
    key = ("finals", rows["name"])
    if key not in _REF:
        _REF[key] = _frozen(ts.reference(rows))
    return _REF[key]


def params_case(rows, c):
    """What `tp._assert_params` reads of a case.  It looks its reference up by the case's name: the reference of the R rows
    (`tp.reference`, cached there) is laid out per sample under a name of its own."""
    key = f"{rows['name']}/S{c['S']}"
    if key not in tp._REF:
        terms, sums = tp.reference(rows)
        tp._REF[key] = _frozen((terms[c["cls"]], sums[c["cls"]]))
    return dict(name=key, samples=c["samples"])


def every_sample(assertion, got, want, cls, what):
    """`assertion(got, ref[cls], what)`, all S rows; when it fails, the samples with the largest errors are named."""
    try:
        assertion(got, want, what)
    except AssertionError as e:
        err = np.abs(np.asarray(got) - want).reshape(len(cls), -1).max(axis=1)
        err = np.where(np.isnan(err), np.inf, err)
        top = np.argsort(-err, kind="stable")[:8]
        raise AssertionError(f"{what}: largest errors at (sample, class, error) "
                             f"{[(int(s), int(cls[s]), float(err[s])) for s in top]}; {int((err > 1e-6).sum())} samples off by more than 1e-6") from e


def assert_class_bits(got, cls, what):
    """got[s] carries the bits of got[cls[s]], the first sample of its class."""
    a = np.ascontiguousarray(got).reshape(len(cls), -1).view(np.uint64)
    bad = np.flatnonzero((a != a[cls]).any(axis=1))
    np.testing.assert_array_equal(a, a[cls], err_msg=f"{what}: {bad.size} samples differ from the first sample of their class, the first at "
                                                     f"(sample, class) {[(int(s), int(cls[s])) for s in bad[:8]]}")


def assert_dense(grad, ref_rows, cls, w, sw, rtol, what):
    """`grad` against sum_s w_s ref[cls[s]] in the handle's layout; +0.0 outside the derivatives."""
    want = tg._weighted(ref_rows[cls], w, sw)
    mask = tv.plain_sum(ref_rows[:1], sw)[1]
    bound = rtol * np.abs(w).sum() * max(1.0, np.abs(ref_rows).max())
    worst = np.abs(grad - want).max() / bound
    print(f"SWEEP-EVERY {what}: worst |d grad| / bound = {worst:.3e} (bound {bound:.3e}, max |grad| = {np.abs(want).max():.3e})")
    assert worst <= 1.0 and not np.isnan(grad).any(), what
    zero = grad[~mask]
    assert np.array_equal(zero.view(np.uint64), np.zeros(zero.size, dtype=np.uint64)), what
    assert np.all(grad[mask] != 0), what


def assert_fidelities(fids, J, rows, c, what):
    rfid = ref_finals(rows)[1][c["cls"]]
    every_sample(ts._assert_fids, fids, rfid, c["cls"], "SWEEP-EVERY " + what)
    assert_class_bits(fids, c["cls"], what + " fids")
    if J is not None:
        w = c["weights"]
        bound = ts.FID_ATOL * np.abs(w).sum()
        print(f"SWEEP-EVERY {what} J: |J - w . F_ref| / bound = {abs(J - np.dot(w, rfid)) / bound:.3e}")
        assert abs(J - np.dot(w, rfid)) <= bound, what


def assert_launch(sw, name, S=None, table=CASES, rule=None, kernel=None):
    """The handle's launch form at S against the table and the restated rule: a change of the chunk rule fails here.  `rule(spec, S)`
    and `kernel`: the restated rule and the kernel name of a form that is neither of the two this file runs."""
    spec, wide, (chunk, n_chunks, last), by_sqrt = table[name]
    S = spec[6] if S is None else S
    want = tw.wide_launch(2 * spec[1], spec[2], S, spec[7], wide) if rule is None else rule(spec, S)
    assert sw.kernel_name == (("mfma32-sweep" if wide else "mfma16-sweep") if kernel is None else kernel)
    assert sw.launch(S) == (True, want["chunk"], want["n_chunks"])
    if S == spec[6]:
        assert (want["chunk"], want["n_chunks"], want["last"], want["by_sqrt"]) == (chunk, n_chunks, last, by_sqrt)
    return want


# ---------------------------------------------------------------------------------------------------------------------------------
#  CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_classes_reach_both_ends():
    assert_classes_reach_both_ends({CASES[k][0][6] for k in CASES} | set(GROWTH))


def assert_classes_reach_both_ends(sizes):
    for S in sorted(sizes):
        cls = classes(S)
        assert cls.shape == (S,) and cls.min() == 0 and cls.max() == R - 1
        assert cls[:R].tolist() == list(range(R)) and cls[-R:].tolist() == list(range(R))[::-1]
        counts = np.bincount(cls, minlength=R)
        assert counts.min() >= 2                                                          # no class empty
        np.testing.assert_array_equal(cls, classes(S))
        first = np.array([np.flatnonzero(cls == r)[0] for r in range(R)])
        assert first.tolist() == list(range(R))                                           # got[cls] holds the first sample of each class
        w = weights(S)
        assert w.shape == (S,) and np.all(w > 0) and len(set(w[cls == 0])) > 1            # per sample, not per class


def test_launch_table(qc):
    """The shapes sit on the edges they are named for, by the restated rule and by `qc_sweep_desc_launch`, with and without `wide`."""
    L = qc._lib
    for name, (spec, wide, (chunk, n_chunks, last), by_sqrt) in {**CASES, **KETS3}.items():
        _, levels, m, _, _, _, S, T, _ = spec
        n = 2 * levels
        assert (n > 16) == wide
        want = tw.wide_launch(n, m, S, T, wide)
        assert want == dict(mfma=True, chunk=chunk, n_chunks=n_chunks, last=last, by_sqrt=by_sqrt), name
        assert (n_chunks - 1) * chunk + last == T - 1
        if name in ITEMS_MOD_4:
            assert (S * n_chunks) % 4 == ITEMS_MOD_4[name], name
        for flag in (0, 1):
            D = tw._wdesc(qc, flag, N=levels, m=m, T=T, cols=1)
            mf, ch, nch = C.c_int32(), C.c_int64(), C.c_int64()
            assert L.lib.qc_sweep_desc_launch(C.byref(D.d), S, C.byref(mf), C.byref(ch), C.byref(nch)) == L.QC_OK
            if wide and not flag:
                assert (bool(mf.value), ch.value, nch.value) == (False, T - 1, 0), name
            else:
                assert (bool(mf.value), ch.value, nch.value) == (True, chunk, n_chunks), name
    f = {k: ts.sweep_launch(16, CASES[k][0][2], CASES[k][0][6], CASES[k][0][7]) for k in CASES}
    assert f["sqrt-301"]["n_chunks"] % 2 == 1 and f["sqrt-97"]["n_chunks"] % 2 == 1        # workgroups straddle samples
    assert -(-ts.SWEEP_FILL // 683) == 3 == f["byS-683"]["n_chunks"] and f["byS-683"]["n_chunks"] < 7           # set by S, not by sqrt(49)
    assert f["two-2047"]["n_chunks"] == 2 and f["one-2049"]["n_chunks"] == 1 and 2047 < ts.SWEEP_FILL < 2049
    # the scratch-growth sequence on one handle at T = 24
    assert [ts.sweep_launch(16, 2, S, 24)["n_chunks"] for S in GROWTH] == [5, 1, 5]
    assert GROWTH[1] * 1 > GROWTH[2] * 5 and GROWTH[0] * 5 > GROWTH[2] * 5                # grown, then reused at a smaller size


def test_reference_reuse_is_sound(qc):
    """Two samples with equal rows have equal references, bit for bit: the forward-mode routes treat a sample by its own row alone."""
    rows = tw.build(qc, "every/reuse", ("unitary", 2, 2, 1, True, True, R, 5, U01A2, None))
    rows["cot"] = tv.unit_cotangents(np.random.default_rng(3), R, rows["init"].size)
    c = expand(rows, 2 * R + 3)
    S, cls = c["S"], c["cls"]
    pairs = [(r, S - 1 - r) for r in (0, 3, R - 1)]
    assert all(cls[a] == cls[b] for a, b in pairs)
    c["samples"] = [s for pair in pairs for s in pair]
    gs = tg.reference(c)
    terms, sums = pref.param_terms_forward(c["G0"], c["Gd"], c["Gp"], c["controls"], c["dts"], c["init"], c["theta"], c["scale"], c["samples"],
                                           c["kind"], c["goal"], c["L"], c["subspace"], c["form"])
    pb = vref.pullback_forward(c["G0"], c["Gd"], c["Gp"], c["controls"], c["dts"], c["init"], c["theta"], c["scale"], c["samples"], c["cot"])
    for what, a in dict(grad_samples=gs, terms=terms, sums=sums, **{"vjp " + k: v for k, v in pb.items()}).items():
        assert a.shape[0] == 6 and np.abs(a).max() > 1e-3, what
        np.testing.assert_array_equal(a[0::2].view(np.uint64), a[1::2].view(np.uint64), err_msg=what)
        assert not np.array_equal(a[0], a[2]), what                                         # and distinct rows differ
    # and they are the rows' own references
    np.testing.assert_array_equal(gs[0::2], tg.reference(rows)[[0, 3, R - 1]])


# ---------------------------------------------------------------------------------------------------------------------------------
#  GPU
# ---------------------------------------------------------------------------------------------------------------------------------
def grad_call(sw, Z, c):
    """One `grad_device` call with every output, the buffers prefilled with -7: (J, fids, grad, grad_samples) as numpy arrays."""
    dev = torch.device("cuda:0")
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    mk = lambda *shape: torch.full(shape, -7.0, dtype=torch.float64, device=dev)
    S = c["S"]
    dfid, dJ, dg, dgs = mk(S), mk(1), mk(sw.Z_len), mk(S, sw.T - 1, sw.n_deriv)
    torch.cuda.synchronize()
    sw.grad_device(t(Z), t(c["init"]), S, t(c["theta"]), t(c["scale"]), t(c["weights"]), dfid, dJ, dg, dgs)
    torch.cuda.synchronize()
    return dJ.item(), dfid.cpu().numpy(), dg.cpu().numpy(), dgs.cpu().numpy()


def check_grad(sw, rows, c, what):
    Z = sw.pack(c["controls"], c["dts"])
    cls = c["cls"]
    J, fids, grad, gs = grad_call(sw, Z, c)
    assert gs.shape == (c["S"], c["T"] - 1, sw.n_deriv)
    every_sample(tg._assert_samples, gs, ref_grad(rows)[cls], cls, what)
    assert_class_bits(gs, cls, what + " grad_samples")
    assert_fidelities(fids, J, rows, c, what)
    assert_dense(grad, ref_grad(rows), cls, c["weights"], sw, tg.GRAD_RTOL, what)
    # the host-buffer entry point: the same bits
    host = sw.grad(Z, c["init"], c["theta"], c["scale"], weights=c["weights"], per_sample=True)
    assert host[0] == J
    for a, b, k in zip(host[1:], (fids, grad, gs), ("fids", "grad", "grad_samples")):
        np.testing.assert_array_equal(a, b, err_msg=k)
    return fids, gs


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_grad_every_sample(qc, name):
    rows = build_rows(qc, name)
    c = expand(rows, CASES[name][0][6])
    sw = ts.make_sweep(qc, rows, wide=CASES[name][1])
    try:
        assert_launch(sw, name)
        assert sw.grad_supported
        check_grad(sw, rows, c, f"every/{name}")
    finally:
        sw.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NARROW)
def test_param_grad_every_sample(qc, name):
    """`qc_sweep_grad_params` with every output (the parameter flavour of the walk stores the per-interval derivatives too), then
    `param_grad` as callers use it."""
    rows = build_rows(qc, name)
    c = expand(rows, CASES[name][0][6])
    cls, what = c["cls"], f"every/{name} params"
    sw = ts.make_sweep(qc, rows)
    try:
        assert_launch(sw, name)
        Z = sw.pack(c["controls"], c["dts"])
        o = tp._raw(qc, sw, Z, c["init"], c["theta"], c["scale"], c["weights"])
        tp._assert_params(o["gth"], o["gsc"], params_case(rows, c), what)
        every_sample(tg._assert_samples, o["gs"], ref_grad(rows)[cls], cls, what)
        for k in ("gth", "gsc", "gs"):
            assert_class_bits(o[k], cls, f"{what} {k}")
        assert_fidelities(o["fids"], o["J"], rows, c, what)
        assert_dense(o["grad"], ref_grad(rows), cls, c["weights"], sw, tg.GRAD_RTOL, what)
        fids, gth, gsc = sw.param_grad(Z, c["init"], c["theta"], c["scale"])
        for a, k in ((fids, "fids"), (gth, "gth"), (gsc, "gsc")):
            np.testing.assert_array_equal(a, o[k], err_msg=k)
    finally:
        sw.close()


def check_vjp(sw, rows, c, what, form):
    """One `vjp_device` call with every output the form serves (tv.device_call: buffers prefilled with -7)."""
    Z = sw.pack(c["controls"], c["dts"])
    cls, S = c["cls"], c["S"]
    want = [k for k in tv.OUTPUTS if form == "16" or k not in ("grad_theta", "grad_scale")]
    out = tv.device_call(sw, Z, c, want)
    r = tv.reference(rows, form)
    for k in want:
        if k in ("grad_samples", "grad_theta", "grad_scale"):
            every_sample(tv.assert_samples, out[k], r[k][cls], cls, f"{what} {k}")
    every_sample(tv.assert_init, out["grad_init"], r["grad_init"][cls], cls, f"{what} grad_init")
    every_sample(ts._assert_states, out["finals"], ref_finals(rows)[0].T[cls], cls, f"SWEEP-EVERY {what} finals")
    for k in want:
        if k != "grad":
            assert_class_bits(out[k], cls, f"{what} {k}")
    assert_dense(out["grad"], r["grad_samples"], cls, np.ones(S), sw, tv.VJP_RTOL, what)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES) + list(KETS3))
def test_vjp_every_sample(qc, name):
    table = CASES if name in CASES else KETS3
    rows = build_rows(qc, name, table)
    wide = table[name][1]
    c = expand(rows, table[name][0][6])
    sw = ts.make_sweep(qc, rows, wide=wide)
    try:
        assert_launch(sw, name, table=table)
        assert sw.vjp_supported and sw.grad_supported == (name in CASES)
        check_vjp(sw, rows, c, f"{'32' if wide else '16'}/every/{name}", "32" if wide else "16")
    finally:
        sw.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sqrt-301", "wide-sqrt-301"])
def test_scratch_growth_every_sample(qc, name):
    """One handle at S = 301, then 2049, then 97 with the same T: 5 chunks, 1, 5 again, so dXs / dLs / dPart / dGsamp grow and are then
    reused at a smaller stride.  At every S the outputs of `grad` and `vjp` carry the bits of a fresh handle's and pass check 1."""
    rows = build_rows(qc, name)
    wide = CASES[name][1]
    form = "32" if wide else "16"
    sw = ts.make_sweep(qc, rows, wide=wide)
    try:
        seen = []
        for S in GROWTH:
            c = expand(rows, S)
            seen.append(assert_launch(sw, name, S)["n_chunks"])
            what = f"{form}/every/{name} grown to S = {S}"
            fids, gs = check_grad(sw, rows, c, what)
            out = check_vjp(sw, rows, c, what, form)
            fresh = ts.make_sweep(qc, rows, wide=wide)
            try:
                Z = fresh.pack(c["controls"], c["dts"])
                J2, fids2, grad2, gs2 = grad_call(fresh, Z, c)
                out2 = tv.device_call(fresh, Z, c, list(out))
            finally:
                fresh.close()
            np.testing.assert_array_equal(fids, fids2)
            np.testing.assert_array_equal(gs, gs2)
            for k in out:
                np.testing.assert_array_equal(out[k], out2[k], err_msg=k)
        assert seen == [5, 1, 5]
    finally:
        sw.close()
