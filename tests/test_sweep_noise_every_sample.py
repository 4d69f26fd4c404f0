"""Noise-trajectory sweeps (`qc_sweep_noise_kernel<M>`, `qc_sweep_noise_grad_kernel<M>`, `RolloutSweep.noise_eval` / `noise_grad` and
their device entries) at mid-size and filled launches, EVERY sample against the CPU reference: the method of
tests/test_sweep_every_sample.py applied to the sweeps whose perturbation amplitudes change from interval to interval.
tests/test_sweep_noise.py checks the arithmetic at S <= 40 and T <= 9: no chunk longer than 3 intervals, no launch above 120 items, and
m + n_pert in {1, 2, 3, 8} only.  What is checked here:
  * the mapping from a sample to a wave, a workgroup and a scratch slot -- item = 4 blockIdx + wave, s = item / n_chunks, the partly
    filled last workgroup, workgroups whose waves straddle two samples -- and the sample's own noise at noise + s (T-1) p;
  * the read of the noise one interval ahead (backwards: one behind) and its clamp at the chunk's end, on chunks of 4 .. 32 intervals, on
    3 .. 32 chunks and on a last chunk of 1: a wrong clamp or stride lands on a neighbouring interval's or sample's noise;
  * every instantiation M in {1, 2, 4, 6, 8}: M = 6 at m + p = 6 and at m + p = 5, where one tile slot is zero and the timestep's lane
    (lane m + p) sits below the template's width; two small cases at S = 3 tell a failure of M = 6 from one of the mapping;
  * `sNoise`, `sGnoise` and the scratch shared with `eval` and `grad`: growth and reuse at a smaller stride, host and device entries.

A launch of S samples is made of R = 8 distinct rows (theta[r], scale[r], noise[r, :, :]; the noise uniform in [-0.3, 0.3]); sample s
carries all three of row cls[s] (`classes` of test_sweep_every_sample; "long" and the small cases carry one row per sample).  The
references of tests/sweep_noise_reference.py are computed once for the R rows, so
  1. finals[s], fids[s], grad_samples[s], grad_noise[s] are compared with the reference of cls[s] by the assertions of test_sweep.py
     (states rtol 1e-10 / atol 1e-11, fidelities 1e-9) and test_sweep_noise.py (1e-9 max(1, max |want_s|));
  2. every per-sample output row carries the bits of the first sample of its class; the gradient's fids carry the evaluation's;
  3. the reduced outputs are compared with the reference's own sums: |J - w . F_ref[cls]| <= 1e-9 sum |w|, and `grad` by `assert_dense`;
  4. the host-buffer entry points return the bits of the device calls;
  5. with noise = +0.0 finals, fids, J, grad and grad_samples equal `eval` and `grad` on the same handle, whole arrays: every sample is
     tied to the plain sweep's kernels, which have every-sample tests of their own;
  6. every output buffer is prefilled with -7, so an unwritten row fails 1.
No tolerance is new.  CPU: the launch table, the instantiations, the soundness of sharing references, that no check passes on zeros or on
rows that look alike.  Measured worst ratios: profiles/sweep_hvp_noise_every_sample_summary.txt."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import sweep_noise_reference as nref
import sweep_reference as ref
import test_sweep as ts
import test_sweep_every_sample as te
import test_sweep_grad as tg
import test_sweep_noise as tn
import test_sweep_wide as tw
from test_sweep_every_sample import GROWTH, U, U01A2, KET, assert_class_bits, assert_dense, assert_launch, classes, every_sample, weights

GRAD_RTOL = tn.GRAD_RTOL
assert GRAD_RTOL == 1e-9

# name: ((state, levels, m, p, scale given, free timestep, S, T, fidelity), wide, (chunk, n_chunks, last chunk), chunk count capped by sqrt(T - 1))
CASES = {
    "sqrt-301": (("unitary", 2, 2, 1, True, True, 301, 24, U), False, (5, 5, 3), True),                  # 1505 items: odd n_chunks, partial last workgroup
    "byS-683-M6": (("unitary", 8, 4, 2, False, True, 683, 50, U), False, (17, 3, 15), False),            # chunks of 17; m + p = 6: every slot of M = 6
    "two-2047": (("unitary", 3, 1, 3, True, False, 2047, 8, U01A2), False, (4, 2, 3), False),            # just below the fill threshold; three noise lanes
    "one-2049-M2": (("ket", 4, 1, 1, True, True, 2049, 8, KET), False, (7, 1, 7), False),                # just above it: one chunk of 7
    "sqrt-97-M6pad": (("unitary", 4, 3, 2, False, True, 97, 102, U), False, (10, 11, 1), True),          # 11 chunks, a last chunk of 1; m + p = 5 in M = 6
    "sqrt-301-M1": (("unitary", 2, 0, 1, False, False, 301, 24, U), False, (5, 5, 3), True),             # no drives, fixed timestep: grad_samples has no columns
    "byS-683-M8": (("unitary", 8, 6, 2, True, False, 683, 12, U), False, (4, 3, 3), False),              # every slot of M = 8
    "long": (("unitary", 8, 2, 1, False, True, 2, 1000, U), False, (32, 32, 7), True),                   # 32 chunks of 32 intervals
    "small-M5": (("unitary", 4, 3, 2, True, True, 3, 6, U), False, (2, 3, 1), True),                     # M = 6 with a zero slot, without the mapping
    "small-M6": (("unitary", 4, 2, 4, True, True, 3, 6, U), False, (2, 3, 1), True),                     # M = 6, four noise lanes
}
ITEMS_MOD_4 = {"sqrt-301": 1, "byS-683-M6": 1, "two-2047": 2, "one-2049-M2": 1, "sqrt-97-M6pad": 3, "sqrt-301-M1": 1, "byS-683-M8": 1, "long": 0,
               "small-M5": 1, "small-M6": 1}
TEMPLATE_M = {"sqrt-301": 4, "byS-683-M6": 6, "two-2047": 4, "one-2049-M2": 2, "sqrt-97-M6pad": 6, "sqrt-301-M1": 1, "byS-683-M8": 8, "long": 4,
              "small-M5": 6, "small-M6": 6}
ONE_ROW_PER_SAMPLE = ("long", "small-M5", "small-M6")
OUTPUTS = ("finals", "fids", "gfids", "J", "grad", "grad_samples", "grad_noise")
_REF = {}          # case name -> (finals, fids, grad_samples, grad_noise) of the R rows: computed once, shared, never written to


def template_m(count):
    """The M of `QC_SWEEP_FOR_M`: the smallest of 1, 2, 4, 6, 8 that holds the drive and perturbation tiles."""
    return next(M for M in (1, 2, 4, 6, 8) if count <= M)


def n_rows(name, table=CASES, one_row=ONE_ROW_PER_SAMPLE):
    return table[name][0][6] if name in one_row else te.R


def class_map(name, S, one_row=ONE_ROW_PER_SAMPLE):
    return np.arange(S) if name in one_row else classes(S)


def build_rows(qc, name, table=CASES, rows=None):
    """The case with its distinct rows as the samples (what the references are computed for): theta, scale and a noise trajectory each."""
    spec = table[name][0]
    Rn = n_rows(name) if rows is None else rows
    c = tw.build(qc, "noise-every/" + name, spec[:6] + (Rn,) + spec[7:] + (None,))
    c["noise"] = np.random.default_rng(3).uniform(-0.3, 0.3, (Rn, c["T"] - 1, c["p"]))
    return c


def launch_of(rows, S, cls):
    """The launch of S samples: sample s carries theta, scale and noise of row cls[s]."""
    c = dict(rows)
    c.update(S=S, cls=cls, samples=list(range(S)), theta=np.ascontiguousarray(rows["theta"][cls]), noise=np.ascontiguousarray(rows["noise"][cls]),
             scale=None if rows["scale"] is None else np.ascontiguousarray(rows["scale"][cls]), weights=weights(S))
    return c


def compute_reference(c, samples):
    a = (c["G0"], c["Gd"], c["Gp"], c["controls"], c["dts"], c["init"], c["theta"], c["scale"], c["noise"])
    finals = nref.noise_finals(*a)
    fids = ref.fidelities(finals, c["kind"], c["goal"], c["L"], c["subspace"], c["form"])
    gs, gn = nref.noise_grads_forward(*a, list(samples), c["kind"], c["goal"], c["L"], c["subspace"], c["form"])
    return np.ascontiguousarray(finals.T), fids, gs, gn


def reference(rows):
    """(finals R x ns, fids R, grad_samples R x (T-1) x n_deriv, grad_noise R x (T-1) x p) of the rows."""
    key = rows["name"]
    if key not in _REF:
        _REF[key] = te._frozen(compute_reference(rows, range(rows["S"])))
    return _REF[key]


# ---------------------------------------------------------------------------------------------------------------------------------
#  CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_noise_launch_table(qc):
    """The shapes sit on the edges they are named for, by the restated rule and by `qc_sweep_desc_launch`."""
    L = qc._lib
    assert set(ITEMS_MOD_4) == set(TEMPLATE_M) == set(CASES) and len(CASES) == 10
    for name, (spec, wide, (chunk, n_chunks, last), by_sqrt) in CASES.items():
        state, levels, m, p, _, _, S, T, _ = spec
        assert not wide and state in ("unitary", "ket") and 2 * levels <= 16 and 1 <= p and m + p <= 8
        want = ts.sweep_launch(2 * levels, m, S, T)
        assert want == dict(mfma=True, chunk=chunk, n_chunks=n_chunks, last=last, by_sqrt=by_sqrt), name
        assert (n_chunks - 1) * chunk + last == T - 1
        assert (S * n_chunks) % 4 == ITEMS_MOD_4[name], name
        D = tw._wdesc(qc, 0, N=levels, m=m, T=T, cols=1)
        mf, ch, nch = C.c_int32(), C.c_int64(), C.c_int64()
        assert L.lib.qc_sweep_desc_launch(C.byref(D.d), S, C.byref(mf), C.byref(ch), C.byref(nch)) == L.QC_OK
        assert (bool(mf.value), ch.value, nch.value) == (True, chunk, n_chunks), name
        Dn = tg._GDesc(qc, N=levels, m=m, p=p, T=T, fid_kind=L.QC_FID_KET if state == "ket" else L.QC_FID_UNITARY, **(dict(cols=1) if state == "ket" else {}))
        assert tn._supported(qc, Dn)[:2] == (L.QC_OK, 1), name
    f = {k: dict(zip(("chunk", "n_chunks", "last"), CASES[k][2])) for k in CASES}
    assert f["sqrt-301"]["n_chunks"] % 2 == 1 and f["sqrt-97-M6pad"]["n_chunks"] % 2 == 1 and f["byS-683-M6"]["n_chunks"] % 2 == 1      # workgroups straddle samples
    assert -(-ts.SWEEP_FILL // 683) == 3 == f["byS-683-M6"]["n_chunks"] == f["byS-683-M8"]["n_chunks"]                                    # set by S, not by sqrt(T - 1)
    assert f["two-2047"]["n_chunks"] == 2 and f["one-2049-M2"]["n_chunks"] == 1 and 2047 < ts.SWEEP_FILL < 2049
    assert f["sqrt-97-M6pad"]["last"] == 1 and f["sqrt-97-M6pad"]["n_chunks"] == 11                    # a last chunk of one interval, many chunks
    assert max(v["chunk"] for v in f.values()) == 32 and f["long"]["n_chunks"] == 32 and f["byS-683-M6"]["chunk"] == 17      # long chunks
    # the class map of every S is checked by test_sweep_every_sample.test_classes_reach_both_ends
    mapped = {CASES[k][0][6] for k in CASES if k not in ONE_ROW_PER_SAMPLE}
    assert mapped | set(GROWTH) <= {te.CASES[k][0][6] for k in te.CASES} | set(te.GROWTH)
    for k in ONE_ROW_PER_SAMPLE:
        assert n_rows(k) == CASES[k][0][6] <= te.R and class_map(k, n_rows(k)).tolist() == list(range(n_rows(k)))
    # the scratch-growth sequence on one handle at T = 24
    assert [ts.sweep_launch(4, 2, S, 24)["n_chunks"] for S in GROWTH] == [5, 1, 5]
    assert GROWTH[1] > GROWTH[0] > GROWTH[2]                                               # sNoise, sGnoise: grown twice, then reused smaller


def test_every_noise_template_is_reached():
    """Every M of {1, 2, 4, 6, 8} occurs, M = 6 in both forms: every slot taken (m + p = 6) and one zero slot (m + p = 5), each at a filled
    launch and at S = 3; the m + p = 5 cases have a free timestep, whose lane (lane 5) then sits below the template's width."""
    seen = {}
    for name, (spec, *_) in CASES.items():
        _, _, m, p, _, free, _, _, _ = spec
        assert template_m(m + p) == TEMPLATE_M[name], name
        seen.setdefault(TEMPLATE_M[name], []).append((name, m + p, free))
    assert sorted(seen) == [1, 2, 4, 6, 8]
    six = {name: (count, free) for name, count, free in seen[6]}
    assert six == {"byS-683-M6": (6, True), "sqrt-97-M6pad": (5, True), "small-M5": (5, True), "small-M6": (6, True)}
    assert [template_m(k) for k in range(1, 9)] == [1, 2, 4, 4, 6, 6, 8, 8]
    assert CASES["small-M6"][0][3] == 4 and CASES["sqrt-301-M1"][0][2] == 0 and not CASES["sqrt-301-M1"][0][5]
    # every lane role: drives with and without a scale, 1 .. 4 noise lanes, a timestep lane or none
    assert {CASES[k][0][3] for k in CASES} == {1, 2, 3, 4} and {CASES[k][0][4] for k in CASES} == {True, False}
    assert {CASES[k][0][5] for k in CASES} == {True, False}


def test_noise_reference_reuse_is_sound(qc):
    assert_reference_reuse_is_sound(qc)


def assert_reference_reuse_is_sound(qc, name="reuse", spec=("unitary", 2, 2, 2, True, True, te.R, 5, U01A2)):
    """Two samples with equal rows have equal references, bit for bit, and distinct rows differ: `noise_finals` and `noise_grads_forward`
    treat a sample by its own row (theta, scale, noise) alone.  `spec`: a case tuple with S = R and T = 5."""
    table = {name: (spec, False, None, None)}
    rows = build_rows(qc, name, table, rows=te.R)
    S = 2 * te.R + 3
    c = launch_of(rows, S, classes(S))
    cls = c["cls"]
    pairs = [(r, S - 1 - r) for r in (0, 3, te.R - 1)]
    assert all(cls[a] == cls[b] for a, b in pairs)
    picked = [s for pair in pairs for s in pair]
    finals, fids, gs, gn = compute_reference(c, picked)
    own = compute_reference(rows, [0, 3, te.R - 1])
    for what, a, b in (("finals", finals[picked], own[0][[0, 3, te.R - 1]]), ("fids", fids[picked], own[1][[0, 3, te.R - 1]]),
                       ("grad_samples", gs, own[2]), ("grad_noise", gn, own[3])):
        a = np.ascontiguousarray(a).reshape(6, -1)
        assert np.abs(a).max() > 1e-3, what
        np.testing.assert_array_equal(a[0::2].view(np.uint64), a[1::2].view(np.uint64), err_msg=what)
        assert not np.array_equal(a[0], a[2]), what                                         # and distinct rows differ
        np.testing.assert_array_equal(a[0::2], np.asarray(b).reshape(3, -1), err_msg=what)  # and they are the rows' own references
    # the noise matters on its own: the same (theta, scale) under another trajectory has another final state and other sensitivities
    moved = compute_reference(dict(rows, noise=rows["noise"][::-1].copy()), [0])
    assert np.abs(moved[0][0] - own[0][0]).max() > 1e-3 and np.abs(moved[3][0] - own[3][0]).max() > 1e-3


@pytest.mark.parametrize("name", list(CASES))
def test_noise_rows_are_not_vacuous(qc, name):
    assert_rows_are_not_vacuous(qc, name)


def assert_rows_are_not_vacuous(qc, name, table=CASES, one_row=ONE_ROW_PER_SAMPLE):
    """No class passes on zeros and no class passes for another: every class has max |grad_noise| >= 1e-2, and any two classes differ by
    >= 1e-3 in max-norm in finals, in grad_samples (where it has columns) and in grad_noise -- 10^6 times the gradient bound."""
    Rn = n_rows(name, table, one_row)
    rows = build_rows(qc, name, table, rows=Rn)
    finals, fids, gs, gn = reference(rows)
    assert finals.shape == (Rn, rows["init"].size) and gn.shape == (Rn, rows["T"] - 1, rows["p"]) and np.isfinite(fids).all()
    assert gs.shape == (Rn, rows["T"] - 1, rows["m"] + (1 if np.ndim(rows["dts"]) else 0))
    small = np.abs(gn).reshape(Rn, -1).max(axis=1).min()
    print(f"SWEEP-NOISE every/{name} grad_noise: smallest class maximum {small:.3e}")
    assert small >= 1e-2, name
    for key, a in (("finals", finals), ("grad_samples", gs), ("grad_noise", gn)):
        if not a.size:
            assert key == "grad_samples" and name == "sqrt-301-M1"
            continue
        a = a.reshape(Rn, -1)
        apart = min(np.abs(a[i] - a[j]).max() for i, j in itertools.combinations(range(Rn), 2))
        print(f"SWEEP-NOISE every/{name} {key}: smallest distance between two classes {apart:.3e}")
        assert apart >= 1e-3, (name, key)


# ---------------------------------------------------------------------------------------------------------------------------------
#  GPU
# ---------------------------------------------------------------------------------------------------------------------------------
def device_calls(sw, Z, c):
    """One `noise_eval_device` and one `noise_grad_device` call with every output, the buffers prefilled with -7: numpy arrays."""
    dev = torch.device("cuda:0")
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    mk = lambda *shape: torch.full(shape, -7.0, dtype=torch.float64, device=dev)
    S, T, p = c["S"], sw.T, sw.p
    dZ, dinit, dn, dth, dsc, dw = t(Z), t(c["init"]), t(c["noise"]), t(c["theta"]), t(c["scale"]), t(c["weights"])
    dfin, dfid = mk(S, sw.ns), mk(S)
    dfid2, dJ, dg, dgs, dgn = mk(S), mk(1), mk(sw.Z_len), mk(S, T - 1, sw.n_deriv), mk(S, T - 1, p)
    torch.cuda.synchronize()
    sw.noise_eval_device(dZ, dinit, dn, dth, dsc, dfin, dfid)
    sw.noise_grad_device(dZ, dinit, dn, dth, dsc, dw, dfid2, dJ, dg, dgs, dgn)
    torch.cuda.synchronize()
    return dict(finals=dfin.cpu().numpy(), fids=dfid.cpu().numpy(), gfids=dfid2.cpu().numpy(), J=dJ.item(), grad=dg.cpu().numpy(),
                grad_samples=dgs.cpu().numpy(), grad_noise=dgn.cpu().numpy())


def host_calls(sw, Z, c, noise=None):
    """The same two calls through the host-buffer entry points."""
    noise = c["noise"] if noise is None else noise
    finals, fids = sw.noise_eval(Z, c["init"], noise, c["theta"], c["scale"])
    J, f2, grad, gn, gs = sw.noise_grad(Z, c["init"], noise, c["theta"], c["scale"], weights=c["weights"], per_sample=True)
    return dict(finals=np.ascontiguousarray(finals.T), fids=fids, gfids=f2, J=J, grad=grad, grad_samples=gs, grad_noise=gn)


def assert_same_bits(a, b, what):
    assert set(a) == set(b) == set(OUTPUTS)
    assert a["J"] == b["J"], f"{what}: J"
    for k in OUTPUTS:
        if k != "J":
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


def check_values(sw, out, rows, c, what):
    """Checks 1 to 3: every sample against the reference of its class, the bits of the first sample of its class, the reduced outputs
    against the reference's own sums."""
    cls, S, w = c["cls"], c["S"], c["weights"]
    rfin, rfid, rgs, rgn = reference(rows)
    assert out["finals"].shape == (S, sw.ns) and out["grad_samples"].shape == (S, sw.T - 1, sw.n_deriv) and out["grad_noise"].shape == (S, sw.T - 1, sw.p)
    every_sample(ts._assert_states, out["finals"], rfin[cls], cls, f"SWEEP-NOISE {what} finals")
    every_sample(ts._assert_fids, out["fids"], rfid[cls], cls, f"SWEEP-NOISE {what} fids")
    every_sample(tn._assert_samples, out["grad_noise"], rgn[cls], cls, f"{what} grad_noise")
    if sw.n_deriv:
        every_sample(tn._assert_samples, out["grad_samples"], rgs[cls], cls, f"{what} grad_samples")
    for k in ("finals", "fids", "grad_samples", "grad_noise"):
        assert_class_bits(out[k], cls, f"{what} {k}")
    np.testing.assert_array_equal(out["gfids"], out["fids"], err_msg=f"{what}: the gradient's fids against the evaluation's")
    bound = ts.FID_ATOL * np.abs(w).sum()
    print(f"SWEEP-NOISE {what} J: |J - w . F_ref| / bound = {abs(out['J'] - np.dot(w, rfid[cls])) / bound:.3e}")
    assert abs(out["J"] - np.dot(w, rfid[cls])) <= bound, what
    if sw.n_deriv:
        assert_dense(out["grad"], rgs, cls, w, sw, GRAD_RTOL, f"{what} grad")
    else:       # no drives and a fixed timestep: nothing to differentiate, every entry is written as +0.0
        assert out["grad"].shape == (sw.Z_len,) and np.array_equal(out["grad"].view(np.uint64), np.zeros(sw.Z_len, dtype=np.uint64)), what


def check_zero_noise(sw, Z, c, what):
    """5: an explicit +0.0 noise array is the plain sweep, value for value (np.array_equal: fma(0, P, Ga) may turn a -0 into +0, nothing else)."""
    zero = np.zeros_like(c["noise"])
    assert not np.signbit(zero).any()
    out = host_calls(sw, Z, c, zero)
    finals, fids = sw.eval(Z, c["init"], c["theta"], c["scale"])
    J, f2, grad, gs = sw.grad(Z, c["init"], c["theta"], c["scale"], weights=c["weights"], per_sample=True)
    assert np.array_equal(out["finals"], finals.T) and np.array_equal(out["fids"], fids), f"{what}: zero noise against eval"
    assert out["J"] == J and np.array_equal(out["gfids"], f2) and np.array_equal(out["grad"], grad), f"{what}: zero noise against grad"
    assert gs.shape == out["grad_samples"].shape and np.array_equal(out["grad_samples"], gs), f"{what}: zero noise against grad, per sample"
    assert np.isfinite(out["grad_noise"]).all()
    assert not np.array_equal(out["finals"], host_calls(sw, Z, c)["finals"])                 # and the noise is felt


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_noise_every_sample(qc, name):
    rows = build_rows(qc, name)
    spec = CASES[name][0]
    S = spec[6]
    c = launch_of(rows, S, class_map(name, S))
    sw = ts.make_sweep(qc, rows)
    try:
        want = assert_launch(sw, name, table=CASES)
        assert (want["chunk"], want["n_chunks"], want["last"]) == CASES[name][2] and (S * want["n_chunks"]) % 4 == ITEMS_MOD_4[name]
        assert sw.noise_supported and sw.noise_unsupported_reason is None and sw.grad_supported
        assert template_m(sw.m + sw.p) == TEMPLATE_M[name] and sw.n_deriv == spec[2] + (1 if spec[5] else 0)
        what = f"every/{name}"
        Z = sw.pack(c["controls"], c["dts"])
        out = device_calls(sw, Z, c)
        check_values(sw, out, rows, c, what)
        assert_same_bits(host_calls(sw, Z, c), out, f"{what}: the host entries against the device calls")
        check_zero_noise(sw, Z, c, what)
    finally:
        sw.close()


def scratch_growth(qc, name, table=CASES, **handle):
    """One handle at S = 301 (host buffers), then 2049 (device tensors), then 97 (host buffers) with the same T: 5 chunks, 1, 5 again, so
    dTot / dXs / dLs grow and are then reused at a smaller stride, and so do the staging buffers `sNoise` and `sGnoise`.  At every S both
    noise entries carry the bits of a fresh handle's and pass checks 1 to 3.  `handle`: the keywords of the handle beside the case's own."""
    rows = build_rows(qc, name, table, rows=te.R)
    sw = ts.make_sweep(qc, rows, **handle)
    try:
        seen = []
        for S, calls in zip(GROWTH, (host_calls, device_calls, host_calls)):
            c = launch_of(rows, S, classes(S))
            seen.append(assert_launch(sw, name, S, table=table)["n_chunks"])
            what = f"every/{name} grown to S = {S}"
            Z = sw.pack(c["controls"], c["dts"])
            out = calls(sw, Z, c)
            fresh = ts.make_sweep(qc, rows, **handle)
            try:
                out2 = calls(fresh, Z, c)
            finally:
                fresh.close()
            assert_same_bits(out, out2, f"{what}: against a fresh handle")
            check_values(sw, out, rows, c, what)
        assert seen == [5, 1, 5]
    finally:
        sw.close()


@pytest.mark.gpu
def test_noise_scratch_growth_every_sample(qc):
    scratch_growth(qc, "sqrt-301")
