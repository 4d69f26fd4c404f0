"""Sweep Hessian products (`qc_sweep_hvp_kernel<M>` and its seed and reductions, `RolloutSweep.hvp` / `hvp_device`) at mid-size and filled
launches, EVERY sample against the CPU reference: the method of tests/test_sweep_every_sample.py applied to the tangent of the pullback.
tests/test_sweep_hvp.py checks the arithmetic at S <= 37 (185 items), three samples of S = 2048 and S = 2 at T = 1000; what is checked here
is the mapping from a sample to a wave, a workgroup and a scratch slot -- item = 4 blockIdx + wave, s = item / n_chunks, the chunk-end
states, adjoints and their tangents at item * ns, the partly filled last workgroup, workgroups whose waves straddle two samples -- and the
scratch the Hessian product shares with `grad` and `vjp` on the same handle (`dTot`, `dXs`, `dLs`) next to its own (`dXsT`, `dLsT`,
`dTGsamp`): growth, reuse at a smaller stride, a call of the other entries before and after.

A launch of S samples is made of R = 8 distinct rows (theta, scale, cot, vtheta, vscale, vcot); sample s carries row cls[s] (`classes` of
test_sweep_every_sample).  vcontrols, vdts and vinit are shared by the samples, as the API has it; every direction is non-zero.  The
recurrence route of tests/sweep_hvp_reference.py is computed once for the R rows, so
  1. tgrad_samples[s], tgrad_init[s] are compared with the reference of cls[s] by `test_sweep_hvp.assert_samples` (1e-9 max(1, max |want_s|));
  2. every per-sample output row carries the bits of the first sample of its class;
  3. tgrad is, bit for bit, the plain sum in ascending s of the kernel's own per-sample values (`test_sweep_hvp.scatter`), and is compared
     with the reference's sum by `assert_dense` with unit weights: |tgrad - sum_s ref[cls[s]]| <= 1e-9 S max(1, max |ref|), +0.0 elsewhere;
  4. the host-buffer entry point returns the bits of the device call;
  5. along vcot alone the product is the pullback of vcot, every sample: 2e-9 max(1, max |.|_s), both sides being within 1e-9 of the truth;
  6. every output buffer is prefilled with -7, so an unwritten row fails 1.
No tolerance is new.  CPU: the table, the soundness of sharing references, that no check passes on zeros or on rows that look alike.
The class map's properties at the S used here are test_sweep_every_sample's (no new S).  Measured worst ratios:
profiles/sweep_hvp_noise_every_sample_summary.txt."""
import ctypes as C
import itertools

import numpy as np
import pytest

import sweep_hvp_reference as href
import test_sweep as ts
import test_sweep_every_sample as te
import test_sweep_hvp as th
import test_sweep_jvp_every_sample as tje
import test_sweep_vjp as tv
import test_sweep_wide as tw
from test_sweep_every_sample import GROWTH, R, assert_class_bits, assert_dense, assert_launch, every_sample

HVP_RTOL = th.HVP_RTOL
# the closed cases of the pushforward's table: the five narrow shapes and three kets without a fidelity (a Lindblad handle has no pullback)
TABLE = {k: v for k, v in tje.TABLE.items() if k not in tje.LINDBLAD}
ITEMS_MOD_4 = {k: tje.ITEMS_MOD_4[k] for k in TABLE}
LINEAR = ["sqrt-301", "one-2049-kets3"]
_REF = {}          # case name -> the recurrence reference of the R rows: computed once, shared, never written to


def build_rows(qc, name, table=tje.TABLE):
    """The R rows of test_sweep_jvp_every_sample.build_rows (systems, theta, scale, cot, and a direction with every part non-zero) plus
    the direction of the cotangent, one row per class."""
    rows = tje.build_rows(qc, name, table)
    ns = rows["init"].size
    rows["vcot"] = np.random.default_rng(1).standard_normal((R, ns)) / np.sqrt(ns)
    return rows


def launch_of(rows, S):
    """The launch of S samples: sample s carries row cls[s], its tangent rows included."""
    c = tje.launch_of(rows, S)
    c["vcot"] = np.ascontiguousarray(rows["vcot"][c["cls"]])
    return c


def frechet(c, samples):
    return href.hessian_product_frechet(c["G0"], c["Gd"], c["Gp"], c["controls"], c["dts"], c["init"], c["theta"], c["scale"], samples, c["cot"],
                                        c["vcontrols"], c["vdts"], c["vinit"], c["vtheta"], c["vscale"], c["vcot"])


def reference(rows):
    key = rows["name"]
    if key not in _REF:
        _REF[key] = te._frozen(frechet(rows, range(R)))
    return _REF[key]


# ---------------------------------------------------------------------------------------------------------------------------------
#  CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_hvp_launch_table(qc):
    """The cases are the pushforward's closed ones, and each sits on the edge it is named for, by the restated rule and by
    `qc_sweep_desc_launch`."""
    assert list(TABLE) == ["sqrt-301", "byS-683", "two-2047", "one-2049", "sqrt-97", "one-2049-kets3"] == tje.CLOSED
    assert all(TABLE[k] is tje.TABLE[k] for k in TABLE)
    want = {"sqrt-301": (301, (5, 5, 3)), "byS-683": (683, (17, 3, 15)), "two-2047": (2047, (4, 2, 3)), "one-2049": (2049, (7, 1, 7)),
            "sqrt-97": (97, (10, 11, 1)), "one-2049-kets3": (2049, (7, 1, 7))}
    L = qc._lib
    for name, (spec, wide, (chunk, n_chunks, last), by_sqrt) in TABLE.items():
        _, levels, m, _, _, _, S, T, _ = spec
        assert not wide and 2 * levels <= 16 and (S, (chunk, n_chunks, last)) == want[name]
        assert tw.wide_launch(2 * levels, m, S, T, False) == dict(mfma=True, chunk=chunk, n_chunks=n_chunks, last=last, by_sqrt=by_sqrt), name
        assert (n_chunks - 1) * chunk + last == T - 1
        assert (S * n_chunks) % 4 == ITEMS_MOD_4[name], name
        D = tw._wdesc(qc, 0, N=levels, m=m, T=T, cols=1)
        mf, ch, nch = C.c_int32(), C.c_int64(), C.c_int64()
        assert L.lib.qc_sweep_desc_launch(C.byref(D.d), S, C.byref(mf), C.byref(ch), C.byref(nch)) == L.QC_OK
        assert (bool(mf.value), ch.value, nch.value) == (True, chunk, n_chunks), name
    assert TABLE["byS-683"][0][1] == 8 and TABLE["byS-683"][0][2] == 6                     # 2N = 16, M = 6
    assert TABLE["sqrt-97"][0][7] == 102 and 301 * 5 == 1505 and 2047 < ts.SWEEP_FILL < 2049
    # no S here whose class map test_sweep_every_sample.test_classes_reach_both_ends leaves unchecked
    assert {TABLE[k][0][6] for k in TABLE} | set(GROWTH) <= {te.CASES[k][0][6] for k in te.CASES} | set(te.GROWTH)
    spec = TABLE["sqrt-301"][0]
    assert [ts.sweep_launch(2 * spec[1], spec[2], S, spec[7])["n_chunks"] for S in GROWTH] == [5, 1, 5]
    assert set(LINEAR) <= set(TABLE)


def test_hvp_reference_reuse_is_sound(qc):
    assert_reference_reuse_is_sound(qc)


def assert_reference_reuse_is_sound(qc, name="hvp-reuse", spec=("unitary", 2, 2, 1, True, True, R, 5, te.U01A2)):
    """Two samples with equal rows have equal recurrence references, bit for bit, and distinct rows differ: the route treats a sample by
    its own row (theta, scale, cot, vtheta, vscale, vcot) alone.  `spec`: a case tuple with S = R and T = 5."""
    table = {name: (spec, False, None, None)}
    rows = te.build_rows(qc, name, table)
    rng = np.random.default_rng(3)
    T, m, p, ns = rows["T"], rows["m"], rows["p"], rows["init"].size
    rows.update(vcontrols=rng.standard_normal((m, T)), vdts=0.1 * rng.standard_normal(T), vinit=rng.standard_normal(ns) / np.sqrt(ns),
                vtheta=rng.standard_normal((R, p)), vscale=rng.standard_normal((R, m)), vcot=rng.standard_normal((R, ns)) / np.sqrt(ns))
    c = launch_of(rows, 2 * R + 3)
    S, cls = c["S"], c["cls"]
    pairs = [(r, S - 1 - r) for r in (0, 3, R - 1)]
    assert all(cls[a] == cls[b] for a, b in pairs)
    out = frechet(c, [s for pair in pairs for s in pair])
    own = frechet(rows, [0, 3, R - 1])
    for what in ("tgrad_samples", "tgrad_init"):
        a = out[what]
        assert a.shape[0] == 6 and np.abs(a).max() > 1e-3, what
        np.testing.assert_array_equal(a[0::2].view(np.uint64), a[1::2].view(np.uint64), err_msg=what)
        assert not np.array_equal(a[0], a[2]), what                                        # and distinct rows differ
        np.testing.assert_array_equal(a[0::2], own[what], err_msg=what)                    # and they are the rows' own references
    # the cotangent's direction matters on its own: the same row along another vcot has another product
    moved = frechet(dict(rows, vcot=rows["vcot"][::-1].copy()), [0])
    assert np.abs(moved["tgrad_samples"] - own["tgrad_samples"][:1]).max() > 1e-3 and np.abs(moved["tgrad_init"] - own["tgrad_init"][:1]).max() > 1e-3


@pytest.mark.parametrize("name", list(TABLE))
def test_hvp_rows_are_not_vacuous(qc, name):
    assert_rows_are_not_vacuous(qc, name)


def assert_rows_are_not_vacuous(qc, name, table=TABLE):
    """No class passes on zeros and no class passes for another: every class has max |tgrad_samples| >= 1e-2 and max |tgrad_init| >= 1e-1,
    and any two classes differ by >= 1e-3 in max-norm in both outputs -- 10^6 times the bound a sample is held to."""
    rows = build_rows(qc, name, table)
    for k in ("vcontrols", "vinit", "vtheta", "vscale", "vcot", "cot"):
        assert np.all(rows[k] != 0), k
    assert rows["vdts"] is None or np.all(rows["vdts"] != 0)
    r = reference(rows)
    floor = dict(tgrad_samples=1e-2, tgrad_init=1e-1)
    for key in ("tgrad_samples", "tgrad_init"):
        a = r[key].reshape(R, -1)
        small = np.abs(a).max(axis=1).min()
        apart = min(np.abs(a[i] - a[j]).max() for i, j in itertools.combinations(range(R), 2))
        print(f"SWEEP-HVP every/{name} {key}: smallest class maximum {small:.3e}, smallest distance between two classes {apart:.3e}")
        assert small >= floor[key] and apart >= 1e-3, (name, key)


# ---------------------------------------------------------------------------------------------------------------------------------
#  GPU
# ---------------------------------------------------------------------------------------------------------------------------------
def hvp_call(sw, c, dirs=None):
    """One `hvp_device` call with every output along the full direction (th.device_call: buffers prefilled with -7)."""
    Z = sw.pack(c["controls"], c["dts"])
    if dirs is None:
        dirs = th.direction(sw, c)
        assert all(v is not None and np.all(v != 0) for k, v in dirs.items() if k != "vZ")
        assert np.count_nonzero(dirs["vZ"]) >= (sw.T - 1) * sw.n_deriv
    assert th.outputs_of(sw) == list(th.OUTPUTS)
    return Z, dirs, th.device_call(sw, Z, c, list(th.OUTPUTS), dirs)


def check_values(sw, out, rows, c, what):
    """Checks 1 to 3: every sample against the reference of its class, the bits of the first sample of its class, the sum."""
    cls, S, r = c["cls"], c["S"], reference(rows)
    assert out["tgrad_samples"].shape == (S, sw.T - 1, sw.n_deriv) and out["tgrad_init"].shape == (S, sw.ns)
    every_sample(th.assert_samples, out["tgrad_samples"], r["tgrad_samples"][cls], cls, f"{what} tgrad_samples")
    every_sample(th.assert_samples, out["tgrad_init"], r["tgrad_init"][cls], cls, f"{what} tgrad_init")
    assert_class_bits(out["tgrad_samples"], cls, f"{what} tgrad_samples")
    assert_class_bits(out["tgrad_init"], cls, f"{what} tgrad_init")
    np.testing.assert_array_equal(out["tgrad"], th.scatter(th.layout(sw), out["tgrad_samples"]), err_msg=f"{what}: tgrad is the plain sum")
    assert_dense(out["tgrad"], r["tgrad_samples"], cls, np.ones(S), sw, HVP_RTOL, f"{what} tgrad")


def check_hvp(sw, rows, c, what):
    Z, dirs, out = hvp_call(sw, c)
    check_values(sw, out, rows, c, what)
    # 4: the host-buffer entry point
    host = sw.hvp(Z, c["init"], c["cot"], c["theta"], c["scale"], vZ=dirs["vZ"], vinit=dirs["vinit"], vtheta=dirs["vtheta"], vscale=dirs["vscale"],
                  vcot=dirs["vcot"], per_sample=True, init_grad=True)
    assert len(host) == 3
    for a, k in zip(host, th.OUTPUTS):
        np.testing.assert_array_equal(a, out[k], err_msg=f"{what}: host {k}")
    return Z, dirs, out


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TABLE))
def test_hvp_every_sample(qc, name):
    rows = build_rows(qc, name)
    c = launch_of(rows, TABLE[name][0][6])
    sw = ts.make_sweep(qc, rows)
    try:
        want = assert_launch(sw, name, table=TABLE)
        assert (c["S"] * want["n_chunks"]) % 4 == ITEMS_MOD_4[name]
        assert sw.hvp_supported and sw.hvp_unsupported_reason is None and sw.vjp_supported
        if not TABLE[name][0][4]:
            assert c["scale"] is None and np.all(c["vscale"] != 0)              # the cl = 1, vcl != 0 path
        check_hvp(sw, rows, c, f"every/{name}")
    finally:
        sw.close()


def linear_part(qc, name, table=TABLE, **handle):
    """5: with only vcot given the product is linear in it: tgrad_samples[s] and tgrad_init[s] are the pullback's grad_samples[s] and
    grad_init[s] with cot = vcot, every sample.  Both sides are within 1e-9 of the truth: 2e-9 max(1, max |.|_s).  `handle`: the
    keywords of the handle beside the case's own."""
    rows = build_rows(qc, name, table)
    c = launch_of(rows, table[name][0][6])
    cls = c["cls"]
    sw = ts.make_sweep(qc, rows, **handle)
    try:
        assert_launch(sw, name, table=table)
        Z, _, out = hvp_call(sw, c, dict(vcot=c["vcot"]))
        pull = sw.vjp(Z, c["init"], c["vcot"], c["theta"], c["scale"], per_sample=True, init_grad=True)
        for key, other in (("tgrad_samples", pull[1]), ("tgrad_init", pull[2])):
            got, other = out[key].reshape(c["S"], -1), other.reshape(c["S"], -1)
            ratio = np.abs(got - other).max(axis=1) / (2 * HVP_RTOL * np.maximum(1.0, np.abs(other).max(axis=1)))
            ratio = np.where(np.isnan(ratio), np.inf, ratio)
            print(f"SWEEP-HVP every/{name} {key} along vcot alone vs qc_sweep_vjp: worst error / bound = {ratio.max():.3e} "
                  f"(max |value| = {np.abs(other).max():.3e})")
            top = np.argsort(-ratio, kind="stable")[:8]
            assert ratio.max() <= 1.0, f"{name} {key}: (sample, class, ratio) {[(int(s), int(cls[s]), float(ratio[s])) for s in top]}"
            assert np.abs(other).max(axis=1).min() > 1e-3, key
            assert_class_bits(out[key], cls, f"every/{name} {key} along vcot alone")
        worst = th.ratio(out["tgrad"], pull[0]) / 2
        print(f"SWEEP-HVP every/{name} tgrad along vcot alone vs qc_sweep_vjp: worst error / bound = {worst:.3e} (max |value| = {np.abs(pull[0]).max():.3e})")
        assert worst <= 1.0 and np.abs(pull[0]).max() > 1e-3
    finally:
        sw.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", LINEAR)
def test_hvp_linear_part_every_sample(qc, name):
    linear_part(qc, name)


def scratch_growth(qc, name, table=TABLE, **handle):
    """One handle at S = 301, then 2049, then 97 with the same T: 5 chunks, 1, 5 again, so dTot / dXs / dLs (shared with `grad` and `vjp`)
    and dXsT / dLsT / dTGsamp grow and are then reused at a smaller stride.  At every S, in this order: `grad_device`, `hvp_device`,
    `vjp_device`.  The Hessian product passes checks 1 to 3 and carries the bits of a fresh handle's, and so does the pullback after it.
    `handle`: the keywords of the handle beside the case's own."""
    rows = build_rows(qc, name, table)
    sw = ts.make_sweep(qc, rows, **handle)
    try:
        seen = []
        for S in GROWTH:
            c = launch_of(rows, S)
            seen.append(assert_launch(sw, name, S, table=table)["n_chunks"])
            what = f"every/{name} grown to S = {S}"
            Z = sw.pack(c["controls"], c["dts"])
            J, fids, grad, gs = te.grad_call(sw, Z, c)
            _, dirs, out = hvp_call(sw, c)
            pull = tv.device_call(sw, Z, c, list(tv.OUTPUTS))
            fresh = ts.make_sweep(qc, rows, **handle)
            try:
                _, _, out2 = hvp_call(fresh, c, dirs)
            finally:
                fresh.close()
            fresh = ts.make_sweep(qc, rows, **handle)
            try:
                pull2 = tv.device_call(fresh, Z, c, list(tv.OUTPUTS))
                J2, fids2, grad2, gs2 = te.grad_call(fresh, Z, c)
            finally:
                fresh.close()
            check_values(sw, out, rows, c, what)
            for k in out:
                np.testing.assert_array_equal(out[k], out2[k], err_msg=f"{what}: {k} of a fresh handle")
            for k in pull:
                np.testing.assert_array_equal(pull[k], pull2[k], err_msg=f"{what}: the pullback's {k} after the Hessian product")
            assert J == J2
            for a, b, k in ((fids, fids2, "fids"), (grad, grad2, "grad"), (gs, gs2, "grad_samples")):
                np.testing.assert_array_equal(a, b, err_msg=f"{what}: the gradient's {k} before the Hessian product")
        assert seen == [5, 1, 5]
    finally:
        sw.close()


@pytest.mark.gpu
def test_hvp_scratch_growth_every_sample(qc):
    scratch_growth(qc, "sqrt-301")
