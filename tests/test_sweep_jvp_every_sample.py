"""Sweep pushforwards (`qc_sweep_jvp_kernel<M>`, `qc_sweep_jvp_finish_kernel`) at mid-size and filled launches, EVERY sample against
the CPU reference: the method of tests/test_sweep_every_sample.py applied to the one derivative that came after it.  tests/test_sweep_jvp.py
checks the arithmetic at S <= 11, three samples of S = 2048 and S = 2 with 32 chunks; what is checked here is the mapping from a sample to a
wave, a workgroup and a scratch slot -- item = 4 blockIdx + wave, s = item / n_chunks, the store at tot + item * 512, the finish kernel's
read at tot + s * n_chunks * 512, the partly filled last workgroup, workgroups whose waves straddle two samples -- and the pushforward's own
scratch `dTotJ`: its growth, its reuse at a smaller stride, its independence from the `dTot` of `eval`, `grad` and `vjp` on the same handle.

A launch of S samples is made of R = 8 distinct rows (theta, scale, vtheta, vscale); sample s carries row cls[s] (`classes` of
test_sweep_every_sample).  vZ and vinit are shared by the samples, as the API has it; vscale is given even where the case passes
scale = None (valid: the cl = 1, vcl != 0 path).  The Frechet route of tests/sweep_jvp_reference.py is computed once for the R rows, so
  1. tfinals[s], tfids[s] are compared with the reference of cls[s] by `test_sweep_jvp.assert_samples` (1e-9 max(1, max |want_s|)),
     finals[s] and fids[s] by the assertions of test_sweep.py;
  2. every output row carries the bits of the first sample of its class;
  3. finals and fids carry the bits of `eval` on the same handle and inputs, whole arrays;
  4. the host-buffer entry point returns the bits of the device call;
  5. on closed systems <C_s, tfinals[s]> is the pullback's derivative paired with the direction, every sample, 2e-9 max(1, |rhs|);
  6. every output buffer is prefilled with -7, so an unwritten row fails 1.
No tolerance is new.  CPU: the soundness of sharing references, the Lindblad case's launch edge.  The class map's properties at the S used
here are test_sweep_every_sample's (no new S).  Measured worst ratios: profiles/sweep_jvp_every_sample_summary.txt."""
import ctypes as C

import numpy as np
import pytest

import sweep_jvp_reference as jref
import test_sweep as ts
import test_sweep_every_sample as te
import test_sweep_jvp as tj
import test_sweep_wide as tw
from test_sweep_every_sample import CASES, GROWTH, KETS3, R, assert_class_bits, assert_launch, classes, every_sample, expand

# the Lindblad case: n = 8 (a padded tile), 1505 items, odd n_chunks, a partly filled last workgroup; `grad` and `vjp` refuse the handle
LINDBLAD = {"lindblad-sqrt-301": (("density", 2, 2, 1, True, True, 301, 24, ("density", None, "abs")), False, (5, 5, 3), True)}
TABLE = {**{k: CASES[k] for k in te.NARROW}, "one-2049-kets3": KETS3["one-2049-kets3"], **LINDBLAD}
ITEMS_MOD_4 = {**{k: te.ITEMS_MOD_4[k] for k in te.NARROW}, "one-2049-kets3": 1, "lindblad-sqrt-301": 1}
CLOSED = [k for k in TABLE if k not in LINDBLAD]
_REF = {}          # case name -> the Frechet reference of the R rows: computed once, shared, never written to


def build_rows(qc, name, table=TABLE):
    """The R rows of test_sweep_every_sample.build_rows (the same systems, theta, scale and cotangents) plus a direction with every part
    non-zero: vcontrols, vdts (free timesteps) and vinit shared by the samples, vtheta and vscale one row per class."""
    rows = te.build_rows(qc, name, table)
    rng = np.random.default_rng(11 + sum(map(ord, name)))
    T, m, p, ns = rows["T"], rows["m"], rows["p"], rows["init"].size
    rows["vcontrols"] = rng.standard_normal((m, T))
    rows["vdts"] = 0.1 * rng.standard_normal(T) if np.ndim(rows["dts"]) else None
    rows["vinit"] = rng.standard_normal(ns) / np.sqrt(ns)
    rows["vtheta"] = rng.standard_normal((R, p))
    rows["vscale"] = rng.standard_normal((R, m))
    rows["fid"] = None if rows["kind"] is None else (rows["kind"], rows["goal"], rows["L"], rows["subspace"], rows["form"])
    return rows


def launch_of(rows, S):
    """The launch of S samples: sample s carries row cls[s], its tangent rows included."""
    c = expand(rows, S)
    c["vtheta"] = np.ascontiguousarray(rows["vtheta"][c["cls"]])
    c["vscale"] = np.ascontiguousarray(rows["vscale"][c["cls"]])
    return c


def frechet(c, samples):
    return jref.pushforward_frechet(c["G0"], c["Gd"], c["Gp"], c["controls"], c["dts"], c["init"], c["theta"], c["scale"], samples,
                                    c["vcontrols"], c["vdts"], c["vinit"], c["vtheta"], c["vscale"], c["fid"])


def reference(rows):
    key = rows["name"]
    if key not in _REF:
        _REF[key] = te._frozen(frechet(rows, range(R)))
    return _REF[key]


# ---------------------------------------------------------------------------------------------------------------------------------
#  CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def assert_reference_reuse_is_sound(qc, shapes):
    """Two samples with equal rows have equal Frechet references, bit for bit, and distinct rows differ: the route treats a sample by
    its own row (theta, scale, vtheta, vscale) alone.  `shapes`: (name, case tuple with S = R and T = 5) pairs."""
    for name, spec in shapes:
        table = {"reuse-" + name: (spec, False, None, None)}
        rows = te.build_rows(qc, "reuse-" + name, table)
        rng = np.random.default_rng(3)
        T, m, p, ns = rows["T"], rows["m"], rows["p"], rows["init"].size
        rows.update(vcontrols=rng.standard_normal((m, T)), vdts=0.1 * rng.standard_normal(T), vinit=rng.standard_normal(ns) / np.sqrt(ns),
                    vtheta=rng.standard_normal((R, p)), vscale=rng.standard_normal((R, m)),
                    fid=(rows["kind"], rows["goal"], rows["L"], rows["subspace"], rows["form"]))
        c = launch_of(rows, 2 * R + 3)
        S, cls = c["S"], c["cls"]
        pairs = [(r, S - 1 - r) for r in (0, 3, R - 1)]
        assert all(cls[a] == cls[b] for a, b in pairs)
        out = frechet(c, [s for pair in pairs for s in pair])
        own = frechet(rows, [0, 3, R - 1])
        for what in ("finals", "tfinals", "tfids"):
            a = out[what]
            assert a.shape[0] == 6 and np.abs(a).max() > 1e-3, (name, what)
            np.testing.assert_array_equal(a[0::2].view(np.uint64), a[1::2].view(np.uint64), err_msg=f"{name} {what}")
            assert not np.array_equal(a[0], a[2]), (name, what)                            # and distinct rows differ
            np.testing.assert_array_equal(a[0::2], own[what], err_msg=f"{name} {what}")   # and they are the rows' own references
        # the tangent rows matter on their own: the same (theta, scale) along another (vtheta, vscale) has another tangent
        other = dict(rows, vtheta=rows["vtheta"][::-1].copy(), vscale=rows["vscale"][::-1].copy())
        moved = frechet(other, [0])
        np.testing.assert_array_equal(moved["finals"], own["finals"][:1])
        assert np.abs(moved["tfinals"] - own["tfinals"][:1]).max() > 1e-3


def test_pushforward_reference_reuse_is_sound(qc):
    assert_reference_reuse_is_sound(qc, (("closed", ("unitary", 2, 2, 1, True, True, R, 5, te.U01A2)),
                                         ("open", ("density", 2, 2, 1, False, True, R, 5, ("density", None, "abs")))))


def test_lindblad_launch_edge(qc):
    """Every case sits on the edge it is named for, by the restated rule and by `qc_sweep_desc_launch`; the Lindblad one is new here."""
    L = qc._lib
    for name, (spec, wide, (chunk, n_chunks, last), by_sqrt) in TABLE.items():
        state, levels, m, _, _, _, S, T, _ = spec
        N = levels * levels if state == "density" else levels
        assert not wide and 2 * N <= 16
        want = tw.wide_launch(2 * N, m, S, T, False)
        assert want == dict(mfma=True, chunk=chunk, n_chunks=n_chunks, last=last, by_sqrt=by_sqrt), name
        assert (n_chunks - 1) * chunk + last == T - 1
        assert (S * n_chunks) % 4 == ITEMS_MOD_4[name], name
        D = tw._wdesc(qc, 0, N=N, m=m, T=T, cols=1)
        mf, ch, nch = C.c_int32(), C.c_int64(), C.c_int64()
        assert L.lib.qc_sweep_desc_launch(C.byref(D.d), S, C.byref(mf), C.byref(ch), C.byref(nch)) == L.QC_OK
        assert (bool(mf.value), ch.value, nch.value) == (True, chunk, n_chunks), name
    spec = LINDBLAD["lindblad-sqrt-301"][0]
    assert 2 * spec[1] ** 2 == 8 and LINDBLAD["lindblad-sqrt-301"][2] == (5, 5, 3) and 301 * 5 % 4 == 1
    # no S here whose class map test_sweep_every_sample.test_classes_reach_both_ends leaves unchecked
    assert {TABLE[k][0][6] for k in TABLE} | set(GROWTH) <= {CASES[k][0][6] for k in CASES} | set(te.GROWTH)
    assert [ts.sweep_launch(8, 2, S, spec[7])["n_chunks"] for S in GROWTH] == [5, 1, 5]


# ---------------------------------------------------------------------------------------------------------------------------------
#  GPU
# ---------------------------------------------------------------------------------------------------------------------------------
def jvp_call(sw, c):
    """One `jvp_device` call with every output the handle has along the full direction (tj.device_call: buffers prefilled with -7)."""
    Z = sw.pack(c["controls"], c["dts"])
    dirs = tj.direction(sw, c)
    assert all(v is not None and np.all(v != 0) for k, v in dirs.items() if k != "vZ") and np.count_nonzero(dirs["vZ"]) >= (sw.T - 1) * sw.n_deriv
    return Z, dirs, tj.device_call(sw, Z, c, tj.outputs_of(sw), dirs)


def check_values(out, rows, c, what):
    """Checks 1 and 2: every sample against the reference of its class, and the bits of the first sample of its class."""
    cls, r = c["cls"], reference(rows)
    rfin, rfid = te.ref_finals(rows)
    every_sample(tj.assert_samples, out["tfinals"], r["tfinals"][cls], cls, f"{what} tfinals")
    every_sample(ts._assert_states, out["finals"], rfin.T[cls], cls, f"SWEEP-JVP {what} finals")
    if "tfids" in out:
        every_sample(tj.assert_samples, out["tfids"][:, None], r["tfids"][cls][:, None], cls, f"{what} tfids")
        every_sample(ts._assert_fids, out["fids"], rfid[cls], cls, f"SWEEP-JVP {what} fids")
    for k in out:
        assert_class_bits(out[k], cls, f"{what} {k}")


def check_jvp(sw, rows, c, what):
    Z, dirs, out = jvp_call(sw, c)
    assert set(out) == ({"finals", "fids", "tfinals", "tfids"} if rows["kind"] is not None else {"finals", "tfinals"})
    assert out["tfinals"].shape == (c["S"], sw.ns)
    check_values(out, rows, c, what)
    # 3: the sweep's own finals / fids, whole arrays
    finals, fids = sw.eval(Z, c["init"], c["theta"], c["scale"])
    np.testing.assert_array_equal(out["finals"], finals.T, err_msg=f"{what}: finals against eval")
    if "fids" in out:
        np.testing.assert_array_equal(out["fids"], fids, err_msg=f"{what}: fids against eval")
    else:
        assert fids is None
    # 4: the host-buffer entry point
    host = sw.jvp(Z, c["init"], dirs["vZ"], c["theta"], c["scale"], vinit=dirs["vinit"], vtheta=dirs["vtheta"], vscale=dirs["vscale"], fids="tfids" in out)
    np.testing.assert_array_equal(host[0] if "tfids" in out else host, out["tfinals"], err_msg=f"{what}: host tfinals")
    if "tfids" in out:
        np.testing.assert_array_equal(host[1], out["tfids"], err_msg=f"{what}: host tfids")
    return Z, dirs, out


def check_adjoint(sw, c, Z, dirs, out, what):
    """5: <C_s, tfinals[s]> against the pullback's derivatives paired with the direction, unit cotangents per class, every sample."""
    cot, cls = c["cot"], c["cls"]
    pull = sw.vjp(Z, c["init"], cot, c["theta"], c["scale"], per_sample=True, init_grad=True, params=True)
    lhs = np.einsum("sn,sn->s", cot, out["tfinals"])
    rhs = tj.pairing(sw, c, dirs, pull)
    ratio = np.abs(lhs - rhs) / (2 * tj.JVP_RTOL * np.maximum(1.0, np.abs(rhs)))
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    print(f"SWEEP-JVP {what} adjoint identity: worst error / bound = {ratio.max():.3e} (max |value| = {np.abs(rhs).max():.3e})")
    top = np.argsort(-ratio, kind="stable")[:8]
    assert ratio.max() <= 1.0 and np.abs(rhs).max() > 1e-3, f"{what}: (sample, class, ratio) {[(int(s), int(cls[s]), float(ratio[s])) for s in top]}"
    return pull


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TABLE))
def test_jvp_every_sample(qc, name):
    rows = build_rows(qc, name)
    c = launch_of(rows, TABLE[name][0][6])
    sw = ts.make_sweep(qc, rows)
    try:
        want = assert_launch(sw, name, table=TABLE)
        assert (c["S"] * want["n_chunks"]) % 4 == ITEMS_MOD_4[name]
        assert sw.jvp_supported and sw.jvp_unsupported_reason is None
        assert sw.vjp_supported == (name in CLOSED) and sw.grad_supported == (name in CLOSED and rows["kind"] is not None)
        if name in LINDBLAD:
            assert rows["n"] == 8 and (want["chunk"], want["n_chunks"], want["last"]) == (5, 5, 3) and c["S"] * want["n_chunks"] % 4 == 1
        if not TABLE[name][0][4]:
            assert c["scale"] is None and np.all(c["vscale"] != 0)              # the cl = 1, vcl != 0 path
        Z, dirs, out = check_jvp(sw, rows, c, f"every/{name}")
        if name in CLOSED:
            check_adjoint(sw, c, Z, dirs, out, f"every/{name}")
    finally:
        sw.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sqrt-301", "lindblad-sqrt-301"])
def test_jvp_scratch_growth_every_sample(qc, name):
    """One handle at S = 301, then 2049, then 97 with the same T: 5 chunks, 1, 5 again, so `dTotJ` grows and is then reused at a smaller
    stride.  At every S, in this order: `eval`, `jvp_device`, (closed handle) `vjp`, `jvp_device`.  The two pushforwards are bit-equal, each
    carries the bits of a fresh handle's and passes check 1, and `eval` afterwards returns the bits of `eval` before: `dTotJ` and the
    `dTot` of the other entry points do not touch each other."""
    rows = build_rows(qc, name)
    sw = ts.make_sweep(qc, rows)
    try:
        seen = []
        for S in GROWTH:
            c = launch_of(rows, S)
            seen.append(assert_launch(sw, name, S, table=TABLE)["n_chunks"])
            what = f"every/{name} grown to S = {S}"
            Z = sw.pack(c["controls"], c["dts"])
            before = sw.eval(Z, c["init"], c["theta"], c["scale"])
            _, dirs, first = jvp_call(sw, c)
            if name in CLOSED:
                check_adjoint(sw, c, Z, dirs, first, what)
            _, _, second = jvp_call(sw, c)
            after = sw.eval(Z, c["init"], c["theta"], c["scale"])
            fresh = ts.make_sweep(qc, rows)
            try:
                _, _, third = jvp_call(fresh, c)
            finally:
                fresh.close()
            for k in first:
                np.testing.assert_array_equal(second[k], first[k], err_msg=f"{what}: {k} of the second call")
                np.testing.assert_array_equal(third[k], first[k], err_msg=f"{what}: {k} of a fresh handle")
            check_values(first, rows, c, what)
            check_values(second, rows, c, what + ", second call")
            for a, b, k in zip(after, before, ("finals", "fids")):
                np.testing.assert_array_equal(a, b, err_msg=f"{what}: {k} of eval after the pushforward")
            np.testing.assert_array_equal(first["finals"], before[0].T)
            np.testing.assert_array_equal(first["fids"], before[1])
        assert seen == [5, 1, 5]
    finally:
        sw.close()
