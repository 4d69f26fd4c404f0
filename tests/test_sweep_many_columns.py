"""Sweeps of many-column states (`RolloutSweep(cols=K)`, K kets propagated at once, no fidelity), up to the 4096 entries (2N x state_cols)
that `sweep_validate` admits.  `grad` and `vjp` stop at 16 columns; `eval` and `jvp` serve all of it, and the other sweep tests stop at 128
entries on "mfma16-sweep" and 512 on "mfma32-sweep".  What runs here for the first time, in `qc_sweep_finish_kernel` (ld = 16 and 32) and
`qc_sweep_jvp_finish_kernel`:
  * the second and later trips of every `for (idx = tid; idx < ns; idx += 256)` loop: the state load, the product with idx % n and idx / n,
    the stores of finals and tfinals (ns > 256);
  * the opt-in to more than 64 KiB of dynamic LDS: the pushforward finish asks for (4 ns + 512) 8 bytes (ns > 1920, 135168 bytes at
    ns = 4096), the forward finish for (2 ns + ld^2) 8 bytes (ns > 3968 at ld = 16, ns > 3584 at ld = 32).
The launch is S = 3, T = 10 (3 chunks of 3), free timestep, m = 2, p = 1, scale given, every direction non-zero; one case runs at S = 37
with the class method of tests/test_sweep_every_sample.py (111 items, the scratch stride s * n_chunks * 512 with a multi-trip finish).
Every sample and every entry is compared with `pushforward_frechet` / `sweep_finals`; the tolerances are those of tests/test_sweep.py and
tests/test_sweep_jvp.py, none is new.  Bit for bit: the two entry points' finals, repeated calls, a column against a `cols = 1` handle run on
that column alone (each entry of the finish kernels is its own fma chain in a fixed order, and the chunk totals do not depend on the
state), and a small state before and after a large one has opted the kernels in.  CPU: the descriptor limit, the two reference routes at many
columns, the LDS table (the two formulas restated and matched against the source lines that compute them), the class map at S = 37."""
import ctypes as C
import os

import numpy as np
import pytest

import sweep_jvp_reference as jref
import sweep_reference as ref
import test_sweep as ts
import test_sweep_every_sample as te
import test_sweep_grad as tg
import test_sweep_jvp as tj
import test_sweep_wide as tw
from test_sweep_every_sample import R, assert_class_bits, classes, every_sample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S0, T0, M0, P0 = 3, 10, 2, 1
LDS_OPT_IN = 64 * 1024
# name: (levels N, columns, wide, pushforward finish bytes against 65536, forward finish bytes against 65536)
MANY = {
    "cols17": (8, 17, False, "<", "<"),                       # ns = 272: the second trip of the strided loops, for 16 threads only
    "cols120": (8, 120, False, "=", "<"),                     # ns = 1920: pushforward finish at exactly 65536 bytes, no opt-in
    "cols121": (8, 121, False, ">", "<"),                     # ns = 1936: the first size at which the pushforward finish opts in
    "cols248": (8, 248, False, ">", "="),                     # ns = 3968: forward finish at exactly 65536 bytes
    "cols256": (8, 256, False, ">", ">"),                     # ns = 4096, the largest state: both opt in, 135168 bytes
    "levels3-cols682": (3, 682, False, ">", ">"),             # ns = 4092, n = 6: idx % n off a power of two, padded tile, 16 trips
    "levels2-cols1024": (2, 1024, False, ">", ">"),           # ns = 4096, n = 4
    "wide-levels9-cols227": (9, 227, True, None, ">"),        # ns = 4086, n = 18: the ld = 32 opt-in (ns > 3584); eval only
    "wide-levels16-cols128": (16, 128, True, None, ">"),      # ns = 4096: a full 32-wide tile at the largest state; eval only
}
NARROW = [k for k in MANY if not MANY[k][2]]
WIDE = [k for k in MANY if MANY[k][2]]
NS = {"cols17": 272, "cols120": 1920, "cols121": 1936, "cols248": 3968, "cols256": 4096, "levels3-cols682": 4092, "levels2-cols1024": 4096,
      "wide-levels9-cols227": 4086, "wide-levels16-cols128": 4096}
S_BIG = 37         # `cols121` once more, with R classes over 37 samples
_REF = {}          # (what, case name) -> reference: computed once, shared, never written to


def jvp_finish_lds(ns):
    """qc_sweep_jvp_finish_kernel: x, its successor, their tangents, one chunk total and its tangent (ld = 16)."""
    return (4 * ns + 512) * 8


def finish_lds(ns, ld):
    """qc_sweep_finish_kernel: x, its successor, one chunk total."""
    return (2 * ns + ld * ld) * 8


def side(nbytes):
    return "<" if nbytes < LDS_OPT_IN else ("=" if nbytes == LDS_OPT_IN else ">")


def build_many(qc, name, N, cols, S=S0):
    """test_sweep_wide.build's system, controls and samples for K kets, the K columns drawn here: random complex, normalised.  With a
    direction whose every part is non-zero."""
    c = tw.build(qc, "many/" + name, ("kets3", N, M0, P0, True, True, S, T0, None, None))
    rng = np.random.default_rng(23 + sum(map(ord, name)))
    K = rng.standard_normal((N, cols)) + 1j * rng.standard_normal((N, cols))
    K /= np.linalg.norm(K, axis=0)
    c["init"], c["cols"] = ref.operator_to_iso_vec(K), cols
    ns = c["init"].size
    assert ns == 2 * N * cols
    c["vcontrols"] = rng.standard_normal((M0, T0))
    c["vdts"] = 0.1 * rng.standard_normal(T0)
    c["vinit"] = rng.standard_normal(ns) / np.sqrt(ns)
    c["vtheta"] = rng.standard_normal((S, P0))
    c["vscale"] = rng.standard_normal((S, M0))
    c["fid"] = None
    return c


def case(qc, name):
    N, cols, _, _, _ = MANY[name]
    return build_many(qc, name, N, cols)


def frechet(c, samples):
    return jref.pushforward_frechet(c["G0"], c["Gd"], c["Gp"], c["controls"], c["dts"], c["init"], c["theta"], c["scale"], samples,
                                    c["vcontrols"], c["vdts"], c["vinit"], c["vtheta"], c["vscale"], None)


def reference(c):
    key = ("frechet", c["name"], c["S"])
    if key not in _REF:
        _REF[key] = te._frozen(frechet(c, range(c["S"])))
    return _REF[key]


def column(c, k):
    """The case with column k of init and vinit alone: what a `cols = 1` handle is run on."""
    n = c["n"]
    one = dict(c, cols=1, init=np.ascontiguousarray(c["init"][k * n:(k + 1) * n]), vinit=np.ascontiguousarray(c["vinit"][k * n:(k + 1) * n]))
    return one


# ---------------------------------------------------------------------------------------------------------------------------------
#  CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_lds_table():
    """The two LDS formulas restated, each case on the side of 65536 bytes it is named for, and the source lines that compute them: a change
    of either finish kernel's LDS layout fails here and is not silently moved off the edge."""
    for name, (N, cols, wide, jside, fside) in MANY.items():
        ns = 2 * N * cols
        assert ns == NS[name] and ns <= 4096 and (2 * N > 16) == wide and cols > 16, name
        assert side(finish_lds(ns, 32 if wide else 16)) == fside, name
        if not wide:
            assert side(jvp_finish_lds(ns)) == jside, name
    assert jvp_finish_lds(1920) == LDS_OPT_IN == finish_lds(3968, 16) == finish_lds(3584, 32)
    assert jvp_finish_lds(1936) == 66048 and jvp_finish_lds(4096) == 135168 == 132 * 1024
    assert finish_lds(4096, 16) == 67584 and finish_lds(4086, 32) == 73568 and finish_lds(4096, 32) == 73728
    assert jvp_finish_lds(4096) + 128 <= 160 * 1024              # with the static reduction array: inside the 160 KiB of a CU
    assert NS["cols17"] - 256 == 16 and -(-NS["levels3-cols682"] // 256) == 16
    src = lambda f: open(os.path.join(ROOT, "quantumcollocation.jl_amd", "csrc", f)).read()
    jvp, fwd = src("qc_sweep_jvp.hip"), src("qc_sweep.hip")
    assert "const size_t lds = ((size_t)4 * h->ns + 512) * 8;" in jvp and "if (lds > 64 * 1024)" in jvp
    assert "double* Q = sm + 4 * ns;" in jvp and "double* Qd = Q + l2;" in jvp and "constexpr int ld = 16, l2 = 256;" in jvp
    assert "const size_t lds = ((size_t)2 * h->ns + (size_t)F.ld * F.ld) * 8;" in fwd and "if (lds > 64 * 1024)" in fwd
    assert "double* Q = sm + 2 * ns;" in fwd and "constexpr int kFinT = 256;" in fwd and "constexpr int kFinT = 256;" in jvp
    assert "states of more than 4096 entries" in fwd


def test_descriptor_limit_without_a_device(qc):
    L = qc._lib
    val = lambda D: L.lib.qc_sweep_desc_validate(C.byref(D.d))
    msg = lambda: L.lib.qc_sweep_last_error(None).decode()
    assert val(ts._Desc(qc, N=8, cols=256)) == L.QC_OK
    assert val(ts._Desc(qc, N=8, cols=257)) == L.QC_ERR_UNSUPPORTED and "4096 entries" in msg()
    assert val(ts._Desc(qc, N=3, cols=682)) == L.QC_OK
    assert val(ts._Desc(qc, N=3, cols=683)) == L.QC_ERR_UNSUPPORTED and "4096 entries" in msg()
    assert val(tw._wdesc(qc, 1, N=16, cols=128)) == L.QC_OK
    assert val(tw._wdesc(qc, 1, N=16, cols=129)) == L.QC_ERR_UNSUPPORTED and "4096 entries" in msg()
    assert tj._supported(qc, tg._GDesc(qc, N=8, m=2, cols=256))[:2] == (L.QC_OK, 1)
    assert tj._supported(qc, tg._GDesc(qc, N=8, m=2, cols=257))[0] == L.QC_ERR_UNSUPPORTED
    ok = C.c_int32(-1)
    assert L.lib.qc_sweep_desc_vjp_supported(C.byref(tg._GDesc(qc, N=8, m=2, cols=256).d), C.byref(ok)) == L.QC_OK and ok.value == 0
    assert "16 columns" in msg()


def test_reference_routes_agree_at_many_columns(qc):
    """expm_frechet along the recurrence against the complex step through expm on 40 kets of a qutrit: 1e-11 max(1, max |want|), the
    bound of test_sweep_jvp.test_reference_routes_agree."""
    c = build_many(qc, "routes-levels3-cols40", 3, 40, S=2)
    args = (c["G0"], c["Gd"], c["Gp"], c["controls"], c["dts"], c["init"], c["theta"], c["scale"], [0, 1])
    kw = dict(vcontrols=c["vcontrols"], vdts=c["vdts"], vinit=c["vinit"], vtheta=c["vtheta"], vscale=c["vscale"], fid=None)
    a, b = jref.pushforward_frechet(*args, **kw), jref.pushforward_complex_step(*args, **kw)
    assert a["tfinals"].shape == b["tfinals"].shape == (2, 240) and a["tfids"] is None and b["tfids"] is None
    for key in ("finals", "tfinals"):
        err = np.abs(a[key] - b[key]).max() / max(1.0, np.abs(a[key]).max())
        print(f"SWEEP-JVP reference n=6 cols=40 {key}: frechet vs complex step {err:.2e}, max |value| {np.abs(a[key]).max():.3f}")
        assert err <= 1e-11 and np.abs(a[key]).max() > 1e-3, key


def test_launches_and_class_map():
    """S = 3, T = 10: 3 chunks of 3.  S = 37: n_chunks = min(ceil(2048 / 37), 3) = 3, 111 items, 111 % 4 == 3.  The class map at the one
    S that test_sweep_every_sample does not check."""
    f = ts.sweep_launch(16, M0, S0, T0)
    assert (f["chunk"], f["n_chunks"], f["last"]) == (3, 3, 3) and f["by_sqrt"]
    g = ts.sweep_launch(16, M0, S_BIG, T0)
    assert -(-ts.SWEEP_FILL // S_BIG) == 56 and g["n_chunks"] == min(56, 3) == 3 and g["chunk"] == 3
    assert S_BIG * g["n_chunks"] == 111 and 111 % 4 == 3
    assert tw.wide_launch(18, M0, S0, T0) == tw.wide_launch(32, M0, S0, T0) == f
    cls = classes(S_BIG)
    assert cls.shape == (S_BIG,) and cls.min() == 0 and cls.max() == R - 1
    assert cls[:R].tolist() == list(range(R)) and cls[-R:].tolist() == list(range(R))[::-1]
    assert np.bincount(cls, minlength=R).min() >= 2
    np.testing.assert_array_equal(cls, classes(S_BIG))
    assert [int(np.flatnonzero(cls == r)[0]) for r in range(R)] == list(range(R))


# ---------------------------------------------------------------------------------------------------------------------------------
#  GPU
# ---------------------------------------------------------------------------------------------------------------------------------
def run(sw, c):
    """`eval` finals (S x ns) and one `jvp_device` call with finals and tfinals along the full direction (buffers prefilled with -7)."""
    Z = sw.pack(c["controls"], c["dts"])
    finals, fids = sw.eval(Z, c["init"], c["theta"], c["scale"])
    assert fids is None and finals.shape == (sw.ns, c["S"])
    dirs = tj.direction(sw, c)
    assert all(np.all(v != 0) for k, v in dirs.items() if k != "vZ")
    out = tj.device_call(sw, Z, c, tj.outputs_of(sw), dirs)
    assert set(out) == {"finals", "tfinals"}
    return np.ascontiguousarray(finals.T), out


def assert_narrow_scope(sw, c, S):
    want = ts.sweep_launch(c["n"], c["m"], S, c["T"])
    assert sw.kernel_name == "mfma16-sweep" and sw.launch(S) == (True, 3, 3) == (True, want["chunk"], want["n_chunks"])
    assert sw.ns == c["init"].size == c["n"] * c["cols"]
    assert sw.jvp_supported and sw.jvp_unsupported_reason is None
    assert not sw.vjp_supported and "16 columns" in sw.vjp_unsupported_reason
    assert not sw.grad_supported


@pytest.mark.gpu
@pytest.mark.parametrize("name", NARROW)
def test_many_columns_match_the_reference(qc, name):
    c = case(qc, name)
    sw = ts.make_sweep(qc, c)
    try:
        assert_narrow_scope(sw, c, S0)
        assert sw.ns == NS[name] and side(jvp_finish_lds(sw.ns)) == MANY[name][3] and side(finish_lds(sw.ns, 16)) == MANY[name][4]
        finals, out = run(sw, c)
        r = reference(c)
        ts._assert_states(finals, r["finals"], f"SWEEP-MANY {name} eval finals")
        ts._assert_states(out["finals"], r["finals"], f"SWEEP-MANY {name} jvp finals")
        tj.assert_samples(out["tfinals"], r["tfinals"], f"many/{name} tfinals")
        np.testing.assert_array_equal(out["finals"], finals, err_msg="finals of jvp_device against eval")
        finals2, again = run(sw, c)
        np.testing.assert_array_equal(finals2, finals, err_msg="eval, second call")
        for k in out:
            np.testing.assert_array_equal(again[k], out[k], err_msg=k + ", second call")
    finally:
        sw.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", WIDE)
def test_wide_many_columns_match_the_reference(qc, name):
    c = case(qc, name)
    sw = ts.make_sweep(qc, c, wide=True)
    try:
        want = tw.wide_launch(c["n"], c["m"], S0, c["T"])
        assert sw.kernel_name == "mfma32-sweep" and sw.launch(S0) == (True, want["chunk"], want["n_chunks"]) == (True, 3, 3)
        assert sw.ns == NS[name] and side(finish_lds(sw.ns, 32)) == ">"
        assert not sw.jvp_supported and "not served in the mfma32-sweep form" in sw.jvp_unsupported_reason
        assert not sw.vjp_supported and "16 columns" in sw.vjp_unsupported_reason
        Z = sw.pack(c["controls"], c["dts"])
        finals, fids = sw.eval(Z, c["init"], c["theta"], c["scale"])
        again, _ = sw.eval(Z, c["init"], c["theta"], c["scale"])
    finally:
        sw.close()
    rf, _ = ts.reference(c)
    assert fids is None and finals.shape == rf.shape == (NS[name], S0)
    tw._report(name, finals, rf)
    ts._assert_states(finals, rf, f"SWEEP-MANY {name} eval finals")
    np.testing.assert_array_equal(again, finals)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cols256", "levels3-cols682"])
def test_columns_are_independent_bit_for_bit(qc, name):
    """Column k of the many-column finals and tfinals carries the bits of a `cols = 1` handle run on column k alone, with the same Z, rows
    and direction: the sharpest check of idx / n and idx % n across the trips of the strided loops."""
    c = case(qc, name)
    n, cols = c["n"], c["cols"]
    sw = ts.make_sweep(qc, c)
    try:
        finals, out = run(sw, c)
    finally:
        sw.close()
    assert cols - 1 > 42
    for k in (0, 15, 16, 42, cols - 1):
        one = column(c, k)
        sw1 = ts.make_sweep(qc, one)
        try:
            assert sw1.ns == n and sw1.kernel_name == "mfma16-sweep" and sw1.launch(S0) == (True, 3, 3)
            f1, o1 = run(sw1, one)
        finally:
            sw1.close()
        sl = slice(k * n, (k + 1) * n)
        np.testing.assert_array_equal(finals[:, sl], f1, err_msg=f"eval finals, column {k}")
        for key in ("finals", "tfinals"):
            np.testing.assert_array_equal(out[key][:, sl], o1[key], err_msg=f"{key}, column {k}")
        assert np.abs(o1["tfinals"]).max() > 1e-3


@pytest.mark.gpu
def test_lds_opt_in_is_sticky_and_harmless(qc):
    """A small state, the largest one (both finish kernels opt in to more than 64 KiB, for the rest of the process), the small state again
    on its first handle and on a fresh one: the same bits every time."""
    small, big = case(qc, "cols17"), case(qc, "cols256")
    first = ts.make_sweep(qc, small)
    try:
        f0, o0 = run(first, small)
        sw = ts.make_sweep(qc, big)
        try:
            fb, ob = run(sw, big)
        finally:
            sw.close()
        rb = reference(big)
        ts._assert_states(fb, rb["finals"], "SWEEP-MANY cols256 between two cols17: eval finals")
        tj.assert_samples(ob["tfinals"], rb["tfinals"], "many/cols256 between two cols17 tfinals")
        f1, o1 = run(first, small)
    finally:
        first.close()
    fresh = ts.make_sweep(qc, small)
    try:
        f2, o2 = run(fresh, small)
    finally:
        fresh.close()
    for f, o, what in ((f1, o1, "the first handle after the large state"), (f2, o2, "a fresh handle after the large state")):
        np.testing.assert_array_equal(f, f0, err_msg=what)
        for k in o0:
            np.testing.assert_array_equal(o[k], o0[k], err_msg=f"{k}: {what}")
    tj.assert_samples(o0["tfinals"], reference(small)["tfinals"], "many/cols17 before the large state tfinals")


@pytest.mark.gpu
def test_sample_mapping_with_a_big_state(qc):
    """`cols121` at S = 37, R = 8 rows (theta, scale, vtheta, vscale) laid out by `classes`: 111 items, 111 % 4 == 3, three chunks per
    sample; every sample against the reference of its class, the bits of the first sample of its class, the bits of `eval`."""
    N, cols = MANY["cols121"][:2]
    rows = build_many(qc, "cols121-rows", N, cols, S=R)
    cls = classes(S_BIG)
    c = dict(rows, S=S_BIG, cls=cls, samples=list(range(S_BIG)))
    for k in ("theta", "scale", "vtheta", "vscale"):
        c[k] = np.ascontiguousarray(rows[k][cls])
    sw = ts.make_sweep(qc, rows)
    try:
        assert_narrow_scope(sw, c, S_BIG)
        assert sw.launch(S_BIG)[2] * S_BIG == 111 and side(jvp_finish_lds(sw.ns)) == ">"
        finals, out = run(sw, c)
    finally:
        sw.close()
    r = reference(rows)
    every_sample(tj.assert_samples, out["tfinals"], r["tfinals"][cls], cls, "many/cols121 S = 37 tfinals")
    every_sample(ts._assert_states, out["finals"], r["finals"][cls], cls, "SWEEP-MANY cols121 S = 37 finals")
    for k in out:
        assert_class_bits(out[k], cls, f"cols121 S = 37 {k}")
    assert_class_bits(finals, cls, "cols121 S = 37 eval finals")
    np.testing.assert_array_equal(out["finals"], finals)
