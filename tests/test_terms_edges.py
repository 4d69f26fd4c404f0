"""Trajectory-term kernels (qc_terms.hip, terms_knot<EXT> and qc_terms_sum_kernel) past one wave of entries and of pairs: knots of
more than 64 entries, pair lists of more than 64 pairs, adjacency lists up to the hub's degree, a timestep at entry 0, at a multiple
of 64, last and absent, min_time_knots in {0, 1, T-1, T}, every (cross, cross_p) combination, global tails on both sides of 256 and
knot counts on both sides of 256 and past 1024.  Handles are made from raw descriptors (CASES); every output number is compared with
the long-double term-by-term reference (terms_slow_reference.py).

Tolerance.  For every output number, |kernel - slow| <= k 2^-52 A, where A is the sum of the absolute values of the terms that make
the number up (the reference returns it) and k counts the roundings on the longest path from an input to that number: a term's own
roundings plus every later addition it takes part in.  A difference that is squared counts twice.  Fused multiply-adds only remove
roundings, and the build does not reassociate.  Counted in qc_terms.hip, with nz = ceil(zdim / 64), np = ceil(n_pair / 64),
nT = ceil(T / 256):

  gradient entry j != off_dt (entry loop, lines 83-126)                                       k = max(7, deg(j) + 4)
      regulariser part: dv (88), w sc, sc, dv (89) = 4; then g += gs (109), the fma with the pair part (118), g += lw (121): 7
      smoothness part: x - z_prev, w (103) or dn (105), w dn (106); gs -= (106); then 109, 118, 121: 6
      pair part: x - z_partner, then one fma per partner (117): 1 + deg; sc sc and the fma (118), 121: deg + 4
  timestep entry of the gradient (lines 90, 130, 144-150, 155 / 159)                           k = max(nz, np) + 12
      q: dv twice (it is squared), w dv, nz fmas (90), 6 shuffle additions (150), q + qp, its product with dt, + mt (155): nz + 12; qp alike (129-130, 145)
  Hessian, single products                                                                     k = 2: R sc^2 (93), Q sc^2 (133)
                                                                                               k = 3: 2 dt R dv (94), 2 dt Q d (138-139)
                                                                                               k = 0: S (1 or 2) and -S (112-113), exact
  Hessian, (dt, dt) values q (161) and qp (156)                                                k = nz + 9 and np + 9
  J (lines 154 / 158, then qc_terms_sum_kernel, 177-188)                   k = max(max(nz, np) + 22, 2 nz + 19) + nT
      q reduced: nz + 9; q + qp, sc sc, the product, + r, + mt dt (154): + 5; the strided sum (180): nT; the tree (183-186): 8
      r: dn twice, w dn, up to two fmas per pass (107, 122): 2 nz + 3; 6 shuffles (146); + r, + mt dt: 2 nz + 11; then nT + 8
No count exceeds 40 (the largest is 30: J of the 289-entry knot of the Python-layer case; 29 for J of long-1030).  These are at most the counts deg(j) + 8, nz + np + 12 and
nz + np + nT + 22 that suffice by a coarser reading.  Numbers with A = 0 must be exactly +0.0.

Share of the reference itself: the float64 restatement (terms_ext_reference.py) agrees with the long-double reference within
4 2^-52 A on every case (asserted below; the largest measured |f64 - slow| / (2^-52 A) is 0.9 for J, 2.4 for a gradient entry and
2.1 for a Hessian value), and the long-double sums themselves are good to about 2^-63 A per addition.

GPU, measured on an MI355X: the largest err / bound over all cases is 0.035 for J (plain-z131-dt64), 0.26 for a gradient entry
(long-1030) and 0.48 for a Hessian value (count-513; the single products, k = 2 and 3).  The 24 GPU tests take 3.2 s together, loading the library included.

The mutation tests feed the same checker outputs built from the reference with one defect each (a lane sum that keeps its last
addend, a block stored modulo 64, a short adjacency walk, ...) and assert which cases reject them."""
import ctypes as C
import functools
import math
import types

import numpy as np
import pytest

import terms_ext_reference as ref
import terms_slow_reference as slow_ref
from test_terms_ext import ext_struct

U = 2.0 ** -52
GUARD = 64


# ------------------------------------------------------------------------------------------------------------ the table
def _spec(T, zdim, off_dt, n_reg, n_smooth, n_pair, hub, n_lin, gd, scaled=True, baseline=False, n_mt=0, ext=True, hub_entry=None,
          lin_has=None):
    return types.SimpleNamespace(T=T, zdim=zdim, off_dt=off_dt, n_reg=n_reg, n_smooth=n_smooth, n_pair=n_pair, hub=hub, n_lin=n_lin,
                                 gd=gd, scaled=scaled, baseline=baseline, n_mt=n_mt, ext=ext, hub_entry=hub_entry, lin_has=lin_has)


COUNT_T = (1, 2, 3, 4, 255, 256, 257, 513)
SPECS = {
    "z64-p64": _spec(5, 64, 63, 40, 40, 64, 3, 5, 0, n_mt=4),
    "z65-p65": _spec(5, 65, 0, 64, 64, 65, 3, 3, 0, baseline=True, n_mt=5, hub_entry=64, lin_has=64),
    "z131-p130": _spec(7, 131, 64, 70, 66, 130, 5, 65, 257, baseline=True, n_mt=6),
    "z129-fixed-plain": _spec(6, 129, -1, 128, 100, 64, 5, 0, 256, scaled=False),
    "z129-fixed-scaled": _spec(6, 129, -1, 128, 100, 64, 5, 7, 255, baseline=True),
    "z130-free-plain": _spec(6, 130, 129, 60, 60, 70, 4, 10, 1, scaled=False, n_mt=1),
    "pair-only": _spec(3, 70, 33, 0, 0, 66, 4, 0, 0, n_mt=2),
    "reg-only-ext": _spec(3, 70, 33, 66, 5, 0, 0, 0, 0, n_mt=2),
    "lin-only": _spec(4, 80, 79, 0, 0, 0, 0, 70, 3, n_mt=3),
    "smooth-only-T1": _spec(1, 66, -1, 0, 66, 0, 0, 0, 0),
    "smooth-only-T2": _spec(2, 66, -1, 0, 66, 0, 0, 0, 0),
    "plain-z131-dt0": _spec(6, 131, 0, 130, 0, 0, 0, 0, 600, baseline=True, n_mt=0, ext=False),
    "plain-z131-dt64": _spec(6, 131, 64, 130, 0, 0, 0, 0, 600, baseline=True, n_mt=6, ext=False),
    "long-1030": _spec(1030, 66, 65, 20, 10, 9, 4, 4, 600, baseline=True, n_mt=1030),
}
for _i, _T in enumerate(COUNT_T):                       # n_mt cycles through 0, 1, T - 1, T
    SPECS[f"count-{_T}"] = _spec(_T, 66, 65, 20, 10, 9, 4, 4, 0, n_mt=(0, 1, _T - 1, _T)[_i % 4])
NAMES = list(SPECS)


@functools.lru_cache(maxsize=None)
def case(name):
    """The case `name`: description (the restatement's TermsExt), Z, and the counts the bounds need.  Drawn from a generator seeded
    by the name; the result is shared between tests and never modified."""
    sp = SPECS[name]
    rng = np.random.default_rng(list(name.encode()))
    T, zdim, off = sp.T, sp.zdim, sp.off_dt
    others = np.array([j for j in range(zdim) if j != off])
    reg_index = np.sort(rng.choice(others, sp.n_reg, replace=False))
    s_index = rng.choice(others, sp.n_smooth, replace=False)
    l_index = rng.choice(others, sp.n_lin, replace=False)
    if sp.lin_has is not None and sp.lin_has not in l_index:
        l_index[0] = sp.lin_has
    pa, pb = [], []
    hub = None
    if sp.n_pair:
        hub = int(sp.hub_entry if sp.hub_entry is not None else rng.choice(others))
        rest = others[others != hub]
        for i, b in enumerate(rng.choice(rest, sp.hub, replace=False)):      # the hub alternates as pair_a and pair_b
            pa.append(hub if i % 2 == 0 else int(b))
            pb.append(int(b) if i % 2 == 0 else hub)
        a, b = (int(v) for v in rng.choice(rest, 2, replace=False))           # one pair twice (two Q) and once reversed
        pa += [a, a, b]
        pb += [b, b, a]
        for _ in range(sp.n_pair - sp.hub - 3):
            a, b = (int(v) for v in rng.choice(rest, 2, replace=False))
            pa.append(a)
            pb.append(b)
        order = rng.permutation(sp.n_pair)                                    # the hub's and the repeated pairs land in any pass
        pa, pb = np.array(pa)[order], np.array(pb)[order]
    free = off >= 0
    Z = rng.standard_normal(T * zdim + sp.gd)
    if free:
        Z[off:T * zdim:zdim] = rng.uniform(0.1, 0.3, T)
    tm = ref.TermsExt(T=T, zdim=zdim, off_dt=off, dt_fixed=0.0 if free else float(rng.uniform(0.1, 0.3)), global_dim=sp.gd,
                      dt_scaled=sp.scaled, reg_index=reg_index, reg_R=rng.uniform(0.5, 2.0, sp.n_reg),
                      baseline=rng.standard_normal((T, sp.n_reg)) if sp.baseline and sp.n_reg else None,
                      D=float(rng.uniform(0.5, 2.0)) if free else 0.0, n_mt=sp.n_mt if free else 0,
                      s_index=s_index, s_R=rng.uniform(0.5, 3.0, sp.n_smooth), p_a=ref._i(pa), p_b=ref._i(pb),
                      p_Q=rng.uniform(0.5, 100.0, sp.n_pair), l_index=l_index, l_w=rng.uniform(0.05, 0.2, sp.n_lin))
    return finish_case(name, tm, Z, sp.ext, hub)


def finish_case(name, tm, Z, ext=True, hub=None):
    deg = np.zeros(tm.zdim, dtype=np.int64)
    np.add.at(deg, tm.p_a, 1)
    np.add.at(deg, tm.p_b, 1)
    return types.SimpleNamespace(name=name, tm=tm, Z=Z, ext=ext, hub=hub, deg=deg, nz=-(-tm.zdim // 64), np_=-(-len(tm.p_a) // 64),
                                 nT=-(-tm.T // 256), n=Z.size)


@functools.lru_cache(maxsize=None)
def slow(name):
    c = case(name)
    return slow_ref.evaluate(c.tm, c.Z)


def layout(tm):
    """Value offsets of the library's COO order: values per knot of the prefix, start of the smoothness block, start and values per
    knot of the pairwise block, total."""
    nr, ns, npr = len(tm.reg_index), len(tm.s_index), len(tm.p_a)
    per_knot = nr * (1 + tm.cross) + tm.cross
    hs_base = tm.T * per_knot
    hp_base = hs_base + ns * (2 * tm.T - 1)
    hp_knot = 3 * npr + tm.cross_p * (2 * npr + 1)
    return types.SimpleNamespace(per_knot=per_knot, hs_base=hs_base, hp_base=hp_base, hp_knot=hp_knot, nnz=hp_base + tm.T * hp_knot)


def smooth_block(tm, t):
    """[start, stop) of knot t's values inside the smoothness block."""
    ns = len(tm.s_index)
    lo = layout(tm).hs_base + 2 * ns * t
    return lo, lo + ns * (2 if t + 1 < tm.T else 1)


# ------------------------------------------------------------------------------------------------------- bounds and checker
def k_values(c):
    """(k of J, k per gradient entry, k per Hessian value), from the counts in the module docstring."""
    tm = c.tm
    kJ = max(max(c.nz, c.np_) + 22, 2 * c.nz + 19) + c.nT
    kg = np.zeros(c.n)
    row = np.maximum(7, c.deg + 4).astype(np.float64)
    if tm.off_dt >= 0:
        row[tm.off_dt] = max(c.nz, c.np_) + 12
    kg[:tm.T * tm.zdim] = np.tile(row, tm.T)
    lay = layout(tm)
    nr, npr = len(tm.reg_index), len(tm.p_a)
    kH = np.zeros(lay.nnz)                                    # the smoothness block stays 0: its values are exact
    pre = np.concatenate([np.full(nr, 2.0), np.full(nr, 3.0), [c.nz + 9.0]])[:lay.per_knot]
    kH[:lay.hs_base] = np.tile(pre, tm.T)
    pair = np.concatenate([np.full(3 * npr, 2.0), np.full(2 * npr, 3.0), [c.np_ + 9.0]])[:lay.hp_knot]
    kH[lay.hp_base:] = np.tile(pair, tm.T)
    return kJ, kg, kH


def _ratios(got, want, A, k, what):
    """err / bound per number; a number with A = 0 must be +0.0; anything else outside k 2^-52 A (NaN included) is a failure."""
    got = np.atleast_1d(np.asarray(got, dtype=np.float64))
    want, A = np.atleast_1d(want), np.atleast_1d(A)
    assert got.shape == want.shape == A.shape, f"{what}: {got.shape} values, expected {want.shape}"
    err = np.abs(got.astype(slow_ref.L) - want)
    bound = np.broadcast_to(np.asarray(k, dtype=slow_ref.L), A.shape) * slow_ref.L(U) * A
    zero = A == 0
    bad0 = zero & ((got != 0.0) | np.signbit(got))
    assert not bad0.any(), f"{what}: {bad0.sum()} numbers without terms are not +0.0, first at {np.nonzero(bad0)[0][0]}: {got[bad0][0]!r}"
    bad = ~(err <= bound)
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        raise AssertionError(f"{what}: {bad.sum()} numbers outside k 2^-52 A, first at {i}: got {got[i]!r}, expected {float(want[i])!r}, "
                             f"err {float(err[i]):.3e}, bound {float(bound[i]):.3e}")
    pos = bound > 0
    return float(np.max(err[pos] / bound[pos])) if pos.any() else 0.0


def check_outputs(c, s, J=None, g=None, H=None):
    """Every given output against the slow reference `s` within the derived bound; returns the largest err / bound per output."""
    kJ, kg, kH = k_values(c)
    out = {}
    if J is not None:
        out["J"] = _ratios(J, s.J, s.A_J, kJ, f"{c.name}: J")
    if g is not None:
        g = np.asarray(g)
        assert g.shape == (c.n,), f"{c.name}: gradient of length {g.shape}"
        nk = c.tm.T * c.tm.zdim
        out["grad"] = _ratios(g, s.g, s.A_g, kg, f"{c.name}: gradient")
        tail = g[nk:]
        assert tail.tobytes() == np.zeros(c.n - nk).tobytes(), f"{c.name}: gradient tail is not all +0.0"
    if H is not None:
        out["hess"] = _ratios(H, s.H, s.A_H, kH, f"{c.name}: Hessian values")
    return out


def report(name, what, r):
    print(f"[terms-edges] {name} {what}: largest err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))


def f64(s):
    """The reference's numbers rounded to double: what a correct kernel may return at best."""
    return float(s.J), s.g.astype(np.float64), s.H.astype(np.float64)


# -------------------------------------------------------------------------------------------------------------------- CPU
def test_table_reaches_every_form():
    cs = [case(n) for n in NAMES]
    ext = [c for c in cs if c.ext]
    assert {1, 2, 3} <= {c.nz for c in ext} and {1, 2, 3} <= {c.np_ for c in ext if len(c.tm.p_a)}
    assert {c.nz for c in cs if not c.ext} == {3}
    assert max(int(c.deg.max()) for c in ext) >= 5
    assert all(c.deg[c.hub] == SPECS[c.name].hub for c in ext if c.hub is not None)
    offs = {("none" if c.tm.off_dt < 0 else "first" if c.tm.off_dt == 0 else "last" if c.tm.off_dt == c.tm.zdim - 1 else
             "mult64" if c.tm.off_dt % 64 == 0 else "other") for c in ext}
    assert {"none", "first", "mult64", "last"} <= offs
    assert {(bool(c.tm.cross), bool(c.tm.cross_p)) for c in ext} == {(False, False), (False, True), (True, False), (True, True)}
    assert {(c.tm.dt_scaled, c.tm.free) for c in ext} == {(True, True), (True, False), (False, True), (False, False)}
    gds = {c.tm.global_dim for c in cs}
    assert {0, 1, 255, 256, 257, 600} <= gds
    assert {c.tm.T % 4 for c in ext} == {0, 1, 2, 3}
    Ts = {c.tm.T for c in ext}
    assert {255, 256, 257} <= Ts and max(Ts) > 1024
    kinds = set()
    for c in cs:
        if c.tm.free:
            kinds |= {k for k, v in (("0", 0), ("1", 1), ("T-1", c.tm.T - 1), ("T", c.tm.T)) if c.tm.n_mt == v and c.tm.T > 2}
    assert kinds == {"0", "1", "T-1", "T"}
    assert {c.tm.n_mt for c in cs if not c.ext and c.tm.free} == {0, 6}
    z65 = case("z65-p65")
    assert 64 in z65.tm.reg_index and 64 in z65.tm.s_index and 64 in z65.tm.l_index and z65.deg[64] >= 1
    assert all(c.tm.baseline is not None for c in cs if SPECS[c.name].baseline)
    # the repeated pair: twice in one direction, once reversed
    for c in ext:
        if len(c.tm.p_a):
            prs = list(zip(c.tm.p_a.tolist(), c.tm.p_b.tolist()))
            assert any(prs.count(p) >= 2 and prs.count(p[::-1]) >= 1 for p in prs), c.name
    k_all = [np.max(np.concatenate([[kJ], kg, kH])) for kJ, kg, kH in (k_values(c) for c in cs)]
    assert max(k_all) <= 40


@pytest.mark.parametrize("name", NAMES)
def test_structure_equals_the_slow_reference(qc, name):
    """qc_terms_desc_ext_hess_nnz / _structure (no device) against the slow reference's structure, entry for entry."""
    L = qc._lib
    c, s = case(name), slow(name)
    keep = []
    d, x = ext_struct(qc, c.tm, keep, baseline=True)
    nnz = C.c_int64(-1)
    assert L.lib.qc_terms_desc_ext_hess_nnz(C.byref(d), C.byref(x), C.byref(nnz)) == 0, L.lib.qc_terms_last_error(None)
    assert nnz.value == s.H.size == layout(c.tm).nnz
    r = np.full(nnz.value + 1, -7, dtype=np.int64)
    cc = np.full(nnz.value + 1, -7, dtype=np.int64)
    assert L.lib.qc_terms_desc_ext_hess_structure(C.byref(d), C.byref(x), L.iptr(r), L.iptr(cc), 0) == 0
    np.testing.assert_array_equal(r[:-1], s.rows)
    np.testing.assert_array_equal(cc[:-1], s.cols)
    assert r[-1] == -7 and cc[-1] == -7 and np.all(s.rows <= s.cols)
    if not c.ext:
        assert L.lib.qc_terms_desc_hess_nnz(C.byref(d), C.byref(nnz)) == 0 and nnz.value == s.H.size


@pytest.mark.parametrize("name", NAMES)
def test_float64_restatement_agrees_with_the_slow_reference(name):
    """The reference's own share of the bound: terms_ext_reference.py in float64 within 4 2^-52 A of the long-double loops."""
    c, s = case(name), slow(name)
    r = {"J": _ratios(ref.value(c.tm, c.Z), s.J, s.A_J, 4, f"{name}: J of the restatement"),
         "grad": _ratios(ref.grad(c.tm, c.Z), s.g, s.A_g, 4, f"{name}: gradient of the restatement"),
         "hess": _ratios(ref.hess_values(c.tm, c.Z), s.H, s.A_H, 4, f"{name}: Hessian values of the restatement")}
    report(name, "float64 restatement, in units of 4 2^-52 A", r)
    np.testing.assert_array_equal(ref.hess_structure(c.tm)[0], s.rows)
    np.testing.assert_array_equal(ref.hess_structure(c.tm)[1], s.cols)


SMALL = [n for n in NAMES if SPECS[n].T * SPECS[n].zdim + SPECS[n].gd <= 330]


@pytest.mark.parametrize("name", SMALL)
def test_slow_hessian_is_the_derivative_of_the_slow_gradient(name):
    """The COO values summed into a dense matrix (upper triangle mirrored) equal a central difference of the slow gradient, which
    is symmetric to the same tolerance."""
    c, s = case(name), slow(name)
    assert np.all(s.rows <= s.cols)
    Hd = slow_ref.dense_hessian(s, c.n)
    assert np.array_equal(Hd, Hd.T)
    h = slow_ref.L(1e-6)
    Z = np.asarray(c.Z, dtype=slow_ref.L)
    Hfd = np.zeros((c.n, c.n), dtype=slow_ref.L)
    for i in range(c.n):
        e = np.zeros(c.n, dtype=slow_ref.L)
        e[i] = h
        Hfd[i] = (slow_ref.evaluate(c.tm, Z + e, want_hess=False).g - slow_ref.evaluate(c.tm, Z - e, want_hess=False).g) / (2 * h)
    scale = max(1.0, float(np.max(np.abs(Hd))))
    assert float(np.max(np.abs(Hfd - Hfd.T))) <= 1e-7 * scale
    assert float(np.max(np.abs(Hd - Hfd))) <= 1e-7 * scale


def test_slow_reference_known_answers():
    """One term of each kind, by hand."""
    tm = ref.TermsExt(T=2, zdim=3, off_dt=2, reg_index=ref._i([0]), reg_R=ref._f([2.0]), D=3.0, n_mt=1, s_index=ref._i([1]),
                      s_R=ref._f([4.0]), p_a=ref._i([0]), p_b=ref._i([1]), p_Q=ref._f([8.0]), l_index=ref._i([1]), l_w=ref._f([0.5]))
    Z = np.array([1.0, 2.0, 0.5, 3.0, -1.0, 0.25])
    s = slow_ref.evaluate(tm, Z)
    # knot 0: reg 1/2 .25 2 1 = .25, mt 1.5, pair 1/2 .25 8 1 = 1, lin 1; knot 1: reg 1/2 .0625 2 9 = .5625, pair 1/2 .0625 8 16 = 4,
    # lin -.5; smoothness 1/2 4 9 = 18
    assert float(s.J) == 0.25 + 1.5 + 1.0 + 1.0 + 0.5625 + 4.0 - 0.5 + 18.0
    assert float(s.A_J) == 0.25 + 1.5 + 1.0 + 1.0 + 0.5625 + 4.0 + 0.5 + 18.0
    # d/dx_0[1]: smoothness -4 (-3) = 12, pair -(8 .25 (-1)) = 2, lin .5
    assert float(s.g[1]) == 14.5 and float(s.A_g[1]) == 14.5
    # d/ddt_0: dt (2 1 + 8 1) + D = 8
    assert float(s.g[2]) == 8.0
    assert s.H.size == 2 * 3 + 3 + 2 * 6 == ref.hess_nnz(tm)


# ---- the checks can fail: outputs built from the reference with one defect each
def _passes(c, s, J, g, H):
    check_outputs(c, s, J, g, H)
    return True


def _rejects(c, s, J, g, H, what):
    with pytest.raises(AssertionError, match=what):
        check_outputs(c, s, J, g, H)
    return True


def test_unmodified_reference_outputs_pass():
    for name in NAMES:
        c, s = case(name), slow(name)
        r = check_outputs(c, s, *f64(s))
        assert max(r.values()) <= 0.25, name          # rounding to double alone: 2^-53 A, and no k below 2 where A > 0 is inexact


def test_mutation_regulariser_part_from_entry_j_minus_64():
    def mutate(name):
        c, s = case(name), slow(name)
        J, g, H = f64(s)
        zd = c.tm.zdim
        for t in range(c.tm.T):
            gr = s.detail["g_reg"][t]
            for j in range(64, zd):
                if j != c.tm.off_dt:
                    g[t * zd + j] = float(s.g[t * zd + j] - gr.get(j, 0) + gr.get(j - 64, 0))
        return c, s, J, g, H
    assert _passes(*mutate("z64-p64"))
    for name in ("z65-p65", "z131-p130", "z129-fixed-plain", "plain-z131-dt0"):
        assert _rejects(*mutate(name), "gradient")


def _q_last_addend(c, adds):
    """The lane sum if every lane kept only its last addend: (index, value) pairs walked in strides of 64."""
    last = {}
    for i, v in sorted(adds, key=lambda iv: iv[0]):
        last[i % 64] = v
    return sum(last.values(), slow_ref.L(0))


def test_mutation_q_from_each_lanes_last_addend():
    def mutate(name):
        c, s = case(name), slow(name)
        J, g, H = f64(s)
        tm, lay = c.tm, layout(c.tm)
        Jm = s.J
        for t in range(tm.T):
            adds = s.detail["q_add"][t]
            drop = sum((v for _, v in adds), slow_ref.L(0)) - _q_last_addend(c, adds)
            Jm = Jm - s.detail["sc"][t] ** 2 * drop / 2
            if tm.free and tm.dt_scaled:
                i = t * tm.zdim + tm.off_dt
                g[i] = float(s.g[i] - s.detail["dt"][t] * drop)
            if tm.cross:
                e = t * lay.per_knot + 2 * len(tm.reg_index)
                H[e] = float(s.H[e] - drop)
        return c, s, float(Jm), g, H
    assert _passes(*mutate("z64-p64")) and _passes(*mutate("z65-p65"))      # no lane has a second addend there
    c, s, J, g, H = mutate("z131-p130")
    assert _rejects(c, s, J, None, None, "J") and _rejects(c, s, None, g, None, "gradient") and _rejects(c, s, None, None, H, "Hessian")
    c, s, J, g, H = mutate("z129-fixed-plain")
    assert _rejects(c, s, J, None, None, "J") and _passes(c, s, None, g, H)  # no timestep entry and no (dt, dt) value there
    c, s, J, g, H = mutate("plain-z131-dt64")
    assert _rejects(c, s, J, None, None, "J") and _rejects(c, s, None, g, None, "gradient") and _rejects(c, s, None, None, H, "Hessian")


def test_mutation_pair_blocks_taken_from_pair_p_minus_64():
    def mutate(name):
        c, s = case(name), slow(name)
        J, g, H = f64(s)
        tm, lay = c.tm, layout(c.tm)
        npr = len(tm.p_a)
        for t in range(tm.T):
            for blk in range(5 if tm.cross_p else 3):
                b0 = lay.hp_base + t * lay.hp_knot + blk * npr
                for p in range(64, npr):
                    H[b0 + p] = float(s.H[b0 + p - 64])
        return c, s, J, g, H
    for name in ("z64-p64", "z129-fixed-plain"):
        assert _passes(*mutate(name))
    for name in ("z65-p65", "z131-p130", "z130-free-plain", "pair-only"):
        assert _rejects(*mutate(name), "Hessian")


def test_mutation_hub_gradient_from_its_first_two_partners():
    def mutate(name):
        c, s = case(name), slow(name)
        J, g, H = f64(s)
        for t in range(c.tm.T):
            i = t * c.tm.zdim + c.hub
            g[i] = float(s.g[i] - sum(s.detail["g_pair"][t][c.hub][2:], slow_ref.L(0)))
        return c, s, J, g, H
    for name in ("z64-p64", "z65-p65", "z131-p130", "z129-fixed-scaled", "pair-only", "count-3"):
        assert _rejects(*mutate(name), "gradient")


def test_mutation_tail_entry_256_left_nan():
    for name in ("z131-p130", "plain-z131-dt0", "long-1030"):
        c, s = case(name), slow(name)
        J, g, H = f64(s)
        g[c.tm.T * c.tm.zdim + 256] = np.nan
        assert _rejects(c, s, J, g, H, "gradient")
    assert case("z129-fixed-plain").tm.global_dim == 256                     # the tail that ends one short of it


def test_mutation_timestep_entry_overwritten_by_the_entry_loop():
    """The entry loop's value at the timestep is 0.0: no regulariser, smoothness, pair or slack may sit on that entry."""
    for name in ("z64-p64", "z65-p65", "z131-p130", "z130-free-plain", "plain-z131-dt0", "plain-z131-dt64", "lin-only"):
        c, s = case(name), slow(name)
        J, g, H = f64(s)
        g[c.tm.off_dt:c.tm.T * c.tm.zdim:c.tm.zdim] = 0.0
        assert _rejects(c, s, J, g, H, "gradient")
    # in z130-free-plain the timestep entry is the minimum-time weight of knot 0 alone
    c, s = case("z130-free-plain"), slow("z130-free-plain")
    col = s.g[c.tm.off_dt:c.tm.T * c.tm.zdim:c.tm.zdim].astype(np.float64)
    assert col[0] == c.tm.D and np.all(col[1:] == 0.0)


def test_mutation_part_256_dropped_from_J():
    for name in ("long-1030", "count-257", "count-513"):
        c, s = case(name), slow(name)
        assert _rejects(c, s, float(s.J - s.detail["part"][256]), None, None, "J")
    assert case("count-256").tm.T == 256


# -------------------------------------------------------------------------------------------------------------------- GPU
def make_handle(qc, c, keep):
    L = qc._lib
    d, x = ext_struct(qc, c.tm, keep, baseline=True)
    h = C.c_void_p()
    rc = L.lib.qc_terms_create_ext(C.byref(d), C.byref(x), C.byref(h)) if c.ext else L.lib.qc_terms_create(C.byref(d), C.byref(h))
    assert rc == 0, L.lib.qc_terms_last_error(None)
    nnz = C.c_int64(-1)
    assert L.lib.qc_terms_hess_nnz(h, C.byref(nnz)) == 0 and nnz.value == layout(c.tm).nnz
    return h


def eval_dev(qc, h, c, grad=True, hess=True):
    """qc_terms_eval_dev into NaN-filled device buffers with a guard tail; (J, g, H) as host arrays with their guards."""
    import torch
    nan = lambda n: torch.full((n + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    dZ = torch.from_numpy(c.Z).cuda()
    dJ, dg, dH = nan(1), nan(c.n) if grad else None, nan(layout(c.tm).nnz) if hess else None
    rc = qc._lib.lib.qc_terms_eval_dev(h, dZ.data_ptr(), dJ.data_ptr(), dg.data_ptr() if grad else None, dH.data_ptr() if hess else None,
                                       torch.cuda.current_stream().cuda_stream)
    assert rc == 0, qc._lib.lib.qc_terms_last_error(h)
    torch.cuda.synchronize()
    return tuple(None if v is None else v.cpu().numpy() for v in (dJ, dg, dH))


def split_guard(c, J, g, H):
    """Strip the guard tails, which must still be NaN."""
    nnz = layout(c.tm).nnz
    out = []
    for v, n, what in ((J, 1, "J"), (g, c.n, "gradient"), (H, nnz, "Hessian")):
        if v is None:
            out.append(None)
            continue
        assert v.size == n + GUARD and np.isnan(v[n:]).all(), f"{c.name}: the guard behind {what} was written"
        out.append(v[:n])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_kernel_meets_the_derived_bound(qc, name):
    L = qc._lib
    c, s = case(name), slow(name)
    nnz = layout(c.tm).nnz
    keep = []
    h = make_handle(qc, c, keep)
    try:
        J, g, H = split_guard(c, *eval_dev(qc, h, c))
        report(name, "qc_terms_eval_dev", check_outputs(c, s, J[0], g, H))        # NaN left in range fails the bound
        if name == "lin-only":
            assert nnz == 0 and H.size == 0                                        # the Hessian pointer was not NULL: untouched
        if name == "smooth-only-T1":
            assert J[0] == 0.0 and not g.any() and not H.any()
        # a second call, the host entry and the calls without gradient and / or Hessian: the same bits
        J2, g2, H2 = split_guard(c, *eval_dev(qc, h, c))
        assert J2.tobytes() == J.tobytes() and g2.tobytes() == g.tobytes() and H2.tobytes() == H.tobytes()
        hJ = C.c_double(float("nan"))
        hg, hH = np.full(c.n + GUARD, np.nan), np.full(nnz + GUARD, np.nan)
        assert L.lib.qc_terms_eval(h, L.dptr(c.Z), C.byref(hJ), L.dptr(hg), L.dptr(hH)) == 0, L.lib.qc_terms_last_error(h)
        _, g3, H3 = split_guard(c, None, hg, hH)
        assert np.float64(hJ.value).tobytes() == J.tobytes() and g3.tobytes() == g.tobytes() and H3.tobytes() == H.tobytes()
        for grad, hess in ((False, True), (True, False), (False, False)):
            Jn, gn, Hn = split_guard(c, *eval_dev(qc, h, c, grad=grad, hess=hess))
            assert Jn.tobytes() == J.tobytes(), (name, grad, hess)
            assert gn is None or gn.tobytes() == g.tobytes(), (name, grad, hess)
            assert Hn is None or Hn.tobytes() == H.tobytes(), (name, grad, hess)
    finally:
        L.lib.qc_terms_destroy(h)


@pytest.mark.gpu
def test_knot_values_do_not_depend_on_the_wave_slot(qc):
    """A handle over knots 1 .. T-1 of z131-p130 (same arrays, baseline rows shifted): knot t sits in another wave of its workgroup,
    and the gradient rows and per-knot Hessian blocks of the knots interior in both handles are the full handle's bit for bit."""
    c = case("z131-p130")
    tm, zd = c.tm, c.tm.zdim
    sub_tm = ref.TermsExt(**{**tm.__dict__, "T": tm.T - 1, "baseline": tm.baseline[1:], "n_mt": tm.n_mt - 1})
    sub = finish_case("z131-p130-from-knot-1", sub_tm, np.ascontiguousarray(c.Z[zd:]))
    keep = []
    outs = []
    for cc in (c, sub):
        h = make_handle(qc, cc, keep)
        try:
            outs.append(split_guard(cc, *eval_dev(qc, h, cc)))
        finally:
            qc._lib.lib.qc_terms_destroy(h)
    report(sub.name, "qc_terms_eval_dev", check_outputs(sub, slow_ref.evaluate(sub.tm, sub.Z), outs[1][0][0], outs[1][1], outs[1][2]))
    (_, g, H), (_, gs, Hs) = outs
    lay, lays = layout(tm), layout(sub_tm)
    assert lay.per_knot == lays.per_knot and lay.hp_knot == lays.hp_knot
    for t in range(2, tm.T - 1):                                 # interior in both: knot t of the full handle is knot t - 1 of the other
        assert g[t * zd:(t + 1) * zd].tobytes() == gs[(t - 1) * zd:t * zd].tobytes(), t
        assert H[t * lay.per_knot:(t + 1) * lay.per_knot].tobytes() == Hs[(t - 1) * lay.per_knot:t * lay.per_knot].tobytes(), t
        (a, b), (a2, b2) = smooth_block(tm, t), smooth_block(sub_tm, t - 1)
        assert b - a == b2 - a2 == 2 * len(tm.s_index) and H[a:b].tobytes() == Hs[a2:b2].tobytes(), t
        a, a2 = lay.hp_base + t * lay.hp_knot, lays.hp_base + (t - 1) * lay.hp_knot
        assert H[a:a + lay.hp_knot].tobytes() == Hs[a2:a2 + lay.hp_knot].tobytes(), t


@pytest.mark.gpu
def test_python_layer_past_one_wave(qc):
    """TrajectoryObjective over a 289-entry knot (u, v: 70; w: 5; a: 3; two slack components of 70; a free timestep in the middle)
    against the slow reference built from the raw offsets."""
    rng = np.random.default_rng(list(b"python-layer"))
    T = 5
    comps = {"u": rng.standard_normal((70, T)), "v": rng.standard_normal((70, T)), "Δt": rng.uniform(0.1, 0.3, (1, T)),
             "w": rng.standard_normal((5, T)), "a": rng.standard_normal((3, T)), "s1_u": rng.standard_normal((70, T)),
             "s2_u": rng.standard_normal((70, T))}
    traj = qc.NamedTrajectory(comps, controls=("a", "s1_u", "s2_u"), timestep="Δt", global_data={"g": rng.standard_normal(4)})
    Ra, Ru, Su, Q, w = rng.uniform(0.5, 2.0, 3), rng.uniform(0.5, 2.0, 70), rng.uniform(0.5, 3.0, 70), rng.uniform(0.5, 100.0), rng.uniform(0.05, 0.2, 70)
    base = rng.standard_normal((3, T))
    spec = (qc.QuadraticRegularizer("a", traj, Ra, baseline=base) + qc.QuadraticRegularizer("u", traj, Ru)
            + qc.QuadraticSmoothnessRegularizer("u", traj, Su) + qc.PairwiseQuadraticRegularizer(traj, Q, [("u", "v")])
            + qc.L1Regularizer("u", traj, w))
    cp = {k: np.asarray(v) for k, v in traj.components.items()}
    reg = np.concatenate([cp["u"], cp["a"]])                                   # u lies before a: already increasing
    assert np.all(np.diff(reg) > 0)
    bl = np.zeros((T, 73))
    bl[:, 70:] = base.T
    tm = ref.TermsExt(T=T, zdim=traj.dim, off_dt=traj.offset("Δt"), dt_fixed=0.0, global_dim=4, dt_scaled=True, reg_index=reg,
                      reg_R=np.concatenate([Ru, Ra]), baseline=bl, D=0.0, n_mt=0, s_index=cp["u"], s_R=Su, p_a=cp["u"], p_b=cp["v"],
                      p_Q=np.full(70, Q), l_index=np.concatenate([cp["s1_u"], cp["s2_u"]]), l_w=np.concatenate([w, w]))
    assert tm.zdim == 289 and tm.off_dt == 140
    c = finish_case("python-layer", tm, traj.datavec)
    s = slow_ref.evaluate(tm, c.Z)
    obj = qc.TrajectoryObjective(spec, traj)
    try:
        assert obj.has_ext and obj.hess_nnz == s.H.size
        np.testing.assert_array_equal(obj.hess_structure[0], s.rows)
        np.testing.assert_array_equal(obj.hess_structure[1], s.cols)
        J, g, H = obj.L_grad_hess(c.Z)
        report(c.name, "TrajectoryObjective.L_grad_hess", check_outputs(c, s, J, g, H))
    finally:
        obj.close()
