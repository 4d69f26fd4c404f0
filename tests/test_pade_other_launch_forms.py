"""The three Pade kernel families that tests/test_pade4_launch_forms.py leaves out, behind a SINGLE handle, at every form their launchers
can start on qc_plan.cpp's default paths: every value of F, dF and mu_d2F against the C restatement of the oracle (oracle/qc_oracle_c.py)
in NaN-filled device buffers between two guard margins, the suite's tolerances as they stand (assert_close: rtol 1e-10, atol 1e-12 x the
largest entry for F and dF; assert_close_h: 1e-11 x for mu_d2F).  The harness is that file's check_case / compare; each case builds its
problem here (Case.problem: oracle_bridge.random_problem / sparse_drive_problem, seed 1, then what the case changes), asserts
qc_kernel_name and the part of the form it was written for, and prints one line: case, kernel names, intervals, form, the worst error of
F / dF / mu_d2F relative to max(1, the largest reference entry).  test_cases_reach_every_form (no GPU) compares what the case lists reach,
by the launch code restated below, with a written-out table; the mutation tests (no GPU) feed defective copies of the oracle's own
vectors through the same compare / assert_close path and require each to be rejected.

Forms by launcher, conditions copied from the launch code, and the ids that reach them.  N = levels (2N rows), nc = state columns.

A. qc_launch_mfma64_F_jac (qc_mfma64_kernels.hip; 32 < 2N <= 64): qc_mfma64_pade4_kernel<JAC>, one 1024-thread workgroup per CU.
   JAC = true: "parts = 1; while (parts < 4 && 2 * parts * n_int <= 256) parts *= 2", grid n_int * parts; workgroup `part` of an interval
   takes the drives part, part + parts, ... ("ml = part < m ? (m - part + parts - 1) / parts : 0") and the copies part, part + parts, ...
   of B / -F; part 0 also the residual, d/dh and the derivative integrators' rows.  JAC = false (F alone): parts = 1, grid n_int, the
   bits of the residuals of F + dF.  Stores are masked below 64 rows / 32 columns (a runtime mask, no instantiation).
       parts 4 (n_int <= 64)       test_mfma64_F_dF[N32-n64] (unmasked, shares 1 1 1 0) [N17-n64] (2 1 1 1; 17 copies dealt 5 4 4 4)
                                   [N24k5-n64] (1 0 0 0) [N20k17-n64] (1 1 0 0) [N32-m6-n64] (2 2 1 1) [N32-n64-shuffled]
       parts 2 (65 .. 128)         [*-n65] [*-n128] of the four systems (2 1 / 3 2 / 1 0 / 1 1), [N32-m0-n65] (no drive in either part),
                                   [N32-n128-fixed]
       parts 1 (129 ..)            [*-n129], [N32-n129-general] (generators that are not antisymmetric)
B. qc_launch_mfma64_hess (qc_mfma64_hess.hip; the plan: "P.m <= kHMax64 (14)", else `lds-gws-hess`): qc_mfma64_pade4_hess_kernel on
   "grid = n_int < 256 ? n_int : 256" workgroups walking b = blockIdx, blockIdx + grid, ..., two scratch sets per workgroup reused from
   trip to trip and from launch to launch; Gram slots N_0 .. N_m-1, M1 | V_0 .. V_m-1, R_h, G D (m = 14: slot 15 in use).
       one trip (256)              test_mfma64_hessian[N32-m1-n256] [N32-m14-n256] [N17-m3-n256] [N20k17-m2-n256]
       workgroup 0 takes two (257) [N32-m1-n257] [N32-m14-n257] [N17-m3-n257] (launched twice) [N20k17-m2-n257] [N32-m2-n257-general]
                                   [N32-m13-n257-fixed]
       three / two (513)           [N32-m1-n513] [N32-m14-n513] [N17-m3-n513] [N20k17-m2-n513] [N32-m2-n513-general]
       m = 14 / 15 at 3 intervals  [N32-m14-n3] (`mfma64-pade4-hess`) [N32-m15-n3] (`lds-gws-hess`); [N32-m14-n3-align16] (hess_align = 16)
   These cases launch mu_d2F and F alone; A's cases launch all three.
C. qc_launch_mfma16_padeP / qc_launch_mfma16_padeP_hess (qc_mfma_padeP.hip, qc_mfma_padeP_hess.hip; order != 4, 2N <= 16, nc <= 8): grid
   n_int, interval qc_xcd_remap(blockIdx, n_int).  mu_d2F: "P.m <= kPHMaxM (8)" and "ph_layout(p, m).total * 8 <= 160 * 1024", else
   `lds-hess`; drive j on wave (j + 2) mod 8 (waves 0 and 1 also run the M_q and the Krylov chain), tp = (p + 1) / 2 tiles per drive.
   The residual-only launch of this family does not promise the bits of F + dF's residuals: both are compared with the oracle.
       m = 1 .. 8 (every wave)     test_any_order[o6-m1] ... [o6-m8] (m = 7, 8: drives 6, 7 on waves 0, 1)
       p = 10 / 1 / 4 / 5 / 6      [o20-m8] (the largest layout, 154 240 bytes) [o2-m8] (tp = 1) [N5-o8-m7] (masked rows) [N3k2-o10-m4]
                                   (masked rows and columns) [o12-m7-fixed]; [o6-m8-general]; [o6-m9]: `lds-hess`
       263 intervals (remainder 7) [o6-m6-n263] [o12-m8-n263];  1030 (more than 1024: past one round; remainder 6) [o6-m6-n1030] [o12-m8-n1030]
D. qc_launch_mfma32_ell_F_jac / _hess / _fused (qc_mfma32_ell.hip; 2N = 32, unitary, antisymmetric generators, 1 <= m <= 8):
   qc_mfma32_ell_kernel<R, JAC, HESS, false, SLOTS> by QC_ELL_LAUNCH, <JAC, HESS> = <true, false> / <false, true> / <true, true>; R (1, 2)
   = the most non-zeros in a drive generator's row, SLOTS (1, 2, 4) = the most drives non-zero at one entry, rounded up
   (qc_mfma32_ell_build; R > 2 or more than 4 drives on an entry: the dense-image kernels).  Inside: "dfast = ft && n_deriv <= 2 &&
   ddim_i <= 64" (else qc_hess_tail), "rows_fast = JAC && n_deriv <= kDF (2) && ddim_i <= 64" (else deriv_rows_generic), h_pad zeros.
       <1, 1> <1, 2> <1, 4> <2, 1> <2, 2> <2, 4>, m = 8      test_row_gather_2N32[R1S1-m8] ... [R2S4-m8] and [R*S*-m8-n263]
       <2, 1> (reached by no other test), m = 1, 2, 5        [R2S1-m1] [R2S1-m2] [R2S1-m5]; past one round: [R2S1-m8-n1030]
       dfast = false                                         [R1S2-m8-n263-fixed] (fixed dt), [R1S1-m8-n263-derivs3] (three integrators:
                                                             rows_fast = false as well), [R2S2-m3-derivs3-align16] (qc_hess_tail's padding)
       h_pad zeros on the fast path                          [R2S2-m8-align16]
       others                                                [R1S4-m8-shuffled] [R2S4-m5-diagdrift] [R2S1-m3-derivs0]
       five drives on one entry                              [diag5]: `mfma32-pade4` / `mfma32-pade4-hess`
   The one call gives dF and mu_d2F of the two launches bit for bit (the file is compiled with contraction off for this promise)."""
import numpy as np
import pytest
import torch

import test_pade4_launch_forms as forms4
from oracle_bridge import random_problem, sparse_drive_problem
from test_gpu_parity import RawHandle, assert_close, assert_close_h
from test_list_launch import GUARD, PATTERN, Guarded
from test_pade4_launch_forms import BIG, check_case, compare, rel_err
from types import SimpleNamespace

TAG = "PADE-OTHER-FORMS"


# ------------------------------------------------------------------------------------------------
#  The launch code, restated
# ------------------------------------------------------------------------------------------------
def jac64_form(n_int, m, with_dF):
    """(parts, grid, drives of each part) of qc_launch_mfma64_F_jac."""
    parts = 1
    if with_dF:
        while parts < 4 and 2 * parts * n_int <= 256:
            parts *= 2
    return parts, n_int * parts, [-(-(m - q) // parts) if q < m else 0 for q in range(parts)]


def copies64(nc, parts):
    """Copies of B / -F that each part of an interval stores ("ncl = part < nc ? (nc - part + step - 1) / step : 0")."""
    return [-(-(nc - q) // parts) if q < nc else 0 for q in range(parts)]


def hess64_form(n_int, m):
    """(kernel name, grid, trips of workgroup 0, trips of the last workgroup) of mu_d2F at 32 < 2N <= 64."""
    if m > 14:
        return "lds-gws-hess", None, None, None
    grid = min(n_int, 256)
    return "mfma64-pade4-hess", grid, -(-n_int // grid), -(-(n_int - (grid - 1)) // grid)


def ph_layout(p, m):
    """qc_mfma_padeP_hess.hip's PHLayout: (doubles in all, tp)."""
    tp = (p + 1) // 2
    return 3 * p * 256 + tp * 256 + max(max(m, 1) * tp, 8) * 256 + 16 + 64, tp


def padeP_hess_waves(m):
    """{wave: drives} of qc_mfma16_padeP_hess_kernel."""
    waves = {}
    for j in range(m):
        waves.setdefault((j + 2) % 8, []).append(j)
    return waves


def padeP_hess_name(p, m):
    return "mfma16-padeP-hess" if m <= 8 and ph_layout(p, m)[0] * 8 <= 160 * 1024 else "lds-hess"


def xcd_remap(b, nb):
    q, r, x, i = nb >> 3, nb & 7, b & 7, b >> 3
    return x * (q + 1) + i if x < r else r * (q + 1) + (x - r) * q + i


def ell_form(G_drives):
    """(R, SLOTS) of qc_mfma32_ell_build for the drive generators (m, 32, 32), or 0: the dense-image kernels."""
    nz = np.asarray(G_drives) != 0.0
    R = int(nz.sum(axis=2).max())
    slots = int(nz.sum(axis=0).max())
    if R < 1 or R > 2 or slots > 4:
        return 0
    return R, 1 if slots <= 1 else 2 if slots <= 2 else 4


def ell_flags(prob):
    """(rows_fast of the JAC instantiations, dfast) of qc_mfma32_ell_kernel."""
    small = len(prob.derivs) <= 2 and all(d.dim <= 64 for d in prob.derivs)
    return small, small and prob.off_dt >= 0


# ------------------------------------------------------------------------------------------------
#  Sparse Hermitian drives at N = 16 with a prescribed (R, SLOTS)
# ------------------------------------------------------------------------------------------------
# A drive is a sum of parts (kind, d): a coupling of every level pair (a, a ^ d) -- the fifteen matchings a -> a ^ d share no pair --
# that is real (generator entries (a, N + b), (N + a, b)), imaginary ((a, b), (N + a, N + b)) or complex (both: two entries per row),
# or a real diagonal ((a, N + a), (N + a, a)).  Parts of different kind or d share no entry of the generator; a real and an imaginary
# part of the same d share their level pairs only.
ELL_FIRST = {1: (("real", 1),), 2: (("complex", 1),)}
ELL_POOL = {1: [(("imag", 1),), (("diag", 0),), (("real", 3),), (("imag", 2),), (("real", 5),), (("imag", 6),), (("real", 7),)],
            2: [(("complex", 2),), (("real", 7), ("imag", 8)), (("diag", 0), ("real", 9)), (("complex", 3),), (("complex", 4),),
                (("real", 5), ("real", 6)), (("complex", 10),)]}


def ell_drive_H(parts, k, N=16):
    H = np.zeros((N, N), dtype=complex)
    for kind, d in parts:
        for a in range(N):
            w = (0.5 + 0.125 * ((5 * k + 3 * a + d) % 8)) * (-1.0 if (a + k) % 3 == 0 else 1.0)
            if kind == "diag":
                H[a, a] += w
            elif a < a ^ d:
                c = w if kind == "real" else 1j * w if kind == "imag" else w * np.exp(1j * (0.3 + 0.11 * k + 0.05 * a))
                H[a, a ^ d] += c
                H[a ^ d, a] += np.conj(c)
    return H


def ell_drives(o, m, R, S, N=16):
    """m drive generators with R entries per row at most; S = 1: no entry shared, 2: two drives on ELL_FIRST's matching, 4: three
    (R = 1: the plan's fourth slot stays empty) or four (R = 2) of them, spread over the drive indices."""
    share = {1: 1, 2: 2, 4: 3 if R == 1 else 4}[S]
    assert share <= m <= share + len(ELL_POOL[R])
    at = {(i * m) // share for i in range(share)}
    rest = iter(ELL_POOL[R])
    return np.array([o.generator(ell_drive_H(ELL_FIRST[R] if k in at else next(rest), k, N)) for k in range(m)]).reshape(m, 2 * N, 2 * N)


# ------------------------------------------------------------------------------------------------
#  The cases
# ------------------------------------------------------------------------------------------------
class Case:
    """fam "m64" / "padeP" / "ell"; N levels, m drives, n_int intervals, ncol kets (0: a unitary); ell = (R, SLOTS) of ell_drives, or
    "diag5"; derivs: how many derivative integrators (None: random_problem's two); align: qc_desc.hess_align."""

    def __init__(self, fam, tag, N, m, n_int, ncol=0, free=True, herm=True, order=4, layout="standard", align=0, derivs=None, ell=None,
                 dense_drift=True, with_dF=True, twice=False):
        self.fam, self.id, self.N, self.m, self.n_int, self.ncol, self.free, self.herm = fam, tag, N, m, n_int, ncol, free, herm
        self.order, self.layout, self.align, self.derivs, self.ell, self.dense_drift = order, layout, align, derivs, ell, dense_drift
        self.with_dF, self.twice = with_dF, twice
        self.nc = ncol or N
        self.p = order // 2
        self._problem, self.form = None, None

    def problem(self, o):
        if self._problem is None:
            T = self.n_int + 1
            if self.fam == "ell":
                kinds = ("diag",) if self.ell == "diag5" else ("real", "imag", "diag")
                prob, Z = sparse_drive_problem(o, m=self.m, T=T, R=1, free_time=self.free, layout=self.layout, seed=1, dense_drift=self.dense_drift, kinds=kinds)
                if self.ell != "diag5":
                    prob.G_drives = ell_drives(o, self.m, *self.ell)
            else:
                prob, Z = random_problem(o, N=self.N, m=max(self.m, 1), T=T, order=self.order, free_time=self.free, hermitian=self.herm,
                                         ncol=self.ncol, layout=self.layout, seed=1)
                if self.m == 0:      # no drives: no derivative integrators either
                    prob.m, prob.G_drives, prob.derivs = 0, prob.G_drives[:0], []
            if self.derivs == 0:
                prob.derivs = []
            elif self.derivs == 3:      # a third integrator on the same components: a(t+1) - a(t) - dt dda(t)
                prob.derivs.append(o.DerivSpec(prob.derivs[0].x_off, prob.derivs[1].dx_off, self.m))
            prob.hess_align = self.align or 1
            self._problem = prob, Z
        return self._problem

    def names(self):
        if self.fam == "m64":
            return "mfma64-pade4", hess64_form(self.n_int, self.m)[0], "two-launches"
        if self.fam == "padeP":
            return "mfma16-padeP", padeP_hess_name(self.p, self.m), "two-launches"
        if self.form:
            return "mfma32-pade4-ell", "mfma32-pade4-hess-ell", "mfma32-pade4-fused-ell"
        return "mfma32-pade4", "mfma32-pade4-hess", "two-launches"

    def set_form(self, o):
        """The row-gather family's form follows from the generators: (R, SLOTS) or 0."""
        self.form = ell_form(self.problem(o)[0].G_drives) if self.fam == "ell" else None
        return self.form


def make(qc, oracle, case):
    prob, Z = case.problem(oracle)
    case.set_form(oracle)
    h = RawHandle(qc, prob, hess_align=case.align)
    desc = SimpleNamespace(integrator=0, N=prob.N, state_cols=case.ncol, off_dt=prob.off_dt, hess_offset=0, m=prob.m)

    def close():      # (the case lists live as long as the session: the trajectory does not)
        h.close()
        case._problem = None
    return prob, Z, h.h, h.dims, SimpleNamespace(_desc=desc, dims=h.dims), close


def form_text(case):
    if case.fam == "m64":
        parts, grid, shares = jac64_form(case.n_int, case.m, True)
        name, hgrid, t0, tl = hess64_form(case.n_int, case.m)
        jac = f"F + dF on {grid} workgroups, {parts} per interval, drives {shares}, copies {copies64(case.nc, parts)}; " if case.with_dF else ""
        return f"{jac}F alone on {case.n_int}; mu_d2F " + (f"on {hgrid} workgroups, trips {t0} / {tl}" if hgrid else "by the global-workspace kernel")
    if case.fam == "padeP":
        return (f"p = {case.p}, LDS {ph_layout(case.p, case.m)[0] * 8} bytes, drives by wave {padeP_hess_waves(case.m)}, "
                f"remap remainder {case.n_int & 7}, {'past' if case.n_int > 1024 else 'within'} one round")
    if not case.form:
        return "the dense-image kernels: more than four drives on one entry"
    rows_fast, dfast = ell_flags(case.problem(None)[0])
    return f"<R, SLOTS> = {case.form}, rows_fast {rows_fast}, dfast {dfast}, hess_align {case.align}, remap remainder {case.n_int & 7}"


def ids(cases):
    return [c.id for c in cases]


def m64(tag, N, m, n_int, **kw):
    return Case("m64", tag, N, m, n_int, **kw)


JAC64_COUNTS = {64: 4, 65: 2, 128: 2, 129: 1}                     # intervals: parts
JAC64_SYSTEMS = {"N32": (32, 0, 3), "N17": (17, 0, 5), "N24k5": (24, 5, 1), "N20k17": (20, 17, 2)}      # N, kets, drives
JAC64 = ([m64(f"{s}-n{n}", N, m, n, ncol=k) for s, (N, k, m) in JAC64_SYSTEMS.items() for n in JAC64_COUNTS] +
         [m64("N32-m0-n65", 32, 0, 65), m64("N32-m6-n64", 32, 6, 64), m64("N32-n128-fixed", 32, 2, 128, free=False),
          m64("N32-n129-general", 32, 2, 129, herm=False), m64("N32-n64-shuffled", 32, 3, 64, layout="shuffled")])
HESS64_COUNTS = {256: (1, 1), 257: (2, 1), 513: (3, 2)}           # intervals: trips of workgroup 0, of the last workgroup
HESS64 = ([m64(f"N32-m1-n{n}", 32, 1, n, with_dF=False) for n in HESS64_COUNTS] +
          [m64(f"N32-m14-n{n}", 32, 14, n, with_dF=False) for n in HESS64_COUNTS] +      # (513: 31.6 M values, compared in slices)
          [m64(f"N17-m3-n{n}", 17, 3, n, with_dF=False, twice=n == 257) for n in HESS64_COUNTS] +
          [m64(f"N20k17-m2-n{n}", 20, 2, n, ncol=17, with_dF=False) for n in HESS64_COUNTS] +
          [m64(f"N32-m2-n{n}-general", 32, 2, n, herm=False, with_dF=False) for n in (257, 513)] +
          [m64("N32-m13-n257-fixed", 32, 13, 257, free=False, with_dF=False)])
HESS64_SHORT = [m64("N32-m14-n3", 32, 14, 3, with_dF=False), m64("N32-m15-n3", 32, 15, 3, with_dF=False),
                m64("N32-m14-n3-align16", 32, 14, 3, align=16, with_dF=False)]


def padeP(tag, N, m, order, n_int=5, **kw):
    return Case("padeP", tag, N, m, n_int, order=order, **kw)


PADEP = ([padeP(f"o6-m{m}", 8, m, 6) for m in range(1, 9)] +
         [padeP("o20-m8", 8, 8, 20), padeP("o2-m8", 8, 8, 2), padeP("N5-o8-m7", 5, 7, 8), padeP("N3k2-o10-m4", 3, 4, 10, ncol=2),
          padeP("o6-m8-general", 8, 8, 6, herm=False), padeP("o12-m7-fixed", 8, 7, 12, free=False), padeP("o6-m9", 8, 9, 6)] +
         [padeP(f"o{o}-m{m}-n{n}", 8, m, o, n_int=n) for n in (263, 1030) for o, m in ((6, 6), (12, 8))])


def ell(tag, m, n_int=5, form=None, **kw):
    return Case("ell", tag, 16, m, n_int, ell=form, **kw)


ELL_FORMS = [(R, S) for R in (1, 2) for S in (1, 2, 4)]
ELL = ([ell(f"R{R}S{S}-m8", 8, form=(R, S)) for R, S in ELL_FORMS] + [ell(f"R2S1-m{m}", m, form=(2, 1)) for m in (1, 2, 5)] +
       [ell(f"R{R}S{S}-m8-n263", 8, 263, form=(R, S)) for R, S in ELL_FORMS] + [ell("R2S1-m8-n1030", 8, 1030, form=(2, 1))] +
       [ell("R1S2-m8-n263-fixed", 8, 263, form=(1, 2), free=False), ell("R1S1-m8-n263-derivs3", 8, 263, form=(1, 1), derivs=3),
        ell("R2S2-m3-derivs3-align16", 3, form=(2, 2), derivs=3, align=16), ell("R2S2-m8-align16", 8, form=(2, 2), align=16),
        ell("R1S4-m8-shuffled", 8, form=(1, 4), layout="shuffled"), ell("R2S4-m5-diagdrift", 5, form=(2, 4), dense_drift=False),
        ell("R2S1-m3-derivs0", 3, form=(2, 1), derivs=0)])
ELL_DENSE = [ell("diag5", 5, form="diag5")]
EVERY_CASE = JAC64 + HESS64 + HESS64_SHORT + PADEP + ELL + ELL_DENSE


# ------------------------------------------------------------------------------------------------
#  Without a GPU: the table, the restated rules at their edges, the checker against defective vectors
# ------------------------------------------------------------------------------------------------
def test_cases_reach_every_form(oracle):
    """What the case lists reach, by the restated launch code, against the forms of the module docstring written out."""
    assert len({c.id for c in EVERY_CASE}) == len(EVERY_CASE)
    # A: parts x masked, and per number of parts the drives a part can hold: none, one, two or more (one part: all m >= 1 of them)
    jac, held = set(), {1: set(), 2: set(), 4: set()}
    for c in JAC64:
        parts, grid, shares = jac64_form(c.n_int, c.m, True)
        assert c.with_dF and sum(shares) == c.m and sum(copies64(c.nc, parts)) == c.nc and jac64_form(c.n_int, c.m, False)[:2] == (1, c.n_int)
        jac.add((parts, c.N != 32 or c.nc != 32))
        held[parts] |= {min(k, 2) for k in shares}
    assert jac == {(parts, masked) for parts in (1, 2, 4) for masked in (False, True)}, jac
    assert held == {1: {1, 2}, 2: {0, 1, 2}, 4: {0, 1, 2}}, held
    assert {(c.free, c.herm, c.layout) for c in JAC64} >= {(False, True, "standard"), (True, False, "standard"), (True, True, "shuffled")}
    # B: trips, the drive cap, masks, the padded layout, a second launch
    hess = {}
    for c in HESS64 + HESS64_SHORT:
        assert not c.with_dF
        name, grid, t0, tl = hess64_form(c.n_int, c.m)
        assert c.names()[1] == name == ("lds-gws-hess" if c.m > 14 else "mfma64-pade4-hess")
        if c.m <= 14:
            hess.setdefault((t0, tl), set()).add((c.m, c.N != 32 or c.nc != 32, c.herm, c.free))
    assert set(hess) == {(1, 1), (2, 1), (3, 2)}
    assert {m for m, *_ in hess[(2, 1)]} >= {1, 13, 14} and {c.m for c in HESS64_SHORT} == {14, 15}
    for trips in ((2, 1), (3, 2)):
        assert {(masked, herm) for _, masked, herm, _ in hess[trips]} >= {(False, True), (True, True), (False, False)}, trips
    assert any(not free for *_, free in hess[(2, 1)]) and any(c.align == 16 and c.m == 14 for c in HESS64_SHORT)
    assert [c.id for c in HESS64 if c.twice] == ["N17-m3-n257"]
    # C: every wave assignment, every p of the kernel's callers, masks, one round and more, a remainder in the remap
    on_kernel = [c for c in PADEP if c.names()[1] == "mfma16-padeP-hess"]
    assert {c.m for c in on_kernel if c.n_int == 5} == set(range(1, 9)) and {c.p for c in on_kernel} == {1, 3, 4, 5, 6, 10}
    assert [c.id for c in PADEP if c not in on_kernel] == ["o6-m9"]
    assert all(ph_layout(c.p, c.m)[0] * 8 <= 160 * 1024 for c in on_kernel) and max(ph_layout(c.p, c.m)[0] * 8 for c in on_kernel) == 154240
    assert {(c.N, c.nc) for c in on_kernel} >= {(8, 8), (5, 5), (3, 2)} and {(c.herm, c.free) for c in on_kernel} == {(True, True), (False, True), (True, False)}
    assert {(c.p, c.m, c.n_int & 7, c.n_int > 1024) for c in on_kernel if c.n_int > 5} == {(p, m, r, over) for p, m in ((3, 6), (6, 8)) for r, over in ((7, False), (6, True))}
    # D: the 18 instantiations, both values of rows_fast and dfast with many intervals, the padding on both paths
    inst, flags, pads = set(), set(), set()
    for c in ELL:
        assert c.set_form(oracle) == c.ell, (c.id, c.form)
        assert np.array_equal(c.problem(oracle)[0].G_drives, -np.transpose(c.problem(oracle)[0].G_drives, (0, 2, 1)))
        inst |= {(*c.form, entry) for entry in ("F_jac", "hess", "fused")}
        rows_fast, dfast = ell_flags(c.problem(oracle)[0])
        flags |= {("rows_fast", rows_fast, c.n_int > 5), ("dfast", dfast, c.n_int > 5)}
        pads.add((c.align, dfast))
    assert inst == {(R, S, e) for R in (1, 2) for S in (1, 2, 4) for e in ("F_jac", "hess", "fused")} and len(inst) == 18
    assert flags == {(f, v, long) for f in ("rows_fast", "dfast") for v in (True, False) for long in (True, False)}, flags
    assert pads == {(0, True), (0, False), (16, True), (16, False)}
    for n in (5, 263, 1030):
        assert {c.form for c in ELL if c.n_int == n} >= ({(2, 1)} if n == 1030 else set(ELL_FORMS))
    assert {c.m for c in ELL if c.form == (2, 1) and c.n_int == 5} >= {1, 2, 5, 8}
    assert ELL_DENSE[0].set_form(oracle) == 0 and ELL_DENSE[0].names()[:2] == ("mfma32-pade4", "mfma32-pade4-hess")


def test_restated_rules_at_their_edges(oracle):
    assert [jac64_form(n, 3, True)[:2] for n in (1, 64, 65, 128, 129)] == [(4, 4), (4, 256), (2, 130), (2, 256), (1, 129)]
    assert [jac64_form(n, 3, False)[:2] for n in (64, 129)] == [(1, 64), (1, 129)]
    assert jac64_form(64, 6, True)[2] == [2, 2, 1, 1] and jac64_form(64, 1, True)[2] == [1, 0, 0, 0] and jac64_form(65, 0, True)[2] == [0, 0]
    assert copies64(17, 4) == [5, 4, 4, 4] and copies64(5, 4) == [2, 1, 1, 1] and copies64(32, 2) == [16, 16]
    assert [hess64_form(n, 14)[1:] for n in (3, 256, 257, 513)] == [(3, 1, 1), (256, 1, 1), (256, 2, 1), (256, 3, 2)]
    assert hess64_form(3, 14)[0] == "mfma64-pade4-hess" and hess64_form(3, 15) == ("lds-gws-hess", None, None, None)
    # PHLayout: 3 p + tp tiles, then max(8, m tp) (the eight partial sums of G share the A block), 16 coefficients, the 8 x 8 sums
    assert ph_layout(10, 8) == (19280, 5) and ph_layout(1, 8) == (3152, 1) and ph_layout(3, 1) == (4944, 2) and ph_layout(3, 0) == ph_layout(3, 4)
    assert ph_layout(10, 8)[0] * 8 == 154240 <= 160 * 1024 < ph_layout(10, 9)[0] * 8
    assert padeP_hess_name(3, 8) == "mfma16-padeP-hess" and padeP_hess_name(3, 9) == "lds-hess"
    assert padeP_hess_waves(8) == {2: [0], 3: [1], 4: [2], 5: [3], 6: [4], 7: [5], 0: [6], 1: [7]} and padeP_hess_waves(1) == {2: [0]}
    for nb in (5, 263, 1030):
        assert sorted(xcd_remap(b, nb) for b in range(nb)) == list(range(nb))
    assert (263 & 7, 1030 & 7) == (7, 6) and xcd_remap(8, 263) == 1 and xcd_remap(1, 263) == 33 and xcd_remap(7, 263) == 231
    # qc_mfma32_ell_build's counting, on the generator of this file and beside it
    for R, S in ELL_FORMS:
        assert ell_form(ell_drives(oracle, 8, R, S)) == (R, S)
    G = ell_drives(oracle, 8, 1, 1)
    assert int((G != 0).sum(axis=0).max()) == 1 and ell_form(ell_drives(oracle, 8, 1, 4)) == (1, 4) and int((ell_drives(oracle, 8, 1, 4) != 0).sum(axis=0).max()) == 3
    G[3][0, :5] = 1.0
    assert ell_form(G) == 0                                   # more than two entries in a row
    assert ell_form(np.array([G[2]] * 5)) == 0 and ell_form(np.array([G[2]] * 4)) == (1, 4)


class HostVector(Guarded):
    """test_list_launch.Guarded's vector in host memory, holding `values`: what compare() reads after a launch."""

    def __init__(self, values):
        self.n = int(values.size)
        self.all = torch.empty(self.n + 2 * GUARD, dtype=torch.float64)
        self.all.view(torch.int64).fill_(PATTERN)
        self.t = self.all[GUARD:GUARD + self.n]
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(values)))


MUTATION_CASES = [m64("mutation-N17k3-m2-n257", 17, 2, 257, ncol=3), padeP("mutation-o6-m3", 8, 3, 6), ell("mutation-R2S1-m2", 2, form=(2, 1))]


@pytest.mark.parametrize("big", [BIG, 1 << 12], ids=["whole", "slices"])
@pytest.mark.parametrize("case", MUTATION_CASES, ids=ids(MUTATION_CASES))
def test_the_checker_rejects_defective_vectors(oracle, coracle, monkeypatch, case, big):
    """The C oracle's own dF and mu_d2F of one small case per family pass compare() with the suite's tolerances (whole, and in slices of
    intervals as vectors beyond BIG are read); each of these defects does not: one value off by 2e-10 x the largest entry; the blocks of
    two drives swapped (dF: d/da_0 and d/da_1; mu_d2F: (a_0, U_t+1) and (a_1, U_t+1)); the copies of B / -F that a second workgroup of the
    interval stores left at the NaN prefill; an interval holding the values of the one its workgroup computed before (interval 256 of 257
    those of interval 0; elsewhere the last those of the one before)."""
    monkeypatch.setattr(torch.cuda, "synchronize", lambda: None)
    monkeypatch.setattr(forms4, "BIG", big)
    prob, Z = case.problem(oracle)
    ref = coracle.COracle(prob)
    n_int, n, s, nc, m = case.n_int, prob.n, prob.s, prob.nc, prob.m
    mu = np.random.default_rng(5).standard_normal(prob.n_rows)
    refs = {"dF": (lambda a, b: ref.F_dF(Z, a, b, False, True)[1], assert_close), "mu_d2F": (lambda a, b: ref.mu_d2F(Z, mu, a, b), assert_close_h)}

    def check(which, V):
        return compare(HostVector(V.reshape(-1)), n_int, *refs[which], f"{case.id}: {which}")[0]

    stale = (n_int - 1, 0) if n_int == 257 else (n_int - 1, n_int - 2)
    caught = []
    for which in refs:
        good = refs[which][0](0, n_int).reshape(n_int, -1)
        assert check(which, good) == 0.0
        a0 = 2 * nc * n * n if which == "dF" else m * s           # dF: [-F copies | B copies | d/da_j | d/dh | ...]; mu_d2F: [(U_t, a_j) | (a_j, U_t+1) | ...]
        defects = {"one value off": lambda V: V.__setitem__((n_int // 2, a0 + 5), V[n_int // 2, a0 + 5] + 2e-10 * np.abs(good).max()),
                   "two drives' blocks swapped": lambda V: V.__setitem__((slice(None), slice(a0, a0 + 2 * s)), np.roll(V[:, a0:a0 + 2 * s], s, axis=1)),
                   "a stale interval": lambda V: V.__setitem__(stale[0], V[stale[1]])}
        if which == "dF":
            defects["every second copy of B / -F not written"] = lambda V: [V.__setitem__((slice(None), slice(o + q * n * n, o + (q + 1) * n * n)), np.nan)
                                                                       for o in (0, nc * n * n) for q in range(1, nc, 2)]
        for name, apply in defects.items():
            V = good.copy()
            apply(V)
            assert not np.array_equal(V, good, equal_nan=True) and (name != "one value off" or 0.0 < rel_err(V, good) < 3e-10), (which, name)
            with pytest.raises(AssertionError):
                check(which, V)
            caught.append(f"{which}: {name}")
    print(f"{TAG} {case.id} ({'whole vectors' if big == BIG else 'slices of intervals'}): rejected -- {'; '.join(caught)}")


# ------------------------------------------------------------------------------------------------
#  A. F + dF and F alone at 32 < 2N <= 64
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", JAC64, ids=ids(JAC64))
def test_mfma64_F_dF(qc, oracle, coracle, case):
    """64 / 65 / 128 / 129 intervals: the last count with four workgroups per interval, the first and the last with two, the first with
    one; 32 levels, 17 (one live row in the second row tile, 17 copies), 5 kets of 24 levels (one column tile, parts without a drive)
    and 17 kets of 20 levels (one live column in the second column tile)."""
    parts, grid, shares = jac64_form(case.n_int, case.m, True)
    assert parts == (4 if case.n_int <= 64 else 2 if case.n_int <= 128 else 1) and grid == parts * case.n_int and grid <= 256
    assert len(shares) == parts and sum(shares) == case.m and max(shares) - min(shares) <= 1
    check_case(qc, oracle, coracle, case, make=make, form=form_text, tag=TAG)


# ------------------------------------------------------------------------------------------------
#  B. mu_d2F at 32 < 2N <= 64
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", HESS64, ids=ids(HESS64))
def test_mfma64_hessian(qc, oracle, coracle, case):
    """256 intervals: one trip of the 256 workgroups; 257: workgroup 0 walks on to a second interval, into the scratch sets of its
    first; 513: three trips of workgroup 0, two of the others.  One case launches twice on its handle: the same bits."""
    name, grid, t0, tl = hess64_form(case.n_int, case.m)
    assert (name, grid) == ("mfma64-pade4-hess", 256) and (t0, tl) == HESS64_COUNTS[case.n_int]
    check_case(qc, oracle, coracle, case, make=make, with_dF=False, twice=case.twice, form=form_text, tag=TAG)


@pytest.mark.gpu
@pytest.mark.parametrize("case", HESS64_SHORT, ids=ids(HESS64_SHORT))
def test_mfma64_hessian_drive_cap(qc, oracle, coracle, case):
    """14 drives fill the 16 Gram slots (N_0 .. N_13, M1 | V_0 .. V_13, R_h, G D), also with the value blocks padded to whole lines;
    15 go to the global-workspace kernel."""
    assert case.names()[1] == ("mfma64-pade4-hess" if case.m <= 14 else "lds-gws-hess")
    check_case(qc, oracle, coracle, case, make=make, with_dF=False, form=form_text, tag=TAG)


# ------------------------------------------------------------------------------------------------
#  C. Any order but 4 at 2N <= 16
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", PADEP, ids=ids(PADEP))
def test_any_order(qc, oracle, coracle, case):
    """One to eight drives (drive j on wave (j + 2) mod 8: seven and eight put a drive on the waves of the M_q and the Krylov chain),
    p = 1 .. 10 with the largest LDS layout, masked rows and columns, 263 intervals (a remainder of 7 in qc_xcd_remap) and 1030 (past
    one round of the device); nine drives: the LDS Hessian kernel."""
    waves = padeP_hess_waves(case.m)
    assert sorted(j for w in waves.values() for j in w) == list(range(case.m)) and all(w == (js[0] + 2) % 8 for w, js in waves.items())
    if case.m <= 8:
        assert max(len(js) for js in waves.values()) == 1 and ph_layout(case.p, case.m)[0] * 8 <= 160 * 1024
        assert (0 in waves, 1 in waves) == (case.m >= 7, case.m >= 8)
    assert case.names()[1] == ("mfma16-padeP-hess" if case.m <= 8 else "lds-hess")
    check_case(qc, oracle, coracle, case, make=make, F_bits=False, form=form_text, tag=TAG)


# ------------------------------------------------------------------------------------------------
#  D. Sparse drive generators at 2N = 32
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", ELL + ELL_DENSE, ids=ids(ELL + ELL_DENSE))
def test_row_gather_2N32(qc, oracle, coracle, case):
    """The six <R, SLOTS> instantiations of each entry point (F + dF and F alone, mu_d2F, all three in one call) at 5 and 263 intervals
    and one past a round, with the generic derivative-integrator and padding branches; the one call: dF and mu_d2F of the two launches
    bit for bit.  Five drives on one entry: the dense-image kernels."""
    form = case.set_form(oracle)
    assert form == (0 if case.ell == "diag5" else case.ell)
    assert case.names()[2] == ("mfma32-pade4-fused-ell" if form else "two-launches")
    check_case(qc, oracle, coracle, case, make=make, one_call_bits=True, form=form_text, tag=TAG)
