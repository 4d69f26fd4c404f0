"""The order-4 Pade kernels up to 2N = 32 behind a SINGLE handle, at every form their launchers can start: every value of F, dF and
mu_d2F against the C restatement of the oracle (oracle/qc_oracle_c.py), the suite's tolerances as they stand (rtol 1e-10, atol 1e-12 x
the largest entry for F and dF, 1e-11 x for mu_d2F).  tests/test_list_launch.py does the same for the batched launchers.

Every case builds a random dense problem (oracle_bridge.random_problem, seed 1; the row-gather child: the host layer's three-qubit
Pauli system), opens a handle through the raw descriptor, asserts qc_kernel_name, launches qc_eval_F_jac_dev (with dF, then with
dvals = NULL: F alone, which must give the bits of the F of F + dF), qc_eval_hess_dev and -- where qc_kernel_name(h, 2) names a
one-call kernel -- qc_eval_F_jac_hess_dev (against the two launches: assert_same_hessian_values) into NaN-filled device buffers between
two guard margins (test_list_launch.Guarded): every value inside finite, both margins untouched.  Jacobian value arrays beyond 2^24
doubles stay on the device and are compared in slices of intervals (the C oracle's t_begin / t_end), with the atol of each slice taken
from the slice's own largest entry: never looser than the suite's.  Which instantiation a case reaches follows from the launch code,
restated by jac16_form / hess16_form / jac32_form / hess32_form below; every test asserts the part of the form it was written for, and
test_cases_reach_every_instantiation compares what the case lists reach with the instantiations written out here.  Each test prints
one line: case, kernel names, forms, intervals, the worst error of F / dF / mu_d2F relative to max(1, the largest reference entry).

Instantiations by launcher, conditions copied from the launch code, and the ids that reach them.  N = levels (2N rows), nc = state
columns (N for a unitary), masked tile (KET) = "nc != 8 || n != 16" at 2N <= 16 and "nc != 16 || n != 32" at 2N = 32, kMU / HM = the next
even number >= m, at least 2, at most 8.  Left out everywhere: the diagnostic builds (QC_STAMPS, QC_DEBUG_SKIP: DIAG = true and the
stamped instantiations; QC_STORE_MODE 0 / 1: MODE != 2; QC_FUSED_VARIANT).

1. qc_launch_mfma16_F_jac (qc_mfma_kernels.hip): qc_mfma16_pade4_kernel<JAC, 2, false, kMU, KET, false, ONCE, HEAD>.
   n_wg = n_int; grid = n_wg < kMaxGrid (1024) ? n_wg : kMaxGrid; JAC = (dJ != NULL); ONCE = (grid == n_wg).
   persistent (ONCE = false: more than 1024 intervals), JAC = true and false (every case launches both):
       unmasked kMU 2 / 4 / 6 / 8:  test_F_dF_persistent[N8-m2-n1025] [N8-m3-n1025] [N8-m6-n1025] [N8-m7-n1025]
       masked   kMU 2 / 4 / 6 / 8:  test_F_dF_persistent[N5-m1-n1025] [N5-m4-n1025] [N5-m5-n1025] [N5-m8-n1025]; by kets: [N8k3-m4-n1025]
       the loop over drives beyond the hand-off block (m > 8), both arms of `k + 2 <= m`: [N8-m9-n1025] (one drive left: the arm
       that repeats image k + 1) and [N8-m10-n1025] (a full pair); a third trip [N8-m6-n2050]; [N8-m4-n1025-fixed]; [N8-m6-n1025-general]
   loop-free (ONCE = true), masked kMU 2 / 4 / 6 / 8: the one-wave child's [N3-m1] [N3-m4] [N3-m5] [N3-m8] (both JAC)
   loop-free, unmasked: the one-wave child's [N8-m1] [N8-m4] [N8-m5] [N8-m8], Hermitian and general, and test_hand_over[m2 / m4 / m6];
       with JAC = true launch16m takes HEAD = true where "P.head && P.dbg_skip == 0 && P.m == MU && P.copies == 8 && P.copies >=
       QC_EARLY_COPIES && P.dwin_n > 0 && P.off_dt >= 0 && dF != nullptr && P.antisym" (the Hermitian cases with even m), ONCE alone
       otherwise (odd m, the general cases); the library has no query for it, the two are one entry of the table below.
2. qc_launch_mfma16_hess (qc_mfma_hess.hip), the one-wave kernels.  window = "P.antisym && P.m > 4 && P.m <= 6 && P.n_int > 1536 &&
   P.n_int <= 2048 && !gather"; grid = (n_int <= once_max && !window) ? n_int : min(n_int, grid_cap); once = (grid == n_int);
   grid_cap = 1024 and once_max = 2^30 unless QC_HESS_GRID / QC_HESS_ONCE_MAX say otherwise (read once per process).
   qc_mfma16_pade4_hess_anti_kernel<HM, KET, false, ONCE> (P.antisym):
       persistent, by the window (HM = 6 only): unmasked test_window[N8-m5-n1537] [N8-m5-n2048] [N8-m6-n1537] [N8-m6-n2048]
           [N8-m6-n1537-fixed], masked [N5-m5-n1537] [N5-m5-n2048] [N5-m6-n1537] [N5-m6-n2048]; n1536 and n2049 of each: loop-free
       persistent, HM 2 / 4 / 6 / 8 x unmasked / masked (reachable with QC_HESS_ONCE_MAX / QC_HESS_GRID only):
           test_one_wave_persistent_forms_in_a_child, cases [N8-m1] [N8-m4] [N8-m5] [N8-m8] and [N3-m1] [N3-m4] [N3-m5] [N3-m8]
       loop-free unmasked HM 2 / 4 / 6: test_hand_over[m2-n1025] [m4-n1025] [m6-n1025]; HM 8: test_F_dF_persistent[N8-m7-n1025]
       loop-free masked HM 2 / 4 / 6 / 8: test_F_dF_persistent[N5-m1-n1025] [N5-m4-n1025] [N5-m5-n1025] [N5-m8-n1025]
   <HM, false, false, true, false, true> (row gathers: `once && gather`, HM <= 6; the plan passes gather = true only under QC_HESS_G2=0,
       the name stays "mfma16-pade4-hess-gather" -- by default that name is qc_mfma_hess_g2.hip):
       test_row_gather_form_in_a_child, cases [pauli-m1] [pauli-m2] (HM 2), [pauli-m3] [pauli-m4] (4), [pauli-m5] [pauli-m6]
       [pauli-m6-n1025] (6)
   qc_mfma16_pade4_hess_kernel<HM, KET, false, ONCE> (general generators):
       persistent, all eight: the one-wave child's [N8-m*-general] and [N3-m*-general]
       loop-free, all eight: test_general_one_wave_loop_free[N8-m1] ... [N3-m8]; test_F_dF_persistent[N8-m6-n1025-general]
3. qc_launch_mfma16_hess2 (qc_mfma_hess2.hip; the plan: "sw.hess_two_waves && P.n_int <= kTwoWavesMaxIntervals (1024) &&
   qc_mfma16_hess2_supported"): qc_mfma16_pade4_hess2_kernel<2 / 4 / 6, false>: test_hand_over[m2-n1024] [m4-n1024] [m6-n1024]; one
   interval more, [m*-n1025], is the one-wave kernel.
4. qc_launch_mfma32_F_jac (qc_mfma32_kernels.hip): qc_mfma32_pade4_kernel<JAC, false, KET, SINGLE, ONCE>.  n_wg = (n_int + 1) / 2;
   once = n_wg <= kMaxGrid32 (1024); SINGLE: "dJ && !diag && P.n_int <= 256" (<true, false, KET, true, true>, grid n_int).
       SINGLE            unmasked test_dense_image_F_dF[N16-n256]; masked [N11-n256] [N16k5-n256]
       pair, loop-free   JAC = true: [N16-n257] [N16-n2048]; [N11-n257] [N11-n2048] [N16k5-n257] [N16k5-n2048]
                         JAC = false: the same and the n256 cases (F alone never takes SINGLE)
       pair, persistent  JAC = true and false: [N16-n2049]; [N11-n2049] [N11-n2049-fixed] [N16k5-n2049] (1025 pairs: the second trip
                         of workgroup 0 holds interval 2048 and an empty slot)
5. qc_launch_mfma32_hess (qc_mfma32_hess.hip): qc_mfma32_pade4_hess_kernel<false, ANTI, FULL>.  per_wg = ceil(n_int / kHCUs (256));
   grid = ceil(n_int / per_wg).
       <false, true, true>  "P.antisym && P.n == 32 && P.nc == 16": test_dense_image_hessian[N16-m1-n257] ... [N16-m8-n770]
       <false, true>        "P.antisym": [N11-m*-n*] and [N16k5-m*-n*]
       <false, false>       else: [N16general-m*-n*]
   each at 257 (per_wg 2, 129 workgroups, the last run holds one), 512 (2, 256, exact) and 770 intervals (4, 193, the last holds two)."""
import ctypes as C
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle_bridge import assert_same_hessian_values, problem_from_inputs, random_problem
from test_gpu_parity import RawHandle, assert_close, assert_close_h
from test_list_launch import GUARD, PATTERN, Guarded

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 1 << 24                  # doubles: a value array beyond this is compared on the device's copy, in slices of intervals
B = {True: "true", False: "false"}


# ------------------------------------------------------------------------------------------------
#  The launch code, restated
# ------------------------------------------------------------------------------------------------
def even_class(m):
    return 2 if m <= 2 else 4 if m <= 4 else 6 if m <= 6 else 8


def jac16_form(N, nc, m, n_int, with_dF):
    """(instantiation, grid) of qc_launch_mfma16_F_jac."""
    ket = nc != 8 or N != 8
    grid = min(n_int, 1024)
    once = grid == n_int
    head = " (HEAD where launch16m's condition holds)" if once and with_dF and not ket else ""
    return f"qc_mfma16_pade4_kernel<{B[with_dF]}, 2, false, {even_class(m)}, {B[ket]}, false{', true' if once else ''}>{head}", grid


def hess16_form(N, nc, m, n_int, antisym, gather=False, two_waves=True, once_max=1 << 30, grid_cap=1024):
    """(instantiation, grid) of mu_d2F alone at 2N <= 16: the plan's choice between qc_launch_mfma16_hess2 and qc_launch_mfma16_hess."""
    ket = nc != 8 or N != 8
    if m > 8:
        return "lds", n_int
    if two_waves and not gather and n_int <= 1024 and antisym and not ket and 1 <= m <= 6:
        return f"qc_mfma16_pade4_hess2_kernel<{even_class(m)}, false>", n_int
    window = antisym and 4 < m <= 6 and 1536 < n_int <= 2048 and not gather
    grid = n_int if (n_int <= once_max and not window) else min(n_int, grid_cap)
    once = grid == n_int
    hm = even_class(m)
    if antisym and once and gather and not ket and hm <= 6:
        return f"qc_mfma16_pade4_hess_anti_kernel<{hm}, false, false, true, false, true>", grid
    if antisym:
        return f"qc_mfma16_pade4_hess_anti_kernel<{hm}, {B[ket]}, false, {B[once]}>", grid
    return f"qc_mfma16_pade4_hess_kernel<{hm}, {B[ket]}, false{', true' if once else ''}>", grid


def jac32_form(N, nc, n_int, with_dF):
    """(instantiation, grid) of qc_launch_mfma32_F_jac."""
    ket = nc != 16 or N != 16
    n_wg = (n_int + 1) // 2
    if with_dF and n_int <= 256:
        return f"qc_mfma32_pade4_kernel<true, false, {B[ket]}, true, true>", n_int
    return f"qc_mfma32_pade4_kernel<{B[with_dF]}, false, {B[ket]}, false, {B[n_wg <= 1024]}>", min(n_wg, 1024)


def hess32_form(N, nc, n_int, antisym):
    """(instantiation, per_wg, grid, intervals of the last run) of qc_launch_mfma32_hess."""
    per_wg = -(-n_int // 256)
    grid = -(-n_int // per_wg)
    full = antisym and N == 16 and nc == 16
    name = "qc_mfma32_pade4_hess_kernel<false, true, true>" if full else f"qc_mfma32_pade4_hess_kernel<false, {B[antisym]}>"
    return name, per_wg, grid, n_int - (grid - 1) * per_wg


class Case:
    """N levels, m random dense drives, n_int intervals, ncol kets (0: a unitary); `env`: the one-wave launcher's switches in a child."""

    def __init__(self, N, m, n_int, ncol=0, free=True, herm=True, tag="", pauli=False, **env):
        self.N, self.m, self.n_int, self.ncol, self.free, self.herm, self.pauli, self.env = N, m, n_int, ncol, free, herm, pauli, env
        self.nc = ncol or N
        self.id = tag

    def forms(self):
        """The instantiations of F + dF, F alone and mu_d2F alone (with the grids), as the launch code gives them."""
        if self.N <= 8:
            return (jac16_form(self.N, self.nc, self.m, self.n_int, True), jac16_form(self.N, self.nc, self.m, self.n_int, False),
                    hess16_form(self.N, self.nc, self.m, self.n_int, self.herm, **self.env))
        return (jac32_form(self.N, self.nc, self.n_int, True), jac32_form(self.N, self.nc, self.n_int, False),
                hess32_form(self.N, self.nc, self.n_int, self.herm))

    def names(self):
        """qc_kernel_name(h, 0 / 1 / 2) as the plan (qc_plan.cpp) decides them for this case."""
        if self.N > 8:
            return "mfma32-pade4", "mfma32-pade4-hess", "two-launches"
        hess = self.forms()[2][0]
        fusable = self.herm and self.N == 8 and self.nc == 8 and 1 <= self.m <= 6
        return ("mfma16-pade4",
                "lds-hess" if hess == "lds" else "mfma16-pade4-hess2" if "hess2" in hess else
                "mfma16-pade4-hess-gather" if self.pauli else "mfma16-pade4-hess",
                None if self.pauli else "mfma16-pade4-fused" if fusable else "two-launches")      # (Pauli drives: either fused form, by length)


def ids(cases):
    return [c.id for c in cases]


PERSISTENT_16 = ([Case(8, m, 1025, tag=f"N8-m{m}-n1025") for m in (2, 3, 6, 7)] + [Case(5, m, 1025, tag=f"N5-m{m}-n1025") for m in (1, 4, 5, 8)] +
                 [Case(8, 4, 1025, ncol=3, tag="N8k3-m4-n1025"), Case(8, 9, 1025, tag="N8-m9-n1025"), Case(8, 10, 1025, tag="N8-m10-n1025"),
                  Case(8, 6, 2050, tag="N8-m6-n2050"), Case(8, 4, 1025, free=False, tag="N8-m4-n1025-fixed"),
                  Case(8, 6, 1025, herm=False, tag="N8-m6-n1025-general")])
WINDOW_COUNTS = {1536: False, 1537: True, 2048: True, 2049: False}      # just outside, first inside, last inside, just outside
WINDOW = ([Case(N, m, n, tag=f"N{N}-m{m}-n{n}") for N in (8, 5) for m in (5, 6) for n in WINDOW_COUNTS] +
          [Case(8, 6, 1537, free=False, tag="N8-m6-n1537-fixed")])
HAND_OVER = [Case(8, m, n, tag=f"m{m}-n{n}") for m in (2, 4, 6) for n in (1024, 1025)]
GENERAL_ONCE = [Case(N, m, 5, herm=False, tag=f"N{N}-m{m}") for N in (8, 3) for m in (1, 4, 5, 8)]
DENSE32_COUNTS = {256: "single", 257: "pair", 2048: "pair", 2049: "persistent"}
DENSE32_SYSTEMS = {"N16": (16, 0), "N11": (11, 0), "N16k5": (16, 5)}
# (the unmasked 2049-interval case: m = 1, 554 MB of Jacobian values)
DENSE32 = ([Case(N, {256: 2, 257: 3, 2048: 2, 2049: 1}[n] if s == "N16" else 1 + (k + j) % 3, n, ncol=ncol, tag=f"{s}-n{n}")
            for k, (s, (N, ncol)) in enumerate(DENSE32_SYSTEMS.items()) for j, n in enumerate(DENSE32_COUNTS)] +
           [Case(11, 2, 2049, free=False, tag="N11-n2049-fixed")])
HESS32_COUNTS = {257: (2, 129, 1), 512: (2, 256, 2), 770: (4, 193, 2)}      # intervals: per_wg, workgroups, intervals of the last run
HESS32_SYSTEMS = {"N16": (16, 0, True), "N11": (11, 0, True), "N16k5": (16, 5, True), "N16general": (16, 0, False)}
HESS32 = [Case(N, m, n, ncol=ncol, herm=herm, tag=f"{s}-m{m}-n{n}") for s, (N, ncol, herm) in HESS32_SYSTEMS.items() for m in (1, 8) for n in HESS32_COUNTS]
# the two children (switches read once per process)
ENV_ONE_WAVE = {"QC_HESS_ELL": "0", "QC_HESS_TWO_WAVES": "0", "QC_HESS_ONCE_MAX": "0", "QC_HESS_GRID": "8"}
ENV_GATHER = {"QC_HESS_G2": "0"}
CHILD_ONE_WAVE = [Case(N, m, 19, herm=herm, tag=f"N{N}-m{m}{'' if herm else '-general'}", two_waves=False, once_max=0, grid_cap=8)
                  for herm in (True, False) for N in (8, 3) for m in (1, 4, 5, 8)]
CHILD_GATHER = ([Case(8, m, 5, pauli=True, tag=f"pauli-m{m}", gather=True) for m in range(1, 7)] +
                [Case(8, 6, 1025, pauli=True, tag="pauli-m6-n1025", gather=True)])
EVERY_CASE = PERSISTENT_16 + WINDOW + HAND_OVER + GENERAL_ONCE + DENSE32 + HESS32 + CHILD_ONE_WAVE + CHILD_GATHER


# ------------------------------------------------------------------------------------------------
#  One case: the launches, the oracle, the comparisons
# ------------------------------------------------------------------------------------------------
def rel_err(got, ref):
    return float(np.max(np.abs(got - ref))) / max(1.0, float(np.max(np.abs(ref)))) if ref.size else 0.0


def compare(g, n_int, ref_of, close, what):
    """The Guarded device vector `g` (n_int equal interval blocks) against ref_of(a, b), the reference of intervals [a, b): margins
    untouched, every value finite and within `close`.  Returns (worst relative error, the values or None where they stayed on the device)."""
    if g.n <= BIG:
        got = g.result(what)
        ref = ref_of(0, n_int)
        assert got.shape == ref.shape, what
        close(got, ref, what)
        return rel_err(got, ref), got
    torch.cuda.synchronize()
    for part, where in ((g.all[:GUARD], "in front of"), (g.all[GUARD + g.n:], "behind")):
        assert (part.cpu().numpy().view(np.uint64) == PATTERN).all(), f"{what}: the margin {where} the vector was written"
    w = g.n // n_int
    step = max(1, (BIG // 4) // w)
    worst = 0.0
    for a in range(0, n_int, step):
        b = min(n_int, a + step)
        got = g.t[a * w:b * w].cpu().numpy()
        bad = np.flatnonzero(~np.isfinite(got))
        assert bad.size == 0, f"{what}: {bad.size} values of intervals {a} .. {b - 1} not written or not finite, first at {a * w + bad[:5]}"
        ref = ref_of(a, b)
        close(got, ref, f"{what}, intervals {a} .. {b - 1}")
        worst = max(worst, float(np.max(np.abs(got - ref))) / max(1.0, float(np.max(np.abs(ref)))))
    return worst, None


def build(qc, oracle, case):
    """(oracle Problem, Z, handle, dims, what assert_same_hessian_values reads, close())."""
    if case.pauli:
        full = qc.multi_qubit_system(3)
        inp = qc.unitary_smooth_pulse_inputs(qc.QuantumSystem(full.H_drift, list(full.H_drives)[:case.m]), qc.GATES["TOFFOLI"], case.n_int + 1)
        prob = problem_from_inputs(inp)
        prob.hess_align = 1
        Z = inp.traj.datavec + 1e-2 * np.random.default_rng(case.m).standard_normal(inp.traj.datavec.size)
        dyn = qc.QuantumDynamics(inp.integrators, inp.traj)
        return prob, Z, dyn._h, dyn.dims, dyn, dyn.close
    prob, Z = random_problem(oracle, N=case.N, m=case.m, T=case.n_int + 1, free_time=case.free, hermitian=case.herm, ncol=case.ncol, seed=1)
    h = RawHandle(qc, prob)
    desc = SimpleNamespace(integrator=0, N=prob.N, state_cols=case.ncol, off_dt=prob.off_dt, hess_offset=0, m=prob.m)
    return prob, Z, h.h, h.dims, SimpleNamespace(_desc=desc, dims=h.dims), h.close


def form_text(case):
    (jf, jg), (ff, fg), hf = case.forms()
    return f"F + dF {jf} on {jg} workgroups; F alone {ff} on {fg}; mu_d2F {hf[0]} on {hf[-2] if len(hf) > 2 else hf[1]}"


def check_case(qc, oracle, coracle, case, make=None, with_dF=True, F_bits=True, twice=False, one_call_bits=False, form=form_text, tag="PADE4-FORMS"):
    """The launches of one case against the C oracle.  What tests/test_pade_other_launch_forms.py chooses (the defaults: this file):
    `make(qc, oracle, case)` in place of build(); with_dF = False: F alone and mu_d2F only (no dF vector is allocated); F_bits = False:
    a family whose residual-only launch does not promise the bits of F + dF's residuals (both are compared with the oracle); twice:
    mu_d2F a second time on the same handle, the bits of the first; one_call_bits: the one call's mu_d2F equals the launch's in every
    bit, the (a, a) block included; form(case): the form's part of the printed line."""
    prob, Z, h, dims, like, close = (make or build)(qc, oracle, case)
    try:
        L = qc._lib
        what = case.id
        n_int = case.n_int
        assert int(dims.n_intervals) == n_int and (prob.n, prob.nc, prob.m) == (2 * case.N, case.nc, case.m), what
        names = tuple(L.lib.qc_kernel_name(h, k).decode() for k in (0, 1, 2))
        want = case.names()
        assert names[:2] == want[:2] and (want[2] is None or names[2] == want[2]), (what, names, want)
        ref = coracle.COracle(prob)
        assert (int(dims.ddim), int(dims.jac_nnz_interval), int(dims.hess_nnz_interval)) == (ref.ddim, ref.jac_nnz, ref.hess_nnz + ref.hess_pad), what
        mu = np.random.default_rng(n_int + case.m).standard_normal(prob.n_rows)
        dZ, dmu = torch.from_numpy(Z).cuda(), torch.from_numpy(mu).cuda()
        pZ, pmu = C.c_void_p(dZ.data_ptr()), C.c_void_p(dmu.data_ptr())
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        # F + dF, F alone (dvals = NULL), mu_d2F alone
        F1, H = Guarded(dims.F_len), Guarded(dims.hess_nnz)
        Fr = ref.F_dF(Z, 0, n_int, True, False)[0]
        eJ, J, Jv = 0.0, None, None
        if with_dF:
            F, J = Guarded(dims.F_len), Guarded(dims.jac_nnz)
            L.check(L.lib.qc_eval_F_jac_dev(h, pZ, F.ptr(), J.ptr(), st), h)
        L.check(L.lib.qc_eval_F_jac_dev(h, pZ, F1.ptr(), None, st), h)
        L.check(L.lib.qc_eval_hess_dev(h, pZ, pmu, H.ptr(), st), h)
        if with_dF:
            eF, Fv = compare(F, n_int, lambda a, b: Fr, assert_close, what + ": F")
            eJ, Jv = compare(J, n_int, lambda a, b: ref.F_dF(Z, a, b, False, True)[1], assert_close, what + ": dF")
        eF1, F1v = compare(F1, n_int, lambda a, b: Fr, assert_close, what + ": F alone")
        if not with_dF:
            eF, Fv = eF1, F1v
        elif F_bits:
            assert np.array_equal(F1v, Fv), f"{what}: F alone differs from the F of F + dF in {(F1v != Fv).sum()} values, first at {np.flatnonzero(F1v != Fv)[:5]}"
        eH, Hv = compare(H, n_int, lambda a, b: ref.mu_d2F(Z, mu, a, b), assert_close_h, what + ": mu_d2F")
        if twice:      # (a kernel that keeps per-workgroup scratch between its trips: the second launch starts from what the first left)
            assert Hv is not None
            H.t.fill_(float("nan"))
            L.check(L.lib.qc_eval_hess_dev(h, pZ, pmu, H.ptr(), st), h)
            Hw = H.result(what + ": mu_d2F, second launch")
            assert np.array_equal(Hw, Hv), f"{what}: the second mu_d2F launch differs from the first in {(Hw != Hv).sum()} values, first at {np.flatnonzero(Hw != Hv)[:5]}"
        del H
        print(f"{tag} {what}: kernels {names[0]} / {names[1]} / {names[2]}; intervals {n_int}; {form(case)}; "
              f"worst rel. error F {max(eF, eF1):.2e} dF {eJ:.2e} mu_d2F {eH:.2e}")
        if names[2] != "two-launches":      # the one call against the two launches (each compared with the oracle above)
            assert with_dF and Hv is not None
            F2, J2, H2 = Guarded(dims.F_len), Guarded(dims.jac_nnz), Guarded(dims.hess_nnz)
            L.check(L.lib.qc_eval_F_jac_hess_dev(h, pZ, pmu, F2.ptr(), J2.ptr(), H2.ptr(), st), h)
            F2v, H2v = F2.result(what + ": one call, F"), H2.result(what + ": one call, mu_d2F")
            assert_close(F2v, Fv, what + ": one call, F")
            if Jv is not None:
                J2v = J2.result(what + ": one call, dF")
                assert np.array_equal(J2v, Jv), f"{what}: one call, dF differs from the dF launch in {(J2v != Jv).sum()} values"
            else:      # both vectors stayed on the device; the launch's values were found finite above, so bitwise equality is torch.equal
                compare(J2, n_int, lambda a, b: ref.F_dF(Z, a, b, False, True)[1], assert_close, what + ": one call, dF")
                assert torch.equal(J2.t, J.t), f"{what}: one call, dF differs from the dF launch in {int((J2.t != J.t).sum())} values"
            assert_same_hessian_values(H2v, Hv, like, what + ": one call against two launches")
            if one_call_bits:
                assert np.array_equal(H2v, Hv), f"{what}: one call, mu_d2F differs from the mu_d2F launch in {(H2v != Hv).sum()} values"
            assert_close_h(H2v, ref.mu_d2F(Z, mu), what + ": one call, mu_d2F")
    finally:
        close()


# ------------------------------------------------------------------------------------------------
#  The table
# ------------------------------------------------------------------------------------------------
def test_cases_reach_every_instantiation():
    """What the case lists reach, by the restated launch code, against the instantiations of the module docstring written out."""
    jac, hess = set(), set()
    for c in EVERY_CASE:
        (jf, _), (ff, _), hf = c.forms()
        jac |= {jf.split(" (")[0], ff}
        hess.add(hf[0])
    tf = ("true", "false")
    jac16 = {f"qc_mfma16_pade4_kernel<{j}, 2, false, {mu}, {k}, false{o}>" for j in tf for mu in (2, 4, 6, 8) for k in tf for o in ("", ", true")}
    jac32 = ({f"qc_mfma32_pade4_kernel<true, false, {k}, true, true>" for k in tf} |
             {f"qc_mfma32_pade4_kernel<{j}, false, {k}, false, {o}>" for j in tf for k in tf for o in tf})
    assert len(jac16) == 32 and len(jac32) == 10 and jac == jac16 | jac32, sorted(jac ^ (jac16 | jac32))
    hess16 = ({f"qc_mfma16_pade4_hess_anti_kernel<{hm}, {k}, false, {o}>" for hm in (2, 4, 6, 8) for k in tf for o in tf} |
              {f"qc_mfma16_pade4_hess_kernel<{hm}, {k}, false{o}>" for hm in (2, 4, 6, 8) for k in tf for o in ("", ", true")} |
              {f"qc_mfma16_pade4_hess_anti_kernel<{hm}, false, false, true, false, true>" for hm in (2, 4, 6)})
    hess2 = {f"qc_mfma16_pade4_hess2_kernel<{mu}, false>" for mu in (2, 4, 6)}
    hess32 = {"qc_mfma32_pade4_hess_kernel<false, true, true>", "qc_mfma32_pade4_hess_kernel<false, true>", "qc_mfma32_pade4_hess_kernel<false, false>"}
    assert len(hess16) == 35 and hess == hess16 | hess2 | hess32 | {"lds"}, sorted(hess ^ (hess16 | hess2 | hess32 | {"lds"}))
    assert len({c.id for c in PERSISTENT_16 + WINDOW + HAND_OVER + GENERAL_ONCE + DENSE32 + HESS32}) == len(EVERY_CASE) - len(CHILD_ONE_WAVE) - len(CHILD_GATHER)


# ------------------------------------------------------------------------------------------------
#  1. F + dF and F alone at 2N <= 16, persistent
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PERSISTENT_16, ids=ids(PERSISTENT_16))
def test_F_dF_persistent(qc, oracle, coracle, case):
    """1025 intervals: one workgroup past one trip of kMaxGrid = 1024 (2050: two past two trips), in every drive-count class, masked by
    levels and by kets, with one and two drives beyond the hand-off block."""
    (jf, jg), (ff, fg), _ = case.forms()
    assert jg == fg == 1024 and jf.endswith(", false>") and ff.endswith(", false>") and case.n_int in (1025, 2050)
    check_case(qc, oracle, coracle, case)


# ------------------------------------------------------------------------------------------------
#  2. mu_d2F, the one-wave kernel's window
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", WINDOW, ids=ids(WINDOW))
def test_window(qc, oracle, coracle, case):
    """Antisymmetric generators, 5 or 6 drives, 1537 .. 2048 intervals: the persistent instantiation on 1024 workgroups (masked at
    five levels); one interval less or more: one interval per workgroup."""
    name, grid = case.forms()[2]
    inside = WINDOW_COUNTS[case.n_int]
    assert grid == (1024 if inside else case.n_int)
    assert name == f"qc_mfma16_pade4_hess_anti_kernel<6, {B[case.N != 8]}, false, {B[not inside]}>"
    check_case(qc, oracle, coracle, case)


# ------------------------------------------------------------------------------------------------
#  3. The hand-over between the two-wave and the one-wave kernel
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", HAND_OVER, ids=ids(HAND_OVER))
def test_hand_over(qc, oracle, coracle, case):
    """1024 intervals: `mfma16-pade4-hess2`; 1025: `mfma16-pade4-hess`, one interval per workgroup."""
    assert case.names()[1] == ("mfma16-pade4-hess2" if case.n_int == 1024 else "mfma16-pade4-hess")
    check_case(qc, oracle, coracle, case)


@pytest.mark.parametrize("case", GENERAL_ONCE, ids=ids(GENERAL_ONCE))
def test_general_one_wave_loop_free(qc, oracle, coracle, case):
    """Generators that are not antisymmetric (`hermitian=False`), five intervals: the loop-free instantiations of the general kernel."""
    assert case.forms()[2][0] == f"qc_mfma16_pade4_hess_kernel<{even_class(case.m)}, {B[case.N != 8]}, false, true>"
    check_case(qc, oracle, coracle, case)


# ------------------------------------------------------------------------------------------------
#  4. Forms behind a switch read once per process: one fresh child each
# ------------------------------------------------------------------------------------------------
CHILD = """
import sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import test_pade4_launch_forms as t
t.child_main(sys.argv[2])
"""
CHILDREN = {"one-wave": (ENV_ONE_WAVE, CHILD_ONE_WAVE), "gather": (ENV_GATHER, CHILD_GATHER)}


def child_main(which):
    """In the child: every case of the list, asserted here; the parent reads the exit status."""
    import __graft_entry__ as g
    import oracle.qc_oracle_c as oc
    env, cases = CHILDREN[which]
    assert all(os.environ.get(k) == v for k, v in env.items()), "the child was started without its switches"
    qc, o = g.load_package(), g.load_oracle()
    for case in cases:
        check_case(qc, o, oc, case)
    print(f"PADE4-FORMS child {which}: {len(cases)} cases")


def run_child(which):
    env = dict(os.environ, **CHILDREN[which][0])
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, which], env=env, capture_output=True, text=True, timeout=240)
    print(r.stdout)
    assert r.returncode == 0, f"the child ended with status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    assert f"PADE4-FORMS child {which}: {len(CHILDREN[which][1])} cases" in r.stdout


def test_one_wave_persistent_forms_in_a_child():
    """QC_HESS_ELL=0 QC_HESS_TWO_WAVES=0 QC_HESS_ONCE_MAX=0 QC_HESS_GRID=8: 19 intervals on 8 persistent workgroups (trips of 3, 3, 3, 2,
    2, 2, 2, 2), HM 2 / 4 / 6 / 8 x unmasked (N = 8) / masked (N = 3) x antisymmetric / general: the 16 persistent instantiations of the
    two one-wave kernels (and, 19 intervals being one trip of F + dF, that launcher's loop-free instantiations)."""
    for case in CHILD_ONE_WAVE:
        name, grid = case.forms()[2]
        kernel = "qc_mfma16_pade4_hess_anti_kernel" if case.herm else "qc_mfma16_pade4_hess_kernel"
        assert grid == 8 and name == (f"{kernel}<{even_class(case.m)}, {B[case.N != 8]}, false, false>" if case.herm else
                                      f"{kernel}<{even_class(case.m)}, {B[case.N != 8]}, false>")
    run_child("one-wave")


def test_row_gather_form_in_a_child():
    """QC_HESS_G2=0: three-qubit Pauli drives, m = 1 .. 6 at T = 6 and m = 6 at 1025 intervals take the one-wave kernel's row-gather
    instantiation (HM = 2, 4, 6), loop-free at any length, under the name `mfma16-pade4-hess-gather`."""
    for case in CHILD_GATHER:
        name, grid = case.forms()[2]
        assert grid == case.n_int and name == f"qc_mfma16_pade4_hess_anti_kernel<{even_class(case.m)}, false, false, true, false, true>"
    run_child("gather")


# ------------------------------------------------------------------------------------------------
#  5. The dense-image F + dF kernel at 2N = 32
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", DENSE32, ids=ids(DENSE32))
def test_dense_image_F_dF(qc, oracle, coracle, case):
    """256 intervals: the last SINGLE count (F alone: pairs); 257: pairs, the last slot empty; 2048: 1024 pairs, the last loop-free
    count; 2049: persistent, the empty slot of the odd count on the second trip."""
    (jf, jg), (ff, fg), _ = case.forms()
    kind = DENSE32_COUNTS[case.n_int]
    assert (jg, fg) == {"single": (256, 128), "pair": ((case.n_int + 1) // 2,) * 2, "persistent": (1024, 1024)}[kind]
    assert jf.endswith({"single": ", true, true>", "pair": ", false, true>", "persistent": ", false, false>"}[kind])
    assert ff.endswith(", false, false>" if kind == "persistent" else ", false, true>") and ff.startswith("qc_mfma32_pade4_kernel<false")
    check_case(qc, oracle, coracle, case)


# ------------------------------------------------------------------------------------------------
#  6. The dense-image mu_d2F kernel at 2N = 32
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", HESS32, ids=ids(HESS32))
def test_dense_image_hessian(qc, oracle, coracle, case):
    """Runs of per_wg = ceil(n_int / 256) intervals per workgroup with a ragged last run, one drive and eight (one wave per drive), in
    the three instantiations."""
    name, per_wg, grid, last = case.forms()[2]
    assert (per_wg, grid, last) == HESS32_COUNTS[case.n_int]
    assert name == {"N16": "qc_mfma32_pade4_hess_kernel<false, true, true>", "N16general": "qc_mfma32_pade4_hess_kernel<false, false>"}.get(
        case.id.split("-")[0], "qc_mfma32_pade4_hess_kernel<false, true>")
    check_case(qc, oracle, coracle, case)
