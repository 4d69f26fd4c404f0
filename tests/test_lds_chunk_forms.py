"""The LDS / global-workspace kernels (qc_lds_kernels.hip: qc_lds_pade_kernel<JAC, GWS>, qc_lds_pade_hess_kernel<GWS>, qc_lds_exp_kernel<JAC,
GWS>; qc_lds_exp_hess.hip: qc_lds_exp_hess_kernel<GWS>) behind a SINGLE handle at every drive-chunk form their launchers can start:
every value of F, dF and mu_d2F against the C restatement of the oracle (oracle/qc_oracle_c.py) in NaN-filled device buffers between
two guard margins, the suite's tolerances as they stand (assert_close: rtol 1e-10, atol 1e-12 x the largest entry for F and dF;
assert_close_h: 1e-11 x for mu_d2F), F alone equal to the F of F + dF bit for bit.  The harness is tests/test_pade4_launch_forms.py's
check_case / compare; each case builds its problem here (Case.problem: oracle_bridge.random_problem, seed 1, then what the case
changes), asserts qc_kernel_name and prints one line: case, kernel names, intervals, the chunk forms with the bytes of LDS or the
workspace stride, the worst error of F / dF / mu_d2F relative to max(1, the largest reference entry).

What a launch looks like follows from the LDS budget, restated below from the library's text and compared, case by case, with what the
device-free half of qc_create reports (tests/lds_forms_test.cpp, no GPU: test_the_restated_budget_equals_the_library).
N = levels (n = 2N rows), nc = state columns, s = n nc, p = order / 2, m1 = max(m, 1), e(x) = x rounded up to even; sizes in doubles.

  jac_layout (Pade F + dF)       2 e(zdim) + p n^2 + 2 (p + 1) n nc + p n nc + jchunk p n nc
  hess_layout (Pade mu_d2F)      2 e(zdim) + e(ddim) + p n^2 + 3 (p + 1) n nc + 3 p n nc + n^2 + e(m1^2)
                                 + max(2 cj p n nc, 3 cj pm1 n nc), pm1 = max(p - 1, 1) (order 2: the clamp; its (a, a) block is zeros)
  exp_layout (exp. F + dF)       2 e(zdim) + 7 n^2 + 3 cj n^2 + n nc + 16
  layout (exp. mu_d2F)           e(zdim) + e(s) + 3 n nc + 16 + 10 n^2 + 6 cj n^2
  the chunk                      cj = m1; while (cj > 1 && bytes(cj) > limit) cj = (cj + 1) / 2 -- limit 64 KiB for P.jchunk (qc_host.cpp),
                                 exp_chunk and chunk_of, 96 KiB for hess_chunk; a chunk of one drive is taken whatever it needs
                                 (P.jchunk of an exponential handle is not read by its kernels: the loop halves it to 1 above 64 KiB)
  the switch                     bytes of F + dF or of mu_d2F "> 160 * 1024": scratch in the global workspace, every chunk min(m1, 2),
                                 ws_stride = (max(the two byte counts) / 8 + 1) & ~1 doubles per interval, 1024 threads
  the kernels                    for (j0 = 0; j0 < m; j0 += cj) jc = min(cj, m - j0); the (a_i, a_j) block of the Pade Hessian: the same
                                 loop over i0 inside it; dynamic LDS beyond 64 KiB is asked for by raise_lds_limit; grid = n_int,
                                 interval qc_xcd_remap(blockIdx.x, n_int), workspace slot blockIdx.x.

Chunk forms, named by the drives of each pass: "one" (cj >= m >= 1), "equal" (cj divides m), "ragged" (a shorter last pass, cj >= 2),
"ones" (cj = 1 < m), "no drives".  In the workspace form a chunk of one is the single chunk of m = 1.  Intervals: 263 (a remainder of
7 in the remap) where the larger launch of the case takes at most 96 KiB of LDS, 13 for the larger ones and for the workspace, 1 once
per kernel.  The cases and what they were chosen for (ids of test_every_value; bytes of F + dF / mu_d2F):
  p4-N12-m9 (5+4 / 3+3+3)  p4-N12-m13 (7+6, 65 152 / 4+4+4+1)  p4-N14-m13 (6x2+1 / 13x1)  p4-N12-m8 (4+4 both)  p4-N8-m33 (17+16 / 9+9+9+6,
  the default plan)  p4-N16-m9 (default plan: mu_d2F alone is the LDS kernel, 9x1 in 115 936) and -lds (F + dF 9x1 in 65 984)
  p4-N16-m33  p4-N18-m40 (160 544)  p4-N19-m12 (163 680 of the CU's 163 840 bytes: the largest)  p4-N19-m13 (its workspace neighbour,
  6x2+1)  p4-N20-m5 / -m4 / -m2 / -m1-n1 / -m0-fixed (workspace: 2+2+1, 2+2, one, one, none)  p6-N12-m5 (default plan, 3+2 / 5x1)
  p12-N8-m13 (4+4+4+1 / 6x2+1)  p12-N10-m5  p12-N12k7-m5 (F + dF in exactly 65 536 bytes: the `<=` of both P.jchunk's loop and
  raise_lds_limit)  p12-N16k7-m13 (default plan, 99 968 / 161 696)  p12-N12-m5 (default plan, workspace at 2N = 24)  p2-N12-m9 (p = 1)
  p20-N9-m5  p4-N5-m3-n1  e-N8-m9 (default plan: nine drives are the LDS class, 5+4 / 3+3+3)  e-N8-m13 (7+6 / 6x2+1)  e-N8-m12 (6+6 / 3+3+3+3)
  e-N12-m3 (3x1, mu_d2F in 85 KiB)  e-N16-m5 (5x1, 94 592 / 151 808)  e-N17k11-m3 (101 744 / 163 136: the largest)  e-N17k12-m3 (its
  workspace neighbour)  e-N17-m5 (default plan) / -m4 / -m2 / -m1-n1 / -m0-fixed  e-N5-m3-n1
  twins: -fixed, -general (hermitian=False), kets (p4-N16k7-m9 5+4, e-N16k3-m5), -align16, -shuffled of p4-N12-m9 and e-N8-m13.
Further tests, one LDS and one workspace case per integrator: a second mu_d2F launch (check_case's twice) and a second F + dF launch
after it on the same handle give the bits of the first (the workspace then starts from what the other kernel left); knot shards
(t_range) from an odd first interval at two lengths concatenate to the full launch bit for bit.  The mutation tests (no GPU) feed
defective copies of the oracle's own vectors through the same compare / assert_close path and require each to be rejected."""
import ctypes as C
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import test_pade4_launch_forms as forms4
from oracle_bridge import random_problem
from test_gpu_parity import RawHandle, assert_close, assert_close_h
from test_list_launch import Guarded
from test_pade4_launch_forms import BIG, check_case, compare
from test_pade_other_launch_forms import HostVector, xcd_remap

TAG = "LDS-CHUNK-FORMS"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quantumcollocation.jl_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KIB = 1024
WS_SWITCH = 160 * KIB


# ------------------------------------------------------------------------------------------------
#  The LDS budget, restated
# ------------------------------------------------------------------------------------------------
def even_up(x):
    return (x + 1) & ~1


def jac_layout(q, jchunk):
    p = max(q.p, 1)
    return 2 * even_up(q.zdim) + p * q.n2 + 2 * (p + 1) * q.nN + p * q.nN + jchunk * p * q.nN


def hess_layout(q, cj):
    p, m1 = q.p, max(q.m, 1)
    pm1 = p - 1 if p > 1 else 1
    fixed = 2 * even_up(q.zdim) + even_up(q.ddim) + p * q.n2 + 3 * (p + 1) * q.nN + 3 * p * q.nN + q.n2 + even_up(m1 * m1)
    return fixed + max(2 * cj * p * q.nN, cj * pm1 * q.nN + cj * 2 * pm1 * q.nN)


def exp_layout(q, cj):
    return 2 * even_up(q.zdim) + 7 * q.n2 + 3 * cj * q.n2 + q.nN + 16


def exp_hess_layout(q, cj):
    return even_up(q.zdim) + even_up(q.s) + 3 * q.nN + 16 + 10 * q.n2 + 6 * cj * q.n2


def halving(m, layout, limit):
    """(the chunk, every chunk tried) of "while (cj > 1 && bytes(cj) > limit) cj = (cj + 1) / 2"."""
    cj = max(m, 1)
    tried = [cj]
    while cj > 1 and layout(cj) * 8 > limit:
        cj = (cj + 1) // 2
        tried.append(cj)
    return cj, tried


def budget(prob):
    """What qc_blueprint_build decides for the oracle Problem `prob`: jchunk, the chunks of the two launches, their bytes, the switch."""
    pade = prob.integrator == 0
    q = SimpleNamespace(n2=prob.n * prob.n, nN=prob.n * prob.nc, s=prob.s, zdim=prob.zdim, ddim=prob.ddim, p=prob.order // 2 if pade else 2, m=prob.m)
    m1 = max(prob.m, 1)
    jl, hl = (jac_layout, hess_layout) if pade else (exp_layout, exp_hess_layout)
    jl_q, hl_q = (lambda cj: jl(q, cj)), (lambda cj: hl(q, cj))
    limits = (64 * KIB, 96 * KIB if pade else 64 * KIB)
    cj_jac, tried_jac = halving(prob.m, jl_q, limits[0])
    cj_hess, tried_hess = halving(prob.m, hl_q, limits[1])
    bytes_jac, bytes_hess = jl_q(cj_jac) * 8, hl_q(cj_hess) * 8
    jchunk = cj_jac if pade else (m1 if bytes_jac <= 64 * KIB else 1)
    use_ws = bytes_jac > WS_SWITCH or bytes_hess > WS_SWITCH
    ws_stride = 0
    if use_ws:
        jchunk = cj_jac = cj_hess = min(m1, 2)
        bytes_jac, bytes_hess = jl_q(cj_jac) * 8, hl_q(cj_hess) * 8
        ws_stride = (max(bytes_jac, bytes_hess) // 8 + 1) & ~1
    return SimpleNamespace(pade=pade, jchunk=jchunk, cj_jac=cj_jac, cj_hess=cj_hess, bytes_jac=bytes_jac, bytes_hess=bytes_hess, use_ws=use_ws,
                           ws_stride=ws_stride, tried_jac=tried_jac, tried_hess=tried_hess, layout_jac=jl_q, layout_hess=hl_q, limits=limits, m=prob.m)


def passes(m, cj):
    """Drives of each pass of "for (j0 = 0; j0 < m; j0 += cj) jc = min(cj, m - j0)"."""
    return [min(cj, m - j0) for j0 in range(0, m, cj)]


def chunk_form(m, cj):
    if m == 0:
        return "no drives"
    if cj >= m:
        return "one"
    if cj == 1:
        return "ones"
    return "equal" if m % cj == 0 else "ragged"


def pair_kinds(m, cj):
    """The (i-chunk, j-chunk) kinds of the Pade Hessian's double loop over chunks."""
    kind = {jc: "full" if jc == cj else "ragged" for jc in passes(m, cj)}
    return {(kind[ic], kind[jc]) for jc in passes(m, cj) for ic in passes(m, cj)}


def lds_class(nbytes):
    return "<= 64 KiB" if nbytes <= 64 * KIB else "<= 96 KiB" if nbytes <= 96 * KIB else "> 96 KiB"


def passes_text(m, cj):
    ps = passes(m, cj)
    if len(ps) < 2:
        return str(ps[0]) if ps else "no drives"
    full = sum(1 for x in ps if x == cj)
    return (f"{full}x{cj}" if full > 1 else str(cj) if full else "") + (f"+{ps[-1]}" if ps[-1] != cj else "")


# ------------------------------------------------------------------------------------------------
#  The cases
# ------------------------------------------------------------------------------------------------
class Case:
    """integ "pade" / "exp"; N levels, m drives, n_int intervals, ncol kets (0: a unitary); kernel "lds" (forced) or "auto" (the default
    plan; jac: the name of F + dF where that is an MFMA kernel); align: qc_desc.hess_align; twice: check_case launches mu_d2F twice."""

    def __init__(self, tag, integ, N, m, n_int, ncol=0, order=4, free=True, herm=True, layout="standard", align=0, kernel="lds", jac=None, twice=False):
        self.id, self.integ, self.N, self.m, self.n_int, self.ncol, self.order, self.free, self.herm = tag, integ, N, m, n_int, ncol, order, free, herm
        self.layout, self.align, self.kernel, self.jac, self.twice = layout, align, kernel, jac, twice
        self.nc = ncol or N
        self._problem, self._budget, self._oracle = None, None, None

    def problem(self, o, keep=True):
        if self._problem is not None:
            return self._problem
        prob, Z = random_problem(o, N=self.N, m=max(self.m, 1), T=self.n_int + 1, order=self.order, free_time=self.free, hermitian=self.herm,
                                 ncol=self.ncol, layout=self.layout, seed=1, integrator=o.PADE if self.integ == "pade" else o.EXPONENTIAL)
        if self.m == 0:      # no drives: no derivative integrators either (the knot keeps its width)
            prob.m, prob.G_drives, prob.derivs = 0, prob.G_drives[:0], []
        prob.hess_align = self.align or 1
        if keep:
            self._problem = prob, Z
        return prob, Z

    def budget(self, o):
        if self._budget is None:
            self._budget = budget(self.problem(o, keep=False)[0])
        return self._budget

    def names(self, o=None):
        b = self.budget(o or self._oracle)
        hess = {(True, False): "lds-hess", (True, True): "lds-gws-hess", (False, False): "lds-exp-hess", (False, True): "lds-gws-exp-hess"}[(b.pade, b.use_ws)]
        return self.jac or ("lds-gws" if b.use_ws else "lds"), hess, "two-launches"

    def line(self, o):
        """The case as tests/lds_forms_test.cpp reads it: the descriptor's fields with the knot layout random_problem builds."""
        prob = self.problem(o, keep=False)[0]
        derivs = " ".join(f"{d.x_off} {d.dx_off} {d.dim}" for d in prob.derivs)
        return (f"{self.id} {self.order if self.integ == 'pade' else 0} {prob.N} {self.ncol} {prob.m} {prob.T} {prob.zdim} {prob.off_U} {prob.off_a} {prob.off_dt} "
                f"{ {'auto': 0, 'mfma': 1, 'lds': 2}[self.kernel]} {int(self.herm)} {self.align} {len(prob.derivs)} {derivs}").rstrip()


def pade(tag, N, m, n_int, **kw):
    return Case(tag, "pade", N, m, n_int, **kw)


def expo(tag, N, m, n_int, **kw):
    return Case(tag, "exp", N, m, n_int, **kw)


VARIANTS = {"fixed": dict(free=False), "general": dict(herm=False), "align16": dict(align=16), "shuffled": dict(layout="shuffled")}
PADE_CASES = [
    pade("p4-N12-m9", 12, 9, 263, twice=True), pade("p4-N12-m13", 12, 13, 263), pade("p4-N14-m13", 14, 13, 263), pade("p4-N12-m8", 12, 8, 263),
    pade("p4-N8-m33", 8, 33, 263, kernel="auto"), pade("p4-N16-m9", 16, 9, 13, kernel="auto", jac="mfma32-pade4"), pade("p4-N16-m9-lds", 16, 9, 13),
    pade("p4-N16-m33", 16, 33, 13), pade("p4-N18-m40", 18, 40, 13), pade("p4-N19-m12", 19, 12, 13), pade("p4-N19-m13", 19, 13, 13),
    pade("p4-N20-m5", 20, 5, 13, twice=True), pade("p4-N20-m4", 20, 4, 13), pade("p4-N20-m2", 20, 2, 13), pade("p4-N20-m1-n1", 20, 1, 1),
    pade("p4-N20-m0-fixed", 20, 0, 13, free=False), pade("p6-N12-m5", 12, 5, 263, order=6, kernel="auto"), pade("p12-N8-m13", 8, 13, 263, order=12),
    pade("p12-N10-m5", 10, 5, 13, order=12), pade("p12-N12k7-m5", 12, 5, 13, ncol=7, order=12),
    pade("p12-N16k7-m13", 16, 13, 13, ncol=7, order=12, kernel="auto"), pade("p12-N12-m5", 12, 5, 13, order=12, kernel="auto"),
    pade("p2-N12-m9", 12, 9, 263, order=2), pade("p20-N9-m5", 9, 5, 13, order=20), pade("p4-N5-m3-n1", 5, 3, 1), pade("p4-N16k7-m9", 16, 9, 263, ncol=7),
] + [pade(f"p4-N12-m9-{v}", 12, 9, 263, **kw) for v, kw in VARIANTS.items()]
EXP_CASES = [
    expo("e-N8-m9", 8, 9, 263, kernel="auto"), expo("e-N8-m13", 8, 13, 263, twice=True),
    expo("e-N8-m12", 8, 12, 263), expo("e-N12-m3", 12, 3, 263), expo("e-N16-m5", 16, 5, 13), expo("e-N17k11-m3", 17, 3, 13, ncol=11),
    expo("e-N17k12-m3", 17, 3, 13, ncol=12), expo("e-N17-m5", 17, 5, 13, kernel="auto", twice=True), expo("e-N17-m4", 17, 4, 13), expo("e-N17-m2", 17, 2, 13),
    expo("e-N17-m1-n1", 17, 1, 1), expo("e-N17-m0-fixed", 17, 0, 13, free=False), expo("e-N5-m3-n1", 5, 3, 1), expo("e-N16k3-m5", 16, 5, 13, ncol=3),
] + [expo(f"e-N8-m13-{v}", 8, 13, 263, **kw) for v, kw in VARIANTS.items()]
EVERY_CASE = PADE_CASES + EXP_CASES
BY_ID = {c.id: c for c in EVERY_CASE}
# one LDS and one workspace case per integrator: the second launches and the shards
RELAUNCH = ["p4-N12-m9", "p4-N20-m5", "e-N8-m13", "e-N17-m5"]
SHARDS = ((0, 1), (1, 4), (4, 5), (5, 13))      # 1, 3 (odd first interval), 1, 8 (odd first interval) of 13 intervals
# the largest LDS launch of each integrator (bytes of mu_d2F) and the case one step on, in the workspace
LARGEST = {"pade": ("p4-N19-m12", 163680, "p4-N19-m13"), "exp": ("e-N17k11-m3", 163136, "e-N17k12-m3")}
MUTATION_CASES = [pade("mutation-p4-N8-m33", 8, 33, 5), expo("mutation-e-N8-m13", 8, 13, 5)]


def ids(cases):
    return [c.id for c in cases]


def form_text(case):
    b = case.budget(case._oracle)
    where = f"workspace of {b.ws_stride} doubles an interval" if b.use_ws else f"LDS {b.bytes_jac} / {b.bytes_hess} bytes"
    jac = f"by {case.jac}" if case.jac else f"{passes_text(case.m, b.cj_jac)} ({chunk_form(case.m, b.cj_jac)})"
    return (f"chunks F + dF {jac}, mu_d2F {passes_text(case.m, b.cj_hess)} "
            f"({chunk_form(case.m, b.cj_hess)}); {where}; remap remainder {case.n_int & 7}")


def make(qc, oracle, case):
    case._oracle = oracle
    prob, Z = case.problem(oracle)
    h = RawHandle(qc, prob, kernel=case.kernel, hess_align=case.align)
    desc = SimpleNamespace(integrator=prob.integrator, N=prob.N, state_cols=case.ncol, off_dt=prob.off_dt, hess_offset=0, m=prob.m)

    def close():      # (the case lists live as long as the session: the trajectory does not)
        h.close()
        case._problem = None
    return prob, Z, h.h, h.dims, SimpleNamespace(_desc=desc, dims=h.dims), close


# ------------------------------------------------------------------------------------------------
#  Without a GPU: the library's budget against the restatement, the table of forms, the checker against defective vectors
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver_table(tmp_path_factory, oracle):
    """{case id: what tests/lds_forms_test.cpp printed for it}."""
    if not os.path.exists(HIPCC):
        pytest.skip("needs hipcc")
    lib = os.path.join(CSRC, "libqcolloc_hip.so")
    assert os.path.exists(lib), "libqcolloc_hip.so is not built (__graft_entry__.build())"
    tmp = tmp_path_factory.mktemp("lds_forms")
    exe = str(tmp / "lds_forms_test")
    cmd = [HIPCC, "-O1", "-std=c++17", "--offload-arch=gfx950", "-x", "hip", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "lds_forms_test.cpp"), "-o", exe, "-L" + CSRC, "-lqcolloc_hip", "-Wl,-rpath," + CSRC]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    cases = str(tmp / "cases.txt")
    with open(cases, "w") as f:
        f.write("".join(c.line(oracle) + "\n" for c in EVERY_CASE + MUTATION_CASES))
    env = {k: v for k, v in os.environ.items() if not k.startswith("QC_")}
    r = subprocess.run([exe, cases], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    table = {}
    for line in r.stdout.splitlines():
        tag, nums, names = line.split(" | ")
        jchunk, bytes_jac, bytes_hess, use_ws, ws_stride = (int(x) for x in nums.split())
        table[tag] = SimpleNamespace(jchunk=jchunk, bytes_jac=bytes_jac, bytes_hess=bytes_hess, use_ws=use_ws, ws_stride=ws_stride, names=tuple(names.split()))
    print(f"{TAG} the library's table\n" + r.stdout)
    return table


def test_the_restated_budget_equals_the_library(driver_table, oracle):
    """Every case: the restated jchunk, bytes of both launches, use_ws and ws_stride are the library's, the kernel names are the ones
    the case asserts on the device, and each restated chunk is the first of its halving sequence that fits (the chunk tried before it
    does not; a chunk of one is taken whatever it needs)."""
    assert set(driver_table) == {c.id for c in EVERY_CASE + MUTATION_CASES}
    for c in EVERY_CASE + MUTATION_CASES:
        b, d = c.budget(oracle), driver_table[c.id]
        assert (b.jchunk, b.bytes_jac, b.bytes_hess, int(b.use_ws), b.ws_stride) == (d.jchunk, d.bytes_jac, d.bytes_hess, d.use_ws, d.ws_stride), c.id
        assert c.names(oracle) == d.names, (c.id, d.names)
        if b.use_ws:
            assert b.cj_jac == b.cj_hess == min(max(c.m, 1), 2) and b.ws_stride % 2 == 0 and b.ws_stride * 8 >= max(b.bytes_jac, b.bytes_hess), c.id
            lds_jac, lds_hess = (layout(tried[-1]) * 8 for layout, tried in ((b.layout_jac, b.tried_jac), (b.layout_hess, b.tried_hess)))
            assert max(lds_jac, lds_hess) > WS_SWITCH, c.id      # (what the launches would need in LDS)
            continue
        assert max(b.bytes_jac, b.bytes_hess) <= WS_SWITCH, c.id
        for cj, tried, layout, limit in ((b.cj_jac, b.tried_jac, b.layout_jac, b.limits[0]), (b.cj_hess, b.tried_hess, b.layout_hess, b.limits[1])):
            assert tried[0] == max(c.m, 1) and tried[-1] == cj and all(y == (x + 1) // 2 for x, y in zip(tried, tried[1:])), c.id
            assert all(layout(x) * 8 > limit for x in tried[:-1]) and (layout(cj) * 8 <= limit or cj == 1), (c.id, tried)


def test_cases_reach_every_form(driver_table, oracle):
    """What the case lists reach, by the restated budget (which test_the_restated_budget_equals_the_library ties to the library), against
    the forms of the module docstring written out."""
    assert len(BY_ID) == len(EVERY_CASE)
    forms, classes, pairs, counts, plan, gws_m = {}, {}, {False: set(), True: set()}, {}, set(), {"pade": set(), "exp": set()}
    for c in EVERY_CASE:
        b = c.budget(oracle)
        launches = [(f"{c.integ}-hess", b.cj_hess, b.bytes_hess)] + ([] if c.jac else [(f"{c.integ}-jac", b.cj_jac, b.bytes_jac)])
        for kernel, cj, nbytes in launches:
            forms.setdefault((kernel, b.use_ws), set()).add(chunk_form(c.m, cj))
            counts.setdefault(kernel, set()).add(c.n_int)
            if not b.use_ws:
                classes.setdefault(kernel, set()).add(lds_class(nbytes))
            if c.kernel == "auto":
                plan.add((kernel, b.use_ws))
        if c.integ == "pade" and c.m:
            pairs[b.use_ws] |= pair_kinds(c.m, b.cj_hess)
        if b.use_ws:
            gws_m[c.integ].add(c.m if c.m <= 2 else "odd" if c.m % 2 else "even")
        big = max(b.bytes_jac, b.bytes_hess)
        assert c.n_int == (1 if c.id.endswith("-n1") else 13 if b.use_ws or big > 96 * KIB else 263), c.id
    kernels = [f"{i}-{k}" for i in ("pade", "exp") for k in ("jac", "hess")]
    assert forms == {(k, ws): ({"no drives", "one", "equal", "ragged"} if ws else {"one", "equal", "ragged", "ones"}) for k in kernels for ws in (False, True)}, forms
    every_pair = {(a, b) for a in ("full", "ragged") for b in ("full", "ragged")}
    assert pairs == {False: every_pair, True: every_pair}, pairs
    assert classes == {k: {"<= 64 KiB", "<= 96 KiB", "> 96 KiB"} for k in kernels}, classes
    assert counts == {k: {1, 13, 263} for k in kernels}, counts
    # the default plan (kernel = QC_KERNEL_AUTO) reaches every kernel in both scratch forms
    assert plan == {(k, ws) for k in kernels for ws in (False, True)}, plan
    assert gws_m == {"pade": {0, 1, 2, "odd", "even"}, "exp": {0, 1, 2, "odd", "even"}}, gws_m
    for integ, (largest, nbytes, neighbour) in LARGEST.items():
        lds = {c.id: max(c.budget(oracle).bytes_jac, c.budget(oracle).bytes_hess) for c in EVERY_CASE if c.integ == integ and not c.budget(oracle).use_ws}
        assert max(lds, key=lds.get) == largest and lds[largest] == nbytes and WS_SWITCH - 1024 < nbytes <= WS_SWITCH, (integ, lds[largest])
        a, b = BY_ID[largest], BY_ID[neighbour]
        assert b.budget(oracle).use_ws and (a.N, a.order, a.free) == (b.N, b.order, b.free) and (b.m - a.m, b.nc - a.nc) in ((1, 0), (0, 1)), integ
    assert [c.id for c in EVERY_CASE if c.budget(oracle).bytes_jac == 64 * KIB and not c.budget(oracle).use_ws] == ["p12-N12k7-m5"]
    variants = {(c.integ, c.free, c.herm, c.align, c.layout, c.ncol > 0) for c in EVERY_CASE if c.m}
    for integ in ("pade", "exp"):
        assert {(integ, False, True, 0, "standard", False), (integ, True, False, 0, "standard", False), (integ, True, True, 16, "standard", False),
                (integ, True, True, 0, "shuffled", False), (integ, True, True, 0, "standard", True)} <= variants, integ
    assert {c.order for c in PADE_CASES} == {2, 4, 6, 12, 20} and all(chunk_form(c.m, c.budget(oracle).cj_hess) in ("ragged", "ones")
                                                                         for c in PADE_CASES if c.order in (2, 20))
    for c in (BY_ID[i] for i in RELAUNCH):
        assert c.twice and c.n_int in (13, 263)
    assert {(BY_ID[i].integ, BY_ID[i].budget(oracle).use_ws) for i in RELAUNCH} == {(i, ws) for i in ("pade", "exp") for ws in (False, True)}
    assert SHARDS[0][0] == 0 and SHARDS[-1][1] == 13 and all(a[1] == b[0] for a, b in zip(SHARDS, SHARDS[1:]))
    assert len({b - a for a, b in SHARDS if a % 2}) == 2
    for nb in (1, 13, 263):
        assert sorted(xcd_remap(b, nb) for b in range(nb)) == list(range(nb))
    assert 263 & 7 == 7 and xcd_remap(1, 263) == 33 and xcd_remap(1, 13) == 2      # (block and workspace slot 1: interval 33 / 2)


def test_restated_rules_at_their_edges():
    assert [chunk_form(m, cj) for m, cj in ((0, 1), (1, 1), (5, 5), (5, 9), (9, 3), (9, 5), (13, 4), (9, 1), (2, 2), (4, 2), (5, 2))] == [
        "no drives", "one", "one", "one", "equal", "ragged", "ragged", "ones", "one", "equal", "ragged"]
    assert passes(13, 4) == [4, 4, 4, 1] and passes(33, 9) == [9, 9, 9, 6] and passes(0, 1) == [] and passes(9, 1) == [1] * 9
    assert passes_text(13, 4) == "3x4+1" and passes_text(9, 5) == "5+4" and passes_text(5, 1) == "5x1" and passes_text(3, 5) == "3" and passes_text(4, 4) == "4"
    assert pair_kinds(9, 3) == {("full", "full")} and pair_kinds(5, 9) == {("ragged", "ragged")} and len(pair_kinds(13, 4)) == 4
    assert halving(9, lambda cj: 1000 * cj, 8 * 4000) == (3, [9, 5, 3]) and halving(9, lambda cj: 10 ** 6, 1) == (1, [9, 5, 3, 2, 1]) and halving(0, lambda cj: 1, 64) == (1, [1])
    assert [lds_class(b) for b in (65536, 65537, 98304, 98305)] == ["<= 64 KiB", "<= 96 KiB", "<= 96 KiB", "> 96 KiB"]
    # the figures of the module docstring, from a bare description of the shape (zdim = s + 3 m + 1, two integrators of m rows)
    def shape(integ, N, m, nc=0, order=4):
        s = 2 * N * (nc or N)
        return budget(SimpleNamespace(integrator=0 if integ == "pade" else 1, n=2 * N, nc=nc or N, s=s, zdim=s + 3 * m + 1, ddim=s + 2 * m, order=order, m=m))
    got = {k: (b.bytes_jac, b.cj_jac, b.bytes_hess, b.cj_hess, b.use_ws) for k, b in {
        "p4-N12-m13": shape("pade", 12, 13), "p4-N19-m12": shape("pade", 19, 12), "p4-N19-m13": shape("pade", 19, 13),
        "p12-N12k7-m5": shape("pade", 12, 5, 7, 12), "e-N8-m13": shape("exp", 8, 13), "e-N17-m5": shape("exp", 17, 5)}.items()}
    assert got == {"p4-N12-m13": (65152, 7, 94368, 4, False), "p4-N19-m12": (93024, 1, 163680, 1, False), "p4-N19-m13": (104608, 2, 187040, 2, True),
                   "p12-N12k7-m5": (65536, 1, 109408, 1, False), "e-N8-m13": (61184, 7, 50624, 2, False), "e-N17-m5": (134480, 2, 226832, 2, True)}, got
    assert shape("pade", 19, 13).ws_stride == 187040 // 8 and shape("exp", 8, 13).jchunk == 13 and shape("exp", 16, 5).jchunk == 1


def same_bits(got, want, what):
    """The bitwise checks of this file: the second launches, the shards."""
    got, want = np.ascontiguousarray(got).view(np.uint64), np.ascontiguousarray(want).view(np.uint64)
    assert got.shape == want.shape, what
    assert np.array_equal(got, want), f"{what}: {(got != want).sum()} values differ in their bits, first at {np.flatnonzero(got != want)[:5]}"


@pytest.mark.parametrize("big", [BIG, 1 << 12], ids=["whole", "slices"])
@pytest.mark.parametrize("case", MUTATION_CASES, ids=ids(MUTATION_CASES))
def test_the_checker_rejects_defective_vectors(oracle, coracle, monkeypatch, case, big):
    """The C oracle's own dF and mu_d2F of one chunked case per integrator (F + dF 17+16 / 7+6, mu_d2F 9+9+9+6 / 6x2+1) pass compare() with
    the suite's tolerances, whole and in slices of intervals; each of these defects does not: the d/da_j blocks (dF) and the (U_t, a_j)
    blocks (mu_d2F) of the last, ragged chunk zeroed; the same blocks holding the previous chunk's; one (a_i, a_j) entry of a (full,
    ragged) pair of chunks exchanged with the entry at the transposed place inside the pair's block -- (i0 + jj, j0 + ii) for (i0 + ii,
    j0 + jj), what `pr % jc`, `pr / jc` for `pr % ic`, `pr / ic` would do; S_ij exchanged with its mirror S_ji of the (ragged, full) pair
    is no defect of the values: the kernel stores S_ij + S_ji --; one interval holding the block of the one before.  One value off in
    the last bit passes the tolerances, as it must, and is rejected by same_bits."""
    monkeypatch.setattr(torch.cuda, "synchronize", lambda: None)
    monkeypatch.setattr(forms4, "BIG", big)
    prob, Z = case.problem(oracle)
    b = budget(prob)
    assert not b.use_ws and chunk_form(case.m, b.cj_jac) == chunk_form(case.m, b.cj_hess) == "ragged"
    ref = coracle.COracle(prob)
    n_int, m = case.n_int, prob.m
    mu = np.random.default_rng(5).standard_normal(prob.n_rows)
    refs = {"dF": (lambda a, b: ref.F_dF(Z, a, b, False, True)[1], assert_close), "mu_d2F": (lambda a, b: ref.mu_d2F(Z, mu, a, b), assert_close_h)}
    jac_rc = np.array(oracle.jac_structure_local(prob))
    hess_rc = np.array(oracle.hess_structure_local(prob))

    def check(which, V):
        return compare(HostVector(V.reshape(-1)), n_int, *refs[which], f"{case.id}: {which}")[0]

    caught = []
    for which, cj in (("dF", b.cj_jac), ("mu_d2F", b.cj_hess)):
        good = refs[which][0](0, n_int).reshape(n_int, -1)
        assert check(which, good) == 0.0
        if which == "dF":      # the entries of d/da_j in the rows of the states
            block = lambda j: np.flatnonzero((jac_rc[:, 1] == prob.off_a + j) & (jac_rc[:, 0] < prob.s))
        else:                  # the entries (U_t, a_j)
            block = lambda j: np.flatnonzero((hess_rc[:, 1] == prob.off_a + j) & (hess_rc[:, 0] >= prob.off_U) & (hess_rc[:, 0] < prob.off_U + prob.s))
        ps = passes(m, cj)
        j0 = m - ps[-1]
        last = np.concatenate([block(j) for j in range(j0, m)])
        before = np.concatenate([block(j - cj) for j in range(j0, m)])
        assert ps[-1] < cj and last.size == before.size == ps[-1] * prob.s and np.abs(good[:, last]).max() > 0

        def zeroed(V):
            V[:, last] = 0.0

        def previous(V):
            V[:, last] = V[:, before]

        def shifted(V):
            V[n_int // 2] = V[n_int // 2 - 1]

        defects = {"the last chunk's blocks zeroed": zeroed, "the last chunk's blocks hold the chunk's before": previous, "an interval holds the one before": shifted}
        if which == "mu_d2F":
            ii, jj = 1, 3      # i-chunk 0 (full), the last j-chunk (ragged): entry (ii, j0 + jj) against (jj, j0 + ii)
            assert ps[-1] > max(ii, jj) or case.integ == "exp"
            if ps[-1] > max(ii, jj):
                at = lambda i, j: int(np.flatnonzero((hess_rc[:, 0] == prob.off_a + i) & (hess_rc[:, 1] == prob.off_a + j))[0])
                e1, e2 = at(ii, j0 + jj), at(jj, j0 + ii)

                def exchanged(V):
                    V[:, [e1, e2]] = V[:, [e2, e1]]
                defects["an (a_i, a_j) entry at the transposed place of its chunk pair"] = exchanged
        for name, apply in defects.items():
            V = good.copy()
            apply(V)
            assert not np.array_equal(V, good), (which, name)
            with pytest.raises(AssertionError):
                check(which, V)
            caught.append(f"{which}: {name}")
        V = good.copy()
        k = int(np.argmax(np.abs(V[n_int - 1])))
        V[n_int - 1, k] = np.nextafter(V[n_int - 1, k], np.inf)
        assert 0.0 < check(which, V) < 1e-15
        same_bits(good, good.copy(), which)
        with pytest.raises(AssertionError):
            same_bits(V, good, which)
        caught.append(f"{which}: one value off in the last bit (same_bits)")
    case._problem = None
    print(f"{TAG} {case.id} ({'whole vectors' if big == BIG else 'slices of intervals'}): rejected -- {'; '.join(caught)}")


# ------------------------------------------------------------------------------------------------
#  On the device
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", EVERY_CASE, ids=ids(EVERY_CASE))
def test_every_value(qc, oracle, coracle, case):
    """F + dF, F alone (the bits of the F of F + dF) and mu_d2F of one case, every value against the C oracle; the kernel names and the
    scratch form the case was written for."""
    case._oracle = oracle
    b = case.budget(oracle)
    jac, hess, _ = case.names(oracle)
    assert "gws" in hess if b.use_ws else "gws" not in hess
    assert jac == case.jac if case.jac else jac == ("lds-gws" if b.use_ws else "lds")
    check_case(qc, oracle, coracle, case, make=make, twice=case.twice, form=form_text, tag=TAG)


def launch(L, h, dims, pZ, pmu, what, with_hess=True):
    """(F, dF, mu_d2F) of one handle into fresh NaN-filled vectors between guard margins: F + dF first, then mu_d2F."""
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    F, J, H = Guarded(dims.F_len), Guarded(dims.jac_nnz), Guarded(dims.hess_nnz)
    L.check(L.lib.qc_eval_F_jac_dev(h, pZ, F.ptr(), J.ptr(), st), h)
    if with_hess:
        L.check(L.lib.qc_eval_hess_dev(h, pZ, pmu, H.ptr(), st), h)
    return F.result(what + ": F"), J.result(what + ": dF"), H.result(what + ": mu_d2F") if with_hess else None


@pytest.mark.gpu
@pytest.mark.parametrize("tag", RELAUNCH)
def test_second_launches_and_shards(qc, oracle, coracle, tag):
    """F + dF, mu_d2F, F + dF, mu_d2F on one handle: the second F + dF launch finds the scratch (LDS, or its workspace slots) as mu_d2F
    left it and gives the bits of the first, as does the second mu_d2F.  Knot shards of the same trajectory (t_range; 1, 3, 1 and 8
    intervals, two of them from an odd first interval) concatenate to the full launch bit for bit; the full launch against the oracle."""
    full = BY_ID[tag]
    case = Case(tag + "-n13", full.integ, full.N, full.m, 13, ncol=full.ncol, order=full.order, kernel=full.kernel)
    prob, Z = case.problem(oracle)
    b = budget(prob)
    assert b.use_ws == full.budget(oracle).use_ws
    L = qc._lib
    mu = np.random.default_rng(13).standard_normal(prob.n_rows)
    dZ, dmu = torch.from_numpy(Z).cuda(), torch.from_numpy(mu).cuda()
    pZ, pmu = C.c_void_p(dZ.data_ptr()), C.c_void_p(dmu.data_ptr())
    h = RawHandle(qc, prob, kernel=case.kernel)
    try:
        assert tuple(L.lib.qc_kernel_name(h.h, k).decode() for k in (0, 1)) == full.names(oracle)[:2]
        F, J, H = launch(L, h.h, h.dims, pZ, pmu, tag)
        F2, J2, H2 = launch(L, h.h, h.dims, pZ, pmu, tag + ", second launches")
    finally:
        h.close()
    ref = coracle.COracle(prob)
    Fr, Jr = ref.F_dF(Z)
    assert_close(F, Fr, tag + ": F")
    assert_close(J, Jr, tag + ": dF")
    assert_close_h(H, ref.mu_d2F(Z, mu), tag + ": mu_d2F")
    for got, want, what in ((F2, F, "F"), (J2, J, "dF"), (H2, H, "mu_d2F")):
        same_bits(got, want, f"{tag}: {what}, second launch")
    parts = []
    for a, e in SHARDS:
        hs = RawHandle(qc, prob, kernel=case.kernel, t_range=(a, e))
        try:
            assert hs.dims.n_intervals == e - a
            parts.append(launch(L, hs.h, hs.dims, pZ, pmu, f"{tag}: intervals {a} .. {e - 1}"))      # (the full multiplier vector: a shard reads its rows from t_begin on)
        finally:
            hs.close()
    for k, (want, what) in enumerate(((F, "F"), (J, "dF"), (H, "mu_d2F"))):
        same_bits(np.concatenate([p[k] for p in parts]), want, f"{tag}: {what}, shards {SHARDS}")
    print(f"{TAG} {tag}: 13 intervals, {'workspace' if b.use_ws else 'LDS'}: second F + dF and mu_d2F launches and the shards {SHARDS} give the bits of the first")
