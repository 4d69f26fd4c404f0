"""Lists of handles over one trajectory (sampling problems, direct sums) evaluated by ONE launch with gridDim.y = members, every block
reading its member's parameter block from device memory: qc_launch_mfma16_F_jac_batch (qc_mfma_kernels.hip: 4 drive-count classes x
masked / unmasked tile x with / without the Jacobian) and qc_launch_mfma16_hess_batch (qc_mfma_hess.hip: 4 classes x masked / unmasked x
the kernel for antisymmetric generators / the general one), launched from qc_eval_F_jac_dev_multi, qc_eval_hess_dev_multi and the
host-buffer Jacobian path (list_eval_landing).

Every case compares EVERY value with the CPU oracle of the list (the numpy oracle up to T = 12, its C restatement above; the suite's
tolerances as they stand: rtol 1e-10, atol 1e-12 x the largest entry for F and dF, 1e-11 x for mu_d2F), asks qc_debug_list_shares_launch
which path produced the values, and only then compares call forms bit for bit.  Output buffers are NaN-filled between two guard
margins of 64 doubles holding a fixed bit pattern: every value inside must come back finite, both margins untouched.

The batched launches are persistent beyond 1024 workgroups (F + dF, F alone: kMaxGrid, one interval per workgroup) and 4096 (mu_d2F),
read from the launchers as they stand; the long cases sit one and two intervals past whole trips of those grids (T = 1026, 2051: 1025
and 2050 intervals; T = 4098: 4097).

Which test reaches which of the 32 batched instantiations, derived from the launch code (drive-count class = the next even number
>= m, at least 2, at most 8; masked tile = fewer than 8 levels or kets; without the Jacobian = dvals NULL; the general mu_d2F kernel =
handles created under QC_NO_ANTISYM=1), as ids of test_every_instantiation_short[N-m-free-...]:
  qc_mfma16_pade4_kernel<JAC = true (the calls with dF) and false (F alone), 2, kMU, KET, BATCH = true>
      unmasked, kMU = 2 / 4 / 6 / 8:   [8-2-free-created]  [8-4-free-created]  [8-6-free-created]  [8-8-free-created]
      masked,   kMU = 2 / 4 / 6 / 8:   [5-2-free-created]  [5-3-free-created]  [5-6-free-created]  [5-8-free-created]
  qc_mfma16_pade4_hess_anti_kernel<kHM, KET, BATCH = true, ONCE = false>: the same eight ids
  qc_mfma16_pade4_hess_kernel<kHM, KET, BATCH = true>: the same eight with `no_antisym` in place of `created`
The later trips of the persistent loops: test_persistent_trips, test_first_interval_past_the_hessian_grid."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle_bridge import composed_c_oracle, composed_oracle
from test_gpu_parity import assert_close, assert_close_h

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F_JAC, HESS, LANDING = 0, 1, 2          # qc_debug_list_shares_launch's `what`
GUARD = 64
PATTERN = 0x7FF4C0DEC0DEC0DE            # (a signalling NaN's bits: a kernel that READ a margin would show it as well)
GATE = {1: "H", 2: "CNOT", 3: "TOFFOLI"}


# ------------------------------------------------------------------------------------------------
#  Helpers
# ------------------------------------------------------------------------------------------------
class Guarded:
    """An output vector of n doubles on the device, NaN-filled (or zeroed), between two margins of GUARD doubles of PATTERN."""

    def __init__(self, n, fill=float("nan")):
        self.n = int(n)
        self.all = torch.empty(self.n + 2 * GUARD, dtype=torch.float64, device="cuda")
        self.all.view(torch.int64).fill_(PATTERN)
        self.t = self.all[GUARD:GUARD + self.n]
        self.t.fill_(fill)

    def ptr(self):
        return C.c_void_p(self.t.data_ptr())

    def result(self, what, finite=True):
        torch.cuda.synchronize()
        a = self.all.cpu().numpy()
        bits = a.view(np.uint64)
        assert (bits[:GUARD] == PATTERN).all(), f"{what}: the margin in front of the vector was written"
        assert (bits[GUARD + self.n:] == PATTERN).all(), f"{what}: the margin behind the vector was written"
        out = a[GUARD:GUARD + self.n].copy()
        if finite:
            bad = np.flatnonzero(~np.isfinite(out))
            assert bad.size == 0, f"{what}: {bad.size} values not written or not finite, first at {bad[:5]}"
        return out


class DeviceList:
    """The "_dev_multi" entry points (and one call per member) on a list of handles sharing the placement `dims` describes."""

    def __init__(self, qc, handles, dims, Z, mu):
        self.L = qc._lib
        self.hs = list(handles)
        self.arr = (C.c_void_p * len(self.hs))(*self.hs)
        self.lens = (int(dims.F_len), int(dims.jac_nnz), int(dims.hess_nnz))
        self.Z = torch.from_numpy(np.array(Z, dtype=np.float64)).cuda()
        self.mu = torch.from_numpy(np.array(mu, dtype=np.float64)).cuda()
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def shares(self, what):
        return self.L.lib.qc_debug_list_shares_launch(self.arr, len(self.hs), what)

    def F_dF(self, want_F=True, want_J=True, per_member=False, finite=True, what=""):
        F = Guarded(self.lens[0]) if want_F else None
        J = Guarded(self.lens[1]) if want_J else None
        pF, pJ = (F.ptr() if F else None), (J.ptr() if J else None)
        if per_member:
            for h in self.hs:
                self.L.check(self.L.lib.qc_eval_F_jac_dev(h, C.c_void_p(self.Z.data_ptr()), pF, pJ, self.stream), h)
        else:
            self.L.check(self.L.lib.qc_eval_F_jac_dev_multi(self.arr, len(self.hs), C.c_void_p(self.Z.data_ptr()), pF, pJ, self.stream), self.hs[0])
        return (F.result(what + " F", finite) if F else None), (J.result(what + " dF", finite) if J else None)

    def hess(self, per_member=False, finite=True, what=""):
        H = Guarded(self.lens[2])
        args = (C.c_void_p(self.Z.data_ptr()), C.c_void_p(self.mu.data_ptr()), H.ptr(), self.stream)
        if per_member:
            for h in self.hs:
                self.L.check(self.L.lib.qc_eval_hess_dev(h, *args), h)
        else:
            self.L.check(self.L.lib.qc_eval_hess_dev_multi(self.arr, len(self.hs), *args), self.hs[0])
        return H.result(what + " mu_d2F", finite)


def handles_of(dyn):
    return [p[2] for p in dyn._parts]


def reference(inp, Z, mu, hess, t_range=None, want_J=True):
    """(F, dF, mu_d2F) of the list: the numpy oracle up to T = 12, the C oracle above; `t_range`: the intervals of a shard."""
    T = inp.traj.T
    t0, t1 = t_range if t_range else (0, T - 1)
    if T <= 12:
        ref = composed_oracle(inp)
        cut = lambda v: v.reshape(T - 1, -1)[t0:t1].reshape(-1)
        return cut(ref.F(Z)), cut(ref.dF(Z)) if want_J else None, cut(ref.mu_d2F(Z, mu)) if hess else None
    ref = composed_c_oracle(inp)
    F, J = ref.F_dF(Z, t0, t1, True, want_J)
    return F, J, ref.mu_d2F(Z, mu, t0, t1) if hess else None


def hermitian_systems(qc, N, m, K, seed):
    """K systems of N levels: a drift of its own each, the m drives shared."""
    rng = np.random.default_rng(seed)

    def herm():
        A = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
        return (A + A.conj().T) / 2

    drives = [herm() for _ in range(m)]
    return [qc.QuantumSystem(herm(), drives) for _ in range(K)]


def sampling_list(qc, N, m, K, T, free_time=True, seed=0):
    """unitary_sampling_inputs over K random Hermitian systems of N levels.  Without drives the template's two derivative integrators
    have no components and no rows; the library refuses an integrator of dimension 0, so the list goes without them (the same rows)."""
    inp = qc.unitary_sampling_inputs(hermitian_systems(qc, N, m, K, seed), random_unitary(N, N), T, free_time=free_time)
    if m == 0:
        inp.integrators = [I for I in inp.integrators if not isinstance(I, qc.DerivativeIntegrator)]
    return inp


def random_unitary(N, seed):
    rng = np.random.default_rng(seed)
    Q, R = np.linalg.qr(rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N)))
    return Q * (np.diag(R) / np.abs(np.diag(R)))


def qubit_systems(qc, nq, K, drives=None, seed=5):
    rng = np.random.default_rng(seed)
    base = qc.multi_qubit_system(nq)
    Hd = base.H_drives if drives is None else base.H_drives[:drives]
    return [qc.QuantumSystem(base.H_drift * (1.0 + 0.1 * rng.standard_normal()), Hd) for _ in range(K)]


def point(inp, dyn, seed, noise=0.0):
    rng = np.random.default_rng(seed)
    Z = np.array(inp.traj.datavec, dtype=np.float64)
    if noise:
        Z = Z + noise * rng.standard_normal(Z.size)
    return Z, rng.standard_normal(int(dyn.dims.n_rows))


def check_every_call_form(qc, dyn, inp, Z, mu, what, shares_hess=None, t_range=None):
    """The four device calls against the oracle, the shared-launch query, then the call forms against each other bit for bit."""
    hess = int(dyn.dims.hess_nnz) > 0
    dl = DeviceList(qc, handles_of(dyn), dyn.dims, Z, mu)
    assert dl.shares(F_JAC) == 1, what
    assert dl.shares(HESS) == int(hess if shares_hess is None else shares_hess), what
    Fr, Jr, Hr = reference(inp, Z, mu, hess, t_range)
    F, J = dl.F_dF(what=what + ", F with dF")
    assert_close(F, Fr, what + ": F")
    assert_close(J, Jr, what + ": dF")
    F1, _ = dl.F_dF(want_J=False, what=what + ", F alone")
    assert_close(F1, Fr, what + ": F alone")
    _, J1 = dl.F_dF(want_F=False, what=what + ", dF alone")
    assert_close(J1, Jr, what + ": dF alone")
    if hess:
        H = dl.hess(what=what)
        assert_close_h(H, Hr, what + ": mu_d2F")
        assert np.array_equal(dl.hess(what=what + ", again"), H), what + ": mu_d2F, a second call"
    # (each of these arrays has just been compared with the oracle; F + dF took one launch, says the query)
    Fm, Jm = dl.F_dF(per_member=True, what=what + ", one call per member")
    assert_close(Fm, Fr, what + ": F, one call per member")
    assert_close(Jm, Jr, what + ": dF, one call per member")
    F2, J2 = dl.F_dF(what=what + ", again")
    for name, a, b in (("F alone", F1, F), ("dF alone", J1, J), ("F per member", Fm, F), ("dF per member", Jm, J), ("F again", F2, F), ("dF again", J2, J)):
        assert np.array_equal(a, b), f"{what}: {name} differs in {(a != b).sum()} values, first at {np.flatnonzero(a != b)[:5]}"
    return dl


# ------------------------------------------------------------------------------------------------
#  A. Every instantiation, short
# ------------------------------------------------------------------------------------------------
SHORT = [(8, m) for m in range(9)] + [(N, m) for N in (5, 2) for m in (0, 2, 3, 6, 7, 8)]


@pytest.mark.parametrize("antisym", ["created", "no_antisym"])
@pytest.mark.parametrize("free_time", [True, False], ids=["free", "fixed"])
@pytest.mark.parametrize("N,m", SHORT)
def test_every_instantiation_short(qc, monkeypatch, N, m, free_time, antisym):
    if antisym == "no_antisym":
        monkeypatch.setenv("QC_NO_ANTISYM", "1")      # read whenever a handle is created: the general mu_d2F kernel
    inp = sampling_list(qc, N, m, 3, 5, free_time, seed=100 * N + m)
    dyn = qc.QuantumDynamics(inp.integrators, inp.traj)
    try:
        assert isinstance(dyn, qc.ComposedQuantumDynamics) and len(dyn._parts) == 3 and dyn.kernel == "mfma+mfma+mfma"
        assert (int(dyn.dims.hess_nnz) > 0) == (m > 0 or free_time)
        Z, mu = point(inp, dyn, m)
        check_every_call_form(qc, dyn, inp, Z, mu, f"N={N} m={m} {'free' if free_time else 'fixed'} {antisym}")
    finally:
        dyn.close()


@pytest.mark.parametrize("antisym", ["created", "no_antisym"])
@pytest.mark.parametrize("nq,kets", [(3, 1), (3, 3), (3, 7), (2, 3)])
def test_ket_lists_short(qc, monkeypatch, nq, kets, antisym):
    if antisym == "no_antisym":
        monkeypatch.setenv("QC_NO_ANTISYM", "1")
    rng = np.random.default_rng(kets)
    N = 2 ** nq
    psis = [rng.standard_normal(N) + 1j * rng.standard_normal(N) for _ in range(2 * kets)]
    psis = [p / np.linalg.norm(p) for p in psis]
    inp = qc.quantum_state_sampling_inputs(qubit_systems(qc, nq, 2), psis[:kets], psis[kets:], 5)
    dyn = qc.QuantumDynamics(inp.integrators, inp.traj)
    try:
        assert isinstance(dyn, qc.ComposedQuantumDynamics) and len(dyn._parts) == 2
        Z, mu = point(inp, dyn, kets)
        check_every_call_form(qc, dyn, inp, Z, mu, f"{nq} qubits, {kets} kets, {antisym}")
    finally:
        dyn.close()


# ------------------------------------------------------------------------------------------------
#  B. More drives than the registers of mu_d2F hold
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,m", [(8, 9), (8, 32), (2, 9), (2, 32)])
def test_more_drives_than_the_hessian_kernel_holds(qc, N, m):
    inp = sampling_list(qc, N, m, 2, 5, seed=N + m)
    dyn = qc.QuantumDynamics(inp.integrators, inp.traj)
    try:
        Z, mu = point(inp, dyn, m)
        # F + dF in one launch (drive images beyond the eighth from memory); mu_d2F member by member (the LDS class' kernel)
        check_every_call_form(qc, dyn, inp, Z, mu, f"N={N} m={m}", shares_hess=False)
    finally:
        dyn.close()


# ------------------------------------------------------------------------------------------------
#  C. Second and third trip of the persistent loop
# ------------------------------------------------------------------------------------------------
def long_list(qc, nq, drives, T, free_time):
    K = 3 if nq == 1 else 2
    return qc.unitary_sampling_inputs(qubit_systems(qc, nq, K, drives), qc.GATES[GATE[nq]], T, free_time=free_time)


_long_refs = {}


def long_case(qc, nq):
    """The sampling lists at T = 1026, free timestep, with their oracle values: shared by the device and the host-buffer tests."""
    if nq not in _long_refs:
        inp = long_list(qc, nq, None, 1026, True)
        dyn = qc.QuantumDynamics(inp.integrators, inp.traj)
        Z, mu = point(inp, dyn, nq)
        dyn.close()
        ref = tuple(reference(inp, Z, mu, True))
        for a in ref + (Z, mu):
            a.setflags(write=False)
        _long_refs[nq] = (inp, Z, mu, ref)
    return _long_refs[nq]


@pytest.mark.parametrize("free_time", [True, False], ids=["free", "fixed"])
@pytest.mark.parametrize("nq,drives,T", [(1, None, 1026), (1, None, 2051), (2, None, 1026), (2, None, 2051), (3, 2, 1026), (3, 2, 2051), (3, 6, 1026)])
def test_persistent_trips(qc, nq, drives, T, free_time):
    """1025 and 2050 intervals: one workgroup past one trip and two past two trips of the 1024-workgroup grid of F + dF and F alone
    (kMaxGrid in qc_mfma_kernels.hip; one interval per workgroup) -- `vb += gridDim.x` under blockIdx.y, the XCD remap of the later
    trips, the barrier in front of the rewritten hand-off rows.  mu_d2F (grid of 4096) still takes one trip here."""
    if free_time and T == 1026 and drives in (None, 6):
        inp, Z, mu, (Fr, Jr, Hr) = long_case(qc, nq)
    else:
        inp = long_list(qc, nq, drives, T, free_time)
        Z = mu = None
    dyn = qc.QuantumDynamics(inp.integrators, inp.traj)
    try:
        if Z is None:
            Z, mu = point(inp, dyn, nq)
            Fr, Jr, Hr = reference(inp, Z, mu, True)
        what = f"{nq} qubits, {drives or 2 * nq} drives, T={T}"
        dl = DeviceList(qc, handles_of(dyn), dyn.dims, Z, mu)
        assert dl.shares(F_JAC) == 1 and dl.shares(HESS) == 1
        F, J = dl.F_dF(what=what)
        assert_close(F, Fr, what + ": F")
        assert_close(J, Jr, what + ": dF")
        F1, _ = dl.F_dF(want_J=False, what=what + ", F alone")
        assert_close(F1, Fr, what + ": F alone")
        assert_close_h(dl.hess(what=what), Hr, what + ": mu_d2F")
        assert np.array_equal(F1, F), what + ": F alone against F with dF (both compared with the oracle above)"
    finally:
        dyn.close()


@pytest.mark.parametrize("free_time", [True, False], ids=["free", "fixed"])
@pytest.mark.parametrize("nq,drives", [(1, None), (2, None), (3, 2)])
def test_first_interval_past_the_hessian_grid(qc, nq, drives, free_time):
    """4097 intervals: the first one past the 4096-workgroup grid of the batched mu_d2F launch (qc_launch_mfma16_hess_batch), and the
    fifth trip of F alone.  dF as well for the one- and two-qubit lists (the three-qubit list's value array is left out for its size)."""
    inp = long_list(qc, nq, drives, 4098, free_time)
    dyn = qc.QuantumDynamics(inp.integrators, inp.traj)
    try:
        Z, mu = point(inp, dyn, nq)
        want_J = nq < 3
        Fr, Jr, Hr = reference(inp, Z, mu, True, want_J=want_J)
        what = f"{nq} qubits, T=4098"
        dl = DeviceList(qc, handles_of(dyn), dyn.dims, Z, mu)
        assert dl.shares(F_JAC) == 1 and dl.shares(HESS) == 1
        assert_close_h(dl.hess(what=what), Hr, what + ": mu_d2F")
        F1, _ = dl.F_dF(want_J=False, what=what + ", F alone")
        assert_close(F1, Fr, what + ": F alone")
        if want_J:
            F, J = dl.F_dF(what=what)
            assert_close(F, Fr, what + ": F")
            assert_close(J, Jr, what + ": dF")
    finally:
        dyn.close()


def test_persistent_trips_away_from_the_initial_guess(qc):
    """Every component of the knots moved by 1e-2 noise (controls and timesteps too), two qubits, T = 1026."""
    inp = long_list(qc, 2, None, 1026, True)
    dyn = qc.QuantumDynamics(inp.integrators, inp.traj)
    try:
        Z, mu = point(inp, dyn, 7, noise=1e-2)
        check_every_call_form(qc, dyn, inp, Z, mu, "two qubits, T=1026, noise")
    finally:
        dyn.close()


# ------------------------------------------------------------------------------------------------
#  D. Shards
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [2, 3])
def test_shard_of_a_list(qc, nq):
    """Intervals [3, 9) of T = 12: the outputs are the shard's intervals, mu is the full-length vector."""
    inp = qc.unitary_sampling_inputs(qubit_systems(qc, nq, 2), qc.GATES[GATE[nq]], 12)
    dyn = qc.ComposedQuantumDynamics(inp.integrators, inp.traj, t_range=(3, 9))
    try:
        assert int(dyn.dims.n_intervals) == 6 and int(dyn.dims.n_rows) == 11 * dyn.dim and int(dyn.dims.F_len) == 6 * dyn.dim
        Z, mu = point(inp, dyn, nq)
        check_every_call_form(qc, dyn, inp, Z, mu, f"{nq} qubits, intervals 3 .. 8", t_range=(3, 9))
    finally:
        dyn.close()


# ------------------------------------------------------------------------------------------------
#  E. Direct sums
# ------------------------------------------------------------------------------------------------
def direct_sum(qc, nqs, T):
    parts = []
    for k, nq in enumerate(nqs):
        base = qc.multi_qubit_system(nq)
        system = qc.QuantumSystem(base.H_drift * (1.0 + 0.05 * k), base.H_drives)
        parts.append(qc.unitary_smooth_pulse_inputs(system, qc.GATES[GATE[nq]], T, seed=11 + k))
    return qc.unitary_direct_sum_inputs(parts)


@pytest.mark.parametrize("T", [6, 1026])
@pytest.mark.parametrize("members", [2, 3])
def test_direct_sum_of_equal_members(qc, members, T):
    """Every member with controls and derivative integrators of its own; equal shapes: one launch."""
    inp = direct_sum(qc, [2] * members, T)
    dyn = qc.QuantumDynamics(inp.integrators, inp.traj)
    try:
        assert len(dyn._parts) == members
        Z, mu = point(inp, dyn, members)
        check_every_call_form(qc, dyn, inp, Z, mu, f"direct sum of {members}, T={T}")
    finally:
        dyn.close()


def test_direct_sum_of_unequal_members(qc):
    """A six-drive member (three qubits) beside a four-drive member (two qubits): one launch each, the same values."""
    inp = direct_sum(qc, [3, 2], 6)
    dyn = qc.QuantumDynamics(inp.integrators, inp.traj)
    try:
        Z, mu = point(inp, dyn, 1)
        dl = DeviceList(qc, handles_of(dyn), dyn.dims, Z, mu)
        assert dl.shares(F_JAC) == 0 and dl.shares(HESS) == 0 and dl.shares(LANDING) == 0
        Fr, Jr, Hr = reference(inp, Z, mu, True)
        F, J = dl.F_dF(what="unequal members")
        assert_close(F, Fr, "unequal members: F")
        assert_close(J, Jr, "unequal members: dF")
        assert_close_h(dl.hess(what="unequal members"), Hr, "unequal members: mu_d2F")
    finally:
        dyn.close()


# ------------------------------------------------------------------------------------------------
#  F. Lists that must not share a launch, and still be right
# ------------------------------------------------------------------------------------------------
def member_columns(dyn, i):
    """Columns of member i inside an interval's residual rows, Jacobian values and Hessian values."""
    desc, _, _, dims = dyn._parts[i]
    return (slice(int(desc.row_offset), int(desc.row_offset) + int(dims.ddim)),
            slice(int(desc.jac_offset), int(desc.jac_offset) + int(dims.jac_nnz_interval)),
            slice(int(desc.hess_offset), int(desc.hess_offset) + int(dims.hess_nnz_interval)))


def check_members(dl, dyn, present, refs, what):
    """The list `dl` holds the members `present` (index -> the reference triple its values must match) of dyn's placement: their
    columns against the oracle, every other column untouched (still NaN)."""
    n_int = int(dyn.dims.n_intervals)
    F, J = dl.F_dF(finite=False, what=what)
    H = dl.hess(finite=False, what=what)
    for k, (got, width) in enumerate(((F, dyn.dim), (J, int(dyn.dims.jac_nnz_interval)), (H, int(dyn.dims.hess_nnz_interval)))):
        got = got.reshape(n_int, width)
        absent = np.ones(width, dtype=bool)
        for i in range(len(dyn._parts)):
            if i not in present:
                continue
            cols = member_columns(dyn, i)[k]
            absent[cols] = False
            want = refs[present[i]][k].reshape(n_int, width)[:, cols]
            (assert_close_h if k == 2 else assert_close)(got[:, cols], want, f"{what}: member {i}, {'F dF mu_d2F'.split()[k]}")
        assert np.isnan(got[:, absent]).all(), f"{what}: values of an absent member were written ({'F dF mu_d2F'.split()[k]})"
    return F, J, H


@pytest.mark.parametrize("other", ["no_antisym", "lds"])
def test_members_that_differ_in_kind_do_not_share(qc, monkeypatch, other):
    """Member 0 of one evaluator and member 1 of another over the same inputs (the same placement), passed as one array."""
    inp = qc.unitary_sampling_inputs(qubit_systems(qc, 2, 2), qc.GATES["CNOT"], 9)
    dyn_a = qc.QuantumDynamics(inp.integrators, inp.traj)
    if other == "no_antisym":
        monkeypatch.setenv("QC_NO_ANTISYM", "1")
    dyn_b = qc.QuantumDynamics(inp.integrators, inp.traj, kernel="lds" if other == "lds" else "auto")
    monkeypatch.delenv("QC_NO_ANTISYM", raising=False)
    try:
        Z, mu = point(inp, dyn_a, 3)
        dl = DeviceList(qc, [handles_of(dyn_a)[0], handles_of(dyn_b)[1]], dyn_a.dims, Z, mu)
        # generators read as not antisymmetric: another mu_d2F kernel, the same F + dF kernel; the LDS class joins no batched launch
        assert (dl.shares(F_JAC), dl.shares(HESS)) == ((1, 0) if other == "no_antisym" else (0, 0))
        check_members(dl, dyn_a, {0: 0, 1: 0}, [reference(inp, Z, mu, True)], other)
        both = DeviceList(qc, handles_of(dyn_a), dyn_a.dims, Z, mu)
        assert (both.shares(F_JAC), both.shares(HESS)) == (1, 1)
    finally:
        dyn_a.close()
        dyn_b.close()


def test_exponential_members_do_not_share(qc):
    inp = qc.unitary_sampling_inputs(qubit_systems(qc, 2, 3), qc.GATES["CNOT"], 9, integrator="exponential")
    dyn = qc.QuantumDynamics(inp.integrators, inp.traj)
    try:
        Z, mu = point(inp, dyn, 4)
        dl = DeviceList(qc, handles_of(dyn), dyn.dims, Z, mu)
        assert (dl.shares(F_JAC), dl.shares(HESS), dl.shares(LANDING)) == (0, 0, 0)
        check_members(dl, dyn, {0: 0, 1: 0, 2: 0}, [reference(inp, Z, mu, True)], "exponential members")
    finally:
        dyn.close()


def test_a_list_of_one_member_does_not_share(qc):
    inp = qc.unitary_sampling_inputs(qubit_systems(qc, 3, 2), qc.GATES["TOFFOLI"], 7)
    dyn = qc.QuantumDynamics(inp.integrators, inp.traj)
    try:
        Z, mu = point(inp, dyn, 5)
        refs = [reference(inp, Z, mu, True)]
        for i in (0, 1):
            dl = DeviceList(qc, [handles_of(dyn)[i]], dyn.dims, Z, mu)
            assert (dl.shares(F_JAC), dl.shares(HESS), dl.shares(LANDING)) == (0, 0, 0)
            check_members(dl, dyn, {i: 0}, refs, f"member {i} alone")
    finally:
        dyn.close()


def test_the_query_refuses_what_the_entry_points_refuse(qc):
    L = qc._lib
    assert L.lib.qc_debug_list_shares_launch(None, 0, F_JAC) == L.QC_ERR_INVALID
    inp = qc.unitary_sampling_inputs(qubit_systems(qc, 1, 2), qc.GATES["H"], 4)
    dyn = qc.QuantumDynamics(inp.integrators, inp.traj)
    try:
        arr = (C.c_void_p * 2)(handles_of(dyn)[0], None)
        for what in (F_JAC, HESS, LANDING):
            assert L.lib.qc_debug_list_shares_launch(arr, 2, what) == L.QC_ERR_INVALID
        assert L.lib.qc_debug_list_shares_launch(dyn._handles, 2, 3) == L.QC_ERR_INVALID
        assert [L.lib.qc_debug_list_shares_launch(dyn._handles, 2, w) for w in (F_JAC, HESS, LANDING)] == [1, 1, 1]
    finally:
        dyn.close()


# ------------------------------------------------------------------------------------------------
#  G. The leader's cache of its members' parameter blocks
# ------------------------------------------------------------------------------------------------
def test_the_leader_notices_a_changed_member_set(qc):
    """One leader, five lists in a row: the members reordered, one left out, all again, one destroyed and created again over another
    drift (its address may be recycled: the cache compares serial numbers).  Every result against the oracle of the list as it then is."""
    systems = qubit_systems(qc, 2, 3)
    inp = qc.unitary_sampling_inputs(systems, qc.GATES["CNOT"], 8)
    other = qc.QuantumSystem(systems[1].H_drift * 1.7, systems[1].H_drives)
    inp2 = qc.unitary_sampling_inputs([systems[0], other, systems[2]], qc.GATES["CNOT"], 8)      # (the same seed: the same trajectory)
    assert np.array_equal(inp.traj.datavec, inp2.traj.datavec)
    dyn = qc.QuantumDynamics(inp.integrators, inp.traj)
    dyn2 = None
    try:
        Z, mu = point(inp, dyn, 6)
        refs = [reference(inp, Z, mu, True), reference(inp2, Z, mu, True)]
        assert not np.array_equal(refs[0][0], refs[1][0])
        h0, h1, h2 = handles_of(dyn)
        first = None
        for step, (hs, present) in enumerate([((h0, h1, h2), {0: 0, 1: 0, 2: 0}), ((h0, h2, h1), {0: 0, 1: 0, 2: 0}), ((h0, h1), {0: 0, 1: 0}),
                                              ((h0, h1, h2), {0: 0, 1: 0, 2: 0})]):
            dl = DeviceList(qc, hs, dyn.dims, Z, mu)
            assert (dl.shares(F_JAC), dl.shares(HESS)) == (1, 1)
            got = check_members(dl, dyn, present, refs, f"step {step + 1}")
            if step == 0:
                first = got
            elif step in (1, 3):      # the same members: the same values whatever their order (each compared with the oracle above)
                assert all(np.array_equal(a, b) for a, b in zip(got, first)), f"step {step + 1}"
        qc._lib.lib.qc_destroy(h1)
        dyn._parts[1] = (dyn._parts[1][0], dyn._parts[1][1], None, dyn._parts[1][3])
        dyn2 = qc.QuantumDynamics(inp2.integrators, inp2.traj)
        dl = DeviceList(qc, (h0, handles_of(dyn2)[1], h2), dyn.dims, Z, mu)
        assert (dl.shares(F_JAC), dl.shares(HESS)) == (1, 1)
        got = check_members(dl, dyn, {0: 0, 1: 1, 2: 0}, refs, "step 5")
        assert not np.array_equal(got[0], first[0])
    finally:
        dyn.close()
        if dyn2 is not None:
            dyn2.close()


# ------------------------------------------------------------------------------------------------
#  H. Host buffers
# ------------------------------------------------------------------------------------------------
CHILD = """
import sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import __graft_entry__ as g
from test_list_launch import long_list
qc = g.load_package()
out = sys.argv[2]
for nq in (1, 2, 3):
    inp = long_list(qc, nq, None, 1026, True)
    dyn = qc.QuantumDynamics(inp.integrators, inp.traj)
    Z, mu = np.load(f"{out}/Z{nq}.npy"), np.load(f"{out}/mu{nq}.npy")
    shares = qc._lib.lib.qc_debug_list_shares_launch(dyn._handles, len(dyn._parts), 2)
    F, J = dyn.F_dF(Z, fresh=True)
    np.save(f"{out}/child_F{nq}.npy", F)
    np.save(f"{out}/child_J{nq}.npy", J)
    np.save(f"{out}/child_J1{nq}.npy", dyn.dF(Z, fresh=True))
    np.save(f"{out}/child_F1{nq}.npy", dyn.F(Z, fresh=True))
    np.save(f"{out}/child_H{nq}.npy", dyn.mu_d2F(Z, mu, fresh=True))
    np.save(f"{out}/child_shares{nq}.npy", np.array([shares]))
    dyn.close()
"""


def test_host_buffer_calls_and_the_member_by_member_launches(qc, tmp_path):
    """dyn.F_dF / dF / F / mu_d2F on numpy arrays at T = 1026 (the landing path's batched launch takes its second trip), every value
    against the C oracle; a fresh process under QC_LIST_BATCH=0 launches member by member and delivers the same bits."""
    mine = {}
    for nq in (1, 2, 3):
        inp, Z, mu, (Fr, Jr, Hr) = long_case(qc, nq)
        dyn = qc.QuantumDynamics(inp.integrators, inp.traj)
        try:
            assert [qc._lib.lib.qc_debug_list_shares_launch(dyn._handles, len(dyn._parts), w) for w in (F_JAC, HESS, LANDING)] == [1, 1, 1]
            F, J = dyn.F_dF(Z, fresh=True)
            J1, F1, H = dyn.dF(Z, fresh=True), dyn.F(Z, fresh=True), dyn.mu_d2F(Z, mu, fresh=True)
            what = f"{nq} qubits, host buffers"
            assert_close(F, Fr, what + ": F")
            assert_close(J, Jr, what + ": dF")
            assert_close(J1, Jr, what + ": dF alone")
            assert_close(F1, Fr, what + ": F alone")
            assert_close_h(H, Hr, what + ": mu_d2F")
            mine[nq] = dict(F=F, J=J, J1=J1, F1=F1, H=H)
            np.save(tmp_path / f"Z{nq}.npy", Z)
            np.save(tmp_path / f"mu{nq}.npy", mu)
        finally:
            dyn.close()
    env = dict(os.environ, QC_LIST_BATCH="0")
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(tmp_path)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    for nq in (1, 2, 3):
        assert np.load(tmp_path / f"child_shares{nq}.npy")[0] == 0      # the child's values came from one launch per member
        for name, a in mine[nq].items():
            b = np.load(tmp_path / f"child_{name}{nq}.npy")
            assert np.array_equal(a, b), f"{nq} qubits, {name}: {(a != b).sum()} values differ from the member-by-member launches"
