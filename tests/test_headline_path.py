"""The 2N = 16 F + dF kernel (qc_mfma16_pade4_kernel) has a compile-time form, HEAD, for launches in which nothing is left to test at
run time: one interval per workgroup (at most 1024 intervals), m equal to the instantiation's drive count (m even), every copy of the
-F / B blocks (the device entry points), a free timestep, a derivative-integrator window, residuals wanted, exactly antisymmetric
generators.  Every other launch takes the run-time instantiations.  Here every value of F and dF against the C oracle at 1e-12, on
both sides of each of those conditions, and for every case a second handle created under QC_NO_HEAD=1 (the run-time form): the two
value vectors must be equal bit for bit.

Cases (device entry, all copies, unless said otherwise):
  config 3 at T = 2, 1000, 1025 (1, 999, 1024 intervals: loop-free, taken) and T = 1026 (1025 intervals: the persistent grid, not taken);
  m = 6 (taken), m = 5 (the kMU = 6 instantiation with m < kMU: not taken), m = 4 (kMU = 4, taken), m = 3 (not taken);
  a fixed timestep, no derivative integrator, a non-Hermitian drive: not taken;
  the host-buffer entry (one copy of the blocks: not taken) next to the device entry of the same handle;
  a three-shard handle (each shard's launch taken); the batched list launch of three systems (the BATCH instantiation: not taken)."""
import numpy as np
import pytest
import torch

from oracle_bridge import composed_oracle, problem_from_inputs
from test_gpu_parity import RawHandle
from test_passon_fetch import chain_problem, device_F_jac, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-12


def both_forms(monkeypatch, make):
    """make() -> (F, J) of a freshly created handle; once as created by default, once under QC_NO_HEAD=1."""
    out = []
    for flag in ("0", "1"):
        monkeypatch.setenv("QC_NO_HEAD", flag)
        out.append(make())
    monkeypatch.delenv("QC_NO_HEAD")
    (F, J), (F0, J0) = out
    assert np.array_equal(F, F0) and np.array_equal(J, J0), "HEAD and the run-time form differ"
    return F, J


def check_device_entry(qc, coracle, monkeypatch, prob, Z, what, host_entry=False):
    Fr, Jr = coracle.COracle(prob).F_dF(Z)

    def make():
        h = RawHandle(qc, prob, kernel="mfma")
        try:
            if host_entry:
                Fh, Jh = h.F_jac(Z)                   # the compact form: one copy of the blocks
                assert rel_err(Fh, Fr) < TOL and rel_err(Jh, Jr) < TOL, (what, "host entry", rel_err(Fh, Fr), rel_err(Jh, Jr))
            return device_F_jac(qc, h.h, h.dims, Z)   # every copy
        finally:
            h.close()

    F, J = both_forms(monkeypatch, make)
    assert rel_err(F, Fr) < TOL and rel_err(J, Jr) < TOL, (what, rel_err(F, Fr), rel_err(J, Jr))


@pytest.mark.parametrize("T", [2, 1000, 1025, 1026])
def test_config3_lengths(qc, coracle, monkeypatch, T):
    inp = qc.config_inputs(3, T=T)
    prob = problem_from_inputs(inp)
    Z = inp.traj.datavec + 1e-2 * np.random.default_rng(T).standard_normal(inp.traj.datavec.size)
    Fr, Jr = coracle.COracle(prob).F_dF(Z)

    def make():
        dyn = qc.QuantumDynamics(inp.integrators, inp.traj)
        try:
            dF = torch.full((int(dyn.dims.F_len),), float("nan"), dtype=torch.float64, device="cuda")
            dJ = torch.full((int(dyn.dims.jac_nnz),), float("nan"), dtype=torch.float64, device="cuda")
            dyn.F_dF_device(torch.from_numpy(Z).cuda(), dF, dJ)
            torch.cuda.synchronize()
            return dF.cpu().numpy(), dJ.cpu().numpy()
        finally:
            dyn.close()

    F, J = both_forms(monkeypatch, make)
    assert rel_err(F, Fr) < TOL and rel_err(J, Jr) < TOL, (T, rel_err(F, Fr), rel_err(J, Jr))


@pytest.mark.parametrize("m", [6, 5, 4, 3])
@pytest.mark.parametrize("T", [2, 300])
def test_drive_counts(qc, oracle, coracle, monkeypatch, m, T):
    prob, Z = chain_problem(oracle, N=8, m=m, T=T, n_deriv=2, free_time=True, pad=1, seed=m)
    check_device_entry(qc, coracle, monkeypatch, prob, Z, f"m={m} T={T}")


def test_fixed_timestep(qc, oracle, coracle, monkeypatch):
    prob, Z = chain_problem(oracle, N=8, m=6, T=300, n_deriv=2, free_time=False, pad=0, seed=21)
    check_device_entry(qc, coracle, monkeypatch, prob, Z, "fixed timestep")


def test_no_derivative_integrator(qc, oracle, coracle, monkeypatch):
    prob, Z = chain_problem(oracle, N=8, m=6, T=300, n_deriv=0, free_time=True, pad=0, seed=22)
    check_device_entry(qc, coracle, monkeypatch, prob, Z, "no derivative integrator")


def test_non_hermitian_drive(qc, oracle, coracle, monkeypatch):
    prob, Z = chain_problem(oracle, N=8, m=6, T=300, n_deriv=2, free_time=True, pad=0, seed=23)
    rng = np.random.default_rng(24)
    A = rng.standard_normal((8, 8)) + 1j * rng.standard_normal((8, 8))       # not Hermitian: its generator is not antisymmetric
    prob.G_drives[2] = oracle.generator(A)
    assert not np.array_equal(prob.G_drives[2], -prob.G_drives[2].T)
    check_device_entry(qc, coracle, monkeypatch, prob, Z, "non-Hermitian drive")


def test_host_buffer_entry_next_to_device_entry(qc, oracle, coracle, monkeypatch):
    prob, Z = chain_problem(oracle, N=8, m=6, T=300, n_deriv=2, free_time=True, pad=1, seed=25)
    check_device_entry(qc, coracle, monkeypatch, prob, Z, "host and device entries", host_entry=True)


def test_three_shards(qc, coracle, monkeypatch):
    inp = qc.config_inputs(3, T=1000)
    prob = problem_from_inputs(inp)
    Z = inp.traj.datavec + 1e-2 * np.random.default_rng(31).standard_normal(inp.traj.datavec.size)
    Fr, Jr = coracle.COracle(prob).F_dF(Z)

    def make():
        many = qc.QuantumDynamics(inp.integrators, inp.traj, devices=[0, 0, 0])
        try:
            return many.F_dF(Z, fresh=True)
        finally:
            many.close()

    F, J = both_forms(monkeypatch, make)
    assert rel_err(F, Fr) < TOL and rel_err(J, Jr) < TOL, (rel_err(F, Fr), rel_err(J, Jr))
    for a, b in ((0, 333), (333, 666), (666, 999)):       # ... and each shard's own device entry (loop-free, every copy)
        Fs, Js = coracle.COracle(prob).F_dF(Z, a, b)

        def make_shard():
            h = RawHandle(qc, prob, kernel="mfma", t_range=(a, b))
            try:
                return device_F_jac(qc, h.h, h.dims, Z)
            finally:
                h.close()

        F, J = both_forms(monkeypatch, make_shard)
        assert rel_err(F, Fs) < TOL and rel_err(J, Js) < TOL, ((a, b), rel_err(F, Fs), rel_err(J, Js))


def test_batched_list_launch(qc, monkeypatch):
    base = qc.multi_qubit_system(3)
    systems = [qc.QuantumSystem(base.H_drift * f, base.H_drives) for f in (0.9, 1.0, 1.1)]
    inp = qc.unitary_sampling_inputs(systems, qc.GATES["TOFFOLI"], 1000)
    ref = composed_oracle(inp)
    Z = inp.traj.datavec + 1e-2 * np.random.default_rng(41).standard_normal(inp.traj.datavec.size)

    def make():
        dyn = qc.QuantumDynamics(inp.integrators, inp.traj)
        try:
            assert isinstance(dyn, qc.ComposedQuantumDynamics) and len(dyn._parts) == 3
            F = torch.full((int(dyn.dims.F_len),), float("nan"), dtype=torch.float64, device="cuda")
            J = torch.full((int(dyn.dims.jac_nnz),), float("nan"), dtype=torch.float64, device="cuda")
            dyn.F_dF_device(torch.from_numpy(Z).cuda(), F, J)      # one launch for the three systems
            torch.cuda.synchronize()
            return F.cpu().numpy(), J.cpu().numpy()
        finally:
            dyn.close()

    F, J = both_forms(monkeypatch, make)
    assert rel_err(F, ref.F(Z)) < TOL
    assert rel_err(J, ref.dF(Z)) < TOL
