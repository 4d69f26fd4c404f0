"""The 2N = 16 F + dF kernel (qc_mfma16_pade4_kernel) fetches the data its copy wave only passes on -- the states of both knots
and the derivative-integrator window of both knots (QcParams.dwin_lo / dwin_n) -- as 16-byte pieces of the knot, which is only
8-byte aligned when zdim is odd.  Every residual and Jacobian value against the C oracle: the loop-free and the persistent grid,
the masked instantiations (N < 8 levels), free and fixed timesteps, 0 - 4 derivative integrators (the window) and the generic
path (more integrators, or one of more than 64 rows), odd and even zdim, shards, and the batched launch of several handles."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle_bridge import composed_oracle, problem_from_inputs
from test_gpu_parity import RawHandle

pytestmark = pytest.mark.gpu
TOL = 1e-12


def rel_err(got, ref):
    assert got.shape == ref.shape
    return float(np.max(np.abs(got - ref))) / max(1.0, float(np.max(np.abs(ref)))) if ref.size else 0.0


def chain_problem(o, N, m, T, n_deriv, free_time, pad, dd=None, seed=0):
    """A random Pade-4 problem whose knot is [U | a | pad | c_0 .. c_n_deriv | dt]: derivative integrator i is c_i' = c_i+1.
    dd = None: c_0 is the control a (dim m); else the chain is a separate set of components of dim dd."""
    rng = np.random.default_rng(seed)
    n, s = 2 * N, 2 * N * N

    def gen():
        A = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
        return o.generator((A + A.conj().T) / 2)

    off_U, off_a = 0, s
    dim = m if dd is None else dd
    o_chain = s if dd is None else s + m + pad          # c_0 = a, or a separate chain behind a and the padding
    end = o_chain + (n_deriv + 1) * dim + (pad if dd is None else 0)
    derivs = [o.DerivSpec(o_chain + i * dim, o_chain + (i + 1) * dim, dim) for i in range(n_deriv)]
    zdim = end + (1 if free_time else 0)
    off_dt = end if free_time else -1
    prob = o.Problem(N=N, m=m, T=T, zdim=zdim, off_U=off_U, off_a=off_a, off_dt=off_dt, G_drift=gen(),
                     G_drives=np.array([gen() for _ in range(m)]).reshape(m, n, n), dt_fixed=0.13, order=4, derivs=derivs)
    Z = rng.standard_normal(zdim * T) * 0.5
    if free_time:
        Z[off_dt::zdim] = rng.uniform(0.1, 0.3, size=T)
    return prob, Z


def device_F_jac(qc, h, dims, Z):
    L = qc._lib
    dZ = torch.from_numpy(Z).cuda()
    F = torch.full((int(dims.F_len),), float("nan"), dtype=torch.float64, device="cuda")
    J = torch.full((int(dims.jac_nnz),), float("nan"), dtype=torch.float64, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(L.lib.qc_eval_F_jac_dev(h, dZ.data_ptr(), F.data_ptr(), J.data_ptr(), s), h)
    torch.cuda.synchronize()
    return F.cpu().numpy(), J.cpu().numpy()


def check_both_entries(qc, coracle, prob, Z, what, t_range=None):
    co = coracle.COracle(prob)
    Fr, Jr = co.F_dF(Z, *(t_range or (0, prob.T - 1)))
    h = RawHandle(qc, prob, kernel="mfma", t_range=t_range)
    try:
        F, J = h.F_jac(Z)                                       # host entry: the compact form (one copy of the blocks)
        Fd, Jd = device_F_jac(qc, h.h, h.dims, Z)               # device entry: every copy
    finally:
        h.close()
    assert rel_err(F, Fr) < TOL and rel_err(J, Jr) < TOL, (what, rel_err(F, Fr), rel_err(J, Jr))
    assert rel_err(Fd, Fr) < TOL and rel_err(Jd, Jr) < TOL, (what, rel_err(Fd, Fr), rel_err(Jd, Jr))


@pytest.mark.parametrize("T", [1000, 2100])     # loop-free grid (999 workgroups), persistent grid (2099 intervals)
def test_config3_every_value(qc, coracle, T):
    inp = qc.config_inputs(3, T=T)
    prob = problem_from_inputs(inp)
    assert prob.zdim % 2 == 1                   # every other knot is 8-byte aligned only
    rng = np.random.default_rng(T)
    Z = inp.traj.datavec + 1e-2 * rng.standard_normal(inp.traj.datavec.size)
    Fr, Jr = coracle.COracle(prob).F_dF(Z)
    dyn = qc.QuantumDynamics(inp.integrators, inp.traj)
    try:
        F, J = dyn.F_dF(Z)
        dF = torch.empty(int(dyn.dims.F_len), dtype=torch.float64, device="cuda")
        dJ = torch.empty(int(dyn.dims.jac_nnz), dtype=torch.float64, device="cuda")
        dyn.F_dF_device(torch.from_numpy(Z).cuda(), dF, dJ)
        torch.cuda.synchronize()
    finally:
        dyn.close()
    assert rel_err(F, Fr) < TOL and rel_err(J, Jr) < TOL
    assert np.array_equal(dF.cpu().numpy(), F) and np.array_equal(dJ.cpu().numpy(), J)


@pytest.mark.parametrize("cfg", [1, 2])         # N < 8 levels: the masked instantiation
def test_masked_configs_every_value(qc, coracle, cfg):
    inp = qc.config_inputs(cfg)
    prob = problem_from_inputs(inp)
    Z = inp.traj.datavec + 1e-2 * np.random.default_rng(cfg).standard_normal(inp.traj.datavec.size)
    dyn = qc.QuantumDynamics(inp.integrators, inp.traj)
    try:
        F, J = dyn.F_dF(Z)
    finally:
        dyn.close()
    Fr, Jr = coracle.COracle(prob).F_dF(Z)
    assert rel_err(F, Fr) < TOL and rel_err(J, Jr) < TOL


@pytest.mark.parametrize("n_deriv", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("free_time", [True, False])
@pytest.mark.parametrize("pad", [0, 1])         # flips the parity of zdim
@pytest.mark.parametrize("T", [40, 1100])
def test_derivative_windows(qc, oracle, coracle, n_deriv, free_time, pad, T):
    prob, Z = chain_problem(oracle, N=8, m=3, T=T, n_deriv=n_deriv, free_time=free_time, pad=pad, seed=10 * n_deriv + pad)
    check_both_entries(qc, coracle, prob, Z, f"n_deriv={n_deriv} free_time={free_time} zdim={prob.zdim} T={T}")


@pytest.mark.parametrize("dd,n_deriv", [(70, 1), (64, 2), (40, 4), (8, 4)])
@pytest.mark.parametrize("free_time", [True, False])
@pytest.mark.parametrize("pad", [0, 1])
def test_derivative_components_of_other_sizes(qc, oracle, coracle, dd, n_deriv, free_time, pad):
    """Chains beyond one window (a component of more than 64 rows, or components spanning more than 128 doubles): the generic path;
    chains within one: the window, placed anywhere in the knot, the window's last piece ending at the end of the knot included."""
    prob, Z = chain_problem(oracle, N=8, m=2, T=37, n_deriv=n_deriv, free_time=free_time, pad=pad, dd=dd, seed=dd + pad)
    check_both_entries(qc, coracle, prob, Z, f"dd={dd} n_deriv={n_deriv} free_time={free_time} zdim={prob.zdim}")


def test_shards(qc, oracle, coracle):
    prob, Z = chain_problem(oracle, N=8, m=3, T=1500, n_deriv=2, free_time=True, pad=1, seed=3)
    assert prob.zdim % 2 == 1
    for a, b in ((0, 1), (1, 700), (700, 1499)):       # odd and even first knots; one interval; loop-free and persistent grids
        check_both_entries(qc, coracle, prob, Z, f"shard [{a}, {b})", t_range=(a, b))


def test_batched_launch(qc, coracle):
    base = qc.multi_qubit_system(3)
    systems = [qc.QuantumSystem(base.H_drift * f, base.H_drives) for f in (0.9, 1.0, 1.1)]
    inp = qc.unitary_sampling_inputs(systems, qc.GATES["TOFFOLI"], 1100)   # 1099 intervals: the persistent grid
    ref = composed_oracle(inp)
    Z = inp.traj.datavec + 1e-2 * np.random.default_rng(1).standard_normal(inp.traj.datavec.size)
    dyn = qc.QuantumDynamics(inp.integrators, inp.traj)
    try:
        assert isinstance(dyn, qc.ComposedQuantumDynamics) and len(dyn._parts) == 3
        F = torch.full((int(dyn.dims.F_len),), float("nan"), dtype=torch.float64, device="cuda")
        J = torch.full((int(dyn.dims.jac_nnz),), float("nan"), dtype=torch.float64, device="cuda")
        dyn.F_dF_device(torch.from_numpy(Z).cuda(), F, J)      # one launch for the three systems (qc_eval_F_jac_dev_multi)
        torch.cuda.synchronize()
    finally:
        dyn.close()
    assert rel_err(F.cpu().numpy(), ref.F(Z)) < TOL
    assert rel_err(J.cpu().numpy(), ref.dF(Z)) < TOL
