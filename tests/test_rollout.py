"""Rollouts.  CPU: the oracle's rollout against scipy's expm and unitarity / trace invariants.
GPU: `qc_rollout` (three-level scan of propagators) against the oracle for unitaries, kets and density operators,
across chunk boundaries, and the rollout fidelity."""
import numpy as np
import pytest
import scipy.linalg as sla

from oracle_bridge import problem_from_inputs


def test_oracle_rollout_matches_scipy_and_stays_unitary(qc, oracle):
    inp = qc.config_inputs(2, T=12)
    prob = problem_from_inputs(inp)
    Z = inp.traj.datavec
    N = inp.system.levels
    init = qc.operator_to_iso_vec(np.eye(N, dtype=complex))
    R = oracle.rollout(prob, Z, init)
    assert R.shape == (2 * N * N, 12)
    U = np.eye(N, dtype=complex)
    Zm = Z.reshape(12, -1)
    for t in range(11):
        a = Zm[t, prob.off_a:prob.off_a + prob.m]
        H = inp.system.H_drift + sum(x * Hk for x, Hk in zip(a, inp.system.H_drives))
        U = sla.expm(-1j * Zm[t, prob.off_dt] * H) @ U
        np.testing.assert_allclose(qc.iso_vec_to_operator(R[:, t + 1]), U, atol=1e-12)
    np.testing.assert_allclose(U.conj().T @ U, np.eye(N), atol=1e-12)
    # the rolled-out states satisfy the exponential-integrator constraint exactly
    inp_e = qc.unitary_smooth_pulse_inputs(inp.system, qc.GATES["CX"], 12, integrator="exponential")
    pe = problem_from_inputs(inp_e)
    Ze = inp_e.traj.datavec.copy().reshape(12, -1)
    Re = oracle.rollout(pe, Ze.ravel(), init)
    Ze[:, pe.off_U:pe.off_U + pe.s] = Re.T
    F = oracle.F(pe, Ze.ravel()).reshape(11, -1)
    assert np.abs(F[:, :pe.s]).max() < 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,T", [(1, 2), (1, 5), (1, 50), (2, 37), (3, 101), (5, 9)])
def test_unitary_rollout_kernel(qc, oracle, cfg, T):
    inp = qc.config_inputs(cfg, T=T)
    prob = problem_from_inputs(inp)
    Z = inp.traj.datavec
    N = inp.system.levels
    rng = np.random.default_rng(T)
    init = qc.operator_to_iso_vec(sla.expm(1j * (lambda A: (A + A.conj().T) / 2)(rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N)))))
    ref = oracle.rollout(prob, Z, init)
    dyn = qc.QuantumDynamics(inp.integrators, inp.traj)          # a Pade handle: the rollout is exponential regardless
    got = dyn.rollout(Z, init)
    np.testing.assert_allclose(got, ref, rtol=1e-10, atol=1e-11)
    dyn.close()
    a = inp.traj["a"]
    dts = inp.traj["Δt"].ravel()
    got2 = qc.unitary_rollout(init, a, dts, inp.system)
    np.testing.assert_allclose(got2, ref, rtol=1e-10, atol=1e-11)


@pytest.mark.gpu
def test_rollout_large_generator_norm_and_fixed_time(qc, oracle):
    """Strong drives (several squarings) and a scalar timestep."""
    base = qc.multi_qubit_system(2)
    sys_ = qc.QuantumSystem(40.0 * base.H_drift, [25.0 * H for H in base.H_drives])
    rng = np.random.default_rng(5)
    T = 30
    a = rng.uniform(-1, 1, (sys_.n_drives, T))
    init = qc.operator_to_iso_vec(np.eye(4, dtype=complex))
    got = qc.unitary_rollout(init, a, 0.37, sys_)
    U = np.eye(4, dtype=complex)
    for t in range(T - 1):
        H = sys_.H_drift + sum(x * Hk for x, Hk in zip(a[:, t], sys_.H_drives))
        U = sla.expm(-1j * 0.37 * H) @ U
        np.testing.assert_allclose(qc.iso_vec_to_operator(got[:, t + 1]), U, atol=1e-9)


@pytest.mark.gpu
def test_ket_and_density_rollouts(qc, oracle):
    import test_density
    base = qc.multi_qubit_system(2)
    rng = np.random.default_rng(2)
    T = 26
    a = rng.uniform(-1, 1, (base.n_drives, T))
    dts = rng.uniform(0.1, 0.3, T)
    psi = rng.standard_normal(4) + 1j * rng.standard_normal(4)
    psi /= np.linalg.norm(psi)
    got = qc.rollout(np.concatenate([psi.real, psi.imag]), a, dts, base)
    v = psi.copy()
    for t in range(T - 1):
        H = base.H_drift + sum(x * Hk for x, Hk in zip(a[:, t], base.H_drives))
        v = sla.expm(-1j * dts[t] * H) @ v
    np.testing.assert_allclose(got[:4, -1] + 1j * got[4:, -1], v, atol=1e-11)
    osys = test_density.open_system(qc, 2, gamma=0.1)
    rho0 = np.outer(psi, psi.conj())
    R = qc.open_rollout(qc.density_to_iso_vec(rho0), a, dts, osys)
    x = qc.density_to_iso_vec(rho0)
    for t in range(T - 1):
        x = sla.expm(dts[t] * osys.G(a[:, t])) @ x
    np.testing.assert_allclose(R[:, -1], x, atol=1e-11)
    rho = qc.iso_vec_to_density(R[:, -1])
    assert abs(np.trace(rho) - 1) < 1e-11 and np.linalg.eigvalsh((rho + rho.conj().T) / 2).min() > -1e-10


@pytest.mark.gpu
def test_unitary_rollout_fidelity(qc, oracle):
    inp = qc.config_inputs(1, T=40)
    f = qc.unitary_rollout_fidelity(inp.traj, inp.system)
    prob = problem_from_inputs(inp)
    R = oracle.rollout(prob, inp.traj.datavec, qc.operator_to_iso_vec(np.eye(2, dtype=complex)))
    assert abs(f - oracle.iso_vec_unitary_fidelity(R[:, -1], inp.traj.goal["Ũ⃗"])) < 1e-12
    assert 0.0 <= f <= 1.0 + 1e-12


@pytest.mark.gpu
def test_rollout_is_bit_reproducible(qc, oracle):
    """Every knot's state is written by ONE workgroup: until round 4 the first knot of a scan chunk was written twice (by the chunk that
    starts there and by the one that ends there, products in different orders, one ulp apart) and repeated calls differed in the last
    bit at the chunk boundaries."""
    for cfg, T in [(2, 9), (2, 50), (3, 101), (1, 17)]:
        inp = qc.config_inputs(cfg, T=T)
        dyn = qc.QuantumDynamics(inp.integrators, inp.traj)
        N = inp.system.levels
        init = qc.operator_to_iso_vec(np.eye(N, dtype=complex))
        first = dyn.rollout(inp.traj.datavec, init)
        for _ in range(6):
            np.testing.assert_array_equal(dyn.rollout(inp.traj.datavec, init), first)
        dyn.close()


def test_control_guess_derivatives_and_linear_interpolation(qc):
    """Host side of `initialize_trajectory(...; a_guess, geodesic=false)` (reference trajectory_initialization.jl:176-188,225-244)."""
    from qcolloc_amd.trajectory_initialization import control_derivatives_from_guess, unitary_linear_interpolation
    rng = np.random.default_rng(2)
    a = rng.standard_normal((3, 9))
    dts = rng.uniform(0.1, 0.3, 9)
    a0, da, dda = control_derivatives_from_guess(a, dts, 2)
    np.testing.assert_array_equal(a0, a)
    np.testing.assert_allclose(a[:, 1:] - a[:, :-1] - dts[:-1] * da[:, :-1], 0.0, atol=1e-15)         # DerivativeIntegrator(a, da) rows
    np.testing.assert_allclose(da[:, 1:] - da[:, :-1] - dts[:-1] * dda[:, :-1], 0.0, atol=1e-14)     # DerivativeIntegrator(da, dda)
    U = qc.GATES["CNOT"]
    lin = unitary_linear_interpolation(np.eye(4, dtype=complex), U, 5)
    np.testing.assert_array_equal(lin[:, 0], qc.operator_to_iso_vec(np.eye(4, dtype=complex)))
    np.testing.assert_allclose(lin[:, -1], qc.operator_to_iso_vec(U), atol=1e-15)
    np.testing.assert_allclose(lin[:, 2], 0.5 * (lin[:, 0] + lin[:, -1]), atol=1e-15)


@pytest.mark.gpu
@pytest.mark.parametrize("nq,T,free_time", [(1, 20, True), (2, 33, False), (3, 50, True)])
def test_trajectory_from_a_control_guess_satisfies_the_exponential_dynamics(qc, oracle, nq, T, free_time):
    """`initialize_trajectory(U_goal, T, dt, ...; a_guess, system)` rolls the guess out (reference trajectory_initialization.jl:422-426):
    the rollout kernel's states are a zero of the exponential integrator's residual kernel (x_{t+1} = exp(dt G(a_t)) x_t on both
    sides, two independent implementations: scan of propagators vs per-interval expm), and the differenced controls a zero of the
    derivative rows."""
    from qcolloc_amd.trajectory_initialization import initialize_trajectory
    system = qc.multi_qubit_system(nq)
    m = system.n_drives
    rng = np.random.default_rng(nq)
    a_guess = 0.5 * np.sin(np.linspace(0, 3, T))[None, :] * rng.uniform(0.5, 1.0, (m, 1))
    gate = {1: "H", 2: "CNOT", 3: "TOFFOLI"}[nq]
    traj = initialize_trajectory(qc.GATES[gate], T, 0.2, m, ([1.0] * m, [np.inf] * m, [1.0] * m), free_time=free_time,
                                 a_guess=a_guess, system=system)
    integ = [qc.UnitaryExponentialIntegrator("Ũ⃗", "a", system, traj), qc.DerivativeIntegrator("a", "da", traj), qc.DerivativeIntegrator("da", "dda", traj)]
    dyn = qc.QuantumDynamics(integ, traj, eval_hessian=False)
    F = dyn.F(traj.datavec)
    assert np.abs(F).max() < 5e-13, np.abs(F).max()
    dyn.close()
    # ... and of the order-12 Pade residual to its truncation error, of the order-4 residual only to O(dt^5)
    integ12 = [qc.UnitaryPadeIntegrator("Ũ⃗", "a", system, traj, order=12)] + integ[1:]
    dyn12 = qc.QuantumDynamics(integ12, traj)
    assert np.abs(dyn12.F(traj.datavec)).max() < 1e-12
    dyn12.close()
    with pytest.raises(ValueError):
        initialize_trajectory(qc.GATES[gate], T, 0.2, m, ([1.0] * m, [np.inf] * m, [1.0] * m), a_guess=a_guess)     # no system


@pytest.mark.gpu
def test_ket_rollout_fidelity(qc, oracle):
    """`rollout_fidelity(prob.trajectory, sys; state_name)` (reference quantum_state_smooth_pulse_problem.jl:247-249,
    quantum_state_sampling_problem.jl:187-189) against a scipy rollout of the same controls."""
    system = qc.multi_qubit_system(2)
    basis = np.eye(4, dtype=complex)
    inp = qc.quantum_state_smooth_pulse_inputs(system, [basis[:, 0], basis[:, 1]], [basis[:, 3], (basis[:, 0] + 1j * basis[:, 2]) / np.sqrt(2)], 31)
    a, dts = inp.traj["a"], inp.traj["Δt"].ravel()
    for k, name in enumerate(("ψ̃1", "ψ̃2")):
        v = basis[:, k].copy()
        for t in range(inp.traj.T - 1):
            H = system.H_drift + sum(x * Hk for x, Hk in zip(a[:, t], system.H_drives))
            v = sla.expm(-1j * dts[t] * H) @ v
        goal = inp.traj.goal[name]
        want = abs(np.vdot(goal[:4] + 1j * goal[4:], v)) ** 2
        got = qc.rollout_fidelity(inp.traj, system, state_name=name)
        assert abs(got - want) < 1e-12, (name, got, want)


# ---------------------------------------------------------------------------------------------- launch forms ----
# qc_launch_rollout's host rule (qc_rollout.hip:253-273, the switch at :297-303) restated: the compiled matrix size NT (0: the
# generic instantiation), the dynamic LDS of the propagator / chunk-total / chain launches (opt-in past 64 KB) and the chunking.
def rollout_launch(n, nc, T):
    n_int = T - 1
    chunk = 1
    while chunk * chunk < n_int:
        chunk += 1
    return dict(NT=n if n in (4, 8, 16, 32) else 0, lds_prop=32 * n * n, lds_tot=24 * n * n, lds_st=(2 * n * nc + n * n) * 8,
                chunk=chunk, n_chunks=-(-n_int // chunk), n_int=n_int)


def _herm(rng, N, scale=1.0):
    X = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
    return scale * (X + X.conj().T) / 2


def _random_system(qc, N, seed, m=2, scale=1.0):
    rng = np.random.default_rng(seed)
    return qc.QuantumSystem(_herm(rng, N, scale), [_herm(rng, N, scale) for _ in range(m)])


def _open_system(qc, N, seed, gamma=0.1):
    rng = np.random.default_rng(seed)
    lower = np.diag(np.sqrt(np.arange(1, N)), 1).astype(complex)
    return qc.OpenQuantumSystem(_herm(rng, N), [_herm(rng, N, 0.5)], [np.sqrt(gamma) * lower, np.sqrt(gamma / 2) * _herm(rng, N, 0.3)])


# name: (state kind, levels N, T); the launch form each reaches is restated by rollout_launch
ROLLOUT_CASES = {
    "qutrit-T2": ("unitary", 3, 2),
    "qutrit-T102": ("unitary", 3, 102),            # n_int = 101: chunk 11, the last chunk is short
    "qutrit-T10001": ("unitary", 3, 10001),        # 100 chunks: the start chain runs 99 steps
    "levels12-T101": ("unitary", 12, 101),
    "levels23-T40": ("unitary", 23, 40),           # n = 46: propagator opt-in
    "qubits5-T2": ("unitary", 32, 2),              # n = 64: propagator and chunk-total opt-in
    "qubits5-T300": ("unitary", 32, 300),
    "qubits5-ket-T65": ("ket", 32, 65),            # n = 64, nc = 1
    "open5-T30": ("density", 5, 30),               # n = 2 * 25 = 50: propagator opt-in
    "qubits3-T10001": ("unitary", 8, 10001),       # compiled NT = 16, long chains
}


def _rollout_case_launch(name):
    kind, N, T = ROLLOUT_CASES[name]
    n = 2 * N * N if kind == "density" else 2 * N
    return rollout_launch(n, N if kind == "unitary" else 1, T)


def test_rollout_launch_coverage():
    """The GPU cases below reach the generic NT = 0 instantiation with and without the LDS opt-ins, a short last chunk, long start
    chains, one state column at n = 64 and a compiled NT over 100 chunks."""
    f = {k: _rollout_case_launch(k) for k in ROLLOUT_CASES}
    assert rollout_launch(64, 64, 300)["lds_st"] > 65536 and rollout_launch(46, 46, 2)["lds_prop"] > 65536
    assert rollout_launch(45, 45, 2)["lds_prop"] <= 65536 and rollout_launch(52, 52, 2)["lds_tot"] <= 65536 < rollout_launch(53, 53, 2)["lds_tot"]
    zero = [v for v in f.values() if v["NT"] == 0]
    assert any(v["lds_prop"] <= 65536 for v in zero)
    assert any(65536 < v["lds_prop"] and v["lds_tot"] <= 65536 for v in zero)
    assert any(v["lds_tot"] > 65536 and v["n_chunks"] > 1 for v in zero)
    assert any(v["n_chunks"] >= 100 for v in zero) and any(v["n_chunks"] >= 100 for v in f.values() if v["NT"])
    assert any(v["n_int"] % v["chunk"] for v in zero) and any(v["n_int"] == 1 for v in zero)
    assert f["qubits5-ket-T65"]["NT"] == 0 and f["qubits5-ket-T65"]["lds_st"] == (2 * 64 + 64 * 64) * 8
    assert f["open5-T30"]["NT"] == 0 and f["qubits3-T10001"]["NT"] == 16


def _expm_chain(system, init, a, dts):
    """x_{t+1} = expm(dt_t G(a_t)) x_t with scipy, in the real iso form the kernels use: (n nc) x T."""
    n = 2 * system.state_levels
    X = np.asarray(init, dtype=float).reshape(n, -1, order="F")
    out = np.empty((X.size, a.shape[1]))
    out[:, 0] = X.ravel(order="F")
    for t in range(a.shape[1] - 1):
        G = system.G_drift + sum(x * Gk for x, Gk in zip(a[:, t], system.G_drives))
        X = sla.expm(dts[t] * G) @ X
        out[:, t + 1] = X.ravel(order="F")
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ROLLOUT_CASES))
def test_rollout_launch_forms(qc, name):
    """Every launch form of qc_launch_rollout against a scipy expm chain, plus unitarity / trace of the GPU states."""
    kind, N, T = ROLLOUT_CASES[name]
    rng = np.random.default_rng(list(ROLLOUT_CASES).index(name) * 7919 + T)
    if kind == "density":
        system = _open_system(qc, N, seed=N)
    elif N == 32:
        base = qc.multi_qubit_system(5)                                # strong drive: ||dt G||_1 well past 1/4, several squarings
        system = qc.QuantumSystem(8.0 * base.H_drift, [6.0 * H for H in base.H_drives])
    elif N == 8:
        system = qc.multi_qubit_system(3)
    else:
        system = _random_system(qc, N, seed=N)
    a = rng.uniform(-1, 1, (system.n_drives, T))
    dts = rng.uniform(0.1, 0.3, T)
    if kind == "unitary":
        U0 = sla.expm(1j * _herm(rng, N))
        init = qc.operator_to_iso_vec(U0)
        got = qc.unitary_rollout(init, a, dts, system)
    elif kind == "ket":
        psi = rng.standard_normal(N) + 1j * rng.standard_normal(N)
        psi /= np.linalg.norm(psi)
        init = np.concatenate([psi.real, psi.imag])
        got = qc.rollout(init, a, dts, system)
    else:
        v = rng.standard_normal(N) + 1j * rng.standard_normal(N)
        rho0 = 0.7 * np.outer(v, v.conj()) / np.vdot(v, v).real + 0.3 * np.eye(N) / N
        init = qc.density_to_iso_vec(rho0)
        got = qc.open_rollout(init, a, dts, system)
    ref = _expm_chain(system, init, a, dts)
    assert got.shape == ref.shape
    np.testing.assert_allclose(got, ref, rtol=1e-10, atol=1e-11)
    if kind == "unitary":
        U = got.reshape(N, 2, N, T, order="F")                        # [row, part, column, knot]
        U = np.moveaxis(U[:, 0] + 1j * U[:, 1], -1, 0)
        assert np.abs(np.swapaxes(U.conj(), 1, 2) @ U - np.eye(N)).max() < 1e-10
    elif kind == "ket":
        assert np.abs(np.sum(got * got, axis=0) - 1.0).max() < 1e-10
    else:
        tr = np.array([np.trace(qc.iso_vec_to_density(got[:, t])) for t in range(T)])
        assert np.abs(tr - 1.0).max() < 1e-10
    if T == 10001 or N == 32:
        again = {"unitary": qc.unitary_rollout, "ket": qc.rollout}[kind](init, a, dts, system)
        np.testing.assert_array_equal(again, got)


@pytest.mark.gpu
def test_rollout_through_a_multi_device_handle(qc, oracle):
    """qc_rollout on a [0, 0, 0] multi-device handle is served by shard 0: the single handle's states bit for bit."""
    inp = qc.config_inputs(3, T=101)
    Z = inp.traj.datavec
    N = inp.system.levels
    init = qc.operator_to_iso_vec(sla.expm(1j * _herm(np.random.default_rng(4), N)))
    one = qc.QuantumDynamics(inp.integrators, inp.traj)
    many = qc.QuantumDynamics(inp.integrators, inp.traj, devices=[0, 0, 0])
    try:
        assert many.n_shards == 3
        got = many.rollout(Z, init)
        np.testing.assert_array_equal(got, one.rollout(Z, init))
        np.testing.assert_allclose(got, oracle.rollout(problem_from_inputs(inp), Z, init), rtol=1e-10, atol=1e-11)
    finally:
        one.close()
        many.close()
