"""Inputs to the hot path for the BASELINE.json configurations, built the way
`UnitarySmoothPulseProblem` builds them (reference unitary_smooth_pulse_problem.jl:70-191): trajectory
via `initialize_trajectory`, then [unitary integrator, DerivativeIntegrator(a, da),
DerivativeIntegrator(da, dda)] (:163-179).  Objectives, bounds handling, Ipopt and the problem
struct stay on the reference side and are out of scope.

Synthetic inputs follow SURVEY.md section 8(d): seed 20250218, drift 0.1 * sum Z_i Z_{i+1}
(1 qubit: 0.1 Z as in reference test/test_utils.jl:123), drives X_i, Y_i per qubit, geodesic states +
N(0, 1e-2) noise, a in U(-1,1) with zero ends, da/dda ~ N(0, 0.1^2), dt = 0.2.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from .gates import GATES, operator_from_string
from .integrators import (DensityOperatorExponentialIntegrator, DerivativeIntegrator, QuantumStateExponentialIntegrator, QuantumStatePadeIntegrator,
                          UnitaryExponentialIntegrator, UnitaryPadeIntegrator)
from .named_trajectory import NamedTrajectory
from .quantum_systems import QuantumSystem
from .trajectory_initialization import initialize_trajectory

SEED = 20250218


@dataclass
class ConfigSpec:
    name: str
    n_qubits: int
    gate: str
    T: int
    description: str


CONFIGS = {
    1: ConfigSpec("config1", 1, "H", 50, "1-qubit Hadamard UnitarySmoothPulseProblem, T=50, dt=0.2, X/Y drives"),
    2: ConfigSpec("config2", 2, "CNOT", 200, "2-qubit CNOT UnitarySmoothPulseProblem, T=200, 4th-order Pade"),
    3: ConfigSpec("config3", 3, "TOFFOLI", 1000, "3-qubit Toffoli UnitarySmoothPulseProblem, T=1000"),
    4: ConfigSpec("config4", 3, "TOFFOLI", 8000, "3-qubit Toffoli T=8000, knot-sharded across GPUs"),
    5: ConfigSpec("config5", 4, "QFT16", 500, "4-qubit QFT UnitaryMinimumTimeProblem, T=500, free dt"),
}


def multi_qubit_system(n_qubits: int, zz: float = 0.1) -> QuantumSystem:
    def term(op: str, i: int) -> np.ndarray:
        return operator_from_string("".join(op if k == i else "I" for k in range(n_qubits)))

    if n_qubits == 1:
        H_drift = zz * operator_from_string("Z")
    else:
        H_drift = sum(zz * operator_from_string("".join("Z" if k in (i, i + 1) else "I" for k in range(n_qubits)))
                      for i in range(n_qubits - 1))
    H_drives = []
    for i in range(n_qubits):
        H_drives += [term("X", i), term("Y", i)]
    return QuantumSystem(H_drift, H_drives)


@dataclass
class HotPathInputs:
    system: QuantumSystem
    traj: NamedTrajectory
    integrators: List
    spec: Optional[ConfigSpec] = None


def unitary_smooth_pulse_inputs(system: QuantumSystem, U_goal: np.ndarray, T: int, dt: float = 0.2, *,
                                free_time: bool = True, integrator: str = "pade", pade_order: int = 4,
                                a_bound: float = 1.0, dda_bound: float = 1.0, state_noise: float = 1e-2,
                                seed: int = SEED) -> HotPathInputs:
    rng = np.random.default_rng(seed)
    m = system.n_drives
    traj = initialize_trajectory(
        U_goal, T, dt, m, ([a_bound] * m, [np.inf] * m, [dda_bound] * m),
        free_time=free_time, state_noise=state_noise, rng=rng)
    if integrator == "pade":
        U_int = UnitaryPadeIntegrator("Ũ⃗", "a", system, traj, order=pade_order)
    elif integrator == "exponential":
        U_int = UnitaryExponentialIntegrator("Ũ⃗", "a", system, traj)
    else:
        raise ValueError("integrator must be one of ('pade', 'exponential')")
    integrators = [U_int, DerivativeIntegrator("a", "da", traj), DerivativeIntegrator("da", "dda", traj)]
    return HotPathInputs(system, traj, integrators)


def config_inputs(cfg: int, T: Optional[int] = None, **kw) -> HotPathInputs:
    spec = CONFIGS[cfg]
    system = multi_qubit_system(spec.n_qubits)
    out = unitary_smooth_pulse_inputs(system, GATES[spec.gate], T if T is not None else spec.T, **kw)
    out.spec = spec
    return out


def quantum_state_smooth_pulse_inputs(system: QuantumSystem, psi_inits, psi_goals, T: int, dt: float = 0.2, *,
                                      free_time: bool = True, integrator: str = "pade", pade_order: int = 4,
                                      seed: int = SEED) -> HotPathInputs:
    """Inputs of `QuantumStateSmoothPulseProblem` (reference quantum_state_smooth_pulse_problem.jl:57-208): one
    trajectory component and one integrator per ket (:146-152), then the two derivative integrators.  States are
    linear interpolations init -> goal plus noise (the hot path does not care how the guess was made)."""
    from .named_trajectory import NamedTrajectory
    rng = np.random.default_rng(seed)
    m, N = system.n_drives, system.levels
    comps = {}
    names = []
    inits, goals = {}, {}
    for k, (p0, p1) in enumerate(zip(psi_inits, psi_goals)):
        p0 = np.asarray(p0, dtype=complex)
        p1 = np.asarray(p1, dtype=complex)
        lam = np.linspace(0.0, 1.0, T)[None, :]
        iso0 = np.concatenate([p0.real, p0.imag])[:, None]
        iso1 = np.concatenate([p1.real, p1.imag])[:, None]
        name = f"ψ̃{k + 1}" if len(psi_inits) > 1 else "ψ̃"
        comps[name] = iso0 * (1 - lam) + iso1 * lam + 1e-2 * rng.standard_normal((2 * N, T))
        names.append(name)
        inits[name], goals[name] = iso0[:, 0], iso1[:, 0]
    a = np.zeros((m, T))
    a[:, 1:T - 1] = rng.uniform(-1, 1, size=(m, T - 2))
    comps["a"] = a
    comps["da"] = 0.1 * rng.standard_normal((m, T))
    comps["dda"] = 0.1 * rng.standard_normal((m, T))
    if free_time:
        comps["Δt"] = np.full((1, T), dt)
    traj = NamedTrajectory(comps, controls=("dda", "Δt") if free_time else ("dda",), timestep="Δt" if free_time else dt,
                           initial=inits, goal=goals)
    cls = QuantumStatePadeIntegrator if integrator == "pade" else QuantumStateExponentialIntegrator
    kw = {"order": pade_order} if integrator == "pade" else {}
    integrators = [cls(nm, "a", system, traj, **kw) for nm in names]
    integrators += [DerivativeIntegrator("a", "da", traj), DerivativeIntegrator("da", "dda", traj)]
    return HotPathInputs(system, traj, integrators)


def density_operator_smooth_pulse_inputs(system, rho_init: np.ndarray, psi_goal: np.ndarray, T: int, dt: float = 0.2, *,
                                         free_time: bool = True, seed: int = SEED) -> HotPathInputs:
    """Inputs of `DensityOperatorSmoothPulseProblem` (reference density_operator_smooth_pulse_problem.jl:3-124): state
    component `ρ⃗̃` = iso-vec of vec(rho), the density-operator exponential integrator (:104-106) followed by the two
    derivative integrators (:108-112).  The guess interpolates rho_init -> |psi_goal><psi_goal| linearly plus noise."""
    from .isomorphisms import density_to_iso_vec
    from .named_trajectory import NamedTrajectory
    rng = np.random.default_rng(seed)
    m, N = system.n_drives, system.levels
    psi_goal = np.asarray(psi_goal, dtype=complex)
    r0 = density_to_iso_vec(rho_init)[:, None]
    r1 = density_to_iso_vec(np.outer(psi_goal, psi_goal.conj()))[:, None]
    lam = np.linspace(0.0, 1.0, T)[None, :]
    comps = {"ρ⃗̃": r0 * (1 - lam) + r1 * lam + 1e-2 * rng.standard_normal((2 * N * N, T))}
    a = np.zeros((m, T))
    a[:, 1:T - 1] = rng.uniform(-1, 1, size=(m, T - 2))
    comps["a"] = a
    comps["da"] = 0.1 * rng.standard_normal((m, T))
    comps["dda"] = 0.1 * rng.standard_normal((m, T))
    if free_time:
        comps["Δt"] = np.full((1, T), dt)
    traj = NamedTrajectory(comps, controls=("dda", "Δt") if free_time else ("dda",), timestep="Δt" if free_time else dt,
                           goal={"ρ⃗̃": r1[:, 0]})
    integrators = [DensityOperatorExponentialIntegrator("ρ⃗̃", "a", system, traj),
                   DerivativeIntegrator("a", "da", traj), DerivativeIntegrator("da", "dda", traj)]
    return HotPathInputs(system, traj, integrators)


def unitary_sampling_inputs(systems, U_goal: np.ndarray, T: int, dt: float = 0.2, *, free_time: bool = True,
                            integrator: str = "pade", pade_order: int = 4, seed: int = SEED) -> HotPathInputs:
    """Inputs of `UnitarySamplingProblem` (reference unitary_sampling_problem.jl:44-167): K systems share the
    controls of one merged trajectory with components `Ũ⃗_system_k` (:103-107), one unitary integrator per system
    followed by the two derivative integrators (:134-155)."""
    from .named_trajectory import NamedTrajectory
    from .trajectory_initialization import unitary_geodesic
    rng = np.random.default_rng(seed)
    m = systems[0].n_drives
    N = systems[0].levels
    comps = {}
    names = []
    for k in range(len(systems)):
        name = f"Ũ⃗_system_{k + 1}"
        comps[name] = unitary_geodesic(np.eye(N, dtype=complex), U_goal, T) + 1e-2 * rng.standard_normal((2 * N * N, T))
        names.append(name)
    a = np.zeros((m, T))
    a[:, 1:T - 1] = rng.uniform(-1, 1, size=(m, T - 2))
    comps["a"] = a
    comps["da"] = 0.1 * rng.standard_normal((m, T))
    comps["dda"] = 0.1 * rng.standard_normal((m, T))
    if free_time:
        comps["Δt"] = np.full((1, T), dt)
    from .isomorphisms import operator_to_iso_vec
    traj = NamedTrajectory(comps, controls=("dda", "Δt") if free_time else ("dda",), timestep="Δt" if free_time else dt,
                           goal={nm: operator_to_iso_vec(U_goal) for nm in names})
    cls = UnitaryPadeIntegrator if integrator == "pade" else UnitaryExponentialIntegrator
    kw = {"order": pade_order} if integrator == "pade" else {}
    integrators = [cls(nm, "a", sys_, traj, **kw) for nm, sys_ in zip(names, systems)]
    integrators += [DerivativeIntegrator("a", "da", traj), DerivativeIntegrator("da", "dda", traj)]
    return HotPathInputs(systems[0], traj, integrators)


def quantum_state_sampling_inputs(systems, psi_inits, psi_goals, T: int, dt: float = 0.2, *, free_time: bool = True,
                                  integrator: str = "pade", pade_order: int = 4, seed: int = SEED) -> HotPathInputs:
    """Inputs of `QuantumStateSamplingProblem` (reference quantum_state_sampling_problem.jl:5-120): K systems share the
    controls; system j carries its own copies of the kets, components `ψ̃{i}_system_{j}` (:40-43), one ket integrator per
    (state, system) in system-major order (:98-110), then the two derivative integrators."""
    from .named_trajectory import NamedTrajectory
    rng = np.random.default_rng(seed)
    m, N = systems[0].n_drives, systems[0].levels
    comps, names = {}, []
    lam = np.linspace(0.0, 1.0, T)[None, :]
    for jsys in range(len(systems)):
        row = []
        for i, (p0, p1) in enumerate(zip(psi_inits, psi_goals)):
            p0, p1 = np.asarray(p0, dtype=complex), np.asarray(p1, dtype=complex)
            iso0 = np.concatenate([p0.real, p0.imag])[:, None]
            iso1 = np.concatenate([p1.real, p1.imag])[:, None]
            name = f"ψ̃{i + 1}_system_{jsys + 1}"
            comps[name] = iso0 * (1 - lam) + iso1 * lam + 1e-2 * rng.standard_normal((2 * N, T))
            row.append(name)
        names.append(row)
    a = np.zeros((m, T))
    a[:, 1:T - 1] = rng.uniform(-1, 1, size=(m, T - 2))
    comps["a"] = a
    comps["da"] = 0.1 * rng.standard_normal((m, T))
    comps["dda"] = 0.1 * rng.standard_normal((m, T))
    if free_time:
        comps["Δt"] = np.full((1, T), dt)
    traj = NamedTrajectory(comps, controls=("dda", "Δt") if free_time else ("dda",), timestep="Δt" if free_time else dt)
    cls = QuantumStatePadeIntegrator if integrator == "pade" else QuantumStateExponentialIntegrator
    kw = {"order": pade_order} if integrator == "pade" else {}
    integrators = [cls(nm, "a", sys_, traj, **kw) for row, sys_ in zip(names, systems) for nm in row]
    integrators += [DerivativeIntegrator("a", "da", traj), DerivativeIntegrator("da", "dda", traj)]
    return HotPathInputs(systems[0], traj, integrators)


def unitary_bang_bang_inputs(system: QuantumSystem, U_goal: np.ndarray, T: int, dt: float = 0.2, *, free_time: bool = True,
                             integrator: str = "pade", pade_order: int = 4, control_name: str = "a",
                             seed: int = SEED) -> HotPathInputs:
    """Inputs of `UnitaryBangBangProblem` (reference unitary_bang_bang_problem.jl:73-188): ONE control derivative
    (`initialize_trajectory(..., (a_bounds, da_bounds))`, :102-121), the unitary integrator and a single
    `DerivativeIntegrator(a, da)` (:163-175).  The L1 regulariser on `da` appends two slack components of the size of `da`
    to the trajectory (`L1Regularizer!(constraints, control_names[2], traj, ...)`, :149-152; their names come from
    QuantumCollocationCore and are a choice of this build): the dynamics never read them, they only widen the knots.
    The reference's own test runs this template with `pade_order=12` and `control_name=:u` (:205-215)."""
    rng = np.random.default_rng(seed)
    m = system.n_drives
    base = initialize_trajectory(U_goal, T, dt, m, ([1.0] * m, [1.0] * m), free_time=free_time, rng=rng)
    a, da = control_name, "d" + control_name
    names = {"a": a, "da": da}
    comps = {}
    for nm in base.names:
        comps[names.get(nm, nm)] = np.array(base[nm])
    comps[f"s1_{da}"] = np.maximum(comps[da], 0.0)
    comps[f"s2_{da}"] = np.maximum(-comps[da], 0.0)
    controls = tuple(names.get(c, c) for c in base.controls) + (f"s1_{da}", f"s2_{da}")
    tstep = base.timestep
    traj = NamedTrajectory(comps, controls=controls, timestep=tstep,
                           goal={names.get(k, k): v for k, v in base.goal.items()})
    if integrator == "pade":
        U_int = UnitaryPadeIntegrator("Ũ⃗", a, system, traj, order=pade_order)
    elif integrator == "exponential":
        U_int = UnitaryExponentialIntegrator("Ũ⃗", a, system, traj)
    else:
        raise ValueError("integrator must be one of ('pade', 'exponential')")
    return HotPathInputs(system, traj, [U_int, DerivativeIntegrator(a, da, traj)])


def unitary_direct_sum_inputs(parts, labels=None) -> HotPathInputs:
    """Inputs of `UnitaryDirectSumProblem` (reference unitary_direct_sum_problem.jl:48-186) from the hot-path inputs of its
    member problems (smooth-pulse problems only, :72): the members' trajectories merged with their labels as suffixes
    (`merge([add_suffix(p.trajectory, l) ...])`, :104) and every member's integrators re-pointed at the merged
    trajectory, member after member (:127-130) -- [U_1, D, D, U_2, D, D, ...]: every member keeps its OWN controls, unlike
    the sampling problem.  The reference's test builds the members with `free_time=false` (:196: a constant timestep, no
    `Δt` rows); with free time this build keeps ONE shared, un-suffixed timestep component after the members' components
    (what the merge does with several timestep rows is NamedTrajectories' business and unverified here)."""
    from .integrators import _UnitaryIntegrator
    labels = [str(i + 1) for i in range(len(parts))] if labels is None else [str(l) for l in labels]
    if len(labels) != len(parts) or len(parts) < 2:
        raise ValueError("at least two problems, one label each")
    T = parts[0].traj.T
    free = [isinstance(p.traj.timestep, str) for p in parts]
    if any(free) and not all(free):
        raise ValueError("members must all have a free timestep or all a fixed one")
    if not free[0] and len({float(p.traj.timestep) for p in parts}) != 1:
        raise ValueError("members with fixed timesteps must share the timestep")
    comps, controls, goal = {}, [], {}
    for p, l in zip(parts, labels):
        if p.traj.T != T:
            raise ValueError("the member trajectories must have the same number of knots")
        if "dda" not in p.traj.names:
            raise ValueError("Only smooth pulse problems are supported.")
        for nm in p.traj.names:
            if nm != p.traj.timestep:
                comps[nm + l] = np.array(p.traj[nm])
        controls += [c + l for c in p.traj.controls if c != p.traj.timestep]
        goal.update({k + l: v for k, v in p.traj.goal.items()})
    if free[0]:
        tname = parts[0].traj.timestep
        comps[tname] = np.array(parts[0].traj[tname])
        controls.append(tname)
        tstep = tname
    else:
        tstep = float(parts[0].traj.timestep)
    traj = NamedTrajectory(comps, controls=tuple(controls), timestep=tstep, goal=goal)
    integrators = []
    for p, l in zip(parts, labels):
        for I in p.integrators:
            if isinstance(I, _UnitaryIntegrator):
                kw = {"order": I.order} if isinstance(I, UnitaryPadeIntegrator) else {}
                integrators.append(type(I)(I.state_name + l, I.control_name + l, I.system, traj, **kw))
            elif isinstance(I, DerivativeIntegrator):
                integrators.append(DerivativeIntegrator(I.x + l, I.dx + l, traj))
            else:
                raise NotImplementedError("direct sums of unitary smooth-pulse problems")
    return HotPathInputs(parts[0].system, traj, integrators)


@dataclass
class ControlProblemInputs:
    """What `QuantumControlEvaluator(QuantumDynamics(integrators, traj), objectives, constraints)` needs."""
    system: QuantumSystem
    traj: NamedTrajectory
    integrators: List
    objectives: List
    constraints: List


def unitary_robustness_problem(H_error, inputs: HotPathInputs, *, objectives=(), constraints=(), final_fidelity: Optional[float] = None,
                               subspace=None, phase_name: str = "ϕ", phase_operators=None, eval_hessian: bool = True,
                               unitary_name: str = "Ũ⃗", device: int = 0) -> ControlProblemInputs:
    """`UnitaryRobustnessProblem(H_error, trajectory, system, objective, integrators, constraints; ...)` (reference
    unitary_robustness_problem.jl:28-99): the given objectives plus `UnitaryRobustnessObjective(H_error=H_error)` (:46-49), the
    given constraints plus a final-fidelity constraint on `subspace` (:58-84) -- `FinalUnitaryFidelityConstraint`, or the
    free-phase variant over `traj.global_data[phase_name]` when `phase_operators` is given.  `final_fidelity=None`: the
    trajectory's current (free-phase) fidelity."""
    from .objectives import (FinalUnitaryFidelityConstraint, FinalUnitaryFreePhaseFidelityConstraint, UnitaryRobustnessObjective,
                             iso_vec_unitary_fidelity, iso_vec_unitary_free_phase_fidelity)
    traj = inputs.traj
    if unitary_name not in traj.names:
        raise ValueError(f"trajectory has no component {unitary_name}")
    rob = UnitaryRobustnessObjective(traj, H_error=H_error, eval_hessian=eval_hessian, symb=unitary_name, device=device)
    U_T = np.array(traj[unitary_name][:, -1])
    U_G = np.asarray(traj.goal[unitary_name], dtype=np.float64)
    sub = None if subspace is None else [int(s) for s in subspace]
    if phase_operators is None:
        if final_fidelity is None:
            final_fidelity = iso_vec_unitary_fidelity(U_T, U_G, subspace=sub, device=device)
        con = FinalUnitaryFidelityConstraint(unitary_name, final_fidelity, traj, subspace=sub, device=device)
    else:
        if final_fidelity is None:
            final_fidelity = iso_vec_unitary_free_phase_fidelity(U_T, U_G, traj.global_data[phase_name], phase_operators, subspace=sub,
                                                                 device=device)
        con = FinalUnitaryFreePhaseFidelityConstraint(unitary_name, phase_name, phase_operators, final_fidelity, traj, subspace=sub,
                                                      device=device)
    return ControlProblemInputs(inputs.system, traj, list(inputs.integrators), list(objectives) + [rob], list(constraints) + [con])


def add_l1_slacks(inp: HotPathInputs, name: str, indices, *, integrator: str = "pade", pade_order: int = 4) -> HotPathInputs:
    """The trajectory side of `L1Regularizer!(constraints, name, traj; indices)` (reference _problem_templates.jl:41-54) on the
    inputs of a unitary smooth-pulse problem: two slack components `slack_names(name)` with one entry per index, appended to the
    controls and started at max(+-x, 0) so that their rows x - s1 + s2 = 0 hold (as `unitary_bang_bang_inputs` does), and the
    integrators rebuilt on the wider knots.  The dynamics never read the slacks."""
    from .objectives import slack_names
    traj = inp.traj
    x = np.array(traj[name])[np.asarray(indices, dtype=np.int64), :]
    s1, s2 = slack_names(name)
    comps = {nm: np.array(traj[nm]) for nm in traj.names}
    comps[s1], comps[s2] = np.maximum(x, 0.0), np.maximum(-x, 0.0)
    traj = NamedTrajectory(comps, controls=tuple(traj.controls) + (s1, s2), timestep=traj.timestep, initial=traj.initial, goal=traj.goal)
    if integrator == "pade":
        U_int = UnitaryPadeIntegrator("Ũ⃗", "a", inp.system, traj, order=pade_order)
    elif integrator == "exponential":
        U_int = UnitaryExponentialIntegrator("Ũ⃗", "a", inp.system, traj)
    else:
        raise ValueError("integrator must be one of ('pade', 'exponential')")
    return HotPathInputs(inp.system, traj, [U_int, DerivativeIntegrator("a", "da", traj), DerivativeIntegrator("da", "dda", traj)])


def unitary_smooth_pulse_problem(system: QuantumSystem, U_goal, T: int, dt: float = 0.2, *, Q: float = 100.0, R: float = 1e-2,
                                 R_a=None, R_da=None, R_dda=None, leakage_suppression: bool = False, R_leakage: float = 1e-1,
                                 additional_objective=None, timesteps_all_equal: bool = False, integrator: str = "pade",
                                 pade_order: int = 4, free_time: bool = True, device: int = 0, seed: int = SEED) -> ControlProblemInputs:
    """`UnitarySmoothPulseProblem(system, U_goal, T, dt; Q, R, R_a, R_da, R_dda, leakage_suppression, R_leakage,
    additional_objective, ...)` (reference unitary_smooth_pulse_problem.jl:70-191 with `apply_piccolo_options!`,
    _problem_templates.jl:31-75): the infidelity objective (on the subspace of an `EmbeddedOperator` goal) plus ONE
    `TrajectoryObjective` holding the regularisers on a / da / dda, `additional_objective` and, with `leakage_suppression`, the
    `L1Regularizer` on the leakage entries of `Ũ⃗` (`EmbeddedOperator.leakage_indices`).  Leakage suppression appends two slack
    components `slack_names("Ũ⃗")` to the controls, started at max(+-x, 0) (as `unitary_bang_bang_inputs` does), and their rows
    `L1SlackConstraint` to the constraints; the bounds s >= 0 are the solver's.  An `EmbeddedOperator` goal starts its geodesic
    toward `embed(fill=1)`."""
    from .gates import EmbeddedOperator
    from .objectives import (L1Regularizer, L1SlackConstraint, QuadraticRegularizer, TimeStepsAllEqualConstraint, TrajectoryObjective,
                             UnitaryInfidelityObjective)
    emb = U_goal if isinstance(U_goal, EmbeddedOperator) else None
    U = emb.embed(fill=1.0) if emb is not None else np.asarray(U_goal, dtype=complex)
    sub = emb.subspace if emb is not None else None
    inp = unitary_smooth_pulse_inputs(system, U, T, dt, free_time=free_time, integrator=integrator, pade_order=pade_order, seed=seed)
    traj, integrators = inp.traj, inp.integrators
    constraints = []
    if leakage_suppression:
        if emb is None:
            raise ValueError("leakage suppression needs an EmbeddedOperator goal (its leakage indices)")
        leak = emb.leakage_indices()
        inp = add_l1_slacks(inp, "Ũ⃗", leak, integrator=integrator, pade_order=pade_order)
        traj, integrators = inp.traj, inp.integrators
        constraints.append(L1SlackConstraint("Ũ⃗", traj, leak))
    if free_time and timesteps_all_equal:
        constraints.append(TimeStepsAllEqualConstraint(traj.timestep, traj))
    spec = (QuadraticRegularizer("a", traj, R if R_a is None else R_a) + QuadraticRegularizer("da", traj, R if R_da is None else R_da)
            + QuadraticRegularizer("dda", traj, R if R_dda is None else R_dda))
    if additional_objective is not None:
        spec = spec + additional_objective
    if leakage_suppression:
        spec = spec + L1Regularizer("Ũ⃗", traj, R_leakage)
    objectives = [UnitaryInfidelityObjective("Ũ⃗", traj, Q, subspace=sub, device=device),
                  TrajectoryObjective(spec, traj, device=device)]
    return ControlProblemInputs(system, traj, integrators, objectives, constraints)


def direct_sum_graph(labels, graph, boundary_values, Q_symb: str, names):
    """The edges of `UnitaryDirectSumProblem` (reference unitary_direct_sum_problem.jl:75-100) as component names: returns
    (edges, boundary) with edges [(name_i, name_j)] and boundary [(name, baseline)].  graph=None: the chain over the labels.
    Otherwise every edge is either two labels -- (Q_symb+l1, Q_symb+l2) -- a label and a key of `boundary_values` -- a boundary
    edge, a baseline regulariser on Q_symb+label -- or two component names of the merged trajectory (the reference's Symbol
    graph); anything else is a ValueError."""
    labels = [str(l) for l in labels]
    boundary_values = boundary_values or {}
    if graph is None:
        return [(Q_symb + a, Q_symb + b) for a, b in zip(labels[:-1], labels[1:])], []
    edges, boundary = [], []
    for e in graph:
        a, b = (str(x) for x in e)
        if a in labels and b in labels:
            edges.append((Q_symb + a, Q_symb + b))
        elif a in boundary_values and b in labels:
            boundary.append((Q_symb + b, np.asarray(boundary_values[a], dtype=np.float64)))
        elif a in labels and b in boundary_values:
            boundary.append((Q_symb + a, np.asarray(boundary_values[b], dtype=np.float64)))
        elif a in names and b in names:
            edges.append((a, b))
        else:
            raise ValueError(f"edge ({a}, {b}): edge labels must be in the problem labels or the boundary values, or be component names")
    return edges, boundary


def unitary_direct_sum_problem(parts, final_fidelity: float, *, labels=None, graph=None, boundary_values=None, Q=100.0,
                               Q_symb: str = "dda", R: float = 1e-2, R_a=None, R_da=None, R_dda=None, R_b=None,
                               fidelity_cost: bool = False, subspace=None, drive_reset_ratio: float = 0.5,
                               drive_derivative_sigma: float = 0.01, seed: int = SEED, device: int = 0) -> ControlProblemInputs:
    """`UnitaryDirectSumProblem(probs, final_fidelity; prob_labels, graph, boundary_values, Q, Q_symb, R, R_a, R_da, R_dda, R_b,
    drive_reset_ratio, fidelity_cost, subspace)` (reference unitary_direct_sum_problem.jl:48-186) on the hot-path inputs of its
    members (`unitary_direct_sum_inputs`): the members' controls are mixed with a fresh draw (`drive_reset_ratio`, :106-123),
    the graph becomes a `PairwiseQuadraticRegularizer` (`direct_sum_graph`), boundary edges baseline regularisers with weight
    R_b, every member gets its a / da / dda regularisers and a `FinalUnitaryFidelityConstraint`, and with `fidelity_cost` an
    infidelity objective (weight Q, or Q[0] for a per-edge Q).  A baseline regulariser and a plain one on the same component
    cannot share a terms handle, so the baselines then go into a second `TrajectoryObjective`."""
    from .objectives import (FinalUnitaryFidelityConstraint, PairwiseQuadraticRegularizer, QuadraticRegularizer, TrajectoryObjective,
                             UnitaryInfidelityObjective)
    from .trajectory_initialization import initialize_control_trajectory
    labels = [str(i + 1) for i in range(len(parts))] if labels is None else [str(l) for l in labels]
    boundary_values = {str(k): v for k, v in (boundary_values or {}).items()}
    if set(boundary_values) & set(labels):
        raise ValueError("boundary value keys cannot be problem labels")
    if not 0.0 <= drive_reset_ratio <= 1.0:
        raise ValueError("drive_reset_ratio must be in [0, 1]")
    inp = unitary_direct_sum_inputs(parts, labels)
    traj = inp.traj
    edges, boundary = direct_sum_graph(labels, graph, boundary_values, Q_symb, traj.names)
    if drive_reset_ratio > 0:
        rng = np.random.default_rng(seed)
        for l in labels:
            m = len(traj.components["a" + l])
            fresh = initialize_control_trajectory(m, 2, traj.T, [1.0] * m, drive_derivative_sigma, rng)
            for nm, v in zip(("a", "da", "dda"), fresh):
                traj[nm + l][:, :] = (1 - drive_reset_ratio) * traj[nm + l] + drive_reset_ratio * v
    R_b = R if R_b is None else R_b
    main = [PairwiseQuadraticRegularizer(traj, Q, edges)] if edges else []
    for l in labels:
        main += [QuadraticRegularizer("a" + l, traj, R if R_a is None else R_a), QuadraticRegularizer("da" + l, traj, R if R_da is None else R_da),
                 QuadraticRegularizer("dda" + l, traj, R if R_dda is None else R_dda)]
    base = [QuadraticRegularizer(nm, traj, R_b, baseline=val) for nm, val in boundary]
    plain = {t.name for t in main if isinstance(t, QuadraticRegularizer)}
    if any(b.name in plain for b in base):
        objectives = [TrajectoryObjective(main, traj, device=device), TrajectoryObjective(base, traj, device=device)]
    else:
        objectives = [TrajectoryObjective(main + base, traj, device=device)]
    sub = None if subspace is None else [int(s) for s in subspace]
    constraints = [FinalUnitaryFidelityConstraint("Ũ⃗" + l, final_fidelity, traj, subspace=sub, device=device) for l in labels]
    if fidelity_cost:
        Q_fid = float(np.asarray(Q, dtype=np.float64).ravel()[0])
        objectives += [UnitaryInfidelityObjective("Ũ⃗" + l, traj, Q_fid, subspace=sub, device=device) for l in labels]
    return ControlProblemInputs(inp.system, traj, inp.integrators, objectives, constraints)
