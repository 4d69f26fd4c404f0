#!/usr/bin/env python3
"""The reference's "Robust and Subspace Templates" test (src/problem_templates/unitary_robustness_problem.jl:129-180) in two
stages on the interior-point driver of examples/ipm_solve.py, with exact second derivatives -- the dense Hessian of the
robustness term included:

  1. a smooth-pulse problem on a 3-level system (H_drift = 0, drives a + a' and i(a' - a), T = 51, dt = 0.2) whose goal is X on
     levels {0, 1} (completed by the identity on level 2 for the initial geodesic), infidelity measured on that subspace;
  2. from its solution, `unitary_robustness_problem(H_error = Z on {0, 1})`: the same objective plus
     `UnitaryRobustnessObjective`, and the final fidelity held at least at its current value (`final_fidelity=None`).

    python examples/robust_solve.py [stage-1 iterations] [stage-2 iterations]
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import __graft_entry__ as g  # noqa: E402
from ipm_solve import interior_point  # noqa: E402

SUBSPACE = [0, 1]


def solve(iters1: int = 40, iters2: int = 50, verbose: bool = True, R: float = 1e-2):
    """Stage 2 runs the reference's 50 iterations; stage 1 runs 40 where the reference asks Ipopt for 15 (this driver has no
    filter and no second-order correction: after 15 of its iterations the dynamics are still far from feasible)."""
    qc = g.load_package()
    a = np.diag(np.sqrt(np.arange(1.0, 3.0)), 1)                    # annihilation operator, 3 levels
    system = qc.QuantumSystem(np.zeros((3, 3)), [a + a.T, 1j * (a.T - a)])
    U_goal = qc.EmbeddedOperator("X", SUBSPACE, 3)
    H_error = qc.EmbeddedOperator("Z", SUBSPACE, 3)
    inp = qc.unitary_smooth_pulse_inputs(system, U_goal.embed(fill=1.0), 51, 0.2)
    traj = inp.traj
    T, zdim, comps = traj.T, traj.dim, traj.components
    dyn = qc.QuantumDynamics(inp.integrators, traj)
    infid = qc.UnitaryInfidelityObjective("Ũ⃗", traj, Q=100.0, subspace=SUBSPACE, form="abs2")
    reg = qc.TrajectoryObjective(qc.QuadraticRegularizer("a", traj, R) + qc.QuadraticRegularizer("da", traj, R)
                                 + qc.QuadraticRegularizer("dda", traj, R), traj)

    # pinned: the initial unitary, the first and last controls; bounds of the smooth-pulse template
    nv = T * zdim + traj.global_dim
    pinned = np.zeros(nv, dtype=bool)
    pinned[comps["Ũ⃗"].start:comps["Ũ⃗"].stop] = True
    for t_pin in (0, T - 1):
        pinned[t_pin * zdim + comps["a"].start:t_pin * zdim + comps["a"].stop] = True
    free = np.flatnonzero(~pinned)
    lb, ub = np.full(nv, -np.inf), np.full(nv, np.inf)
    for t in range(T):
        for nm in ("a", "dda"):
            sl = slice(t * zdim + comps[nm].start, t * zdim + comps[nm].stop)
            lb[sl], ub[sl] = -1.0, 1.0
        i = t * zdim + comps["Δt"].start
        lb[i], ub[i] = 0.1, 0.3

    def rollout_fidelity(z):
        traj.data[:, :] = z[:T * zdim].reshape(zdim, T, order="F")
        return qc.unitary_rollout_fidelity(traj, system, subspace=SUBSPACE)

    # stage 1: the smooth-pulse problem
    z0 = traj.datavec.copy()
    ev1 = qc.QuantumControlEvaluator(dyn, [infid, reg])
    fid_before = rollout_fidelity(z0)
    z1, it1 = interior_point(ev1, z0, free, lb, ub, max_iter=iters1, verbose=verbose)
    fid_after = rollout_fidelity(z1)                               # (leaves z1 in traj: stage 2 starts from it)
    if verbose:
        print(f"stage 1: {it1} iterations, subspace rollout fidelity {fid_before:.6f} -> {fid_after:.6f}")

    # stage 2: the robustness problem from that solution
    prob = qc.unitary_robustness_problem(H_error, inp, objectives=[infid, reg], subspace=SUBSPACE)
    rob, con = prob.objectives[-1], prob.constraints[-1]
    ev2 = qc.QuantumControlEvaluator(dyn, prob.objectives, prob.constraints)
    loss_before = rob.L(z1)
    z2, it2 = interior_point(ev2, z1, free, lb, ub, max_iter=iters2, verbose=verbose, n_ineq=1)
    out = dict(fidelity_before=fid_before, fidelity_after=fid_after, iterations=(it1, it2), robustness_before=loss_before,
               robustness_after=rob.L(z2), final_fidelity=con.value, fidelity_residual=float(con.g(z2)[0]),
               dynamics_residual=float(np.abs(dyn.F(z2)).max()), n_robust_vars=rob.n_vars, stats=dict(ev2.stats))
    if verbose:
        print(f"stage 2: {it2} iterations, robustness loss {out['robustness_before']:.6e} -> {out['robustness_after']:.6e}  "
              f"fidelity constraint F - {con.value:.6f} = {out['fidelity_residual']:.2e}  max |dynamics residual| "
              f"{out['dynamics_residual']:.2e}  (V = {rob.n_vars} robustness variables)")
    for o in (dyn, infid, reg, rob, con):
        o.close()
    return out


if __name__ == "__main__":
    solve(*(int(x) for x in sys.argv[1:3]))
