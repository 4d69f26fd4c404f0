#!/usr/bin/env python3
"""The reference's leakage-suppression case (src/problem_templates/unitary_smooth_pulse_problem.jl:290-309) on the interior-point
driver of examples/ipm_solve.py, with exact second derivatives: a 4-level system (H_drift = 0, drives (a + a')/2 and
(a - a')/(2i)), T = 50, dt = 0.2, the goal H on levels {0, 1}, `leakage_suppression=true, R_leakage=1e-1`.  The template adds two
slack components s1_Ũ⃗ / s2_Ũ⃗ on the 8 leakage entries of Ũ⃗, their L1 cost to the trajectory objective and the slack rows
x - s1 + s2 = 0 to the constraints; the slacks are bounded below by 0 here, as the solver's bounds.

    python examples/leakage_solve.py [iterations]
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


def solve(iters: int = 40, verbose: bool = True):
    """40 iterations where the reference asks Ipopt for 20 (this driver has no filter and no second-order correction)."""
    qc = g.load_package()
    a = np.diag(np.sqrt(np.arange(1.0, 4.0)), 1)                    # annihilation operator, 4 levels
    system = qc.QuantumSystem(np.zeros((4, 4)), [(a + a.T) / 2, (a - a.T) / 2j])
    U_goal = qc.EmbeddedOperator("H", SUBSPACE, 4)
    prob = qc.unitary_smooth_pulse_problem(system, U_goal, 50, 0.2, leakage_suppression=True, R_leakage=1e-1)
    traj = prob.traj
    T, zdim, comps = traj.T, traj.dim, traj.components
    dyn = qc.QuantumDynamics(prob.integrators, traj)
    slack = prob.constraints[0]

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
        for nm in qc.slack_names("Ũ⃗"):
            lb[t * zdim + comps[nm].start:t * zdim + comps[nm].stop] = 0.0
        i = t * zdim + comps["Δt"].start
        lb[i], ub[i] = 0.1, 0.3

    def rollout_fidelity(z):
        traj.data[:, :] = z[:T * zdim].reshape(zdim, T, order="F")
        return qc.unitary_rollout_fidelity(traj, system, subspace=SUBSPACE)

    z0 = traj.datavec.copy()
    ev = qc.QuantumControlEvaluator(dyn, prob.objectives, prob.constraints)
    fid_before = rollout_fidelity(z0)
    leak = U_goal.leakage_indices()
    z, it = interior_point(ev, z0, free, lb, ub, max_iter=iters, verbose=verbose)
    fid_after = rollout_fidelity(z)
    U = z[:T * zdim].reshape(T, zdim)[:, comps["Ũ⃗"].start:comps["Ũ⃗"].stop]
    out = dict(fidelity_before=fid_before, fidelity_after=fid_after, iterations=it, n_leakage=int(leak.size),
               slack_residual=float(np.abs(slack.g(z)).max()), dynamics_residual=float(np.abs(dyn.F(z)).max()),
               leakage_l1_before=float(np.abs(z0.reshape(T, zdim)[:, comps["Ũ⃗"].start + leak]).sum()),
               leakage_l1_after=float(np.abs(U[:, leak]).sum()), objective=ev.eval_objective(z))
    if verbose:
        print(f"{it} iterations, subspace rollout fidelity {fid_before:.4f} -> {fid_after:.4f}, sum |leakage entries| "
              f"{out['leakage_l1_before']:.3f} -> {out['leakage_l1_after']:.3f}, max |slack row| {out['slack_residual']:.2e}, "
              f"max |dynamics residual| {out['dynamics_residual']:.2e}")
    for o in [dyn] + prob.objectives:
        o.close()
    return out


if __name__ == "__main__":
    solve(*(int(x) for x in sys.argv[1:2]))
