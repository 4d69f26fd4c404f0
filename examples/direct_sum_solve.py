#!/usr/bin/env python3
"""The reference's direct-sum problem (src/problem_templates/unitary_direct_sum_problem.jl:48-186, test :186-272) solved on the
interior-point driver of examples/ipm_solve.py, with exact second derivatives.  Two 1-qubit members (H_drift = 0.01 Z, drives X
and Y, T = 50, dt = 0.2, `free_time=false`) with goals X and U_eps' X U_eps are first solved on their own (smooth-pulse
problems); `unitary_direct_sum_problem` then joins them: a `PairwiseQuadraticRegularizer` between their `dda` (the default chain,
Q = 100), each member's regularisers, and each member's final fidelity held by a `FinalUnitaryFidelityConstraint`.

    python examples/direct_sum_solve.py [member iterations] [direct-sum iterations]
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


def bounds(traj, pinned_states, controls):
    """Pinned: the initial states and the first and last controls `a*`; -1 <= a*, dda* <= 1."""
    T, zdim, comps = traj.T, traj.dim, traj.components
    nv = T * zdim + traj.global_dim
    pinned = np.zeros(nv, dtype=bool)
    for s in pinned_states:
        pinned[comps[s].start:comps[s].stop] = True
    lb, ub = np.full(nv, -np.inf), np.full(nv, np.inf)
    for a, dda in controls:
        for t_pin in (0, T - 1):
            pinned[t_pin * zdim + comps[a].start:t_pin * zdim + comps[a].stop] = True
        for t in range(T):
            for nm in (a, dda):
                sl = slice(t * zdim + comps[nm].start, t * zdim + comps[nm].stop)
                lb[sl], ub[sl] = -1.0, 1.0
    return np.flatnonzero(~pinned), lb, ub


def solve(iters1: int = 30, iters2: int = 30, verbose: bool = True, final_fidelity: float = 0.99):
    qc = g.load_package()
    system = qc.QuantumSystem(0.01 * qc.GATES["Z"], [qc.GATES["X"], qc.GATES["Y"]])
    th = 0.33
    U_eps = np.cos(th / 2) * np.eye(2) - 1j * np.sin(th / 2) * qc.GATES["Y"]      # a fixed small rotation
    goals = [qc.GATES["X"], U_eps.conj().T @ qc.GATES["X"] @ U_eps]
    parts, member_fid = [], []
    for k, U_goal in enumerate(goals):
        prob = qc.unitary_smooth_pulse_problem(system, U_goal, 50, 0.2, free_time=False, seed=100 + k)
        dyn = qc.QuantumDynamics(prob.integrators, prob.traj)
        free, lb, ub = bounds(prob.traj, ["Ũ⃗"], [("a", "dda")])
        ev = qc.QuantumControlEvaluator(dyn, prob.objectives, prob.constraints)
        z, _ = interior_point(ev, prob.traj.datavec.copy(), free, lb, ub, max_iter=iters1, verbose=False)
        prob.traj.data[:, :] = z.reshape(prob.traj.dim, prob.traj.T, order="F")
        member_fid.append(qc.iso_vec_unitary_fidelity(np.array(prob.traj["Ũ⃗"][:, -1]), prob.traj.goal["Ũ⃗"]))
        parts.append(qc.problems.HotPathInputs(system, prob.traj, prob.integrators))
        for o in [dyn] + prob.objectives:
            o.close()
    F_min = min(final_fidelity, min(member_fid) - 1e-4)
    ds = qc.unitary_direct_sum_problem(parts, F_min, drive_reset_ratio=0.0)
    traj = ds.traj
    dyn = qc.QuantumDynamics(ds.integrators, traj)
    pair = qc.TrajectoryObjective([qc.PairwiseQuadraticRegularizer(traj, 100.0, [("dda1", "dda2")])], traj)
    free, lb, ub = bounds(traj, ["Ũ⃗1", "Ũ⃗2"], [("a1", "dda1"), ("a2", "dda2")])
    ev = qc.QuantumControlEvaluator(dyn, ds.objectives, ds.constraints)
    z0 = traj.datavec.copy()
    z, it = interior_point(ev, z0, free, lb, ub, max_iter=iters2, verbose=verbose, n_ineq=len(ds.constraints))
    out = dict(member_fidelity=member_fid, final_fidelity=F_min, iterations=it, pairwise_before=pair.L(z0), pairwise_after=pair.L(z),
               fidelity_residuals=[float(c.g(z)[0]) for c in ds.constraints], dynamics_residual=float(np.abs(dyn.F(z)).max()),
               n_objectives=len(ds.objectives))
    if verbose:
        print(f"members' final fidelities {member_fid[0]:.5f}, {member_fid[1]:.5f}; direct sum: {it} iterations, pairwise term "
              f"{out['pairwise_before']:.4e} -> {out['pairwise_after']:.4e}, F - {F_min:.4f} = "
              f"{', '.join(f'{r:+.2e}' for r in out['fidelity_residuals'])}, max |dynamics residual| {out['dynamics_residual']:.2e}")
    for o in [dyn, pair] + ds.objectives + ds.constraints:
        o.close()
    return out


if __name__ == "__main__":
    solve(*(int(x) for x in sys.argv[1:3]))
