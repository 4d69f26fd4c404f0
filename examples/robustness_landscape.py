#!/usr/bin/env python3
"""Robustness landscape of a solved pulse, the shape of the reference's own robustness check
(reference src/problem_templates/unitary_sampling_problem.jl:204-244): solve the 1-qubit Hadamard problem (T = 50, dt = 0.2,
X / Y drives; examples/solve_hadamard.py), then ask how good the pulse is when the system is not the one it was optimised
for -- systems(zeta) = QuantumSystem(zeta Z, [X, Y]) for zeta = -0.05:0.01:0.05, and a relative amplitude error on both drives.
Every landscape is ONE call of `rollout_sweep` (`qc_sweep_eval`): one trajectory of controls, S systems, S fidelities.

    python examples/robustness_landscape.py [max_iter]
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as g
from solve_hadamard import solve


def landscape(max_iter: int = 60, verbose: bool = True):
    qc = g.load_package()
    f0, f1, viol, z, traj, system = solve(max_iter, T=50, verbose=verbose, return_solution=True)
    zdim, comps = traj.dim, traj.components
    K = z[:traj.T * zdim].reshape(traj.T, zdim)
    controls = K[:, comps["a"].start:comps["a"].stop].T.copy()
    dts = K[:, comps["Δt"].start].copy()
    init = qc.operator_to_iso_vec(np.eye(2, dtype=complex))
    goal = qc.operator_to_iso_vec(qc.GATES["H"])
    zetas = np.arange(-5, 6) * 0.01
    # detuning: G_s = zeta_s iso(-iZ) + sum_k a_k G_k
    _, F_det = qc.rollout_sweep(init, controls, dts, system, [qc.GATES["Z"]], zetas[:, None], goal=goal, fid_kind="unitary")
    # amplitude miscalibration: both drives scaled by 1 + eps
    eps = np.arange(-5, 6) * 0.01
    _, F_amp = qc.rollout_sweep(init, controls, dts, system, [], np.zeros((eps.size, 0)), 1.0 + np.repeat(eps[:, None], system.n_drives, axis=1),
                                goal=goal, fid_kind="unitary")
    # a Monte-Carlo cloud over both at once
    rng = np.random.default_rng(0)
    S = 4096
    theta = rng.normal(0.0, 0.02, (S, 1))
    scale = 1.0 + rng.normal(0.0, 0.02, (S, system.n_drives))
    _, F_mc = qc.rollout_sweep(init, controls, dts, system, [qc.GATES["Z"]], theta, scale, goal=goal, fid_kind="unitary")
    if verbose:
        print(f"rollout fidelity of the solved pulse: {f1:.6f}")
        print("   zeta     F(detuning zeta Z)      eps     F(drives x (1 + eps))")
        for zt, fd, e, fa in zip(zetas, F_det, eps, F_amp):
            print(f"  {zt:+.2f}     {fd:.6f}             {e:+.2f}     {fa:.6f}")
        print(f"Monte-Carlo, {S} systems, sigma = 0.02 on the detuning and on both amplitudes: mean F = {F_mc.mean():.6f}, "
              f"5th percentile = {np.percentile(F_mc, 5):.6f}, worst = {F_mc.min():.6f}")
    return zetas, F_det, eps, F_amp, F_mc


if __name__ == "__main__":
    landscape(int(sys.argv[1]) if len(sys.argv) > 1 else 60)
