#!/usr/bin/env python3
"""Polish a solved pulse for robustness: take the solved 1-qubit Hadamard pulse of examples/robustness_landscape.py and minimise the
MEAN infidelity over a grid of detunings, systems(zeta) = QuantumSystem(zeta Z, [X, Y]), by gradient steps on the controls.  The
objective is `SweepInfidelityObjective`; every gradient is ONE adjoint sweep (`RolloutSweep.grad`, `qc_sweep_grad`), whatever the
number of systems and drives.  scipy's L-BFGS-B moves the controls of knots 1 .. T-2 inside the pulse's own amplitude bound; the
timesteps stay as solved.  The landscape is printed before and after.

    python examples/robust_polish.py [max_iter] [grid] [steps]
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as g
from solve_hadamard import solve


def polish(T: int = 50, grid: int = 11, max_iter: int = 60, steps: int = 60, width: float = 0.05, verbose: bool = True):
    """(mean infidelity before, after) over `grid` detunings in [-width, width]."""
    from scipy.optimize import minimize
    qc = g.load_package()
    f0, f1, viol, z, traj, system = solve(max_iter, T=T, verbose=False, return_solution=True)
    zetas = np.linspace(-width, width, grid)
    obj = qc.SweepInfidelityObjective(traj, system, [qc.GATES["Z"]], zetas[:, None])
    zdim, a = traj.dim, traj.components["a"]
    idx = np.concatenate([t * zdim + np.arange(a.start, a.stop) for t in range(1, T - 1)])      # the first and last controls stay pinned
    z = np.array(z, dtype=np.float64)
    bound = max(1.0, float(np.abs(z[idx]).max()))

    def fun(v):
        zz = z.copy()
        zz[idx] = v
        J, fids, grad = obj.J_fids_grad(zz)
        return 1.0 - J, -grad[idx]

    F_before = obj.fidelities(z)
    res = minimize(fun, z[idx], jac=True, method="L-BFGS-B", bounds=[(-bound, bound)] * idx.size, options={"maxiter": steps})
    z_after = z.copy()
    z_after[idx] = res.x
    F_after = obj.fidelities(z_after)
    before, after = float(1.0 - F_before.mean()), float(1.0 - F_after.mean())
    if verbose:
        print(f"rollout fidelity of the solved pulse: {f1:.6f}; {res.nit} L-BFGS iterations, {res.nfev} gradient calls")
        print("   zeta     F before      F after")
        for zt, fb, fa in zip(zetas, F_before, F_after):
            print(f"  {zt:+.3f}    {fb:.6f}     {fa:.6f}")
        print(f"mean infidelity over the grid: {before:.3e} -> {after:.3e}")
    obj.close()
    return before, after


if __name__ == "__main__":
    arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
    polish(max_iter=arg(1, 60), grid=arg(2, 11), steps=arg(3, 60))
