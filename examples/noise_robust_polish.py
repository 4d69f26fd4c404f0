#!/usr/bin/env python3
"""Polish a solved pulse against noise that changes DURING the pulse: take the solved 1-qubit Hadamard pulse of
examples/solve_hadamard.py and minimise the MEAN infidelity over S fixed realisations of an Ornstein-Uhlenbeck detuning,

    H_s(t) = xi_s(t) Z + a_x(t) X + a_y(t) Y,      d xi = -(xi / tau) dt + sigma sqrt(2 / tau) dW      (stationary: std sigma, correlation time tau),

sampled exactly on the pulse's own timesteps (numpy, from `dts`, sigma, tau) and held constant inside an interval.  The realisations are
drawn once (common random numbers), so the objective is a smooth function of the controls and scipy's L-BFGS-B can move the controls of
knots 1 .. T-2 inside the pulse's amplitude bound; the timesteps stay as solved.  The objective is `SweepNoiseInfidelityObjective`:
every value is ONE noise sweep and every gradient ONE adjoint noise sweep (`qc_sweep_noise_eval`, `qc_sweep_noise_grad`), all S
realisations in one launch.  Printed: the mean infidelity before and after, and the time profile mean_s |dF_s/dxi_t| of the polished
pulse -- when in the pulse a detuning kick hurts (the time-domain filter function), from the same adjoint sweep.

Other noise models are a choice of perturbation.  Additive noise on drive line k is P_j = G_k with xi the noise itself.
Multiplicative amplitude noise eps_{s,t} a_{t,k} G_k is P_j = G_k with xi[s, t] = eps[s, t] a[t, k]; xi then depends on the controls, and
the control gradient gains eps[s, t] * grad_noise[s, t, j] by the chain rule (weighted as the samples are).

    python examples/noise_robust_polish.py [max_iter] [S] [steps]
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as g
from solve_hadamard import solve


def ou_realisations(rng, S: int, dts, sigma: float, tau: float) -> np.ndarray:
    """S x len(dts) samples of a stationary Ornstein-Uhlenbeck process at the interval starts: xi_0 ~ N(0, sigma^2),
    xi_{t+1} = r_t xi_t + sigma sqrt(1 - r_t^2) N(0, 1) with r_t = exp(-dt_t / tau) (the exact transition, any step)."""
    dts = np.asarray(dts, dtype=np.float64)
    xi = np.empty((S, dts.size))
    xi[:, 0] = sigma * rng.standard_normal(S)
    for t in range(dts.size - 1):
        r = np.exp(-dts[t] / tau)
        xi[:, t + 1] = r * xi[:, t] + sigma * np.sqrt(1.0 - r * r) * rng.standard_normal(S)
    return xi


def polish(T: int = 50, S: int = 64, max_iter: int = 60, steps: int = 60, sigma: float = 0.05, tau: float = 2.0, seed: int = 0,
           verbose: bool = True):
    """(mean infidelity before, after, profile) over S Ornstein-Uhlenbeck detuning realisations; profile[t] = mean_s |dF_s/dxi_t| after."""
    from scipy.optimize import minimize
    qc = g.load_package()
    f0, f1, viol, z, traj, system = solve(max_iter, T=T, verbose=False, return_solution=True)
    z = np.array(z, dtype=np.float64)
    zdim, a = traj.dim, traj.components["a"]
    dts = z[:T * zdim].reshape(T, zdim)[:T - 1, traj.components["Δt"].start]
    noise = ou_realisations(np.random.default_rng(seed), S, dts, sigma, tau)            # S x (T-1): one perturbation
    obj = qc.SweepNoiseInfidelityObjective(traj, system, [qc.GATES["Z"]], noise)
    idx = np.concatenate([t * zdim + np.arange(a.start, a.stop) for t in range(1, T - 1)])      # the first and last controls stay pinned
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
    profile = np.abs(obj.noise_sensitivity(z_after)[:, :, 0]).mean(axis=0)
    before, after = float(1.0 - F_before.mean()), float(1.0 - F_after.mean())
    if verbose:
        print(f"rollout fidelity of the solved pulse without noise: {f1:.6f}; {S} realisations, sigma = {sigma}, tau = {tau}")
        print(f"{res.nit} L-BFGS iterations, {res.nfev} gradient calls")
        print(f"mean infidelity over the realisations: {before:.3e} -> {after:.3e}")
        print("  interval   time      mean_s |dF_s/dxi_t|")
        for t, (tt, pr) in enumerate(zip(np.concatenate([[0.0], np.cumsum(dts)[:-1]]), profile)):
            print(f"  {t:5d}    {tt:7.3f}    {pr:.4e}")
    obj.close()
    return before, after, profile


if __name__ == "__main__":
    arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
    polish(max_iter=arg(1, 60), S=arg(2, 64), steps=arg(3, 60))
