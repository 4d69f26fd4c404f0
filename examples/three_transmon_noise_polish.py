#!/usr/bin/env python3
"""Polish a three-transmon pulse against qubit frequencies that DRIFT during the gate, on the matrix cores: examples/transmon_noise_polish.py
at the size of examples/three_transmon_robustness.py -- three coupled three-level transmons, 27 levels, 2N = 54, "mfma64-sweep" -- with an
Ornstein-Uhlenbeck detuning on EACH transmon (flux noise),

    H_s(t) = H_drift + sum_q xi_{s,q}(t) n_q + sum_k a_k(t) H_k,      n_q the number operator of transmon q,

three perturbations whose amplitudes change from interval to interval (n_pert = 3), S realisations drawn once (common random numbers, the
sampler of examples/noise_robust_polish.py).  The objective is the mean infidelity in the computational subspace,
`SweepNoiseInfidelityObjective(..., wide=True, wide64=True, wide64_grad=True, wide64_noise=True)`: every value is ONE noise sweep and every
gradient ONE adjoint noise sweep in the 4 x 4-tile form (`qc_sweep_noise_eval`, `qc_sweep_noise_grad` with QC_SWEEP_WIDE_64_NOISE), all S
realisations in one launch.  A few L-BFGS steps move the controls of knots 1 .. T-2; the timesteps stay.  Printed: the mean infidelity
before and after, and per interval the largest |dF_s/dxi_{s,t,q}| over the realisations of the polished pulse for each transmon -- when in
the gate a frequency kick hurts most.

    python examples/three_transmon_noise_polish.py [T] [S] [steps]          (the defaults are small: seconds)
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as g
from noise_robust_polish import ou_realisations
from three_transmon_robustness import LEVELS, SUBSPACE, goal_gate, three_transmons
from three_transmon_worst_case import number_operators


def polish(T: int = 12, S: int = 8, steps: int = 5, sigma: float = 2 * np.pi * 0.002, tau: float = 20.0, duration: float = 40.0,
           seed: int = 0, verbose: bool = True):
    """(mean infidelity before, after, profile, kernel) over S realisations of the three detunings; profile[t, q] = max_s |dF_s/dxi_{t,q}|
    of the polished pulse, (T-1) x 3."""
    from scipy.optimize import minimize
    qc = g.load_package()
    H0, drives, _ = three_transmons()
    numbers = number_operators()
    system = qc.QuantumSystem(H0, drives)
    N, m = LEVELS ** 3, len(drives)
    dt = duration / (T - 1)
    # the start of three_transmon_polish.py: half a Rabi turn on the first transmon's x drive, a little of everything else
    rng = np.random.default_rng(seed)
    window = np.sin(np.pi * np.linspace(0.0, 1.0, T)) ** 2
    a = 0.1 * (np.pi / 2) / (duration * 0.5) * rng.uniform(-1, 1, (m, 1)) * window
    a[0] += (np.pi / 2) / (duration * 0.5) * window
    init = np.asarray(qc.operator_to_iso_vec(np.eye(N, dtype=complex)), dtype=np.float64)
    traj = qc.NamedTrajectory({"Ũ⃗": np.repeat(init[:, None], T, axis=1), "a": a, "Δt": np.full((1, T), dt)}, controls=("a",), timestep="Δt",
                              initial={"Ũ⃗": init}, goal={"Ũ⃗": np.asarray(qc.operator_to_iso_vec(goal_gate()), dtype=np.float64)})
    dts = np.full(T - 1, dt)
    noise = np.stack([ou_realisations(rng, S, dts, sigma, tau) for _ in numbers], axis=2)      # S x (T-1) x 3: independent detunings
    obj = qc.SweepNoiseInfidelityObjective(traj, system, numbers, noise, subspace=SUBSPACE, wide=True, wide64=True, wide64_grad=True,
                                           wide64_noise=True)
    kernel = obj._sweep.kernel_name
    z = np.array(traj.datavec, dtype=np.float64)
    rows = traj.components["a"]
    idx = np.concatenate([t * traj.dim + np.arange(rows.start, rows.stop) for t in range(1, T - 1)])      # the first and last controls stay pinned

    def fun(v):
        zz = z.copy()
        zz[idx] = v
        J, fids, grad = obj.J_fids_grad(zz)
        return 1.0 - J, -grad[idx]

    before = float(1.0 - obj.fidelities(z).mean())
    res = minimize(fun, z[idx], jac=True, method="L-BFGS-B", options={"maxiter": steps})
    z_after = z.copy()
    z_after[idx] = res.x
    after = float(1.0 - obj.fidelities(z_after).mean())
    profile = np.abs(obj.noise_sensitivity(z_after)).max(axis=0)
    if verbose:
        print(f"three three-level transmons (27 levels, 2N = 54), {T} knots of {dt:.2f} ns, kernel {kernel}; {S} realisations of three "
              f"Ornstein-Uhlenbeck detunings, sigma = {sigma:.4f} rad / ns, tau = {tau} ns")
        print(f"{res.nit} L-BFGS iterations, {res.nfev} gradient calls (one adjoint noise sweep each)")
        print(f"mean subspace infidelity over the realisations: {before:.3e} -> {after:.3e}")
        print("  interval   time      max_s |dF_s/dxi_t|: transmon 1   transmon 2   transmon 3")
        for t in range(T - 1):
            print(f"  {t:5d}    {t * dt:7.3f}    {profile[t, 0]:.4e}   {profile[t, 1]:.4e}   {profile[t, 2]:.4e}")
    obj.close()
    return before, after, profile, kernel


if __name__ == "__main__":
    arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
    polish(T=arg(1, 12), S=arg(2, 8), steps=arg(3, 5))
