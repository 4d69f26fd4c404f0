#!/usr/bin/env python3
"""Polishing a three-transmon pulse against a frequency error, on the matrix cores: the system of three_transmon_robustness.py (three
coupled three-level transmons, 27 levels, 2N = 54), the eight computational columns |q1 q2 q3> of the propagator as the state, and a few
steps of scipy's L-BFGS-B on the mean subspace infidelity over a grid of detunings of the first transmon,

    L(a) = mean_s (1 - |tr(G^dag U_s[sub, sub])|^2 / 64),        H_s = H(a) + zeta_s b_1^dag b_1.

The loss is written in torch on the final states of `RolloutSweep.finals_autograd`; every gradient is ONE pullback of the sweep over all
detunings (`qc_sweep_vjp_dev`).  At this size that needs `RolloutSweep(..., wide=True, wide64=True, wide64_grad=True)`: the forward sweep
"mfma64-sweep" and its closed adjoint walk, one workgroup per (sample, chunk of intervals) with the 64 x 64 matrices in LDS.  Eight of the
27 columns are enough for the subspace fidelity and cost a single column tile.

    python examples/three_transmon_polish.py [T] [grid] [steps]          (small sizes, e.g. 6 3 2, run in seconds)
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch
from scipy.optimize import minimize

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
from three_transmon_robustness import LEVELS, SUBSPACE, goal_gate, three_transmons


def run(T: int = 40, grid: int = 9, steps: int = 10, width: float = 2 * np.pi * 0.002, duration: float = 40.0, verbose: bool = True):
    """Returns the mean infidelity over `grid` detunings in [-width, width] before and after `steps` L-BFGS iterations on the controls."""
    qc = g.load_package()
    H0, drives, n1 = three_transmons()
    system = qc.QuantumSystem(H0, drives)
    N, m, cols = LEVELS ** 3, len(drives), len(SUBSPACE)
    dt = duration / (T - 1)
    rng = np.random.default_rng(0)
    window = np.sin(np.pi * np.linspace(0.0, 1.0, T)) ** 2
    a0 = 0.1 * (np.pi / 2) / (duration * 0.5) * rng.uniform(-1, 1, (m, 1)) * window
    a0[0] += (np.pi / 2) / (duration * 0.5) * window
    # the state: the computational columns of the identity, [Re; Im] per column
    E = np.zeros((2 * N, cols))
    E[SUBSPACE, np.arange(cols)] = 1.0
    zeta = np.linspace(-width, width, grid)[:, None]
    dev = torch.device("cuda:0")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)
    Gsub = goal_gate()[np.ix_(SUBSPACE, SUBSPACE)]
    Gr, Gi = t(Gsub.real), t(Gsub.imag)
    sub = torch.tensor(SUBSPACE, device=dev)
    sweep = qc.RolloutSweep(system, [n1], T, cols=cols, wide=True, wide64=True, wide64_grad=True)
    try:
        kernel = sweep.kernel_name
        init, theta, dts = t(E.reshape(-1, order="F")), t(zeta), torch.full((T, 1), dt, dtype=torch.float64, device=dev)

        def loss_of(a):
            Z = torch.cat([a.T, dts], dim=1).reshape(-1)                 # knot layout [a, dt]
            X = sweep.finals_autograd(Z, init, theta).reshape(grid, cols, 2 * N)      # [sample, column, row]
            Ur, Ui = X[:, :, :N][:, :, sub].transpose(1, 2), X[:, :, N:][:, :, sub].transpose(1, 2)      # [sample, sub row, column]
            tr = (Gr * Ur + Gi * Ui).sum(dim=(1, 2))                      # tr(G^dag U): real and imaginary part
            ti = (Gr * Ui - Gi * Ur).sum(dim=(1, 2))
            return (1.0 - (tr * tr + ti * ti) / cols ** 2).mean()

        def fun(v):      # value and gradient for scipy: one forward sweep and one pullback
            a = t(v.reshape(m, T)).requires_grad_(True)
            value = loss_of(a)
            value.backward()
            return float(value.detach()), a.grad.cpu().numpy().ravel()

        before, g0 = fun(a0.ravel())
        grad_norm = float(np.linalg.norm(g0))
        bound = 4.0 * np.abs(a0).max()
        res = minimize(fun, a0.ravel(), jac=True, method="L-BFGS-B", bounds=[(-bound, bound)] * a0.size, options={"maxiter": steps})
        after, controls = float(res.fun), res.x.reshape(m, T)
    finally:
        sweep.close()
    if verbose:
        print(f"three three-level transmons (27 levels, 2N = 54), {T} knots of {dt:.2f} ns, {cols} state columns, {grid} detunings per sweep")
        print(f"kernel {kernel}; mean subspace infidelity {before:.6f} -> {after:.6f} after {res.nit} L-BFGS iterations, {res.nfev} pullbacks "
              f"(|grad| at the start {grad_norm:.3e})")
    return dict(before=before, after=after, kernel=kernel, columns=cols, levels=N, grad_norm=grad_norm, controls=controls, iterations=res.nit)


if __name__ == "__main__":
    arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
    run(T=arg(1, 40), grid=arg(2, 9), steps=arg(3, 10))
