#!/usr/bin/env python3
"""Worst-case search over a box of system errors: take the solved 1-qubit Hadamard pulse of examples/robustness_landscape.py and look
for the system inside

    theta in [-0.05, 0.05]  (detuning theta Z),     c_1, c_2 in [0.95, 1.05]  (relative amplitude of the X and Y drives)

on which the pulse does worst.  S projected-gradient ascents of the infidelity 1 - F run at once, one per start, with backtracking and
a step size per start; every iteration is ONE call of `RolloutSweep.param_grad` (`qc_sweep_grad_params`), which returns the S
fidelities and their derivatives with respect to theta and c from one backward walk.  The box's eight corners are among the starts.
The result is printed beside the worst of a 9 x 9 x 9 grid over the box, evaluated by one `rollout_sweep` call.

    python examples/worst_case_search.py [T] [starts] [iters]
"""
from __future__ import annotations

import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

LO = np.array([-0.05, 0.95, 0.95])
HI = np.array([0.05, 1.05, 1.05])


def ascend(evaluate, x0, lo, hi, iters):
    """Projected-gradient ascent of S functions at once.  evaluate(x) -> (values S, gradients S x d) at the S points x (S x d); every
    iteration calls it once, at the candidates x_s + step_s g_s clipped to the box.  A candidate that does not lower its start's value
    is taken and the start's step doubles; otherwise the start stays where it is and its step halves.  Returns (x, values, history):
    history[i] are the S values after i iterations, non-decreasing in i for every start."""
    x = np.clip(np.asarray(x0, dtype=np.float64), lo, hi)
    val, grad = evaluate(x)
    # first steps of a quarter of the box's smallest width along the gradient
    gmax = np.abs(grad).max(axis=1)
    step = 0.25 * float(np.min(hi - lo)) / np.where(gmax > 0, gmax, 1.0)
    history = [val.copy()]
    for _ in range(iters):
        cand = np.clip(x + step[:, None] * grad, lo, hi)
        cval, cgrad = evaluate(cand)
        take = cval >= val
        x[take], val[take], grad[take] = cand[take], cval[take], cgrad[take]
        step = np.where(take, 2.0 * step, 0.5 * step)
        history.append(val.copy())
    return x, val, history


def box_starts(starts, lo, hi, rng):
    """The box's corners, then uniform draws."""
    corners = np.array(list(itertools.product(*zip(lo, hi))))
    if starts < len(corners):
        raise ValueError(f"at least {len(corners)} starts: the box's corners")
    return np.concatenate([corners, rng.uniform(lo, hi, (starts - len(corners), len(lo)))])


def worst_case(T: int = 50, starts: int = 64, iters: int = 30, max_iter: int = 60, verbose: bool = True, seed: int = 0):
    """(grid_worst, found_worst, history): the largest infidelity over the 9^3 grid, the largest the ascents reached, and the S
    infidelities after every iteration."""
    import __graft_entry__ as g
    from solve_hadamard import solve
    qc = g.load_package()
    f0, f1, viol, z, traj, system = solve(max_iter, T=T, verbose=False, return_solution=True)
    zdim, comps = traj.dim, traj.components
    K = np.asarray(z)[:traj.T * zdim].reshape(traj.T, zdim)
    controls = K[:, comps["a"].start:comps["a"].stop].T.copy()
    dts = K[:, comps["Δt"].start].copy()
    init = qc.operator_to_iso_vec(np.eye(2, dtype=complex))
    goal = qc.operator_to_iso_vec(qc.GATES["H"])
    perts = [qc.GATES["Z"]]

    axes = [np.linspace(l, h, 9) for l, h in zip(LO, HI)]
    grid = np.array(list(itertools.product(*axes)))
    _, F_grid = qc.rollout_sweep(init, controls, dts, system, perts, grid[:, :1], grid[:, 1:], goal=goal, fid_kind="unitary")
    k = int(np.argmin(F_grid))
    grid_worst = float(1.0 - F_grid[k])

    sw = qc.RolloutSweep(system, perts, T, goal=goal, fid_kind="unitary")
    try:
        Z = sw.pack(controls, dts)

        def evaluate(x):
            fids, gth, gsc = sw.param_grad(Z, init, x[:, :1], x[:, 1:])
            return 1.0 - fids, -np.concatenate([gth, gsc], axis=1)

        x, val, history = ascend(evaluate, box_starts(starts, LO, HI, np.random.default_rng(seed)), LO, HI, iters)
    finally:
        sw.close()
    b = int(np.argmax(val))
    found_worst = float(val[b])
    if verbose:
        print(f"rollout fidelity of the solved pulse: {f1:.6f}")
        print(f"9 x 9 x 9 grid:  worst infidelity {grid_worst:.6e} at theta = {grid[k, 0]:+.4f}, c = ({grid[k, 1]:.4f}, {grid[k, 2]:.4f})")
        print(f"{starts} ascents, {iters} iterations ({iters + 1} param_grad calls): worst infidelity {found_worst:.6e} at "
              f"theta = {x[b, 0]:+.4f}, c = ({x[b, 1]:.4f}, {x[b, 2]:.4f}); "
              f"{int(np.sum(val >= grid_worst - 1e-9))} of {starts} starts reached the grid's worst or better")
    return grid_worst, found_worst, history


if __name__ == "__main__":
    arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
    worst_case(T=arg(1, 50), starts=arg(2, 64), iters=arg(3, 30))
