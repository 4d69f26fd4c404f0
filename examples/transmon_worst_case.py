#!/usr/bin/env python3
"""Worst-case search for a two-transmon pulse, on the matrix cores: the two coupled three-level transmons of
examples/transmon_robustness.py (9 levels, 2N = 18), its smooth start pulse, the subspace fidelity on the computational levels, and the
search of examples/worst_case_search.py over the box

    zeta in [-width, width]  (detuning zeta b_1^dag b_1 of the first transmon),     c in [1 - amp, 1 + amp]  (one factor on all four drives)

for the system on which the pulse does worst.  The starts are a grid over the box; from every one of them a projected-gradient ascent
of the subspace infidelity 1 - F runs, all at once, and every iteration is ONE `RolloutSweep.param_grad` call on a handle made with
`wide=True, wide_params=True` (kernel "mfma32-sweep"): the S fidelities with dF_s/dzeta_s and dF_s/dc_{s,k} from one backward walk
(dF_s/dc_s is the sum over the four drives).  Without `wide_params` a system of this size has no parameter gradients and the same numbers
cost 2 (1 + 4) forward sweeps by central differences.  Printed: the grid's worst fidelity and the worst fidelity found.

    python examples/transmon_worst_case.py [T] [grid] [iters]
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as g
from transmon_robustness import SUBSPACE, LEVELS, goal_gate, two_transmons
from worst_case_search import ascend


def worst_case(T: int = 40, grid: int = 7, iters: int = 20, width: float = 2 * np.pi * 0.002, amp: float = 0.05, duration: float = 40.0,
               verbose: bool = True):
    """(grid_worst, found_worst, history, kernel): the largest infidelity among the grid x grid starts, the largest the ascents reached,
    the S infidelities after every iteration, and the kernel that served the calls."""
    qc = g.load_package()
    H0, drives, n1 = two_transmons()
    system = qc.QuantumSystem(H0, drives)
    N, m = LEVELS * LEVELS, len(drives)
    dts = np.full(T, duration / (T - 1))
    # the start pulse of transmon_robustness.run: half a Rabi turn on the first transmon's x drive, a little of everything else
    rng = np.random.default_rng(0)
    window = np.sin(np.pi * np.linspace(0.0, 1.0, T)) ** 2
    a = 0.1 * (np.pi / 2) / (duration * 0.5) * rng.uniform(-1, 1, (m, 1)) * window
    a[0] += (np.pi / 2) / (duration * 0.5) * window
    init, goal = qc.operator_to_iso_vec(np.eye(N, dtype=complex)), qc.operator_to_iso_vec(goal_gate())
    lo, hi = np.array([-width, 1.0 - amp]), np.array([width, 1.0 + amp])
    starts = np.array([(z, c) for z in np.linspace(lo[0], hi[0], grid) for c in np.linspace(lo[1], hi[1], grid)])

    sw = qc.RolloutSweep(system, [n1], T, goal=goal, fid_kind="unitary", subspace=SUBSPACE, wide=True, wide_params=True)
    try:
        kernel = sw.kernel_name
        Z = sw.pack(a, dts)

        def evaluate(x):
            fids, gth, gsc = sw.param_grad(Z, init, x[:, :1], np.repeat(x[:, 1:], m, axis=1))
            return 1.0 - fids, -np.concatenate([gth, gsc.sum(axis=1, keepdims=True)], axis=1)

        x, val, history = ascend(evaluate, starts, lo, hi, iters)
    finally:
        sw.close()
    k, b = int(np.argmax(history[0])), int(np.argmax(val))
    grid_worst, found_worst = float(history[0][k]), float(val[b])
    if verbose:
        mhz = lambda z: 1e3 * z / (2 * np.pi)
        print(f"two three-level transmons, {T} knots, kernel {kernel}; {grid} x {grid} starts, {iters} iterations ({iters + 1} param_grad calls)")
        print(f"grid:    worst fidelity {1.0 - grid_worst:.9f} at zeta / 2 pi = {mhz(starts[k, 0]):+.3f} MHz, c = {starts[k, 1]:.4f}")
        print(f"ascents: worst fidelity {1.0 - found_worst:.9f} at zeta / 2 pi = {mhz(x[b, 0]):+.3f} MHz, c = {x[b, 1]:.4f}")
        print(f"worst infidelity: grid {grid_worst:.12e} found {found_worst:.12e}")
    return grid_worst, found_worst, history, kernel


if __name__ == "__main__":
    arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
    worst_case(T=arg(1, 40), grid=arg(2, 7), iters=arg(3, 20))
