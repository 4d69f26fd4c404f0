#!/usr/bin/env python3
"""Polish a two-transmon pulse against a frequency error with EXACT curvature, on the matrix cores: the problem of
examples/transmon_gauss_newton.py -- two coupled three-level transmons (9 levels, 2N = 18, "mfma32-sweep"), an X gate on the first, the
squared distance of the computational columns to the goal inside the computational subspace plus the population they leave outside it,
over a grid of detunings of the first transmon -- driven by the truncated-Newton loop of examples/robust_newton_cg.py.

The loss is a `SweepFinalStateObjective(..., wide=True, wide_tangent=True, wide_hessian=True)`.  Every product with its Hessian is
`hessian_times`: one wide pushforward (`qc_sweep_jvp_dev`, QC_SWEEP_WIDE_TANGENT) and one wide tangent pullback (`qc_sweep_hvp_dev`,
QC_SWEEP_WIDE_HESSIAN), whatever the number of detunings.  It is the Gauss-Newton product of transmon_gauss_newton.py plus the curvature
of the sweep map, sum_s <dl/dx_s, d2 x_s / dZ2 v>, which for the leakage term -- small residuals, strongly curved states -- is what
Gauss-Newton misses.  Where the first conjugate-gradient direction already has non-positive curvature the step falls back to
`gauss_newton_times`, as there.  The trajectory vector, the directions and every product stay on the device.

    python examples/transmon_newton_cg.py [T] [grid] [steps]
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from robust_newton_cg import truncated_newton
from transmon_gauss_newton import problem


def main(T: int = 40, grid: int = 9, steps: int = 8, weight: float = 1.0, width: float = 2 * np.pi * 0.002, duration: float = 40.0,
         cg_iter: int = 20, halvings: int = 5, damping: float = 1.0, verbose: bool = True):
    """Returns what robust_newton_cg.main returns (the loss after every accepted step, the counts, the `summary` line) plus the mean
    leakage before and after."""
    obj, Z, idx, leakage, dt = problem(T, grid, weight, width, duration, wide_tangent=True, wide_hessian=True)
    leak_before = leakage(Z)
    # the start pulse is far from the goal: a small lambda oversteps (transmon_gauss_newton.py)
    res = truncated_newton(obj, Z, idx, steps, cg_iter=cg_iter, halvings=halvings, lam=damping, verbose=verbose)
    leak_after = leakage(res["Z"])
    out = dict(res, kernel=obj._sweep.kernel_name, T=T, S=grid, controls=res["Z"].cpu().numpy(), leakage_before=leak_before,
               leakage_after=leak_after)
    del out["Z"]
    if verbose:
        print(f"two three-level transmons, {T} knots of {dt:.2f} ns, {grid} detunings in [-{width:.4f}, {width:.4f}] rad / ns, kernel {out['kernel']}")
        print(out["summary"])
        print(f"mean leakage {leak_before:.3e} -> {leak_after:.3e}")
    obj.close()
    return out


if __name__ == "__main__":
    arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
    main(T=arg(1, 40), grid=arg(2, 9), steps=arg(3, 8))
