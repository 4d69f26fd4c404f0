"""examples/al_solve.py: the Hadamard problem by an augmented-Lagrangian loop on the device -- F, the fidelity's and the regularisers'
gradients and the transposed product dF'(lam + rho F) through qc_eval_vjp_dev; no Jacobian value leaves the library.  Asserts what the reference's own
solve tests assert (`@test final > initial`, unitary_smooth_pulse_problem.jl:218-221): the rollout fidelity improved, and the
dynamics residual shrank.  No fidelity level is fixed (observed numbers: profiles/products_summary.txt)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_augmented_lagrangian_solve_improves_fidelity_and_feasibility(qc):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import al_solve
    f0, f1, v0, v1 = al_solve.solve(T=20, outer=6, inner=25, verbose=False)
    print(f"rollout fidelity {f0:.6f} -> {f1:.6f}, |F|_inf {v0:.3e} -> {v1:.3e}")
    assert f1 > f0, (f0, f1)
    assert v1 < v0, (v0, v1)
