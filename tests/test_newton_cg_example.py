"""examples/newton_cg_solve.py: the Hadamard problem by the augmented-Lagrangian loop of examples/al_solve.py with a truncated-Newton
inner loop on the device -- conjugate gradients on hess L_rho v = hess J v + ((lam + rho F) d2F) v + rho dF'(dF v), the middle term
through qc_eval_hvp_dev; no Jacobian or Hessian value of the dynamics leaves the library.  Asserts what tests/test_al_example.py asserts
(the reference's `@test final > initial`, unitary_smooth_pulse_problem.jl:218-221): the rollout fidelity improved, and the dynamics
residual shrank.  No level is fixed."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_newton_cg_solve_improves_fidelity_and_feasibility(qc):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import newton_cg_solve
    f0, f1, v0, v1 = newton_cg_solve.solve(T=20, outer=5, inner=5, cg=15, verbose=False)
    print(f"rollout fidelity {f0:.6f} -> {f1:.6f}, |F|_inf {v0:.3e} -> {v1:.3e}")
    assert f1 > f0, (f0, f1)
    assert v1 < v0, (v0, v1)
