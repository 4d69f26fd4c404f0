"""The reference's "Robust and Subspace Templates" (src/problem_templates/unitary_robustness_problem.jl:129-180) through
examples/robust_solve.py: a smooth-pulse solve on a 3-level system, then the robustness problem from its solution with the exact
dense Hessian of the robustness term inside the KKT solve (V = 51 knots x (8 subspace entries + dt) = 459 variables).

Measured on an MI355X (40 + 50 iterations): subspace rollout fidelity 0.0240 -> 0.1384 in stage 1; robustness loss
0.5200 -> 0.2572 in stage 2 with the final fidelity held above 0.2149 (residual +0.537) and max |dynamics residual| 2.3e-3."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_robust_and_subspace_templates():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import robust_solve
    out = robust_solve.solve(verbose=False)
    print(out)
    assert out["n_robust_vars"] == 459
    assert out["fidelity_after"] > out["fidelity_before"]              # stage 1: the subspace gate improves
    assert out["robustness_after"] < out["robustness_before"]          # stage 2: more robust (no `before < 0.25` escape)
    assert out["fidelity_residual"] >= -1e-3
    assert out["dynamics_residual"] < 1e-2
