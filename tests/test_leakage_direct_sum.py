"""Leakage suppression and the direct-sum problem: `EmbeddedOperator.leakage_indices`, the L1 slack rows, the reference's
"Additional Objective" identity (unitary_smooth_pulse_problem.jl:311-340), the reference's "Construct direct sum problem"
cases (unitary_direct_sum_problem.jl:186-272) and the direct-sum objective against the numpy restatement."""
import numpy as np
import pytest

import terms_ext_reference as ref
from oracle_bridge import problem_from_inputs


def four_level(qc):
    a = np.diag(np.sqrt(np.arange(1.0, 4.0)), 1)
    return qc.QuantumSystem(np.zeros((4, 4)), [(a + a.T) / 2, (a - a.T) / 2j])


def leakage_inputs(qc, T=7, free_time=True):
    U_goal = qc.EmbeddedOperator("H", [0, 1], 4)
    inp = qc.unitary_smooth_pulse_inputs(four_level(qc), U_goal.embed(fill=1.0), T, 0.2, free_time=free_time)
    leak = U_goal.leakage_indices()
    return qc.add_l1_slacks(inp, "Ũ⃗", leak), leak


def test_leakage_indices(qc):
    idx = qc.EmbeddedOperator("H", [0, 1], 4).leakage_indices()
    # Ũ⃗ = vec(vcat(real(U), imag(U))): column c occupies 8c .. 8c+7, rows 2 and 3 lie outside {0, 1}
    np.testing.assert_array_equal(idx, [2, 3, 6, 7, 10, 11, 14, 15])
    U = np.zeros((4, 4), dtype=complex)
    U[2:, :2] = 1 + 1j
    np.testing.assert_array_equal(np.flatnonzero(qc.operator_to_iso_vec(U)), idx)
    # a subspace that is not a prefix: rows outside {1, 3}, columns inside it
    idx2 = qc.EmbeddedOperator("X", [1, 3], 4).leakage_indices()
    U = np.zeros((4, 4), dtype=complex)
    U[np.ix_([0, 2], [1, 3])] = 1 + 1j
    np.testing.assert_array_equal(np.flatnonzero(qc.operator_to_iso_vec(U)), idx2)


@pytest.mark.parametrize("free_time", [True, False])
def test_slack_rows(qc, free_time):
    inp, leak = leakage_inputs(qc, free_time=free_time)
    traj = inp.traj
    s1, s2 = qc.slack_names("Ũ⃗")
    assert traj.controls[-2:] == (s1, s2) and len(traj.components[s1]) == len(traj.components[s2]) == 8
    con = qc.L1SlackConstraint("Ũ⃗", traj, leak)
    assert con.dim == traj.T * 8
    Z = traj.datavec.copy()
    assert np.all(con.g(Z) == 0.0)                          # started at max(+-x, 0)
    rng = np.random.default_rng(0)
    Z = Z + rng.standard_normal(Z.size)
    X = Z.reshape(traj.T, traj.dim)
    off = traj.offset("Ũ⃗")
    want = (X[:, off + leak] - X[:, list(traj.components[s1])] + X[:, list(traj.components[s2])]).ravel()
    np.testing.assert_array_equal(con.g(Z), want)
    rows, cols = con.jac_structure
    J = np.zeros((con.dim, Z.size))
    np.add.at(J, (rows, cols), con.dg(Z))
    np.testing.assert_allclose(J @ Z, want, atol=1e-13)
    assert not hasattr(con, "mu_d2g")                        # linear: no Hessian


@pytest.mark.parametrize("free_time", [True, False])
def test_dynamics_never_read_the_slacks(qc, oracle, free_time):
    inp, leak = leakage_inputs(qc, T=6, free_time=free_time)
    prob = problem_from_inputs(inp)
    traj = inp.traj
    Z = traj.datavec
    slack = np.concatenate([np.array(traj.components[n]) for n in qc.slack_names("Ũ⃗")])
    r, c = oracle.jac_structure(prob)
    assert not np.isin(c % traj.dim, slack).any()
    hr, hc = oracle.hess_structure(prob)
    assert not np.isin(hr % traj.dim, slack).any() and not np.isin(hc % traj.dim, slack).any()
    Z2 = Z.copy().reshape(traj.T, traj.dim)
    Z2[:, slack] = np.random.default_rng(1).standard_normal((traj.T, slack.size))
    np.testing.assert_array_equal(oracle.F(prob, Z2.reshape(-1)), oracle.F(prob, Z))


def members(qc, n=2, T=50):
    """The reference test's members: 0.01 Z drift, X / Y drives, free_time=false."""
    sys_ = qc.QuantumSystem(0.01 * qc.GATES["Z"], [qc.GATES["X"], qc.GATES["Y"]])
    th = 0.33
    U_eps = np.cos(th / 2) * np.eye(2) - 1j * np.sin(th / 2) * qc.GATES["Y"]
    goals = [qc.GATES["X"], U_eps.conj().T @ qc.GATES["X"] @ U_eps, qc.GATES["X"]]
    return [qc.unitary_smooth_pulse_inputs(sys_, goals[k], T, 0.2, free_time=False, seed=k) for k in range(n)]


def names_with(inp, labels, names):
    return {nm + l for l in labels for nm in names}


def test_direct_sum_names_labels_and_graphs(qc):
    """The reference's "Construct direct sum problem" cases, on the host side: name sets, labels, a bad graph, a component-name
    graph, a triple and boundary values."""
    parts = members(qc)
    state_names = ["Ũ⃗"]
    control_names = ["dda"]
    ds = qc.unitary_direct_sum_inputs(parts)
    T = ds.traj
    assert set(T.names) == names_with(parts[0], "12", ["Ũ⃗", "a", "da", "dda"])
    assert set(T.controls) == names_with(parts[0], "12", control_names)
    assert {n for n in T.names if n.startswith("Ũ⃗")} == names_with(parts[0], "12", state_names)
    assert qc.direct_sum_graph(["1", "2"], None, {}, "dda", T.names) == ([("dda1", "dda2")], [])
    # labels
    ab = qc.unitary_direct_sum_inputs(parts, labels=["a", "b"]).traj
    assert set(ab.names) == names_with(parts[0], "ab", ["Ũ⃗", "a", "da", "dda"]) and set(ab.controls) == {"ddaa", "ddab"}
    assert qc.direct_sum_graph(["a", "b"], [("a", "b")], {}, "dda", ab.names) == ([("ddaa", "ddab")], [])
    # bad graph: raised before any device object is made
    with pytest.raises(ValueError):
        qc.direct_sum_graph(["a", "b"], [("x", "b")], {}, "dda", ab.names)
    with pytest.raises(ValueError):
        qc.unitary_direct_sum_problem(parts, 0.99, labels=["a", "b"], graph=[("x", "b")])
    # component-name graph (the reference's Symbol graph)
    assert qc.direct_sum_graph(["1", "2"], [("a1", "a2")], {}, "dda", T.names) == ([("a1", "a2")], [])
    # triple: the default chain has two edges, the middle member in both
    T3 = qc.unitary_direct_sum_inputs(members(qc, 3)).traj
    assert set(T3.names) == names_with(parts[0], "123", ["Ũ⃗", "a", "da", "dda"])
    assert qc.direct_sum_graph(["1", "2", "3"], None, {}, "dda", T3.names)[0] == [("dda1", "dda2"), ("dda2", "dda3")]
    # boundary values: an edge to a key of boundary_values becomes a baseline regulariser
    bv = {"x": np.array(parts[0].traj["dda"])}
    edges, boundary = qc.direct_sum_graph(["1", "2"], [("x", "1"), ("1", "2")], bv, "dda", T.names)
    assert edges == [("dda1", "dda2")] and len(boundary) == 1 and boundary[0][0] == "dda1"
    np.testing.assert_array_equal(boundary[0][1], bv["x"])
    with pytest.raises(ValueError):
        qc.unitary_direct_sum_problem(parts, 0.99, boundary_values={"1": bv["x"]})     # keys cannot be labels
    with pytest.raises(ValueError):
        qc.unitary_direct_sum_problem(parts, 0.99, drive_reset_ratio=1.5)


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_additional_objective_identity(qc):
    """L_vanilla + L_extra == L_additional, the reference's "Additional Objective" test."""
    sys_ = qc.QuantumSystem(qc.GATES["Z"], [qc.GATES["X"], qc.GATES["Y"]])
    vanilla = qc.unitary_smooth_pulse_problem(sys_, qc.GATES["H"], 50, 0.2)
    extra = qc.QuadraticSmoothnessRegularizer("dda", vanilla.traj, 10.0)
    additional = qc.unitary_smooth_pulse_problem(sys_, qc.GATES["H"], 50, 0.2, additional_objective=extra)
    Z = vanilla.traj.datavec
    np.testing.assert_array_equal(Z, additional.traj.datavec)
    L_extra = qc.TrajectoryObjective(extra, vanilla.traj)
    Lv = sum(o.L(Z) for o in vanilla.objectives)
    La = sum(o.L(Z) for o in additional.objectives)
    assert L_extra.L(Z) > 0.0
    assert abs(Lv + L_extra.L(Z) - La) <= 1e-12 * abs(La)
    for o in vanilla.objectives + additional.objectives + [L_extra]:
        o.close()


@pytest.mark.gpu
def test_leakage_problem_objective(qc):
    """The leakage template's trajectory objective = regularisers + R_leakage * sum(s1 + s2), against the restatement."""
    U_goal = qc.EmbeddedOperator("H", [0, 1], 4)
    prob = qc.unitary_smooth_pulse_problem(four_level(qc), U_goal, 50, 0.2, leakage_suppression=True, R_leakage=0.1, R=0.02)
    traj = prob.traj
    assert len(prob.objectives) == 2 and len(prob.constraints) == 1 and prob.constraints[0].dim == 50 * 8
    c = traj.components
    reg = np.sort(np.concatenate([np.asarray(c[n]) for n in ("a", "da", "dda")]))
    lin = np.concatenate([np.asarray(c[n]) for n in qc.slack_names("Ũ⃗")])
    tm = ref.TermsExt(T=50, zdim=traj.dim, off_dt=traj.offset("Δt"), reg_index=reg, reg_R=np.full(reg.size, 0.02), l_index=lin,
                      l_w=np.full(lin.size, 0.1))
    Z = traj.datavec + 0.01 * np.random.default_rng(2).standard_normal(traj.datavec.size)
    obj = prob.objectives[1]
    J, g, H = obj.L_grad_hess(Z)
    assert abs(J - ref.value(tm, Z)) <= 1e-12 * abs(J)
    np.testing.assert_allclose(g, ref.grad(tm, Z), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(H, ref.hess_values(tm, Z), rtol=1e-12, atol=1e-14)
    for o in prob.objectives:
        o.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["default", "labels", "names", "triple", "boundary"])
def test_direct_sum_problem_objective(qc, case):
    """The templates' objectives against the restatement; the boundary case returns two trajectory objectives."""
    n = 3 if case == "triple" else 2
    parts = members(qc, n)
    kw = dict(labels=["a", "b"], graph=[("a", "b")]) if case == "labels" else \
        dict(graph=[("a1", "a2")]) if case == "names" else \
        dict(graph=[("x", "1"), ("1", "2")], R_b=1e3, boundary_values={"x": np.array(parts[0].traj["dda"])}) if case == "boundary" else {}
    ds = qc.unitary_direct_sum_problem(parts, 0.99, Q=100.0, R=1e-2, fidelity_cost=(case == "triple"), **kw)
    traj = ds.traj
    labels = kw.get("labels", [str(i + 1) for i in range(n)])
    assert len(ds.constraints) == n and all(isinstance(c, qc.FinalUnitaryFidelityConstraint) for c in ds.constraints)
    n_traj = 2 if case == "boundary" else 1
    assert len(ds.objectives) == n_traj + (n if case == "triple" else 0)
    c = traj.components
    edges = {"default": [("dda1", "dda2")], "labels": [("ddaa", "ddab")], "names": [("a1", "a2")],
             "triple": [("dda1", "dda2"), ("dda2", "dda3")], "boundary": [("dda1", "dda2")]}[case]
    reg = np.concatenate([np.asarray(c[nm + l]) for l in labels for nm in ("a", "da", "dda")])
    o = np.argsort(reg)
    tm = ref.TermsExt(T=traj.T, zdim=traj.dim, dt_fixed=0.2, reg_index=reg[o], reg_R=np.full(reg.size, 1e-2),
                      p_a=np.concatenate([np.asarray(c[a]) for a, _ in edges]), p_b=np.concatenate([np.asarray(c[b]) for _, b in edges]),
                      p_Q=np.full(2 * len(edges), 100.0))
    Z = traj.datavec
    obj = ds.objectives[0]
    J, g, H = obj.L_grad_hess(Z)
    assert abs(J - ref.value(tm, Z)) <= 1e-12 * abs(J)
    np.testing.assert_allclose(g, ref.grad(tm, Z), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(H, ref.hess_values(tm, Z), rtol=1e-12, atol=1e-14)
    if case == "boundary":
        b = ref.TermsExt(T=traj.T, zdim=traj.dim, dt_fixed=0.2, reg_index=np.asarray(c["dda1"]), reg_R=np.full(2, 1e3),
                         baseline=np.array(parts[0].traj["dda"]).T)
        assert abs(ds.objectives[1].L(Z) - ref.value(b, Z)) <= 1e-12 * max(1.0, ref.value(b, Z))
    for x in ds.objectives + ds.constraints:
        x.close()


@pytest.mark.gpu
def test_leakage_solve():
    """examples/leakage_solve.py: the reference's 4-level, T = 50 leakage case (unitary_smooth_pulse_problem.jl:290-309).

    Measured on an MI355X (40 iterations): subspace rollout fidelity 0.3746 -> 0.5088, max |slack row| 7.9e-12, max |dynamics
    residual| 3.3e-5.  The summed |leakage entries| over all knots rose 3.03 -> 18.96: at R_leakage = 0.1 against Q = 100 the
    fidelity term dominates, and the reference's test asserts only the fidelity."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import leakage_solve
    out = leakage_solve.solve(verbose=False)
    print(out)
    assert out["n_leakage"] == 8
    assert out["fidelity_after"] > out["fidelity_before"]
    assert out["slack_residual"] < 1e-6
    assert out["dynamics_residual"] < 1e-2


@pytest.mark.gpu
def test_direct_sum_solve():
    """examples/direct_sum_solve.py: two 1-qubit members, each solved for 30 iterations, joined by the pairwise term on dda.

    Measured on an MI355X: members' final-knot fidelities 0.518 and 0.935 (the constraint floor 0.5175); in 30 direct-sum
    iterations the pairwise term fell 89.49 -> 1.1e-4 with both fidelity constraints held (residuals +0.351, +0.268) and max
    |dynamics residual| 1.6e-3."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import direct_sum_solve
    out = direct_sum_solve.solve(verbose=False)
    print(out)
    assert out["pairwise_after"] < out["pairwise_before"]
    assert min(out["fidelity_residuals"]) >= -1e-3
    assert out["dynamics_residual"] < 1e-2
