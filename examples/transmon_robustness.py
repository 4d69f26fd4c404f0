#!/usr/bin/env python3
"""Robustness of a two-transmon pulse against a frequency error, on the matrix cores: two coupled three-level transmons (9 levels,
2N = 18), a short pulse, the subspace fidelity on the computational levels {|00>, |01>, |10>, |11>}.

    H(a) = sum_q -(alpha_q / 2) b_q^dag b_q^dag b_q b_q + g (b_1^dag b_2 + b_1 b_2^dag) + sum_q a_qx (b_q + b_q^dag) + a_qy i (b_q^dag - b_q)
    H_s  = H + zeta_s b_1^dag b_1                    (the first transmon detuned by zeta_s)

in the frame rotating with the drives (energies in rad / ns).  The detuning landscape F(zeta) is ONE wide sweep
(`RolloutSweep(..., wide=True)`, kernel "mfma32-sweep"); a few L-BFGS steps then lower the MEAN infidelity over a detuning grid through
`SweepInfidelityObjective(wide=True)`, every gradient one adjoint sweep.  Without `wide` a system of this size runs one rollout per
sample and has no sweep gradient.

    python examples/transmon_robustness.py [T] [grid] [steps]
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g

LEVELS = 3
SUBSPACE = [0, 1, 3, 4]          # |q1 q2> has index 3 q1 + q2


def two_transmons(alpha=(2 * np.pi * 0.22, 2 * np.pi * 0.20), coupling=2 * np.pi * 0.004):
    """(H_drift, [four drive operators], number operator of the first transmon), 9 x 9 complex."""
    b = np.diag(np.sqrt(np.arange(1.0, LEVELS)), 1).astype(complex)
    one = np.eye(LEVELS, dtype=complex)
    b1, b2 = np.kron(b, one), np.kron(one, b)
    dag = lambda A: A.conj().T
    H0 = sum(-0.5 * al * dag(bq) @ dag(bq) @ bq @ bq for al, bq in zip(alpha, (b1, b2))) + coupling * (dag(b1) @ b2 + b1 @ dag(b2))
    drives = [bq + dag(bq) for bq in (b1, b2)] + [1j * (dag(bq) - bq) for bq in (b1, b2)]
    return H0, drives, dag(b1) @ b1


def goal_gate():
    """X on the first transmon's qubit, identity on the second, embedded in the 9 levels (identity outside the subspace)."""
    U = np.eye(LEVELS * LEVELS, dtype=complex)
    X = np.array([[0, 1], [1, 0]], dtype=complex)
    U[np.ix_(SUBSPACE, SUBSPACE)] = np.kron(X, np.eye(2))
    return U


def run(T: int = 40, grid: int = 9, steps: int = 12, landscape: int = 41, width: float = 2 * np.pi * 0.002, duration: float = 40.0,
        verbose: bool = True):
    """Returns the mean infidelity over the grid after every accepted L-BFGS step (`history`, the start value first), the landscape
    before and after over `landscape` detunings in [-2 width, 2 width], and the kernel that served the sweeps."""
    from scipy.optimize import minimize
    qc = g.load_package()
    H0, drives, n1 = two_transmons()
    system = qc.QuantumSystem(H0, drives)
    N, m = LEVELS * LEVELS, len(drives)
    dt = duration / (T - 1)
    # a smooth start: half a Rabi turn on the first transmon's x drive, a little of everything else
    rng = np.random.default_rng(0)
    tt = np.linspace(0.0, 1.0, T)
    window = np.sin(np.pi * tt) ** 2
    a = 0.1 * (np.pi / 2) / (duration * 0.5) * rng.uniform(-1, 1, (m, 1)) * window
    a[0] += (np.pi / 2) / (duration * 0.5) * window
    iso = lambda U: np.concatenate([U.reshape(-1, order="F").real, U.reshape(-1, order="F").imag])
    init, goal = iso(np.eye(N, dtype=complex)), iso(goal_gate())
    traj = qc.NamedTrajectory({"Ũ⃗": np.repeat(init[:, None], T, axis=1), "a": a, "Δt": np.full((1, T), dt)}, controls=("a",), timestep="Δt",
                              initial={"Ũ⃗": init}, goal={"Ũ⃗": goal})
    # the landscape: one wide sweep over every detuning
    zl = np.linspace(-2 * width, 2 * width, landscape)
    sweep = qc.RolloutSweep(system, [n1], T, goal=goal, fid_kind="unitary", subspace=SUBSPACE, zdim=traj.dim, off_a=traj.offset("a"),
                            off_dt=traj.offset("Δt"), wide=True)
    kernel = sweep.kernel_name
    z = np.array(traj.datavec, dtype=np.float64)
    F_before = sweep.eval(z, init, zl[:, None], finals=False)[1]
    # polish the mean infidelity over the grid; the first and last controls stay pinned, the timesteps as they are
    zetas = np.linspace(-width, width, grid)
    obj = qc.SweepInfidelityObjective(traj, system, [n1], zetas[:, None], subspace=SUBSPACE, wide=True)
    rows = traj.components["a"]
    idx = np.concatenate([t * traj.dim + np.arange(rows.start, rows.stop) for t in range(1, T - 1)])
    bound = 4.0 * float(np.abs(a).max())

    last = {}

    def fun(v):
        zz = z.copy()
        zz[idx] = v
        J, fids, grad = obj.J_fids_grad(zz)
        last["v"], last["L"] = v.copy(), 1.0 - J
        return 1.0 - J, -grad[idx]

    history = [fun(z[idx])[0]]

    def accepted(v):      # L-BFGS-B accepts the point of its last evaluation: no sweep of its own
        history.append(last["L"] if np.array_equal(last["v"], v) else fun(v)[0])

    res = minimize(fun, z[idx], jac=True, method="L-BFGS-B", bounds=[(-bound, bound)] * idx.size, callback=accepted, options={"maxiter": steps})
    z_after = z.copy()
    z_after[idx] = res.x
    F_after = sweep.eval(z_after, init, zl[:, None], finals=False)[1]
    if verbose:
        print(f"two three-level transmons, {T} knots of {dt:.2f} ns, kernel {kernel}; {res.nit} L-BFGS steps, {res.nfev + 1} gradient calls")
        print("mean infidelity over the grid after every step: " + " ".join(f"{v:.3e}" for v in history))
        print("  zeta / 2 pi (MHz)    F before      F after")
        for zt, fb, fa in zip(zl[::max(1, landscape // 10)], F_before[::max(1, landscape // 10)], F_after[::max(1, landscape // 10)]):
            print(f"  {1e3 * zt / (2 * np.pi):+10.3f}        {fb:.6f}     {fa:.6f}")
    obj.close()
    sweep.close()
    return dict(history=history, landscape_before=F_before, landscape_after=F_after, detunings=zl, kernel=kernel, controls=z_after[idx])


if __name__ == "__main__":
    arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
    run(T=arg(1, 40), grid=arg(2, 9), steps=arg(3, 12))
