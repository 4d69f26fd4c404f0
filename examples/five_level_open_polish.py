#!/usr/bin/env python3
"""Polish a pi pulse against the OPEN five-level system it will run on: a transmon with its higher levels kept, energy relaxation down
the ladder and pure dephasing in the Lindblad form,

    d rho/dt = -i [H_s(t), rho] + sum_L ( L rho L' - 1/2 {L'L, rho} ),
    H_s(t) = delta_s n + (alpha / 2) n (n - 1) + ( a_x(t) (a + a') + i a_y(t) (a - a') ) / 2,        n = a'a,
    L = sqrt(1 / T1) a,  sqrt(gamma_phi) n,

the transfer |0> -> |1> scored by the density-operator fidelity <1| rho(T) |1>, and a small grid of S detunings delta_s as the sweep's
`theta`.  levels^2 = 25, 2N = 50: the density operator is one column of 50 entries and the handle takes the "mfma64-sweep" form.  The
objective is `SweepInfidelityObjective(wide=True, wide64=True, wide64_grad=True, stored_states=True, wide64_stored=True)`: every value
is ONE sweep and every gradient ONE backward walk over stored forward states on 4 x 4 tiles, all S detunings in one launch; scipy's
L-BFGS-B moves the two quadratures inside an amplitude bound, the timestep stays fixed.

Printed: the mean infidelity over the grid of the starting pulse and of the polished one.

    python examples/five_level_open_polish.py [T] [S] [steps]
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g

LEVELS = 5


def _iso_operator(L):
    return np.block([[L.real, -L.imag], [L.imag, L.real]])


def polish(T: int = 16, S: int = 3, steps: int = 20, duration: float = 6.0, alpha: float = -1.5, t1: float = 80.0, gamma_phi: float = 0.005,
           width: float = 0.05, bound: float = 2.0, verbose: bool = True):
    """(mean infidelity of the starting pulse, of the polished pulse) over the S detunings of the grid, on the open system."""
    from scipy.optimize import minimize
    qc = g.load_package()
    dt = duration / (T - 1)
    a = np.diag(np.sqrt(np.arange(1.0, LEVELS)), 1).astype(complex)
    num = a.conj().T @ a
    H0 = 0.5 * alpha * num @ (num - np.eye(LEVELS))
    Hd = [0.5 * (a + a.conj().T), 0.5j * (a - a.conj().T)]
    Ls = [np.sqrt(1.0 / t1) * a, np.sqrt(gamma_phi) * num]
    system = qc.OpenQuantumSystem(H0, Hd, Ls)
    delta = np.linspace(-width, width, S).reshape(S, 1)
    detuning = _iso_operator(system.hamiltonian_superoperator(num))      # the commutator superoperator, a generator matrix
    t = (np.arange(T) + 0.5) / T
    a0 = np.vstack([(np.pi / duration) * np.sin(np.pi * t) ** 2 * 2.0 * 0.8, np.zeros(T)])      # a smooth pulse of 0.8 pi: under-rotated, no DRAG
    goal = np.zeros(LEVELS, dtype=complex)
    goal[1] = 1.0
    goal_ket = np.concatenate([goal.real, goal.imag])                    # [Re psi; Im psi]
    rho0 = np.zeros(2 * LEVELS * LEVELS)
    rho0[0] = 1.0                                                        # |0><0| as [vec(Re rho); vec(Im rho)]
    traj = qc.NamedTrajectory({"ρ̃⃗": np.repeat(rho0[:, None], T, axis=1), "a": a0}, controls=("a",), timestep=dt, initial={"ρ̃⃗": rho0})
    obj = qc.SweepInfidelityObjective(traj, system, [detuning], delta, state_name="ρ̃⃗", goal_ket=goal_ket, wide=True, wide64=True,
                                      wide64_grad=True, stored_states=True, wide64_stored=True)
    z = np.array(traj.datavec, dtype=np.float64)
    comp = traj.components["a"]
    idx = np.concatenate([k * traj.dim + np.arange(comp.start, comp.stop) for k in range(T - 1)])      # the last knot's controls enter no interval

    def fun(v):
        zz = z.copy()
        zz[idx] = v
        J, fids, grad = obj.J_fids_grad(zz)
        return 1.0 - J, -grad[idx]

    before = obj.L(z)
    res = minimize(fun, z[idx], jac=True, method="L-BFGS-B", bounds=[(-bound, bound)] * idx.size, options={"maxiter": steps})
    zz = z.copy()
    zz[idx] = res.x
    after = obj.L(zz)
    if verbose:
        print(f"five-level transmon, anharmonicity {alpha}, T1 = {t1}, gamma_phi = {gamma_phi}; pulse of {T - 1} intervals, duration {duration}; "
              f"{S} detunings in [-{width}, {width}]")
        print(f"polish on the open system: {res.nit} L-BFGS iterations, {res.nfev} gradient calls ({obj._sweep.kernel_name}, stored states)")
        print(f"mean infidelity over the detunings: {before:.4e} -> {after:.4e}")
    obj.close()
    return before, after


if __name__ == "__main__":
    arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
    polish(T=arg(1, 16), S=arg(2, 3), steps=arg(3, 20))
