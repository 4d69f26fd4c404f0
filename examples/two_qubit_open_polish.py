#!/usr/bin/env python3
"""Polish an entangling pulse against the OPEN two-qubit system it will run on: two qubits with a fixed ZZ coupling, each with energy
relaxation (T1) and pure dephasing in the Lindblad form,

    d rho/dt = -i [H_s(t), rho] + sum_L ( L rho L' - 1/2 {L'L, rho} ),
    H_s(t) = (J / 2) Z Z + (delta_s / 2) (Z I + I Z) + sum_q ( a_qx(t) X_q + a_qy(t) Y_q ) / 2,
    L = sqrt(1 / T1) |0><1|_q,  sqrt(gamma_phi / 2) Z_q        (q = 1, 2),

the transfer |00> -> (|00> - i |11>) / sqrt(2) (what exp(-i pi/4 X X) makes of |00>) scored by the density-operator fidelity
<psi| rho(T) |psi>, and a small grid of S common detunings delta_s as the sweep's `theta`.  levels^2 = 16, 2N = 32: the density operator is
one column of 32 entries and the handle takes the "mfma32-sweep" form.  The objective is
`SweepInfidelityObjective(wide=True, stored_states=True, wide_stored=True)`: every value is ONE wide sweep and every gradient ONE
backward walk over stored forward states on 2 x 2 tiles, all S detunings in one launch; scipy's L-BFGS-B moves the four controls
inside an amplitude bound, the timestep stays fixed.

Printed: the mean infidelity over the grid of the starting pulse and of the polished one.

    python examples/two_qubit_open_polish.py [T] [S] [steps]
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g

SX = np.array([[0, 1], [1, 0]], dtype=complex)
SY = np.array([[0, -1j], [1j, 0]], dtype=complex)
SZ = np.array([[1, 0], [0, -1]], dtype=complex)
SM = np.array([[0, 1], [0, 0]], dtype=complex)      # |0><1|
I2 = np.eye(2, dtype=complex)


def _iso_operator(L):
    return np.block([[L.real, -L.imag], [L.imag, L.real]])


def polish(T: int = 30, S: int = 5, steps: int = 80, duration: float = 8.0, coupling: float = 0.5, t1: float = 60.0, gamma_phi: float = 0.01,
           width: float = 0.1, bound: float = 2.0, verbose: bool = True):
    """(mean infidelity of the starting pulse, of the polished pulse) over the S detunings of the grid, on the open system."""
    from scipy.optimize import minimize
    qc = g.load_package()
    k = np.kron
    dt = duration / (T - 1)
    H0 = 0.5 * coupling * k(SZ, SZ)
    Hd = [0.5 * k(SX, I2), 0.5 * k(SY, I2), 0.5 * k(I2, SX), 0.5 * k(I2, SY)]
    Ls = [np.sqrt(1.0 / t1) * k(SM, I2), np.sqrt(1.0 / t1) * k(I2, SM), np.sqrt(gamma_phi / 2) * k(SZ, I2), np.sqrt(gamma_phi / 2) * k(I2, SZ)]
    system = qc.OpenQuantumSystem(H0, Hd, Ls)
    delta = np.linspace(-width, width, S).reshape(S, 1)
    detuning = _iso_operator(system.hamiltonian_superoperator(0.5 * (k(SZ, I2) + k(I2, SZ))))      # the commutator superoperator, a generator matrix
    rng = np.random.default_rng(0)
    a0 = 0.3 * rng.standard_normal((4, T))                                                       # a starting pulse with no structure
    psi = np.array([1.0, 0.0, 0.0, -1.0j]) / np.sqrt(2.0)
    goal_ket = np.concatenate([psi.real, psi.imag])                                               # [Re psi; Im psi]
    rho0 = np.zeros(32)
    rho0[0] = 1.0                                                                                 # |00><00| as [vec(Re rho); vec(Im rho)]
    traj = qc.NamedTrajectory({"ρ̃⃗": np.repeat(rho0[:, None], T, axis=1), "a": a0}, controls=("a",), timestep=dt, initial={"ρ̃⃗": rho0})
    obj = qc.SweepInfidelityObjective(traj, system, [detuning], delta, state_name="ρ̃⃗", goal_ket=goal_ket, wide=True, stored_states=True,
                                      wide_stored=True)
    z = np.array(traj.datavec, dtype=np.float64)
    a = traj.components["a"]
    idx = np.concatenate([t * traj.dim + np.arange(a.start, a.stop) for t in range(T - 1)])      # the last knot's controls enter no interval

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
        print(f"two qubits, ZZ coupling {coupling}, T1 = {t1}, gamma_phi = {gamma_phi}; pulse of {T - 1} intervals, duration {duration}; "
              f"{S} detunings in [-{width}, {width}]")
        print(f"polish on the open system: {res.nit} L-BFGS iterations, {res.nfev} gradient calls ({obj._sweep.kernel_name}, stored states)")
        print(f"mean infidelity over the detunings: {before:.4e} -> {after:.4e}")
    obj.close()
    return before, after


if __name__ == "__main__":
    arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
    polish(T=arg(1, 30), S=arg(2, 5), steps=arg(3, 80))
