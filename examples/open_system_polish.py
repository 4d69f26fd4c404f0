#!/usr/bin/env python3
"""Polish a pulse against the OPEN system it will run on: one qubit with energy relaxation (T1) and pure dephasing (T2) in the Lindblad
form,

    d rho/dt = -i [H_s(t), rho] + sum_L ( L rho L' - 1/2 {L'L, rho} ),     H_s(t) = (delta_s / 2) Z + a_x(t) X / 2 + a_y(t) Y / 2,
    L_1 = sqrt(1 / T1) |0><1|,   L_2 = sqrt(gamma_phi / 2) Z,

a state transfer |0> -> |1> (an X gate on the ground state) scored by the density-operator fidelity <1| rho(T) |1>, and a grid of S
detunings delta_s as the sweep's `theta`.  The objective is `SweepInfidelityObjective(stored_states=True)`: every value is ONE sweep and
every gradient ONE backward walk over stored forward states (`qc_sweep_grad` on a handle with reserved1[0] = QC_SWEEP_STORED_STATES),
all S detunings in one launch; scipy's L-BFGS-B moves the controls inside an amplitude bound, the timestep stays fixed.

Printed: the mean infidelity over the grid of the starting pulse (a resonant square pi pulse) and of the polished one, and the same
figure -- on the open system -- for the pulse polished on the CLOSED model of the same qubit (ket fidelity, no dissipators): what
ignoring T1 / T2 during the polish costs.

    python examples/open_system_polish.py [T] [S] [steps]
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


def _iso_operator(L):
    return np.block([[L.real, -L.imag], [L.imag, L.real]])


def polish(T: int = 24, S: int = 9, steps: int = 60, duration: float = 6.0, t1: float = 40.0, gamma_phi: float = 0.02, width: float = 0.5,
           bound: float = 2.0, verbose: bool = True):
    """(mean infidelity of the starting pulse, of the pulse polished on the open system, of the pulse polished on the closed model),
    all three over the S detunings of the grid and on the open system."""
    from scipy.optimize import minimize
    qc = g.load_package()
    dt = duration / (T - 1)
    Hd = [0.5 * SX, 0.5 * SY]
    open_sys = qc.OpenQuantumSystem(np.zeros((2, 2)), Hd, [np.sqrt(1.0 / t1) * SM, np.sqrt(gamma_phi / 2) * SZ])
    closed_sys = qc.QuantumSystem(np.zeros((2, 2)), Hd)
    delta = np.linspace(-width, width, S).reshape(S, 1)
    detuning_closed = 0.5 * SZ                                                                 # a Hermitian operator: delta_s Z / 2
    detuning_open = _iso_operator(open_sys.hamiltonian_superoperator(detuning_closed))         # its commutator superoperator, a generator matrix
    a0 = np.zeros((2, T))
    a0[0, :] = np.pi / duration                                                               # the resonant square pi pulse
    ket0, ket1 = np.array([1.0, 0.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0, 0.0])                # [Re psi; Im psi]
    rho0 = np.zeros(8)
    rho0[0] = 1.0                                                                              # |0><0| as [vec(Re rho); vec(Im rho)]
    traj_open = qc.NamedTrajectory({"ρ̃⃗": np.repeat(rho0[:, None], T, axis=1), "a": a0}, controls=("a",), timestep=dt, initial={"ρ̃⃗": rho0})
    traj_closed = qc.NamedTrajectory({"ψ̃": np.repeat(ket0[:, None], T, axis=1), "a": a0}, controls=("a",), timestep=dt, initial={"ψ̃": ket0},
                                     goal={"ψ̃": ket1})
    obj_open = qc.SweepInfidelityObjective(traj_open, open_sys, [detuning_open], delta, state_name="ρ̃⃗", goal_ket=ket1, stored_states=True)
    obj_closed = qc.SweepInfidelityObjective(traj_closed, closed_sys, [detuning_closed], delta, state_name="ψ̃")

    def run(obj, traj):
        z = np.array(traj.datavec, dtype=np.float64)
        a = traj.components["a"]
        idx = np.concatenate([t * traj.dim + np.arange(a.start, a.stop) for t in range(T - 1)])      # the last knot's controls enter no interval

        def fun(v):
            zz = z.copy()
            zz[idx] = v
            J, fids, grad = obj.J_fids_grad(zz)
            return 1.0 - J, -grad[idx]

        res = minimize(fun, z[idx], jac=True, method="L-BFGS-B", bounds=[(-bound, bound)] * idx.size, options={"maxiter": steps})
        return res.x.reshape(T - 1, 2).T, res

    def open_infidelity(controls):
        zz = np.array(traj_open.datavec, dtype=np.float64)
        K = zz[:T * traj_open.dim].reshape(T, traj_open.dim)
        K[:T - 1, traj_open.components["a"]] = controls.T
        return obj_open.L(zz)

    before = open_infidelity(a0[:, :T - 1])
    a_open, res_open = run(obj_open, traj_open)
    a_closed, res_closed = run(obj_closed, traj_closed)
    after, closed = open_infidelity(a_open), open_infidelity(a_closed)
    if verbose:
        print(f"qubit with T1 = {t1}, gamma_phi = {gamma_phi}; pulse of {T - 1} intervals, duration {duration}; {S} detunings in [-{width}, {width}]")
        print(f"polish on the open system: {res_open.nit} L-BFGS iterations, {res_open.nfev} gradient calls ({obj_open._sweep.kernel_name}, stored states)")
        print(f"mean infidelity over the detunings, open system: {before:.4e} -> {after:.4e}")
        print(f"the pulse polished on the closed model ({res_closed.nit} iterations), on the open system: {closed:.4e}")
    obj_open.close()
    obj_closed.close()
    return before, after, closed


if __name__ == "__main__":
    arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
    polish(T=arg(1, 24), S=arg(2, 9), steps=arg(3, 60))
