#!/usr/bin/env python3
"""The Hadamard problem of examples/solve_hadamard.py (BASELINE config 1: 1-qubit UnitarySmoothPulseProblem, X / Y drives) solved
by an augmented-Lagrangian loop that never leaves the GPU and never takes the values of the dynamics Jacobian:

    L_rho(Z) = J(Z) + lam' F(Z) + rho/2 |F(Z)|^2,        grad L_rho = grad J + dF(Z)' (lam + rho F(Z))

    F                    qc_eval_F_jac_dev with no value buffer (residual-only launch)
    dF' (lam + rho F)    qc_eval_vjp_dev -- the transposed product (two vectors in and out; the values stay in the handle's scratch)
    grad J               qc_fidelity_eval_dev (infidelity of the final knot) + qc_terms_eval_dev (regularisers)

Z, lam, F and every gradient are device tensors; torch is the plumbing for the vector updates.  Inner iterations: projected
gradient steps with Barzilai-Borwein step lengths and Armijo backtracking on L_rho; bounds and pinned variables (initial state,
first and last controls) are handled by projection.  Outer iterations: lam += rho F, rho grows while |F| does not shrink.
Only scalars (merit values, norms) cross to the host.  Prints the initial and final rollout fidelity and |F|_inf.

    python examples/al_solve.py [T] [outer] [inner]
"""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g


def solve(T: int = 50, outer: int = 10, inner: int = 40, rho: float = 10.0, verbose: bool = True):
    qc = g.load_package()
    L = qc._lib
    inp = qc.config_inputs(1, T=T)
    traj = inp.traj
    U_goal = qc.GATES["H"]
    dyn = qc.QuantumDynamics(inp.integrators, traj)
    obj = qc.UnitaryInfidelityObjective("Ũ⃗", traj, Q=100.0)
    R = 1e-2
    reg = qc.TrajectoryObjective(qc.QuadraticRegularizer("a", traj, R) + qc.QuadraticRegularizer("da", traj, R)
                                 + qc.QuadraticRegularizer("dda", traj, R), traj)
    nv, nF, zdim, comps = int(dyn.dims.Z_len), int(dyn.dims.F_len), traj.dim, traj.components
    # the start of solve_hadamard.py: the template's guess with milder controls; bounds |a|, |dda| <= 1, dt in [0.1, 0.3];
    # pinned variables have lb = ub
    z0 = traj.datavec.copy()
    for t in range(T):
        for nm in ("a", "da", "dda"):
            if nm != "a" or 0 < t < T - 1:
                z0[t * zdim + comps[nm].start:t * zdim + comps[nm].stop] *= 0.2
    lb, ub = np.full(nv, -np.inf), np.full(nv, np.inf)
    for t in range(T):
        for nm in ("a", "dda"):
            sl = slice(t * zdim + comps[nm].start, t * zdim + comps[nm].stop)
            lb[sl], ub[sl] = -1.0, 1.0
        lb[t * zdim + comps["Δt"].start], ub[t * zdim + comps["Δt"].start] = 0.1, 0.3
    pin = [slice(comps["Ũ⃗"].start, comps["Ũ⃗"].stop)] + [slice(t * zdim + comps["a"].start, t * zdim + comps["a"].stop) for t in (0, T - 1)]
    for sl in pin:
        lb[sl] = ub[sl] = z0[sl]

    dev = torch.device("cuda", dyn.device)
    f64 = dict(dtype=torch.float64, device=dev)
    Z, lo, hi = (torch.from_numpy(x).to(dev) for x in (z0, lb, ub))
    lam, F, mul = torch.zeros(nF, **f64), torch.empty(nF, **f64), torch.empty(nF, **f64)
    w, tg = torch.empty(nv, **f64), torch.empty(nv, **f64)
    fval, fgrad, tJ = torch.empty(2, **f64), torch.empty(obj.s, **f64), torch.empty(1, **f64)
    first = obj.first                      # the final knot's state: the fidelity's input, in place inside Z
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + 8 * off)      # noqa: E731

    def merit(Zt, rho, grad: bool):
        """L_rho(Zt) as a device scalar, F in `F`; with grad=True its gradient as well -- three launches and the product."""
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        dyn.F_dF_device(Zt, F, None)
        L.check(L.lib.qc_fidelity_eval_dev(obj._f._h, ptr(Zt, first), ptr(fval), ptr(fgrad) if grad else None, None, st))
        L.check(L.lib.qc_terms_eval_dev(reg._h, ptr(Zt), ptr(tJ), ptr(tg) if grad else None, None, st))
        val = obj.Q * fval[1] + tJ[0] + torch.dot(lam, F) + 0.5 * rho * torch.dot(F, F)
        if not grad:
            return val, None
        torch.add(lam, F, alpha=rho, out=mul)
        dyn.dFT_times_device(Zt, mul, w)      # dF' (lam + rho F): two vectors cross the interface, no Jacobian value
        gr = w + tg
        gr[first:first + obj.s] -= torch.sign(1.0 - fval[0]) * obj.Q * fgrad
        return val, gr

    def rollout_fidelity(z):
        states = dyn.rollout(z, qc.operator_to_iso_vec(np.eye(2, dtype=complex)))
        return qc.iso_vec_unitary_fidelity(states[:, -1], qc.operator_to_iso_vec(U_goal))

    f_before = rollout_fidelity(z0)
    merit(Z, rho, False)
    viol_before = viol = float(F.abs().max())
    n_grad = 0
    for k in range(outer):
        val, gr = merit(Z, rho, True)
        step = 1.0 / max(1.0, float(gr.abs().max()))
        for _ in range(inner):
            n_grad += 1
            for _ in range(30):                                        # Armijo backtracking along the projection arc
                Zn = torch.minimum(torch.maximum(Z - step * gr, lo), hi)
                d = Zn - Z
                vn, _ = merit(Zn, rho, False)
                if float(vn) <= float(val) + 1e-4 * float(torch.dot(gr, d)):
                    break
                step *= 0.5
            vn, gn = merit(Zn, rho, True)
            dg = gn - gr
            sy = float(torch.dot(d, dg))
            step = min(1e3, max(1e-8, float(torch.dot(d, d)) / sy)) if sy > 0 else min(1e3, 2.0 * step)      # Barzilai-Borwein
            Z, val, gr = Zn, vn, gn
            if float(d.abs().max()) < 1e-12:
                break
        merit(Z, rho, False)
        new_viol = float(F.abs().max())
        lam.add_(F, alpha=rho)
        if new_viol > 0.5 * viol:
            rho *= 4.0
        viol = new_viol
        if verbose:
            print(f"outer {k + 1:2d}: L_rho {float(val):.6f}  |F|_inf {viol:.3e}  rho {rho:g}  infidelity {float(fval[1]):.3e}")
    z = Z.cpu().numpy()
    f_after = rollout_fidelity(z)
    if verbose:
        print(f"{n_grad} gradient evaluations  rollout fidelity {f_before:.6f} -> {f_after:.6f}  |F|_inf {viol_before:.3e} -> {viol:.3e}  "
              f"products on {dyn.product_kernel_names[1]}")
    for o in (dyn, obj, reg):
        o.close()
    return f_before, f_after, viol_before, viol


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:4]]
    solve(*a)
