#!/usr/bin/env python3
"""The Hadamard problem of examples/al_solve.py (BASELINE config 1: 1-qubit UnitarySmoothPulseProblem, X / Y drives) by the same
augmented-Lagrangian outer loop, with a truncated-Newton inner loop: the step comes from conjugate gradients on

    hess L_rho(Z) v = hess J(Z) v + ((lam + rho F) d2F)(Z) v + rho dF(Z)' (dF(Z) v)

and no value of the dynamics' Jacobian or Hessian ever leaves the library:

    F                        qc_eval_F_jac_dev with no value buffer (residual-only launch)
    dF v, dF' y              qc_eval_jvp_dev, qc_eval_vjp_dev
    ((lam + rho F) d2F) v    qc_eval_hvp_dev -- the Hessian product (three vectors in, one out)
    grad J, hess J           qc_fidelity_eval_dev (infidelity of the final knot) + qc_terms_eval_dev (regularisers): their values
                             once per Newton iteration, their symmetric COO product per CG iteration

Z, lam, F, every gradient and every CG vector are device tensors; torch is the plumbing for the vector updates.  Bounds and pinned
variables (initial state, first and last controls) are handled by projection, as in al_solve.py: CG runs on the variables that are
free at the current point (not pinned, not held at a bound by the gradient), stops at negative curvature, and the step is
backtracked along the projection arc (Armijo on L_rho).  Outer iterations: lam += rho F, rho grows while |F| does not shrink.  Only
scalars cross to the host.  Prints the initial and final rollout fidelity and |F|_inf.

    python examples/newton_cg_solve.py [T] [outer] [inner] [cg]
"""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g


def solve(T: int = 50, outer: int = 8, inner: int = 8, cg: int = 25, rho: float = 10.0, verbose: bool = True):
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
    # the start, the bounds and the pinned variables of al_solve.py
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
    w, tg, y = torch.empty(nv, **f64), torch.empty(nv, **f64), torch.empty(nF, **f64)
    fval, fgrad, tJ = torch.empty(2, **f64), torch.empty(obj.s, **f64), torch.empty(1, **f64)
    # the objectives' Hessian values (upper triangles) and their coordinates
    fH, tH = torch.empty(obj.s * (obj.s + 1) // 2, **f64), torch.empty(max(1, reg.hess_nnz), **f64)
    coords = []
    for r, c in (obj.hess_structure, reg.hess_structure):
        r, c = torch.from_numpy(np.asarray(r, dtype=np.int64)).to(dev), torch.from_numpy(np.asarray(c, dtype=np.int64)).to(dev)
        coords.append((r, c, torch.nonzero(r != c).ravel()))
    first = obj.first                      # the final knot's state: the fidelity's input, in place inside Z
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + 8 * off)      # noqa: E731

    def merit(Zt, rho, grad: bool):
        """L_rho(Zt) as a device scalar, F in `F`; with grad=True its gradient, lam + rho F in `mul` and the objectives' Hessian
        values in `fH`, `tH` as well."""
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        dyn.F_dF_device(Zt, F, None)
        L.check(L.lib.qc_fidelity_eval_dev(obj._f._h, ptr(Zt, first), ptr(fval), ptr(fgrad) if grad else None, ptr(fH) if grad else None, st))
        L.check(L.lib.qc_terms_eval_dev(reg._h, ptr(Zt), ptr(tJ), ptr(tg) if grad else None, ptr(tH) if grad and reg.hess_nnz else None, st))
        val = obj.Q * fval[1] + tJ[0] + torch.dot(lam, F) + 0.5 * rho * torch.dot(F, F)
        if not grad:
            return val, None
        torch.add(lam, F, alpha=rho, out=mul)
        dyn.dFT_times_device(Zt, mul, w)
        gr = w + tg
        gr[first:first + obj.s] -= torch.sign(1.0 - fval[0]) * obj.Q * fgrad
        return val, gr

    def sym_times(out, vals, rc, v):
        """out += (the full symmetric matrix of an upper-triangle COO piece) v"""
        r, c, off = rc
        out.index_add_(0, r, vals * v[c])
        out.index_add_(0, c[off], vals[off] * v[r[off]])

    def hess_times(Zt, rho, v):
        """hess L_rho(Zt) v at the point of the last merit(Zt, rho, True): four launches of the library and the objectives' pieces"""
        hv = torch.empty(nv, **f64)
        dyn.mu_d2F_times_device(Zt, mul, v, hv)            # ((lam + rho F) d2F) v
        dyn.dF_times_device(Zt, v, y)
        dyn.dFT_times_device(Zt, y, w)                     # dF' (dF v)
        hv.add_(w, alpha=rho)
        sym_times(hv, -torch.sign(1.0 - fval[0]) * obj.Q * fH, coords[0], v)
        if reg.hess_nnz:
            sym_times(hv, tH[:reg.hess_nnz], coords[1], v)
        return hv

    def newton_step(Zt, rho, gr):
        """Truncated CG on the free variables; the steepest-descent direction where the first CG direction has negative curvature."""
        free = ((lo < hi) & ~((Zt <= lo) & (gr > 0)) & ~((Zt >= hi) & (gr < 0))).to(torch.float64)
        r = -gr * free
        p, d, rr = torch.zeros_like(r), r.clone(), float(torch.dot(r, r))
        tol2 = min(0.25, rr ** 0.5) * rr
        n_hv = 0
        for _ in range(cg):
            if rr <= tol2 or rr == 0.0:
                break
            hd = hess_times(Zt, rho, d) * free
            n_hv += 1
            curv = float(torch.dot(d, hd))
            if curv <= 1e-12 * float(torch.dot(d, d)):
                if n_hv == 1:
                    p = d.clone()
                break
            alpha = rr / curv
            p.add_(d, alpha=alpha)
            r.sub_(hd, alpha=alpha)
            rr_new = float(torch.dot(r, r))
            d = r + (rr_new / rr) * d
            rr = rr_new
        return p, n_hv

    def rollout_fidelity(z):
        states = dyn.rollout(z, qc.operator_to_iso_vec(np.eye(2, dtype=complex)))
        return qc.iso_vec_unitary_fidelity(states[:, -1], qc.operator_to_iso_vec(U_goal))

    f_before = rollout_fidelity(z0)
    merit(Z, rho, False)
    viol_before = viol = float(F.abs().max())
    n_newton = n_products = 0
    for k in range(outer):
        for _ in range(inner):
            val, gr = merit(Z, rho, True)
            p, n_hv = newton_step(Z, rho, gr)
            n_newton += 1
            n_products += n_hv
            step, moved = 1.0, False
            for _ in range(30):                                        # Armijo backtracking along the projection arc
                Zn = torch.minimum(torch.maximum(Z + step * p, lo), hi)
                d = Zn - Z
                vn, _ = merit(Zn, rho, False)
                if float(vn) <= float(val) + 1e-4 * float(torch.dot(gr, d)):
                    moved = True
                    break
                step *= 0.5
            if not moved or float(d.abs().max()) < 1e-12:
                break
            Z = Zn
        merit(Z, rho, False)
        new_viol = float(F.abs().max())
        lam.add_(F, alpha=rho)
        if new_viol > 0.5 * viol:
            rho *= 4.0
        viol = new_viol
        if verbose:
            print(f"outer {k + 1:2d}: |F|_inf {viol:.3e}  rho {rho:g}  infidelity {float(fval[1]):.3e}")
    z = Z.cpu().numpy()
    f_after = rollout_fidelity(z)
    if verbose:
        print(f"{n_newton} Newton iterations, {n_products} Hessian products  rollout fidelity {f_before:.6f} -> {f_after:.6f}  "
              f"|F|_inf {viol_before:.3e} -> {viol:.3e}  Hessian products on {dyn.hess_product_kernel_name}")
    for o in (dyn, obj, reg):
        o.close()
    return f_before, f_after, viol_before, viol


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:5]]
    solve(*a)
