#!/usr/bin/env python3
"""Polish a solved pulse for robustness with CURVATURE: take the solved 1-qubit Hadamard pulse of examples/robust_polish.py and
minimise the mean squared distance of the final states to the goal over a grid of detunings,

    loss(Z) = sum_s || x_s(Z) - g ||^2 / (2 S),     systems(zeta_s) = QuantumSystem(zeta_s Z, [X, Y]),

(g: the iso-vector of the Hadamard gate in the global phase the solved pulse reaches it with) by damped Gauss-Newton steps.  The
loss is a `SweepFinalStateObjective`; its gradient is one adjoint sweep, and every product with the
Gauss-Newton matrix J^T J / S is `gauss_newton_times`: one pushforward (`qc_sweep_jvp_dev`) and one pullback (`qc_sweep_vjp_dev`),
whatever the number of systems.  Conjugate gradients solve (J^T J / S + lambda I) d = -grad on the controls of knots 1 .. T-2
(the timesteps stay as solved), a step is accepted when the loss falls, lambda shrinks after an accepted step and grows after a
refused one.  The trajectory vector, the direction and every product stay on the device; the host sees scalars.  With `verbose`
(only then) the iteration count is printed beside that of L-BFGS, the optimiser of robust_polish.py: the count is not taken from
that script, whose loss is the mean infidelity -- scipy's L-BFGS-B is re-run here, on the host, on THIS loss, from the same solved
pulse, on the same grid and the same free controls, so that the two counts belong to one problem.

    python examples/robust_gauss_newton.py [max_iter] [grid] [steps]
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as g
from solve_hadamard import solve


def conjugate_gradients(times, b, max_iter: int, rtol: float = 1e-4):
    """x with times(x) ~ b for a symmetric positive definite `times`, on torch tensors; (x, iterations)."""
    x = torch.zeros_like(b)
    r = b.clone()
    d = r.clone()
    rr = float(r @ r)
    stop = rtol * rtol * rr
    k = 0
    while k < max_iter and rr > stop and rr > 0.0:
        Ad = times(d)
        alpha = rr / float(d @ Ad)
        x += alpha * d
        r -= alpha * Ad
        rr_new = float(r @ r)
        d = r + (rr_new / rr) * d
        rr = rr_new
        k += 1
    return x, k


def main(T: int = 50, grid: int = 11, steps: int = 10, verbose: bool = True, max_iter: int = 60, width: float = 0.05, cg_iter: int = 25):
    qc = g.load_package()
    f0, f1, viol, z, traj, system = solve(max_iter, T=T, verbose=False, return_solution=True)
    zetas = np.linspace(-width, width, grid)
    dev = torch.device("cuda", 0)
    target = {}
    loss = lambda X: ((X - target["g"]) ** 2).sum() / (2 * X.shape[0])
    obj = qc.SweepFinalStateObjective(traj, system, [qc.GATES["Z"]], zetas[:, None], loss)
    # g: the goal in the global phase the solved pulse reaches it with.  Traceless drives keep det U = 1 while det H = -1, so the pulse
    # ends at +-i H, where Re tr(H' U) = 0 and the distance to H itself is stationary in every control: nothing to descend along.
    N = system.levels
    G = qc.GATES["H"]
    V = obj.finals(z).reshape(grid, N, 2 * N)                                # [s, column, row]: Re rows, then Im rows
    U = (V[:, :, :N] + 1j * V[:, :, N:]).transpose(0, 2, 1)
    phase = np.exp(1j * np.angle((G.conj()[None] * U).sum()))
    target["g"] = torch.from_numpy(np.ascontiguousarray(qc.operator_to_iso_vec(phase * G), dtype=np.float64)).to(dev)
    zdim, a = traj.dim, traj.components["a"]
    idx_host = np.concatenate([t * zdim + np.arange(a.start, a.stop) for t in range(1, T - 1)])      # the first and last controls stay pinned
    idx = torch.from_numpy(idx_host).to(dev)
    Z = torch.from_numpy(np.array(z, dtype=np.float64)).to(dev)

    def lift(v):
        full = torch.zeros_like(Z)
        full[idx] = v
        return full

    history = [obj.L(Z)]
    lam, accepted, products, cg_total = 1e-3, 0, 0, 0
    for it in range(steps):
        grad = obj.grad_L(Z)[idx]
        if float(grad.abs().max()) == 0.0:
            break

        def times(v, lam=lam):
            nonlocal products
            products += 1
            return obj.gauss_newton_times(Z, lift(v))[idx] + lam * v

        step, k = conjugate_gradients(times, -grad, cg_iter)
        cg_total += k
        trial = Z + lift(step)
        L_trial = obj.L(trial)
        ok = L_trial < history[-1]
        if ok:
            Z, lam, accepted = trial, max(lam / 10.0, 1e-12), accepted + 1
            history.append(L_trial)
        else:
            lam *= 10.0
        if verbose:
            print(f"  step {it + 1:2d}: {k:2d} CG iterations, loss {L_trial:.6e} ({'accepted' if ok else 'refused'}), lambda -> {lam:.1e}")
    out = dict(loss_history=history, accepted=accepted, gn_products=products, cg_iterations=cg_total, kernel=obj._sweep.kernel_name,
               controls=Z.cpu().numpy())
    if verbose:
        from scipy.optimize import minimize
        z0 = np.array(z, dtype=np.float64)

        def fun(v):
            zz = z0.copy()
            zz[idx_host] = v
            return obj.L(zz), obj.grad_L(zz)[idx_host]

        res = minimize(fun, z0[idx_host], jac=True, method="L-BFGS-B", options={"maxiter": 200})
        out["lbfgs_iterations"], out["lbfgs_loss"] = int(res.nit), float(res.fun)
        print(f"rollout fidelity of the solved pulse: {f1:.6f}; {grid} detunings in [-{width}, {width}], T = {T}")
        print(f"damped Gauss-Newton: {accepted} accepted steps of {steps}, {products} Gauss-Newton products (one pushforward + one pullback each): "
              f"loss {history[0]:.6e} -> {history[-1]:.6e}")
        print(f"L-BFGS on the same loss: {res.nit} iterations, {res.nfev} gradient calls: loss {history[0]:.6e} -> {res.fun:.6e}")
    obj.close()
    return out


if __name__ == "__main__":
    arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
    main(max_iter=arg(1, 60), grid=arg(2, 11), steps=arg(3, 10))
