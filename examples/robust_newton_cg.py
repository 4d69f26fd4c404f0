#!/usr/bin/env python3
"""Polish a solved pulse for robustness with EXACT curvature: the problem of examples/robust_gauss_newton.py -- the solved 1-qubit
Hadamard pulse, the mean squared distance of the final states to the goal over a grid of detunings,

    loss(Z) = sum_s || x_s(Z) - g ||^2 / (2 S),     systems(zeta_s) = QuantumSystem(zeta_s Z, [X, Y]),

-- minimised by truncated-Newton steps.  Every product with the Hessian of the loss is `SweepFinalStateObjective.hessian_times`: one
pushforward (`qc_sweep_jvp_dev`) and one tangent pullback (`qc_sweep_hvp_dev`), whatever the number of systems.  It is the Gauss-Newton
product J^T J / S plus the curvature of the sweep map, sum_s <x_s - g, d2 x_s / dZ2 v> / S, which Gauss-Newton drops.

Conjugate gradients solve (H + lambda I) d = -grad on the controls of knots 1 .. T-2 (the timesteps stay as solved) and leave at
the first direction of non-positive curvature, with what they have by then (Steihaug's exit without a trust region).  The exact Hessian
need not be positive definite away from a minimum: when the FIRST direction already has non-positive curvature the step falls back to
`gauss_newton_times` plus damping, the step of robust_gauss_newton.py.  The step is halved until the loss falls (a forward sweep per
trial); lambda shrinks after a full step and grows after a step that had to be quartered or was refused.  The trajectory vector, the
directions and every product stay on the device; the host sees scalars.

    python examples/robust_newton_cg.py [max_iter] [grid] [steps]
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as g
from robust_gauss_newton import conjugate_gradients
from solve_hadamard import solve


def newton_cg(times, b, max_iter: int, rtol: float = 1e-4):
    """Conjugate gradients on times(x) = b for a symmetric `times` that need not be positive definite, on torch tensors: stops at the first
    direction d with d' times(d) <= 0 and returns what it has.  (x, iterations, negative): `negative` says the exit was taken; x is None
    when it was taken at the first direction."""
    x = torch.zeros_like(b)
    r = b.clone()
    d = r.clone()
    rr = float(r @ r)
    stop = rtol * rtol * rr
    k = 0
    while k < max_iter and rr > stop and rr > 0.0:
        Ad = times(d)
        curv = float(d @ Ad)
        if curv <= 0.0:
            return (None if k == 0 else x), k, True
        alpha = rr / curv
        x += alpha * d
        r -= alpha * Ad
        rr_new = float(r @ r)
        d = r + (rr_new / rr) * d
        rr = rr_new
        k += 1
    return x, k, False


def truncated_newton(obj, Z, idx, steps: int, cg_iter: int = 25, halvings: int = 5, lam: float = 1e-3, verbose: bool = True):
    """The truncated-Newton loop described above on a `SweepFinalStateObjective`: Z the trajectory vector on the device, idx the entries the
    steps may move.  Shared with examples/transmon_newton_cg.py.  Returns the final Z, the loss after every accepted step (the start
    value first), the counts and the `summary` line."""

    def lift(v):
        full = torch.zeros_like(Z)
        full[idx] = v
        return full

    history = [obj.L(Z)]
    accepted, exact, gn, cg_total, fallbacks, trials = 0, 0, 0, 0, 0, 0
    for it in range(steps):
        grad = obj.grad_L(Z)[idx]
        if float(grad.abs().max()) == 0.0:
            break

        def exact_times(v, lam=lam):
            nonlocal exact
            exact += 1
            return obj.hessian_times(Z, lift(v))[idx] + lam * v

        def gn_times(v, lam=lam):
            nonlocal gn
            gn += 1
            return obj.gauss_newton_times(Z, lift(v))[idx] + lam * v

        step, k, negative = newton_cg(exact_times, -grad, cg_iter)
        how = "exact, left at negative curvature" if negative else "exact"
        if step is None:      # non-positive curvature along the gradient itself: the damped Gauss-Newton step
            step, k = conjugate_gradients(gn_times, -grad, cg_iter)
            how, fallbacks = "Gauss-Newton", fallbacks + 1
        cg_total += k
        # CG iterates started at zero are descent directions, the one it left with at negative curvature included: halve the step until
        # the loss falls (a forward sweep each), at most `halvings` times
        full, alpha, ok = lift(step), 1.0, False
        for _ in range(halvings + 1):
            trial = Z + alpha * full
            L_trial = obj.L(trial)
            trials += 1
            ok = L_trial < history[-1]
            if ok:
                break
            alpha *= 0.5
        if ok:
            Z, accepted = trial, accepted + 1
            history.append(L_trial)
            lam = max(lam / 10.0, 1e-12) if alpha == 1.0 else lam * (1.0 if alpha == 0.5 else 10.0)
        else:
            lam *= 10.0
        if verbose:
            print(f"  step {it + 1:2d} ({how}): {k:2d} CG iterations, step length {alpha:.3g}, loss {L_trial:.6e} ({'accepted' if ok else 'refused'}), "
                  f"lambda -> {lam:.1e}")
    summary = (f"truncated Newton: {accepted} accepted steps of {steps}, {exact} exact Hessian products (one pushforward + one tangent pullback each), "
               f"{gn} Gauss-Newton products in {fallbacks} fall-back steps: loss {history[0]:.6e} -> {history[-1]:.6e}")
    return dict(Z=Z, loss_history=history, accepted=accepted, exact_products=exact, gn_products=gn, fallbacks=fallbacks, cg_iterations=cg_total,
                loss_evaluations=trials, summary=summary)


def main(T: int = 50, grid: int = 11, steps: int = 10, verbose: bool = True, max_iter: int = 60, width: float = 0.05, cg_iter: int = 25,
         halvings: int = 5):
    qc = g.load_package()
    f0, f1, viol, z, traj, system = solve(max_iter, T=T, verbose=False, return_solution=True)
    zetas = np.linspace(-width, width, grid)
    dev = torch.device("cuda", 0)
    target = {}
    loss = lambda X: ((X - target["g"]) ** 2).sum() / (2 * X.shape[0])
    obj = qc.SweepFinalStateObjective(traj, system, [qc.GATES["Z"]], zetas[:, None], loss)
    # g: the goal in the global phase the solved pulse reaches it with (robust_gauss_newton.py says why)
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
    res = truncated_newton(obj, Z, idx, steps, cg_iter=cg_iter, halvings=halvings, verbose=verbose)
    out = dict(res, kernel=obj._sweep.kernel_name, T=T, S=grid, controls=res["Z"].cpu().numpy())
    del out["Z"]
    if verbose:
        print(f"rollout fidelity of the solved pulse: {f1:.6f}; {grid} detunings in [-{width}, {width}], T = {T}")
        print(out["summary"])
    obj.close()
    return out


if __name__ == "__main__":
    arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
    main(max_iter=arg(1, 60), grid=arg(2, 11), steps=arg(3, 10))
