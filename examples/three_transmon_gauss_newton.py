#!/usr/bin/env python3
"""Polish a three-transmon pulse against a frequency error with CURVATURE, on the matrix cores: examples/transmon_gauss_newton.py at the
size of examples/three_transmon_robustness.py (three coupled three-level transmons, 27 levels, 2N = 54, "mfma64-sweep"), an X gate on the
first transmon, a grid of detunings zeta_s of the first transmon.  The loss is that example's least-squares function of the final states,

    loss(Z) = sum_s sum_{c in comp} ( || P (U_s e_c - g_c) ||^2 + weight || (1 - P) U_s e_c ||^2 ) / (2 S),

over the eight computational columns (P projects on the computational subspace; g: the goal in the global phase the start pulse reaches
it with).  The loss is a `SweepFinalStateObjective(..., wide=True, wide64=True, wide64_grad=True, wide64_tangent=True)`: its gradient is
one adjoint sweep on 4 x 4 tiles, and every product with the Gauss-Newton matrix is `gauss_newton_times`, one pushforward
(`qc_sweep_jvp_dev`, QC_SWEEP_WIDE_64_TANGENT) and one pullback (`qc_sweep_vjp_dev`, QC_SWEEP_WIDE_64_GRAD), whatever the number of
detunings.  Damped Gauss-Newton steps with conjugate gradients on the controls of knots 1 .. T-2, as examples/robust_gauss_newton.py:
the trajectory vector, the direction and every product stay on the device.  The default size is small, so that it finishes in seconds.

    python examples/three_transmon_gauss_newton.py [T] [grid] [steps]
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
from three_transmon_robustness import LEVELS, SUBSPACE, goal_gate, three_transmons


def problem(T: int, grid: int, weight: float, width: float, duration: float):
    """The three-transmon problem described above.  Returns (obj, Z, idx, leakage, dt): the objective, the start trajectory vector on the
    device, the entries the steps may move (the controls of knots 1 .. T-2) and the mean leakage of a trajectory vector."""
    qc = g.load_package()
    H0, drives, n1 = three_transmons()
    system = qc.QuantumSystem(H0, drives)
    N, m = LEVELS ** 3, len(drives)
    dt = duration / (T - 1)
    # the start of three_transmon_polish.py: half a Rabi turn on the first transmon's x drive, a little of everything else
    rng = np.random.default_rng(0)
    window = np.sin(np.pi * np.linspace(0.0, 1.0, T)) ** 2
    a = 0.1 * (np.pi / 2) / (duration * 0.5) * rng.uniform(-1, 1, (m, 1)) * window
    a[0] += (np.pi / 2) / (duration * 0.5) * window
    init = np.asarray(qc.operator_to_iso_vec(np.eye(N, dtype=complex)), dtype=np.float64)
    traj = qc.NamedTrajectory({"Ũ⃗": np.repeat(init[:, None], T, axis=1), "a": a, "Δt": np.full((1, T), dt)}, controls=("a",), timestep="Δt",
                              initial={"Ũ⃗": init}, goal={"Ũ⃗": np.asarray(qc.operator_to_iso_vec(goal_gate()), dtype=np.float64)})
    zetas = np.linspace(-width, width, grid)
    dev = torch.device("cuda", 0)
    sub = torch.tensor(SUBSPACE, device=dev)
    rows_in = torch.cat([sub, sub + N])
    rows_out = torch.tensor([r + o for o in (0, N) for r in range(N) if r not in SUBSPACE], device=dev)
    target = {}

    def terms(X):
        """(distance, leakage) summed over the samples and the computational columns."""
        V = X.reshape(X.shape[0], N, 2 * N)[:, sub]                          # [s, computational column, row]: Re rows, then Im rows
        return ((V[:, :, rows_in] - target["g"]) ** 2).sum(), (V[:, :, rows_out] ** 2).sum()

    def loss(X):
        dist, leak = terms(X)
        return (dist + weight * leak) / (2 * X.shape[0])

    obj = qc.SweepFinalStateObjective(traj, system, [n1], zetas[:, None], loss, wide=True, wide64=True, wide64_grad=True, wide64_tangent=True)
    z = np.array(traj.datavec, dtype=np.float64)
    # g: the goal's computational block in the global phase the start pulse reaches it with (robust_gauss_newton.py says why)
    G = goal_gate()[np.ix_(SUBSPACE, SUBSPACE)]
    V0 = obj.finals(z).reshape(grid, N, 2 * N)                               # [s, column, row]
    U0 = (V0[:, :, :N] + 1j * V0[:, :, N:]).transpose(0, 2, 1)[:, SUBSPACE][:, :, SUBSPACE]
    Gp = np.exp(1j * np.angle((G.conj()[None] * U0).sum())) * G
    target["g"] = torch.from_numpy(np.ascontiguousarray(np.concatenate([Gp.real.T, Gp.imag.T], axis=1))).to(dev)      # [column, (Re rows, Im rows)]
    rows = traj.components["a"]
    idx = torch.from_numpy(np.concatenate([t * traj.dim + np.arange(rows.start, rows.stop) for t in range(1, T - 1)])).to(dev)
    Z = torch.from_numpy(z).to(dev)

    def leakage(Zv):
        with torch.no_grad():
            X = torch.from_numpy(np.ascontiguousarray(obj.finals(Zv.cpu().numpy()))).to(dev)
            return float(terms(X)[1]) / (grid * len(SUBSPACE))

    return obj, Z, idx, leakage, dt


def main(T: int = 10, grid: int = 3, steps: int = 3, weight: float = 1.0, width: float = 2 * np.pi * 0.002, duration: float = 40.0,
         cg_iter: int = 8, damping: float = 1.0, verbose: bool = True):
    """Returns the loss after every accepted step (`loss_history`, the start value first), the counts, the mean leakage before and
    after, and the kernel that served the sweeps."""
    obj, Z, idx, leakage, dt = problem(T, grid, weight, width, duration)

    def lift(v):
        full = torch.zeros_like(Z)
        full[idx] = v
        return full

    leak_before = leakage(Z)
    history = [obj.L(Z)]
    lam, accepted, products, cg_total = damping, 0, 0, 0      # the start pulse is far from the goal: a small lambda oversteps
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
    leak_after = leakage(Z)
    kernel = obj._sweep.kernel_name
    if verbose:
        print(f"three three-level transmons (27 levels, 2N = 54), {T} knots of {dt:.2f} ns, {grid} detunings in [-{width:.4f}, {width:.4f}] rad / ns, kernel {kernel}")
        print(f"damped Gauss-Newton: {accepted} accepted steps of {steps}, {products} Gauss-Newton products (one pushforward + one pullback each)")
        print(f"loss before {history[0]:.6e}, loss after {history[-1]:.6e};  mean leakage {leak_before:.3e} -> {leak_after:.3e}")
    obj.close()
    return dict(loss_history=history, accepted=accepted, gn_products=products, cg_iterations=cg_total, kernel=kernel, leakage_before=leak_before,
                leakage_after=leak_after, controls=Z.cpu().numpy())


if __name__ == "__main__":
    arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
    main(T=arg(1, 10), grid=arg(2, 3), steps=arg(3, 3))
