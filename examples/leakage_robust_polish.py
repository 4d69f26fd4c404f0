#!/usr/bin/env python3
"""Polish a pulse against leakage AND detuning at once, with a loss written in torch on the final states of a rollout sweep.

A three-level transmon (anharmonicity -200 MHz, drives on both quadratures) starts from a square pi pulse of 10 ns: fast enough to leak
into the third level.  Over a grid of detunings zeta (perturbation zeta a'a) the loss is

    mean_s (1 - |tr(G' U_s[sub, sub])| / 2)  +  weight x mean_s  sum |U_s[out, in]|^2 / 2,

the subspace infidelity of an X gate plus the population that the two computational columns leave outside the subspace.  Neither the
leakage term nor their sum is a fidelity the sweep handle knows: the final states come from `RolloutSweep.finals_autograd` as a
differentiable S x (2N cols) tensor, the loss is ordinary torch on top, and every backward pass is ONE adjoint sweep
(`qc_sweep_vjp_dev`), whatever the number of detunings.  torch's L-BFGS (strong Wolfe line search) moves the controls; the landscape
and the leakage are printed before and after.  `--wide`: two coupled transmons of three levels each (2N = 18, "mfma32-sweep"), an X gate
on the first, leakage out of the four computational levels.

    python examples/leakage_robust_polish.py [--wide] [steps] [grid] [T]
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g

ANHARM = -2 * np.pi * 0.2          # rad / ns
COUPLING = 2 * np.pi * 0.005
DURATION = 10.0                    # ns


def transmons(wide: bool):
    """(H_drift, H_drives, detuning operator, computational levels, goal on those levels)."""
    a = np.diag(np.sqrt(np.arange(1, 3)), 1).astype(complex)
    n = a.conj().T @ a
    kerr = 0.5 * ANHARM * (n @ n - n)
    X = np.array([[0, 1], [1, 0]], dtype=complex)
    if not wide:
        return kerr, [(a + a.conj().T) / 2, 1j * (a.conj().T - a) / 2], n, [0, 1], X
    I = np.eye(3)
    a1, a2 = np.kron(a, I), np.kron(I, a)
    H0 = np.kron(kerr, I) + np.kron(I, kerr) + COUPLING * (a1.conj().T @ a2 + a2.conj().T @ a1)
    return H0, [(a1 + a1.conj().T) / 2, 1j * (a1.conj().T - a1) / 2], np.kron(n, I), [0, 1, 3, 4], np.kron(X, np.eye(2))


def main(T: int = 40, grid: int = 9, steps: int = 10, weight: float = 2.0, width: float = 2 * np.pi * 0.005, wide: bool = False,
         verbose: bool = True, device: int = 0):
    qc = g.load_package()
    H0, Hd, P, sub, goal = transmons(wide)
    system = qc.QuantumSystem(H0, Hd)
    N, m, n_sub = system.levels, len(Hd), len(sub)
    out = [k for k in range(N) if k not in sub]
    dt = DURATION / (T - 1)
    zetas = np.linspace(-width, width, grid)
    sw = qc.RolloutSweep(system, [P], T, dt_fixed=dt, device=device, wide=wide)
    if not sw.vjp_supported:
        raise RuntimeError(sw.vjp_unsupported_reason)
    dev = torch.device("cuda", device)
    put = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    controls = np.zeros((m, T))
    controls[0] = np.pi / DURATION                                    # a square pi pulse on the first quadrature
    dZ = put(sw.pack(controls)).requires_grad_(True)
    dinit, dtheta = put(qc.operator_to_iso_vec(np.eye(N, dtype=complex))), put(zetas[:, None])
    G = put(goal)

    def terms(Z):
        """(infidelity, leakage) of every detuning, S values each."""
        V = sw.finals_autograd(Z, dinit, dtheta).reshape(grid, N, 2 * N)      # [s, column, row]: Re rows, then Im rows
        U = torch.complex(V[:, :, :N], V[:, :, N:]).transpose(1, 2)           # [s, row, column]
        tr = (G.conj() * U[:, sub][:, :, sub]).sum(dim=(1, 2))
        return 1.0 - tr.abs() / n_sub, (U[:, out][:, :, sub].abs() ** 2).sum(dim=(1, 2)) / n_sub

    def loss(Z):
        infid, leak = terms(Z)
        return infid.mean() + weight * leak.mean()

    with torch.no_grad():
        infid0, leak0 = (t.cpu().numpy() for t in terms(dZ))
        loss0 = float(loss(dZ))
    opt = torch.optim.LBFGS([dZ], max_iter=steps, line_search_fn="strong_wolfe")
    calls = [0]

    def closure():
        opt.zero_grad()
        L = loss(dZ)
        L.backward()
        calls[0] += 1
        return L

    opt.step(closure)
    with torch.no_grad():
        infid1, leak1 = (t.cpu().numpy() for t in terms(dZ))
        loss1 = float(loss(dZ))
    kernel = sw.kernel_name
    if verbose:
        print(f"{kernel}: {N} levels, T = {T}, {grid} detunings; {steps} L-BFGS iterations, {calls[0]} adjoint sweeps")
        print("   zeta/2pi [MHz]   infidelity before -> after       leakage before -> after")
        for z, a0, a1, b0, b1 in zip(zetas, infid0, infid1, leak0, leak1):
            print(f"     {1e3 * z / (2 * np.pi):+7.2f}         {a0:.3e} -> {a1:.3e}        {b0:.3e} -> {b1:.3e}")
        print(f"loss {loss0:.4e} -> {loss1:.4e};  mean leakage {leak0.mean():.3e} -> {leak1.mean():.3e}")
    sw.close()
    return dict(kernel=kernel, loss_before=loss0, loss_after=loss1, leakage_before=float(leak0.mean()), leakage_after=float(leak1.mean()),
                infidelity_before=infid0, infidelity_after=infid1, controls=dZ.detach().cpu().numpy())


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--wide"]
    arg = lambda i, d: int(args[i]) if len(args) > i else d
    main(steps=arg(0, 10), grid=arg(1, 9), T=arg(2, 40), wide="--wide" in sys.argv[1:])
