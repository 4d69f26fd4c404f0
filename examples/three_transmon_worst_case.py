#!/usr/bin/env python3
"""Worst-case search for a three-transmon pulse, on the matrix cores: the system of three_transmon_polish.py (three coupled three-level
transmons, 27 levels, 2N = 54), its smooth start pulse, the eight computational columns |q1 q2 q3> of the propagator as the state, and
the search of examples/transmon_worst_case.py over the box

    zeta_k in [-width, width], k = 1, 2, 3  (detuning zeta_k b_k^dag b_k of each transmon),     c in [1 - amp, 1 + amp]  (one factor on all six drives)

for the system on which the pulse does worst.  The starts are the box's sixteen corners and uniform draws; from every one of them a
projected-gradient ascent of the subspace infidelity 1 - |tr(G^dag U_s[sub, sub])|^2 / 64 runs, all at once.  Every iteration is one
forward sweep (the final states, on which the loss and its cotangent are written in numpy) and ONE pullback with parameter cotangents,
`RolloutSweep.vjp(..., params=True)`, on a handle made with `wide=True, wide64=True, wide64_grad=True, wide64_params=True` (kernel
"mfma64-sweep"): d(1 - F_s)/dzeta_{s,k} and d(1 - F_s)/dc_{s,j} of every start from one backward walk (the derivative with respect to
the common factor is the sum over the six drives).  Without `wide64_params` a system of this size has no parameter derivative and the
same numbers cost 2 (3 + 6) forward sweeps by central differences.  Printed: the starts' worst infidelity and the worst found.

    python examples/three_transmon_worst_case.py [T] [starts] [iters]          (small sizes, e.g. 6 16 2, run in seconds)
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as g
from three_transmon_robustness import LEVELS, SUBSPACE, goal_gate, three_transmons
from worst_case_search import ascend, box_starts


def number_operators():
    """b_k^dag b_k of each transmon, 27 x 27 (|q1 q2 q3> has index 9 q1 + 3 q2 + q3: the first transmon is the leftmost factor)."""
    n, one = np.diag(np.arange(LEVELS, dtype=complex)), np.eye(LEVELS, dtype=complex)
    return [np.kron(np.kron(n, one), one), np.kron(np.kron(one, n), one), np.kron(np.kron(one, one), n)]


def infidelity_and_cotangent(X, Gsub):
    """1 - |tr(G^dag U_s[sub, sub])|^2 / 64 of every sample and its derivative with respect to the final states, both for X[sample, column,
    row] with rows [Re; Im]: with t = tr(G^dag U), d value = -(2 / 64) Re(conj(t) sum conj(G_ab) dU_ab), so the real rows receive
    Re(-(2 / 64) t G_ab) and the imaginary rows its imaginary part."""
    N, cols = X.shape[2] // 2, X.shape[1]
    U = (X[:, :, :N] + 1j * X[:, :, N:])[:, :, SUBSPACE].transpose(0, 2, 1)            # [sample, sub row, column]
    tr = np.einsum("ab,sab->s", Gsub.conj(), U)
    W = (-2.0 / cols ** 2 * tr[:, None, None] * Gsub[None]).transpose(0, 2, 1)         # [sample, column, sub row]
    cot = np.zeros_like(X)
    cot[:, :, SUBSPACE] = W.real
    cot[:, :, [N + i for i in SUBSPACE]] = W.imag
    return 1.0 - np.abs(tr) ** 2 / cols ** 2, cot


def main(T: int = 40, starts: int = 64, iters: int = 10, width: float = 2 * np.pi * 0.002, amp: float = 0.05, duration: float = 40.0,
         verbose: bool = True, seed: int = 0):
    """Returns a dictionary: `start_worst`, the largest infidelity among the starts; `found_worst`, the largest the ascents reached;
    `history`, the S infidelities after every iteration; `kernel`; `x`, the S points reached (zeta_1, zeta_2, zeta_3, c)."""
    qc = g.load_package()
    H0, drives, n1 = three_transmons()
    perts = number_operators()
    assert np.allclose(perts[0], n1)          # b^dag b of that file, there to rounding ((sqrt 2)^2)
    system = qc.QuantumSystem(H0, drives)
    N, m, p, cols = LEVELS ** 3, len(drives), len(perts), len(SUBSPACE)
    dts = np.full(T, duration / (T - 1))
    # the start pulse of three_transmon_polish.run: half a Rabi turn on the first transmon's x drive, a little of everything else
    rng = np.random.default_rng(0)
    window = np.sin(np.pi * np.linspace(0.0, 1.0, T)) ** 2
    a = 0.1 * (np.pi / 2) / (duration * 0.5) * rng.uniform(-1, 1, (m, 1)) * window
    a[0] += (np.pi / 2) / (duration * 0.5) * window
    # the state: the computational columns of the identity, [Re; Im] per column
    E = np.zeros((2 * N, cols))
    E[SUBSPACE, np.arange(cols)] = 1.0
    init = E.reshape(-1, order="F")
    Gsub = goal_gate()[np.ix_(SUBSPACE, SUBSPACE)]
    lo, hi = np.array([-width] * p + [1.0 - amp]), np.array([width] * p + [1.0 + amp])
    x0 = box_starts(starts, lo, hi, np.random.default_rng(seed))
    S = x0.shape[0]

    sw = qc.RolloutSweep(system, perts, T, cols=cols, wide=True, wide64=True, wide64_grad=True, wide64_params=True)
    try:
        kernel = sw.kernel_name
        Z = sw.pack(a, dts)

        def evaluate(x):
            theta, scale = np.ascontiguousarray(x[:, :p]), np.repeat(x[:, p:], m, axis=1)
            X = sw.eval(Z, init, theta, scale, fids=False)[0].T.reshape(S, cols, 2 * N)          # [sample, column, row]
            value, cot = infidelity_and_cotangent(X, Gsub)
            _, gth, gsc = sw.vjp(Z, init, cot.reshape(S, -1), theta, scale, params=True)
            return value, np.concatenate([gth, gsc.sum(axis=1, keepdims=True)], axis=1)

        x, val, history = ascend(evaluate, x0, lo, hi, iters)
    finally:
        sw.close()
    k, b = int(np.argmax(history[0])), int(np.argmax(val))
    start_worst, found_worst = float(history[0][k]), float(val[b])
    if verbose:
        mhz = lambda z: ", ".join(f"{1e3 * v / (2 * np.pi):+.3f}" for v in z)
        print(f"three three-level transmons (27 levels, 2N = 54), {T} knots, {cols} state columns, kernel {kernel}; {S} starts, {iters} iterations "
              f"({iters + 1} sweeps and pullbacks)")
        print(f"starts:  worst infidelity {start_worst:.9f} at zeta / 2 pi = ({mhz(x0[k, :p])}) MHz, c = {x0[k, p]:.4f}")
        print(f"ascents: worst infidelity {found_worst:.9f} at zeta / 2 pi = ({mhz(x[b, :p])}) MHz, c = {x[b, p]:.4f}")
        print(f"worst infidelity: starts {start_worst:.12e} found {found_worst:.12e}")
    return dict(start_worst=start_worst, found_worst=found_worst, history=history, kernel=kernel, x=x, starts=S)


if __name__ == "__main__":
    arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
    main(T=arg(1, 40), starts=arg(2, 64), iters=arg(3, 10))
