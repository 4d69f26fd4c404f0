#!/usr/bin/env python3
"""Robustness of a three-transmon pulse against a frequency error, on the matrix cores: three coupled three-level transmons in a chain
(27 levels, 2N = 54), a short pulse, the subspace fidelity on the eight computational levels |q1 q2 q3>, q in {0, 1}.

    H(a) = sum_q -(alpha_q / 2) b_q^dag b_q^dag b_q b_q + g (b_1^dag b_2 + b_1 b_2^dag + b_2^dag b_3 + b_2 b_3^dag)
           + sum_q a_qx (b_q + b_q^dag) + a_qy i (b_q^dag - b_q)
    H_s  = H + zeta_s b_1^dag b_1                    (the first transmon detuned by zeta_s)

in the frame rotating with the drives (energies in rad / ns).  The detuning landscape F(zeta) is ONE sweep over every detuning,
`RolloutSweep(..., wide=True, wide64=True)`: kernel "mfma64-sweep", one workgroup per (sample, chunk of intervals) with the 64 x 64
matrices in LDS.  Without `wide64` a system of this size runs one rollout per sample (the same call without the keyword: pass 0 as the
third argument to see it).  A handle made this way serves the forward sweep; with `wide64_grad=True` as well it serves gradients and
pullbacks, which three_transmon_polish.py uses to polish this pulse.

    python examples/three_transmon_robustness.py [T] [landscape] [wide64]
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g

LEVELS = 3
# |q1 q2 q3> has index 9 q1 + 3 q2 + q3
SUBSPACE = [9 * q1 + 3 * q2 + q3 for q1 in (0, 1) for q2 in (0, 1) for q3 in (0, 1)]


def three_transmons(alpha=(2 * np.pi * 0.22, 2 * np.pi * 0.20, 2 * np.pi * 0.21), coupling=2 * np.pi * 0.004):
    """(H_drift, [six drive operators], number operator of the first transmon), 27 x 27 complex."""
    b = np.diag(np.sqrt(np.arange(1.0, LEVELS)), 1).astype(complex)
    one = np.eye(LEVELS, dtype=complex)
    kron3 = lambda A, B, C_: np.kron(np.kron(A, B), C_)
    bs = (kron3(b, one, one), kron3(one, b, one), kron3(one, one, b))
    dag = lambda A: A.conj().T
    H0 = sum(-0.5 * al * dag(bq) @ dag(bq) @ bq @ bq for al, bq in zip(alpha, bs))
    H0 = H0 + coupling * sum(dag(bs[q]) @ bs[q + 1] + bs[q] @ dag(bs[q + 1]) for q in range(2))
    drives = [bq + dag(bq) for bq in bs] + [1j * (dag(bq) - bq) for bq in bs]
    return H0, drives, dag(bs[0]) @ bs[0]


def goal_gate():
    """X on the first transmon's qubit, identity on the others, embedded in the 27 levels (identity outside the subspace)."""
    U = np.eye(LEVELS ** 3, dtype=complex)
    X = np.array([[0, 1], [1, 0]], dtype=complex)
    U[np.ix_(SUBSPACE, SUBSPACE)] = np.kron(X, np.eye(4))
    return U


def run(T: int = 40, landscape: int = 41, wide64: bool = True, width: float = 2 * np.pi * 0.002, duration: float = 40.0, verbose: bool = True):
    """Returns the landscape over `landscape` detunings in [-2 width, 2 width], the kernel that served it and its launch."""
    qc = g.load_package()
    H0, drives, n1 = three_transmons()
    system = qc.QuantumSystem(H0, drives)
    N, m = LEVELS ** 3, len(drives)
    dt = duration / (T - 1)
    # a smooth pulse: half a Rabi turn on the first transmon's x drive, a little of everything else
    rng = np.random.default_rng(0)
    window = np.sin(np.pi * np.linspace(0.0, 1.0, T)) ** 2
    a = 0.1 * (np.pi / 2) / (duration * 0.5) * rng.uniform(-1, 1, (m, 1)) * window
    a[0] += (np.pi / 2) / (duration * 0.5) * window
    init, goal = qc.operator_to_iso_vec(np.eye(N, dtype=complex)), qc.operator_to_iso_vec(goal_gate())
    zl = np.linspace(-2 * width, 2 * width, landscape)
    sweep = qc.RolloutSweep(system, [n1], T, goal=goal, fid_kind="unitary", subspace=SUBSPACE, wide=True, wide64=wide64)
    try:
        kernel, launch = sweep.kernel_name, sweep.launch(landscape)
        Z = sweep.pack(a, np.full(T, dt))
        sweep.eval(Z, init, zl[:, None], finals=False)          # the first call loads the code objects
        t0 = time.perf_counter()
        F = sweep.eval(Z, init, zl[:, None], finals=False)[1]
        ms = 1e3 * (time.perf_counter() - t0)
    finally:
        sweep.close()
    if verbose:
        print(f"three three-level transmons (27 levels, 2N = 54), {T} knots of {dt:.2f} ns, {landscape} detunings in one sweep")
        print(f"kernel {kernel}; launch (mfma, chunk, n_chunks) = {launch}; second call {ms:.2f} ms with host copies")
        print("  zeta / 2 pi (MHz)    F")
        for zt, f in zip(zl[::max(1, landscape // 10)], F[::max(1, landscape // 10)]):
            print(f"  {1e3 * zt / (2 * np.pi):+10.3f}        {f:.6f}")
    return dict(landscape=F, detunings=zl, kernel=kernel, launch=launch, ms=ms)


if __name__ == "__main__":
    arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
    run(T=arg(1, 40), landscape=arg(2, 41), wide64=bool(arg(3, 1)))
