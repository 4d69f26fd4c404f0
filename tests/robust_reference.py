"""Independent numpy restatement of UnitaryRobustnessObjective (reference unitary_robustness_problem.jl:46-49):

    A_t = V_t' H V_t,   tau = sum_{t<K} dt_t,   R = (1/tau) sum_{t<K} dt_t A_t,   L = Re tr(R'R) / n

written in real iso arithmetic (iso(X) = [[Re X, -Im X], [Im X, Re X]], iso(X') = iso(X)^T) so that every quantity is an
analytic function of Z and the complex step applies: `loss` certifies `grad` (complex step of L), and `hessian` is the
complex step of the analytic gradient.  It is not the GPU's decomposition (no Gram rows, no corrections).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np


@dataclass
class RobustSpec:
    T: int
    zdim: int
    off_state: int
    N: int
    H: np.ndarray                      # n x n complex
    subspace: Optional[Sequence[int]] = None
    off_dt: int = -1
    dt_fixed: float = 0.0
    K: Optional[int] = None
    global_dim: int = 0

    @property
    def sub(self):
        return list(range(self.N)) if self.subspace is None else list(self.subspace)

    @property
    def n(self):
        return len(self.sub)

    @property
    def nK(self):
        return self.T if self.K is None else self.K


def iso(Xr, Xi):
    """(..., n, n) planes -> (..., 2n, 2n)."""
    top = np.concatenate([Xr, -Xi], axis=-1)
    bot = np.concatenate([Xi, Xr], axis=-1)
    return np.concatenate([top, bot], axis=-2)


def _state_index(s: RobustSpec):
    """(2, n, n) local offsets: [part, a, b] -> offset of Re/Im U[s_a, s_b] inside a knot."""
    sub = np.asarray(s.sub)
    a, b = np.meshgrid(sub, sub, indexing="ij")
    return np.stack([s.off_state + b * 2 * s.N + a, s.off_state + b * 2 * s.N + s.N + a])


def variables(s: RobustSpec) -> np.ndarray:
    """Sorted global indices of the term's variables."""
    loc = list(_state_index(s).ravel())
    if s.off_dt >= 0:
        loc.append(s.off_dt)
    loc = np.sort(np.asarray(loc))
    return (np.arange(s.nK)[:, None] * s.zdim + loc[None, :]).ravel()


def _pieces(Z, s: RobustSpec):
    Zk = Z[:s.T * s.zdim].reshape(s.T, s.zdim)[:s.nK]
    idx = _state_index(s)
    V = iso(Zk[:, idx[0]], Zk[:, idx[1]])                             # (K, 2n, 2n)
    Hi = iso(np.asarray(s.H).real, np.asarray(s.H).imag)
    dt = Zk[:, s.off_dt] if s.off_dt >= 0 else np.full(s.nK, s.dt_fixed)
    A = np.swapaxes(V, 1, 2) @ Hi @ V                                 # iso(V' H V)
    tau = dt.sum()
    R = np.tensordot(dt, A, axes=1) / tau
    return Zk, idx, V, Hi, dt, A, tau, R


def loss(Z, s: RobustSpec):
    R = _pieces(Z, s)[-1]
    return (R * R).sum() / (2 * s.n)                                  # tr(iso(R)^T iso(R)) = 2 Re tr(R'R)


def grad(Z, s: RobustSpec):
    """Analytic gradient, dense over Z (zeros outside the variables)."""
    Zk, idx, V, Hi, dt, A, tau, R = _pieces(Z, s)
    n = s.n
    G = Hi @ V @ R.T + Hi.T @ V @ R                                   # iso(H V R' + H' V R)
    G = G * (2.0 * dt / (n * tau))[:, None, None]
    out = np.zeros(Z.shape, dtype=Z.dtype)
    gk = out[:s.T * s.zdim].reshape(s.T, s.zdim)
    gk[:s.nK, idx[0]] = G[:, :n, :n]                                  # Re G
    gk[:s.nK, idx[1]] = G[:, n:, :n]                                  # Im G
    if s.off_dt >= 0:
        gk[:s.nK, s.off_dt] = np.einsum("ij,tij->t", R, A - R[None]) / (n * tau)
    return out


def complex_step_grad(Z, s: RobustSpec, h: float = 1e-30):
    Zc = np.asarray(Z, dtype=complex)
    out = np.zeros(Z.size)
    for i in variables(s):
        Zc[i] += 1j * h
        out[i] = loss(Zc, s).imag / h
        Zc[i] -= 1j * h
    return out


def hessian(Z, s: RobustSpec, h: float = 1e-30):
    """Dense V x V Hessian over `variables(s)`: column v is the complex step of the analytic gradient along v."""
    vs = variables(s)
    Zc = np.asarray(Z, dtype=complex)
    Hm = np.empty((vs.size, vs.size))
    for c, i in enumerate(vs):
        Zc[i] += 1j * h
        Hm[:, c] = grad(Zc, s)[vs].imag / h
        Zc[i] -= 1j * h
    return Hm


def packed_upper(Hm):
    """Column-major upper triangle: entry (i <= j) at j(j+1)/2 + i."""
    r, c = np.triu_indices(Hm.shape[0])
    order = np.lexsort((r, c))
    return Hm[r[order], c[order]]


def hessian_columns(Z, s: RobustSpec, cols, h: float = 1e-30):
    """Whole columns `cols` (positions in `variables(s)`) of the V x V Hessian, the method of `hessian`: (V, len(cols))."""
    vs = variables(s)
    Zc = np.asarray(Z, dtype=complex)
    out = np.empty((vs.size, len(cols)))
    for c, k in enumerate(cols):
        Zc[vs[k]] += 1j * h
        out[:, c] = grad(Zc, s)[vs].imag / h
        Zc[vs[k]] -= 1j * h
    return out


def hessian_vector_product(Z, s: RobustSpec, v, h: float = 1e-30):
    """H v over `variables(s)` by one complex step of the analytic gradient along v (no matrix is formed)."""
    vs = variables(s)
    Zc = np.asarray(Z, dtype=complex)
    Zc[vs] += 1j * h * np.asarray(v, dtype=float)
    return grad(Zc, s)[vs].imag / h


def packed_column(Hp, k):
    """Whole column k of the symmetric matrix whose column-major upper triangle is `Hp` (entry (i <= j) at j(j+1)/2 + i)."""
    V = int((np.sqrt(8.0 * Hp.size + 1.0) - 1.0) / 2.0 + 0.5)
    below = np.arange(k + 1, V, dtype=np.int64)
    return np.concatenate([Hp[k * (k + 1) // 2:k * (k + 1) // 2 + k + 1], Hp[below * (below + 1) // 2 + k]])


def packed_matvec(Hp, X):
    """(H X, |H| |X|) for the symmetric H packed in `Hp` and X (V, m), one stored column at a time: every value takes part."""
    X = np.asarray(X, dtype=float)
    V = X.shape[0]
    assert Hp.size == V * (V + 1) // 2
    Y, A = np.zeros_like(X), np.zeros_like(X)
    Xa = np.abs(X)
    for j in range(V):
        col = Hp[j * (j + 1) // 2:j * (j + 1) // 2 + j + 1]          # H[0..j, j]
        Y[:j + 1] += np.outer(col, X[j])
        A[:j + 1] += np.outer(np.abs(col), Xa[j])
        if j:
            Y[j] += col[:j] @ X[:j]                                   # H[j, 0..j-1] from the symmetric half
            A[j] += np.abs(col[:j]) @ Xa[:j]
    return Y, A
