"""numpy restatement of the trajectory-terms pass with its extension terms (include/qcolloc.h, qc_terms_ext):

    J = sum_t 1/2 sc_t^2 sum_k R_k (x_t[r_k] - b_tk)^2 + D sum_{t<n_mt} dt_t          regulariser, minimum time
      + 1/2 sum_{t<T-1} sum_k S_k (x_{t+1}[s_k] - x_t[s_k])^2                          smoothness
      + sum_t 1/2 sc_t^2 sum_p Q_p (x_t[a_p] - x_t[b_p])^2                             pairwise
      + sum_t sum_k w_k x_t[l_k]                                                       linear slack cost

with sc_t = dt_t (dt_scaled) or 1.  `value` accepts complex Z (complex-step derivatives); `grad` is analytic and dense;
`hess_values` / `hess_structure` restate the library's COO layout; `hess_dense` sums them into the full symmetric matrix.
tests/test_terms_ext.py certifies `grad` by complex step and `hess_dense` by finite differences of `grad`."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional

import numpy as np


def _i(a):
    return np.asarray(a if a is not None else [], dtype=np.int64)


def _f(a):
    return np.asarray(a if a is not None else [], dtype=np.float64)


@dataclass
class TermsExt:
    T: int
    zdim: int
    off_dt: int = -1
    dt_fixed: float = 0.2
    global_dim: int = 0
    dt_scaled: bool = True
    reg_index: np.ndarray = field(default_factory=lambda: _i(None))
    reg_R: np.ndarray = field(default_factory=lambda: _f(None))
    baseline: Optional[np.ndarray] = None          # (T, n_reg)
    D: float = 0.0
    n_mt: int = 0
    s_index: np.ndarray = field(default_factory=lambda: _i(None))
    s_R: np.ndarray = field(default_factory=lambda: _f(None))
    p_a: np.ndarray = field(default_factory=lambda: _i(None))
    p_b: np.ndarray = field(default_factory=lambda: _i(None))
    p_Q: np.ndarray = field(default_factory=lambda: _f(None))
    l_index: np.ndarray = field(default_factory=lambda: _i(None))
    l_w: np.ndarray = field(default_factory=lambda: _f(None))

    @property
    def free(self):
        return self.off_dt >= 0

    @property
    def cross(self):
        return self.dt_scaled and self.free and len(self.reg_index) > 0

    @property
    def cross_p(self):
        return self.dt_scaled and self.free and len(self.p_a) > 0

    @property
    def Z_len(self):
        return self.T * self.zdim + self.global_dim


def _knots(tm: TermsExt, Z):
    X = Z[:tm.T * tm.zdim].reshape(tm.T, tm.zdim)
    dt = X[:, tm.off_dt] if tm.free else np.full(tm.T, tm.dt_fixed)
    sc = dt if tm.dt_scaled else np.ones(tm.T)
    return X, dt, sc


def value(tm: TermsExt, Z):
    X, dt, sc = _knots(tm, Z)
    J = 0.0
    if len(tm.reg_index):
        dv = X[:, tm.reg_index] - (tm.baseline if tm.baseline is not None else 0.0)
        J = J + 0.5 * np.sum(sc ** 2 * np.sum(tm.reg_R * dv ** 2, axis=1))
    if tm.D:
        J = J + tm.D * np.sum(dt[:tm.n_mt])
    if len(tm.s_index) and tm.T > 1:
        df = X[1:, tm.s_index] - X[:-1, tm.s_index]
        J = J + 0.5 * np.sum(tm.s_R * df ** 2)
    if len(tm.p_a):
        d = X[:, tm.p_a] - X[:, tm.p_b]
        J = J + 0.5 * np.sum(sc ** 2 * np.sum(tm.p_Q * d ** 2, axis=1))
    if len(tm.l_index):
        J = J + np.sum(X[:, tm.l_index] * tm.l_w)
    return J


def grad(tm: TermsExt, Z):
    Z = np.asarray(Z, dtype=np.float64)
    X, dt, sc = _knots(tm, Z)
    G = np.zeros((tm.T, tm.zdim))
    if len(tm.reg_index):
        dv = X[:, tm.reg_index] - (tm.baseline if tm.baseline is not None else 0.0)
        np.add.at(G, (slice(None), tm.reg_index), (sc ** 2)[:, None] * tm.reg_R * dv)
        if tm.free and tm.dt_scaled:
            G[:, tm.off_dt] += dt * np.sum(tm.reg_R * dv ** 2, axis=1)
    if tm.D and tm.free:
        G[:tm.n_mt, tm.off_dt] += tm.D
    if len(tm.s_index) and tm.T > 1:
        df = tm.s_R * (X[1:, tm.s_index] - X[:-1, tm.s_index])
        G[:-1, tm.s_index] -= df
        G[1:, tm.s_index] += df
    if len(tm.p_a):
        d = X[:, tm.p_a] - X[:, tm.p_b]
        gp = (sc ** 2)[:, None] * tm.p_Q * d
        np.add.at(G, (slice(None), tm.p_a), gp)
        np.add.at(G, (slice(None), tm.p_b), -gp)
        if tm.free and tm.dt_scaled:
            G[:, tm.off_dt] += dt * np.sum(tm.p_Q * d ** 2, axis=1)
    if len(tm.l_index):
        G[:, tm.l_index] += tm.l_w
    return np.concatenate([G.ravel(), np.zeros(tm.global_dim)])


def hess_nnz(tm: TermsExt):
    nr, ns, npr = len(tm.reg_index), len(tm.s_index), len(tm.p_a)
    return tm.T * (nr * (1 + tm.cross) + tm.cross) + ns * (2 * tm.T - 1) + tm.T * (3 * npr + tm.cross_p * (2 * npr + 1))


def hess_structure(tm: TermsExt):
    rows, cols = [], []

    def put(r, c):
        rows.append(min(r, c))
        cols.append(max(r, c))
    for t in range(tm.T):
        c0 = t * tm.zdim
        for j in tm.reg_index:
            put(c0 + j, c0 + j)
        if tm.cross:
            for j in tm.reg_index:
                put(c0 + j, c0 + tm.off_dt)
            put(c0 + tm.off_dt, c0 + tm.off_dt)
    for t in range(tm.T):
        c0 = t * tm.zdim
        for j in tm.s_index:
            put(c0 + j, c0 + j)
        if t + 1 < tm.T:
            for j in tm.s_index:
                put(c0 + j, c0 + tm.zdim + j)
    for t in range(tm.T):
        c0 = t * tm.zdim
        for a in tm.p_a:
            put(c0 + a, c0 + a)
        for b in tm.p_b:
            put(c0 + b, c0 + b)
        for a, b in zip(tm.p_a, tm.p_b):
            put(c0 + a, c0 + b)
        if tm.cross_p:
            for a in tm.p_a:
                put(c0 + a, c0 + tm.off_dt)
            for b in tm.p_b:
                put(c0 + b, c0 + tm.off_dt)
            put(c0 + tm.off_dt, c0 + tm.off_dt)
    return np.array(rows, dtype=np.int64), np.array(cols, dtype=np.int64)


def hess_values(tm: TermsExt, Z):
    Z = np.asarray(Z, dtype=np.float64)
    X, dt, sc = _knots(tm, Z)
    out = []
    for t in range(tm.T):
        if len(tm.reg_index):
            dv = X[t, tm.reg_index] - (tm.baseline[t] if tm.baseline is not None else 0.0)
            out.append(tm.reg_R * sc[t] ** 2)
            if tm.cross:
                out.append(2.0 * dt[t] * tm.reg_R * dv)
                out.append([np.sum(tm.reg_R * dv ** 2)])
    for t in range(tm.T):
        nb = (t > 0) + (t + 1 < tm.T)
        out.append(tm.s_R * nb)
        if t + 1 < tm.T:
            out.append(-tm.s_R)
    for t in range(tm.T):
        if not len(tm.p_a):
            break
        d = X[t, tm.p_a] - X[t, tm.p_b]
        v = tm.p_Q * sc[t] ** 2
        out += [v, v, -v]
        if tm.cross_p:
            out += [2.0 * dt[t] * tm.p_Q * d, -2.0 * dt[t] * tm.p_Q * d, [np.sum(tm.p_Q * d ** 2)]]
    return np.concatenate([np.asarray(o, dtype=np.float64).ravel() for o in out]) if out else np.zeros(0)


def hess_dense(tm: TermsExt, Z):
    r, c = hess_structure(tm)
    H = np.zeros((tm.Z_len, tm.Z_len))
    np.add.at(H, (r, c), hess_values(tm, Z))
    return np.triu(H) + np.triu(H, 1).T
