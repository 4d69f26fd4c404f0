"""Term-by-term restatement of the trajectory-terms pass in np.longdouble: plain Python loops over (knot, term), no array
arithmetic and no code shared with terms_ext_reference.py.  The cost (include/qcolloc.h, qc_terms_desc / qc_terms_ext) is

    J = sum_t 1/2 sc_t^2 sum_k R_k (x_t[r_k] - b_tk)^2 + D sum_{t<n_mt} dt_t          regulariser, minimum time
      + 1/2 sum_{t<T-1} sum_k S_k (x_{t+1}[s_k] - x_t[s_k])^2                          smoothness
      + sum_t 1/2 sc_t^2 sum_p Q_p (x_t[a_p] - x_t[b_p])^2                             pairwise
      + sum_t sum_k w_k x_t[l_k]                                                       linear slack cost

with sc_t = dt_t (dt_scaled) or 1 and dt_t = x_t[off_dt] (free timestep) or dt_fixed.

`evaluate(tm, Z)` reads the description by attribute name (T, zdim, off_dt, dt_fixed, global_dim, dt_scaled, reg_index, reg_R,
baseline (T, n_reg) or None, D, n_mt, s_index, s_R, p_a, p_b, p_Q, l_index, l_w) and returns a `Slow` with J, the gradient and the
Hessian values in the library's COO order, and next to every one of those numbers the sum of the absolute values of the terms
that make it up: A_J, A_g[i], A_H[e].  A Hessian value that is one product has A_H = its absolute value; the two (dt, dt) sums
sum_k R_k dv_k^2 and sum_p Q_p d_p^2 have the sum of their absolute addends.  `Slow.detail` keeps the addends themselves (per knot,
per entry, per pair), from which tests build deliberately wrong outputs."""
import numpy as np

L = np.longdouble


class Slow:
    pass


def _accumulator(n):
    val = [L(0)] * n
    mag = [L(0)] * n

    def add(i, term):
        val[i] = val[i] + term
        mag[i] = mag[i] + abs(term)
    return val, mag, add


def evaluate(tm, Z, want_hess=True):
    T, zd, off = int(tm.T), int(tm.zdim), int(tm.off_dt)
    free = off >= 0
    scaled = bool(tm.dt_scaled)
    z = np.asarray(Z, dtype=L)
    x = lambda t, j: z[t * zd + int(j)]
    half, two = L(1) / L(2), L(2)
    n_reg, n_s, n_p, n_l = len(tm.reg_index), len(tm.s_index), len(tm.p_a), len(tm.l_index)
    R = [L(v) for v in tm.reg_R]
    S = [L(v) for v in tm.s_R]
    Q = [L(v) for v in tm.p_Q]
    W = [L(v) for v in tm.l_w]
    D = L(tm.D)
    cross = scaled and free and n_reg > 0
    cross_p = scaled and free and n_p > 0

    n = T * zd + int(tm.global_dim)
    g, A_g, add_g = _accumulator(n)
    Jv, A_J, add_J = _accumulator(1)
    part = [L(0)] * T                      # the terms of J that knot t owns (a forward difference belongs to its left end)
    q_add = [[] for _ in range(T)]         # (entry, R_k dv^2)
    qp_add = [[] for _ in range(T)]        # (pair, Q_p d^2)
    g_reg = [dict() for _ in range(T)]     # entry -> R_k sc^2 dv
    g_pair = [dict() for _ in range(T)]    # entry -> [Q_p sc^2 (x_j - x_partner) in pair order]
    rows, cols, H, A_H = [], [], [], []

    def put(r, c, v, a=None):
        rows.append(min(r, c))
        cols.append(max(r, c))
        H.append(v)
        A_H.append(abs(v) if a is None else a)

    def own(t, term):
        add_J(0, term)
        part[t] = part[t] + term

    dts = [x(t, off) if free else L(tm.dt_fixed) for t in range(T)]
    scs = [dts[t] if scaled else L(1) for t in range(T)]

    # regulariser and minimum time; Hessian prefix
    for t in range(T):
        dt, sc, c0 = dts[t], scs[t], t * zd
        dvs = []
        for k in range(n_reg):
            j = int(tm.reg_index[k])
            dv = x(t, j) - (L(tm.baseline[t][k]) if tm.baseline is not None else L(0))
            dvs.append(dv)
            own(t, half * sc * sc * R[k] * dv * dv)
            gr = R[k] * sc * sc * dv
            add_g(c0 + j, gr)
            g_reg[t][j] = gr
            q_add[t].append((j, R[k] * dv * dv))
            if scaled and free:
                add_g(c0 + off, dt * R[k] * dv * dv)
        if free and t < int(tm.n_mt):
            own(t, D * dt)
            add_g(c0 + off, D)
        if want_hess:
            for k in range(n_reg):
                j = c0 + int(tm.reg_index[k])
                put(j, j, R[k] * sc * sc)
            if cross:
                for k in range(n_reg):
                    put(c0 + int(tm.reg_index[k]), c0 + off, two * dt * R[k] * dvs[k])
                terms = [R[k] * dvs[k] * dvs[k] for k in range(n_reg)]
                put(c0 + off, c0 + off, sum(terms, L(0)), sum((abs(v) for v in terms), L(0)))

    # smoothness
    for t in range(T):
        c0 = t * zd
        if t + 1 < T:
            for k in range(n_s):
                j = int(tm.s_index[k])
                dn = x(t + 1, j) - x(t, j)
                own(t, half * S[k] * dn * dn)
                add_g(c0 + j, -(S[k] * dn))
                add_g(c0 + zd + j, S[k] * dn)
        if want_hess:
            nb = L(int(t > 0) + int(t + 1 < T))
            for k in range(n_s):
                j = c0 + int(tm.s_index[k])
                put(j, j, S[k] * nb)
            if t + 1 < T:
                for k in range(n_s):
                    j = c0 + int(tm.s_index[k])
                    put(j, j + zd, -S[k])

    # pairwise
    for t in range(T):
        dt, sc, c0 = dts[t], scs[t], t * zd
        ds = []
        for p in range(n_p):
            a, b = int(tm.p_a[p]), int(tm.p_b[p])
            d = x(t, a) - x(t, b)
            ds.append(d)
            own(t, half * sc * sc * Q[p] * d * d)
            add_g(c0 + a, Q[p] * sc * sc * d)
            add_g(c0 + b, -(Q[p] * sc * sc * d))
            g_pair[t].setdefault(a, []).append(Q[p] * sc * sc * d)
            g_pair[t].setdefault(b, []).append(-(Q[p] * sc * sc * d))
            qp_add[t].append((p, Q[p] * d * d))
            if scaled and free:
                add_g(c0 + off, dt * Q[p] * d * d)
        if want_hess and n_p:
            for p in range(n_p):
                put(c0 + int(tm.p_a[p]), c0 + int(tm.p_a[p]), Q[p] * sc * sc)
            for p in range(n_p):
                put(c0 + int(tm.p_b[p]), c0 + int(tm.p_b[p]), Q[p] * sc * sc)
            for p in range(n_p):
                put(c0 + int(tm.p_a[p]), c0 + int(tm.p_b[p]), -(Q[p] * sc * sc))
            if cross_p:
                for p in range(n_p):
                    put(c0 + int(tm.p_a[p]), c0 + off, two * dt * Q[p] * ds[p])
                for p in range(n_p):
                    put(c0 + int(tm.p_b[p]), c0 + off, -(two * dt * Q[p] * ds[p]))
                terms = [Q[p] * ds[p] * ds[p] for p in range(n_p)]
                put(c0 + off, c0 + off, sum(terms, L(0)), sum((abs(v) for v in terms), L(0)))

    # linear slack cost
    for t in range(T):
        for k in range(n_l):
            j = int(tm.l_index[k])
            own(t, W[k] * x(t, j))
            add_g(t * zd + j, W[k])

    s = Slow()
    s.J, s.A_J = Jv[0], A_J[0]
    s.g, s.A_g = np.array(g, dtype=L), np.array(A_g, dtype=L)
    s.H, s.A_H = np.array(H, dtype=L), np.array(A_H, dtype=L)
    s.rows, s.cols = np.array(rows, dtype=np.int64), np.array(cols, dtype=np.int64)
    s.detail = {"part": part, "q_add": q_add, "qp_add": qp_add, "g_reg": g_reg, "g_pair": g_pair, "dt": dts, "sc": scs,
                "cross": cross, "cross_p": cross_p}
    return s


def dense_hessian(s, n):
    """The full symmetric matrix of the COO values (repeated positions add up)."""
    M = np.zeros((n, n), dtype=L)
    for r, c, v in zip(s.rows, s.cols, s.H):
        M[r, c] += v
        if r != c:
            M[c, r] += v
    return M
