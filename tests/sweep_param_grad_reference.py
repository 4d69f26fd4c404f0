"""Reference for the sweep parameter gradients (`qc_sweep_grad_params*`): dF_s/dtheta[s, j] and dF_s/dc[s, k] of the fidelities of
tests/sweep_reference.py, the derivatives with respect to the parameters a sample's system is made of,

    G_s(a) = G_drift + sum_j theta[s, j] P_j + sum_k c[s, k] a_k G_k.

Nothing here calls the library.  Two routes, as in tests/sweep_grad_reference.py:

  * `param_terms_forward`: forward mode.  A perturbation of theta[s, j] moves x_{t+1} by L(dt G; dt P_j) x_t in EVERY interval, one of
    c[s, k] by L(dt G; dt a_{t,k} G_k) x_t (scipy.linalg.expm_frechet); each interval's move is carried to the final knot by the later
    propagators and through the fidelity's differential.  Returns the per-interval terms, len(samples) x (T-1) x (p + m) (the
    perturbations, then the drives), and their sums over the intervals, len(samples) x (p + m): the derivatives.
  * `param_grad_fd`: central differences of `sweep_reference.fidelities(sweep_reference.sweep_finals(...))` in theta and c."""
import numpy as np
import scipy.linalg as sla

import sweep_grad_reference as gref
import sweep_reference as ref


def param_terms_forward(G0, Gd, Gp, controls, dts, init, theta, scale, samples, kind, goal_iso, N, subspace=None, form="abs"):
    G0 = np.asarray(G0, dtype=np.float64)
    n, m, p = G0.shape[0], len(Gd), len(Gp)
    controls = np.asarray(controls, dtype=np.float64)
    controls = controls.reshape(m, -1) if m else controls.reshape(0, controls.shape[-1])
    T = controls.shape[1]
    h = np.asarray(dts, dtype=np.float64).ravel() if np.ndim(dts) != 0 else np.full(T, float(dts))
    S = ref._n_samples(theta, scale)
    theta = np.asarray(theta, dtype=np.float64).reshape(S, p) if p else None
    scale = np.ones((S, m)) if scale is None else np.asarray(scale, dtype=np.float64).reshape(S, m)
    X0 = np.asarray(init, dtype=np.float64).reshape(n, -1, order="F")
    terms = np.zeros((len(samples), T - 1, p + m))
    for q, s in enumerate(samples):
        th = theta[s] if theta is not None else ()
        Gs = [ref.sample_generator(G0, Gd, Gp, controls[:, t], th, scale[s]) for t in range(T - 1)]
        Es = [sla.expm(h[t] * Gs[t]) for t in range(T - 1)]
        X = [X0]
        for t in range(T - 1):
            X.append(Es[t] @ X[t])
        xT = X[-1].reshape(-1, order="F")
        B = np.eye(n)                         # E_{T-2} ... E_{t+1}
        for t in range(T - 2, -1, -1):
            dirs = [h[t] * np.asarray(P, dtype=np.float64) for P in Gp] + \
                   [(h[t] * controls[k, t]) * np.asarray(Gd[k], dtype=np.float64) for k in range(m)]
            for i, D in enumerate(dirs):
                Li = sla.expm_frechet(h[t] * Gs[t], D, compute_expm=False)
                dx = (B @ (Li @ X[t])).reshape(-1, order="F")
                terms[q, t, i] = gref.fidelity_differential(xT, dx, kind, goal_iso, N, subspace, form)
            B = B @ Es[t]
    return terms, terms.sum(axis=1)


def param_grad_fd(G0, Gd, Gp, controls, dts, init, theta, scale, samples, kind, goal_iso, N, subspace=None, form="abs", step=1e-5):
    m, p = len(Gd), len(Gp)
    S = ref._n_samples(theta, scale)
    samples = list(samples)
    th = np.asarray(theta, dtype=np.float64).reshape(S, p)[samples] if p else np.zeros((len(samples), 0))
    sc = np.ones((len(samples), m)) if scale is None else np.asarray(scale, dtype=np.float64).reshape(S, m)[samples]

    def F(t_, c_):
        return ref.fidelities(ref.sweep_finals(G0, Gd, Gp, controls, dts, init, t_, c_), kind, goal_iso, N, subspace, form)

    out = np.zeros((len(samples), p + m))
    for j in range(p):          # the samples are independent: one step moves parameter j of every sample at once
        tp, tm = th.copy(), th.copy()
        tp[:, j] += step
        tm[:, j] -= step
        out[:, j] = (F(tp, sc) - F(tm, sc)) / (2 * step)
    for k in range(m):
        cp, cm = sc.copy(), sc.copy()
        cp[:, k] += step
        cm[:, k] -= step
        out[:, p + k] = (F(th, cp) - F(th, cm)) / (2 * step)
    return out
