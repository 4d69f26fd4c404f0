"""Reference for the noise-trajectory sweeps (`qc_sweep_noise_*`): the scipy chain of tests/sweep_reference.py with a generator that
changes from interval to interval,

    G_{s,t} = G_drift + sum_j (theta[s, j] + noise[s, t, j]) P_j + sum_k c[s, k] a_{t,k} G_k,      x_{t+1} = expm(dt_t G_{s,t}) x_t,

and its derivatives in the pattern of tests/sweep_grad_reference.py.  Nothing here calls the library.

  * `noise_finals`: the final states, (n cols) x S.
  * `noise_grads_forward`: forward mode.  A perturbation of a_{t,k} moves x_{t+1} by L(dt G; dt c_k G_k) x_t, one of noise[s,t,j] by
    L(dt G; dt P_j) x_t (scipy.linalg.expm_frechet), one of dt_t by G x_{t+1}; all are carried to the final knot by the later
    propagators, and the fidelity's differential is sweep_grad_reference.fidelity_differential.
  * `noise_grads_fd`: central differences of `sweep_reference.fidelities(noise_finals(...))`.

The gradient routes return (grad_samples, grad_noise): len(samples) x (T-1) x (m + free) -- per interval the m drives, then the timestep
when `dts` is an array -- and len(samples) x (T-1) x p."""
import numpy as np
import scipy.linalg as sla

import sweep_grad_reference as gref
import sweep_reference as ref


def _args(G0, Gd, Gp, controls, dts, theta, scale, noise):
    m, p = len(Gd), len(Gp)
    noise = np.asarray(noise, dtype=np.float64)
    S, T = noise.shape[0], noise.shape[1] + 1              # the noise gives both (m may be 0: the controls cannot)
    noise = noise.reshape(S, T - 1, p)
    controls = np.asarray(controls, dtype=np.float64).reshape(m, T)
    free = np.ndim(dts) != 0
    h = np.asarray(dts, dtype=np.float64).ravel() if free else np.full(T, float(dts))
    theta = np.zeros((S, p)) if theta is None else np.asarray(theta, dtype=np.float64).reshape(S, p)
    scale = np.ones((S, m)) if scale is None else np.asarray(scale, dtype=np.float64).reshape(S, m)
    return controls, T, free, h, S, noise, theta, scale


def interval_generator(G0, Gd, Gp, a, theta_s, c_s, xi_st):
    """G_{s,t}: sweep_reference.sample_generator at theta + xi."""
    return ref.sample_generator(G0, Gd, Gp, a, np.asarray(theta_s) + np.asarray(xi_st), c_s)


def noise_finals(G0, Gd, Gp, controls, dts, init, theta, scale, noise):
    """Final states, (n cols) x S.  noise S x (T-1) x p (S x (T-1) when p = 1); theta S x p or None = zeros; scale S x m or None."""
    G0 = np.asarray(G0, dtype=np.float64)
    n = G0.shape[0]
    controls, T, free, h, S, noise, theta, scale = _args(G0, Gd, Gp, controls, dts, theta, scale, noise)
    X0 = np.asarray(init, dtype=np.float64).reshape(n, -1, order="F")
    out = np.empty((X0.size, S))
    for s in range(S):
        X = X0.copy()
        for t in range(T - 1):
            X = sla.expm(h[t] * interval_generator(G0, Gd, Gp, controls[:, t], theta[s], scale[s], noise[s, t])) @ X
        out[:, s] = X.reshape(-1, order="F")
    return out


def noise_grads_forward(G0, Gd, Gp, controls, dts, init, theta, scale, noise, samples, kind, goal_iso, N, subspace=None, form="abs"):
    G0 = np.asarray(G0, dtype=np.float64)
    n, m, p = G0.shape[0], len(Gd), len(Gp)
    controls, T, free, h, S, noise, theta, scale = _args(G0, Gd, Gp, controls, dts, theta, scale, noise)
    X0 = np.asarray(init, dtype=np.float64).reshape(n, -1, order="F")
    gs = np.zeros((len(samples), T - 1, m + (1 if free else 0)))
    gn = np.zeros((len(samples), T - 1, p))
    for q, s in enumerate(samples):
        Gs = [interval_generator(G0, Gd, Gp, controls[:, t], theta[s], scale[s], noise[s, t]) for t in range(T - 1)]
        Es = [sla.expm(h[t] * Gs[t]) for t in range(T - 1)]
        X = [X0]
        for t in range(T - 1):
            X.append(Es[t] @ X[t])
        xT = X[-1].reshape(-1, order="F")
        dF = lambda dx: gref.fidelity_differential(xT, dx.reshape(-1, order="F"), kind, goal_iso, N, subspace, form)
        B = np.eye(n)                         # E_{T-2} ... E_{t+1}
        for t in range(T - 2, -1, -1):
            for k in range(m):
                Lk = sla.expm_frechet(h[t] * Gs[t], (h[t] * scale[s, k]) * np.asarray(Gd[k], dtype=np.float64), compute_expm=False)
                gs[q, t, k] = dF(B @ (Lk @ X[t]))
            for j in range(p):
                Lj = sla.expm_frechet(h[t] * Gs[t], h[t] * np.asarray(Gp[j], dtype=np.float64), compute_expm=False)
                gn[q, t, j] = dF(B @ (Lj @ X[t]))
            if free:
                gs[q, t, m] = dF(B @ (Gs[t] @ X[t + 1]))
            B = B @ Es[t]
    return gs, gn


def noise_grads_fd(G0, Gd, Gp, controls, dts, init, theta, scale, noise, samples, kind, goal_iso, N, subspace=None, form="abs", step=1e-5):
    m, p = len(Gd), len(Gp)
    controls, T, free, h, S, noise, theta, scale = _args(G0, Gd, Gp, controls, dts, theta, scale, noise)
    samples = list(samples)
    th, sc, xi = theta[samples], scale[samples], noise[samples]

    def F(c, d, x):
        return ref.fidelities(noise_finals(G0, Gd, Gp, c, d, init, th, sc, x), kind, goal_iso, N, subspace, form)

    gs = np.zeros((len(samples), T - 1, m + (1 if free else 0)))
    gn = np.zeros((len(samples), T - 1, p))
    d0 = h if free else float(dts)
    for t in range(T - 1):
        for k in range(m):
            cp, cm = controls.copy(), controls.copy()
            cp[k, t] += step
            cm[k, t] -= step
            gs[:, t, k] = (F(cp, d0, xi) - F(cm, d0, xi)) / (2 * step)
        for j in range(p):      # every sample's own noise entry moves: the samples are independent
            xp, xm = xi.copy(), xi.copy()
            xp[:, t, j] += step
            xm[:, t, j] -= step
            gn[:, t, j] = (F(controls, d0, xp) - F(controls, d0, xm)) / (2 * step)
        if free:
            dp, dm = h.copy(), h.copy()
            dp[t] += step
            dm[t] -= step
            gs[:, t, m] = (F(controls, dp, xi) - F(controls, dm, xi)) / (2 * step)
    return gs, gn
