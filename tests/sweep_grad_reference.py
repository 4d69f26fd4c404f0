"""Reference for the sweep gradients (`qc_sweep_grad*`): dF_s/da_{t,k} and dF_s/ddt_t of the fidelities of tests/sweep_reference.py.
Nothing here calls the library.  Two routes:

  * `grad_samples_forward`: forward mode.  E_t = expm(dt_t G_s(a_t)); a perturbation of a_{t,k} moves x_{t+1} by
    L(dt G; dt c_k G_k) x_t (scipy.linalg.expm_frechet), one of dt_t by G x_{t+1}; both are carried to the final knot by the product
    of the later propagators, and the fidelity's differential is the linearisation of sweep_reference's definitions in the complex
    overlap t: d|t|/n = Re(conj(t) dt) / (|t| n), d|t|^2 = 2 Re(conj(t) dt).
  * `grad_samples_fd`: central differences of `sweep_reference.fidelities(sweep_reference.sweep_finals(...))`, which shares nothing
    with the first route but the chain itself.

Both return an array of len(samples) x (T-1) x (m + free): per interval the m drives, then the timestep when `dts` is an array."""
import numpy as np
import scipy.linalg as sla

import sweep_reference as ref


def _overlap(x, kind, goal_iso, N, subspace):
    """The complex overlap t the fidelity is a function of, and its normaliser n; linear in x."""
    if kind == "unitary":
        U, G = ref.iso_vec_to_operator(x, N), ref.iso_vec_to_operator(goal_iso, N)
        if subspace is not None:
            ix = np.ix_(list(subspace), list(subspace))
            U, G = U[ix], G[ix]
        return np.trace(G.conj().T @ U), U.shape[0]
    L = len(goal_iso) // 2
    psi = np.asarray(x[:L]) + 1j * np.asarray(x[L:])
    g = np.asarray(goal_iso[:L]) + 1j * np.asarray(goal_iso[L:])
    return np.vdot(g, psi), 1


def fidelity_differential(x, dx, kind, goal_iso, N, subspace=None, form="abs"):
    """dF at the state x in the direction dx."""
    t, n = _overlap(x, kind, goal_iso, N, subspace)
    dt, _ = _overlap(dx, kind, goal_iso, N, subspace)
    re = (np.conj(t) * dt).real
    if kind == "unitary" and form == "abs":
        return re / (abs(t) * n)
    if kind == "unitary":
        return 2.0 * re / (n * n)
    return 2.0 * re


def grad_samples_forward(G0, Gd, Gp, controls, dts, init, theta, scale, samples, kind, goal_iso, N, subspace=None, form="abs"):
    G0 = np.asarray(G0, dtype=np.float64)
    n, m = G0.shape[0], len(Gd)
    controls = np.asarray(controls, dtype=np.float64).reshape(m, -1)
    T = controls.shape[1]
    free = np.ndim(dts) != 0
    h = np.asarray(dts, dtype=np.float64).ravel() if free else np.full(T, float(dts))
    S = ref._n_samples(theta, scale)
    theta = np.asarray(theta, dtype=np.float64).reshape(S, len(Gp)) if len(Gp) else None
    scale = np.ones((S, m)) if scale is None else np.asarray(scale, dtype=np.float64).reshape(S, m)
    X0 = np.asarray(init, dtype=np.float64).reshape(n, -1, order="F")
    out = np.zeros((len(samples), T - 1, m + (1 if free else 0)))
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
            for k in range(m):
                Lk = sla.expm_frechet(h[t] * Gs[t], (h[t] * scale[s, k]) * np.asarray(Gd[k], dtype=np.float64), compute_expm=False)
                dx = (B @ (Lk @ X[t])).reshape(-1, order="F")
                out[q, t, k] = fidelity_differential(xT, dx, kind, goal_iso, N, subspace, form)
            if free:
                dx = (B @ (Gs[t] @ X[t + 1])).reshape(-1, order="F")
                out[q, t, m] = fidelity_differential(xT, dx, kind, goal_iso, N, subspace, form)
            B = B @ Es[t]
    return out


def grad_samples_fd(G0, Gd, Gp, controls, dts, init, theta, scale, samples, kind, goal_iso, N, subspace=None, form="abs", step=1e-5):
    m = len(Gd)
    controls = np.asarray(controls, dtype=np.float64).reshape(m, -1)
    T = controls.shape[1]
    free = np.ndim(dts) != 0
    S = ref._n_samples(theta, scale)
    samples = list(samples)
    th = np.asarray(theta, dtype=np.float64).reshape(S, -1)[samples]
    sc = None if scale is None else np.asarray(scale, dtype=np.float64).reshape(S, m)[samples]

    def F(c, d):
        return ref.fidelities(ref.sweep_finals(G0, Gd, Gp, c, d, init, th, sc), kind, goal_iso, N, subspace, form)

    out = np.zeros((len(samples), T - 1, m + (1 if free else 0)))
    for t in range(T - 1):
        for k in range(m):
            cp, cm = controls.copy(), controls.copy()
            cp[k, t] += step
            cm[k, t] -= step
            out[:, t, k] = (F(cp, dts) - F(cm, dts)) / (2 * step)
        if free:
            dp, dm = np.array(dts, dtype=np.float64), np.array(dts, dtype=np.float64)
            dp[t] += step
            dm[t] -= step
            out[:, t, m] = (F(controls, dp) - F(controls, dm)) / (2 * step)
    return out
