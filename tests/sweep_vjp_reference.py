"""Reference for the sweep pullbacks (`qc_sweep_vjp*`): the derivatives of phi_s = <cot[s], x_final[s]> over the final states of
tests/sweep_reference.py, with respect to the controls and timesteps of every interval, the initial state, theta[s, :] and c[s, :].
Nothing here calls the library.  Two routes:

  * `pullback_forward`: forward mode, the route of sweep_grad_reference.grad_samples_forward.  Per sample the columns of the Jacobian
    of the final state are built one by one -- a perturbation of a_{t,k} moves x_{t+1} by L(dt G; dt c_k G_k) x_t
    (scipy.linalg.expm_frechet), one of dt_t by G x_{t+1}, one of theta_j by L(dt G; dt P_j) x_t in EVERY interval, one of c_k by
    L(dt G; dt a_{t,k} G_k) x_t in every interval; each is carried to the final knot by the product of the later propagators -- and
    contracted with cot[s].  The final state is W x_0 with W the product of the expms, so grad_init = W^T cot[s].
  * `pullback_fd`: central differences of <cot[s], sweep_reference.sweep_finals(...)[:, s]>, which shares nothing with the first route
    but the chain itself.

Both return a dict: grad_samples len(samples) x (T-1) x (m + free), grad_init len(samples) x (n cols), grad_theta len(samples) x p,
grad_scale len(samples) x m.  cot is S x (n cols), indexed by the sample's own number."""
import numpy as np
import scipy.linalg as sla

import sweep_reference as ref


def _unpack(G0, Gd, Gp, controls, dts, theta, scale):
    G0 = np.asarray(G0, dtype=np.float64)
    n, m, p = G0.shape[0], len(Gd), len(Gp)
    controls = np.asarray(controls, dtype=np.float64)
    controls = controls.reshape(m, -1) if m else controls.reshape(0, controls.shape[-1])
    T = controls.shape[1]
    free = np.ndim(dts) != 0
    h = np.asarray(dts, dtype=np.float64).ravel() if free else np.full(T, float(dts))
    S = ref._n_samples(theta, scale)
    theta = np.asarray(theta, dtype=np.float64).reshape(S, p) if p else np.zeros((S, 0))
    scale = np.ones((S, m)) if scale is None else np.asarray(scale, dtype=np.float64).reshape(S, m)
    return G0, n, m, p, controls, T, free, h, S, theta, scale


def pullback_forward(G0, Gd, Gp, controls, dts, init, theta, scale, samples, cot):
    G0, n, m, p, controls, T, free, h, S, theta, scale = _unpack(G0, Gd, Gp, controls, dts, theta, scale)
    X0 = np.asarray(init, dtype=np.float64).reshape(n, -1, order="F")
    cot = np.asarray(cot, dtype=np.float64).reshape(S, -1)
    samples = list(samples)
    out = dict(grad_samples=np.zeros((len(samples), T - 1, m + (1 if free else 0))), grad_init=np.zeros((len(samples), X0.size)),
               grad_theta=np.zeros((len(samples), p)), grad_scale=np.zeros((len(samples), m)))
    for q, s in enumerate(samples):
        C = cot[s].reshape(n, -1, order="F")
        dot = lambda dX: float(np.sum(C * dX))
        Gs = [ref.sample_generator(G0, Gd, Gp, controls[:, t], theta[s], scale[s]) for t in range(T - 1)]
        Es = [sla.expm(h[t] * Gs[t]) for t in range(T - 1)]
        X = [X0]
        for t in range(T - 1):
            X.append(Es[t] @ X[t])
        B = np.eye(n)                         # E_{T-2} ... E_{t+1}
        for t in range(T - 2, -1, -1):
            frechet = lambda D: B @ (sla.expm_frechet(h[t] * Gs[t], D, compute_expm=False) @ X[t])
            for k in range(m):
                Gk = np.asarray(Gd[k], dtype=np.float64)
                out["grad_samples"][q, t, k] = dot(frechet((h[t] * scale[s, k]) * Gk))
                out["grad_scale"][q, k] += dot(frechet((h[t] * controls[k, t]) * Gk))
            for j in range(p):
                out["grad_theta"][q, j] += dot(frechet(h[t] * np.asarray(Gp[j], dtype=np.float64)))
            if free:
                out["grad_samples"][q, t, m] = dot(B @ (Gs[t] @ X[t + 1]))
            B = B @ Es[t]
        out["grad_init"][q] = (B.T @ C).reshape(-1, order="F")          # B = W now
    return out


def pullback_fd(G0, Gd, Gp, controls, dts, init, theta, scale, samples, cot, step=1e-5):
    G0, n, m, p, controls, T, free, h, S, theta, scale = _unpack(G0, Gd, Gp, controls, dts, theta, scale)
    samples = list(samples)
    init = np.asarray(init, dtype=np.float64).ravel()
    C = np.asarray(cot, dtype=np.float64).reshape(S, -1)[samples]
    th, sc = theta[samples], scale[samples]

    def phi(c=controls, d=dts, x0=init, t_=th, c_=sc):
        finals = ref.sweep_finals(G0, Gd, Gp, c, d, x0, t_ if p else np.zeros((len(samples), 0)), c_)      # (n cols) x len(samples)
        return np.einsum("sn,ns->s", C, finals)

    def central(make):
        return (phi(**make(+step)) - phi(**make(-step))) / (2 * step)

    def bumped(a, idx, e):
        b = np.array(a, dtype=np.float64)
        b[idx] += e
        return b

    out = dict(grad_samples=np.zeros((len(samples), T - 1, m + (1 if free else 0))), grad_init=np.zeros((len(samples), init.size)),
               grad_theta=np.zeros((len(samples), p)), grad_scale=np.zeros((len(samples), m)))
    for t in range(T - 1):
        for k in range(m):
            out["grad_samples"][:, t, k] = central(lambda e: dict(c=bumped(controls, (k, t), e)))
        if free:
            out["grad_samples"][:, t, m] = central(lambda e: dict(d=bumped(dts, t, e)))
    for i in range(init.size):
        out["grad_init"][:, i] = central(lambda e: dict(x0=bumped(init, i, e)))
    for j in range(p):          # the samples are independent: one step moves parameter j of every sample at once
        out["grad_theta"][:, j] = central(lambda e: dict(t_=bumped(th, (slice(None), j), e)))
    for k in range(m):
        out["grad_scale"][:, k] = central(lambda e: dict(c_=bumped(sc, (slice(None), k), e)))
    return out
