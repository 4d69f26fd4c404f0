"""Reference for the sweep Hessian products (`qc_sweep_hvp*`): the tangent of the pullback of tests/sweep_vjp_reference.py along one
direction (vcontrols, vdts, vinit, vtheta, vscale, vcot).  With phi_s = <cot[s], x_final[s]>, g_s = dphi_s/d(a_t, h_t) and
q_s = dphi_s/dinit:

    tgrad_samples[s] = d/de g_s(Z + e vZ, init + e vinit, theta + e vtheta, c + e vc; cot + e vcot) at e = 0
    tgrad_init[s]    = d/de q_s

Nothing here calls the library.  Two routes that share only the chain:

  * `hessian_product_frechet`: the recurrences.  A_t = h_t G_s(a_t), Adot_t = vh_t G_s(a_t) + h_t Gdot_t; E_t, Edot_t from
    scipy.linalg.expm_frechet; xdot_{t+1} = E_t xdot_t + Edot_t x_t forwards, lambdadot_t = E_t^T lambdadot_{t+1} + Edot_t^T lambda_{t+1}
    backwards from lambdadot_{T-1} = vcot[s]; with D_k = h c_k G_k and Ddot_k = (vh c_k + h vc_k) G_k

        gdot_{t,k} = <lambdadot_{t+1}, L(A; D_k) x_t> + <lambda_{t+1}, L2(A; D_k, Adot) x_t> + <lambda_{t+1}, L(A; Ddot_k) x_t>
                     + <lambda_{t+1}, L(A; D_k) xdot_t>
        gdot_{t,h} = <lambdadot_{t+1}, G x_{t+1}> + <lambda_{t+1}, Gdot x_{t+1}> + <lambda_{t+1}, G xdot_{t+1}>

    L from expm_frechet, the second Frechet derivative L2(A; D1, D2) as the top-right block of expm of the 4n x 4n matrix
    [[A, D1, D2, 0], [0, A, 0, D2], [0, 0, A, D1], [0, 0, 0, A]].
  * `hessian_product_complex_step`: the complex step, eps = 1e-30, through a transcription of sweep_vjp_reference.pullback_forward that
    takes complex arrays (expm_frechet accepts them; the pairing is the bilinear sum, not the Hermitian one).  Tangent = Im / eps.

Both return a dict: tgrad_samples len(samples) x (T-1) x (m + free), tgrad_init len(samples) x (n cols).  cot and vcot are
S x (n cols), indexed by the sample's own number; every direction may be None (zero)."""
import numpy as np
import scipy.linalg as sla

import sweep_jvp_reference as jref
import sweep_reference as ref

EPS = 1e-30


def frechet2(A, D1, D2):
    """The second Frechet derivative of exp at A in the directions D1, D2."""
    n = A.shape[0]
    Z = np.zeros_like(A)
    M = np.block([[A, D1, D2, Z], [Z, A, Z, D2], [Z, Z, A, D1], [Z, Z, Z, A]])
    return sla.expm(M)[:n, 3 * n:]


def _cot(a, S, shape):
    return np.zeros((S,) + shape) if a is None else np.asarray(a, dtype=np.float64).reshape(S, -1)


def hessian_product_frechet(G0, Gd, Gp, controls, dts, init, theta, scale, samples, cot, vcontrols=None, vdts=None, vinit=None, vtheta=None,
                            vscale=None, vcot=None):
    G0, n, m, p, controls, T, h, theta, scale, va, vh, X0, V0, vth, vsc = jref._unpack(G0, Gd, Gp, controls, dts, theta, scale, vcontrols, vdts,
                                                                                         vinit, vtheta, vscale, init)
    free = np.ndim(dts) != 0
    S = theta.shape[0]
    cot, vcot = _cot(cot, S, (X0.size,)), _cot(vcot, S, (X0.size,))
    samples = list(samples)
    Gk = [np.asarray(G, dtype=np.float64) for G in Gd]
    out = dict(tgrad_samples=np.zeros((len(samples), T - 1, m + (1 if free else 0))), tgrad_init=np.zeros((len(samples), X0.size)))
    dot = lambda a, b: float(np.sum(a * b))
    for q, s in enumerate(samples):
        G = [ref.sample_generator(G0, Gd, Gp, controls[:, t], theta[s], scale[s]) for t in range(T - 1)]
        Gdot = [jref._generator_tangent(Gd, Gp, controls[:, t], va[:, t], scale[s], vth[s], vsc[s], n) for t in range(T - 1)]
        A = [h[t] * G[t] for t in range(T - 1)]
        Adot = [vh[t] * G[t] + h[t] * Gdot[t] for t in range(T - 1)]
        EL = [sla.expm_frechet(A[t], Adot[t]) for t in range(T - 1)]
        X, V = [X0], [V0]
        for t in range(T - 1):
            E, Ed = EL[t]
            V.append(E @ V[t] + Ed @ X[t])
            X.append(E @ X[t])
        lam, lamd = cot[s].reshape(n, -1, order="F"), vcot[s].reshape(n, -1, order="F")
        for t in range(T - 2, -1, -1):
            E, Ed = EL[t]
            for k in range(m):
                D = (h[t] * scale[s, k]) * Gk[k]
                Dd = (vh[t] * scale[s, k] + h[t] * vsc[s, k]) * Gk[k]
                L1 = sla.expm_frechet(A[t], D, compute_expm=False)
                out["tgrad_samples"][q, t, k] = (dot(lamd, L1 @ X[t]) + dot(lam, frechet2(A[t], D, Adot[t]) @ X[t])
                                                 + dot(lam, sla.expm_frechet(A[t], Dd, compute_expm=False) @ X[t]) + dot(lam, L1 @ V[t]))
            if free:
                out["tgrad_samples"][q, t, m] = dot(lamd, G[t] @ X[t + 1]) + dot(lam, Gdot[t] @ X[t + 1]) + dot(lam, G[t] @ V[t + 1])
            lamd = E.T @ lamd + Ed.T @ lam
            lam = E.T @ lam
        out["tgrad_init"][q] = lamd.reshape(-1, order="F")
    return out


def hessian_product_complex_step(G0, Gd, Gp, controls, dts, init, theta, scale, samples, cot, vcontrols=None, vdts=None, vinit=None, vtheta=None,
                                 vscale=None, vcot=None):
    G0, n, m, p, controls, T, h, theta, scale, va, vh, X0, V0, vth, vsc = jref._unpack(G0, Gd, Gp, controls, dts, theta, scale, vcontrols, vdts,
                                                                                         vinit, vtheta, vscale, init)
    free = np.ndim(dts) != 0
    S = theta.shape[0]
    cot, vcot = _cot(cot, S, (X0.size,)), _cot(vcot, S, (X0.size,))
    samples = list(samples)
    Gk = [np.asarray(G, dtype=np.float64) for G in Gd]
    Pj = [np.asarray(P, dtype=np.float64) for P in Gp]
    # every input complexified: value + i eps direction
    ac, hc, X0c = controls + 1j * EPS * va, h + 1j * EPS * vh, X0 + 1j * EPS * V0
    out = dict(tgrad_samples=np.zeros((len(samples), T - 1, m + (1 if free else 0))), tgrad_init=np.zeros((len(samples), X0.size)))
    gs = np.zeros((T - 1, m + (1 if free else 0)), dtype=complex)
    for q, s in enumerate(samples):
        th, sc = theta[s] + 1j * EPS * vth[s], scale[s] + 1j * EPS * vsc[s]
        C = (cot[s] + 1j * EPS * vcot[s]).reshape(n, -1, order="F")
        dot = lambda dX: np.sum(C * dX)
        # sweep_vjp_reference.pullback_forward from here on, in complex arithmetic
        Gs = []
        for t in range(T - 1):
            G = G0.astype(complex)
            for j in range(p):
                G = G + th[j] * Pj[j]
            for k in range(m):
                G = G + (sc[k] * ac[k, t]) * Gk[k]
            Gs.append(G)
        Es = [sla.expm(hc[t] * Gs[t]) for t in range(T - 1)]
        X = [X0c]
        for t in range(T - 1):
            X.append(Es[t] @ X[t])
        B = np.eye(n, dtype=complex)                         # E_{T-2} ... E_{t+1}
        for t in range(T - 2, -1, -1):
            for k in range(m):
                gs[t, k] = dot(B @ (sla.expm_frechet(hc[t] * Gs[t], (hc[t] * sc[k]) * Gk[k], compute_expm=False) @ X[t]))
            if free:
                gs[t, m] = dot(B @ (Gs[t] @ X[t + 1]))
            B = B @ Es[t]
        out["tgrad_samples"][q] = gs.imag / EPS
        out["tgrad_init"][q] = ((B.T @ C).imag / EPS).reshape(-1, order="F")          # B = W now
    return out


def pullback_loss_terms(X, G):
    """The loss l(X) = mean_s ( 1/2 ||X_s - G||^2 + 1/4 ||X_s||^4 ) of the `hessian_times` test, in closed form: its gradient (S x ns)
    and the map Xdot -> d2 l(X) Xdot."""
    S = X.shape[0]
    r2 = np.sum(X * X, axis=1, keepdims=True)
    grad = ((X - G) + r2 * X) / S
    hess_times = lambda Xd: (Xd + r2 * Xd + 2.0 * np.sum(X * Xd, axis=1, keepdims=True) * X) / S
    return grad, hess_times
