"""Reference for the sweep pushforwards (`qc_sweep_jvp*`): the tangent of the final states of tests/sweep_reference.py, and of their
fidelities, along one direction (vcontrols, vdts, vinit, vtheta, vscale).  Nothing here calls the library.

    d(hG)_t = vh_t G_s(a_t) + h_t ( sum_j vtheta[s, j] P_j + sum_k ( vscale[s, k] a_{t,k} + c[s, k] va_{t,k} ) G_k )
    xdot_0  = vinit,    xdot_{t+1} = E_t xdot_t + L(h_t G; d(hG)_t) x_t,    t = 0 .. T-2

Two routes that share only the chain:

  * `pushforward_frechet`: the recurrence as written, L from scipy.linalg.expm_frechet.
  * `pushforward_complex_step`: the complex step.  Generators, timesteps and the initial state are complexified, X + i eps Xdot with
    eps = 1e-30, the chain is scipy.linalg.expm of complex matrices, and the tangent is Im(x_final) / eps: no subtraction, so no
    cancellation, and an O(eps^2) truncation that is far below one ulp.

Both return a dict: finals and tfinals, len(samples) x (n cols), and tfids, len(samples) values (None without `fid`).
vcontrols is m x T (only knots 0 .. T-2 act), vdts T values or None (None: no timestep tangent; a fixed timestep has none), vinit
n cols values, vtheta S x p, vscale S x m; whichever is None is zero.  fid = (kind, goal_iso, levels, subspace, form)."""
import numpy as np
import scipy.linalg as sla

import sweep_grad_reference as gref
import sweep_reference as ref

EPS = 1e-30


def _unpack(G0, Gd, Gp, controls, dts, theta, scale, vcontrols, vdts, vinit, vtheta, vscale, init):
    G0 = np.asarray(G0, dtype=np.float64)
    n, m, p = G0.shape[0], len(Gd), len(Gp)
    controls = np.asarray(controls, dtype=np.float64)
    controls = controls.reshape(m, -1) if m else controls.reshape(0, controls.shape[-1])
    T = controls.shape[1]
    h = np.asarray(dts, dtype=np.float64).ravel() if np.ndim(dts) else np.full(T, float(dts))
    S = ref._n_samples(theta, scale)
    theta = np.asarray(theta, dtype=np.float64).reshape(S, p) if p else np.zeros((S, 0))
    scale = np.ones((S, m)) if scale is None else np.asarray(scale, dtype=np.float64).reshape(S, m)
    va = np.zeros((m, T)) if vcontrols is None else np.asarray(vcontrols, dtype=np.float64).reshape(m, T)
    vh = np.zeros(T) if vdts is None else np.asarray(vdts, dtype=np.float64).ravel()
    X0 = np.asarray(init, dtype=np.float64).reshape(n, -1, order="F")
    V0 = np.zeros_like(X0) if vinit is None else np.asarray(vinit, dtype=np.float64).reshape(n, -1, order="F")
    vth = np.zeros((S, p)) if vtheta is None else np.asarray(vtheta, dtype=np.float64).reshape(S, p)
    vsc = np.zeros((S, m)) if vscale is None else np.asarray(vscale, dtype=np.float64).reshape(S, m)
    return G0, n, m, p, controls, T, h, theta, scale, va, vh, X0, V0, vth, vsc


def fidelity_tangent(x, dx, fid):
    """<dF/dx(x), dx> from the definitions of sweep_reference: the density fidelity is linear in x."""
    kind, goal, L, subspace, form = fid
    if kind == "density":
        return ref.density_fidelity(dx, goal)
    return gref.fidelity_differential(x, dx, kind, goal, L, subspace, form)


def _generator_tangent(Gd, Gp, a, va, c_s, vth_s, vc_s, n):
    D = np.zeros((n, n))
    for j, P in enumerate(Gp):
        D = D + vth_s[j] * np.asarray(P, dtype=np.float64)
    for k, Gk in enumerate(Gd):
        D = D + (vc_s[k] * a[k] + c_s[k] * va[k]) * np.asarray(Gk, dtype=np.float64)
    return D


def _pack(finals, tfinals, fid):
    tfids = None if fid is None else np.array([fidelity_tangent(x, dx, fid) for x, dx in zip(finals, tfinals)])
    return dict(finals=np.array(finals), tfinals=np.array(tfinals), tfids=tfids)


def pushforward_frechet(G0, Gd, Gp, controls, dts, init, theta, scale, samples, vcontrols=None, vdts=None, vinit=None, vtheta=None, vscale=None,
                        fid=None):
    G0, n, m, p, controls, T, h, theta, scale, va, vh, X0, V0, vth, vsc = _unpack(G0, Gd, Gp, controls, dts, theta, scale, vcontrols, vdts, vinit,
                                                                                    vtheta, vscale, init)
    finals, tfinals = [], []
    for s in samples:
        X, V = X0.copy(), V0.copy()
        for t in range(T - 1):
            G = ref.sample_generator(G0, Gd, Gp, controls[:, t], theta[s], scale[s])
            D = vh[t] * G + h[t] * _generator_tangent(Gd, Gp, controls[:, t], va[:, t], scale[s], vth[s], vsc[s], n)
            E, Lt = sla.expm_frechet(h[t] * G, D)
            V = E @ V + Lt @ X
            X = E @ X
        finals.append(X.reshape(-1, order="F"))
        tfinals.append(V.reshape(-1, order="F"))
    return _pack(finals, tfinals, fid)


def pushforward_complex_step(G0, Gd, Gp, controls, dts, init, theta, scale, samples, vcontrols=None, vdts=None, vinit=None, vtheta=None,
                             vscale=None, fid=None):
    G0, n, m, p, controls, T, h, theta, scale, va, vh, X0, V0, vth, vsc = _unpack(G0, Gd, Gp, controls, dts, theta, scale, vcontrols, vdts, vinit,
                                                                                    vtheta, vscale, init)
    finals, tfinals = [], []
    for s in samples:
        X = X0 + 1j * EPS * V0
        for t in range(T - 1):
            G = ref.sample_generator(G0, Gd, Gp, controls[:, t], theta[s], scale[s])
            Gc = G + 1j * EPS * _generator_tangent(Gd, Gp, controls[:, t], va[:, t], scale[s], vth[s], vsc[s], n)
            X = sla.expm((h[t] + 1j * EPS * vh[t]) * Gc) @ X
        finals.append(X.real.reshape(-1, order="F"))
        tfinals.append((X.imag / EPS).reshape(-1, order="F"))
    return _pack(finals, tfinals, fid)
