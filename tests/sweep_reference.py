"""Reference for the rollout sweeps (`qc_sweep_*`): a scipy chain in the iso form the kernels use, the pattern of
tests/test_rollout.py::_expm_chain, and the fidelities from the definitions in include/qcolloc.h.  Nothing here calls the library.

    G_s(a)  = G_drift + sum_j theta[s, j] P_j + sum_k c[s, k] a_k G_k
    x_{t+1} = expm(dt_t G_s(a_t)) x_t,   t = 0 .. T-2

`sweep_finals_eigh` is the independent route for Hermitian systems (complex arithmetic, eigendecompositions) that checks the
chain itself."""
import numpy as np
import scipy.linalg as sla


def iso_generator(H):
    """iso(-iH) = [[Im H, Re H], [-Re H, Im H]]"""
    H = np.asarray(H, dtype=complex)
    return np.block([[H.imag, H.real], [-H.real, H.imag]])


def operator_to_iso_vec(U):
    U = np.asarray(U, dtype=complex)
    return np.concatenate([U.real, U.imag], axis=0).reshape(-1, order="F")


def iso_vec_to_operator(v, N):
    M = np.asarray(v).reshape(2 * N, -1, order="F")
    return M[:N] + 1j * M[N:]


def sample_generator(G0, Gd, Gp, a, theta_s, c_s):
    G = np.array(G0, dtype=np.float64)
    for j, P in enumerate(Gp):
        G = G + theta_s[j] * P
    for k, Gk in enumerate(Gd):
        G = G + (c_s[k] * a[k]) * Gk
    return G


def _n_samples(theta, scale):
    """S from theta (S x p; S x 0 without perturbations) or, failing that, from scale (S x m)."""
    if theta is not None and np.ndim(theta) >= 1:
        return np.shape(theta)[0]
    return np.shape(scale)[0]


def sweep_finals(G0, Gd, Gp, controls, dts, init, theta, scale=None):
    """Final states, (n cols) x S.  controls m x T, dts T (or a scalar), init of n cols entries (column-major), theta S x p,
    scale S x m or None."""
    G0 = np.asarray(G0, dtype=np.float64)
    n = G0.shape[0]
    controls = np.asarray(controls, dtype=np.float64).reshape(len(Gd), -1)
    T = controls.shape[1]
    dts = np.full(T, float(dts)) if np.ndim(dts) == 0 else np.asarray(dts, dtype=np.float64).ravel()
    S = _n_samples(theta, scale)
    theta = np.asarray(theta, dtype=np.float64).reshape(S, len(Gp)) if len(Gp) else None
    scale = np.ones((S, len(Gd))) if scale is None else np.asarray(scale, dtype=np.float64).reshape(S, len(Gd))
    X0 = np.asarray(init, dtype=np.float64).reshape(n, -1, order="F")
    out = np.empty((X0.size, S))
    for s in range(S):
        X = X0.copy()
        th = theta[s] if theta is not None else ()
        for t in range(T - 1):
            X = sla.expm(dts[t] * sample_generator(G0, Gd, Gp, controls[:, t], th, scale[s])) @ X
        out[:, s] = X.reshape(-1, order="F")
    return out


def sweep_finals_eigh(H0, Hd, Hp, controls, dts, init, theta, scale=None):
    """The same final states for Hermitian H0, H_k, P_j by U = V exp(-i dt w) V' in complex arithmetic."""
    H0 = np.asarray(H0, dtype=complex)
    N = H0.shape[0]
    controls = np.asarray(controls, dtype=np.float64).reshape(len(Hd), -1)
    T = controls.shape[1]
    dts = np.full(T, float(dts)) if np.ndim(dts) == 0 else np.asarray(dts, dtype=np.float64).ravel()
    S = _n_samples(theta, scale)
    theta = np.asarray(theta, dtype=np.float64).reshape(S, len(Hp)) if len(Hp) else None
    scale = np.ones((S, len(Hd))) if scale is None else np.asarray(scale, dtype=np.float64).reshape(S, len(Hd))
    X0 = iso_vec_to_operator(init, N)
    out = np.empty((2 * X0.size, S))
    for s in range(S):
        X = X0.copy()
        Hs = H0 + sum((theta[s, j] * np.asarray(P, dtype=complex) for j, P in enumerate(Hp)), np.zeros_like(H0))
        for t in range(T - 1):
            H = Hs + sum(((scale[s, k] * controls[k, t]) * np.asarray(Hk, dtype=complex) for k, Hk in enumerate(Hd)), np.zeros_like(H0))
            w, V = np.linalg.eigh(H)
            X = (V * np.exp(-1j * dts[t] * w)) @ (V.conj().T @ X)
        out[:, s] = operator_to_iso_vec(X)
    return out


def unitary_fidelity(x, goal_iso, N, subspace=None, form="abs"):
    """|tr(U_goal' U)| / n over the subspace block, or its square (QC_FID_FORM_ABS / QC_FID_FORM_ABS2)."""
    U, G = iso_vec_to_operator(x, N), iso_vec_to_operator(goal_iso, N)
    if subspace is not None:
        ix = np.ix_(list(subspace), list(subspace))
        U, G = U[ix], G[ix]
    t = abs(np.trace(G.conj().T @ U)) / U.shape[0]
    return t * t if form == "abs2" else t


def ket_fidelity(x, goal_iso):
    """|<psi_goal|psi>|^2"""
    N = len(goal_iso) // 2
    psi = np.asarray(x[:N]) + 1j * np.asarray(x[N:])
    g = np.asarray(goal_iso[:N]) + 1j * np.asarray(goal_iso[N:])
    return abs(np.vdot(g, psi)) ** 2


def density_fidelity(x, goal_iso):
    """psi_goal' rho psi_goal with rho~ = [vec(Re rho); vec(Im rho)] (column-major)"""
    L = len(goal_iso) // 2
    x = np.asarray(x)
    rho = x[:L * L].reshape(L, L, order="F") + 1j * x[L * L:].reshape(L, L, order="F")
    g = np.asarray(goal_iso[:L]) + 1j * np.asarray(goal_iso[L:])
    return float(np.real(np.vdot(g, rho @ g)))


def fidelities(finals, kind, goal_iso, N, subspace=None, form="abs"):
    if kind == "unitary":
        return np.array([unitary_fidelity(finals[:, s], goal_iso, N, subspace, form) for s in range(finals.shape[1])])
    if kind == "ket":
        return np.array([ket_fidelity(finals[:, s], goal_iso) for s in range(finals.shape[1])])
    return np.array([density_fidelity(finals[:, s], goal_iso) for s in range(finals.shape[1])])
