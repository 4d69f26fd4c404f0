"""Reference for the open-system sweep gradients (stored-state walk, `qc_sweep_desc.reserved1[0] = QC_SWEEP_STORED_STATES`).  Nothing here
calls the library.  The generators are restated (Lindblad superoperators of vec(rho), column-major, in the real isomorphism; iso
generators of non-Hermitian effective Hamiltonians); the derivatives come from the forward-mode routes that hold for ANY generator,
scipy.linalg.expm_frechet per interval:

  * unitary / ket fidelities: sweep_grad_reference.grad_samples_forward and sweep_param_grad_reference.param_terms_forward;
  * the density-operator fidelity F = psi' rho psi is LINEAR in the state, F = <c, x> with the constant vector `density_cotangent`, so
    its derivatives are sweep_vjp_reference.pullback_forward with cot[s] = c (the same expm_frechet route; the fidelity differential of
    sweep_grad_reference is written for the |t|^2 forms only).
Central differences (`forward_vs_fd`) are the self-check of both."""
import numpy as np

import sweep_grad_reference as gref
import sweep_param_grad_reference as pref
import sweep_reference as ref
import sweep_vjp_reference as vref


def iso_operator(L):
    """The real form of a complex linear map on [Re v; Im v]."""
    L = np.asarray(L, dtype=complex)
    return np.block([[L.real, -L.imag], [L.imag, L.real]])


def lindblad_generator(H, Ls=()):
    """d vec(rho)/dt = [-i (I x H - H^T x I) + sum_L (conj(L) x L - 1/2 (I x L'L + (L'L)^T x I))] vec(rho), real form, 2 levels^2 square."""
    H = np.asarray(H, dtype=complex)
    I = np.eye(H.shape[0])
    S = -1j * (np.kron(I, H) - np.kron(H.T, I))
    for L in Ls:
        L = np.asarray(L, dtype=complex)
        LdL = L.conj().T @ L
        S = S + np.kron(L.conj(), L) - 0.5 * (np.kron(I, LdL) + np.kron(LdL.T, I))
    return iso_operator(S)


def density_iso(rho):
    rho = np.asarray(rho, dtype=complex)
    return np.concatenate([rho.real.reshape(-1, order="F"), rho.imag.reshape(-1, order="F")])


def density_cotangent(goal_ket_iso):
    """c with psi' rho psi = <c, [vec(Re rho); vec(Im rho)]>: Re rho_ab enters with Re(conj(g_a) g_b), Im rho_ab with -Im(conj(g_a) g_b)."""
    L = len(goal_ket_iso) // 2
    g = np.asarray(goal_ket_iso[:L]) + 1j * np.asarray(goal_ket_iso[L:])
    M = np.outer(g.conj(), g)
    return np.concatenate([M.real.reshape(-1, order="F"), -M.imag.reshape(-1, order="F")])


def _args(c):
    return c["G0"], c["Gd"], c["Gp"], c["controls"], c["dts"], c["init"], c["theta"], c["scale"]


def fidelities(c):
    return ref.fidelities(ref.sweep_finals(*_args(c)), c["kind"], c["goal"], c["L"], c.get("subspace"), c.get("form", "abs"))


def grad_forward(c, samples=None, params=True):
    """dict(grad_samples len(samples) x (T-1) x nd[, grad_theta len(samples) x p, grad_scale len(samples) x m]) of the case's fidelity."""
    samples = list(c["samples"] if samples is None else samples)
    if c["kind"] == "density":
        S = ref._n_samples(c["theta"], c["scale"])
        cot = np.tile(density_cotangent(c["goal"]), (S, 1))
        out = vref.pullback_forward(*_args(c), samples, cot)
        return dict(grad_samples=out["grad_samples"], grad_theta=out["grad_theta"], grad_scale=out["grad_scale"])
    fid = (c["kind"], c["goal"], c["L"], c.get("subspace"), c.get("form", "abs"))
    out = dict(grad_samples=gref.grad_samples_forward(*_args(c), samples, *fid))
    if params:
        sums = pref.param_terms_forward(*_args(c), samples, *fid)[1]
        out["grad_theta"], out["grad_scale"] = sums[:, :len(c["Gp"])], sums[:, len(c["Gp"]):]
    return out


def forward_vs_fd(c, samples, step=1e-5):
    """(relative difference of the two routes over grad_samples, grad_theta, grad_scale; the largest derivative)."""
    fid = (c["kind"], c["goal"], c["L"], c.get("subspace"), c.get("form", "abs"))
    a = grad_forward(c, samples)
    b = gref.grad_samples_fd(*_args(c), samples, *fid, step=step)
    bp = pref.param_grad_fd(*_args(c), samples, *fid, step=step)
    p = len(c["Gp"])
    big = max(1.0, np.abs(a["grad_samples"]).max())
    err = max(np.abs(a["grad_samples"] - b).max(), np.abs(a["grad_theta"] - bp[:, :p]).max(initial=0.0),
              np.abs(a["grad_scale"] - bp[:, p:]).max(initial=0.0)) / big
    return err, np.abs(a["grad_samples"]).max()
