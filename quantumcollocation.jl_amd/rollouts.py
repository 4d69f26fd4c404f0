"""Rollouts on the GPU through `qc_rollout`:

    unitary_rollout(Ũ⃗_init, controls, Δt, system)          trajectory_initialization.jl:426
    rollout(ψ̃_init, controls, Δt, system)                   trajectory_initialization.jl:493
    open_rollout(ρ⃗̃_init, controls, Δt, system)             trajectory_initialization.jl:547
    unitary_rollout_fidelity(traj, system; subspace)        unitary_smooth_pulse_problem.jl:218

x_{t+1} = exp(Δt_t G(a_t)) x_t; the result has one column per knot.  The functions taking raw controls build a
minimal trajectory layout [state, a, Δt] for the descriptor; `QuantumDynamics.rollout` reuses an existing handle.

Sweeps through `qc_sweep_*`: one trajectory of controls, S perturbed systems, S final states and fidelities in one call --
the loop of the reference's robustness check, `unitary_rollout(traj.a, timesteps, systems(ζ))[:, end]` and
`iso_vec_unitary_fidelity` for every ζ of a grid (unitary_sampling_problem.jl:204-244):

    rollout_sweep(init, controls, Δt, system, perturbations, θ, scale)     (finals, fids)
    unitary_rollout_fidelity_sweep(traj, system, perturbations, θ)         S fidelities of the rolled-out unitary
    rollout_fidelity_sweep(traj, system, perturbations, θ; state_name)     ... of a ket
    rollout_sweep_parameter_gradient(init, controls, Δt, system, perturbations, θ, scale)   (fids, dF/dθ, dF/dscale)
    RolloutSweep                                                            the handle, for callers that sweep repeatedly
    RolloutSweep.vjp / .vjp_device / .finals_autograd                       the pullback of the final states (`qc_sweep_vjp*`): any loss of
                                                                            them, in torch, differentiated by one adjoint sweep
    RolloutSweep.jvp / .jvp_device                                          the pushforward (`qc_sweep_jvp*`): tangents of the final states and
                                                                            fidelities along one direction, open systems included
    RolloutSweep.hvp / .hvp_device                                          the tangent of the pullback (`qc_sweep_hvp*`): exact Hessian products of
                                                                            any loss of the final states
    rollout_noise_sweep(init, controls, Δt, system, perturbations, ξ, θ)   (finals, fids) under per-interval perturbations ξ[s, t, j]
    RolloutSweep.noise_eval / .noise_grad (+ _device)                       noise trajectories (`qc_sweep_noise_*`): the sweep and its gradient with
                                                                            θ[s, j] + ξ[s, t, j] in interval t, and dF_s/dξ[s, t, j] of every sample
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from .isomorphisms import operator_to_iso_vec
from .named_trajectory import NamedTrajectory
from .objectives import iso_vec_unitary_fidelity


def _rollout(init: np.ndarray, controls: np.ndarray, dts, system, cols: int, device: int = 0) -> np.ndarray:
    controls = np.asarray(controls, dtype=np.float64)
    if controls.ndim != 2 or controls.shape[0] != system.n_drives:
        raise ValueError("controls must be n_drives x T")
    m, T = controls.shape
    dts = np.full(T, float(dts)) if np.ndim(dts) == 0 else np.asarray(dts, dtype=np.float64).ravel()
    if dts.size != T:
        raise ValueError("one timestep per knot expected")
    init = np.ascontiguousarray(init, dtype=np.float64).ravel()
    n = 2 * system.state_levels
    if init.size != n * cols:
        raise ValueError(f"initial state has length {init.size}, expected {n * cols}")
    if T < 2:
        return init[:, None].copy()
    s = init.size
    d = _lib.qc_desc()
    d.N, d.m, d.T, d.zdim, d.global_dim = system.state_levels, m, T, s + m + 1, 0
    d.off_U, d.off_a, d.off_dt, d.dt_fixed = 0, s, s + m, 0.0
    d.integrator, d.pade_order, d.n_deriv = _lib.QC_EXPONENTIAL, 0, 0
    d.state_cols = 0 if cols == system.state_levels else cols
    G0 = np.asfortranarray(system.G_drift, dtype=np.float64)
    Gd = np.ascontiguousarray(np.stack([np.asarray(G, dtype=np.float64).reshape(-1, order="F") for G in system.G_drives])
                              if m else np.zeros((1, n * n)))
    d.G_drift, d.G_drives = _lib.dptr(G0), _lib.dptr(Gd)
    d.device, d.kernel = device, _lib.QC_KERNEL_LDS
    h = C.c_void_p()
    _lib.check(_lib.lib.qc_create(C.byref(d), C.byref(h)))
    try:
        Z = np.zeros((T, s + m + 1))
        Z[:, s:s + m] = controls.T
        Z[:, s + m] = dts
        out = np.empty((T, s))
        _lib.check(_lib.lib.qc_rollout(h, _lib.dptr(Z), _lib.dptr(init), _lib.dptr(out)), h)
    finally:
        _lib.lib.qc_destroy(h)
    return np.ascontiguousarray(out.T)


def unitary_rollout(U_iso_init: np.ndarray, controls: np.ndarray, dts, system, device: int = 0) -> np.ndarray:
    """Ũ⃗ trajectory (2N^2 x T)."""
    return _rollout(U_iso_init, controls, dts, system, system.levels, device)


def rollout(psi_iso_init: np.ndarray, controls: np.ndarray, dts, system, device: int = 0) -> np.ndarray:
    """ψ̃ trajectory (2N x T) of one ket."""
    return _rollout(psi_iso_init, controls, dts, system, 1, device)


def open_rollout(rho_iso_init: np.ndarray, controls: np.ndarray, dts, system, device: int = 0) -> np.ndarray:
    """ρ⃗̃ trajectory (2N^2 x T) under the Lindblad generators of an `OpenQuantumSystem`."""
    return _rollout(rho_iso_init, controls, dts, system, 1, device)


def unitary_rollout_fidelity(traj: NamedTrajectory, system, state_name: str = "Ũ⃗", control_name: str = "a",
                             subspace: Optional[Sequence[int]] = None, device: int = 0) -> float:
    """Fidelity of the rolled-out final unitary with `traj.goal[state_name]`."""
    init = traj.initial.get(state_name) if getattr(traj, "initial", None) else None
    if init is None:
        init = operator_to_iso_vec(np.eye(system.levels, dtype=complex))
    dts = traj[traj.timestep].ravel() if isinstance(traj.timestep, str) else float(traj.timestep)
    U = unitary_rollout(np.asarray(init, dtype=np.float64), traj[control_name], dts, system, device)
    return iso_vec_unitary_fidelity(U[:, -1], np.asarray(traj.goal[state_name], dtype=np.float64), subspace, device)


def rollout_fidelity(traj: NamedTrajectory, system, state_name: str = "ψ̃", control_name: str = "a", device: int = 0) -> float:
    """`rollout_fidelity(traj, system; state_name)` for a ket component (reference quantum_state_smooth_pulse_problem.jl:247-249,
    quantum_state_sampling_problem.jl:187-189): the ket rolled out from its first knot under the trajectory's controls, |<goal|psi_T>|^2
    with `traj.goal[state_name]`."""
    from .objectives import iso_fidelity
    init = traj.initial.get(state_name) if getattr(traj, "initial", None) else None
    if init is None:
        init = traj[state_name][:, 0]
    dts = traj[traj.timestep].ravel() if isinstance(traj.timestep, str) else float(traj.timestep)
    psi = rollout(np.ascontiguousarray(init, dtype=np.float64), traj[control_name], dts, system, device)
    return iso_fidelity(psi[:, -1], np.asarray(traj.goal[state_name], dtype=np.float64), device)


# ---------------------------------------------------------------------------------------------------------------
#  Rollout sweeps over perturbed systems through `qc_sweep_*`
# ---------------------------------------------------------------------------------------------------------------
_ERR = "qc_sweep_last_error"      # what `_lib.check_rc` asks for the message of a failed `qc_sweep_*` call
_FID_KINDS = {None: _lib.QC_SWEEP_FID_NONE, "none": _lib.QC_SWEEP_FID_NONE, "unitary": _lib.QC_FID_UNITARY, "ket": _lib.QC_FID_KET,
              "density": _lib.QC_FID_DENSITY}


def _sweep_generators(system, perturbations) -> list:
    """Perturbation generators (2N x 2N): Hermitian operators of a `QuantumSystem` go through `iso_generator`, as its
    Hamiltonians do; an `OpenQuantumSystem` takes generator matrices as they are."""
    from .isomorphisms import iso_generator
    from .quantum_systems import OpenQuantumSystem
    n = 2 * system.state_levels
    out = []
    for P in perturbations:
        P = np.asarray(P)
        G = np.asarray(P, dtype=np.float64) if isinstance(system, OpenQuantumSystem) else iso_generator(np.asarray(P, dtype=complex))
        if G.shape != (n, n):
            raise ValueError(f"perturbation has generator shape {G.shape}, expected ({n}, {n})")
        out.append(G)
    return out


def _sweep_samples(p: int, m: int, theta, scale):
    """(S, theta S x p or None, scale S x m or None) from what the caller passed."""
    theta = None if theta is None else np.asarray(theta, dtype=np.float64)
    if theta is not None and theta.ndim == 1:
        theta = theta.reshape(-1, 1) if p == 1 else theta.reshape(-1, p)
    scale = None if scale is None else np.asarray(scale, dtype=np.float64)
    if scale is not None and scale.ndim == 1:
        scale = scale.reshape(-1, 1) if m == 1 else scale.reshape(-1, m)
    if theta is None and scale is None:
        raise ValueError("theta (S x n_pert) or scale (S x m) must give the number of samples")
    S = theta.shape[0] if theta is not None else scale.shape[0]
    if theta is not None and theta.shape != (S, p):
        raise ValueError(f"theta must be S x {p}")
    if p and theta is None:
        raise ValueError("theta is required: the handle has perturbations")
    if scale is not None and scale.shape != (S, m):
        raise ValueError(f"scale must be {S} x {m}")
    if S < 1:
        raise ValueError("at least one sample")
    return S, (np.ascontiguousarray(theta) if p else None), (np.ascontiguousarray(scale) if scale is not None and m else None)


def _host_ptr(a, given: bool = False):
    """double* of an optional host array: null when it is None or empty -- or, with `given` (the directions vZ, vinit, vtheta, vscale,
    vcot, which the library counts as given even when empty), only when it is None."""
    return _lib.dptr(a) if (a is not None and (given or a.size)) else None


def _dev_ptr(t, use=True):
    """Device pointer of an optional tensor: null when it is None or has no elements, or when the handle has no `use` for it."""
    return t.data_ptr() if (t is not None and use and t.numel()) else None


def _stream_of(stream):
    return stream.cuda_stream if stream is not None else torch.cuda.current_stream().cuda_stream


def _refuse_all_none(what: str, *tensors):
    for t in tensors:
        if t is not None:
            return
    raise ValueError(f"every {what} is None")


def _device_counts(sw) -> dict:
    """Entries of every named tensor of the device entries as (per sample, shared by the samples): a call with S samples expects
    per sample * S + shared of them."""
    shared = lambda cnt: (0, cnt)
    Z, state, states, one = shared(sw.Z_len), shared(sw.ns), (sw.ns, 0), (1, 0)
    theta, scale, derivs, noise = (sw.p, 0), (sw.m, 0), ((sw.T - 1) * sw.n_deriv, 0), ((sw.T - 1) * sw.p, 0)
    return {"dZ": Z, "dinit": state, "dtheta": theta, "dscale": scale, "dweights": one, "dcot": states,
            "dvZ": Z, "dvinit": state, "dvtheta": theta, "dvscale": scale, "dvcot": states, "dnoise": noise,
            "dfinals": states, "dfids": one, "dJ": shared(1), "dgrad": Z, "dgrad_samples": derivs, "dgrad_init": states,
            "dgrad_theta": theta, "dgrad_scale": scale, "dgrad_noise": noise,
            "dtfinals": states, "dtfids": one, "dtgrad": Z, "dtgrad_samples": derivs, "dtgrad_init": states}


class RolloutSweep:
    """S rollouts of one trajectory of controls under S perturbed systems, final states and fidelities only:

        G_s(a) = G_drift + sum_j theta[s, j] P_j + sum_k scale[s, k] a_k G_k,     x_{t+1} = exp(dt_t G_s(a_t)) x_t

    system         `QuantumSystem` or `OpenQuantumSystem`
    perturbations  Hermitian operators (QuantumSystem) or generator matrices (OpenQuantumSystem), at most 8
    T              knots
    cols           columns of the state: system.levels for a unitary, K for K kets, 1 for a density operator (default: unitary)
    goal, fid_kind fidelity of every final state: "unitary" (goal = iso-vec of U_goal; `subspace`, `fid_form`), "ket" or
                   "density" (goal = [Re psi; Im psi]); None: final states only
    The trajectory vector is knot-major with the controls at `off_a` and the timestep at `off_dt` of every knot of `zdim`
    entries (default: the minimal layout [a, dt], built by `pack`; dt_fixed: no timestep in the knot).
    wide           True: systems of 16 < 2N <= 32 with up to 8 drives run on the matrix cores too ("mfma32-sweep", with gradients over the
                   controls and timesteps) instead of one rollout per sample.  Nothing changes at 2N <= 16.
    wide_params    True (only with `wide`): an "mfma32-sweep" handle also serves `param_grad`, the `params` of `vjp` and the theta /
                   scale gradients of `finals_autograd`.  Without it those refuse there, as they always did; nothing else changes.
    stored_states  True: `grad`, `grad_params` and `vjp` keep the forward states of every sample on the device (S x (T-1) x 2N x cols
                   doubles) and read them on the way back instead of reversing the step.  That serves ANY generators in the
                   "mfma16-sweep" form: an `OpenQuantumSystem` with the "density" fidelity, a non-Hermitian effective Hamiltonian.
                   Closed systems give the same derivatives either way (to rounding); `hvp` and `noise_grad` keep their scope.
    wide_stored    True (only with `wide` and `stored_states`): an "mfma32-sweep" handle serves the stored-state walk too -- two qubits
                   with T1 / T2 (levels^2 = 16), a three-level transmon with relaxation, 9 .. 16 levels with a non-Hermitian
                   Hamiltonian.  The device buffer is S x (T-1) x 2N x cols doubles: 32 a knot for a two-qubit density operator
                   (250 MiB at S = 1024, T = 1000), 512 a knot for a 16-level unitary (4 GiB).  Parameter outputs there also need
                   `wide_params`.  Without it such handles refuse reverse mode, as they always did; nothing else changes.
    wide_tangent   True (only with `wide`): an "mfma32-sweep" handle serves `jvp`, `jvp_device` and the forward-mode rule of
                   `finals_autograd` -- any generators, open systems included, with no state buffer (nothing is reversed): about three
                   forward sweeps by the instruction count.  Without it those refuse there, as they always did; nothing else changes
                   (`hvp` in that form is `wide_hessian`'s to serve).
    wide_noise     True (only with `wide`): an "mfma32-sweep" handle serves `noise_eval`, `noise_grad` and their device forms with at
                   least one perturbation -- up to 8 drives and 8 perturbations, no tile limit (that form keeps no generator resident).
                   Without it those refuse there, as they always did; nothing else changes, and nothing changes at 2N <= 16.
    wide_hessian   True (only with `wide`): an "mfma32-sweep" handle of a closed system (antisymmetric generators, at most 16 state
                   columns) serves `hvp` and `hvp_device`: one tangent forward walk and one backward walk on 2 x 2 tiles, about 3.4
                   pullbacks by the instruction count.  It does not need `wide_tangent`.  Without it those refuse there, as they
                   always did; nothing else changes, and nothing changes at 2N <= 16, where `hvp` needs no flag.
    wide64         True (only with `wide`): systems of 32 < 2N <= 64 with up to 16 drives -- 5 qubits, three coupled three-level
                   transmons, a five-level Lindblad model -- run on the matrix cores as well ("mfma64-sweep": one workgroup per
                   (sample, chunk of intervals), the matrices in LDS) instead of one rollout per sample.  That form serves `eval` and
                   `eval_device` only: `grad`, `param_grad`, `vjp`, `jvp`, `hvp` and the noise sweeps refuse there, naming the form
                   (`wide64_grad` adds `grad` and `vjp`, `wide64_params` their parameter outputs, `wide64_tangent` `jvp`,
                   `wide64_noise` the noise sweeps).
                   Nothing changes at 2N <= 32, and nothing changes without it.
    wide64_grad    True (only with `wide64`): an "mfma64-sweep" handle of a closed system (antisymmetric generators, at most 32 state
                   columns: a full unitary of 32 levels fits) also serves `grad`, `vjp`, their device forms and the backward rule of
                   `finals_autograd`, by the closed adjoint walk on 4 x 4 tiles.  `param_grad`, the `params` of `vjp`, `stored_states`,
                   `hvp` and the noise sweeps still refuse there, naming the form; `jvp` is `wide64_tangent`'s to serve, the noise
                   sweeps `wide64_noise`'s.  Nothing
                   else changes, nothing changes at 2N <= 32, and nothing changes without it.
    wide64_params  True (only with `wide64_grad`): such a handle also serves `param_grad`, `param_grad_device`, the `params` of `vjp` and
                   the theta / scale cotangents of `finals_autograd`, by the parameter flavour of the same walk: one call gives
                   dF_s/dtheta and dF_s/dscale of every sample (dF_s/dscale is taken before the factor scale, so it is defined at
                   scale = 0).  `stored_states`, `hvp` and the noise sweeps still refuse there (`jvp` is `wide64_tangent`'s to
                   serve, the noise sweeps `wide64_noise`'s).  Without it `param_grad` and the `params` of `vjp` refuse there, as they did; nothing else changes, and
                   nothing changes at 2N <= 32.
    wide64_tangent True (only with `wide64`; it needs neither `wide64_grad` nor `wide64_params`): an "mfma64-sweep" handle also serves
                   `jvp`, `jvp_device` and the forward-mode rule of `finals_autograd` -- any generators, open systems included (a
                   five-level Lindblad model: 2N = 50), any fidelity, states of 2N x cols <= 2048 entries (every full unitary of the
                   form) -- by the paired exponential on 4 x 4 tiles: three forward sweeps by the instruction count.  Above that size
                   `jvp` refuses, naming the form, 2N and the size.  `hvp`, the noise sweeps (`wide64_noise`'s to serve) and
                   `stored_states` still refuse there.
                   Without it `jvp` refuses there, as it did; nothing else changes, and nothing changes at 2N <= 32.
    wide64_noise   True (only with `wide64`; it needs none of `wide64_grad`, `wide64_params`, `wide64_tangent`): an "mfma64-sweep"
                   handle also serves `noise_eval` and `noise_eval_device` with at least one perturbation -- up to 16 drives and 8
                   perturbations, any generators, open systems included, any fidelity or none.  `noise_grad` and its device form
                   also need `wide64_grad` and its scope (a closed system, at most 32 state columns, a unitary or ket fidelity);
                   without it they refuse with the gradient's reason.  At zero noise the outputs carry the bits of `eval` / `grad`
                   on the same handle.  `hvp` and `stored_states` still refuse there.  Without it the noise sweeps refuse there,
                   as they did; nothing else changes, and nothing changes at 2N <= 32.
    wide64_stored  True (only with `wide64_grad` and `stored_states`): an "mfma64-sweep" handle serves the stored-state walk too, on
                   4 x 4 tiles -- ANY generators with at most 32 state columns: a five-level Lindblad model with the "density"
                   fidelity (N = 25, 2N = 50), 17 .. 32 levels with a non-Hermitian Hamiltonian.  `grad`, `vjp`, their device forms
                   and the backward rule of `finals_autograd` take that walk whatever the generators; `param_grad` and the `params`
                   of `vjp` there also need `wide64_params`.  The device buffer is S x (T-1) x 2N x cols doubles: 50 a knot for the
                   five-level density operator, 432 for eight columns at 27 levels.  `hvp` (not served in this form), `noise_grad`
                   of open systems and more than 32 state columns still refuse.  Without it `stored_states` refuses there, as it
                   did; nothing else changes, and nothing changes at 2N <= 32."""

    def __init__(self, system, perturbations, T: int, cols: Optional[int] = None, goal=None, fid_kind=None, subspace=None,
                 fid_form: int = _lib.QC_FID_FORM_ABS, zdim: Optional[int] = None, off_a: int = 0, off_dt: Optional[int] = None,
                 dt_fixed: Optional[float] = None, global_dim: int = 0, device: int = 0, wide: bool = False,
                 stored_states: bool = False, wide_params: bool = False, wide_stored: bool = False, wide_tangent: bool = False,
                 wide_noise: bool = False, wide_hessian: bool = False, wide64: bool = False, wide64_noise: bool = False,
                 wide64_stored: bool = False, wide64_grad: bool = False, wide64_tangent: bool = False, wide64_params: bool = False):
        self._h = None
        flags = (   # (keyword, given, its bit of qc_sweep_desc.wide, what it needs, the refusal without that)
            ("wide64_stored", wide64_stored, _lib.QC_SWEEP_WIDE_64_STORED, wide64_grad and stored_states,
             "wide64_stored=True needs wide64_grad=True and stored_states=True"),
            ("wide64_params", wide64_params, _lib.QC_SWEEP_WIDE_64_PARAMS, wide64_grad, "wide64_params=True needs wide64_grad=True"),
            ("wide64_grad", wide64_grad, _lib.QC_SWEEP_WIDE_64_GRAD, wide64, "wide64_grad=True needs wide64=True"),
            ("wide64_tangent", wide64_tangent, _lib.QC_SWEEP_WIDE_64_TANGENT, wide64, "wide64_tangent=True needs wide64=True"),
            ("wide64_noise", wide64_noise, _lib.QC_SWEEP_WIDE_64_NOISE, wide64, "wide64_noise=True needs wide64=True"),
            ("wide64", wide64, _lib.QC_SWEEP_WIDE_64, wide, "wide64=True needs wide=True"),
            ("wide_hessian", wide_hessian, _lib.QC_SWEEP_WIDE_HESSIAN, wide, "wide_hessian=True needs wide=True"),
            ("wide_noise", wide_noise, _lib.QC_SWEEP_WIDE_NOISE, wide, "wide_noise=True needs wide=True"),
            ("wide_params", wide_params, _lib.QC_SWEEP_WIDE_PARAMS, wide, "wide_params=True needs wide=True"),
            ("wide_tangent", wide_tangent, _lib.QC_SWEEP_WIDE_TANGENT, wide, "wide_tangent=True needs wide=True"),
            ("wide_stored", wide_stored, _lib.QC_SWEEP_WIDE_STORED, wide and stored_states,
             "wide_stored=True needs wide=True and stored_states=True"),
            ("wide", wide, _lib.QC_SWEEP_WIDE, True, None))
        wide_bits = 0
        for keyword, given, bit, needs, refusal in flags:
            if given and not needs:
                raise ValueError(refusal)
            setattr(self, keyword, bool(given))
            wide_bits |= bit if given else 0
        m = system.n_drives
        N = system.state_levels
        n = 2 * N
        gens = _sweep_generators(system, perturbations)
        if zdim is None:
            zdim, off_a, off_dt = (max(m, 1), 0, -1) if dt_fixed is not None else (m + 1, 0, m)
        elif off_dt is None:
            off_dt = -1
        self.N, self.n, self.m, self.T, self.p = N, n, m, int(T), len(gens)
        self.cols = system.levels if cols is None else int(cols)
        self.ns = n * self.cols
        self.zdim, self.off_a, self.off_dt, self.global_dim = int(zdim), int(off_a), int(off_dt), int(global_dim)
        self.Z_len = self.T * self.zdim + self.global_dim
        self.fid_kind = _FID_KINDS[fid_kind] if (fid_kind is None or isinstance(fid_kind, str)) else int(fid_kind)
        flat = lambda Gs: np.ascontiguousarray(np.stack([np.asarray(G, dtype=np.float64).reshape(-1, order="F") for G in Gs]))
        self._G0 = np.ascontiguousarray(np.asarray(system.G_drift, dtype=np.float64).reshape(-1, order="F"))
        self._Gd = flat(system.G_drives) if m else None
        self._Gp = flat(gens) if gens else None
        self._goal = None if goal is None else np.ascontiguousarray(goal, dtype=np.float64).ravel()
        self._sub = None if subspace is None else np.ascontiguousarray(subspace, dtype=np.int32)
        d = _lib.qc_sweep_desc()
        d.T, d.zdim, d.off_a, d.off_dt, d.N = self.T, self.zdim, self.off_a, self.off_dt, N
        d.dt_fixed = 0.0 if dt_fixed is None else float(dt_fixed)
        d.global_dim, d.m, d.n_pert = self.global_dim, m, self.p
        d.state_cols = 0 if self.cols == N else self.cols
        d.fid_kind, d.fid_form = self.fid_kind, int(fid_form)
        d.G_drift = _lib.dptr(self._G0)
        d.G_drives = _lib.dptr(self._Gd) if m else None
        d.G_pert = _lib.dptr(self._Gp) if gens else None
        d.goal_iso = _lib.dptr(self._goal) if self._goal is not None else None
        d.subspace = self._sub.ctypes.data_as(C.POINTER(C.c_int32)) if self._sub is not None else None
        d.n_sub = 0 if self._sub is None else int(self._sub.size)
        d.device = device
        d.wide = wide_bits
        d.reserved1[0] = _lib.QC_SWEEP_STORED_STATES if stored_states else 0
        self.stored_states = bool(stored_states)
        self._desc = d
        self._counts = _device_counts(self)
        h = C.c_void_p()
        _lib.check_rc(_lib.lib.qc_sweep_create(C.byref(d), C.byref(h)), _ERR)
        self._h = h

    @property
    def wide64_grad(self) -> bool:
        """Whether the handle was made with `wide64_grad` (kept outside the instance's public flags, which are what they were)."""
        return self._wide64_grad

    @wide64_grad.setter
    def wide64_grad(self, given):
        self._wide64_grad = bool(given)

    @property
    def wide64_stored(self) -> bool:
        """Whether the handle was made with `wide64_stored` (kept outside the instance's public flags, as `wide64_grad` is)."""
        return self._wide64_stored

    @wide64_stored.setter
    def wide64_stored(self, given):
        self._wide64_stored = bool(given)

    @property
    def wide64_params(self) -> bool:
        """Whether the handle was made with `wide64_params` (kept outside the instance's public flags, as `wide64_grad` is)."""
        return self._wide64_params

    @wide64_params.setter
    def wide64_params(self, given):
        self._wide64_params = bool(given)

    @property
    def wide64_tangent(self) -> bool:
        """Whether the handle was made with `wide64_tangent` (kept outside the instance's public flags, as `wide64_grad` is)."""
        return self._wide64_tangent

    @wide64_tangent.setter
    def wide64_tangent(self, given):
        self._wide64_tangent = bool(given)

    @property
    def wide64_noise(self) -> bool:
        """Whether the handle was made with `wide64_noise` (kept outside the instance's public flags, as `wide64_grad` is)."""
        return self._wide64_noise

    @wide64_noise.setter
    def wide64_noise(self, given):
        self._wide64_noise = bool(given)

    def _scope(self, supported):
        """(served?, the library's reason why not or None) from a `qc_sweep_desc_*_supported` function."""
        ok = C.c_int32()
        _lib.check_rc(supported(C.byref(self._desc), C.byref(ok)), _ERR)
        return bool(ok.value), (None if ok.value else _lib.lib.qc_sweep_last_error(None).decode())

    @property
    def kernel_name(self) -> str:
        """"mfma16-sweep" (2N <= 16, up to 8 drives), "mfma32-sweep" (`wide`, 16 < 2N <= 32, up to 8 drives), "mfma64-sweep" (`wide` and
        `wide64`, 32 < 2N <= 64, up to 16 drives) or "rollout-per-sample"."""
        return _lib.lib.qc_sweep_kernel_name(self._h).decode()

    def launch(self, S: int):
        """(mfma, chunk, n_chunks) of a call with S samples: `qc_sweep_desc_launch`."""
        mf, ch, nch = C.c_int32(), C.c_int64(), C.c_int64()
        _lib.check_rc(_lib.lib.qc_sweep_desc_launch(C.byref(self._desc), int(S), C.byref(mf), C.byref(ch), C.byref(nch)), _ERR)
        return bool(mf.value), ch.value, nch.value

    def pack(self, controls, dts=None) -> np.ndarray:
        """The trajectory vector of this handle's layout from controls (m x T) and timesteps (scalar or one per knot)."""
        controls = np.asarray(controls, dtype=np.float64).reshape(self.m, -1) if self.m else np.zeros((0, self.T))
        if controls.shape[1] != self.T:
            raise ValueError(f"controls must be {self.m} x {self.T}")
        Z = np.zeros(self.Z_len)
        K = Z[:self.T * self.zdim].reshape(self.T, self.zdim)
        K[:, self.off_a:self.off_a + self.m] = controls.T
        if self.off_dt >= 0:
            if dts is None:
                raise ValueError("this handle reads its timesteps from the trajectory vector")
            K[:, self.off_dt] = np.full(self.T, float(dts)) if np.ndim(dts) == 0 else np.asarray(dts, dtype=np.float64).ravel()
        return Z

    def _samples(self, theta, scale):
        return _sweep_samples(self.p, self.m, theta, scale)

    # -- the argument checks of the host entries ... --------------------------------------------------------------------------------
    def _host_Z_init(self, Z, init):
        Z = np.ascontiguousarray(Z, dtype=np.float64).ravel()
        if Z.size != self.Z_len:
            raise ValueError(f"Z has length {Z.size}, expected {self.Z_len}")
        init = np.ascontiguousarray(init, dtype=np.float64).ravel()
        if init.size != self.ns:
            raise ValueError(f"initial state has length {init.size}, expected {self.ns}")
        return Z, init

    @staticmethod
    def _host_weights(weights, S):
        if weights is not None:
            weights = np.ascontiguousarray(weights, dtype=np.float64).ravel()
            if weights.size != S:
                raise ValueError(f"weights must have {S} entries")
        return weights

    @staticmethod
    def _host_direction(a, cnt, what):
        """A direction as a flat array of `cnt` entries; None stays None."""
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=np.float64).ravel()
        if a.size != cnt:
            raise ValueError(f"{what} has {a.size} entries, expected {cnt}")
        return a

    # -- ... and of the device entries ------------------------------------------------------------------------------------------------
    def _check_device(self, S, **tensors):
        """Every tensor that is given is contiguous float64 with the count `_device_counts` states for its name."""
        for what, t in tensors.items():
            if t is not None:
                per_sample, shared = self._counts[what]
                cnt = per_sample * S + shared
                if t.numel() != cnt or t.dtype != torch.float64 or not t.is_contiguous():
                    raise ValueError(f"{what} must be a contiguous float64 tensor of {cnt} entries")

    def _require_dtheta(self, dtheta):
        if self.p and dtheta is None:
            raise ValueError("dtheta is required: the handle has perturbations")

    def _refuse_unbacked(self, what_theta, like_theta, what_scale, like_scale):
        """A tensor shaped like theta on a handle without perturbations, one shaped like scale on a handle without drives."""
        if like_theta is not None and not self.p:
            raise ValueError(f"{what_theta} is given but the handle has no perturbations")
        if like_scale is not None and not self.m:
            raise ValueError(f"{what_scale} is given but the handle has no drives")

    def _noise_S(self, dnoise):
        if dnoise is None:
            raise ValueError("dnoise is required")
        per = (self.T - 1) * self.p
        if not per or dnoise.numel() % per or not dnoise.numel():
            raise ValueError(f"dnoise must hold S x {self.T - 1} x {self.p} entries")
        return dnoise.numel() // per

    def eval(self, Z, init, theta, scale=None, finals: bool = True, fids: Optional[bool] = None):
        """(finals, fids): finals (2N cols) x S or None; fids S values or None (default: when the handle has a fidelity)."""
        Z, init = self._host_Z_init(Z, init)
        S, theta, scale = self._samples(theta, scale)
        if fids is None:
            fids = self.fid_kind != _lib.QC_SWEEP_FID_NONE
        out = np.empty((S, self.ns)) if finals else None
        f = np.empty(S) if fids else None
        _lib.check_rc(_lib.lib.qc_sweep_eval(self._h, _lib.dptr(Z), _lib.dptr(init), S, _host_ptr(theta), _host_ptr(scale), _host_ptr(out),
                                             _host_ptr(f)), _ERR, self._h)
        return (np.ascontiguousarray(out.T) if finals else None), f

    def eval_device(self, dZ, dinit, dtheta, dscale, dfinals, dfids, stream=None):
        """Device-resident evaluation on torch CUDA tensors (float64), asynchronous on `stream`: dtheta S x n_pert (None
        without perturbations: dfinals / dfids give S), dscale S x m or None, dfinals S x (2N cols) or None, dfids S or None."""
        s = _stream_of(stream)
        if dfids is not None:
            S = dfids.numel()       # (dfids gives S and is not checked further, as ever)
        elif dfinals is not None:
            S = dfinals.numel() // self.ns
        else:
            raise ValueError("dfinals and dfids are both None")
        self._check_device(S, dtheta=dtheta, dscale=dscale, dfinals=dfinals, dZ=dZ, dinit=dinit)
        _lib.check_rc(_lib.lib.qc_sweep_eval_dev(self._h, dZ.data_ptr(), dinit.data_ptr(), S, _dev_ptr(dtheta, self.p), _dev_ptr(dscale, self.m),
                                                 _dev_ptr(dfinals), _dev_ptr(dfids), s), _ERR, self._h)

    # -- gradients: the adjoint of the sweep -------------------------------------------------------------------------------------
    @property
    def n_deriv(self) -> int:
        """Derivatives per interval and sample: the m drives, then the timestep when the trajectory vector carries it."""
        return self.m + (1 if self.off_dt >= 0 else 0)

    @property
    def grad_supported(self) -> bool:
        """Does `grad` serve this handle?  (`qc_sweep_desc_grad_supported`: the MFMA form, a unitary or ket fidelity, at most 16
        state columns, antisymmetric generators; with `stored_states` the "mfma16-sweep" form -- with `wide_stored` the "mfma32-sweep"
        form as well, with `wide64_grad` and `wide64_stored` the "mfma64-sweep" form with at most 32 state columns --, any fidelity, any generators.)
        `grad_unsupported_reason` says why not."""
        return self._scope(_lib.lib.qc_sweep_desc_grad_supported)[0]

    @property
    def grad_unsupported_reason(self) -> Optional[str]:
        return self._scope(_lib.lib.qc_sweep_desc_grad_supported)[1]

    def grad(self, Z, init, theta, scale=None, weights=None, per_sample: bool = False):
        """(J, fids, grad[, grad_samples]): J = sum_s w_s F_s (weights: S values, default 1/S each), the S fidelities, the dense
        gradient of J over the trajectory vector (zero outside the controls and timesteps of knots 0 .. T-2) and, with
        `per_sample`, dF_s/d(a_t, dt_t) as an S x (T-1) x n_deriv array (drives, then the timestep)."""
        Z, init = self._host_Z_init(Z, init)
        S, theta, scale = self._samples(theta, scale)
        weights = self._host_weights(weights, S)
        f, J, g = np.empty(S), C.c_double(), np.empty(self.Z_len)
        gs = np.empty((S, self.T - 1, self.n_deriv)) if per_sample else None
        _lib.check_rc(_lib.lib.qc_sweep_grad(self._h, _lib.dptr(Z), _lib.dptr(init), S, _host_ptr(theta), _host_ptr(scale), _host_ptr(weights),
                                             _lib.dptr(f), C.byref(J), _lib.dptr(g), _host_ptr(gs)), _ERR, self._h)
        return (J.value, f, g, gs) if per_sample else (J.value, f, g)

    def grad_device(self, dZ, dinit, S: int, dtheta=None, dscale=None, dweights=None, dfids=None, dJ=None, dgrad=None, dgrad_samples=None,
                    stream=None):
        """Device-resident gradient on torch CUDA tensors (float64), asynchronous on `stream`: `qc_sweep_grad_dev`.  Outputs are
        optional one at a time: dfids S, dJ one value, dgrad Z_len, dgrad_samples S x (T-1) x n_deriv."""
        s = _stream_of(stream)
        S = int(S)
        ptr = _dev_ptr
        _refuse_all_none("output", dfids, dJ, dgrad, dgrad_samples)
        self._check_device(S, dZ=dZ, dinit=dinit, dtheta=dtheta, dscale=dscale, dweights=dweights, dfids=dfids, dJ=dJ, dgrad=dgrad,
                           dgrad_samples=dgrad_samples)
        self._require_dtheta(dtheta)
        _lib.check_rc(_lib.lib.qc_sweep_grad_dev(self._h, dZ.data_ptr(), dinit.data_ptr(), S, ptr(dtheta, self.p), ptr(dscale, self.m), ptr(dweights),
                                                 ptr(dfids), ptr(dJ), ptr(dgrad), ptr(dgrad_samples), s), _ERR, self._h)

    # -- gradients with respect to the systems: dF_s/dtheta and dF_s/dscale ---------------------------------------------------
    def param_grad(self, Z, init, theta, scale=None, weights=None, with_controls: bool = False):
        """(fids, grad_theta, grad_scale): the S fidelities, dF_s/dtheta[s, j] (S x n_pert) and dF_s/dscale[s, k] (S x m; `scale`
        None: taken at all ones), raw per-sample values from one backward walk (`qc_sweep_grad_params`; "mfma16-sweep" handles,
        "mfma32-sweep" handles made with `wide_params` and "mfma64-sweep" handles made with `wide64_params`).  With `with_controls`:
        (J, fids, grad, grad_theta, grad_scale), J and the dense gradient over the trajectory vector as `grad` returns them."""
        Z, init = self._host_Z_init(Z, init)
        S, theta, scale = self._samples(theta, scale)
        weights = self._host_weights(weights, S)
        f, gth, gsc = np.empty(S), np.empty((S, self.p)), np.empty((S, self.m))
        J, g = C.c_double(), (np.empty(self.Z_len) if with_controls else None)
        _lib.check_rc(_lib.lib.qc_sweep_grad_params(self._h, _lib.dptr(Z), _lib.dptr(init), S, _host_ptr(theta), _host_ptr(scale), _host_ptr(weights),
                                                    _lib.dptr(f), C.byref(J) if with_controls else None, _host_ptr(g), None, _host_ptr(gth),
                                                    _host_ptr(gsc)), _ERR, self._h)
        return (J.value, f, g, gth, gsc) if with_controls else (f, gth, gsc)

    def param_grad_device(self, dZ, dinit, S: int, dtheta=None, dscale=None, dweights=None, dfids=None, dJ=None, dgrad=None, dgrad_samples=None,
                          dgrad_theta=None, dgrad_scale=None, stream=None):
        """`grad_device` plus dgrad_theta (S x n_pert) and dgrad_scale (S x m): `qc_sweep_grad_params_dev`.  Every output is
        optional; without dgrad and dgrad_samples no per-interval buffer is written."""
        s = _stream_of(stream)
        S = int(S)
        ptr = _dev_ptr
        _refuse_all_none("output", dfids, dJ, dgrad, dgrad_samples, dgrad_theta, dgrad_scale)
        self._refuse_unbacked("dgrad_theta", dgrad_theta, "dgrad_scale", dgrad_scale)
        self._check_device(S, dZ=dZ, dinit=dinit, dtheta=dtheta, dscale=dscale, dweights=dweights, dfids=dfids, dJ=dJ, dgrad=dgrad,
                           dgrad_samples=dgrad_samples, dgrad_theta=dgrad_theta, dgrad_scale=dgrad_scale)
        self._require_dtheta(dtheta)
        _lib.check_rc(_lib.lib.qc_sweep_grad_params_dev(self._h, dZ.data_ptr(), dinit.data_ptr(), S, ptr(dtheta, self.p), ptr(dscale, self.m),
                                                        ptr(dweights), ptr(dfids), ptr(dJ), ptr(dgrad), ptr(dgrad_samples), ptr(dgrad_theta),
                                                        ptr(dgrad_scale), s), _ERR, self._h)

    # -- pullbacks: the derivatives of any function of the final states -------------------------------------------------------------
    @property
    def vjp_supported(self) -> bool:
        """Does `vjp` serve this handle?  (`qc_sweep_desc_vjp_supported`: the MFMA forms, at most 16 state columns, antisymmetric
        generators; with `stored_states` the "mfma16-sweep" form (with `wide_stored`: or "mfma32-sweep"; with `wide64_grad` and `wide64_stored`: or "mfma64-sweep", at most 32 columns) and any generators; any
        fidelity or none.)
        `vjp_unsupported_reason` says why not."""
        return self._scope(_lib.lib.qc_sweep_desc_vjp_supported)[0]

    @property
    def vjp_unsupported_reason(self) -> Optional[str]:
        return self._scope(_lib.lib.qc_sweep_desc_vjp_supported)[1]

    def vjp(self, Z, init, cot, theta, scale=None, per_sample: bool = False, init_grad: bool = False, params: bool = False):
        """The pullback of the final states: with phi_s = <cot[s], x_final[s]> (cot: S x (2N cols), one cotangent per sample), returns
        `grad`, the plain sum over the samples of dphi_s/dZ as a dense vector over the trajectory vector, followed -- in this order --
        by what was asked for:
            per_sample   grad_samples, S x (T-1) x n_deriv: dphi_s/d(a_t, dt_t)
            init_grad    grad_init, S x (2N cols): dphi_s/dinit
            params       grad_theta (S x n_pert) and grad_scale (S x m), two entries ("mfma16-sweep" handles, "mfma32-sweep" handles made
                         with `wide_params` and "mfma64-sweep" handles made with `wide64_params`)."""
        Z, init = self._host_Z_init(Z, init)
        S, theta, scale = self._samples(theta, scale)
        cot = np.ascontiguousarray(cot, dtype=np.float64)
        if cot.shape != (S, self.ns):
            raise ValueError(f"cot must be {S} x {self.ns}")
        g = np.empty(self.Z_len)
        gs = np.empty((S, self.T - 1, self.n_deriv)) if per_sample else None
        gi = np.empty((S, self.ns)) if init_grad else None
        gth, gsc = (np.empty((S, self.p)), np.empty((S, self.m))) if params else (None, None)
        _lib.check_rc(_lib.lib.qc_sweep_vjp(self._h, _lib.dptr(Z), _lib.dptr(init), S, _host_ptr(theta), _host_ptr(scale), _lib.dptr(cot), None,
                                            _lib.dptr(g), _host_ptr(gs), _host_ptr(gi), _host_ptr(gth), _host_ptr(gsc)), _ERR, self._h)
        return (g,) + ((gs,) if per_sample else ()) + ((gi,) if init_grad else ()) + ((gth, gsc) if params else ())

    def vjp_device(self, dZ, dinit, S: int, dcot, dtheta=None, dscale=None, dfinals=None, dgrad=None, dgrad_samples=None, dgrad_init=None,
                   dgrad_theta=None, dgrad_scale=None, stream=None):
        """Device-resident pullback on torch CUDA tensors (float64), asynchronous on `stream`: `qc_sweep_vjp_dev`.  dcot S x (2N cols);
        outputs optional one at a time: dfinals S x (2N cols) (the bits of `eval_device`), dgrad Z_len, dgrad_samples
        S x (T-1) x n_deriv, dgrad_init S x (2N cols), dgrad_theta S x n_pert, dgrad_scale S x m."""
        s = _stream_of(stream)
        S = int(S)
        ptr = _dev_ptr
        _refuse_all_none("output", dfinals, dgrad, dgrad_samples, dgrad_init, dgrad_theta, dgrad_scale)
        if dcot is None:
            raise ValueError("dcot is required")
        self._refuse_unbacked("dgrad_theta", dgrad_theta, "dgrad_scale", dgrad_scale)
        self._check_device(S, dZ=dZ, dinit=dinit, dcot=dcot, dtheta=dtheta, dscale=dscale, dfinals=dfinals, dgrad=dgrad, dgrad_samples=dgrad_samples,
                           dgrad_init=dgrad_init, dgrad_theta=dgrad_theta, dgrad_scale=dgrad_scale)
        self._require_dtheta(dtheta)
        _lib.check_rc(_lib.lib.qc_sweep_vjp_dev(self._h, dZ.data_ptr(), dinit.data_ptr(), S, ptr(dtheta, self.p), ptr(dscale, self.m), ptr(dcot),
                                                ptr(dfinals), ptr(dgrad), ptr(dgrad_samples), ptr(dgrad_init), ptr(dgrad_theta), ptr(dgrad_scale), s),
                      _ERR, self._h)

    # -- pushforwards: the tangent of the final states and fidelities along one direction -------------------------------------------
    @property
    def jvp_supported(self) -> bool:
        """Does `jvp` serve this handle?  (`qc_sweep_desc_jvp_supported`: the "mfma16-sweep" form, "mfma32-sweep" with `wide_tangent`, or "mfma64-sweep" with `wide64_tangent` and 2N x cols <= 2048; any generators -- Lindblad ones
        included -- and any fidelity or none.)  `jvp_unsupported_reason` says why not."""
        return self._scope(_lib.lib.qc_sweep_desc_jvp_supported)[0]

    @property
    def jvp_unsupported_reason(self) -> Optional[str]:
        return self._scope(_lib.lib.qc_sweep_desc_jvp_supported)[1]

    def jvp(self, Z, init, vZ, theta, scale=None, vinit=None, vtheta=None, vscale=None, fids: bool = False):
        """The pushforward of the final states along the direction (vZ, vinit, vtheta, vscale): `tfinals`, S x (2N cols), row s the tangent
        of sample s's final state, and with `fids` also `tfids`, the S tangents of the fidelities.  vZ (Z_len, the layout of Z: only the
        controls and timesteps of knots 0 .. T-2 act) and vinit (2N cols) are shared by the samples, vtheta is S x n_pert, vscale S x m
        (valid with scale = None: taken at all ones); whichever is None is zero, at least one must be given."""
        Z, init = self._host_Z_init(Z, init)
        if theta is None and scale is None and (vtheta is not None or vscale is not None):
            S = np.asarray(vtheta if vtheta is not None else vscale).reshape(-1, self.p if vtheta is not None else self.m).shape[0]
        else:
            S, theta, scale = self._samples(theta, scale)
        vec, ptr = self._host_direction, _host_ptr
        vZ, vinit = vec(vZ, self.Z_len, "vZ"), vec(vinit, self.ns, "vinit")
        vtheta, vscale = vec(vtheta, S * self.p, "vtheta"), vec(vscale, S * self.m, "vscale")
        tf = np.empty((S, self.ns))
        tfid = np.empty(S) if fids else None
        _lib.check_rc(_lib.lib.qc_sweep_jvp(self._h, _lib.dptr(Z), _lib.dptr(init), S, ptr(theta), ptr(scale), ptr(vZ, True), ptr(vinit, True),
                                            ptr(vtheta, True), ptr(vscale, True), None, None, _lib.dptr(tf), ptr(tfid)), _ERR, self._h)
        return (tf, tfid) if fids else tf

    def jvp_device(self, dZ, dinit, S: int, dtheta=None, dscale=None, dvZ=None, dvinit=None, dvtheta=None, dvscale=None, dfinals=None, dfids=None,
                   dtfinals=None, dtfids=None, stream=None):
        """Device-resident pushforward on torch CUDA tensors (float64), asynchronous on `stream`: `qc_sweep_jvp_dev`.  Directions, each
        optional, at least one: dvZ Z_len, dvinit 2N cols, dvtheta S x n_pert, dvscale S x m.  Outputs, each optional, at least one:
        dfinals S x (2N cols) and dfids S (the bits of `eval_device`), dtfinals S x (2N cols), dtfids S."""
        s = _stream_of(stream)
        S = int(S)
        ptr = _dev_ptr
        _refuse_all_none("direction", dvZ, dvinit, dvtheta, dvscale)
        _refuse_all_none("output", dfinals, dfids, dtfinals, dtfids)
        self._refuse_unbacked("dvtheta", dvtheta, "dvscale", dvscale)
        self._check_device(S, dZ=dZ, dinit=dinit, dtheta=dtheta, dscale=dscale, dvZ=dvZ, dvinit=dvinit, dvtheta=dvtheta, dvscale=dvscale,
                           dfinals=dfinals, dfids=dfids, dtfinals=dtfinals, dtfids=dtfids)
        self._require_dtheta(dtheta)
        _lib.check_rc(_lib.lib.qc_sweep_jvp_dev(self._h, dZ.data_ptr(), dinit.data_ptr(), S, ptr(dtheta, self.p), ptr(dscale, self.m), ptr(dvZ),
                                                ptr(dvinit), ptr(dvtheta), ptr(dvscale), ptr(dfinals), ptr(dfids), ptr(dtfinals), ptr(dtfids), s),
                      _ERR, self._h)

    # -- Hessian products: the tangent of the pullback along one direction ------------------------------------------------------------
    @property
    def hvp_supported(self) -> bool:
        """Does `hvp` serve this handle?  (`qc_sweep_desc_hvp_supported`: the closed scope of `vjp` -- antisymmetric generators, at most
        16 state columns, any fidelity or none -- in the "mfma16-sweep" form, or in the "mfma32-sweep" form of a handle made with
        `wide_hessian`.)  `hvp_unsupported_reason` says why not."""
        return self._scope(_lib.lib.qc_sweep_desc_hvp_supported)[0]

    @property
    def hvp_unsupported_reason(self) -> Optional[str]:
        """None when `hvp` is served, else the library's reason: the pullback's first (the rollout-per-sample form with its cause,
        "... is not antisymmetric", more than 16 columns), then "Hessian products are not served in the mfma32-sweep form" for a wide
        handle made without `wide_hessian`."""
        return self._scope(_lib.lib.qc_sweep_desc_hvp_supported)[1]

    def hvp(self, Z, init, cot, theta, scale=None, vZ=None, vinit=None, vtheta=None, vscale=None, vcot=None, per_sample: bool = False,
            init_grad: bool = False):
        """The tangent of the pullback `vjp` along the direction (vZ, vinit, vtheta, vscale, vcot), each None = zero, at least one given:
        returns `tgrad` (Z_len), the directional derivative of `vjp`'s `grad`, followed -- in this order -- by what was asked for:
            per_sample   tgrad_samples, S x (T-1) x n_deriv: the derivative of `grad_samples`
            init_grad    tgrad_init, S x (2N cols): the derivative of `grad_init`
        With cot = d loss/dX and vcot = (d2 loss/dX2) Xdot (Xdot: `jvp` along vZ) `tgrad` is the exact Hessian product of loss(X(Z)) with
        vZ; with vcot = None it is the curvature of the sweep map alone, what a Gauss-Newton product drops."""
        Z, init = self._host_Z_init(Z, init)
        cot = np.ascontiguousarray(cot, dtype=np.float64)
        if theta is None and scale is None:
            S = cot.reshape(-1, self.ns).shape[0]
        else:
            S, theta, scale = self._samples(theta, scale)
        if cot.size != S * self.ns:
            raise ValueError(f"cot must be {S} x {self.ns}")
        vec, ptr = self._host_direction, _host_ptr
        vZ, vinit, vcot = vec(vZ, self.Z_len, "vZ"), vec(vinit, self.ns, "vinit"), vec(vcot, S * self.ns, "vcot")
        vtheta, vscale = vec(vtheta, S * self.p, "vtheta"), vec(vscale, S * self.m, "vscale")
        tg = np.empty(self.Z_len)
        tgs = np.empty((S, self.T - 1, self.n_deriv)) if per_sample else None
        tgi = np.empty((S, self.ns)) if init_grad else None
        _lib.check_rc(_lib.lib.qc_sweep_hvp(self._h, _lib.dptr(Z), _lib.dptr(init), S, ptr(theta), ptr(scale), _lib.dptr(cot), ptr(vZ, True),
                                            ptr(vinit, True), ptr(vtheta, True), ptr(vscale, True), ptr(vcot, True), _lib.dptr(tg), ptr(tgs), ptr(tgi)),
                      _ERR, self._h)
        return (tg,) + ((tgs,) if per_sample else ()) + ((tgi,) if init_grad else ())

    def hvp_device(self, dZ, dinit, S: int, dcot, dtheta=None, dscale=None, dvZ=None, dvinit=None, dvtheta=None, dvscale=None, dvcot=None,
                   dtgrad=None, dtgrad_samples=None, dtgrad_init=None, stream=None):
        """Device-resident Hessian product on torch CUDA tensors (float64), asynchronous on `stream`: `qc_sweep_hvp_dev`.  dcot
        S x (2N cols); directions, each optional, at least one: dvZ Z_len, dvinit 2N cols, dvtheta S x n_pert, dvscale S x m, dvcot
        S x (2N cols).  Outputs, each optional, at least one: dtgrad Z_len, dtgrad_samples S x (T-1) x n_deriv, dtgrad_init S x (2N cols)."""
        s = _stream_of(stream)
        S = int(S)
        ptr = _dev_ptr
        if dcot is None:
            raise ValueError("dcot is required")
        _refuse_all_none("direction", dvZ, dvinit, dvtheta, dvscale, dvcot)
        _refuse_all_none("output", dtgrad, dtgrad_samples, dtgrad_init)
        self._refuse_unbacked("dvtheta", dvtheta, "dvscale", dvscale)
        self._check_device(S, dZ=dZ, dinit=dinit, dcot=dcot, dtheta=dtheta, dscale=dscale, dvZ=dvZ, dvinit=dvinit, dvtheta=dvtheta, dvscale=dvscale,
                           dvcot=dvcot, dtgrad=dtgrad, dtgrad_samples=dtgrad_samples, dtgrad_init=dtgrad_init)
        self._require_dtheta(dtheta)
        _lib.check_rc(_lib.lib.qc_sweep_hvp_dev(self._h, dZ.data_ptr(), dinit.data_ptr(), S, ptr(dtheta, self.p), ptr(dscale, self.m), ptr(dcot),
                                                ptr(dvZ), ptr(dvinit), ptr(dvtheta), ptr(dvscale), ptr(dvcot), ptr(dtgrad), ptr(dtgrad_samples),
                                                ptr(dtgrad_init), s), _ERR, self._h)

    # -- noise trajectories: perturbation amplitudes that change from interval to interval ---------------------------------------------
    @property
    def noise_supported(self) -> bool:
        """Do `noise_eval` / `noise_eval_device` serve this handle?  (`qc_sweep_desc_noise_supported`: the "mfma16-sweep" form, at least
        one perturbation, drives and perturbations together at most 8; or the "mfma32-sweep" form of a handle made with `wide_noise`, at
        least one perturbation, no limit on drives and perturbations together; or the "mfma64-sweep" form of a handle made with
        `wide64_noise`, likewise.)  `noise_unsupported_reason` says why not.  `noise_grad` also needs `grad_supported` (in the
        "mfma64-sweep" form: `wide64_grad`)."""
        return self._scope(_lib.lib.qc_sweep_desc_noise_supported)[0]

    @property
    def noise_unsupported_reason(self) -> Optional[str]:
        return self._scope(_lib.lib.qc_sweep_desc_noise_supported)[1]

    def _noise_samples(self, noise, theta, scale):
        """(S, noise S x (T-1) x p, theta S x p, scale S x m or None): the noise gives S; theta None means zeros."""
        if noise is None:
            raise ValueError("noise is required: S x (T-1) x n_pert")
        noise = np.asarray(noise, dtype=np.float64)
        if noise.ndim == 2 and self.p == 1:
            noise = noise[:, :, None]
        if noise.ndim != 3 or noise.shape[0] < 1 or noise.shape[1:] != (self.T - 1, self.p):
            raise ValueError(f"noise must be S x {self.T - 1} x {self.p}" + (f" (or S x {self.T - 1})" if self.p == 1 else ""))
        S = noise.shape[0]
        if theta is None:
            theta = np.zeros((S, self.p))
        S2, theta, scale = _sweep_samples(self.p, self.m, theta, scale)
        if S2 != S:
            raise ValueError(f"theta / scale give {S2} samples, noise gives {S}")
        return S, np.ascontiguousarray(noise), theta, scale

    def noise_eval(self, Z, init, noise, theta=None, scale=None, finals: bool = True, fids: Optional[bool] = None):
        """`eval` with a noise trajectory per sample: in interval t sample s sees theta[s, j] + noise[s, t, j] on perturbation j
        (`qc_sweep_noise_eval`).  noise: S x (T-1) x n_pert (S x (T-1) when n_pert = 1); theta: S x n_pert or None = zeros.
        Returns (finals, fids) as `eval`."""
        Z, init = self._host_Z_init(Z, init)
        S, noise, theta, scale = self._noise_samples(noise, theta, scale)
        if fids is None:
            fids = self.fid_kind != _lib.QC_SWEEP_FID_NONE
        out = np.empty((S, self.ns)) if finals else None
        f = np.empty(S) if fids else None
        _lib.check_rc(_lib.lib.qc_sweep_noise_eval(self._h, _lib.dptr(Z), _lib.dptr(init), S, _host_ptr(theta), _host_ptr(scale), _host_ptr(noise),
                                                   _host_ptr(out), _host_ptr(f)), _ERR, self._h)
        return (np.ascontiguousarray(out.T) if finals else None), f

    def _device_theta(self, dtheta, S, like):
        """theta=None means zeros: one zero tensor per S, kept by the handle."""
        if dtheta is not None or not self.p:
            return dtheta
        z = getattr(self, "_zero_theta", None)
        if z is None or z.numel() != S * self.p or z.device != like.device:
            z = self._zero_theta = torch.zeros(S * self.p, dtype=torch.float64, device=like.device)
        return z

    def noise_eval_device(self, dZ, dinit, dnoise, dtheta=None, dscale=None, dfinals=None, dfids=None, stream=None):
        """Device-resident `noise_eval` on torch CUDA tensors (float64), asynchronous on `stream`: `qc_sweep_noise_eval_dev`.  dnoise
        S x (T-1) x n_pert gives S; dtheta S x n_pert or None = zeros; dscale S x m or None; dfinals S x (2N cols) or None; dfids S
        or None."""
        s = _stream_of(stream)
        S = self._noise_S(dnoise)
        ptr = _dev_ptr
        if dfinals is None and dfids is None:
            raise ValueError("dfinals and dfids are both None")
        dtheta = self._device_theta(dtheta, S, dnoise)
        self._check_device(S, dZ=dZ, dinit=dinit, dnoise=dnoise, dtheta=dtheta, dscale=dscale, dfinals=dfinals, dfids=dfids)
        _lib.check_rc(_lib.lib.qc_sweep_noise_eval_dev(self._h, dZ.data_ptr(), dinit.data_ptr(), S, ptr(dtheta, self.p), ptr(dscale, self.m),
                                                       ptr(dnoise), ptr(dfinals), ptr(dfids), s), _ERR, self._h)

    def noise_grad(self, Z, init, noise, theta=None, scale=None, weights=None, per_sample: bool = False):
        """(J, fids, grad, grad_noise[, grad_samples]) under the noise trajectories of `noise_eval` (`qc_sweep_noise_grad`): J, fids and
        the dense gradient as `grad` returns them, and grad_noise[s, t, j] = dF_s/dnoise[s, t, j], S x (T-1) x n_pert, raw per-sample
        values -- the time-resolved noise sensitivity of every sample.  With `per_sample` also dF_s/d(a_t, dt_t) as in `grad`."""
        Z, init = self._host_Z_init(Z, init)
        S, noise, theta, scale = self._noise_samples(noise, theta, scale)
        weights = self._host_weights(weights, S)
        f, J, g, gn = np.empty(S), C.c_double(), np.empty(self.Z_len), np.empty((S, self.T - 1, self.p))
        gs = np.empty((S, self.T - 1, self.n_deriv)) if per_sample else None
        _lib.check_rc(_lib.lib.qc_sweep_noise_grad(self._h, _lib.dptr(Z), _lib.dptr(init), S, _host_ptr(theta), _host_ptr(scale), _host_ptr(noise),
                                                   _host_ptr(weights), _lib.dptr(f), C.byref(J), _lib.dptr(g), _host_ptr(gs), _host_ptr(gn)),
                      _ERR, self._h)
        return (J.value, f, g, gn, gs) if per_sample else (J.value, f, g, gn)

    def noise_grad_device(self, dZ, dinit, dnoise, dtheta=None, dscale=None, dweights=None, dfids=None, dJ=None, dgrad=None, dgrad_samples=None,
                          dgrad_noise=None, stream=None):
        """Device-resident `noise_grad`: `qc_sweep_noise_grad_dev`.  dnoise S x (T-1) x n_pert gives S.  Outputs are optional one at
        a time: dfids S, dJ one value, dgrad Z_len, dgrad_samples S x (T-1) x n_deriv, dgrad_noise S x (T-1) x n_pert."""
        s = _stream_of(stream)
        S = self._noise_S(dnoise)
        ptr = _dev_ptr
        _refuse_all_none("output", dfids, dJ, dgrad, dgrad_samples, dgrad_noise)
        dtheta = self._device_theta(dtheta, S, dnoise)
        self._check_device(S, dZ=dZ, dinit=dinit, dnoise=dnoise, dtheta=dtheta, dscale=dscale, dweights=dweights, dfids=dfids, dJ=dJ, dgrad=dgrad,
                           dgrad_samples=dgrad_samples, dgrad_noise=dgrad_noise)
        _lib.check_rc(_lib.lib.qc_sweep_noise_grad_dev(self._h, dZ.data_ptr(), dinit.data_ptr(), S, ptr(dtheta, self.p), ptr(dscale, self.m),
                                                       ptr(dnoise), ptr(dweights), ptr(dfids), ptr(dJ), ptr(dgrad), ptr(dgrad_samples),
                                                       ptr(dgrad_noise), s), _ERR, self._h)

    def finals_autograd(self, dZ, dinit, dtheta=None, dscale=None):
        """The S x (2N cols) final states as a differentiable torch tensor: forward is `eval_device` on the current stream, backward one
        `vjp_device` call, and under `torch.autograd.forward_ad` the tangent is one `jvp_device` call ("mfma16-sweep" handles, "mfma32-sweep" handles made with `wide_tangent` and "mfma64-sweep" handles made with `wide64_tangent`).  dZ
        (Z_len), dinit (2N cols), dtheta (S x n_pert), dscale (S x m or None) are float64 CUDA tensors; whichever requires grad
        receives one: Z the plain sum over the samples, init the sum of the per-sample derivatives, theta and scale their per-sample
        values ("mfma16-sweep" handles, "mfma32-sweep" handles made with `wide_params` and "mfma64-sweep" handles made with
        `wide64_params`: on a wide handle made without it a theta or scale that requires grad raises in backward)."""
        if dtheta is None and dscale is None:
            raise ValueError("dtheta (S x n_pert) or dscale (S x m) must give the number of samples")
        S = (dtheta if dtheta is not None else dscale).shape[0]
        return _SweepFinals.apply(self, int(S), dZ, dinit, dtheta, dscale)

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib.qc_sweep_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _SweepFinals(torch.autograd.Function):
    """`RolloutSweep.finals_autograd`: final states forward, one pullback call backward, only the outputs whose inputs need them."""

    @staticmethod
    def forward(ctx, sw, S, dZ, dinit, dtheta, dscale):
        ctx.init_shape = dinit.shape
        dZ, dinit = dZ.detach().contiguous(), dinit.detach().contiguous().reshape(-1)
        dtheta = None if dtheta is None else dtheta.detach().contiguous()
        dscale = None if dscale is None else dscale.detach().contiguous()
        out = torch.empty((S, sw.ns), dtype=torch.float64, device=dZ.device)
        sw.eval_device(dZ, dinit, dtheta, dscale, out, None)
        ctx.sw, ctx.S = sw, S
        ctx.save_for_backward(dZ, dinit, dtheta, dscale)
        ctx.save_for_forward(dZ, dinit, dtheta, dscale)
        return out

    @staticmethod
    def jvp(ctx, _sw, _S, tZ, tinit, ttheta, tscale):
        """Forward mode: tangents for whichever of Z, init, theta, scale carry one, one `jvp_device` call."""
        sw, S = ctx.sw, ctx.S
        dZ, dinit, dtheta, dscale = ctx.saved_tensors
        flat = lambda t: None if t is None else t.detach().contiguous().reshape(-1)
        tZ, tinit = flat(tZ), flat(tinit)
        ttheta = flat(ttheta) if sw.p else None
        tscale = flat(tscale) if sw.m else None
        out = torch.empty((S, sw.ns), dtype=torch.float64, device=dZ.device)
        if all(t is None for t in (tZ, tinit, ttheta, tscale)):
            return out.zero_()
        sw.jvp_device(dZ, dinit, S, dtheta, dscale, dvZ=tZ, dvinit=tinit, dvtheta=ttheta, dvscale=tscale, dtfinals=out)
        return out

    @staticmethod
    def backward(ctx, grad_output):
        sw, S = ctx.sw, ctx.S
        dZ, dinit, dtheta, dscale = ctx.saved_tensors
        need_Z, need_init, need_theta, need_scale = ctx.needs_input_grad[2:6]
        if not (need_Z or need_init or need_theta or need_scale):
            return (None,) * 6
        if sw.kernel_name == "mfma32-sweep" and not sw.wide_params and (need_theta or need_scale):
            raise _lib.QCollocError(_lib.QC_ERR_UNSUPPORTED, "qc_sweep pullback: parameter cotangents are not served in the mfma32-sweep form")
        mk = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dZ.device)
        gZ = mk(sw.Z_len) if need_Z else None
        gI = mk(S, sw.ns) if need_init else None
        gT = mk(S, sw.p) if (need_theta and sw.p) else None
        gC = mk(S, sw.m) if (need_scale and sw.m) else None
        if any(t is not None for t in (gZ, gI, gT, gC)):
            sw.vjp_device(dZ, dinit, S, grad_output.contiguous(), dtheta, dscale, dgrad=gZ, dgrad_init=gI, dgrad_theta=gT, dgrad_scale=gC)
        if need_theta and gT is None:
            gT = torch.zeros_like(dtheta)
        if need_scale and gC is None:
            gC = torch.zeros_like(dscale)
        return None, None, gZ, (gI.sum(0).reshape(ctx.init_shape) if need_init else None), gT, gC


def _one_shot(entry, init, controls, dts, system, perturbations, args, cols, **handle):
    """`entry(sw, Z, init, *args)` on a handle made for this call: T and (by default) cols from the arguments, the trajectory vector
    packed from controls and timesteps, `handle` as `RolloutSweep` takes it."""
    controls = np.asarray(controls, dtype=np.float64)
    if controls.ndim != 2 or controls.shape[0] != system.n_drives:
        raise ValueError("controls must be n_drives x T")
    T = controls.shape[1]
    init = np.ascontiguousarray(init, dtype=np.float64).ravel()
    n = 2 * system.state_levels
    if cols is None:
        cols = init.size // n
    sw = RolloutSweep(system, perturbations, T, cols=cols, **handle)
    try:
        return entry(sw, sw.pack(controls, dts), init, *args)
    finally:
        sw.close()


def rollout_sweep(init, controls, dts, system, perturbations, theta, scale=None, cols: Optional[int] = None, goal=None, fid_kind=None,
                  subspace=None, device: int = 0, fid_form: int = _lib.QC_FID_FORM_ABS, wide: bool = False, stored_states: bool = False,
                  wide_stored: bool = False, wide_tangent: bool = False, wide64: bool = False):
    """(finals, fids) of S rollouts under the perturbed systems: finals is (2N cols) x S, fids S values (None without `fid_kind`).
    theta is S x len(perturbations) (S x 0 without perturbations), scale S x n_drives or None (all ones); `wide`, `stored_states`,
    `wide_stored` and `wide_tangent` as `RolloutSweep` (the forward sweep itself looks at none of the last three); `wide64` (only with
    `wide`) as `RolloutSweep`: 32 < 2N <= 64 with up to 16 drives on the matrix cores ("mfma64-sweep")."""
    return _one_shot(RolloutSweep.eval, init, controls, dts, system, perturbations, (theta, scale), cols, goal=goal, fid_kind=fid_kind,
                     subspace=subspace, fid_form=fid_form, device=device, wide=wide, stored_states=stored_states, wide_stored=wide_stored,
                     wide_tangent=wide_tangent, wide64=wide64)


def rollout_noise_sweep(init, controls, dts, system, perturbations, noise, theta=None, scale=None, cols: Optional[int] = None, goal=None,
                        fid_kind=None, subspace=None, device: int = 0, fid_form: int = _lib.QC_FID_FORM_ABS, wide: bool = False,
                        wide64: bool = False):
    """(finals, fids) of S rollouts whose perturbation amplitudes change from interval to interval: in interval t sample s sees
    theta[s, j] + noise[s, t, j] on perturbation j.  noise is S x (T-1) x len(perturbations) (S x (T-1) for one perturbation), theta
    S x len(perturbations) or None (zeros); everything else as `rollout_sweep`.  `wide=True` serves 16 < 2N <= 32 on the matrix cores
    (the handle is made with `wide` and `wide_noise`); `wide=True, wide64=True` serves 32 < 2N <= 64 with up to 16 drives as well (the
    handle is made with `wide64` and `wide64_noise` too)."""
    return _one_shot(RolloutSweep.noise_eval, init, controls, dts, system, perturbations, (noise, theta, scale), cols, goal=goal, fid_kind=fid_kind,
                     subspace=subspace, fid_form=fid_form, device=device, wide=wide, wide_noise=wide, wide64=wide64, wide64_noise=wide64)


def rollout_sweep_parameter_gradient(init, controls, dts, system, perturbations, theta, scale=None, cols: Optional[int] = None, goal=None,
                                     fid_kind="unitary", subspace=None, device: int = 0, fid_form: int = _lib.QC_FID_FORM_ABS,
                                     stored_states: bool = False, wide: bool = False, wide_stored: bool = False, wide64: bool = False,
                                     wide64_stored: bool = False, wide64_grad: bool = False, wide64_params: bool = False):
    """(fids, grad_theta, grad_scale) of S rollouts under the perturbed systems: the fidelities of `rollout_sweep` and their derivatives
    with respect to theta (S x len(perturbations)) and scale (S x n_drives; None: taken at all ones).  Arguments as `rollout_sweep`;
    `stored_states=True` serves open systems (`RolloutSweep`); `wide=True` serves 16 < 2N <= 32 on the matrix cores (the handle is made
    with `wide` and `wide_params`); all three of `wide`, `stored_states` and `wide_stored` serve open systems there (wide = 11);
    all four of `wide`, `wide64`, `wide64_grad` and `wide64_params` serve closed systems of 32 < 2N <= 64 ("mfma64-sweep"), and with
    `stored_states` and `wide64_stored` as well open systems there."""
    return _one_shot(RolloutSweep.param_grad, init, controls, dts, system, perturbations, (theta, scale), cols, goal=goal, fid_kind=fid_kind,
                     subspace=subspace, fid_form=fid_form, device=device, stored_states=stored_states, wide=wide, wide_params=wide,
                     wide_stored=wide_stored, wide64=wide64, wide64_grad=wide64_grad, wide64_params=wide64_params,
                     wide64_stored=wide64_stored)


def _traj_dts(traj):
    return traj[traj.timestep].ravel() if isinstance(traj.timestep, str) else float(traj.timestep)


def unitary_rollout_fidelity_sweep(traj: NamedTrajectory, system, perturbations, theta, scale=None, state_name: str = "Ũ⃗",
                                   control_name: str = "a", subspace: Optional[Sequence[int]] = None, device: int = 0, wide: bool = False,
                                   wide64: bool = False) -> np.ndarray:
    """`unitary_rollout_fidelity` under S perturbed systems: initial state, goal and timesteps as that function takes them; `wide` and
    `wide64` as `rollout_sweep` (both True: up to 32 levels on the matrix cores)."""
    init = traj.initial.get(state_name) if getattr(traj, "initial", None) else None
    if init is None:
        init = operator_to_iso_vec(np.eye(system.levels, dtype=complex))
    return rollout_sweep(np.asarray(init, dtype=np.float64), traj[control_name], _traj_dts(traj), system, perturbations, theta, scale,
                         cols=system.levels, goal=np.asarray(traj.goal[state_name], dtype=np.float64), fid_kind="unitary", subspace=subspace,
                         device=device, wide=wide, wide64=wide64)[1]


def rollout_fidelity_sweep(traj: NamedTrajectory, system, perturbations, theta, scale=None, state_name: str = "ψ̃", control_name: str = "a",
                           device: int = 0, wide: bool = False, wide64: bool = False) -> np.ndarray:
    """`rollout_fidelity` of a ket component under S perturbed systems; `wide` and `wide64` as `rollout_sweep`."""
    init = traj.initial.get(state_name) if getattr(traj, "initial", None) else None
    if init is None:
        init = traj[state_name][:, 0]
    return rollout_sweep(np.ascontiguousarray(init, dtype=np.float64), traj[control_name], _traj_dts(traj), system, perturbations, theta, scale,
                         cols=1, goal=np.asarray(traj.goal[state_name], dtype=np.float64), fid_kind="ket", device=device, wide=wide, wide64=wide64)[1]
