"""Final-knot fidelity terms ("next" row 1), evaluated on the GPU through
`qc_fidelity_*` (include/qcolloc.h):

    iso_vec_unitary_fidelity(U_T, U_G; subspace)                      unitary_minimum_time_problem.jl:77
    UnitaryInfidelityObjective(state_name, traj, Q; subspace)         unitary_smooth_pulse_problem.jl:133-137
    FinalUnitaryFidelityConstraint(state_name, val, traj; subspace)   unitary_minimum_time_problem.jl:80-84

Loss per the reference docstring (unitary_smooth_pulse_problem.jl:23-28): l = |1 - |tr(U_goal' U_T)| / N|.
Only the last knot's state enters; gradients/Hessians are returned on those `2N^2` variables together with
their global indices.

Whole-trajectory terms through `qc_terms_*`: `QuadraticRegularizer`, `MinimumTimeObjective`,
`QuadraticSmoothnessRegularizer`, `PairwiseQuadraticRegularizer`, `L1Regularizer` (summed into one `TrajectoryObjective`) and
the constant `TimeStepsAllEqualConstraint` / `L1SlackConstraint`; through `qc_robust_*`:
`UnitaryRobustnessObjective` (unitary_robustness_problem.jl:46-49).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from .named_trajectory import NamedTrajectory


class _Fidelity:
    def __init__(self, goal_iso: np.ndarray, subspace: Optional[Sequence[int]] = None, device: int = 0, kind: str = "unitary",
                 form: str = "abs", phase_operators: Optional[Sequence[np.ndarray]] = None):
        goal_iso = np.ascontiguousarray(goal_iso, dtype=np.float64)
        self._h = C.c_void_p()
        self.K = 0
        if kind == "unitary":
            self.N = int(round((goal_iso.size / 2) ** 0.5))
            self.s = 2 * self.N * self.N
            if goal_iso.size != self.s:
                raise ValueError("goal must be an iso-vec of length 2 N^2")
            sub = None if subspace is None else np.ascontiguousarray(subspace, dtype=np.int32)
            d = _lib.qc_fidelity_desc()
            d.kind, d.N, d.goal_iso = _lib.QC_FID_UNITARY, self.N, _lib.dptr(goal_iso)
            d.subspace = None if sub is None else sub.ctypes.data_as(C.POINTER(C.c_int32))
            d.n_sub = 0 if sub is None else sub.size
            d.form = {"abs": _lib.QC_FID_FORM_ABS, "abs2": _lib.QC_FID_FORM_ABS2}[form]
            d.device = device
            keep = []
            if phase_operators is not None and len(phase_operators):
                ops = [np.asarray(Op, dtype=complex) for Op in phase_operators]
                dims = np.ascontiguousarray([Op.shape[0] for Op in ops], dtype=np.int32)
                planes = np.ascontiguousarray(np.concatenate([np.concatenate([Op.real.reshape(-1, order="F"), Op.imag.reshape(-1, order="F")])
                                                              for Op in ops]))
                d.n_phases = self.K = len(ops)
                d.phase_dims = dims.ctypes.data_as(C.POINTER(C.c_int32))
                d.phase_ops = _lib.dptr(planes)
                keep = [dims, planes]
            rc = _lib.lib.qc_fidelity_create_desc(C.byref(d), C.byref(self._h))
            del keep
        else:   # "ket": state psi~ (2N);  "density": state rho~ (2N^2) against the pure goal |psi_goal><psi_goal|
            if subspace is not None or phase_operators is not None or form != "abs":
                raise ValueError("subspace, form and free phases apply to unitary fidelities only")
            if goal_iso.size % 2:
                raise ValueError("the goal ket must be an iso-vec [Re psi; Im psi]")
            self.N = goal_iso.size // 2
            self.s = 2 * self.N if kind == "ket" else 2 * self.N * self.N
            rc = _lib.lib.qc_fidelity_create_kind(_lib.QC_FID_KET if kind == "ket" else _lib.QC_FID_DENSITY, self.N, _lib.dptr(goal_iso),
                                                  device, C.byref(self._h))
        _lib.check_rc(rc, "qc_fidelity_last_error")
        self.P = self.s + self.K          # input length: [state ; free phases]

    def eval(self, u: np.ndarray, grad: bool = True, hess: bool = True):
        u = np.ascontiguousarray(u, dtype=np.float64)
        if u.size != self.P:
            raise ValueError(f"input has length {u.size}, expected {self.P} (state{' + phases' if self.K else ''})")
        F, L = C.c_double(), C.c_double()
        g = np.empty(self.P) if grad else None
        H = np.empty(self.P * (self.P + 1) // 2) if hess else None
        rc = _lib.lib.qc_fidelity_eval(self._h, _lib.dptr(u), C.byref(F), C.byref(L), _lib.dptr(g) if grad else None,
                                       _lib.dptr(H) if hess else None)
        _lib.check_rc(rc, "qc_fidelity_last_error", self._h)
        return F.value, L.value, g, H

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib.qc_fidelity_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def iso_vec_unitary_fidelity(U_T: np.ndarray, U_G: np.ndarray, subspace: Optional[Sequence[int]] = None, device: int = 0,
                             form: str = "abs") -> float:
    """`form`: "abs" = |tr(U_G' U_T)| / n (the reference's docstring), "abs2" = |tr|^2 / n^2 (INTEGRATION.md, table of choices)."""
    f = _Fidelity(U_G, subspace, device, form=form)
    try:
        return f.eval(U_T, grad=False, hess=False)[0]
    finally:
        f.close()


def iso_vec_unitary_free_phase_fidelity(U_T: np.ndarray, U_G: np.ndarray, phases, phase_operators, subspace=None, device: int = 0,
                                        form: str = "abs") -> float:
    """|tr(U_G' R(phi) U_T)| / n with R(phi) = kron_k exp(i phi_k Op_k) (reference unitary_minimum_time_problem.jl:86-90)."""
    f = _Fidelity(U_G, subspace, device, form=form, phase_operators=phase_operators)
    try:
        return f.eval(np.concatenate([np.asarray(U_T, dtype=np.float64), np.asarray(phases, dtype=np.float64).ravel()]),
                      grad=False, hess=False)[0]
    finally:
        f.close()


class _FinalKnotTerm:
    _ALIASES = {}
    _KIND = "unitary"

    def __init__(self, state_name: str, traj: NamedTrajectory, subspace, device, goal=None, form: str = "abs",
                 phase_name: Optional[str] = None, phase_operators=None):
        self.traj = traj
        self.s = len(traj.components[state_name])
        self.first = (traj.T - 1) * traj.dim + traj.offset(state_name)     # 0-based global index of the final state
        goal = traj.goal.get(state_name) if goal is None else goal
        if goal is None:
            raise ValueError(f"trajectory has no goal for {state_name}")
        self._f = _Fidelity(np.asarray(goal, dtype=np.float64), subspace, device, kind=type(self)._KIND, form=form,
                            phase_operators=phase_operators)
        if self._f.s != self.s:
            raise ValueError(f"component {state_name} has length {self.s}, the goal implies {self._f.s}")
        idx = np.arange(self.first, self.first + self.s)
        if self._f.K:
            # the free phases are global variables behind the knots: Z = [vec(data) ; global_data...]  (trajectory_initialization.jl:370-380)
            off = traj.T * traj.dim
            for name, v in traj.global_data.items():
                if name == phase_name:
                    break
                off += v.size
            else:
                raise ValueError(f"trajectory has no global component {phase_name}")
            if traj.global_data[phase_name].size != self._f.K:
                raise ValueError("one phase per phase operator")
            idx = np.concatenate([idx, np.arange(off, off + self._f.K)])
        self.state_indices = idx           # variables of the term: the final state (and the free phases)
        P = idx.size
        r, c = np.triu_indices(P)
        # column-major upper triangle: entry (i <= j) at j(j+1)/2 + i
        order = np.lexsort((r, c))
        self.hess_structure = (idx[r[order]], idx[c[order]])

    def _u(self, Z):
        Z = np.asarray(Z, dtype=np.float64)
        return Z[self.state_indices]

    def __getattr__(self, name):
        al = type(self)._ALIASES
        if name in al:
            return getattr(self, al[name])
        raise AttributeError(name)

    def close(self):
        self._f.close()


class UnitaryInfidelityObjective(_FinalKnotTerm):
    """Q * |1 - F(U~_T)|.  `L(Z)`, `grad_L(Z)` (values on `state_indices`), `hess_L(Z)` (values on `hess_structure`);
    `getattr(obj, "∇L")` / `"∂²L"` resolve to the same members."""
    _ALIASES = {"∇L": "grad_L", "∂²L": "hess_L", "∂²L_structure": "hess_structure"}

    def __init__(self, state_name: str, traj: NamedTrajectory, Q: float = 100.0, subspace=None, device: int = 0, form: str = "abs"):
        super().__init__(state_name, traj, subspace, device, form=form)
        self.Q = float(Q)

    def L(self, Z) -> float:
        return self.Q * self._f.eval(self._u(Z), grad=False, hess=False)[1]

    def grad_L(self, Z) -> np.ndarray:
        F, _, g, _ = self._f.eval(self._u(Z), grad=True, hess=False)
        return -np.sign(1.0 - F) * self.Q * g if F != 1.0 else -self.Q * g

    def hess_L(self, Z) -> np.ndarray:
        F, _, _, H = self._f.eval(self._u(Z), grad=False, hess=True)
        return -(1.0 if 1.0 - F >= 0 else -1.0) * self.Q * H


class FinalUnitaryFidelityConstraint(_FinalKnotTerm):
    """g(Z) = F(U~_T) - value >= 0 (one row).  `g`, `dg` (values on `state_indices`), `mu_d2g(Z, mu)`."""
    _ALIASES = {"∂g": "dg", "μ∂²g": "mu_d2g", "μ∂²g_structure": "hess_structure"}

    def __init__(self, state_name: str, value: float, traj: NamedTrajectory, subspace=None, device: int = 0, form: str = "abs"):
        super().__init__(state_name, traj, subspace, device, form=form)
        self.value = float(value)
        self.dim = 1

    def g(self, Z) -> np.ndarray:
        return np.array([self._f.eval(self._u(Z), grad=False, hess=False)[0] - self.value])

    def dg(self, Z) -> np.ndarray:
        return self._f.eval(self._u(Z), grad=True, hess=False)[2]

    def mu_d2g(self, Z, mu) -> np.ndarray:
        return float(np.asarray(mu).ravel()[0]) * self._f.eval(self._u(Z), grad=False, hess=True)[3]


class UnitaryFreePhaseInfidelityObjective(UnitaryInfidelityObjective):
    """Q * |1 - F(U~_T, phi)| with free phases (reference unitary_smooth_pulse_problem.jl:138-143): variables = the final state
    and the K global phases `traj.global_data[phase_name]`."""

    def __init__(self, state_name: str, phase_name: str, phase_operators, traj: NamedTrajectory, Q: float = 100.0, subspace=None,
                 device: int = 0, form: str = "abs"):
        _FinalKnotTerm.__init__(self, state_name, traj, subspace, device, form=form, phase_name=phase_name, phase_operators=phase_operators)
        self.Q = float(Q)


class FinalUnitaryFreePhaseFidelityConstraint(FinalUnitaryFidelityConstraint):
    """g(Z) = F(U~_T, phi) - value >= 0 (reference unitary_minimum_time_problem.jl:95-100)."""

    def __init__(self, state_name: str, phase_name: str, phase_operators, value: float, traj: NamedTrajectory, subspace=None,
                 device: int = 0, form: str = "abs"):
        _FinalKnotTerm.__init__(self, state_name, traj, subspace, device, form=form, phase_name=phase_name, phase_operators=phase_operators)
        self.value = float(value)
        self.dim = 1


def iso_fidelity(psi_iso: np.ndarray, psi_goal_iso: np.ndarray, device: int = 0) -> float:
    """|<psi_goal|psi>|^2 on ket iso-vecs (reference quantum_state_minimum_time_problem.jl:50)."""
    f = _Fidelity(psi_goal_iso, None, device, kind="ket")
    try:
        return f.eval(psi_iso, grad=False, hess=False)[0]
    finally:
        f.close()


class QuantumStateObjective(UnitaryInfidelityObjective):
    """Q * |1 - |<psi_goal|psi_T>|^2| on the final ket (reference quantum_state_smooth_pulse_problem.jl:133)."""
    _KIND = "ket"

    def __init__(self, state_name: str, traj: NamedTrajectory, Q: float = 100.0, device: int = 0):
        _FinalKnotTerm.__init__(self, state_name, traj, None, device)
        self.Q = float(Q)


class FinalQuantumStateFidelityConstraint(FinalUnitaryFidelityConstraint):
    """g(Z) = |<psi_goal|psi_T>|^2 - value >= 0 (reference quantum_state_minimum_time_problem.jl:55-62)."""
    _KIND = "ket"

    def __init__(self, state_name: str, value: float, traj: NamedTrajectory, device: int = 0):
        _FinalKnotTerm.__init__(self, state_name, traj, None, device)
        self.value = float(value)
        self.dim = 1


class DensityOperatorPureStateInfidelityObjective(UnitaryInfidelityObjective):
    """Q * |1 - psi_goal' rho_T psi_goal| on the final density iso-vec (reference density_operator_smooth_pulse_problem.jl:55)."""
    _KIND = "density"

    def __init__(self, state_name: str, psi_goal: np.ndarray, traj: NamedTrajectory, Q: float = 100.0, device: int = 0):
        psi_goal = np.asarray(psi_goal, dtype=complex)
        _FinalKnotTerm.__init__(self, state_name, traj, None, device, goal=np.concatenate([psi_goal.real, psi_goal.imag]))
        self.Q = float(Q)


# ---------------------------------------------------------------------------------------------------------------
#  Whole-trajectory cost terms through `qc_terms_*`
# ---------------------------------------------------------------------------------------------------------------
class QuadraticRegularizer:
    """`QuadraticRegularizer(name, traj, R; baseline, timestep_name)` (reference call sites
    unitary_smooth_pulse_problem.jl:151-153): 1/2 sum_t sum_i R_i (dt_t (x_ti - b_ti))^2.  A description only; add it
    to a `TrajectoryObjective` to evaluate it."""

    def __init__(self, name: str, traj: NamedTrajectory, R, baseline: Optional[np.ndarray] = None, timestep_name: Optional[str] = None):
        self.name = name
        self.dim = len(traj.components[name])
        R = np.asarray(R, dtype=np.float64)
        self.R = np.full(self.dim, float(R)) if R.ndim == 0 else R.copy()
        if self.R.shape != (self.dim,):
            raise ValueError(f"R has shape {self.R.shape}, expected ({self.dim},)")
        self.baseline = None if baseline is None else np.asarray(baseline, dtype=np.float64).reshape(self.dim, traj.T)
        self.timestep_name = timestep_name if timestep_name is not None else (traj.timestep if isinstance(traj.timestep, str) else None)

    def __add__(self, other):
        return TrajectoryObjectiveSpec([self]) + other


class MinimumTimeObjective:
    """`MinimumTimeObjective(traj; D)` (reference unitary_minimum_time_problem.jl:67-69): D * sum_{t=1}^{T-1} dt_t."""

    def __init__(self, traj: NamedTrajectory, D: float = 1.0, timestep_name: Optional[str] = None):
        self.D = float(D)
        self.timestep_name = timestep_name if timestep_name is not None else traj.timestep
        if not isinstance(self.timestep_name, str):
            raise ValueError("a minimum-time objective needs a free timestep component")

    def __add__(self, other):
        return TrajectoryObjectiveSpec([self]) + other


class QuadraticSmoothnessRegularizer:
    """`QuadraticSmoothnessRegularizer(name, traj, R)` (reference test "Additional Objective",
    unitary_smooth_pulse_problem.jl:311-340): 1/2 sum_{t<T-1} sum_i R_i (x_{t+1,i} - x_{t,i})^2, no timestep inside the square.
    A description only; add it to a `TrajectoryObjective` to evaluate it."""

    def __init__(self, name: str, traj: NamedTrajectory, R):
        self.name = name
        self.dim = len(traj.components[name])
        R = np.asarray(R, dtype=np.float64)
        self.R = np.full(self.dim, float(R)) if R.ndim == 0 else R.copy()
        if self.R.shape != (self.dim,):
            raise ValueError(f"R has shape {self.R.shape}, expected ({self.dim},)")

    def __add__(self, other):
        return TrajectoryObjectiveSpec([self]) + other


class PairwiseQuadraticRegularizer:
    """`PairwiseQuadraticRegularizer(traj, Q, graph)` (reference unitary_direct_sum_problem.jl:130-169): for every edge
    (A, B) of `graph`, two components of equal length, sum_t 1/2 Q_e sc_t^2 ||x_t[A] - x_t[B]||^2 with the weighting of the
    quadratic regulariser.  `Q` is a scalar or one value per edge.  A description only."""

    def __init__(self, traj: NamedTrajectory, Q, graph):
        self.graph = [(str(a), str(b)) for a, b in graph]
        Q = np.asarray(Q, dtype=np.float64)
        self.Q = np.full(len(self.graph), float(Q)) if Q.ndim == 0 else Q.copy()
        if self.Q.shape != (len(self.graph),):
            raise ValueError(f"Q has shape {self.Q.shape}, expected one value per edge ({len(self.graph)},)")
        for a, b in self.graph:
            if len(traj.components[a]) != len(traj.components[b]):
                raise ValueError(f"edge ({a}, {b}): the components differ in length")

    def pairs(self, traj: NamedTrajectory):
        """(a, b, Q): the edges flattened into scalar pairs of knot offsets, edge after edge."""
        a = [np.asarray(traj.components[x]) for x, _ in self.graph]
        b = [np.asarray(traj.components[y]) for _, y in self.graph]
        Q = [np.full(len(ai), q) for ai, q in zip(a, self.Q)]
        cat = lambda v, dt: np.concatenate(v).astype(dt) if v else np.zeros(0, dtype=dt)
        return cat(a, np.int32), cat(b, np.int32), cat(Q, np.float64)

    def __add__(self, other):
        return TrajectoryObjectiveSpec([self]) + other


def slack_names(name: str):
    """Names of the two slack components of `L1Regularizer!` on component `name` (a choice of this build: QuantumCollocationCore,
    which names them, is not vendored; INTEGRATION.md, table of choices)."""
    return f"s1_{name}", f"s2_{name}"


class L1Regularizer:
    """The cost of `L1Regularizer!(constraints, name, traj; R_value, indices)` (reference _problem_templates.jl:41-54):
    sum_t sum_i R_i (s1_{t,i} + s2_{t,i}) over the two slack components of `name` (`slack_names(name)`), which the problem
    templates add to the trajectory.  Linear: constant gradient, no Hessian.  The slack rows are `L1SlackConstraint`; the bounds
    s >= 0 stay with the solver.  A description only."""

    def __init__(self, name: str, traj: NamedTrajectory, R):
        self.name = name
        self.slacks = slack_names(name)
        self.dim = len(traj.components[self.slacks[0]])
        if len(traj.components[self.slacks[1]]) != self.dim:
            raise ValueError("the two slack components differ in length")
        R = np.asarray(R, dtype=np.float64)
        self.R = np.full(self.dim, float(R)) if R.ndim == 0 else R.copy()
        if self.R.shape != (self.dim,):
            raise ValueError(f"R has shape {self.R.shape}, expected ({self.dim},)")

    def __add__(self, other):
        return TrajectoryObjectiveSpec([self]) + other


class L1SlackConstraint:
    """The slack rows of `L1Regularizer!` (reference _problem_templates.jl:41-54): x_t[i_k] - s1_t[k] + s2_t[k] = 0 for every knot
    t and every entry i_k of `indices` (offsets inside component `name`; default: all of it), knot-major.  Linear with a constant
    Jacobian (+1, -1, +1), no Hessian: described on the host, like `TimeStepsAllEqualConstraint`."""

    def __init__(self, name: str, traj: NamedTrajectory, indices=None):
        comp = np.asarray(traj.components[name])
        idx = np.arange(comp.size) if indices is None else np.asarray(indices, dtype=np.int64)
        s1, s2 = (np.asarray(traj.components[n]) for n in slack_names(name))
        if s1.size != idx.size or s2.size != idx.size:
            raise ValueError(f"the slack components of {name} must have one entry per index ({idx.size})")
        n = idx.size
        self.dim = traj.T * n
        t = np.repeat(np.arange(traj.T, dtype=np.int64) * traj.dim, n)
        self.x_indices = t + np.tile(comp[idx], traj.T)
        self.s1_indices = t + np.tile(s1, traj.T)
        self.s2_indices = t + np.tile(s2, traj.T)
        rows = np.repeat(np.arange(self.dim, dtype=np.int64), 3)
        cols = np.stack([self.x_indices, self.s1_indices, self.s2_indices], axis=1).ravel()
        self.jac_structure = (rows, cols)
        self.jac_values = np.tile([1.0, -1.0, 1.0], self.dim)

    def g(self, Z) -> np.ndarray:
        Z = np.asarray(Z, dtype=np.float64)
        return Z[self.x_indices] - Z[self.s1_indices] + Z[self.s2_indices]

    def dg(self, Z=None) -> np.ndarray:
        return self.jac_values


_EXT_TERMS = (QuadraticSmoothnessRegularizer, PairwiseQuadraticRegularizer, L1Regularizer)


class TrajectoryObjectiveSpec:
    def __init__(self, terms):
        self.terms = list(terms)

    def __add__(self, other):
        more = other.terms if isinstance(other, TrajectoryObjectiveSpec) else [other]
        return TrajectoryObjectiveSpec(self.terms + list(more))


class TrajectoryObjective:
    """Sum of `QuadraticRegularizer` / `MinimumTimeObjective` / `QuadraticSmoothnessRegularizer` /
    `PairwiseQuadraticRegularizer` / `L1Regularizer` terms evaluated in one pass over the knots on the GPU.
    `L(Z)`, `grad_L(Z)` (dense, length `len(Z)`), `hess_L(Z)` (values on `hess_structure`); `"∇L"`, `"∂²L"`,
    `"∂²L_structure"` resolve to the same members."""
    _ALIASES = {"∇L": "grad_L", "∂²L": "hess_L", "∂²L_structure": "hess_structure"}

    def __init__(self, terms, traj: NamedTrajectory, dt_scaled: bool = True, device: int = 0):
        """dt_scaled=True (default): 1/2 sum_t R (dt_t x_t)^2, the weighting the templates' `timestep_name=` argument implies
        (unitary_smooth_pulse_problem.jl:151-153); False: the docstring's 1/2 sum_t R x_t^2 (QC_REG_PLAIN)."""
        if isinstance(terms, TrajectoryObjectiveSpec):
            terms = terms.terms
        elif isinstance(terms, (QuadraticRegularizer, MinimumTimeObjective) + _EXT_TERMS):
            terms = [terms]
        self.traj = traj
        w = np.zeros(traj.dim)
        used = np.zeros(traj.dim, dtype=bool)
        base = np.zeros((traj.dim, traj.T))
        any_base = False
        D = 0.0
        ts_names = set()
        ws, used_s = np.zeros(traj.dim), np.zeros(traj.dim, dtype=bool)
        wl, used_l = np.zeros(traj.dim), np.zeros(traj.dim, dtype=bool)
        pairs = []
        for term in terms:
            if isinstance(term, QuadraticRegularizer):
                idx = np.asarray(traj.components[term.name])
                w[idx] += term.R
                if term.baseline is not None:
                    if used[idx].any():
                        raise ValueError(f"{term.name}: a baseline cannot be combined with another regulariser on the same component")
                    base[idx, :] = term.baseline
                    any_base = True
                used[idx] = True
                if term.timestep_name is not None:
                    ts_names.add(term.timestep_name)
            elif isinstance(term, MinimumTimeObjective):
                D += term.D
                ts_names.add(term.timestep_name)
            elif isinstance(term, QuadraticSmoothnessRegularizer):
                idx = np.asarray(traj.components[term.name])
                ws[idx] += term.R
                used_s[idx] = True
            elif isinstance(term, PairwiseQuadraticRegularizer):
                pairs.append(term.pairs(traj))
            elif isinstance(term, L1Regularizer):
                for nm in term.slacks:
                    idx = np.asarray(traj.components[nm])
                    wl[idx] += term.R
                    used_l[idx] = True
            else:
                raise TypeError(f"unsupported term {type(term).__name__}")
        if len(ts_names) > 1:
            raise ValueError(f"terms disagree on the timestep component: {sorted(ts_names)}")
        free = isinstance(traj.timestep, str)
        self._index = np.ascontiguousarray(np.nonzero(used)[0], dtype=np.int32)
        self._R = np.ascontiguousarray(w[self._index])
        self._base = np.ascontiguousarray(base[self._index, :].T) if any_base else None      # (T, n_reg): entry-fastest
        d = _lib.qc_terms_desc()
        d.T = traj.T
        d.zdim = traj.dim
        d.off_dt = traj.offset(traj.timestep) if free else -1
        d.global_dim = traj.global_dim
        d.dt_fixed = 0.0 if free else float(traj.timestep)
        d.n_reg = self._index.size
        d.weighting = _lib.QC_REG_DT_SCALED if dt_scaled else _lib.QC_REG_PLAIN
        d.reg_index = self._index.ctypes.data_as(C.POINTER(C.c_int32))
        d.reg_R = _lib.dptr(self._R) if self._R.size else None
        d.reg_baseline = _lib.dptr(self._base) if self._base is not None else None
        d.min_time_D = D
        d.min_time_knots = traj.T - 1 if D != 0.0 else 0
        d.device = device
        self._desc = d
        self._s_index = np.ascontiguousarray(np.nonzero(used_s)[0], dtype=np.int32)
        self._s_R = np.ascontiguousarray(ws[self._s_index])
        self._l_index = np.ascontiguousarray(np.nonzero(used_l)[0], dtype=np.int32)
        self._l_w = np.ascontiguousarray(wl[self._l_index])
        cat = lambda k, dt: np.ascontiguousarray(np.concatenate([p[k] for p in pairs]) if pairs else np.zeros(0), dtype=dt)
        self._p_a, self._p_b, self._p_Q = cat(0, np.int32), cat(1, np.int32), cat(2, np.float64)
        self.has_ext = bool(self._s_index.size or self._l_index.size or self._p_a.size)
        self._ext = None
        if self.has_ext:
            x = _lib.qc_terms_ext()
            x.n_smooth, x.n_pair, x.n_lin = self._s_index.size, self._p_a.size, self._l_index.size
            ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)) if a.size else None
            dp = lambda a: _lib.dptr(a) if a.size else None
            x.smooth_index, x.smooth_R = ip(self._s_index), dp(self._s_R)
            x.pair_a, x.pair_b, x.pair_Q = ip(self._p_a), ip(self._p_b), dp(self._p_Q)
            x.lin_index, x.lin_w = ip(self._l_index), dp(self._l_w)
            self._ext = x
        self.Z_len = traj.T * traj.dim + traj.global_dim
        self._h = C.c_void_p()
        if self.has_ext:
            rc = _lib.lib.qc_terms_create_ext(C.byref(d), C.byref(self._ext), C.byref(self._h))
        else:
            rc = _lib.lib.qc_terms_create(C.byref(d), C.byref(self._h))
        _lib.check_rc(rc, "qc_terms_last_error")
        nnz = C.c_int64()
        _lib.lib.qc_terms_hess_nnz(self._h, C.byref(nnz))
        self.hess_nnz = nnz.value
        r = np.empty(self.hess_nnz, dtype=np.int64)
        c = np.empty(self.hess_nnz, dtype=np.int64)
        _lib.lib.qc_terms_hess_structure(self._h, _lib.iptr(r), _lib.iptr(c), 0)
        self.hess_structure = (r, c)

    def _eval(self, Z, grad: bool, hess: bool):
        Z = np.ascontiguousarray(Z, dtype=np.float64)
        if Z.size != self.Z_len:
            raise ValueError(f"Z has length {Z.size}, expected {self.Z_len}")
        J = C.c_double()
        g = np.empty(self.Z_len) if grad else None
        H = np.empty(self.hess_nnz) if hess else None
        rc = _lib.lib.qc_terms_eval(self._h, _lib.dptr(Z), C.byref(J), _lib.dptr(g) if grad else None, _lib.dptr(H) if hess else None)
        _lib.check_rc(rc, "qc_terms_last_error", self._h)
        return J.value, g, H

    def L(self, Z) -> float:
        return self._eval(Z, False, False)[0]

    def grad_L(self, Z) -> np.ndarray:
        return self._eval(Z, True, False)[1]

    def hess_L(self, Z) -> np.ndarray:
        return self._eval(Z, False, True)[2]

    def L_grad_hess(self, Z):
        return self._eval(Z, True, True)

    def eval_device(self, dZ, dJ, dgrad=None, dhess=None, stream=None):
        """Device-resident evaluation on torch CUDA tensors (float64), asynchronous on `stream`."""
        s = stream.cuda_stream if stream is not None else torch.cuda.current_stream().cuda_stream
        rc = _lib.lib.qc_terms_eval_dev(self._h, dZ.data_ptr(), dJ.data_ptr(), dgrad.data_ptr() if dgrad is not None else None,
                                        dhess.data_ptr() if dhess is not None else None, s)
        _lib.check_rc(rc, "qc_terms_last_error", self._h)

    def __getattr__(self, name):
        al = type(self)._ALIASES
        if name in al:
            return getattr(self, al[name])
        raise AttributeError(name)

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib.qc_terms_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TimeStepsAllEqualConstraint:
    """`TimeStepsAllEqualConstraint(timestep_name, traj)` (reference _problem_templates.jl:57-63): the T-1 linear rows
    dt_t - dt_T = 0.  Constant Jacobian (+1, -1), no Hessian: nothing to evaluate on a device; provided so that the
    whole constraint set of a problem template can be described on this side of the boundary."""

    def __init__(self, timestep_name: str, traj: NamedTrajectory):
        off = traj.offset(timestep_name)
        self.dim = traj.T - 1
        self.indices = np.arange(traj.T, dtype=np.int64) * traj.dim + off
        rows = np.repeat(np.arange(self.dim, dtype=np.int64), 2)
        cols = np.stack([self.indices[:-1], np.full(self.dim, self.indices[-1])], axis=1).ravel()
        self.jac_structure = (rows, cols)
        self.jac_values = np.tile([1.0, -1.0], self.dim)

    def g(self, Z) -> np.ndarray:
        Z = np.asarray(Z, dtype=np.float64)
        return Z[self.indices[:-1]] - Z[self.indices[-1]]

    def dg(self, Z=None) -> np.ndarray:
        return self.jac_values


# ---------------------------------------------------------------------------------------------------------------
#  UnitaryRobustnessObjective (reference unitary_robustness_problem.jl:46-49) through `qc_robust_*`
# ---------------------------------------------------------------------------------------------------------------
class UnitaryRobustnessObjective:
    """L = Re tr(R'R) / n,  R = (1/tau) sum_{t<K} dt_t V_t' H V_t,  V_t = U_t[S, S],  tau = sum_{t<K} dt_t: how strongly the error
    operator H (`unembed(H_error)`) survives, averaged over the trajectory in the toggling frame.  `L(Z)`, `grad_L(Z)` (dense,
    length `len(Z)`), `hess_L(Z)` (values on `hess_structure`: the dense upper triangle over `variables`, column-major),
    `L_grad_hess(Z)`, `eval_device(...)`; `"∇L"`, `"∂²L"`, `"∂²L_structure"` resolve to the same members.

    H_error   N x N array (subspace = None: all levels; otherwise its [S, S] block is used) or an `EmbeddedOperator`
              (its `unembed()` and `subspace`)
    knots     K, the knots that enter the sum (default: all T)
    """
    _ALIASES = {"∇L": "grad_L", "∂²L": "hess_L", "∂²L_structure": "hess_structure"}

    def __init__(self, traj: NamedTrajectory, H_error=None, eval_hessian: bool = True, symb: str = "Ũ⃗", subspace=None,
                 knots: Optional[int] = None, device: int = 0):
        from .gates import EmbeddedOperator
        if H_error is None:
            raise ValueError("H_error is required")
        s = len(traj.components[symb])
        N = int(round((s / 2) ** 0.5))
        if 2 * N * N != s:
            raise ValueError(f"component {symb} has length {s}, not 2 N^2")
        if isinstance(H_error, EmbeddedOperator):
            if H_error.N != N:
                raise ValueError(f"H_error is embedded in {H_error.N} levels, the trajectory's unitary has {N}")
            if subspace is not None and list(subspace) != H_error.subspace:
                raise ValueError("subspace differs from H_error.subspace")
            H, sub = H_error.unembed(), H_error.subspace
        else:
            H = np.asarray(H_error, dtype=complex)
            sub = None if subspace is None else [int(x) for x in subspace]
            if sub is not None and H.shape == (N, N):
                H = H[np.ix_(sub, sub)]
        n = N if sub is None else len(sub)
        if H.shape != (n, n):
            raise ValueError(f"H_error has shape {H.shape}, expected ({n}, {n}) or ({N}, {N})")
        self.traj = traj
        self.H = H
        self.subspace = sub
        self.eval_hessian = bool(eval_hessian)
        free = isinstance(traj.timestep, str)
        self._Hre = np.ascontiguousarray(H.real.reshape(-1, order="F"))
        self._Him = np.ascontiguousarray(H.imag.reshape(-1, order="F"))
        self._sub = None if sub is None else np.ascontiguousarray(sub, dtype=np.int32)
        d = _lib.qc_robust_desc()
        d.T = traj.T
        d.zdim = traj.dim
        d.off_state = traj.offset(symb)
        d.N = N
        d.n_sub = 0 if sub is None else len(sub)
        d.subspace = None if sub is None else self._sub.ctypes.data_as(C.POINTER(C.c_int32))
        d.H_re = _lib.dptr(self._Hre)
        d.H_im = _lib.dptr(self._Him)
        d.off_dt = traj.offset(traj.timestep) if free else -1
        d.dt_fixed = 0.0 if free else float(traj.timestep)
        d.global_dim = traj.global_dim
        d.n_knots = traj.T if knots is None else int(knots)
        d.hessian = _lib.QC_ROBUST_HESS_EXACT if eval_hessian else _lib.QC_ROBUST_HESS_NONE
        d.device = device
        self._desc = d
        self.Z_len = traj.T * traj.dim + traj.global_dim
        self._h = C.c_void_p()
        rc = _lib.lib.qc_robust_create(C.byref(d), C.byref(self._h))
        _lib.check_rc(rc, "qc_robust_last_error")
        v = C.c_int64()
        _lib.lib.qc_robust_n_vars(self._h, C.byref(v))
        self.n_vars = v.value
        self.variables = np.empty(self.n_vars, dtype=np.int64)
        _lib.lib.qc_robust_vars(self._h, _lib.iptr(self.variables))
        _lib.lib.qc_robust_hess_nnz(self._h, C.byref(v))
        self.hess_nnz = v.value
        self._structure = None

    @property
    def hess_structure(self):
        """(rows, cols) of the Hessian values: the upper triangle over `variables`, entry (i <= j) at j(j+1)/2 + i; empty
        with eval_hessian=False.  Built on first use (V(V+1)/2 entries)."""
        if self._structure is None:
            r = np.empty(self.hess_nnz, dtype=np.int64)
            c = np.empty(self.hess_nnz, dtype=np.int64)
            rc = _lib.lib.qc_robust_hess_structure(self._h, _lib.iptr(r), _lib.iptr(c), 0)
            _lib.check_rc(rc, "qc_robust_last_error", self._h)
            self._structure = (r, c)
        return self._structure

    def _eval(self, Z, grad: bool, hess: bool):
        Z = np.ascontiguousarray(Z, dtype=np.float64)
        if Z.size != self.Z_len:
            raise ValueError(f"Z has length {Z.size}, expected {self.Z_len}")
        if hess and not self.eval_hessian:
            raise RuntimeError("the objective was built with eval_hessian=False")
        L = C.c_double()
        g = np.empty(self.Z_len) if grad else None
        H = np.empty(self.hess_nnz) if hess else None
        rc = _lib.lib.qc_robust_eval(self._h, _lib.dptr(Z), C.byref(L), _lib.dptr(g) if grad else None,
                                     _lib.dptr(H) if hess and self.hess_nnz else None)
        _lib.check_rc(rc, "qc_robust_last_error", self._h)
        return L.value, g, H

    def L(self, Z) -> float:
        return self._eval(Z, False, False)[0]

    def grad_L(self, Z) -> np.ndarray:
        return self._eval(Z, True, False)[1]

    def hess_L(self, Z) -> np.ndarray:
        return self._eval(Z, False, True)[2]

    def L_grad_hess(self, Z):
        return self._eval(Z, True, self.eval_hessian)

    def eval_device(self, dZ, dL, dgrad=None, dhess=None, stream=None):
        """Device-resident evaluation on torch CUDA tensors (float64), asynchronous on `stream`; dL holds one double."""
        s = stream.cuda_stream if stream is not None else torch.cuda.current_stream().cuda_stream
        rc = _lib.lib.qc_robust_eval_dev(self._h, dZ.data_ptr(), dL.data_ptr() if dL is not None else None,
                                         dgrad.data_ptr() if dgrad is not None else None, dhess.data_ptr() if dhess is not None else None, s)
        _lib.check_rc(rc, "qc_robust_last_error", self._h)

    def __getattr__(self, name):
        al = type(self)._ALIASES
        if name in al:
            return getattr(self, al[name])
        raise AttributeError(name)

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib.qc_robust_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SweepInfidelityObjective:
    """L(Z) = 1 - sum_s w_s F_s: the mean (weighted) infidelity of the trajectory's pulse over S perturbed systems

        G_s(a) = G_drift + sum_j theta[s, j] P_j + sum_k scale[s, k] a_k G_k,

    each F_s the fidelity of the rollout from the trajectory's initial state to its goal (`RolloutSweep.grad`: one adjoint sweep per
    gradient, whatever the number of drives).  `L(Z)`, `grad_L(Z)` (dense, length `len(Z)`; only the controls and timesteps carry
    entries).  First order only: `hess_structure` is empty and `hess_L` raises, so the term belongs in a
    `QuantumControlEvaluator(eval_hessian=False)`.  The layout comes from the trajectory: `traj.dim`, the offsets of `control_name`
    and of the timestep, `traj.global_dim`.

    state_name  a unitary component (2 N^2 entries: unitary fidelity, `subspace`, `form`) or a ket component (2 N entries); with an
                `OpenQuantumSystem` the iso-vec of a density operator (2 levels^2 entries: the density fidelity <psi|rho|psi>)
    theta       S x len(perturbations);  scale  S x n_drives or None;  weights  S values or None (1/S each)
    wide        as `RolloutSweep`: True serves systems of 16 < 2N <= 32 (9 .. 16 levels) in the "mfma32-sweep" form
    stored_states  as `RolloutSweep`: True takes the gradient by the stored-state walk, which serves open systems
    wide_stored as `RolloutSweep` (only with `wide` and `stored_states`): that walk in the "mfma32-sweep" form, e.g. two qubits with T1 / T2
    wide_noise  as `RolloutSweep` (only with `wide`): what `SweepNoiseInfidelityObjective` needs in the "mfma32-sweep" form; nothing here reads it
    wide64, wide64_grad  as `RolloutSweep` (only with `wide`; `wide64_grad` only with `wide64`): all three True serve closed systems of
                32 < 2N <= 64 (17 .. 32 levels: three coupled transmons, 5 qubits) in the "mfma64-sweep" form
    wide64_params  as `RolloutSweep` (only with `wide64_grad`): the handle also serves `param_grad` and parameter cotangents there
    wide64_noise  as `RolloutSweep` (only with `wide64`): what `SweepNoiseInfidelityObjective` needs in the "mfma64-sweep" form; nothing here reads it
    wide64_stored  as `RolloutSweep` (only with `wide64_grad` and `stored_states`): the stored-state walk in the "mfma64-sweep" form, e.g. a
                five-level Lindblad model (N = 25) with `goal_ket`
    goal_ket    density component only: [Re psi; Im psi] (2 levels entries) of the pure state the fidelity compares with"""
    _ALIASES = {"∇L": "grad_L", "∂²L": "hess_L", "∂²L_structure": "hess_structure"}

    def __init__(self, traj: NamedTrajectory, system, perturbations, theta, scale=None, weights=None, state_name: str = "Ũ⃗",
                 control_name: str = "a", subspace=None, form: str = "abs", device: int = 0, wide: bool = False,
                 stored_states: bool = False, goal_ket=None, wide_stored: bool = False, wide_noise: bool = False, wide64_noise: bool = False,
                 wide64: bool = False, wide64_stored: bool = False, wide64_grad: bool = False, wide64_params: bool = False):
        from .rollouts import RolloutSweep
        self._sweep = None
        if state_name not in traj.components:
            raise ValueError(f"the trajectory has no component {state_name}")
        if control_name not in traj.components:
            raise ValueError(f"the trajectory has no component {control_name}")
        if form not in ("abs", "abs2"):
            raise ValueError("form must be 'abs' or 'abs2'")
        N, m = system.state_levels, system.n_drives
        if len(traj.components[control_name]) != m:
            raise ValueError(f"component {control_name} has {len(traj.components[control_name])} rows, the system has {m} drives")
        s = len(traj.components[state_name])
        is_open = system.state_levels != system.levels
        if is_open and s == 2 * N:
            kind, cols = "density", 1
        elif s == 2 * N * N and N > 1:
            kind, cols = "unitary", N
        elif s == 2 * N:
            kind, cols = "ket", 1
        else:
            raise ValueError(f"component {state_name} has length {s}: neither a unitary (2 N^2) nor a ket (2 N) of N = {N} levels")
        if kind != "unitary" and (subspace is not None or form != "abs"):
            raise ValueError("subspace and form apply to a unitary component only")
        if (goal_ket is not None) != (kind == "density"):
            raise ValueError("goal_ket ([Re psi; Im psi]) is given exactly when the component is a density operator of an OpenQuantumSystem")
        if kind == "density":
            goal = np.asarray(goal_ket, dtype=np.float64).ravel()
            if goal.size != 2 * system.levels:
                raise ValueError(f"goal_ket must have {2 * system.levels} entries")
        elif state_name not in traj.goal:
            raise ValueError(f"the trajectory has no goal for {state_name}")
        else:
            goal = np.asarray(traj.goal[state_name], dtype=np.float64)
        init = traj.initial.get(state_name)
        if init is None:
            init = traj[state_name][:, 0]
        from .rollouts import _sweep_samples
        self.S, self._theta, self._scale = _sweep_samples(len(perturbations), m, theta, scale)
        self._weights = None
        if weights is not None:
            self._weights = np.ascontiguousarray(weights, dtype=np.float64).ravel()
            if self._weights.size != self.S:
                raise ValueError(f"weights must have {self.S} entries")
        free = isinstance(traj.timestep, str)
        self.traj = traj
        self.Z_len = traj.T * traj.dim + traj.global_dim
        self._init = np.ascontiguousarray(init, dtype=np.float64).ravel()
        sw = RolloutSweep(system, perturbations, traj.T, cols=cols, goal=goal, fid_kind=kind,
                          subspace=subspace, fid_form=_lib.QC_FID_FORM_ABS2 if form == "abs2" else _lib.QC_FID_FORM_ABS, zdim=traj.dim,
                          off_a=traj.offset(control_name), off_dt=traj.offset(traj.timestep) if free else -1,
                          dt_fixed=None if free else float(traj.timestep), global_dim=traj.global_dim, device=device, wide=wide,
                          stored_states=stored_states, wide_stored=wide_stored, wide_noise=wide_noise, wide64=wide64, wide64_grad=wide64_grad,
                          wide64_params=wide64_params, wide64_noise=wide64_noise, wide64_stored=wide64_stored)
        self._sweep = sw
        self.stored_states = sw.stored_states
        self.wide_stored = sw.wide_stored
        if not sw.grad_supported:
            why = sw.grad_unsupported_reason
            sw.close()
            raise _lib.QCollocError(_lib.QC_ERR_UNSUPPORTED, why)
        self.hess_structure = (np.empty(0, dtype=np.int64), np.empty(0, dtype=np.int64))

    def J_fids_grad(self, Z):
        """(J, fids, dJ/dZ) of one adjoint sweep."""
        return self._sweep.grad(Z, self._init, self._theta, self._scale, self._weights)

    def fidelities(self, Z) -> np.ndarray:
        return self._sweep.eval(Z, self._init, self._theta, self._scale, finals=False)[1]

    def L(self, Z) -> float:
        f = self.fidelities(Z)
        w = np.full(self.S, 1.0 / self.S) if self._weights is None else self._weights
        return 1.0 - float(np.dot(w, f))

    def grad_L(self, Z) -> np.ndarray:
        return -self.J_fids_grad(Z)[2]

    def hess_L(self, Z):
        raise RuntimeError("SweepInfidelityObjective is first order: build the evaluator with eval_hessian=False")

    def __getattr__(self, name):
        al = type(self)._ALIASES
        if name in al:
            return getattr(self, al[name])
        raise AttributeError(name)

    def close(self):
        if getattr(self, "_sweep", None) is not None:
            self._sweep.close()
            self._sweep = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SweepNoiseInfidelityObjective(SweepInfidelityObjective):
    """L(Z) = 1 - sum_s w_s F_s over S noise realisations: `SweepInfidelityObjective` with perturbation amplitudes that change from
    interval to interval,

        G_{s,t} = G_drift + sum_j (theta[s, j] + noise[s, t, j]) P_j + sum_k scale[s, k] a_{t,k} G_k

    (`RolloutSweep.noise_eval` / `noise_grad`: one sweep per value, one adjoint sweep per gradient).  The realisations are fixed at
    construction (common random numbers: the same S noise trajectories at every iterate), so L is a smooth deterministic function of
    the pulse.  Interface and first-order rule of `SweepInfidelityObjective`.

    noise       S x (T-1) x len(perturbations), or S x (T-1) with one perturbation: it gives S
    theta       S x len(perturbations) or None (zeros);  scale  S x n_drives or None;  weights  S values or None (1/S each)
    wide, wide_noise  as `RolloutSweep`: both True serve systems of 16 < 2N <= 32 (two three-level transmons, a 4-qubit register) in the
                "mfma32-sweep" form, with up to 8 drives and 8 perturbations
    wide64, wide64_grad, wide64_noise  as `RolloutSweep` (only with `wide`): all four True serve closed systems of 32 < 2N <= 64 (three coupled
                three-level transmons, a 5-qubit register) in the "mfma64-sweep" form, with up to 16 drives and 8 perturbations
    `noise_sensitivity(Z)` returns dF_s/dnoise[s, t, j], S x (T-1) x len(perturbations): the time-domain filter function of the pulse."""

    def __init__(self, traj: NamedTrajectory, system, perturbations, noise, theta=None, scale=None, weights=None, state_name: str = "Ũ⃗",
                 control_name: str = "a", subspace=None, form: str = "abs", device: int = 0, wide: bool = False, wide_noise: bool = False,
                 wide64: bool = False, wide64_grad: bool = False, wide64_noise: bool = False):
        p = len(perturbations)
        if noise is None:
            raise ValueError("noise is required: S x (T-1) x len(perturbations)")
        noise = np.asarray(noise, dtype=np.float64)
        if noise.ndim == 2 and p == 1:
            noise = noise[:, :, None]
        if noise.ndim != 3 or noise.shape[0] < 1 or noise.shape[1:] != (traj.T - 1, p):
            raise ValueError(f"noise must be S x {traj.T - 1} x {p}")
        if theta is None:
            theta = np.zeros((noise.shape[0], p))
        super().__init__(traj, system, perturbations, theta, scale=scale, weights=weights, state_name=state_name, control_name=control_name,
                         subspace=subspace, form=form, device=device, wide=wide, wide_noise=wide_noise, wide64=wide64,
                         wide64_grad=wide64_grad, wide64_noise=wide64_noise)
        sw = self._sweep
        if self.S != noise.shape[0]:
            sw.close()
            raise ValueError(f"theta / scale give {self.S} samples, noise gives {noise.shape[0]}")
        if not sw.noise_supported:
            why = sw.noise_unsupported_reason
            sw.close()
            raise _lib.QCollocError(_lib.QC_ERR_UNSUPPORTED, why)
        self._noise = np.ascontiguousarray(noise)

    def J_fids_grad(self, Z):
        """(J, fids, dJ/dZ) of one adjoint sweep."""
        return self._sweep.noise_grad(Z, self._init, self._noise, self._theta, self._scale, self._weights)[:3]

    def fidelities(self, Z) -> np.ndarray:
        return self._sweep.noise_eval(Z, self._init, self._noise, self._theta, self._scale, finals=False)[1]

    def noise_sensitivity(self, Z) -> np.ndarray:
        """dF_s/dnoise[s, t, j], S x (T-1) x len(perturbations), raw per-sample values."""
        return self._sweep.noise_grad(Z, self._init, self._noise, self._theta, self._scale, self._weights)[3]


class SweepFinalStateObjective:
    """L(Z) = loss(X): any function, written in torch, of the final states of the trajectory's pulse over S perturbed systems (the
    systems of `SweepInfidelityObjective`).  X is the S x (2N cols) float64 device tensor of `RolloutSweep.finals_autograd`, row s the
    final state of sample s, column-major 2N x cols ([Re; Im] per column); `loss` maps it to a 0-dim tensor.  `L(Z)` evaluates it,
    `grad_L(Z)` (dense, length `len(Z)`) runs torch's backward through the sweep's pullback: one adjoint sweep per gradient.  First
    order only, as `SweepInfidelityObjective`: `hess_structure` is empty and `hess_L` raises.  Curvature is matrix-free:
    `gauss_newton_times(Z, v)` is the generalized Gauss-Newton product of the loss, one pushforward and one pullback of the sweep;
    `hessian_times(Z, v)` is the exact Hessian product, one pushforward and one tangent pullback (`RolloutSweep.hvp_device`).
    `L`, `grad_L`, `gauss_newton_times` and `hessian_times` also take Z (and v) as float64 tensors on the handle's device; `grad_L` and
    the two products then return device tensors, so an optimiser can keep the trajectory vector there.  numpy in, numpy out is
    unchanged.

    state_name  a unitary component (2 N^2 entries), a component of K kets (2 N K entries, the kets side by side) or a list of ket
                component names (stacked as columns in that order).  No goal is read: the loss carries whatever it compares with.
    theta       S x len(perturbations);  scale  S x n_drives or None
    wide        as `RolloutSweep`
    stored_states  as `RolloutSweep`: True takes the pullback by the stored-state walk, which serves open systems (gradients and
                `gauss_newton_times`; `hessian_times` keeps the scope of `RolloutSweep.hvp`)
    wide_stored as `RolloutSweep` (only with `wide` and `stored_states`): that walk in the "mfma32-sweep" form (gradients only, unless
                `wide_tangent` is set as well)
    wide_tangent  as `RolloutSweep` (only with `wide`): the pushforward in the "mfma32-sweep" form, so that `gauss_newton_times` is
                served there (closed systems, and open ones with `stored_states` and `wide_stored`)
    wide_hessian  as `RolloutSweep` (only with `wide`): the Hessian product in the "mfma32-sweep" form.  `hessian_times` there needs
                `wide_tangent` as well (one `jvp_device`, one `hvp_device`); with one of the two it raises the handle's reason
    wide64, wide64_grad  as `RolloutSweep` (only with `wide`; `wide64_grad` only with `wide64`): all three True serve closed systems of
                32 < 2N <= 64 in the "mfma64-sweep" form, gradients only (`gauss_newton_times` needs `wide64_tangent` as well;
                `hessian_times` raises the handle's reason)
    wide64_tangent  as `RolloutSweep` (only with `wide64`): the pushforward in the "mfma64-sweep" form, so that `gauss_newton_times` is
                served there beside the gradients of `wide64_grad` (2N x cols <= 2048); `hessian_times` still raises
    wide64_params  as `RolloutSweep` (only with `wide64_grad`): the handle also serves `param_grad` and parameter cotangents there
    wide64_stored  as `RolloutSweep` (only with `wide64_grad` and `stored_states`): the stored-state walk in the "mfma64-sweep" form, which
                serves open systems there (gradients; `gauss_newton_times` with `wide64_tangent` as well; `hessian_times` still raises)"""
    _ALIASES = {"∇L": "grad_L", "∂²L": "hess_L", "∂²L_structure": "hess_structure"}

    def __init__(self, traj: NamedTrajectory, system, perturbations, theta, loss, scale=None, state_name="Ũ⃗", control_name: str = "a",
                 device: int = 0, wide: bool = False, stored_states: bool = False, wide_stored: bool = False, wide_tangent: bool = False,
                 wide_hessian: bool = False, wide64: bool = False, wide64_stored: bool = False, wide64_grad: bool = False,
                 wide64_tangent: bool = False, wide64_params: bool = False):
        from .rollouts import RolloutSweep, _sweep_samples
        self._sweep = None
        if not callable(loss):
            raise ValueError("loss must be a callable from the S x (2N cols) tensor of final states to a 0-dim tensor")
        names = [state_name] if isinstance(state_name, str) else list(state_name)
        for name in names + [control_name]:
            if name not in traj.components:
                raise ValueError(f"the trajectory has no component {name}")
        N, m = system.state_levels, system.n_drives
        if len(traj.components[control_name]) != m:
            raise ValueError(f"component {control_name} has {len(traj.components[control_name])} rows, the system has {m} drives")
        cols, init = 0, []
        for name in names:
            s = len(traj.components[name])
            if s % (2 * N) or (len(names) > 1 and s != 2 * N):
                raise ValueError(f"component {name} has length {s}: " + ("not a ket (2 N)" if len(names) > 1 else "no multiple of 2 N") + f" of N = {N} levels")
            cols += s // (2 * N)
            x0 = traj.initial.get(name)
            init.append(np.asarray(traj[name][:, 0] if x0 is None else x0, dtype=np.float64).ravel())
        self.S, theta, scale = _sweep_samples(len(perturbations), m, theta, scale)
        free = isinstance(traj.timestep, str)
        self.traj, self.loss = traj, loss
        self.Z_len = traj.T * traj.dim + traj.global_dim
        sw = RolloutSweep(system, perturbations, traj.T, cols=cols, zdim=traj.dim, off_a=traj.offset(control_name),
                          off_dt=traj.offset(traj.timestep) if free else -1, dt_fixed=None if free else float(traj.timestep),
                          global_dim=traj.global_dim, device=device, wide=wide, stored_states=stored_states, wide_stored=wide_stored,
                          wide_tangent=wide_tangent, wide_hessian=wide_hessian, wide64=wide64, wide64_grad=wide64_grad,
                          wide64_tangent=wide64_tangent, wide64_params=wide64_params, wide64_stored=wide64_stored)
        self._sweep = sw
        self.wide_hessian = sw.wide_hessian
        self.stored_states = sw.stored_states
        self.wide_stored = sw.wide_stored
        self.wide_tangent = sw.wide_tangent
        if not sw.vjp_supported:
            why = sw.vjp_unsupported_reason
            sw.close()
            self._sweep = None
            raise _lib.QCollocError(_lib.QC_ERR_UNSUPPORTED, why)
        dev = torch.device("cuda", device)
        put = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self._dev = dev
        self._dinit, self._dtheta, self._dscale = put(np.concatenate(init)), put(theta), put(scale)
        if self._dtheta is None and self._dscale is None:      # samples without any parameter: S identical systems
            self._dtheta = torch.zeros((self.S, 0), dtype=torch.float64, device=dev)
        self.hess_structure = (np.empty(0, dtype=np.int64), np.empty(0, dtype=np.int64))

    def _loss(self, Z, grad: bool):
        on_device = torch.is_tensor(Z)      # a float64 tensor on the handle's device: the gradient stays there
        if not on_device:
            Z = np.ascontiguousarray(Z, dtype=np.float64).ravel()
        if (Z.numel() if on_device else Z.size) != self.Z_len:
            raise ValueError(f"Z has length {Z.numel() if on_device else Z.size}, expected {self.Z_len}")
        with torch.cuda.device(self._dev):
            dZ = (Z.detach().to(self._dev).reshape(-1).clone() if on_device else torch.from_numpy(Z).to(self._dev)).requires_grad_(grad)
            with torch.set_grad_enabled(grad):
                L = self.loss(self._sweep.finals_autograd(dZ, self._dinit, self._dtheta, self._dscale))
            if L.dim() != 0:
                raise ValueError("loss must return a 0-dim tensor")
            if not grad:
                return float(L), None
            L.backward()
            g = dZ.grad
            if on_device:
                return float(L.detach()), (torch.zeros_like(dZ.detach()) if g is None else g)
            return float(L.detach()), (np.zeros(self.Z_len) if g is None else g.cpu().numpy())

    def finals(self, Z) -> np.ndarray:
        """The S x (2N cols) final states the loss sees."""
        return self._sweep.eval(Z, self._dinit.cpu().numpy(), None if self._dtheta is None else self._dtheta.cpu().numpy(),
                                None if self._dscale is None else self._dscale.cpu().numpy(), fids=False)[0].T

    def L(self, Z) -> float:
        """loss(X(Z)); Z a numpy vector or a float64 tensor on the handle's device."""
        return self._loss(Z, False)[0]

    def grad_L(self, Z):
        """The dense gradient, length `len(Z)`: a numpy array for a numpy Z, a tensor on the handle's device for a tensor Z (nothing
        crosses to the host but the loss value)."""
        return self._loss(Z, True)[1]

    def hess_L(self, Z):
        raise RuntimeError("SweepFinalStateObjective is first order: build the evaluator with eval_hessian=False")

    def gauss_newton_times(self, Z, v):
        """The generalized Gauss-Newton product J^T (d2 loss / dX2) J v as a dense vector of length `len(Z)`, J the Jacobian of the
        final states X with respect to Z: one pushforward (X and Xdot = J v, `jvp_device`), the loss's own Hessian product
        u = d2 loss(X) Xdot by double backward on the loss alone (X a detached leaf), one pullback (`vjp_device`, cot = u).  A loss
        that is linear in X gives zeros.  Z and v are numpy arrays (the result is one) or float64 tensors on the handle's device (the
        result stays there).  Needs the pushforward's scope beside the pullback's: an "mfma16-sweep" handle, an "mfma32-sweep" handle
        made with `wide_tangent`, or an "mfma64-sweep" handle made with `wide64_tangent`."""
        sw = self._sweep
        if not sw.jvp_supported:
            raise _lib.QCollocError(_lib.QC_ERR_UNSUPPORTED, sw.jvp_unsupported_reason)
        on_device = torch.is_tensor(Z) and torch.is_tensor(v)
        put = lambda a: (a.detach() if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))).to(self._dev).contiguous().reshape(-1)
        dZ, dv = put(Z), put(v)
        if dZ.numel() != self.Z_len or dv.numel() != self.Z_len:
            raise ValueError(f"Z and v must have length {self.Z_len}")
        with torch.cuda.device(self._dev):
            X = torch.empty((self.S, sw.ns), dtype=torch.float64, device=self._dev)
            Xd = torch.empty_like(X)
            sw.jvp_device(dZ, self._dinit, self.S, self._dtheta, self._dscale, dvZ=dv, dfinals=X, dtfinals=Xd)
            u = None
            with torch.enable_grad():
                X.requires_grad_(True)
                L = self.loss(X)
                if L.dim() != 0:
                    raise ValueError("loss must return a 0-dim tensor")
                g = torch.autograd.grad(L, X, create_graph=True, allow_unused=True)[0] if L.requires_grad else None
                if g is not None and g.requires_grad:
                    u = torch.autograd.grad(g, X, grad_outputs=Xd, allow_unused=True)[0]
            out = torch.zeros(self.Z_len, dtype=torch.float64, device=self._dev)
            if u is not None:      # (a loss linear in X has no second derivative: exact zeros, no pullback)
                sw.vjp_device(dZ, self._dinit, self.S, u.detach().contiguous(), self._dtheta, self._dscale, dgrad=out)
        return out if on_device else out.cpu().numpy()

    def hessian_times(self, Z, v):
        """The EXACT Hessian product d2 L / dZ2 v as a dense vector of length `len(Z)`: one pushforward (X and Xdot = J v, `jvp_device`),
        cot = d loss/dX and vcot = (d2 loss/dX2) Xdot by torch on the loss alone (X a detached leaf), one `hvp_device` call -- the tangent
        of the pullback along (v, vcot).  It is `gauss_newton_times` plus the curvature of the sweep map, sum_s <cot_s, d2 X_s/dZ2 v>, which
        for a loss that is linear or nearly linear in X is the whole Hessian.  A loss linear in X gives vcot = 0, not a skipped call.  Z and
        v are numpy arrays (the result is one) or float64 tensors on the handle's device (the result stays there).  Needs the Hessian
        product's scope and the pushforward's: closed systems on an "mfma16-sweep" handle, or on an "mfma32-sweep" handle made with both
        `wide_tangent` (the `jvp_device` call) and `wide_hessian` (the `hvp_device` call); with one of the two it raises
        QC_ERR_UNSUPPORTED with the handle's reason."""
        sw = self._sweep
        if not sw.hvp_supported:
            raise _lib.QCollocError(_lib.QC_ERR_UNSUPPORTED, sw.hvp_unsupported_reason)
        if not sw.jvp_supported:
            raise _lib.QCollocError(_lib.QC_ERR_UNSUPPORTED, sw.jvp_unsupported_reason)
        on_device = torch.is_tensor(Z) and torch.is_tensor(v)
        put = lambda a: (a.detach() if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))).to(self._dev).contiguous().reshape(-1)
        dZ, dv = put(Z), put(v)
        if dZ.numel() != self.Z_len or dv.numel() != self.Z_len:
            raise ValueError(f"Z and v must have length {self.Z_len}")
        with torch.cuda.device(self._dev):
            X = torch.empty((self.S, sw.ns), dtype=torch.float64, device=self._dev)
            Xd = torch.empty_like(X)
            sw.jvp_device(dZ, self._dinit, self.S, self._dtheta, self._dscale, dvZ=dv, dfinals=X, dtfinals=Xd)
            g = u = None
            with torch.enable_grad():
                X.requires_grad_(True)
                L = self.loss(X)
                if L.dim() != 0:
                    raise ValueError("loss must return a 0-dim tensor")
                g = torch.autograd.grad(L, X, create_graph=True, allow_unused=True)[0] if L.requires_grad else None
                if g is not None and g.requires_grad:
                    u = torch.autograd.grad(g, X, grad_outputs=Xd, allow_unused=True)[0]
            out = torch.zeros(self.Z_len, dtype=torch.float64, device=self._dev)
            if g is not None:      # (a loss that does not depend on X: exact zeros)
                cot = g.detach().contiguous()
                vcot = torch.zeros_like(cot) if u is None else u.detach().contiguous()
                sw.hvp_device(dZ, self._dinit, self.S, cot, self._dtheta, self._dscale, dvZ=dv, dvcot=vcot, dtgrad=out)
        return out if on_device else out.cpu().numpy()

    def __getattr__(self, name):
        al = type(self)._ALIASES
        if name in al:
            return getattr(self, al[name])
        raise AttributeError(name)

    def close(self):
        if getattr(self, "_sweep", None) is not None:
            self._sweep.close()
            self._sweep = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
