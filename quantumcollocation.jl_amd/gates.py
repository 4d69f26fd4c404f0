"""Gate / Pauli tables used by the reference's templates and tests (`GATES[:H]`, `PAULIS[:Z]`,
reference test/test_utils.jl:123-126, unitary_smooth_pulse_problem.jl:206-207)."""
from __future__ import annotations

from functools import reduce

import numpy as np

_I = np.eye(2, dtype=complex)
_X = np.array([[0, 1], [1, 0]], dtype=complex)
_Y = np.array([[0, -1j], [1j, 0]], dtype=complex)
_Z = np.array([[1, 0], [0, -1]], dtype=complex)

PAULIS = {"I": _I, "X": _X, "Y": _Y, "Z": _Z}


def operator_from_string(s: str) -> np.ndarray:
    """Kronecker product of single-qubit Paulis, e.g. "XIZ"."""
    return reduce(np.kron, [PAULIS[ch] for ch in s])


def qft(n_qubits: int) -> np.ndarray:
    d = 2 ** n_qubits
    w = np.exp(2j * np.pi / d)
    j, k = np.meshgrid(np.arange(d), np.arange(d), indexing="ij")
    return w ** (j * k) / np.sqrt(d)


def _controlled(U: np.ndarray, n_controls: int) -> np.ndarray:
    d = U.shape[0] * 2 ** n_controls
    out = np.eye(d, dtype=complex)
    out[-U.shape[0]:, -U.shape[0]:] = U
    return out


GATES = {
    "I": _I,
    "X": _X,
    "Y": _Y,
    "Z": _Z,
    "H": np.array([[1, 1], [1, -1]], dtype=complex) / np.sqrt(2),
    "CX": _controlled(_X, 1),
    "CNOT": _controlled(_X, 1),
    "CZ": _controlled(_Z, 1),
    "XI": np.kron(_X, _I),
    "TOFFOLI": _controlled(_X, 2),
    "QFT16": qft(4),
}


class EmbeddedOperator:
    """An operator on a subspace of an N-level system (PiccoloQuantumObjects' `EmbeddedOperator(op, subspace, levels)`):
    `operator` is n x n, `subspace` the n 0-based levels it acts on (default: the first n), `N` the full dimension.
    `unembed()` is the n x n operator; `embed(fill)` the N x N matrix with `fill` on the diagonal outside the subspace."""

    def __init__(self, operator, subspace=None, N: int = None):
        if isinstance(operator, str):
            operator = GATES[operator]
        self.operator = np.asarray(operator, dtype=complex)
        n = self.operator.shape[0]
        if self.operator.shape != (n, n):
            raise ValueError("operator must be square")
        self.subspace = list(range(n)) if subspace is None else [int(s) for s in subspace]
        if len(self.subspace) != n or len(set(self.subspace)) != n:
            raise ValueError("subspace must list one distinct level per row of the operator")
        self.N = max(self.subspace) + 1 if N is None else int(N)
        if min(self.subspace) < 0 or max(self.subspace) >= self.N:
            raise ValueError("subspace levels must lie in 0 .. N-1")

    def unembed(self) -> np.ndarray:
        return self.operator.copy()

    def embed(self, fill: complex = 0.0) -> np.ndarray:
        out = np.diag(np.full(self.N, fill, dtype=complex))
        out[np.ix_(self.subspace, self.subspace)] = self.operator
        return out

    def leakage_indices(self) -> np.ndarray:
        """Entries of the iso-vec `Ũ⃗ = vec(vcat(real(U), imag(U)))` (column-major, N x N) that carry population leaving the
        subspace: row outside it, column inside it, real and imaginary parts, ascending.  PiccoloQuantumObjects'
        `get_leakage_indices(op)` is recalled to pick this set (not vendored; INTEGRATION.md, table of choices)."""
        S = set(self.subspace)
        out = [c * 2 * self.N + part * self.N + r for c in self.subspace for part in (0, 1) for r in range(self.N) if r not in S]
        return np.array(sorted(out), dtype=np.int64)
