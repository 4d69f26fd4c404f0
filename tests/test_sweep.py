"""Rollout sweeps (`qc_sweep_*`, `rollout_sweep`, `RolloutSweep`): final states and fidelities of one trajectory of controls under
S perturbed systems.  CPU: the scipy reference (tests/sweep_reference.py) against an independent eigendecomposition route, the
descriptor's layout and validation, the restated launch rule.  GPU: parity with the reference in both launch forms ("mfma16-sweep",
"rollout-per-sample"), generator norms over 0 .. 8 squarings, exact cases, consistency with `unitary_rollout`, the reference's own
robustness check, bit reproducibility, device-resident calls on a side stream, non-finite input.

Tolerances (GPU against the reference): states rtol 1e-10 / atol 1e-11, the project's rollout tolerance (tests/test_rollout.py);
fidelities 1e-9 absolute, which the state tolerance implies (|dF| <= sqrt(N) max|dU| for N <= 32).  The reference itself agrees with
the independent route to better than 1e-12 (first test).
States of many columns, up to the 4096 entries the descriptor admits (the strided loops and the LDS opt-in of the finish kernels):
tests/test_sweep_many_columns.py; every sample of the pushforward's launches: tests/test_sweep_jvp_every_sample.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import sweep_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE_RTOL, STATE_ATOL, FID_ATOL = 1e-10, 1e-11, 1e-9
SWEEP_FILL = 2048          # waves that give every SIMD a couple: 256 CUs x 4 SIMDs x 2


def sweep_launch(n, m, S, T):
    """The launch rule of qc_sweep.hip, restated: the MFMA form for 2N <= 16 with up to 8 drives, one wavefront per (sample, chunk);
    one chunk once S alone fills the device, else ceil(2048 / S) chunks, at most ceil(sqrt(T - 1))."""
    if n > 16 or m > 8:
        return dict(mfma=False, chunk=T - 1, n_chunks=0, last=0)
    n_int = T - 1
    want = 1 if S >= SWEEP_FILL else -(-SWEEP_FILL // S)
    r = 1
    while r * r < n_int:
        r += 1
    nch = min(want, r)
    chunk = -(-n_int // nch)
    n_chunks = -(-n_int // chunk)
    return dict(mfma=True, chunk=chunk, n_chunks=n_chunks, last=n_int - (n_chunks - 1) * chunk, by_sqrt=want > r)


def _herm(rng, N, scale=None):
    X = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
    return (N ** -0.5 if scale is None else scale) * (X + X.conj().T) / 2


def _unitary(rng, N):
    import scipy.linalg as sla
    return sla.expm(1j * _herm(rng, N, 1.0))


# name: (state, levels, m, p, scale given, free timestep, S, T, fidelity)
#   state     unitary | ket | kets3 | density (an open system of `levels` levels: n = 2 levels^2)
#   fidelity  (kind, subspace, form) or None
SWEEP_CASES = {
    "qubit-S11-T50": ("unitary", 2, 2, 1, False, True, 11, 50, ("unitary", None, "abs")),
    "qutrit-S300-T102": ("unitary", 3, 1, 3, True, False, 300, 102, ("unitary", [0, 1], "abs2")),      # padded tile; 7 chunks of 15, the last 11
    "levels4-S2048-T50": ("unitary", 4, 6, 8, True, True, 2048, 50, ("unitary", [0, 1], "abs")),      # one chunk
    "qubits3-S1-T1000": ("unitary", 8, 6, 1, False, True, 1, 1000, ("unitary", None, "abs2")),        # 32 chunks of 32, the last 7
    "qubits3-S11-T1000": ("unitary", 8, 8, 0, True, False, 11, 1000, ("unitary", None, "abs")),
    "qubits3-S300-T102": ("unitary", 8, 2, 3, True, True, 300, 102, None),
    "ket4-S2048-T2": ("ket", 4, 2, 1, False, True, 2048, 2, ("ket", None, "abs")),
    "kets3-S11-T102": ("kets3", 4, 1, 3, True, False, 11, 102, None),
    "open2-S300-T50": ("density", 2, 2, 1, True, True, 300, 50, ("density", None, "abs")),            # n = 8, non-antisymmetric generators
    "open2-S11-T2": ("density", 2, 1, 0, False, False, 11, 2, ("density", None, "abs")),
    "levels12-S11-T50": ("unitary", 12, 2, 1, False, True, 11, 50, ("unitary", [0, 1, 2, 3], "abs")),  # n = 24: per-sample form
    "qubits5-S11-T102": ("unitary", 32, 1, 3, True, False, 11, 102, ("unitary", None, "abs2")),       # n = 64
    "open5-S11-T50": ("density", 5, 2, 1, True, True, 11, 50, ("density", None, "abs")),              # n = 50
    "levels12-S300-T2": ("unitary", 12, 6, 8, False, True, 300, 2, None),
    "ket12-S2048-T2": ("ket", 12, 2, 1, True, True, 2048, 2, ("ket", None, "abs")),
    "qubit-9drives-S11-T50": ("unitary", 2, 9, 1, True, True, 11, 50, ("unitary", None, "abs")),     # more drives than tiles: per-sample form
}


def _case_n(name):
    state, L = SWEEP_CASES[name][:2]
    return 2 * L * L if state == "density" else 2 * L


def build_case(qc, name, seed=None):
    """Everything a sweep call and the reference need, from a seeded generator."""
    state, L, m, p, use_scale, free, S, T, fid = SWEEP_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)) if seed is None else seed)
    H0 = _herm(rng, L)
    Hd = [_herm(rng, L, (L * max(m, 1)) ** -0.5) for _ in range(m)]
    if state == "density":
        diss = [0.3 * (rng.standard_normal((L, L)) + 1j * rng.standard_normal((L, L))) / L ** 0.5]
        system = qc.OpenQuantumSystem(H0, Hd, diss)
        # perturbations of an open system are generator matrices: an extra decay channel, then Hamiltonian terms
        perts = []
        for j in range(p):
            if j == 0:
                Lx = (rng.standard_normal((L, L)) + 1j * rng.standard_normal((L, L))) / L ** 0.5
                perts.append(np.asarray(qc.iso_operator(qc.OpenQuantumSystem.dissipator_superoperator(Lx))))
            else:
                perts.append(np.asarray(qc.iso_operator(qc.OpenQuantumSystem.hamiltonian_superoperator(_herm(rng, L)))))
        G0, Gd, Gp = np.asarray(system.G_drift), [np.asarray(G) for G in system.G_drives], perts
        psi = rng.standard_normal(L) + 1j * rng.standard_normal(L)
        psi /= np.linalg.norm(psi)
        init = qc.density_to_iso_vec(np.outer(psi, psi.conj()))
        cols = 1
    else:
        system = qc.QuantumSystem(H0, Hd)
        perts = [_herm(rng, L) for _ in range(p)]
        G0, Gd, Gp = ref.iso_generator(H0), [ref.iso_generator(H) for H in Hd], [ref.iso_generator(P) for P in perts]
        if state == "unitary":
            init, cols = ref.operator_to_iso_vec(_unitary(rng, L)), L
        else:
            cols = 1 if state == "ket" else 3
            K = rng.standard_normal((L, cols)) + 1j * rng.standard_normal((L, cols))
            K /= np.linalg.norm(K, axis=0)
            init = ref.operator_to_iso_vec(K)
    goal = subspace = None
    kind = form = None
    if fid is not None:
        kind, subspace, form = fid
        if kind == "unitary":
            goal = ref.operator_to_iso_vec(_unitary(rng, L))
        else:
            g = rng.standard_normal(L) + 1j * rng.standard_normal(L)
            g /= np.linalg.norm(g)
            goal = np.concatenate([g.real, g.imag])
    controls = rng.uniform(-1, 1, (m, T))
    dts = rng.uniform(0.1, 0.3, T) if free else 0.2
    theta = rng.uniform(-0.3, 0.3, (S, p))
    if state == "density":
        theta = np.abs(theta)         # the first perturbation is a decay channel: a rate, not negative
    scale = rng.uniform(0.9, 1.1, (S, m)) if use_scale else None
    return dict(name=name, state=state, L=L, N=system.state_levels, n=2 * system.state_levels, m=m, p=p, S=S, T=T, system=system, perts=perts,
                G0=G0, Gd=Gd, Gp=Gp, init=init, cols=cols, goal=goal, kind=kind, subspace=subspace, form=form, controls=controls, dts=dts,
                theta=theta, scale=scale, H=(H0, Hd, perts))


def make_sweep(qc, c, **kw):
    form = qc._lib.QC_FID_FORM_ABS2 if c["form"] == "abs2" else qc._lib.QC_FID_FORM_ABS
    return qc.RolloutSweep(c["system"], c["perts"], c["T"], cols=c["cols"], goal=c["goal"], fid_kind=c["kind"], subspace=c["subspace"],
                           fid_form=form, dt_fixed=None if np.ndim(c["dts"]) else float(c["dts"]), **kw)


def reference(c):
    finals = ref.sweep_finals(c["G0"], c["Gd"], c["Gp"], c["controls"], c["dts"], c["init"], c["theta"], c["scale"])
    fids = None
    if c["kind"] is not None:
        fids = ref.fidelities(finals, c["kind"], c["goal"], c["L"], c["subspace"], c["form"])
    return finals, fids


# ---------------------------------------------------------------------------------------------------------------------------------
#  CPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,T,S", [(2, 50, 11), (3, 102, 7), (8, 1000, 6)])
def test_reference_agrees_with_an_independent_route(N, T, S):
    """The scipy chain on iso generators against eigendecompositions in complex arithmetic: better than 1e-12, two orders of
    magnitude inside the GPU tolerance."""
    rng = np.random.default_rng(100 * N + S)
    m, p = 2, 2
    H0, Hd, Hp = _herm(rng, N), [_herm(rng, N, (2 * N) ** -0.5) for _ in range(m)], [_herm(rng, N) for _ in range(p)]
    controls, dts = rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T)
    theta, scale = rng.uniform(-0.3, 0.3, (S, p)), rng.uniform(0.9, 1.1, (S, m))
    init = ref.operator_to_iso_vec(_unitary(rng, N))
    a = ref.sweep_finals(ref.iso_generator(H0), [ref.iso_generator(H) for H in Hd], [ref.iso_generator(H) for H in Hp], controls, dts, init,
                         theta, scale)
    b = ref.sweep_finals_eigh(H0, Hd, Hp, controls, dts, init, theta, scale)
    err = np.abs(a - b).max()
    print(f"reference vs eigh route, N={N} T={T} S={S}: {err:.2e}")
    assert err < 1e-12
    for s in range(S):   # and the final states are unitary
        U = ref.iso_vec_to_operator(a[:, s], N)
        np.testing.assert_allclose(U.conj().T @ U, np.eye(N), atol=1e-11)


def test_reference_fidelities_follow_the_definitions():
    rng = np.random.default_rng(3)
    N = 4
    U, G = _unitary(rng, N), _unitary(rng, N)
    x, g = ref.operator_to_iso_vec(U), ref.operator_to_iso_vec(G)
    assert abs(ref.unitary_fidelity(g, g, N) - 1) < 1e-14 and abs(ref.unitary_fidelity(x, g, N) - abs(np.trace(G.conj().T @ U)) / N) < 1e-15
    sub = [0, 2]
    t = sum(np.conj(G[a, b]) * U[a, b] for a in sub for b in sub)
    assert abs(ref.unitary_fidelity(x, g, N, sub, "abs2") - abs(t) ** 2 / 4) < 1e-15
    psi, phi = U[:, 0], G[:, 1]
    pv, gv = np.concatenate([psi.real, psi.imag]), np.concatenate([phi.real, phi.imag])
    assert abs(ref.ket_fidelity(pv, gv) - abs(np.vdot(phi, psi)) ** 2) < 1e-15
    rho = np.outer(psi, psi.conj())
    rv = np.concatenate([rho.reshape(-1, order="F").real, rho.reshape(-1, order="F").imag])
    assert abs(ref.density_fidelity(rv, gv) - abs(np.vdot(phi, psi)) ** 2) < 1e-14


class _Desc:
    """A qc_sweep_desc with arrays of its own (kept alive here)."""

    def __init__(self, qc, N=2, m=2, T=10, p=1, cols=0, zdim=None, off_a=0, off_dt=None, fid_kind=None, fid_form=0, subspace=None, with_pert=True):
        L = qc._lib
        n = 2 * N
        self.G0 = np.zeros(n * n)
        self.Gd = np.zeros(max(m, 1) * n * n)
        self.Gp = np.zeros(max(p, 1) * n * n)
        self.goal = np.zeros(2 * N * N)
        self.sub = None if subspace is None else np.ascontiguousarray(subspace, dtype=np.int32)
        d = L.qc_sweep_desc()
        d.T, d.N, d.m, d.n_pert, d.state_cols = T, N, m, p, cols
        d.zdim = m + 1 if zdim is None else zdim
        d.off_a = off_a
        d.off_dt = m if off_dt is None else off_dt
        d.fid_kind = L.QC_SWEEP_FID_NONE if fid_kind is None else fid_kind
        d.fid_form = fid_form
        d.G_drift, d.G_drives = L.dptr(self.G0), L.dptr(self.Gd)
        d.G_pert = L.dptr(self.Gp) if with_pert else None
        d.goal_iso = L.dptr(self.goal)
        if self.sub is not None:
            d.subspace, d.n_sub = self.sub.ctypes.data_as(C.POINTER(C.c_int32)), self.sub.size
        self.d = d


def test_sweep_desc_size_matches_the_mirror_and_c(qc, tmp_path):
    L = qc._lib
    assert L.lib.qc_sizeof_sweep_desc() == C.sizeof(L.qc_sweep_desc)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "qcolloc.h"\n'
                   'int main(){printf("%zu %zu %zu %zu %zu %zu %d %d\\n", sizeof(qc_sweep_desc), offsetof(qc_sweep_desc, dt_fixed), '
                   'offsetof(qc_sweep_desc, G_drift), offsetof(qc_sweep_desc, fid_form), offsetof(qc_sweep_desc, subspace), '
                   'offsetof(qc_sweep_desc, device), QC_MAX_PERT, QC_SWEEP_FID_NONE);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    d = L.qc_sweep_desc
    assert got == [C.sizeof(d), d.dt_fixed.offset, d.G_drift.offset, d.fid_form.offset, d.subspace.offset, d.device.offset, L.QC_MAX_PERT,
                   L.QC_SWEEP_FID_NONE]
    assert qc._lib.lib.qc_abi_version() == 6      # purely additive: the ABI stays 0.6


def test_sweep_desc_validate_without_a_device(qc):
    L = qc._lib
    val = lambda D: L.lib.qc_sweep_desc_validate(C.byref(D.d))
    msg = lambda: L.lib.qc_sweep_last_error(None).decode()
    assert val(_Desc(qc)) == L.QC_OK
    assert val(_Desc(qc, p=0, with_pert=False)) == L.QC_OK
    assert val(_Desc(qc, p=8)) == L.QC_OK
    assert val(_Desc(qc, fid_kind=L.QC_FID_UNITARY, fid_form=L.QC_FID_FORM_ABS2, subspace=[0, 1])) == L.QC_OK
    assert val(_Desc(qc, N=4, cols=1, fid_kind=L.QC_FID_KET)) == L.QC_OK
    assert val(_Desc(qc, N=4, cols=1, fid_kind=L.QC_FID_DENSITY)) == L.QC_OK
    assert val(_Desc(qc, off_dt=-1)) == L.QC_OK
    bad = {
        "n_pert > 8": _Desc(qc, p=9),
        "n_pert > 0, G_pert NULL": _Desc(qc, p=2, with_pert=False),
        "off_a outside": _Desc(qc, m=2, zdim=3, off_a=2),
        "off_a negative": _Desc(qc, off_a=-1),
        "off_dt outside": _Desc(qc, m=2, zdim=3, off_dt=3),
        "off_dt below -1": _Desc(qc, off_dt=-2),
        "subspace index >= N": _Desc(qc, N=3, fid_kind=L.QC_FID_UNITARY, subspace=[0, 3]),
        "repeated subspace index": _Desc(qc, N=3, fid_kind=L.QC_FID_UNITARY, subspace=[1, 1]),
        "ket with 2 columns": _Desc(qc, N=4, cols=2, fid_kind=L.QC_FID_KET),
        "ket on a unitary": _Desc(qc, N=4, cols=0, fid_kind=L.QC_FID_KET),
        "unknown fid_kind": _Desc(qc, fid_kind=7),
        "unknown fid_form": _Desc(qc, fid_kind=L.QC_FID_UNITARY, fid_form=2),
        "T < 2": _Desc(qc, T=1),
    }
    for what, D in bad.items():
        assert val(D) == L.QC_ERR_INVALID, what
        assert msg().startswith("qc_sweep") and len(msg()) > 12, what
    assert L.lib.qc_sweep_desc_validate(None) == L.QC_ERR_INVALID and msg()
    assert val(_Desc(qc, N=33)) == L.QC_ERR_UNSUPPORTED and "2N" in msg()
    assert L.lib.qc_sweep_kernel_name(None) == b"none"


@pytest.mark.skipif(torch.cuda.is_available(), reason="this box has a GPU")
def test_sweep_create_without_a_gpu_fails_loudly(qc):
    L = qc._lib
    h = C.c_void_p()
    assert L.lib.qc_sweep_create(C.byref(_Desc(qc).d), C.byref(h)) == L.QC_ERR_NO_DEVICE
    assert not h.value and L.lib.qc_sweep_last_error(None).decode()
    sys_ = qc.QuantumSystem(np.zeros((2, 2)), [qc.GATES["X"], qc.GATES["Y"]])
    with pytest.raises(qc.QCollocError) as e:
        qc.rollout_sweep(ref.operator_to_iso_vec(np.eye(2)), np.zeros((2, 5)), 0.2, sys_, [qc.GATES["Z"]], np.zeros((3, 1)))
    assert e.value.code == L.QC_ERR_NO_DEVICE


def test_sweep_launch_rule_and_coverage(qc):
    """The restated rule is the library's (`qc_sweep_desc_launch`, device-free), and the GPU cases reach every branch of it: one chunk,
    several chunks limited by the sample count and by sqrt(T - 1), a short last chunk, S = 1, T = 2, and the per-sample form."""
    L = qc._lib
    got = {}
    shapes = [(_case_n(k), SWEEP_CASES[k][2], SWEEP_CASES[k][6], SWEEP_CASES[k][7]) for k in SWEEP_CASES]
    shapes += [(16, 6, S, T) for S in (1, 2, 64, 300, 1024, 2047, 2048, 8192) for T in (2, 3, 50, 102, 1000, 10001)] + [(4, 9, 11, 50), (18, 1, 5, 9)]
    for n, m, S, T in shapes:
        D = _Desc(qc, N=n // 2, m=m, T=T, cols=1)
        mf, ch, nch = C.c_int32(), C.c_int64(), C.c_int64()
        assert L.lib.qc_sweep_desc_launch(C.byref(D.d), S, C.byref(mf), C.byref(ch), C.byref(nch)) == L.QC_OK
        want = sweep_launch(n, m, S, T)
        assert (bool(mf.value), ch.value, nch.value) == (want["mfma"], want["chunk"], want["n_chunks"]), (n, m, S, T)
        if want["mfma"]:
            assert (nch.value - 1) * ch.value < T - 1 <= nch.value * ch.value
        got[(n, m, S, T)] = want
    assert L.lib.qc_sweep_desc_launch(C.byref(_Desc(qc).d), 0, None, None, None) == L.QC_ERR_INVALID
    f = {k: sweep_launch(_case_n(k), SWEEP_CASES[k][2], SWEEP_CASES[k][6], SWEEP_CASES[k][7]) for k in SWEEP_CASES}
    assert f["levels4-S2048-T50"] == dict(mfma=True, chunk=49, n_chunks=1, last=49, by_sqrt=False)
    assert f["qutrit-S300-T102"] == dict(mfma=True, chunk=15, n_chunks=7, last=11, by_sqrt=False)        # limited by the sample count, short last chunk
    assert f["qubits3-S1-T1000"] == dict(mfma=True, chunk=32, n_chunks=32, last=7, by_sqrt=True)          # S = 1, limited by sqrt(T - 1)
    assert f["qubit-S11-T50"]["n_chunks"] == 7 and f["qubit-S11-T50"]["by_sqrt"]
    assert f["ket4-S2048-T2"]["n_chunks"] == 1 and f["open2-S11-T2"] == dict(mfma=True, chunk=1, n_chunks=1, last=1, by_sqrt=True)
    assert not f["levels12-S11-T50"]["mfma"] and not f["qubits5-S11-T102"]["mfma"] and not f["open5-S11-T50"]["mfma"]
    assert not f["qubit-9drives-S11-T50"]["mfma"] and f["open2-S300-T50"]["mfma"]
    # every value the cases are asked to cover
    col = lambda i: {SWEEP_CASES[k][i] for k in SWEEP_CASES}
    assert {2, 3, 4, 8, 12, 32} <= {SWEEP_CASES[k][1] for k in SWEEP_CASES if SWEEP_CASES[k][0] == "unitary"}
    assert {"ket", "kets3", "density"} <= col(0) and {2, 5} <= {SWEEP_CASES[k][1] for k in SWEEP_CASES if SWEEP_CASES[k][0] == "density"}
    assert {1, 2, 6, 8} <= col(2) and {0, 1, 3, 8} <= col(3) and col(4) == {True, False} == col(5)
    assert {1, 11, 300, 2048} <= col(6) and {2, 50, 102, 1000} <= col(7)
    fids = {SWEEP_CASES[k][8] and (SWEEP_CASES[k][8][0], SWEEP_CASES[k][8][1] is not None, SWEEP_CASES[k][8][2]) for k in SWEEP_CASES}
    assert {("unitary", False, "abs"), ("unitary", False, "abs2"), ("unitary", True, "abs"), ("unitary", True, "abs2"), ("ket", False, "abs"),
            ("density", False, "abs"), None} <= fids


# ---------------------------------------------------------------------------------------------------------------------------------
#  GPU
# ---------------------------------------------------------------------------------------------------------------------------------
def _assert_states(got, want, what):
    err = np.abs(got - want)
    print(f"{what}: max |d state| = {err.max():.3e}, worst against the tolerance = {(err / (STATE_ATOL + STATE_RTOL * np.abs(want))).max():.3f}")
    np.testing.assert_allclose(got, want, rtol=STATE_RTOL, atol=STATE_ATOL, err_msg=what)


def _assert_fids(got, want, what):
    print(f"{what}: max |d fidelity| = {np.abs(got - want).max():.3e}")
    assert np.abs(got - want).max() <= FID_ATOL, what


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SWEEP_CASES))
def test_sweep_matches_the_reference(qc, name):
    c = build_case(qc, name)
    want = sweep_launch(c["n"], c["m"], c["S"], c["T"])
    sw = make_sweep(qc, c)
    try:
        assert sw.kernel_name == ("mfma16-sweep" if want["mfma"] else "rollout-per-sample")
        assert sw.launch(c["S"]) == (want["mfma"], want["chunk"], want["n_chunks"])
        finals, fids = sw.eval(sw.pack(c["controls"], c["dts"]), c["init"], c["theta"], c["scale"])
        if c["kind"] is not None:   # fidelities alone: the same values
            _, f2 = sw.eval(sw.pack(c["controls"], c["dts"]), c["init"], c["theta"], c["scale"], finals=False)
            np.testing.assert_array_equal(f2, fids)
    finally:
        sw.close()
    rf, rfid = reference(c)
    assert finals.shape == rf.shape == (c["n"] * c["cols"], c["S"])
    _assert_states(finals, rf, name)
    if c["kind"] is None:
        assert fids is None
    else:
        _assert_fids(fids, rfid, name)
        assert np.all(fids > -1e-9) and np.all(fids < 1 + 1e-9)
    # the one-call form
    if c["S"] <= 11:
        f3, fid3 = qc.rollout_sweep(c["init"], c["controls"], c["dts"], c["system"], c["perts"], c["theta"], c["scale"], cols=c["cols"],
                                    goal=c["goal"], fid_kind=c["kind"], subspace=c["subspace"],
                                    fid_form=qc._lib.QC_FID_FORM_ABS2 if c["form"] == "abs2" else qc._lib.QC_FID_FORM_ABS)
        if np.ndim(c["dts"]):     # (rollout_sweep reads its timesteps from the trajectory vector: the same launch for free timesteps only)
            np.testing.assert_array_equal(f3, finals)
        else:
            _assert_states(f3, rf, name + " (rollout_sweep)")
        if fid3 is not None:
            _assert_fids(fid3, rfid, name + " (rollout_sweep)")


def _squarings(norm):
    """The kernels' rule: the smallest sq with norm / 2^sq <= 1/8."""
    sq = 0
    while norm / 2.0 ** sq > 0.125:
        sq += 1
    return sq


@pytest.mark.gpu
def test_sweep_generator_norms(qc):
    """One case per number of squarings 0 .. 8 (the system scaled as test_rollout_large_generator_norm_and_fixed_time scales its own),
    with a strong perturbation so that the samples of one call need different numbers of squarings."""
    rng = np.random.default_rng(17)
    N, m, T, S = 4, 2, 12, 5
    H0, Hd, P = _herm(rng, N), [_herm(rng, N, 0.25) for _ in range(m)], _herm(rng, N)
    controls = rng.uniform(-1, 1, (m, T))
    init = ref.operator_to_iso_vec(_unitary(rng, N))
    goal = ref.operator_to_iso_vec(_unitary(rng, N))
    theta = np.array([[0.0], [0.5], [1.5], [4.0], [-9.0]])
    dt = 0.2
    base = max(np.abs(dt * ref.sample_generator(ref.iso_generator(H0), [ref.iso_generator(H) for H in Hd], [], controls[:, t], (), np.ones(m))).sum(axis=0).max()
               for t in range(T - 1))
    seen = set()
    for k in range(9):
        f = 0.09 * 2.0 ** k / base              # the unperturbed sample: ||dt G||_1 <= 0.09 2^k, k squarings at its largest interval
        sys_ = qc.QuantumSystem(f * H0, [f * H for H in Hd])
        G0, Gd, Gp = ref.iso_generator(f * H0), [ref.iso_generator(f * H) for H in Hd], [ref.iso_generator(f * P)]
        per_sample = [max(_squarings(np.abs(dt * ref.sample_generator(G0, Gd, Gp, controls[:, t], theta[s], np.ones(m))).sum(axis=0).max())
                          for t in range(T - 1)) for s in range(S)]
        assert per_sample[0] == k and len(set(per_sample)) > 1, (k, per_sample)
        seen |= set(per_sample)
        finals, fids = qc.rollout_sweep(init, controls, dt, sys_, [f * P], theta, goal=goal, fid_kind="unitary")
        rf = ref.sweep_finals(G0, Gd, Gp, controls, dt, init, theta)
        _assert_states(finals, rf, f"squarings {per_sample}")
        _assert_fids(fids, ref.fidelities(rf, "unitary", goal, N), f"squarings {per_sample}")
    assert set(range(9)) <= seen


@pytest.mark.gpu
@pytest.mark.parametrize("N", [4, 12])
def test_sweep_exact_cases(qc, N):
    """Zero generators and controls: finals are init, bit for bit.  theta = 0 with c = 1: the bits of scale = NULL, n_pert = 0."""
    rng = np.random.default_rng(N)
    T, S, m = 40, 7, 2
    init = ref.operator_to_iso_vec(_unitary(rng, N))
    zsys = qc.QuantumSystem(np.zeros((N, N)), [np.zeros((N, N))] * m)
    finals, _ = qc.rollout_sweep(init, np.zeros((m, T)), rng.uniform(0.1, 0.3, T), zsys, [np.zeros((N, N))], rng.uniform(-1, 1, (S, 1)))
    np.testing.assert_array_equal(finals, np.repeat(init[:, None], S, axis=1))
    sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, 0.3) for _ in range(m)])
    controls, dts = rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T)
    goal = ref.operator_to_iso_vec(_unitary(rng, N))
    a = qc.rollout_sweep(init, controls, dts, sys_, [_herm(rng, N), _herm(rng, N)], np.zeros((S, 2)), np.ones((S, m)), goal=goal, fid_kind="unitary")
    b = qc.rollout_sweep(init, controls, dts, sys_, [], np.zeros((S, 0)), None, goal=goal, fid_kind="unitary")
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    assert np.all(a[0] == a[0][:, :1]) and np.abs(a[0][:, 0] - init).max() > 1e-3


@pytest.mark.gpu
def test_sweep_is_consistent_with_the_rollout(qc):
    """S = 1 against the last column of `unitary_rollout` on the equivalent system (another algorithm: the state tolerance, not bits),
    and `unitary_rollout_fidelity_sweep` at theta = 0 against `unitary_rollout_fidelity`."""
    for N, T in [(2, 50), (8, 300), (12, 30)]:
        rng = np.random.default_rng(N + T)
        m = 2
        H0, Hd, P = _herm(rng, N), [_herm(rng, N, 0.3) for _ in range(m)], _herm(rng, N)
        controls, dts = rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T)
        init = ref.operator_to_iso_vec(_unitary(rng, N))
        th, c = 0.17, np.array([[1.05, 0.96]])
        finals, _ = qc.rollout_sweep(init, controls, dts, qc.QuantumSystem(H0, Hd), [P], np.array([[th]]), c)
        eq = qc.QuantumSystem(H0 + th * P, [c[0, k] * Hd[k] for k in range(m)])
        _assert_states(finals[:, 0], qc.unitary_rollout(init, controls, dts, eq)[:, -1], f"S = 1 against unitary_rollout, N = {N}")
    inp = qc.config_inputs(1, T=40)
    Zop = qc.GATES["Z"]
    f0 = qc.unitary_rollout_fidelity(inp.traj, inp.system)
    fs = qc.unitary_rollout_fidelity_sweep(inp.traj, inp.system, [Zop], np.zeros((3, 1)))
    assert fs.shape == (3,) and np.abs(fs - f0).max() <= FID_ATOL
    f1 = qc.unitary_rollout_fidelity_sweep(inp.traj, inp.system, [Zop], np.array([0.0, 0.05]))
    assert abs(f1[0] - f0) <= FID_ATOL and abs(f1[1] - f0) > 1e-6
    # a ket component
    rng = np.random.default_rng(9)
    N, T = 4, 30
    sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, 0.3)])
    psi0, g = _unitary(rng, N)[:, 0], _unitary(rng, N)[:, 0]
    iso = lambda v: np.concatenate([v.real, v.imag])
    traj = qc.NamedTrajectory({"ψ̃": np.repeat(iso(psi0)[:, None], T, axis=1), "a": rng.uniform(-1, 1, (1, T)), "Δt": rng.uniform(0.1, 0.3, (1, T))},
                              controls=("a",), timestep="Δt", initial={"ψ̃": iso(psi0)}, goal={"ψ̃": iso(g)})
    fk = qc.rollout_fidelity_sweep(traj, sys_, [_herm(rng, N)], np.zeros((2, 1)))
    assert np.abs(fk - qc.rollout_fidelity(traj, sys_)).max() <= FID_ATOL


@pytest.mark.gpu
def test_sweep_reproduces_the_reference_robustness_check(qc):
    """systems(zeta) = QuantumSystem(zeta Z, [X, Y]), H gate, T = 50, dt = 0.2, zeta = -0.05:0.01:0.05
    (reference unitary_sampling_problem.jl:204-244): eleven fidelities from one call against eleven rollouts."""
    X, Y, Zop, Hgate = qc.GATES["X"], qc.GATES["Y"], qc.GATES["Z"], qc.GATES["H"]
    T, dt = 50, 0.2
    zetas = np.arange(-5, 6) * 0.01
    rng = np.random.default_rng(2024)
    controls = rng.uniform(-1, 1, (2, T))
    init = ref.operator_to_iso_vec(np.eye(2))
    goal = ref.operator_to_iso_vec(Hgate)
    systems = lambda z: qc.QuantumSystem(z * Zop, [X, Y])
    finals, fids = qc.rollout_sweep(init, controls, dt, systems(0.0), [Zop], zetas[:, None], goal=goal, fid_kind="unitary")
    one_by_one = np.array([qc.iso_vec_unitary_fidelity(qc.unitary_rollout(init, controls, dt, systems(z))[:, -1], goal) for z in zetas])
    _assert_fids(fids, one_by_one, "sweep against 11 rollouts")
    G0, Gd, Gp = np.zeros((4, 4)), [ref.iso_generator(X), ref.iso_generator(Y)], [ref.iso_generator(Zop)]
    rf = ref.sweep_finals(G0, Gd, Gp, controls, dt, init, zetas[:, None])
    _assert_states(finals, rf, "systems(zeta)")
    _assert_fids(fids, ref.fidelities(rf, "unitary", goal, 2), "systems(zeta)")
    assert len(set(np.round(fids, 9))) > 5      # the detuning matters


@pytest.mark.gpu
def test_sweep_is_bit_reproducible(qc):
    """Six repeated calls return the same bits in both forms; the host and device entry points return the same bits."""
    rng = np.random.default_rng(8)
    for N, T, S in [(8, 1000, 300), (12, 40, 9)]:
        m = 6 if N == 8 else 2
        sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, (N * m) ** -0.5) for _ in range(m)])
        perts = [_herm(rng, N)]
        goal = ref.operator_to_iso_vec(_unitary(rng, N))
        sw = qc.RolloutSweep(sys_, perts, T, goal=goal, fid_kind="unitary")
        assert sw.kernel_name == ("mfma16-sweep" if N == 8 else "rollout-per-sample")
        Z = sw.pack(rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T))
        init = ref.operator_to_iso_vec(_unitary(rng, N))
        theta, scale = rng.uniform(-0.3, 0.3, (S, 1)), rng.uniform(0.9, 1.1, (S, m))
        first = sw.eval(Z, init, theta, scale)
        for _ in range(6):
            again = sw.eval(Z, init, theta, scale)
            np.testing.assert_array_equal(again[0], first[0])
            np.testing.assert_array_equal(again[1], first[1])
        dev = torch.device("cuda:0")
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        dfin, dfid = torch.empty((S, sw.ns), dtype=torch.float64, device=dev), torch.empty(S, dtype=torch.float64, device=dev)
        sw.eval_device(t(Z), t(init), t(theta), t(scale), dfin, dfid)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(dfin.cpu().numpy().T, first[0])
        np.testing.assert_array_equal(dfid.cpu().numpy(), first[1])
        sw.close()


@pytest.mark.gpu
def test_sweep_eval_device_on_a_side_stream_and_growing_S(qc):
    rng = np.random.default_rng(21)
    N, m, T = 4, 2, 60
    sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, 0.3) for _ in range(m)])
    goal = ref.operator_to_iso_vec(_unitary(rng, N))
    sw = qc.RolloutSweep(sys_, [_herm(rng, N), _herm(rng, N)], T, goal=goal, fid_kind="unitary", subspace=[0, 1])
    Z = sw.pack(rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T))
    init = ref.operator_to_iso_vec(_unitary(rng, N))
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    side = torch.cuda.Stream(device=dev)
    for S in (5, 700, 3000, 64):          # growing S reallocates the handle's scratch; a smaller S afterwards reuses it
        theta, scale = rng.uniform(-0.3, 0.3, (S, 2)), rng.uniform(0.9, 1.1, (S, m))
        host = sw.eval(Z, init, theta, scale)
        dZ, dinit, dth, dsc = t(Z), t(init), t(theta), t(scale)
        dfin, dfid = torch.full((S, sw.ns), -7.0, dtype=torch.float64, device=dev), torch.full((S,), -7.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            sw.eval_device(dZ, dinit, dth, dsc, dfin, dfid, stream=side)
        side.synchronize()
        np.testing.assert_array_equal(dfin.cpu().numpy().T, host[0])
        np.testing.assert_array_equal(dfid.cpu().numpy(), host[1])
        # outputs are optional one at a time
        dfid2 = torch.empty(S, dtype=torch.float64, device=dev)
        sw.eval_device(dZ, dinit, dth, None, None, dfid2, stream=side)
        side.synchronize()
        np.testing.assert_array_equal(dfid2.cpu().numpy(), sw.eval(Z, init, theta, None, finals=False)[1])
    with pytest.raises(ValueError):
        sw.eval_device(t(Z), t(init), t(np.zeros((3, 2))), None, None, None)
    sw.close()


@pytest.mark.gpu
@pytest.mark.parametrize("N", [4, 12])
def test_sweep_non_finite_input(qc, N):
    """One NaN control does not raise; it reaches every sample here (the controls are shared), so every final state and fidelity is
    NaN; the handle then serves a finite call as if nothing had happened."""
    rng = np.random.default_rng(N)
    m, T, S = 2, 30, 6
    sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, 0.3) for _ in range(m)])
    goal = ref.operator_to_iso_vec(_unitary(rng, N))
    sw = qc.RolloutSweep(sys_, [_herm(rng, N)], T, goal=goal, fid_kind="unitary")
    controls, dts = rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T)
    init = ref.operator_to_iso_vec(_unitary(rng, N))
    theta = rng.uniform(-0.3, 0.3, (S, 1))
    good = sw.eval(sw.pack(controls, dts), init, theta)
    bad_controls = controls.copy()
    bad_controls[1, 7] = np.nan
    finals, fids = sw.eval(sw.pack(bad_controls, dts), init, theta)
    assert np.isnan(finals).all() and np.isnan(fids).all()
    bad_controls[1, 7] = controls[1, 7]
    bad_controls[0, T - 1] = np.nan          # the last knot's controls drive no interval
    again = sw.eval(sw.pack(bad_controls, dts), init, theta)
    np.testing.assert_array_equal(again[0], good[0])
    np.testing.assert_array_equal(again[1], good[1])
    sw.close()


@pytest.mark.gpu
@pytest.mark.parametrize("N,m,T,sizes", [(2, 2, 5, (1, 7, 3)), (9, 1, 3, (1, 3))], ids=["mfma16-sweep", "rollout-per-sample"])
def test_sweep_scratch_grows_and_is_reused(qc, N, m, T, sizes):
    """One handle serves S = 1, then a larger S, then (MFMA form) a smaller one, through the host-buffer and the device entry point: the
    scratch behind them (the chunk totals or the per-sample finals, and the staging of theta, scale, finals, fidelities) is freed and
    taken afresh when S grows, and reused when it shrinks.  Every result carries the bits a fresh handle returns at that S."""
    rng = np.random.default_rng(100 + N)
    sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, 0.3) for _ in range(m)])
    perts = [_herm(rng, N)]
    goal = ref.operator_to_iso_vec(_unitary(rng, N))
    make = lambda: qc.RolloutSweep(sys_, perts, T, goal=goal, fid_kind="unitary")
    sw = make()
    assert sw.kernel_name == ("mfma16-sweep" if 2 * N <= 16 else "rollout-per-sample")
    Z = sw.pack(rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T))
    init = ref.operator_to_iso_vec(_unitary(rng, N))
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    for S in sizes:
        theta, scale = rng.uniform(-0.3, 0.3, (S, 1)), rng.uniform(0.9, 1.1, (S, m))
        fresh = make()
        want = fresh.eval(Z, init, theta, scale)
        fresh.close()
        got = sw.eval(Z, init, theta, scale)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])
        dfin, dfid = torch.full((S, sw.ns), -7.0, dtype=torch.float64, device=dev), torch.full((S,), -7.0, dtype=torch.float64, device=dev)
        sw.eval_device(t(Z), t(init), t(theta), t(scale), dfin, dfid)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(dfin.cpu().numpy().T, want[0])
        np.testing.assert_array_equal(dfid.cpu().numpy(), want[1])
    sw.close()
