"""Open-system sweep gradients on wide handles ("mfma32-sweep", 16 < 2N <= 32): the stored-state walk on 2 x 2 tiles
(`qc_sweep_desc.wide` bit 3 = QC_SWEEP_WIDE_STORED together with `reserved1[0] = QC_SWEEP_STORED_STATES`;
`RolloutSweep(wide=True, stored_states=True, wide_stored=True)`; csrc/qc_sweep32_open_grad.hip).  Two qubits with T1 / T2 (levels^2 = 16,
2N = 32), a three-level transmon with relaxation (2N = 18), 10 .. 16 levels with a non-Hermitian effective Hamiltonian.

CPU: the bit field through `qc_sweep_desc_validate`, constants and ABI, the launch and scope queries, the Python keywords, the Julia
text, and the self-check of the reference (forward mode against central differences, 1e-6) on every system the GPU cases use.
GPU: every value against the forward-mode reference (tests/sweep_open_reference.py, tests/sweep_vjp_reference.py, as they are).

Tolerance, the project's own (tests/test_sweep_grad.py): per sample |got - want| <= 1e-9 max(1, max |want of that sample|).  `fids` and
`finals` are compared with `qc_sweep_eval` bit for bit.  Measured worst errors: profiles/sweep_wide_open_summary.txt."""
import ctypes as C
import functools
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import sweep_open_reference as oref
import sweep_reference as ref
import sweep_vjp_reference as vref
import test_sweep as ts
import test_sweep_open_grad as too
import test_sweep_wide as tw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_herm, _unitary = ts._herm, ts._unitary
SX, SY, SZ, SM = too.SX, too.SY, too.SZ, too.SM
I2 = np.eye(2, dtype=complex)
_worst, _Z, squarings = too._worst, too._Z, too.squarings


def two_qubit_case(qc, name, S, T, free=True, gamma1=0.12, gamma2=0.08, dt=(0.1, 0.3), samples=None):
    """Two qubits with a ZZ coupling, each with T1 (rate gamma1) and pure dephasing (rate gamma2): levels 4, N = 16, 2N = 32 (full tiles);
    one drive on each qubit, a common detuning as the perturbation, the density fidelity of one input state against an entangled goal."""
    rng = np.random.default_rng(sum(map(ord, name)))
    k = np.kron
    H0 = 0.3 * k(SZ, SZ) + 0.2 * k(SZ, I2) - 0.15 * k(I2, SZ) + 0.1 * k(SX, SX)
    Hd = [0.5 * k(SX, I2), 0.5 * k(I2, SY)]
    Ls = [np.sqrt(gamma1) * k(SM, I2), np.sqrt(gamma1) * k(I2, SM), np.sqrt(gamma2 / 2) * k(SZ, I2), np.sqrt(gamma2 / 2) * k(I2, SZ)]
    Pz = oref.lindblad_generator(0.5 * (k(SZ, I2) + k(I2, SZ)))
    psi0 = _unitary(rng, 4)[:, 0]
    g = np.array([1, 0, 0, 1j], dtype=complex) / np.sqrt(2)
    m = 2
    c = dict(name=name, L=4, N=16, m=m, p=1, S=S, T=T, G0=oref.lindblad_generator(H0, Ls), Gd=[oref.lindblad_generator(H) for H in Hd], Gp=[Pz],
             init=oref.density_iso(np.outer(psi0, psi0.conj())), cols=1, goal=np.concatenate([g.real, g.imag]), kind="density", subspace=None,
             form="abs", controls=rng.uniform(-1, 1, (m, T)), dts=rng.uniform(dt[0], dt[1], T) if free else 0.5 * (dt[0] + dt[1]),
             theta=rng.uniform(-0.3, 0.3, (S, 1)), scale=rng.uniform(0.9, 1.1, (S, m)), samples=list(range(S)) if samples is None else list(samples))
    c["system"] = qc.OpenQuantumSystem(H0, Hd, Ls) if qc is not None else None
    c["perts"] = [Pz]
    return c


def qutrit_case(qc, name, S, T, free=True, gamma1=0.15, gamma2=0.1, dt=(0.1, 0.3), samples=None):
    """A three-level transmon with relaxation (sqrt(gamma1) a) and dephasing (sqrt(gamma2) a'a): levels 3, N = 9, 2N = 18 -- the second tile
    row and column are zero-padded from entry 2 on."""
    rng = np.random.default_rng(sum(map(ord, name)))
    a = np.diag(np.sqrt([1.0, 2.0]), 1).astype(complex)
    num = a.conj().T @ a
    H0 = 0.2 * num - 0.15 * num @ (num - np.eye(3))
    Hd = [0.25 * (a + a.conj().T), 0.25j * (a - a.conj().T)]
    Ls = [np.sqrt(gamma1) * a, np.sqrt(gamma2) * num]
    Pz = oref.lindblad_generator(0.5 * num)
    v = _unitary(rng, 3)
    psi0, g = v[:, 0], v[:, 1]
    m = 2
    c = dict(name=name, L=3, N=9, m=m, p=1, S=S, T=T, G0=oref.lindblad_generator(H0, Ls), Gd=[oref.lindblad_generator(H) for H in Hd], Gp=[Pz],
             init=oref.density_iso(np.outer(psi0, psi0.conj())), cols=1, goal=np.concatenate([g.real, g.imag]), kind="density", subspace=None,
             form="abs", controls=rng.uniform(-1, 1, (m, T)), dts=rng.uniform(dt[0], dt[1], T) if free else 0.5 * (dt[0] + dt[1]),
             theta=rng.uniform(-0.3, 0.3, (S, 1)), scale=rng.uniform(0.9, 1.1, (S, m)), samples=list(range(S)) if samples is None else list(samples))
    c["system"] = qc.OpenQuantumSystem(H0, Hd, Ls) if qc is not None else None
    c["perts"] = [Pz]
    return c


SUB12 = [0, 1, 3, 4, 7, 10]
# the GPU cases of the issue's table
CASES = {
    "two-qubit-lindblad": lambda qc: two_qubit_case(qc, "two-qubit-lindblad", S=5, T=9),                                  # chunks 3, 3, 2
    "qutrit-lindblad": lambda qc: qutrit_case(qc, "qutrit-lindblad", S=3, T=6, free=False),
    "nonherm12-m8": lambda qc: too.nonherm_case(qc, "nonherm12-m8", 12, 8, 1, 3, 6, False, ("unitary", SUB12, "abs")),
    "nonherm16-m1": lambda qc: too.nonherm_case(qc, "nonherm16-m1", 16, 1, 1, 2, 3, False, ("unitary", None, "abs2")),
    "ket10-one-interval": lambda qc: too.nonherm_case(qc, "ket10-one-interval", 10, 2, 1, 1, 2, True, ("ket", None, "abs")),
    "one-chunk": lambda qc: qutrit_case(qc, "one-chunk", S=2049, T=3, samples=(0, 1, 1024, 2047, 2048)),
    "sq0": lambda qc: qutrit_case(qc, "sq0", S=3, T=5, dt=(0.01, 0.02)),
    "sq3": lambda qc: qutrit_case(qc, "sq3", S=3, T=5, dt=(0.9, 1.4)),
    "strong-dissipation": lambda qc: qutrit_case(qc, "strong-dissipation", S=3, T=9, gamma1=10.0, gamma2=2.0, dt=(0.4, 0.6)),
}
PARAM_CASES = ("two-qubit-lindblad", "nonherm12-m8")


def _pullback_case(qc):
    return too.nonherm_case(qc, "pullback-kets3", 10, 2, 1, 3, 5, True, None, cols=3)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The forward-mode derivatives of a case, computed once and shared (read-only) by the tests that need them."""
    out = oref.grad_forward(CASES[name](None))
    for v in out.values():
        v.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
#  CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_wide_values_through_validate(qc):
    L = qc._lib
    val = lambda D: L.lib.qc_sweep_desc_validate(C.byref(D.d))
    for N in (12, 16, 2):
        for good in (0, 1, 3, 9, 11):
            assert val(tw._wdesc(qc, good, N=N)) == L.QC_OK, (N, good)
        for bad in (4, 8, 10, 12, 13, 15, 2, 5, 7, -1):
            assert val(tw._wdesc(qc, bad, N=N)) == L.QC_ERR_INVALID, (N, bad)
            assert L.lib.qc_sweep_last_error(None).decode().startswith("qc_sweep: wide"), (N, bad)
    for flag_bad in (2, -1, 1 << 40):      # reserved1[0] keeps its own rule beside the new bit
        assert val(too._ODesc(qc, flag=flag_bad, wide=9, N=12)) == L.QC_ERR_INVALID
        assert "reserved1[0]" in L.lib.qc_sweep_last_error(None).decode()


def test_constants_and_abi(qc, tmp_path):
    L = qc._lib
    assert (L.QC_SWEEP_WIDE, L.QC_SWEEP_WIDE_PARAMS, L.QC_SWEEP_WIDE_STORED, L.QC_SWEEP_STORED_STATES) == (1, 2, 8, 1)
    header = open(os.path.join(ROOT, "include", "qcolloc.h")).read()
    assert re.search(r"^#define QC_SWEEP_WIDE_STORED 8\b", header, re.M)
    assert L.lib.qc_abi_version() == 6
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "qcolloc.h"\nint main(){printf("%zu %d %d %d\\n", sizeof(qc_sweep_desc), QC_SWEEP_WIDE, '
                   'QC_SWEEP_WIDE_PARAMS, QC_SWEEP_WIDE_STORED);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [128, 1, 2, 8] and L.lib.qc_sizeof_sweep_desc() == C.sizeof(L.qc_sweep_desc) == 128


def test_launch_query_does_not_see_the_bit(qc):
    """`qc_sweep_desc_launch` answers for wide = 9 and 11 what it answers for wide = 1 (the grid of tests/test_sweep_wide_param_grad.py)."""
    L = qc._lib
    for n in (16, 18, 24, 32, 34):
        for m in (1, 8, 9):
            for S, T in ((1, 2), (2, 102), (5, 12), (11, 50), (300, 2), (2047, 50), (2048, 3), (8192, 1000)):
                got = []
                for wide in (1, 9, 11):
                    D = tw._wdesc(qc, wide, N=n // 2, m=m, T=T, cols=1)
                    mf, ch, nch = C.c_int32(), C.c_int64(), C.c_int64()
                    assert L.lib.qc_sweep_desc_launch(C.byref(D.d), S, C.byref(mf), C.byref(ch), C.byref(nch)) == L.QC_OK
                    got.append((bool(mf.value), ch.value, nch.value))
                want = tw.wide_launch(n, m, S, T)
                assert got[0] == got[1] == got[2] == (want["mfma"], want["chunk"], want["n_chunks"]), (n, m, S, T)


def test_scope_queries_follow_both_switches(qc):
    L = qc._lib
    rng = np.random.default_rng(0)
    UN = L.QC_FID_UNITARY

    def desc(flag, wide, **kw):
        D = too._ODesc(qc, flag=flag, wide=wide, **{**dict(N=16, m=2, cols=1, fid_kind=L.QC_FID_DENSITY), **kw})
        D.G0[:] = rng.standard_normal(D.G0.size)       # not antisymmetric
        return D

    old = "stored-state gradients are not served in the mfma32-sweep form"
    for fn, pre in (("qc_sweep_desc_grad_supported", "qc_sweep gradients: "), ("qc_sweep_desc_vjp_supported", "qc_sweep pullback: ")):
        for wide in (9, 11):
            assert too._query(qc, fn, desc(1, wide))[:2] == (L.QC_OK, 1), (fn, wide)                     # served
            rc, ok, msg = too._query(qc, fn, desc(0, wide))                                              # the bit alone: the closed scope
            assert (rc, ok) == (L.QC_OK, 0) and msg.startswith(pre) and "is not antisymmetric" in msg
            assert too._query(qc, fn, desc(1, wide, N=9))[:2] == (L.QC_OK, 1)                            # 2N = 18
            rc, ok, msg = too._query(qc, fn, desc(1, wide, N=12, cols=17, fid_kind=None))
            assert (rc, ok) == (L.QC_OK, 0) and "16 columns" in msg
            rc, ok, msg = too._query(qc, fn, desc(1, wide, N=17, cols=0, fid_kind=UN))
            assert (rc, ok) == (L.QC_OK, 0) and "2N = 34 > 32" in msg
            rc, ok, msg = too._query(qc, fn, desc(1, wide, N=12, m=9, cols=0, fid_kind=UN))
            assert (rc, ok) == (L.QC_OK, 0) and "9 drives > 8" in msg
            assert too._query(qc, fn, desc(1, wide, N=4))[:2] == (L.QC_OK, 1)                            # harmless on "mfma16-sweep"
        for wide in (1, 3):                                                                              # the old message, verbatim
            rc, ok, msg = too._query(qc, fn, desc(1, wide))
            assert (rc, ok) == (L.QC_OK, 0) and msg == pre + old, msg
    # no fidelity: the gradient refuses, the pullback serves
    rc, ok, msg = too._query(qc, "qc_sweep_desc_grad_supported", desc(1, 9, N=12, cols=3, fid_kind=None))
    assert (rc, ok) == (L.QC_OK, 0) and "no fidelity" in msg
    assert too._query(qc, "qc_sweep_desc_vjp_supported", desc(1, 9, N=12, cols=3, fid_kind=None))[:2] == (L.QC_OK, 1)
    # the forms that are out of scope on wide handles stay so
    for wide in (1, 9):
        rc, ok, msg = too._query(qc, "qc_sweep_desc_jvp_supported", desc(1, wide))
        assert (rc, ok) == (L.QC_OK, 0) and msg == "qc_sweep pushforward: pushforwards are not served in the mfma32-sweep form", msg
        rc, ok, msg9 = too._query(qc, "qc_sweep_desc_hvp_supported", desc(1, wide))
        assert (rc, ok) == (L.QC_OK, 0) and "is not antisymmetric" in msg9      # Hessian products keep the closed scope, whatever the switches


def test_python_keywords(qc):
    for f in (qc.RolloutSweep.__init__, qc.rollout_sweep, qc.rollout_sweep_parameter_gradient, qc.SweepInfidelityObjective.__init__,
              qc.SweepFinalStateObjective.__init__):
        par = inspect.signature(f).parameters
        assert "wide_stored" in par and par["wide_stored"].default is False, f
    rng = np.random.default_rng(0)
    sys9 = qc.QuantumSystem(_herm(rng, 9), [_herm(rng, 9)])
    for kw in (dict(), dict(wide=True), dict(stored_states=True)):      # before the library is touched: no device is needed to be told so
        with pytest.raises(ValueError, match="wide_stored"):
            qc.RolloutSweep(sys9, [], 5, wide_stored=True, **kw)


def test_julia_text(qc):
    julia = open(os.path.join(ROOT, "julia", "QCollocHIP.jl"), encoding="utf-8").read()
    assert julia.count("stored_states::Bool=false") == 4 and julia.count("wide_stored::Bool=false") == 4
    assert julia.count("(wide_stored ? 8 : 0)") == 4
    par = julia[julia.index("function rollout_sweep_parameter_gradient("):julia.index("function rollout_sweep_pullback(")]
    assert "wide ? 3 : 0" in par and "(wide ? 3 : 0) | (wide_stored ? 8 : 0)" in par
    pull = julia[julia.index("function rollout_sweep_pullback("):]
    pull = pull[:pull.index("\nend\n")]
    assert "(wide ? 1 : 0) | (wide_params ? 2 : 0) | (wide_stored ? 8 : 0)" in pull


def test_restated_generators_match_the_package(qc):
    for c in (two_qubit_case(qc, "two-qubit-lindblad", S=2, T=3), qutrit_case(qc, "qutrit-lindblad", S=2, T=3)):
        assert np.array_equal(c["G0"], c["system"].G_drift) and all(np.array_equal(a, b) for a, b in zip(c["Gd"], c["system"].G_drives))
        assert c["G0"].shape == (2 * c["N"], 2 * c["N"]) and np.abs(c["G0"] + c["G0"].T).max() > 0.05      # not antisymmetric


@pytest.mark.parametrize("name", list(CASES) + ["pullback-kets3"])
def test_reference_routes_agree(name):
    """Forward mode (expm_frechet) against central differences on the systems, rates and steps the GPU cases use: 1e-6 relative."""
    if name == "pullback-kets3":      # no fidelity on that handle: a ket fidelity on the same generators (same name, same draws) stands in
        c = too.nonherm_case(None, "pullback-kets3", 10, 2, 1, 3, 5, True, ("ket", None, "abs"))
        assert np.array_equal(c["G0"], _pullback_case(None)["G0"])
    else:
        c = CASES[name](None)
    err, big = oref.forward_vs_fd(c, c["samples"][:2])
    print(f"{name}: forward vs central differences {err:.2e}, max |grad| {big:.3e}")
    assert err < 1e-6 and big > 1e-6


# ---------------------------------------------------------------------------------------------------------------------------------
#  GPU
# ---------------------------------------------------------------------------------------------------------------------------------
def _handle(qc, c, params=False, stored=True, wide_stored=True, fid=True):
    return too._handle(qc, c, stored=stored, fid=fid, wide=True, wide_params=params, wide_stored=wide_stored)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_wide_stored_gradients_against_reference(qc, name):
    c = CASES[name](qc)
    lo, hi = squarings(c)      # the rule restated: the smallest sq with ||dt G||_1 / 2^sq <= 1/8
    if name == "sq0":
        assert hi == 0
    if name == "sq3":
        assert lo >= 3
    if name == "strong-dissipation":
        assert 35.0 < 10.0 * c["dts"][:c["T"] - 1].sum() < 50.0      # gamma sum h ~ 40: E^T is nowhere near E^-1
    sw = _handle(qc, c)
    assert sw.kernel_name == "mfma32-sweep" and sw.wide_stored and sw.stored_states and not sw.wide_params and sw.grad_supported
    if name == "two-qubit-lindblad":
        assert sw.launch(c["S"])[2] > 1 and (c["T"] - 1) % sw.launch(c["S"])[1] != 0      # several chunks, the last one short
    if name == "one-chunk":
        assert sw.launch(c["S"])[2] == 1
    Z = _Z(sw, c)
    S, sel = c["S"], c["samples"]
    w = np.random.default_rng(5).uniform(0.5, 1.5, S)
    w /= w.sum()
    want = _reference(name)
    J, f, g, gs = sw.grad(Z, c["init"], c["theta"], c["scale"], w, per_sample=True)
    assert np.array_equal(f, sw.eval(Z, c["init"], c["theta"], c["scale"], finals=False)[1]), "fids must carry the bits of qc_sweep_eval"
    if S <= 16:
        assert np.abs(f - oref.fidelities(c)).max() < 1e-9
    print(f"{name}: squarings {(lo, hi)}, max |grad| {np.abs(want['grad_samples']).max():.3e}")
    worst = _worst(gs[sel], want["grad_samples"], "grad_samples")
    assert abs(J - w @ f) < 1e-12
    if len(sel) == S:
        dense = np.zeros(sw.Z_len)
        K = dense[:sw.T * sw.zdim].reshape(sw.T, sw.zdim)
        acc = np.einsum("s,stk->tk", w, want["grad_samples"])
        K[:sw.T - 1, sw.off_a:sw.off_a + sw.m] = acc[:, :sw.m]
        if sw.off_dt >= 0:
            K[:sw.T - 1, sw.off_dt] = acc[:, sw.m]
        worst = max(worst, _worst(g[None], dense[None], "grad"))
    sw.close()
    print(f"SUMMARY {name}: worst error {worst:.3e} of its bound")


@pytest.mark.gpu
@pytest.mark.parametrize("name", PARAM_CASES)
def test_parameter_gradients_with_wide_11(qc, name):
    c = CASES[name](qc)
    sw = _handle(qc, c, params=True)
    assert sw.kernel_name == "mfma32-sweep" and sw.wide_stored and sw.wide_params and sw.grad_supported
    Z = _Z(sw, c)
    want = _reference(name)
    init, theta, scale = (np.ascontiguousarray(c[k]) for k in ("init", "theta", "scale"))
    w = np.full(c["S"], 1.0 / c["S"])
    names = ("fids", "J", "grad", "grad_samples", "grad_theta", "grad_scale")
    full = too._raw_grad_params(qc, sw, Z, init, theta, scale, w, names)
    worst = max(_worst(full["grad_theta"], want["grad_theta"], "grad_theta"), _worst(full["grad_scale"], want["grad_scale"], "grad_scale"),
                _worst(full["grad_samples"], want["grad_samples"], "grad_samples (parameter flavour)"))
    # the per-interval values do not depend on whether the parameter outputs are asked for, nor the parameter values on gs
    J, f, g, gs = sw.grad(Z, init, theta, scale, w, per_sample=True)
    assert np.array_equal(gs, full["grad_samples"]) and np.array_equal(g, full["grad"]) and np.array_equal(f, full["fids"])
    f2, gth, gsc = sw.param_grad(Z, init, theta, scale)      # gs = NULL
    assert np.array_equal(gth, full["grad_theta"]) and np.array_equal(gsc, full["grad_scale"]) and np.array_equal(f2, f)
    for k in ("grad_theta", "grad_scale"):
        assert np.array_equal(too._raw_grad_params(qc, sw, Z, init, theta, scale, w, (k,))[k], full[k]), k
    sw.close()
    print(f"SUMMARY parameters-{name}: worst error {worst:.3e} of its bound")


@pytest.mark.gpu
def test_pullback_against_reference(qc):
    c = _pullback_case(qc)
    cot = np.random.default_rng(11).standard_normal((c["S"], 2 * c["L"] * c["cols"]))
    want = vref.pullback_forward(c["G0"], c["Gd"], c["Gp"], c["controls"], c["dts"], c["init"], c["theta"], c["scale"], c["samples"], cot)
    sw9, sw11 = _handle(qc, c, fid=False), _handle(qc, c, params=True, fid=False)
    assert sw9.vjp_supported and not sw9.grad_supported and sw9.kernel_name == "mfma32-sweep" and sw9.cols == 3
    Z = _Z(sw9, c)
    g, gs, gi = sw9.vjp(Z, c["init"], cot, c["theta"], c["scale"], per_sample=True, init_grad=True)
    worst = max(_worst(gs, want["grad_samples"], "grad_samples"), _worst(gi, want["grad_init"], "grad_init"))
    g2, gs2, gi2, gth, gsc = sw11.vjp(Z, c["init"], cot, c["theta"], c["scale"], per_sample=True, init_grad=True, params=True)
    assert np.array_equal(gs2, gs) and np.array_equal(gi2, gi) and np.array_equal(g2, g)
    worst = max(worst, _worst(gth, want["grad_theta"], "grad_theta"), _worst(gsc, want["grad_scale"], "grad_scale"))
    acc = np.zeros_like(gs[0])          # grad: the plain sum in ascending s, +0.0 everywhere else
    for q in range(c["S"]):
        acc = acc + gs[q]
    K = g[:sw9.T * sw9.zdim].reshape(sw9.T, sw9.zdim).copy()
    assert np.array_equal(K[:sw9.T - 1, :sw9.n_deriv], acc)
    K[:sw9.T - 1, :sw9.n_deriv] = 0.0
    assert not K.any() and not np.signbit(K).any()
    # the final states of the pullback carry the bits of qc_sweep_eval
    L = qc._lib
    fin, gz = np.empty((c["S"], sw9.ns)), np.empty(sw9.Z_len)
    th, sc = np.ascontiguousarray(c["theta"]), np.ascontiguousarray(c["scale"])
    rc = L.lib.qc_sweep_vjp(sw9._h, L.dptr(Z), L.dptr(np.ascontiguousarray(c["init"])), c["S"], L.dptr(th), L.dptr(sc), L.dptr(cot), L.dptr(fin),
                            L.dptr(gz), None, None, None, None)
    assert rc == L.QC_OK and np.array_equal(gz, g)
    assert np.array_equal(fin.T, sw9.eval(Z, c["init"], c["theta"], c["scale"], fids=False)[0])
    sw9.close()
    sw11.close()
    print(f"SUMMARY pullback-kets3: worst error {worst:.3e} of its bound")


@pytest.mark.gpu
def test_closed_system_cross_check(qc, monkeypatch):
    """An antisymmetric 12-level system: wide = 9 with the flag (the stored-state walk) against wide = 1 (the closed walk) within the 1e-9
    rule, fids bit-equal; wide = 9 WITHOUT the flag is the closed walk, bit for bit."""
    rng = np.random.default_rng(12)
    Ln, m, S, T = 12, 3, 4, 8
    system = qc.QuantumSystem(_herm(rng, Ln), [_herm(rng, Ln, (Ln * m) ** -0.5) for _ in range(m)])
    perts = [_herm(rng, Ln)]
    init, goal = ref.operator_to_iso_vec(_unitary(rng, Ln)), ref.operator_to_iso_vec(_unitary(rng, Ln))
    controls, dts = rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T)
    theta, scale = rng.uniform(-0.3, 0.3, (S, 1)), rng.uniform(0.9, 1.1, (S, m))
    cot = rng.standard_normal((S, 2 * Ln * Ln))

    def outputs(**kw):
        sw = qc.RolloutSweep(system, perts, T, goal=goal, fid_kind="unitary", subspace=[0, 2, 3, 7], wide=True, **kw)
        assert sw.kernel_name == "mfma32-sweep" and sw.grad_supported
        Z = sw.pack(controls, dts)
        J, f, g, gs = sw.grad(Z, init, theta, scale, per_sample=True)
        vg, vgs, vgi = sw.vjp(Z, init, cot, theta, scale, per_sample=True, init_grad=True)
        wide = sw._desc.wide
        sw.close()
        return wide, dict(fids=f, J=np.array([J]), grad=g[None], grad_samples=gs, vjp_grad=vg[None], vjp_samples=vgs, vjp_init=vgi)

    w1, off = outputs()
    w9, on = outputs(stored_states=True, wide_stored=True)
    assert (w1, w9) == (1, 9)
    assert np.array_equal(off["fids"], on["fids"]) and off["J"][0] == on["J"][0]
    worst = max(_worst(on[k], off[k], k) for k in off if k not in ("fids", "J"))
    assert any(not np.array_equal(on[k], off[k]) for k in ("grad_samples", "vjp_samples")), "the flag must choose another walk"
    # wide = 9 without reserved1[0]: the constructor does not build that descriptor, so bit 0 carries bit 3 along for one handle
    monkeypatch.setattr(qc._lib, "QC_SWEEP_WIDE", 9)
    w9_alone, alone = outputs()
    monkeypatch.undo()
    assert w9_alone == 9
    for k in off:
        assert np.array_equal(alone[k], off[k]), k
    print(f"SUMMARY closed-cross-check: worst difference stored / closed walk {worst:.3e} of the bound")


@pytest.mark.gpu
def test_bit_level_properties(qc):
    import torch
    c = two_qubit_case(qc, "bits", S=6, T=8)
    sw = _handle(qc, c, params=True)
    Z = _Z(sw, c)
    init, theta, scale = (np.ascontiguousarray(c[k]) for k in ("init", "theta", "scale"))
    w = np.random.default_rng(3).uniform(0.5, 1.5, c["S"])
    names = ("fids", "J", "grad", "grad_samples", "grad_theta", "grad_scale")
    a = too._raw_grad_params(qc, sw, Z, init, theta, scale, w, names)
    for _ in range(5):      # six calls in all
        b = too._raw_grad_params(qc, sw, Z, init, theta, scale, w, names)
        for k in names:
            assert np.array_equal(a[k], b[k]), f"repeated calls: {k}"
    for k in names:
        assert np.array_equal(too._raw_grad_params(qc, sw, Z, init, theta, scale, w, (k,))[k], a[k]), f"{k} alone against {k} with every other output"
    # grad: +0.0 outside the controls and timesteps of knots 0 .. T-2
    K = a["grad"][:sw.T * sw.zdim].reshape(sw.T, sw.zdim).copy()
    assert np.abs(K[:sw.T - 1, :sw.n_deriv]).min() > 0.0
    K[:sw.T - 1, :sw.n_deriv] = 0.0
    rest = np.concatenate([K.ravel(), a["grad"][sw.T * sw.zdim:]])
    assert not rest.any() and not np.signbit(rest).any()
    # the device entry points give the bits of the host entry points
    dev = torch.device("cuda", 0)
    put = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    new = lambda *shape: torch.full(shape, np.nan, dtype=torch.float64, device=dev)
    S = c["S"]
    d = dict(fids=new(S), J=new(1), grad=new(sw.Z_len), grad_samples=new(S, sw.T - 1, sw.n_deriv), grad_theta=new(S, sw.p), grad_scale=new(S, sw.m))
    sw.param_grad_device(put(Z), put(init), S, put(theta), put(scale), put(w), d["fids"], d["J"], d["grad"], d["grad_samples"], d["grad_theta"],
                         d["grad_scale"])
    torch.cuda.synchronize()
    for k in names:
        assert np.array_equal(d[k].cpu().numpy().reshape(a[k].shape), a[k]), f"device against host: {k}"
    d2 = dict(fids=new(S), J=new(1), grad=new(sw.Z_len), grad_samples=new(S, sw.T - 1, sw.n_deriv))
    sw.grad_device(put(Z), put(init), S, put(theta), put(scale), put(w), d2["fids"], d2["J"], d2["grad"], d2["grad_samples"])
    torch.cuda.synchronize()
    for k in d2:
        assert np.array_equal(d2[k].cpu().numpy().reshape(a[k].shape), a[k]), f"qc_sweep_grad_dev against host: {k}"
    # a NaN in one sample's theta reaches that sample's outputs and grad, nothing else
    bad = theta.copy()
    bad[2, 0] = np.nan
    n = too._raw_grad_params(qc, sw, Z, init, bad, scale, w, names)
    keep = [s for s in range(S) if s != 2]
    for k in ("fids", "grad_samples", "grad_theta", "grad_scale"):
        assert not np.isfinite(n[k][2]).any(), k
        assert np.array_equal(n[k][keep], a[k][keep]), k
    assert not np.isfinite(n["J"]).any() and not np.isfinite(n["grad"][:(sw.T - 1) * sw.zdim].reshape(sw.T - 1, sw.zdim)[:, :sw.n_deriv]).any()
    sw.close()


@pytest.mark.gpu
def test_refusals_without_wide_params(qc):
    L = qc._lib
    c = qutrit_case(qc, "refusals", S=3, T=5)
    sw = _handle(qc, c)
    Z = _Z(sw, c)
    assert sw.grad_supported and sw.vjp_supported and not sw.jvp_supported and not sw.hvp_supported
    with pytest.raises(qc.QCollocError) as e:
        sw.param_grad(Z, c["init"], c["theta"], c["scale"])
    assert e.value.code == L.QC_ERR_UNSUPPORTED and "qc_sweep gradients: parameter gradients are not served in the mfma32-sweep form" in str(e.value)
    S = c["S"]
    cot, gth = np.ones((S, sw.ns)), np.empty((S, sw.p))
    th, sc = np.ascontiguousarray(c["theta"]), np.ascontiguousarray(c["scale"])
    rc = L.lib.qc_sweep_vjp(sw._h, L.dptr(Z), L.dptr(np.ascontiguousarray(c["init"])), S, L.dptr(th), L.dptr(sc), L.dptr(cot), None, None, None, None,
                            L.dptr(gth), None)
    assert rc == L.QC_ERR_UNSUPPORTED
    assert L.lib.qc_sweep_last_error(sw._h).decode() == "qc_sweep pullback: parameter cotangents are not served in the mfma32-sweep form"
    sw.close()
    # without the bit the handle refuses reverse mode as it always did; the forward sweep gives the same bits either way
    sw0 = _handle(qc, c, wide_stored=False)
    assert not sw0.grad_supported and "stored-state gradients are not served in the mfma32-sweep form" in sw0.grad_unsupported_reason
    sw1 = _handle(qc, c)
    for a, b in zip(sw1.eval(Z, c["init"], c["theta"], c["scale"]), sw0.eval(Z, c["init"], c["theta"], c["scale"])):
        assert np.array_equal(a, b)
    sw0.close()
    sw1.close()


@pytest.mark.gpu
def test_two_qubit_open_polish_example(qc):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import two_qubit_open_polish
    before, after = two_qubit_open_polish.polish(T=10, S=3, steps=6, verbose=False)
    print(f"mean infidelity over the detunings {before:.4e} -> {after:.4e}")
    assert after < before
