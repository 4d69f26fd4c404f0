"""Open-system sweep gradients in the "mfma64-sweep" form (32 < 2N <= 64): the stored-state walk on 4 x 4 tiles in LDS
(`qc_sweep_desc.wide` bit 18 = QC_SWEEP_WIDE_64_STORED together with bits 0, 10, 11 and `reserved1[0] = QC_SWEEP_STORED_STATES`;
`RolloutSweep(wide=True, wide64=True, wide64_grad=True, stored_states=True, wide64_stored=True)`; csrc/qc_sweep64_open_grad.hip).
A five-level transmon with relaxation and dephasing in the Lindblad form (N = 25, 2N = 50), 17 and 32 levels with a non-Hermitian
effective Hamiltonian (decay out of the top level), states of 1, 17 and 32 columns.

CPU: the bit field through `qc_sweep_desc_validate`, the device-free scope queries with flag and bit, the queries the bit must not
move, constants / keywords / header / Julia text, and the self-check of the reference (forward mode against central differences, 1e-6)
at the GPU cases' shapes.
GPU: every value of every sample against the forward-mode reference (tests/sweep_open_reference.py, tests/sweep_vjp_reference.py, as
they are).  Each case asserts through `launch` (the launch query) that the chunk shape it is meant for is reached.  The form's chunk
rule gives at most ceil(sqrt(T - 1)) chunks, so S = 1 at T = 9 walks chunks of 3, 3 and 2 intervals; chunks of ONE interval (the store
kernel's path without an exponential) are reached by T = 2 and by S = 255 at T = 3, and asserted there.

Tolerances, the suite's own: per sample |got - want| <= 1e-9 max(1, max |want of that sample|) (test_sweep_open_grad._worst);
`grad_init` rtol 1e-10 / atol 1e-11 (test_sweep_vjp); `fids` and `finals` against `qc_sweep_eval` bit for bit; `finals_autograd` against
central differences eps 1e-6, atol 1e-6 (test_sweep_wide64_grad)."""
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
import test_sweep_grad as tg
import test_sweep_open_grad as too
import test_sweep_vjp as tv
import test_sweep_wide as tw
import test_sweep_wide64 as t64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_herm, _unitary = ts._herm, ts._unitary
_worst, _Z = too._worst, too._Z
W64, WG, WP, WS = t64.W64, 2048, 8192, 262144
OPEN = 1 | W64 | WG | WS          # 265217
QUERIES = t64.QUERIES
HANDLE = dict(wide=True, wide64=True, wide64_grad=True, wide64_stored=True)


def transmon5_case(qc, name, S, T, free=True, gamma1=0.15, gamma2=0.1, dt=(0.1, 0.3), samples=None, dts=None, spread=0.3):
    """A five-level transmon with relaxation (sqrt(gamma1) a) and dephasing (sqrt(gamma2) a'a) in the Lindblad form: levels 5, N = 25,
    2N = 50 -- the last tile row and column are zero-padded from entry 2 on.  Two quadrature drives, a detuning as the perturbation, the
    density fidelity of one input state against a goal ket."""
    rng = np.random.default_rng(sum(map(ord, name)))
    a = np.diag(np.sqrt(np.arange(1.0, 5.0)), 1).astype(complex)
    num = a.conj().T @ a
    H0 = 0.2 * num - 0.15 * num @ (num - np.eye(5))
    Hd = [0.25 * (a + a.conj().T), 0.25j * (a - a.conj().T)]
    Ls = [np.sqrt(gamma1) * a, np.sqrt(gamma2) * num]
    Pz = oref.lindblad_generator(0.5 * num)
    v = _unitary(rng, 5)
    psi0, g = v[:, 0], v[:, 1]
    m = 2
    if dts is None:
        dts = rng.uniform(dt[0], dt[1], T) if free else 0.5 * (dt[0] + dt[1])
    c = dict(name=name, L=5, N=25, m=m, p=1, S=S, T=T, G0=oref.lindblad_generator(H0, Ls), Gd=[oref.lindblad_generator(H) for H in Hd], Gp=[Pz],
             init=oref.density_iso(np.outer(psi0, psi0.conj())), cols=1, goal=np.concatenate([g.real, g.imag]), kind="density", subspace=None,
             form="abs", controls=rng.uniform(-1, 1, (m, T)), dts=dts, theta=rng.uniform(-spread, spread, (S, 1)),
             scale=rng.uniform(1.0 - spread / 3, 1.0 + spread / 3, (S, m)), samples=list(range(S)) if samples is None else list(samples))
    c["system"] = qc.OpenQuantumSystem(H0, Hd, Ls) if qc is not None else None
    c["perts"] = [Pz]
    return c


def top_decay_case(qc, name, L, m, p, S, T, free, fid, cols=None, gamma=0.4, antisymmetric=False, samples=None):
    """H_eff = H - i (gamma / 2) |top><top|: decay out of the top level, iso generators that are not antisymmetric (`antisymmetric`: gamma = 0,
    a closed system).  fid = (kind, subspace, form) or None; cols: several kets without a fidelity."""
    rng = np.random.default_rng(sum(map(ord, name)))
    top = np.zeros((L, L), dtype=complex)
    top[L - 1, L - 1] = 1.0
    H0 = _herm(rng, L) - (0.0 if antisymmetric else 0.5j * gamma) * top
    Hd = [_herm(rng, L, (L * max(m, 1)) ** -0.5) for _ in range(m)]
    perts = [_herm(rng, L) - (0.0 if antisymmetric else 0.1j) * top for _ in range(p)]      # a detuning that also moves the loss rate
    kind, subspace, form = fid if fid is not None else (None, None, "abs")
    if kind == "unitary":
        init, ncol, goal = ref.operator_to_iso_vec(_unitary(rng, L)), L, ref.operator_to_iso_vec(_unitary(rng, L))
    else:
        ncol = cols or 1
        K = rng.standard_normal((L, ncol)) + 1j * rng.standard_normal((L, ncol))
        init = ref.operator_to_iso_vec(K / np.linalg.norm(K, axis=0))
        gk = rng.standard_normal(L) + 1j * rng.standard_normal(L)
        gk /= np.linalg.norm(gk)
        goal = np.concatenate([gk.real, gk.imag]) if kind else None
    c = dict(name=name, L=L, N=L, m=m, p=p, S=S, T=T, G0=ref.iso_generator(H0), Gd=[ref.iso_generator(H) for H in Hd],
             Gp=[ref.iso_generator(P) for P in perts], init=init, cols=ncol, goal=goal, kind=kind, subspace=subspace, form=form,
             controls=rng.uniform(-1, 1, (m, T)), dts=rng.uniform(0.1, 0.3, T) if free else 0.2, theta=rng.uniform(-0.3, 0.3, (S, p)),
             scale=rng.uniform(0.9, 1.1, (S, m)), samples=list(range(S)) if samples is None else list(samples))
    c["system"] = qc.QuantumSystem(H0, Hd) if qc is not None else None
    c["perts"] = perts
    c["cot"] = tv.unit_cotangents(rng, S, init.size)
    return c


def interval_squarings(c):
    """The rule of the kernels per (checked sample, interval): the smallest sq with ||dt G||_1 / 2^sq <= 1/8."""
    h = np.full(c["T"], c["dts"]) if np.ndim(c["dts"]) == 0 else c["dts"]
    out = np.zeros((len(c["samples"]), c["T"] - 1), dtype=int)
    for q, s in enumerate(c["samples"]):
        for t in range(c["T"] - 1):
            nrm = np.abs(h[t] * ref.sample_generator(c["G0"], c["Gd"], c["Gp"], c["controls"][:, t], c["theta"][s], c["scale"][s])).sum(axis=0).max()
            out[q, t] = 0 if nrm <= 0.125 else int(np.ceil(np.log2(nrm / 0.125)))
    return out


SQ_TARGETS = (3, 8, 0, 7, 1, 6, 2, 5, None, 4)      # None: the interval with h = 0
SQ_GAMMA = 0.5


def squarings_case(qc):
    """Relaxation at gamma1 = SQ_GAMMA with timesteps chosen per interval from sample 0's generator so that sq runs through
    SQ_TARGETS: every value 0 .. 8, neighbours differ, one interval with h = 0.  The samples differ little (spread 0.003), so every
    sample takes the same sq."""
    T = len(SQ_TARGETS) + 1
    c = transmon5_case(qc, "squarings", S=2, T=T, gamma1=SQ_GAMMA, gamma2=1.0, spread=0.003)
    h = np.zeros(T)
    for t, q in enumerate(SQ_TARGETS):
        if q is not None:
            nrm = np.abs(ref.sample_generator(c["G0"], c["Gd"], c["Gp"], c["controls"][:, t], c["theta"][0], c["scale"][0])).sum(axis=0).max()
            h[t] = 0.75 * 2.0 ** q / 8.0 / nrm
    h[T - 1] = 0.1
    c["dts"] = h
    return c


U17 = ("unitary", [0, 1, 3, 4], "abs")
# the GPU cases of the gradient: name -> case
CASES = {
    "lindblad5": lambda qc: transmon5_case(qc, "lindblad5", S=4, T=9),                                     # chunks 3, 3, 2
    "lindblad5-fixed-dt": lambda qc: transmon5_case(qc, "lindblad5-fixed-dt", S=4, T=9, free=False),
    "topdecay17-ket": lambda qc: top_decay_case(qc, "topdecay17-ket", 17, 2, 1, 3, 6, True, ("ket", None, "abs")),
    "squarings": squarings_case,
    "strong-dissipation": lambda qc: transmon5_case(qc, "strong-dissipation", S=3, T=9, gamma1=10.0, gamma2=2.0, dt=(0.4, 0.6)),
    "S1-T9": lambda qc: transmon5_case(qc, "S1-T9", S=1, T=9),                                              # one sample: chunks 3, 3, 2
    "one-interval": lambda qc: top_decay_case(qc, "one-interval", 17, 2, 1, 3, 2, True, ("ket", None, "abs")),      # T = 2
    "S259-T3": lambda qc: top_decay_case(qc, "S259-T3", 17, 1, 1, 259, 3, True, ("ket", None, "abs")),      # one chunk of two intervals
    "S255-T3": lambda qc: top_decay_case(qc, "S255-T3", 17, 1, 1, 255, 3, True, ("ket", None, "abs")),      # two chunks of one interval
}
# what `launch` must answer: (chunk, n_chunks)
SHAPES = {"lindblad5": (3, 3), "lindblad5-fixed-dt": (3, 3), "topdecay17-ket": (2, 3), "squarings": (3, 4), "strong-dissipation": (3, 3), "S1-T9": (3, 3), "one-interval": (1, 1),
          "S259-T3": (2, 1), "S255-T3": (1, 2)}
PARAM_CASES = ("lindblad5", "lindblad5-fixed-dt")
# the pullback's cases: several columns, no fidelity
VJP_CASES = {
    "topdecay17-cols17": lambda qc: top_decay_case(qc, "topdecay17-cols17", 17, 2, 1, 3, 5, True, None, cols=17),      # nct = 2, one live column in the second tile
    "topdecay32-cols32": lambda qc: top_decay_case(qc, "topdecay32-cols32", 32, 2, 1, 2, 4, True, None, cols=32),      # no padding anywhere
}


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The forward-mode derivatives of a case, computed once and shared (read-only) by the tests that need them."""
    if name in VJP_CASES:
        c = VJP_CASES[name](None)
        out = vref.pullback_forward(c["G0"], c["Gd"], c["Gp"], c["controls"], c["dts"], c["init"], c["theta"], c["scale"], c["samples"], c["cot"])
    else:
        out = oref.grad_forward(CASES[name](None))
    for v in out.values():
        v.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
#  CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_wide64_stored_field_is_validated(qc):
    L = qc._lib
    val = lambda D: L.lib.qc_sweep_desc_validate(C.byref(D.d))
    assert L.QC_SWEEP_WIDE_64_STORED == WS == 1 << 18
    for N in (25, 12, 2):
        for bad in (WS, WS | 1, WS | 1025, WS | 1 | 2048, WS | 3073 | (1 << 19), WS | 3073 | (1 << 17), WS | 3073 | (1 << 20), (1 << 19) | 3073):
            assert val(tw._wdesc(qc, bad, N=N)) == L.QC_ERR_INVALID, (N, bad)
            text = L.lib.qc_sweep_last_error(None).decode()
            assert text.startswith("qc_sweep: wide"), text
            for words in ("17, 19, 25 or 27", "QC_SWEEP_WIDE_TANGENT (16)", "QC_SWEEP_WIDE_NOISE (64)", "QC_SWEEP_WIDE_HESSIAN (256)", "QC_SWEEP_WIDE_64 (1024)",
                          "QC_SWEEP_WIDE_64_GRAD (2048)", "QC_SWEEP_WIDE_64_PARAMS (8192)", "QC_SWEEP_WIDE_64_TANGENT (16384)",
                          "QC_SWEEP_WIDE_64_NOISE (65536)", "QC_SWEEP_WIDE_64_STORED (262144)"):
                assert words in text, (words, text)
        for good in (WS | 3073, WS | 3073 | 8192, WS | 3073 | 16384, WS | 3073 | 65536, WS | 3073 | 8192 | 16384 | 65536):
            assert val(tw._wdesc(qc, good, N=N)) == L.QC_OK, (N, good)
        # every value valid before the bit stays valid, and gains the bit exactly when it has bits 0, 10 and 11
        for v in t64._valid_today():
            for hi in (0, W64, W64 | WG, W64 | WG | WP, W64 | 16384, W64 | 65536, W64 | WG | 65536):
                if v == 0 and hi:
                    continue
                assert val(tw._wdesc(qc, v | hi, N=N)) == L.QC_OK, (N, v | hi)
                want = L.QC_OK if (v & 1) and (hi & W64) and (hi & WG) else L.QC_ERR_INVALID
                assert val(tw._wdesc(qc, v | hi | WS, N=N)) == want, (N, v | hi | WS)
    ok = C.c_int32(-1)
    assert L.lib.qc_sweep_desc_grad_supported(C.byref(tw._wdesc(qc, WS | 1025, N=25).d), C.byref(ok)) == L.QC_ERR_INVALID


def _desc(qc, wide, stored=0, lindblad=False, **kw):
    D = tg._GDesc(qc, **kw)
    if lindblad:
        D.G0[:] = np.random.default_rng(0).standard_normal(D.G0.size)       # not antisymmetric
    D.d.wide = wide
    D.d.reserved1[0] = stored
    return D


def test_scope_queries_follow_flag_and_bit(qc):
    L = qc._lib
    DEN, KET, UN = L.QC_FID_DENSITY, L.QC_FID_KET, L.QC_FID_UNITARY
    lind = dict(lindblad=True, N=25, m=2, cols=1, fid_kind=DEN)
    for wide in (OPEN, OPEN | WP, OPEN | 346):
        for which in ("grad", "vjp"):
            assert t64._query(qc, which, _desc(qc, wide, 1, **lind)) == (L.QC_OK, 1, None), (which, wide)                    # flag and bit: served
            assert t64._query(qc, which, _desc(qc, wide, 1, lindblad=True, N=17, m=2, cols=1, fid_kind=KET)) == (L.QC_OK, 1, None)
            rc, ok, text = t64._query(qc, which, _desc(qc, wide, 0, **lind))                                                 # the bit alone: the closed scope
            assert (rc, ok) == (L.QC_OK, 0) and "G_drift is not antisymmetric" in text, text
            rc, ok, text = t64._query(qc, which, _desc(qc, wide, 1, lindblad=True, N=17, m=2, cols=33))
            assert (rc, ok) == (L.QC_OK, 0) and "32 columns" in text and "mfma64-sweep" in text and "2N = 34" in text and "state_cols = 33" in text, text
            rc, ok, text = t64._query(qc, which, _desc(qc, wide, 1, lindblad=True, N=17, m=18, cols=1, fid_kind=KET))
            assert (rc, ok) == (L.QC_OK, 0) and "rollout-per-sample" in text and "18 drives > 16" in text, text
        assert t64._query(qc, "vjp", _desc(qc, wide, 1, lindblad=True, N=17, m=2, cols=17)) == (L.QC_OK, 1, None)
        assert t64._query(qc, "vjp", _desc(qc, wide, 1, lindblad=True, N=32, m=2, cols=32)) == (L.QC_OK, 1, None)
        rc, ok, text = t64._query(qc, "grad", _desc(qc, wide, 1, lindblad=True, N=17, m=2, cols=17))
        assert (rc, ok) == (L.QC_OK, 0) and "no fidelity" in text
        # antisymmetric generators are served with the flag as well
        assert t64._query(qc, "grad", _desc(qc, wide, 1, N=17, m=2, fid_kind=UN)) == (L.QC_OK, 1, None)
    # the flag without the bit: the refusal it always had, text for text
    for wide in (1 | W64 | WG, 1 | W64 | WG | WP):
        for which, pre in (("grad", "qc_sweep gradients: "), ("vjp", "qc_sweep pullback: ")):
            rc, ok, text = t64._query(qc, which, _desc(qc, wide, 1, **lind))
            assert (rc, ok) == (L.QC_OK, 0) and text == pre + "the handle takes the mfma64-sweep form (2N = 50), which does not serve stored-state gradients", text
    # N = 16 and below ignore the bit: every answer and every text is that of the descriptor without it
    for kw, lindblad, stored in ((dict(N=16, m=2, cols=1, fid_kind=DEN), True, 1), (dict(N=16, m=2, cols=1, fid_kind=DEN), True, 0),
                                 (dict(N=12, m=2, fid_kind=UN), False, 1), (dict(N=4, m=2, cols=1, fid_kind=DEN), True, 1), (dict(N=12, m=2, cols=17), False, 1)):
        for low in (1, 9, 11, 347):
            answers = [[t64._query(qc, which, _desc(qc, low | W64 | WG | bit, stored, lindblad, **kw)) for which in QUERIES] for bit in (0, WS)]
            assert answers[0] == answers[1], (kw, lindblad, stored, low)
    assert t64._query(qc, "grad", _desc(qc, 9 | W64 | WG | WS, 1, lindblad=True, N=16, m=2, cols=1, fid_kind=DEN)) == (L.QC_OK, 1, None)


def test_other_queries_do_not_see_the_bit(qc):
    """hvp, noise, noise_grad, jvp and the launch rule answer with the bit what they answer without it, text for text."""
    L = qc._lib
    others = [q for q in QUERIES if q not in ("grad", "vjp")]
    assert {"hvp", "jvp", "noise"} <= set(others)
    kinds = (dict(lindblad=True, N=25, m=2, p=1, cols=1, fid_kind=L.QC_FID_DENSITY), dict(N=17, m=2, p=1, cols=1, fid_kind=L.QC_FID_KET),
             dict(N=27, m=6, p=1, fid_kind=L.QC_FID_UNITARY), dict(lindblad=True, N=17, m=2, cols=33))
    for kw in kinds:
        for stored in (0, 1):
            for base in (1 | W64 | WG, 1 | W64 | WG | WP, 1 | W64 | WG | 16384, 1 | W64 | WG | 65536, 1 | W64 | WG | WP | 16384 | 65536):
                for which in others:
                    assert t64._query(qc, which, _desc(qc, base, stored, **kw)) == t64._query(qc, which, _desc(qc, base | WS, stored, **kw)), (which, kw, stored, base)
    # the noise gradient keeps its closed scope on an open handle
    D = _desc(qc, OPEN | 65536, 1, lindblad=True, N=25, m=2, p=1, cols=1, fid_kind=L.QC_FID_DENSITY)
    if "noise_grad" in QUERIES:
        rc, ok, text = t64._query(qc, "noise_grad", D)
        assert (rc, ok) == (L.QC_OK, 0) and "is not antisymmetric" in text, text
    rc, ok, text = t64._query(qc, "hvp", D)
    assert (rc, ok) == (L.QC_OK, 0) and "mfma64-sweep" in text and "Hessian products" in text, text

    def launch(n, m, S, T, wide):
        D = tw._wdesc(qc, wide, N=n // 2, m=m, T=T, cols=1)
        mf, ch, nch = C.c_int32(), C.c_int64(), C.c_int64()
        assert L.lib.qc_sweep_desc_launch(C.byref(D.d), S, C.byref(mf), C.byref(ch), C.byref(nch)) == L.QC_OK
        return bool(mf.value), ch.value, nch.value

    for n in (16, 32, 34, 50, 64):
        for m in (1, 16, 17):
            for S, T in ((1, 2), (1, 9), (2, 102), (4, 9), (255, 3), (256, 3), (259, 3), (8192, 1000)):
                want = t64.launch64(n, m, S, T, 1 | W64)
                assert launch(n, m, S, T, OPEN) == launch(n, m, S, T, 1 | W64 | WG) == (want["mfma"], want["chunk"], want["n_chunks"]), (n, m, S, T)
    # the GPU cases reach the chunk shapes they are meant for
    for name, make in list(CASES.items()) + list(VJP_CASES.items()):
        c = make(None)
        f = t64.launch64(2 * c["N"], c["m"], c["S"], c["T"], OPEN)
        assert f["mfma"] and 32 < 2 * c["N"] <= 64, name
        if name in SHAPES:
            assert (f["chunk"], f["n_chunks"]) == SHAPES[name], (name, f)
    assert t64.launch64(34, 1, 255, 3, OPEN)["last"] == 1 and t64.launch64(50, 2, 1, 9, OPEN)["last"] == 2


def test_constants_keywords_and_texts(qc, tmp_path):
    L = qc._lib
    header = open(os.path.join(ROOT, "include", "qcolloc.h")).read()
    assert re.search(r"^#define QC_SWEEP_WIDE_64_STORED 262144\b", header, re.M) and L.lib.qc_abi_version() == 6
    for words in ("Bit 18, QC_SWEEP_WIDE_64_STORED", "qc_sweep64_open_grad.hip", "50 doubles a knot", "432 for eight columns at 27 levels"):
        assert words in header, words
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "qcolloc.h"\nint main(){printf("%zu %d\\n", sizeof(qc_sweep_desc), QC_SWEEP_WIDE_64_STORED);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [128, 262144] and L.lib.qc_sizeof_sweep_desc() == C.sizeof(L.qc_sweep_desc) == 128
    for f in (qc.RolloutSweep.__init__, qc.SweepInfidelityObjective.__init__, qc.SweepFinalStateObjective.__init__, qc.rollout_sweep_parameter_gradient):
        p = inspect.signature(f).parameters
        assert p["wide64_stored"].default is False and list(p)[-1] == "wide64_params", f
    assert "wide64_stored" in qc.RolloutSweep.__doc__ and "wide64_stored" in qc.SweepInfidelityObjective.__doc__
    assert "wide64_stored" in qc.SweepFinalStateObjective.__doc__
    assert isinstance(qc.RolloutSweep.wide64_stored, property)
    # refused before the library is touched: no system is looked at
    for kw in (dict(), dict(wide=True, wide64=True, wide64_grad=True), dict(stored_states=True), dict(wide=True, wide64=True, stored_states=True)):
        with pytest.raises(ValueError, match="wide64_stored=True needs wide64_grad=True and stored_states=True"):
            qc.RolloutSweep(None, [], 5, wide64_stored=True, **kw)
    julia = open(os.path.join(ROOT, "julia", "QCollocHIP.jl"), encoding="utf-8").read()
    assert "const QC_SWEEP_WIDE_64_STORED = 262144" in julia and julia.count("wide64_stored::Bool=false") == 3
    assert julia.count("(wide64_stored ? QC_SWEEP_WIDE_64_STORED : 0)") == 3
    for fn in ("function rollout_sweep_gradient(", "function rollout_sweep_pullback(", "function rollout_sweep_parameter_gradient("):
        body = julia[julia.index(fn):]
        body = body[:body.index("\nend\n")]
        assert "wide64_stored::Bool=false" in body and "QC_SWEEP_WIDE_64_STORED" in body, fn
    for doc in ("DESIGN.md", "README.md"):
        text = open(os.path.join(ROOT, doc), encoding="utf-8").read()
        assert "QC_SWEEP_WIDE_64_STORED" in text and "qc_sweep64_open_grad.hip" in text, doc
    assert "5.8.17" in open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    # no new exported symbol; the new file is built
    names = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "qc_sweep_grad" in names and "sweep64" not in names
    kernel = open(os.path.join(ROOT, "quantumcollocation.jl_amd", "csrc", "qc_sweep64_open_grad.hip")).read()
    assert "qc_sweep64_open_store_kernel" in kernel and "qc_sweep64_open_grad_kernel" in kernel and "Barriers of one interval" in kernel
    assert "qc_sweep64_open_grad.hip" in open(os.path.join(ROOT, "quantumcollocation.jl_amd", "csrc", "Makefile")).read()


def test_restated_generators_match_the_package(qc):
    c = transmon5_case(qc, "lindblad5", S=2, T=3)
    assert np.array_equal(c["G0"], c["system"].G_drift) and all(np.array_equal(a, b) for a, b in zip(c["Gd"], c["system"].G_drives))
    assert c["G0"].shape == (50, 50) and np.abs(c["G0"] + c["G0"].T).max() > 0.05      # not antisymmetric
    c = top_decay_case(qc, "topdecay17-ket", 17, 2, 1, 2, 3, True, ("ket", None, "abs"))
    assert np.array_equal(c["G0"], c["system"].G_drift) and np.abs(c["G0"] + c["G0"].T).max() > 0.1
    c = top_decay_case(qc, "closed17", 17, 2, 1, 2, 3, True, U17, antisymmetric=True)
    assert np.abs(c["G0"] + c["G0"].T).max() == 0.0


def test_squarings_case_is_what_it_says():
    c = squarings_case(None)
    sq = interval_squarings(c)
    want = [0 if q is None else q for q in SQ_TARGETS]
    assert all(list(row) == want for row in sq), sq
    assert sorted(set(want)) == list(range(9)) and all(a != b for a, b in zip(want, want[1:]))
    h = c["dts"][:c["T"] - 1]
    assert h[SQ_TARGETS.index(None)] == 0.0 and np.all(np.delete(h, SQ_TARGETS.index(None)) > 0.0)
    d = CASES["strong-dissipation"](None)
    assert 35.0 < 10.0 * d["dts"][:d["T"] - 1].sum() < 50.0      # gamma sum h ~ 40: E^T is nowhere near E^-1


@pytest.mark.parametrize("name", list(CASES) + list(VJP_CASES))
def test_reference_routes_agree(name):
    """Forward mode (expm_frechet) against central differences on the systems, rates and steps the GPU cases use: 1e-6 relative."""
    if name in VJP_CASES:      # no fidelity on those handles: a ket fidelity on the same generators (same name) stands in
        v = VJP_CASES[name](None)
        c = top_decay_case(None, name, v["L"], v["m"], v["p"], v["S"], v["T"], True, ("ket", None, "abs"))
        assert np.array_equal(c["G0"], v["G0"]) and all(np.array_equal(a, b) for a, b in zip(c["Gd"] + c["Gp"], v["Gd"] + v["Gp"]))
    else:
        c = CASES[name](None)
    err, big = oref.forward_vs_fd(c, c["samples"][:2])
    print(f"{name}: forward vs central differences {err:.2e}, max |grad| {big:.3e}")
    assert err < 1e-6 and big > 1e-6


# ---------------------------------------------------------------------------------------------------------------------------------
#  GPU
# ---------------------------------------------------------------------------------------------------------------------------------
def _handle(qc, c, params=False, stored=True, bit=True, fid=True, **kw):
    flags = dict(HANDLE, wide64_stored=bit and stored, wide64_params=params, **kw)
    return too._handle(qc, c, stored=stored, fid=fid, **flags)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_open_gradients_against_reference(qc, name):
    c = CASES[name](qc)
    sw = _handle(qc, c)
    assert sw.kernel_name == "mfma64-sweep" and sw.wide64_stored and sw.stored_states and sw.grad_supported and sw._desc.wide == OPEN
    mf, chunk, n_chunks = sw.launch(c["S"])
    assert mf and (chunk, n_chunks) == SHAPES[name], (chunk, n_chunks)
    Z = _Z(sw, c)
    S, sel = c["S"], c["samples"]
    w = np.random.default_rng(5).uniform(0.5, 1.5, S)
    w /= w.sum()
    want = _reference(name)
    J, f, g, gs = sw.grad(Z, c["init"], c["theta"], c["scale"], w, per_sample=True)
    assert np.array_equal(f, sw.eval(Z, c["init"], c["theta"], c["scale"], finals=False)[1]), "fids must carry the bits of qc_sweep_eval"
    if S <= 16:
        assert np.abs(f - oref.fidelities(c)).max() < 1e-9
    sq = interval_squarings(c)
    print(f"{name}: squarings {sq.min()} .. {sq.max()}, max |grad| {np.abs(want['grad_samples']).max():.3e}")
    if name == "squarings":
        k0 = SQ_TARGETS.index(None)
        assert np.isfinite(gs[:, k0]).all() and np.all(gs[:, k0, :c["m"]] == 0.0) and np.abs(want["grad_samples"][:, k0, c["m"]]).min() > 1e-6
    worst = _worst(gs[sel], want["grad_samples"], "grad_samples")
    assert abs(J - w @ f) < 1e-12
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
def test_parameter_gradients_with_wide64_params(qc, name):
    c = CASES[name](qc)
    sw = _handle(qc, c, params=True)
    assert sw.kernel_name == "mfma64-sweep" and sw.wide64_stored and sw.wide64_params and sw._desc.wide == OPEN | WP
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
    plain = _handle(qc, c)      # the handle without QC_SWEEP_WIDE_64_PARAMS: the flavour <false>
    assert np.array_equal(plain.grad(Z, init, theta, scale, w, per_sample=True)[3], gs), "grad_samples must not depend on the flavour"
    plain.close()
    f2, gth, gsc = sw.param_grad(Z, init, theta, scale)      # gs = NULL
    assert np.array_equal(gth, full["grad_theta"]) and np.array_equal(gsc, full["grad_scale"]) and np.array_equal(f2, f)
    for k in ("grad_theta", "grad_scale"):
        assert np.array_equal(too._raw_grad_params(qc, sw, Z, init, theta, scale, w, (k,))[k], full[k]), k
    sw.close()
    print(f"SUMMARY parameters-{name}: worst error {worst:.3e} of its bound")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(VJP_CASES))
def test_pullback_against_reference(qc, name):
    c = VJP_CASES[name](qc)
    cot = c["cot"]
    want = _reference(name)
    sw, swp = _handle(qc, c, fid=False), _handle(qc, c, params=True, fid=False)
    assert sw.vjp_supported and not sw.grad_supported and sw.kernel_name == "mfma64-sweep" and sw.cols == c["cols"]
    assert sw.launch(c["S"])[2] > 1
    Z = _Z(sw, c)
    g, gs, gi = sw.vjp(Z, c["init"], cot, c["theta"], c["scale"], per_sample=True, init_grad=True)
    worst = _worst(gs, want["grad_samples"], "grad_samples")
    np.testing.assert_allclose(gi, want["grad_init"], rtol=1e-10, atol=1e-11)
    g2, gs2, gi2, gth, gsc = swp.vjp(Z, c["init"], cot, c["theta"], c["scale"], per_sample=True, init_grad=True, params=True)
    assert np.array_equal(gs2, gs) and np.array_equal(gi2, gi) and np.array_equal(g2, g)
    worst = max(worst, _worst(gth, want["grad_theta"], "grad_theta"), _worst(gsc, want["grad_scale"], "grad_scale"))
    acc = np.zeros_like(gs[0])          # grad: the plain sum in ascending s, +0.0 everywhere else
    for q in range(c["S"]):
        acc = acc + gs[q]
    K = g[:sw.T * sw.zdim].reshape(sw.T, sw.zdim).copy()
    assert np.array_equal(K[:sw.T - 1, :sw.n_deriv], acc)
    K[:sw.T - 1, :sw.n_deriv] = 0.0
    assert not K.any() and not np.signbit(K).any()
    # the final states of the pullback carry the bits of qc_sweep_eval
    L = qc._lib
    fin, gz = np.empty((c["S"], sw.ns)), np.empty(sw.Z_len)
    th, sc = np.ascontiguousarray(c["theta"]), np.ascontiguousarray(c["scale"])
    rc = L.lib.qc_sweep_vjp(sw._h, L.dptr(Z), L.dptr(np.ascontiguousarray(c["init"])), c["S"], L.dptr(th), L.dptr(sc), L.dptr(cot), L.dptr(fin),
                            L.dptr(gz), None, None, None, None)
    assert rc == L.QC_OK and np.array_equal(gz, g)
    assert np.array_equal(fin.T, sw.eval(Z, c["init"], c["theta"], c["scale"], fids=False)[0])
    sw.close()
    swp.close()
    print(f"SUMMARY pullback-{name}: worst error {worst:.3e} of its bound")


@pytest.mark.gpu
def test_closed_system_cross_check(qc):
    """An antisymmetric 17-level system: flag and bit on (the stored-state walk) against the closed walk of the same descriptor without
    them, within the 1e-9 rule; fids and finals bit-equal."""
    c = top_decay_case(qc, "closed17", 17, 3, 1, 4, 8, True, U17, antisymmetric=True)
    cot = tv.unit_cotangents(np.random.default_rng(12), c["S"], c["init"].size)

    def outputs(stored):
        sw = _handle(qc, c, stored=stored)
        assert sw.kernel_name == "mfma64-sweep" and sw.grad_supported and sw.launch(c["S"])[2] > 1
        Z = _Z(sw, c)
        J, f, g, gs = sw.grad(Z, c["init"], c["theta"], c["scale"], per_sample=True)
        vg, vgs, vgi = sw.vjp(Z, c["init"], cot, c["theta"], c["scale"], per_sample=True, init_grad=True)
        fin = sw.eval(Z, c["init"], c["theta"], c["scale"], fids=False)[0]
        wide = sw._desc.wide
        sw.close()
        return wide, dict(fids=f, J=np.array([J]), finals=fin, grad=g[None], grad_samples=gs, vjp_grad=vg[None], vjp_samples=vgs, vjp_init=vgi)

    w_off, off = outputs(False)
    w_on, on = outputs(True)
    assert (w_off, w_on) == (1 | W64 | WG, OPEN)
    assert np.array_equal(off["fids"], on["fids"]) and off["J"][0] == on["J"][0] and np.array_equal(off["finals"], on["finals"])
    worst = max(_worst(on[k], off[k], k) for k in off if k not in ("fids", "J", "finals"))
    assert any(not np.array_equal(on[k], off[k]) for k in ("grad_samples", "vjp_samples")), "flag and bit must choose another walk"
    print(f"SUMMARY closed-cross-check: worst difference stored / closed walk {worst:.3e} of the bound")


@pytest.mark.gpu
def test_bits_host_device_side_stream_and_scratch(qc):
    """Repeated calls return identical bits; the host and device entry points agree bit for bit, on a side stream; a handle whose dXall
    grows, shrinks and is reused (S = 5, 2, 5) returns the bits of a fresh handle at every S, for `grad`, `param_grad` and `vjp`."""
    import torch
    c = transmon5_case(qc, "bits", S=5, T=8)
    rng = np.random.default_rng(8)
    sw = _handle(qc, c, params=True)
    Z = _Z(sw, c)
    init = np.ascontiguousarray(c["init"])
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    side = torch.cuda.Stream(device=dev)
    names = ("fids", "J", "grad", "grad_samples", "grad_theta", "grad_scale")
    try:
        for S in (5, 2, 5):
            theta, scale, w = rng.uniform(-0.3, 0.3, (S, 1)), rng.uniform(0.9, 1.1, (S, 2)), rng.uniform(0.5, 1.5, S)
            cot = tv.unit_cotangents(rng, S, sw.ns)
            fresh = _handle(qc, c, params=True)
            first = too._raw_grad_params(qc, fresh, Z, init, theta, scale, w, names)
            first_v = fresh.vjp(Z, init, cot, theta, scale, per_sample=True, init_grad=True)
            fresh.close()
            for _ in range(3):
                again = too._raw_grad_params(qc, sw, Z, init, theta, scale, w, names)
                for k in names:
                    np.testing.assert_array_equal(again[k], first[k], err_msg=k)
                for a, b in zip(sw.vjp(Z, init, cot, theta, scale, per_sample=True, init_grad=True), first_v):
                    np.testing.assert_array_equal(a, b)
            for k in names:
                assert np.array_equal(too._raw_grad_params(qc, sw, Z, init, theta, scale, w, (k,))[k], first[k]), f"{k} alone against {k} with every other output"
            assert np.isfinite(first["grad_samples"]).all() and np.abs(first["grad_samples"]).max() > 1e-3
            mk = lambda *shape: torch.full(shape, -7.0, dtype=torch.float64, device=dev)
            d = dict(fids=mk(S), J=mk(1), grad=mk(sw.Z_len), grad_samples=mk(S, sw.T - 1, sw.n_deriv), grad_theta=mk(S, sw.p), grad_scale=mk(S, sw.m))
            sw.param_grad_device(t(Z), t(init), S, t(theta), t(scale), t(w), d["fids"], d["J"], d["grad"], d["grad_samples"], d["grad_theta"], d["grad_scale"])
            torch.cuda.synchronize()
            for k in names:
                np.testing.assert_array_equal(d[k].cpu().numpy().reshape(first[k].shape), first[k], err_msg=f"device against host: {k}")
            dfid, dJ, dg, dgs = mk(S), mk(1), mk(sw.Z_len), mk(S, sw.T - 1, sw.n_deriv)
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                sw.grad_device(t(Z), t(init), S, t(theta), t(scale), t(w), dfid, dJ, dg, dgs, stream=side)
            side.synchronize()
            for k, a in (("fids", dfid), ("J", dJ), ("grad", dg), ("grad_samples", dgs)):
                np.testing.assert_array_equal(a.cpu().numpy().reshape(first[k].shape), first[k], err_msg=f"side stream: {k}")
            with torch.cuda.stream(side):
                out = tv.device_call(sw, Z, dict(S=S, init=init, theta=theta, scale=scale, cot=cot), ["grad", "grad_samples", "grad_init"], stream=side)
            for k, b in zip(("grad", "grad_samples", "grad_init"), first_v):
                np.testing.assert_array_equal(out[k], b, err_msg=k)
        # a NaN in one sample's theta is evaluated: it reaches that sample's outputs and grad, nothing else
        bad = theta.copy()
        bad[2, 0] = np.nan
        n = too._raw_grad_params(qc, sw, Z, init, bad, scale, w, names)
        keep = [s for s in range(S) if s != 2]
        for k in ("fids", "grad_samples", "grad_theta", "grad_scale"):
            assert not np.isfinite(n[k][2]).any(), k
            assert np.array_equal(n[k][keep], first[k][keep]), k
    finally:
        sw.close()


@pytest.mark.gpu
def test_refusals_on_live_handles(qc):
    L = qc._lib
    UNS = L.QC_ERR_UNSUPPORTED
    c = transmon5_case(qc, "refusals", S=3, T=5)
    sw = _handle(qc, c, wide64_noise=True)          # flag and bit, no QC_SWEEP_WIDE_64_PARAMS
    Z = _Z(sw, c)
    S = c["S"]
    args = (Z, c["init"], c["theta"], c["scale"])
    try:
        assert sw.grad_supported and sw.vjp_supported and not sw.hvp_supported and not sw.jvp_supported and np.isfinite(sw.grad(*args)[2]).all()
        with pytest.raises(qc.QCollocError) as e:
            sw.param_grad(*args)
        assert e.value.code == UNS and "qc_sweep gradients: parameter gradients are not served in the mfma64-sweep form (2N = 50)" in str(e.value)
        cot, gth = np.ones((S, sw.ns)), np.empty((S, sw.p))
        th, sc = np.ascontiguousarray(c["theta"]), np.ascontiguousarray(c["scale"])
        rc = L.lib.qc_sweep_vjp(sw._h, L.dptr(Z), L.dptr(np.ascontiguousarray(c["init"])), S, L.dptr(th), L.dptr(sc), L.dptr(cot), None, None, None, None,
                                L.dptr(gth), None)
        assert rc == UNS
        assert L.lib.qc_sweep_last_error(sw._h).decode() == "qc_sweep pullback: parameter cotangents are not served in the mfma64-sweep form (2N = 50)"
        with pytest.raises(qc.QCollocError) as e:
            sw.hvp(Z, c["init"], cot, c["theta"], c["scale"], vZ=np.ones(sw.Z_len))
        assert e.value.code == UNS and "mfma64-sweep" in str(e.value) and "Hessian products" in str(e.value)
        assert sw.noise_supported
        with pytest.raises(qc.QCollocError) as e:
            sw.noise_grad(Z, c["init"], np.zeros((S, c["T"] - 1, 1)), c["theta"], c["scale"])
        assert e.value.code == UNS and "is not antisymmetric" in str(e.value)
        # the flag without the bit: the text it always had; the forward sweep gives the same bits on every handle
        sw0 = _handle(qc, c, bit=False)
        assert sw0._desc.wide == 1 | W64 | WG and sw0.stored_states and not sw0.wide64_stored and not sw0.grad_supported and not sw0.vjp_supported
        with pytest.raises(qc.QCollocError) as e:
            sw0.grad(*args)
        assert e.value.code == UNS and str(e.value).endswith("the handle takes the mfma64-sweep form (2N = 50), which does not serve stored-state gradients")
        sw1 = _handle(qc, c, stored=False)           # neither: the closed scope
        with pytest.raises(qc.QCollocError) as e:
            sw1.grad(*args)
        assert e.value.code == UNS and "is not antisymmetric" in str(e.value)
        for other in (sw0, sw1):
            for a, b in zip(sw.eval(*args), other.eval(*args)):
                assert np.array_equal(a, b)
            other.close()
    finally:
        sw.close()


@pytest.mark.gpu
def test_finals_autograd_backward_on_the_lindblad_handle(qc):
    """One backward pass of a torch loss on `finals_autograd` against central differences of the forward sweep (the step and tolerance of
    test_sweep_wide64_grad.test_wide64_finals_autograd_backward: eps 1e-6, atol 1e-6)."""
    import torch
    c = transmon5_case(qc, "autograd", S=2, T=4)
    sw = _handle(qc, c, fid=False)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    T, S = c["T"], c["S"]
    try:
        Z0 = _Z(sw, c)
        init, theta, scale = t(c["init"]), t(c["theta"]), t(c["scale"])
        Wt = t(np.random.default_rng(31).standard_normal((S, sw.ns)))
        loss = lambda Z_: ((sw.finals_autograd(Z_, init, theta, scale) * Wt).sum() + 0.5 * (sw.finals_autograd(Z_, init, theta, scale) ** 2 * Wt).sum())
        Z = t(Z0).requires_grad_(True)
        X = sw.finals_autograd(Z, init, theta, scale)
        fin = torch.empty((S, sw.ns), dtype=torch.float64, device=dev)
        sw.eval_device(Z.detach(), init, theta, scale, fin, None)
        assert torch.equal(X.detach(), fin)
        loss(Z).backward()
        got = Z.grad.cpu().numpy()
        eps, fd = 1e-6, np.zeros(sw.Z_len)
        with torch.no_grad():
            for i in range((T - 1) * sw.zdim):
                e = np.zeros(sw.Z_len)
                e[i] = eps
                fd[i] = (loss(t(Z0 + e)).item() - loss(t(Z0 - e)).item()) / (2 * eps)
        print(f"finals_autograd on the Lindblad handle: max |backward - central differences| = {np.abs(got - fd).max():.3e} (bound 1e-6)")
        np.testing.assert_allclose(got, fd, rtol=0, atol=1e-6)
        assert np.abs(fd).max() > 1e-2 and np.all(got[(T - 1) * sw.zdim:] == 0.0)
    finally:
        sw.close()


@pytest.mark.gpu
def test_five_level_open_polish_example(qc):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import five_level_open_polish
    before, after = five_level_open_polish.polish(T=8, S=3, steps=5, verbose=False)
    print(f"mean infidelity over the detunings {before:.4e} -> {after:.4e}")
    assert after < before
