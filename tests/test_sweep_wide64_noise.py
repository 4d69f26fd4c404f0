"""Noise-trajectory sweeps in the "mfma64-sweep" form (`qc_sweep_desc.wide` bit 16, QC_SWEEP_WIDE_64_NOISE;
`RolloutSweep(..., wide=True, wide64=True, wide64_noise=True)`, gradients with `wide64_grad=True` as well): `qc_sweep_noise_eval*` and
`qc_sweep_noise_grad*` for 32 < 2N <= 64 (csrc/qc_sweep64_noise.hip), up to 16 drives and 8 perturbations.  CPU: the bit, the device-free
scope queries with and without it, that nothing else sees it, the reference's two routes at 2N = 34, the launch table of the GPU cases.
GPU: every output against the scipy reference of tests/sweep_noise_reference.py through the host and the device entry with guarded
NaN-filled buffers, the squarings, exact equalities at zero noise, the resolution identity, additive control noise against single-sample
calls, a Lindblad handle at 2N = 50, a filled and a mid-size launch at every sample, bit-level properties, a NaN, the refusals, the
objective and the example.

Tolerances are those at the top of tests/test_sweep_noise.py, always against the reference: states rtol 1e-10 / atol 1e-11, fidelities
1e-9, every gradient output (grad_noise included) per sample |got - want| <= 1e-9 max(1, max |want_s|).  The helpers are those of the
existing files, imported, not copied.

"transmons27-sub8": a unitary fidelity needs all N columns (tests/test_sweep_wide64_grad.py), so the case is the full 27-column unitary
with the fidelity on the 8 computational levels; the 8-column state itself has no fidelity and is put to `noise_eval` alone."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import sweep_noise_reference as nref
import sweep_reference as ref
import test_sweep as ts
import test_sweep_grad as tg
import test_sweep_noise as tn
import test_sweep_open_grad as too
import test_sweep_wide as tw
import test_sweep_wide64 as t64
import test_sweep_wide64_jvp as t64j

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_herm, _unitary = ts._herm, ts._unitary
W64, GRAD64, PARAMS64, TAN64, NOISE64 = 1024, 2048, 8192, 16384, 65536
EVAL = dict(wide=True, wide64=True, wide64_noise=True)             # wide = 66561
HANDLE = dict(EVAL, wide64_grad=True)                              # wide = 68609
SUB8 = [9 * a + 3 * b + c for a in (0, 1) for b in (0, 1) for c in (0, 1)]

# name: (state, levels, m, p, scale given, free timestep, S, T, (kind, subspace, form))
CASES = {
    "levels17-S3": ("unitary", 17, 2, 1, False, True, 3, 6, ("unitary", None, "abs")),                 # padded tiles; three ragged chunks 2, 2, 1
    "levels32-full": ("unitary", 32, 3, 2, True, False, 2, 4, ("unitary", list(range(8)), "abs")),     # full tiles, 32 columns, subspace fidelity
    "levels20-ket": ("ket", 20, 1, 2, False, False, 5, 9, ("ket", None, "abs")),                       # one state column
    "transmons27-sub8": ("unitary", 27, 2, 3, True, True, 3, 5, ("unitary", SUB8, "abs")),             # three transmons' shape
    "generators24": ("unitary", 17, 16, 8, True, True, 3, 5, ("unitary", None, "abs")),                # 24 generators, the timestep in lane 24
    "generators23-fixed": ("unitary", 17, 15, 8, False, False, 3, 5, ("unitary", None, "abs")),        # no timestep lane
    "no-drives": ("unitary", 17, 0, 1, False, True, 3, 5, ("unitary", None, "abs")),                   # every coefficient is noise
}
# chunk, n_chunks, last chunk of each case's launch
CHUNKS = {"levels17-S3": (2, 3, 1), "levels32-full": (2, 2, 1), "levels20-ket": (3, 3, 2), "transmons27-sub8": (2, 2, 2), "generators24": (2, 2, 2),
          "generators23-fixed": (2, 2, 2), "no-drives": (2, 2, 2)}
_CASES = {}


def build(qc, name):
    """The draws of test_sweep_wide_noise.build at this form's sizes; built once (the reference cache of test_sweep_noise is keyed by name)."""
    if name in _CASES:
        return _CASES[name]
    state, L, m, p, use_scale, free, S, T, fid = CASES[name]
    rng = np.random.default_rng(sum(map(ord, "wide64-noise " + name)))
    H0 = _herm(rng, L)
    Hd = [_herm(rng, L, (L * max(m, 1)) ** -0.5) for _ in range(m)]
    system = qc.QuantumSystem(H0, Hd)
    perts = [_herm(rng, L) for _ in range(p)]
    G0, Gd, Gp = ref.iso_generator(H0), [ref.iso_generator(H) for H in Hd], [ref.iso_generator(P) for P in perts]
    kind, subspace, form = fid
    if state == "unitary":
        init, cols, goal = ref.operator_to_iso_vec(_unitary(rng, L)), L, ref.operator_to_iso_vec(_unitary(rng, L))
    else:
        v = _unitary(rng, L)
        init, cols, goal = ref.operator_to_iso_vec(v[:, :1]), 1, np.concatenate([v[:, 1].real, v[:, 1].imag])
    controls = rng.uniform(-1, 1, (m, T))
    dts = rng.uniform(0.1, 0.3, T) if free else 0.2
    theta = rng.uniform(-0.3, 0.3, (S, p))
    scale = rng.uniform(0.9, 1.1, (S, m)) if use_scale else None
    noise = rng.uniform(-0.3, 0.3, (S, T - 1, p))
    _CASES[name] = dict(name="wide64 " + name, L=L, m=m, p=p, S=S, T=T, system=system, perts=perts, G0=G0, Gd=Gd, Gp=Gp, init=init, cols=cols,
                        goal=goal, kind=kind, subspace=subspace, form=form, controls=controls, dts=dts, theta=theta, scale=scale, noise=noise)
    return _CASES[name]


def _make(qc, c, **kw):
    return tn._make(qc, c, **{**HANDLE, **kw})


def _squaring_case(qc):
    """test_sweep_wide_noise._squaring_case at 17 levels: a small drift, P = diag(+-1) (column sums of its iso generator: 1) and
    |dt xi| = 0.08 2^k, k = 0 .. 7: about k squarings per interval."""
    rng = np.random.default_rng(23)
    N, m, p, T, S, dt = 17, 1, 1, 8, 4, 0.2
    H0, Hd = _herm(rng, N, 0.003), [_herm(rng, N, 0.003)]
    P = np.diag((-1.0) ** np.arange(N)).astype(complex)
    system = qc.QuantumSystem(H0, Hd)
    G0, Gd, Gp = ref.iso_generator(H0), [ref.iso_generator(Hd[0])], [ref.iso_generator(P)]
    controls = rng.uniform(-1, 1, (m, T))
    init, goal = ref.operator_to_iso_vec(_unitary(rng, N)), ref.operator_to_iso_vec(_unitary(rng, N))
    k = np.array([[0, 3, 6, 1, 2, 4, 5], [6, 0, 7, 2, 2, 2, 2], [1, 1, 1, 5, 0, 6, 3], [0, 0, 0, 0, 0, 0, 4]], dtype=np.float64)
    noise = (0.4 * 2.0 ** k * rng.choice([-1.0, 1.0], (S, T - 1)))[:, :, None]
    theta = np.zeros((S, 1))
    sq = np.array([[ts._squarings(np.abs(dt * nref.interval_generator(G0, Gd, Gp, controls[:, t], theta[s], np.ones(m), noise[s, t])).sum(axis=0).max())
                    for t in range(T - 1)] for s in range(S)])
    c = dict(name="wide64 squarings", L=N, m=m, p=p, S=S, T=T, system=system, perts=[P], G0=G0, Gd=Gd, Gp=Gp, init=init, cols=N, goal=goal,
             kind="unitary", subspace=None, form="abs", controls=controls, dts=dt, theta=theta, scale=None, noise=noise)
    return c, sq


FILLED_S, FILLED_T = 256, 3
MID_S, MID_T = 50, 27


def _ket_case(qc, name, seed, S, T, classes):
    """A ket at 17 levels, two drives, one perturbation: `classes` distinct (theta, c, xi) rows (the reference's case), tiled to S samples."""
    rng = np.random.default_rng(seed)
    N, m, p = 17, 2, 1
    H0, Hd, perts = _herm(rng, N), [_herm(rng, N, (N * m) ** -0.5) for _ in range(m)], [_herm(rng, N)]
    system = qc.QuantumSystem(H0, Hd)
    G0, Gd, Gp = ref.iso_generator(H0), [ref.iso_generator(H) for H in Hd], [ref.iso_generator(P) for P in perts]
    v = _unitary(rng, N)
    init, goal = ref.operator_to_iso_vec(v[:, :1]), np.concatenate([v[:, 1].real, v[:, 1].imag])
    controls, dts = rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T)
    th, sc, xi = rng.uniform(-0.3, 0.3, (classes, p)), rng.uniform(0.9, 1.1, (classes, m)), rng.uniform(-0.3, 0.3, (classes, T - 1, p))
    rows = dict(name=name + " (classes)", L=N, m=m, p=p, S=classes, T=T, system=system, perts=perts, G0=G0, Gd=Gd, Gp=Gp, init=init, cols=1, goal=goal,
                kind="ket", subspace=None, form="abs", controls=controls, dts=dts, theta=th, scale=sc, noise=xi)
    rep = -(-S // classes)
    full = dict(rows, name=name, S=S, theta=np.tile(th, (rep, 1))[:S], scale=np.tile(sc, (rep, 1))[:S], noise=np.tile(xi, (rep, 1, 1))[:S])
    return rows, full


def _filled_case(qc):
    return _ket_case(qc, "wide64 filled", 77, FILLED_S, FILLED_T, 4)


def _mid_case(qc):
    return _ket_case(qc, "wide64 mid", 78, MID_S, MID_T, MID_S)[1]


# ---------------------------------------------------------------------------------------------------------------------------------
#  CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def _valid_without_the_bit():
    """Every value valid before bit 16: those of test_sweep_wide64_jvp._valid_without_the_bit, and those with bits 0 and 10 | 16384."""
    before = t64j._valid_without_the_bit()
    return before | {v | TAN64 for v in before if v & 1 and v & W64}


def test_wide_values_with_the_noise64_bit(qc):
    L = qc._lib
    val = lambda D: L.lib.qc_sweep_desc_validate(C.byref(D.d))
    assert L.QC_SWEEP_WIDE_64_NOISE == NOISE64 == 1 << 16
    header = open(os.path.join(ROOT, "include", "qcolloc.h")).read()
    assert "#define QC_SWEEP_WIDE_64_NOISE 65536" in header
    before = _valid_without_the_bit()
    assert len(before) == 33 + 3 * 32 + 3 * 32
    for N in (20, 12, 2):
        for v in sorted(before):
            assert val(tw._wdesc(qc, v, N=N)) == L.QC_OK, (N, v)
            want = L.QC_OK if (v & 1 and v & W64) else L.QC_ERR_INVALID      # valid exactly beside bits 0 and 10; none of 11, 13, 14 needed
            assert val(tw._wdesc(qc, v | NOISE64, N=N)) == want, (N, v)
        for bad in (NOISE64, NOISE64 | 1, NOISE64 | W64, NOISE64 | 1 | GRAD64, NOISE64 | 1 | W64 | 4, NOISE64 | 1 | W64 | 512, NOISE64 | 1 | W64 | 4096,
                    NOISE64 | 1 | W64 | (1 << 15), NOISE64 | 1 | W64 | (1 << 17), NOISE64 | 1 | W64 | (1 << 20), 1 | W64 | (1 << 15), 1 | W64 | (1 << 20)):
            assert val(tw._wdesc(qc, bad, N=N)) == L.QC_ERR_INVALID, (N, bad)
            text = L.lib.qc_sweep_last_error(None).decode()
            assert text.startswith("qc_sweep: wide"), text
            for words in ("17, 19, 25 or 27", "QC_SWEEP_WIDE_TANGENT (16)", "QC_SWEEP_WIDE_NOISE (64)", "QC_SWEEP_WIDE_HESSIAN (256)",
                          "QC_SWEEP_WIDE_64 (1024)", "QC_SWEEP_WIDE_64_GRAD (2048)", "QC_SWEEP_WIDE_64_PARAMS (8192)",
                          "QC_SWEEP_WIDE_64_TANGENT (16384)", "QC_SWEEP_WIDE_64_NOISE (65536)"):
                assert words in text, (words, text)
        for good in (1 | W64 | NOISE64, 27 | W64 | NOISE64, 347 | W64 | NOISE64, 1 | W64 | GRAD64 | NOISE64, 1 | W64 | TAN64 | NOISE64,
                     3 | W64 | GRAD64 | PARAMS64 | TAN64 | NOISE64):
            assert val(tw._wdesc(qc, good, N=N)) == L.QC_OK, (N, good)


def test_python_keywords(qc):
    sys2 = qc.QuantumSystem(np.zeros((2, 2)), [qc.GATES["X"]])
    with pytest.raises(ValueError, match="wide64_noise=True needs wide64=True"):
        qc.RolloutSweep(sys2, [qc.GATES["Z"]], 4, wide=True, wide64_noise=True)
    with pytest.raises(ValueError, match="wide64=True needs wide=True"):
        qc.RolloutSweep(sys2, [qc.GATES["Z"]], 4, wide64=True, wide64_noise=True)
    assert isinstance(qc.RolloutSweep.wide64_noise, property)
    import inspect
    assert inspect.signature(qc.RolloutSweep.__init__).parameters["wide64_noise"].default is False
    assert inspect.signature(qc.rollout_noise_sweep).parameters["wide64"].default is False
    for kw in ("wide64", "wide64_grad", "wide64_noise"):
        assert inspect.signature(qc.SweepNoiseInfidelityObjective.__init__).parameters[kw].default is False
    assert inspect.signature(qc.SweepInfidelityObjective.__init__).parameters["wide64_noise"].default is False


def _lindblad(qc, wide, **kw):
    return t64j._lindblad(qc, wide, **kw)


def test_noise_scope_follows_the_bit(qc):
    L = qc._lib
    U = L.QC_FID_UNITARY
    q = lambda D: tn._supported(qc, D)
    for bits in (1 | W64, 27 | W64, 1 | W64 | GRAD64, 3 | W64 | GRAD64 | PARAMS64 | TAN64):
        for m, p in ((2, 1), (16, 8), (0, 1)):
            for make in (lambda w: too._ODesc(qc, wide=w, N=27, m=m, p=p, fid_kind=U), lambda w: _lindblad(qc, w, m=m, p=p),
                         lambda w: too._ODesc(qc, wide=w, N=17, m=m, p=p, cols=33)):
                assert q(make(bits | NOISE64))[:2] == (L.QC_OK, 1), (bits, m, p)
                rc, ok, text = q(make(bits))
                assert (rc, ok) == (L.QC_OK, 0) and "mfma64-sweep form (2N = " in text, (bits, m, p, text)
    # today's two texts, verbatim, without the bit
    assert q(too._ODesc(qc, wide=1 | W64, N=27, m=6, fid_kind=U)) == \
        (L.QC_OK, 0, "qc_sweep noise: the handle takes the mfma64-sweep form (2N = 54), which serves the forward sweep only")
    assert q(too._ODesc(qc, wide=1 | W64 | GRAD64 | PARAMS64 | TAN64, N=27, m=6, fid_kind=U)) == \
        (L.QC_OK, 0, "qc_sweep noise: the handle takes the mfma64-sweep form (2N = 54), which does not serve noise trajectories")
    # with it: n_pert = 0, and 17 drives (the per-sample text)
    rc, ok, text = q(too._ODesc(qc, wide=1 | W64 | NOISE64, N=27, m=6, p=0, fid_kind=U))
    assert (rc, ok) == (L.QC_OK, 0) and text.startswith("qc_sweep noise: ") and "n_pert = 0" in text
    rc, ok, text = q(too._ODesc(qc, wide=1 | W64 | NOISE64, N=27, m=17, fid_kind=U))
    assert (rc, ok) == (L.QC_OK, 0) and text == "qc_sweep noise: the handle takes the rollout-per-sample form (17 drives > 16)"
    # at 2N <= 32 the answers and texts are those without the bit
    for N, m, p in ((12, 2, 1), (12, 5, 4), (12, 2, 0), (12, 9, 1), (8, 6, 3), (8, 6, 2), (2, 2, 1), (2, 0, 8)):
        for base in (1 | W64, 65 | W64, 27 | W64 | GRAD64):
            a, b = q(too._ODesc(qc, wide=base, N=N, m=m, p=p, fid_kind=U)), q(too._ODesc(qc, wide=base | NOISE64, N=N, m=m, p=p, fid_kind=U))
            assert a[:2] == b[:2] and (a[1] == 1 or a[2] == b[2]), (N, m, p, base, a, b)


def test_nothing_else_sees_the_bit(qc):
    """grad, vjp, jvp and hvp queries and the launch rule: the same answers and texts with and without bit 16, over the descriptor
    families of test_sweep_wide64_jvp.test_other_scope_queries_do_not_see_the_bit."""
    L = qc._lib
    U = L.QC_FID_UNITARY
    makers = [lambda w, N=N: too._ODesc(qc, wide=w, N=N, m=2, fid_kind=U) for N in (17, 27, 32, 12, 4)]
    makers += [lambda w: too._ODesc(qc, wide=w, N=17, m=2, cols=1, fid_kind=L.QC_FID_KET), lambda w: _lindblad(qc, w), lambda w: _lindblad(qc, w, flag=1),
               lambda w: too._ODesc(qc, wide=w, N=27, m=6, fid_kind=U, flag=1), lambda w: _lindblad(qc, w, N=16), lambda w: too._ODesc(qc, wide=w, N=27, m=17, fid_kind=U)]
    seen = set()
    for make in makers:
        for base in (1 | W64, 347 | W64, 1 | W64 | GRAD64, 1 | W64 | GRAD64 | PARAMS64, 27 | W64 | GRAD64 | PARAMS64, 1 | W64 | TAN64,
                     3 | W64 | GRAD64 | PARAMS64 | TAN64):
            for which in ("grad", "vjp", "jvp", "hvp"):
                fn = f"qc_sweep_desc_{which}_supported"
                a, b = too._query(qc, fn, make(base)), too._query(qc, fn, make(base | NOISE64))
                assert a[0] == b[0] == L.QC_OK and a[1] == b[1], (which, base)
                if a[1] == 0:
                    assert a[2] == b[2], (which, base, a[2], b[2])
                    seen.add(a[2])
            for S in (1, 5, 255, 256, 300, 8192):
                out = []
                for D in (make(base), make(base | NOISE64)):
                    mf, ch, nch = C.c_int32(), C.c_int64(), C.c_int64()
                    assert L.lib.qc_sweep_desc_launch(C.byref(D.d), S, C.byref(mf), C.byref(ch), C.byref(nch)) == L.QC_OK
                    out.append((mf.value, ch.value, nch.value))
                assert out[0] == out[1], (base, S)
    assert any("which serves the forward sweep only" in s for s in seen) and any("which does not serve" in s for s in seen)
    D = too._ODesc(qc, wide=1 | W64 | GRAD64 | PARAMS64 | TAN64 | NOISE64, N=27, m=6, fid_kind=U)
    assert too._query(qc, "qc_sweep_desc_hvp_supported", D) == (L.QC_OK, 0, "qc_sweep Hessian product: the handle takes the mfma64-sweep form (2N = 54), which does not serve Hessian products")


def test_reference_routes_agree_at_17_levels():
    """Forward mode (expm_frechet) against central differences of the chain at 2N = 34: 1e-6 relative, as in test_sweep_noise.py."""
    rng = np.random.default_rng(1717)
    N, m, p, T, S = 17, 2, 2, 3, 2
    G0, Gd = ref.iso_generator(_herm(rng, N)), [ref.iso_generator(_herm(rng, N, 0.3)) for _ in range(m)]
    Gp = [ref.iso_generator(_herm(rng, N)) for _ in range(p)]
    controls, dts = rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T)
    theta, scale, noise = rng.uniform(-0.3, 0.3, (S, p)), rng.uniform(0.9, 1.1, (S, m)), rng.uniform(-0.3, 0.3, (S, T - 1, p))
    v = _unitary(rng, N)
    init, goal = ref.operator_to_iso_vec(v[:, :1]), np.concatenate([v[:, 1].real, v[:, 1].imag])
    args = (G0, Gd, Gp, controls, dts, init, theta, scale, noise, [0, 1], "ket", goal, N, None, "abs")
    (a, an), (b, bn) = nref.noise_grads_forward(*args), nref.noise_grads_fd(*args)
    assert a.shape == b.shape == (2, T - 1, m + 1) and an.shape == bn.shape == (2, T - 1, p)
    for what, x, y in (("controls", a, b), ("noise", an, bn)):
        err = np.abs(x - y).max() / max(1.0, np.abs(x).max())
        print(f"L=17 {what}: forward vs central differences {err:.2e}, max |grad| {np.abs(x).max():.3f}")
        assert err < 1e-6 and np.abs(x).max() > 1e-3
    # constant noise is a shifted theta at this size
    const = np.broadcast_to(rng.uniform(-0.2, 0.2, (S, 1, p)), (S, T - 1, p))
    x = nref.noise_finals(G0, Gd, Gp, controls, dts, init, theta, scale, const)
    y = nref.noise_finals(G0, Gd, Gp, controls, dts, init, theta + const[:, 0], scale, np.zeros((S, T - 1, p)))
    ts._assert_states(x, y, "constant noise = shifted theta at L = 17")
    gx = nref.noise_grads_forward(G0, Gd, Gp, controls, dts, init, theta, scale, const, [0, 1], "ket", goal, N)
    gy = nref.noise_grads_forward(G0, Gd, Gp, controls, dts, init, theta + const[:, 0], scale, np.zeros((S, T - 1, p)), [0, 1], "ket", goal, N)
    for u, v_ in zip(gx, gy):
        tn._assert_samples(u, v_, "constant noise = shifted theta at L = 17, gradients")


def _launch(qc, N, m, p, S, T, bits=1 | W64 | NOISE64):
    D = tw._wdesc(qc, bits, N=N, m=m, p=p, T=T)
    mf, ch, nch = C.c_int32(), C.c_int64(), C.c_int64()
    assert qc._lib.lib.qc_sweep_desc_launch(C.byref(D.d), S, C.byref(mf), C.byref(ch), C.byref(nch)) == qc._lib.QC_OK
    return bool(mf.value), ch.value, nch.value


def test_the_launch_table_of_the_gpu_cases(qc):
    """Chunk, n_chunks and the last chunk of every GPU case, pinned through `qc_sweep_desc_launch`; each on the side of the rule it is named for."""
    for name, (chunk, n_chunks, last) in CHUNKS.items():
        state, lv, m, p, _, _, S, T, _ = CASES[name]
        assert _launch(qc, lv, m, p, S, T) == (True, chunk, n_chunks), name
        assert (T - 1) - (n_chunks - 1) * chunk == last and n_chunks > 1, name
        w = t64.launch64(2 * lv, m, S, T, 1 | W64 | NOISE64)
        assert (w["chunk"], w["n_chunks"], w["last"]) == (chunk, n_chunks, last), name
        assert 32 < 2 * lv <= 64 and m <= 16 and 1 <= p <= 8
    assert CHUNKS["levels17-S3"] == (2, 3, 1)                                # several chunks, the last one shorter
    assert CASES["generators24"][2:4] == (16, 8) and CASES["generators24"][5]          # 24 generators and a free timestep: lane 24
    assert CASES["generators23-fixed"][2:4] == (15, 8) and not CASES["generators23-fixed"][5]
    assert _launch(qc, 17, 1, 1, 4, 8) == (True, 3, 3)                       # the squaring case: chunks 3, 3, 1
    assert _launch(qc, 17, 2, 1, FILLED_S, FILLED_T) == (True, FILLED_T - 1, 1)       # the fill constant: one chunk, 256 workgroups
    assert _launch(qc, 17, 2, 1, FILLED_S - 1, FILLED_T) == (True, 1, 2)              # one sample fewer: two
    assert _launch(qc, 17, 2, 1, MID_S, MID_T) == (True, 5, 6)               # ragged: five chunks of 5, one of 1
    assert _launch(qc, 25, 2, 1, 3, 5) == (True, 2, 2)                       # the Lindblad case
    # the bit does not move the table
    for name in CASES:
        state, lv, m, p, _, _, S, T, _ = CASES[name]
        assert _launch(qc, lv, m, p, S, T, 1 | W64) == _launch(qc, lv, m, p, S, T)


def test_the_special_cases_are_what_they_claim(qc):
    c, sq = _squaring_case(qc)
    first = sq[:, :3]                                       # the first chunk of every sample
    assert first[0].min() == 0 and first[0].max() >= 6      # 0 .. at least 6 inside one workgroup's chunk
    assert sq.max() >= 7 and len({tuple(r) for r in sq}) == c["S"] and len({r.max() for r in first}) >= 3
    rows, full = _filled_case(qc)
    assert full["noise"].shape == (FILLED_S, FILLED_T - 1, 1) and np.array_equal(full["noise"][4:8], rows["noise"])
    assert len({tuple(r.ravel()) for r in rows["noise"]}) == 4


# ---------------------------------------------------------------------------------------------------------------------------------
#  GPU
# ---------------------------------------------------------------------------------------------------------------------------------
GUARD = 64


def _guarded(count, dev):
    """A NaN-filled device buffer of `count` doubles between two guards of -7."""
    whole = torch.full((count + 2 * GUARD,), -7.0, dtype=torch.float64, device=dev)
    whole[GUARD:GUARD + count] = float("nan")
    return whole, whole[GUARD:GUARD + count]


def _device_call(sw, Z, c, weights=None, stream=None):
    """`noise_eval_device` and `noise_grad_device` into guarded NaN-filled buffers: (finals, fids, J, fids2, grad, gn, gs) as host arrays.
    Everything is written and nothing lands outside."""
    dev = torch.device("cuda:0")
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    S, T, p = c["S"], c["T"], c["p"]
    counts = dict(fin=S * sw.ns, fid=S, fid2=S, J=1, g=sw.Z_len, gs=S * (T - 1) * sw.n_deriv, gn=S * (T - 1) * p)
    buf = {k: _guarded(n, dev) for k, n in counts.items()}
    v = {k: b[1] for k, b in buf.items()}
    dZ, dinit, dn, dth, dsc, dw = t(Z), t(c["init"]), t(c["noise"]), t(c["theta"]), t(c["scale"]), t(weights)
    torch.cuda.synchronize()
    run = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(run):
        sw.noise_eval_device(dZ, dinit, dn, dth, dsc, v["fin"], v["fid"], stream=stream)
        sw.noise_grad_device(dZ, dinit, dn, dth, dsc, dw, v["fid2"], v["J"], v["g"], v["gs"] if counts["gs"] else None, v["gn"], stream=stream)
    run.synchronize()
    for k, (whole, view) in buf.items():
        h = whole.cpu().numpy()
        assert np.all(h[:GUARD] == -7.0) and np.all(h[GUARD + counts[k]:] == -7.0), k
        if k != "gs" or counts["gs"]:
            assert not np.isnan(h[GUARD:GUARD + counts[k]]).any(), k
    o = {k: b[1].cpu().numpy() for k, b in buf.items()}
    return (o["fin"].reshape(S, sw.ns).T, o["fid"], o["J"][0], o["fid2"], o["g"], o["gn"].reshape(S, T - 1, p), o["gs"].reshape(S, T - 1, sw.n_deriv))


def _both_entries(sw, Z, c, weights=None):
    """tn._check_call (the host entry against the reference) and the device entry with guards: the same bits."""
    finals, fids, J, grad, gn, gs = tn._check_call(sw, Z, c, weights=weights)
    d = _device_call(sw, Z, c, weights=weights)
    assert np.array_equal(d[0], finals) and np.array_equal(d[1], fids) and d[2] == J and np.array_equal(d[3], fids)
    assert np.array_equal(d[4], grad) and np.array_equal(d[5], gn) and np.array_equal(d[6], gs)
    return finals, fids, J, grad, gn, gs


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_wide64_noise_matches_the_reference(qc, name):
    c = build(qc, name)
    sw = _make(qc, c)
    try:
        assert sw._desc.wide == 1 | W64 | GRAD64 | NOISE64 and sw.kernel_name == "mfma64-sweep" and sw.wide64_noise
        assert sw.noise_supported and sw.noise_unsupported_reason is None and sw.grad_supported
        chunk, n_chunks, _ = CHUNKS[name]
        assert sw.launch(c["S"]) == (True, chunk, n_chunks)
        Z = sw.pack(c["controls"], c["dts"])
        finals, fids = _both_entries(sw, Z, c)[:2]
        if name == "levels17-S3":
            _both_entries(sw, Z, c, weights=np.array([0.2, 1.5, 0.7]))
            f3, fid3 = qc.rollout_noise_sweep(c["init"], c["controls"], c["dts"], c["system"], c["perts"], c["noise"], c["theta"], cols=c["cols"],
                                              goal=c["goal"], fid_kind="unitary", wide=True, wide64=True)
            np.testing.assert_array_equal(f3, finals)
            np.testing.assert_array_equal(fid3, fids)
    finally:
        sw.close()
    if name == "transmons27-sub8":      # the 8 computational columns as the state: no fidelity is defined, the evaluation alone
        E = np.zeros((2 * c["L"], 8))
        E[SUB8, np.arange(8)] = 1.0
        init8 = E.reshape(-1, order="F")
        sw = qc.RolloutSweep(c["system"], c["perts"], c["T"], cols=8, **EVAL)
        try:
            assert sw.kernel_name == "mfma64-sweep" and sw.noise_supported and not sw.grad_supported
            f8, none = sw.noise_eval(sw.pack(c["controls"], c["dts"]), init8, c["noise"], c["theta"], c["scale"])
            want = nref.noise_finals(c["G0"], c["Gd"], c["Gp"], c["controls"], c["dts"], init8, c["theta"], c["scale"], c["noise"])
            assert none is None
            ts._assert_states(f8, want, "wide64 transmons27, 8 columns")
        finally:
            sw.close()


@pytest.mark.gpu
def test_wide64_noise_through_the_squarings(qc):
    """Noise strong enough that the intervals of ONE workgroup's chunk need 0 .. 7 squarings, differently in every sample."""
    c, sq = _squaring_case(qc)
    print("squarings per sample and interval:\n", sq)
    assert sq[0, :3].min() == 0 and sq[0, :3].max() >= 6
    sw = _make(qc, c)
    try:
        assert sw.kernel_name == "mfma64-sweep" and sw.launch(c["S"]) == (True, 3, 3)
        _both_entries(sw, sw.pack(c["controls"]), c)
    finally:
        sw.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["levels17-S3", "levels20-ket", "generators24"])
def test_wide64_zero_noise_is_the_sweep(qc, name):
    """An explicit +0.0 noise array: finals and fids carry the bits of `eval`, fids / J / grad / grad_samples those of `grad` on the same
    handle.  And sum_t grad_noise[s, t, j] agrees with grad_theta[s, j] of `param_grad` (bits 11 and 13) to the gradient tolerance."""
    c = build(qc, name)
    sw = _make(qc, c, wide64_params=True)
    try:
        assert sw._desc.wide == 1 | W64 | GRAD64 | PARAMS64 | NOISE64 and sw.kernel_name == "mfma64-sweep"
        Z = sw.pack(c["controls"], c["dts"])
        zero = np.zeros((c["S"], c["T"] - 1, c["p"]))
        assert not np.signbit(zero).any()
        w = np.linspace(0.5, 1.5, c["S"])
        finals, fids = sw.noise_eval(Z, c["init"], zero, c["theta"], c["scale"])
        f0, fid0 = sw.eval(Z, c["init"], c["theta"], c["scale"])
        assert np.array_equal(finals, f0) and np.array_equal(fids, fid0)
        J, f2, grad, gn, gs = sw.noise_grad(Z, c["init"], zero, c["theta"], c["scale"], weights=w, per_sample=True)
        J0, f20, grad0, gs0 = sw.grad(Z, c["init"], c["theta"], c["scale"], weights=w, per_sample=True)
        assert J == J0 and np.array_equal(f2, f20) and np.array_equal(grad, grad0) and np.array_equal(gs, gs0)
        assert np.abs(gs0).max() > 1e-3
        _, gth, _ = sw.param_grad(Z, c["init"], c["theta"], c["scale"])
        tot = gn.sum(axis=1)
        worst = 0.0
        for s in range(c["S"]):
            worst = max(worst, np.abs(tot[s] - gth[s]).max() / (1e-9 * max(1.0, np.abs(gth[s]).max())))
        print(f"SWEEP-WIDE64-NOISE {name} resolution identity: worst |sum_t grad_noise - grad_theta| / bound = {worst:.2e}, max |grad_theta| = {np.abs(gth).max():.3e}")
        assert worst <= 1.0 and np.abs(gth).max() > 1e-3
    finally:
        sw.close()


@pytest.mark.gpu
def test_wide64_additive_control_noise_against_single_sample_calls(qc):
    """P_0 = H_drive_0 at 17 levels: one noise sweep against S = 5 single-sample `eval` calls that each carry a_{t,0} + xi[s, t] in a
    trajectory vector of their own."""
    rng = np.random.default_rng(31)
    N, m, T, S = 17, 2, 9, 5
    H0, Hd = _herm(rng, N), [_herm(rng, N, 0.3) for _ in range(m)]
    system = qc.QuantumSystem(H0, Hd)
    v = _unitary(rng, N)
    init = ref.operator_to_iso_vec(v[:, :3])
    controls, dts = rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T)
    noise = rng.uniform(-0.2, 0.2, (S, T - 1))
    sw = qc.RolloutSweep(system, [Hd[0]], T, cols=3, **EVAL)
    plain = qc.RolloutSweep(system, [], T, cols=3, wide=True, wide64=True)
    try:
        assert sw.kernel_name == plain.kernel_name == "mfma64-sweep"
        finals, fids = sw.noise_eval(sw.pack(controls, dts), init, noise)
        assert fids is None and finals.shape == (2 * N * 3, S)
        for s in range(S):
            cs = controls.copy()
            cs[0, :T - 1] += noise[s]
            one, _ = plain.eval(plain.pack(cs, dts), init, np.zeros((1, 0)))
            ts._assert_states(finals[:, s], one[:, 0], f"wide64 additive control noise, sample {s}")
    finally:
        sw.close()
        plain.close()


def _open_case(qc):
    """A five-level system with decay (N = 25, 2N = 50) and a decay channel whose rate fluctuates."""
    rng = np.random.default_rng(41)
    L, m, T, S = 5, 2, 5, 3
    H0, Hd = _herm(rng, L), [_herm(rng, L, 0.4) for _ in range(m)]
    lower = np.diag(np.sqrt(np.arange(1.0, L)), 1).astype(complex)
    diss = [0.2 * lower, 0.15 * np.diag(np.arange(L)).astype(complex)]
    system = qc.OpenQuantumSystem(H0, Hd, diss)
    perts = [np.asarray(qc.iso_operator(qc.OpenQuantumSystem.dissipator_superoperator(lower)))]
    psi = rng.standard_normal(L) + 1j * rng.standard_normal(L)
    psi /= np.linalg.norm(psi)
    gk = rng.standard_normal(L) + 1j * rng.standard_normal(L)
    gk /= np.linalg.norm(gk)
    return dict(name="wide64 open5", L=L, m=m, p=1, S=S, T=T, system=system, perts=perts, G0=np.asarray(system.G_drift),
                Gd=[np.asarray(G) for G in system.G_drives], Gp=perts, init=qc.density_to_iso_vec(np.outer(psi, psi.conj())), cols=1,
                goal=np.concatenate([gk.real, gk.imag]), kind="density", subspace=None, form="abs", controls=rng.uniform(-1, 1, (m, T)),
                dts=rng.uniform(0.1, 0.3, T), theta=rng.uniform(0.1, 0.3, (S, 1)), scale=None, noise=rng.uniform(0.0, 0.2, (S, T - 1, 1)))


@pytest.mark.gpu
def test_wide64_noise_on_a_lindblad_handle(qc):
    """N = 25 = 5^2, the density-operator fidelity: the evaluation serves generators that are not antisymmetric; the gradient is refused
    with the gradient's own reason."""
    c = _open_case(qc)
    sw = _make(qc, c)
    try:
        assert sw.N == 25 and sw.kernel_name == "mfma64-sweep" and sw.noise_supported and not sw.grad_supported
        assert sw.launch(c["S"]) == (True, 2, 2)
        Z = sw.pack(c["controls"], c["dts"])
        finals, fids = sw.noise_eval(Z, c["init"], c["noise"], c["theta"])
        want = nref.noise_finals(c["G0"], c["Gd"], c["Gp"], c["controls"], c["dts"], c["init"], c["theta"], None, c["noise"])
        ts._assert_states(finals, want, "wide64 open5 with noise")
        ts._assert_fids(fids, ref.fidelities(want, "density", c["goal"], c["L"]), "wide64 open5 with noise")
        with pytest.raises(qc.QCollocError) as e:
            sw.noise_grad(Z, c["init"], c["noise"], c["theta"])
        assert e.value.code == qc._lib.QC_ERR_UNSUPPORTED and "is not antisymmetric" in str(e.value) and str(e.value).count("qc_sweep noise: ") == 1
        f2, fid2 = sw.noise_eval(Z, c["init"], c["noise"], c["theta"])       # the handle is usable afterwards
        assert np.array_equal(f2, finals) and np.array_equal(fid2, fids)
    finally:
        sw.close()


@pytest.mark.gpu
def test_wide64_noise_filled_launch(qc):
    """S = 256: `launch(S)` reports one chunk, 256 workgroups.  EVERY sample against the reference row of its class (4 distinct
    (theta, c, xi) rows, tiled), and every sample carries the bits of the first of its class in every per-sample output."""
    rows, full = _filled_case(qc)
    sw = _make(qc, full)
    try:
        assert sw.kernel_name == "mfma64-sweep" and sw.launch(FILLED_S) == (True, FILLED_T - 1, 1)
        Z = sw.pack(full["controls"], full["dts"])
        rf, rfid, rgs, rgn = tn.reference(rows)
        rep = FILLED_S // 4
        finals, fids = sw.noise_eval(Z, full["init"], full["noise"], full["theta"], full["scale"])
        J, f2, grad, gn, gs = sw.noise_grad(Z, full["init"], full["noise"], full["theta"], full["scale"], per_sample=True)
        ts._assert_states(finals, np.tile(rf, (1, rep)), "wide64 filled")
        ts._assert_fids(fids, np.tile(rfid, rep), "wide64 filled")
        tn._assert_samples(gs, np.tile(rgs, (rep, 1, 1)), "wide64 filled grad_samples")
        tn._assert_samples(gn, np.tile(rgn, (rep, 1, 1)), "wide64 filled grad_noise")
        assert np.abs(rgn).max() > 1e-3
        np.testing.assert_array_equal(f2, fids)
        for s in range(4):
            assert np.array_equal(finals[:, s::4], np.repeat(finals[:, s:s + 1], rep, axis=1)), s
            assert np.all(fids[s::4] == fids[s]), s
            assert np.array_equal(gn[s::4], np.broadcast_to(gn[s], gn[s::4].shape)) and np.array_equal(gs[s::4], np.broadcast_to(gs[s], gs[s::4].shape)), s
    finally:
        sw.close()


@pytest.mark.gpu
def test_wide64_noise_mid_size_launch(qc):
    """S = 50, T = 27: 300 workgroups, chunks of 5, 5, 5, 5, 5, 1; every sample against the reference, host and device entry."""
    c = _mid_case(qc)
    sw = _make(qc, c)
    try:
        assert sw.kernel_name == "mfma64-sweep" and sw.launch(MID_S) == (True, 5, 6)
        _both_entries(sw, sw.pack(c["controls"], c["dts"]), c, weights=np.linspace(0.5, 1.5, MID_S))
    finally:
        sw.close()


@pytest.mark.gpu
def test_wide64_noise_bits(qc):
    """Repeated calls, host entry = device entry = device entry on a side stream, one handle grown through S = 3, 300, 5 against fresh
    handles; grad_samples absent, grad_noise absent or both present: the same bits in what remains."""
    c = build(qc, "transmons27-sub8")
    rng = np.random.default_rng(8)
    sw = _make(qc, c)
    T, m, p = c["T"], c["m"], c["p"]
    Z, init = sw.pack(c["controls"], c["dts"]), c["init"]
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    mk = lambda *shape: torch.full(shape, -7.0, dtype=torch.float64, device=dev)
    side = torch.cuda.Stream(device=dev)
    try:
        for i, S in enumerate((3, 300, 5)):
            theta, scale, w = rng.uniform(-0.3, 0.3, (S, p)), rng.uniform(0.9, 1.1, (S, m)), rng.uniform(0.5, 1.5, S)
            noise = rng.uniform(-0.3, 0.3, (S, T - 1, p))
            finals, fids = sw.noise_eval(Z, init, noise, theta, scale)
            first = sw.noise_grad(Z, init, noise, theta, scale, weights=w, per_sample=True)      # J, fids, grad, grad_noise, grad_samples
            np.testing.assert_array_equal(first[1], fids)
            fresh = _make(qc, c)
            try:
                f2, fid2 = fresh.noise_eval(Z, init, noise, theta, scale)
                again = fresh.noise_grad(Z, init, noise, theta, scale, weights=w, per_sample=True)
            finally:
                fresh.close()
            assert np.array_equal(f2, finals) and np.array_equal(fid2, fids) and again[0] == first[0]
            for a, b in zip(again[1:], first[1:]):
                np.testing.assert_array_equal(a, b)
            if i == 0:
                for _ in range(3):
                    again = sw.noise_grad(Z, init, noise, theta, scale, weights=w, per_sample=True)
                    assert again[0] == first[0]
                    for a, b in zip(again[1:], first[1:]):
                        np.testing.assert_array_equal(a, b)
                    f2, fid2 = sw.noise_eval(Z, init, noise, theta, scale)
                    assert np.array_equal(f2, finals) and np.array_equal(fid2, fids)
            if i == 1:
                continue
            dZ, dinit, dth, dsc, dw, dn = t(Z), t(init), t(theta), t(scale), t(w), t(noise)
            torch.cuda.synchronize()
            for stream in (None, side):
                dfin, dfid = mk(S, sw.ns), mk(S)
                dfid2, dJ, dg, dgs, dgn = mk(S), mk(1), mk(sw.Z_len), mk(S, T - 1, sw.n_deriv), mk(S, T - 1, p)
                with torch.cuda.stream(side if stream is not None else torch.cuda.current_stream()):
                    sw.noise_eval_device(dZ, dinit, dn, dth, dsc, dfin, dfid, stream=stream)
                    sw.noise_grad_device(dZ, dinit, dn, dth, dsc, dw, dfid2, dJ, dg, dgs, dgn, stream=stream)
                (side if stream is not None else torch.cuda.current_stream()).synchronize()
                np.testing.assert_array_equal(dfin.cpu().numpy().T, finals)
                np.testing.assert_array_equal(dfid.cpu().numpy(), fids)
                assert dJ.item() == first[0]
                for a, b in zip((dfid2, dg, dgn, dgs), first[1:]):
                    np.testing.assert_array_equal(a.cpu().numpy(), b)
            # outputs are optional one at a time, and none depends on the others: grad_noise alone launches the walk without grad_samples,
            # grad_samples or grad alone without grad_noise
            for k, (key, shape) in enumerate((("dJ", (1,)), ("dfids", (S,)), ("dgrad", (sw.Z_len,)), ("dgrad_noise", (S, T - 1, p)),
                                              ("dgrad_samples", (S, T - 1, sw.n_deriv)))):
                out = mk(*shape)
                sw.noise_grad_device(dZ, dinit, dn, dth, dsc, dw, **{key: out})
                torch.cuda.synchronize()
                np.testing.assert_array_equal(out.cpu().numpy().reshape(np.shape(first[k])), first[k])
            only_f, only_fid = mk(S, sw.ns), mk(S)
            sw.noise_eval_device(dZ, dinit, dn, dth, dsc, dfinals=only_f)
            sw.noise_eval_device(dZ, dinit, dn, dth, dsc, dfids=only_fid)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(only_f.cpu().numpy().T, finals)
            np.testing.assert_array_equal(only_fid.cpu().numpy(), fids)
    finally:
        sw.close()


@pytest.mark.gpu
def test_wide64_noise_bit_changes_nothing_else_on_the_device(qc):
    """On handles made with and without bit 16 (every other mfma64 bit set), `eval`, `grad`, `param_grad`, `vjp` and `jvp` return the
    same bits, and kernel name and launch are the same."""
    c = build(qc, "levels17-S3")
    every = dict(wide=True, wide64=True, wide64_grad=True, wide64_params=True, wide64_tangent=True)
    a, b = tn._make(qc, c, **every, wide64_noise=True), tn._make(qc, c, **every)
    try:
        assert a._desc.wide == b._desc.wide | NOISE64 and b._desc.wide == 1 | W64 | GRAD64 | PARAMS64 | TAN64
        assert a.kernel_name == b.kernel_name == "mfma64-sweep" and all(a.launch(S) == b.launch(S) for S in (1, 3, 300, 2048))
        assert a.noise_supported and not b.noise_supported
        assert b.grad_supported == a.grad_supported and b.vjp_supported == a.vjp_supported and b.jvp_supported == a.jvp_supported
        Z = a.pack(c["controls"], c["dts"])
        rng = np.random.default_rng(4)
        cot, vZ = rng.standard_normal((c["S"], a.ns)), rng.standard_normal(a.Z_len)
        vth = rng.standard_normal((c["S"], c["p"]))
        calls = (lambda s: s.eval(Z, c["init"], c["theta"], c["scale"]), lambda s: s.grad(Z, c["init"], c["theta"], c["scale"], per_sample=True),
                 lambda s: s.param_grad(Z, c["init"], c["theta"], c["scale"], with_controls=True),
                 lambda s: s.vjp(Z, c["init"], cot, c["theta"], c["scale"], per_sample=True, init_grad=True, params=True),
                 lambda s: s.jvp(Z, c["init"], vZ, c["theta"], c["scale"], vtheta=vth, fids=True))
        for call in calls:
            xs, ys = call(a), call(b)
            flat = lambda r: [q for item in (r if isinstance(r, tuple) else (r,)) for q in (item if isinstance(item, tuple) else (item,))]
            fx, fy = flat(xs), flat(ys)
            assert len(fx) == len(fy) and len(fx) >= 1
            for x, y in zip(fx, fy):
                if x is None:
                    assert y is None
                else:
                    np.testing.assert_array_equal(np.asarray(x), np.asarray(y))
    finally:
        a.close()
        b.close()


@pytest.mark.gpu
def test_wide64_noise_non_finite_input(qc):
    """A NaN at noise[1, 2, 0] of three samples does not raise: samples 0 and 2 carry the bits of the clean run in every per-sample
    output, sample 1 and the sums over the samples are not finite, and the handle then serves a clean call as if nothing had happened."""
    c = build(qc, "levels17-S3")
    sw = _make(qc, c)
    try:
        Z = sw.pack(c["controls"], c["dts"])
        call = lambda noise: sw.noise_eval(Z, c["init"], noise, c["theta"]) + sw.noise_grad(Z, c["init"], noise, c["theta"], per_sample=True)
        good = call(c["noise"])            # finals, fids, J, fids, grad, grad_noise, grad_samples
        assert all(np.isfinite(x).all() for x in good)
        bad = c["noise"].copy()
        bad[1, 2, 0] = np.nan
        finals, fids, J, f2, grad, gn, gs = call(bad)
        for s in (0, 2):
            assert np.array_equal(finals[:, s], good[0][:, s]) and fids[s] == good[1][s] and f2[s] == good[3][s]
            assert np.array_equal(gn[s], good[5][s]) and np.array_equal(gs[s], good[6][s])
        assert np.isnan(finals[:, 1]).all() and np.isnan(fids[1]) and np.isnan(f2[1]) and np.isnan(gn[1]).all() and np.isnan(gs[1]).all()
        assert np.isnan(J) and not np.isfinite(grad).all()
        after = call(c["noise"])
        for x, y in zip(after, good):
            np.testing.assert_array_equal(x, y)
    finally:
        sw.close()


@pytest.mark.gpu
def test_wide64_noise_refusals(qc):
    """Raised through Python with QC_ERR_UNSUPPORTED and exactly one "qc_sweep noise: " prefix, or QC_ERR_INVALID for the arguments; the
    handle serves `eval` afterwards."""
    L = qc._lib
    rng = np.random.default_rng(2)
    T, N = 5, 17
    sys17 = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, 0.2)])
    goal = ref.operator_to_iso_vec(_unitary(rng, N))
    common = dict(goal=goal, fid_kind="unitary")
    form, served = "the handle takes the mfma64-sweep form (2N = 34), which ", "which serves the forward sweep only"
    # (what, the word in noise_eval's refusal or None when served, the word in noise_grad's, the handle)
    made = [
        ("no bit", form + "serves the forward sweep only", form + "serves the forward sweep only",
         qc.RolloutSweep(sys17, [_herm(rng, N)], T, wide=True, wide64=True, **common)),
        ("grad without the bit", form + "does not serve noise trajectories", form + "does not serve noise trajectories",
         qc.RolloutSweep(sys17, [_herm(rng, N)], T, wide=True, wide64=True, wide64_grad=True, **common)),
        ("no perturbations", "n_pert = 0", "n_pert = 0", qc.RolloutSweep(sys17, [], T, **HANDLE, **common)),
        ("the bit without bit 11", None, served, qc.RolloutSweep(sys17, [_herm(rng, N)], T, **EVAL, **common)),
    ]
    for name, word_eval, word_grad, sw in made:
        try:
            assert sw.kernel_name == "mfma64-sweep" and sw.noise_supported == (word_eval is None), name
            if word_eval is not None:
                assert word_eval in sw.noise_unsupported_reason and sw.noise_unsupported_reason.startswith("qc_sweep noise: "), name
            S = 2
            Z = sw.pack(rng.uniform(-1, 1, (sw.m, T)), rng.uniform(0.1, 0.3, T))
            init = ref.operator_to_iso_vec(np.eye(sw.N))
            noise, theta = np.zeros((S, T - 1, sw.p)), np.zeros((S, sw.p))
            for call, word in ((sw.noise_eval, word_eval), (sw.noise_grad, word_grad)):
                if word is None:
                    assert np.isfinite(call(Z, init, noise, theta)[0]).all()
                    continue
                with pytest.raises(qc.QCollocError) as e:
                    call(Z, init, noise, theta)
                assert e.value.code == L.QC_ERR_UNSUPPORTED and word in str(e.value) and str(e.value).count("qc_sweep noise: ") == 1, (name, str(e.value))
            finals, _ = sw.eval(Z, init, theta, fids=False)
            assert np.isfinite(finals).all()
        finally:
            sw.close()
    # the stored-state flag: refused in this form as it was, by the descriptor's scope and at the call
    sw = qc.RolloutSweep(sys17, [_herm(rng, N)], T, stored_states=True, **HANDLE, **common)
    try:
        assert sw.noise_supported and not sw.grad_supported and "stored-state gradients" in sw.grad_unsupported_reason
        Z, init = sw.pack(rng.uniform(-1, 1, (1, T)), rng.uniform(0.1, 0.3, T)), ref.operator_to_iso_vec(np.eye(N))
        with pytest.raises(qc.QCollocError) as e:
            sw.grad(Z, init, np.zeros((2, 1)))
        assert e.value.code == L.QC_ERR_UNSUPPORTED and "stored-state gradients" in str(e.value)
        assert np.isfinite(sw.noise_eval(Z, init, np.zeros((2, T - 1, 1)))[0]).all()      # the evaluation does not look at the flag
    finally:
        sw.close()
    # NULL noise and noise overlapping an output, through the C entry points
    sw = qc.RolloutSweep(sys17, [_herm(rng, N)], T, **HANDLE, **common)
    try:
        S = 2
        dev = torch.device("cuda:0")
        z = lambda n: torch.zeros(n, dtype=torch.float64, device=dev)
        dZ, dinit, dth = z(sw.Z_len), z(sw.ns), z(S)
        big = z(S * (T - 1) + S * sw.ns)
        ptr = lambda x: C.c_void_p(x.data_ptr())
        rc = L.lib.qc_sweep_noise_eval_dev(sw._h, ptr(dZ), ptr(dinit), S, ptr(dth), None, None, ptr(big), None, None)
        assert rc == L.QC_ERR_INVALID and "noise is NULL" in L.lib.qc_sweep_last_error(sw._h).decode()
        rc = L.lib.qc_sweep_noise_eval_dev(sw._h, ptr(dZ), ptr(dinit), S, ptr(dth), None, ptr(big), ptr(big), None, None)
        assert rc == L.QC_ERR_INVALID and "noise overlaps an output" in L.lib.qc_sweep_last_error(sw._h).decode()
        rc = L.lib.qc_sweep_noise_grad_dev(sw._h, ptr(dZ), ptr(dinit), S, ptr(dth), None, None, None, None, None, None, None, ptr(big), None)
        assert rc == L.QC_ERR_INVALID and "noise is NULL" in L.lib.qc_sweep_last_error(sw._h).decode()
        rc = L.lib.qc_sweep_noise_grad_dev(sw._h, ptr(dZ), ptr(dinit), S, ptr(dth), None, ptr(big), None, None, None, None, None, ptr(big), None)
        assert rc == L.QC_ERR_INVALID and "noise overlaps an output" in L.lib.qc_sweep_last_error(sw._h).decode()
        torch.cuda.synchronize()
    finally:
        sw.close()


@pytest.mark.gpu
def test_wide64_noise_objective_in_an_evaluator(qc):
    """`SweepNoiseInfidelityObjective(wide=True, wide64=True, wide64_grad=True, wide64_noise=True)` at 17 levels, T = 6, S = 3: grad_L
    against central differences of its own value (1e-6), and the term inside a first-order `QuantumControlEvaluator`."""
    rng = np.random.default_rng(14)
    N, m, T, S = 17, 2, 6, 3
    traj = tg._traj(qc, rng, N=N, m=m, T=T)
    sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, 0.3) for _ in range(m)])
    perts = [_herm(rng, N), _herm(rng, N)]
    noise, w = rng.uniform(-0.2, 0.2, (S, T - 1, 2)), rng.uniform(0.1, 0.3, S)
    with pytest.raises(qc.QCollocError) as e:
        qc.SweepNoiseInfidelityObjective(traj, sys_, perts, noise, weights=w, wide=True, wide64=True, wide64_grad=True)
    assert e.value.code == qc._lib.QC_ERR_UNSUPPORTED and "mfma64-sweep" in str(e.value)
    obj = qc.SweepNoiseInfidelityObjective(traj, sys_, perts, noise, weights=w, **HANDLE)
    Z = traj.datavec
    assert obj._sweep.kernel_name == "mfma64-sweep" and obj.S == S
    g0 = obj.grad_L(Z)
    assert obj.noise_sensitivity(Z).shape == (S, T - 1, 2)
    for k in (2 * traj.dim + traj.offset("a"), 4 * traj.dim + traj.offset("a") + 1, 3 * traj.dim + traj.offset("Δt")):
        e_k = np.zeros(Z.size)
        e_k[k] = 1e-5
        fd = (obj.L(Z + e_k) - obj.L(Z - e_k)) / 2e-5
        print(f"wide64 noise objective entry {k}: central difference {fd:.9e}, grad_L {g0[k]:.9e}")
        assert abs(fd - g0[k]) <= 1e-6 * max(1.0, abs(fd)), k

    class _Dyn:      # the evaluator reads the dimensions and structures of its dynamics at construction, nothing else here
        class dims:
            Z_len, n_rows, jac_nnz, hess_nnz = Z.size, 0, 0, 0
        dF_structure = (np.empty(0, dtype=np.int64), np.empty(0, dtype=np.int64))
        mu_d2F_structure = (np.empty(0, dtype=np.int64), np.empty(0, dtype=np.int64))

    reg = qc.TrajectoryObjective(qc.QuadraticRegularizer("a", traj, 1e-2), traj)
    ev = qc.QuantumControlEvaluator(_Dyn(), [reg, obj], eval_hessian=False)
    g = np.empty(Z.size)
    ev.eval_objective_gradient(g, Z)
    np.testing.assert_array_equal(g, (np.zeros(Z.size) + reg.grad_L(Z)) + obj.grad_L(Z))
    assert ev.eval_objective(Z) == float(reg.L(Z) + obj.L(Z))
    obj.close()


@pytest.mark.gpu
def test_three_transmon_noise_polish_example(qc):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import three_transmon_noise_polish
    before, after, profile, kernel = three_transmon_noise_polish.polish(T=6, S=3, steps=2, verbose=False)
    print(f"mean infidelity over the realisations {before:.6e} -> {after:.6e}; profile {np.array2string(profile, precision=3)}")
    assert kernel == "mfma64-sweep" and after < before
    assert profile.shape == (5, 3) and np.isfinite(profile).all() and profile.max() > 0
