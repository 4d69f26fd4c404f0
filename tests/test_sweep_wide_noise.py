"""Noise-trajectory sweeps on wide handles ("mfma32-sweep" with QC_SWEEP_WIDE_NOISE, csrc/qc_sweep32_noise.hip): `qc_sweep_noise_eval*` and
`qc_sweep_noise_grad*` for 16 < 2N <= 32, every matrix 2 x 2 tiles, with up to 8 drives and 8 perturbations (no tile limit: nothing is
resident in that form).  CPU: the new bit of `qc_sweep_desc.wide`, the device-free scope queries, the reference's two routes at a wide
size, and the preconditions the GPU cases exist for.  GPU: every output against the scipy reference of tests/sweep_noise_reference.py,
the squarings, exact equalities at zero noise, the resolution identity, additive control noise against single-sample calls, a Lindblad
handle at 2N = 32, a filled launch, bit-level properties, a NaN, the refusals, the objective and the example.

Tolerances are those at the top of tests/test_sweep_noise.py, always against the reference: states rtol 1e-10 / atol 1e-11, fidelities
1e-9, every gradient output (grad_noise included) per sample |got - want| <= 1e-9 max(1, max |.|).
Every sample of mid-size and filled launches, long chunks, 15 and 16 generators: tests/test_sweep_wide_noise_every_sample.py."""
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
import test_sweep_wide as tw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_herm, _unitary = ts._herm, ts._unitary
NOISE = 64          # QC_SWEEP_WIDE_NOISE
ODD = (1, 3, 9, 11, 17, 19, 25, 27)

# name: (state, levels, m, p, scale given, free timestep, S, T, (kind, subspace, form))
WIDE_NOISE_CASES = {
    "levels9-S3": ("unitary", 9, 2, 1, False, True, 3, 6, ("unitary", None, "abs")),               # padded tiles; chunks of 2, 2, 1
    "levels16-full": ("unitary", 16, 3, 2, True, False, 2, 4, ("unitary", [0, 1, 2, 3], "abs")),   # full tiles; 16 state columns
    "levels10-ket": ("ket", 10, 1, 2, False, False, 5, 9, ("ket", None, "abs")),                   # one state column
    "many-generators": ("unitary", 9, 5, 4, True, True, 3, 5, ("unitary", None, "abs")),           # m + p = 9; the timestep in lane 9
    "no-drives": ("unitary", 9, 0, 1, False, True, 3, 5, ("unitary", None, "abs")),                # every coefficient lane reads noise
}
# chunk, n_chunks, last chunk of each case's launch
WIDE_NOISE_CHUNKS = {"levels9-S3": (2, 3, 1), "levels16-full": (2, 2, 1), "levels10-ket": (3, 3, 2), "many-generators": (2, 2, 2), "no-drives": (2, 2, 2)}


def build(qc, name):
    state, L, m, p, use_scale, free, S, T, fid = WIDE_NOISE_CASES[name]
    rng = np.random.default_rng(sum(map(ord, "wide-noise " + name)))
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
    # the name keys the shared reference cache of test_sweep_noise.reference: kept apart from that file's own cases
    return dict(name="wide " + name, L=L, m=m, p=p, S=S, T=T, system=system, perts=perts, G0=G0, Gd=Gd, Gp=Gp, init=init, cols=cols, goal=goal,
                kind=kind, subspace=subspace, form=form, controls=controls, dts=dts, theta=theta, scale=scale, noise=noise)


def _make(qc, c, **kw):
    return tn._make(qc, c, **{**dict(wide=True, wide_noise=True), **kw})


def _squaring_case(qc):
    """L = 9, a small drift, P = diag(+-1) (column sums of its iso generator: 1) and |dt xi| = 0.08 2^k: about k squarings per interval."""
    rng = np.random.default_rng(23)
    N, m, p, T, S, dt = 9, 1, 1, 8, 4, 0.2
    H0, Hd = _herm(rng, N, 0.003), [_herm(rng, N, 0.003)]
    P = np.diag(np.array([1.0, -1.0, 1.0, -1.0, 1.0, -1.0, 1.0, -1.0, 1.0])).astype(complex)
    system = qc.QuantumSystem(H0, Hd)
    G0, Gd, Gp = ref.iso_generator(H0), [ref.iso_generator(Hd[0])], [ref.iso_generator(P)]
    controls = rng.uniform(-1, 1, (m, T))
    init, goal = ref.operator_to_iso_vec(_unitary(rng, N)), ref.operator_to_iso_vec(_unitary(rng, N))
    k = np.array([[0, 3, 6, 1, 2, 4, 5], [6, 0, 7, 2, 2, 2, 2], [1, 1, 1, 5, 0, 6, 3], [0, 0, 0, 0, 0, 0, 4]], dtype=np.float64)
    noise = (0.4 * 2.0 ** k * rng.choice([-1.0, 1.0], (S, T - 1)))[:, :, None]
    theta = np.zeros((S, 1))
    sq = np.array([[ts._squarings(np.abs(dt * nref.interval_generator(G0, Gd, Gp, controls[:, t], theta[s], np.ones(m), noise[s, t])).sum(axis=0).max())
                    for t in range(T - 1)] for s in range(S)])
    c = dict(name="wide squarings", L=N, m=m, p=p, S=S, T=T, system=system, perts=[P], G0=G0, Gd=Gd, Gp=Gp, init=init, cols=N, goal=goal,
             kind="unitary", subspace=None, form="abs", controls=controls, dts=dt, theta=theta, scale=None, noise=noise)
    return c, sq


FILLED_S, FILLED_T = 2048, 3


def _filled_case(qc):
    """S = 2048 fills the device: one chunk.  Noise, theta and scale are 4 distinct samples, tiled."""
    rng = np.random.default_rng(77)
    N, m, p, T, S = 9, 2, 1, FILLED_T, FILLED_S
    H0, Hd, perts = _herm(rng, N), [_herm(rng, N, (N * m) ** -0.5) for _ in range(m)], [_herm(rng, N)]
    system = qc.QuantumSystem(H0, Hd)
    G0, Gd, Gp = ref.iso_generator(H0), [ref.iso_generator(H) for H in Hd], [ref.iso_generator(P) for P in perts]
    init, goal = ref.operator_to_iso_vec(_unitary(rng, N)), ref.operator_to_iso_vec(_unitary(rng, N))
    controls, dts = rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T)
    theta4, scale4, noise4 = rng.uniform(-0.3, 0.3, (4, p)), rng.uniform(0.9, 1.1, (4, m)), rng.uniform(-0.3, 0.3, (4, T - 1, p))
    four = dict(name="wide filled (first 4)", L=N, m=m, p=p, S=4, T=T, system=system, perts=perts, G0=G0, Gd=Gd, Gp=Gp, init=init, cols=N, goal=goal,
                kind="unitary", subspace=None, form="abs", controls=controls, dts=dts, theta=theta4, scale=scale4, noise=noise4)
    rep = S // 4
    full = dict(four, name="wide filled", S=S, theta=np.tile(theta4, (rep, 1)), scale=np.tile(scale4, (rep, 1)), noise=np.tile(noise4, (rep, 1, 1)))
    return four, full


# ---------------------------------------------------------------------------------------------------------------------------------
#  CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_wide_noise_bit_is_validated(qc):
    L = qc._lib
    val = lambda D: L.lib.qc_sweep_desc_validate(C.byref(D.d))
    assert L.QC_SWEEP_WIDE_NOISE == NOISE == 64
    header = open(os.path.join(ROOT, "include", "qcolloc.h")).read()
    assert "#define QC_SWEEP_WIDE_NOISE 64" in header
    for N in (9, 4):        # 2N = 18 and 2N = 8
        for good in (0,) + ODD + tuple(v | NOISE for v in ODD):
            assert val(tw._wdesc(qc, good, N=N)) == L.QC_OK, (N, good)
        for bad in (64, 66, 68, 69, 96 | 1, 128 | 1, 4, 5, 12, 13, 15, 20, 21, 33):
            assert val(tw._wdesc(qc, bad, N=N)) == L.QC_ERR_INVALID, (N, bad)
            msg = L.lib.qc_sweep_last_error(None).decode()
            assert msg.startswith("qc_sweep: wide") and "17, 19, 25 or 27" in msg and "QC_SWEEP_WIDE_TANGENT (16)" in msg, (N, bad, msg)
            assert "QC_SWEEP_WIDE_NOISE (64)" in msg, (N, bad, msg)
    with pytest.raises(ValueError, match="wide_noise=True needs wide=True"):
        qc.RolloutSweep(qc.QuantumSystem(np.zeros((2, 2)), [qc.GATES["X"]]), [qc.GATES["Z"]], 4, wide_noise=True)


def _wd(qc, wide, **kw):
    D = tg._GDesc(qc, **kw)
    D.d.wide = wide
    return D


def test_wide_noise_scope_without_a_device(qc):
    L = qc._lib
    U = L.QC_FID_UNITARY
    old = "qc_sweep noise: noise trajectories are not served in the mfma32-sweep form"
    rc, ok, msg = tn._supported(qc, _wd(qc, 1, N=12, m=2, fid_kind=U))
    assert (rc, ok) == (L.QC_OK, 0) and msg == old       # the old message verbatim
    for bits in (1, 3, 9, 27):
        assert tn._supported(qc, _wd(qc, bits, N=12, m=2, fid_kind=U))[2] == old, bits
    for m, p in ((2, 1), (5, 4), (8, 8), (0, 1)):
        for bits in (65, 65 | 2, 65 | 16, 27 | 64):
            assert tn._supported(qc, _wd(qc, bits, N=12, m=m, p=p, fid_kind=U))[:2] == (L.QC_OK, 1), (m, p, bits)
    rc, ok, msg = tn._supported(qc, _wd(qc, 65, N=12, m=2, p=0, fid_kind=U))
    assert (rc, ok) == (L.QC_OK, 0) and msg.startswith("qc_sweep noise: ") and "n_pert = 0" in msg
    rc, ok, msg = tn._supported(qc, _wd(qc, 65, N=8, m=6, p=3, fid_kind=U))       # 2N = 16: the 16 x 16 form and its rule
    assert (rc, ok) == (L.QC_OK, 0) and "m + n_pert = 6 + 3 exceeds the 8 tiles" in msg
    assert tn._supported(qc, _wd(qc, 65, N=8, m=6, p=2, fid_kind=U))[:2] == (L.QC_OK, 1)
    rc, ok, msg = tn._supported(qc, _wd(qc, 0, N=12, m=2, fid_kind=U))
    assert (rc, ok) == (L.QC_OK, 0) and "rollout-per-sample form (2N = 24 > 16)" in msg
    rc, ok, msg = tn._supported(qc, _wd(qc, 65, N=20, m=2, fid_kind=U))
    assert (rc, ok) == (L.QC_OK, 0) and "rollout-per-sample form (2N = 40 > 32)" in msg
    rc, ok, msg = tn._supported(qc, _wd(qc, 65, N=12, m=9, fid_kind=U))
    assert (rc, ok) == (L.QC_OK, 0) and "rollout-per-sample form (9 drives > 8)" in msg
    # an open system (2N = 32, density fidelity): the evaluation is served
    open4 = _wd(qc, 65, N=16, m=2, cols=1, fid_kind=L.QC_FID_DENSITY)
    open4.G0[:] = np.random.default_rng(0).standard_normal(32 * 32)
    assert tn._supported(qc, open4)[:2] == (L.QC_OK, 1)


def test_wide_noise_bit_changes_no_other_scope(qc):
    """`qc_sweep_desc_grad_supported`, `_vjp_`, `_jvp_` and `_hvp_supported`, and the launch: the same answers and messages with and
    without the bit."""
    L = qc._lib
    U = L.QC_FID_UNITARY

    def variants(bits):
        plain = _wd(qc, bits, N=12, m=2, fid_kind=U)
        open_ = _wd(qc, bits, N=16, m=2, cols=1, fid_kind=L.QC_FID_DENSITY)
        open_.G0[:] = np.random.default_rng(1).standard_normal(32 * 32)
        stored = _wd(qc, bits, N=16, m=2, cols=1, fid_kind=L.QC_FID_DENSITY)
        stored.G0[:] = open_.G0
        stored.d.reserved1[0] = L.QC_SWEEP_STORED_STATES
        return dict(plain=plain, open=open_, stored=stored, narrow=_wd(qc, bits, N=4, m=2, fid_kind=U), large=_wd(qc, bits, N=20, m=2, fid_kind=U))

    for bits in ODD:
        a, b = variants(bits), variants(bits | NOISE)
        for what in a:
            for fn in ("qc_sweep_desc_grad_supported", "qc_sweep_desc_vjp_supported", "qc_sweep_desc_jvp_supported", "qc_sweep_desc_hvp_supported"):
                got = []
                for D in (a[what], b[what]):
                    ok = C.c_int32(-1)
                    rc = getattr(L.lib, fn)(C.byref(D.d), C.byref(ok))
                    got.append((rc, ok.value, L.lib.qc_sweep_last_error(None).decode() if not ok.value else None))
                assert got[0] == got[1], (bits, what, fn, got)
            for S in (1, 5, 300, 2048):
                out = []
                for D in (a[what], b[what]):
                    mf, ch, nch = C.c_int32(), C.c_int64(), C.c_int64()
                    assert L.lib.qc_sweep_desc_launch(C.byref(D.d), S, C.byref(mf), C.byref(ch), C.byref(nch)) == L.QC_OK
                    out.append((mf.value, ch.value, nch.value))
                assert out[0] == out[1], (bits, what, S)


def test_wide_reference_routes_agree():
    """Forward mode (expm_frechet) against central differences of the chain at L = 9 (2N = 18): 1e-6 relative, as in test_sweep_noise.py."""
    rng = np.random.default_rng(909)
    N, m, p, T, S = 9, 2, 2, 4, 2
    G0, Gd = ref.iso_generator(_herm(rng, N)), [ref.iso_generator(_herm(rng, N, 0.3)) for _ in range(m)]
    Gp = [ref.iso_generator(_herm(rng, N)) for _ in range(p)]
    controls, dts = rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T)
    theta, scale, noise = rng.uniform(-0.3, 0.3, (S, p)), rng.uniform(0.9, 1.1, (S, m)), rng.uniform(-0.3, 0.3, (S, T - 1, p))
    init, goal = ref.operator_to_iso_vec(_unitary(rng, N)), ref.operator_to_iso_vec(_unitary(rng, N))
    args = (G0, Gd, Gp, controls, dts, init, theta, scale, noise, [0, 1], "unitary", goal, N, [0, 1, 3, 4], "abs")
    (a, an), (b, bn) = nref.noise_grads_forward(*args), nref.noise_grads_fd(*args)
    assert a.shape == b.shape == (2, T - 1, m + 1) and an.shape == bn.shape == (2, T - 1, p)
    for what, x, y in (("controls", a, b), ("noise", an, bn)):
        err = np.abs(x - y).max() / max(1.0, np.abs(x).max())
        print(f"L=9 {what}: forward vs central differences {err:.2e}, max |grad| {np.abs(x).max():.3f}")
        assert err < 1e-6 and np.abs(x).max() > 1e-3


def _launch(qc, N, m, p, S, T, bits=65):
    D = tw._wdesc(qc, bits, N=N, m=m, p=p, T=T)
    mf, ch, nch = C.c_int32(), C.c_int64(), C.c_int64()
    assert qc._lib.lib.qc_sweep_desc_launch(C.byref(D.d), S, C.byref(mf), C.byref(ch), C.byref(nch)) == qc._lib.QC_OK
    return bool(mf.value), ch.value, nch.value


@pytest.mark.parametrize("name", list(WIDE_NOISE_CASES))
def test_the_cases_are_what_they_claim(qc, name):
    """What each GPU case exists for, from numpy and the device-free launch query: the chunks, and derivatives that are not small."""
    c = build(qc, name)
    chunk, n_chunks, last = WIDE_NOISE_CHUNKS[name]
    assert _launch(qc, c["L"], c["m"], c["p"], c["S"], c["T"]) == (True, chunk, n_chunks)
    assert n_chunks > 1 and (c["T"] - 1) - (n_chunks - 1) * chunk == last
    if name == "levels9-S3":
        assert (chunk, n_chunks, last) == (2, 3, 1)          # several chunks, the last one shorter
    if name == "many-generators":
        assert c["m"] + c["p"] == 9 and np.ndim(c["dts"]) == 1       # what the 16 x 16 form refuses; the timestep's value in lane 9
    if name == "levels16-full":
        assert 2 * c["L"] == 32 and c["cols"] == 16
    rf, rfid, rgs, rgn = tn.reference(c)
    assert np.abs(rgn).max() > 1e-3 and (rgs.size == 0 or np.abs(rgs).max() > 1e-3)
    assert rgn.shape == (c["S"], c["T"] - 1, c["p"])


def test_the_special_cases_are_what_they_claim(qc):
    c, sq = _squaring_case(qc)
    assert _launch(qc, c["L"], c["m"], c["p"], c["S"], c["T"]) == (True, 3, 3)
    first = sq[:, :3]                                       # the first chunk of every sample
    assert first[0].min() == 0 and first[0].max() >= 6      # 0 .. at least 6 inside one chunk
    assert len({tuple(r) for r in sq}) == c["S"] and len({r.max() for r in first}) >= 3      # and different from sample to sample
    assert _launch(qc, 9, 2, 1, FILLED_S, FILLED_T) == (True, FILLED_T - 1, 1)       # the filled launch: one chunk
    four, full = _filled_case(qc)
    assert full["noise"].shape == (FILLED_S, FILLED_T - 1, 1) and np.array_equal(full["noise"][4:8], four["noise"])
    assert len({tuple(r.ravel()) for r in four["noise"]}) == 4
    assert np.abs(tn.reference(four)[3]).max() > 1e-3


# ---------------------------------------------------------------------------------------------------------------------------------
#  GPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(WIDE_NOISE_CASES))
def test_wide_noise_matches_the_reference(qc, name):
    c = build(qc, name)
    sw = _make(qc, c)
    try:
        assert sw.kernel_name == "mfma32-sweep" and sw.wide_noise and sw.noise_supported and sw.noise_unsupported_reason is None and sw.grad_supported
        chunk, n_chunks, _ = WIDE_NOISE_CHUNKS[name]
        assert sw.launch(c["S"]) == (True, chunk, n_chunks)
        Z = sw.pack(c["controls"], c["dts"])
        finals, fids = tn._check_call(sw, Z, c)[:2]
        if name == "levels9-S3":
            tn._check_call(sw, Z, c, weights=np.array([0.2, 1.5, 0.7]))
            f3, fid3 = qc.rollout_noise_sweep(c["init"], c["controls"], c["dts"], c["system"], c["perts"], c["noise"], c["theta"], cols=c["cols"],
                                              goal=c["goal"], fid_kind="unitary", wide=True)
            np.testing.assert_array_equal(f3, finals)
            np.testing.assert_array_equal(fid3, fids)
    finally:
        sw.close()


@pytest.mark.gpu
def test_wide_noise_through_the_squarings(qc):
    """Noise strong enough that the intervals of ONE chunk need 0 .. 7 squarings, differently in every sample."""
    c, sq = _squaring_case(qc)
    print("squarings per sample and interval:\n", sq)
    assert sq[0, :3].min() == 0 and sq[0, :3].max() >= 6
    sw = _make(qc, c)
    try:
        assert sw.kernel_name == "mfma32-sweep" and sw.launch(c["S"]) == (True, 3, 3)
        tn._check_call(sw, sw.pack(c["controls"]), c)
    finally:
        sw.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["levels9-S3", "levels10-ket"])
def test_wide_zero_noise_is_the_sweep(qc, name):
    """An explicit +0.0 noise array: finals and fids equal `eval`'s, fids / J / grad / grad_samples equal `grad`'s on the same handle,
    value for value.  And sum_t grad_noise[s, t, j] = grad_theta[s, j] of `param_grad` on a `wide_params` handle."""
    c = build(qc, name)
    sw = _make(qc, c, wide_params=True)
    try:
        assert sw._desc.wide == 1 | 2 | 64 and sw.kernel_name == "mfma32-sweep"
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
        tot, mag = gn.sum(axis=1), np.abs(gn).sum(axis=1)
        worst = (np.abs(tot - gth) / (1e-9 * np.maximum(1.0, mag))).max()
        print(f"SWEEP-WIDE-NOISE {name} resolution identity: worst |sum_t grad_noise - grad_theta| / bound = {worst:.2e}, max |grad_theta| = {np.abs(gth).max():.3e}")
        assert worst <= 1.0 and np.abs(gth).max() > 1e-3
    finally:
        sw.close()


@pytest.mark.gpu
def test_wide_additive_control_noise_against_single_sample_calls(qc):
    """P_0 = H_drive_0 at L = 9: one noise sweep against S = 5 single-sample `eval` calls on a `wide=True` handle that each carry
    a_{t,0} + xi[s, t] in a trajectory vector of their own."""
    rng = np.random.default_rng(31)
    N, m, T, S = 9, 2, 9, 5
    H0, Hd = _herm(rng, N), [_herm(rng, N, 0.3) for _ in range(m)]
    system = qc.QuantumSystem(H0, Hd)
    init = ref.operator_to_iso_vec(_unitary(rng, N))
    controls, dts = rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T)
    noise = rng.uniform(-0.2, 0.2, (S, T - 1))
    sw = qc.RolloutSweep(system, [Hd[0]], T, wide=True, wide_noise=True)
    plain = qc.RolloutSweep(system, [], T, wide=True)
    try:
        assert sw.kernel_name == plain.kernel_name == "mfma32-sweep"
        finals, fids = sw.noise_eval(sw.pack(controls, dts), init, noise)
        assert fids is None and finals.shape == (2 * N * N, S)
        for s in range(S):
            cs = controls.copy()
            cs[0, :T - 1] += noise[s]
            one, _ = plain.eval(plain.pack(cs, dts), init, np.zeros((1, 0)))
            ts._assert_states(finals[:, s], one[:, 0], f"wide additive control noise, sample {s}")
    finally:
        sw.close()
        plain.close()


def _open_case(qc):
    """Two qubits with T1 / T2 (levels 4, N = 16, 2N = 32) and a decay channel whose rate fluctuates."""
    rng = np.random.default_rng(41)
    L, m, T, S = 4, 2, 5, 3
    H0, Hd = _herm(rng, L), [_herm(rng, L, 0.4) for _ in range(m)]
    lower = np.array([[0, 1], [0, 0]], dtype=complex)
    one = np.eye(2, dtype=complex)
    diss = [0.2 * np.kron(lower, one), 0.2 * np.kron(one, lower), 0.15 * np.kron(np.diag([1.0, -1.0]).astype(complex), one)]
    system = qc.OpenQuantumSystem(H0, Hd, diss)
    perts = [np.asarray(qc.iso_operator(qc.OpenQuantumSystem.dissipator_superoperator(np.kron(one, lower))))]
    psi = rng.standard_normal(L) + 1j * rng.standard_normal(L)
    psi /= np.linalg.norm(psi)
    gk = rng.standard_normal(L) + 1j * rng.standard_normal(L)
    gk /= np.linalg.norm(gk)
    return dict(name="wide open4", L=L, m=m, p=1, S=S, T=T, system=system, perts=perts, G0=np.asarray(system.G_drift),
                Gd=[np.asarray(G) for G in system.G_drives], Gp=perts, init=qc.density_to_iso_vec(np.outer(psi, psi.conj())), cols=1,
                goal=np.concatenate([gk.real, gk.imag]), kind="density", subspace=None, form="abs", controls=rng.uniform(-1, 1, (m, T)),
                dts=rng.uniform(0.1, 0.3, T), theta=rng.uniform(0.1, 0.3, (S, 1)), scale=None, noise=rng.uniform(0.0, 0.2, (S, T - 1, 1)))


@pytest.mark.gpu
def test_wide_noise_on_a_lindblad_handle(qc):
    """N = 16 = 4^2, the density-operator fidelity: the evaluation serves generators that are not antisymmetric; the gradient is refused
    with the gradient's own reason, the stored-state flags set as well (they do not widen its scope)."""
    c = _open_case(qc)
    sw = _make(qc, c, stored_states=True, wide_stored=True)
    try:
        assert sw.N == 16 and sw.kernel_name == "mfma32-sweep" and sw.noise_supported and sw.grad_supported      # `grad` takes the stored-state walk
        Z = sw.pack(c["controls"], c["dts"])
        finals, fids = sw.noise_eval(Z, c["init"], c["noise"], c["theta"])
        want = nref.noise_finals(c["G0"], c["Gd"], c["Gp"], c["controls"], c["dts"], c["init"], c["theta"], None, c["noise"])
        ts._assert_states(finals, want, "wide open4 with noise")
        ts._assert_fids(fids, ref.fidelities(want, "density", c["goal"], c["L"]), "wide open4 with noise")
        with pytest.raises(qc.QCollocError) as e:
            sw.noise_grad(Z, c["init"], c["noise"], c["theta"])
        assert e.value.code == qc._lib.QC_ERR_UNSUPPORTED and "is not antisymmetric" in str(e.value) and str(e.value).count("qc_sweep noise: ") == 1
        f2, fid2 = sw.noise_eval(Z, c["init"], c["noise"], c["theta"])       # the handle is usable afterwards
        assert np.array_equal(f2, finals) and np.array_equal(fid2, fids)
    finally:
        sw.close()


@pytest.mark.gpu
def test_wide_noise_filled_launch(qc):
    """S = 2048: `launch(S)` reports one chunk.  The first 4 samples against the reference; every other sample is a copy of one of them
    and carries its bits in every per-sample output."""
    four, full = _filled_case(qc)
    sw = _make(qc, full)
    try:
        assert sw.kernel_name == "mfma32-sweep" and sw.launch(FILLED_S) == (True, FILLED_T - 1, 1)
        Z = sw.pack(full["controls"], full["dts"])
        rf, rfid, rgs, rgn = tn.reference(four)
        finals, fids = sw.noise_eval(Z, full["init"], full["noise"], full["theta"], full["scale"])
        J, f2, grad, gn, gs = sw.noise_grad(Z, full["init"], full["noise"], full["theta"], full["scale"], per_sample=True)
        ts._assert_states(finals[:, :4], rf, "wide filled")
        ts._assert_fids(fids[:4], rfid, "wide filled")
        tn._assert_samples(gs[:4], rgs, "wide filled grad_samples")
        tn._assert_samples(gn[:4], rgn, "wide filled grad_noise")
        np.testing.assert_array_equal(f2, fids)
        for s in range(4):
            assert np.array_equal(finals[:, s::4], np.repeat(finals[:, s:s + 1], FILLED_S // 4, axis=1)), s
            assert np.all(fids[s::4] == fids[s]), s
            assert np.array_equal(gn[s::4], np.broadcast_to(gn[s], gn[s::4].shape)) and np.array_equal(gs[s::4], np.broadcast_to(gs[s], gs[s::4].shape)), s
    finally:
        sw.close()


@pytest.mark.gpu
def test_wide_noise_bits_host_device_and_side_stream(qc):
    """Host entry = device entry = device entry on a side stream; repeated calls identical; every subset of one gradient output alone
    gives the bits it gives with the others."""
    c = build(qc, "many-generators")
    rng = np.random.default_rng(8)
    sw = _make(qc, c)
    T, m, p = c["T"], c["m"], c["p"]
    Z, init = sw.pack(c["controls"], c["dts"]), c["init"]
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    mk = lambda *shape: torch.full(shape, -7.0, dtype=torch.float64, device=dev)
    side = torch.cuda.Stream(device=dev)
    try:
        for i, S in enumerate((3, 40, 5)):
            theta, scale, w = rng.uniform(-0.3, 0.3, (S, p)), rng.uniform(0.9, 1.1, (S, m)), rng.uniform(0.5, 1.5, S)
            noise = rng.uniform(-0.3, 0.3, (S, T - 1, p))
            finals, fids = sw.noise_eval(Z, init, noise, theta, scale)
            first = sw.noise_grad(Z, init, noise, theta, scale, weights=w, per_sample=True)      # J, fids, grad, grad_noise, grad_samples
            np.testing.assert_array_equal(first[1], fids)
            if i == 1:
                for _ in range(3):
                    again = sw.noise_grad(Z, init, noise, theta, scale, weights=w, per_sample=True)
                    assert again[0] == first[0]
                    for a, b in zip(again[1:], first[1:]):
                        np.testing.assert_array_equal(a, b)
                    f2, fid2 = sw.noise_eval(Z, init, noise, theta, scale)
                    assert np.array_equal(f2, finals) and np.array_equal(fid2, fids)
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
            # outputs are optional one at a time, and none depends on the others
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
def test_wide_noise_bit_changes_nothing_else(qc):
    """A wide = 65 handle's `eval` / `grad` / `vjp` outputs, kernel name and launch equal a wide = 1 handle's; at 2N = 8 a wide = 65
    handle's noise outputs equal a wide = 0 handle's."""
    c = build(qc, "levels9-S3")
    Zc = (c["controls"], c["dts"])
    a, b = _make(qc, c), tn._make(qc, c, wide=True)
    try:
        assert (a._desc.wide, b._desc.wide) == (65, 1)
        assert a.kernel_name == b.kernel_name == "mfma32-sweep" and all(a.launch(S) == b.launch(S) for S in (1, 3, 300, 2048))
        assert not b.noise_supported and b.grad_supported == a.grad_supported and b.vjp_supported == a.vjp_supported and b.jvp_supported == a.jvp_supported
        Z = a.pack(*Zc)
        cot = np.random.default_rng(4).standard_normal((c["S"], a.ns))
        for call in (lambda s: s.eval(Z, c["init"], c["theta"], c["scale"]), lambda s: s.grad(Z, c["init"], c["theta"], c["scale"], per_sample=True),
                     lambda s: s.vjp(Z, c["init"], cot, c["theta"], c["scale"], per_sample=True, init_grad=True)):
            for x, y in zip(call(a), call(b)):
                np.testing.assert_array_equal(x, y)
    finally:
        a.close()
        b.close()
    n = tn.build(qc, "qubits3-full")      # 2N = 16: the 16 x 16 form, whatever the bits
    a, b = tn._make(qc, n, wide=True, wide_noise=True), tn._make(qc, n)
    try:
        assert (a._desc.wide, b._desc.wide) == (65, 0) and a.kernel_name == b.kernel_name == "mfma16-sweep"
        Z = a.pack(n["controls"], n["dts"])
        for x, y in zip(a.noise_eval(Z, n["init"], n["noise"], n["theta"], n["scale"]), b.noise_eval(Z, n["init"], n["noise"], n["theta"], n["scale"])):
            np.testing.assert_array_equal(x, y)
        for x, y in zip(a.noise_grad(Z, n["init"], n["noise"], n["theta"], n["scale"], per_sample=True),
                        b.noise_grad(Z, n["init"], n["noise"], n["theta"], n["scale"], per_sample=True)):
            np.testing.assert_array_equal(x, y)
    finally:
        a.close()
        b.close()


@pytest.mark.gpu
def test_wide_noise_non_finite_input(qc):
    """A NaN at noise[1, 2, 0] of three samples does not raise: samples 0 and 2 carry the bits of the clean run in every per-sample
    output, sample 1 and the sums over the samples are not finite, and the handle then serves a clean call as if nothing had happened."""
    c = build(qc, "levels9-S3")
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
def test_wide_noise_refusals(qc):
    """Raised through Python with QC_ERR_UNSUPPORTED and exactly one "qc_sweep noise: " prefix; the handle serves `eval` afterwards."""
    L = qc._lib
    rng = np.random.default_rng(2)
    T = 5
    sys12 = qc.QuantumSystem(_herm(rng, 12), [_herm(rng, 12, 0.2)])
    goal12 = ref.operator_to_iso_vec(_unitary(rng, 12))
    sys20 = qc.QuantumSystem(_herm(rng, 20), [_herm(rng, 20, 0.2)])
    goal20 = ref.operator_to_iso_vec(_unitary(rng, 20))
    made = [
        ("wide without the bit", "noise trajectories are not served in the mfma32-sweep form",
         qc.RolloutSweep(sys12, [_herm(rng, 12)], T, goal=goal12, fid_kind="unitary", wide=True)),
        ("no perturbations", "n_pert = 0", qc.RolloutSweep(sys12, [], T, goal=goal12, fid_kind="unitary", wide=True, wide_noise=True)),
        ("per-sample: size", "rollout-per-sample form (2N = 40 > 32)",
         qc.RolloutSweep(sys20, [_herm(rng, 20)], T, goal=goal20, fid_kind="unitary", wide=True, wide_noise=True)),
    ]
    for name, word, sw in made:
        try:
            assert not sw.noise_supported and word in sw.noise_unsupported_reason and sw.noise_unsupported_reason.startswith("qc_sweep noise: "), name
            S = 2
            Z = sw.pack(rng.uniform(-1, 1, (sw.m, T)), 0.2)
            init = ref.operator_to_iso_vec(np.eye(sw.N))
            noise, theta = np.zeros((S, T - 1, sw.p)), np.zeros((S, sw.p))
            for call in (sw.noise_eval, sw.noise_grad):
                with pytest.raises(qc.QCollocError) as e:
                    call(Z, init, noise, theta)
                assert e.value.code == L.QC_ERR_UNSUPPORTED and word in str(e.value) and str(e.value).count("qc_sweep noise: ") == 1, name
            finals, _ = sw.eval(Z, init, theta, fids=False)
            assert np.isfinite(finals).all()
        finally:
            sw.close()


@pytest.mark.gpu
def test_wide_noise_objective_in_an_evaluator(qc):
    """`SweepNoiseInfidelityObjective(wide=True, wide_noise=True)` at L = 9, T = 6, S = 3: grad_L against central differences of its own
    value (1e-6), and the term inside a first-order `QuantumControlEvaluator`."""
    rng = np.random.default_rng(14)
    N, m, T, S = 9, 2, 6, 3
    traj = tg._traj(qc, rng, N=N, m=m, T=T)
    sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, 0.3) for _ in range(m)])
    perts = [_herm(rng, N), _herm(rng, N)]
    noise, w = rng.uniform(-0.2, 0.2, (S, T - 1, 2)), rng.uniform(0.1, 0.3, S)
    with pytest.raises(qc.QCollocError) as e:
        qc.SweepNoiseInfidelityObjective(traj, sys_, perts, noise, weights=w, wide=True)
    assert e.value.code == qc._lib.QC_ERR_UNSUPPORTED and "mfma32-sweep" in str(e.value)
    obj = qc.SweepNoiseInfidelityObjective(traj, sys_, perts, noise, weights=w, wide=True, wide_noise=True)
    Z = traj.datavec
    assert obj._sweep.kernel_name == "mfma32-sweep" and obj.S == S
    g0 = obj.grad_L(Z)
    assert obj.noise_sensitivity(Z).shape == (S, T - 1, 2)
    for k in (2 * traj.dim + traj.offset("a"), 4 * traj.dim + traj.offset("a") + 1, 3 * traj.dim + traj.offset("Δt")):
        e_k = np.zeros(Z.size)
        e_k[k] = 1e-5
        fd = (obj.L(Z + e_k) - obj.L(Z - e_k)) / 2e-5
        print(f"wide noise objective entry {k}: central difference {fd:.9e}, grad_L {g0[k]:.9e}")
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
def test_transmon_noise_polish_example(qc):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import transmon_noise_polish
    before, after, profile, kernel = transmon_noise_polish.polish(T=8, S=4, steps=3, verbose=False)
    print(f"mean infidelity over the realisations {before:.6e} -> {after:.6e}; profile {np.array2string(profile, precision=3)}")
    assert kernel == "mfma32-sweep" and after < before
    assert profile.shape == (7, 2) and np.isfinite(profile).all() and profile.max() > 0
