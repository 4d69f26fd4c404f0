"""Parameter gradients and parameter cotangents in the "mfma64-sweep" form (32 < 2N <= 64): `qc_sweep_desc.wide = QC_SWEEP_WIDE |
QC_SWEEP_WIDE_64 | QC_SWEEP_WIDE_64_GRAD | QC_SWEEP_WIDE_64_PARAMS` (11265), `RolloutSweep(..., wide=True, wide64=True, wide64_grad=True,
wide64_params=True)`: dF_s/dtheta[s, j] and dF_s/dc[s, k] from the parameter flavour of the 4 x 4-tile walk (csrc/qc_sweep64_grad.hip,
qc_sweep64_grad_kernel<true>).  CPU: the bit's validation, the launch rule and scope queries with and without it, keywords, the
reference's two routes at 17 levels.  GPU: every value of grad_theta / grad_scale against the forward-mode reference of
tests/sweep_param_grad_reference.py (handles without a fidelity: `sweep_vjp_reference.pullback_forward`) at the smallest shapes that reach
each path of the kernel, the squarings, the identity between the outputs of one call, bits, the pullback, every sample on both sides of
the fill constant, refusals, a NaN in one sample, the example.

Tolerances are test_sweep_param_grad.py's (read its header): per sample |got - want| <= 1e-9 max(1, A_s), A_s the largest sum over the
intervals of |term| among the sample's parameters; identities between outputs of one call to 1e-12 max(1, A_s).  `pullback_forward`
returns sums, not terms, so pullback outputs are held to the rule of test_sweep_vjp.py, 1e-9 max(1, max |want_s|), which is never wider
(max |want_s| <= A_s).  Measured worst ratios: DESIGN.md 5.8.13 and profiles/sweep_wide64_param_summary.txt.

The case "chunks" (S = 3, T = 26) runs five chunks of five intervals a sample, the last one full; ragged last chunks are "chunks-ragged"
(T = 12: 3, 3, 3, 2), the squaring cases (the same) and the bits test (T = 27: five chunks of 5 and one of 1).  "no-drives-free-dt"
(m = 0 with a free timestep: nd = 1, the perturbations in lanes 1 and 2) and "subspace-abs2" (a unitary fidelity on levels 0, 1, 3, 4 in
the squared form) are lane maps and a seed no other case here reaches.  Every sample of launches of 250 .. 510 workgroups with several
chunks of several intervals: tests/test_sweep_wide64_params_every_sample.py."""
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest
import torch

import sweep_param_grad_reference as pref
import sweep_reference as ref
import test_sweep as ts
import test_sweep_grad as tg
import test_sweep_param_grad as tp
import test_sweep_vjp as tv
import test_sweep_wide as tw
import test_sweep_wide64 as t64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_herm, _unitary = ts._herm, ts._unitary
W64, WG, WP = t64.W64, 2048, 8192
WIDE_G = 1 | W64 | WG             # 3073: gradients and pullbacks, no parameter outputs
WIDE = WIDE_G | WP                # 11265
HANDLE = dict(wide=True, wide64=True, wide64_grad=True, wide64_params=True)
HANDLE_G = dict(wide=True, wide64=True, wide64_grad=True)
FORM = "64par"                    # the key of test_sweep_vjp.reference's cache for this file's pullback cases

# name: (levels, state columns, m, p, free timestep, S, T, fidelity kind (full space, "abs") | (kind, subspace, form) | None,
#        scale: None | "given" | (sample, drive) of an exact zero)
CASES = {
    "pad": (17, 17, 2, 1, True, 3, 6, "unitary", (1, 0)),                   # zero padding to 64, second column tile with one live column
    "full": (32, 32, 3, 2, False, 2, 4, "unitary", (0, 2)),                 # no padding, nd = m
    "ket": (20, 1, 1, 8, True, 3, 5, "ket", None),                          # QC_MAX_PERT: theta lanes up to m + 1 + 8
    "many-drives": (17, 8, 16, 8, True, 2, 3, None, "given"),               # nd + p = 25, the widened part[] row
    "no-drives": (20, 8, 0, 2, False, 2, 4, None, None),                    # nd = 0: only the perturbation lanes
    "chunks": (17, 8, 2, 2, True, 3, 26, None, "given"),                    # five chunks a sample
    "chunks-ragged": (17, 8, 2, 2, True, 3, 12, None, (2, 1)),              # chunks of 3, 3, 3, 2
    "one-interval-chunks": (17, 8, 2, 1, True, 5, 3, None, "given"),        # two chunks of one interval: the chunk loop runs once
    "no-drives-free-dt": (17, 8, 0, 2, True, 2, 4, None, None),             # nd = 1: lane 0 is the timestep's, perturbations in lanes 1, 2; lane < m never
    "subspace-abs2": (17, 17, 2, 2, True, 3, 6, ("unitary", [0, 1, 3, 4], "abs2"), "given"),      # the fidelity's seed on a subspace, squared form
}
_BUILT = {}


def case(qc, name):
    """The case dictionary test_sweep.make_sweep, test_sweep_param_grad.reference and test_sweep_vjp.check_case read.  Sample 0 has
    theta = 0."""
    if name in _BUILT:
        return _BUILT[name]
    N, nc, m, p, free, S, T, fid, sc = CASES[name]
    kind, subspace, form = fid if isinstance(fid, tuple) else (fid, None, "abs")
    rng = np.random.default_rng(640 + sum(map(ord, name)))
    H0 = _herm(rng, N)
    Hd = [_herm(rng, N, (N * max(m, 1)) ** -0.5) for _ in range(m)]
    perts = [_herm(rng, N) for _ in range(p)]
    goal = None
    if kind == "unitary":
        init, goal = ref.operator_to_iso_vec(_unitary(rng, N)), ref.operator_to_iso_vec(_unitary(rng, N))
    else:
        K = rng.standard_normal((N, nc)) + 1j * rng.standard_normal((N, nc))
        init = ref.operator_to_iso_vec(K / np.linalg.norm(K, axis=0))
        if kind == "ket":
            gk = rng.standard_normal(N) + 1j * rng.standard_normal(N)
            gk /= np.linalg.norm(gk)
            goal = np.concatenate([gk.real, gk.imag])
    theta = rng.uniform(-0.3, 0.3, (S, p))
    theta[0] = 0.0
    scale = None if sc is None else rng.uniform(0.9, 1.1, (S, m))
    if isinstance(sc, tuple):
        scale[sc] = 0.0
    c = dict(name=("" if kind is None else "w64par/") + name, L=N, N=N, n=2 * N, m=m, p=p, S=S, T=T,
             system=qc.QuantumSystem(H0, Hd) if qc is not None else None, perts=perts, G0=ref.iso_generator(H0),
             Gd=[ref.iso_generator(H) for H in Hd], Gp=[ref.iso_generator(P) for P in perts], init=init, cols=nc, goal=goal, kind=kind,
             subspace=subspace, form=form, controls=rng.uniform(-1, 1, (m, T)), dts=rng.uniform(0.1, 0.3, T) if free else 0.2, theta=theta,
             scale=scale, samples=list(range(S)), zero=sc if isinstance(sc, tuple) else None)
    c["cot"] = tv.unit_cotangents(rng, S, init.size)
    _BUILT[name] = c
    return c


# ---------------------------------------------------------------------------------------------------------------------------------
#  CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_wide64_params_field_is_validated(qc):
    L = qc._lib
    val = lambda D: L.lib.qc_sweep_desc_validate(C.byref(D.d))
    today = t64._valid_today()
    assert len(today) == 33 and L.QC_SWEEP_WIDE_64_PARAMS == WP == 1 << 13
    for N in (20, 12, 2):
        for v in today:
            assert val(tw._wdesc(qc, v, N=N)) == L.QC_OK, (N, v)
            if v:
                for more in (W64, W64 | WG, W64 | WG | WP):          # every value valid today, and each of them with bits 0, 10, 11 | 8192
                    assert val(tw._wdesc(qc, v | more, N=N)) == L.QC_OK, (N, v | more)
                assert val(tw._wdesc(qc, v | WP, N=N)) == L.QC_ERR_INVALID, (N, v | WP)
                assert val(tw._wdesc(qc, v | W64 | WP, N=N)) == L.QC_ERR_INVALID, (N, v | W64 | WP)          # without bit 11
                assert val(tw._wdesc(qc, v | WG | WP, N=N)) == L.QC_ERR_INVALID, (N, v | WG | WP)            # without bit 10
        for bad in (8192, 8193, 8192 | 1025, 8192 | 2049, 4096 | 3073, (1 << 20) | 11265, 4096 | 11265, 512 | 11265, 11264):
            assert val(tw._wdesc(qc, bad, N=N)) == L.QC_ERR_INVALID, (N, bad)
            text = L.lib.qc_sweep_last_error(None).decode()
            assert text.startswith("qc_sweep: wide"), text
            for words in ("17, 19, 25 or 27", "QC_SWEEP_WIDE_TANGENT (16)", "QC_SWEEP_WIDE_NOISE (64)", "QC_SWEEP_WIDE_HESSIAN (256)",
                          "QC_SWEEP_WIDE_64 (1024)", "QC_SWEEP_WIDE_64_GRAD (2048)", "QC_SWEEP_WIDE_64_PARAMS (8192)"):
                assert words in text, (words, text)
    ok = C.c_int32(-1)
    assert L.lib.qc_sweep_desc_grad_supported(C.byref(tw._wdesc(qc, 8193, N=20).d), C.byref(ok)) == L.QC_ERR_INVALID
    assert L.lib.qc_sweep_desc_launch(C.byref(tw._wdesc(qc, 8192 | 1025, N=20).d), 5, None, None, None) == L.QC_ERR_INVALID


def test_wide64_params_launch_rule_and_scope_are_unchanged(qc):
    """`qc_sweep_desc_launch` and every `qc_sweep_desc_*_supported` query answer with the bit what they answer without it, text for text."""
    L = qc._lib

    def launch(n, m, S, T, wide):
        D = tw._wdesc(qc, wide, N=n // 2, m=m, T=T, cols=1)
        mf, ch, nch = C.c_int32(), C.c_int64(), C.c_int64()
        assert L.lib.qc_sweep_desc_launch(C.byref(D.d), S, C.byref(mf), C.byref(ch), C.byref(nch)) == L.QC_OK
        return bool(mf.value), ch.value, nch.value

    for n in (16, 24, 32, 34, 54, 64):
        for m in (1, 8, 16, 17):
            for S, T in ((1, 2), (2, 102), (5, 12), (50, 26), (255, 5), (256, 3), (257, 5), (300, 3), (8192, 1000)):
                want = t64.launch64(n, m, S, T, 1 | W64)
                assert launch(n, m, S, T, WIDE) == launch(n, m, S, T, WIDE_G) == (want["mfma"], want["chunk"], want["n_chunks"]), (n, m, S, T)
    for name, spec in CASES.items():
        assert 32 < 2 * spec[0] <= 64 and t64.launch64(2 * spec[0], spec[2], spec[5], spec[6], WIDE)["mfma"], name
    f = t64.launch64(34, 2, 3, 26, WIDE)
    assert (f["chunk"], f["n_chunks"], f["last"]) == (5, 5, 5)
    f = t64.launch64(34, 2, 3, 12, WIDE)
    assert (f["chunk"], f["n_chunks"], f["last"]) == (3, 4, 2)
    f = t64.launch64(34, 2, 5, 3, WIDE)
    assert (f["chunk"], f["n_chunks"]) == (1, 2)
    Uk = L.QC_FID_UNITARY
    descs = [(dict(N=27, m=6, fid_kind=Uk), False, 0), (dict(N=17, m=2, cols=1, fid_kind=L.QC_FID_KET), False, 0), (dict(N=32, m=16, fid_kind=Uk), False, 0),
             (dict(N=20, m=2, cols=17), False, 0), (dict(N=17, m=2, cols=33), False, 0), (dict(N=27, m=17, fid_kind=Uk), False, 0),
             (dict(N=27, m=6, fid_kind=Uk), False, 1), (dict(N=25, m=2, cols=1, fid_kind=L.QC_FID_DENSITY), True, 0),
             (dict(N=12, m=2, fid_kind=Uk), False, 0), (dict(N=4, m=2, p=2, fid_kind=Uk), False, 0), (dict(N=12, m=2, fid_kind=Uk), False, 1)]
    for kw, lindblad, stored in descs:
        for low in (1, 3, 347):
            answers = [[t64._query(qc, which, _desc(qc, low | W64 | WG | bit, stored, lindblad, **kw)) for which in t64.QUERIES] for bit in (0, WP)]
            assert answers[0] == answers[1], (kw, lindblad, stored, low)
            assert all(rc == L.QC_OK for rc, _, _ in answers[0])
    for which in ("grad", "vjp"):
        assert t64._query(qc, which, _desc(qc, WIDE, N=27, m=6, p=3, fid_kind=Uk)) == (L.QC_OK, 1, None)


def _desc(qc, wide, stored=0, lindblad=False, **kw):
    D = tg._GDesc(qc, **kw)
    if lindblad:
        D.G0[:] = np.random.default_rng(0).standard_normal(D.G0.size)
    D.d.wide = wide
    D.d.reserved1[0] = stored
    return D


def test_wide64_params_keywords_constants_and_texts(qc):
    L = qc._lib
    for f in (qc.RolloutSweep.__init__, qc.SweepInfidelityObjective.__init__, qc.SweepFinalStateObjective.__init__,
              qc.rollout_sweep_parameter_gradient):
        p = inspect.signature(f).parameters
        assert list(p)[-1] == "wide64_params" and p["wide64_params"].default is False, f
        assert p["wide64_grad"].default is False and p["wide64"].default is False, f
    assert "wide64_params" in qc.RolloutSweep.__doc__
    # refused before the library is touched: no system is looked at
    with pytest.raises(ValueError, match="wide64_params=True needs wide64_grad=True"):
        qc.RolloutSweep(None, [], 5, wide=True, wide64=True, wide64_params=True)
    with pytest.raises(ValueError, match="wide64_params=True needs wide64_grad=True"):
        qc.RolloutSweep(None, [], 5, wide64_params=True)
    with pytest.raises(ValueError, match="wide64_grad=True needs wide64=True"):
        qc.RolloutSweep(None, [], 5, wide=True, wide64_grad=True, wide64_params=True)
    header = open(os.path.join(ROOT, "include", "qcolloc.h")).read()
    assert "#define QC_SWEEP_WIDE_64_PARAMS 8192 " in header and L.lib.qc_abi_version() == 6
    assert L.lib.qc_sizeof_sweep_desc() == C.sizeof(L.qc_sweep_desc) == 128
    julia = open(os.path.join(ROOT, "julia", "QCollocHIP.jl"), encoding="utf-8").read()
    assert "const QC_SWEEP_WIDE_64_PARAMS = 8192" in julia and julia.count("wide64_params::Bool=false") == 2
    for fn in ("function rollout_sweep_parameter_gradient(", "function rollout_sweep_pullback("):
        body = julia[julia.index(fn):]
        assert "wide64_params::Bool=false" in body[:body.index("\nend\n")] and "QC_SWEEP_WIDE_64_PARAMS" in body[:body.index("\nend\n")], fn
    for doc in ("DESIGN.md", "README.md"):
        assert "QC_SWEEP_WIDE_64_PARAMS" in open(os.path.join(ROOT, doc), encoding="utf-8").read(), doc


def test_reference_routes_agree_at_17_levels():
    """Forward mode (expm_frechet) against central differences of the sweep reference on a closed 17-level system: 1e-6 relative.  The
    yardstick of this file at its own size."""
    N, m, p, T, S = 17, 2, 2, 5, 2
    rng = np.random.default_rng(1764)
    G0, Gd = ref.iso_generator(_herm(rng, N)), [ref.iso_generator(_herm(rng, N, 0.4)) for _ in range(m)]
    Gp = [ref.iso_generator(_herm(rng, N)) for _ in range(p)]
    controls, dts = rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T)
    theta, scale = rng.uniform(-0.3, 0.3, (S, p)), rng.uniform(0.9, 1.1, (S, m))
    init, goal = ref.operator_to_iso_vec(_unitary(rng, N)), ref.operator_to_iso_vec(_unitary(rng, N))
    args = (G0, Gd, Gp, controls, dts, init, theta, scale, [0, 1], "unitary", goal, N, None, "abs")
    (terms, a), b = pref.param_terms_forward(*args), pref.param_grad_fd(*args)
    assert terms.shape == (S, T - 1, p + m) and a.shape == b.shape == (S, p + m)
    err = np.abs(a - b).max() / max(1.0, np.abs(a).max())
    print(f"SWEEP-WIDE64-PARAM reference at N = 17: forward mode vs central differences {err:.2e} (bound 1e-6), max |g| {np.abs(a).max():.3f}")
    assert err < 1e-6 and np.abs(a).max() > 1e-3


# ---------------------------------------------------------------------------------------------------------------------------------
#  GPU: values
# ---------------------------------------------------------------------------------------------------------------------------------
def _check_fidelity_case(qc, c, sw):
    """`param_grad` against the forward-mode reference at every sample; the fidelities carry the bits of `eval`."""
    Z = sw.pack(c["controls"], c["dts"])
    fids, gth, gsc = sw.param_grad(Z, c["init"], c["theta"], c["scale"])
    assert fids.shape == (c["S"],) and gth.shape == (c["S"], c["p"]) and gsc.shape == (c["S"], c["m"])
    tp._assert_params(gth, gsc, c, c["name"])
    np.testing.assert_array_equal(fids, sw.eval(Z, c["init"], c["theta"], c["scale"], finals=False)[1])
    return Z, fids, gth, gsc


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_wide64_param_grad_matches_the_reference(qc, name):
    c = case(qc, name)
    want = t64.launch64(c["n"], c["m"], c["S"], c["T"], WIDE)
    sw = ts.make_sweep(qc, c, **HANDLE)
    try:
        assert sw.kernel_name == "mfma64-sweep" and sw.wide64_params and sw.wide64_grad and sw._desc.wide == WIDE and sw.vjp_supported
        assert sw.launch(c["S"]) == (True, want["chunk"], want["n_chunks"])
        if name.startswith("chunks"):
            assert sw.launch(c["S"])[2] > 1
        if name == "one-interval-chunks":
            assert (want["chunk"], want["n_chunks"]) == (1, 2)
        if name == "many-drives":
            assert sw.n_deriv + sw.p == 25
        if name == "ket":
            assert sw.p == qc._lib.QC_MAX_PERT == 8
        if name == "no-drives-free-dt":
            assert (sw.m, sw.n_deriv, sw.p) == (0, 1, 2)
        if name == "subspace-abs2":
            assert (c["subspace"], c["form"]) == ([0, 1, 3, 4], "abs2")
        if c["kind"] is not None:
            assert sw.grad_supported
            Z, fids, gth, gsc = _check_fidelity_case(qc, c, sw)
            if name == "subspace-abs2":        # |tr|^2 / 16 of a 4-level block of a random 17-level unitary is small: still 10^6 bounds
                assert np.abs(gth).max() > 1e-3 and np.abs(gsc).max() > 1e-3
        else:
            assert not sw.grad_supported and "no fidelity" in sw.grad_unsupported_reason
            out = tv.check_case(sw, c, form=FORM, params=True)
            gth, gsc = out["grad_theta"], out.get("grad_scale")
            assert np.abs(gth).max() > 1e-3
        if c["zero"] is not None:          # an exact zero in `scale`: the derivative there is defined and not zero
            assert c["scale"][c["zero"]] == 0.0 and np.isfinite(gsc).all() and abs(gsc[c["zero"]]) > 1e-6, gsc[c["zero"]]
        assert np.all(c["theta"][0] == 0.0) and np.isfinite(gth).all()
        if name == "no-drives":            # grad_scale on a handle without drives: QC_ERR_INVALID, as in the smaller forms
            L = qc._lib
            assert sw.n_deriv == 0 and sw.m == 0
            Z = sw.pack(c["controls"], c["dts"])
            x = np.zeros(c["S"])
            rc = L.lib.qc_sweep_vjp(sw._h, L.dptr(Z), L.dptr(np.ascontiguousarray(c["init"])), c["S"], L.dptr(np.ascontiguousarray(c["theta"])), None,
                                    L.dptr(np.ascontiguousarray(c["cot"])), None, None, None, None, None, L.dptr(x))
            msg = L.lib.qc_sweep_last_error(sw._h)
            assert rc == L.QC_ERR_INVALID and b"grad_scale" in msg and b"m = 0" in msg
    finally:
        sw.close()


@pytest.mark.gpu
def test_wide64_param_grad_through_the_squarings(qc):
    """test_sweep_wide.squaring_cases at N = 17 for the systems whose first sample squares 0, 3 and 5 times: the samples of one call differ
    (up to 7), and the strong theta that makes them differ is the very parameter being differentiated."""
    seen = set()
    for k, per_sample, c in tw.squaring_cases(qc, N=17, m=2, T=12):
        if k not in (0, 3, 5):
            continue
        seen |= set(per_sample)
        c = dict(c, name="w64par/N17 " + c["name"], p=1)
        sw = ts.make_sweep(qc, c, **HANDLE)
        try:
            assert sw.kernel_name == "mfma64-sweep" and sw.launch(c["S"])[1:] == (3, 4)
            _check_fidelity_case(qc, c, sw)
        finally:
            sw.close()
    assert {0, 3, 7} <= seen


# ---------------------------------------------------------------------------------------------------------------------------------
#  GPU: identity and bits
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["pad", "full"])
def test_wide64_param_grad_euler_identity_on_device_outputs(qc, name):
    """Between the outputs of ONE call, within 1e-12 max(1, A_s): c[s, k] grad_scale[s, k] = sum_t a_{t,k} grad_samples[s, t, k]."""
    c = case(qc, name)
    sw = ts.make_sweep(qc, c, **HANDLE)
    try:
        o = tp._raw(qc, sw, sw.pack(c["controls"], c["dts"]), c["init"], c["theta"], c["scale"])
    finally:
        sw.close()
    m, T = c["m"], c["T"]
    bound = tp.ID_RTOL * np.maximum(1.0, tp.magnitudes(tp.reference(c)[0]))[:, None]
    lhs = c["scale"] * o["gsc"]
    rhs = np.einsum("kt,stk->sk", c["controls"][:, :T - 1], o["gs"][:, :, :m])
    euler = (np.abs(lhs - rhs) / bound).max()
    print(f"SWEEP-WIDE64-PARAM {name}: Euler identity, worst |difference| / bound = {euler:.4f}")
    assert euler <= 1.0 and np.abs(rhs).max() > 1e-4      # eight orders above the bound: the identity is not 0 = 0
    assert lhs[c["zero"]] == 0.0 and abs(rhs[c["zero"]]) <= bound[c["zero"][0], 0]


def _bits_setup(qc, T):
    rng = np.random.default_rng(88)
    N, m, p = 17, 2, 2
    sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, (N * m) ** -0.5) for _ in range(m)])
    perts = [_herm(rng, N) for _ in range(p)]
    goal = ref.operator_to_iso_vec(_unitary(rng, N))
    mk = lambda **kw: qc.RolloutSweep(sys_, perts, T, goal=goal, fid_kind="unitary", subspace=[0, 1, 3, 4], **kw)
    controls, dts = rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T)
    return rng, m, p, mk, controls, dts, ref.operator_to_iso_vec(_unitary(rng, N))


@pytest.mark.gpu
def test_wide64_param_grad_bits_across_outputs_and_flavours(qc):
    """fids, J, grad and grad_samples of the parameter flavour carry the bits of `grad` on the same handle and on a handle made without
    the bit; grad_theta / grad_scale do not depend on which other outputs are requested -- the calls without a per-interval output take
    the walk's gs = NULL path --, the device entry with dgrad_theta alone included; repeated calls return the same bits.  Several chunks
    (S = 5: chunks of 4, 4, 4, 1) and one (S = 256)."""
    rng, m, p, mk, controls, dts, init = _bits_setup(qc, T=14)
    sw, plain = mk(**HANDLE), mk(**HANDLE_G)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    try:
        assert sw.kernel_name == plain.kernel_name == "mfma64-sweep" and sw.wide64_params and not plain.wide64_params
        Z = sw.pack(controls, dts)
        for S in (5, 256):
            theta, scale, w = rng.uniform(-0.3, 0.3, (S, p)), rng.uniform(0.9, 1.1, (S, m)), rng.uniform(0.5, 1.5, S)
            assert sw.launch(S)[2] == (1 if S == 256 else 4)
            full = tp._raw(qc, sw, Z, init, theta, scale, w)
            assert np.isfinite(full["gth"]).all() and np.abs(full["gth"]).max() > 1e-3 and np.abs(full["gsc"]).max() > 1e-3
            for _ in range(3):
                again = tp._raw(qc, sw, Z, init, theta, scale, w)
                assert again["J"] == full["J"]
                for k in ("fids", "grad", "gs", "gth", "gsc"):
                    np.testing.assert_array_equal(again[k], full[k], err_msg=k)
            for want in (("gth", "gsc"), ("gth",), ("gsc",), ("fids", "gsc"), ("grad", "gth"), ("gs", "gth", "gsc")):
                part = tp._raw(qc, sw, Z, init, theta, scale, w, want=want)
                for k in want:
                    np.testing.assert_array_equal(part[k], full[k], err_msg=f"{k} of {want}")
            only = torch.full((S, p), -7.0, dtype=torch.float64, device=dev)
            sw.param_grad_device(t(Z), t(init), S, t(theta), t(scale), dgrad_theta=only)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(only.cpu().numpy(), full["gth"])
            Jc, fc, gc, gthc, gscc = sw.param_grad(Z, init, theta, scale, weights=w, with_controls=True)
            assert Jc == full["J"] and np.array_equal(gc, full["grad"]) and np.array_equal(gthc, full["gth"]) and np.array_equal(gscc, full["gsc"])
            for h in (sw, plain):
                J, f, g, gs = h.grad(Z, init, theta, scale, weights=w, per_sample=True)
                assert J == full["J"]
                for a, k in ((f, "fids"), (g, "grad"), (gs, "gs")):
                    np.testing.assert_array_equal(a, full[k], err_msg=k)
            # the pullback: parameter cotangents with and without the per-interval outputs, host and device
            cot = tv.unit_cotangents(rng, S, sw.ns)
            c = dict(S=S, init=init, theta=theta, scale=scale, cot=cot)
            allv = tv.device_call(sw, Z, c, ["grad", "grad_samples", "grad_init", "grad_theta", "grad_scale"])
            for want in (["grad_theta", "grad_scale"], ["grad_theta"], ["grad_scale"], ["grad_init", "grad_scale"], ["grad", "grad_theta"]):
                part = tv.device_call(sw, Z, c, want)
                for k in want:
                    np.testing.assert_array_equal(part[k], allv[k], err_msg=f"vjp {k} of {want}")
            host = sw.vjp(Z, init, cot, theta, scale, per_sample=True, init_grad=True, params=True)
            for a, k in zip(host, ("grad", "grad_samples", "grad_init", "grad_theta", "grad_scale")):
                np.testing.assert_array_equal(a, allv[k], err_msg="host vjp " + k)
            other = tv.device_call(plain, Z, c, ["grad", "grad_samples", "grad_init"])
            for k, v in other.items():
                np.testing.assert_array_equal(v, allv[k], err_msg="vjp without the bit: " + k)
        print("SWEEP-WIDE64-PARAM bits: outputs of param_grad vs grad, any subset of outputs, repeats, host / device identical (bound: 0 differing bits)")
    finally:
        sw.close()
        plain.close()


@pytest.mark.gpu
def test_wide64_param_grad_bits_host_device_side_stream_and_scratch(qc):
    """The host and device entry points return identical bits on a side stream; one handle at S = 3 (six chunks: five of 5 and one of
    1), then 100 (three chunks), then 7 returns the bits of fresh handles: dPart and the other scratch are grown on demand and reused at
    another n_chunks."""
    rng, m, p, mk, controls, dts, init = _bits_setup(qc, T=27)
    sw = mk(**HANDLE)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    new = lambda *shape: torch.full(shape, -7.0, dtype=torch.float64, device=dev)
    side = torch.cuda.Stream(device=dev)
    try:
        Z = sw.pack(controls, dts)
        assert [sw.launch(S)[1:] for S in (3, 100, 7)] == [(5, 6), (9, 3), (5, 6)]
        for S in (3, 100, 7):
            theta, scale, w = rng.uniform(-0.3, 0.3, (S, p)), rng.uniform(0.9, 1.1, (S, m)), rng.uniform(0.5, 1.5, S)
            fresh = mk(**HANDLE)
            first = tp._raw(qc, fresh, Z, init, theta, scale, w)
            fresh.close()
            got = tp._raw(qc, sw, Z, init, theta, scale, w)
            assert got["J"] == first["J"]
            for k in ("fids", "grad", "gs", "gth", "gsc"):
                np.testing.assert_array_equal(got[k], first[k], err_msg=f"S = {S}: {k}")
            dfid, dJ, dg, dgs, dgth, dgsc = new(S), new(1), new(sw.Z_len), new(S, sw.T - 1, sw.n_deriv), new(S, p), new(S, m)
            args = (t(Z), t(init), S, t(theta), t(scale), t(w))
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                sw.param_grad_device(*args, dfid, dJ, dg, dgs, dgth, dgsc, stream=side)
            side.synchronize()
            assert dJ.item() == first["J"]
            for a, k in ((dfid, "fids"), (dg, "grad"), (dgs, "gs"), (dgth, "gth"), (dgsc, "gsc")):
                np.testing.assert_array_equal(a.cpu().numpy(), first[k], err_msg=f"S = {S}: device {k}")
            cot = tv.unit_cotangents(rng, S, sw.ns)
            c = dict(S=S, init=init, theta=theta, scale=scale, cot=cot)
            with torch.cuda.stream(side):
                out = tv.device_call(sw, Z, c, ["grad_theta", "grad_scale"], stream=side)
            host = sw.vjp(Z, init, cot, theta, scale, params=True)
            np.testing.assert_array_equal(out["grad_theta"], host[1])
            np.testing.assert_array_equal(out["grad_scale"], host[2])
        print("SWEEP-WIDE64-PARAM bits: host / device / side stream and S = 3 -> 100 -> 7 identical (bound: 0 differing bits)")
    finally:
        sw.close()


# ---------------------------------------------------------------------------------------------------------------------------------
#  GPU: pullback and autograd
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cols", [1, 8, 17])
def test_wide64_vjp_parameter_cotangents(qc, cols):
    """test_sweep_vjp.check_case with `params` at 1, 8 and 17 state columns (one column tile, one, two with a single live column):
    grad_theta and grad_scale against `pullback_forward` beside every other output; grad, grad_samples, grad_init and finals carry the
    bits of the same call on a handle made without the bit."""
    rng = np.random.default_rng(170 + cols)
    N, m, p, S, T = 17, 2, 2, 3, 5
    H0, Hd, perts = _herm(rng, N), [_herm(rng, N, (N * m) ** -0.5) for _ in range(m)], [_herm(rng, N) for _ in range(p)]
    K = rng.standard_normal((N, cols)) + 1j * rng.standard_normal((N, cols))
    init = ref.operator_to_iso_vec(K / np.linalg.norm(K, axis=0))
    c = dict(name=f"cols{cols}", L=N, m=m, p=p, S=S, T=T, system=qc.QuantumSystem(H0, Hd), perts=perts, G0=ref.iso_generator(H0),
             Gd=[ref.iso_generator(H) for H in Hd], Gp=[ref.iso_generator(P) for P in perts], init=init, cols=cols, goal=None, kind=None,
             subspace=None, form="abs", controls=rng.uniform(-1, 1, (m, T)), dts=rng.uniform(0.1, 0.3, T), theta=rng.uniform(-0.3, 0.3, (S, p)),
             scale=rng.uniform(0.9, 1.1, (S, m)), samples=list(range(S)), cot=tv.unit_cotangents(rng, S, init.size))
    sw, plain = ts.make_sweep(qc, c, **HANDLE), ts.make_sweep(qc, c, **HANDLE_G)
    try:
        assert sw.kernel_name == "mfma64-sweep" and sw.vjp_supported and sw.cols == cols
        out = tv.check_case(sw, c, form=FORM, params=True)
        assert np.abs(out["grad_theta"]).max() > 1e-3 and np.abs(out["grad_scale"]).max() > 1e-3
        keys = ["finals", "grad", "grad_samples", "grad_init"]
        other = tv.device_call(plain, plain.pack(c["controls"], c["dts"]), c, keys)
        for k in keys:
            np.testing.assert_array_equal(out[k], other[k], err_msg=k)
    finally:
        sw.close()
        plain.close()


@pytest.mark.gpu
def test_wide64_vjp_consistent_with_param_grad(qc):
    """With C_s = dF_s/dx formed on the host the pullback's parameter outputs are `param_grad`'s, to the 1e-12 rule (not bit for bit: the
    host forms the seed in another order)."""
    c = case(qc, "pad")
    sw = ts.make_sweep(qc, c, **HANDLE)
    try:
        Z = sw.pack(c["controls"], c["dts"])
        finals = sw.eval(Z, c["init"], c["theta"], c["scale"], fids=False)[0]
        cot = np.stack([tv.fidelity_seed(finals[:, s], c) for s in range(c["S"])])
        _, gth, gsc = sw.vjp(Z, c["init"], cot, c["theta"], c["scale"], params=True)
        _, wth, wsc = sw.param_grad(Z, c["init"], c["theta"], c["scale"])
    finally:
        sw.close()
    bound = tp.ID_RTOL * np.maximum(1.0, tp.magnitudes(tp.reference(c)[0]))[:, None]
    worst = max((np.abs(gth - wth) / bound).max(), (np.abs(gsc - wsc) / bound).max())
    print(f"SWEEP-WIDE64-PARAM pad: pullback of the fidelity's differential vs param_grad, worst |difference| / bound = {worst:.4f}")
    assert worst <= 1.0 and np.abs(wth).max() > 1e-3 and np.abs(wsc).max() > 1e-3


@pytest.mark.gpu
def test_wide64_finals_autograd_theta_and_scale(qc):
    """One backward pass of a torch loss on `finals_autograd` with theta and scale requiring grad against central differences of the
    forward sweep (the step and tolerance of test_sweep_wide64_grad.test_wide64_finals_autograd_backward: eps 1e-6, atol 1e-6), and
    against the tensors of a direct `vjp_device` call, bit for bit."""
    rng = np.random.default_rng(32)
    N, m, p, T, S = 17, 2, 2, 3, 2
    sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, 0.3) for _ in range(m)])
    sw = qc.RolloutSweep(sys_, [_herm(rng, N) for _ in range(p)], T, cols=2, **HANDLE)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    try:
        Z = t(sw.pack(rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T)))
        init, Wt = t(rng.standard_normal(sw.ns)), t(rng.standard_normal((S, sw.ns)))
        th0, sc0 = rng.uniform(-0.3, 0.3, (S, p)), rng.uniform(0.9, 1.1, (S, m))
        sc0[1, 0] = 0.0

        def loss(th_, sc_):
            X = sw.finals_autograd(Z, init, th_, sc_)
            return (X * Wt).sum() + 0.5 * (X ** 2 * Wt).sum()

        th, sc = t(th0).requires_grad_(True), t(sc0).requires_grad_(True)
        loss(th, sc).backward()
        got = np.concatenate([th.grad.cpu().numpy().ravel(), sc.grad.cpu().numpy().ravel()])
        x0, eps = np.concatenate([th0.ravel(), sc0.ravel()]), 1e-6
        split = lambda x: (t(x[:S * p].reshape(S, p)), t(x[S * p:].reshape(S, m)))
        fd = np.zeros(x0.size)
        with torch.no_grad():
            for i in range(x0.size):
                e = np.zeros(x0.size)
                e[i] = eps
                fd[i] = (loss(*split(x0 + e)).item() - loss(*split(x0 - e)).item()) / (2 * eps)
        print(f"SWEEP-WIDE64-PARAM finals_autograd: max |backward - central differences| = {np.abs(got - fd).max():.3e} (bound 1e-6)")
        np.testing.assert_allclose(got, fd, rtol=0, atol=1e-6)
        assert np.abs(fd).max() > 1e-2 and abs(sc.grad[1, 0].item()) > 1e-4
        X = sw.finals_autograd(Z, init, t(th0), t(sc0)).detach()
        want = tv.device_call(sw, Z.cpu().numpy(), dict(S=S, init=init.cpu().numpy(), theta=th0, scale=sc0, cot=(Wt + X * Wt).cpu().numpy()),
                              ["grad_theta", "grad_scale"])
        np.testing.assert_array_equal(th.grad.cpu().numpy(), want["grad_theta"])
        np.testing.assert_array_equal(sc.grad.cpu().numpy(), want["grad_scale"])
    finally:
        sw.close()


# ---------------------------------------------------------------------------------------------------------------------------------
#  GPU: every sample on both sides of the fill constant
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_wide64_param_grad_every_sample_around_the_fill_constant(qc):
    """N = 17, one column, m = p = 1, T = 3 at S = 255 (two chunks of one interval a sample), 256 and 257 (one chunk) on one handle, every
    sample against the reference: the item <-> (sample, chunk) index of the share's store where n_chunks changes.  The samples of the three
    calls are prefixes of one set, so one reference serves them."""
    S_max, T = 257, 3
    rng = np.random.default_rng(255)
    N, m, p = 17, 1, 1
    H0, Hd, P = _herm(rng, N), [_herm(rng, N, N ** -0.5)], _herm(rng, N)
    K = rng.standard_normal((N, 1)) + 1j * rng.standard_normal((N, 1))
    gk = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    gk /= np.linalg.norm(gk)
    c = dict(name="w64par/fill", L=N, m=m, p=p, S=S_max, T=T, system=qc.QuantumSystem(H0, Hd), perts=[P], G0=ref.iso_generator(H0),
             Gd=[ref.iso_generator(Hd[0])], Gp=[ref.iso_generator(P)], init=ref.operator_to_iso_vec(K / np.linalg.norm(K)), cols=1,
             goal=np.concatenate([gk.real, gk.imag]), kind="ket", subspace=None, form="abs", controls=rng.uniform(-1, 1, (m, T)),
             dts=rng.uniform(0.1, 0.3, T), theta=rng.uniform(-0.3, 0.3, (S_max, p)), scale=rng.uniform(0.9, 1.1, (S_max, m)),
             samples=list(range(S_max)))
    terms, sums = tp.reference(c)
    sw = ts.make_sweep(qc, c, **HANDLE)
    try:
        Z = sw.pack(c["controls"], c["dts"])
        assert [sw.launch(S)[2] for S in (255, 256, 257)] == [2, 1, 1]
        for S in (255, 256, 257):
            fids, gth, gsc = sw.param_grad(Z, c["init"], c["theta"][:S], c["scale"][:S])
            got = np.concatenate([gth, gsc], axis=1)
            bound = tp.PAR_RTOL * np.maximum(1.0, tp.magnitudes(terms[:S]))
            ratio = (np.abs(got - sums[:S]).max(axis=1) / bound).max()
            print(f"SWEEP-WIDE64-PARAM fill S = {S}: worst |d g| / bound = {ratio:.4f} over {S} samples")
            assert ratio <= 1.0 and not np.isnan(got).any(), S
            np.testing.assert_array_equal(fids, sw.eval(Z, c["init"], c["theta"][:S], c["scale"][:S], finals=False)[1])
        assert np.abs(sums).min(axis=0).max() > 0 and np.abs(sums).max() > 1e-3
    finally:
        sw.close()


# ---------------------------------------------------------------------------------------------------------------------------------
#  GPU: refusals, non-finite input, the example
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_wide64_params_refusals_on_live_handles(qc):
    L = qc._lib
    UNS = L.QC_ERR_UNSUPPORTED
    rng = np.random.default_rng(3)
    N, m, T, S = 20, 2, 6, 3
    sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, 0.3) for _ in range(m)])
    goal, P = ref.operator_to_iso_vec(_unitary(rng, N)), _herm(rng, N)
    init, theta = ref.operator_to_iso_vec(_unitary(rng, N)), rng.uniform(-0.3, 0.3, (S, 1))
    sw = qc.RolloutSweep(sys_, [P], T, goal=goal, fid_kind="unitary", **HANDLE)
    without = qc.RolloutSweep(sys_, [P], T, goal=goal, fid_kind="unitary", **HANDLE_G)
    try:
        Z = sw.pack(rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T))
        named = lambda e: e.value.code == UNS and "mfma64-sweep" in str(e.value) and "2N = 40" in str(e.value) and "rollout-per-sample" not in str(e.value)
        # a handle made without the bit: today's two texts, word for word
        with pytest.raises(qc.QCollocError) as e:
            without.param_grad(Z, init, theta)
        assert e.value.code == UNS and "qc_sweep gradients: parameter gradients are not served in the mfma64-sweep form (2N = 40)" in str(e.value)
        with pytest.raises(qc.QCollocError) as e:
            without.vjp(Z, init, np.zeros((S, sw.ns)), theta, params=True)
        assert e.value.code == UNS and "qc_sweep pullback: parameter cotangents are not served in the mfma64-sweep form (2N = 40)" in str(e.value)
        # with it both are served, and the other outputs carry the other handle's bits
        fids, gth, gsc = sw.param_grad(Z, init, theta)
        assert np.isfinite(gth).all() and np.isfinite(gsc).all() and np.abs(gth).max() > 1e-4
        np.testing.assert_array_equal(fids, without.grad(Z, init, theta)[1])
        for which, call in (("jvp", lambda: sw.jvp(Z, init, np.ones_like(Z), theta)),
                            ("hvp", lambda: sw.hvp(Z, init, np.zeros((S, sw.ns)), theta, vZ=np.ones_like(Z))),
                            ("noise", lambda: sw.noise_eval(Z, init, np.zeros((S, T - 1, 1))))):
            assert not getattr(sw, which + "_supported") and "mfma64-sweep" in getattr(sw, which + "_unsupported_reason")
            with pytest.raises(qc.QCollocError) as e:
                call()
            assert named(e), which
    finally:
        sw.close()
        without.close()
    stored = qc.RolloutSweep(sys_, [P], T, goal=goal, fid_kind="unitary", stored_states=True, **HANDLE)          # the stored-state flag
    try:
        assert not stored.grad_supported and not stored.vjp_supported
        with pytest.raises(qc.QCollocError) as e:
            stored.param_grad(Z, init, theta)
        assert e.value.code == UNS and "mfma64-sweep" in str(e.value) and "stored-state" in str(e.value)
        assert np.isfinite(stored.eval(Z, init, theta)[0]).all()
    finally:
        stored.close()


@pytest.mark.gpu
def test_wide64_param_grad_nan_in_one_sample(qc):
    """A NaN in one sample's theta does not raise: that sample's rows are non-finite, every other row carries the bits of the clean call."""
    rng = np.random.default_rng(10)
    N, m, T, S = 17, 2, 11, 5           # 4 chunks
    sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, 0.3) for _ in range(m)])
    goal, init = ref.operator_to_iso_vec(_unitary(rng, N)), ref.operator_to_iso_vec(_unitary(rng, N))
    sw = qc.RolloutSweep(sys_, [_herm(rng, N)], T, goal=goal, fid_kind="unitary", **HANDLE)
    try:
        assert sw.kernel_name == "mfma64-sweep" and sw.launch(S)[2] == 4
        Z = sw.pack(rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T))
        theta, scale = rng.uniform(-0.3, 0.3, (S, 1)), rng.uniform(0.9, 1.1, (S, m))
        good = sw.param_grad(Z, init, theta, scale)
        assert all(np.isfinite(a).all() for a in good)
        bad = theta.copy()
        bad[2, 0] = np.nan
        got = sw.param_grad(Z, init, bad, scale)
        others = [0, 1, 3, 4]
        for a, b in zip(got, good):
            assert not np.isfinite(a[2]).any()
            assert np.isfinite(a[others]).all()
            np.testing.assert_array_equal(a[others], b[others])
        for a, b in zip(sw.param_grad(Z, init, theta, scale), good):
            np.testing.assert_array_equal(a, b)
    finally:
        sw.close()


@pytest.mark.gpu
def test_wide64_free_function(qc):
    c = case(qc, "pad")
    fids, gth, gsc = qc.rollout_sweep_parameter_gradient(c["init"], c["controls"], c["dts"], c["system"], c["perts"], c["theta"], c["scale"],
                                                         goal=c["goal"], fid_kind="unitary", **HANDLE)
    tp._assert_params(gth, gsc, c, "pad through rollout_sweep_parameter_gradient")


@pytest.mark.gpu
def test_three_transmon_worst_case_example(qc):
    """The example's `main` at a small size: every ascent starts at a start point and never loses, so the worst infidelity found is the
    starts' worst or larger."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import three_transmon_worst_case as ex
        out = ex.main(T=6, starts=16, iters=2, verbose=False)
    finally:
        sys.path.pop(0)
    assert out["kernel"] == "mfma64-sweep" and out["starts"] == 16 and len(out["history"]) == 3
    assert 0.0 < out["start_worst"] < 1.0 and out["found_worst"] >= out["start_worst"]
    assert all(np.all(b >= a) for a, b in zip(out["history"], out["history"][1:]))
