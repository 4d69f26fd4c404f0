"""Parameter gradients and parameter cotangents on wide handles (`qc_sweep_desc.wide = QC_SWEEP_WIDE | QC_SWEEP_WIDE_PARAMS`,
`RolloutSweep(..., wide=True, wide_params=True)`): dF_s/dtheta[s, j] and dF_s/dc[s, k] in the "mfma32-sweep" form, from the parameter
flavour of the 2 x 2-tile walk (csrc/qc_sweep32_grad.hip, qc_sweep32_grad_kernel<true>).  CPU: the bit field's validation, constants and
ABI, the device-free queries with and without the bit, the constructor, the Julia text.  GPU: every value of grad_theta and grad_scale
against the forward-mode reference of tests/sweep_param_grad_reference.py (pullback: tests/sweep_vjp_reference.py), the squarings, the
Euler identity on device outputs, bits (against `grad`, against a handle made with `wide` alone, across requested outputs, repeats, entry
points, a growing handle), autograd, the refusals that stay, a NaN in one sample, the example.

Tolerances are test_sweep_param_grad.py's (read its header): per sample |got - want| <= 1e-9 max(1, A_s), A_s the largest sum over the
intervals of |term| among the sample's parameters; identities between outputs of one call to 1e-12 max(1, A_s); pullback outputs at the
rule of test_sweep_vjp.py.  A parameter derivative is a sum of bounded bilinear forms whatever the size of the matrices.
Measured worst ratios: profiles/sweep_wide_param_summary.txt.
Every sample of mid-size and filled launches (S = 301 .. 2049): tests/test_sweep_wide_params_every_sample.py."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import sweep_reference as ref
import test_sweep as ts
import test_sweep_grad as tg
import test_sweep_param_grad as tp
import test_sweep_vjp as tv
import test_sweep_vjp_wide as tvw
import test_sweep_wide as tw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_herm, _unitary = ts._herm, ts._unitary
U, USUB = ("unitary", None, "abs"), ("unitary", [0, 1, 3, 4], "abs")

# name: (state, levels, m, p, scale given, free timestep, S, T, fidelity, samples checked against the reference or None = all)
WIDE_PARAM_CASES = {
    "transmons9": ("unitary", 9, 2, 1, False, True, 5, 11, USUB, None),                                   # padded tiles; chunks of 3, 3, 3, 1
    "levels12-p2-fixed": ("unitary", 12, 3, 2, True, False, 3, 8, ("unitary", None, "abs2"), None),       # two perturbations, fixed timestep
    "levels16-8drives": ("unitary", 16, 8, 1, False, True, 3, 6, ("unitary", None, "abs2"), None),        # full tiles, all eight drive lanes
    "ket10": ("ket", 10, 2, 1, True, True, 11, 6, ("ket", None, "abs"), None),
    "one-interval": ("unitary", 9, 2, 1, False, True, 3, 2, U, None),                                     # T = 2
    "one-chunk": ("unitary", 9, 2, 1, True, True, 2048, 3, U, (0, 1000, 2047)),                           # n_chunks = 1
    "sqrt-capped": ("unitary", 9, 2, 1, False, True, 2, 102, USUB, None),                                 # 11 chunks of 10, the last of 1
}


def build(qc, name):
    """The case under a name of its own: tp.reference caches by name, and its own cases have a "one-chunk" and a "one-interval" too."""
    return tw.build(qc, "wide-par/" + name, WIDE_PARAM_CASES[name])


def make(qc, c, **kw):
    return ts.make_sweep(qc, c, wide=True, wide_params=True, **kw)


# ---------------------------------------------------------------------------------------------------------------------------------
#  CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_wide_is_a_bit_field(qc):
    L = qc._lib
    val = lambda D: L.lib.qc_sweep_desc_validate(C.byref(D.d))
    for N in (12, 2):
        for good in (0, 1, 3):
            assert val(tw._wdesc(qc, good, N=N)) == L.QC_OK, (N, good)
        for bad in (2, 5, 7, -1, (1 << 20) | 1):
            assert val(tw._wdesc(qc, bad, N=N)) == L.QC_ERR_INVALID, (N, bad)
            assert L.lib.qc_sweep_last_error(None).decode().startswith("qc_sweep: wide"), (N, bad)


def test_constants_and_abi(qc, tmp_path):
    L = qc._lib
    assert L.QC_SWEEP_WIDE == 1 and L.QC_SWEEP_WIDE_PARAMS == 2
    header = open(os.path.join(ROOT, "include", "qcolloc.h")).read()
    assert re.search(r"^#define QC_SWEEP_WIDE_PARAMS 2\b", header, re.M)
    assert L.lib.qc_abi_version() == 6
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "qcolloc.h"\nint main(){printf("%zu %d %d\\n", sizeof(qc_sweep_desc), QC_SWEEP_WIDE, '
                   'QC_SWEEP_WIDE_PARAMS);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(L.qc_sweep_desc), 1, 2] and L.lib.qc_sizeof_sweep_desc() == C.sizeof(L.qc_sweep_desc) == 128      # as before the bit


def test_device_free_queries_do_not_see_the_bit(qc):
    """`qc_sweep_desc_launch`, `qc_sweep_desc_grad_supported` and `qc_sweep_desc_vjp_supported` answer for wide = 3 what they answer for
    wide = 1, message for message."""
    L = qc._lib
    for n in (16, 18, 24, 32, 34):
        for m in (1, 8, 9):
            for S, T in ((1, 2), (2, 102), (5, 12), (11, 50), (300, 2), (2047, 50), (2048, 3), (8192, 1000)):
                got = []
                for wide in (1, 3):
                    D = tw._wdesc(qc, wide, N=n // 2, m=m, T=T, cols=1)
                    mf, ch, nch = C.c_int32(), C.c_int64(), C.c_int64()
                    assert L.lib.qc_sweep_desc_launch(C.byref(D.d), S, C.byref(mf), C.byref(ch), C.byref(nch)) == L.QC_OK
                    got.append((bool(mf.value), ch.value, nch.value))
                want = tw.wide_launch(n, m, S, T)
                assert got[0] == got[1] == (want["mfma"], want["chunk"], want["n_chunks"]), (n, m, S, T)

    def answers(fill=None, **kw):
        out = []
        for wide in (1, 3):
            D = tg._GDesc(qc, **kw)
            D.d.wide = wide
            if fill is not None:
                D.G0[:] = fill
            for fn in (L.lib.qc_sweep_desc_grad_supported, L.lib.qc_sweep_desc_vjp_supported):
                ok = C.c_int32(-1)
                rc = fn(C.byref(D.d), C.byref(ok))
                out.append((rc, ok.value, "" if ok.value else L.lib.qc_sweep_last_error(None).decode()))
        return out

    UN = L.QC_FID_UNITARY
    a = answers(N=9, m=2, fid_kind=UN, subspace=[0, 1, 3, 4])                # served, wide
    assert a[:2] == a[2:] and [x[:2] for x in a] == [(L.QC_OK, 1)] * 4
    a = answers(fill=np.random.default_rng(0).standard_normal(32 * 32), N=16, m=2, cols=1, fid_kind=L.QC_FID_DENSITY)      # a Lindblad generator
    assert a[:2] == a[2:] and all(x[:2] == (L.QC_OK, 0) and "antisymmetric" in x[2] for x in a)
    a = answers(N=12, m=9, fid_kind=UN)
    assert a[:2] == a[2:] and all(x[:2] == (L.QC_OK, 0) and "9 drives" in x[2] for x in a)
    a = answers(N=17, m=2, fid_kind=UN)
    assert a[:2] == a[2:] and all(x[:2] == (L.QC_OK, 0) and "2N = 34 > 32" in x[2] for x in a)
    a = answers(N=4, m=2, fid_kind=UN)                                       # harmless at 2N <= 16
    assert a[:2] == a[2:] and [x[:2] for x in a] == [(L.QC_OK, 1)] * 4
    a = answers(N=12, m=2)                                                   # no fidelity: the gradient refuses, the pullback serves
    assert a[:2] == a[2:] and a[0][:2] == (L.QC_OK, 0) and "no fidelity" in a[0][2] and a[1][:2] == (L.QC_OK, 1)


def test_constructor_and_keywords(qc):
    import inspect
    rng = np.random.default_rng(0)
    sys9 = qc.QuantumSystem(_herm(rng, 9), [_herm(rng, 9)])
    with pytest.raises(ValueError, match="wide_params"):          # before the library is touched: no device is needed to be told so
        qc.RolloutSweep(sys9, [_herm(rng, 9)], 5, wide_params=True)
    assert inspect.signature(qc.RolloutSweep.__init__).parameters["wide_params"].default is False
    assert inspect.signature(qc.rollout_sweep_parameter_gradient).parameters["wide"].default is False


def test_julia_text(qc):
    julia = open(os.path.join(ROOT, "julia", "QCollocHIP.jl"), encoding="utf-8").read()
    assert julia.count("stored_states::Bool=false") == 4 and "wide::Bool=false" in julia
    par = julia[julia.index("function rollout_sweep_parameter_gradient("):julia.index("function rollout_sweep_pullback(")]
    assert "wide::Bool=false" in par and "wide ? 3 : 0" in par
    pull = julia[julia.index("function rollout_sweep_pullback("):]
    pull = pull[:pull.index("\nend\n")]
    assert "wide::Bool=false" in pull and "wide_params::Bool=false" in pull and "(wide ? 1 : 0) | (wide_params ? 2 : 0)" in pull


# ---------------------------------------------------------------------------------------------------------------------------------
#  GPU: parity
# ---------------------------------------------------------------------------------------------------------------------------------
def _check_case(qc, c, sw=None, theta="case"):
    own = sw is None
    sw = make(qc, c) if own else sw
    try:
        assert sw.kernel_name == "mfma32-sweep" and sw.wide and sw.wide_params and sw.grad_supported
        Z = sw.pack(c["controls"], c["dts"])
        theta = c["theta"] if isinstance(theta, str) else theta
        fids, gth, gsc = sw.param_grad(Z, c["init"], theta, c["scale"])
        assert fids.shape == (c["S"],) and gth.shape == (c["S"], len(c["Gp"])) and gsc.shape == (c["S"], c["m"])
        tp._assert_params(gth, gsc, c, c["name"])
        np.testing.assert_array_equal(fids, sw.eval(Z, c["init"], theta, c["scale"], finals=False)[1])
        return Z, fids, gth, gsc
    finally:
        if own:
            sw.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(WIDE_PARAM_CASES))
def test_wide_param_grad_matches_the_reference(qc, name):
    c = build(qc, name)
    want = tw.wide_launch(c["n"], c["m"], c["S"], c["T"])
    assert want["mfma"] and 16 < c["n"] <= 32
    if name == "transmons9":
        assert (want["chunk"], want["n_chunks"], want["last"]) == (3, 4, 1)
    if name in ("one-chunk", "one-interval"):
        assert want["n_chunks"] == 1
    if name == "sqrt-capped":
        assert want["by_sqrt"] and (want["chunk"], want["n_chunks"], want["last"]) == (10, 11, 1)
    sw = make(qc, c)
    try:
        assert sw.launch(c["S"]) == (True, want["chunk"], want["n_chunks"])
        _check_case(qc, c, sw)
    finally:
        sw.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["no-perturbations", "no-perturbations-scale", "no-drives", "zeros-in-scale"])
def test_wide_param_grad_new_shapes(qc, shape):
    """test_sweep_param_grad.test_param_grad_new_shapes at 9 levels: no perturbation at all, m = 0 with a fixed timestep (the control
    gradient launches no walk there, this call must), exact zeros in `scale`."""
    L = qc._lib
    if shape.startswith("no-perturbations"):
        c = tp.custom(qc, "wide-par/" + shape, N=9, m=2, p=0, T=7, S=5, free=True, use_scale=shape.endswith("scale"), seed=143)
        if c["scale"] is None:
            c["theta"] = np.zeros((c["S"], 0))
    elif shape == "no-drives":
        c = tp.custom(qc, "wide-par/" + shape, N=9, m=0, p=2, T=7, S=5, free=False, use_scale=False, seed=141)
    else:
        c = tp.custom(qc, "wide-par/" + shape, N=9, m=2, p=1, T=9, S=6, free=True, use_scale=True, seed=144)
        c["scale"][1, 0] = c["scale"][3, 1] = 0.0
        c["scale"][4, :] = 0.0
    sw = make(qc, c)
    try:
        theta = c["theta"] if (c["p"] or c["scale"] is None) else None        # theta = None: `scale` gives the number of samples
        Z, fids, gth, gsc = _check_case(qc, c, sw, theta=theta)
        if shape == "zeros-in-scale":
            assert np.all(np.isfinite(gsc)) and np.all(np.abs(gsc[4]) > 1e-6)      # defined and not zero where c = 0
        if shape == "no-drives":
            assert sw.n_deriv == 0
            J, f2, grad, gth2, gsc2 = sw.param_grad(Z, c["init"], theta, None, with_controls=True)
            np.testing.assert_array_equal(gth2, gth)
            assert np.array_equal(grad.view(np.uint64), np.zeros(grad.size, dtype=np.uint64)) and abs(J - f2.mean()) <= 1e-14
        if shape.startswith("no-perturbations"):
            x, f = np.zeros(c["S"]), np.zeros(c["S"])
            sc = None if c["scale"] is None else L.dptr(np.ascontiguousarray(c["scale"]))
            rc = L.lib.qc_sweep_grad_params(sw._h, L.dptr(Z), L.dptr(np.ascontiguousarray(c["init"])), c["S"], None, sc, None, L.dptr(f), None, None,
                                            None, L.dptr(x), None)
            msg = L.lib.qc_sweep_last_error(sw._h)
            assert rc == L.QC_ERR_INVALID and b"grad_theta" in msg and b"n_pert = 0" in msg
    finally:
        sw.close()


@pytest.mark.gpu
def test_wide_param_grad_through_the_squarings(qc):
    """test_sweep_wide.squaring_cases: 0 .. 6 squarings and above, different per sample within one call; the strong theta that makes them
    differ is the very parameter being differentiated."""
    seen = set()
    for k, per_sample, c in tw.squaring_cases(qc):
        seen |= set(per_sample)
        c = dict(c, name="wide-par/" + c["name"])
        sw = qc.RolloutSweep(c["system"], c["perts"], c["T"], goal=c["goal"], fid_kind="unitary", dt_fixed=c["dts"], wide=True, wide_params=True)
        try:
            _check_case(qc, c, sw)
        finally:
            sw.close()
    assert set(range(7)) <= seen


# ---------------------------------------------------------------------------------------------------------------------------------
#  GPU: identity and bits
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["transmons9", "levels12-p2-fixed", "levels16-8drives"])
def test_wide_param_grad_euler_identity_on_device_outputs(qc, name):
    """Between the outputs of ONE call, within 1e-12 max(1, A_s): c[s, k] grad_scale[s, k] = sum_t a_{t,k} grad_samples[s, t, k]."""
    c = build(qc, name)
    sw = make(qc, c)
    try:
        o = tp._raw(qc, sw, sw.pack(c["controls"], c["dts"]), c["init"], c["theta"], c["scale"])
    finally:
        sw.close()
    m, T = c["m"], c["T"]
    bound = tp.ID_RTOL * np.maximum(1.0, tp.magnitudes(tp.reference(c)[0]))[:, None]
    scale = np.ones((c["S"], m)) if c["scale"] is None else c["scale"]
    lhs = scale * o["gsc"]
    rhs = np.einsum("kt,stk->sk", c["controls"][:, :T - 1], o["gs"][:, :, :m])
    euler = (np.abs(lhs - rhs) / bound).max()
    print(f"SWEEP-WIDE-PARAM {name}: Euler identity, worst |difference| / bound = {euler:.4f}")
    assert euler <= 1.0 and np.abs(rhs).max() > 1e-4      # eight orders above the bound: the identity is not 0 = 0


def _bits_setup(qc, T=20):
    rng = np.random.default_rng(8)
    N, m, p = 9, 2, 2
    sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, (N * m) ** -0.5) for _ in range(m)])
    perts = [_herm(rng, N) for _ in range(p)]
    goal = ref.operator_to_iso_vec(_unitary(rng, N))
    mk = lambda **kw: qc.RolloutSweep(sys_, perts, T, goal=goal, fid_kind="unitary", subspace=[0, 1, 3, 4], wide=True, **kw)
    controls, dts = rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T)
    return rng, m, p, mk, controls, dts, ref.operator_to_iso_vec(_unitary(rng, N))


@pytest.mark.gpu
def test_wide_param_grad_bits_across_outputs_and_flavours(qc):
    """fids, J, grad and grad_samples of the parameter flavour carry the bits of `grad` on the same handle and on a handle made with
    `wide` alone (the walk without the flavour); grad_theta / grad_scale do not depend on which other outputs are requested, the device
    entry with dgrad_theta alone included; six repeated calls return the same bits.  Several chunks (S = 5) and one (S = 2048)."""
    rng, m, p, mk, controls, dts, init = _bits_setup(qc, T=14)
    sw, plain = mk(wide_params=True), mk()
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    try:
        assert sw.kernel_name == plain.kernel_name == "mfma32-sweep" and sw.wide_params and not plain.wide_params
        Z = sw.pack(controls, dts)
        for S in (5, 2048):
            theta, scale, w = rng.uniform(-0.3, 0.3, (S, p)), rng.uniform(0.9, 1.1, (S, m)), rng.uniform(0.5, 1.5, S)
            assert (sw.launch(S)[2] == 1) == (S == 2048)
            full = tp._raw(qc, sw, Z, init, theta, scale, w)
            for _ in range(6):
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
                np.testing.assert_array_equal(h.eval(Z, init, theta, scale, finals=False)[1], full["fids"])
    finally:
        sw.close()
        plain.close()


@pytest.mark.gpu
def test_wide_param_grad_bits_host_device_side_stream_and_scratch(qc):
    """The host and device entry points return identical bits on a side stream; one handle at S = 3, then 150, then 7 returns the bits
    of fresh handles (dPart and the other scratch are grown on demand and reused at a smaller stride)."""
    rng, m, p, mk, controls, dts, init = _bits_setup(qc)
    sw = mk(wide_params=True)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    new = lambda *shape: torch.full(shape, -7.0, dtype=torch.float64, device=dev)
    side = torch.cuda.Stream(device=dev)
    try:
        Z = sw.pack(controls, dts)
        for S in (3, 150, 7):
            theta, scale, w = rng.uniform(-0.3, 0.3, (S, p)), rng.uniform(0.9, 1.1, (S, m)), rng.uniform(0.5, 1.5, S)
            fresh = mk(wide_params=True)
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
    finally:
        sw.close()


# ---------------------------------------------------------------------------------------------------------------------------------
#  GPU: pullback and autograd
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["transmons9", "kets3-levels10", "levels16-8drives"])
def test_wide_vjp_parameter_cotangents(qc, name):
    """test_sweep_vjp.check_case with `params` on a wide_params handle: grad_theta and grad_scale against the reference, beside every
    other output; grad, grad_samples, grad_init and finals carry the bits of the same call on a handle made with `wide` alone."""
    c = tv.build(qc, name, tvw.WIDE_VJP_CASES)
    sw, plain = make(qc, c), ts.make_sweep(qc, c, wide=True)
    try:
        assert sw.kernel_name == "mfma32-sweep" and sw.vjp_supported
        assert sw.grad_supported == (name != "kets3-levels10")
        out = tv.check_case(sw, c, form="32", params=True)
        assert "grad_theta" in out and "grad_scale" in out and np.abs(out["grad_theta"]).max() > 1e-3 and np.abs(out["grad_scale"]).max() > 1e-3
        keys = ["finals", "grad", "grad_samples", "grad_init"]
        other = tv.device_call(plain, plain.pack(c["controls"], c["dts"]), c, keys)
        for k in keys:
            np.testing.assert_array_equal(out[k], other[k], err_msg=k)
    finally:
        sw.close()
        plain.close()


@pytest.mark.gpu
def test_wide_vjp_consistent_with_param_grad(qc):
    """With C_s = dF_s/dx formed on the host the pullback's parameter outputs are `param_grad`'s, to the 1e-12 rule (not bit for bit: the
    host forms the seed in another order)."""
    c = build(qc, "transmons9")
    sw = make(qc, c)
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
    print(f"SWEEP-WIDE-PARAM transmons9: pullback of the fidelity's differential vs param_grad, worst |difference| / bound = {worst:.4f}")
    assert worst <= 1.0 and np.abs(wth).max() > 1e-3 and np.abs(wsc).max() > 1e-3


@pytest.mark.gpu
def test_wide_finals_autograd_theta_and_scale(qc):
    """A loss on `finals_autograd` with theta and scale requiring grad on a wide_params handle: the tensors of a direct `vjp_device` call."""
    c = build(qc, "levels12-p2-fixed")
    c["cot"] = tv.unit_cotangents(np.random.default_rng(5), c["S"], c["init"].size)
    sw = make(qc, c)
    dev = torch.device("cuda:0")
    t = lambda a, g=False: torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(g)
    try:
        Zh = sw.pack(c["controls"], c["dts"])
        Z, init, th, sc, W = t(Zh, True), t(c["init"], True), t(c["theta"], True), t(c["scale"], True), t(c["cot"])
        (sw.finals_autograd(Z, init, th, sc) * W).sum().backward()
        want = tv.device_call(sw, Zh, c, ["grad", "grad_init", "grad_theta", "grad_scale"])
        np.testing.assert_array_equal(Z.grad.cpu().numpy(), want["grad"])
        np.testing.assert_array_equal(init.grad.cpu().numpy(), t(want["grad_init"]).sum(0).cpu().numpy())
        np.testing.assert_array_equal(th.grad.cpu().numpy(), want["grad_theta"])
        np.testing.assert_array_equal(sc.grad.cpu().numpy(), want["grad_scale"])
        assert np.abs(want["grad_theta"]).max() > 1e-3 and np.abs(want["grad_scale"]).max() > 1e-3
        th2, sc2 = t(c["theta"], True), t(c["scale"], True)          # theta and scale alone: the same bits
        (sw.finals_autograd(t(Zh), t(c["init"]), th2, sc2) * W).sum().backward()
        np.testing.assert_array_equal(th2.grad.cpu().numpy(), want["grad_theta"])
        np.testing.assert_array_equal(sc2.grad.cpu().numpy(), want["grad_scale"])
    finally:
        sw.close()


# ---------------------------------------------------------------------------------------------------------------------------------
#  GPU: what the bit does not change, non-finite input, the example
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_wide_param_grad_scope_reasons_under_the_bit(qc):
    """With the bit the parameter entries answer as on "mfma16-sweep" handles: outside the gradient's scope with the scope's own reason."""
    L = qc._lib
    specs = {
        "open4": (("density", 4, 1, 0, False, False, 3, 4, ("density", None, "abs"), None), "antisymmetric", "mfma32-sweep", {}),
        "kets3-levels10": (("kets3", 10, 1, 1, True, False, 3, 4, None, None), "no fidelity", "mfma32-sweep", {}),
        "levels12-stored": (("unitary", 12, 2, 1, True, True, 3, 4, U, None), "stored-state gradients are not served in the mfma32-sweep form",
                            "mfma32-sweep", dict(stored_states=True)),
        "levels12-9drives": (("unitary", 12, 9, 1, True, True, 3, 4, U, None), "9 drives", "rollout-per-sample", {}),
    }
    for name, (spec, word, kernel, kw) in specs.items():
        c = tw.build(qc, name, spec)
        sw = make(qc, c, **kw)
        try:
            assert sw.kernel_name == kernel and not sw.grad_supported and word in sw.grad_unsupported_reason, name
            Z = sw.pack(c["controls"], c["dts"])
            with pytest.raises(qc.QCollocError) as e:
                sw.param_grad(Z, c["init"], c["theta"], c["scale"])
            assert e.value.code == L.QC_ERR_UNSUPPORTED and str(e.value).count("qc_sweep gradients: ") == 1 and word in str(e.value), name
            assert sw.grad_unsupported_reason in str(e.value)
            assert np.isfinite(sw.eval(Z, c["init"], c["theta"], c["scale"], fids=False)[0]).all()
        finally:
            sw.close()


@pytest.mark.gpu
def test_wide_param_grad_nan_in_one_sample(qc):
    """A NaN in one sample's theta does not raise: that sample's rows are non-finite, every other row carries the bits of the clean call."""
    rng = np.random.default_rng(10)
    N, m, T, S = 9, 2, 11, 5           # 4 chunks
    sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, 0.3) for _ in range(m)])
    goal, init = ref.operator_to_iso_vec(_unitary(rng, N)), ref.operator_to_iso_vec(_unitary(rng, N))
    sw = qc.RolloutSweep(sys_, [_herm(rng, N)], T, goal=goal, fid_kind="unitary", wide=True, wide_params=True)
    try:
        assert sw.kernel_name == "mfma32-sweep" and sw.launch(S)[2] == 4
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
def test_wide_free_function(qc):
    c = build(qc, "transmons9")
    fids, gth, gsc = qc.rollout_sweep_parameter_gradient(c["init"], c["controls"], c["dts"], c["system"], c["perts"], c["theta"], c["scale"],
                                                         goal=c["goal"], fid_kind="unitary", subspace=c["subspace"], wide=True)
    tp._assert_params(gth, gsc, c, "transmons9 through rollout_sweep_parameter_gradient")
    _, want = qc.rollout_sweep(c["init"], c["controls"], c["dts"], c["system"], c["perts"], c["theta"], c["scale"], goal=c["goal"],
                               fid_kind="unitary", subspace=c["subspace"], wide=True)
    np.testing.assert_array_equal(fids, want)


@pytest.mark.gpu
def test_transmon_worst_case_example():
    """The example as users run it, with its small arguments: exit status 0; every ascent starts at a grid point and never loses, so the
    worst infidelity found is the grid's worst or larger."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "transmon_worst_case.py"), "8", "3", "3"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    assert "kernel mfma32-sweep" in r.stdout
    mm = re.search(r"worst infidelity: grid (\S+) found (\S+)", r.stdout)
    grid_worst, found_worst = float(mm.group(1)), float(mm.group(2))
    assert 0.0 < grid_worst < 1.0 and found_worst >= grid_worst - 1e-9
