"""Sweep pullbacks on wide handles ("mfma32-sweep": qc_sweep32_cot_seed_kernel and the wide walk, 16 < 2N <= 32): every requested output
against the forward-mode reference of tests/sweep_vjp_reference.py, with the checks and the tolerances of test_sweep_vjp.py (read its
header); no parameter cotangents in this form.  Measured worst errors: profiles/sweep_vjp_summary.txt.
Every sample of mid-size and filled launches (S = 301 .. 2049) against the reference: tests/test_sweep_every_sample.py."""
import numpy as np
import pytest
import torch

import sweep_reference as ref
import test_sweep as ts
import test_sweep_vjp as tv
import test_sweep_wide as tw
import test_sweep_wide_grad as twg

_herm, _unitary = ts._herm, ts._unitary

# name: (state, levels, m, p, scale given, free timestep, S, T, fidelity, samples checked against the reference)
WIDE_VJP_CASES = {
    "transmons9": ("unitary", 9, 2, 1, False, True, 5, 11, ("unitary", [0, 1, 3, 4], "abs"), None),       # chunks of 3, 3, 3, 1
    "levels16-8drives": ("unitary", 16, 8, 1, False, True, 3, 6, ("unitary", None, "abs2"), None),         # full tiles
    "kets3-levels10": ("kets3", 10, 1, 1, True, False, 3, 4, None, None),                                  # `grad` refuses this handle
    "one-interval": ("unitary", 9, 2, 1, False, True, 3, 2, ("unitary", None, "abs"), None),                # T = 2
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(WIDE_VJP_CASES))
def test_wide_vjp_matches_the_reference(qc, name):
    c = tv.build(qc, name, WIDE_VJP_CASES)
    sw = ts.make_sweep(qc, c, wide=True)
    try:
        assert sw.kernel_name == "mfma32-sweep" and sw.vjp_supported and sw.vjp_unsupported_reason is None
        want = tw.wide_launch(c["n"], c["m"], c["S"], c["T"])
        assert sw.launch(c["S"]) == (True, want["chunk"], want["n_chunks"])
        if name == "transmons9":
            assert (want["chunk"], want["n_chunks"], want["last"]) == (3, 4, 1)
        if name == "one-interval":
            assert want["n_chunks"] == 1
        if name == "kets3-levels10":
            assert not sw.grad_supported and "no fidelity" in sw.grad_unsupported_reason
        tv.check_case(sw, c, form="32", params=False)
    finally:
        sw.close()


@pytest.mark.gpu
def test_wide_vjp_consistent_with_the_fidelity_gradient(qc):
    c = tw.build(qc, "transmons9", twg.WIDE_GRAD_CASES["transmons9"])
    sw = ts.make_sweep(qc, c, wide=True)
    try:
        tv.check_against_the_fidelity_gradient(sw, c, "32/transmons9-abs")
    finally:
        sw.close()


@pytest.mark.gpu
def test_wide_vjp_bits_host_device_and_side_stream(qc):
    rng = np.random.default_rng(8)
    N, m, T = 9, 2, 20
    sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, (N * m) ** -0.5) for _ in range(m)])
    perts = [_herm(rng, N)]
    make = lambda: qc.RolloutSweep(sys_, perts, T, wide=True)
    sw = make()
    assert sw.kernel_name == "mfma32-sweep"
    Z = sw.pack(rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T))
    sw.close()
    tv.check_bits(qc, make, Z, ref.operator_to_iso_vec(_unitary(rng, N)), m, 2 * N * N, T)


@pytest.mark.gpu
def test_wide_vjp_isolation_of_a_non_finite_cotangent(qc):
    c = tv.build(qc, "transmons9", WIDE_VJP_CASES)
    sw = ts.make_sweep(qc, c, wide=True)
    try:
        tv.check_isolation(sw, c)
    finally:
        sw.close()


@pytest.mark.gpu
def test_wide_finals_autograd(qc):
    """Gradients for Z and init flow on a wide handle (against the pullback called by hand); a theta that requires grad raises."""
    c = tv.build(qc, "transmons9", WIDE_VJP_CASES)
    sw = ts.make_sweep(qc, c, wide=True)
    dev = torch.device("cuda:0")
    t = lambda a, g=False: torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(g)
    try:
        Zh = sw.pack(c["controls"], c["dts"])
        Z, init, W = t(Zh, True), t(c["init"], True), t(c["cot"])
        (sw.finals_autograd(Z, init, t(c["theta"])) * W).sum().backward()
        grad, grad_init = sw.vjp(Zh, c["init"], c["cot"], c["theta"], init_grad=True)
        np.testing.assert_array_equal(Z.grad.cpu().numpy(), grad)
        np.testing.assert_array_equal(init.grad.cpu().numpy(), t(grad_init).sum(0).cpu().numpy())
        assert np.abs(grad).max() > 1e-3 and np.abs(grad_init).max() > 1e-3
        loss = (sw.finals_autograd(t(Zh, True), t(c["init"]), t(c["theta"], True)) * W).sum()
        with pytest.raises(qc.QCollocError) as e:
            loss.backward()
        assert e.value.code == qc._lib.QC_ERR_UNSUPPORTED and "parameter cotangents are not served in the mfma32-sweep form" in str(e.value)
    finally:
        sw.close()


@pytest.mark.gpu
def test_leakage_robust_polish_example_wide(qc):
    import os
    import sys
    sys.path.insert(0, os.path.join(tv.ROOT, "examples"))
    import leakage_robust_polish
    out = leakage_robust_polish.main(T=6, grid=3, steps=3, wide=True, verbose=False)
    print(f"loss {out['loss_before']:.4e} -> {out['loss_after']:.4e}, leakage {out['leakage_before']:.4e} -> {out['leakage_after']:.4e}")
    assert out["kernel"] == "mfma32-sweep"
    assert out["loss_after"] <= out["loss_before"] and out["leakage_after"] < out["leakage_before"]
