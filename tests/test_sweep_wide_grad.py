"""Sweep gradients on wide handles ("mfma32-sweep", csrc/qc_sweep32_grad.hip): dF_s/da_{t,k} and dF_s/ddt_t for 16 < 2N <= 32.  Every
value of `grad_samples` against the forward-mode reference of tests/sweep_grad_reference.py, `fids` against `eval` on the same handle
(bits), `J` and `grad` against the weighted sum, +0.0 outside the derivatives, the scratch path (test_sweep_grad._check_call), the
squarings, bits, refusals, non-finite input, the objective inside an evaluator and the example.

Tolerance: test_sweep_grad.py's, per sample |got - want| <= 1e-9 max(1, max |grad F_s|); a gradient entry is a bounded bilinear form in
the state and the adjoint, whatever the size.  Measured worst errors: profiles/sweep_wide_summary.txt.
Every sample of mid-size and filled launches (S = 301 .. 2049) against the reference: tests/test_sweep_every_sample.py."""
import os
import sys

import numpy as np
import pytest
import torch

import sweep_reference as ref
import test_sweep as ts
import test_sweep_grad as tg
import test_sweep_wide as tw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_herm, _unitary = ts._herm, ts._unitary

# name: (state, levels, m, p, scale given, free timestep, S, T, fidelity, samples checked against the reference)
WIDE_GRAD_CASES = {
    "transmons9": ("unitary", 9, 2, 1, False, True, 5, 11, ("unitary", [0, 1, 3, 4], "abs"), None),         # chunks of 3, 3, 3, 1
    "levels12-3drives": ("unitary", 12, 3, 1, True, False, 3, 8, ("unitary", None, "abs2"), None),           # fixed timestep
    "levels16-6drives": ("unitary", 16, 6, 1, True, True, 3, 6, ("unitary", None, "abs"), None),             # full tiles
    "levels16-8drives": ("unitary", 16, 8, 1, False, True, 3, 6, ("unitary", None, "abs2"), None),
    "ket10": ("ket", 10, 2, 1, True, True, 11, 6, ("ket", None, "abs"), None),
    "one-interval": ("unitary", 9, 2, 1, False, True, 3, 2, ("unitary", None, "abs"), None),                  # T = 2
    "one-chunk": ("unitary", 9, 2, 1, True, True, 2048, 3, ("unitary", None, "abs"), (0, 1000, 2047)),       # n_chunks = 1
    "sqrt-capped": ("unitary", 9, 2, 1, False, True, 2, 102, ("unitary", [0, 1, 3, 4], "abs"), None),        # 11 chunks of 10, the last 1
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(WIDE_GRAD_CASES))
def test_wide_grad_matches_the_reference(qc, name):
    c = tw.build(qc, name, WIDE_GRAD_CASES[name])
    sw = ts.make_sweep(qc, c, wide=True)
    try:
        assert sw.kernel_name == "mfma32-sweep" and sw.grad_supported and sw.grad_unsupported_reason is None
        want = tw.wide_launch(c["n"], c["m"], c["S"], c["T"])
        assert sw.launch(c["S"]) == (True, want["chunk"], want["n_chunks"])
        if name == "transmons9":
            assert (want["chunk"], want["n_chunks"], want["last"]) == (3, 4, 1)
        if name in ("one-chunk", "one-interval"):
            assert want["n_chunks"] == 1
        if name == "sqrt-capped":
            assert want["by_sqrt"] and (want["chunk"], want["n_chunks"], want["last"]) == (10, 11, 1)
        tg._check_call(sw, sw.pack(c["controls"], c["dts"]), c)
    finally:
        sw.close()


@pytest.mark.gpu
def test_wide_grad_through_the_squarings(qc):
    seen = set()
    for k, per_sample, c in tw.squaring_cases(qc):
        seen |= set(per_sample)
        sw = qc.RolloutSweep(c["system"], c["perts"], c["T"], goal=c["goal"], fid_kind="unitary", dt_fixed=c["dts"], wide=True)
        try:
            assert sw.kernel_name == "mfma32-sweep"
            tg._check_call(sw, sw.pack(c["controls"]), c)
        finally:
            sw.close()
    assert set(range(7)) <= seen


@pytest.mark.gpu
def test_wide_grad_bits_host_device_and_side_stream(qc):
    """Six repeated calls return identical bits; the host and device entry points return identical bits on a side stream; S grows, then
    shrinks: the bits of a fresh handle; non-uniform weights."""
    rng = np.random.default_rng(8)
    N, m, T = 9, 2, 20
    sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, (N * m) ** -0.5) for _ in range(m)])
    perts = [_herm(rng, N)]
    goal = ref.operator_to_iso_vec(_unitary(rng, N))
    make = lambda: qc.RolloutSweep(sys_, perts, T, goal=goal, fid_kind="unitary", subspace=[0, 1, 3, 4], wide=True)
    sw = make()
    Z = sw.pack(rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T))
    init = ref.operator_to_iso_vec(_unitary(rng, N))
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    side = torch.cuda.Stream(device=dev)
    try:
        for i, S in enumerate((3, 150, 7)):
            theta, scale, w = rng.uniform(-0.3, 0.3, (S, 1)), rng.uniform(0.9, 1.1, (S, m)), rng.uniform(0.5, 1.5, S)
            fresh = make()
            first = fresh.grad(Z, init, theta, scale, weights=w, per_sample=True)
            fresh.close()
            got = sw.grad(Z, init, theta, scale, weights=w, per_sample=True)
            assert got[0] == first[0]
            for a, b in zip(got[1:], first[1:]):
                np.testing.assert_array_equal(a, b)
            if i == 1:
                for _ in range(6):
                    again = sw.grad(Z, init, theta, scale, weights=w, per_sample=True)
                    assert again[0] == first[0]
                    for a, b in zip(again[1:], first[1:]):
                        np.testing.assert_array_equal(a, b)
            dZ, dinit, dth, dsc, dw = t(Z), t(init), t(theta), t(scale), t(w)
            mk = lambda *shape: torch.full(shape, -7.0, dtype=torch.float64, device=dev)
            dfid, dJ, dg, dgs = mk(S), mk(1), mk(sw.Z_len), mk(S, T - 1, sw.n_deriv)
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                sw.grad_device(dZ, dinit, S, dth, dsc, dw, dfid, dJ, dg, dgs, stream=side)
            side.synchronize()
            assert dJ.item() == first[0]
            for a, b in zip((dfid, dg, dgs), first[1:]):
                np.testing.assert_array_equal(a.cpu().numpy(), b)
            dg2 = mk(sw.Z_len)          # outputs are optional one at a time
            sw.grad_device(dZ, dinit, S, dth, dsc, dw, dgrad=dg2, stream=side)
            side.synchronize()
            np.testing.assert_array_equal(dg2.cpu().numpy(), first[2])
    finally:
        sw.close()


@pytest.mark.gpu
def test_wide_grad_refused_handles(qc):
    """Wide handles outside the scope say so and still serve the sweep; parameter gradients are refused on every mfma32-sweep handle."""
    L = qc._lib
    par_msg = "qc_sweep gradients: parameter gradients are not served in the mfma32-sweep form"
    specs = {
        "open4": (("density", 4, 1, 0, False, False, 3, 4, ("density", None, "abs"), None), "antisymmetric"),
        "levels12-9drives": (("unitary", 12, 9, 1, True, True, 3, 4, ("unitary", None, "abs"), None), "9 drives"),
        "kets3-levels10": (("kets3", 10, 1, 1, True, False, 3, 4, None, None), "no fidelity"),
    }
    for name, (spec, word) in specs.items():
        c = tw.build(qc, name, spec)
        sw = ts.make_sweep(qc, c, wide=True)
        try:
            assert sw.kernel_name == ("rollout-per-sample" if name == "levels12-9drives" else "mfma32-sweep")
            assert not sw.grad_supported and word in sw.grad_unsupported_reason, name
            Z = sw.pack(c["controls"], c["dts"])
            with pytest.raises(qc.QCollocError) as e:
                sw.grad(Z, c["init"], c["theta"], c["scale"])
            assert e.value.code == L.QC_ERR_UNSUPPORTED and word in str(e.value), name
            with pytest.raises(qc.QCollocError) as e:
                sw.param_grad(Z, c["init"], c["theta"], c["scale"])
            assert e.value.code == L.QC_ERR_UNSUPPORTED
            if sw.kernel_name == "mfma32-sweep":
                assert par_msg in str(e.value)
            finals, _ = sw.eval(Z, c["init"], c["theta"], c["scale"], fids=False)
            assert np.isfinite(finals).all()
        finally:
            sw.close()
    # a handle whose control gradients are served
    c = tw.build(qc, "transmons9", WIDE_GRAD_CASES["transmons9"])
    sw = ts.make_sweep(qc, c, wide=True)
    try:
        Z = sw.pack(c["controls"], c["dts"])
        assert sw.grad_supported
        with pytest.raises(qc.QCollocError) as e:
            sw.param_grad(Z, c["init"], c["theta"], c["scale"])
        assert e.value.code == L.QC_ERR_UNSUPPORTED and par_msg in str(e.value)
        dev = torch.device("cuda:0")
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        with pytest.raises(qc.QCollocError) as e:
            sw.param_grad_device(t(Z), t(c["init"]), c["S"], t(c["theta"]), dgrad_theta=torch.zeros((c["S"], 1), dtype=torch.float64, device=dev))
        assert e.value.code == L.QC_ERR_UNSUPPORTED and par_msg in str(e.value)
        assert np.isfinite(sw.eval(Z, c["init"], c["theta"], c["scale"])[1]).all()
        assert np.isfinite(sw.grad(Z, c["init"], c["theta"], c["scale"])[2]).all()
    finally:
        sw.close()


@pytest.mark.gpu
def test_wide_grad_non_finite_input(qc):
    """test_grad_non_finite_input on a wide handle of 9 levels: a NaN control in the last knot reaches nothing; inside the trajectory it
    reaches every sample, the entries that are no derivative stay +0.0, and the handle then serves a finite call."""
    rng = np.random.default_rng(4)
    N, m, T, S = 9, 2, 14, 4
    sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, 0.3) for _ in range(m)])
    goal = ref.operator_to_iso_vec(_unitary(rng, N))
    zdim = m + 3
    sw = qc.RolloutSweep(sys_, [_herm(rng, N)], T, goal=goal, fid_kind="unitary", zdim=zdim, off_a=1, off_dt=m + 2, global_dim=2, wide=True)
    try:
        assert sw.kernel_name == "mfma32-sweep"
        controls, dts = rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T)
        init, theta = ref.operator_to_iso_vec(_unitary(rng, N)), rng.uniform(-0.3, 0.3, (S, 1))
        good = sw.grad(sw.pack(controls, dts), init, theta, per_sample=True)
        assert np.isfinite(good[2]).all() and np.isfinite(good[3]).all()
        bad = controls.copy()
        bad[0, T - 1] = np.nan
        again = sw.grad(sw.pack(bad, dts), init, theta, per_sample=True)
        assert again[0] == good[0]
        for a, b in zip(again[1:], good[1:]):
            np.testing.assert_array_equal(a, b)
        bad = controls.copy()
        bad[1, 7] = np.nan
        J, fids, grad, gs = sw.grad(sw.pack(bad, dts), init, theta, per_sample=True)
        assert np.isnan(J) and np.isnan(fids).all() and np.isnan(gs).all()
        K = grad[:T * zdim].reshape(T, zdim)
        assert np.isnan(K[:T - 1, 1:1 + m]).all() and np.isnan(K[:T - 1, m + 2]).all()
        for zero in (K[:, 0], K[:, m + 1], K[T - 1], grad[T * zdim:]):
            assert np.array_equal(zero.view(np.uint64), np.zeros(zero.size, dtype=np.uint64))
        after = sw.grad(sw.pack(controls, dts), init, theta, per_sample=True)
        for a, b in zip(after[1:], good[1:]):
            np.testing.assert_array_equal(a, b)
    finally:
        sw.close()


@pytest.mark.gpu
def test_wide_objective_in_an_evaluator(qc):
    """`SweepInfidelityObjective(wide=True)` at 9 levels inside a first-order evaluator: the objective gradient against central
    differences of the objective, every control and timestep entry, 1e-6 relative (the finite-difference bound of
    test_reference_routes_agree: error / max(1, max |grad|))."""
    rng = np.random.default_rng(21)
    N, m, T, S = 9, 2, 5, 3
    traj = tg._traj(qc, rng, N=N, m=m, T=T)
    sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, 0.5) for _ in range(m)])
    P = np.diag(np.arange(N) // 3).astype(complex)
    theta, w = rng.uniform(-0.2, 0.2, (S, 1)), rng.uniform(0.1, 0.5, S)
    with pytest.raises(qc.QCollocError) as e:
        qc.SweepInfidelityObjective(traj, sys_, [P], theta, weights=w, subspace=[0, 1, 3, 4])
    assert e.value.code == qc._lib.QC_ERR_UNSUPPORTED and "2N = 18" in str(e.value)
    obj = qc.SweepInfidelityObjective(traj, sys_, [P], theta, weights=w, subspace=[0, 1, 3, 4], wide=True)
    Z = traj.datavec

    class _Dyn:      # the evaluator reads the dimensions and structures of its dynamics at construction, nothing else here
        class dims:
            Z_len, n_rows, jac_nnz, hess_nnz = Z.size, 0, 0, 0
        dF_structure = (np.empty(0, dtype=np.int64), np.empty(0, dtype=np.int64))
        mu_d2F_structure = (np.empty(0, dtype=np.int64), np.empty(0, dtype=np.int64))

    try:
        ev = qc.QuantumControlEvaluator(_Dyn(), [obj], eval_hessian=False)
        g = np.empty(Z.size)
        ev.eval_objective_gradient(g, Z)
        np.testing.assert_array_equal(g, np.zeros(Z.size) + obj.grad_L(Z))
        assert ev.eval_objective(Z) == obj.L(Z)
        idx = [t * traj.dim + o for t in range(T - 1) for o in list(range(traj.offset("a"), traj.offset("a") + m)) + [traj.offset("Δt")]]
        fd = np.zeros(Z.size)
        for k in idx:
            e_k = np.zeros(Z.size)
            e_k[k] = 1e-5
            fd[k] = (ev.eval_objective(Z + e_k) - ev.eval_objective(Z - e_k)) / 2e-5
        err = np.abs(fd - g).max() / max(1.0, np.abs(g).max())
        print(f"SWEEP-WIDE objective: central differences vs grad_L {err:.2e} (bound 1e-6), max |grad| {np.abs(g).max():.3f}")
        assert err < 1e-6 and np.abs(g[idx]).min() > 0 and np.count_nonzero(g) == len(idx)
    finally:
        obj.close()


@pytest.mark.gpu
def test_transmon_robustness_example(qc):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import transmon_robustness
    out = transmon_robustness.run(T=12, grid=5, steps=4, landscape=9, verbose=False)
    hist = out["history"]
    print(f"mean infidelity over the grid: {' -> '.join(f'{v:.4e}' for v in hist)}")
    assert len(hist) >= 2 and all(b < a for a, b in zip(hist, hist[1:])) and hist[-1] < hist[0]
    assert out["kernel"] == "mfma32-sweep" and out["landscape_before"].shape == (9,) == out["landscape_after"].shape
    for F in (out["landscape_before"], out["landscape_after"]):
        assert np.all(F > -1e-9) and np.all(F < 1 + 1e-9)
