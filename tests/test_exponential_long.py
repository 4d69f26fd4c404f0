"""The exponential integrator's MFMA kernels past 256 intervals (qc_mfma_exp.hip, qc_mfma_exp_hess.hip: two intervals per four-wave
workgroup, kIPW = 2, beyond 256 intervals; one wave per interval for dense-image F + dF from 768 intervals) and at config 5's size
(qc_mfma32_exp*.hip, T = 500): every value against the C oracle, placement invariance bit for bit, NaN-poisoned device outputs with a
guard tail, the benchmark's workload, layouts.  Every case asserts the kernel names it was written for; the launch form inside a kernel
(kMU drives a wave, kW waves an interval, kIPW intervals a workgroup) follows from m and the interval count (hess_form / jac_form mirror
the two dispatchers), and test_cases_reach_every_launch_form checks that CASES reaches each of them."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle_bridge import problem_from_inputs, random_problem, sparse_drive_problem
from test_gpu_parity import RawHandle, assert_close_h, kernels_for

pytestmark = pytest.mark.gpu
STEPS = [0.2, 0.01, 1.1, 0.45, 2.0]          # 0 .. 5 squarings: the two intervals of a paired workgroup take different counts
COUNTS = (256, 257, 258, 767, 768, 999)      # last unpaired, first paired (odd), even paired, the dense F + dF switch, the benchmark


def hess_form(m, n_int):
    """(kMU, kW, kIPW) of qc_launch_mfma_exp_hess."""
    kmu, kw = {1: (1, 1), 2: (2, 1), 3: (3, 1), 4: (2, 2), 5: (3, 2), 6: (3, 2), 7: (4, 2), 8: (4, 2)}[m]
    return kmu, kw, 2 if kw == 2 and n_int > 256 else 1


def jac_form(m, n_int, ell):
    """(kMU, kW, kIPW) of qc_launch_mfma_exp (F + dF)."""
    if m <= 1:
        return 1, 1, 1
    if not ell and n_int >= 768:
        return 2 * ((m + 1) // 2), 1, 1
    return (m + 1) // 2, 2, 2 if n_int > 256 else 1


# (system, m, intervals, free Δt, row gathers): "pauli" = multi_qubit_system(2 or 3) (dense images with QC_NO_ELL=1), "sparse" =
# sparse_drive_problem(N=8, R=1) (row gathers), "random" = random dense Hermitian drives at N = 8 (dense images)
CASES = [
    ("sparse", 1, 257, True, True), ("sparse", 2, 256, False, True), ("sparse", 2, 258, True, True), ("sparse", 3, 767, False, True),
    ("pauli", 4, 256, True, True), ("pauli", 4, 257, True, True), ("pauli", 6, 256, False, True), ("pauli", 6, 258, True, True),
    ("pauli", 6, 768, True, True), ("sparse", 7, 256, True, True), ("sparse", 8, 257, True, True), ("sparse", 7, 999, False, True),
    ("random", 1, 258, True, False), ("random", 2, 256, False, False), ("random", 2, 257, True, False), ("random", 2, 768, False, False),
    ("random", 3, 256, True, False), ("pauli", 4, 257, True, False), ("random", 4, 256, False, False), ("random", 4, 999, True, False),
    ("random", 6, 256, True, False), ("pauli", 6, 767, True, False), ("pauli", 6, 768, False, False), ("random", 5, 257, False, False),
    ("random", 8, 256, False, False), ("random", 8, 258, True, False), ("random", 7, 768, True, False),
]


def case_id(c):
    return f"{c[0]}{c[1]}-n{c[2]}-{'ft' if c[3] else 'fixed'}-{'gather' if c[4] else 'dense'}"


def make_case(qc, oracle, monkeypatch, system, m, n_int, free_time, ell, seed=0):
    """The oracle Problem, the knot vector (step column STEPS where the step is free) and a handle of the MFMA kernels."""
    T = n_int + 1
    if system == "pauli":
        nq = {4: 2, 6: 3}[m]
        inp = qc.unitary_smooth_pulse_inputs(qc.multi_qubit_system(nq), qc.GATES[{2: "CNOT", 3: "TOFFOLI"}[nq]], T,
                                             integrator="exponential", free_time=free_time)
        prob, Z = problem_from_inputs(inp), inp.traj.datavec.copy()
    elif system == "sparse":
        prob, Z = sparse_drive_problem(oracle, m=m, T=T, R=1, N=8, free_time=free_time, seed=60 + m + seed, integrator=oracle.EXPONENTIAL)
    else:
        prob, Z = random_problem(oracle, N=8, m=m, T=T, free_time=free_time, integrator=oracle.EXPONENTIAL, seed=80 + m + seed)
    assert prob.m == m
    if free_time:
        Z[prob.off_dt::prob.zdim] = np.resize(STEPS, T)
    assert kernels_for(qc, prob) == ["lds", "mfma"]
    if not ell:
        monkeypatch.setenv("QC_NO_ELL", "1")
    h = RawHandle(qc, prob, kernel="mfma")
    monkeypatch.delenv("QC_NO_ELL", raising=False)
    names = tuple(qc._lib.lib.qc_kernel_name(h.h, k).decode() for k in (0, 1))
    assert names == (("mfma16-exp-gather", "mfma16-exp-hess-gather") if ell else ("mfma16-exp", "mfma16-exp-hess")), names
    assert h.dims.n_intervals == n_int
    return prob, Z, h


def assert_F_J(F, J, Fo, Jo, what):
    np.testing.assert_allclose(F, Fo, rtol=1e-10, atol=1e-12, err_msg=what)
    np.testing.assert_allclose(J, Jo, rtol=1e-10, atol=1e-11 * max(1.0, np.abs(Jo).max()), err_msg=what)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def test_cases_reach_every_launch_form():
    """CASES reach every (kMU, kW, kIPW) of both dispatchers in both drive-image forms, kIPW = 2 wherever it exists, and every count
    of COUNTS."""
    got_h = {(ell,) + hess_form(m, n) for _, m, n, _, ell in CASES}
    got_j = {(ell,) + jac_form(m, n, ell) for _, m, n, _, ell in CASES}
    for ell in (True, False):
        for m in (1, 2, 3, 4, 6, 8):
            for n in (256, 257):
                assert (ell,) + hess_form(m, n) in got_h, ("mu_d2F", ell, m, n)
                assert (ell,) + jac_form(m, n, ell) in got_j, ("F + dF", ell, m, n)
    for m in (2, 4, 6, 8):
        assert (False,) + jac_form(m, 768, False) in got_j, ("F + dF one wave", m)
    assert set(COUNTS) <= {n for _, _, n, _, _ in CASES}
    assert {True, False} == {ft for _, _, _, ft, _ in CASES}


@pytest.mark.parametrize("system,m,n_int,free_time,ell", CASES, ids=[case_id(c) for c in CASES])
def test_every_value_against_the_c_oracle(qc, oracle, coracle, monkeypatch, system, m, n_int, free_time, ell):
    """F + dF, F alone and mu_d2F (mu = ones and random) of every launch form across the 256-interval switch, every value against the
    C oracle."""
    prob, Z, h = make_case(qc, oracle, monkeypatch, system, m, n_int, free_time, ell)
    ref = coracle.COracle(prob)
    what = f"{case_id((system, m, n_int, free_time, ell))}: F + dF {jac_form(m, n_int, ell)}, mu_d2F {hess_form(m, n_int)}"
    Fo, Jo = ref.F_dF(Z)
    F, J = h.F_jac(Z)
    assert_F_J(F, J, Fo, Jo, what)
    np.testing.assert_allclose(h.F(Z), Fo, rtol=1e-10, atol=1e-12, err_msg=f"{what}: F alone")
    for mu in (np.ones(prob.n_rows), np.random.default_rng(n_int + m).standard_normal(prob.n_rows)):
        Ho = ref.mu_d2F(Z, mu)
        assert h.dims.hess_nnz == Ho.size
        assert_close_h(h.hess(Z, mu), Ho, what)
    h.close()


# 256, 1, 257 (odd t_begin, odd count), 1, 484 (odd t_begin, even count) intervals: kIPW = 1, 1, 2, 1, 2
SHARDS = ((0, 256), (256, 257), (257, 514), (514, 515), (515, 999))


@pytest.mark.parametrize("ell", [True, False], ids=["gather", "dense"])
def test_shards_equal_the_paired_launch_bit_for_bit(qc, oracle, monkeypatch, ell):
    """One handle over 999 intervals (the paired form) against knot shards of the same trajectory (t_range) that run kIPW = 1 and
    kIPW = 2 from odd first intervals: the concatenated values are the same bits.  Dense images: mu_d2F only (the full handle's
    F + dF takes one wave per interval, the shards' two)."""
    prob, Z, full = make_case(qc, oracle, monkeypatch, "pauli", 6, 999, True, ell)
    mu = np.random.default_rng(3).standard_normal(prob.n_rows)
    F, J = full.F_jac(Z)
    H = full.hess(Z, mu)
    full.close()
    Fs, Js, Hs = [], [], []
    if not ell:
        monkeypatch.setenv("QC_NO_ELL", "1")
    for a, b in SHARDS:
        h = RawHandle(qc, prob, kernel="mfma", t_range=(a, b))
        assert h.dims.n_intervals == b - a
        f, j = h.F_jac(Z)
        Fs.append(f)
        Js.append(j)
        Hs.append(h.hess(Z, mu))          # (the full multiplier vector: a shard reads its rows from t_begin on)
        h.close()
    monkeypatch.delenv("QC_NO_ELL", raising=False)
    if ell:
        np.testing.assert_array_equal(bits(np.concatenate(Fs)), bits(F))
        np.testing.assert_array_equal(bits(np.concatenate(Js)), bits(J))
    np.testing.assert_array_equal(bits(np.concatenate(Hs)), bits(H))


@pytest.mark.parametrize("n_int", [257, 999])
@pytest.mark.parametrize("system,m,ell", [("pauli", 6, True), ("pauli", 6, False), ("sparse", 8, True), ("random", 7, False)],
                         ids=["pauli6-gather", "pauli6-dense", "sparse8-gather", "random7-dense"])
def test_poisoned_device_outputs_and_guard_tail(qc, oracle, monkeypatch, n_int, system, m, ell):
    """Device-resident F + dF and mu_d2F into NaN-filled buffers one interval block longer than the handle's: every value in range is
    written (and equals the host path's), the guard block stays NaN -- the odd count's idle half of the last workgroup returns before
    it stores anything."""
    prob, Z, h = make_case(qc, oracle, monkeypatch, system, m, n_int, True, ell, seed=5)
    L = qc._lib
    d = h.dims
    mu = np.random.default_rng(n_int).standard_normal(prob.n_rows)
    F, J = h.F_jac(Z)
    H = h.hess(Z, mu)
    Zd, mud = torch.from_numpy(Z).cuda(), torch.from_numpy(mu).cuda()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    Fd, Jd, Hd = (torch.full((int(n) + int(k),), float("nan"), dtype=torch.float64, device="cuda")
                  for n, k in ((d.F_len, d.ddim), (d.jac_nnz, d.jac_nnz_interval), (d.hess_nnz, d.hess_nnz_interval)))
    L.check(L.lib.qc_eval_F_jac_dev(h.h, Zd.data_ptr(), Fd.data_ptr(), Jd.data_ptr(), st), h.h)
    L.check(L.lib.qc_eval_hess_dev(h.h, Zd.data_ptr(), mud.data_ptr(), Hd.data_ptr(), st), h.h)
    torch.cuda.synchronize()
    for buf, n, host, what in ((Fd, d.F_len, F, "F"), (Jd, d.jac_nnz, J, "dF"), (Hd, d.hess_nnz, H, "mu_d2F")):
        v = buf.cpu().numpy()
        assert np.isfinite(v[:n]).all(), f"{what}: {int((~np.isfinite(v[:n])).sum())} values in range not written"
        assert np.isnan(v[n:]).all(), f"{what}: the guard block was written"
        np.testing.assert_array_equal(bits(v[:n]), bits(host), err_msg=what)
    h.close()


def test_benchmark_workload(qc, coracle):
    """bench.py's exponential_integrator record: config 3 (3-qubit Toffoli, six Pauli drives) at T = 1000 -- 999 intervals, the paired
    row-gather forms.  Every value against the C oracle; the one-call device path is the two launches, bit for bit."""
    inp = qc.config_inputs(3, T=1000, integrator="exponential")
    prob = problem_from_inputs(inp)
    Z = inp.traj.datavec
    dyn = qc.QuantumDynamics(inp.integrators, inp.traj)
    assert dyn.kernel_names == ("mfma16-exp-gather", "mfma16-exp-hess-gather")
    assert dyn.fused_kernel_name == "two-launches"
    assert (prob.m, dyn.dims.n_intervals) == (6, 999) and hess_form(6, 999) == (3, 2, 2) and jac_form(6, 999, True) == (3, 2, 2)
    ref = coracle.COracle(prob)
    Fo, Jo = ref.F_dF(Z)
    F, J = dyn.F_dF(Z, fresh=True)
    assert_F_J(F, J, Fo, Jo, "config 3, T = 1000")
    np.testing.assert_allclose(dyn.F(Z, fresh=True), Fo, rtol=1e-10, atol=1e-12, err_msg="F alone")
    mu = np.random.default_rng(1000).standard_normal(int(dyn.dims.n_rows))
    H = dyn.mu_d2F(Z, mu, fresh=True)
    assert_close_h(H, ref.mu_d2F(Z, mu), "config 3, T = 1000")
    d = dyn.dims
    dZ, dmu = torch.from_numpy(Z).cuda(), torch.from_numpy(mu).cuda()
    nan = lambda n: torch.full((int(n),), float("nan"), dtype=torch.float64, device="cuda")
    F1, J1, H1, F2, J2, H2 = nan(d.F_len), nan(d.jac_nnz), nan(d.hess_nnz), nan(d.F_len), nan(d.jac_nnz), nan(d.hess_nnz)
    dyn.F_dF_mu_d2F_device(dZ, dmu, F1, J1, H1)
    dyn.F_dF_device(dZ, F2, J2)
    dyn.mu_d2F_device(dZ, dmu, H2)
    torch.cuda.synchronize()
    for one, two, host, what in ((F1, F2, F, "F"), (J1, J2, J, "dF"), (H1, H2, H, "mu_d2F")):
        a, b = one.cpu().numpy(), two.cpu().numpy()
        np.testing.assert_array_equal(bits(a), bits(b), err_msg=f"{what}: one call against two launches")
        np.testing.assert_array_equal(bits(a), bits(host), err_msg=f"{what}: device against host buffers")
    dyn.close()


def test_config5_size_both_forms(qc, coracle, monkeypatch):
    """2N = 32 at config 5's size (4 qubits, eight Pauli drives, T = 500: the README's mfma32-exp and mfma32-exp-hess times), the
    row-gather and the dense-image forms, every value of F + dF and mu_d2F against the C oracle."""
    inp = qc.config_inputs(5, T=500, integrator="exponential")
    prob = problem_from_inputs(inp)
    Z = inp.traj.datavec
    gather = qc.QuantumDynamics(inp.integrators, inp.traj)
    monkeypatch.setenv("QC_NO_ELL", "1")
    dense = qc.QuantumDynamics(inp.integrators, inp.traj)
    monkeypatch.delenv("QC_NO_ELL")
    assert gather.kernel_names == ("mfma32-exp-gather", "mfma32-exp-hess-gather")
    assert dense.kernel_names == ("mfma32-exp", "mfma32-exp-hess")
    ref = coracle.COracle(prob)
    Fo, Jo = ref.F_dF(Z)
    mu = np.random.default_rng(500).standard_normal(int(gather.dims.n_rows))
    Ho = ref.mu_d2F(Z, mu)
    for dyn, what in ((gather, "row gathers"), (dense, "dense images")):
        F, J = dyn.F_dF(Z, fresh=True)
        assert_F_J(F, J, Fo, Jo, what)
        assert_close_h(dyn.mu_d2F(Z, mu, fresh=True), Ho, what)
        dyn.close()


@pytest.mark.parametrize("m,n_int", [(4, 257), (7, 768)])
def test_ket_states_past_256_intervals(qc, oracle, coracle, m, n_int):
    """Three ket columns (state_cols = 3) at 2N = 16 with dense drives: F + dF (paired two-wave, one-wave) and mu_d2F (paired) against
    the C oracle."""
    prob, Z = random_problem(oracle, N=8, m=m, T=n_int + 1, integrator=oracle.EXPONENTIAL, seed=33 + m, ncol=3)
    Z[prob.off_dt::prob.zdim] = np.resize(STEPS, prob.T)
    h = RawHandle(qc, prob, kernel="mfma")
    assert (qc._lib.lib.qc_kernel_name(h.h, 0), qc._lib.lib.qc_kernel_name(h.h, 1)) == (b"mfma16-exp", b"mfma16-exp-hess")
    ref = coracle.COracle(prob)
    Fo, Jo = ref.F_dF(Z)
    F, J = h.F_jac(Z)
    assert_F_J(F, J, Fo, Jo, f"kets, m = {m}")
    np.testing.assert_allclose(h.F(Z), Fo, rtol=1e-10, atol=1e-12)
    mu = np.random.default_rng(m).standard_normal(prob.n_rows)
    assert_close_h(h.hess(Z, mu), ref.mu_d2F(Z, mu), f"kets, m = {m}")
    h.close()


@pytest.mark.parametrize("ell", [True, False], ids=["gather", "dense"])
def test_hess_align_16_past_256_intervals(qc, monkeypatch, ell):
    """hess_align = 16 on an exponential handle at T = 1000 (config 3): the padding of every interval block is exact zeros (written by
    the kernel: device buffers start NaN), its structure repeats the interval's first entry, and the interval's own values are the
    hess_align = 0 handle's, bit for bit."""
    inp = qc.config_inputs(3, T=1000, integrator="exponential")
    Z = inp.traj.datavec
    if not ell:
        monkeypatch.setenv("QC_NO_ELL", "1")
    plain = qc.QuantumDynamics(inp.integrators, inp.traj)
    padded = qc.QuantumDynamics(inp.integrators, inp.traj, hess_align=16)
    monkeypatch.delenv("QC_NO_ELL", raising=False)
    names = ("mfma16-exp-gather", "mfma16-exp-hess-gather") if ell else ("mfma16-exp", "mfma16-exp-hess")
    assert plain.kernel_names == padded.kernel_names == names
    own, wide, n = int(plain.dims.hess_nnz_interval), int(padded.dims.hess_nnz_interval), int(plain.dims.n_intervals)
    assert n == 999 and wide % 16 == 0 and own < wide < own + 16
    mu = np.random.default_rng(16).standard_normal(int(plain.dims.n_rows))
    H0 = plain.mu_d2F(Z, mu, fresh=True).reshape(n, own)
    dH = torch.full((n * wide,), float("nan"), dtype=torch.float64, device="cuda")
    padded.mu_d2F_device(torch.from_numpy(Z).cuda(), torch.from_numpy(mu).cuda(), dH)
    torch.cuda.synchronize()
    for H1 in (dH.cpu().numpy().reshape(n, wide), padded.mu_d2F(Z, mu, fresh=True).reshape(n, wide)):
        assert not bits(H1[:, own:]).any(), "padding is not +0.0"
        np.testing.assert_array_equal(bits(H1[:, :own]), bits(H0))
    hr0, hc0 = (x.reshape(n, own) for x in plain.mu_d2F_structure)
    hr1, hc1 = (x.reshape(n, wide) for x in padded.mu_d2F_structure)
    np.testing.assert_array_equal(hr1[:, :own], hr0)
    np.testing.assert_array_equal(hc1[:, :own], hc0)
    np.testing.assert_array_equal(hr1[:, own:], np.repeat(hr0[:, :1], wide - own, axis=1))
    np.testing.assert_array_equal(hc1[:, own:], np.repeat(hc0[:, :1], wide - own, axis=1))
    F0, J0 = plain.F_dF(Z, fresh=True)
    F1, J1 = padded.F_dF(Z, fresh=True)
    np.testing.assert_array_equal(bits(F1), bits(F0))
    np.testing.assert_array_equal(bits(J1), bits(J0))
    plain.close()
    padded.close()
