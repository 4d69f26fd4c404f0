"""Matrix-free product with the Hessian of the Lagrangian of the dynamics, w = H(Z, mu) v (qc_eval_hvp and its device, list and
host-layer forms), against the CPU oracle.

Reference, never the library's own Hessian: U = coo_matrix((oracle.mu_d2F(prob, Z, mu), oracle.hess_structure(prob))) (the C
restatement of the oracle where the trajectory is long), H_ref = U + U' - diag(U), w_ref = H_ref @ v in float64.

Tolerance (derived, not chosen): the project's parity contract is 1e-10 relative per Hessian entry (tests/test_gpu_parity.py, RTOL),
so a sum of such terms obeys
    |w - w_ref|_i <= 1e-10 (|H_ref| |v|)_i + 1e-12 max|w_ref|        for every i, no entry left out,
with the bound computed from H_ref.  Entries with (|H_ref| |v|)_i = 0 must be exactly +0.0.  w is prefilled with NaN before every call.

Every case of the fused list runs on the handle as the plan serves it and again on a handle created under QC_NO_PRODUCT_MFMA=1.  The
library holds no fused Hessian-product kernel (profiles/hess_products_summary.txt): both run "generic-hvp" today, and the
parametrisation stays so that a fused kernel, when one ships, meets the same cases.  The product kernel runs one workgroup per knot
without a grid limit; long_1030 / long_2051 are past one and two passes of the 1024-workgroup persistent grids of the mu_d2F kernels
that fill the scratch."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from oracle_bridge import composed_oracle, problem_from_inputs, random_problem
from test_products import FUSED_CASES, GENERIC_CASES, build_case, deriv_problem, list_inputs

gpu = pytest.mark.gpu
PLAN_NAME = "generic-hvp"      # what qc_plan chooses for a handle the fused Jacobian-product kernel serves: there is no fused hvp kernel
HVP_CASES = FUSED_CASES + ["nonherm"]


# ------------------------------------------------------------------------------------------------
#  Handles straight from an oracle Problem (raw C descriptor), with every descriptor field the cases vary
# ------------------------------------------------------------------------------------------------
def fill_desc(L, prob, *, kernel="auto", t_range=None, hess_align=0, hess_block_order=None):
    d = L.qc_desc()
    d.N, d.m, d.T, d.zdim, d.global_dim = prob.N, prob.m, prob.T, prob.zdim, prob.global_dim
    d.off_U, d.off_a, d.off_dt, d.dt_fixed = prob.off_U, prob.off_a, prob.off_dt, prob.dt_fixed
    d.integrator, d.pade_order = prob.integrator, prob.order
    d.n_deriv = len(prob.derivs)
    for i, dv in enumerate(prob.derivs):
        d.deriv_x_off[i], d.deriv_dx_off[i], d.deriv_dim[i] = dv.x_off, dv.dx_off, dv.dim
    G0 = np.asfortranarray(prob.G_drift)
    Gd = np.ascontiguousarray(np.stack([g.reshape(-1, order="F") for g in prob.G_drives])) if prob.m else np.zeros((1, 1))
    d.G_drift, d.G_drives = L.dptr(G0), L.dptr(Gd)
    d.state_cols = getattr(prob, "ncol", 0)
    d.kernel = {"auto": L.QC_KERNEL_AUTO, "lds": L.QC_KERNEL_LDS, "mfma": L.QC_KERNEL_MFMA}[kernel]
    if prob.deriv_rows is not None:
        d.row_placement = L.QC_ROWS_BY_COMPONENT
        d.rows_per_interval, d.row_offset = prob.rows_per_interval, prob.row_offset
        for i, r in enumerate(prob.deriv_rows):
            d.deriv_row_off[i] = r
    d.hess_align = hess_align
    if hess_block_order is not None:
        for i, x in enumerate(hess_block_order):
            d.hess_block_order[i] = x
    if t_range:
        d.t_begin, d.t_end = t_range
    return d, (G0, Gd)


class Handle:
    def __init__(self, qc, prob, *, generic=False, **kw):
        self.qc, self.L = qc, qc._lib
        L = self.L
        d, self._keep = fill_desc(L, prob, **kw)
        self.h = C.c_void_p()
        old = os.environ.pop("QC_NO_PRODUCT_MFMA", None)
        if generic:
            os.environ["QC_NO_PRODUCT_MFMA"] = "1"      # read when the handle is created
        try:
            L.check(L.lib.qc_create(C.byref(d), C.byref(self.h)))
        finally:
            os.environ.pop("QC_NO_PRODUCT_MFMA", None)
            if old is not None:
                os.environ["QC_NO_PRODUCT_MFMA"] = old
        self.dims = L.qc_dims_t()
        L.check(L.lib.qc_dims(self.h, C.byref(self.dims)), self.h)

    @property
    def name(self):
        return self.L.lib.qc_kernel_name(self.h, 5).decode()

    def hvp_dev(self, dZ, dmu, dv, dw):
        p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
        self.L.check(self.L.lib.qc_eval_hvp_dev(self.h, p(dZ), p(dmu), p(dv), p(dw), C.c_void_p(torch.cuda.current_stream().cuda_stream)), self.h)

    def hvp(self, Z, mu, v):
        dw = torch.full((int(self.dims.Z_len),), float("nan"), dtype=torch.float64, device="cuda")
        self.hvp_dev(torch.from_numpy(Z).cuda(), torch.from_numpy(mu).cuda(), torch.from_numpy(v).cuda(), dw)
        return dw.cpu().numpy()

    def close(self):
        self.L.lib.qc_destroy(self.h)


def sym_from_upper(vals, rows, cols, n):
    """H_ref = U + U' - diag(U) of the upper-triangle COO piece (duplicates summed), and |H_ref|."""
    U = sp.coo_matrix((vals, (rows, cols)), shape=(n, n)).tocsr()
    H = (U + U.T - sp.diags(U.diagonal())).tocsr()
    return H, abs(H)


def reference(oracle, prob, Z, mu, t_range=None, coracle=None):
    t0, t1 = t_range if t_range else (0, prob.T - 1)
    vals = coracle.COracle(prob).mu_d2F(Z, mu, t0, t1) if coracle is not None else oracle.mu_d2F(prob, Z, mu, t0, t1)
    rows, cols = oracle.hess_structure(prob, t_begin=t0, t_end=t1)
    return sym_from_upper(vals, rows, cols, prob.n_vars)


def bound_of(Habs, v, w_ref):
    return 1e-10 * (Habs @ np.abs(v)) + 1e-12 * np.abs(w_ref).max()


def assert_within(w, H, Habs, v, what):
    """Every entry of w against H v within the derived bound; entries nothing touches exactly +0.0.  Returns the bound."""
    assert np.isfinite(w).all(), f"{what}: {np.count_nonzero(~np.isfinite(w))} entries of w were not written"
    w_ref = H @ v
    scale = Habs @ np.abs(v)
    zero = scale == 0.0
    assert np.all(w[zero] == 0.0) and not np.signbit(w[zero]).any(), f"{what}: entries no Hessian entry touches must be exactly +0.0"
    err, bnd = np.abs(w - w_ref), bound_of(Habs, v, w_ref)
    print(f"{what}: (mu d2F) v max err / bound = {np.max(err / bnd):.3e}")
    assert np.all(err <= bnd), f"{what}: misses the bound by up to {np.max(err / bnd):.3g} x"
    return bnd


def mu_of(prob, seed):
    return np.random.default_rng(seed).standard_normal(prob.row_stride * (prob.T - 1))


def hvp_case(oracle, qc, name):
    if name == "nonherm":      # generators that are not antisymmetric
        return random_problem(oracle, N=4, m=3, T=4, hermitian=False)
    return build_case(oracle, qc, name)


_refs = {}


def case_reference(oracle, coracle, qc, name):
    """(prob, Z, mu, H_ref, |H_ref|), computed once per case and shared by the tests that need it (read-only)."""
    if name not in _refs:
        prob, Z = hvp_case(oracle, qc, name)
        mu = mu_of(prob, 5)
        _refs[name] = (prob, Z, mu) + reference(oracle, prob, Z, mu, coracle=coracle if name.startswith("long_") else None)
    return _refs[name]


def check_product(h, H, Habs, Z, mu, seed, what):
    v = np.random.default_rng(seed).standard_normal(H.shape[0])
    w = h.hvp(Z, mu, v)
    return v, w, assert_within(w, H, Habs, v, what)


# ------------------------------------------------------------------------------------------------
#  GPU: the cases
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("path", ["fused", "generic"])
@pytest.mark.parametrize("name", HVP_CASES)
def test_cases_on_both_paths_against_the_oracle(qc, oracle, coracle, name, path):
    prob, Z, mu, H, Habs = case_reference(oracle, coracle, qc, name)
    h = Handle(qc, prob, generic=path == "generic")
    assert h.name == (PLAN_NAME if path == "fused" else "generic-hvp")
    _, w, _ = check_product(h, H, Habs, Z, mu, 7, f"{name} {path}")
    if name == "q3_T2":      # one interval: both knots are written, the last one from its left interval alone
        assert np.any(w[:prob.zdim] != 0.0) and np.any(w[prob.zdim:2 * prob.zdim] != 0.0)
    h.close()


@gpu
@pytest.mark.parametrize("name", GENERIC_CASES)
def test_generic_path_against_the_oracle(qc, oracle, coracle, name):
    prob, Z, mu, H, Habs = case_reference(oracle, coracle, qc, name)
    h = Handle(qc, prob, kernel="lds" if name == "lds_3" else "auto")
    assert h.name == "generic-hvp"
    check_product(h, H, Habs, Z, mu, 8, name)
    h.close()


@gpu
@pytest.mark.parametrize("name,generic", [("pad_3_3", False), ("pad_3_3", True), ("q3_T3", False), ("q3_T3", True), ("pade6_4", False)])
def test_layout_options_cannot_change_a_product(qc, oracle, coracle, name, generic):
    """hess_align = 16 (zero padding after each interval's values, recorded as duplicates of its first entry) and a permuted
    hess_block_order: the same bits as the default layout."""
    prob, Z, mu, H, Habs = case_reference(oracle, coracle, qc, name)
    h0 = Handle(qc, prob, generic=generic)
    v, w0, _ = check_product(h0, H, Habs, Z, mu, 9, f"{name} default layout")
    for kw in (dict(hess_align=16), dict(hess_block_order=[6, 4, 2, 0, 7, 5, 3, 1]), dict(hess_align=16, hess_block_order=[7, 1, 0, 3, 2, 5, 4, 6])):
        h1 = Handle(qc, prob, generic=generic, **kw)
        if "hess_align" in kw:
            assert h1.dims.hess_nnz_interval % 16 == 0
        np.testing.assert_array_equal(h1.hvp(Z, mu, v), w0, err_msg=str(kw))
        h1.close()
    h0.close()


@gpu
@pytest.mark.parametrize("generic", [False, True])
def test_shard_writes_every_entry_of_w(qc, oracle, generic):
    """t_range = (2, 5) of T = 8: mu is the full vector, w the whole vector, exactly +0.0 on every knot outside 2 .. 5 and on the
    global_dim tail; a full handle leaves the last knot's controls and timestep at +0.0."""
    prob, Z = deriv_problem(oracle, 2, 2, (2, 2), T=8, seed=70, global_dim=2)
    mu = mu_of(prob, 6)
    H, Habs = reference(oracle, prob, Z, mu, (2, 5))
    h = Handle(qc, prob, t_range=(2, 5), generic=generic)
    assert h.dims.Z_len == prob.n_vars
    _, w, _ = check_product(h, H, Habs, Z, mu, 10, "shard")
    zd = prob.zdim
    assert np.all(w[:2 * zd] == 0.0) and np.all(w[6 * zd:] == 0.0) and np.any(w[2 * zd:6 * zd] != 0.0)
    assert not np.signbit(w[:2 * zd]).any() and not np.signbit(w[6 * zd:]).any()
    h.close()
    full = Handle(qc, prob, generic=generic)
    Hf, Hfa = reference(oracle, prob, Z, mu)
    _, w, _ = check_product(full, Hf, Hfa, Z, mu, 11, "full")
    last = w[7 * zd:8 * zd]
    assert np.all(last[prob.off_a:prob.off_a + prob.m] == 0.0) and last[prob.off_dt] == 0.0 and np.all(w[8 * zd:] == 0.0)
    assert np.any(last[prob.off_U:prob.off_U + prob.s] != 0.0)
    full.close()


@gpu
@pytest.mark.parametrize("name,generic", [("q3_T6", False), ("kets_3", False), ("pade6_4", False), ("q3_T6", True)])
def test_symmetry(qc, oracle, coracle, name, generic):
    """u'(H v) = v'(H u) within the sum of the two derived bounds, |u|' b(v) + |v|' b(u)."""
    prob, Z, mu, H, Habs = case_reference(oracle, coracle, qc, name)
    h = Handle(qc, prob, generic=generic)
    rng = np.random.default_rng(12)
    u, v = rng.standard_normal(H.shape[0]), rng.standard_normal(H.shape[0])
    wu, wv = h.hvp(Z, mu, u), h.hvp(Z, mu, v)
    bound = float(np.abs(u) @ bound_of(Habs, v, H @ v) + np.abs(v) @ bound_of(Habs, u, H @ u))
    lhs, rhs = float(u @ wv), float(v @ wu)
    print(f"{name}: |u'(H v) - v'(H u)| / bound = {abs(lhs - rhs) / bound:.3e}")
    assert abs(lhs - rhs) <= bound
    h.close()


@gpu
@pytest.mark.parametrize("name,generic", [("q3_T6", False), ("long_1030", False), ("pad_5_7", True), ("exp_4", False)])
def test_repeated_calls_return_the_same_bits(qc, oracle, coracle, name, generic):
    prob, Z, mu, H, _ = case_reference(oracle, coracle, qc, name)
    h = Handle(qc, prob, generic=generic)
    rng = np.random.default_rng(13)
    n = H.shape[0]
    dZ, dmu, dv = torch.from_numpy(Z).cuda(), torch.from_numpy(mu).cuda(), torch.from_numpy(rng.standard_normal(n)).cuda()
    dmu2, dv2 = torch.from_numpy(rng.standard_normal(mu.size)).cuda(), torch.from_numpy(rng.standard_normal(n)).cuda()
    ws = []
    for _ in range(3):
        w = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
        h.hvp_dev(dZ, dmu, dv, w)
        ws.append(w.cpu().numpy())
        w2 = torch.zeros_like(w)      # a call into another buffer, with other vectors, in between
        h.hvp_dev(dZ, dmu2, dv2, w2)
    for k in (1, 2):
        np.testing.assert_array_equal(ws[k], ws[0])
    h.close()


# ------------------------------------------------------------------------------------------------
#  Integrator lists: the "_dev_multi" entry and ComposedQuantumDynamics against the composed oracle's symmetric product
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", ["sampling", "direct_sum"])
def test_integrator_lists(qc, oracle, kind):
    inp = list_inputs(qc, kind)
    dyn = qc.QuantumDynamics(inp.integrators, inp.traj)
    assert isinstance(dyn, qc.ComposedQuantumDynamics) and len(dyn._parts) == 2
    assert dyn.hess_product_kernel_name == PLAN_NAME
    ref = composed_oracle(inp)
    rng = np.random.default_rng(14)
    Z = inp.traj.datavec + 0.2 * rng.standard_normal(inp.traj.datavec.size)
    n = int(dyn.dims.Z_len)
    mu, v = rng.standard_normal(int(dyn.dims.n_rows)), rng.standard_normal(n)
    rows, cols = ref.hess_structure()
    H, Habs = sym_from_upper(ref.mu_d2F(Z, mu), rows, cols, n)
    # through ComposedQuantumDynamics (numpy in, numpy out) ...
    w = np.array(dyn.mu_d2F_times(Z, mu, v))
    assert_within(w, H, Habs, v, f"{kind} list")
    # ... through the C entry on device buffers, w prefilled with NaN: the first member overwrites, the second adds ...
    L = qc._lib
    dZ, dmu, dv = (torch.from_numpy(x).cuda() for x in (Z, mu, v))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    nan = lambda: torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")      # noqa: E731
    dw = nan()
    L.check(L.lib.qc_eval_hvp_dev_multi(dyn._handles, 2, p(dZ), p(dmu), p(dv), p(dw), st), dyn._parts[0][2])
    np.testing.assert_array_equal(dw.cpu().numpy(), w)
    # ... and member by member: the sum in member order, bit for bit
    parts = []
    for _, _, h, _ in dyn._parts:
        dwk = nan()
        L.check(L.lib.qc_eval_hvp_dev(h, p(dZ), p(dmu), p(dv), p(dwk), st), h)
        parts.append(dwk.cpu().numpy())
    np.testing.assert_array_equal(parts[0] + parts[1], w)
    # a list whose shared Hessian block is line-aligned (padding behind the last member's values): the same bits
    padded = qc.QuantumDynamics(inp.integrators, inp.traj, hess_align=16)
    np.testing.assert_array_equal(np.array(padded.mu_d2F_times(Z, mu, v)), w)
    padded.close()
    # repeated, a call with other vectors into another buffer in between: the same bits
    dmu2, dv2 = torch.from_numpy(rng.standard_normal(mu.size)).cuda(), torch.from_numpy(rng.standard_normal(n)).cuda()
    for _ in range(2):
        dw2 = torch.zeros_like(dw)
        L.check(L.lib.qc_eval_hvp_dev_multi(dyn._handles, 2, p(dZ), p(dmu2), p(dv2), p(dw2), st), dyn._parts[0][2])
        dw3 = nan()
        L.check(L.lib.qc_eval_hvp_dev_multi(dyn._handles, 2, p(dZ), p(dmu), p(dv), p(dw3), st), dyn._parts[0][2])
        np.testing.assert_array_equal(dw3.cpu().numpy(), w)
    dyn.close()


# ------------------------------------------------------------------------------------------------
#  Host layers
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kernel", ["auto", "lds"])
def test_host_buffer_form_equals_the_device_form(qc, oracle, kernel):
    inp = qc.config_inputs(2, T=7)
    dyn = qc.QuantumDynamics(inp.integrators, inp.traj, kernel=kernel)
    assert dyn.hess_product_kernel_name == (PLAN_NAME if kernel == "auto" else "generic-hvp")
    rng = np.random.default_rng(15)
    Z = inp.traj.datavec + 0.1 * rng.standard_normal(inp.traj.datavec.size)
    n = int(dyn.dims.Z_len)
    mu, v = rng.standard_normal(int(dyn.dims.n_rows)), rng.standard_normal(n)
    dZ, dmu, dv = (torch.from_numpy(x).cuda() for x in (Z, mu, v))
    dw = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    dyn.mu_d2F_times_device(dZ, dmu, dv, dw)
    w = np.array(dyn.mu_d2F_times(Z, mu, v, out=np.full(n, np.nan)))
    np.testing.assert_array_equal(w, dw.cpu().numpy())
    # set_new_x(False) after a call that uploaded Z: the knots on the device are used and Z is not read at all
    gen = dyn.knot_generation()
    dyn.set_new_x(False)
    garbage = np.full_like(Z, np.nan)
    np.testing.assert_array_equal(np.array(dyn.mu_d2F_times(garbage, mu, v)), w)
    assert dyn.knot_generation() == gen
    dyn.set_new_x(True)
    assert np.isnan(np.array(dyn.mu_d2F_times(garbage, mu, v))).any() and dyn.knot_generation() == gen + 1
    # against the oracle as well
    prob = problem_from_inputs(inp)
    H, Habs = reference(oracle, prob, Z, mu)
    assert_within(w, H, Habs, v, f"host buffers, kernel={kernel}")
    dyn.close()


def linear_problem(oracle):
    """No drives and a fixed timestep: the constraint is linear, hess_nnz = 0."""
    N, T = 2, 4
    n, s = 2 * N, 2 * N * N
    rng = np.random.default_rng(80)
    A = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
    prob = oracle.Problem(N=N, m=0, T=T, zdim=s, off_U=0, off_a=s, off_dt=-1, G_drift=oracle.generator((A + A.conj().T) / 2),
                          G_drives=np.zeros((0, n, n)), dt_fixed=0.17, integrator=oracle.PADE, order=4, derivs=[], ncol=0)
    return prob


@gpu
def test_refusals_carry_a_code_and_a_message(qc, oracle):
    L = qc._lib
    inp = qc.config_inputs(1, T=6)
    dyn = qc.QuantumDynamics(inp.integrators, inp.traj)
    n = int(dyn.dims.Z_len)
    buf = torch.zeros(n, dtype=torch.float64, device="cuda")
    p, host = C.c_void_p(buf.data_ptr()), np.zeros(n)
    hp = L.dptr(host)
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert L.lib.qc_eval_hvp_dev(dyn._h, *args, None) == L.QC_ERR_INVALID and L.lib.qc_last_error(dyn._h)
        hs = (C.c_void_p * 1)(dyn._h)
        assert L.lib.qc_eval_hvp_dev_multi(hs, 1, *args, None) == L.QC_ERR_INVALID and L.lib.qc_last_error(dyn._h)
    for args in ((None, hp, hp, hp), (hp, None, hp, hp), (hp, hp, None, hp), (hp, hp, hp, None)):
        assert L.lib.qc_eval_hvp(dyn._h, *args) == L.QC_ERR_INVALID and L.lib.qc_last_error(dyn._h)
    assert L.lib.qc_eval_hvp_dev(None, p, p, p, p, None) == L.QC_ERR_INVALID and L.lib.qc_last_error(None)
    assert L.lib.qc_eval_hvp_dev_multi(None, 0, p, p, p, p, None) == L.QC_ERR_INVALID and L.lib.qc_last_error(None)
    dyn.close()
    # a multi-device handle (two shards on device 0): refused
    multi = qc.QuantumDynamics(inp.integrators, inp.traj, devices=[0, 0])
    assert L.lib.qc_eval_hvp_dev(multi._h, p, p, p, p, None) == L.QC_ERR_UNSUPPORTED and L.lib.qc_last_error(multi._h)
    assert L.lib.qc_eval_hvp(multi._h, hp, hp, hp, hp) == L.QC_ERR_UNSUPPORTED and L.lib.qc_last_error(multi._h)
    hs = (C.c_void_p * 1)(multi._h)
    assert L.lib.qc_eval_hvp_dev_multi(hs, 1, p, p, p, p, None) == L.QC_ERR_UNSUPPORTED and L.lib.qc_last_error(multi._h)
    with pytest.raises(qc.QCollocError) as e:
        multi.mu_d2F_times(host, np.zeros(int(multi.dims.n_rows)), host)
    assert e.value.code == L.QC_ERR_UNSUPPORTED and str(e.value)
    multi.close()
    # a handle without an analytic Hessian (hess_nnz = 0) ...
    lin = Handle(qc, linear_problem(oracle))
    assert lin.dims.hess_nnz == 0
    assert L.lib.qc_eval_hvp_dev(lin.h, p, p, p, p, None) == L.QC_ERR_UNSUPPORTED and b"Hessian" in L.lib.qc_last_error(lin.h)
    assert L.lib.qc_eval_hvp(lin.h, hp, hp, hp, hp) == L.QC_ERR_UNSUPPORTED and b"Hessian" in L.lib.qc_last_error(lin.h)
    hs = (C.c_void_p * 1)(lin.h)
    assert L.lib.qc_eval_hvp_dev_multi(hs, 1, p, p, p, p, None) == L.QC_ERR_UNSUPPORTED and b"Hessian" in L.lib.qc_last_error(lin.h)
    lin.close()
    # ... and dynamics built with eval_hessian=False
    nohess = qc.QuantumDynamics(inp.integrators, inp.traj, eval_hessian=False)
    with pytest.raises(qc.QCollocError) as e:
        nohess.mu_d2F_times(host, np.zeros(int(nohess.dims.n_rows)), host)
    assert e.value.code == L.QC_ERR_UNSUPPORTED and str(e.value)
    with pytest.raises(qc.QCollocError) as e:
        nohess.mu_d2F_times_device(buf, buf, buf, buf)
    assert e.value.code == L.QC_ERR_UNSUPPORTED
    nohess.close()


@gpu
def test_kernel_names(qc, oracle, coracle):
    """A 3-qubit order-4 handle reports what the plan chose; an order-6 handle and the forced-generic handle report "generic-hvp"."""
    L = qc._lib
    q3 = qc.QuantumDynamics(*(lambda i: (i.integrators, i.traj))(qc.config_inputs(3, T=5)))
    assert L.lib.qc_kernel_name(q3._h, 5) == PLAN_NAME.encode() and q3.hess_product_kernel_name == PLAN_NAME
    assert q3.product_kernel_names[0] == "mfma16-pade4-jvp"      # (a handle the fused Jacobian-product kernel serves)
    q3.close()
    prob = case_reference(oracle, coracle, qc, "pade6_4")[0]
    h = Handle(qc, prob)
    assert h.name == "generic-hvp"
    h.close()
    prob = case_reference(oracle, coracle, qc, "q3_T3")[0]
    h = Handle(qc, prob, generic=True)
    assert h.name == "generic-hvp" and h.L.lib.qc_kernel_name(h.h, 3) == b"generic-jvp"
    h.close()


@gpu
def test_evaluator_product_equals_the_lagrangian_hessian_times_the_vector(qc):
    """QuantumControlEvaluator on the 1-qubit problem with an infidelity objective, regularisers and a nonlinear constraint behind the
    dynamics rows, against its own assembled matrix: hessian_lagrangian_matrix(x, sigma, mu) @ v, with the bound of this file computed
    from that matrix."""
    inp = qc.config_inputs(1, T=8)
    traj = inp.traj
    dyn = qc.QuantumDynamics(inp.integrators, traj)
    obj = qc.UnitaryInfidelityObjective("Ũ⃗", traj, Q=100.0)
    reg = qc.TrajectoryObjective(qc.QuadraticRegularizer("a", traj, 1e-2) + qc.QuadraticRegularizer("da", traj, 1e-2)
                                 + qc.QuadraticRegularizer("dda", traj, 1e-2), traj)
    con = qc.FinalUnitaryFidelityConstraint("Ũ⃗", 0.9, traj)
    ev = qc.QuantumControlEvaluator(dyn, [obj, reg], [con])
    rng = np.random.default_rng(16)
    x = traj.datavec + 0.1 * rng.standard_normal(traj.datavec.size)
    sigma, mu, v = 0.7, rng.standard_normal(ev.n_constraints), rng.standard_normal(ev.n_variables)
    H = ev.hessian_lagrangian_matrix(x, sigma, mu).tocsr()
    Habs = abs(H)
    w = ev.hessian_lagrangian_times(x, sigma, mu, v)
    assert w.shape == (ev.n_variables,)
    assert_within(w, H, Habs, v, "evaluator")
    # every part took part: the product differs from the dynamics' part alone on the final state (objective, constraint) and the controls
    wd = np.array(dyn.mu_d2F_times(x, mu[:ev.n_dynamics_rows], v))
    assert np.any(w[obj.state_indices] != wd[obj.state_indices]) and np.count_nonzero(w != wd) > obj.state_indices.size
    quasi = qc.QuantumControlEvaluator(dyn, [obj, reg], [con], eval_hessian=False)
    with pytest.raises(RuntimeError):
        quasi.hessian_lagrangian_times(x, sigma, mu, v)
    for o in (con, obj, reg, dyn):
        o.close()


# ------------------------------------------------------------------------------------------------
#  CPU
# ------------------------------------------------------------------------------------------------
def test_prototypes_exist_and_nothing_crashes_without_a_handle(qc):
    L = qc._lib
    names = ("qc_eval_hvp_dev", "qc_eval_hvp", "qc_eval_hvp_dev_multi")
    for name in names:
        assert name in L.SYMBOLS and getattr(L.lib, name).argtypes == L.SYMBOLS[name][1]
    x = np.zeros(4)
    assert L.lib.qc_eval_hvp(None, L.dptr(x), L.dptr(x), L.dptr(x), L.dptr(x)) == L.QC_ERR_INVALID
    assert b"NULL handle" in L.lib.qc_last_error(None)
    p = C.c_void_p(x.ctypes.data)
    assert L.lib.qc_eval_hvp_dev(None, p, p, p, p, None) == L.QC_ERR_INVALID and b"NULL handle" in L.lib.qc_last_error(None)
    assert L.lib.qc_eval_hvp_dev_multi(None, 0, p, p, p, p, None) == L.QC_ERR_INVALID and L.lib.qc_last_error(None)
    hs = (C.c_void_p * 1)(None)
    assert L.lib.qc_eval_hvp_dev_multi(hs, 1, p, p, p, p, None) == L.QC_ERR_INVALID and b"NULL handle" in L.lib.qc_last_error(None)
    assert L.lib.qc_kernel_name(None, 5) == L.lib.qc_kernel_name(None, 3) == L.lib.qc_kernel_name(None, 4) == b"none"
    for meth in ("mu_d2F_times", "mu_d2F_times_device"):
        assert callable(getattr(qc.QuantumDynamics, meth)) and callable(getattr(qc.ComposedQuantumDynamics, meth))
        assert getattr(qc.ComposedQuantumDynamics, meth) is not getattr(qc.QuantumDynamics, meth)      # (the list form is its own)
    assert isinstance(qc.QuantumDynamics.hess_product_kernel_name, property)
    assert callable(qc.QuantumControlEvaluator.hessian_lagrangian_times)


def test_julia_glue_declares_the_product():
    """mu_d2F_mul! exists in julia/QCollocHIP.jl and calls the host entry (its ccall signature is checked against the header by
    tests/test_abi.py::test_julia_ccalls_match_the_header)."""
    import test_abi
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "julia", "QCollocHIP.jl"), encoding="utf-8").read()
    assert "function mu_d2F_mul!(" in txt and "(:qc_eval_hvp, LIB[])" in txt
    test_abi.test_julia_ccalls_match_the_header()


def test_reference_construction_agrees_with_the_dense_symmetric_matrix(oracle):
    """U + U' - diag(U) @ v against oracle.dense_from_coo(..., symmetric=True) @ v (the reference's `dense`, test_utils.jl:14-27) on a
    small problem, with the alignment padding (zero duplicates of the first entry) in the structure: summation rounding only."""
    prob, Z = random_problem(oracle, N=2, m=2, T=4, seed=3)
    prob.hess_align = 16
    mu = mu_of(prob, 4)
    vals = oracle.mu_d2F(prob, Z, mu)
    rows, cols = oracle.hess_structure(prob)
    assert vals.size == rows.size and oracle.hess_pad(prob) > 0
    H, Habs = sym_from_upper(vals, rows, cols, prob.n_vars)
    D = oracle.dense_from_coo(vals, rows, cols, (prob.n_vars, prob.n_vars), symmetric=True)
    np.testing.assert_array_equal(D, D.T)
    v = np.random.default_rng(5).standard_normal(prob.n_vars)
    assert np.all(np.abs(H @ v - D @ v) <= 1e-14 * (np.abs(D) @ np.abs(v)))
    assert np.all((Habs @ np.abs(v) == 0.0) == (np.abs(D) @ np.abs(v) == 0.0))


@pytest.mark.parametrize("hermitian", [True, False])
def test_fused_kernel_formulas_agree_with_the_oracle(oracle, hermitian):
    """The per-interval formulas of the withdrawn fused kernel (kept for the next attempt), restated in numpy
    matrix by matrix, against the oracle's symmetric product within the bound of this file -- for antisymmetric generators and for
    generators that are not (the formulas use G' and Gv', never -G)."""
    prob, Z = random_problem(oracle, N=3, m=2, T=3, seed=1, hermitian=hermitian)
    mu = mu_of(prob, 2)
    H, Habs = reference(oracle, prob, Z, mu)
    v = np.random.default_rng(3).standard_normal(prob.n_vars)
    n, nc, s, m, zd = 2 * prob.N, prob.N, prob.s, prob.m, prob.zdim
    c1, c2 = 0.5, 1.0 / 12.0
    w = np.zeros(prob.n_vars)
    for t in range(prob.T - 1):
        z0, z1, v0, v1 = Z[t * zd:(t + 1) * zd], Z[(t + 1) * zd:(t + 2) * zd], v[t * zd:(t + 1) * zd], v[(t + 1) * zd:(t + 2) * zd]
        mut = mu[t * prob.row_stride:(t + 1) * prob.row_stride]
        mat = lambda x: x[prob.off_U:prob.off_U + s].reshape(nc, n).T      # noqa: E731
        U0, U1, X0, X1, M = mat(z0), mat(z1), mat(v0), mat(v1), mut[:s].reshape(nc, n).T
        a, al = z0[prob.off_a:prob.off_a + m], v0[prob.off_a:prob.off_a + m]
        h, eta = z0[prob.off_dt], v0[prob.off_dt]
        G, Gv = prob.G_drift + np.tensordot(a, prob.G_drives, 1), np.tensordot(al, prob.G_drives, 1)
        S, D, Sv, Dv = U1 + U0, U1 - U0, X1 + X0, X1 - X0
        K1, K2 = G.T @ M, Gv.T @ M
        lin, quad = c1 * (h * K2 + eta * K1), c2 * (h * h * (G.T @ K2 + Gv.T @ K1) + 2 * h * eta * G.T @ K1)
        R = -c1 * (h * Sv + eta * S) + c2 * h * h * (G @ Dv + Gv @ D) + 2 * c2 * h * eta * G @ D
        Q, Q2 = c2 * h * (h * Dv + 2 * eta * D), c2 * h * h * D
        W = M @ R.T + K1 @ Q.T + K2 @ Q2.T
        wh = -c1 * np.sum(M * (G @ Sv + Gv @ S)) + 2 * c2 * (h * np.sum(K1 * (G @ Dv + Gv @ D)) + h * np.sum(K2 * (G @ D)) + eta * np.sum(K1 * (G @ D)))
        b0, b1 = t * zd, (t + 1) * zd
        w[b1 + prob.off_U:b1 + prob.off_U + s] += (-lin + quad).T.reshape(-1)
        w[b0 + prob.off_U:b0 + prob.off_U + s] += (-lin - quad).T.reshape(-1)
        w[b0 + prob.off_a:b0 + prob.off_a + m] += [np.sum(Gk * W) for Gk in prob.G_drives]
        r0 = s
        for d in prob.derivs:
            mx = mut[r0:r0 + d.dim]
            w[b0 + d.dx_off:b0 + d.dx_off + d.dim] += -mx * eta
            wh += -np.sum(mx * v0[d.dx_off:d.dx_off + d.dim])
            r0 += d.dim
        w[b0 + prob.off_dt] += wh
    assert_within(w, H, Habs, v, f"formulas, hermitian={hermitian}")
