"""Matrix-free Jacobian products of the dynamics, y = dF(Z) v and w = dF(Z)' lam (qc_eval_jvp / qc_eval_vjp and their device, list and
host-layer forms), against the CPU oracle.

Reference: J_ref = coo_matrix((oracle.dF(prob, Z), oracle.jac_structure(prob))), y_ref = J_ref @ v, w_ref = J_ref.T @ lam in float64
(the C restatement of the oracle where the trajectory is long), never the library's own Jacobian.

Tolerance (derived, not chosen): the project's parity contract is 1e-10 relative per Jacobian entry (tests/test_gpu_parity.py, RTOL),
so a sum of such terms obeys
    |y - y_ref|_i <= 1e-10 (|J_ref| |v|)_i + 1e-12 max|y_ref|,      |w - w_ref|_i <= 1e-10 (|J_ref|' |lam|)_i + 1e-12 max|w_ref|
with the bound computed from J_ref.  The fused kernels and the generic path (the same handle created under QC_NO_PRODUCT_MFMA=1) meet
the same bound, so they agree within twice it.  Every call prefills its output: y with a sentinel (rows without a structural entry must
keep it), w with NaN (every entry must be written; entries without a structural entry must be exactly 0.0).

The fused forward kernel runs one workgroup per interval on a grid of at most 1024 workgroups (kMaxGrid, qc_mfma_products.hip) and loops
beyond it: T = 1030 is the first pass plus a few, T = 2051 is past two full passes.  (The generic transposed kernel runs one workgroup
per knot without a limit.)"""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from oracle_bridge import composed_oracle, problem_from_inputs, random_problem

gpu = pytest.mark.gpu
SENTINEL = -7.25e33
# What a handle that the fused kernels serve runs on.  The forward product has its fused kernel; the transposed product's fused kernel
# missed the issue's condition on the device (profiles/products_summary.txt) and, as the issue rules for that case, is not shipped:
# dF' lam runs the generic path on every handle, and "fused" below means "the handle as the plan serves it".
FUSED_NAMES = ("mfma16-pade4-jvp", "generic-vjp")


# ------------------------------------------------------------------------------------------------
#  Handles straight from an oracle Problem (raw C descriptor), with every descriptor field the cases vary
# ------------------------------------------------------------------------------------------------
class Handle:
    def __init__(self, qc, prob, *, kernel="auto", t_range=None, generic=False, jac_block_order=None):
        self.qc, self.L = qc, qc._lib
        L = self.L
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
        if jac_block_order is not None:
            for i, x in enumerate(jac_block_order):
                d.jac_block_order[i] = x
        if t_range:
            d.t_begin, d.t_end = t_range
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
        self._keep = (G0, Gd)

    @property
    def names(self):
        return self.L.lib.qc_kernel_name(self.h, 3).decode(), self.L.lib.qc_kernel_name(self.h, 4).decode()

    def jvp_dev(self, dZ, dv, dy):
        self.L.check(self.L.lib.qc_eval_jvp_dev(self.h, C.c_void_p(dZ.data_ptr()), C.c_void_p(dv.data_ptr()), C.c_void_p(dy.data_ptr()),
                                                C.c_void_p(torch.cuda.current_stream().cuda_stream)), self.h)

    def vjp_dev(self, dZ, dl, dw):
        self.L.check(self.L.lib.qc_eval_vjp_dev(self.h, C.c_void_p(dZ.data_ptr()), C.c_void_p(dl.data_ptr()), C.c_void_p(dw.data_ptr()),
                                                C.c_void_p(torch.cuda.current_stream().cuda_stream)), self.h)

    def jvp(self, Z, v):
        dy = torch.full((int(self.dims.F_len),), SENTINEL, dtype=torch.float64, device="cuda")
        self.jvp_dev(torch.from_numpy(Z).cuda(), torch.from_numpy(v).cuda(), dy)
        return dy.cpu().numpy()

    def vjp(self, Z, lam):
        dw = torch.full((int(self.dims.Z_len),), float("nan"), dtype=torch.float64, device="cuda")
        self.vjp_dev(torch.from_numpy(Z).cuda(), torch.from_numpy(lam).cuda(), dw)
        return dw.cpu().numpy()

    def close(self):
        self.L.lib.qc_destroy(self.h)


def reference(oracle, prob, Z, t_range=None, coracle=None):
    """J_ref of the handle's intervals as a CSR matrix (rows of the handle's slice) and |J_ref|."""
    t0, t1 = t_range if t_range else (0, prob.T - 1)
    vals = coracle.COracle(prob).F_dF(Z, t0, t1, want_F=False)[1] if coracle is not None else oracle.dF(prob, Z, t0, t1)
    rows, cols = oracle.jac_structure(prob, t_begin=t0, t_end=t1)
    shape = ((t1 - t0) * prob.row_stride, prob.n_vars)
    J = sp.coo_matrix((vals, (rows - t0 * prob.row_stride, cols)), shape=shape).tocsr()
    return J, abs(J)


def check_products(h, J, Jabs, Z, seed, what):
    """Both products of handle `h` against J within the derived bound; returns (v, lam, y, w)."""
    rng = np.random.default_rng(seed)
    v, lam = rng.standard_normal(J.shape[1]), rng.standard_normal(J.shape[0])
    y, w = h.jvp(Z, v), h.vjp(Z, lam)
    y_ref, w_ref = J @ v, J.T @ lam
    own_row = np.asarray(Jabs.sum(axis=1)).ravel() > 0
    np.testing.assert_array_equal(y[~own_row], SENTINEL, err_msg=f"{what}: a row no integrator owns was written")
    ey, by = np.abs(y - y_ref)[own_row], (1e-10 * (Jabs @ np.abs(v)) + 1e-12 * np.abs(y_ref).max())[own_row]
    print(f"{what}: dF v   max err / bound = {np.max(ey / by):.3e}")
    assert np.all(ey <= by), f"{what}: dF v misses the bound by up to {np.max(ey / by):.3g} x"
    assert np.isfinite(w).all(), f"{what}: {np.count_nonzero(~np.isfinite(w))} entries of w were not written"
    touched = np.asarray(Jabs.sum(axis=0)).ravel() > 0
    assert np.all(w[~touched] == 0.0) and not np.signbit(w[~touched]).any(), f"{what}: untouched variables must be exactly 0.0"
    ew, bw = np.abs(w - w_ref), 1e-10 * (Jabs.T @ np.abs(lam)) + 1e-12 * np.abs(w_ref).max()
    print(f"{what}: dF' lam max err / bound = {np.max(ew / bw):.3e}")
    assert np.all(ew <= bw), f"{what}: dF' lam misses the bound by up to {np.max(ew / bw):.3g} x"
    return v, lam, y, w


# ------------------------------------------------------------------------------------------------
#  The cases
# ------------------------------------------------------------------------------------------------
def deriv_problem(oracle, N, m, dims, T=4, seed=0, global_dim=0):
    """[U, a, then (x, dx) pairs chained where the dimension allows, dt]: any number of derivative integrators."""
    rng = np.random.default_rng(seed)
    n, s = 2 * N, 2 * N * N
    A = lambda: (lambda X: (X + X.conj().T) / 2)(rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N)))   # noqa: E731
    G0 = oracle.generator(A())
    Gd = np.array([oracle.generator(A()) for _ in range(m)]).reshape(m, n, n)
    off, derivs, prev_off, prev_dim = s + m, [], s, m
    for d in dims:
        if d == prev_dim:
            x_off = prev_off
        else:
            x_off = off
            off += d
        derivs.append(oracle.DerivSpec(x_off, off, d))
        prev_off, prev_dim = off, d
        off += d
    zdim = off + 1
    prob = oracle.Problem(N=N, m=m, T=T, zdim=zdim, off_U=0, off_a=s, off_dt=zdim - 1, G_drift=G0, G_drives=Gd, dt_fixed=0.17,
                          integrator=oracle.PADE, order=4, derivs=derivs, ncol=0, global_dim=global_dim)
    Z = rng.standard_normal(zdim * T + global_dim) * 0.5
    Z[zdim - 1:zdim * T:zdim] = rng.uniform(0.1, 0.3, size=T)
    return prob, Z


def by_component_problem(oracle):
    """Rows at their state component's position with gaps: rows 0-1, 10-12 and the last two of 21 belong to no integrator."""
    prob, Z = random_problem(oracle, N=2, m=3, T=5, seed=21)
    s = prob.s
    prob.rows_per_interval, prob.row_offset, prob.deriv_rows = s + 2 * 3 + 7, 2, [2 + s + 3, 2 + s + 3 + 3 + 0]
    return prob, Z


def build_case(oracle, qc, name):
    rp = lambda **kw: random_problem(oracle, **kw)      # noqa: E731
    if name.startswith("q3_T"):                          # 3 qubits, free timestep, two derivative integrators
        return rp(N=8, m=6, T=int(name[4:]), seed=31)
    if name == "q3_fixed":
        return rp(N=8, m=6, T=4, free_time=False, seed=32)
    if name.startswith("pad_"):                          # zero-padded tiles
        N, m = map(int, name[4:].split("_"))
        return rp(N=N, m=m, T=4, seed=40 + N)
    if name.startswith("kets_"):
        return rp(N=4, m=3, T=4, ncol=int(name[5:]), seed=45)
    if name.startswith("long_"):                         # past the persistent-grid limit of 1024 workgroups
        return rp(N=2, m=2, T=int(name[5:]), seed=50)
    if name == "shuffled":
        return rp(N=2, m=3, T=5, layout="shuffled", seed=51)
    if name == "by_component":
        return by_component_problem(oracle)
    if name == "global_dim":
        return deriv_problem(oracle, 3, 2, (2, 2), T=4, seed=52, global_dim=3)
    if name.startswith("derivs_"):
        dims = {0: (), 1: (None,), 3: (None, None, None), 5: (3, None, 65, None, 1)}[int(name[7:])]
        return deriv_problem(oracle, 4, 3, [3 if d is None else d for d in dims], T=3, seed=53)
    # ---- the generic path only ----
    if name.startswith("exp_"):
        return rp(N=int(name[4:]), m=2, T=4, integrator=oracle.EXPONENTIAL, seed=60)
    if name == "pade6_4":
        return rp(N=4, m=2, T=4, order=6, seed=61)
    if name == "pade12_2":
        return rp(N=2, m=2, T=4, order=12, seed=62)
    if name == "pade4_16":
        return rp(N=16, m=2, T=4, seed=63)
    if name == "pade4_20":
        return rp(N=20, m=2, T=3, seed=64)
    if name == "lds_3":
        return rp(N=3, m=2, T=4, seed=65)
    if name == "density":
        import test_density
        inp = qc.density_operator_smooth_pulse_inputs(test_density.open_system(qc, 1), np.eye(2) / 2, np.array([0.6, 0.8j]), 5)
        rng = np.random.default_rng(66)
        return problem_from_inputs(inp), inp.traj.datavec + 0.3 * rng.standard_normal(inp.traj.datavec.size)
    raise ValueError(name)


FUSED_CASES = ["q3_T2", "q3_T3", "q3_T6", "q3_fixed", "pad_2_2", "pad_3_3", "pad_5_7", "kets_1", "kets_3", "long_1030", "long_2051",
               "shuffled", "by_component", "global_dim", "derivs_0", "derivs_1", "derivs_3", "derivs_5"]
GENERIC_CASES = ["exp_2", "exp_4", "pade6_4", "pade12_2", "pade4_16", "pade4_20", "lds_3", "density"]
_refs = {}


def case_reference(oracle, coracle, qc, name):
    """(prob, Z, J_ref, |J_ref|), computed once per case and shared by the tests that need it (read-only)."""
    if name not in _refs:
        prob, Z = build_case(oracle, qc, name)
        _refs[name] = (prob, Z) + reference(oracle, prob, Z, coracle=coracle if name.startswith("long_") else None)
    return _refs[name]


@gpu
@pytest.mark.parametrize("path", ["fused", "generic"])
@pytest.mark.parametrize("name", FUSED_CASES)
def test_fused_cases_on_both_paths_against_the_oracle(qc, oracle, coracle, name, path):
    prob, Z, J, Jabs = case_reference(oracle, coracle, qc, name)
    h = Handle(qc, prob, generic=path == "generic")
    assert h.names == (FUSED_NAMES if path == "fused" else ("generic-jvp", "generic-vjp"))
    check_products(h, J, Jabs, Z, 7, f"{name} {path}")
    h.close()


@gpu
@pytest.mark.parametrize("name", GENERIC_CASES)
def test_generic_path_against_the_oracle(qc, oracle, coracle, name):
    prob, Z, J, Jabs = case_reference(oracle, coracle, qc, name)
    h = Handle(qc, prob, kernel="lds" if name == "lds_3" else "auto")
    assert h.names == ("generic-jvp", "generic-vjp")
    check_products(h, J, Jabs, Z, 8, name)
    h.close()


@gpu
@pytest.mark.parametrize("name,generic", [("pad_3_3", False), ("pad_3_3", True), ("pade6_4", False)])
def test_block_order_cannot_change_a_product(qc, oracle, coracle, name, generic):
    prob, Z, J, Jabs = case_reference(oracle, coracle, qc, name)
    h0, h1 = Handle(qc, prob, generic=generic), Handle(qc, prob, generic=generic, jac_block_order=[4, 2, 0, 3, 1])
    v, lam, y1, w1 = check_products(h1, J, Jabs, Z, 9, f"{name} shuffled blocks")
    np.testing.assert_array_equal(h0.jvp(Z, v), y1)      # the same sums in the same order: bit for bit
    np.testing.assert_array_equal(h0.vjp(Z, lam), w1)
    h0.close()
    h1.close()


@gpu
@pytest.mark.parametrize("generic", [False, True])
def test_shard_writes_every_entry_of_w(qc, oracle, generic):
    """t_range = (2, 5) of T = 8: y and lam are the shard's rows, w is the whole vector, exactly 0.0 on every knot outside 2 .. 5,
    on the last knot's controls (dda: no interval reads them) and timestep of a full handle, and on the global_dim tail."""
    prob, Z = deriv_problem(oracle, 2, 2, (2, 2), T=8, seed=70, global_dim=2)
    J, Jabs = reference(oracle, prob, Z, (2, 5))
    h = Handle(qc, prob, t_range=(2, 5), generic=generic)
    assert h.dims.F_len == 3 * prob.ddim and h.dims.Z_len == prob.n_vars
    _, _, _, w = check_products(h, J, Jabs, Z, 10, "shard")
    zd = prob.zdim
    assert np.all(w[:2 * zd] == 0.0) and np.all(w[6 * zd:] == 0.0) and np.any(w[2 * zd:6 * zd] != 0.0)
    h.close()
    full = Handle(qc, prob, generic=generic)
    Jf, Jfa = reference(oracle, prob, Z)
    _, _, _, w = check_products(full, Jf, Jfa, Z, 11, "full")
    last = w[7 * zd:8 * zd]
    ctrl = prob.derivs[-1]      # the trajectory's control component (dda): dx of the last integrator, x of none
    assert np.all(last[ctrl.dx_off:ctrl.dx_off + ctrl.dim] == 0.0) and last[prob.off_dt] == 0.0 and np.all(w[8 * zd:] == 0.0)
    assert np.any(last[prob.off_U:prob.off_U + prob.s] != 0.0)
    full.close()


@gpu
@pytest.mark.parametrize("name,generic", [("q3_T6", False), ("kets_3", False), ("pade6_4", False), ("q3_T6", True)])
def test_adjoint_identity(qc, oracle, coracle, name, generic):
    prob, Z, J, Jabs = case_reference(oracle, coracle, qc, name)
    h = Handle(qc, prob, generic=generic)
    rng = np.random.default_rng(12)
    v, lam = rng.standard_normal(J.shape[1]), rng.standard_normal(J.shape[0])
    y, w = h.jvp(Z, v), h.vjp(Z, lam)
    own = np.asarray(Jabs.sum(axis=1)).ravel() > 0
    lhs, rhs = float(lam[own] @ y[own]), float(w @ v)
    bound = 1e-12 * float(np.abs(lam) @ (Jabs @ np.abs(v)))
    print(f"{name}: |lam'(dF v) - (dF' lam)'v| / bound = {abs(lhs - rhs) / bound:.3e}")
    assert abs(lhs - rhs) <= bound
    h.close()


@gpu
@pytest.mark.parametrize("name,generic", [("q3_T6", False), ("long_1030", False), ("pad_5_7", True), ("exp_4", False)])
def test_repeated_calls_return_the_same_bits(qc, oracle, coracle, name, generic):
    prob, Z, J, _ = case_reference(oracle, coracle, qc, name)
    h = Handle(qc, prob, generic=generic)
    rng = np.random.default_rng(13)
    dZ = torch.from_numpy(Z).cuda()
    dv, dl = torch.from_numpy(rng.standard_normal(J.shape[1])).cuda(), torch.from_numpy(rng.standard_normal(J.shape[0])).cuda()
    dv2, dl2 = torch.from_numpy(rng.standard_normal(J.shape[1])).cuda(), torch.from_numpy(rng.standard_normal(J.shape[0])).cuda()
    ys, ws = [], []
    for _ in range(3):
        y, w = torch.zeros(J.shape[0], dtype=torch.float64, device="cuda"), torch.zeros(J.shape[1], dtype=torch.float64, device="cuda")
        h.jvp_dev(dZ, dv, y)
        h.vjp_dev(dZ, dl, w)
        ys.append(y.cpu().numpy())
        ws.append(w.cpu().numpy())
        y2, w2 = torch.zeros_like(y), torch.zeros_like(w)      # a call into another buffer, with other vectors, in between
        h.jvp_dev(dZ, dv2, y2)
        h.vjp_dev(dZ, dl2, w2)
    for k in (1, 2):
        np.testing.assert_array_equal(ys[k], ys[0])
        np.testing.assert_array_equal(ws[k], ws[0])
    h.close()


# ------------------------------------------------------------------------------------------------
#  Integrator lists: the "_dev_multi" entries and ComposedQuantumDynamics against the oracle's stacked Jacobian
# ------------------------------------------------------------------------------------------------
def list_inputs(qc, kind):
    s1 = qc.multi_qubit_system(1)
    if kind == "sampling":
        systems = [qc.QuantumSystem(0.3 * qc.PAULIS["Z"], s1.H_drives), qc.QuantumSystem(-0.3 * qc.PAULIS["Z"], s1.H_drives)]
        return qc.unitary_sampling_inputs(systems, qc.GATES["H"], 6)
    return qc.unitary_direct_sum_inputs([qc.unitary_smooth_pulse_inputs(s1, qc.GATES["X"], 6, free_time=False),
                                         qc.unitary_smooth_pulse_inputs(s1, qc.GATES["Y"], 6, free_time=False, seed=9)])


@gpu
@pytest.mark.parametrize("kind", ["sampling", "direct_sum"])
def test_integrator_lists(qc, oracle, kind):
    inp = list_inputs(qc, kind)
    dyn = qc.QuantumDynamics(inp.integrators, inp.traj)
    assert isinstance(dyn, qc.ComposedQuantumDynamics) and len(dyn._parts) == 2
    assert dyn.product_kernel_names == FUSED_NAMES
    ref = composed_oracle(inp)
    rng = np.random.default_rng(14)
    Z = inp.traj.datavec + 0.2 * rng.standard_normal(inp.traj.datavec.size)
    rows, cols = ref.structure()
    J = sp.coo_matrix((ref.dF(Z), (rows, cols)), shape=(int(dyn.dims.F_len), int(dyn.dims.Z_len))).tocsr()
    Jabs = abs(J)
    v, lam = rng.standard_normal(J.shape[1]), rng.standard_normal(J.shape[0])
    y_ref, w_ref = J @ v, J.T @ lam
    by = 1e-10 * (Jabs @ np.abs(v)) + 1e-12 * np.abs(y_ref).max()
    bw = 1e-10 * (Jabs.T @ np.abs(lam)) + 1e-12 * np.abs(w_ref).max()
    # through ComposedQuantumDynamics (numpy in, numpy out) ...
    y, w = dyn.dF_times(Z, v), dyn.dFT_times(Z, lam)
    assert np.all(np.abs(y - y_ref) <= by) and np.all(np.abs(w - w_ref) <= bw)
    # ... and through the C entries on device buffers, w prefilled with NaN: the first member overwrites, the second adds
    L = qc._lib
    dZ, dv, dl = (torch.from_numpy(x).cuda() for x in (Z, v, lam))
    dy = torch.full((J.shape[0],), SENTINEL, dtype=torch.float64, device="cuda")
    dw = torch.full((J.shape[1],), float("nan"), dtype=torch.float64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    L.check(L.lib.qc_eval_jvp_dev_multi(dyn._handles, 2, p(dZ), p(dv), p(dy), st), dyn._parts[0][2])
    L.check(L.lib.qc_eval_vjp_dev_multi(dyn._handles, 2, p(dZ), p(dl), p(dw), st), dyn._parts[0][2])
    np.testing.assert_array_equal(dy.cpu().numpy(), y)
    np.testing.assert_array_equal(dw.cpu().numpy(), w)
    # each entry three times, a call with other vectors into another buffer in between: the same bits
    dv2, dl2 = torch.from_numpy(rng.standard_normal(J.shape[1])).cuda(), torch.from_numpy(rng.standard_normal(J.shape[0])).cuda()
    for _ in range(2):
        dy2, dw2 = torch.zeros_like(dy), torch.zeros_like(dw)
        L.check(L.lib.qc_eval_jvp_dev_multi(dyn._handles, 2, p(dZ), p(dv2), p(dy2), st), dyn._parts[0][2])
        L.check(L.lib.qc_eval_vjp_dev_multi(dyn._handles, 2, p(dZ), p(dl2), p(dw2), st), dyn._parts[0][2])
        dy3 = torch.full_like(dy, SENTINEL)
        dw3 = torch.full_like(dw, float("nan"))
        L.check(L.lib.qc_eval_jvp_dev_multi(dyn._handles, 2, p(dZ), p(dv), p(dy3), st), dyn._parts[0][2])
        L.check(L.lib.qc_eval_vjp_dev_multi(dyn._handles, 2, p(dZ), p(dl), p(dw3), st), dyn._parts[0][2])
        np.testing.assert_array_equal(dy3.cpu().numpy(), y)
        np.testing.assert_array_equal(dw3.cpu().numpy(), w)
    dyn.close()


# ------------------------------------------------------------------------------------------------
#  Host layers
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kernel", ["auto", "lds"])
def test_host_buffer_forms_equal_the_device_forms(qc, oracle, kernel):
    inp = qc.config_inputs(2, T=7)
    dyn = qc.QuantumDynamics(inp.integrators, inp.traj, kernel=kernel)
    assert dyn.product_kernel_names == (FUSED_NAMES if kernel == "auto" else ("generic-jvp", "generic-vjp"))
    rng = np.random.default_rng(15)
    Z = inp.traj.datavec + 0.1 * rng.standard_normal(inp.traj.datavec.size)
    v, lam = rng.standard_normal(int(dyn.dims.Z_len)), rng.standard_normal(int(dyn.dims.F_len))
    dZ, dv, dl = (torch.from_numpy(x).cuda() for x in (Z, v, lam))
    dy, dw = torch.empty(lam.size, dtype=torch.float64, device="cuda"), torch.empty(v.size, dtype=torch.float64, device="cuda")
    dyn.dF_times_device(dZ, dv, dy)
    dyn.dFT_times_device(dZ, dl, dw)
    y, w = dyn.dF_times(Z, v), dyn.dFT_times(Z, lam)
    np.testing.assert_array_equal(y, dy.cpu().numpy())
    np.testing.assert_array_equal(w, dw.cpu().numpy())
    # set_new_x(False): the knots on the device are used and Z is not read at all
    gen = dyn.knot_generation()
    dyn.set_new_x(False)
    garbage = np.full_like(Z, np.nan)
    np.testing.assert_array_equal(dyn.dF_times(garbage, v), y)
    np.testing.assert_array_equal(dyn.dFT_times(garbage, lam), w)
    assert dyn.knot_generation() == gen
    dyn.set_new_x(True)
    assert np.isnan(dyn.dF_times(garbage, v)).any() and dyn.knot_generation() == gen + 1
    # against the oracle as well
    prob = problem_from_inputs(inp)
    J, Jabs = reference(oracle, prob, Z)
    assert np.all(np.abs(y - J @ v) <= 1e-10 * (Jabs @ np.abs(v)) + 1e-12 * np.abs(J @ v).max())
    assert np.all(np.abs(w - J.T @ lam) <= 1e-10 * (Jabs.T @ np.abs(lam)) + 1e-12 * np.abs(J.T @ lam).max())
    dyn.close()


@gpu
def test_refusals_carry_a_code_and_a_message(qc):
    L = qc._lib
    inp = qc.config_inputs(1, T=6)
    dyn = qc.QuantumDynamics(inp.integrators, inp.traj)
    n = int(dyn.dims.Z_len)
    buf = torch.zeros(n, dtype=torch.float64, device="cuda")
    p, host = C.c_void_p(buf.data_ptr()), np.zeros(n)
    for fn in (L.lib.qc_eval_jvp_dev, L.lib.qc_eval_vjp_dev):
        for args in ((None, p, p), (p, None, p), (p, p, None)):
            assert fn(dyn._h, *args, None) == L.QC_ERR_INVALID and L.lib.qc_last_error(dyn._h)
        assert fn(None, p, p, p, None) == L.QC_ERR_INVALID and L.lib.qc_last_error(None)
    for fn in (L.lib.qc_eval_jvp, L.lib.qc_eval_vjp):
        for args in ((None, host, host), (host, None, host), (host, host, None)):
            assert fn(dyn._h, *[None if a is None else L.dptr(a) for a in args]) == L.QC_ERR_INVALID and L.lib.qc_last_error(dyn._h)
    for fn in (L.lib.qc_eval_jvp_dev_multi, L.lib.qc_eval_vjp_dev_multi):
        assert fn(None, 0, p, p, p, None) == L.QC_ERR_INVALID and L.lib.qc_last_error(None)
        hs = (C.c_void_p * 1)(dyn._h)
        assert fn(hs, 1, p, None, p, None) == L.QC_ERR_INVALID and L.lib.qc_last_error(dyn._h)
    dyn.close()
    # a multi-device handle (two shards on device 0): out of scope, refused
    multi = qc.QuantumDynamics(inp.integrators, inp.traj, devices=[0, 0])
    for fn in (L.lib.qc_eval_jvp_dev, L.lib.qc_eval_vjp_dev):
        assert fn(multi._h, p, p, p, None) == L.QC_ERR_UNSUPPORTED and L.lib.qc_last_error(multi._h)
    for fn in (L.lib.qc_eval_jvp, L.lib.qc_eval_vjp):
        assert fn(multi._h, L.dptr(host), L.dptr(host), L.dptr(host)) == L.QC_ERR_UNSUPPORTED and L.lib.qc_last_error(multi._h)
    hs = (C.c_void_p * 1)(multi._h)
    assert L.lib.qc_eval_vjp_dev_multi(hs, 1, p, p, p, None) == L.QC_ERR_UNSUPPORTED
    with pytest.raises(qc.QCollocError) as e:
        multi.dF_times(host, host)
    assert e.value.code == L.QC_ERR_UNSUPPORTED
    multi.close()
    lst = list_inputs(qc, "sampling")
    comp = qc.QuantumDynamics(lst.integrators, lst.traj, devices=[0, 0])
    with pytest.raises(qc.QCollocError) as e:
        comp.dFT_times(np.zeros(int(comp.dims.Z_len)), np.zeros(int(comp.dims.F_len)))
    assert e.value.code == L.QC_ERR_UNSUPPORTED
    comp.close()


@gpu
def test_kernel_names(qc):
    L = qc._lib
    fused = qc.QuantumDynamics(*(lambda i: (i.integrators, i.traj))(qc.config_inputs(3, T=5)))
    assert (L.lib.qc_kernel_name(fused._h, 3), L.lib.qc_kernel_name(fused._h, 4)) == tuple(n.encode() for n in FUSED_NAMES)
    assert fused.product_kernel_names == FUSED_NAMES
    fused.close()
    inp = qc.unitary_smooth_pulse_inputs(qc.multi_qubit_system(2), qc.GATES["CNOT"], 5, integrator="exponential")
    generic = qc.QuantumDynamics(inp.integrators, inp.traj)
    assert (L.lib.qc_kernel_name(generic._h, 3), L.lib.qc_kernel_name(generic._h, 4)) == (b"generic-jvp", b"generic-vjp")
    generic.close()


@gpu
def test_evaluator_products_equal_the_dense_jacobian_times_the_vector(qc, oracle):
    """QuantumControlEvaluator on the 1-qubit problem, with a nonlinear constraint behind the dynamics rows.  Reference: the oracle's
    Jacobian for the dynamics rows (the file's bound), the evaluator's own dense row for the constraint (the same numbers the product
    methods use: summation rounding only)."""
    inp = qc.config_inputs(1, T=8)
    dyn = qc.QuantumDynamics(inp.integrators, inp.traj)
    con = qc.FinalUnitaryFidelityConstraint("Ũ⃗", 0.9, inp.traj)
    ev = qc.QuantumControlEvaluator(dyn, [], [con])
    rng = np.random.default_rng(16)
    x = inp.traj.datavec + 0.1 * rng.standard_normal(inp.traj.datavec.size)
    v, lam = rng.standard_normal(ev.n_variables), rng.standard_normal(ev.n_constraints)
    Jd, _ = reference(oracle, problem_from_inputs(inp), x)
    J = sp.vstack([Jd, ev.jacobian_matrix(x)[ev.n_dynamics_rows:]]).tocsr()
    Jabs = abs(J)
    y, w = ev.constraint_jacobian_times(x, v), ev.constraint_jacobian_transpose_times(x, lam)
    assert y.shape == (ev.n_constraints,) and w.shape == (ev.n_variables,)
    assert np.all(np.abs(y - J @ v) <= 1e-10 * (Jabs @ np.abs(v)) + 1e-12 * np.abs(J @ v).max())
    assert np.all(np.abs(w - J.T @ lam) <= 1e-10 * (Jabs.T @ np.abs(lam)) + 1e-12 * np.abs(J.T @ lam).max())
    assert y[-1] != 0.0      # the constraint's dense row took part
    con.close()
    dyn.close()


# ------------------------------------------------------------------------------------------------
#  CPU
# ------------------------------------------------------------------------------------------------
def test_prototypes_exist_and_nothing_crashes_without_a_handle(qc):
    L = qc._lib
    names = ("qc_eval_jvp_dev", "qc_eval_vjp_dev", "qc_eval_jvp", "qc_eval_vjp", "qc_eval_jvp_dev_multi", "qc_eval_vjp_dev_multi")
    for name in names:
        assert name in L.SYMBOLS and getattr(L.lib, name).argtypes == L.SYMBOLS[name][1]
    x = np.zeros(4)
    for name in names[2:4]:
        assert getattr(L.lib, name)(None, L.dptr(x), L.dptr(x), L.dptr(x)) == L.QC_ERR_INVALID
        assert b"NULL handle" in L.lib.qc_last_error(None)
    assert L.lib.qc_kernel_name(None, 3) == b"none" and L.lib.qc_kernel_name(None, 4) == b"none"
    for meth in ("dF_times", "dFT_times", "dF_times_device", "dFT_times_device"):
        assert callable(getattr(qc.QuantumDynamics, meth)) and callable(getattr(qc.ComposedQuantumDynamics, meth))
    for meth in ("constraint_jacobian_times", "constraint_jacobian_transpose_times"):
        assert callable(getattr(qc.QuantumControlEvaluator, meth))


def test_julia_glue_declares_the_products():
    """dF_mul! / dFt_mul! exist in julia/QCollocHIP.jl and call the host entries (their ccall signatures are checked against the
    header by tests/test_abi.py::test_julia_ccalls_match_the_header)."""
    import test_abi
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "julia", "QCollocHIP.jl"), encoding="utf-8").read()
    for fn, sym in (("dF_mul!", "qc_eval_jvp"), ("dFt_mul!", "qc_eval_vjp")):
        assert f"function {fn}(" in txt and f"(:{sym}, LIB[])" in txt
    test_abi.test_julia_ccalls_match_the_header()
