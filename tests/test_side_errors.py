"""Return codes and messages of the four side-handle families (qc_fidelity, qc_terms, qc_robust, qc_sweep) on every refusal that
needs no device: one line `family | case name | return code | message` per case, equal to tests/golden/side_errors.txt line by line.
That file was recorded from the library as it was before the families' error recording, device check and allocation moved into
csrc/qc_side.h, so the messages (API: bindings match on them) are the ones each family wrote by hand.

Cases against the `?fail(` call sites of the sources (`qc_sweep_fail(` in qc_sweep.hip; the one-line definitions of ffail / tfail / rfail /
qc_sweep_fail not counted; several cases may reach one site through different fields or entry points):
    qc_fidelity.hip  24 sites, 20 reached by 24 cases
    qc_terms.hip     29 sites, 26 reached by 30 cases
    qc_robust.hip    31 sites, 25 reached by 27 cases
    qc_sweep.hip     38 sites, 29 reached by 33 cases   (one site holds two texts, ket and density operator: a case each; the NULL
                     handle of qc_sweep_eval and of qc_sweep_eval_dev is one site, in qc_sweep_check, which every entry point of the
                     family calls first)
plus one valid descriptor per family, refused with QC_ERR_NO_DEVICE where there is no GPU ("<create>: no HIP device visible"; the other
text of that check in qc_side.h, "<create>: device ordinal out of range", needs a visible device to be out of range of).
Sites without a case: each needs a created handle or a failing HIP call.
    qc_fidelity.hip  qc_fidelity_eval_dev "NULL buffer", "kernel launch: ..."; qc_fidelity_eval "NULL input";
                     "qc_hermitian_eig: did not converge" (a helper, no handle entry point; the same routine's refusal inside
                     qc_fidelity_create_desc is a case)
    qc_terms.hip     qc_terms_eval_dev "NULL buffer", "kernel launch: ..."; qc_terms_eval "NULL input"
    qc_robust.hip    qc_robust_hess_structure "NULL output"; qc_robust_eval_dev and qc_robust_eval "NULL input" and "Hessian values
                     requested from a handle created without a Hessian"; qc_robust_eval_dev "kernel launch: ..."
    qc_sweep.hip     qc_sweep_check (the lines every entry point shares) the entry's scope, "NULL input", "<input> is NULL", "S must be in
                     1 .. 2^24", "theta is NULL but ..."; qc_sweep_eval_dev and qc_sweep_eval "finals and fids are both NULL",
                     "fidelities requested from a handle created without one", "kernel launch: ..."; and, needing neither, the
                     descriptor's "wide must be 0 or QC_SWEEP_WIDE (1)" (tests/test_sweep_wide.py holds the return code)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "side_errors.txt")

_keep = []      # arrays the descriptors point into


def _d(*v):
    a = np.array(v, dtype=np.float64)
    _keep.append(a)
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _i(*v):
    a = np.array(v, dtype=np.int32)
    _keep.append(a)
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _with(make, **kw):
    d = make()
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def fidelity_cases(L):
    lib = L.lib
    out = C.c_void_p()

    def desc(**kw):
        def make():
            d = L.qc_fidelity_desc()
            d.kind, d.N, d.goal_iso, d.device = L.QC_FID_UNITARY, 2, _d(*np.arange(1.0, 9.0)), 0
            return d
        return _with(make, **kw)

    def create(name, **kw):
        return name, lambda: lib.qc_fidelity_create_desc(C.byref(desc(**kw)), C.byref(out))

    def phases(**kw):       # two free phases on a 2 x 2 subspace of N = 4: dims (2, 1), operators Z and (1)
        base = dict(N=4, goal_iso=_d(*np.arange(32.0)), subspace=_i(0, 1), n_sub=2, n_phases=2, phase_dims=_i(2, 1),
                    phase_ops=_d(1, 0, 0, -1, 0, 0, 0, 0, 1, 0))
        base.update(kw)
        return base

    nan = float("nan")
    return [
        ("create_desc: out is NULL", lambda: lib.qc_fidelity_create_desc(C.byref(desc()), None)),
        ("create_desc: descriptor is NULL", lambda: lib.qc_fidelity_create_desc(None, C.byref(out))),
        create("create_desc: ket with a subspace", kind=L.QC_FID_KET, subspace=_i(0), n_sub=1),
        create("create_desc: density operator with a form", kind=L.QC_FID_DENSITY, form=L.QC_FID_FORM_ABS2),
        create("create_desc: unknown kind", kind=7),
        create("create_desc: N = 0", N=0),
        create("create_desc: N = 65", N=65),
        create("create_desc: goal is NULL", goal_iso=None),
        create("create_desc: n_sub = 3 of N = 2", subspace=_i(0, 1, 1), n_sub=3),
        create("create_desc: unknown form", form=2),
        create("create_desc: subspace index 2 of N = 2", subspace=_i(0, 2), n_sub=2),
        create("create_desc: n_phases = 17", n_phases=17),
        create("create_desc: phase arrays missing", **phases(phase_ops=None)),
        create("create_desc: phase dimension 0", **phases(phase_dims=_i(2, 0))),
        create("create_desc: phase dimensions 2 x 2 on a subspace of 2", **phases(phase_dims=_i(2, 2))),
        create("create_desc: phase operator not Hermitian", **phases(phase_ops=_d(1, 0, 1, -1, 0, 0, 0, 0, 1, 0))),
        create("create_desc: phase operator of NaN", **phases(phase_ops=_d(nan, nan, nan, nan, 0, 0, 0, 0, 1, 0))),
        create("create_desc: ket with N = 0 (through create_kind)", kind=L.QC_FID_KET, N=0),
        ("create_kind: out is NULL", lambda: lib.qc_fidelity_create_kind(L.QC_FID_KET, 2, _d(1, 0, 0, 0), 0, None)),
        ("create_kind: unitary", lambda: lib.qc_fidelity_create_kind(L.QC_FID_UNITARY, 2, _d(1, 0, 0, 0), 0, C.byref(out))),
        ("create_kind: goal is NULL", lambda: lib.qc_fidelity_create_kind(L.QC_FID_KET, 2, None, 0, C.byref(out))),
        ("hermitian_eig: d = 0", lambda: lib.qc_hermitian_eig(0, None, None, None, None, None)),
        ("eval: NULL handle", lambda: lib.qc_fidelity_eval(None, None, None, None, None, None)),
        ("eval_dev: NULL handle", lambda: lib.qc_fidelity_eval_dev(None, None, None, None, None, None)),
    ], ("valid descriptor", lambda: lib.qc_fidelity_create_desc(C.byref(desc()), C.byref(out)))


def terms_cases(L):
    lib = L.lib
    out = C.c_void_p()
    nnz = C.c_int64()
    rows = (C.c_int64 * 64)()

    def desc(**kw):
        def make():
            d = L.qc_terms_desc()
            d.T, d.zdim, d.off_dt, d.n_reg, d.weighting = 3, 4, 3, 2, L.QC_REG_DT_SCALED
            d.reg_index, d.reg_R = _i(0, 1), _d(1.0, 2.0)
            return d
        return _with(make, **kw)

    def ext(**kw):
        def make():
            x = L.qc_terms_ext()
            x.n_smooth, x.smooth_index, x.smooth_R = 1, _i(0), _d(1.0)
            x.n_pair, x.pair_a, x.pair_b, x.pair_Q = 1, _i(0), _i(1), _d(1.0)
            x.n_lin, x.lin_index, x.lin_w = 1, _i(2), _d(1.0)
            return x
        return _with(make, **kw)

    def v(name, **kw):
        return name, lambda: lib.qc_terms_desc_hess_nnz(C.byref(desc(**kw)), C.byref(nnz))

    def xv(name, **kw):
        return name, lambda: lib.qc_terms_desc_ext_hess_nnz(C.byref(desc()), C.byref(ext(**kw)), C.byref(nnz))

    return [
        ("desc: NULL descriptor", lambda: lib.qc_terms_desc_hess_nnz(None, C.byref(nnz))),
        v("desc: T = 0", T=0),
        v("desc: global_dim = -1", global_dim=-1),
        v("desc: off_dt = zdim", off_dt=4),
        v("desc: n_reg = 5 of zdim = 4", n_reg=5),
        v("desc: reg_R is NULL", reg_R=None),
        v("desc: reg_index not increasing", reg_index=_i(1, 0)),
        v("desc: reg_index holds the timestep", reg_index=_i(0, 3)),
        v("desc: retired weighting 1", weighting=1),
        v("desc: minimum time without a free timestep", off_dt=-1, min_time_D=1.0),
        v("desc: min_time_knots = 4 of T = 3", min_time_knots=4),
        ("desc_hess_nnz: NULL output", lambda: lib.qc_terms_desc_hess_nnz(C.byref(desc()), None)),
        ("desc_hess_structure: NULL output", lambda: lib.qc_terms_desc_hess_structure(C.byref(desc()), None, rows, 0)),
        ("desc_ext: bad descriptor under a valid extension", lambda: lib.qc_terms_desc_ext_hess_nnz(C.byref(desc(zdim=0)), C.byref(ext()), C.byref(nnz))),
        xv("ext: n_pair = -1", n_pair=-1),
        xv("ext: smooth_R is NULL", smooth_R=None),
        xv("ext: smooth_index = zdim", smooth_index=_i(4)),
        xv("ext: repeated smooth_index", n_smooth=2, smooth_index=_i(1, 1), smooth_R=_d(1.0, 1.0)),
        xv("ext: lin_index is the timestep", lin_index=_i(3)),
        xv("ext: repeated lin_index", n_lin=2, lin_index=_i(2, 2), lin_w=_d(1.0, 1.0)),
        xv("ext: pair_b = -1", pair_b=_i(-1)),
        xv("ext: pair_a = pair_b", pair_b=_i(0)),
        ("desc_ext_hess_nnz: NULL output", lambda: lib.qc_terms_desc_ext_hess_nnz(C.byref(desc()), C.byref(ext()), None)),
        ("desc_ext_hess_structure: NULL output", lambda: lib.qc_terms_desc_ext_hess_structure(C.byref(desc()), C.byref(ext()), rows, None, 0)),
        ("create: out is NULL", lambda: lib.qc_terms_create(C.byref(desc()), None)),
        ("create_ext: invalid extension", lambda: lib.qc_terms_create_ext(C.byref(desc()), C.byref(ext(n_lin=-2)), C.byref(out))),
        ("hess_nnz: NULL handle", lambda: lib.qc_terms_hess_nnz(None, C.byref(nnz))),
        ("hess_structure: NULL handle", lambda: lib.qc_terms_hess_structure(None, rows, rows, 0)),
        ("eval: NULL handle", lambda: lib.qc_terms_eval(None, None, None, None, None)),
        ("eval_dev: NULL handle", lambda: lib.qc_terms_eval_dev(None, None, None, None, None, None)),
    ], ("valid descriptor", lambda: lib.qc_terms_create_ext(C.byref(desc()), C.byref(ext()), C.byref(out)))


def robust_cases(L):
    lib = L.lib
    out = C.c_void_p()
    n64 = C.c_int64()
    rows = (C.c_int64 * 64)()

    def desc(**kw):
        def make():
            d = L.qc_robust_desc()
            d.T, d.zdim, d.off_state, d.N, d.off_dt, d.n_knots = 3, 9, 0, 2, 8, 3
            d.H_re = _d(1.0, 0.0, 0.0, -1.0)
            return d
        return _with(make, **kw)

    def v(name, **kw):
        return name, lambda: lib.qc_robust_desc_n_vars(C.byref(desc(**kw)), C.byref(n64))

    return [
        ("desc: NULL descriptor", lambda: lib.qc_robust_desc_n_vars(None, C.byref(n64))),
        v("desc: T = 0", T=0),
        v("desc: N = 0", N=0),
        v("desc: state past the knot", off_state=2),
        v("desc: off_dt = zdim", off_dt=9),
        v("desc: off_dt inside the state", off_dt=3),
        v("desc: n_knots = 4 of T = 3", n_knots=4),
        v("desc: hessian = 2", hessian=2),
        v("desc: H_re is NULL", H_re=None),
        v("desc: n_sub = 3 of N = 2", subspace=_i(0, 1, 0), n_sub=3),
        v("desc: repeated subspace level", subspace=_i(1, 1), n_sub=2),
        v("desc: subspace level 2 of N = 2", subspace=_i(0, 2), n_sub=2),
        v("desc: NULL subspace with n_sub = 1", n_sub=1),
        v("desc: 2N = 66", N=33, zdim=2 * 33 * 33 + 1, off_dt=2 * 33 * 33),
        v("desc: exact Hessian past 2^27 entries", N=8, zdim=129, off_dt=128, T=200, n_knots=200, hessian=L.QC_ROBUST_HESS_EXACT,
          H_re=_d(*np.zeros(64))),
        ("desc_n_vars: NULL output", lambda: lib.qc_robust_desc_n_vars(C.byref(desc()), None)),
        ("desc_vars: NULL output", lambda: lib.qc_robust_desc_vars(C.byref(desc()), None)),
        ("desc_hess_nnz: NULL output", lambda: lib.qc_robust_desc_hess_nnz(C.byref(desc()), None)),
        ("desc_hess_structure: NULL output", lambda: lib.qc_robust_desc_hess_structure(C.byref(desc(hessian=L.QC_ROBUST_HESS_EXACT)), rows, None, 0)),
        ("create: out is NULL", lambda: lib.qc_robust_create(C.byref(desc()), None)),
        ("create: invalid descriptor", lambda: lib.qc_robust_create(C.byref(desc(n_knots=0)), C.byref(out))),
        ("n_vars: NULL handle", lambda: lib.qc_robust_n_vars(None, C.byref(n64))),
        ("vars: NULL handle", lambda: lib.qc_robust_vars(None, rows)),
        ("hess_nnz: NULL handle", lambda: lib.qc_robust_hess_nnz(None, C.byref(n64))),
        ("hess_structure: NULL handle", lambda: lib.qc_robust_hess_structure(None, rows, rows, 0)),
        ("eval: NULL handle", lambda: lib.qc_robust_eval(None, None, None, None, None)),
        ("eval_dev: NULL handle", lambda: lib.qc_robust_eval_dev(None, None, None, None, None, None)),
    ], ("valid descriptor", lambda: lib.qc_robust_create(C.byref(desc()), C.byref(out)))


def sweep_cases(L):
    lib = L.lib
    out = C.c_void_p()
    g16 = np.zeros(16)

    def desc(**kw):
        def make():
            d = L.qc_sweep_desc()
            d.T, d.zdim, d.off_a, d.off_dt, d.N, d.m, d.fid_kind = 3, 2, 0, 1, 2, 1, L.QC_SWEEP_FID_NONE
            d.G_drift, d.G_drives = _d(*g16), _d(*g16)
            return d
        return _with(make, **kw)

    def v(name, **kw):
        return name, lambda: lib.qc_sweep_desc_validate(C.byref(desc(**kw)))

    def fid(name, kind=None, **kw):
        base = dict(fid_kind=L.QC_FID_UNITARY if kind is None else kind, goal_iso=_d(*np.arange(8.0)))
        base.update(kw)
        return v(name, **base)

    return [
        ("desc: NULL descriptor", lambda: lib.qc_sweep_desc_validate(None)),
        v("desc: N = 0", N=0),
        v("desc: m = -1", m=-1),
        v("desc: T = 1", T=1),
        v("desc: T = 2^30 + 1", T=(1 << 30) + 1),
        v("desc: zdim = 0", zdim=0),
        v("desc: drives past the knot", off_a=2),
        v("desc: off_dt = zdim", off_dt=2),
        v("desc: n_pert = 9", n_pert=9),
        v("desc: G_pert is NULL", n_pert=1),
        v("desc: G_drift is NULL", G_drift=None),
        v("desc: G_drives is NULL", G_drives=None),
        v("desc: state_cols = -1", state_cols=-1),
        fid("desc: fid_kind = 5", kind=5),
        fid("desc: fid_form = 2", fid_form=2),
        fid("desc: fidelity without a goal", goal_iso=None),
        fid("desc: unitary fidelity of one column", state_cols=1),
        fid("desc: n_sub = 3 of N = 2", subspace=_i(0, 1, 0), n_sub=3),
        fid("desc: subspace index 2 of N = 2", subspace=_i(0, 2), n_sub=2),
        fid("desc: repeated subspace level", subspace=_i(1, 1), n_sub=2),
        fid("desc: ket fidelity with a form", kind=L.QC_FID_KET, state_cols=1, fid_form=L.QC_FID_FORM_ABS2),
        fid("desc: ket fidelity of N columns", kind=L.QC_FID_KET),
        fid("desc: density fidelity of N columns", kind=L.QC_FID_DENSITY),
        fid("desc: density fidelity with N = 2", kind=L.QC_FID_DENSITY, state_cols=1),
        v("desc: 2N = 66", N=33),
        v("desc: state of 64 x 65 entries", N=32, state_cols=65),
        v("desc: m = 65", m=65, zdim=66, off_dt=65),
        ("desc_launch: invalid descriptor", lambda: lib.qc_sweep_desc_launch(C.byref(desc(m=-3)), 1, None, None, None)),
        ("desc_launch: S = 0", lambda: lib.qc_sweep_desc_launch(C.byref(desc()), 0, None, None, None)),
        ("create: out is NULL", lambda: lib.qc_sweep_create(C.byref(desc()), None)),
        ("create: invalid descriptor", lambda: lib.qc_sweep_create(C.byref(desc(T=0)), C.byref(out))),
        ("eval: NULL handle", lambda: lib.qc_sweep_eval(None, None, None, 1, None, None, None, None)),
        ("eval_dev: NULL handle", lambda: lib.qc_sweep_eval_dev(None, None, None, 1, None, None, None, None, None)),
    ], ("valid descriptor", lambda: lib.qc_sweep_create(
        C.byref(desc(fid_kind=L.QC_FID_UNITARY, goal_iso=_d(*np.arange(8.0)), subspace=_i(1, 0), n_sub=2)), C.byref(out)))


FAMILIES = (("fidelity", fidelity_cases), ("terms", terms_cases), ("robust", robust_cases), ("sweep", sweep_cases))


def lines_of(L, family, cases):
    last = getattr(L.lib, f"qc_{family}_last_error")
    out = []
    for name, call in cases:
        rc = call()
        out.append(f"{family} | {name} | {rc} | {last(None).decode()}")
    return out


def golden(family, valid):
    with open(GOLDEN) as f:
        rows = [ln.rstrip("\n") for ln in f if ln.startswith(family + " | ")]
    return [r for r in rows if (" | valid descriptor | " in r) == valid]


@pytest.mark.parametrize("family,make", FAMILIES, ids=[f for f, _ in FAMILIES])
def test_refusals_without_a_device(qc, family, make):
    cases, _ = make(qc._lib)
    got, want = lines_of(qc._lib, family, cases), golden(family, False)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
        assert g.split(" | ")[2] in (str(qc._lib.QC_ERR_INVALID), str(qc._lib.QC_ERR_UNSUPPORTED))


@pytest.mark.skipif(torch.cuda.is_available(), reason="this box has a GPU")
@pytest.mark.parametrize("family,make", FAMILIES, ids=[f for f, _ in FAMILIES])
def test_valid_descriptor_without_a_device(qc, family, make):
    _, valid = make(qc._lib)
    got, want = lines_of(qc._lib, family, [valid]), golden(family, True)
    assert got == want
    assert got[0].split(" | ")[2] == str(qc._lib.QC_ERR_NO_DEVICE)


def test_last_error_of_one_family_only(qc):
    """qc_X_last_error(NULL) is family X's last message on this thread: another family's refusal does not replace it."""
    lib = qc._lib.lib
    assert lib.qc_terms_eval(None, None, None, None, None) == qc._lib.QC_ERR_INVALID
    mine = lib.qc_terms_last_error(None)
    assert lib.qc_sweep_desc_validate(None) == qc._lib.QC_ERR_INVALID
    assert lib.qc_robust_eval(None, None, None, None, None) == qc._lib.QC_ERR_INVALID
    assert lib.qc_fidelity_eval(None, None, None, None, None, None) == qc._lib.QC_ERR_INVALID
    assert lib.qc_terms_last_error(None) == mine == b"qc_terms_eval: NULL handle"
    assert lib.qc_sweep_last_error(None) == b"qc_sweep: NULL descriptor"
