"""Wide rollout sweeps (`qc_sweep_desc.wide = QC_SWEEP_WIDE`, `RolloutSweep(..., wide=True)`): the matrix-core form "mfma32-sweep" for
16 < 2N <= 32 with up to 8 drives (csrc/qc_sweep32.hip).  CPU: the descriptor field, the restated launch rule with and without the flag,
the gradient scope, the struct mirror.  GPU: parity with the scipy reference of tests/sweep_reference.py at the smallest shapes at which
tiling, padding, chunking and squaring can go wrong, exact cases, bits, non-finite input, the unchanged default.

Tolerances are test_sweep.py's (states rtol 1e-10 / atol 1e-11, fidelities 1e-9 absolute; its argument |dF| <= sqrt(N) max|dU| holds for
N <= 32).  Every test prints its worst error against the bound; measured values: profiles/sweep_wide_summary.txt.
Wide states of many columns (more than 3584 entries: the finish kernel's LDS opt-in at ld = 32): tests/test_sweep_many_columns.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import sweep_reference as ref
import test_sweep as ts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_herm, _unitary = ts._herm, ts._unitary


def wide_launch(n, m, S, T, wide=True):
    """The launch rule restated: with `wide` the MFMA forms reach 2N = 32 (m <= 8); chunks by test_sweep.sweep_launch's rule."""
    if not wide:
        return ts.sweep_launch(n, m, S, T)
    if n > 32 or m > 8:
        return dict(mfma=False, chunk=T - 1, n_chunks=0, last=0)
    return ts.sweep_launch(16, m, S, T)          # the chunk rule does not depend on the size


def wide_name(n, m):
    return "rollout-per-sample" if (n > 32 or m > 8) else ("mfma16-sweep" if n <= 16 else "mfma32-sweep")


# name: (state, levels, m, p, scale given, free timestep, S, T, fidelity, samples checked by the gradient tests or None = all)
WIDE_CASES = {
    "transmons9-S11-T50": ("unitary", 9, 2, 1, False, True, 11, 50, ("unitary", [0, 1, 3, 4], "abs"), None),   # second tile row / column almost empty
    "levels12-S300-T2": ("unitary", 12, 6, 8, False, True, 300, 2, ("unitary", None, "abs"), None),          # one interval, every perturbation slot
    "levels16-S5-T12": ("unitary", 16, 8, 0, True, False, 5, 12, ("unitary", None, "abs2"), None),           # full tiles, 8 drives
    "levels16-S2-T102": ("unitary", 16, 1, 3, True, True, 2, 102, ("unitary", None, "abs"), None),           # sqrt-capped chunks, short last chunk
    "ket12-S2048-T2": ("ket", 12, 2, 1, True, True, 2048, 2, ("ket", None, "abs"), None),                    # one chunk
    "kets3-levels10": ("kets3", 10, 1, 3, True, False, 11, 20, None, None),
    "open4-S11-T20": ("density", 4, 2, 1, True, True, 11, 20, ("density", None, "abs"), None),               # n = 32, Lindblad generators
}


def build(qc, name, spec):
    """test_sweep.build_case for a case tuple given by the caller (that function reads its own table), plus what
    test_sweep_grad._check_call reads (`samples`)."""
    state, L, m, p, use_scale, free, S, T, fid, samples = spec
    rng = np.random.default_rng(sum(map(ord, name)))
    H0 = _herm(rng, L)
    Hd = [_herm(rng, L, (L * max(m, 1)) ** -0.5) for _ in range(m)]
    if state == "density":
        diss = [0.3 * (rng.standard_normal((L, L)) + 1j * rng.standard_normal((L, L))) / L ** 0.5]
        system = qc.OpenQuantumSystem(H0, Hd, diss)
        perts = []
        for q in range(p):
            if q == 0:
                Lx = (rng.standard_normal((L, L)) + 1j * rng.standard_normal((L, L))) / L ** 0.5
                perts.append(np.asarray(qc.iso_operator(qc.OpenQuantumSystem.dissipator_superoperator(Lx))))
            else:
                perts.append(np.asarray(qc.iso_operator(qc.OpenQuantumSystem.hamiltonian_superoperator(_herm(rng, L)))))
        G0, Gd, Gp = np.asarray(system.G_drift), [np.asarray(G) for G in system.G_drives], perts
        psi = rng.standard_normal(L) + 1j * rng.standard_normal(L)
        psi /= np.linalg.norm(psi)
        init = qc.density_to_iso_vec(np.outer(psi, psi.conj()))
        cols = 1
    else:
        system = qc.QuantumSystem(H0, Hd)
        perts = [_herm(rng, L) for _ in range(p)]
        G0, Gd, Gp = ref.iso_generator(H0), [ref.iso_generator(H) for H in Hd], [ref.iso_generator(P) for P in perts]
        if state == "unitary":
            init, cols = ref.operator_to_iso_vec(_unitary(rng, L)), L
        else:
            cols = 1 if state == "ket" else 3
            K = rng.standard_normal((L, cols)) + 1j * rng.standard_normal((L, cols))
            K /= np.linalg.norm(K, axis=0)
            init = ref.operator_to_iso_vec(K)
    goal = subspace = kind = form = None
    if fid is not None:
        kind, subspace, form = fid
        if kind == "unitary":
            goal = ref.operator_to_iso_vec(_unitary(rng, L))
        else:
            gk = rng.standard_normal(L) + 1j * rng.standard_normal(L)
            gk /= np.linalg.norm(gk)
            goal = np.concatenate([gk.real, gk.imag])
    controls = rng.uniform(-1, 1, (m, T))
    dts = rng.uniform(0.1, 0.3, T) if free else 0.2
    theta = rng.uniform(-0.3, 0.3, (S, p))
    if state == "density":
        theta = np.abs(theta)
    scale = rng.uniform(0.9, 1.1, (S, m)) if use_scale else None
    return dict(name=name, state=state, L=L, N=system.state_levels, n=2 * system.state_levels, m=m, p=p, S=S, T=T, system=system, perts=perts,
                G0=G0, Gd=Gd, Gp=Gp, init=init, cols=cols, goal=goal, kind=kind, subspace=subspace, form=form, controls=controls, dts=dts,
                theta=theta, scale=scale, samples=list(range(S)) if samples is None else list(samples))


# ---------------------------------------------------------------------------------------------------------------------------------
#  CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def _wdesc(qc, wide, **kw):
    D = ts._Desc(qc, **kw)
    D.d.wide = wide
    return D


def test_wide_field_is_validated(qc):
    L = qc._lib
    val = lambda D: L.lib.qc_sweep_desc_validate(C.byref(D.d))
    assert L.QC_SWEEP_WIDE == 1
    assert val(_wdesc(qc, 0, N=12)) == L.QC_OK and val(_wdesc(qc, 1, N=12)) == L.QC_OK and val(_wdesc(qc, 1, N=2)) == L.QC_OK
    for bad in (2, -1, 7):
        assert val(_wdesc(qc, bad, N=12)) == L.QC_ERR_INVALID
        assert L.lib.qc_sweep_last_error(None).decode().startswith("qc_sweep: wide")
    ok = C.c_int32(-1)
    assert L.lib.qc_sweep_desc_grad_supported(C.byref(_wdesc(qc, 2, N=12).d), C.byref(ok)) == L.QC_ERR_INVALID
    assert L.lib.qc_sweep_desc_launch(C.byref(_wdesc(qc, 2, N=12).d), 5, None, None, None) == L.QC_ERR_INVALID


def test_wide_launch_rule(qc):
    """`qc_sweep_desc_launch` against the restated rule: MFMA iff 2N <= 32 and m <= 8 with the flag, iff 2N <= 16 and m <= 8 without."""
    L = qc._lib
    seen = set()
    for n in (16, 18, 24, 32, 34):
        for m in (1, 8, 9):
            for S, T in ((1, 2), (2, 102), (5, 12), (11, 50), (300, 2), (2047, 50), (2048, 3), (8192, 1000)):
                for wide in (0, 1):
                    D = _wdesc(qc, wide, N=n // 2, m=m, T=T, cols=1)
                    mf, ch, nch = C.c_int32(), C.c_int64(), C.c_int64()
                    assert L.lib.qc_sweep_desc_launch(C.byref(D.d), S, C.byref(mf), C.byref(ch), C.byref(nch)) == L.QC_OK
                    want = wide_launch(n, m, S, T, bool(wide))
                    assert (bool(mf.value), ch.value, nch.value) == (want["mfma"], want["chunk"], want["n_chunks"]), (n, m, S, T, wide)
                    if want["mfma"]:
                        assert (nch.value - 1) * ch.value < T - 1 <= nch.value * ch.value
                    seen.add((n, m, wide, want["mfma"]))
    assert (24, 8, 1, True) in seen and (24, 8, 0, False) in seen and (32, 1, 1, True) in seen and (34, 1, 1, False) in seen
    assert (24, 9, 1, False) in seen and (16, 8, 0, True) in seen and (16, 8, 1, True) in seen
    f = wide_launch(32, 1, 2, 102)          # the sqrt-capped GPU case: 11 chunks of 10, the last of 1
    assert f["by_sqrt"] and (f["chunk"], f["n_chunks"], f["last"]) == (10, 11, 1)
    assert wide_launch(24, 2, 2048, 2)["n_chunks"] == 1


def test_wide_grad_scope_without_a_device(qc):
    L = qc._lib
    import test_sweep_grad as tg

    def supported(wide, **kw):
        D = tg._GDesc(qc, **kw)
        D.d.wide = wide
        ok = C.c_int32(-1)
        rc = L.lib.qc_sweep_desc_grad_supported(C.byref(D.d), C.byref(ok))
        return rc, ok.value, L.lib.qc_sweep_last_error(None).decode()

    U = L.QC_FID_UNITARY
    assert supported(1, N=12, m=2, fid_kind=U)[:2] == (L.QC_OK, 1)
    assert supported(1, N=9, m=8, fid_kind=U, subspace=[0, 1, 3, 4], fid_form=L.QC_FID_FORM_ABS2)[:2] == (L.QC_OK, 1)
    assert supported(1, N=16, m=1, fid_kind=U)[:2] == (L.QC_OK, 1)
    assert supported(1, N=10, m=2, cols=1, fid_kind=L.QC_FID_KET)[:2] == (L.QC_OK, 1)
    assert supported(1, N=4, m=2, fid_kind=U)[:2] == (L.QC_OK, 1)             # harmless at 2N <= 16
    # a Lindblad generator of 4 levels: N = 16, not antisymmetric
    D = tg._GDesc(qc, N=16, m=2, cols=1, fid_kind=L.QC_FID_DENSITY)
    D.d.wide = 1
    D.G0[:] = np.random.default_rng(0).standard_normal(D.G0.size)
    ok = C.c_int32(-1)
    assert L.lib.qc_sweep_desc_grad_supported(C.byref(D.d), C.byref(ok)) == L.QC_OK and ok.value == 0
    assert "antisymmetric" in L.lib.qc_sweep_last_error(None).decode()
    rc, ok, msg = supported(1, N=17, m=2, fid_kind=U)
    assert (rc, ok) == (L.QC_OK, 0) and "2N = 34" in msg and msg.startswith("qc_sweep gradients:")
    rc, ok, msg = supported(1, N=12, m=9, fid_kind=U)
    assert (rc, ok) == (L.QC_OK, 0) and "9 drives" in msg
    rc, ok, msg = supported(1, N=12, m=2)
    assert (rc, ok) == (L.QC_OK, 0) and "no fidelity" in msg
    rc, ok, msg = supported(1, N=12, m=2, cols=17)
    assert (rc, ok) == (L.QC_OK, 0) and "16 columns" in msg
    rc, ok, msg = supported(0, N=12, m=2, fid_kind=U)
    assert (rc, ok) == (L.QC_OK, 0) and "2N = 24" in msg and "> 16" in msg


def test_wide_desc_mirror_and_header(qc, tmp_path):
    L = qc._lib
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "qcolloc.h"\n'
                   'int main(){printf("%zu %zu %zu %zu %d\\n", sizeof(qc_sweep_desc), offsetof(qc_sweep_desc, device), '
                   'offsetof(qc_sweep_desc, wide), offsetof(qc_sweep_desc, reserved1), QC_SWEEP_WIDE);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    d = L.qc_sweep_desc
    assert got == [C.sizeof(d), d.device.offset, d.wide.offset, d.reserved1.offset, L.QC_SWEEP_WIDE]
    assert d.wide.offset == d.device.offset + 4 and d.wide.size == 4
    assert L.lib.qc_sizeof_sweep_desc() == C.sizeof(d) and L.lib.qc_abi_version() == 6      # a renamed reserved field: the ABI stays 0.6
    julia = open(os.path.join(ROOT, "julia", "QCollocHIP.jl")).read()
    assert "device::Int32; wide::Int32; reserved1::NTuple{2,Int64}" in julia and "wide::Bool=false" in julia
    import inspect
    for f in (qc.RolloutSweep.__init__, qc.rollout_sweep, qc.SweepInfidelityObjective.__init__):
        assert inspect.signature(f).parameters["wide"].default is False


# ---------------------------------------------------------------------------------------------------------------------------------
#  GPU
# ---------------------------------------------------------------------------------------------------------------------------------
def _report(what, got, want, fids=None, rfids=None):
    err = np.abs(got - want)
    worst = (err / (ts.STATE_ATOL + ts.STATE_RTOL * np.abs(want))).max()
    line = f"SWEEP-WIDE {what}: max |d state| = {err.max():.3e}, worst / tolerance = {worst:.4f}"
    if fids is not None:
        line += f", max |d fidelity| = {np.abs(fids - rfids).max():.3e} (bound {ts.FID_ATOL:.0e})"
    print(line)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(WIDE_CASES))
def test_wide_sweep_matches_the_reference(qc, name):
    c = build(qc, name, WIDE_CASES[name])
    want = wide_launch(c["n"], c["m"], c["S"], c["T"])
    assert want["mfma"] and 16 < c["n"] <= 32
    sw = ts.make_sweep(qc, c, wide=True)
    try:
        assert sw.kernel_name == "mfma32-sweep" and sw.wide
        assert sw.launch(c["S"]) == (True, want["chunk"], want["n_chunks"])
        if name == "levels16-S2-T102":
            assert want["by_sqrt"] and want["n_chunks"] >= 3 and want["last"] < want["chunk"]
        if name in ("ket12-S2048-T2", "levels12-S300-T2"):
            assert want["n_chunks"] == 1
        Z = sw.pack(c["controls"], c["dts"])
        finals, fids = sw.eval(Z, c["init"], c["theta"], c["scale"])
        if c["kind"] is not None:   # fidelities alone: the same values
            np.testing.assert_array_equal(sw.eval(Z, c["init"], c["theta"], c["scale"], finals=False)[1], fids)
    finally:
        sw.close()
    rf, rfid = ts.reference(c)
    assert finals.shape == rf.shape == (c["n"] * c["cols"], c["S"])
    _report(name, finals, rf, fids, rfid)
    ts._assert_states(finals, rf, name)
    if c["kind"] is None:
        assert fids is None
    else:
        ts._assert_fids(fids, rfid, name)
    if c["S"] <= 11 and np.ndim(c["dts"]):       # the one-call form: the same launch for free timesteps
        f3, fid3 = qc.rollout_sweep(c["init"], c["controls"], c["dts"], c["system"], c["perts"], c["theta"], c["scale"], cols=c["cols"],
                                    goal=c["goal"], fid_kind=c["kind"], subspace=c["subspace"],
                                    fid_form=qc._lib.QC_FID_FORM_ABS2 if c["form"] == "abs2" else qc._lib.QC_FID_FORM_ABS, wide=True)
        np.testing.assert_array_equal(f3, finals)
        if fids is not None:
            np.testing.assert_array_equal(fid3, fids)


def squaring_cases(qc, N=9, m=2, T=12):
    """One system per number of squarings 0 .. 6, scaled as test_grad_through_the_squarings scales its own; a strong perturbation makes
    the samples of one call differ.  Yields (k, squarings per sample, case dictionary)."""
    rng = np.random.default_rng(17)
    H0, Hd, P = _herm(rng, N), [_herm(rng, N, 0.25) for _ in range(m)], _herm(rng, N)
    controls = rng.uniform(-1, 1, (m, T))
    init, goal = ref.operator_to_iso_vec(_unitary(rng, N)), ref.operator_to_iso_vec(_unitary(rng, N))
    theta = np.array([[0.0], [0.5], [1.5], [4.0], [-9.0]])
    S, dt = theta.shape[0], 0.2
    base = max(np.abs(dt * ref.sample_generator(ref.iso_generator(H0), [ref.iso_generator(H) for H in Hd], [], controls[:, t], (), np.ones(m))).sum(axis=0).max()
               for t in range(T - 1))
    for k in range(7):
        f = 0.09 * 2.0 ** k / base
        G0, Gd, Gp = ref.iso_generator(f * H0), [ref.iso_generator(f * H) for H in Hd], [ref.iso_generator(f * P)]
        per_sample = [max(ts._squarings(np.abs(dt * ref.sample_generator(G0, Gd, Gp, controls[:, t], theta[s], np.ones(m))).sum(axis=0).max())
                          for t in range(T - 1)) for s in range(S)]
        assert per_sample[0] == k and len(set(per_sample)) > 1
        yield k, per_sample, dict(name=f"squarings {per_sample}", L=N, m=m, S=S, T=T, system=qc.QuantumSystem(f * H0, [f * H for H in Hd]),
                                  perts=[f * P], G0=G0, Gd=Gd, Gp=Gp, init=init, cols=N, goal=goal, kind="unitary", subspace=None, form="abs",
                                  controls=controls, dts=dt, theta=theta, scale=None, samples=list(range(S)))


@pytest.mark.gpu
def test_wide_sweep_generator_norms(qc):
    seen = set()
    for k, per_sample, c in squaring_cases(qc):
        seen |= set(per_sample)
        finals, fids = qc.rollout_sweep(c["init"], c["controls"], c["dts"], c["system"], c["perts"], c["theta"], goal=c["goal"], fid_kind="unitary",
                                        wide=True)
        rf, rfid = ts.reference(c)
        _report(c["name"], finals, rf, fids, rfid)
        ts._assert_states(finals, rf, c["name"])
        ts._assert_fids(fids, rfid, c["name"])
    assert set(range(7)) <= seen


@pytest.mark.gpu
def test_wide_sweep_exact_cases(qc):
    """A zero generator gives the identity bits: finals are init.  theta = 0, scale = 1 on a wide N = 12 handle: the bits of the handle
    without perturbations, the per-sample form of the default handle to the state tolerance, and `unitary_rollout`."""
    N, T, S, m = 12, 14, 7, 2
    rng = np.random.default_rng(N)
    init = ref.operator_to_iso_vec(_unitary(rng, N))
    zsys = qc.QuantumSystem(np.zeros((N, N)), [np.zeros((N, N))] * m)
    finals, _ = qc.rollout_sweep(init, rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T), zsys, [np.zeros((N, N))], rng.uniform(-1, 1, (S, 1)),
                                 wide=True)
    np.testing.assert_array_equal(finals, np.repeat(init[:, None], S, axis=1))
    sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, 0.3) for _ in range(m)])
    controls, dts = rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T)
    goal = ref.operator_to_iso_vec(_unitary(rng, N))
    perts = [_herm(rng, N), _herm(rng, N)]
    a = qc.rollout_sweep(init, controls, dts, sys_, perts, np.zeros((S, 2)), np.ones((S, m)), goal=goal, fid_kind="unitary", wide=True)
    b = qc.rollout_sweep(init, controls, dts, sys_, [], np.zeros((S, 0)), None, goal=goal, fid_kind="unitary", wide=True)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    assert np.all(a[0] == a[0][:, :1]) and np.abs(a[0][:, 0] - init).max() > 1e-3
    narrow = qc.rollout_sweep(init, controls, dts, sys_, perts, np.zeros((S, 2)), np.ones((S, m)), goal=goal, fid_kind="unitary")
    _report("wide against the per-sample form", a[0], narrow[0], a[1], narrow[1])
    ts._assert_states(a[0], narrow[0], "wide against the per-sample form")
    ts._assert_fids(a[1], narrow[1], "wide against the per-sample form")
    roll = qc.unitary_rollout(init, controls, dts, sys_)[:, -1]
    _report("wide against unitary_rollout", a[0][:, 0], roll)
    ts._assert_states(a[0][:, 0], roll, "wide against unitary_rollout")


@pytest.mark.gpu
def test_wide_sweep_bits_host_device_side_stream_and_scratch(qc):
    """Six repeated calls return identical bits; the host and device entry points agree bit for bit, on a side stream too; a handle whose
    S grows and then shrinks returns the bits of a fresh handle at every S (the S x n_chunks x 1024 totals are grown on demand)."""
    rng = np.random.default_rng(8)
    N, m, T = 9, 2, 20
    sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, (N * m) ** -0.5) for _ in range(m)])
    perts = [_herm(rng, N)]
    goal = ref.operator_to_iso_vec(_unitary(rng, N))
    make = lambda: qc.RolloutSweep(sys_, perts, T, goal=goal, fid_kind="unitary", subspace=[0, 1, 3, 4], wide=True)
    sw = make()
    assert sw.kernel_name == "mfma32-sweep"
    Z = sw.pack(rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T))
    init = ref.operator_to_iso_vec(_unitary(rng, N))
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    side = torch.cuda.Stream(device=dev)
    try:
        for i, S in enumerate((3, 150, 7)):
            theta, scale = rng.uniform(-0.3, 0.3, (S, 1)), rng.uniform(0.9, 1.1, (S, m))
            fresh = make()
            want = fresh.eval(Z, init, theta, scale)
            fresh.close()
            got = sw.eval(Z, init, theta, scale)
            np.testing.assert_array_equal(got[0], want[0])
            np.testing.assert_array_equal(got[1], want[1])
            if i == 1:
                for _ in range(6):
                    again = sw.eval(Z, init, theta, scale)
                    np.testing.assert_array_equal(again[0], want[0])
                    np.testing.assert_array_equal(again[1], want[1])
            dZ, dinit, dth, dsc = t(Z), t(init), t(theta), t(scale)
            dfin, dfid = torch.full((S, sw.ns), -7.0, dtype=torch.float64, device=dev), torch.full((S,), -7.0, dtype=torch.float64, device=dev)
            sw.eval_device(dZ, dinit, dth, dsc, dfin, dfid)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(dfin.cpu().numpy().T, want[0])
            np.testing.assert_array_equal(dfid.cpu().numpy(), want[1])
            dfin2, dfid2 = torch.full_like(dfin, -7.0), torch.full_like(dfid, -7.0)
            with torch.cuda.stream(side):
                sw.eval_device(dZ, dinit, dth, dsc, dfin2, dfid2, stream=side)
            side.synchronize()
            np.testing.assert_array_equal(dfin2.cpu().numpy().T, want[0])
            np.testing.assert_array_equal(dfid2.cpu().numpy(), want[1])
    finally:
        sw.close()


@pytest.mark.gpu
def test_wide_sweep_non_finite_input(qc):
    rng = np.random.default_rng(12)
    N, m, T, S = 12, 2, 14, 6
    sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, 0.3) for _ in range(m)])
    goal = ref.operator_to_iso_vec(_unitary(rng, N))
    sw = qc.RolloutSweep(sys_, [_herm(rng, N)], T, goal=goal, fid_kind="unitary", wide=True)
    try:
        assert sw.kernel_name == "mfma32-sweep"
        controls, dts = rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T)
        init = ref.operator_to_iso_vec(_unitary(rng, N))
        theta = rng.uniform(-0.3, 0.3, (S, 1))
        good = sw.eval(sw.pack(controls, dts), init, theta)
        assert np.isfinite(good[0]).all()
        bad = controls.copy()
        bad[1, 7] = np.nan
        finals, fids = sw.eval(sw.pack(bad, dts), init, theta)
        assert np.isnan(finals).all() and np.isnan(fids).all()
        bad = controls.copy()
        bad[0, T - 1] = np.nan          # the last knot's controls drive no interval
        again = sw.eval(sw.pack(bad, dts), init, theta)
        np.testing.assert_array_equal(again[0], good[0])
        np.testing.assert_array_equal(again[1], good[1])
    finally:
        sw.close()


@pytest.mark.gpu
def test_default_is_unchanged(qc):
    """Without `wide`, N = 12 is still the per-sample form and still refuses gradients with "2N = 24"; with it, 2N <= 16 is still
    "mfma16-sweep" with the bits of the default handle."""
    rng = np.random.default_rng(3)
    N, m, T, S = 12, 2, 6, 3
    sys_ = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, 0.3) for _ in range(m)])
    goal = ref.operator_to_iso_vec(_unitary(rng, N))
    sw = qc.RolloutSweep(sys_, [_herm(rng, N)], T, goal=goal, fid_kind="unitary")
    try:
        assert sw.kernel_name == "rollout-per-sample" and not sw.wide and sw.launch(S) == (False, T - 1, 0)
        assert not sw.grad_supported and "2N = 24" in sw.grad_unsupported_reason
        Z = sw.pack(rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T))
        init, theta = ref.operator_to_iso_vec(_unitary(rng, N)), rng.uniform(-0.3, 0.3, (S, 1))
        with pytest.raises(qc.QCollocError) as e:
            sw.grad(Z, init, theta)
        assert e.value.code == qc._lib.QC_ERR_UNSUPPORTED and "2N = 24" in str(e.value)
        assert np.isfinite(sw.eval(Z, init, theta)[0]).all()
    finally:
        sw.close()
    N = 4
    sys4 = qc.QuantumSystem(_herm(rng, N), [_herm(rng, N, 0.3) for _ in range(m)])
    goal, init, P = ref.operator_to_iso_vec(_unitary(rng, N)), ref.operator_to_iso_vec(_unitary(rng, N)), _herm(rng, N)
    a, b = (qc.RolloutSweep(sys4, [P], T, goal=goal, fid_kind="unitary", wide=w) for w in (False, True))
    try:
        assert a.kernel_name == b.kernel_name == "mfma16-sweep"
        Z = a.pack(rng.uniform(-1, 1, (m, T)), rng.uniform(0.1, 0.3, T))
        ra, rb = a.grad(Z, init, theta, per_sample=True), b.grad(Z, init, theta, per_sample=True)
        assert ra[0] == rb[0]
        for u, v in zip(ra[1:], rb[1:]):
            np.testing.assert_array_equal(u, v)
        pa, pb = a.param_grad(Z, init, theta), b.param_grad(Z, init, theta)
        for u, v in zip(pa, pb):
            np.testing.assert_array_equal(u, v)
    finally:
        a.close()
        b.close()
