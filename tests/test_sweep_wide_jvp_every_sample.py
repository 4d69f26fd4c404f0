"""Wide sweep pushforwards (`qc_sweep32_jvp_kernel`, the ld = 32 instantiation of `jvp_finish`: `qc_sweep_jvp*` on "mfma32-sweep" handles
made with `wide=True, wide_tangent=True`) at mid-size and filled launches, EVERY sample against the CPU reference: the method of
tests/test_sweep_jvp_every_sample.py (read its header and that of tests/test_sweep_every_sample.py: R = 8 rows, sample s carries row
cls[s], the Frechet reference once for the R rows) applied to wide handles, its helpers imported.  tests/test_sweep_wide_jvp.py checks the
arithmetic at up to 20 work items and three samples of one S = 2048 launch; what is checked here is what that kernel has of its own:
  * two waves a workgroup: item = 2 blockIdx + wave, s = item / n_chunks, the store at tot + item * 2048, the finish kernel's read at
    tot + s * n_chunks * 2048, an odd item count (the last workgroup's second wave exits), workgroups that straddle two samples;
  * the lane's output address parked in LDS as a double, at launches whose items lie 16 KiB .. 32 MiB apart;
  * the scratch `dTotJ` at 2048 doubles an item: its growth, its reuse at a smaller size, its independence from the `dTot` of `eval`,
    `grad` and `vjp` on the same handle;
  * the one-slot branch of `jvp_finish<32, 1024>`, which no runtime that grants 144 KiB of dynamic LDS ever takes: reached through the
    diagnostic override QC_SWEEP_JVP_ONE_SLOT in a fresh child process, bit for bit against the two-slot path of the parent and, on its
    own, against the reference; the override's stderr line proves which branch ran;
  * `gauss_newton_times` on a wide handle at 1204 items with per-sample weights in the loss.

Checks 1 to 6 of tests/test_sweep_jvp_every_sample.py, unchanged (`check_jvp`, `check_values`, `check_adjoint`).  Check 5, the adjoint
identity, pairs the `wide` = 17 handle's tangents with the pullback of a second handle that serves one: `wide` = 19 (closed cases), `wide`
= 27 with stored states (the Lindblad case); that handle's `tfinals` carry the bits of the first one's.  No tolerance is new: JVP_RTOL of
tests/test_sweep_jvp.py, the state and fidelity tolerances of tests/test_sweep.py, 2 JVP_RTOL max(1, |rhs|) for the adjoint identity, the
1e-9 max(1, max |want|) and the 1e-9 relative symmetry of test_sweep_wide_jvp.test_gauss_newton_product_on_a_wide_handle.
CPU: the launch table against the restated rule and `qc_sweep_desc_launch`, the soundness of sharing references on the wide shapes.
Measured worst ratios and times: profiles/sweep_wide_jvp_every_sample_summary.txt."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import sweep_jvp_reference as jref
import sweep_reference as ref
import test_sweep as ts
import test_sweep_every_sample as te
import test_sweep_jvp as tj
import test_sweep_vjp as tv
import test_sweep_wide as tw
import test_sweep_wide_jvp as twj
import test_sweep_jvp_every_sample as tje
from test_sweep_every_sample import CASES, GROWTH, KETS3, R, _frozen, assert_launch, classes
from test_sweep_jvp_every_sample import assert_reference_reuse_is_sound, build_rows, check_adjoint, check_jvp, check_values, jvp_call, launch_of, reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DENSITY = ("density", None, "abs")
# n = 32, full tiles, generators not antisymmetric: the case only forward mode serves without stored states
LINDBLAD = {"wide-lindblad-301": (("density", 4, 2, 1, True, True, 301, 24, DENSITY), True, (5, 5, 3), True)}
# the tuple layout of test_sweep_every_sample.CASES
TABLE = {"wide-sqrt-301": CASES["wide-sqrt-301"],                       # 1505 items: odd n_chunks, odd item count, scale = None with vscale given
         "wide-byS-683": CASES["wide-byS-683"],                         # 2049 items: the chunk count set by S, the fixed timestep (h_n = h)
         "wide-one-2049-kets3": KETS3["wide-one-2049-kets3"],           # past the fill threshold, one chunk, no tfids
         **LINDBLAD}
ITEMS_MOD_2 = {"wide-sqrt-301": 1, "wide-byS-683": 1, "wide-one-2049-kets3": 1, "wide-lindblad-301": 1}
CLOSED = [k for k in TABLE if k not in LINDBLAD]
TANGENT = dict(wide=True, wide_tangent=True)                            # wide = 17
# the handle whose pullback check 5 pairs the tangents with: wide = 19, and wide = 27 with reserved1[0] = 1 on the Lindblad case
PULLBACK = {**{k: dict(wide_params=True) for k in CLOSED}, "wide-lindblad-301": dict(wide_params=True, wide_stored=True, stored_states=True)}
GN = dict(N=9, m=2, T=11, S=301, launch=(3, 4, 1))                      # the Gauss-Newton launch: 1204 items, an even count
ONE_SLOT = "QC_SWEEP_JVP_ONE_SLOT"
ONE_SLOT_LINE = "qcolloc: QC_SWEEP_JVP_ONE_SLOT is active: pushforward finish kernel through one slot"
ONE_SLOT_CASES = ["many-columns", "n9-S5-T11", "two-qubit-lindblad", "wide-sqrt-301"]


def _N(spec):
    return spec[1] * spec[1] if spec[0] == "density" else spec[1]


def timed_reference(rows):
    """`reference(rows)` of the narrow file (computed once, shared, frozen), with the CPU time of its first build on the record."""
    t0 = time.process_time()
    fresh = rows["name"] not in tje._REF
    r = reference(rows)
    if fresh:
        print(f"SWEEP-WIDE-EVERY reference {rows['name']}: Frechet route over {R} rows built in {time.process_time() - t0:.2f} s of CPU time")
    return r


# ---------------------------------------------------------------------------------------------------------------------------------
#  CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_wide_launch_table(qc):
    """Every case sits on the edge it is named for, by the restated rule and by `qc_sweep_desc_launch` with `wide` = 17; the item counts
    are odd where the case is there for the wave that exits; no S whose class map nobody checks."""
    L = qc._lib
    for name, (spec, wide, (chunk, n_chunks, last), by_sqrt) in TABLE.items():
        state, levels, m, _, _, _, S, T, _ = spec
        N = _N(spec)
        assert wide and 16 < 2 * N <= 32, name
        want = tw.wide_launch(2 * N, m, S, T, True)
        assert want == dict(mfma=True, chunk=chunk, n_chunks=n_chunks, last=last, by_sqrt=by_sqrt), name
        assert (n_chunks - 1) * chunk + last == T - 1
        assert (S * n_chunks) % 2 == ITEMS_MOD_2[name], name
        D = tw._wdesc(qc, 17, N=N, m=m, T=T, cols=1)
        mf, ch, nch = C.c_int32(), C.c_int64(), C.c_int64()
        assert L.lib.qc_sweep_desc_launch(C.byref(D.d), S, C.byref(mf), C.byref(ch), C.byref(nch)) == L.QC_OK
        assert (bool(mf.value), ch.value, nch.value) == (True, chunk, n_chunks), name
    f = {k: TABLE[k][2] for k in TABLE}
    assert f["wide-sqrt-301"][1] % 2 == 1 and f["wide-lindblad-301"][1] % 2 == 1          # two-wave workgroups straddle samples
    assert 301 * 5 == 1505 and 683 * 3 == 2049 and -(-ts.SWEEP_FILL // 683) == 3 == f["wide-byS-683"][1]
    assert f["wide-one-2049-kets3"][1] == 1 and ts.SWEEP_FILL < 2049
    spec = LINDBLAD["wide-lindblad-301"][0]
    assert 2 * _N(spec) == 32 and TABLE["wide-byS-683"][0][5] is False and TABLE["wide-sqrt-301"][0][4] is False
    # no S here whose class map test_sweep_every_sample.test_classes_reach_both_ends leaves unchecked
    assert {TABLE[k][0][6] for k in TABLE} | set(GROWTH) | {GN["S"]} <= {CASES[k][0][6] for k in CASES} | set(te.GROWTH)
    # the scratch-growth sequence on one handle at T = 24: dTotJ grows, grows, and is then reused at a smaller size
    for name in ("wide-sqrt-301", "wide-lindblad-301"):
        sp = TABLE[name][0]
        assert sp[7] == 24 and [tw.wide_launch(2 * _N(sp), sp[2], S, 24)["n_chunks"] for S in GROWTH] == [5, 1, 5]
    assert GROWTH[0] * 5 < GROWTH[1] * 1 and GROWTH[2] * 5 < GROWTH[0] * 5
    # the Gauss-Newton launch: an even item count
    w = tw.wide_launch(2 * GN["N"], GN["m"], GN["S"], GN["T"])
    assert (w["chunk"], w["n_chunks"], w["last"]) == GN["launch"] and GN["S"] * w["n_chunks"] == 1204
    # the one-slot cases below: more than one chunk on three of them, 136 KiB on the first
    for name, want in (("n9-S5-T11", 4), ("two-qubit-lindblad", 3)):
        assert tw.wide_launch(32, 2, 5, {"n9-S5-T11": 11, "two-qubit-lindblad": 9}[name])["n_chunks"] == want
    assert tw.wide_launch(32, 2, 2, 3)["n_chunks"] == 2 and (4 * 4096 + 1024) * 8 == 136 * 1024


def test_pushforward_reference_reuse_is_sound(qc):
    """The narrow file's check on one wide closed shape (9 levels) and on the n = 32 Lindblad shape: equal rows give bit-equal Frechet
    references, distinct rows differ, the tangent rows matter on their own."""
    assert_reference_reuse_is_sound(qc, (("wide-closed", ("unitary", 9, 2, 1, True, True, R, 5, ("unitary", [0, 1, 3, 4], "abs"))),
                                         ("wide-lindblad", ("density", 4, 2, 1, True, True, R, 5, DENSITY))))


# ---------------------------------------------------------------------------------------------------------------------------------
#  GPU: every sample
# ---------------------------------------------------------------------------------------------------------------------------------
def same_bits(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        np.testing.assert_array_equal(a[k].view(np.uint64), b[k].view(np.uint64), err_msg=f"{what}: {k}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TABLE))
def test_wide_jvp_every_sample(qc, name):
    t_wall = time.perf_counter()
    rows = build_rows(qc, name, TABLE)
    c = launch_of(rows, TABLE[name][0][6])
    what = f"wide-every/{name}"
    timed_reference(rows)
    sw = ts.make_sweep(qc, rows, **TANGENT)
    back = None
    try:
        want = assert_launch(sw, name, table=TABLE)
        assert (c["S"] * want["n_chunks"]) % 2 == ITEMS_MOD_2[name]
        assert sw._desc.wide == 17 and sw.jvp_supported and sw.jvp_unsupported_reason is None
        assert sw.vjp_supported == (name in CLOSED) and sw.grad_supported == (name in CLOSED and rows["kind"] is not None)
        if name in LINDBLAD:
            assert rows["n"] == 32 and np.abs(rows["G0"] + rows["G0"].T).max() > 0.05 and not sw.stored_states
        if not TABLE[name][0][4]:
            assert c["scale"] is None and np.all(c["vscale"] != 0)              # the cl = 1, vcl != 0 path
        if not TABLE[name][0][5]:
            assert np.ndim(c["dts"]) == 0 and c["vdts"] is None                 # the h_n = h path
        Z, dirs, out = check_jvp(sw, rows, c, what)
        # 5: the adjoint identity against the pullback of a handle that serves one; its pushforward carries the bits of `sw`'s
        back = ts.make_sweep(qc, rows, **TANGENT, **PULLBACK[name])
        assert back._desc.wide == (19 if name in CLOSED else 27) and back._desc.reserved1[0] == (0 if name in CLOSED else 1)
        assert back.kernel_name == "mfma32-sweep" and back.vjp_supported and back.jvp_supported
        _, _, again = jvp_call(back, c)
        same_bits(again, out, f"{what}: the wide = {back._desc.wide} handle against the wide = 17 handle")
        check_adjoint(back, c, Z, dirs, again, what)
    finally:
        sw.close()
        if back is not None:
            back.close()
    print(f"SWEEP-WIDE-EVERY {what}: {time.perf_counter() - t_wall:.2f} s of wall time")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["wide-sqrt-301", "wide-lindblad-301"])
def test_wide_jvp_scratch_growth_every_sample(qc, name):
    """One handle at S = 301, then 2049, then 97 with T = 24: 5 chunks, 1, 5 again, so `dTotJ` grows to 301 x 5 x 2048 doubles, then to
    2049 x 2048, and is then reused at 97 x 5 x 2048.  At every S, in this order: `eval`, `jvp_device`, (closed handle, `wide` = 19) `vjp`
    with the adjoint check, `jvp_device`, `eval`.  The two pushforwards are bit-equal, each carries the bits of a fresh handle's and passes
    check 1, and `eval` afterwards returns the bits of `eval` before: `dTotJ` and the `dTot` of the other entry points do not touch each
    other."""
    t_wall = time.perf_counter()
    rows = build_rows(qc, name, TABLE)
    kw = dict(TANGENT, **(PULLBACK[name] if name in CLOSED else {}))
    timed_reference(rows)
    sw = ts.make_sweep(qc, rows, **kw)
    try:
        assert sw._desc.wide == (19 if name in CLOSED else 17)
        seen = []
        for S in GROWTH:
            c = launch_of(rows, S)
            seen.append(assert_launch(sw, name, S, table=TABLE)["n_chunks"])
            what = f"wide-every/{name} grown to S = {S}"
            Z = sw.pack(c["controls"], c["dts"])
            before = sw.eval(Z, c["init"], c["theta"], c["scale"])
            _, dirs, first = jvp_call(sw, c)
            if name in CLOSED:
                check_adjoint(sw, c, Z, dirs, first, what)
            _, _, second = jvp_call(sw, c)
            after = sw.eval(Z, c["init"], c["theta"], c["scale"])
            fresh = ts.make_sweep(qc, rows, **kw)
            try:
                _, _, third = jvp_call(fresh, c)
            finally:
                fresh.close()
            same_bits(second, first, f"{what}: the second call")
            same_bits(third, first, f"{what}: a fresh handle")
            check_values(first, rows, c, what)
            check_values(second, rows, c, what + ", second call")
            for a, b, k in zip(after, before, ("finals", "fids")):
                np.testing.assert_array_equal(a, b, err_msg=f"{what}: {k} of eval after the pushforward")
            np.testing.assert_array_equal(first["finals"], before[0].T)
            np.testing.assert_array_equal(first["fids"], before[1])
        assert seen == [5, 1, 5]
    finally:
        sw.close()
    print(f"SWEEP-WIDE-EVERY wide-every/{name} growth: {time.perf_counter() - t_wall:.2f} s of wall time")


# ---------------------------------------------------------------------------------------------------------------------------------
#  GPU: the one-slot branch of jvp_finish<32, 1024> in a fresh child process
# ---------------------------------------------------------------------------------------------------------------------------------
CHILD = """
import sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import test_sweep_wide_jvp_every_sample as t
t.child_main(sys.argv[2], sys.argv[3])
"""


def one_slot_case(qc, name):
    """(case, rows or None): the launch and, for the every-sample case, the R rows its reference is computed for."""
    if name == "many-columns":
        return twj.many_columns(qc), None
    if name in TABLE:
        rows = build_rows(qc, name, TABLE)
        return launch_of(rows, TABLE[name][0][6]), rows
    return twj.build(qc, name), None


def one_slot_calls(qc, c):
    """What parent and child both do: one `jvp_device` call with every output the handle has, one call of the host entry point.
    Returns the arrays and the number of pushforward launches made."""
    sw = twj.handle(qc, c)
    try:
        assert sw.kernel_name == "mfma32-sweep" and sw.jvp_supported
        Z = sw.pack(c["controls"], c["dts"])
        dirs = tj.direction(sw, c)
        out = tj.device_call(sw, Z, c, tj.outputs_of(sw), dirs)
        fid = "tfids" in out
        host = sw.jvp(Z, c["init"], dirs["vZ"], c["theta"], c["scale"], vinit=dirs["vinit"], vtheta=dirs["vtheta"], vscale=dirs["vscale"], fids=fid)
        out["host_tfinals"] = host[0] if fid else host
        if fid:
            out["host_tfids"] = host[1]
    finally:
        sw.close()
    return out, 2


def child_main(name, out_dir):
    """In the child: the calls of `one_slot_calls`, the arrays left in `out_dir`; the parent compares."""
    import __graft_entry__ as g
    qc = g.load_package()
    out, launches = one_slot_calls(qc, one_slot_case(qc, name)[0])
    np.savez(os.path.join(out_dir, "child.npz"), **out)
    print(f"ONE-SLOT child {name}: {launches} launches")


def run_child(name, value, out_dir):
    """One fresh child with QC_SWEEP_JVP_ONE_SLOT = value; nothing else is started before its return code is known to be 0."""
    env = dict(os.environ, **{ONE_SLOT: value})
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, name, str(out_dir)], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, f"the child ended with status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    assert f"ONE-SLOT child {name}: 2 launches" in r.stdout
    with np.load(os.path.join(out_dir, "child.npz")) as z:
        return {k: z[k] for k in z.files}, r.stderr.count(ONE_SLOT_LINE)


def check_against_the_reference(out, c, rows, what):
    """The reference check of the case, on these arrays alone: every sample of the every-sample case by its class (`check_values`), the
    cases of tests/test_sweep_wide_jvp.py by the assertions of `tj.check_case` and `test_many_columns`."""
    four = {k: out[k] for k in tj.OUTPUTS if k in out}
    if rows is not None:
        check_values(four, rows, c, what)
    else:
        r = tj.reference(c)
        tj.assert_samples(out["tfinals"], r["tfinals"], f"{what} tfinals")
        np.testing.assert_allclose(out["finals"], r["finals"], rtol=ts.STATE_RTOL, atol=ts.STATE_ATOL, err_msg=f"{what} finals")
        if "tfids" in out:
            tj.assert_samples(out["tfids"][:, None], r["tfids"][:, None], f"{what} tfids")
            ts._assert_fids(out["fids"], ts.reference(c)[1], f"SWEEP-WIDE-EVERY {what} fids")
    np.testing.assert_array_equal(out["host_tfinals"], out["tfinals"], err_msg=f"{what}: host tfinals")
    if "tfids" in out:
        np.testing.assert_array_equal(out["host_tfids"], out["tfids"], err_msg=f"{what}: host tfids")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ONE_SLOT_CASES)
def test_one_slot_finish_path_in_a_child(qc, name, tmp_path, capfd):
    """The parent makes the calls without the override (the two-slot path: its stderr does not carry the override's line); one fresh child
    makes them with QC_SWEEP_JVP_ONE_SLOT=1.  The child's line occurs once per pushforward launch, every array of the child is bit-equal to
    the parent's, and the child's arrays pass the reference check of their case on their own."""
    t_wall = time.perf_counter()
    assert os.environ.get(ONE_SLOT) in (None, "", "0"), "the parent must run without the override"
    c, rows = one_slot_case(qc, name)
    if name == "many-columns":
        assert (4 * c["init"].size + 1024) * 8 == 136 * 1024 and tw.wide_launch(c["n"], c["m"], c["S"], c["T"])["n_chunks"] == 2
    if rows is not None:
        timed_reference(rows)
    capfd.readouterr()
    mine, launches = one_slot_calls(qc, c)
    assert ONE_SLOT_LINE not in capfd.readouterr().err
    assert set(mine) == ({"finals", "tfinals", "host_tfinals"} | ({"fids", "tfids", "host_tfids"} if c["kind"] is not None else set()))
    theirs, lines = run_child(name, "1", tmp_path)
    assert lines == launches == 2, f"{lines} lines on the child's stderr for {launches} launches"
    same_bits(theirs, mine, f"one-slot/{name}: the child under {ONE_SLOT}=1 against the parent")
    check_against_the_reference(theirs, c, rows, f"one-slot/{name}")
    check_against_the_reference(mine, c, rows, f"two-slot/{name}")
    print(f"SWEEP-WIDE-EVERY one-slot/{name}: {time.perf_counter() - t_wall:.2f} s of wall time")


@pytest.mark.gpu
@pytest.mark.parametrize("value", ["0", "abc"])
def test_one_slot_override_zero_and_garbage_mean_not_set(qc, value, tmp_path):
    """QC_SWEEP_JVP_ONE_SLOT=0 and text: the line does not occur, the arrays are the parent's."""
    name = "n9-S5-T11"
    c, _ = one_slot_case(qc, name)
    mine, _ = one_slot_calls(qc, c)
    theirs, lines = run_child(name, value, tmp_path)
    assert lines == 0
    same_bits(theirs, mine, f"{ONE_SLOT}={value}")


# ---------------------------------------------------------------------------------------------------------------------------------
#  GPU: Gauss-Newton products at a mid-size launch
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gauss_newton_product_at_a_mid_size_launch(qc):
    """`gauss_newton_times` on 9 levels (m = 2, T = 11) at S = 301 -- the launch (3, 4, 1), 1204 items -- with theta and scale the R rows
    expanded by `classes(301)` and per-sample weights in the loss, sum_s w_s ||X_s - G||^2 / 2, against sum_r W_r J_r^T J_r v, W_r the
    weight of class r, J_r from the Frechet route over the 30 unit directions of the R rows (computed once): 1e-9 max(1, max |want|);
    symmetry; the device-tensor call against the host call bit for bit."""
    t_wall = time.perf_counter()
    rng = np.random.default_rng(43)
    N, m, T, S = GN["N"], GN["m"], GN["T"], GN["S"]
    traj = tv._traj3(qc, rng, N, m, T)
    H0, Hd, P = ts._herm(rng, N), [ts._herm(rng, N, 0.5) for _ in range(m)], ts._herm(rng, N)
    sys_ = qc.QuantumSystem(H0, Hd)
    cls, w = classes(S), te.weights(S)
    theta_r, scale_r = rng.uniform(-0.2, 0.2, (R, 1)), rng.uniform(0.9, 1.1, (R, m))
    theta, scale = np.ascontiguousarray(theta_r[cls]), np.ascontiguousarray(scale_r[cls])
    goal = torch.from_numpy(np.ascontiguousarray(traj.goal["Ũ⃗"])).cuda()
    dw = torch.from_numpy(w).cuda()
    obj = qc.SweepFinalStateObjective(traj, sys_, [P], theta, lambda X: ((X - goal) ** 2 * dw[:, None]).sum() / 2, scale=scale, wide=True, wide_tangent=True)
    Z = traj.datavec
    nZ = Z.size
    try:
        want_launch = tw.wide_launch(2 * N, m, S, T)
        assert obj.wide_tangent and obj._sweep.kernel_name == "mfma32-sweep" and obj._sweep.launch(S) == (True, want_launch["chunk"], want_launch["n_chunks"])
        assert (want_launch["chunk"], want_launch["n_chunks"], want_launch["last"]) == GN["launch"] and (S * want_launch["n_chunks"]) % 2 == 0
        G0, Gd, Gp = ref.iso_generator(H0), [ref.iso_generator(H) for H in Hd], [ref.iso_generator(P)]
        a0, dt0 = traj.offset("a"), traj.offset("Δt")
        K = Z[:T * traj.dim].reshape(T, traj.dim)
        controls, dts, init = K[:, a0:a0 + m].T.copy(), K[:, dt0].copy(), traj.initial["Ũ⃗"]
        t0 = time.process_time()
        J = np.zeros((R, init.size, nZ))
        directions = 0
        for t in range(T - 1):
            for o in list(range(a0, a0 + m)) + [dt0]:
                va, vh = np.zeros((m, T)), np.zeros(T)
                if o == dt0:
                    vh[t] = 1.0
                else:
                    va[o - a0, t] = 1.0
                J[:, :, t * traj.dim + o] = jref.pushforward_frechet(G0, Gd, Gp, controls, dts, init, theta_r, scale_r, range(R), va, vh)["tfinals"]
                directions += 1
        (J,) = _frozen((J,))
        assert directions == 30
        print(f"SWEEP-WIDE-EVERY reference gauss-newton: {directions} unit directions on {R} rows built in {time.process_time() - t0:.2f} s of CPU time")
        W = np.bincount(cls, weights=w, minlength=R)
        assert np.all(W > 0) and len(set(w[cls == 0])) > 1
        u, v = rng.standard_normal(nZ), rng.standard_normal(nZ)
        want = np.einsum("rnz,rn->z", J, W[:, None] * np.einsum("rnz,z->rn", J, v))
        got = obj.gauss_newton_times(Z, v)
        assert got.shape == (nZ,)
        err = np.abs(got - want).max() / max(1.0, np.abs(want).max())
        print(f"SWEEP-WIDE-EVERY gauss_newton_times at S = {S} vs sum_r W_r J_r^T J_r v: error / bound = {err / 1e-9:.3e} (bound 1e-9 max(1, max |want|)), "
              f"max |value| {np.abs(want).max():.3f}")
        assert err <= 1e-9 and np.abs(want).max() > 1e-3
        gu = obj.gauss_newton_times(Z, u)
        sym = abs(u @ got - v @ gu) / abs(u @ got)
        print(f"SWEEP-WIDE-EVERY gauss_newton_times symmetry: |u.Gv - v.Gu| / |u.Gv| / bound = {sym / 1e-9:.3e} (bound 1e-9), |u.Gv| = {abs(u @ got):.3e}")
        assert abs(u @ got - v @ gu) <= 1e-9 * abs(u @ got) and abs(u @ got) > 1e-3
        dgot = obj.gauss_newton_times(torch.from_numpy(Z).cuda(), torch.from_numpy(v).cuda())
        assert torch.is_tensor(dgot) and dgot.is_cuda
        np.testing.assert_array_equal(dgot.cpu().numpy(), got)
    finally:
        obj.close()
    print(f"SWEEP-WIDE-EVERY gauss-newton: {time.perf_counter() - t_wall:.2f} s of wall time")
