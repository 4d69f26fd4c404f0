"""A/B of the rollout sweep against the per-system loop it replaces, device events, one process, alternating rounds.

  (a) one qc_sweep_eval_dev over S perturbed systems
  (b) S handles created beforehand, one per perturbed system; S x (qc_rollout_dev + qc_fidelity_eval_dev) in a loop on one stream
      (handle creation is timed separately and reported)

Sizes: config 3's system (N = 8, m = 6) at T = 1000 with S in {64, 1024, 8192}, and the reference robustness check's size
(N = 2, T = 50) with S = 8192.  Where S = 8192 handles are impractical for (b), it runs at 1024 and is scaled linearly (said in the
output).  `--trace S` runs path (a) alone a few times at config 3's size, for a separate `rocprofv3 --kernel-trace --stats` run.

    python profiles/sweep_probe.py [--rounds 5] [--out profiles/sweep_summary.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

MAX_B_HANDLES = 1024
PEAK_F64_MATRIX_TFLOPS = 78.6      # MI355X, vendor figure for FP64 matrix


def squarings(norm):
    sq = 0
    while norm / 2.0 ** sq > 0.125:
        sq += 1
    return sq


def make_problem(qc, which, T, S, rng):
    if which == "config3":
        inp = qc.config_inputs(3, T=T)
        base = inp.system
        H0, Hd = base.H_drift, base.H_drives
        N = base.levels
        Zq = np.kron(qc.GATES["Z"], np.eye(N // 2))                # detuning of the first qubit
        goal = qc.operator_to_iso_vec(qc.GATES["TOFFOLI"]) if qc.GATES["TOFFOLI"].shape[0] == N else qc.operator_to_iso_vec(np.eye(N, dtype=complex))
        controls = np.asarray(inp.traj["a"], dtype=np.float64)
        ts = inp.traj.timestep
        dts = np.asarray(inp.traj[ts]).ravel() if isinstance(ts, str) else np.full(T, float(ts))
    else:   # the reference's robustness check: systems(zeta) = QuantumSystem(zeta Z, [X, Y]), H gate, dt = 0.2
        N = 2
        H0, Hd, Zq = np.zeros((2, 2), dtype=complex), [qc.GATES["X"], qc.GATES["Y"]], qc.GATES["Z"]
        goal = qc.operator_to_iso_vec(qc.GATES["H"])
        controls, dts = rng.uniform(-1, 1, (2, T)), np.full(T, 0.2)
    m = len(Hd)
    theta = rng.uniform(-0.05, 0.05, (S, 1))
    scale = 1.0 + rng.uniform(-0.02, 0.02, (S, m))
    return dict(N=N, m=m, T=T, S=S, H0=np.asarray(H0, dtype=complex), Hd=[np.asarray(H, dtype=complex) for H in Hd], P=np.asarray(Zq, dtype=complex),
                goal=goal, controls=controls, dts=dts, theta=theta, scale=scale)


def event_ms(fn, stream):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def run_size(qc, which, T, S, rounds, rng, log):
    L = qc._lib
    pb = make_problem(qc, which, T, S, rng)
    N, m = pb["N"], pb["m"]
    n, s = 2 * N, 2 * N * N
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    init = qc.operator_to_iso_vec(np.eye(N, dtype=complex))
    # ---- (a) --------------------------------------------------------------------------------------------------------------
    t0 = time.perf_counter()
    sw = qc.RolloutSweep(qc.QuantumSystem(pb["H0"], pb["Hd"]), [pb["P"]], T, goal=pb["goal"], fid_kind="unitary")
    create_a = time.perf_counter() - t0
    dZa, dinit, dth, dsc = t(sw.pack(pb["controls"], pb["dts"])), t(init), t(pb["theta"]), t(pb["scale"])
    dfid = torch.empty(S, dtype=torch.float64, device=dev)
    path_a = lambda: sw.eval_device(dZa, dinit, dth, dsc, None, dfid, stream=stream)
    # ---- (b) --------------------------------------------------------------------------------------------------------------
    Sb = min(S, MAX_B_HANDLES)
    Zb = np.zeros((T, s + m + 1))
    Zb[:, s:s + m] = pb["controls"].T
    Zb[:, s + m] = pb["dts"]
    dZb = t(Zb)
    dout = torch.empty((T, s), dtype=torch.float64, device=dev)
    dval = torch.empty((Sb, 2), dtype=torch.float64, device=dev)
    handles, keep = [], []
    t0 = time.perf_counter()
    for k in range(Sb):
        sysk = qc.QuantumSystem(pb["H0"] + pb["theta"][k, 0] * pb["P"], [pb["scale"][k, j] * pb["Hd"][j] for j in range(m)])
        d = L.qc_desc()
        d.N, d.m, d.T, d.zdim, d.global_dim = N, m, T, s + m + 1, 0
        d.off_U, d.off_a, d.off_dt, d.dt_fixed = 0, s, s + m, 0.0
        d.integrator, d.pade_order, d.n_deriv = L.QC_EXPONENTIAL, 0, 0
        G0 = np.asfortranarray(sysk.G_drift, dtype=np.float64)
        Gd = np.ascontiguousarray(np.stack([np.asarray(G, dtype=np.float64).reshape(-1, order="F") for G in sysk.G_drives]))
        keep.append((G0, Gd))
        d.G_drift, d.G_drives = L.dptr(G0), L.dptr(Gd)
        d.device, d.kernel = 0, L.QC_KERNEL_LDS
        h = C.c_void_p()
        L.check(L.lib.qc_create(C.byref(d), C.byref(h)))
        handles.append(h)
    fh = C.c_void_p()
    rc = L.lib.qc_fidelity_create(N, L.dptr(np.ascontiguousarray(pb["goal"])), None, 0, 0, C.byref(fh))
    assert rc == 0
    create_b = time.perf_counter() - t0
    last = dout.data_ptr() + (T - 1) * s * 8
    st = stream.cuda_stream

    def path_b():
        for k, h in enumerate(handles):
            rc1 = L.lib.qc_rollout_dev(h, dZb.data_ptr(), dinit.data_ptr(), dout.data_ptr(), st)
            rc2 = L.lib.qc_fidelity_eval_dev(fh, last, dval.data_ptr() + 16 * k, None, None, st)
            if rc1 or rc2:
                raise RuntimeError(f"path (b), system {k}: qc_rollout_dev -> {rc1}, qc_fidelity_eval_dev -> {rc2}")

    with torch.cuda.stream(stream):
        for _ in range(2):      # warm-up: scratch of both paths, code objects
            path_a()
            path_b()
        stream.synchronize()
        fa = dfid.cpu().numpy()[:Sb].copy()
        fb = dval.cpu().numpy()[:, 0].copy()
        ta, tb = [], []
        for _ in range(rounds):
            ta.append(event_ms(path_a, stream))
            tb.append(event_ms(path_b, stream) * (S / Sb))
    agree = float(np.abs(fa - fb).max())
    # MFMAs per interval from the shapes: 8 Horner steps and the product of 4 each, 4 per squaring
    G0 = qc.iso_generator(pb["H0"])
    Gd = [qc.iso_generator(H) for H in pb["Hd"]]
    sqs = [squarings(np.abs(pb["dts"][k] * (G0 + sum(a * G for a, G in zip(pb["controls"][:, k], Gd)))).sum(axis=0).max()) for k in range(T - 1)]
    mfma = 36 + 4 * float(np.mean(sqs))
    flops = S * (T - 1) * mfma * 2 * 16 * 16 * 4
    log(f"== {which}: N = {N}, m = {m}, T = {T}, S = {S}; sweep kernel {sw.kernel_name}, (mfma, chunk, n_chunks) = {sw.launch(S)}")
    log(f"   (a) one qc_sweep_eval_dev           ms per round: {' '.join(f'{x:.3f}' for x in ta)}   (handle creation {create_a * 1e3:.1f} ms)")
    scaled = f", timed at S = {Sb} and scaled by {S // Sb}" if Sb != S else ""
    log(f"   (b) S x (rollout + fidelity){scaled}   ms per round: {' '.join(f'{x:.3f}' for x in tb)}   (creation of {Sb} handles {create_b * 1e3:.1f} ms, not included)")
    log(f"   ratio of medians (b)/(a) = {np.median(tb) / np.median(ta):.1f};  every (a) below every (b): {max(ta) < min(tb)};  max |F_a - F_b| over {Sb} samples = {agree:.2e}")
    log(f"   squarings per interval: mean {np.mean(sqs):.2f} (unperturbed system) -> {mfma:.1f} MFMAs (16x16x4 f64) per interval, {flops / 1e9:.2f} GFLOP per call:"
        f" {flops / (np.median(ta) * 1e-3) / 1e12:.2f} TFLOP/s over the whole call = {100 * flops / (np.median(ta) * 1e-3) / 1e12 / PEAK_F64_MATRIX_TFLOPS:.1f} % of {PEAK_F64_MATRIX_TFLOPS} (timing by events; the kernel's own share: the trace)")
    for h in handles:
        L.lib.qc_destroy(h)
    L.lib.qc_fidelity_destroy(fh)
    sw.close()
    if not agree <= 1e-9:
        log(f"   THE TWO PATHS DISAGREE: max |F_a - F_b| = {agree:.2e} > 1e-9")
    return max(ta) < min(tb), agree <= 1e-9


def trace_only(qc, S, reps=5):
    rng = np.random.default_rng(0)
    pb = make_problem(qc, "config3", 1000, S, rng)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    sw = qc.RolloutSweep(qc.QuantumSystem(pb["H0"], pb["Hd"]), [pb["P"]], 1000, goal=pb["goal"], fid_kind="unitary")
    dZ, dinit, dth, dsc = t(sw.pack(pb["controls"], pb["dts"])), t(qc.operator_to_iso_vec(np.eye(pb["N"], dtype=complex))), t(pb["theta"]), t(pb["scale"])
    dfid = torch.empty(S, dtype=torch.float64, device=dev)
    for _ in range(reps):
        sw.eval_device(dZ, dinit, dth, dsc, None, dfid)
    torch.cuda.synchronize()
    sw.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", type=int, default=0, help="path (a) alone at config 3's size with this S (for a kernel trace)")
    ap.add_argument("--sizes", default="config3:1000:64,config3:1000:1024,config3:1000:8192,qubit:50:8192")
    args = ap.parse_args()
    qc = g.load_package()
    if args.trace:
        trace_only(qc, args.trace)
        return 0
    lines = []

    def log(sx):
        print(sx, flush=True)
        lines.append(sx)

    log(f"rollout sweep A/B, {torch.cuda.get_device_name(0)}, {qc._lib.lib.qc_version().decode()}; device events, {args.rounds} alternating rounds after 2 warm-up rounds")
    rng = np.random.default_rng(0)
    ok = True
    for spec in args.sizes.split(","):
        which, T, S = spec.split(":")
        won, same = run_size(qc, which, int(T), int(S), args.rounds, rng, log)
        ok = ok and same              # a baseline that computes something else is no baseline
        if int(S) >= 1024:
            ok = ok and won
    log(f"acceptance (every round of (a) below every round of (b) at S >= 1024, the two paths' fidelities within 1e-9 at every size): {'met' if ok else 'NOT met'}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
