#!/usr/bin/env python3
"""The "mfma64-sweep" form (32 < 2N <= 64) against the path the same descriptor takes without QC_SWEEP_WIDE_64.

Systems: 5 qubits (`multi_qubit_system(5)`, N = 32, 10 drives) and three coupled three-level transmons (N = 27, 6 drives,
examples/three_transmon_robustness.py), T = 100, each at S in {64, 1024}:

    (a) qc_sweep_eval_dev on a handle with wide = QC_SWEEP_WIDE | QC_SWEEP_WIDE_64     the S fidelities, "mfma64-sweep"
    (b) qc_sweep_eval_dev on the same descriptor with wide = QC_SWEEP_WIDE             "rollout-per-sample": what (a) has to beat

timed by device events on one stream, (a) and (b) alternating over the rounds after one warm-up round, one process.  "faster" is written
only where every round of (a) is below every round of (b).  The share of the f64 matrix peak is the MFMA work of the call,
(kDeg + sq + 1) x 256 instructions of 16 x 16 x 4 per interval with the sq every sample takes in every interval (recomputed on the host), over the call's time: an end-to-end figure,
not a kernel's.  `--trace S` runs (a) alone a few times on the transmon system, for a separate `rocprofv3 --kernel-trace --stats` run
that gives the sweep kernel's share of the call.

    python profiles/sweep_wide64_bench.py [--rounds 5] [--out profiles/sweep_wide64_summary.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
import __graft_entry__ as g  # noqa: E402
from sweep_probe import PEAK_F64_MATRIX_TFLOPS, event_ms, squarings  # noqa: E402

K_DEG = 8


def make_problem(qc, which, S, T, rng):
    if which == "qubits5":
        system = qc.multi_qubit_system(5)
        N = system.levels
        P = np.kron(qc.GATES["Z"], np.eye(N // 2))                  # detuning of the first qubit
        goal = qc.operator_to_iso_vec(np.kron(qc.GATES["X"], np.eye(N // 2)).astype(complex))
        controls = rng.uniform(-1, 1, (system.n_drives, T))
        dts = np.full(T, 0.2)
        subspace = None
        width = 0.05
    else:
        import three_transmon_robustness as tr
        H0, drives, P = tr.three_transmons()
        system, N = qc.QuantumSystem(H0, drives), 27
        goal = qc.operator_to_iso_vec(tr.goal_gate())
        window = np.sin(np.pi * np.linspace(0.0, 1.0, T)) ** 2
        controls = 0.08 * rng.uniform(-1, 1, (len(drives), 1)) * window
        dts = np.full(T, 40.0 / (T - 1))
        subspace = tr.SUBSPACE
        width = 2 * np.pi * 0.002
    m = system.n_drives
    theta = rng.uniform(-width, width, (S, 1))
    scale = 1.0 + rng.uniform(-0.02, 0.02, (S, m))
    return dict(which=which, N=N, m=m, T=T, S=S, system=system, P=np.asarray(P, dtype=complex), goal=goal, controls=controls, dts=dts, theta=theta,
                scale=scale, subspace=subspace)


def handles(qc, pb):
    mk = lambda w64: qc.RolloutSweep(pb["system"], [pb["P"]], pb["T"], goal=pb["goal"], fid_kind="unitary", subspace=pb["subspace"], wide=True, wide64=w64)
    new, old = mk(True), mk(False)
    assert new.kernel_name == "mfma64-sweep" and old.kernel_name == "rollout-per-sample"
    return new, old


def mean_squarings(qc, pb):
    """The mean number of squarings over every (sample, interval) of the call, from the generators the kernel forms:
    G_s(a_t) = G_drift + theta[s] P + sum_k scale[s, k] a_k(t) G_k, the rule on the largest column sum of |dt_t G_s(a_t)|."""
    G0 = qc.iso_generator(np.asarray(pb["system"].H_drift))
    Gd = np.stack([qc.iso_generator(np.asarray(H)) for H in pb["system"].H_drives])
    base = G0[None] + pb["theta"][:, 0, None, None] * qc.iso_generator(pb["P"])[None]          # S x n x n
    total = 0
    for k in range(pb["T"] - 1):
        G = base + np.einsum("sm,mij->sij", pb["scale"] * pb["controls"][None, :, k], Gd)
        norms = np.abs(pb["dts"][k] * G).sum(axis=1).max(axis=1)
        total += sum(squarings(v) for v in norms)
    return total / (pb["S"] * (pb["T"] - 1))


def run_size(qc, which, S, T, rounds, rng, log):
    pb = make_problem(qc, which, S, T, rng)
    N, m = pb["N"], pb["m"]
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    new, old = handles(qc, pb)
    b = dict(dZ=t(new.pack(pb["controls"], pb["dts"])), dinit=t(qc.operator_to_iso_vec(np.eye(N, dtype=complex))), dth=t(pb["theta"]), dsc=t(pb["scale"]),
             fa=torch.empty(S, dtype=torch.float64, device=dev), fb=torch.empty(S, dtype=torch.float64, device=dev))
    stream = torch.cuda.Stream(device=dev)
    fa = lambda: new.eval_device(b["dZ"], b["dinit"], b["dth"], b["dsc"], None, b["fa"], stream=stream)
    fb = lambda: old.eval_device(b["dZ"], b["dinit"], b["dth"], b["dsc"], None, b["fb"], stream=stream)
    with torch.cuda.stream(stream):
        fa(); fb()
        stream.synchronize()
        ta, tb = [], []
        for _ in range(rounds):
            ta.append(event_ms(fa, stream))
            tb.append(event_ms(fb, stream))
    agree = float((b["fa"] - b["fb"]).abs().max().item())
    sq = mean_squarings(qc, pb)
    mfmas = (K_DEG + sq + 1) * 256
    flops = S * (T - 1) * mfmas * 2 * 16 * 16 * 4
    share = 100 * flops / (np.median(ta) * 1e-3) / 1e12 / PEAK_F64_MATRIX_TFLOPS
    fmt = lambda xs: " ".join(f"{x:.3f}" for x in xs)
    faster = max(ta) < min(tb)
    log(f"== {which}: N = {N} (2N = {2 * N}), m = {m}, T = {T}, S = {S}; launch of the new handle (mfma, chunk, n_chunks) = {new.launch(S)}; "
        f"squarings per interval, mean over every sample and interval: {sq:.3f}")
    log(f"   (a) mfma64-sweep               ms per round: {fmt(ta)}   min {min(ta):.3f}  median {np.median(ta):.3f}")
    log(f"   (b) same descriptor, no bit 10 ms per round: {fmt(tb)}   min {min(tb):.3f}  median {np.median(tb):.3f}")
    log(f"   every round of (a) below every round of (b): {faster}{' -- faster' if faster else ' -- NOT faster'}; median (b) / median (a) = "
        f"{np.median(tb) / np.median(ta):.1f}; max |F(a) - F(b)| = {agree:.2e}")
    log(f"   MFMA work {mfmas:.0f} instructions per interval, {flops / 1e9:.1f} GFLOP per call, over the call's time: {flops / (np.median(ta) * 1e-3) / 1e12:.2f} "
        f"TFLOP/s = {share:.1f} % of {PEAK_F64_MATRIX_TFLOPS} TFLOP/s (f64 matrix, vendor figure; whole call by device events, not a kernel time)")
    new.close()
    old.close()
    return faster


def trace_only(qc, S, T, reps=5):
    pb = make_problem(qc, "transmons3", S, T, np.random.default_rng(0))
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    new, old = handles(qc, pb)
    old.close()
    dZ, dinit, dth, dsc = t(new.pack(pb["controls"], pb["dts"])), t(qc.operator_to_iso_vec(np.eye(pb["N"], dtype=complex))), t(pb["theta"]), t(pb["scale"])
    dfid = torch.empty(S, dtype=torch.float64, device=dev)
    for _ in range(reps):
        new.eval_device(dZ, dinit, dth, dsc, None, dfid)
    torch.cuda.synchronize()
    new.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--sizes", default="64,1024")
    ap.add_argument("--systems", default="qubits5,transmons3")
    ap.add_argument("--trace", type=int, default=0, help="(a) alone on the transmon system with this S (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sweep_wide64_bench.py measures on a GPU; none is visible")
    qc = g.load_package()
    if args.trace:
        trace_only(qc, args.trace, args.T)
        return 0
    lines = []

    def log(sx):
        print(sx, flush=True)
        lines.append(sx)

    log(f"mfma64-sweep against the per-sample form, {torch.cuda.get_device_name(0)}, {qc._lib.lib.qc_version().decode()}; device events, "
        f"{args.rounds} alternating rounds (a), (b) after one warm-up round, one process")
    rng = np.random.default_rng(0)
    ok = True
    for which in args.systems.split(","):
        for S in args.sizes.split(","):
            ok = run_size(qc, which, int(S), args.T, args.rounds, rng, log) and ok
    log(f"every round of (a) below every round of (b), at every size: {ok}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
