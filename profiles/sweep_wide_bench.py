#!/usr/bin/env python3
"""The wide sweep ("mfma32-sweep", 16 < 2N <= 32) against the path the same descriptor takes without the flag, and its gradient.

Systems: config 5's (4 qubits, N = 16, 8 drives, its own T = 500) and two coupled three-level transmons (N = 9, 4 drives, T = 100,
examples/transmon_robustness.py), each at S in {64, 1024}:

    (a) qc_sweep_eval_dev on a handle with wide = QC_SWEEP_WIDE      the S fidelities, "mfma32-sweep"
    (b) qc_sweep_eval_dev on the same descriptor with wide = 0        "rollout-per-sample": what (a) has to beat
    (c) qc_sweep_grad_dev on the wide handle                          J and the dense gradient

timed by device events on one stream, (a), (b), (c) alternating over the rounds after one warm-up round.  Done means every round of
(a) is below every round of (b).  (c) / (a) is held against the kernels' MFMA counts per interval: forward 288 + 32 sq, gradient walk
848 + 96 sq on top of the forward totals it launches first.  The share of the f64 matrix peak is the MFMA work of the call over the
call's time: an end-to-end figure, not a kernel's.

    python profiles/sweep_wide_bench.py [--rounds 5] [--out profiles/sweep_wide_summary.txt]
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


def make_problem(qc, which, S, rng):
    if which == "config5":
        inp = qc.config_inputs(5)
        system, T = inp.system, inp.traj.T
        N = system.levels
        P = np.kron(qc.GATES["Z"], np.eye(N // 2))                  # detuning of the first qubit
        goal = np.asarray(inp.traj.goal["Ũ⃗"], dtype=np.float64)
        controls = np.asarray(inp.traj["a"], dtype=np.float64)
        ts = inp.traj.timestep
        dts = np.asarray(inp.traj[ts]).ravel() if isinstance(ts, str) else np.full(T, float(ts))
        subspace = None
        width = 0.05
    else:
        import transmon_robustness as tr
        H0, drives, P = tr.two_transmons()
        system, T, N = qc.QuantumSystem(H0, drives), 100, 9
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


def run_size(qc, which, S, rounds, rng, log):
    pb = make_problem(qc, which, S, rng)
    T, N, m = pb["T"], pb["N"], pb["m"]
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    mk = lambda wide: qc.RolloutSweep(pb["system"], [pb["P"]], T, goal=pb["goal"], fid_kind="unitary", subspace=pb["subspace"], wide=wide)
    wide, narrow = mk(True), mk(False)
    assert wide.kernel_name == "mfma32-sweep" and narrow.kernel_name == "rollout-per-sample" and wide.grad_supported
    b = dict(dZ=t(wide.pack(pb["controls"], pb["dts"])), dinit=t(qc.operator_to_iso_vec(np.eye(N, dtype=complex))), dth=t(pb["theta"]), dsc=t(pb["scale"]),
             fa=torch.empty(S, dtype=torch.float64, device=dev), fb=torch.empty(S, dtype=torch.float64, device=dev),
             dJ=torch.empty(1, dtype=torch.float64, device=dev), dg=torch.empty(wide.Z_len, dtype=torch.float64, device=dev))
    stream = torch.cuda.Stream(device=dev)
    fa = lambda: wide.eval_device(b["dZ"], b["dinit"], b["dth"], b["dsc"], None, b["fa"], stream=stream)
    fb = lambda: narrow.eval_device(b["dZ"], b["dinit"], b["dth"], b["dsc"], None, b["fb"], stream=stream)
    fc = lambda: wide.grad_device(b["dZ"], b["dinit"], S, b["dth"], b["dsc"], None, None, b["dJ"], b["dg"], None, stream=stream)
    with torch.cuda.stream(stream):
        fa(); fb(); fc()
        stream.synchronize()
        ta, tb, tc = [], [], []
        for _ in range(rounds):
            ta.append(event_ms(fa, stream))
            tb.append(event_ms(fb, stream))
            tc.append(event_ms(fc, stream))
    agree = float((b["fa"] - b["fb"]).abs().max().item())
    G0 = qc.iso_generator(np.asarray(pb["system"].H_drift))
    Gd = [qc.iso_generator(np.asarray(H)) for H in pb["system"].H_drives]
    sq = float(np.mean([squarings(np.abs(pb["dts"][k] * (G0 + sum(a * G for a, G in zip(pb["controls"][:, k], Gd)))).sum(axis=0).max()) for k in range(T - 1)]))
    mf_f, mf_g = 288 + 32 * sq, 848 + 96 * sq
    per_mfma = 2 * 16 * 16 * 4
    fl_a, fl_c = S * (T - 1) * mf_f * per_mfma, S * (T - 1) * (mf_f + mf_g) * per_mfma
    share = lambda fl, ms: 100 * fl / (ms * 1e-3) / 1e12 / PEAK_F64_MATRIX_TFLOPS
    fmt = lambda xs: " ".join(f"{x:.3f}" for x in xs)
    log(f"== {which}: N = {N} (2N = {2 * N}), m = {m}, T = {T}, S = {S}; launch of the wide handle (mfma, chunk, n_chunks) = {wide.launch(S)}; "
        f"squarings per interval (unperturbed): mean {sq:.2f}")
    log(f"   (a) wide forward sweep        ms per round: {fmt(ta)}   min {min(ta):.3f}  median {np.median(ta):.3f}")
    log(f"   (b) wide = 0, per-sample form ms per round: {fmt(tb)}   min {min(tb):.3f}  median {np.median(tb):.3f}")
    log(f"   (c) wide gradient             ms per round: {fmt(tc)}   min {min(tc):.3f}  median {np.median(tc):.3f}")
    log(f"   every round of (a) below every round of (b): {max(ta) < min(tb)}; median (b) / median (a) = {np.median(tb) / np.median(ta):.1f}; "
        f"max |F(a) - F(b)| = {agree:.2e}")
    log(f"   median (c) / median (a) = {np.median(tc) / np.median(ta):.2f}; MFMA counts per interval: forward {mf_f:.0f}, walk {mf_g:.0f}: "
        f"expected {(mf_f + mf_g) / mf_f:.2f}")
    log(f"   MFMA work over the call's time, of {PEAK_F64_MATRIX_TFLOPS} TFLOP/s (f64 matrix, vendor figure): (a) {share(fl_a, np.median(ta)):.1f} %, "
        f"(c) {share(fl_c, np.median(tc)):.1f} %  (whole calls by device events, not kernel times)")
    wide.close()
    narrow.close()
    return max(ta) < min(tb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="64,1024")
    ap.add_argument("--systems", default="config5,transmons")
    args = ap.parse_args()
    qc = g.load_package()
    lines = []

    def log(sx):
        print(sx, flush=True)
        lines.append(sx)

    log(f"wide sweep against the per-sample form, {torch.cuda.get_device_name(0)}, {qc._lib.lib.qc_version().decode()}; device events, "
        f"{args.rounds} alternating rounds (a), (b), (c) after one warm-up round, one process")
    rng = np.random.default_rng(0)
    ok = True
    for which in args.systems.split(","):
        for S in args.sizes.split(","):
            ok = run_size(qc, which, int(S), args.rounds, rng, log) and ok
    log(f"every round of (a) below every round of (b), at every size: {ok}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
