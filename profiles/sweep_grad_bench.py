#!/usr/bin/env python3
"""Sweep gradients against the forward sweep: config 3's system (3 qubits, 2N = 16) at T = 1000, S in {64, 1024, 8192}.

    (g) one qc_sweep_grad_dev        J and the dense gradient (per-sample derivatives in the handle's scratch)
    (f) one qc_sweep_eval_dev        the S fidelities: the forward sweep, whose kernels this change leaves as they were

timed by device events in alternating rounds after warm-up, on one handle and one stream.  The expectation to hold the ratio against
is the kernels' own MFMA count per interval: (112 + 12 sq) for the gradient walk plus (36 + 4 sq + 4) for the forward totals it
launches first, over the forward sweep's (36 + 4 sq + 4).

    python profiles/sweep_grad_bench.py [--rounds 7] [--out profiles/sweep_grad_summary.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python profiles/sweep_grad_bench.py --trace 1024      (the kernels' own times)
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as g  # noqa: E402
from sweep_probe import PEAK_F64_MATRIX_TFLOPS, event_ms, make_problem, squarings  # noqa: E402

T = 1000


def setup(qc, S, rng):
    pb = make_problem(qc, "config3", T, S, rng)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    sw = qc.RolloutSweep(qc.QuantumSystem(pb["H0"], pb["Hd"]), [pb["P"]], T, goal=pb["goal"], fid_kind="unitary")
    assert sw.grad_supported, sw.grad_unsupported_reason
    bufs = dict(dZ=t(sw.pack(pb["controls"], pb["dts"])), dinit=t(qc.operator_to_iso_vec(np.eye(pb["N"], dtype=complex))), dth=t(pb["theta"]),
                dsc=t(pb["scale"]), dfid=torch.empty(S, dtype=torch.float64, device=dev), dJ=torch.empty(1, dtype=torch.float64, device=dev),
                dg=torch.empty(sw.Z_len, dtype=torch.float64, device=dev))
    return pb, sw, bufs


def run_size(qc, S, rounds, rng, log):
    pb, sw, b = setup(qc, S, rng)
    stream = torch.cuda.Stream(device=torch.device("cuda:0"))
    grad = lambda: sw.grad_device(b["dZ"], b["dinit"], S, b["dth"], b["dsc"], None, None, b["dJ"], b["dg"], None, stream=stream)
    fwd = lambda: sw.eval_device(b["dZ"], b["dinit"], b["dth"], b["dsc"], None, b["dfid"], stream=stream)
    with torch.cuda.stream(stream):
        for _ in range(2):
            grad()
            fwd()
        stream.synchronize()
        tg, tf = [], []
        for _ in range(rounds):
            tg.append(event_ms(grad, stream))
            tf.append(event_ms(fwd, stream))
    G0 = qc.iso_generator(pb["H0"])
    Gd = [qc.iso_generator(H) for H in pb["Hd"]]
    sqs = [squarings(np.abs(pb["dts"][k] * (G0 + sum(a * G for a, G in zip(pb["controls"][:, k], Gd)))).sum(axis=0).max()) for k in range(T - 1)]
    sq = float(np.mean(sqs))
    mf_f, mf_g = 40 + 4 * sq, 112 + 12 * sq
    flops = S * (T - 1) * (mf_f + mf_g) * 2 * 16 * 16 * 4
    ratio, expect = np.median(tg) / np.median(tf), (mf_f + mf_g) / mf_f
    log(f"== config 3's system: N = {pb['N']}, m = {pb['m']}, T = {T}, S = {S}; (mfma, chunk, n_chunks) = {sw.launch(S)}; squarings per interval: mean {sq:.2f}")
    log(f"   (g) qc_sweep_grad_dev   ms per round: {' '.join(f'{x:.3f}' for x in tg)}")
    log(f"   (f) qc_sweep_eval_dev   ms per round: {' '.join(f'{x:.3f}' for x in tf)}")
    log(f"   ratio of medians (g)/(f) = {ratio:.2f};  MFMA counts per interval: forward {mf_f:.1f}, gradient walk {mf_g:.1f}: expected ratio {expect:.2f}; "
        f"measured / expected = {ratio / expect:.2f}")
    log(f"   {flops / 1e9:.1f} GFLOP of MFMA work per gradient call: {flops / (np.median(tg) * 1e-3) / 1e12:.2f} TFLOP/s over the whole call = "
        f"{100 * flops / (np.median(tg) * 1e-3) / 1e12 / PEAK_F64_MATRIX_TFLOPS:.1f} % of {PEAK_F64_MATRIX_TFLOPS} (events; the kernels' own shares: the trace)")
    sw.close()


def trace_only(qc, S, reps=5):
    _, sw, b = setup(qc, S, np.random.default_rng(0))
    for _ in range(reps):
        sw.grad_device(b["dZ"], b["dinit"], S, b["dth"], b["dsc"], None, None, b["dJ"], b["dg"], None)
    torch.cuda.synchronize()
    sw.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", type=int, default=0, help="gradient calls alone at this S (for a kernel trace)")
    ap.add_argument("--sizes", default="64,1024,8192")
    args = ap.parse_args()
    qc = g.load_package()
    if args.trace:
        trace_only(qc, args.trace)
        return 0
    lines = []

    def log(sx):
        print(sx, flush=True)
        lines.append(sx)

    log(f"sweep gradient against the forward sweep, {torch.cuda.get_device_name(0)}, {qc._lib.lib.qc_version().decode()}; device events, "
        f"{args.rounds} alternating rounds after 2 warm-up rounds")
    rng = np.random.default_rng(0)
    for S in args.sizes.split(","):
        run_size(qc, int(S), args.rounds, rng, log)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
