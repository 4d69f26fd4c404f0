#!/usr/bin/env python3
"""Sweep pushforwards against the forward sweep and the sweep gradient, on one handle and the same inputs: config 3's system
(2N = 16, "mfma16-sweep") at T = 1000, S in {64, 1024}.

    (a) qc_sweep_eval_dev, fids              the forward kernel, 36 + 4 sq MFMAs per interval, and the final-state launch
    (b) qc_sweep_jvp_dev, all four outputs   the differentiated forward kernel, 108 + 12 sq, and its final-state launch
    (c) qc_sweep_grad_dev, grad              the forward kernel, the seed, the backward walk (112 + 12 sq) and the reduction

timed by device events around whole calls, alternating, five rounds after two warm-up rounds, on one stream.  Reported: medians and
ranges, (b) / (a) against the MFMA model (108 + 12 sq) / (36 + 4 sq), the MFMA work of (b) over its call time as a fraction of the f64
matrix peak, and whether every round of (b) is below every round of (c) (the model: 0.7 of a gradient call).  Reported, not gated.
With --worst LOG the lines "SWEEP-JVP ..." of a run of the GPU tests (pytest -s) are appended.

    python profiles/sweep_jvp_bench.py [--rounds 5] [--worst LOG] [--out profiles/sweep_jvp_summary.txt]
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


def run_size(qc, S, rounds, rng, log):
    pb = make_problem(qc, "config3", T, S, rng)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    mk = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    sw = qc.RolloutSweep(qc.QuantumSystem(pb["H0"], pb["Hd"]), [pb["P"]], T, goal=pb["goal"], fid_kind="unitary")
    assert sw.jvp_supported and sw.grad_supported
    dZ, dinit, dth, dsc = t(sw.pack(pb["controls"], pb["dts"])), t(qc.operator_to_iso_vec(np.eye(pb["N"], dtype=complex))), t(pb["theta"]), t(pb["scale"])
    dvZ, dvinit = t(rng.standard_normal(sw.Z_len)), t(rng.standard_normal(sw.ns))
    dvth, dvsc = t(rng.standard_normal((S, sw.p))), t(rng.standard_normal((S, sw.m)))
    dfid, dfin, dtfin, dtfid, dJ, dg = mk(S), mk(S, sw.ns), mk(S, sw.ns), mk(S), mk(1), mk(sw.Z_len)
    stream = torch.cuda.Stream(device=dev)
    calls = {
        "(a) qc_sweep_eval_dev, fids  ": lambda: sw.eval_device(dZ, dinit, dth, dsc, None, dfid, stream=stream),
        "(b) qc_sweep_jvp_dev, all out": lambda: sw.jvp_device(dZ, dinit, S, dth, dsc, dvZ=dvZ, dvinit=dvinit, dvtheta=dvth, dvscale=dvsc, dfinals=dfin,
                                                               dfids=dfid, dtfinals=dtfin, dtfids=dtfid, stream=stream),
        "(c) qc_sweep_grad_dev, grad  ": lambda: sw.grad_device(dZ, dinit, S, dth, dsc, None, None, dJ, dg, None, stream=stream),
    }
    times = {k: [] for k in calls}
    with torch.cuda.stream(stream):
        for _ in range(2):
            for fn in calls.values():
                fn()
        stream.synchronize()
        for _ in range(rounds):
            for k, fn in calls.items():
                times[k].append(event_ms(fn, stream))
    G0 = qc.iso_generator(pb["H0"])
    Gd = [qc.iso_generator(H) for H in pb["Hd"]]
    # squarings of every (sample, interval) the call launches: G_s(a_t) with the sample's own theta and scale, the kernels' rule
    Gp = qc.iso_generator(np.asarray(pb["P"], dtype=complex))
    Gd3, h, a = np.stack(Gd), np.asarray(pb["dts"], dtype=np.float64)[:T - 1], pb["controls"][:, :T - 1]
    sq_sum = 0
    for s in range(S):
        Gs = G0 + pb["theta"][s, 0] * Gp + np.einsum("kt,kij->tij", pb["scale"][s][:, None] * a, Gd3)
        norms = np.abs(h[:, None, None] * Gs).sum(axis=1).max(axis=1)
        sq_sum += sum(squarings(x) for x in norms)
    sq = sq_sum / (S * (T - 1))
    mf_a, mf_b, mf_c = 36 + 4 * sq, 108 + 12 * sq, (36 + 4 * sq) + (4 + 112 + 12 * sq)
    log(f"== config 3's system: N = {pb['N']}, m = {pb['m']}, T = {T}, S = {S}; {sw.kernel_name}, (mfma, chunk, n_chunks) = {sw.launch(S)}; "
        f"squarings per (sample, interval), from every sample's own theta and scale: mean {sq:.3f}")
    for k, xs in times.items():
        log(f"   {k}  ms per round: {' '.join(f'{x:.3f}' for x in xs)}   median {np.median(xs):.3f}  range {min(xs):.3f} .. {max(xs):.3f}")
    med = {k[:3]: float(np.median(xs)) for k, xs in times.items()}
    tb, tc = times["(b) qc_sweep_jvp_dev, all out"], times["(c) qc_sweep_grad_dev, grad  "]
    flops = S * (T - 1) * mf_b * 2 * 16 * 16 * 4
    log(f"   median (b) / median (a) = {med['(b)'] / med['(a)']:.2f}; MFMA model (108 + 12 sq) / (36 + 4 sq) = {mf_b / mf_a:.2f}; "
        f"measured / model = {med['(b)'] / med['(a)'] / (mf_b / mf_a):.2f}")
    log(f"   {flops / 1e9:.1f} GFLOP of MFMA work per pushforward call: {flops / (med['(b)'] * 1e-3) / 1e12:.2f} TFLOP/s over the whole call = "
        f"{100 * flops / (med['(b)'] * 1e-3) / 1e12 / PEAK_F64_MATRIX_TFLOPS:.1f} % of {PEAK_F64_MATRIX_TFLOPS} (events around the call)")
    log(f"   median (b) / median (c) = {med['(b)'] / med['(c)']:.2f} (MFMA model {mf_b / mf_c:.2f}); every round of (b) below every round of (c): "
        f"{'yes' if max(tb) < min(tc) else 'no'} (max (b) {max(tb):.3f}, min (c) {min(tc):.3f})")
    sw.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="64,1024")
    ap.add_argument("--worst", default=None, help="output of `pytest -m gpu -s tests/test_sweep_jvp.py`")
    args = ap.parse_args()
    qc = g.load_package()
    lines = []

    def log(sx):
        print(sx, flush=True)
        lines.append(sx)

    log(f"sweep pushforward against the forward sweep and the sweep gradient, {torch.cuda.get_device_name(0)}, {qc._lib.lib.qc_version().decode()}; "
        f"device events, {args.rounds} alternating rounds after 2 warm-up rounds")
    rng = np.random.default_rng(0)
    for S in args.sizes.split(","):
        run_size(qc, int(S), args.rounds, rng, log)
    if args.worst:
        log("== the GPU tests' worst errors over their bounds (tests/test_sweep_jvp.py)")
        for line in open(args.worst):
            k = line.find("SWEEP-JVP ")
            if k >= 0 and " reference " not in line:
                log("   " + line[k + len("SWEEP-JVP "):].rstrip())
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
