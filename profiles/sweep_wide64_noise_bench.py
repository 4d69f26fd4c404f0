#!/usr/bin/env python3
"""Noise-trajectory sweeps in the "mfma64-sweep" form (csrc/qc_sweep64_noise.hip) against the plain sweep and gradient of the same handle.

Systems: those of profiles/sweep_wide64_bench.py, T = 100, each at S in {64, 1024}, one perturbation (the detuning of that file) whose
amplitude is a noise trajectory of the width of theta (the squarings stay those of the plain sweep), the full unitary with its fidelity
(three transmons: on the 8 computational levels), on handles made with wide = QC_SWEEP_WIDE | QC_SWEEP_WIDE_64 | QC_SWEEP_WIDE_64_GRAD |
QC_SWEEP_WIDE_64_NOISE.  Timed by device events on one stream, alternating over the rounds after one warm-up round, one process:

    (ne) qc_sweep_noise_eval_dev (fids)                       (e) qc_sweep_eval_dev (fids)
    (ng) qc_sweep_noise_grad_dev (fids, grad, grad_noise)     (g) qc_sweep_grad_dev (fids, grad)
    (n1) S calls of qc_sweep_noise_eval_dev with one sample each, at S = 64: the only loop a user could write at this size

By the instruction count (ne) / (e) = (ng) / (g) = 1: the MFMAs are the same, (9 + sq) x 256 forward and (4352 + 1152 nct) + 768 sq in the
walk per interval and workgroup.  The extra work is p more 32 KiB image reads and 4 p fmas per thread and interval forward, p more
contractions (4 loads, 4 fmas, one wave sum) in the walk.  The share of the f64 matrix peak is the MFMA work over the call's time: an
end-to-end figure (totals, seed, walk and reduction launches), not a kernel's.

--plain times (e) and (g) alone on a handle WITHOUT the noise bit: run once per build (the library of the parent commit and this one,
alternating processes on one box), the kernels behind them are meant to be identical, so every round of one must lie inside the spread of
the other.

    python profiles/sweep_wide64_noise_bench.py [--rounds 5] [--plain] [--out FILE]          (profiles/sweep_wide64_noise_summary.txt)
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
from sweep_probe import PEAK_F64_MATRIX_TFLOPS, event_ms  # noqa: E402
from sweep_wide64_bench import make_problem, mean_squarings  # noqa: E402


def run_size(qc, which, S, T, rounds, rng, log, plain):
    pb = make_problem(qc, which, S, T, rng)
    N, m = pb["N"], pb["m"]
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    flags = dict(wide=True, wide64=True, wide64_grad=True)
    if not plain:
        flags["wide64_noise"] = True
    sw = qc.RolloutSweep(pb["system"], [pb["P"]], T, goal=pb["goal"], fid_kind="unitary", subspace=pb["subspace"], **flags)
    assert sw.kernel_name == "mfma64-sweep" and sw.grad_supported and sw.noise_supported == (not plain)
    nct = -(-N // 16)
    width = float(np.abs(pb["theta"]).max())
    noise = rng.uniform(-width, width, (S, T - 1, 1))
    dZ, dinit, dth, dsc, dn = t(sw.pack(pb["controls"], pb["dts"])), t(qc.operator_to_iso_vec(np.eye(N, dtype=complex))), t(pb["theta"]), t(pb["scale"]), t(noise)
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    fe_, fne_, fg_, fng_, gg, gng, gn = new(S), new(S), new(S), new(S), new(sw.Z_len), new(sw.Z_len), new(S, T - 1, 1)
    stream = torch.cuda.Stream(device=dev)
    calls = {"e": lambda: sw.eval_device(dZ, dinit, dth, dsc, None, fe_, stream=stream),
             "g": lambda: sw.grad_device(dZ, dinit, S, dth, dsc, None, fg_, None, gg, None, stream=stream)}
    if not plain:
        calls["ne"] = lambda: sw.noise_eval_device(dZ, dinit, dn, dth, dsc, None, fne_, stream=stream)
        calls["ng"] = lambda: sw.noise_grad_device(dZ, dinit, dn, dth, dsc, None, fng_, None, gng, None, gn, stream=stream)
        if S <= 64:
            one = [(dn[s:s + 1], dth[s:s + 1], dsc[s:s + 1], fne_[s:s + 1]) for s in range(S)]

            def loop():
                for xn, xt, xs, xf in one:
                    sw.noise_eval_device(dZ, dinit, xn, xt, xs, None, xf, stream=stream)
            calls["n1"] = loop
    times = {k: [] for k in calls}
    with torch.cuda.stream(stream):
        for f in calls.values():
            f()
        stream.synchronize()
        for _ in range(rounds):
            for k, f in calls.items():
                times[k].append(event_ms(f, stream))
    sq = mean_squarings(qc, pb)      # without the noise; its width is theta's, the counts move by a few per mille at most
    fwd = 2304 + 256 * sq
    walk = 4352 + 1152 * nct + 768 * sq
    fmt = lambda xs: " ".join(f"{x:.3f}" for x in xs)
    med = {k: float(np.median(v)) for k, v in times.items()}
    log(f"== {which}: N = {N} (2N = {2 * N}), m = {m}, p = 1, {N} state columns (nct = {nct}), T = {T}, S = {S}; launch (mfma, chunk, n_chunks) = {sw.launch(S)}; "
        f"squarings per interval, mean: {sq:.3f}; handle wide = {sw._desc.wide}")
    names = {"e": "(e)  eval (fids)             ", "ne": "(ne) noise_eval (fids)       ", "g": "(g)  grad (fids, grad)       ",
             "ng": "(ng) noise_grad (+grad_noise)", "n1": "(n1) S noise_eval calls, S=1 "}
    for k in ("e", "ne", "g", "ng", "n1"):
        if k in times:
            log(f"   {names[k]} ms per round: {fmt(times[k])}   min {min(times[k]):.3f}  median {med[k]:.3f}")
    if not plain:
        spread = lambda k: (max(times[k]) - min(times[k])) / med[k]
        log(f"   median (ne) / median (e) = {med['ne'] / med['e']:.3f} (instruction count: 1; round-to-round spread of (e): {100 * spread('e'):.1f} %)   "
            f"median (ng) / median (g) = {med['ng'] / med['g']:.3f} (instruction count: 1; spread of (g): {100 * spread('g'):.1f} %)")
        for k, work in (("ne", fwd), ("ng", fwd + walk)):
            flops = S * (T - 1) * work * 2 * 16 * 16 * 4
            rate = flops / (med[k] * 1e-3) / 1e12
            log(f"   ({k}) MFMA work {work:.0f} instructions per interval, {flops / 1e9:.1f} GFLOP per call: {rate:.2f} TFLOP/s = "
                f"{100 * rate / PEAK_F64_MATRIX_TFLOPS:.1f} % of {PEAK_F64_MATRIX_TFLOPS} TFLOP/s (f64 matrix, vendor figure; whole call by device events)")
        if "n1" in med:
            log(f"   one noise_eval call of S = {S} against S calls of one sample: {med['n1'] / med['ne']:.1f} x faster")
    sw.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--sizes", default="64,1024")
    ap.add_argument("--systems", default="qubits5,transmons3")
    ap.add_argument("--plain", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sweep_wide64_noise_bench.py measures on a GPU; none is visible")
    qc = g.load_package()
    lines = []

    def log(sx):
        print(sx, flush=True)
        lines.append(sx)

    log(f"mfma64-sweep {'plain sweep and gradient on a handle without the noise bit' if args.plain else 'noise sweeps against the plain sweep and gradient of the same handle'}, "
        f"{torch.cuda.get_device_name(0)}, {qc._lib.lib.qc_version().decode()}, library {os.path.basename(qc._lib.LIB_PATH)}; device events, {args.rounds} alternating rounds "
        f"after one warm-up round, one process")
    rng = np.random.default_rng(0)
    for which in args.systems.split(","):
        for S in args.sizes.split(","):
            run_size(qc, which, int(S), args.T, args.rounds, rng, log, args.plain)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
