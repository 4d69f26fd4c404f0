#!/usr/bin/env python3
"""The backward walk of the "mfma64-sweep" form (csrc/qc_sweep64_grad.hip) against the forward sweep of the same handle.

Systems: those of profiles/sweep_wide64_bench.py, T = 100, each at S in {64, 1024}, on handles made with
wide = QC_SWEEP_WIDE | QC_SWEEP_WIDE_64 | QC_SWEEP_WIDE_64_GRAD:

    5 qubits (N = 32, 10 drives), the full unitary (32 state columns, two column tiles):   (g) qc_sweep_grad_dev (fids, grad)
                                                                                          (e) qc_sweep_eval_dev (fids)
    three transmons (N = 27, 6 drives), the eight computational columns (one column tile; no fidelity is defined on 8 of 27 columns, so
    the derivative call is the pullback, which runs the same seed chains and the same walk): (g) qc_sweep_vjp_dev (grad)
                                                                                          (e) qc_sweep_eval_dev (finals)

timed by device events on one stream, (g) and (e) alternating over the rounds after one warm-up round, one process.  The forward kernel is
not touched by the walk (its instructions are those it had before the walk existed), so (e) is a yardstick that predates it.  The model is the MFMA count of the kernels as built, per interval
and workgroup, nct = ceil(columns / 16):

    forward   (9 + sq) x 256                         = 2304 + 256 sq
    walk      8 x (16 x (32 + 4 nct) + 4 nct x 16) + sq x 16 x 48 + 16 x 16 + 8 nct x 16   = (4352 + 1152 nct) + 768 sq
    (g) / (e) by the model: (forward + walk) / forward

with the sq every sample takes in every interval (recomputed on the host).  The share of the f64 matrix peak is that MFMA work over the
call's time: an end-to-end figure (totals, seed, walk and reduction launches), not a kernel's.

    python profiles/sweep_wide64_grad_bench.py [--rounds 5] [--out FILE]          (section 2 of profiles/sweep_wide64_grad_summary.txt)
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


def run_size(qc, which, S, T, rounds, rng, log):
    pb = make_problem(qc, which, S, T, rng)
    N, m = pb["N"], pb["m"]
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    flags = dict(wide=True, wide64=True, wide64_grad=True)
    if which == "qubits5":
        cols = N
        sw = qc.RolloutSweep(pb["system"], [pb["P"]], T, goal=pb["goal"], fid_kind="unitary", **flags)
        init = qc.operator_to_iso_vec(np.eye(N, dtype=complex))
    else:
        import three_transmon_robustness as tr
        cols = len(tr.SUBSPACE)
        sw = qc.RolloutSweep(pb["system"], [pb["P"]], T, cols=cols, **flags)
        E = np.zeros((2 * N, cols))
        E[tr.SUBSPACE, np.arange(cols)] = 1.0
        init = E.reshape(-1, order="F")
    assert sw.kernel_name == "mfma64-sweep" and sw.vjp_supported
    nct = -(-cols // 16)
    dZ, dinit, dth, dsc = t(sw.pack(pb["controls"], pb["dts"])), t(init), t(pb["theta"]), t(pb["scale"])
    dgrad = torch.empty(sw.Z_len, dtype=torch.float64, device=dev)
    stream = torch.cuda.Stream(device=dev)
    if which == "qubits5":
        dfid, dfid2 = (torch.empty(S, dtype=torch.float64, device=dev) for _ in range(2))
        fg = lambda: sw.grad_device(dZ, dinit, S, dth, dsc, None, dfid, None, dgrad, None, stream=stream)
        fe = lambda: sw.eval_device(dZ, dinit, dth, dsc, None, dfid2, stream=stream)
        what = "qc_sweep_grad_dev (fids, grad) against qc_sweep_eval_dev (fids)"
    else:
        dcot = t(np.random.default_rng(1).standard_normal((S, sw.ns)))
        dfin = torch.empty((S, sw.ns), dtype=torch.float64, device=dev)
        fg = lambda: sw.vjp_device(dZ, dinit, S, dcot, dth, dsc, dgrad=dgrad, stream=stream)
        fe = lambda: sw.eval_device(dZ, dinit, dth, dsc, dfin, None, stream=stream)
        what = "qc_sweep_vjp_dev (grad) against qc_sweep_eval_dev (finals)"
    with torch.cuda.stream(stream):
        fg(); fe()
        stream.synchronize()
        tg, te = [], []
        for _ in range(rounds):
            tg.append(event_ms(fg, stream))
            te.append(event_ms(fe, stream))
    if which == "qubits5":
        assert torch.equal(dfid, dfid2)          # the fidelities of the gradient call carry the bits of the forward sweep
    sq = mean_squarings(qc, pb)
    fwd = 2304 + 256 * sq
    walk = 4352 + 1152 * nct + 768 * sq
    model = (fwd + walk) / fwd
    ratio = np.median(tg) / np.median(te)
    flops = S * (T - 1) * (fwd + walk) * 2 * 16 * 16 * 4
    rate = flops / (np.median(tg) * 1e-3) / 1e12
    fmt = lambda xs: " ".join(f"{x:.3f}" for x in xs)
    log(f"== {which}: N = {N} (2N = {2 * N}), m = {m}, {cols} state columns (nct = {nct}), T = {T}, S = {S}; launch (mfma, chunk, n_chunks) = {sw.launch(S)}; "
        f"squarings per interval, mean: {sq:.3f}; {what}")
    log(f"   (g) derivative call  ms per round: {fmt(tg)}   min {min(tg):.3f}  median {np.median(tg):.3f}")
    log(f"   (e) forward sweep    ms per round: {fmt(te)}   min {min(te):.3f}  median {np.median(te):.3f}")
    log(f"   median (g) / median (e) = {ratio:.2f}; model ({fwd:.0f} + {walk:.0f}) / {fwd:.0f} = {model:.2f}; measured / model = {ratio / model:.2f} "
        f"(the wide gradient's figure: 4.4 / 3.96 = 1.11)")
    log(f"   MFMA work {fwd + walk:.0f} instructions per interval, {flops / 1e9:.1f} GFLOP per call, over the call's time: {rate:.2f} TFLOP/s = "
        f"{100 * rate / PEAK_F64_MATRIX_TFLOPS:.1f} % of {PEAK_F64_MATRIX_TFLOPS} TFLOP/s (f64 matrix, vendor figure; whole call by device events)")
    sw.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--sizes", default="64,1024")
    ap.add_argument("--systems", default="qubits5,transmons3")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sweep_wide64_grad_bench.py measures on a GPU; none is visible")
    qc = g.load_package()
    lines = []

    def log(sx):
        print(sx, flush=True)
        lines.append(sx)

    log(f"mfma64-sweep derivative calls against the forward sweep of the same handle, {torch.cuda.get_device_name(0)}, {qc._lib.lib.qc_version().decode()}; "
        f"device events, {args.rounds} alternating rounds (g), (e) after one warm-up round, one process")
    rng = np.random.default_rng(0)
    for which in args.systems.split(","):
        for S in args.sizes.split(","):
            run_size(qc, which, int(S), args.T, args.rounds, rng, log)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
