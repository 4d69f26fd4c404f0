#!/usr/bin/env python3
"""The wide sweep pushforward ("mfma32-sweep" handles made with QC_SWEEP_WIDE_TANGENT) against the forward sweep on the same handle.

Systems: those of profiles/sweep_wide_bench.py -- config 5's (4 qubits, N = 16, 8 drives, its own T = 500) and two coupled three-level
transmons (N = 9, 4 drives, T = 100) -- each at S in {64, 1024}:

    (a) qc_sweep_eval_dev      the S final states, qc_sweep_mfma32_kernel + qc_sweep_finish_kernel
    (b) qc_sweep_jvp_dev       the S final states and their tangents along one direction of the controls and timesteps,
                               qc_sweep32_jvp_kernel + qc_sweep32_jvp_finish_kernel

timed by device events on one stream, (a) and (b) alternating over the rounds after one warm-up round.  (b) / (a) is held against
the kernels' MFMA counts per interval: forward 288 + 32 sq, pushforward 864 + 96 sq, so 3.0 by the count; the forward kernel runs two
waves per SIMD and the pushforward kernel one, so the measured ratio need not be the count's.  The share of the f64 matrix peak is the
MFMA work of the call over the call's time: an end-to-end figure, not a kernel's.  What a user without the pushforward would do
instead -- a central difference of two forward sweeps, 2.0 (a) -- is run once and its distance to the tangent recorded.

    python profiles/sweep_wide_jvp_bench.py [--rounds 5] [--out profiles/sweep_wide_jvp_summary.txt]
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
from sweep_wide_bench import make_problem  # noqa: E402


def run_size(qc, which, S, rounds, rng, log):
    pb = make_problem(qc, which, S, rng)
    T, N, m = pb["T"], pb["N"], pb["m"]
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    sw = qc.RolloutSweep(pb["system"], [pb["P"]], T, goal=pb["goal"], fid_kind="unitary", subspace=pb["subspace"], wide=True, wide_tangent=True)
    assert sw.kernel_name == "mfma32-sweep" and sw.jvp_supported
    vrng = np.random.default_rng(1)
    vZ = sw.pack(vrng.standard_normal((m, T)) * np.abs(pb["controls"]).max(), 0.01 * pb["dts"] * vrng.standard_normal(T))
    Z = sw.pack(pb["controls"], pb["dts"])
    new = lambda: torch.empty((S, sw.ns), dtype=torch.float64, device=dev)
    b = dict(dZ=t(Z), dvZ=t(vZ), dinit=t(qc.operator_to_iso_vec(np.eye(N, dtype=complex))), dth=t(pb["theta"]), dsc=t(pb["scale"]), xa=new(), xb=new(), tb=new())
    stream = torch.cuda.Stream(device=dev)
    fa = lambda: sw.eval_device(b["dZ"], b["dinit"], b["dth"], b["dsc"], b["xa"], None, stream=stream)
    fb = lambda: sw.jvp_device(b["dZ"], b["dinit"], S, b["dth"], b["dsc"], dvZ=b["dvZ"], dfinals=b["xb"], dtfinals=b["tb"], stream=stream)
    with torch.cuda.stream(stream):
        fa(); fb()
        stream.synchronize()
        ta, tb = [], []
        for _ in range(rounds):
            ta.append(event_ms(fa, stream))
            tb.append(event_ms(fb, stream))
        same = bool(torch.equal(b["xa"], b["xb"]))
        # the central difference of two forward sweeps a user would otherwise take: step 1e-6 along vZ
        eps = 1e-6
        xp, xm = new(), new()
        sw.eval_device(b["dZ"] + eps * b["dvZ"], b["dinit"], b["dth"], b["dsc"], xp, None, stream=stream)
        sw.eval_device(b["dZ"] - eps * b["dvZ"], b["dinit"], b["dth"], b["dsc"], xm, None, stream=stream)
        stream.synchronize()
        fd = (xp - xm) / (2 * eps)
        fd_err = float((fd - b["tb"]).abs().max() / b["tb"].abs().max())
    G0 = qc.iso_generator(np.asarray(pb["system"].H_drift))
    Gd = [qc.iso_generator(np.asarray(H)) for H in pb["system"].H_drives]
    sq = float(np.mean([squarings(np.abs(pb["dts"][k] * (G0 + sum(a * G for a, G in zip(pb["controls"][:, k], Gd)))).sum(axis=0).max()) for k in range(T - 1)]))
    mf_f, mf_j = 288 + 32 * sq, 864 + 96 * sq
    per_mfma = 2 * 16 * 16 * 4
    fl_a, fl_b = S * (T - 1) * mf_f * per_mfma, S * (T - 1) * mf_j * per_mfma
    share = lambda fl, ms: 100 * fl / (ms * 1e-3) / 1e12 / PEAK_F64_MATRIX_TFLOPS
    fmt = lambda xs: " ".join(f"{x:.3f}" for x in xs)
    log(f"== {which}: N = {N} (2N = {2 * N}), m = {m}, T = {T}, S = {S}; launch (mfma, chunk, n_chunks) = {sw.launch(S)}; "
        f"squarings per interval (unperturbed): mean {sq:.2f}")
    log(f"   (a) wide forward sweep   ms per round: {fmt(ta)}   min {min(ta):.3f}  median {np.median(ta):.3f}")
    log(f"   (b) wide pushforward     ms per round: {fmt(tb)}   min {min(tb):.3f}  median {np.median(tb):.3f}")
    log(f"   median (b) / median (a) = {np.median(tb) / np.median(ta):.2f}; MFMA counts per interval: forward {mf_f:.0f}, pushforward {mf_j:.0f}: "
        f"by the count {mf_j / mf_f:.2f}; finals of (b) are the bits of (a): {same}")
    log(f"   MFMA work over the call's time, of {PEAK_F64_MATRIX_TFLOPS} TFLOP/s (f64 matrix, vendor figure): (a) {share(fl_a, np.median(ta)):.1f} %, "
        f"(b) {share(fl_b, np.median(tb)):.1f} %  (whole calls by device events, not kernel times)")
    log(f"   central difference of two forward sweeps (2.0 (a), step 1e-6): max |difference to tfinals| / max |tfinals| = {fd_err:.1e}")
    sw.close()


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

    log(f"wide sweep pushforward against the forward sweep on the same handle, {torch.cuda.get_device_name(0)}, {qc._lib.lib.qc_version().decode()}; "
        f"device events, {args.rounds} alternating rounds (a), (b) after one warm-up round, one process")
    rng = np.random.default_rng(0)
    for which in args.systems.split(","):
        for S in args.sizes.split(","):
            run_size(qc, which, int(S), args.rounds, rng, log)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
