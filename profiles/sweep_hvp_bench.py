#!/usr/bin/env python3
"""Sweep Hessian products against the pullback and the pushforward, on one handle and the same inputs: config 3's system
(2N = 16, "mfma16-sweep") at T = 1000, S in {64, 1024}.

    (a) qc_sweep_vjp_dev, grad               the forward kernel (36 + 4 sq MFMAs per interval), the seed, the backward walk (112 + 12 sq + 4)
    (b) qc_sweep_jvp_dev, finals + tfinals   the differentiated forward kernel, 108 + 12 sq, and its final-state launch
    (c) qc_sweep_hvp_dev, tgrad              the differentiated forward kernel (108 + 12 sq), the seed, the twice-differentiated backward
                                             walk (408 + 36 sq) and the reduction

timed by device events around whole calls, alternating, five rounds after two warm-up rounds, on one stream.  Reported: medians and
ranges, (c) / (a) and (c) / (b) against the MFMA model, and the MFMA work of (c) over its call time as a fraction of the f64 matrix
peak.  Reported, not gated.  With --worst LOG the lines "SWEEP-HVP ..." of a run of the GPU tests (pytest -s) are appended.

    python profiles/sweep_hvp_bench.py [--rounds 5] [--worst LOG] [--out profiles/sweep_hvp_summary.txt]
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
    assert sw.hvp_supported and sw.jvp_supported and sw.vjp_supported
    dZ, dinit, dth, dsc = t(sw.pack(pb["controls"], pb["dts"])), t(qc.operator_to_iso_vec(np.eye(pb["N"], dtype=complex))), t(pb["theta"]), t(pb["scale"])
    dvZ = t(rng.standard_normal(sw.Z_len))
    dcot, dvcot = t(rng.standard_normal((S, sw.ns))), t(rng.standard_normal((S, sw.ns)))
    dfin, dtfin, dg, dtg = mk(S, sw.ns), mk(S, sw.ns), mk(sw.Z_len), mk(sw.Z_len)
    stream = torch.cuda.Stream(device=dev)
    calls = {
        "(a) qc_sweep_vjp_dev, grad     ": lambda: sw.vjp_device(dZ, dinit, S, dcot, dth, dsc, dgrad=dg, stream=stream),
        "(b) qc_sweep_jvp_dev, tfinals  ": lambda: sw.jvp_device(dZ, dinit, S, dth, dsc, dvZ=dvZ, dfinals=dfin, dtfinals=dtfin, stream=stream),
        "(c) qc_sweep_hvp_dev, tgrad    ": lambda: sw.hvp_device(dZ, dinit, S, dcot, dth, dsc, dvZ=dvZ, dvcot=dvcot, dtgrad=dtg, stream=stream),
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
    mf_a, mf_b, mf_c = (36 + 4 * sq) + (4 + 112 + 12 * sq), 108 + 12 * sq, (108 + 12 * sq) + (408 + 36 * sq)
    log(f"== config 3's system: N = {pb['N']}, m = {pb['m']}, T = {T}, S = {S}; {sw.kernel_name}, (mfma, chunk, n_chunks) = {sw.launch(S)}; "
        f"squarings per (sample, interval), from every sample's own theta and scale: mean {sq:.3f}")
    for k, xs in times.items():
        log(f"   {k}  ms per round: {' '.join(f'{x:.3f}' for x in xs)}   median {np.median(xs):.3f}  range {min(xs):.3f} .. {max(xs):.3f}")
    med = {k[:3]: float(np.median(xs)) for k, xs in times.items()}
    flops = S * (T - 1) * mf_c * 2 * 16 * 16 * 4
    log(f"   median (c) / median (a) = {med['(c)'] / med['(a)']:.2f}; MFMA model (516 + 48 sq) / (152 + 16 sq) = {mf_c / mf_a:.2f}; "
        f"measured / model = {med['(c)'] / med['(a)'] / (mf_c / mf_a):.2f}")
    log(f"   median (c) / median (b) = {med['(c)'] / med['(b)']:.2f}; MFMA model (516 + 48 sq) / (108 + 12 sq) = {mf_c / mf_b:.2f}; "
        f"measured / model = {med['(c)'] / med['(b)'] / (mf_c / mf_b):.2f}")
    log(f"   {flops / 1e9:.1f} GFLOP of MFMA work per Hessian product: {flops / (med['(c)'] * 1e-3) / 1e12:.2f} TFLOP/s over the whole call = "
        f"{100 * flops / (med['(c)'] * 1e-3) / 1e12 / PEAK_F64_MATRIX_TFLOPS:.1f} % of {PEAK_F64_MATRIX_TFLOPS} (events around the call)")
    log(f"   an exact product (one (b) + one (c)): {med['(b)'] + med['(c)']:.3f} ms; a Gauss-Newton product (one (b) + one (a)): {med['(b)'] + med['(a)']:.3f} ms; "
        f"three pullback calls: {3 * med['(a)']:.3f} ms")
    sw.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="64,1024")
    ap.add_argument("--worst", default=None, help="output of `pytest -m gpu -s tests/test_sweep_hvp.py`")
    args = ap.parse_args()
    qc = g.load_package()
    lines = []

    def log(sx):
        print(sx, flush=True)
        lines.append(sx)

    log(f"sweep Hessian product against the pullback and the pushforward, {torch.cuda.get_device_name(0)}, {qc._lib.lib.qc_version().decode()}; "
        f"device events, {args.rounds} alternating rounds after 2 warm-up rounds")
    rng = np.random.default_rng(0)
    for S in args.sizes.split(","):
        run_size(qc, int(S), args.rounds, rng, log)
    if args.worst:
        log("== the GPU tests' worst errors over their bounds (tests/test_sweep_hvp.py)")
        for line in open(args.worst):
            k = line.find("SWEEP-HVP ")
            if k >= 0 and " reference " not in line:
                log("   " + line[k + len("SWEEP-HVP "):].rstrip())
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
