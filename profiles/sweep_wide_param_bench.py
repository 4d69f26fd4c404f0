#!/usr/bin/env python3
"""Parameter gradients on wide handles ("mfma32-sweep", wide = QC_SWEEP_WIDE | QC_SWEEP_WIDE_PARAMS) against the control gradient of the
same handle and against the central-difference route they replace.

Systems and sizes of profiles/sweep_wide_bench.py: config 5's (N = 16, 8 drives, T = 500, one perturbation) and two coupled three-level
transmons (N = 9, 4 drives, T = 100, one perturbation), each at S in {64, 1024}:

    (a) qc_sweep_grad_dev          J and the dense gradient: the walk's flavour <false>
    (b) qc_sweep_grad_params_dev   grad_theta and grad_scale only: flavour <true>, no per-interval buffer
    (c) qc_sweep_grad_params_dev   every output: flavour <true> with the per-interval store
    (d) 2 (p + m) qc_sweep_eval_dev calls: the forward sweeps of central differences in every parameter, the only route without the bit

timed by device events around whole calls on one stream, the legs alternating over the rounds after one warm-up round, one process.
Done means every round of (c) is below every round of (d).  The flavour adds no MFMA, so (b) and (c) should sit near (a); the 16 form's
own ratios are in profiles/sweep_param_grad_summary.txt.

    python profiles/sweep_wide_param_bench.py [--rounds 5] [--out FILE]
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
from sweep_probe import event_ms  # noqa: E402
from sweep_wide_bench import make_problem  # noqa: E402


def run_size(qc, which, S, rounds, rng, log):
    pb = make_problem(qc, which, S, rng)
    T, N, m, p = pb["T"], pb["N"], pb["m"], 1
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    sw = qc.RolloutSweep(pb["system"], [pb["P"]], T, goal=pb["goal"], fid_kind="unitary", subspace=pb["subspace"], wide=True, wide_params=True)
    assert sw.kernel_name == "mfma32-sweep" and sw.grad_supported
    dZ, dinit, dth, dsc = t(sw.pack(pb["controls"], pb["dts"])), t(qc.operator_to_iso_vec(np.eye(N, dtype=complex))), t(pb["theta"]), t(pb["scale"])
    dfid, dJ, dg, dgs, dgth, dgsc = new(S), new(1), new(sw.Z_len), new(S, T - 1, sw.n_deriv), new(S, p), new(S, m)
    gth_b, gsc_b = new(S, p), new(S, m)
    stream = torch.cuda.Stream(device=dev)
    fa = lambda: sw.grad_device(dZ, dinit, S, dth, dsc, None, None, dJ, dg, None, stream=stream)
    fb = lambda: sw.param_grad_device(dZ, dinit, S, dth, dsc, dgrad_theta=gth_b, dgrad_scale=gsc_b, stream=stream)
    fc = lambda: sw.param_grad_device(dZ, dinit, S, dth, dsc, None, dfid, dJ, dg, dgs, dgth, dgsc, stream=stream)

    def fd():
        for _ in range(2 * (p + m)):
            sw.eval_device(dZ, dinit, dth, dsc, None, dfid, stream=stream)

    legs = (fa, fb, fc, fd)
    times = [[] for _ in legs]
    with torch.cuda.stream(stream):
        for f in legs:
            f()
        stream.synchronize()
        for _ in range(rounds):
            for f, ts in zip(legs, times):
                ts.append(event_ms(f, stream))
    same = bool(torch.equal(gth_b, dgth) and torch.equal(gsc_b, dgsc))
    ta, tb, tc, td = times
    fmt = lambda xs: " ".join(f"{x:.3f}" for x in xs)
    med = lambda xs: float(np.median(xs))
    log(f"== {which}: N = {N} (2N = {2 * N}), m = {m}, p = {p}, T = {T}, S = {S}; launch (mfma, chunk, n_chunks) = {sw.launch(S)}")
    log(f"   (a) grad                                ms per round: {fmt(ta)}   min {min(ta):.3f}  median {med(ta):.3f}")
    log(f"   (b) param_grad, theta and scale only    ms per round: {fmt(tb)}   min {min(tb):.3f}  median {med(tb):.3f}")
    log(f"   (c) param_grad, every output            ms per round: {fmt(tc)}   min {min(tc):.3f}  median {med(tc):.3f}")
    log(f"   (d) {2 * (p + m):2d} wide forward sweeps              ms per round: {fmt(td)}   min {min(td):.3f}  median {med(td):.3f}")
    log(f"   median (b) / (a) = {med(tb) / med(ta):.3f}; median (c) / (a) = {med(tc) / med(ta):.3f}; median (d) / (c) = {med(td) / med(tc):.2f}; "
        f"(c) in forward sweeps = {med(tc) / (med(td) / (2 * (p + m))):.2f}")
    log(f"   every round of (c) below every round of (d): {max(tc) < min(td)}; grad_theta / grad_scale of (b) and (c) bit-equal: {same}")
    sw.close()
    return max(tc) < min(td)


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

    log(f"wide parameter gradients, {torch.cuda.get_device_name(0)}, {qc._lib.lib.qc_version().decode()}; device events around whole calls, "
        f"{args.rounds} alternating rounds (a), (b), (c), (d) after one warm-up round, one process")
    rng = np.random.default_rng(0)
    ok = True
    for which in args.systems.split(","):
        for S in args.sizes.split(","):
            ok = run_size(qc, which, int(S), args.rounds, rng, log) and ok
    log(f"every round of (c) below every round of (d), at every size: {ok}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
