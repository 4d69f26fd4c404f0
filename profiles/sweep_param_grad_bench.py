#!/usr/bin/env python3
"""Sweep parameter gradients against the control gradient and against central differences: config 3's system (3 qubits, 2N = 16, six
drives: the register-tight M = 6 instantiation), T = 1000, one detuning perturbation, S in {64, 1024, 8192}.

    (a) one qc_sweep_grad_dev, dgrad only            the control gradient (per-sample derivatives in the handle's scratch)
    (b) one qc_sweep_grad_params_dev, parameters only grad_theta and grad_scale: no per-interval store, no reduce over Z
    (c) one qc_sweep_grad_params_dev, everything      fids, J, grad, grad_samples, grad_theta, grad_scale
    (d) 2 (n_pert + m) qc_sweep_eval_dev, fids only   the central differences a user runs without (b)

timed by device events around work that ends in a synchronise, the four legs alternating in every round after warm-up, on one handle and
one stream.  The expectation to confirm or refute: (b) <= (a) -- the same MFMAs, less memory traffic.

    python profiles/sweep_param_grad_bench.py [--rounds 7] [--out FILE]
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
from sweep_grad_bench import T, setup  # noqa: E402
from sweep_probe import event_ms  # noqa: E402


def run_size(qc, S, rounds, rng, log):
    pb, sw, b = setup(qc, S, rng)
    dev = torch.device("cuda:0")
    m, p = sw.m, sw.p
    mk = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    dgs, dgth, dgsc = mk(S, T - 1, sw.n_deriv), mk(S, p), mk(S, m)
    stream = torch.cuda.Stream(device=dev)
    n_fd = 2 * (p + m)
    legs = {
        "a": lambda: sw.grad_device(b["dZ"], b["dinit"], S, b["dth"], b["dsc"], dgrad=b["dg"], stream=stream),
        "b": lambda: sw.param_grad_device(b["dZ"], b["dinit"], S, b["dth"], b["dsc"], dgrad_theta=dgth, dgrad_scale=dgsc, stream=stream),
        "c": lambda: sw.param_grad_device(b["dZ"], b["dinit"], S, b["dth"], b["dsc"], None, b["dfid"], b["dJ"], b["dg"], dgs, dgth, dgsc, stream=stream),
        "d": lambda: [sw.eval_device(b["dZ"], b["dinit"], b["dth"], b["dsc"], None, b["dfid"], stream=stream) for _ in range(n_fd)],
    }
    times = {k: [] for k in legs}
    with torch.cuda.stream(stream):
        for _ in range(2):
            for fn in legs.values():
                fn()
        stream.synchronize()
        for _ in range(rounds):
            for k, fn in legs.items():
                times[k].append(event_ms(fn, stream))
    what = {"a": "qc_sweep_grad_dev, dgrad only", "b": "params call, parameters only", "c": "params call, every output",
            "d": f"{n_fd} qc_sweep_eval_dev (central differences)"}
    log(f"== config 3's system: N = {pb['N']}, m = {m}, n_pert = {p}, T = {T}, S = {S}; (mfma, chunk, n_chunks) = {sw.launch(S)}; "
        f"per-interval buffer {S * (T - 1) * sw.n_deriv * 8 / 1e6:.1f} MB")
    for k in legs:
        log(f"   ({k}) {what[k]:42s} min {min(times[k]):9.3f}  median {np.median(times[k]):9.3f} ms   rounds: {' '.join(f'{x:.3f}' for x in times[k])}")
    med = {k: float(np.median(v)) for k, v in times.items()}
    log(f"   medians: b/a = {med['b'] / med['a']:.3f}   c/a = {med['c'] / med['a']:.3f}   d/b = {med['d'] / med['b']:.2f};   "
        f"round-to-round spread of (a): (max - min) / median = {(max(times['a']) - min(times['a'])) / med['a']:.3f}")
    sw.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="64,1024,8192")
    args = ap.parse_args()
    qc = g.load_package()
    lines = []

    def log(sx):
        print(sx, flush=True)
        lines.append(sx)

    log(f"sweep parameter gradients, {torch.cuda.get_device_name(0)}, {qc._lib.lib.qc_version().decode()}; device events, {args.rounds} rounds of the "
        f"four legs in turn after 2 warm-up rounds")
    rng = np.random.default_rng(0)
    for S in args.sizes.split(","):
        run_size(qc, int(S), args.rounds, rng, log)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
