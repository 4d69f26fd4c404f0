#!/usr/bin/env python3
"""Noise-trajectory sweeps against the plain sweep and against the loop they replace: config 3's system (3 qubits, 2N = 16, six drives)
with one detuning perturbation -- seven tiles, so the noise kernels run their M = 8 instantiation against the sweep's M = 6 --
T = 1000, S in {64, 1024}.

    (a) one qc_sweep_eval_dev, fids only                      the sweep at constant theta
    (b) one qc_sweep_noise_eval_dev, fids only                the same with a noise trajectory per sample
    (c) one qc_sweep_grad_dev, every output
    (d) one qc_sweep_noise_grad_dev, every output             (c) plus grad_noise
    (e) S calls of qc_sweep_eval_dev with S = 1               the loop (b) replaces: a handle that carries P_0 as a seventh drive, every
                                                              call with a trajectory vector of its own that holds theta[s] + noise[s, t]

timed by device events around whole calls that end in a synchronise, the five legs alternating in every round after warm-up, one stream.
(b)/(a), (d)/(c) and (e)/(b) are reported; the fidelities of (e) are compared with those of (b).

    python profiles/sweep_noise_bench.py [--rounds 5] [--out FILE]
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
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    m, p = sw.m, sw.p
    assert p == 1 and sw.noise_supported, sw.noise_unsupported_reason
    mk = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    noise = 0.05 * rng.standard_normal((S, T - 1, p))
    dn, dgs, dgn, dfid_n = t(noise), mk(S, T - 1, sw.n_deriv), mk(S, T - 1, p), mk(S)
    # (e): P_0 as a seventh drive, one trajectory vector per sample
    sw7 = qc.RolloutSweep(qc.QuantumSystem(pb["H0"], list(pb["Hd"]) + [pb["P"]]), [], T, goal=pb["goal"], fid_kind="unitary")
    Z7 = np.empty((S, sw7.Z_len))
    for s in range(S):
        a7 = np.vstack([pb["controls"], np.concatenate([pb["theta"][s, 0] + noise[s, :, 0], [0.0]])[None, :]])
        Z7[s] = sw7.pack(a7, pb["dts"])
    dZ7, dsc7, dfid_e = t(Z7), t(np.hstack([pb["scale"], np.ones((S, 1))])), mk(S)
    stream = torch.cuda.Stream(device=dev)

    def loop():
        for s in range(S):
            sw7.eval_device(dZ7[s], b["dinit"], None, dsc7[s:s + 1], None, dfid_e[s:s + 1], stream=stream)

    legs = {
        "a": lambda: sw.eval_device(b["dZ"], b["dinit"], b["dth"], b["dsc"], None, b["dfid"], stream=stream),
        "b": lambda: sw.noise_eval_device(b["dZ"], b["dinit"], dn, b["dth"], b["dsc"], None, dfid_n, stream=stream),
        "c": lambda: sw.grad_device(b["dZ"], b["dinit"], S, b["dth"], b["dsc"], None, b["dfid"], b["dJ"], b["dg"], dgs, stream=stream),
        "d": lambda: sw.noise_grad_device(b["dZ"], b["dinit"], dn, b["dth"], b["dsc"], None, dfid_n, b["dJ"], b["dg"], dgs, dgn, stream=stream),
        "e": loop,
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
    what = {"a": "qc_sweep_eval_dev", "b": "qc_sweep_noise_eval_dev", "c": "qc_sweep_grad_dev, every output", "d": "qc_sweep_noise_grad_dev, every output",
            "e": f"{S} qc_sweep_eval_dev of one sample each"}
    log(f"== config 3's system: N = {pb['N']}, m = {m}, n_pert = {p}, T = {T}, S = {S}; (mfma, chunk, n_chunks) = {sw.launch(S)}; "
        f"noise {S * (T - 1) * p * 8 / 1e6:.1f} MB, per-interval buffer {S * (T - 1) * sw.n_deriv * 8 / 1e6:.1f} MB")
    for k in legs:
        log(f"   ({k}) {what[k]:42s} min {min(times[k]):9.3f}  median {np.median(times[k]):9.3f} ms   rounds: {' '.join(f'{x:.3f}' for x in times[k])}")
    med = {k: float(np.median(v)) for k, v in times.items()}
    spread = lambda k: (max(times[k]) - min(times[k])) / med[k]
    log(f"   medians: b/a = {med['b'] / med['a']:.3f}   d/c = {med['d'] / med['c']:.3f}   e/b = {med['e'] / med['b']:.1f};   "
        f"round-to-round spread (max - min) / median: a {spread('a'):.3f}  b {spread('b'):.3f}  c {spread('c'):.3f}  d {spread('d'):.3f}")
    log(f"   fidelities of the loop (e) against the one call (b): max |difference| = {(dfid_e - dfid_n).abs().max().item():.2e}")
    sw.close()
    sw7.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="64,1024")
    args = ap.parse_args()
    qc = g.load_package()
    lines = []

    def log(sx):
        print(sx, flush=True)
        lines.append(sx)

    log(f"noise-trajectory sweeps, {torch.cuda.get_device_name(0)}, {qc._lib.lib.qc_version().decode()}; device events, {args.rounds} rounds of the "
        f"five legs in turn after 2 warm-up rounds")
    rng = np.random.default_rng(0)
    for S in args.sizes.split(","):
        run_size(qc, int(S), args.rounds, rng, log)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
