#!/usr/bin/env python3
"""Sweep pullbacks against sweep gradients, on the same handle and inputs: config 3's system (2N = 16, "mfma16-sweep", T = 1000) and,
wide, config 5's system (2N = 32, "mfma32-sweep", T = 500), S in {64, 1024}.

    (g) qc_sweep_grad_dev, grad only          the fidelity seed, the walk, the weighted reduction
    (v) qc_sweep_vjp_dev, grad only           the cotangent seed, the same walk, the plain sum
    (i) (v) plus grad_init                    one more transposed product per sample in the seed
    (f) (v) plus finals                       one more store per sample in the seed

timed by device events in alternating rounds after warm-up, on one handle and one stream.  (g) and (v) launch the same forward kernel
and the same walk and differ in the seed and the reduction only, so the expectation is parity: an expectation, not a gate.  With
--worst LOG the lines "SWEEP-VJP ..." of a run of the GPU tests (pytest -s) are appended: their worst errors over their bounds.

    python profiles/sweep_vjp_bench.py [--rounds 7] [--worst LOG] [--out profiles/sweep_vjp_summary.txt]
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
from sweep_probe import event_ms, make_problem  # noqa: E402


def problem(qc, which, S, rng):
    """(system, perturbation, T, goal, controls, dts, theta, scale, wide)"""
    if which == "config3":
        pb = make_problem(qc, "config3", 1000, S, rng)
        return qc.QuantumSystem(pb["H0"], pb["Hd"]), pb["P"], 1000, pb["goal"], pb["controls"], pb["dts"], pb["theta"], pb["scale"], False
    inp = qc.config_inputs(5, T=500)
    system, T = inp.system, inp.traj.T
    P = np.kron(qc.GATES["Z"], np.eye(system.levels // 2))            # detuning of the first qubit
    ts = inp.traj.timestep
    dts = np.asarray(inp.traj[ts]).ravel() if isinstance(ts, str) else np.full(T, float(ts))
    theta, scale = rng.uniform(-0.05, 0.05, (S, 1)), 1.0 + rng.uniform(-0.02, 0.02, (S, system.n_drives))
    return system, P, T, np.asarray(inp.traj.goal["Ũ⃗"], dtype=np.float64), np.asarray(inp.traj["a"], dtype=np.float64), dts, theta, scale, True


def run_size(qc, which, S, rounds, rng, log):
    system, P, T, goal, controls, dts, theta, scale, wide = problem(qc, which, S, rng)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    sw = qc.RolloutSweep(system, [np.asarray(P, dtype=complex)], T, goal=goal, fid_kind="unitary", wide=wide)
    assert sw.grad_supported and sw.vjp_supported
    N = system.levels
    cot = rng.standard_normal((S, sw.ns))
    cot /= np.linalg.norm(cot, axis=1, keepdims=True)
    mk = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    dZ, dinit, dth, dsc, dcot = t(sw.pack(controls, dts)), t(qc.operator_to_iso_vec(np.eye(N, dtype=complex))), t(theta), t(scale), t(cot)
    dJ, dg, dv, dgi, dfin = mk(1), mk(sw.Z_len), mk(sw.Z_len), mk(S, sw.ns), mk(S, sw.ns)
    stream = torch.cuda.Stream(device=dev)
    calls = {
        "(g) qc_sweep_grad_dev, grad": lambda: sw.grad_device(dZ, dinit, S, dth, dsc, None, None, None, dg, None, stream=stream),
        "(v) qc_sweep_vjp_dev, grad ": lambda: sw.vjp_device(dZ, dinit, S, dcot, dth, dsc, dgrad=dv, stream=stream),
        "(i) (v) + grad_init        ": lambda: sw.vjp_device(dZ, dinit, S, dcot, dth, dsc, dgrad=dv, dgrad_init=dgi, stream=stream),
        "(f) (v) + finals           ": lambda: sw.vjp_device(dZ, dinit, S, dcot, dth, dsc, dgrad=dv, dfinals=dfin, stream=stream),
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
    log(f"== {which}: N = {N} (2N = {2 * N}), m = {system.n_drives}, T = {T}, S = {S}; {sw.kernel_name}, (mfma, chunk, n_chunks) = {sw.launch(S)}")
    for k, xs in times.items():
        log(f"   {k}  ms per round: {' '.join(f'{x:.3f}' for x in xs)}   median {np.median(xs):.3f}  range {min(xs):.3f} .. {max(xs):.3f}")
    med = {k[:3]: float(np.median(xs)) for k, xs in times.items()}
    log(f"   median (v) / median (g) = {med['(v)'] / med['(g)']:.3f} (expectation: parity);  grad_init on top: {1e3 * (med['(i)'] - med['(v)']):+.1f} us "
        f"({100 * (med['(i)'] / med['(v)'] - 1):+.2f} %);  finals on top: {1e3 * (med['(f)'] - med['(v)']):+.1f} us ({100 * (med['(f)'] / med['(v)'] - 1):+.2f} %)")
    sw.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="64,1024")
    ap.add_argument("--systems", default="config3,config5")
    ap.add_argument("--worst", default=None, help="output of `pytest -m gpu -s tests/test_sweep_vjp.py tests/test_sweep_vjp_wide.py`")
    args = ap.parse_args()
    qc = g.load_package()
    lines = []

    def log(sx):
        print(sx, flush=True)
        lines.append(sx)

    log(f"sweep pullback against the sweep gradient, {torch.cuda.get_device_name(0)}, {qc._lib.lib.qc_version().decode()}; device events, "
        f"{args.rounds} alternating rounds after 2 warm-up rounds")
    rng = np.random.default_rng(0)
    for which in args.systems.split(","):
        for S in args.sizes.split(","):
            run_size(qc, which, int(S), args.rounds, rng, log)
    if args.worst:
        log("== the GPU tests' worst errors over their bounds (tests/test_sweep_vjp.py, tests/test_sweep_vjp_wide.py)")
        for line in open(args.worst):
            k = line.find("SWEEP-VJP ")
            if k >= 0:
                log("   " + line[k + len("SWEEP-VJP "):].rstrip())
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
