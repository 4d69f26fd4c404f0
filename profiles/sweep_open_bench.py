#!/usr/bin/env python3
"""The stored-state walk (reserved1[0] = QC_SWEEP_STORED_STATES) against the closed walk, on the same system and inputs: config 3's system
(2N = 16, "mfma16-sweep", T = 1000; antisymmetric generators, so both walks serve it), S in {64, 1024}:

    (1) qc_sweep_grad_dev, grad only, flag off    the parent's path: totals, seed, closed walk, reduction -- the yardstick
    (2) the same call on a handle with the flag   totals, seed, the store launch, the stored-state walk, reduction
    (3) qc_sweep_eval_dev, fidelities             totals and the finish launch

and on the qubit Lindblad system (N = 4, 2N = 8, density fidelity, T = 1000): (3) and (2); the closed walk refuses it.
Device events around whole calls, alternating rounds after warm-up, one handle per flag, one stream.  Every (system, S) runs in a process
of its own under `timeout`; the first that fails ends the run.

MFMA model per interval (sq squarings): forward 40 + 4 sq; closed gradient = forward + walk = 152 + 16 sq; stored-state gradient =
forward + store (40 + 4 sq, the last interval of a chunk skipped) + walk (104 + 12 sq) = 184 + 20 sq: (2) / (1) ~ 1.21 at sq = 0 .. 1.24
at large sq.  An expectation, not a gate.  With --worst LOG the lines "SUMMARY ..." of a run of the GPU tests (pytest -s
tests/test_sweep_open_grad.py) are appended: their worst errors as a share of their bounds.

    python profiles/sweep_open_bench.py [--rounds 5] [--worst LOG] [--out profiles/sweep_open_summary.txt]
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SX = np.array([[0, 1], [1, 0]], dtype=complex)
SY = np.array([[0, -1j], [1j, 0]], dtype=complex)
SZ = np.array([[1, 0], [0, -1]], dtype=complex)
SM = np.array([[0, 1], [0, 0]], dtype=complex)


def run_one(which, S, rounds):
    import torch
    import __graft_entry__ as g
    from sweep_probe import event_ms, make_problem
    qc = g.load_package()
    rng = np.random.default_rng(0)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    mk = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    T = 1000
    if which == "config3":
        pb = make_problem(qc, "config3", T, S, rng)
        system, perts = qc.QuantumSystem(pb["H0"], pb["Hd"]), [np.asarray(pb["P"], dtype=complex)]
        kw = dict(goal=pb["goal"], fid_kind="unitary")
        init = qc.operator_to_iso_vec(np.eye(system.levels, dtype=complex))
        controls, dts, theta, scale = pb["controls"], pb["dts"], pb["theta"], pb["scale"]
        flags = (False, True)
    else:
        system = qc.OpenQuantumSystem(0.4 * SZ, [0.5 * SX, 0.5 * SY], [np.sqrt(0.02) * SM, np.sqrt(0.01) * SZ])
        Lz = system.hamiltonian_superoperator(0.5 * SZ)
        perts = [np.block([[Lz.real, -Lz.imag], [Lz.imag, Lz.real]])]
        kw = dict(cols=1, goal=np.array([0.0, 1.0, 0.0, 0.0]), fid_kind="density")
        init = np.zeros(8)
        init[0] = 1.0
        controls, dts = rng.uniform(-1, 1, (2, T)), rng.uniform(0.05, 0.15, T)
        theta, scale = rng.uniform(-0.05, 0.05, (S, 1)), 1.0 + rng.uniform(-0.02, 0.02, (S, 2))
        flags = (True,)
    sws = {f: qc.RolloutSweep(system, perts, T, stored_states=f, **kw) for f in flags}
    sw = sws[True]
    dZ, dinit, dth, dsc = t(sw.pack(controls, dts)), t(init), t(theta), t(scale)
    dg = {f: mk(sw.Z_len) for f in flags}
    dfid = mk(S)
    stream = torch.cuda.Stream(device=dev)
    calls = {}
    if False in flags:
        calls["(1) qc_sweep_grad_dev, flag off"] = lambda: sws[False].grad_device(dZ, dinit, S, dth, dsc, None, None, None, dg[False], None, stream=stream)
    calls["(2) qc_sweep_grad_dev, flag on "] = lambda: sw.grad_device(dZ, dinit, S, dth, dsc, None, None, None, dg[True], None, stream=stream)
    calls["(3) qc_sweep_eval_dev, fids    "] = lambda: sw.eval_device(dZ, dinit, dth, dsc, None, dfid, stream=stream)
    times = {k: [] for k in calls}
    with torch.cuda.stream(stream):
        for _ in range(2):
            for fn in calls.values():
                fn()
        stream.synchronize()
        for _ in range(rounds):
            for k, fn in calls.items():
                times[k].append(event_ms(fn, stream))
    n_int, ns = T - 1, sw.ns
    print(f"== {which}: 2N = {sw.n}, m = {sw.m}, T = {T}, S = {S}; {sw.kernel_name}, (mfma, chunk, n_chunks) = {sw.launch(S)}; "
          f"state buffer S (T-1) 2N cols = {S * n_int * ns * 8 / 2**20:.2f} MiB")
    for k, xs in times.items():
        print(f"   {k}  ms per round: {' '.join(f'{x:.3f}' for x in xs)}   median {np.median(xs):.3f}  range {min(xs):.3f} .. {max(xs):.3f}")
    med = {k[:3]: float(np.median(xs)) for k, xs in times.items()}
    if "(1)" in med:
        diff = float((dg[True] - dg[False]).abs().max() / max(1.0, float(dg[False].abs().max())))
        print(f"   (2) / (1) = {med['(2)'] / med['(1)']:.3f} (MFMA model: 1.21 .. 1.24);  (1) / (3) = {med['(1)'] / med['(3)']:.2f} (model 3.8 .. 4.0);  "
              f"(2) / (3) = {med['(2)'] / med['(3)']:.2f} (model 4.6 .. 5.0);  max |grad on - grad off| / max(1, max |grad|) = {diff:.2e}")
    else:
        print(f"   (2) / (3) = {med['(2)'] / med['(3)']:.2f} (MFMA model 4.6 .. 5.0)")
    for s in sws.values():
        s.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="64,1024")
    ap.add_argument("--systems", default="config3,lindblad")
    ap.add_argument("--timeout", type=int, default=240, help="seconds for one (system, S)")
    ap.add_argument("--worst", default=None, help="output of `pytest -m gpu -s tests/test_sweep_open_grad.py`")
    ap.add_argument("--one", nargs=2, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        return run_one(args.one[0], int(args.one[1]), args.rounds)
    lines = [f"the stored-state walk against the closed walk; device events, {args.rounds} alternating rounds after 2 warm-up rounds"]
    print(lines[0], flush=True)
    rc = 0
    for which in args.systems.split(","):
        for S in args.sizes.split(","):
            r = subprocess.run(["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--rounds", str(args.rounds),
                                "--one", which, S], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            print(r.stdout, end="", flush=True)
            lines += r.stdout.rstrip().split("\n")
            if r.returncode != 0:      # nothing more is started on the device after a failed step
                lines.append(f"   {which} S = {S}: exit status {r.returncode}; stopped")
                print(lines[-1], flush=True)
                rc = r.returncode
                break
        if rc:
            break
    if args.worst and not rc:
        lines.append("== the GPU tests' worst errors as a share of their bounds (tests/test_sweep_open_grad.py)")
        for line in open(args.worst):
            k = line.find("SUMMARY ")
            if k >= 0:
                lines.append("   " + line[k + len("SUMMARY "):].rstrip())
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
