#!/usr/bin/env python3
"""The stored-state walk of the "mfma32-sweep" form (wide = QC_SWEEP_WIDE | QC_SWEEP_WIDE_STORED, reserved1[0] = QC_SWEEP_STORED_STATES)
against the closed wide walk, on the same system and inputs: config 5's system (2N = 32, closed: antisymmetric generators, so both walks
serve it; unitary fidelity, 16 columns), S in {64, 1024}:

    (1) qc_sweep_grad_dev, grad only, wide = 1, flag off    totals, seed, the closed wide walk, reduction -- the yardstick
    (2) the same call with wide = 9 and the flag            totals, seed, the store launch, the stored-state wide walk, reduction
    (3) qc_sweep_eval_dev, fidelities                       totals and the finish launch

and on a two-qubit Lindblad system (levels 4, N = 16, 2N = 32, density fidelity, one column, T = 1000): (3) and (2); the closed walk
refuses it.  Device events around whole calls, alternating rounds after warm-up, one handle per setting, one stream.  Every (system, S)
runs in a process of its own under `timeout`; the first that fails ends the run.

MFMA model per interval (sq squarings): forward 288 + 32 sq; closed gradient = forward + walk = 1136 + 128 sq; stored-state gradient =
forward + store (272 + 32 sq, the last interval of a chunk skipped) + walk (800 + 96 sq) = 1360 + 160 sq: (2) / (1) ~ 1.20 at sq = 0 ..
1.25 at large sq, before the state traffic.  An expectation, not a gate.  With --worst LOG the lines "SUMMARY ..." of a run of the GPU
tests (pytest -s tests/test_sweep_wide_open_grad.py) are appended: their worst errors as a share of their bounds.

    python profiles/sweep_wide_open_bench.py [--rounds 5] [--worst LOG] [--out profiles/sweep_wide_open_summary.txt]
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
I2 = np.eye(2, dtype=complex)


def run_one(which, S, rounds):
    import torch
    import __graft_entry__ as g
    from sweep_probe import event_ms, squarings
    qc = g.load_package()
    rng = np.random.default_rng(0)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    mk = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    k = np.kron
    if which == "config5":
        inp = qc.config_inputs(5)
        system, T = inp.system, inp.traj.T
        N = system.levels
        perts = [np.asarray(k(qc.GATES["Z"], np.eye(N // 2)), dtype=complex)]      # detuning of the first qubit
        kw = dict(goal=np.asarray(inp.traj.goal["Ũ⃗"], dtype=np.float64), fid_kind="unitary")
        init = qc.operator_to_iso_vec(np.eye(N, dtype=complex))
        controls = np.asarray(inp.traj["a"], dtype=np.float64)
        ts = inp.traj.timestep
        dts = np.asarray(inp.traj[ts]).ravel() if isinstance(ts, str) else np.full(T, float(ts))
        theta, scale = rng.uniform(-0.05, 0.05, (S, 1)), 1.0 + rng.uniform(-0.02, 0.02, (S, system.n_drives))
        settings = ("closed", "stored")
    else:
        T = 1000
        Hd = [0.5 * k(SX, I2), 0.5 * k(SY, I2), 0.5 * k(I2, SX), 0.5 * k(I2, SY)]
        system = qc.OpenQuantumSystem(0.25 * k(SZ, SZ), Hd, [np.sqrt(0.02) * k(SM, I2), np.sqrt(0.02) * k(I2, SM), np.sqrt(0.01) * k(SZ, I2),
                                                             np.sqrt(0.01) * k(I2, SZ)])
        Lz = system.hamiltonian_superoperator(0.5 * (k(SZ, I2) + k(I2, SZ)))
        perts = [np.block([[Lz.real, -Lz.imag], [Lz.imag, Lz.real]])]
        psi = np.array([1.0, 0.0, 0.0, -1.0j]) / np.sqrt(2.0)
        kw = dict(cols=1, goal=np.concatenate([psi.real, psi.imag]), fid_kind="density")
        init = np.zeros(32)
        init[0] = 1.0
        controls, dts = rng.uniform(-1, 1, (4, T)), rng.uniform(0.05, 0.15, T)
        theta, scale = rng.uniform(-0.05, 0.05, (S, 1)), 1.0 + rng.uniform(-0.02, 0.02, (S, 4))
        settings = ("stored",)
    flags = {"closed": dict(), "stored": dict(stored_states=True, wide_stored=True)}
    sws = {s: qc.RolloutSweep(system, perts, T, wide=True, **flags[s], **kw) for s in settings}
    sw = sws["stored"]
    assert all(h.kernel_name == "mfma32-sweep" and h.grad_supported for h in sws.values())
    dZ, dinit, dth, dsc = t(sw.pack(controls, dts)), t(init), t(theta), t(scale)
    dg = {s: mk(sw.Z_len) for s in settings}
    dfid = mk(S)
    stream = torch.cuda.Stream(device=dev)
    calls = {}
    if "closed" in sws:
        calls["(1) qc_sweep_grad_dev, wide = 1, flag off"] = lambda: sws["closed"].grad_device(dZ, dinit, S, dth, dsc, None, None, None, dg["closed"], None,
                                                                                             stream=stream)
    calls["(2) qc_sweep_grad_dev, wide = 9, flag on "] = lambda: sw.grad_device(dZ, dinit, S, dth, dsc, None, None, None, dg["stored"], None, stream=stream)
    calls["(3) qc_sweep_eval_dev, fids              "] = lambda: sw.eval_device(dZ, dinit, dth, dsc, None, dfid, stream=stream)
    times = {c: [] for c in calls}
    with torch.cuda.stream(stream):
        for _ in range(2):
            for fn in calls.values():
                fn()
        stream.synchronize()
        for _ in range(rounds):
            for c, fn in calls.items():
                times[c].append(event_ms(fn, stream))
    n_int, ns = T - 1, sw.ns
    G = np.asarray(system.G_drift) + sum(a * np.asarray(Gk) for a, Gk in zip(controls[:, T // 2], system.G_drives))
    sq = squarings(float(np.abs(dts[T // 2] * G).sum(axis=0).max()))
    print(f"== {which}: 2N = {sw.n}, cols = {sw.cols}, m = {sw.m}, T = {T}, S = {S}; {sw.kernel_name}, (mfma, chunk, n_chunks) = {sw.launch(S)}; "
          f"sq = {sq} at the middle interval; state buffer S (T-1) 2N cols = {S * n_int * ns * 8 / 2**20:.2f} MiB")
    for c, xs in times.items():
        print(f"   {c}  ms per round: {' '.join(f'{x:.3f}' for x in xs)}   median {np.median(xs):.3f}  range {min(xs):.3f} .. {max(xs):.3f}")
    med = {c[:3]: float(np.median(xs)) for c, xs in times.items()}
    model21 = (1360 + 160 * sq) / (1136 + 128 * sq)
    model23 = (1360 + 160 * sq) / (288 + 32 * sq)
    if "(1)" in med:
        diff = float((dg["stored"] - dg["closed"]).abs().max() / max(1.0, float(dg["closed"].abs().max())))
        print(f"   (2) / (1) = {med['(2)'] / med['(1)']:.3f} (MFMA model at this sq: {model21:.2f});  (1) / (3) = {med['(1)'] / med['(3)']:.2f} "
              f"(model {(1136 + 128 * sq) / (288 + 32 * sq):.2f});  (2) / (3) = {med['(2)'] / med['(3)']:.2f} (model {model23:.2f});  "
              f"max |grad stored - grad closed| / max(1, max |grad|) = {diff:.2e}")
    else:
        print(f"   (2) / (3) = {med['(2)'] / med['(3)']:.2f} (MFMA model at this sq: {model23:.2f})")
    for h in sws.values():
        h.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="64,1024")
    ap.add_argument("--systems", default="config5,lindblad2q")
    ap.add_argument("--timeout", type=int, default=240, help="seconds for one (system, S)")
    ap.add_argument("--worst", default=None, help="output of `pytest -m gpu -s tests/test_sweep_wide_open_grad.py`")
    ap.add_argument("--one", nargs=2, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        return run_one(args.one[0], int(args.one[1]), args.rounds)
    lines = [f"the stored-state wide walk against the closed wide walk; device events, {args.rounds} alternating rounds after 2 warm-up rounds"]
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
        lines.append("== the GPU tests' worst errors as a share of their bounds (tests/test_sweep_wide_open_grad.py)")
        for line in open(args.worst):
            i = line.find("SUMMARY ")
            if i >= 0:
                lines.append("   " + line[i + len("SUMMARY "):].rstrip())
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
