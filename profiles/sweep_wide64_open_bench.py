#!/usr/bin/env python3
"""Stored-state gradients in the "mfma64-sweep" form (csrc/qc_sweep64_open_grad.hip) against the closed walk and the forward sweep.

One process per (system, S); device events around whole calls on one stream; alternating rounds after one warm-up round.

    transmons3   the three-transmon system of examples/three_transmon_robustness.py (closed: antisymmetric generators), the 8 computational
                 kets as the state (nc = 8, nct = 1), no fidelity: qc_sweep_vjp_dev (grad) with unit cotangents
    lindblad5    a five-level transmon with relaxation and dephasing in the Lindblad form (N = 25, 2N = 50), the density fidelity, one
                 column: qc_sweep_grad_dev (fids, grad).  The closed walk does not serve it: column (1) is empty there.

Columns: (1) the call with the flag off (closed walk), (2) with reserved1[0] = QC_SWEEP_STORED_STATES and QC_SWEEP_WIDE_64_STORED (store
launch + stored-state walk), (3) qc_sweep_eval_dev.  Beside (2)/(1) and (2)/(3) stand the ratios of the MFMA model per interval and
workgroup:  eval (9 + sq) x 256;  closed call 6656 + 1152 nct + 1024 sq;  stored-state call 8448 + 1152 nct + 1280 sq
(totals 2304 + 256 sq, store (8 + sq) x 256 + 64 nct, walk 4096 + 1088 nct + 768 sq).  The state buffer is S x (T-1) x 2N x cols doubles.

--existing times eval, grad and noise_grad on handles WITHOUT the bit (transmons3 with its unitary fidelity): run it once with the
library of the parent commit (QCOLLOC_HIP_VARIANT=parent) and once with this one, alternating processes on one machine; each median
of this commit must be at or below the parent's largest round.

    python profiles/sweep_wide64_open_bench.py --system lindblad5 --S 64 [--rounds 5] [--existing] [--out FILE]    (profiles/sweep_wide64_open_summary.txt)
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
from sweep_wide64_bench import make_problem, mean_squarings, squarings  # noqa: E402

CLOSED = dict(wide=True, wide64=True, wide64_grad=True)
OPEN = dict(CLOSED, stored_states=True, wide64_stored=True)


def _iso_operator(L):
    return np.block([[L.real, -L.imag], [L.imag, L.real]])


def lindblad5(qc, S, T, rng):
    a = np.diag(np.sqrt(np.arange(1.0, 5.0)), 1).astype(complex)
    num = a.conj().T @ a
    H0 = -0.75 * num @ (num - np.eye(5))
    Hd = [0.5 * (a + a.conj().T), 0.5j * (a - a.conj().T)]
    system = qc.OpenQuantumSystem(H0, Hd, [np.sqrt(1.0 / 80.0) * a, np.sqrt(0.005) * num])
    P = _iso_operator(system.hamiltonian_superoperator(num))
    goal = np.zeros(10)
    goal[1] = 1.0
    rho0 = np.zeros(50)
    rho0[0] = 1.0
    window = np.sin(np.pi * np.linspace(0.0, 1.0, T)) ** 2
    return dict(which="lindblad5", N=25, m=2, T=T, S=S, system=system, P=P, goal=goal, init=rho0, controls=rng.uniform(-1, 1, (2, 1)) * window,
                dts=np.full(T, 6.0 / (T - 1)), theta=rng.uniform(-0.05, 0.05, (S, 1)), scale=1.0 + rng.uniform(-0.02, 0.02, (S, 2)), cols=1)


def lindblad_mean_squarings(pb):
    G0, Gd = np.asarray(pb["system"].G_drift), [np.asarray(G) for G in pb["system"].G_drives]
    total = 0
    for s in range(pb["S"]):
        for k in range(pb["T"] - 1):
            G = G0 + pb["theta"][s, 0] * pb["P"] + sum(pb["scale"][s, q] * pb["controls"][q, k] * Gd[q] for q in range(2))
            total += squarings(np.abs(pb["dts"][k] * G).sum(axis=0).max())
    return total / (pb["S"] * (pb["T"] - 1))


def timed(calls, rounds, stream):
    times = {k: [] for k in calls}
    with torch.cuda.stream(stream):
        for f in calls.values():
            f()
        stream.synchronize()
        for _ in range(rounds):
            for k, f in calls.items():
                times[k].append(event_ms(f, stream))
    return times


def run(qc, which, S, T, rounds, log):
    rng = np.random.default_rng(0)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    stream = torch.cuda.Stream(device=dev)
    calls, handles = {}, []
    if which == "lindblad5":
        pb = lindblad5(qc, S, T, rng)
        sq = lindblad_mean_squarings(pb)
        sw = qc.RolloutSweep(pb["system"], [pb["P"]], T, cols=1, goal=pb["goal"], fid_kind="density", **OPEN)
        handles.append(sw)
        dZ, dinit, dth, dsc = t(sw.pack(pb["controls"], pb["dts"])), t(pb["init"]), t(pb["theta"]), t(pb["scale"])
        f2, f3, g2 = new(S), new(S), new(sw.Z_len)
        calls["2"] = lambda: sw.grad_device(dZ, dinit, S, dth, dsc, None, f2, None, g2, None, stream=stream)
        calls["3"] = lambda: sw.eval_device(dZ, dinit, dth, dsc, None, f3, stream=stream)
    else:
        import three_transmon_robustness as tr
        pb = make_problem(qc, "transmons3", S, T, rng)
        sq = mean_squarings(qc, pb)
        kets = np.zeros((27, 8), dtype=complex)
        kets[tr.SUBSPACE, np.arange(8)] = 1.0
        init = qc.operator_to_iso_vec(kets)
        off = qc.RolloutSweep(pb["system"], [pb["P"]], T, cols=8, **CLOSED)
        on = qc.RolloutSweep(pb["system"], [pb["P"]], T, cols=8, **OPEN)
        handles += [off, on]
        sw = on
        cot = rng.standard_normal((S, on.ns))
        dZ, dinit, dth, dsc, dcot = t(on.pack(pb["controls"], pb["dts"])), t(init), t(pb["theta"]), t(pb["scale"]), t(cot / np.linalg.norm(cot, axis=1, keepdims=True))
        g1, g2, x3 = new(on.Z_len), new(on.Z_len), new(S, on.ns)
        calls["1"] = lambda: off.vjp_device(dZ, dinit, S, dcot, dth, dsc, dgrad=g1, stream=stream)
        calls["2"] = lambda: on.vjp_device(dZ, dinit, S, dcot, dth, dsc, dgrad=g2, stream=stream)
        calls["3"] = lambda: on.eval_device(dZ, dinit, dth, dsc, x3, None, stream=stream)
    assert sw.kernel_name == "mfma64-sweep" and sw.vjp_supported
    times = timed(calls, rounds, stream)
    nct = -(-sw.cols // 16)
    model = {"1": 6656 + 1152 * nct + 1024 * sq, "2": 8448 + 1152 * nct + 1280 * sq, "3": 2304 + 256 * sq}
    med = {k: float(np.median(v)) for k, v in times.items()}
    fmt = lambda xs: " ".join(f"{x:.3f}" for x in xs)
    log(f"== {which}: 2N = {sw.n}, m = {sw.m}, p = 1, {sw.cols} state columns (nct = {nct}), T = {T}, S = {S}; launch (mfma, chunk, n_chunks) = {sw.launch(S)}; "
        f"squarings per interval, mean: {sq:.3f}; state buffer {S * (T - 1) * sw.ns * 8 / 2 ** 20:.2f} MiB ({sw.ns} doubles a knot)")
    names = {"1": "(1) flag off: closed walk      ", "2": "(2) flag and bit: stored states", "3": "(3) eval                       "}
    for k in ("1", "2", "3"):
        if k in times:
            log(f"   {names[k]} ms per round: {fmt(times[k])}   min {min(times[k]):.3f}  median {med[k]:.3f}  (MFMA model {model[k]:.0f} per interval and workgroup)")
    if "1" in med:
        r, rm = med["2"] / med["1"], model["2"] / model["1"]
        log(f"   (2)/(1) measured {r:.3f}, model {rm:.3f}: measured / model = {r / rm:.3f} (yardstick: within 1.11)")
    r, rm = med["2"] / med["3"], model["2"] / model["3"]
    log(f"   (2)/(3) measured {r:.3f}, model {rm:.3f}: measured / model = {r / rm:.3f} (yardstick: within 1.11)")
    for h in handles:
        h.close()


def run_existing(qc, S, T, rounds, log):
    """eval, grad and noise_grad on handles without the bit: the calls whose kernels this commit must not move."""
    rng = np.random.default_rng(0)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    stream = torch.cuda.Stream(device=dev)
    pb = make_problem(qc, "transmons3", S, T, rng)
    sw = qc.RolloutSweep(pb["system"], [pb["P"]], T, goal=pb["goal"], fid_kind="unitary", subspace=pb["subspace"], wide64_noise=True, **CLOSED)
    dZ, dinit, dth, dsc = t(sw.pack(pb["controls"], pb["dts"])), t(qc.operator_to_iso_vec(np.eye(27, dtype=complex))), t(pb["theta"]), t(pb["scale"])
    dn = t(np.zeros((S, T - 1, 1)))
    fe, fg, fn, gg, gn, gnn = new(S), new(S), new(S), new(sw.Z_len), new(sw.Z_len), new(S, T - 1, 1)
    calls = {"eval": lambda: sw.eval_device(dZ, dinit, dth, dsc, None, fe, stream=stream),
             "grad": lambda: sw.grad_device(dZ, dinit, S, dth, dsc, None, fg, None, gg, None, stream=stream),
             "noise_grad": lambda: sw.noise_grad_device(dZ, dinit, dn, dth, dsc, None, fn, None, gn, None, gnn, stream=stream)}
    times = timed(calls, rounds, stream)
    log(f"== existing calls, transmons3 (unitary, 27 columns), T = {T}, S = {S}, handle wide = {sw._desc.wide}")
    for k, v in times.items():
        log(f"   {k:<11} ms per round: {' '.join(f'{x:.3f}' for x in v)}   min {min(v):.3f}  median {np.median(v):.3f}  max {max(v):.3f}")
    sw.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--system", default="lindblad5", choices=("lindblad5", "transmons3"))
    ap.add_argument("--S", type=int, default=64)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--existing", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sweep_wide64_open_bench.py measures on a GPU; none is visible")
    qc = g.load_package()
    lines = []

    def log(sx):
        print(sx, flush=True)
        lines.append(sx)

    log(f"mfma64-sweep stored-state gradients, {torch.cuda.get_device_name(0)}, {qc._lib.lib.qc_version().decode()}, library {os.path.basename(qc._lib.LIB_PATH)}; "
        f"device events, {args.rounds} alternating rounds after one warm-up round, one process per (system, S)")
    if args.existing:
        run_existing(qc, args.S, args.T, args.rounds, log)
    else:
        run(qc, args.system, args.S, args.T, args.rounds, log)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
