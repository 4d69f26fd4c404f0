#!/usr/bin/env python3
"""Wide noise-trajectory sweeps ("mfma32-sweep" handles made with QC_SWEEP_WIDE_NOISE) against what they extend and what they replace.

Systems: those of profiles/sweep_wide_bench.py -- config 5's (4 qubits, N = 16, 8 drives, its own T = 500; ONE perturbation, the detuning of
the first qubit) and two coupled three-level transmons (N = 9, 4 drives, T = 100; TWO perturbations, the number operators of both) --
each at S in {64, 1024}:

    (a) on one handle:  qc_sweep_eval_dev against qc_sweep_noise_eval_dev (fidelities), and qc_sweep_grad_dev against
        qc_sweep_noise_grad_dev (fids, J, the dense gradient; the noise call also grad_noise).  The MFMA counts per interval are equal
        (288 + 32 sq forward, 848 + 96 sq backward); the noise call adds n_pert image reads of 8 loads a lane and 16 n_pert fmas per
        interval, the gradient n_pert wave sums.
    (b) additive noise on drive 0 (P_0 = G_0), which the library could already express: ONE noise call for S realisations against the
        loop of S single-sample qc_sweep_eval_dev calls on a wide handle without perturbations, each with the noise written into a
        trajectory vector of its own (the S vectors are on the device before the clock starts: the loop's best case).

Timed by device events on one stream, the two sides alternating over the rounds after one warm-up round; every round is reported.

    python profiles/sweep_wide_noise_bench.py [--rounds 5] [--out profiles/sweep_wide_noise_summary.txt]
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
from sweep_probe import event_ms, squarings  # noqa: E402
from sweep_wide_bench import make_problem  # noqa: E402

fmt = lambda xs: " ".join(f"{x:.3f}" for x in xs)


def perturbations(pb):
    if pb["which"] == "config5":
        return [pb["P"]]
    import transmon_robustness as tr
    b = np.diag(np.sqrt(np.arange(1.0, tr.LEVELS)), 1).astype(complex)
    return [pb["P"], np.kron(np.eye(tr.LEVELS, dtype=complex), b.conj().T @ b)]


def run_size(qc, which, S, rounds, rng, log):
    pb = make_problem(qc, which, S, rng)
    T, N, m = pb["T"], pb["N"], pb["m"]
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    perts = perturbations(pb)
    p = len(perts)
    sigma = float(np.abs(pb["theta"]).max())
    noise = rng.uniform(-sigma, sigma, (S, T - 1, p))
    theta = np.repeat(pb["theta"], p, axis=1)
    sw = qc.RolloutSweep(pb["system"], perts, T, goal=pb["goal"], fid_kind="unitary", subspace=pb["subspace"], wide=True, wide_noise=True)
    assert sw.kernel_name == "mfma32-sweep" and sw.noise_supported and sw.grad_supported
    Z = sw.pack(pb["controls"], pb["dts"])
    init = qc.operator_to_iso_vec(np.eye(N, dtype=complex))
    b = dict(dZ=t(Z), dinit=t(init), dth=t(theta), dsc=t(pb["scale"]), dn=t(noise), dzero=torch.zeros((S, T - 1, p), dtype=torch.float64, device=dev),
             fa=new(S), fb=new(S), ga=new(sw.Z_len), gb=new(sw.Z_len), Ja=new(1), Jb=new(1), gn=new(S, T - 1, p))
    stream = torch.cuda.Stream(device=dev)
    calls = {
        "eval": lambda: sw.eval_device(b["dZ"], b["dinit"], b["dth"], b["dsc"], None, b["fa"], stream=stream),
        "noise_eval": lambda: sw.noise_eval_device(b["dZ"], b["dinit"], b["dn"], b["dth"], b["dsc"], None, b["fb"], stream=stream),
        "grad": lambda: sw.grad_device(b["dZ"], b["dinit"], S, b["dth"], b["dsc"], None, b["fa"], b["Ja"], b["ga"], stream=stream),
        "noise_grad": lambda: sw.noise_grad_device(b["dZ"], b["dinit"], b["dn"], b["dth"], b["dsc"], None, b["fb"], b["Jb"], b["gb"], None, b["gn"],
                                                   stream=stream),
    }
    times = {k: [] for k in calls}
    with torch.cuda.stream(stream):
        for f in calls.values():
            f()
        stream.synchronize()
        for _ in range(rounds):
            for k, f in calls.items():
                times[k].append(event_ms(f, stream))
        # at zero noise the noise calls give the values of the plain calls
        sw.noise_grad_device(b["dZ"], b["dinit"], b["dzero"], b["dth"], b["dsc"], None, b["fb"], b["Jb"], b["gb"], None, b["gn"], stream=stream)
        sw.grad_device(b["dZ"], b["dinit"], S, b["dth"], b["dsc"], None, b["fa"], b["Ja"], b["ga"], stream=stream)
        stream.synchronize()
        same = bool(torch.equal(b["fa"], b["fb"]) and torch.equal(b["ga"], b["gb"]) and torch.equal(b["Ja"], b["Jb"]))
    G0 = qc.iso_generator(np.asarray(pb["system"].H_drift))
    Gd = [qc.iso_generator(np.asarray(H)) for H in pb["system"].H_drives]
    sq = float(np.mean([squarings(np.abs(pb["dts"][k] * (G0 + sum(a * G for a, G in zip(pb["controls"][:, k], Gd)))).sum(axis=0).max()) for k in range(T - 1)]))
    med = {k: float(np.median(v)) for k, v in times.items()}
    log(f"== (a) {which}: N = {N} (2N = {2 * N}), m = {m}, n_pert = {p}, T = {T}, S = {S}; launch (mfma, chunk, n_chunks) = {sw.launch(S)}; "
        f"squarings per interval (unperturbed): mean {sq:.2f}")
    for k in calls:
        log(f"   {k:<11s} ms per round: {fmt(times[k])}   min {min(times[k]):.3f}  median {med[k]:.3f}")
    log(f"   median noise_eval / eval = {med['noise_eval'] / med['eval']:.3f}; median noise_grad / grad = {med['noise_grad'] / med['grad']:.3f}; "
        f"generators read per interval: {m} -> {m + p} forward ({(m + p) / max(m, 1):.3f}), contractions per interval {m} -> {m + p}; "
        f"zero noise gives the bits of grad (fids, J, grad): {same}")
    sw.close()

    # (b) additive noise on drive 0: one noise call against S single-sample calls
    add = qc.RolloutSweep(pb["system"], [np.asarray(pb["system"].H_drives[0])], T, wide=True, wide_noise=True)
    plain = qc.RolloutSweep(pb["system"], [], T, wide=True)
    assert add.kernel_name == plain.kernel_name == "mfma32-sweep"
    amp = 0.05 * float(np.abs(pb["controls"]).max())
    xi = rng.uniform(-amp, amp, (S, T - 1))
    Zs = np.empty((S, plain.Z_len))
    for s in range(S):
        cs = pb["controls"].copy()
        cs[0, :T - 1] += xi[s]
        Zs[s] = plain.pack(cs, pb["dts"])
    d = dict(dZ=t(add.pack(pb["controls"], pb["dts"])), dZs=t(Zs), dinit=t(init), dxi=t(xi[:, :, None]), one=new(S, add.ns), loop=new(S, add.ns))
    rows = [d["dZs"][s] for s in range(S)]
    outs = [d["loop"][s:s + 1] for s in range(S)]
    f_one = lambda: add.noise_eval_device(d["dZ"], d["dinit"], d["dxi"], None, None, d["one"], None, stream=stream)

    def f_loop():
        for s in range(S):
            plain.eval_device(rows[s], d["dinit"], None, None, outs[s], None, stream=stream)

    t_one, t_loop = [], []
    with torch.cuda.stream(stream):
        f_one(); f_loop()
        stream.synchronize()
        for _ in range(rounds):
            t_one.append(event_ms(f_one, stream))
            t_loop.append(event_ms(f_loop, stream))
        err = float((d["one"] - d["loop"]).abs().max())
    log(f"== (b) {which}, S = {S}: additive noise on drive 0 (P_0 = G_0), final states of all S realisations")
    log(f"   one noise call               ms per round: {fmt(t_one)}   min {min(t_one):.3f}  max {max(t_one):.3f}")
    log(f"   loop of S single-sample eval ms per round: {fmt(t_loop)}   min {min(t_loop):.3f}  max {max(t_loop):.3f}")
    log(f"   every round of the one call below every round of the loop: {max(t_one) < min(t_loop)}; median loop / median one call = "
        f"{np.median(t_loop) / np.median(t_one):.1f}; max |difference of the final states| = {err:.1e}")
    add.close()
    plain.close()
    return max(t_one) < min(t_loop)


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

    log(f"wide noise-trajectory sweeps, {torch.cuda.get_device_name(0)}, {qc._lib.lib.qc_version().decode()}; device events around whole calls, "
        f"{args.rounds} alternating rounds after one warm-up round, one process")
    rng = np.random.default_rng(0)
    ok = True
    for which in args.systems.split(","):
        for S in args.sizes.split(","):
            ok = run_size(qc, which, int(S), args.rounds, rng, log) and ok
    log(f"acceptance of (b), every round of the one call below every round of the loop at every size: {ok}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
