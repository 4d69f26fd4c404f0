#!/usr/bin/env python3
"""The wide sweep Hessian product ("mfma32-sweep" handles made with QC_SWEEP_WIDE_HESSIAN) against the wide pullback and the wide
pushforward on the same handle.

Systems: those of profiles/sweep_wide_bench.py -- config 5's (4 qubits, N = 16, 8 drives, its own T = 500) and two coupled three-level
transmons (N = 9, 4 drives, T = 100) -- each at S in {64, 1024}, on one handle made with wide = 1 | 16 | 256:

    (a) qc_sweep_vjp_dev  producing grad    qc_sweep_mfma32_kernel, the seed, qc_sweep32_grad_kernel<false>, the plain sum
    (b) qc_sweep_jvp_dev                    qc_sweep32_jvp_kernel + qc_sweep32_jvp_finish_kernel
    (c) qc_sweep_hvp_dev  producing tgrad   qc_sweep32_jvp_kernel, qc_sweep32_hvp_seed_kernel, qc_sweep32_hvp_kernel, the plain sum

timed by device events on one stream, (a), (b), (c) alternating over the rounds after one warm-up round.  MFMA counts per interval:
(a) 288 + 32 sq forward + 848 + 96 sq backward = 1136 + 128 sq; (b) 864 + 96 sq; (c) 864 + 96 sq for the tangent totals + 3120 + 288 sq
for the walk = 3984 + 384 sq.  The condition of the kernel's acceptance: (c) <= 1.25 x (the count's ratio) x (a) in every round.  The
share of the f64 matrix peak is the MFMA work of the call over the call's time: an end-to-end figure, not a kernel's.  What a user
without the product would do instead -- a central difference of two pullbacks, 2.0 (a) -- is run once and its distance to tgrad recorded.

    python profiles/sweep_wide_hvp_bench.py [--rounds 5] [--out profiles/sweep_wide_hvp_summary.txt]
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

MARGIN = 1.25


def run_size(qc, which, S, rounds, rng, log):
    pb = make_problem(qc, which, S, rng)
    T, N, m = pb["T"], pb["N"], pb["m"]
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    sw = qc.RolloutSweep(pb["system"], [pb["P"]], T, goal=pb["goal"], fid_kind="unitary", subspace=pb["subspace"], wide=True, wide_tangent=True,
                         wide_hessian=True)
    assert sw.kernel_name == "mfma32-sweep" and sw.jvp_supported and sw.hvp_supported and sw.vjp_supported
    vrng = np.random.default_rng(1)
    vZ = sw.pack(vrng.standard_normal((m, T)) * np.abs(pb["controls"]).max(), 0.01 * pb["dts"] * vrng.standard_normal(T))
    Z = sw.pack(pb["controls"], pb["dts"])
    cot = vrng.standard_normal((S, sw.ns)) / np.sqrt(sw.ns)
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    b = dict(dZ=t(Z), dvZ=t(vZ), dinit=t(qc.operator_to_iso_vec(np.eye(N, dtype=complex))), dth=t(pb["theta"]), dsc=t(pb["scale"]), cot=t(cot),
             ga=new(sw.Z_len), xb=new(S, sw.ns), tb=new(S, sw.ns), gc=new(sw.Z_len))
    stream = torch.cuda.Stream(device=dev)
    fa = lambda: sw.vjp_device(b["dZ"], b["dinit"], S, b["cot"], b["dth"], b["dsc"], dgrad=b["ga"], stream=stream)
    fb = lambda: sw.jvp_device(b["dZ"], b["dinit"], S, b["dth"], b["dsc"], dvZ=b["dvZ"], dfinals=b["xb"], dtfinals=b["tb"], stream=stream)
    fc = lambda: sw.hvp_device(b["dZ"], b["dinit"], S, b["cot"], b["dth"], b["dsc"], dvZ=b["dvZ"], dtgrad=b["gc"], stream=stream)
    with torch.cuda.stream(stream):
        fa(); fb(); fc()
        stream.synchronize()
        ta, tb, tc = [], [], []
        for _ in range(rounds):
            ta.append(event_ms(fa, stream))
            tb.append(event_ms(fb, stream))
            tc.append(event_ms(fc, stream))
        # the central difference of two pullbacks a user would otherwise take: step 1e-6 along vZ
        eps = 1e-6
        gp, gm = new(sw.Z_len), new(sw.Z_len)
        sw.vjp_device(b["dZ"] + eps * b["dvZ"], b["dinit"], S, b["cot"], b["dth"], b["dsc"], dgrad=gp, stream=stream)
        sw.vjp_device(b["dZ"] - eps * b["dvZ"], b["dinit"], S, b["cot"], b["dth"], b["dsc"], dgrad=gm, stream=stream)
        stream.synchronize()
        fd = (gp - gm) / (2 * eps)
        fd_err = float((fd - b["gc"]).abs().max() / b["gc"].abs().max())
    G0 = qc.iso_generator(np.asarray(pb["system"].H_drift))
    Gd = [qc.iso_generator(np.asarray(H)) for H in pb["system"].H_drives]
    sq = float(np.mean([squarings(np.abs(pb["dts"][k] * (G0 + sum(a * G for a, G in zip(pb["controls"][:, k], Gd)))).sum(axis=0).max()) for k in range(T - 1)]))
    mf_a, mf_b, mf_c = 1136 + 128 * sq, 864 + 96 * sq, 3984 + 384 * sq
    per_mfma = 2 * 16 * 16 * 4
    share = lambda mf, ms: 100 * S * (T - 1) * mf * per_mfma / (ms * 1e-3) / 1e12 / PEAK_F64_MATRIX_TFLOPS
    fmt = lambda xs: " ".join(f"{x:.3f}" for x in xs)
    med = lambda xs: float(np.median(xs))
    model_a, model_b = mf_c / mf_a, mf_c / mf_b
    worst = max(c / a for a, c in zip(ta, tc))
    log(f"== {which}: N = {N} (2N = {2 * N}), m = {m}, T = {T}, S = {S}; launch (mfma, chunk, n_chunks) = {sw.launch(S)}; "
        f"squarings per interval (unperturbed): mean {sq:.2f}")
    log(f"   (a) wide pullback (grad)         ms per round: {fmt(ta)}   min {min(ta):.3f}  median {med(ta):.3f}")
    log(f"   (b) wide pushforward             ms per round: {fmt(tb)}   min {min(tb):.3f}  median {med(tb):.3f}")
    log(f"   (c) wide Hessian product (tgrad) ms per round: {fmt(tc)}   min {min(tc):.3f}  median {med(tc):.3f}")
    log(f"   MFMA counts per interval: (a) {mf_a:.0f}, (b) {mf_b:.0f}, (c) {mf_c:.0f};  median (c)/(a) = {med(tc) / med(ta):.2f} against {model_a:.2f} by the count "
        f"(measured over model {med(tc) / med(ta) / model_a:.2f});  median (c)/(b) = {med(tc) / med(tb):.2f} against {model_b:.2f} (measured over model {med(tc) / med(tb) / model_b:.2f})")
    log(f"   condition (c) <= {MARGIN} x {model_a:.2f} x (a) in every round: worst round (c)/(a) = {worst:.2f} against {MARGIN * model_a:.2f}: "
        f"{'HOLDS' if worst <= MARGIN * model_a else 'FAILS'}")
    log(f"   MFMA work over the call's time, of {PEAK_F64_MATRIX_TFLOPS} TFLOP/s (f64 matrix, vendor figure): (a) {share(mf_a, med(ta)):.1f} %, "
        f"(b) {share(mf_b, med(tb)):.1f} %, (c) {share(mf_c, med(tc)):.1f} %  (whole calls by device events, not kernel times)")
    log(f"   central difference of two pullbacks (2.0 (a), step 1e-6): max |difference to tgrad| / max |tgrad| = {fd_err:.1e}")
    sw.close()
    return worst <= MARGIN * model_a


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

    log(f"wide sweep Hessian product against the wide pullback and the wide pushforward on the same handle, {torch.cuda.get_device_name(0)}, "
        f"{qc._lib.lib.qc_version().decode()}; device events, {args.rounds} alternating rounds (a), (b), (c) after one warm-up round, one process")
    rng = np.random.default_rng(0)
    ok = True
    for which in args.systems.split(","):
        for S in args.sizes.split(","):
            ok = run_size(qc, which, int(S), args.rounds, rng, log) and ok
    log(f"condition at every size: {'HOLDS' if ok else 'FAILS'}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
