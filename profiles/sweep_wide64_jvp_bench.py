#!/usr/bin/env python3
"""The pushforward of the "mfma64-sweep" form (csrc/qc_sweep64_jvp.hip, qc_sweep64_jvp_finish_kernel) against the forward sweep of the same
handle, and that forward sweep against a build of the parent commit.

Systems: those of profiles/sweep_wide64_bench.py with the full unitary as the state (5 qubits: N = 32, 10 drives, 32 columns, ns = 2048;
three transmons: N = 27, 6 drives, 27 columns), T = 100, each at S in {64, 1024}, on handles made with
wide = QC_SWEEP_WIDE | QC_SWEEP_WIDE_64 | QC_SWEEP_WIDE_64_TANGENT:

    (j) qc_sweep_jvp_dev (finals, tfinals) along a direction of the controls and timesteps
    (e) qc_sweep_eval_dev (finals) on the same handle
    (0) with --parent-lib FILE (libqcolloc_hip.so of the parent commit): qc_sweep_eval_dev of that build, through its C ABI, on a handle made
        from the same descriptor without bit 14

timed by device events on one stream, the legs alternating over the rounds after one warm-up round, one process.  The model is the MFMA
count of the kernels as built, per interval and workgroup:

    forward       (9 + sq) x 256
    pushforward   (27 + 3 sq) x 256          (j) / (e) by the count: 3.0

with the sq every sample takes in every interval (recomputed on the host).  The share of the f64 matrix peak is that MFMA work over the
call's time: an end-to-end figure (totals and finish launches), not a kernel's.  The last figure is the distance of (j)'s tfinals from
a central difference of two forward sweeps at step 1e-6, as a share of the largest tangent.

    python profiles/sweep_wide64_jvp_bench.py [--rounds 5] [--parent-lib FILE] [--out FILE]      (profiles/sweep_wide64_jvp_summary.txt)
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
import __graft_entry__ as g  # noqa: E402
from sweep_probe import PEAK_F64_MATRIX_TFLOPS, event_ms  # noqa: E402
from sweep_wide64_bench import make_problem, mean_squarings  # noqa: E402

COUNT = 3.0
TARGET = 1.11          # the margin DESIGN 5.8.12 set for its walk against its own count


class ParentBuild:
    """qc_sweep_create / qc_sweep_eval_dev / qc_sweep_destroy of another build of the library, by its C ABI."""

    def __init__(self, path):
        self.lib = C.CDLL(path, mode=C.RTLD_LOCAL)
        P, I = C.c_void_p, C.c_int64
        self.lib.qc_sweep_create.argtypes, self.lib.qc_sweep_create.restype = [P, C.POINTER(P)], C.c_int
        self.lib.qc_sweep_destroy.argtypes, self.lib.qc_sweep_destroy.restype = [P], None
        self.lib.qc_sweep_eval_dev.argtypes, self.lib.qc_sweep_eval_dev.restype = [P, P, P, I] + [P] * 5, C.c_int
        self.lib.qc_version.restype = C.c_char_p

    def create(self, desc, wide):
        d = type(desc).from_buffer_copy(desc)          # the caller's arrays stay alive with the handle the descriptor came from
        d.wide = wide
        h = C.c_void_p()
        rc = self.lib.qc_sweep_create(C.byref(d), C.byref(h))
        assert rc == 0, f"qc_sweep_create of the parent build: {rc}"
        return h


def run_size(qc, which, S, T, rounds, rng, parent, log):
    pb = make_problem(qc, which, S, T, rng)
    N, m = pb["N"], pb["m"]
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    ptr = lambda x: None if x is None else x.data_ptr()
    sw = qc.RolloutSweep(pb["system"], [pb["P"]], T, wide=True, wide64=True, wide64_tangent=True)
    assert sw.kernel_name == "mfma64-sweep" and sw.jvp_supported and sw.cols == N
    init = qc.operator_to_iso_vec(np.eye(N, dtype=complex))
    Z = sw.pack(pb["controls"], pb["dts"])
    vrng = np.random.default_rng(1)
    vZ = sw.pack(vrng.standard_normal(np.shape(pb["controls"])), 0.1 * np.asarray(pb["dts"]) * vrng.standard_normal(np.shape(pb["dts"])))
    dZ, dvZ, dinit, dth, dsc = t(Z), t(vZ), t(init), t(pb["theta"]), t(pb["scale"])
    dfin, dtfin, dfin2, dfin3 = (torch.empty((S, sw.ns), dtype=torch.float64, device=dev) for _ in range(4))
    stream = torch.cuda.Stream(device=dev)
    legs = {"j": lambda: sw.jvp_device(dZ, dinit, S, dth, dsc, dvZ=dvZ, dfinals=dfin, dtfinals=dtfin, stream=stream),
            "e": lambda: sw.eval_device(dZ, dinit, dth, dsc, dfin2, None, stream=stream)}
    hp = None
    if parent is not None:
        hp = parent.create(sw._desc, sw._desc.wide & ~qc._lib.QC_SWEEP_WIDE_64_TANGENT)
        legs["0"] = lambda: parent.lib.qc_sweep_eval_dev(hp, ptr(dZ), ptr(dinit), S, ptr(dth), ptr(dsc), ptr(dfin3), None, stream.cuda_stream)
    times = {k: [] for k in legs}
    with torch.cuda.stream(stream):
        for f in legs.values():
            f()
        stream.synchronize()
        for _ in range(rounds):
            for k, f in legs.items():
                times[k].append(event_ms(f, stream))
        stream.synchronize()
        assert torch.equal(dfin, dfin2)              # the final states of the pushforward carry the bits of the forward sweep
        if parent is not None:
            assert torch.equal(dfin3, dfin2)         # and both carry the parent build's
            parent.lib.qc_sweep_destroy(hp)
        # a central difference of two forward sweeps at step 1e-6
        step = 1e-6
        up, down = torch.empty_like(dfin), torch.empty_like(dfin)
        sw.eval_device(dZ + step * dvZ, dinit, dth, dsc, up, None, stream=stream)
        sw.eval_device(dZ - step * dvZ, dinit, dth, dsc, down, None, stream=stream)
        stream.synchronize()
        cd = float(((up - down) / (2 * step) - dtfin).abs().max() / dtfin.abs().max())
    med = {k: float(np.median(v)) for k, v in times.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
    sq = mean_squarings(qc, pb)
    fwd, push = (9 + sq) * 256, (27 + 3 * sq) * 256
    ratio = med["j"] / med["e"]
    flops = S * (T - 1) * push * 2 * 16 * 16 * 4
    rate = flops / (med["j"] * 1e-3) / 1e12
    fmt = lambda xs: " ".join(f"{x:.3f}" for x in xs)
    log(f"== {which}: N = {N} (2N = {2 * N}), m = {m}, {sw.cols} state columns (ns = {sw.ns}), T = {T}, S = {S}; launch (mfma, chunk, n_chunks) = {sw.launch(S)}; "
        f"squarings per interval, mean: {sq:.3f}")
    log(f"   (j) pushforward      ms per round: {fmt(times['j'])}   min {min(times['j']):.3f}  median {med['j']:.3f}  spread {100 * spread['j']:.2f} %")
    log(f"   (e) forward sweep    ms per round: {fmt(times['e'])}   min {min(times['e']):.3f}  median {med['e']:.3f}  spread {100 * spread['e']:.2f} %")
    log(f"   median (j) / median (e) = {ratio:.3f}; count {push:.0f} / {fwd:.0f} = {push / fwd:.2f}; measured / count = {ratio / COUNT:.3f} "
        f"(target at S = 1024: <= {TARGET}: {'met' if ratio / COUNT <= TARGET else 'MISSED'})")
    if parent is not None:
        log(f"   (0) parent's forward ms per round: {fmt(times['0'])}   min {min(times['0']):.3f}  median {med['0']:.3f}  spread {100 * spread['0']:.2f} %")
        inside = abs(med["e"] / med["0"] - 1.0) <= max(spread["e"], spread["0"])
        log(f"   median (e) / median (0) = {med['e'] / med['0']:.4f}, minima {min(times['e']) / min(times['0']):.4f} "
            f"({'inside' if inside else 'OUTSIDE'} the legs' spread); final states bit-identical")
    log(f"   MFMA work {push:.0f} instructions per interval, {flops / 1e9:.1f} GFLOP per call, over the call's time: {rate:.2f} TFLOP/s = "
        f"{100 * rate / PEAK_F64_MATRIX_TFLOPS:.1f} % of {PEAK_F64_MATRIX_TFLOPS} TFLOP/s (f64 matrix, vendor figure; whole call by device events)")
    log(f"   central difference of two forward sweeps at step 1e-6: {cd:.2e} of the largest tangent away from tfinals")
    sw.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--sizes", default="64,1024")
    ap.add_argument("--systems", default="qubits5,transmons3")
    ap.add_argument("--parent-lib", default=None, help="libqcolloc_hip.so built from the parent commit, for (0)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sweep_wide64_jvp_bench.py measures on a GPU; none is visible")
    qc = g.load_package()
    parent = ParentBuild(args.parent_lib) if args.parent_lib else None
    lines = []

    def log(sx):
        print(sx, flush=True)
        lines.append(sx)

    log(f"mfma64-sweep pushforward against the forward sweep of the same handle, {torch.cuda.get_device_name(0)}, {qc._lib.lib.qc_version().decode()}; "
        f"device events, {args.rounds} alternating rounds (j), (e){', (0)' if parent else ''} after one warm-up round, one process"
        + (f"; (0): the parent commit's build, {parent.lib.qc_version().decode()}" if parent else ""))
    rng = np.random.default_rng(0)
    for which in args.systems.split(","):
        for S in args.sizes.split(","):
            run_size(qc, which, int(S), args.T, args.rounds, rng, parent, log)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
