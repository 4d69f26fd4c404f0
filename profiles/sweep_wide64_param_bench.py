#!/usr/bin/env python3
"""The parameter flavour of the "mfma64-sweep" walk (csrc/qc_sweep64_grad.hip, qc_sweep64_grad_kernel<true>) against the gradient call,
against central differences, and the gradient call against a build of the parent commit.

Systems: those of profiles/sweep_wide64_grad_bench.py with perturbations to search over, T = 100, each at S in {64, 1024}, on handles made
with wide = QC_SWEEP_WIDE | QC_SWEEP_WIDE_64 | QC_SWEEP_WIDE_64_GRAD | QC_SWEEP_WIDE_64_PARAMS:

    5 qubits (N = 32, m = 10 drives, p = 2 detunings), the full unitary (32 state columns):
        (p) qc_sweep_grad_params_dev (fids, grad, grad_theta, grad_scale)        (g) qc_sweep_grad_dev (fids, grad)        (e) qc_sweep_eval_dev (fids)
    three transmons (N = 27, m = 6 drives, p = 3 detunings, one per transmon), the eight computational columns (no fidelity is defined on
    8 of 27 columns, so the derivative call is the pullback):
        (p) qc_sweep_vjp_dev (grad, grad_theta, grad_scale)                      (g) qc_sweep_vjp_dev (grad)               (e) qc_sweep_eval_dev (finals)

(a) (p) / (g) on the same handle: (g) launches the flavour <false>, which is the parent commit's kernel instruction for instruction; the
    model is 1 plus p image contractions out of L2 per interval (not one MFMA is added).
(b) (p) against 2 (p + m) forward sweeps (e), what central differences in theta and c cost without the flavour.
(c) with --parent-lib FILE (libqcolloc_hip.so of the parent commit): (g) of that build, through its C ABI on a handle made from the same
    descriptor without the new bit, against (g) of this one -- the flavour <false> did not move.

Device events on one stream, the legs alternating over the rounds after one warm-up round, one process.

    python profiles/sweep_wide64_param_bench.py [--rounds 5] [--parent-lib FILE] [--out FILE]      (section 2 of profiles/sweep_wide64_param_summary.txt)
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
from sweep_probe import event_ms  # noqa: E402
from sweep_wide64_bench import make_problem  # noqa: E402


class ParentBuild:
    """qc_sweep_create / qc_sweep_grad_dev / qc_sweep_vjp_dev / qc_sweep_destroy of another build of the library, by its C ABI."""

    def __init__(self, path):
        self.lib = C.CDLL(path, mode=C.RTLD_LOCAL)
        P, I = C.c_void_p, C.c_int64
        self.lib.qc_sweep_create.argtypes, self.lib.qc_sweep_create.restype = [P, C.POINTER(P)], C.c_int
        self.lib.qc_sweep_destroy.argtypes, self.lib.qc_sweep_destroy.restype = [P], None
        self.lib.qc_sweep_grad_dev.argtypes, self.lib.qc_sweep_grad_dev.restype = [P, P, P, I] + [P] * 8, C.c_int
        self.lib.qc_sweep_vjp_dev.argtypes, self.lib.qc_sweep_vjp_dev.restype = [P, P, P, I] + [P] * 10, C.c_int
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
    flags = dict(wide=True, wide64=True, wide64_grad=True, wide64_params=True)
    if which == "qubits5":
        cols = N
        perts = [pb["P"], np.kron(np.eye(2), np.kron(qc.GATES["Z"], np.eye(N // 4))).astype(complex)]      # detunings of the first two qubits
        sw = qc.RolloutSweep(pb["system"], perts, T, goal=pb["goal"], fid_kind="unitary", **flags)
        init = qc.operator_to_iso_vec(np.eye(N, dtype=complex))
        width = 0.05
    else:
        import three_transmon_robustness as tr
        from three_transmon_worst_case import number_operators
        cols = len(tr.SUBSPACE)
        perts = number_operators()
        sw = qc.RolloutSweep(pb["system"], perts, T, cols=cols, **flags)
        E = np.zeros((2 * N, cols))
        E[tr.SUBSPACE, np.arange(cols)] = 1.0
        init = E.reshape(-1, order="F")
        width = 2 * np.pi * 0.002
    p = len(perts)
    assert sw.kernel_name == "mfma64-sweep" and sw.vjp_supported and sw.wide64_params
    theta = rng.uniform(-width, width, (S, p))
    dZ, dinit, dth, dsc = t(sw.pack(pb["controls"], pb["dts"])), t(init), t(theta), t(pb["scale"])
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    dgrad, dgrad2, dgrad3, dgth, dgsc = new(sw.Z_len), new(sw.Z_len), new(sw.Z_len), new(S, p), new(S, m)
    stream = torch.cuda.Stream(device=dev)
    ptr = lambda x: None if x is None else x.data_ptr()
    hp = None
    if which == "qubits5":
        dfid, dfid2, dfid3, dfid4 = (new(S) for _ in range(4))
        fp = lambda: sw.param_grad_device(dZ, dinit, S, dth, dsc, None, dfid, None, dgrad, None, dgth, dgsc, stream=stream)
        fg = lambda: sw.grad_device(dZ, dinit, S, dth, dsc, None, dfid2, None, dgrad2, None, stream=stream)
        fe = lambda: sw.eval_device(dZ, dinit, dth, dsc, None, dfid3, stream=stream)
        what = "(p) qc_sweep_grad_params_dev (fids, grad, grad_theta, grad_scale), (g) qc_sweep_grad_dev (fids, grad), (e) qc_sweep_eval_dev (fids)"
        if parent is not None:
            hp = parent.create(sw._desc, sw._desc.wide & ~qc._lib.QC_SWEEP_WIDE_64_PARAMS)
            f0 = lambda: parent.lib.qc_sweep_grad_dev(hp, ptr(dZ), ptr(dinit), S, ptr(dth), ptr(dsc), None, ptr(dfid4), None, ptr(dgrad3), None,
                                                      stream.cuda_stream)
    else:
        dcot = t(np.random.default_rng(1).standard_normal((S, sw.ns)))
        dfin = new(S, sw.ns)
        fp = lambda: sw.vjp_device(dZ, dinit, S, dcot, dth, dsc, dgrad=dgrad, dgrad_theta=dgth, dgrad_scale=dgsc, stream=stream)
        fg = lambda: sw.vjp_device(dZ, dinit, S, dcot, dth, dsc, dgrad=dgrad2, stream=stream)
        fe = lambda: sw.eval_device(dZ, dinit, dth, dsc, dfin, None, stream=stream)
        what = "(p) qc_sweep_vjp_dev (grad, grad_theta, grad_scale), (g) qc_sweep_vjp_dev (grad), (e) qc_sweep_eval_dev (finals)"
        if parent is not None:
            hp = parent.create(sw._desc, sw._desc.wide & ~qc._lib.QC_SWEEP_WIDE_64_PARAMS)
            f0 = lambda: parent.lib.qc_sweep_vjp_dev(hp, ptr(dZ), ptr(dinit), S, ptr(dth), ptr(dsc), ptr(dcot), None, ptr(dgrad3), None, None, None,
                                                     None, stream.cuda_stream)
    legs = [("p", fp), ("g", fg), ("e", fe)] + ([("0", f0)] if hp is not None else [])
    times = {k: [] for k, _ in legs}
    with torch.cuda.stream(stream):
        for _, f in legs:
            rc = f()
            assert rc in (None, 0), rc
        stream.synchronize()
        for _ in range(rounds):
            for k, f in legs:
                times[k].append(event_ms(f, stream))
    assert torch.equal(dgrad, dgrad2)          # the parameter call's gradient carries the bits of the gradient call
    if hp is not None:
        assert torch.equal(dgrad3, dgrad2)     # and both carry the parent build's
        parent.lib.qc_sweep_destroy(hp)
    if which == "qubits5":
        assert torch.equal(dfid, dfid2) and torch.equal(dfid, dfid3)
    assert torch.isfinite(dgth).all() and torch.isfinite(dgsc).all() and dgth.abs().max().item() > 0 and dgsc.abs().max().item() > 0
    med = {k: float(np.median(v)) for k, v in times.items()}
    fmt = lambda xs: " ".join(f"{x:.3f}" for x in xs)
    spread = (max(times["g"]) - min(times["g"])) / med["g"]
    log(f"== {which}: N = {N} (2N = {2 * N}), m = {m}, p = {p}, {cols} state columns, T = {T}, S = {S}; launch (mfma, chunk, n_chunks) = {sw.launch(S)}; {what}")
    log(f"   (p) parameter call   ms per round: {fmt(times['p'])}   min {min(times['p']):.3f}  median {med['p']:.3f}")
    log(f"   (g) gradient call    ms per round: {fmt(times['g'])}   min {min(times['g']):.3f}  median {med['g']:.3f}   (max - min) / median = {spread:.4f}")
    log(f"   (e) forward sweep    ms per round: {fmt(times['e'])}   min {min(times['e']):.3f}  median {med['e']:.3f}")
    log(f"   (a) median (p) / median (g) = {med['p'] / med['g']:.4f}   (min / min = {min(times['p']) / min(times['g']):.4f}); "
        f"{p} more image contractions per interval beside the {m} it does already, no MFMA added")
    cd = 2 * (p + m) * med["e"]
    log(f"   (b) central differences: 2 (p + m) = {2 * (p + m)} forward sweeps = {cd:.3f} ms; (p) is {cd / med['p']:.2f} times faster "
        f"({med['p'] / med['e']:.2f} forward sweeps)")
    if hp is not None:
        log(f"   (0) parent's gradient ms per round: {fmt(times['0'])}   min {min(times['0']):.3f}  median {med['0']:.3f}")
        log(f"   (c) median (g) / median (0) = {med['g'] / med['0']:.4f}   (min / min = {min(times['g']) / min(times['0']):.4f}); outputs bit-identical")
    sw.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--sizes", default="64,1024")
    ap.add_argument("--systems", default="qubits5,transmons3")
    ap.add_argument("--parent-lib", default=None, help="libqcolloc_hip.so built from the parent commit, for (c)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sweep_wide64_param_bench.py measures on a GPU; none is visible")
    qc = g.load_package()
    parent = ParentBuild(args.parent_lib) if args.parent_lib else None
    lines = []

    def log(sx):
        print(sx, flush=True)
        lines.append(sx)

    log(f"mfma64-sweep parameter calls, {torch.cuda.get_device_name(0)}, {qc._lib.lib.qc_version().decode()}; device events, {args.rounds} alternating "
        f"rounds (p), (g), (e){', (0)' if parent else ''} after one warm-up round, one process"
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
