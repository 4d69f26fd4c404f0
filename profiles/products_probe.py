"""Device-resident time per call of the matrix-free Jacobian products, fused and generic, against what a consumer pays today before
it can multiply at all: qc_eval_F_jac_dev with the values requested, on the same handle in the same run.

Timing as in DESIGN.md 7: stream events around n back-to-back launches over a ring of output buffers, warm-up launches first, several
rounds with the paths alternating inside every round, one process on one device.  Paths per shape:

    baseline   qc_eval_F_jac_dev(F, values)          the values of dF -- the least a consumer of dF pays today (not a kernel of this change)
    F_only     qc_eval_F_jac_dev(F, NULL)            the residual-only launch: the launch floor (orientation)
    jvp / vjp  qc_eval_jvp_dev / qc_eval_vjp_dev     on a handle as the plan serves it (a fused kernel where there is one), and as
                                                     jvp_generic / vjp_generic on the same descriptor created under
                                                     QC_NO_PRODUCT_MFMA=1 (the generic path: dF into a scratch + a product kernel)

Shapes: config 3 at T = 1000, config 3 stretched to T = 8000, config 1.  The condition: at config 3, T = 1000, every round of each
product that runs a fused kernel is below every round of the baseline.  `--trace` runs each product a few times for a separate
`rocprofv3 --kernel-trace --stats` run.

    python profiles/products_probe.py [--rounds 5] [--out profiles/products_summary.txt]
"""
import argparse
import ctypes as C
import functools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

WARMUP = 30


def make(qc, cfg, T, generic):
    inp = qc.config_inputs(cfg, T=T) if T else qc.config_inputs(cfg)
    old = os.environ.pop("QC_NO_PRODUCT_MFMA", None)
    if generic:
        os.environ["QC_NO_PRODUCT_MFMA"] = "1"      # read when the handle is created
    try:
        dyn = qc.QuantumDynamics(inp.integrators, inp.traj)
    finally:
        os.environ.pop("QC_NO_PRODUCT_MFMA", None)
        if old is not None:
            os.environ["QC_NO_PRODUCT_MFMA"] = old
    return inp, dyn


def time_us(calls, n, stream):
    """us per launch of n launches cycling through `calls` (a ring: one bound call per output buffer)."""
    nb = len(calls)
    for i in range(WARMUP):
        calls[i % nb]()
    stream.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for i in range(n):
        rc = calls[i % nb]()
        if rc:
            raise RuntimeError(f"launch failed with status {rc}")
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def run_shape(qc, cfg, T, rounds, log):
    L = qc._lib
    inp, fused = make(qc, cfg, T, False)
    _, generic = make(qc, cfg, T, True)
    d = fused.dims
    rng = np.random.default_rng(0)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    st = C.c_void_p(stream.cuda_stream)
    f64 = dict(dtype=torch.float64, device=dev)
    Z = torch.from_numpy(inp.traj.datavec + 1e-2 * rng.standard_normal(int(d.Z_len))).to(dev)
    v, lam = torch.from_numpy(rng.standard_normal(int(d.Z_len))).to(dev), torch.from_numpy(rng.standard_normal(int(d.F_len))).to(dev)
    nJ = max(2, min(16, (640 << 20) // (8 * int(d.jac_nnz))))          # ring of value vectors: 640 MB, at least two
    Jb = [torch.empty(int(d.jac_nnz), **f64) for _ in range(nJ)]
    Fb = [torch.empty(int(d.F_len), **f64) for _ in range(16)]
    Wb = [torch.empty(int(d.Z_len), **f64) for _ in range(16)]
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    paths = {
        "baseline_F_dF": [functools.partial(L.lib.qc_eval_F_jac_dev, fused._h, p(Z), p(Fb[i % 16]), p(Jb[i]), st) for i in range(nJ)],
        "F_only": [functools.partial(L.lib.qc_eval_F_jac_dev, fused._h, p(Z), p(Fb[i]), None, st) for i in range(16)],
        "jvp": [functools.partial(L.lib.qc_eval_jvp_dev, fused._h, p(Z), p(v), p(Fb[i]), st) for i in range(16)],
        "vjp": [functools.partial(L.lib.qc_eval_vjp_dev, fused._h, p(Z), p(lam), p(Wb[i]), st) for i in range(16)],
        "jvp_generic": [functools.partial(L.lib.qc_eval_jvp_dev, generic._h, p(Z), p(v), p(Fb[i]), st) for i in range(16)],
        "vjp_generic": [functools.partial(L.lib.qc_eval_vjp_dev, generic._h, p(Z), p(lam), p(Wb[i]), st) for i in range(16)],
    }
    # the two paths compute the same products (the tests check both against the oracle; here: against each other at this size)
    y = [torch.empty(int(d.F_len), **f64) for _ in range(2)]
    w = [torch.empty(int(d.Z_len), **f64) for _ in range(2)]
    for k, dyn in enumerate((fused, generic)):
        dyn.dF_times_device(Z, v, y[k])
        dyn.dFT_times_device(Z, lam, w[k])
    torch.cuda.synchronize()
    ey = float((y[0] - y[1]).abs().max() / y[1].abs().max())
    ew = float((w[0] - w[1]).abs().max() / w[1].abs().max())
    n = 200 if int(d.jac_nnz) < (8 << 20) else 50
    res = {k: [] for k in paths}
    for _ in range(rounds):
        for k, calls in paths.items():
            res[k].append(time_us(calls, n, stream))
    names_f, names_g = fused.product_kernel_names, generic.product_kernel_names
    log(f"== config {cfg}, T = {inp.traj.T}: F_len {int(d.F_len)}, Z_len {int(d.Z_len)}, jac_nnz {int(d.jac_nnz)} ({8 * int(d.jac_nnz) / 1e6:.1f} MB); "
        f"F + dF on {fused.kernel_names[0]}; products on {names_f[0]} / {names_f[1]} and {names_g[0]} / {names_g[1]}")
    log(f"   us per call, {rounds} rounds of {n} launches after {WARMUP} warm-up launches each, ring of {nJ} value vectors / 16 result vectors")
    for k, xs in res.items():
        log(f"   {k:14s} {' '.join(f'{x:8.2f}' for x in xs)}   median {np.median(xs):8.2f}")
    log(f"   planned against generic handle, same inputs: max |dy| / max |y| = {ey:.2e}, max |dw| / max |w| = {ew:.2e}")
    on_mfma = [k for k, nm in zip(("jvp", "vjp"), names_f) if nm.startswith("mfma")]      # the products that run a fused kernel on this handle
    won = all(max(res[k]) < min(res["baseline_F_dF"]) for k in on_mfma)
    log(f"   fused kernels on this handle: {', '.join(on_mfma) if on_mfma else 'none'}; every round of each of them below every round of the baseline: "
        f"{won if on_mfma else 'n/a'}; baseline / jvp = {np.median(res['baseline_F_dF']) / np.median(res['jvp']):.2f}, "
        f"baseline / vjp = {np.median(res['baseline_F_dF']) / np.median(res['vjp']):.2f} (medians)")
    fused.close()
    generic.close()
    return won


def trace_only(qc, reps=5):
    """config 3, T = 1000: each product `reps` times, fused then generic, for a kernel trace (a run of its own)."""
    for generic in (False, True):
        inp, dyn = make(qc, 3, 1000, generic)
        d = dyn.dims
        Z = torch.from_numpy(inp.traj.datavec).cuda()
        v, lam = torch.ones(int(d.Z_len), dtype=torch.float64, device="cuda"), torch.ones(int(d.F_len), dtype=torch.float64, device="cuda")
        y, w = torch.empty_like(lam), torch.empty_like(v)
        for _ in range(reps):
            dyn.dF_times_device(Z, v, y)
            dyn.dFT_times_device(Z, lam, w)
        torch.cuda.synchronize()
        dyn.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--shapes", default="3:1000,3:8000,1:0")
    args = ap.parse_args()
    qc = g.load_package()
    if args.trace:
        trace_only(qc)
        return 0
    lines = []

    def log(sx):
        print(sx, flush=True)
        lines.append(sx)

    log(f"Jacobian products against the F + dF launch, {torch.cuda.get_device_name(0)}, {qc._lib.lib.qc_version().decode()}; device events")
    ok = True
    for spec in args.shapes.split(","):
        cfg, T = (int(x) for x in spec.split(":"))
        won = run_shape(qc, cfg, T, args.rounds, log)
        if cfg == 3 and T == 1000:
            ok = won
    log(f"condition (config 3, T = 1000: every round of each product on a fused kernel below every round of the baseline launch): {'met' if ok else 'NOT met'}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
