"""Device-resident time per call of the matrix-free Hessian product (mu d2F) v against the launch whose values it makes unnecessary:
qc_eval_hess_dev on the same handle in the same run (a kernel this change does not touch: the parent commit's launch).

Timing as in DESIGN.md 7 and profiles/headline_path.txt: stream events around K back-to-back launches over a ring of output buffers,
warm-up launches first, several rounds with the paths alternating inside every round, one process on one device.  Paths per shape:

    mu_d2F        qc_eval_hess_dev(values)     the values of mu d2F -- what a consumer pays today before it can multiply at all
    hvp           qc_eval_hvp_dev              on a handle as the plan serves it
    hvp_generic   qc_eval_hvp_dev              on the same descriptor created under QC_NO_PRODUCT_MFMA=1

The rule for a fused kernel: at config 3, T = 1000, K = 2000, every round of hvp on a fused kernel is below every round of mu_d2F.

    python profiles/hess_products_probe.py [--rounds 5] [--steps 2000] [--out profiles/hess_products_summary.txt]
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
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import __graft_entry__ as g  # noqa: E402
from products_probe import make, time_us  # noqa: E402


def run_shape(qc, cfg, T, rounds, steps, log):
    L = qc._lib
    inp, planned = make(qc, cfg, T, False)
    _, generic = make(qc, cfg, T, True)
    d = planned.dims
    rng = np.random.default_rng(0)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    st = C.c_void_p(stream.cuda_stream)
    f64 = dict(dtype=torch.float64, device=dev)
    Z = torch.from_numpy(inp.traj.datavec + 1e-2 * rng.standard_normal(int(d.Z_len))).to(dev)
    v, mu = torch.from_numpy(rng.standard_normal(int(d.Z_len))).to(dev), torch.from_numpy(rng.standard_normal(int(d.n_rows))).to(dev)
    nH = max(2, min(16, (640 << 20) // (8 * int(d.hess_nnz))))          # ring of value vectors: 640 MB, at least two
    Hb = [torch.empty(int(d.hess_nnz), **f64) for _ in range(nH)]
    Wb = [torch.empty(int(d.Z_len), **f64) for _ in range(16)]
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    paths = {
        "mu_d2F": [functools.partial(L.lib.qc_eval_hess_dev, planned._h, p(Z), p(mu), p(Hb[i]), st) for i in range(nH)],
        "hvp": [functools.partial(L.lib.qc_eval_hvp_dev, planned._h, p(Z), p(mu), p(v), p(Wb[i]), st) for i in range(16)],
        "hvp_generic": [functools.partial(L.lib.qc_eval_hvp_dev, generic._h, p(Z), p(mu), p(v), p(Wb[i]), st) for i in range(16)],
    }
    w = [torch.empty(int(d.Z_len), **f64) for _ in range(2)]
    for k, dyn in enumerate((planned, generic)):      # (the first call of a handle builds its table and scratch)
        dyn.mu_d2F_times_device(Z, mu, v, w[k])
    torch.cuda.synchronize()
    ew = float((w[0] - w[1]).abs().max() / w[1].abs().max())
    n = steps if int(d.hess_nnz) < (8 << 20) else max(50, steps // 10)
    res = {k: [] for k in paths}
    for _ in range(rounds):
        for k, calls in paths.items():
            res[k].append(time_us(calls, n, stream))
    names = planned.hess_product_kernel_name, generic.hess_product_kernel_name
    log(f"== config {cfg}, T = {inp.traj.T}: Z_len {int(d.Z_len)} ({8 * int(d.Z_len) / 1e6:.2f} MB), hess_nnz {int(d.hess_nnz)} ({8 * int(d.hess_nnz) / 1e6:.1f} MB); "
        f"mu_d2F on {planned.kernel_names[1]}; products on {names[0]} and {names[1]}")
    log(f"   us per call, {rounds} rounds of {n} launches after 30 warm-up launches each, ring of {nH} value vectors / 16 result vectors")
    for k, xs in res.items():
        log(f"   {k:14s} {' '.join(f'{x:8.2f}' for x in xs)}   median {np.median(xs):8.2f}")
    log(f"   planned against generic handle, same inputs: max |dw| / max |w| = {ew:.2e}")
    fused = names[0].startswith("mfma")
    won = fused and max(res["hvp"]) < min(res["mu_d2F"])
    log(f"   fused kernel on this handle: {names[0] if fused else 'none'}; every round of hvp below every round of mu_d2F: {won if fused else 'n/a'}; "
        f"hvp / mu_d2F = {np.median(res['hvp']) / np.median(res['mu_d2F']):.2f} (medians)")
    planned.close()
    generic.close()
    return fused, won


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="3:1000,3:8000,1:0")
    args = ap.parse_args()
    qc = g.load_package()
    lines = []

    def log(sx):
        print(sx, flush=True)
        lines.append(sx)

    log(f"Hessian product against the mu_d2F launch, {torch.cuda.get_device_name(0)}, {qc._lib.lib.qc_version().decode()}; device events")
    verdict = "no fused kernel in the library: n/a"
    for spec in args.shapes.split(","):
        cfg, T = (int(x) for x in spec.split(":"))
        fused, won = run_shape(qc, cfg, T, args.rounds, args.steps, log)
        if cfg == 3 and T == 1000 and fused:
            verdict = "met" if won else "NOT met"
    log(f"rule (config 3, T = 1000: every round of hvp on a fused kernel below every round of the mu_d2F launch): {verdict}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
