#!/usr/bin/env python3
"""Trajectory-terms pass with the extension terms (qc_terms_create_ext) at config 3: kernel time per evaluation (L + gradient +
Hessian on device buffers, the two launches), the bytes the pass must move and the resulting share of HBM.

Cases: config 3 at T = 1000 and 8000 with the a / da / dda regularisers alone and with a smoothness term on dda and an 8-entry
slack cost added (four Ũ⃗ entries given L1 slacks: the knots widen by 8); a two-member direct sum of config-3 systems with the
regularisers and pairwise terms between the members' Ũ⃗ (128 pairs a knot).

    python profiles/terms_ext_probe.py [--parent LIB] [--reps N]

--parent LIB: a shared library built from the parent commit's qc_terms.hip alone.  Its regulariser-only evaluation of the same
descriptor then alternates with this build's, 20 rounds of N calls each, in the same process: the A/B of the unchanged pass.
Run it once plainly (event timing, printed) and once under `rocprofv3 --kernel-trace --stats` for the per-kernel times."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402

HBM_BPS = 8.0e12          # MI355X peak HBM bandwidth


def timed(fn, reps):
    """Median per-call time (us) of `reps` back-to-back calls, 5 repeats."""
    out = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    return float(np.median(out))


def device_eval(obj):
    Z = torch.from_numpy(obj.traj.datavec.copy()).cuda()
    J = torch.zeros(1, dtype=torch.float64, device="cuda")
    gr = torch.zeros(obj.Z_len, dtype=torch.float64, device="cuda")
    H = torch.zeros(max(obj.hess_nnz, 1), dtype=torch.float64, device="cuda")
    return lambda: obj.eval_device(Z, J, gr, H)


def moved_bytes(obj):
    """Z read once, gradient and Hessian values written, per-knot partials written and read back."""
    T = obj.traj.T
    return 8 * (obj.Z_len + obj.Z_len + obj.hess_nnz + 2 * T)


def report(name, obj, us):
    b = moved_bytes(obj)
    row = dict(case=name, T=obj.traj.T, zdim=obj.traj.dim, hess_nnz=obj.hess_nnz, us=round(us, 2), MB=round(b / 1e6, 3),
               hbm_share=round(b / (us * 1e-6) / HBM_BPS, 4))
    print(json.dumps(row))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    qc = g.load_package()
    rows = []
    for T in (1000, 8000):
        inp = qc.config_inputs(3, T=T)
        traj = inp.traj
        regs = lambda tr: (qc.QuadraticRegularizer("a", tr, 1e-2) + qc.QuadraticRegularizer("da", tr, 1e-2)
                           + qc.QuadraticRegularizer("dda", tr, 1e-2))
        plain = qc.TrajectoryObjective(regs(traj), traj)
        rows.append(report(f"c3 regularisers", plain, timed(device_eval(plain), args.reps)))
        wide = qc.add_l1_slacks(inp, "Ũ⃗", [8, 9, 10, 11])
        tw = wide.traj
        plain_w = qc.TrajectoryObjective(regs(tw), tw)
        ext = qc.TrajectoryObjective(regs(tw) + qc.QuadraticSmoothnessRegularizer("dda", tw, 10.0) + qc.L1Regularizer("Ũ⃗", tw, 0.1), tw)
        rows.append(report("c3 + 8 slacks, regularisers", plain_w, timed(device_eval(plain_w), args.reps)))
        rows.append(report("c3 + 8 slacks, regularisers + smoothness(dda) + slack cost", ext, timed(device_eval(ext), args.reps)))
        if T == 1000:
            ds = qc.unitary_direct_sum_inputs([inp, qc.config_inputs(3, T=T, seed=7)])
            td = ds.traj
            pair = qc.TrajectoryObjective([qc.PairwiseQuadraticRegularizer(td, 100.0, [("Ũ⃗1", "Ũ⃗2")])]
                                          + [qc.QuadraticRegularizer(n + l, td, 1e-2) for l in "12" for n in ("a", "da", "dda")], td)
            rows.append(report("direct sum of two c3, regularisers + 128 pairs", pair, timed(device_eval(pair), args.reps)))
        if args.parent and T == 1000:
            lib = C.CDLL(os.path.abspath(args.parent), mode=C.RTLD_LOCAL)
            lib.qc_terms_create.argtypes = [C.POINTER(qc._lib.qc_terms_desc), C.POINTER(C.c_void_p)]
            lib.qc_terms_eval_dev.argtypes = [C.c_void_p] * 6
            lib.qc_terms_destroy.argtypes = [C.c_void_p]
            h = C.c_void_p()
            assert lib.qc_terms_create(C.byref(plain._desc), C.byref(h)) == 0
            Z = torch.from_numpy(traj.datavec.copy()).cuda()
            bufs = [torch.zeros(n, dtype=torch.float64, device="cuda") for n in (1, plain.Z_len, plain.hess_nnz)]
            s = torch.cuda.current_stream().cuda_stream
            ptrs = [Z.data_ptr()] + [b.data_ptr() for b in bufs] + [s]
            par = lambda: lib.qc_terms_eval_dev(h, *ptrs)
            new = lambda: qc._lib.lib.qc_terms_eval_dev(plain._h, *ptrs)         # the same call through this build
            par()
            torch.cuda.synchronize()
            ref_vals = [b.cpu().numpy().copy() for b in bufs]
            new_bufs = plain.L_grad_hess(traj.datavec)
            same = all(np.asarray(a).ravel().tobytes() == np.asarray(b).ravel().tobytes() for a, b in zip(ref_vals, new_bufs))
            A, B = [], []
            for _ in range(20):
                A.append(timed(par, args.reps))
                B.append(timed(new, args.reps))
            ab = dict(case="A/B c3 T=1000 regularisers", parent_us=round(float(np.median(A)), 3), this_us=round(float(np.median(B)), 3),
                      parent_spread=[round(min(A), 3), round(max(A), 3)], this_spread=[round(min(B), 3), round(max(B), 3)],
                      bit_identical=bool(same))
            print(json.dumps(ab))
            rows.append(ab)
            lib.qc_terms_destroy(h)
    out = os.environ.get("TERMS_EXT_OUT")
    if out:
        with open(out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
