#!/usr/bin/env python3
"""UnitaryRobustnessObjective on the device (qc_robust_eval_dev): device time per call, launches per call and bytes moved against
8 TB/s, at four sizes:

  l_grad_c3     L + grad at config 3's trajectory (T = 1000, N = n = 8, H = ZII)
  l_grad_c4     the same at T = 8000
  hess_459      L + grad + exact Hessian at the reference test's size (N = 3, n = 2, T = 51, free dt: V = 459)
  hess_cap      the same near the cap (T = 1500: V = 13 500, 91 M values, 729 MB)

Run under `rocprofv3 --kernel-trace --stats -- python profiles/robust_probe.py` for the per-kernel split; the times printed here
are CUDA-event times of `reps` back-to-back calls on one stream, divided by `reps`.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402

HBM = 8e12


def synthetic_traj(qc, T, N, free=True, seed=0):
    rng = np.random.default_rng(seed)
    comps = {"Ũ⃗": rng.standard_normal((2 * N * N, T)) / np.sqrt(N), "a": rng.standard_normal((2, T))}
    if free:
        comps["Δt"] = rng.uniform(0.1, 0.3, (1, T))
    return qc.NamedTrajectory(comps, controls=("a",), timestep="Δt" if free else 0.2)


def measure(qc, name, traj, H_error, hess, reps, subspace=None):
    obj = qc.UnitaryRobustnessObjective(traj, H_error=H_error, eval_hessian=hess, subspace=subspace)
    Z = traj.datavec
    dZ = torch.from_numpy(Z).cuda()
    dL = torch.empty(1, dtype=torch.float64, device="cuda")
    dg = torch.empty(Z.size, dtype=torch.float64, device="cuda")
    dH = torch.empty(obj.hess_nnz, dtype=torch.float64, device="cuda") if hess else None
    for _ in range(3):
        obj.eval_device(dZ, dL, dg, dH)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        obj.eval_device(dZ, dL, dg, dH)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / reps
    n = obj.H.shape[0]
    N = int(round((len(traj.components["Ũ⃗"]) / 2) ** 0.5))
    K = traj.T
    # bytes: the subspace entries read (twice: partial sums and gradient launch), the dense gradient written, the Hessian written
    read = 2 * K * 2 * n * n * 8
    written = Z.size * 8 + (obj.hess_nnz * 8 if hess else 0)
    out = dict(name=name, T=traj.T, N=N, n=n, V=obj.n_vars, hessian=hess, hess_values=obj.hess_nnz if hess else 0,
               launches_per_call=4 if hess else 3, device_us_per_call=round(us, 2), bytes_read=read, bytes_written=written,
               fraction_of_8TBps=round((read + written) / (us * 1e-6) / HBM, 4), L=float(dL.item()))
    print(json.dumps(out), flush=True)
    obj.close()
    return out


def main():
    qc = g.load_package()
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    ZII = qc.operator_from_string("ZII")
    res = [measure(qc, "l_grad_c3", qc.config_inputs(3).traj, ZII, False, reps),
           measure(qc, "l_grad_c4", qc.config_inputs(3, T=8000).traj, ZII, False, reps)]
    Zsub = qc.EmbeddedOperator("Z", [0, 1], 3)
    res.append(measure(qc, "hess_459", synthetic_traj(qc, 51, 3), Zsub, True, reps))
    res.append(measure(qc, "hess_cap", synthetic_traj(qc, 1500, 3), Zsub, True, max(3, reps // 4)))
    return res


if __name__ == "__main__":
    main()
