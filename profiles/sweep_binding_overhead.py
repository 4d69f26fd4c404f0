"""Per-call cost of the Python binding of the rollout sweeps: a loop of 1000 `eval_device` calls and a loop of 1000 `hvp_device` calls
(the entry with the most arguments), each followed by one synchronize, on the smallest closed handle (2N = 4, T = 2, S = 1) so that the
host side dominates.

    python profiles/sweep_binding_overhead.py [--package DIR] [--label NAME]

--package: the directory of the package to time (default: this tree's quantumcollocation.jl_amd/; another revision's *.py beside a
csrc/libqcolloc_hip.so compares the two bindings over one library).  Prints one JSON line: seconds per loop of 1000 calls.  Run the two
revisions in turn, one process each (profiles/sweep_binding_overhead.txt has the figures of the last comparison).
"""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np
import torch

CALLS = 1000


def load(pkg_dir):
    spec = importlib.util.spec_from_file_location("qcolloc_timed", os.path.join(pkg_dir, "__init__.py"), submodule_search_locations=[pkg_dir])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["qcolloc_timed"] = mod
    spec.loader.exec_module(mod)
    return mod


def timed(call):
    for _ in range(CALLS):      # warm-up: code objects, the handle's scratch, the interpreter's caches
        call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(CALLS):
        call()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--package", default=os.path.join(here, "quantumcollocation.jl_amd"))
    ap.add_argument("--label", default="tree")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    qc = load(args.package)
    X = np.array([[0, 1], [1, 0]], dtype=complex)
    Zp = np.diag([1.0, -1.0]).astype(complex)
    sw = qc.RolloutSweep(qc.QuantumSystem(Zp, [X]), [Zp], 2, goal=qc.operator_to_iso_vec(np.eye(2, dtype=complex)), fid_kind="unitary")
    assert sw.hvp_supported, sw.hvp_unsupported_reason
    S = 1
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    rng = np.random.default_rng(0)
    dZ = dev(sw.pack(0.3 * rng.standard_normal((1, 2)), 0.1))
    dinit = dev(qc.operator_to_iso_vec(np.eye(2, dtype=complex)))
    dtheta, dscale = dev(0.05 * rng.standard_normal((S, 1))), dev(np.ones((S, 1)))
    dcot, dvcot = dev(rng.standard_normal((S, sw.ns))), dev(rng.standard_normal((S, sw.ns)))
    dvZ, dvinit = dev(rng.standard_normal(sw.Z_len)), dev(rng.standard_normal(sw.ns))
    dvtheta, dvscale = dev(rng.standard_normal((S, 1))), dev(rng.standard_normal((S, 1)))
    out = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda")
    dfinals, dfids = out(S, sw.ns), out(S)
    dtgrad, dtgrad_samples, dtgrad_init = out(sw.Z_len), out(S, sw.T - 1, sw.n_deriv), out(S, sw.ns)
    stream = torch.cuda.current_stream()
    t_eval = timed(lambda: sw.eval_device(dZ, dinit, dtheta, dscale, dfinals, dfids, stream))
    t_hvp = timed(lambda: sw.hvp_device(dZ, dinit, S, dcot, dtheta, dscale, dvZ, dvinit, dvtheta, dvscale, dvcot, dtgrad, dtgrad_samples,
                                        dtgrad_init, stream))
    assert bool(torch.isfinite(dfinals).all()) and bool(torch.isfinite(dtgrad).all())
    print(json.dumps({"label": args.label, "kernel": sw.kernel_name, "calls": CALLS, "eval_device_s": t_eval, "hvp_device_s": t_hvp}))
    sw.close()


if __name__ == "__main__":
    main()
