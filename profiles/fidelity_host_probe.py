#!/usr/bin/env python3
"""Wall time of the host-buffer call qc_fidelity_eval (value, gradient, Hessian) at N = 8: median over 2000 calls after 200 warm-up
calls, one JSON line.  With QCOLLOC_HIP_VARIANT=name it times csrc/libqcolloc_hip.<name>.so (an A/B of two builds, run by run)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402

qc = g.load_package()
from qcolloc_amd.objectives import _Fidelity  # noqa: E402

rng = np.random.default_rng(0)
f = _Fidelity(rng.standard_normal(128))
u = rng.standard_normal(128)
t = []
for k in range(2200):
    t0 = time.perf_counter()
    f.eval(u)
    t.append(time.perf_counter() - t0)
print(json.dumps(dict(case="qc_fidelity_eval N=8", us=round(float(np.median(t[200:])) * 1e6, 2))))
f.close()
