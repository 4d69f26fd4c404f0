"""Which kernel serves a handle (quantumcollocation.jl_amd/csrc/qc_plan.cpp), on the CPU: tests/kernel_plan_test.cpp runs the device-free
half of qc_create and the plan function over a sweep of descriptors and prints one line per case -- the kernel class, the three
kernels (enumerators) and the properties the host paths read -- and then every name qc_kernel_name gave for an enumerator.  The table must equal tests/golden/kernel_selection.txt byte for
byte: that file was recorded from the predicate chains of the launchers, of qc_kernel_name and of the host paths as they were before
one function took their place.

The fourth section is about lists of handles (sampling problems, direct sums): can the members share ONE launch (qc_plan_list)?  Its
lines were checked one by one against the rule that test_list_answers_follow_the_rule_in_words restates from the members' printed
descriptions alone, so the recorded answers do not rest on the function that printed them."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quantumcollocation.jl_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "kernel_selection.txt")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# the recorded sections: (header line of the golden file, sweep, environment)
SECTIONS = [
    ("# section: default", "full", {}),
    ("# section: QC_NO_ELL=1", "switches", {"QC_NO_ELL": "1"}),
    ("# section: QC_HESS_TWO_WAVES=0 QC_HESS_G2=0", "switches", {"QC_HESS_TWO_WAVES": "0", "QC_HESS_G2": "0"}),
    ("# section: lists", "lists", {}),
]
# Families that no descriptor reaches without a switch (or QC_STAMPS): the one-wave mu_d2F kernel's row-gather form stands behind
# qc_mfma_hess_g2.hip, which serves every handle it serves.
SWITCH_GATED = {("hess", "PADE4_16_GATHER")}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("needs hipcc")
    lib = os.path.join(CSRC, "libqcolloc_hip.so")
    assert os.path.exists(lib), "libqcolloc_hip.so is not built (__graft_entry__.build())"
    exe = str(tmp_path_factory.mktemp("kernel_plan") / "kernel_plan_test")
    cmd = [HIPCC, "-O1", "-std=c++17", "--offload-arch=gfx950", "-x", "hip", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "kernel_plan_test.cpp"), "-o", exe, "-L" + CSRC, "-lqcolloc_hip", "-Wl,-rpath," + CSRC]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


def run(exe, sweep, extra_env):
    env = {k: v for k, v in os.environ.items() if not k.startswith("QC_")}      # a fresh process: the switches are read once
    env.update(extra_env)
    r = subprocess.run([exe, sweep], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr
    return r.stdout


def golden_sections():
    out, name = {}, None
    with open(GOLDEN) as f:
        for line in f:
            if line.startswith("# section:"):
                name = line.rstrip("\n")
                out[name] = ""
            else:
                out[name] += line
    return out


def kernels_in(table):
    """(question, enumerator) of every case line `<case> | <class> <F + dF> <mu_d2F> <one call> | <properties>`."""
    seen = set()
    for line in table.splitlines():
        cols = line.split(" | ")
        if len(cols) == 3:      # (not a refusal, not a `name` line)
            seen.update(zip(("jac", "hess", "fused"), cols[1].split()[1:]))
    return seen


def test_kernel_selection_equals_the_recorded_table(driver):
    golden = golden_sections()
    assert list(golden) == [s[0] for s in SECTIONS]
    for header, sweep, env in SECTIONS:
        got = run(driver, sweep, env)
        if got != golden[header]:
            want = golden[header].splitlines()
            diff = [f"{header}, line {i + 1}:\n  recorded {w}\n  now      {g}" for i, (w, g) in enumerate(zip(want, got.splitlines())) if w != g]
            pytest.fail(f"{len(diff)} differing line(s), {len(got.splitlines())} against {len(want)} recorded\n" + "\n".join(diff[:10]))


def test_every_kernel_family_occurs_in_the_table(driver):
    every = {tuple(line.split()) for line in run(driver, "enumerators", {}).splitlines()}
    assert len(every) == 11 + 16 + 4
    golden = golden_sections()
    default = kernels_in(golden[SECTIONS[0][0]])
    assert every - default == SWITCH_GATED          # reached by descriptors alone: everything else
    assert SWITCH_GATED <= kernels_in("".join(golden.values()))      # ... and the rest under the switches of the other sections
    assert kernels_in("".join(golden.values())) <= every


def test_list_answers_follow_the_rule_in_words(driver):
    """One launch serves a list of two or more members when every member is an order-4 Pade integrator of the MFMA class with 2N <= 16
    (the batched kernel: up to 32 drives for F + dF and the host-buffer Jacobian path, up to 8 and a Hessian at all -- drives or a free
    timestep -- for mu_d2F), and the members agree in levels, state columns, drives, first interval, length and knot width; mu_d2F
    also wants them to agree on whether their generators are antisymmetric.  Restated here from the printed descriptions."""
    cols = {"unitary": lambda N: N, "kets": lambda N: max(1, N // 2), "density": lambda N: 1}
    lines = run(driver, "lists", {}).splitlines()
    assert len(lines) >= 70
    seen = set()
    for line in lines:
        head, answers = line.split(" | ")
        count, members = head.split(": ")
        ms = []
        for text in members.split(" ; "):
            integ, N, state, dt, m, gen, t, z, cls = text.split()
            N, m = int(N[2:]), int(m[2:])
            ms.append(dict(batchable=integ == "pade4" and cls == "auto" and 2 * N <= 16 and m <= 32, hess=m <= 8 and (m > 0 or dt == "free"),
                           shape=(N, cols[state](N), m, t, z), anti=gen != "nonanti"))
        assert int(count.split()[1]) == len(ms)
        share = len(ms) >= 2 and all(x["batchable"] for x in ms) and len({x["shape"] for x in ms}) == 1
        hess = share and all(x["hess"] for x in ms) and len({x["anti"] for x in ms}) == 1
        assert answers.split() == [str(int(share)), str(int(hess)), str(int(share))], line
        seen.add((len(ms), share, hess))
    assert {(2, True, True), (3, True, True), (2, True, False), (3, True, False), (2, False, False), (3, False, False), (1, False, False)} <= seen
