#!/usr/bin/env python3
"""Device assembly of the sweep family at two commits, compared per kernel symbol: the instruction stream (labels renumbered, comments
dropped), the .amdhsa_kernel block and the metadata (VGPRs, AGPRs, SGPRs, LDS, scratch, spills, MFMA count).  Needs no GPU.

    for f in <FILES below>; do
        hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S $f.hip -o DIR/$f.s       # once in each tree
    done
    python profiles/sweep_asm_diff.py PARENT_DIR NEW_DIR [--changed qc_sweep_seed_kernel,qc_sweep_grad_kernel,...]

Kernels named by --changed (default: the four seed kernels; a template's name without its arguments names every instantiation) are
reported with their metadata on both sides, wherever they live, and must agree in everything that decides occupancy (VGPRs, AGPRs, LDS,
scratch, spills: none) and in their MFMA count; SGPRs and the instruction count may move.  With --vgpr-ceiling N a changed kernel's VGPR
count may also fall, never rise, and never lie above N (the mfma64 form: 1024 threads, four waves a SIMD, N = 128).  --renamed
PARENT=NEW,... pairs changed kernels whose name differs between the trees.  Every other kernel must be identical.  The exit status says
whether all of that holds."""
import argparse
import os
import re
import subprocess
import sys

FILES = ["qc_sweep", "qc_sweep32", "qc_sweep_grad", "qc_sweep32_grad", "qc_sweep_vjp", "qc_sweep_jvp", "qc_sweep32_jvp", "qc_sweep_hvp",
         "qc_sweep32_hvp", "qc_sweep_noise", "qc_sweep32_noise", "qc_sweep_open_grad", "qc_sweep32_open_grad", "qc_sweep64", "qc_sweep64_grad",
         "qc_sweep64_jvp", "qc_sweep64_noise"]
SEEDS = "qc_sweep_seed_kernel,qc_sweep32_seed_kernel,qc_sweep_cot_seed_kernel,qc_sweep32_cot_seed_kernel"
KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count")
FIXED = ("vgpr_count", "agpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count", "mfma")


def relabel(text):
    return re.sub(r"\.LBB\d+_", ".LBB_", text)


def kernels(path):
    """{mangled name: (instructions, .amdhsa_kernel block, metadata)} of one .s file; a file one tree does not have holds no kernels (its
    kernels on the other side are then reported as "on one side only" unless named by --changed)"""
    if not os.path.exists(path):
        return {}
    txt = open(path).read()
    notes = txt[txt.rfind("amdhsa.kernels"):]
    out = {}
    for m in re.finditer(r"^(_Z\w+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:", txt, re.S | re.M):
        name = m.group(1)
        k = re.search(r"\.amdhsa_kernel %s\n(.*?)\.end_amdhsa_kernel" % name, txt, re.S)
        if not k:
            continue      # a device function
        body = [re.sub(r"\s*;.*$", "", ln) for ln in relabel(m.group(2)).splitlines()]
        body = [ln for ln in body if ln.strip()]
        blk = [b for b in re.split(r"\n  - \.agpr_count", notes) if re.search(r"\.name:\s+%s\n" % name, b)]
        assert len(blk) == 1, name
        meta = {key: int(re.search(r"\.%s:\s+(\d+)" % key, ".agpr_count" + blk[0]).group(1)) for key in KEYS}
        meta["instructions"] = sum(1 for ln in body if ln.startswith("\t") and not ln.strip().startswith("."))
        meta["mfma"] = sum(1 for ln in body if ln.strip().startswith("v_mfma"))
        out[name] = ("\n".join(body), relabel(k.group(1)), meta)
    return out


def plain(name):
    o = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip().replace("(anonymous namespace)::", "")
    return re.match(r"(?:void )?([\w:]+(?:<[^>]*>)?)", o).group(1)


def show(meta):
    return (f"VGPR {meta['vgpr_count']} AGPR {meta['agpr_count']} SGPR {meta['sgpr_count']} LDS {meta['group_segment_fixed_size']} B scratch "
            f"{meta['private_segment_fixed_size']} B spills {meta['sgpr_spill_count']}+{meta['vgpr_spill_count']} MFMA {meta['mfma']} "
            f"instructions {meta['instructions']}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--changed", default=SEEDS)
    ap.add_argument("--vgpr-ceiling", type=int, default=None, metavar="N",
                    help="a changed kernel's VGPR count may fall (never rise, never exceed N); without it any change counts as moved")
    ap.add_argument("--renamed", default="", metavar="PARENT=NEW,...",
                    help="changed kernels whose name differs between the trees: the parent's is compared with, and shown as, the new one")
    a = ap.parse_args()
    changed = set(a.changed.split(","))
    renamed = dict(pair.split("=") for pair in a.renamed.split(",") if pair)
    sides = [{}, {}]
    differ = same = moved = 0
    for f in FILES:
        A, B = (kernels(os.path.join(d, f + ".s")) for d in (a.parent, a.new))
        for name in sorted(set(A) | set(B)):
            p = plain(name)
            if p in changed or p.split("<")[0] in changed:
                for side, K, to in zip(sides, (A, B), (renamed, {})):
                    if name in K:
                        side[to.get(p, p)] = (f, K[name][2])
            elif name in A and name in B and A[name] == B[name]:
                same += 1
                print(f"{f}.hip  {p}: identical instructions and metadata  ({show(A[name][2])})")
            else:
                differ += 1
                print(f"{f}.hip  {p}: DIFFERS" if name in A and name in B else f"{f}.hip  {p}: on one side only")
    for p in sorted(set(sides[0]) | set(sides[1])):
        for label, side in zip(("parent", "new   "), sides):
            if p in side:
                print(f"{p}  {label} ({side[p][0]}.hip): {show(side[p][1])}")
        if p in sides[0] and p in sides[1]:
            A, B = sides[0][p][1], sides[1][p][1]
            fell = a.vgpr_ceiling is not None and B["vgpr_count"] < A["vgpr_count"] and B["vgpr_count"] <= a.vgpr_ceiling
            off = [k for k in FIXED if A[k] != B[k] and not (fell and k == "vgpr_count")]
            off += [k for k in ("sgpr_spill_count", "vgpr_spill_count") if B[k]]
            if a.vgpr_ceiling is not None and B["vgpr_count"] > a.vgpr_ceiling:
                off.append(f"vgpr_count above the ceiling of {a.vgpr_ceiling}")
            if off:
                moved += 1
            ok = f"VGPRs fell {A['vgpr_count']} -> {B['vgpr_count']}, other resources" if fell else "resources"
            print(f"{p}  " + (f"RESOURCES MOVED: {', '.join(off)}" if off else f"{ok} and MFMA count equal, no spills") +
                  f"; SGPR {B['sgpr_count'] - A['sgpr_count']:+d}, instructions {B['instructions'] - A['instructions']:+d}")
        else:
            moved += 1
            print(f"{p}  on one side only")
    print(f"{same} kernels identical in instruction stream and metadata, {differ} differ or exist on one side only; of the "
          f"{len(set(sides[0]) | set(sides[1]))} kernels named as changed, {moved} moved in VGPRs, AGPRs, LDS, scratch, spills or MFMA count")
    return 1 if differ or moved else 0


if __name__ == "__main__":
    sys.exit(main())
