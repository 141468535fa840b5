#!/usr/bin/env python3
"""Kernel-by-kernel comparison of knn.hip's gfx950 assembly at two commits (no GPU needed).

At each commit, with build_native.py's flags for the file (COMMON_FLAGS + PER_FILE_FLAGS), device side only:

    cd fraud_detection_amd/csrc && hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall \\
        -Wno-unused-function -Wno-unused-variable -I. -Ikernels -mllvm -amdgpu-mfma-vgpr-form=1 \\
        --cuda-device-only -S kernels/knn.hip -o knn_<commit>.s
    python tools/knn_isa_compare.py knn_parent.s knn_branch.s > profiles/<dir>/isa_compare.txt

For every kernel of the second file: its instruction text (the function ordinal in .LBB<n>_<m> /
.Lfunc_end<n> and in the loop comments normalised: it shifts when other functions come or go), its
.amdhsa_kernel descriptor and its metadata entry must equal the first file's.  Exit status 1 otherwise.
"""
import re
import subprocess
import sys


def parse(path):
    text = open(path).read()
    funcs = {}
    for m in re.finditer(r"\.type\s+(\S+),@function\n(.*?)\n\.Lfunc_end\d+:", text, re.S):
        body = re.sub(r"(\.L|\b)BB\d+_", r"\1BB#_", m.group(2))
        funcs[m.group(1)] = re.sub(r"[ \t]+;", " ;", body)  # comment columns follow the label's width
    desc = {m.group(1): m.group(0)
            for m in re.finditer(r"\.amdhsa_kernel\s+(\S+)\n.*?\.end_amdhsa_kernel", text, re.S)}
    a = text.index("amdhsa.kernels:")
    meta = {re.search(r"\.name:\s+(\S+)", e).group(1): e.rstrip()
            for e in re.split(r"\n  - ", text[a:text.index("amdhsa.target:", a)])[1:]}
    return funcs, desc, meta


def main():
    (pf, pd, pm), (bf, bd, bm) = parse(sys.argv[1]), parse(sys.argv[2])
    names = sorted(bm)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    field = lambda e, k: (re.search(r"\." + k + r":\s+(\S+)", e) or [0, "-"])[1]  # noqa: E731
    gone_n, new_n = len(set(pm) - set(bm)), len(set(bm) - set(pm))
    print(f"kernels: {len(pm)} before, {len(bm)} after ({gone_n} removed, {new_n} new)")
    print("text / descriptor / metadata against the first file, then VGPR AGPR SGPR LDS-bytes scratch-bytes "
          "VGPR-spills SGPR-spills")
    bad = 0
    for n, d in zip(names, dem):
        d = re.sub(r"\(.*", "", d.replace("void ", "").replace("fdx::(anonymous namespace)::", ""))
        same = [n in pm and x[0].get(n) == x[1][n] for x in ((pf, bf), (pd, bd), (pm, bm))]
        bad += not all(same)
        e = bm[n]
        print(f"{d:32s}" + "".join(" same" if s else " DIFF" for s in same) + "  " + " ".join(
            f"{field(e, k):>5s}" for k in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size",
                                           "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")))
    gone = subprocess.run(["c++filt"], input="\n".join(set(pm) - set(bm)), capture_output=True, text=True).stdout
    print("removed:", ", ".join(sorted({re.sub(r"[<(].*", "", g.replace("void ", "").replace(
        "fdx::(anonymous namespace)::", "")) for g in gone.split("\n") if g})))
    print(f"RESULT: {len(names) - bad} of {len(names)} kernels identical, {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    raise SystemExit(main())
