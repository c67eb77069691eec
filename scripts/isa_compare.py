#!/usr/bin/env python3
"""Compare the device code of two builds, kernel by kernel.

  isa_compare.py A_DIR B_DIR [-o report.txt]

A_DIR and B_DIR hold one gfx950 assembly file per define set under the same names (default.s, timing.s, ...: device.hip
compiled with the Makefile's FLAGS, the set's defines and `--cuda-device-only -S`; `make asm` keeps the same text as
build/device-hip-amdgcn-amd-amdhsa-gfx950.s).  Every function symbol of a file is compared with its namesake in the
other directory: the instruction text (local label numbers normalised, comments and debug directives dropped) and the
resource figures the assembler prints behind each kernel (VGPRs, SGPRs, scratch, LDS, occupancy).  Prints per-file totals
and names every kernel that differs, with the first differing lines.
"""
import argparse
import os
import re
import subprocess
import sys

FIG = ("NumSgprs", "NumVgprs", "NumAgprs", "ScratchSize", "Occupancy", "LDSByteSize", "codeLenInByte")


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def split(path):
    """{symbol: (instruction lines, {figure: value})}"""
    funcs, cur, name, figs = {}, None, None, None
    types = set()
    for raw in open(path, errors="replace"):
        line = raw.rstrip()
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            types.add(m.group(1))
            continue
        m = re.match(r"(\S+):\s*(;.*)?$", line)
        if m and m.group(1) in types and cur is None:
            name, cur, figs = m.group(1), [], {}
            continue
        if cur is None:
            if name is not None:                            # the figures follow the function's end as comments
                m = re.match(r";\s*(\w+):\s*(\d+)\s*$", line)
                if m and m.group(1) in FIG:
                    funcs[name][1][m.group(1)] = int(m.group(2))
            continue
        if re.match(r"\.Lfunc_end\d+:", line):
            funcs[name] = (cur, figs)
            cur = None
            continue
        text = line.split(";")[0].strip()
        if not text or re.match(r"\.(loc|file|cfi_|p2align|section)\b", text):
            continue
        cur.append(re.sub(r"\.L(BB|tmp|func_begin|func_end)\d+(_\d+)?", lambda mm: ".L" + mm.group(1) + (mm.group(2) or ""), text))
    return funcs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("-o", "--out")
    ap.add_argument("--context", type=int, default=3)
    args = ap.parse_args()
    lines = []
    total = same = 0
    for f in sorted(os.listdir(args.a)):
        if not f.endswith(".s") or not os.path.exists(os.path.join(args.b, f)):
            continue
        A, B = split(os.path.join(args.a, f)), split(os.path.join(args.b, f))
        names = demangle(sorted(set(A) | set(B)))
        n = ident = 0
        diffs = []
        for sym in sorted(set(A) | set(B)):
            n += 1
            if sym not in A or sym not in B:
                diffs.append("  only in %s: %s" % ("A" if sym in A else "B", names[sym]))
                continue
            (ia, fa), (ib, fb) = A[sym], B[sym]
            if ia == ib and fa == fb:
                ident += 1
                continue
            diffs.append("  DIFFERS %s" % names[sym])
            for k in FIG:
                if fa.get(k) != fb.get(k):
                    diffs.append("    %s: %s -> %s" % (k, fa.get(k), fb.get(k)))
            if ia != ib:
                i = next((i for i, (x, y) in enumerate(zip(ia, ib)) if x != y), min(len(ia), len(ib)))
                diffs.append("    instructions: %d -> %d, first difference at line %d" % (len(ia), len(ib), i))
                for x in ia[i:i + args.context]:
                    diffs.append("      A: " + x)
                for y in ib[i:i + args.context]:
                    diffs.append("      B: " + y)
        stack = [s for s in A if "k_trace_stack" in s and s in B]
        fig = sorted({(A[s][1].get("NumVgprs"), A[s][1].get("Occupancy")) for s in stack})
        lines.append("%s: %d kernels compared, %d identical%s" % (f[:-2], n, ident, (" (k_trace_stack: %d instantiations, (VGPRs, occupancy) in A: %s, scratch A %d..%d B %d..%d)" % (
            len(stack), fig, min(A[s][1]["ScratchSize"] for s in stack), max(A[s][1]["ScratchSize"] for s in stack),
            min(B[s][1]["ScratchSize"] for s in stack), max(B[s][1]["ScratchSize"] for s in stack))) if stack else ""))
        lines += diffs
        total += n
        same += ident
    lines.append("total: %d kernels compared, %d identical" % (total, same))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        open(args.out, "w").write(text)
    return 0 if total == same else 1


if __name__ == "__main__":
    sys.exit(main())
