#!/usr/bin/env python3
"""Static vector-ALU budget of the kernels (CPU only): compiles ring_zk_amd/csrc/rzk_kernels.hip to gfx950 assembly and
prints, per kernel whose demangled name contains one of the filters and per basic block, how many vector-ALU
instructions (mnemonics starting with v_) it holds, with the most frequent mnemonics of the larger blocks.

usage: tools/inst_budget.py [--asm FILE.s] [--min 40] [--top 6] [FILTER ...]
  --asm FILE.s   read an assembly file made earlier (hipcc -O3 --offload-arch=gfx950 --cuda-device-only -S) instead of compiling
  --min N        list only blocks with at least N vector-ALU instructions (the kernel's total always counts every block)
  FILTER         default: the two Open-cycle instantiations at N = 1024, unit_kernel<10, false, false> and <10, false, true>

The counts are static: a block inside a loop is executed many times, a block behind a branch perhaps never.  They size
what a change to one block can save; the dynamic weights come from the SQ_INSTS_VALU counter (tools/sq_counters.py)."""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "ring_zk_amd", "csrc", "rzk_kernels.hip")
DEFAULT = ["unit_kernel<10, false, false, rzk::WaveTeam>", "unit_kernel<10, false, true, rzk::WaveTeam>"]


def assembly(path):
    if path:
        with open(path) as fh:
            return fh.read()
    hipcc = next((c for c in ("/opt/rocm/bin/hipcc",) if os.path.exists(c)), "hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.check_call([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-S", SRC, "-o", out],
                              stderr=subprocess.DEVNULL)
        with open(out) as fh:
            return fh.read()


def demangle(names):
    try:
        p = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, p.stdout.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def kernels(text):
    """{mangled name: [(block label, Counter of v_ mnemonics)]} for every function of the file"""
    out, name, blocks = {}, None, None
    for line in text.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, blocks = m.group(1), [("entry", collections.Counter())]
            out[name] = blocks
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            name = None
            continue
        m = re.match(r"^(\.LBB\w+):", line)
        if m:
            blocks.append((m.group(1), collections.Counter()))
            continue
        m = re.match(r"^\s+(v_\w+)", line)
        if m:
            blocks[-1][1][m.group(1)] += 1
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--asm")
    ap.add_argument("--min", type=int, default=40)
    ap.add_argument("--top", type=int, default=6)
    ap.add_argument("filters", nargs="*")
    args = ap.parse_args()
    filters = args.filters or DEFAULT
    ks = kernels(assembly(args.asm))
    names = demangle(list(ks))
    shown = 0
    for mangled, blocks in ks.items():
        nice = names[mangled]
        if not any(f in nice for f in filters):
            continue
        shown += 1
        total = sum(sum(c.values()) for _, c in blocks)
        print(f"{nice.split('(')[0]}: {total} vector-ALU instructions in {len(blocks)} blocks")
        for label, c in blocks:
            n = sum(c.values())
            if n >= args.min:
                top = ", ".join(f"{k} {v}" for k, v in c.most_common(args.top))
                print(f"  {label:14s} {n:6d}   {top}")
        allc = collections.Counter()
        for _, c in blocks:
            allc.update(c)
        print("  all blocks: " + ", ".join(f"{k} {v}" for k, v in allc.most_common(12)))
    if not shown:
        sys.exit("no kernel matches " + repr(filters))


if __name__ == "__main__":
    main()
