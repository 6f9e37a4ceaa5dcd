#!/usr/bin/env python3
"""device_asm.py TREE OUTDIR — the gfx950 device code of every .hip file of a tree, one file per (translation unit, function).

A refactor of the host side of a .hip file must leave the device code alone.  Run this on the parent tree and on the
result and compare with `diff -r`: the set of files is the set of kernels, each file holds a kernel's instructions and its
.amdhsa_kernel descriptor.  Block labels carry the function's emission index, which moves with the order of the
instantiations in the source; they are renumbered away, nothing else is."""
import concurrent.futures
import glob
import hashlib
import os
import re
import subprocess
import sys

FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "--offload-device-only", "-S", "-o", "-"]
BEGIN = re.compile(r"; -- Begin function (\S+)")
INDEX = re.compile(r"(BB|func_end|Ltmp)\d+")   # .LBB12_3, BB12_3 in comments, .Lfunc_end12, .Ltmp12


def split(path):
    asm = subprocess.run(["hipcc"] + FLAGS + [path], check=True, capture_output=True, text=True).stdout
    out, name = {}, None
    for line in asm.splitlines():
        m = BEGIN.search(line)
        if m:
            name = m.group(1)
            out[name] = []
        if name:
            out[name].append(" ".join(INDEX.sub(r"\1", line).split()))   # (the padding behind a label follows its length)
        if "; -- End function" in line:
            name = None
    return os.path.basename(path)[:-4], out


def main(tree, outdir):
    srcs = sorted(glob.glob(os.path.join(tree, "ring_zk_amd", "csrc", "*.hip")))
    with concurrent.futures.ThreadPoolExecutor(8) as pool:
        for unit, funcs in pool.map(split, srcs):
            os.makedirs(os.path.join(outdir, unit), exist_ok=True)
            for sym, lines in funcs.items():   # (mangled names pass 255 bytes: keep the readable head, hash the whole)
                fname = sym[:120] + "." + hashlib.sha1(sym.encode()).hexdigest()[:12] + ".s"
                with open(os.path.join(outdir, unit, fname), "w") as fh:
                    fh.write("\n".join(lines) + "\n")
            print(f"{unit}: {len(funcs)} functions")


if __name__ == "__main__":
    main(*sys.argv[1:3])
