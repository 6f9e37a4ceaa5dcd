#!/usr/bin/env python3
"""device_asm.py [--by-content] TREE OUTDIR — the gfx950 device code of every .hip file of a tree, one file per (translation unit, function).

A refactor of the host side of a .hip file must leave the device code alone.  Run this on the parent tree and on the
result and compare with `diff -r`: the set of files is the set of kernels, each file holds a kernel's instructions and its
.amdhsa_kernel descriptor.  Block labels carry the function's emission index, which moves with the order of the
instantiations in the source; they are renumbered away, nothing else is.

--by-content is for a refactor that RENAMES kernels (a kernel that becomes a template instantiation gets another mangled
name).  Inside each function's text the function's own symbol is replaced by a placeholder, the file is named by the hash
of that text, and every unit gets an INDEX file of `hash  symbol` lines.  `diff -r -x INDEX` between two trees is then
empty exactly when every unit holds the same multiset of function bodies, whatever they are called, and the INDEX files
show which symbol became which.  The one line that follows the name's form and not the code is left out: the binding
directive (.globl for a plain kernel, .weak for an instantiation)."""
import collections
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
SELF = "@self@"


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


def write_by_name(udir, funcs):
    for sym, lines in funcs.items():   # (mangled names pass 255 bytes: keep the readable head, hash the whole)
        fname = sym[:120] + "." + hashlib.sha1(sym.encode()).hexdigest()[:12] + ".s"
        with open(os.path.join(udir, fname), "w") as fh:
            fh.write("\n".join(lines) + "\n")


def write_by_content(udir, funcs):
    index, seen = [], collections.Counter()
    for sym, lines in funcs.items():
        body = lines[1:] if lines[0].startswith((".globl", ".weak")) else lines   # (the "Begin function" comment stands behind it)
        text = "\n".join(line.replace(sym, SELF) for line in body) + "\n"
        h = hashlib.sha1(text.encode()).hexdigest()[:16]
        seen[h] += 1   # (two instantiations may share a body: the second copy is a file of its own)
        with open(os.path.join(udir, h + (".s" if seen[h] == 1 else f".{seen[h]}.s")), "w") as fh:
            fh.write(text)
        index.append(f"{h}  {sym}\n")
    with open(os.path.join(udir, "INDEX"), "w") as fh:
        fh.writelines(sorted(index))


def main(argv):
    by_content = "--by-content" in argv
    tree, outdir = [a for a in argv if a != "--by-content"][:2]
    srcs = sorted(glob.glob(os.path.join(tree, "ring_zk_amd", "csrc", "*.hip")))
    with concurrent.futures.ThreadPoolExecutor(8) as pool:
        for unit, funcs in pool.map(split, srcs):
            os.makedirs(os.path.join(outdir, unit), exist_ok=True)
            (write_by_content if by_content else write_by_name)(os.path.join(outdir, unit), funcs)
            print(f"{unit}: {len(funcs)} functions")


if __name__ == "__main__":
    main(sys.argv[1:])
