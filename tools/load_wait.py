#!/usr/bin/env python3
"""Where a kernel's loads stand relative to their waits (CPU only): for every basic block of at least --min vector-ALU
instructions of the kernels whose demangled name contains FILTER, the global / scalar loads, the LDS reads at or beyond
--lds-from bytes (the region behind the teams' slabs: the twiddle images) and every s_waitcnt, each with the number of
vector-ALU instructions of the block issued before it.  The distance between a load's line and the wait that covers it
is the cover the load gets.

usage: tools/load_wait.py --asm FILE.s [--min 400] [--lds-from 33280] FILTER ...
  FILE.s   hipcc -O3 --offload-arch=gfx950 -std=c++17 --cuda-device-only -S ring_zk_amd/csrc/rzk_kernels.hip
  FILTER   e.g. "unit_kernel<10, false, false, rzk::WaveTeamTw>"
"""
import argparse
import re
import subprocess


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--asm", required=True)
    ap.add_argument("--min", type=int, default=400)
    ap.add_argument("--lds-from", type=int, default=33280)
    ap.add_argument("filters", nargs="+")
    args = ap.parse_args()
    with open(args.asm) as fh:
        lines = fh.read().splitlines()
    names = [m.group(1) for m in (re.match(r"^(_Z\w+):", l) for l in lines) if m]
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    wanted = {n for n, p in zip(names, plain) if any(f in p for f in args.filters)}
    pretty = dict(zip(names, plain))
    kernel, block, body = None, None, []

    def flush():
        nv = sum(1 for i in body if i.startswith("v_"))
        if kernel in wanted and block and nv >= args.min:
            print(f"{pretty[kernel].split('(')[0]}  {block}: {nv} vector-ALU instructions")
            v = 0
            for i in body:
                v += i.startswith("v_")
                lds = re.match(r"ds_read\w* .*offset:(\d+)", i)
                if re.match(r"(global_load|s_load|s_waitcnt)", i) or (lds and int(lds.group(1)) >= args.lds_from):
                    print(f"   after {v:4d}  {i}")

    for l in lines:
        m = re.match(r"^(_Z\w+):", l)
        if m:
            flush()
            kernel, block, body = m.group(1), "entry", []
            continue
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            flush()
            block, body = m.group(1), []
            continue
        if l.startswith(".Lfunc_end"):
            flush()
            kernel, block, body = None, None, []
            continue
        if kernel and re.match(r"\s+[a-z]", l):
            body.append(l.strip())


if __name__ == "__main__":
    main()
