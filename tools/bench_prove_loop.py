#!/usr/bin/env python3
"""The zero-knowledge Open prover with its loop in Python (fiat_shamir.open_prove_zk / open_prove_zk32, the parent's code,
unchanged) beside the same prover with the loop inside the library (open_prove_zk_native): one JSON line.

Shapes: Open (1,3,1), N = 512 and 1024, B = 4096 and B = 64 (the launch-bound end).  Per shape, in ONE process, on device
tensors, four variants: python:w64, python:w32, native:w64, native:w32.  All draw under the same key and first nonce, so
every variant runs the same rounds on the same pending sets and returns the same proofs (asserted before anything is timed).
After a warm-up of every variant, --repeats rounds of alternated windows of at least --window-s seconds, device events
around each window (the method of tools/bench_prove32.py).  Reported per variant: median microseconds per batch, the
min-max spread and the raw windows.

The yardstick of a native variant is the Python loop of the same width in the same round of windows:
`faster_in_every_window` = every native window lies below the Python window of the same round; `ratio` = native median /
Python median.  Per shape also: the rounds that ran, the native time per round, the sum of the kernels' own durations of one
native run as rzk_prof_read_all reports them (HIP events around each launch: on a busy stream they include the wait for
the launch before), and the cost of one read-back measured alone (compaction launch, 4-byte copy to the host, synchronise;
host clock, through the Python binding).  Where the native time goes kernel by kernel is a trace's business:
--trace-shape under rocprofv3, --summarise-trace on its CSV (profiles/prove_loop_kernel_trace.txt).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))

from ring_zk_amd import Context  # noqa: E402
from ring_zk_amd import fiat_shamir as FS  # noqa: E402
from ring_zk_amd.backend import KeyedSampler, KeyedSampler32  # noqa: E402
from bench_packed import window  # noqa: E402

KEY = bytes(range(32))
NONCE0 = 1 << 20


def alternate_raw(variants, args):
    """name -> raw windows (us per batch), `repeats` of them, the variants alternated inside every round"""
    for fn in variants.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    iters = {name: max(args.iters, int(args.window_s * 1e6 / window(fn, args.iters)) + 1) for name, fn in variants.items()}
    ts = {name: [] for name in variants}
    for _ in range(args.repeats):
        for name, fn in variants.items():
            ts[name].append(window(fn, iters[name]))
    return ts


def readback_us(ctx, B, reps=200):
    """one round's read-back alone: the compaction launch on B flags, its count to the host, synchronise"""
    live = torch.ones(B, dtype=torch.uint8, device="cuda")
    done = torch.zeros(B, dtype=torch.uint8, device="cuda")
    for _ in range(10):
        ctx.debug_compact(live, done)[1].cpu()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        ctx.debug_compact(live, done)[1].cpu()
        ts.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(ts))


def shape_case(N, B, args):
    n, k, l = 1, 3, 1
    ctx = Context(N, n, k, l)
    ctx.generate_key(7)
    ctx.set_sampler_key(KEY)
    x = ctx.sample_uniform(1, 0, ctx.half, (B, l))
    x32 = ctx.narrow(x)
    ctx.synchronize()
    variants = {
        "python:w64": lambda: FS.open_prove_zk(ctx, x, KeyedSampler(ctx, KEY, NONCE0)),
        "python:w32": lambda: FS.open_prove_zk32(ctx, x32, KeyedSampler32(ctx, KEY, NONCE0)),
        "native:w64": lambda: FS.open_prove_zk_native(ctx, x, KeyedSampler(ctx, KEY, NONCE0)),
        "native:w32": lambda: FS.open_prove_zk_native(ctx, x32, KeyedSampler32(ctx, KEY, NONCE0)),
    }
    # the same proofs from all four
    outs = {name: fn() for name, fn in variants.items()}
    ctx.synchronize()
    for w in ("w64", "w32"):
        assert all(torch.equal(a, b) for a, b in zip(outs["native:" + w], outs["python:" + w])), (N, B, w)
    assert all(torch.equal(a.to(b.dtype), b) for a, b in zip(outs["native:w32"], outs["native:w64"]))
    assert bool(outs["native:w32"][3].all())
    rounds_run = int(outs["native:w32"][5].max()) + 1
    kernel_us = {}
    for w in ("w64", "w32"):
        ctx.prof_enable(True)
        ctx.prof_reset()
        variants["native:" + w]()
        ctx.synchronize()
        kernel_us[w] = round(sum(ctx.prof_read_all()), 1)
        ctx.prof_enable(False)
    ts = alternate_raw(variants, args)
    out = {"rounds_run": rounds_run, "readback_us": round(readback_us(ctx, B), 1)}
    for name, v in ts.items():
        out[name] = {"us": round(float(np.median(v)), 1), "us_min_max": [round(min(v), 1), round(max(v), 1)],
                     "windows_us": [round(t, 1) for t in v]}
    for w in ("w64", "w32"):
        nat, py = ts["native:" + w], ts["python:" + w]
        out["native_vs_python:" + w] = {
            "ratio": round(float(np.median(nat)) / float(np.median(py)), 3),
            "faster_in_every_window": bool(all(a < b for a, b in zip(nat, py))),
            "native_us_per_round": round(float(np.median(nat)) / rounds_run, 1),
            "python_us_per_round": round(float(np.median(py)) / rounds_run, 1),
            "native_kernel_us_sum": kernel_us[w],
        }
    ctx.close()
    return out


def trace_runs(N, B, runs=5):
    """`runs` native 32-bit calls of one shape and nothing else: the process to put behind
    `rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_prove_loop.py --trace-shape N,B`"""
    ctx = Context(N, 1, 3, 1)
    ctx.generate_key(7)
    x32 = ctx.narrow(ctx.sample_uniform(1, 0, ctx.half, (B, 1)))
    for _ in range(runs):
        out = FS.open_prove_zk_native(ctx, x32, KeyedSampler32(ctx, KEY, NONCE0))
    ctx.synchronize()
    print("rounds_run", int(out[5].max()) + 1, "runs", runs)


def summarise_trace(path, runs=5):
    """per kernel name of a rocprofv3 kernel-trace CSV: launches and microseconds per run, mean microseconds per launch"""
    import collections
    import csv
    import re

    dur, cnt = collections.defaultdict(float), collections.Counter()
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        nm = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").replace("rzk::", "")
        nm = re.sub(r"\(.*", "", nm)[:60]
        dur[nm] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        cnt[nm] += 1
    gaps = [(int(b["Start_Timestamp"]) - int(a["End_Timestamp"])) / 1e3 for a, b in zip(rows[:-1], rows[1:])]
    idle = sum(g for g in gaps if 0 < g < 200)   # (longer gaps lie between the runs and before the first)
    print("busy us per run %.1f   idle between kernels (gaps below 200 us) us per run %.1f" % (sum(dur.values()) / runs, idle / runs))
    for nm, d in sorted(dur.items(), key=lambda kv: -kv[1]):
        print("%-62s launches/run %6.1f  us/run %9.1f  us/launch %8.2f" % (nm, cnt[nm] / runs, d / runs, d / cnt[nm]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace-shape", default=None, help="N,B: run five native 32-bit calls of this shape and exit (for a kernel trace)")
    ap.add_argument("--summarise-trace", default=None, help="a rocprofv3 kernel-trace CSV of such a process: print its table and exit")
    ap.add_argument("--iters", type=int, default=3, help="least calls per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.2, help="least duration of a timed window")
    ap.add_argument("--batches", default="4096,64")
    ap.add_argument("--sizes", default="512,1024")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prove_loop_bench.json"))
    args = ap.parse_args()
    if args.summarise_trace:
        return summarise_trace(args.summarise_trace)
    assert torch.cuda.is_available(), "bench_prove_loop.py needs a GPU"
    if args.trace_shape:
        return trace_runs(*[int(v) for v in args.trace_shape.split(",")])
    out = {"repeats": args.repeats, "window_s": args.window_s}
    for B in [int(s) for s in args.batches.split(",")]:
        for N in [int(s) for s in args.sizes.split(",")]:
            out[f"open_n{N}_b{B}"] = shape_case(N, B, args)
    line = json.dumps(out)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
