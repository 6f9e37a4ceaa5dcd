#!/usr/bin/env python3
"""The zero-knowledge Linear and Sum provers with their loop in Python (fiat_shamir.linear_prove_zk / sum_prove_zk, unchanged
code) beside the same provers with the loop inside the library (linear_prove_zk_native / sum_prove_zk_native), and the mask
calls beside the commit calls: one JSON line.  The pattern of tools/bench_prove_loop.py.

Shapes: Linear (1,3,1) at N = 512 and 1024, B = 64 and 4096; Sum V = 2 (1,3,1) at N = 1024, B = 64 and 1024.  Per shape, in
ONE process, on device tensors, the variants python and native draw under the same key and first nonce, so both run the same
rounds on the same pending sets and return the same proofs (asserted before anything is timed).  After a warm-up of every
variant, --repeats rounds of alternated windows of at least --window-s seconds, device events around each window.  Reported
per variant: median microseconds per call, the min-max spread and the raw windows.

The yardstick of the native call is the Python loop in the same round of windows: `ratio` = native median / Python median;
`below_median` = the condition of DESIGN.md section 21, native median below Python median; `slowest_native_below_fastest_python`
says whether the two sets of windows are disjoint.  At the largest B of a row the mask call is timed against the commit
call in the same way (`mask_vs_commit`).  Where the native time goes kernel by kernel is a trace's business: --trace-shape
under a kernel trace.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))

from ring_zk_amd import Context  # noqa: E402
from ring_zk_amd import fiat_shamir as FS  # noqa: E402
from ring_zk_amd.backend import KeyedSampler  # noqa: E402
from bench_prove_loop import alternate_raw  # noqa: E402

KEY = bytes(range(32))
NONCE0 = 1 << 20


def stats(v):
    return {"us": round(float(np.median(v)), 1), "us_min_max": [round(min(v), 1), round(max(v), 1)], "windows_us": [round(t, 1) for t in v]}


def make(N, B, V):
    ctx = Context(N, 1, 3, 1)
    ctx.generate_key(7)
    ctx.set_sampler_key(KEY)
    lead = (B,) if V is None else (B, V)
    g = ctx.sample_uniform(1, 0, ctx.half, lead)
    x = ctx.sample_uniform(2, 0, ctx.half, lead + (ctx.l,))
    ctx.synchronize()
    return ctx, g, x


def provers(ctx, g, x, V):
    if V is None:
        return {"python": lambda: FS.linear_prove_zk(ctx, g, x, KeyedSampler(ctx, KEY, NONCE0)),
                "native": lambda: FS.linear_prove_zk_native(ctx, g, x, KeyedSampler(ctx, KEY, NONCE0))}
    return {"python": lambda: FS.sum_prove_zk(ctx, g, x, KeyedSampler(ctx, KEY, NONCE0)),
            "native": lambda: FS.sum_prove_zk_native(ctx, g, x, KeyedSampler(ctx, KEY, NONCE0))}


def shape_case(N, B, V, with_masks, args):
    ctx, g, x = make(N, B, V)
    variants = provers(ctx, g, x, V)
    outs = {name: fn() for name, fn in variants.items()}
    ctx.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs["native"], outs["python"])), (N, B, V)   # identical proofs
    accepted = int(outs["native"][7].sum())
    rounds_run = int(outs["native"][10].max()) + 1
    ctx.prof_enable(True)
    ctx.prof_reset()
    variants["native"]()
    ctx.synchronize()
    kernel_us = round(sum(ctx.prof_read_all()), 1)
    ctx.prof_enable(False)
    ts = alternate_raw(variants, args)
    nat, py = ts["native"], ts["python"]
    out = {"rounds_run": rounds_run, "accepted": accepted, "python": stats(py), "native": stats(nat),
           "native_vs_python": {"ratio": round(float(np.median(nat)) / float(np.median(py)), 3),
                                "below_median": bool(np.median(nat) < np.median(py)),
                                "faster_in_every_window": bool(all(a < b for a, b in zip(nat, py))),
                                "slowest_native_below_fastest_python": bool(max(nat) < min(py)),
                                "native_kernel_us_sum": kernel_us}}
    if with_masks:
        k = ctx.k
        lead = (B,) if V is None else (B, V)
        r, rp = ctx.sample_uniform(3, 0, ctx.b, lead + (k,)), ctx.sample_uniform(4, 0, ctx.b, (B, k))
        y, yp = ctx.sample_gauss(5, 0, ctx.sigma, lead + (k,)), ctx.sample_gauss(6, 0, ctx.sigma, (B, k))
        ctx.synchronize()
        if V is None:
            calls = {"commit": lambda: ctx.linear_commit(g, x, r, rp, y, yp), "mask": lambda: ctx.linear_mask(g, y, yp)}
        else:
            calls = {"commit": lambda: ctx.sum_commit(g, x, r, rp, y, yp), "mask": lambda: ctx.sum_mask(g, y, yp)}
        full, part = calls["commit"](), calls["mask"]()
        ctx.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(part, full[2:5])), (N, B, V)              # the same t, tp, u
        tm = alternate_raw(calls, args)
        out["commit"], out["mask"] = stats(tm["commit"]), stats(tm["mask"])
        out["mask_vs_commit"] = {"ratio": round(float(np.median(tm["mask"])) / float(np.median(tm["commit"])), 3),
                                 "faster_in_every_window": bool(all(a < b for a, b in zip(tm["mask"], tm["commit"])))}
    ctx.close()
    return out


def trace_runs(kind, N, B, runs=5):
    """`runs` native calls of one shape and nothing else: the process to put behind a kernel trace"""
    V = None if kind == "linear" else 2
    ctx, g, x = make(N, B, V)
    fn = provers(ctx, g, x, V)["native"]
    for _ in range(runs):
        out = fn()
    ctx.synchronize()
    print("rounds_run", int(out[10].max()) + 1, "runs", runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace-shape", default=None, help="linear|sum,N,B: run five native calls of this shape and exit (for a kernel trace)")
    ap.add_argument("--iters", type=int, default=3, help="least calls per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.2, help="least duration of a timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prove_loop_lin_sum_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_prove_loop_lin_sum.py needs a GPU"
    if args.trace_shape:
        kind, N, B = args.trace_shape.split(",")
        return trace_runs(kind, int(N), int(B))
    out = {"repeats": args.repeats, "window_s": args.window_s}
    for N in (512, 1024):
        for B in (64, 4096):
            out[f"linear_n{N}_b{B}"] = shape_case(N, B, None, B == 4096, args)
    for B in (64, 1024):
        out[f"sum_v2_n1024_b{B}"] = shape_case(1024, B, 2, B == 1024, args)
    line = json.dumps(out)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
