#!/usr/bin/env python3
"""XP1 seed expansion (rzk_xof_uniform_batch_dev) beside the two statistical / keyed uniform samplers: one JSON line.

For N in {512, 1024, 2048}, 32 768 polynomials per launch (B = 1024 seeds x 32 rows): output GB/s and polynomials/s of
  * xof        rzk_xof_uniform_batch_dev (SHAKE256, exactly uniform residues, public seeds);
  * philox     rzk_sample_uniform_dev over the full centred range (the statistical generator), as context;
  * chacha20   rzk_sample_uniform_keyed_dev over the same range (the keyed generator), as context.
All three write the same 8 N bytes per polynomial.  Per case, in ONE process and in alternated windows (the method of
tools/bench_fs.py: after a warm-up of every variant, --repeats rounds that time each variant once, device events around
each window); the median is reported with the smallest and largest window.  No figure is a pass condition.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ring_zk_amd import Context  # noqa: E402

SEEDS, ROWS = 1024, 32


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters   # us per launch


def case(N, args):
    ctx = Context(N)
    ctx.set_sampler_key(bytes(range(32)))
    ctx._bind_torch_stream()
    polys = SEEDS * ROWS
    seeds = torch.from_numpy(np.random.default_rng(N).integers(0, 256, (SEEDS, 32), dtype=np.uint8)).cuda()
    out = torch.empty((SEEDS, ROWS, N), dtype=torch.int64, device="cuda")
    L, h, op = ctx._L, ctx._h, C.c_void_p(out.data_ptr())
    nonce = (C.c_uint8 * 16)()

    def check(st):
        assert st == 0, L.rzk_last_error(h).decode()

    variants = {
        "xof": lambda: check(L.rzk_xof_uniform_batch_dev(h, C.c_void_p(seeds.data_ptr()), 1, ROWS, op, SEEDS)),
        "philox": lambda: check(L.rzk_sample_uniform_dev(h, 1, 0, ctx.half, op, polys)),
        "chacha20": lambda: check(L.rzk_sample_uniform_keyed_dev(h, nonce, 0, ctx.half, op, polys)),
    }
    for fn in variants.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    iters = {name: max(args.iters, int(args.window_s * 1e6 / window(fn, args.iters)) + 1) for name, fn in variants.items()}
    ts = {name: [] for name in variants}
    for _ in range(args.repeats):
        for name, fn in variants.items():
            ts[name].append(window(fn, iters[name]))
    res = {"polys": polys, "bytes": polys * N * 8}
    for name, v in ts.items():
        us = float(np.median(v))
        res[name] = {"us": round(us, 1), "us_min_max": [round(min(v), 1), round(max(v), 1)],
                     "GBs": round(polys * N * 8 / us / 1e3, 1), "Mpolys_per_s": round(polys / us, 3)}
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3, help="least launches per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.2, help="least duration of a timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xof_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_xof.py needs a GPU"
    out = {"repeats": args.repeats, "window_s": args.window_s}
    for N in (512, 1024, 2048):
        out[f"n{N}"] = case(N, args)
    line = json.dumps(out)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
