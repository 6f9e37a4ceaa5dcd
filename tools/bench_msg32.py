#!/usr/bin/env python3
"""The transcript hash, the packed codec and the short packed verifier on 32-bit slabs beside their 64-bit siblings on the
same values: one JSON line.

Shapes: Open (1,3,1), B = 4096, N = 512 and 1024.  Per shape, in ONE process: `challenge`, `packed.encode_batch` and
`packed.decode_batch` (MSG_OPEN_SHORT) and `fiat_shamir.open_verify_short_packed`, each in both widths on device tensors,
plus what a holder of 32-bit slabs pays without the 32-bit calls: widen -> 64-bit call -> narrow (`convert`).  The 32-bit
inputs are made once by narrow(), outside the timed region.  After a warm-up of every variant, --repeats rounds of
alternated windows of at least --window-s seconds, device events around each window (the method of
tools/bench_slab32.py).  Reported per call and variant: median microseconds per batch and the min-max spread of the
windows; per kernel: the median of the library's own per-launch events (rzk_prof_*) over --iters calls.

The yardstick of a 32-bit call is its 64-bit sibling in the same windows: `ratio` = 32-bit time / 64-bit time (below 1
= faster), `slower_than_spread` = the 32-bit median lies above the sibling's slowest window.
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

from ring_zk_amd import Context, packed, wire  # noqa: E402
from ring_zk_amd import fiat_shamir as FS  # noqa: E402
from bench_packed import alternate  # noqa: E402

KIND = packed.MSG_OPEN_SHORT


def kernel_medians(ctx, fn, iters):
    """name -> median microseconds of the launches `fn` makes, from the library's events"""
    ctx.prof_enable(True)
    per = {}
    for _ in range(iters):
        ctx.prof_reset()
        fn()
        ctx.synchronize()
        for us, (name, _) in zip(ctx.prof_read_all(), ctx.prof_read_kernels()):
            per.setdefault(name, []).append(us)
    ctx.prof_enable(False)
    return {name: round(float(np.median(v)) * len(v) / iters, 1) for name, v in per.items()}   # x launches per call


def shape_case(N, B, args):
    n, k, l = 1, 3, 1
    ctx = Context(N, n, k, l)
    ctx.generate_key(7)
    x = ctx.sample_uniform(1, 0, ctx.half, (B, l))
    r = ctx.sample_uniform(1, 1, ctx.b, (B, k))
    y = ctx.sample_gauss(1, 2, float(ctx.sigma), (B, k))
    c, t, z, ok = FS.open_prove(ctx, x, r, y)
    d = FS.open_short(ctx, c, t, z)
    rec, eok = packed.encode_batch(ctx, KIND, c, d, z)
    assert bool(ok.all()) and bool(eok.all()) and bool(FS.open_verify_short_packed(ctx, rec).all())
    c32, t32, z32, d32 = (ctx.narrow(a) for a in (c, t, z, d))
    ctx.synchronize()
    # the 32-bit calls compute the same thing
    dd, dig32, _ = FS.challenge32(ctx, wire.MSG_OPEN_COMMITMENT, c32, t32)
    _, dig64, _ = FS.challenge(ctx, wire.MSG_OPEN_COMMITMENT, c, t)
    assert torch.equal(dd, d32) and torch.equal(dig32, dig64)
    assert torch.equal(packed.encode_batch32(ctx, KIND, c32, d32, z32)[0], rec)
    assert all(torch.equal(a, b) for a, b in zip(packed.decode_batch32(ctx, KIND, rec)[:-1], (c32, d32, z32)))
    assert bool(FS.open_verify_short_packed32(ctx, rec).all())

    def challenge_convert():
        dw, _, okw = FS.challenge(ctx, wire.MSG_OPEN_COMMITMENT, ctx.widen(c32), ctx.widen(t32))
        return ctx.narrow(dw), okw

    def decode_convert():
        cw, dw, zw, okw = packed.decode_batch(ctx, KIND, rec)
        return ctx.narrow(cw), ctx.narrow(dw), ctx.narrow(zw), okw

    calls = {
        "challenge": (lambda: FS.challenge(ctx, wire.MSG_OPEN_COMMITMENT, c, t),
                      lambda: FS.challenge32(ctx, wire.MSG_OPEN_COMMITMENT, c32, t32), challenge_convert),
        "encode": (lambda: packed.encode_batch(ctx, KIND, c, d, z), lambda: packed.encode_batch32(ctx, KIND, c32, d32, z32),
                   lambda: packed.encode_batch(ctx, KIND, ctx.widen(c32), ctx.widen(d32), ctx.widen(z32))),
        "decode": (lambda: packed.decode_batch(ctx, KIND, rec), lambda: packed.decode_batch32(ctx, KIND, rec), decode_convert),
        "verify_short_packed": (lambda: FS.open_verify_short_packed(ctx, rec), lambda: FS.open_verify_short_packed32(ctx, rec), None),
    }
    variants = {}
    for name, (f64, f32, fcv) in calls.items():
        variants[name + "64"] = f64
        variants[name + "32"] = f32
        if fcv:
            variants[name + "_convert"] = fcv
    us, span = alternate(variants, args)
    out = {"record_bytes": int(rec.shape[1])}
    for name, (f64, f32, fcv) in calls.items():
        res = {}
        for w in ("64", "32") + (("_convert",) if fcv else ()):
            res["w" + w if w != "_convert" else "convert"] = {"us": round(us[name + w], 1), "us_min_max": [round(v, 1) for v in span[name + w]]}
        res["ratio"] = round(us[name + "32"] / us[name + "64"], 3)
        res["slower_than_spread"] = bool(us[name + "32"] > span[name + "64"][1])
        if fcv:
            res["ratio_over_convert"] = round(us[name + "32"] / us[name + "_convert"], 3)
        res["kernels64_us"] = kernel_medians(ctx, f64, args.iters)
        res["kernels32_us"] = kernel_medians(ctx, f32, args.iters)
        out[name] = res
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5, help="least launches per timed window; calls per kernel median")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.2, help="least duration of a timed window")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--sizes", default="512,1024")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msg32_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_msg32.py needs a GPU"
    out = {"repeats": args.repeats, "window_s": args.window_s, "batch": args.batch}
    for N in [int(s) for s in args.sizes.split(",")]:
        out[f"open_n{N}"] = shape_case(N, args.batch, args)
    line = json.dumps(out)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
