#!/usr/bin/env python3
"""The Open cycle on 32-bit slabs beside its 64-bit siblings on the same values: one JSON line.

Shapes: Open (1,3,1), B = 4096, N = 512 and 1024 (native 32-bit kernels) and N = 2048 (the convert path, for the
record).  Per shape, in ONE process: the four calls (commit, response, verify, recover) in both widths on device
tensors; the 32-bit inputs are made once by narrow(), outside the timed region.  After a warm-up of every variant,
--repeats rounds of alternated windows of at least --window-s seconds, device events around each window (the method of
tools/bench_packed.py).  Reported per call and width: median microseconds per batch, the min-max spread of the windows,
the rate on algorithmic bytes (slabs read + written at the call's width) and that rate over the plain device copy rate
measured in the same process (the method of tools/copy_rate.py).

The yardstick of a 32-bit call is its 64-bit sibling in the same windows: `ratio` = 32-bit time / 64-bit time (below 1
= faster), `slower_than_spread` = the 32-bit median lies above the sibling's slowest window.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))

from ring_zk_amd import Context  # noqa: E402
from bench_packed import alternate, copy_rate, nbytes  # noqa: E402


def shape_case(N, B, cr, args):
    n, k, l = 1, 3, 1
    ctx = Context(N, n, k, l)
    ctx.generate_key(7)
    x = ctx.sample_uniform(1, 0, ctx.half, (B, l))
    r = ctx.sample_uniform(1, 1, ctx.b, (B, k))
    y = ctx.sample_gauss(1, 2, float(ctx.sigma), (B, k))
    d = ctx.sample_challenge(1, 3, (B,))
    c, t, ok = ctx.open_commit(x, r, y)
    z = ctx.open_response(y, r, d)
    assert bool(ok.all()) and bool(ctx.open_verify(z, t, c, d).all())
    x32, r32, y32, d32, c32, t32, z32 = (ctx.narrow(a) for a in (x, r, y, d, c, t, z))
    ctx.synchronize()
    # the 32-bit calls compute the same thing
    cc, tt, _ = ctx.open_commit32(x32, r32, y32)
    assert torch.equal(cc, c32) and torch.equal(tt, t32) and torch.equal(ctx.open_response32(y32, r32, d32), z32)
    assert bool(ctx.open_verify32(z32, t32, c32, d32).all()) and torch.equal(ctx.open_recover32(z32, c32, d32)[0], t32)
    ctx.prof_enable(True)
    ctx.prof_reset()
    ctx.open_verify32(z32, t32, c32, d32)
    kernels = [nm for nm, _ in ctx.prof_read_kernels()]
    ctx.prof_enable(False)
    calls = {
        "commit": (lambda: ctx.open_commit(x, r, y), lambda: ctx.open_commit32(x32, r32, y32), [x, r, y, c, t]),
        "response": (lambda: ctx.open_response(y, r, d), lambda: ctx.open_response32(y32, r32, d32), [y, r, d, z]),
        "verify": (lambda: ctx.open_verify(z, t, c, d), lambda: ctx.open_verify32(z32, t32, c32, d32), [z, t, c[:, :n], d]),
        "recover": (lambda: ctx.open_recover(z, c, d), lambda: ctx.open_recover32(z32, c32, d32), [z, c[:, :n], d, t]),
    }
    variants = {}
    for name, (f64, f32, _) in calls.items():
        variants[name + "64"] = f64
        variants[name + "32"] = f32
    us, span = alternate(variants, args)
    out = {"native": all(nm.endswith("i32>") for nm in kernels), "verify32_kernels": kernels}
    for name, (_, _, slabs) in calls.items():
        b64 = nbytes(slabs)
        rec = {}
        for w, by in (("64", b64), ("32", b64 // 2)):
            tme = us[name + w]
            rec["w" + w] = {"us": round(tme, 1), "us_min_max": [round(v, 1) for v in span[name + w]], "bytes": by,
                            "GBs": round(by / tme / 1e3, 1), "of_copy": round(by / tme / 1e3 / cr, 3)}
        rec["ratio"] = round(us[name + "32"] / us[name + "64"], 3)
        rec["slower_than_spread"] = bool(us[name + "32"] > span[name + "64"][1])
        out[name] = rec
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3, help="least launches per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.2, help="least duration of a timed window")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--sizes", default="512,1024,2048")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slab32_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_slab32.py needs a GPU"
    cr = copy_rate()
    out = {"copy_GBs": round(cr, 1), "repeats": args.repeats, "window_s": args.window_s, "batch": args.batch}
    for N in [int(s) for s in args.sizes.split(",")]:
        out[f"open_n{N}"] = shape_case(N, args.batch, cr, args)
    line = json.dumps(out)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
