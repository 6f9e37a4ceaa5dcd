#!/usr/bin/env python3
"""The Linear proof on 32-bit slabs beside its 64-bit siblings on the same values: one JSON line.

Shapes: Linear (1,3,1), B = 4096, N = 512 and 1024 (native 32-bit kernels) and N = 2048 (the
convert path, for the record).  Per shape, in ONE process: the six calls (commit, mask, response, response_reject, verify,
recover) in both widths on device tensors; the 32-bit inputs are made once by narrow(), outside the timed region, and the
32-bit outputs are asserted identical to narrow() of the siblings' before anything is timed.  After a warm-up of every
variant, --repeats rounds of alternated windows of at least --window-s seconds, device events around each window (the
method of tools/bench_slab32.py and tools/bench_packed.py).  Reported per call and width: median microseconds per batch,
the min-max spread of the windows, the rate on algorithmic bytes (slabs read + written at the call's width; the coin, the
verdict bytes and E are left out) and that rate over the plain device copy rate measured in the same process.

The yardstick of a 32-bit call is its 64-bit sibling in the same windows: `ratio` = 32-bit time / 64-bit time (below 1 =
faster); `disjoint` = the two sets of windows do not overlap; `above_sibling` = the 32-bit windows lie wholly above the
sibling's.
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
from ring_zk_amd.fiat_shamir import zk_lnm  # noqa: E402
from bench_packed import alternate, copy_rate, nbytes  # noqa: E402

R = 1 << 40


def kernels_of(ctx, call):
    ctx.prof_enable(True)
    ctx.prof_reset()
    call()
    names = [nm for nm, _ in ctx.prof_read_kernels()]
    ctx.prof_enable(False)
    return names


def shape_case(N, B, cr, args):
    n, k, l = 1, 3, 1
    ctx = Context(N, n, k, l)
    ctx.generate_key(7)
    g = ctx.sample_uniform(1, 0, ctx.half, (B,))
    x = ctx.sample_uniform(1, 1, ctx.half, (B, l))
    r, rp = ctx.sample_uniform(1, 2, ctx.b, (B, k)), ctx.sample_uniform(1, 3, ctx.b, (B, k))
    y, yp = ctx.sample_gauss(1, 4, float(ctx.sigma), (B, k)), ctx.sample_gauss(1, 5, float(ctx.sigma), (B, k))
    d = ctx.sample_challenge(1, 6, (B,))
    coin = ctx.sample_uniform(1, 7, (1 << 30) - 1, (B,))[:, 0].abs().contiguous()
    lnM = zk_lnm(2)
    c, cp, t, tp, u, ok = ctx.linear_commit(g, x, r, rp, y, yp)
    z, zp = ctx.linear_response(y, yp, r, rp, d)
    assert bool((ok == 3).all()) and bool(ctx.linear_verify(z, zp, c, cp, g, t, tp, u, d).all())
    g3, x3, r3, rp3, y3, yp3, d3, c3, cp3, t3, tp3, u3, z3, zp3 = (
        ctx.narrow(a) for a in (g, x, r, rp, y, yp, d, c, cp, t, tp, u, z, zp))
    ctx.synchronize()
    calls = {
        "commit": (lambda: ctx.linear_commit(g, x, r, rp, y, yp), lambda: ctx.linear_commit32(g3, x3, r3, rp3, y3, yp3),
                   [g, x, r, rp, y, yp, c, cp, t, tp, u]),
        "mask": (lambda: ctx.linear_mask(g, y, yp), lambda: ctx.linear_mask32(g3, y3, yp3), [g, y, yp, t, tp, u]),
        "response": (lambda: ctx.linear_response(y, yp, r, rp, d), lambda: ctx.linear_response32(y3, yp3, r3, rp3, d3),
                     [y, yp, r, rp, d, z, zp]),
        "response_reject": (lambda: ctx.linear_response_reject(y, yp, r, rp, d, coin, R, lnM),
                            lambda: ctx.linear_response_reject32(y3, yp3, r3, rp3, d3, coin, R, lnM), [y, yp, r, rp, d, z, zp]),
        "verify": (lambda: ctx.linear_verify(z, zp, c, cp, g, t, tp, u, d),
                   lambda: ctx.linear_verify32(z3, zp3, c3, cp3, g3, t3, tp3, u3, d3), [z, zp, c, cp, g, t, tp, u, d]),
        "recover": (lambda: ctx.linear_recover(z, zp, c, cp, g, d), lambda: ctx.linear_recover32(z3, zp3, c3, cp3, g3, d3),
                    [z, zp, c, cp, g, d, t, tp, u]),
    }
    # identical outputs before anything is timed: slabs as narrow() of the sibling's, verdict bytes and E as they are
    for name, (f64, f32, _) in calls.items():
        o64, o32 = f64(), f32()
        o64, o32 = (o if isinstance(o, tuple) else (o,) for o in (o64, o32))
        for a, b in zip(o64, o32):
            assert torch.equal(b, ctx.narrow(a) if b.dtype == torch.int32 else a), name
    ctx.synchronize()
    kernels = {name: kernels_of(ctx, f32) for name, (_, f32, _) in calls.items()}
    variants = {}
    for name, (f64, f32, _) in calls.items():
        variants[name + "64"] = f64
        variants[name + "32"] = f32
    us, span = alternate(variants, args)
    out = {"native": not any(nm in ("widen_kernel", "narrow_kernel") for ks in kernels.values() for nm in ks), "kernels32": kernels}
    for name, (_, _, slabs) in calls.items():
        b64 = nbytes(slabs)
        rec = {}
        for w, by in (("64", b64), ("32", b64 // 2)):
            tme = us[name + w]
            rec["w" + w] = {"us": round(tme, 1), "us_min_max": [round(v, 1) for v in span[name + w]], "bytes": by,
                            "GBs": round(by / tme / 1e3, 1), "of_copy": round(by / tme / 1e3 / cr, 3)}
        s64, s32 = span[name + "64"], span[name + "32"]
        rec["ratio"] = round(us[name + "32"] / us[name + "64"], 3)
        rec["disjoint"] = bool(s32[1] < s64[0] or s32[0] > s64[1])
        rec["above_sibling"] = bool(s32[0] > s64[1])
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear32_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_linear32.py needs a GPU"
    cr = copy_rate()
    out = {"copy_GBs": round(cr, 1), "repeats": args.repeats, "window_s": args.window_s, "batch": args.batch}
    for N in [int(s) for s in args.sizes.split(",")]:
        out[f"linear_n{N}"] = shape_case(N, args.batch, cr, args)
    line = json.dumps(out)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
