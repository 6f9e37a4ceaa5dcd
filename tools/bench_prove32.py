#!/usr/bin/env python3
"""The zero-knowledge Open prover on 32-bit slabs beside its 64-bit siblings on the same key and nonces: one JSON line.

Shapes: Open (1,3,1), B = 4096, N = 512 and 1024.  Per shape, in ONE process, on device tensors: the four keyed samplers
(uniform(b), gauss(sigma), dgauss(sigma), challenge), matvec(KEY_A1), open_response_reject and the whole open_prove_zk, each
in three variants: the 64-bit call ("w64"), the 32-bit call ("w32") and what a slab32 holder paid before the 32-bit call
existed ("convert": the 64-bit call followed by narrow of its slab outputs; the prover also widens x first).  After a warm-up
of every variant, --repeats rounds of alternated windows of at least --window-s seconds, device events around each window
(the method of tools/bench_slab32.py).  Reported per call and variant: median microseconds per batch and the min-max
spread of the windows.

The yardstick of a 32-bit call is its 64-bit sibling in the same windows: `ratio` = 32-bit time / 64-bit time (below 1 =
faster), `slower_than_spread` = the 32-bit median lies above the sibling's slowest window, `faster_in_every_window` = the
slowest 32-bit window lies below the sibling's fastest; `ratio_convert` = 32-bit time / convert time.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))

from ring_zk_amd import Context, _lib  # noqa: E402
from ring_zk_amd import fiat_shamir as FS  # noqa: E402
from ring_zk_amd.backend import KeyedSampler, KeyedSampler32  # noqa: E402
from bench_packed import alternate  # noqa: E402

KEY = bytes(range(32))
NONCE = (5).to_bytes(16, "little")
NONCE0 = 1 << 20


def shape_case(N, B, args):
    n, k, l = 1, 3, 1
    ctx = Context(N, n, k, l)
    ctx.generate_key(7)
    ctx.set_sampler_key(KEY)
    sigma, lnM, R = int(ctx.sigma), FS.zk_lnm(1), FS.COIN_R0 * FS.COIN_R0
    x = ctx.sample_uniform(1, 0, ctx.half, (B, l))
    r = ctx.sample_uniform_keyed(NONCE, 1, ctx.b, (B, k))
    y = ctx.sample_gauss_keyed(NONCE, 2, float(sigma), (B, k))
    d = ctx.sample_challenge_keyed(NONCE, 3, (B,))
    coin, _ = FS.draw_coins(KeyedSampler(ctx, KEY, 9), (B,))
    x32, r32, y32, d32 = (ctx.narrow(a) for a in (x, r, y, d))
    ctx.synchronize()
    nar = ctx.narrow

    def prove64():
        return FS.open_prove_zk(ctx, x, KeyedSampler(ctx, KEY, NONCE0))

    def prove32():
        return FS.open_prove_zk32(ctx, x32, KeyedSampler32(ctx, KEY, NONCE0))

    def prove_convert():
        c, t, z, ok, rr, rounds = FS.open_prove_zk(ctx, ctx.widen(x32), KeyedSampler(ctx, KEY, NONCE0))
        return nar(c), nar(t), nar(z), ok, nar(rr), rounds

    calls = {   # name -> (64-bit call returning its slab outputs first, 32-bit call, number of slab outputs to narrow)
        "uniform": (lambda: (ctx.sample_uniform_keyed(NONCE, 1, ctx.b, (B, k)),),
                    lambda: (ctx.sample_uniform_keyed32(NONCE, 1, ctx.b, (B, k)),), 1),
        "gauss": (lambda: (ctx.sample_gauss_keyed(NONCE, 2, float(sigma), (B, k)),),
                  lambda: (ctx.sample_gauss_keyed32(NONCE, 2, float(sigma), (B, k)),), 1),
        "dgauss": (lambda: (ctx.sample_dgauss_keyed(NONCE, 2, sigma, (B, k)),),
                   lambda: (ctx.sample_dgauss_keyed32(NONCE, 2, sigma, (B, k)),), 1),
        "challenge": (lambda: (ctx.sample_challenge_keyed(NONCE, 3, (B,)),),
                      lambda: (ctx.sample_challenge_keyed32(NONCE, 3, (B,)),), 1),
        "matvec_a1": (lambda: (ctx.matvec(_lib.KEY_A1, y),), lambda: (ctx.matvec32(_lib.KEY_A1, y32),), 1),
        "response_reject": (lambda: ctx.open_response_reject(y, r, d, coin, R, lnM),
                            lambda: ctx.open_response_reject32(y32, r32, d32, coin, R, lnM), 1),
    }
    # the 32-bit calls compute the same thing
    for name, (f64, f32, nslab) in calls.items():
        o64, o32 = f64(), f32()
        assert all(torch.equal(a.to(b.dtype), b) for a, b in zip(o32, o64)), name
    p64, p32 = prove64(), prove32()
    assert all(torch.equal(a.to(b.dtype), b) for a, b in zip(p32, p64)) and bool(p32[3].all())
    ctx.prof_enable(True)
    ctx.prof_reset()
    prove32()
    ctx.synchronize()
    kernels = sorted({nm for nm, _ in ctx.prof_read_kernels()})
    ctx.prof_enable(False)
    variants = {}
    for name, (f64, f32, nslab) in calls.items():
        variants[name + ":w64"] = f64
        variants[name + ":w32"] = f32
        variants[name + ":convert"] = lambda f64=f64, nslab=nslab: [nar(a) for a in f64()[:nslab]]
    variants.update({"open_prove_zk:w64": prove64, "open_prove_zk:w32": prove32, "open_prove_zk:convert": prove_convert})
    us, span = alternate(variants, args)
    out = {"rounds_max": int(p32[5].max()), "prove32_kernels": kernels,
           "native": not any(nm in ("widen_kernel", "narrow_kernel") for nm in kernels)}
    for name in list(calls) + ["open_prove_zk"]:
        rec = {w: {"us": round(us[name + ":" + w], 1), "us_min_max": [round(v, 1) for v in span[name + ":" + w]]}
               for w in ("w64", "w32", "convert")}
        rec["ratio"] = round(us[name + ":w32"] / us[name + ":w64"], 3)
        rec["ratio_convert"] = round(us[name + ":w32"] / us[name + ":convert"], 3)
        rec["slower_than_spread"] = bool(us[name + ":w32"] > span[name + ":w64"][1])
        rec["faster_in_every_window"] = bool(span[name + ":w32"][1] < span[name + ":w64"][0])
        out[name] = rec
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3, help="least launches per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.2, help="least duration of a timed window")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--sizes", default="512,1024")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prove32_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_prove32.py needs a GPU"
    out = {"repeats": args.repeats, "window_s": args.window_s, "batch": args.batch}
    for N in [int(s) for s in args.sizes.split(",")]:
        out[f"open_n{N}"] = shape_case(N, args.batch, args)
    line = json.dumps(out)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
