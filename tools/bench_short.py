#!/usr/bin/env python3
"""Short (signature-form) verifiers beside the full Fiat-Shamir verifiers of the same proofs: one JSON line.

Cases, all on device tensors: Open N=1024 (1,3,1) B=4096; Linear N=1024 (1,3,1) B=4096; Sum N=1024 (4,9,4) V=8 B=512.
Per case, in ONE process and in alternated windows (the method of tools/bench_packed.py: after a warm-up of every
variant, --repeats rounds that time each variant once, device events around each window):
  * `short`: *_verify_short (recover, transcript hash under the full commitment kind, compare);
  * `full`: *_verify on the full proof (transcript hash, verifier);
  * Open only, `composed`: the short verifier as a composition of Mat-level calls (three canonicalize, matvec, cmul, sub,
    the hash, eq, open_verify), which is what open_verify_short was before it was re-based on open_recover;
  * the record sizes of both encodings.
`--tree DIR` imports the package from another checkout (the parent commit's, built there) and `--open-only` times only
what every tree has — FS.open_verify_short and FS.open_verify — so that two trees can be run by turns in one session.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters   # us per batch


def alternate(variants, args):
    """variants: name -> fn.  Median and (min, max) microseconds per batch of every variant over alternated windows."""
    for fn in variants.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    iters = {name: max(args.iters, int(args.window_s * 1e6 / window(fn, args.iters)) + 1) for name, fn in variants.items()}
    ts = {name: [] for name in variants}
    for _ in range(args.repeats):
        for name, fn in variants.items():
            ts[name].append(window(fn, iters[name]))
    return {name: {"us": round(float(np.median(v)), 1), "us_min_max": [round(min(v), 1), round(max(v), 1)]} for name, v in ts.items()}


def ratios(res, B):
    res["short_over_full"] = round(res["short"]["us"] / res["full"]["us"], 3)
    res["short_proofs_per_s"] = round(B / res["short"]["us"] * 1e6)
    return res


def open_case(mods, args):
    Context, FS, packed, KEY_A1 = mods
    N, n, k, l, B = 1024, 1, 3, 1, 4096
    ctx = Context(N, n, k, l)
    ctx.generate_key(7)
    x = ctx.sample_uniform(1, 0, ctx.half, (B, l))
    r = ctx.sample_uniform(1, 1, ctx.b, (B, k))
    y = ctx.sample_gauss(1, 2, ctx.sigma, (B, k))
    c, t, z, _ = FS.open_prove(ctx, x, r, y)
    d = FS.open_short(ctx, c, t, z)

    def composed():
        zc, cc, dc = ctx.canonicalize(z), ctx.canonicalize(c), ctx.canonicalize(d)
        t2 = ctx.sub(ctx.matvec(KEY_A1, zc), ctx.cmul(cc[:, :n].contiguous(), dc))
        d2, _, okf = FS.challenge(ctx, packed.MSG_OPEN_COMMITMENT, c, t2)
        same = ctx.eq(d2.reshape(-1, 1, N), dc.reshape(-1, 1, N))
        return ctx.open_verify(z, t2, c, d) & same & okf

    variants = {"short": lambda: FS.open_verify_short(ctx, c, d, z), "full": lambda: FS.open_verify(ctx, c, t, z)}
    if not args.open_only:
        variants["composed"] = composed
    for fn in variants.values():
        assert bool((fn() == 1).all())
    res = ratios(alternate(variants, args), B)
    if "composed" in res:
        res["short_over_composed"] = round(res["short"]["us"] / res["composed"]["us"], 3)
    res["bytes"] = {"short": packed.record_bytes(ctx, packed.MSG_OPEN_SHORT),
                    "full": packed.record_bytes(ctx, packed.MSG_OPEN_COMMITMENT) + packed.record_bytes(ctx, packed.MSG_OPEN_RESPONSE)}
    ctx.close()
    return res


def linear_case(mods, args):
    Context, FS, packed, _ = mods
    N, n, k, l, B = 1024, 1, 3, 1, 4096
    ctx = Context(N, n, k, l)
    ctx.generate_key(8)
    g, x = ctx.sample_uniform(2, 0, ctx.half, (B,)), ctx.sample_uniform(2, 1, ctx.half, (B, l))
    r, rp = ctx.sample_uniform(2, 2, ctx.b, (B, k)), ctx.sample_uniform(2, 3, ctx.b, (B, k))
    y, yp = ctx.sample_gauss(2, 4, ctx.sigma, (B, k)), ctx.sample_gauss(2, 5, ctx.sigma, (B, k))
    c, cp, t, tp, u, z, zp, _ = FS.linear_prove(ctx, g, x, r, rp, y, yp)
    d = FS.linear_short(ctx, c, cp, g, t, tp, u, z, zp)
    variants = {"short": lambda: FS.linear_verify_short(ctx, c, cp, g, d, z, zp),
                "full": lambda: FS.linear_verify(ctx, c, cp, g, t, tp, u, z, zp)}
    for fn in variants.values():
        assert bool((fn() == 1).all())
    res = ratios(alternate(variants, args), B)
    res["bytes"] = {"short": packed.record_bytes(ctx, packed.MSG_LINEAR_SHORT),
                    "full": packed.record_bytes(ctx, packed.MSG_LINEAR_COMMITMENT) + packed.record_bytes(ctx, packed.MSG_LINEAR_RESPONSE)}
    ctx.close()
    return res


def sum_case(mods, args):
    Context, FS, packed, _ = mods
    N, n, k, l, V, B = 1024, 4, 9, 4, 8, 512
    ctx = Context(N, n, k, l)
    ctx.generate_key(9)
    gs, xs = ctx.sample_uniform(3, 0, ctx.half, (B, V)), ctx.sample_uniform(3, 1, ctx.half, (B, V, l))
    rs, rp = ctx.sample_uniform(3, 2, ctx.b, (B, V, k)), ctx.sample_uniform(3, 3, ctx.b, (B, k))
    ys, yp = ctx.sample_gauss(3, 4, ctx.sigma, (B, V, k)), ctx.sample_gauss(3, 5, ctx.sigma, (B, k))
    cs, cp, ts, tp, u, zs, zp, _ = FS.sum_prove(ctx, gs, xs, rs, rp, ys, yp)
    d = FS.sum_short(ctx, cs, cp, gs, ts, tp, u, zs, zp)
    variants = {"short": lambda: FS.sum_verify_short(ctx, cs, cp, gs, d, zs, zp),
                "full": lambda: FS.sum_verify(ctx, cs, cp, gs, ts, tp, u, zs, zp)}
    for fn in variants.values():
        assert bool((fn() == 1).all())
    res = ratios(alternate(variants, args), B)
    res["bytes"] = {"short": packed.record_bytes(ctx, packed.MSG_SUM_SHORT, V),
                    "full": packed.record_bytes(ctx, packed.MSG_SUM_COMMITMENT, V) + packed.record_bytes(ctx, packed.MSG_SUM_RESPONSE, V)}
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3, help="least calls per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.2, help="least duration of a timed window")
    ap.add_argument("--tree", default=ROOT, help="checkout whose ring_zk_amd package (and built library) is measured")
    ap.add_argument("--open-only", action="store_true", help="only FS.open_verify_short and FS.open_verify (any tree has them)")
    ap.add_argument("--out", default=None, help="also write the line here (default: profiles/short_bench.json unless --open-only)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_short.py needs a GPU"
    sys.path.insert(0, os.path.abspath(args.tree))
    from ring_zk_amd import Context, packed
    from ring_zk_amd import fiat_shamir as FS
    from ring_zk_amd._lib import KEY_A1

    mods = (Context, FS, packed, KEY_A1)
    out = {"tree": os.path.relpath(os.path.abspath(args.tree), ROOT), "repeats": args.repeats, "window_s": args.window_s,
           "open_n1024_b4096": open_case(mods, args)}
    if not args.open_only:
        out["linear_n1024_b4096"] = linear_case(mods, args)
        out["sum_n1024_494_v8_b512"] = sum_case(mods, args)
    line = json.dumps(out)
    path = args.out or (None if args.open_only else os.path.join(ROOT, "profiles", "short_bench.json"))
    if path:
        with open(path, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
