#!/usr/bin/env python3
"""Packed records (rzk_packed_{encode,decode}_batch_dev) beside the bincode codec on the same slabs: one JSON line.

Cases: Open N=1024 (1,3,1) B=4096 — commitment { c, t }, response { z } and the short proof { c, d, z } — and one
config-5 chunk (Sum N=2048 (8,17,8) V=32, 512 proofs; commitment and response).  Per case, in ONE process and in
alternated windows (the method of tools/bench_fs.py: after a warm-up of every variant, --repeats rounds that time each
variant once, device events around each window):
  * packed encode and decode: microseconds per batch and GB/s of records + slabs;
  * the baselines on the same slabs: bincode encode and decode at coef_bytes 8 and 4 (for the short proof, which
    has no bincode kind, the three messages Commitment, Challenge and OpenProofResponse that carry the same fields);
  * the plain device copy rate (the method of tools/copy_rate.py: torch copy_ of 1 GiB) and each rate over it.
The yardstick is bincode at 8 bytes: `packed_over_bincode8` is packed time / bincode time per batch (below 1 = faster).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ring_zk_amd import Context, packed, wire  # noqa: E402
from ring_zk_amd import fiat_shamir as FS  # noqa: E402


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters   # us per batch


def copy_rate():
    n = 1024 * 1024 * 1024 // 8
    a = torch.empty(n, dtype=torch.int64, device="cuda").random_()
    b = torch.empty_like(a)
    for _ in range(5):
        b.copy_(a)
    torch.cuda.synchronize()
    us = float(np.median([window(lambda: b.copy_(a), 1) for _ in range(20)]))
    del a, b
    return 2 * n * 8 / us / 1e3   # GB/s read + write


def nbytes(ts):
    return sum(int(t.numel()) * t.element_size() for t in ts)


def alternate(variants, args):
    """variants: name -> fn.  Median microseconds per batch of every variant over alternated windows."""
    for fn in variants.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    iters = {name: max(args.iters, int(args.window_s * 1e6 / window(fn, args.iters)) + 1) for name, fn in variants.items()}
    ts = {name: [] for name in variants}
    for _ in range(args.repeats):
        for name, fn in variants.items():
            ts[name].append(window(fn, iters[name]))
    return {name: float(np.median(v)) for name, v in ts.items()}, {name: [min(v), max(v)] for name, v in ts.items()}


def codec_case(ctx, pkind, slabs, bincode_msgs, V, cr, args):
    """pkind: the packed kind of `slabs`; bincode_msgs: [(bincode kind, slabs of that message)] carrying the same fields."""
    rec, ok = packed.encode_batch(ctx, pkind, *slabs, V=V)
    assert bool((ok == 1).all()), "a benchmark message does not fit the packed format"
    back = packed.decode_batch(ctx, pkind, rec, V=V)
    assert bool((back[-1] == 1).all()) and all(torch.equal(a, b) for a, b in zip(back[:-1], slabs))
    wired = {cb: [wire.encode_batch(ctx, k, *s, V=V, coef_bytes=cb) for k, s in bincode_msgs] for cb in (8, 4)}
    variants = {
        "packed_encode": lambda: packed.encode_batch(ctx, pkind, *slabs, V=V),
        "packed_decode": lambda: packed.decode_batch(ctx, pkind, rec, V=V),
    }
    for cb in (8, 4):
        variants[f"bincode{cb}_encode"] = lambda cb=cb: [wire.encode_batch(ctx, k, *s, V=V, coef_bytes=cb) for k, s in bincode_msgs]
        variants[f"bincode{cb}_decode"] = lambda cb=cb: [wire.decode_batch(ctx, k, *m, V=V, coef_bytes=cb)
                                                         for (k, _), m in zip(bincode_msgs, wired[cb])]
    us, span = alternate(variants, args)
    slab_b = nbytes(slabs)
    wire_b = {"packed": int(rec.numel()), **{f"bincode{cb}": sum(int(d.numel()) + int(o.numel()) * 8 for d, o in wired[cb]) for cb in (8, 4)}}
    out = {"slab_bytes": slab_b, "wire_bytes": wire_b}
    for name, t in us.items():
        traffic = slab_b + wire_b[name.split("_")[0]]
        out[name] = {"us": round(t, 1), "us_min_max": [round(v, 1) for v in span[name]], "GBs": round(traffic / t / 1e3, 1),
                     "of_copy": round(traffic / t / 1e3 / cr, 3)}
    for d in ("encode", "decode"):
        out[f"packed_over_bincode8_{d}"] = round(us[f"packed_{d}"] / us[f"bincode8_{d}"], 3)
        out[f"packed_over_bincode4_{d}"] = round(us[f"packed_{d}"] / us[f"bincode4_{d}"], 3)
    return out


def open_cases(cr, args):
    N, n, k, l, B = 1024, 1, 3, 1, 4096
    ctx = Context(N, n, k, l)
    ctx.generate_key(7)
    x = ctx.sample_uniform(1, 0, ctx.half, (B, l))
    r = ctx.sample_uniform(1, 1, ctx.b, (B, k))
    y = ctx.sample_gauss(1, 2, ctx.sigma, (B, k))
    c, t, z, _ = FS.open_prove(ctx, x, r, y)
    d = FS.open_short(ctx, c, t, z)
    assert bool((FS.open_verify_short(ctx, c, d, z) == 1).all())
    res = {
        "commitment": codec_case(ctx, packed.MSG_OPEN_COMMITMENT, [c, t], [(wire.MSG_OPEN_COMMITMENT, [c, t])], None, cr, args),
        "response": codec_case(ctx, packed.MSG_OPEN_RESPONSE, [z], [(wire.MSG_OPEN_RESPONSE, [z])], None, cr, args),
        "short": codec_case(ctx, packed.MSG_OPEN_SHORT, [c, d, z],
                            [(wire.MSG_COMMITMENT, [c]), (wire.MSG_CHALLENGE, [d]), (wire.MSG_OPEN_RESPONSE, [z])], None, cr, args),
    }
    ctx.close()
    return res


def config5_cases(cr, args):
    N, n, k, l, V, B = 2048, 8, 17, 8, 32, 512
    ctx = Context(N, n, k, l)
    h = ctx.half
    cp, cs = ctx.sample_uniform(2, 0, h, (B, n + l)), ctx.sample_uniform(2, 1, h, (B, V, n + l))
    gs, tp = ctx.sample_uniform(2, 2, h, (B, V)), ctx.sample_uniform(2, 3, h, (B, n))
    ts, u = ctx.sample_uniform(2, 4, h, (B, V, n)), ctx.sample_uniform(2, 5, h, (B, l))
    zp, zs = ctx.sample_gauss(2, 6, ctx.sigma, (B, k)), ctx.sample_gauss(2, 7, ctx.sigma, (B, V, k))
    res = {
        "commitment": codec_case(ctx, packed.MSG_SUM_COMMITMENT, [cp, cs, gs, tp, ts, u],
                                 [(wire.MSG_SUM_COMMITMENT, [cp, cs, gs, tp, ts, u])], V, cr, args),
        "response": codec_case(ctx, packed.MSG_SUM_RESPONSE, [zp, zs], [(wire.MSG_SUM_RESPONSE, [zp, zs])], V, cr, args),
    }
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3, help="least launches per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.2, help="least duration of a timed window")
    ap.add_argument("--open-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed_codec_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_packed.py needs a GPU"
    cr = copy_rate()
    out = {"copy_GBs": round(cr, 1), "repeats": args.repeats, "window_s": args.window_s,
           "open_n1024_b4096": open_cases(cr, args)}
    if not args.open_only:
        out["sum_config5_chunk512"] = config5_cases(cr, args)
    line = json.dumps(out)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
