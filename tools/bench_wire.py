#!/usr/bin/env python3
"""Batched message codec on the GPU (rzk_wire_{decode,encode}_batch_dev): one JSON line.

For Open N=1024 (1,3,1) B=4096 at coefficient widths 8 and 4, and for one config-5 chunk (Sum N=2048 (8,17,8) V=32,
512 proofs), reports per message kind and for the whole verifier input set:
  * decode / encode microseconds from device events (median of --iters launches);
  * GB/s of bytes in + bytes out, and that rate over a plain device copy measured in the same process
    (the method of tools/copy_rate.py: torch copy_ of 1 GiB);
  * decode + verify end to end beside plain verify;
  * Open only: the host path (wire.mat_decode once per matrix) on the same batch, for contrast.
The walk kernel's share is measured separately, in a run of its own under
`rocprofv3 --kernel-trace --stats -- python tools/bench_wire.py --open-only`.
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

from ring_zk_amd import Context, wire  # noqa: E402


def dev_time(fn, iters, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(ts))


def copy_rate():
    n = 1024 * 1024 * 1024 // 8
    a = torch.empty(n, dtype=torch.int64, device="cuda").random_()
    b = torch.empty_like(a)
    us = dev_time(lambda: b.copy_(a), 20, 5)
    del a, b
    return 2 * n * 8 / us / 1e3   # GB/s read + write


def nbytes(ts):
    return sum(int(t.numel()) * t.element_size() for t in ts if t is not None)


def codec_case(ctx, kind, slabs, V, cb, iters, cr):
    data, offsets = wire.encode_batch(ctx, kind, *slabs, V=V, coef_bytes=cb)
    enc_us = dev_time(lambda: wire.encode_batch(ctx, kind, *slabs, V=V, coef_bytes=cb), iters)
    out = wire.decode_batch(ctx, kind, data, offsets, V=V, coef_bytes=cb)
    assert bool((out[-1] == 1).all()), "decode rejected the library's own encoding"
    for got, want in zip(out[:-1], slabs):
        assert torch.equal(got, want)
    dec_us = dev_time(lambda: wire.decode_batch(ctx, kind, data, offsets, V=V, coef_bytes=cb), iters)
    traffic = nbytes(slabs) + int(data.numel()) + int(offsets.numel()) * 8
    return dict(bytes=int(data.numel()), decode_us=round(dec_us, 1), encode_us=round(enc_us, 1),
                decode_GBs=round(traffic / dec_us / 1e3, 1), encode_GBs=round(traffic / enc_us / 1e3, 1),
                decode_of_copy=round(traffic / dec_us / 1e3 / cr, 3),
                encode_of_copy=round(traffic / enc_us / 1e3 / cr, 3)), (data, offsets)


def open_case(cb, iters, cr, host_path):
    N, n, k, l, B = 1024, 1, 3, 1, 4096
    ctx = Context(N, n, k, l)
    ctx.generate_key(7)
    x = ctx.sample_uniform(1, 0, ctx.half, (B, l))
    r = ctx.sample_uniform(1, 1, ctx.b, (B, k))
    y = ctx.sample_gauss(1, 2, ctx.sigma, (B, k))
    d = ctx.sample_challenge(1, 3, (B,))
    c, t, _ = ctx.open_commit(x, r, y)
    z = ctx.open_response(y, r, d)
    res = {}
    msgs = {}
    for name, kind, slabs in (("commitment", wire.MSG_OPEN_COMMITMENT, [c, t]), ("challenge", wire.MSG_CHALLENGE, [d]),
                              ("response", wire.MSG_OPEN_RESPONSE, [z])):
        res[name], msgs[name] = codec_case(ctx, kind, slabs, None, cb, iters, cr)

    def decode_all():
        return (wire.decode_batch(ctx, wire.MSG_OPEN_COMMITMENT, *msgs["commitment"], coef_bytes=cb),
                wire.decode_batch(ctx, wire.MSG_CHALLENGE, *msgs["challenge"], coef_bytes=cb),
                wire.decode_batch(ctx, wire.MSG_OPEN_RESPONSE, *msgs["response"], coef_bytes=cb))

    acc = wire.verify_open(ctx, msgs["commitment"], msgs["challenge"], msgs["response"], coef_bytes=cb)
    assert bool((acc == 1).all())
    res["decode_all_us"] = round(dev_time(decode_all, iters), 1)
    res["verify_us"] = round(dev_time(lambda: ctx.open_verify(z, t, c, d), iters), 1)
    res["decode_verify_us"] = round(dev_time(lambda: wire.verify_open(ctx, msgs["commitment"], msgs["challenge"],
                                                                      msgs["response"], coef_bytes=cb), iters), 1)
    if host_path:   # the host Mat codec, one call per matrix (c, t as n x 1 Mats, z), same coefficients
        cn, tn, zn = (v.cpu().numpy() for v in (c, t, z))
        mats = [wire.mat_encode(a[b][:, None, :], cb) for b in range(B) for a in (cn, tn, zn)]
        t0 = time.perf_counter()
        for m in mats:
            wire.mat_decode(m, N, cb, q=ctx.q)
        res["host_mat_decode_us"] = round((time.perf_counter() - t0) * 1e6, 1)
    ctx.close()
    return res


def config5_case(cb, iters, cr):
    N, n, k, l, V, B = 2048, 8, 17, 8, 32, 512
    ctx = Context(N, n, k, l)
    ctx.generate_key(9)
    h = ctx.half
    cp, cs = ctx.sample_uniform(2, 0, h, (B, n + l)), ctx.sample_uniform(2, 1, h, (B, V, n + l))
    gs, tp = ctx.sample_uniform(2, 2, h, (B, V)), ctx.sample_uniform(2, 3, h, (B, n))
    ts, u = ctx.sample_uniform(2, 4, h, (B, V, n)), ctx.sample_uniform(2, 5, h, (B, l))
    zp, zs = ctx.sample_gauss(2, 6, ctx.sigma, (B, k)), ctx.sample_gauss(2, 7, ctx.sigma, (B, V, k))
    d = ctx.sample_challenge(2, 8, (B,))
    res = {}
    msgs = {}
    res["commitment"], msgs["commitment"] = codec_case(ctx, wire.MSG_SUM_COMMITMENT, [cp, cs, gs, tp, ts, u], V, cb,
                                                       iters, cr)
    res["response"], msgs["response"] = codec_case(ctx, wire.MSG_SUM_RESPONSE, [zp, zs], V, cb, iters, cr)
    res["challenge"], msgs["challenge"] = codec_case(ctx, wire.MSG_CHALLENGE, [d], None, cb, iters, cr)
    # random (not proof) data: verify rejects, its cost is that of the chunk's verify all the same
    res["verify_us"] = round(dev_time(lambda: ctx.sum_verify(zs, zp, cs, cp, gs, ts, tp, u, d), iters), 1)
    res["decode_all_us"] = round(sum(res[m]["decode_us"] for m in ("commitment", "response", "challenge")), 1)
    res["decode_of_verify"] = round(res["decode_all_us"] / res["verify_us"], 3)
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--open-only", action="store_true", help="Open cases only (the rocprofv3 run)")
    ap.add_argument("--no-host", action="store_true", help="skip the host mat_decode contrast")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_wire.py needs a GPU"
    cr = copy_rate()
    out = {"copy_GBs": round(cr, 1)}
    for cb in (8, 4):
        out[f"open_n1024_b4096_w{cb}"] = open_case(cb, args.iters, cr, host_path=not args.no_host and cb == 8)
    if not args.open_only:
        out["sum_config5_chunk512_w8"] = config5_case(8, max(3, args.iters // 3), cr)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
