#!/usr/bin/env python3
"""The rejection-sampling step at Open N = 1024, (1,3,1), B = 4096, in one process: one JSON line (also written to
profiles/reject_open1024_bench.json with --record, or to profiles/NAME with --record-as NAME).

  kernels   the response rows (shift_row_kernel), reject_stat_kernel / reject_decide_kernel and the fused response rows
            (response_stat_kernel) on one honest batch, from the library's per-launch events (rzk_prof_*),
            median of --iters calls; GB/s on the 2 x rows x N x 8 bytes per proof the stat kernel reads;
  calls     the chain (open_response, then reject) against the fused entry point (open_response_reject), timed
            alternately in --repeats windows after a warm-up of both; every window pair is reported;
  provers   fiat_shamir.open_prove_zk against fiat_shamir.open_prove_sampled, both over a SeededSampler, timed
            alternately in --repeats windows after a warm-up of both, device events around each window; rounds used
            and the round-0 acceptance rate of the batch.

On a library without the fused entry points (the parent of the change that added them) the fields that need them are left out.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ring_zk_amd import Context  # noqa: E402
from ring_zk_amd import fiat_shamir as FS  # noqa: E402
from ring_zk_amd.backend import SeededSampler, reject_lnm  # noqa: E402


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters   # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--window-s", type=float, default=0.5, help="least duration of a timed window")
    ap.add_argument("--record", action="store_true", help="write the line to profiles/reject_open1024_bench.json")
    ap.add_argument("--record-as", default=None, metavar="NAME", help="write the line to profiles/NAME")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_reject.py needs a GPU"
    N, n, k, l, B = 1024, 1, 3, 1, args.batch
    ctx = Context(N, n, k, l)
    ctx.generate_key(7)
    x = ctx.sample_uniform(1, 0, ctx.half, (B, l))

    # ---- the two kernels on one honest batch ----------------------------------------------------------------------
    s = SeededSampler(ctx, 11)
    r, y, d = s.uniform(ctx.b, (B, k)), s.gauss(ctx.sigma, (B, k)), s.challenge((B,))
    z = ctx.open_response(y, r, d)
    coin, R = FS.draw_coins(s, (B,))
    lnM = reject_lnm(11.0)
    for _ in range(3):
        acc, _ = ctx.reject([(z, y)], coin, R, lnM)
    has_fused = hasattr(ctx, "open_response_reject")

    def chain():
        zz = ctx.open_response(y, r, d)
        return ctx.reject([(zz, y)], coin, R, lnM)

    def fused():
        return ctx.open_response_reject(y, r, d, coin, R, lnM)

    if has_fused:
        for _ in range(3):
            zf, accf, Ef = fused()
        acc_c, E_c = chain()
        assert torch.equal(zf, z) and torch.equal(accf, acc_c) and torch.equal(Ef, E_c), "fused and chain disagree"
    ctx.prof_enable(True)
    by_prefix = {"shift_row_kernel": [], "reject_stat_kernel": [], "reject_decide_kernel": [], "response_stat_kernel": []}
    for _ in range(args.iters):
        for call in (chain, fused) if has_fused else (chain,):
            ctx.prof_reset()
            call()
            us = ctx.prof_read_all()
            names = [kn for kn, _ in ctx.prof_read_kernels()]
            if call is chain:
                for pre in ("shift_row_kernel", "reject_stat_kernel", "reject_decide_kernel"):
                    by_prefix[pre].append(sum(u for u, kn in zip(us, names) if kn.startswith(pre)))
            else:
                by_prefix["response_stat_kernel"].append(sum(u for u, kn in zip(us, names) if kn.startswith("response_stat_kernel")))
    ctx.prof_enable(False)
    med = lambda pre: float(np.median(by_prefix[pre]))
    response_us, stat_us, decide_us = med("shift_row_kernel"), med("reject_stat_kernel"), med("reject_decide_kernel")
    read_bytes = 2 * k * N * 8 * B

    # ---- the entry points, alternated -----------------------------------------------------------------------------------
    calls = {}
    if has_fused:
        for _ in range(3):
            chain()
            fused()
        torch.cuda.synchronize()
        it_c = max(args.iters, int(args.window_s * 1e6 / window(chain, args.iters)) + 1)
        tc, tf = [], []
        for _ in range(args.repeats):
            tc.append(window(chain, it_c))
            tf.append(window(fused, it_c))
        calls = {
            "response_stat_kernel_us": round(med("response_stat_kernel"), 1),
            "chain_call_us": round(float(np.median(tc)), 1), "fused_call_us": round(float(np.median(tf)), 1),
            "window_pairs_chain_fused_us": [[round(a, 1), round(b, 1)] for a, b in zip(tc, tf)],
            "fused_faster_in_every_pair": bool(all(b < a for a, b in zip(tc, tf))),
            "call_iters": it_c,
        }

    # ---- the provers, alternated --------------------------------------------------------------------------------------
    seeds = iter(range(1000, 1 << 30))
    rounds_used, rate0 = [], []

    def sampled():
        return FS.open_prove_sampled(ctx, x, SeededSampler(ctx, next(seeds)))

    def zk():
        out = FS.open_prove_zk(ctx, x, SeededSampler(ctx, next(seeds)))
        rounds_used.append(out[5])
        return out

    out = zk()
    assert bool((out[3] == 1).all()), "a proof of the benchmark batch was not accepted within 64 rounds"
    for _ in range(3):
        sampled()
        zk()
    torch.cuda.synchronize()
    rounds_used.clear()
    it_s = max(args.iters, int(args.window_s * 1e6 / window(sampled, args.iters)) + 1)
    it_z = max(args.iters, int(args.window_s * 1e6 / window(zk, args.iters)) + 1)
    rounds_used.clear()
    ts, tz = [], []
    for _ in range(args.repeats):
        ts.append(window(sampled, it_s))
        tz.append(window(zk, it_z))
    ratios = [b / a for a, b in zip(ts, tz)]
    rr = torch.stack(rounds_used).to(torch.float64)
    line = {
        "config": f"open N={N} ({n},{k},{l}) B={B}", "iters": [it_s, it_z], "repeats": args.repeats,
        "response_kernel_us": round(response_us, 1),
        "reject_stat_kernel_us": round(stat_us, 1), "reject_decide_kernel_us": round(decide_us, 1),
        "stat_read_bytes": read_bytes, "stat_GBs": round(read_bytes / stat_us / 1e3, 1),
        "decide_GBs": round(B * k * 16 / decide_us / 1e3, 2),
        "kernel_accept_rate": round(float(acc.sum().item()) / B, 4),
        "open_prove_sampled_us": round(float(np.median(ts)), 1), "open_prove_zk_us": round(float(np.median(tz)), 1),
        "ratio_zk_over_sampled": round(float(np.median(ratios)), 3),
        "ratio_min_max": [round(min(ratios), 3), round(max(ratios), 3)],
        "rounds_max": int(rr.max().item()) + 1, "rounds_mean_per_proof": round(float(rr.mean().item()) + 1, 3),
        "round0_accept_rate": round(float((rr == 0).double().mean().item()), 4),
        "zk_proofs_per_s": round(B / float(np.median(tz)) * 1e6),
        "open_prove_zk_windows_us": [round(v, 1) for v in tz],
    }
    line.update(calls)
    ctx.close()
    text = json.dumps(line)
    print(text)
    if args.record or args.record_as:
        with open(os.path.join(ROOT, "profiles", args.record_as or "reject_open1024_bench.json"), "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
