#!/usr/bin/env python3
"""Interactive vs non-interactive (Fiat-Shamir) Open cycle at N = 1024, (1,3,1), B = 4096, in one process: one JSON line.

  interactive       commit + response + verify through the existing entry points, d given (what the protocol cost
                    before the transcript hash existed);
  non_interactive   fiat_shamir.open_prove (commit, challenge, response) + fiat_shamir.open_verify (challenge, verify).
The two cycles are timed alternately, --repeats windows of at least --iters cycles and --window-s seconds each after
a warm-up of both, device events around each window; the figure of record is the median non-interactive / interactive time ratio.  The leaf and root
kernel times come from the library's per-launch events (rzk_prof_*) in windows of their own; bytes hashed per second =
8 N x message polynomials x B over the leaf + root time of one challenge call.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ring_zk_amd import Context, wire  # noqa: E402
from ring_zk_amd import fiat_shamir as FS  # noqa: E402


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters   # us per cycle


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--window-s", type=float, default=0.5, help="least duration of a timed window")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_fs.py needs a GPU"
    N, n, k, l, B = 1024, 1, 3, 1, args.batch
    ctx = Context(N, n, k, l)
    ctx.generate_key(7)
    x = ctx.sample_uniform(1, 0, ctx.half, (B, l))
    r = ctx.sample_uniform(1, 1, ctx.b, (B, k))
    y = ctx.sample_gauss(1, 2, ctx.sigma, (B, k))
    d = ctx.sample_challenge(1, 3, (B,))

    def interactive():
        c, t, _ = ctx.open_commit(x, r, y)
        z = ctx.open_response(y, r, d)
        return ctx.open_verify(z, t, c, d)

    def non_interactive():
        c, t, z, _ = FS.open_prove(ctx, x, r, y)
        return FS.open_verify(ctx, c, t, z)

    acc_i, acc_n = interactive(), non_interactive()
    assert bool((acc_n == 1).all()) and bool((acc_i == 1).all()), "a proof of the benchmark batch was rejected"
    for _ in range(3):   # warm both cycles: code objects, arenas, row programs
        interactive()
        non_interactive()
    torch.cuda.synchronize()
    # a window of a fraction of a second measures the clock and the scheduler: size both from an untimed trial
    iters_i = max(args.iters, int(args.window_s * 1e6 / window(interactive, args.iters)) + 1)
    iters_n = max(args.iters, int(args.window_s * 1e6 / window(non_interactive, args.iters)) + 1)
    ti, tn = [], []
    for _ in range(args.repeats):
        ti.append(window(interactive, iters_i))
        tn.append(window(non_interactive, iters_n))
    ratios = [b / a for a, b in zip(ti, tn)]

    # kernel times of the challenge alone, from the library's per-launch events
    c, t, _ = ctx.open_commit(x, r, y)
    ctx.prof_enable(True)
    leaf, root = [], []
    for _ in range(args.iters):
        ctx.prof_reset()
        FS.challenge(ctx, wire.MSG_OPEN_COMMITMENT, c, t)
        us = ctx.prof_read_all()
        names = [kn for kn, _ in ctx.prof_read_kernels()]
        leaf.append(sum(u for u, kn in zip(us, names) if kn == "fs_leaf_kernel"))
        root.append(sum(u for u, kn in zip(us, names) if kn == "fs_root_kernel"))
    ctx.prof_enable(False)
    leaf_us, root_us = float(np.median(leaf)), float(np.median(root))
    hashed = 8 * N * (n + l + n) * B
    out = {
        "config": f"open N={N} ({n},{k},{l}) B={B}", "iters": [iters_i, iters_n], "repeats": args.repeats,
        "interactive_cycle_us": round(float(np.median(ti)), 1),
        "non_interactive_cycle_us": round(float(np.median(tn)), 1),
        "interactive_proofs_per_s": round(B / float(np.median(ti)) * 1e6),
        "non_interactive_proofs_per_s": round(B / float(np.median(tn)) * 1e6),
        "ratio_non_interactive_over_interactive": round(float(np.median(ratios)), 3),
        "ratio_min_max": [round(min(ratios), 3), round(max(ratios), 3)],
        "fs_leaf_kernel_us": round(leaf_us, 1), "fs_root_kernel_us": round(root_us, 1),
        "challenges_per_cycle": 2,
        "hashed_bytes_per_challenge": hashed,
        "hashed_GBs": round(hashed / (leaf_us + root_us) / 1e3, 1),
    }
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
