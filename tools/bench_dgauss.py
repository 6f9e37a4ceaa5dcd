#!/usr/bin/env python3
"""The exact discrete Gaussian kernel against the keyed Box-Muller kernel at N = 1024, 4096 x 3 polynomials, sigma of the
context: one JSON line, also saved to profiles/dgauss_bench.json.

rzk_sample_dgauss_keyed_dev and rzk_sample_gauss_keyed_dev are timed alternately, --repeats windows of at least --iters
launches and --window-s seconds each after a warm-up of both, device events around each window; GB/s = bytes of output
(8 N per polynomial) over the median time of one launch.  Both calls include their host part (HChaCha20 of the nonce,
and for the exact sampler the parameters of sigma).  tools/copy_rate.py runs in the same session, in a process of its
own after the samplers, and its lines are stored next to the figures.  No pass mark: the exact sampler computes several
ChaCha20 blocks and trials per 8 coefficients where Box-Muller computes one block."""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ring_zk_amd import Context  # noqa: E402


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters   # us per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--window-s", type=float, default=0.3, help="least duration of a timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dgauss_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_dgauss.py needs a GPU"
    N, k, B = 1024, 3, args.batch
    ctx = Context(N, 1, k, 1)
    ctx.set_sampler_key(bytes(range(32)))
    ctx._bind_torch_stream()
    out = torch.empty((B, k, N), dtype=torch.int64, device="cuda")
    p, cnt, L, h = out.data_ptr(), B * k, ctx._L, ctx._h
    nonce = (ctypes.c_uint8 * 16)(*range(16))
    sigma = int(ctx.sigma)
    exact = lambda: L.rzk_sample_dgauss_keyed_dev(h, nonce, 0, sigma, p, cnt * N)
    boxm = lambda: L.rzk_sample_gauss_keyed_dev(h, nonce, 0, float(sigma), p, cnt)
    for fn in (exact, boxm):
        for _ in range(3):
            assert fn() == 0
    torch.cuda.synchronize()
    it_e = max(args.iters, int(args.window_s * 1e6 / window(exact, args.iters)) + 1)
    it_b = max(args.iters, int(args.window_s * 1e6 / window(boxm, args.iters)) + 1)
    te, tb = [], []
    for _ in range(args.repeats):
        te.append(window(exact, it_e))
        tb.append(window(boxm, it_b))
    me, mb = float(np.median(te)), float(np.median(tb))
    nbytes = cnt * N * 8
    res = {
        "config": f"N={N} polynomials={B}x{k} sigma={sigma} output_MB={nbytes / 1e6:.1f}", "repeats": args.repeats,
        "iters": [it_e, it_b],
        "dgauss_us": round(me, 1), "dgauss_us_min_max": [round(min(te), 1), round(max(te), 1)],
        "box_muller_us": round(mb, 1), "box_muller_us_min_max": [round(min(tb), 1), round(max(tb), 1)],
        "dgauss_GBs": round(nbytes / me / 1e3, 1), "box_muller_GBs": round(nbytes / mb / 1e3, 1),
        "dgauss_over_box_muller_time": round(me / mb, 2),
    }
    ctx.close()
    del out
    torch.cuda.empty_cache()
    copy = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "copy_rate.py")], capture_output=True, text=True)
    assert copy.returncode == 0, copy.stderr[-2000:]
    res["copy_rate"] = copy.stdout.splitlines()
    line = json.dumps(res)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
