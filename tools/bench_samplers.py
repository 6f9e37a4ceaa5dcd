#!/usr/bin/env python3
"""Seeded (Philox4x32-10) vs keyed (ChaCha20) device samplers at N = 1024, 4096 x 3 polynomials: one JSON line, also
saved to profiles/keyed_samplers_bench.json.

For each distribution (uniform b = 1, Gaussian sigma of the context, challenge kappa = 36) the two kernels are timed
alternately, --repeats windows of at least --iters launches and --window-s seconds each after a warm-up of both, device
events around each window; GB/s = bytes of output (8 N per polynomial) over the median time of one launch.  The keyed
calls include their host part (HChaCha20 of the nonce, once per call).  tools/copy_rate.py runs in the same session, in
a process of its own after the samplers, and its lines are stored next to the sampler figures: what a plain device copy
and a read reach on this box is the yardstick for "at the HBM write rate".
"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keyed_samplers_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_samplers.py needs a GPU"
    N, k, B = 1024, 3, args.batch
    ctx = Context(N, 1, k, 1)
    ctx.set_sampler_key(bytes(range(32)))
    ctx._bind_torch_stream()
    out = torch.empty((B, k, N), dtype=torch.int64, device="cuda")
    p, cnt, L, h = out.data_ptr(), B * k, ctx._L, ctx._h
    nonce = (ctypes.c_uint8 * 16)(*range(16))
    sigma = float(ctx.sigma)
    pairs = {
        "uniform": (lambda: L.rzk_sample_uniform_dev(h, 1, 0, 1, p, cnt), lambda: L.rzk_sample_uniform_keyed_dev(h, nonce, 0, 1, p, cnt)),
        "gauss": (lambda: L.rzk_sample_gauss_dev(h, 1, 0, sigma, p, cnt), lambda: L.rzk_sample_gauss_keyed_dev(h, nonce, 0, sigma, p, cnt)),
        "challenge": (lambda: L.rzk_sample_challenge_dev(h, 1, 0, p, cnt), lambda: L.rzk_sample_challenge_keyed_dev(h, nonce, 0, p, cnt)),
    }
    nbytes = cnt * N * 8
    res = {"config": f"N={N} polynomials={B}x{k} output_MB={nbytes / 1e6:.1f}", "repeats": args.repeats}
    for name, (philox, chacha) in pairs.items():
        for fn in (philox, chacha):
            for _ in range(3):
                assert fn() == 0, name
        torch.cuda.synchronize()
        it_p = max(args.iters, int(args.window_s * 1e6 / window(philox, args.iters)) + 1)
        it_c = max(args.iters, int(args.window_s * 1e6 / window(chacha, args.iters)) + 1)
        tp, tc = [], []
        for _ in range(args.repeats):
            tp.append(window(philox, it_p))
            tc.append(window(chacha, it_c))
        mp, mc = float(np.median(tp)), float(np.median(tc))
        res[name] = {
            "iters": [it_p, it_c],
            "philox_us": round(mp, 1), "philox_us_min_max": [round(min(tp), 1), round(max(tp), 1)],
            "chacha20_us": round(mc, 1), "chacha20_us_min_max": [round(min(tc), 1), round(max(tc), 1)],
            "philox_GBs": round(nbytes / mp / 1e3, 1), "chacha20_GBs": round(nbytes / mc / 1e3, 1),
            "chacha20_over_philox_time": round(mc / mp, 3),
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
