"""Randomised parity sweep (GPU): shapes, batch sizes, summand counts and tuning knobs drawn from a seeded generator,
every phase of the three protocols compared with the oracle (oracle/rzk_oracle.c) through the C ABI.

The fixed-shape tests pin the BASELINE configurations; this file walks the space between them — keys with k beyond
n + l + 1 (several random columns in a2'), n = l in 1..3, ragged batch sizes (1, 2, 3, 5), V = 1, and the kernel choices
the knobs switch — so that an indexing slip which happens to cancel at (1,3,1) or (4,9,4) still shows.
Reference: src/commit.rs:33-60,109-125, src/prove/open.rs:80-174, linear.rs:82-250, sum.rs:99-320.
"""
import os

import numpy as np
import pytest

from oracle import oracle as O
from ring_zk_amd import synth

from test_gpu_baseline_shapes import (P_of, assert_rotation_band, check_key_products_and_open, check_sum_cycle, dev, make_ctx,  # noqa: F401
                                      plant_edges, torch_mod)

pytestmark = pytest.mark.gpu

KNOBS = [
    {},
    {"RZK_ROW_GROUPS": 0},
    {"RZK_SHIFT": 0},
    {"RZK_PAIRS": 0},
    {"RZK_VEC_ROWS": 0},
    {"RZK_UPT": 64},   # all units of a proof in one wavefront (what batches >= 4096 take), here at batch <= 5
    {"RZK_SLOT_SHARE_MIN": 0, "RZK_ROW_GROUPS": 0},
    {"RZK_BLOCK_MIN_LOGN": 10},
    {"RZK_PAIR_POLY": 0},   # N = 2048: one wavefront per polynomial (the round-2 kernels) instead of two
    {"RZK_UNIT_IO": 1},     # key-product programs through unit_io_kernel at every N (default: N = 512 only)
    {"RZK_UNIT_IO": 0},     # ... and through unit_kernel at N = 512
    {"RZK_UPT": 64, "RZK_PRESET_IN_KERNEL": 0},   # one team per entry, verdict flags preset by a fill launch (default: by the team)
    {"RZK_SUM_D": 1},       # Sum proof: a2.(sum_i g_i v_i - v') whatever the cost model says
    {"RZK_SUM_D": 0},       # ... and sum_i g_i (a2.v_i) - a2.v' row by row
    {"RZK_DKEY": 2},        # the scalar multipliers g / g_i as prepared images whatever the use count
    {"RZK_DKEY": 0},        # ... and transformed by every row that multiplies by them
    {"RZK_DKEY": 2, "RZK_SUM_D": 0},
    {"RZK_LIN_E": 0},       # Linear verifier in the reference's grouping (two products with g) instead of g(.)e - e' - u
    {"RZK_LIN_E": 0, "RZK_DKEY": 2},
    {"RZK_SHIFT": 0, "RZK_DKEY": 2},
    {"RZK_DKEY": 2, "RZK_SUM_D": 1},                 # small shapes through the image paths: multipliers and operand images
    {"RZK_DKEY": 2, "RZK_SUM_D": 1, "RZK_OIMG": 0},  # ... and without the operand images
]


def draw_case(seed):
    rng = np.random.default_rng(9000 + seed)
    N = int(rng.choice([512, 512, 1024, 1024, 2048]))
    nl = int(rng.choice([1, 1, 2, 3]))
    extra = int(rng.choice([1, 1, 2, 3]))            # random columns of a2'
    k = 2 * nl + extra
    if N == 2048 and nl == 3:                         # keep the schoolbook oracle in seconds
        nl, k = 2, 4 + extra
    B = int(rng.choice([1, 2, 3, 5]))
    V = int(rng.choice([1, 2, 3, 5]))
    if N == 2048:
        B, V = min(B, 2), min(V, 3)
    env = KNOBS[int(rng.integers(0, len(KNOBS)))]
    return dict(N=N, n=nl, k=k, l=nl, B=B, V=V, env=env, seed=seed)


def check_linear_cycle(ctx, A, B, seed, entries=None, edges=False, recover=False, torch=None):
    """Linear cycle vs the oracle at `entries` (default every batch entry), the last proof tampered.  The modulus and the
    bound b of r are the context's; `edges`: plant_edges (test_gpu_baseline_shapes) in the transformed operands g and x.
    `recover`: linear_recover gives the oracle's t, t', u at `entries` and accepts every proof; `torch`: the device-pointer
    forms of commit, response, verify (and recover) give the bytes of the host-pointer forms."""
    P = P_of(ctx)
    q = ctx.q
    N, k, l = ctx.N, ctx.k, ctx.l
    rng = np.random.default_rng(seed)
    g = synth.uniform(rng, (B, N), q)
    x = synth.uniform(rng, (B, l, N), q)
    r, rp = synth.small(rng, (B, k, N), ctx.b), synth.small(rng, (B, k, N), ctx.b)
    y, yp = synth.gauss(rng, (B, k, N), P.sigma), synth.gauss(rng, (B, k, N), P.sigma)
    d = synth.challenge(rng, (B,), N, P.kappa)
    if edges:
        plant_edges(g, (q - 1) // 2), plant_edges(x, (q - 1) // 2)
        assert_rotation_band(r, d, q)
    c, cp, t, tp, u, ok = ctx.linear_commit(g, x, r, rp, y, yp)
    z, zp = ctx.linear_response(y, yp, r, rp, d)
    zt = z.copy()
    zt[B - 1, k - 1, N - 1] = O.center(int(zt[B - 1, k - 1, N - 1]) + 1, q)
    acc, acct = ctx.linear_verify(z, zp, c, cp, g, t, tp, u, d), ctx.linear_verify(zt, zp, c, cp, g, t, tp, u, d)
    for b in range(B) if entries is None else entries:
        ref = O.linear_commit(P, A, g[b], x[b], r[b], rp[b], y[b], yp[b])          # linear.rs:82-140
        for got, want, name in zip((c, cp, t, tp, u), ref[:5], ("c", "cp", "t", "tp", "u")):
            assert np.array_equal(got[b], want), (name, b)
        assert int(ok[b]) == ref[5]
        zr, zpr = O.linear_response(P, y[b], yp[b], r[b], rp[b], d[b])              # linear.rs:144-158
        assert np.array_equal(z[b], zr) and np.array_equal(zp[b], zpr)
        assert O.linear_verify(P, A, z[b], zp[b], c[b], cp[b], g[b], t[b], tp[b], u[b], d[b]) == 1   # linear.rs:213-250
    assert acc.tolist() == [1] * B and acct.tolist() == [1] * (B - 1) + [0]
    if recover:
        tr, tpr, ur, accr = ctx.linear_recover(z, zp, c, cp, g, d)
        for b in range(B) if entries is None else entries:
            ref = O.linear_commit(P, A, g[b], x[b], r[b], rp[b], y[b], yp[b])
            assert np.array_equal(tr[b], ref[2]) and np.array_equal(tpr[b], ref[3]) and np.array_equal(ur[b], ref[4]), ("recover", b)
        assert accr.tolist() == [1] * B
    if torch is not None:   # the host-pointer outputs above are the oracle's at `entries`
        D = lambda a: dev(torch, a)   # noqa: E731
        outs = ctx.linear_commit(D(g), D(x), D(r), D(rp), D(y), D(yp))
        for got, want in zip(outs, (c, cp, t, tp, u, ok)):
            assert np.array_equal(got.cpu().numpy(), want)
        zd, zpd = ctx.linear_response(D(y), D(yp), D(r), D(rp), D(d))
        assert np.array_equal(zd.cpu().numpy(), z) and np.array_equal(zpd.cpu().numpy(), zp)
        accd = ctx.linear_verify(D(zt), zpd, outs[0], outs[1], D(g), outs[2], outs[3], outs[4], D(d))
        assert accd.cpu().numpy().tolist() == [1] * (B - 1) + [0]
        if recover:
            rec = ctx.linear_recover(zd, zpd, outs[0], outs[1], D(g), D(d))
            for got, want in zip(rec, (tr, tpr, ur, accr)):
                assert np.array_equal(got.cpu().numpy(), want)


# RZK_SWEEP_CASES / RZK_SWEEP_FIRST: a longer soak over other seeds (e.g. 400 cases from seed 1000: ~10 min on the GPU box)
_SWEEP_N = int(os.environ.get("RZK_SWEEP_CASES", "40"))
_SWEEP_0 = int(os.environ.get("RZK_SWEEP_FIRST", "0"))


@pytest.mark.parametrize("seed", range(_SWEEP_0, _SWEEP_0 + _SWEEP_N))
def test_random_shape_all_protocols_vs_oracle(torch_mod, seed):
    cs = draw_case(seed)
    ctx = make_ctx(cs["N"], cs["n"], cs["k"], cs["l"], env=cs["env"])
    A = synth.key(np.random.default_rng(9100 + seed), cs["N"], cs["n"], cs["k"], cs["l"])
    ctx.load_key(A)
    check_key_products_and_open(ctx, A, cs["B"], 9200 + seed)
    check_linear_cycle(ctx, A, cs["B"], 9300 + seed)
    check_sum_cycle(torch_mod, ctx, A, cs["B"], cs["V"], 9400 + seed, device_too=(seed % 3 == 0))
