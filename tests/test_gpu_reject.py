"""The prover's rejection-sampling step on the GPU (rzk_reject_batch[_dev], Context.reject, fiat_shamir.*_prove_zk)
against tests/reject_ref.py: E bit for bit and the decision on every decidable case (reject_ref: |E - T| > 2 sigma^2
2^-44), host and device entry points, at the shapes where the kernels take another path; every fail cause; the grid
cap; trusted-producer mode; the argument rules; the statistics the step exists for; and the zero-knowledge provers end
to end against the verifiers and the oracle."""
import ctypes as C
import math

import numpy as np
import pytest

import reject_ref as RR
from oracle import oracle as O
from ring_zk_amd import _lib, RzkError
from ring_zk_amd import fiat_shamir as FS
from ring_zk_amd.backend import SeededSampler, reject_lnm
from test_gpu_baseline_shapes import P_of, dev, make_ctx, torch_mod  # noqa: F401
from test_gpu_fiat_shamir import OPEN, LINEAR, SUM, keyed_ctx, ref_challenge

pytestmark = pytest.mark.gpu

R62 = 1 << 62
LNM = 12 / 11 + 1 / 242


def ctx_of(N, env=None):
    ctx = make_ctx(N, 1, 3, 1, env=env, kappa=min(N, 36))
    return ctx, RR.params_of(ctx)


def split(z, y, rows):
    """one slab pair -> the parts of `rows` (an int: one part; a tuple: consecutive parts)"""
    if isinstance(rows, int):
        return [(z, y)]
    edges = np.cumsum((0,) + rows)
    return [(np.ascontiguousarray(z[:, a:b]), np.ascontiguousarray(y[:, a:b])) for a, b in zip(edges[:-1], edges[1:])]


def both(torch, ctx, parts, coin, R, lnM):
    """(accept, E) from the host entry point after checking that the device entry point gives the same bytes."""
    acc, E = ctx.reject(parts, coin, R, lnM)
    dacc, dE = ctx.reject([(dev(torch, z), dev(torch, y)) for z, y in parts], dev(torch, coin), R, lnM)
    ctx.synchronize()
    assert np.array_equal(dacc.cpu().numpy(), acc) and np.array_equal(dE.cpu().numpy(), E)
    return acc, E


def compare(want, acc, E, max_undecidable=2):
    assert RR.count_undecidable(want) <= max_undecidable   # from the reference alone
    for b, w in enumerate(want):
        assert int(E[b]) == w[0], b
        if w[3]:
            assert int(acc[b]) == int(w[2]), b
        assert not (w[1] and acc[b]), b


SHAPES = [(N, rows) for N in (4, 64, 128, 256, 1024, 2048) for rows in (1, 3, (3, 3))] + [(64, 65), (64, 130)]


@pytest.mark.parametrize("N,rows", SHAPES)
def test_matches_reference(torch_mod, N, rows):
    """N = 4: one load in two lanes; 64: half a wave; 128: one full trip; 2048: eight trips of two unrolled groups;
    65 / 130 rows: two / three lane trips of the decide kernel; (3, 3): the second part's base pointer."""
    ctx, P = ctx_of(N)
    total = rows if isinstance(rows, int) else sum(rows)
    for B in (1, 3, 5):
        rng = np.random.default_rng(1000 * N + 10 * total + B)
        z, y = RR.honest(rng, P, B, total)
        parts = split(z, y, rows)
        coin = RR.coins(rng, B, R62)
        want = RR.run(P, parts, coin, R62, LNM)
        assert all(w[1] == 0 for w in want)
        acc, E = both(torch_mod, ctx, parts, coin, R62, LNM)
        compare(want, acc, E)


@pytest.mark.parametrize("rows", [1, (3, 3)])
def test_grid_stride_trips(torch_mod, rows):
    """B = 100 with every grid sized for one CU (8 workgroups of 4 wavefronts): both kernels make four or more trips."""
    total = rows if isinstance(rows, int) else sum(rows)
    ctx1, P = ctx_of(64, env={"RZK_GRID_CUS": 1})
    ctx, _ = ctx_of(64)
    B = 100
    rng = np.random.default_rng(77 + total)
    z, y = RR.honest(rng, P, B, total)
    parts, coin = split(z, y, rows), RR.coins(rng, B, R62)
    acc1, E1 = both(torch_mod, ctx1, parts, coin, R62, LNM)
    acc, E = both(torch_mod, ctx, parts, coin, R62, LNM)
    assert np.array_equal(acc1, acc) and np.array_equal(E1, E)
    compare(RR.run(P, parts, coin, R62, LNM), acc, E)


def raw_call(ctx, fn, parts, coin, R, lnM, acc, E, B, nparts=None, rows=None):
    n = len(parts) if nparts is None else nparts
    ptr = lambda a: a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data
    zp = (C.c_void_p * max(len(parts), 1))(*[ptr(z) for z, _ in parts])
    yp = (C.c_void_p * max(len(parts), 1))(*[ptr(y) for _, y in parts])
    rows = rows or [int(np.prod(z.shape[1:-1])) for z, _ in parts]
    return fn(ctx._h, n, zp, yp, (C.c_uint32 * max(len(rows), 1))(*rows), C.c_void_p(ptr(coin)), R, lnM, C.c_void_p(ptr(acc)),
              C.c_void_p(ptr(E)) if E is not None else None, B)


def test_every_fail_cause_clears_its_own_proof(torch_mod):
    ctx, P = ctx_of(64)
    B, rows = 5, 3
    rng = np.random.default_rng(5)
    z0, y0 = RR.honest(rng, P, B, rows)
    coin0 = np.zeros(B, np.int64)      # u = 1 / R: every honest proof is accepted
    acc, E = both(torch_mod, ctx, [(z0, y0)], coin0, R62, LNM)
    assert acc.tolist() == [1] * B
    edge_at, edge_past = RR.norm_edge_poly(P, 0), RR.norm_edge_poly(P, 1)   # sum c^2 = (vb + 1)^2 - 1 and (vb + 1)^2
    cases = []
    for victim, what in enumerate(("vmax", "norm", "coin_R", "coin_neg", "vmax_ok")):
        z, y, coin = z0.copy(), y0.copy(), coin0.copy()
        if what == "vmax":
            z[victim, 2, 63] = y[victim, 2, 63] + P.vmax + 1
        elif what == "vmax_ok":
            z[victim, 0, 0], victim = y[victim, 0, 0] - P.vmax, None
        elif what == "norm":
            z[victim, 1], y[victim, 1] = edge_past, edge_past - 1
            z[(victim + 1) % B, 0], y[(victim + 1) % B, 0] = edge_at, edge_at + 1     # exactly at the edge passes
        elif what == "coin_R":
            coin[victim] = R62
        else:
            coin[victim] = -1
        want = RR.run(P, [(z, y)], coin, R62, LNM)
        assert [bool(w[1]) for w in want] == [b == victim for b in range(B)], what
        acc, E = both(torch_mod, ctx, [(z, y)], coin, R62, LNM)
        compare(want, acc, E, max_undecidable=0)
        assert acc.tolist() == [int(b != victim) for b in range(B)], what
        cases.append(what)
    # a non-canonical coefficient: RZK_E_ARG from the host entry point, the sticky word from the device entry point
    for where, bad in (((3, 1, 7), P.half + 1), ((0, 2, 0), (1 << 32) + 9), ((4, 0, 63), -P.half - 1)):
        for in_y in (False, True):
            z, y = z0.copy(), y0.copy()
            (y if in_y else z)[where] = bad
            with pytest.raises(RzkError) as e:
                ctx.reject([(z, y)], coin0, R62, LNM)
            assert e.value.status == _lib.RZK_E_ARG
            dacc, _ = ctx.reject([(dev(torch_mod, z), dev(torch_mod, y))], dev(torch_mod, coin0), R62, LNM)
            with pytest.raises(RzkError) as e:
                ctx.synchronize()
            assert e.value.status == _lib.RZK_E_ARG
            assert dacc.cpu().numpy().tolist() == [int(b != where[0]) for b in range(B)]
            ctx.synchronize()   # reported once, then cleared
    acc, _ = ctx.reject([(z0, y0)], coin0, R62, LNM)   # the fault does not leak into the next call
    assert acc.tolist() == [1] * B


def test_trusted_mode_gives_identical_bytes(torch_mod):
    ctx, P = ctx_of(256)
    rng = np.random.default_rng(6)
    z, y = RR.honest(rng, P, 5, 3)
    z[0, 0, 0], y[0, 0, 0], z[1, 2, 255], y[1, 2, 255] = P.half, P.half - 3, -P.half, -P.half + 2   # the ends of the range
    coin = RR.coins(rng, 5, R62)
    acc, E = both(torch_mod, ctx, [(z, y)], coin, R62, LNM)
    ctx.prof_enable(True)
    ctx.prof_reset()
    ctx.reject([(z, y)], coin, R62, LNM)
    names = [n for n, _ in ctx.prof_read_kernels()]
    assert names == ["reject_stat_kernel<false>", "reject_decide_kernel"]
    assert [b for _, b in ctx.prof_read_kernels()] == [5 * 3 * 256 * 16, 5 * 3 * 16]
    ctx.trust_device_outputs(True)
    ctx.prof_reset()
    acc_t, E_t = both(torch_mod, ctx, [(z, y)], coin, R62, LNM)
    assert [n for n, _ in ctx.prof_read_kernels()] == ["reject_stat_kernel<true>", "reject_decide_kernel"] * 2
    ctx.prof_enable(False)
    ctx.trust_device_outputs(False)
    assert acc_t.tobytes() == acc.tobytes() and E_t.tobytes() == E.tobytes()


@pytest.mark.parametrize("N,R", [(64, R62), (1024, R62), (64, (1 << 31) - 1)])
def test_threshold_flip(torch_mod, N, R):
    """c* - delta accepts and c* + delta rejects, delta = ceil(R 2^-40): sixteen times the decidability margin."""
    ctx, P = ctx_of(N)
    z, y = RR.honest(np.random.default_rng(12 + N), P, 1, 3)
    E, flags = RR.proof_stats(P, list(zip(z[0].tolist(), y[0].tolist())))
    c = RR.largest_accepted_coin(P, E, LNM, R)
    delta = -(-R // (1 << 40))
    assert flags == 0 and 0 <= c - delta and c + delta < R
    coin = np.array([c - delta, c + delta], np.int64)
    z2, y2 = np.repeat(z, 2, 0), np.repeat(y, 2, 0)
    want = RR.run(P, [(z2, y2)], coin, R, LNM)
    assert [w[2] for w in want] == [True, False]
    acc, Eg = both(torch_mod, ctx, [(z2, y2)], coin, R, LNM)
    compare(want, acc, Eg, max_undecidable=0)
    assert acc.tolist() == [1, 0]


def test_argument_rules(torch_mod):
    ctx, P = ctx_of(1024)
    L = ctx._L
    assert L.rzk_reject_lnm(11.0) == LNM and reject_lnm(11.0) == LNM
    B = 2
    z, y = RR.honest(np.random.default_rng(3), P, B, 3)
    coin, acc, E = np.zeros(B, np.int64), np.zeros(B, np.uint8), np.zeros(B, np.int64)
    ctx._bind_torch_stream()
    dz, dy, dcoin, dacc, dE = (dev(torch_mod, a) for a in (z, y, coin, acc, E))
    for fn, pz, py, pc, pa, pe in ((L.rzk_reject_batch, z, y, coin, acc, E), (L.rzk_reject_batch_dev, dz, dy, dcoin, dacc, dE)):
        call = lambda parts=None, R=R62, lnM=LNM, E_=pe, B_=B, **kw: raw_call(ctx, fn, parts or [(pz, py)], pc, R, lnM, pa,
                                                                                E_, B_, **kw)
        assert call() == _lib.RZK_OK
        assert call(E_=None) == _lib.RZK_OK                       # E may be NULL
        assert call(R=2) == _lib.RZK_OK and call(R=R62) == _lib.RZK_OK
        assert call(R=1) == _lib.RZK_E_ARG and call(R=0) == _lib.RZK_E_ARG and call(R=R62 + 1) == _lib.RZK_E_ARG
        assert call(lnM=0.0) == _lib.RZK_OK
        assert call(lnM=-1e-9) == _lib.RZK_E_ARG and call(lnM=float("nan")) == _lib.RZK_E_ARG
        assert call(lnM=float("inf")) == _lib.RZK_E_ARG
        assert call(nparts=0) == _lib.RZK_E_ARG
        assert call(parts=[(pz, py)] * 5) == _lib.RZK_E_ARG
        assert call(parts=[(pz, py)] * 4, B_=0) == _lib.RZK_OK   # B == 0 is a no-op
        assert raw_call(ctx, fn, [], pc, R62, LNM, pa, pe, 0, nparts=9) == _lib.RZK_OK
        # rows N 2^24 vmax < 2^52: rows 1024 x 36 < 2^28 <=> rows <= 7281; the check comes before any access
        assert call(rows=[7282]) == _lib.RZK_E_ARG
        assert call(rows=[0]) == _lib.RZK_E_ARG
        ctx.synchronize()
    big = make_ctx(1024, 1, 3, 1, b=1 << 10)                        # verify_bound >= 2^24
    assert big.verify_bound >= 1 << 24
    assert raw_call(big, big._L.rzk_reject_batch, [(z, y)], coin, R62, LNM, acc, E, B) == _lib.RZK_E_ARG
    with pytest.raises(ValueError):
        ctx.reject([(z, y[:, :2])], coin, R62, LNM)
    with pytest.raises(ValueError):
        ctx.reject([], coin, R62, LNM)


# ---- statistics: derived tolerances, fixed seeds, SeededSampler ------------------------------------------------------------
def test_accept_rate_is_one_over_M(torch_mod):
    """Honest Open responses at N = 1024, B = 4096, lnM for alpha = 11: z = y + d r has |d r|_2 <= sigma / 11, so
    D_sigma(z) / (M D_{dr,sigma}(z)) <= 1 except with negligible probability and the accept rate is 1 / M = 0.3346; five
    binomial standard deviations sqrt(p (1 - p) / 4096) = 0.0074 on either side."""
    ctx, _ = ctx_of(1024)
    B = 4096
    s = SeededSampler(ctx, 2024)
    r, y, d = s.uniform(ctx.b, (B, ctx.k)), s.gauss(ctx.sigma, (B, ctx.k)), s.challenge((B,))
    z = ctx.open_response(y, r, d)
    coin, R = FS.draw_coins(s, (B,))
    assert R == ((1 << 31) - 1) ** 2 and R <= R62 and int(coin.min()) >= 0 and int(coin.max()) < R
    acc, _ = ctx.reject([(z, y)], coin, R, reject_lnm(11.0))
    ctx.synchronize()
    p = math.exp(-LNM)
    rate = float(acc.sum().item()) / B
    print("accept rate", rate, "expected", p)
    assert abs(rate - p) <= 5 * math.sqrt(p * (1 - p) / B)


def test_accepted_responses_do_not_lean_towards_v(torch_mod):
    """The leak the step removes.  N = 64, k = 3, B = 120000, z = y + v for ONE v of maximal norm (|v_j| = kappa b):
    over all proofs <z, v> has mean |v|^2 (19 standard errors sigma |v| / sqrt(B) from 0: asserted >= |v|^2 / 2); over
    the accepted ones z is distributed as D_sigma, <z, v> has mean 0 and standard deviation sigma |v|: |mean| within 5
    standard errors."""
    T = torch_mod
    ctx, P = ctx_of(64)
    B, k, N = 120000, ctx.k, 64
    s = SeededSampler(ctx, 77)
    y = s.gauss(ctx.sigma, (B, k))
    sign = T.from_numpy(np.random.default_rng(1).integers(0, 2, (k, N)) * 2 - 1).cuda()
    v = sign * P.vmax
    z = y + v                               # |y| stays far below (q-1)/2: no wrap
    v2 = int((v * v).sum().item())
    assert v2 == k * N * P.vmax ** 2 and v2 / (P.sigma * math.sqrt(v2) / math.sqrt(B)) >= 19
    coin, R = FS.draw_coins(s, (B,))
    acc, E = ctx.reject([(z, y)], coin, R, reject_lnm(11.0))
    ctx.synchronize()
    zv = (z * v).sum(dim=(1, 2))
    assert T.equal(E, v2 - 2 * zv)          # E = |v|^2 - 2 <z, v>
    mean_all = float(zv.double().mean().item())
    a = acc != 0
    n_acc = int(a.sum().item())
    mean_acc = float(zv[a].double().mean().item())
    print("mean <z,v> all", mean_all, "accepted", mean_acc, "n_acc", n_acc, "|v|^2", v2)
    assert mean_all >= v2 / 2
    assert n_acc > B / 5
    assert abs(mean_acc) <= 5 * P.sigma * math.sqrt(v2) / math.sqrt(n_acc)


# ---- the zero-knowledge provers end to end ------------------------------------------------------------------------------------
AUX = bytes(range(50, 82))


def replay(ctx, B, m, max_rounds, r_draws, prove):
    """The loop of fiat_shamir._zk_rounds restated with numpy indexing on the host: prove(idx, sampler) -> (outs, ok,
    parts) as device tensors.  Returns (accepted, rounds, per-proof outputs of the accepting round)."""
    acc_round = np.full(B, -1)
    kept = {}
    outs, ok, parts = prove(None)
    okn = ok.cpu().numpy() != 0
    coin, R = FS.draw_coins(r_draws, (B,))
    acc = ctx.reject(parts, coin, R, FS.zk_lnm(m))[0].cpu().numpy() != 0
    idx = np.arange(B)
    for rnd in range(max_rounds):
        for i, b in enumerate(idx):
            if acc[i] and okn[b]:
                acc_round[b] = rnd
                kept[b] = [o[i].cpu().numpy() for o in outs]
        idx = np.array([b for b in range(B) if okn[b] and acc_round[b] < 0], dtype=np.int64)
        if rnd + 1 == max_rounds or len(idx) == 0:
            break
        outs, _, parts = prove(idx)
        coin, R = FS.draw_coins(r_draws, (len(idx),))
        acc = ctx.reject(parts, coin, R, FS.zk_lnm(m))[0].cpu().numpy() != 0
    return acc_round, kept, okn


def check_zk(got_outs, ok, rounds, acc_round, kept, okn, fresh, max_rounds):
    ok, rounds = ok.cpu().numpy(), rounds.cpu().numpy()
    assert ok.tolist() == [int(a >= 0) for a in acc_round]
    for b in range(len(ok)):
        if ok[b]:
            assert rounds[b] == acc_round[b] < max_rounds
            for i in fresh:
                assert np.array_equal(got_outs[i][b].cpu().numpy(), kept[b][i]), (b, i)
        else:
            assert rounds[b] == 0
            for i in fresh:                     # a rejected attempt never appears in an output
                assert not got_outs[i][b].cpu().numpy().any(), (b, i)


@pytest.mark.parametrize("max_rounds", [64, 1])
def test_open_prove_zk(torch_mod, max_rounds):
    T = torch_mod
    N, B, seed = 64, 12, 31
    ctx, A = keyed_ctx(N, 1, 3, 1, 36, seed=41)
    P = P_of(ctx)
    x = ctx.sample_uniform(9, 0, ctx.half, (B, 1))
    c, t, z, ok, r, rounds = FS.open_prove_zk(ctx, x, SeededSampler(ctx, seed), aux=AUX, max_rounds=max_rounds)
    c0 = FS.open_prove_sampled(ctx, x, SeededSampler(ctx, seed), aux=AUX)[0]
    assert T.equal(c, c0)                                   # c is round 0's c
    s2 = SeededSampler(ctx, seed)
    r2 = s2.uniform(ctx.b, (B, ctx.k))
    assert T.equal(r, r2)

    def prove(idx):
        xs, rs = (x, r2) if idx is None else (x[T.from_numpy(idx).cuda()], r2[T.from_numpy(idx).cuda()])
        y = s2.gauss(ctx.sigma, (xs.shape[0], ctx.k))
        cc, tt, zz, okk = FS.open_prove(ctx, xs, rs, y, aux=AUX)
        return (cc, tt, zz), okk, [(zz, y)]

    acc_round, kept, okn = replay(ctx, B, 1, max_rounds, s2, prove)
    check_zk((c, t, z), ok, rounds, acc_round, kept, okn, (1, 2), max_rounds)
    okh = ok.cpu().numpy().astype(bool)
    if max_rounds == 1:
        assert okn.all() and not okh.all() and okh.any()     # 12 proofs at 1 / M = 0.33: some of each (fixed seed)
    else:
        assert okh.all() and rounds.max().item() >= 1
    v = FS.open_verify(ctx, c, t, z, aux=AUX).cpu().numpy().astype(bool)
    assert (v[okh]).all()
    cn, tn, zn = (a.cpu().numpy() for a in (c, t, z))
    d, _ = ref_challenge(ctx, A, OPEN, None, [cn, tn], AUX)
    for b in np.nonzero(okh)[0]:
        assert O.open_verify(P, A, zn[b], tn[b], cn[b], d[b]) == 1


@pytest.mark.parametrize("max_rounds", [64, 1])
def test_linear_prove_zk(torch_mod, max_rounds):
    T = torch_mod
    N, B, seed = 64, 10, 32
    ctx, A = keyed_ctx(N, 1, 3, 1, 36, seed=42)
    P = P_of(ctx)
    g, x = ctx.sample_uniform(9, 0, ctx.half, (B,)), ctx.sample_uniform(9, 1, ctx.half, (B, 1))
    out = FS.linear_prove_zk(ctx, g, x, SeededSampler(ctx, seed), aux=AUX, max_rounds=max_rounds)
    c, cp, t, tp, u, z, zp, ok, r, rp, rounds = out
    o0 = FS.linear_prove_sampled(ctx, g, x, SeededSampler(ctx, seed), aux=AUX)
    assert T.equal(c, o0[0]) and T.equal(cp, o0[1])
    s2 = SeededSampler(ctx, seed)
    r2, rp2 = s2.uniform(ctx.b, (B, ctx.k)), s2.uniform(ctx.b, (B, ctx.k))

    def prove(idx):
        sel = (lambda a: a) if idx is None else (lambda a: a[T.from_numpy(idx).cuda()])
        n = B if idx is None else len(idx)
        y, yp = s2.gauss(ctx.sigma, (n, ctx.k)), s2.gauss(ctx.sigma, (n, ctx.k))
        o = FS.linear_prove(ctx, sel(g), sel(x), sel(r2), sel(rp2), y, yp, aux=AUX)
        return o[:7], o[7], [(o[5], y), (o[6], yp)]

    acc_round, kept, okn = replay(ctx, B, 2, max_rounds, s2, prove)
    check_zk(out[:7], ok, rounds, acc_round, kept, okn, (2, 3, 4, 5, 6), max_rounds)
    okh = ok.cpu().numpy().astype(bool)
    if max_rounds == 1:
        assert not okh.all()
    else:
        assert okh.all()
    v = FS.linear_verify(ctx, c, cp, g, t, tp, u, z, zp, aux=AUX).cpu().numpy().astype(bool)
    assert v[okh].all()
    h = [a.cpu().numpy() for a in (c, cp, g, t, tp, u, z, zp)]
    d, _ = ref_challenge(ctx, A, LINEAR, None, h[:6], AUX)
    for b in np.nonzero(okh)[0]:
        assert O.linear_verify(P, A, h[6][b], h[7][b], h[0][b], h[1][b], h[2][b], h[3][b], h[4][b], h[5][b], d[b]) == 1


@pytest.mark.parametrize("max_rounds", [64, 1])
def test_sum_prove_zk(torch_mod, max_rounds):
    T = torch_mod
    N, B, V, seed = 64, 8, 2, 33
    ctx, A = keyed_ctx(N, 1, 3, 1, 36, seed=43)
    P = P_of(ctx)
    gs, xs = ctx.sample_uniform(9, 0, ctx.half, (B, V)), ctx.sample_uniform(9, 1, ctx.half, (B, V, 1))
    out = FS.sum_prove_zk(ctx, gs, xs, SeededSampler(ctx, seed), aux=AUX, max_rounds=max_rounds)
    cs, cp, ts, tp, u, zs, zp, ok, rs, rp, rounds = out
    o0 = FS.sum_prove_sampled(ctx, gs, xs, SeededSampler(ctx, seed), aux=AUX)
    assert T.equal(cs, o0[0]) and T.equal(cp, o0[1])
    s2 = SeededSampler(ctx, seed)
    rs2, rp2 = s2.uniform(ctx.b, (B, V, ctx.k)), s2.uniform(ctx.b, (B, ctx.k))

    def prove(idx):
        sel = (lambda a: a) if idx is None else (lambda a: a[T.from_numpy(idx).cuda()])
        n = B if idx is None else len(idx)
        ys, yp = s2.gauss(ctx.sigma, (n, V, ctx.k)), s2.gauss(ctx.sigma, (n, ctx.k))
        o = FS.sum_prove(ctx, sel(gs), sel(xs), sel(rs2), sel(rp2), ys, yp, aux=AUX)
        return o[:7], o[7], [(o[5], ys), (o[6], yp)]

    acc_round, kept, okn = replay(ctx, B, V + 1, max_rounds, s2, prove)
    check_zk(out[:7], ok, rounds, acc_round, kept, okn, (2, 3, 4, 5, 6), max_rounds)
    okh = ok.cpu().numpy().astype(bool)
    if max_rounds == 1:
        assert not okh.all()
    else:
        assert okh.all()
    v = FS.sum_verify(ctx, cs, cp, gs, ts, tp, u, zs, zp, aux=AUX).cpu().numpy().astype(bool)
    assert v[okh].all()
    h = dict(cp=cp, cs=cs, gs=gs, tp=tp, ts=ts, u=u, zs=zs, zp=zp)
    h = {k_: a.cpu().numpy() for k_, a in h.items()}
    d, _ = ref_challenge(ctx, A, SUM, V, [h[k_] for k_ in ("cp", "cs", "gs", "tp", "ts", "u")], AUX)
    for b in np.nonzero(okh)[0]:
        assert O.sum_verify(P, A, h["zs"][b], h["zp"][b], h["cs"][b], h["cp"][b], h["gs"][b], h["ts"][b], h["tp"][b],
                            h["u"][b], d[b]) == 1
