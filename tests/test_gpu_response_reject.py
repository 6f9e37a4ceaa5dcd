"""The response and its rejection test in one call (rzk_*_response_reject_batch[_dev], Context.*_response_reject,
DESIGN.md §17) on the GPU.  Reference for every case: tests/reject_ref.py on (z, y) with z from the existing
Context.*_response; z and E are compared exactly, accept on every decidable case (reject_ref: |E - T| > 2 sigma^2 2^-44;
with integer E and a band of about 5e-5 honest data gives none, and every test first asserts from the reference alone
that at most 2 of its cases are undecidable).  Where the fused kernel runs (N = 512, 1024) the recorded launches name
response_stat_kernel and no reject_stat_kernel; on the fallback shapes the opposite.  The zero-knowledge provers are
compared bit for bit with the replay of test_gpu_reject.py: *_prove, then Context.reject, round by round."""
import ctypes as C

import numpy as np
import pytest

import reject_ref as RR
from ring_zk_amd import _lib, RzkError, synth
from ring_zk_amd import fiat_shamir as FS
from ring_zk_amd.backend import SeededSampler
from test_gpu_baseline_shapes import dev, make_ctx, torch_mod  # noqa: F401
from test_gpu_fiat_shamir import keyed_ctx
from test_gpu_reject import check_zk, replay

pytestmark = pytest.mark.gpu

R62 = 1 << 62
LNM = 12 / 11 + 1 / 242
AUX = bytes(range(50, 82))


def ctx_of(N, shape=(1, 3, 1), env=None):
    ctx = make_ctx(N, *shape, env=env, kappa=min(N, 36))
    return ctx, RR.params_of(ctx)


def inputs(rng, ctx, P, kind, B, V=1):
    """honest inputs of one call, in the argument order of Context.*_response"""
    N, k = ctx.N, ctx.k
    y = lambda *lead: synth.gauss(rng, lead + (k, N), P.sigma)
    r = lambda *lead: synth.small(rng, lead + (k, N), ctx.b)
    d = synth.challenge(rng, (B,), N, ctx.kappa)
    if kind == "open":
        return [y(B), r(B), d]
    if kind == "linear":
        return [y(B), y(B), r(B), r(B), d]
    return [y(B, V), y(B), r(B, V), r(B), d]


def chain(ctx, kind, ins):
    """(response slabs, parts of Context.reject) from the existing response entry point"""
    if kind == "open":
        z = ctx.open_response(*ins)
        return (z,), [(z, ins[0])]
    if kind == "linear":
        z, zp = ctx.linear_response(*ins)
        return (z, zp), [(z, ins[0]), (zp, ins[1])]
    zs, zp = ctx.sum_response(*ins)
    return (zs, zp), [(zs, ins[0]), (zp, ins[1])]


def fused(ctx, kind, ins, coin, R, lnM):
    out = getattr(ctx, kind + "_response_reject")(*ins, coin, R, lnM)
    return tuple(out[:-2]), out[-2], out[-1]


def fused_both(torch, ctx, kind, ins, coin, R, lnM):
    """(z slabs, accept, E) from the host entry point after checking that the device entry point gives the same bytes"""
    zs, acc, E = fused(ctx, kind, ins, coin, R, lnM)
    dzs, dacc, dE = fused(ctx, kind, [dev(torch, a) for a in ins], dev(torch, coin), R, lnM)
    ctx.synchronize()
    assert all(np.array_equal(dz.cpu().numpy(), z) for dz, z in zip(dzs, zs))
    assert np.array_equal(dacc.cpu().numpy(), acc) and np.array_equal(dE.cpu().numpy(), E)
    return zs, acc, E


def compare(want, acc, E, max_undecidable=2):
    assert RR.count_undecidable(want) <= max_undecidable   # from the reference alone
    for b, w in enumerate(want):
        assert int(E[b]) == w[0], b
        if w[3]:
            assert int(acc[b]) == int(w[2]), b
        assert not (w[1] and acc[b]), b


def check(torch, ctx, P, kind, ins, coin, R=R62, lnM=LNM, trusted=False, max_undecidable=2):
    """fused call against chain + reference; returns (reference results, accept, E)"""
    zs_ref, parts = chain(ctx, kind, ins)
    want = RR.run(P, parts, coin, R, lnM, trusted=trusted)
    zs, acc, E = fused_both(torch, ctx, kind, ins, coin, R, lnM)
    assert all(np.array_equal(a, b) for a, b in zip(zs, zs_ref))
    compare(want, acc, E, max_undecidable)
    return want, acc, E


def launches(ctx, call):
    ctx.prof_enable(True)
    ctx.prof_reset()
    call()
    ctx.synchronize()
    recs = ctx.prof_read_kernels()
    ctx.prof_enable(False)
    return recs


def assert_path(names, is_fused):
    has = lambda prefix: any(n.startswith(prefix) for n in names)
    assert has("response_stat_kernel") == is_fused and has("reject_stat_kernel") == (not is_fused), names
    assert names[-1] == "reject_decide_kernel"


OPEN_CASES = [(512, None, True), (1024, None, True), (4, None, False), (64, None, False), (256, None, False),
              (2048, None, False), (1024, {"RZK_SHIFT": 0}, False)]


@pytest.mark.parametrize("N,env,is_fused", OPEN_CASES)
def test_open_matches_chain_and_reference(torch_mod, N, env, is_fused):
    ctx, P = ctx_of(N, env=env)
    for B in (1, 3, 5):
        rng = np.random.default_rng(2000 * N + B)
        ins, coin = inputs(rng, ctx, P, "open", B), RR.coins(rng, B, R62)
        want, _, _ = check(torch_mod, ctx, P, "open", ins, coin)
        assert all(w[1] == 0 for w in want)
    names = [n for n, _ in launches(ctx, lambda: fused(ctx, "open", ins, coin, R62, LNM))]
    assert_path(names, is_fused)
    if is_fused:
        assert names == ["response_stat_kernel<%d, false>" % (N.bit_length() - 1), "reject_decide_kernel"]


def test_linear(torch_mod):
    ctx, P = ctx_of(512)
    for B in (1, 3):
        rng = np.random.default_rng(31 + B)
        ins, coin = inputs(rng, ctx, P, "linear", B), RR.coins(rng, B, R62)
        want, _, _ = check(torch_mod, ctx, P, "linear", ins, coin, lnM=FS.zk_lnm(2))
        assert all(w[1] == 0 for w in want)
    assert_path([n for n, _ in launches(ctx, lambda: fused(ctx, "linear", ins, coin, R62, LNM))], True)


@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("B", [1, 3])
def test_sum_partial_layout(torch_mod, V, B):
    """two launches into one [B][(V + 1) k] table: the summands with group = V from offset 0, z' from offset V k"""
    ctx, P = ctx_of(512)
    rng = np.random.default_rng(41 + 10 * V + B)
    ins, coin = inputs(rng, ctx, P, "sum", B, V), RR.coins(rng, B, R62)
    want, _, _ = check(torch_mod, ctx, P, "sum", ins, coin, lnM=FS.zk_lnm(V + 1))
    assert all(w[1] == 0 for w in want)
    names = [n for n, _ in launches(ctx, lambda: fused(ctx, "sum", ins, coin, R62, LNM))]
    assert names == ["response_stat_kernel<9, false>"] * 2 + ["reject_decide_kernel"]
    # one summand's rows moved to another proof / summand change exactly the proofs involved
    if B > 1:
        ins2 = [a.copy() for a in ins]
        ins2[0][0, V - 1], ins2[0][B - 1, 0] = ins[0][B - 1, 0], ins[0][0, V - 1]
        check(torch_mod, ctx, P, "sum", ins2, coin, lnM=FS.zk_lnm(V + 1))


def test_open_252(torch_mod):
    ctx, P = ctx_of(512, shape=(2, 5, 2))
    rng = np.random.default_rng(252)
    B = 3
    ins, coin = inputs(rng, ctx, P, "open", B), RR.coins(rng, B, R62)
    want, _, _ = check(torch_mod, ctx, P, "open", ins, coin)
    assert all(w[1] == 0 for w in want)
    assert_path([n for n, _ in launches(ctx, lambda: fused(ctx, "open", ins, coin, R62, LNM))], True)


def test_word_path_of_the_fused_kernel(torch_mod):
    """An r with entries of magnitude 200, which the packed-byte rotation refuses, takes the word rotation inside the fused
    kernel; a d with a coefficient 2 (over an all-ones r) stays on bytes.  Both reach |v| > kappa b: flagged, E still the
    exact integer of the reference, accept = 0.  RZK_SHIFT_BYTES=0 runs the word instantiation on honest data."""
    ctx, P = ctx_of(512)
    rng = np.random.default_rng(77)
    B = 4
    y, r, d = inputs(rng, ctx, P, "open", B)
    r[1] = synth.small(rng, r[1].shape, 1) * 200
    r[2], d[2] = 1, np.where(d[2] != 0, 1, 0)          # coefficient N - 1 of d r is the plain sum of d: kappa, and with
    d[2, np.nonzero(d[2])[0][0]] = 2                    # one coefficient 2 it is kappa + 1 > kappa b
    coin = np.zeros(B, np.int64)
    want, acc, _ = check(torch_mod, ctx, P, "open", [y, r, d], coin, max_undecidable=0)
    assert [w[1] for w in want] == [0, RR.VMAX, RR.VMAX, 0] and acc.tolist() == [1, 0, 0, 1]
    ctx0, _ = ctx_of(512, env={"RZK_SHIFT_BYTES": 0})
    ins = inputs(rng, ctx0, P, "open", 3)
    coin = RR.coins(rng, 3, R62)
    check(torch_mod, ctx0, P, "open", ins, coin)
    names = [n for n, _ in launches(ctx0, lambda: fused(ctx0, "open", ins, coin, R62, LNM))]
    assert names == ["response_stat_kernel<9, false, false>", "reject_decide_kernel"]


def test_edges_one_cause_each(torch_mod):
    ctx, P = ctx_of(512)
    N, k, B = 512, 3, 5
    rng = np.random.default_rng(99)
    y0, r0, d0 = inputs(rng, ctx, P, "open", B)
    coin0 = np.zeros(B, np.int64)      # u = 1 / R: every honest proof is accepted
    _, acc, _ = check(torch_mod, ctx, P, "open", [y0, r0, d0], coin0, max_undecidable=0)
    assert acc.tolist() == [1] * B
    # r = 0: z = y; sum c^2 = (verify_bound + 1)^2 - 1 passes, (verify_bound + 1)^2 raises the norm flag
    y, r = y0.copy(), r0.copy()
    r[1], r[3] = 0, 0
    y[1, 2], y[3, 0] = RR.norm_edge_poly(P, 0), RR.norm_edge_poly(P, 1)
    want, acc, _ = check(torch_mod, ctx, P, "open", [y, r, d0], coin0, max_undecidable=0)
    assert [w[1] for w in want] == [0, 0, 0, RR.NORM, 0] and acc.tolist() == [1, 1, 1, 0, 1]
    # y = +-(q-1)/2 where v != 0: z wraps; |z| near (q-1)/2 raises the norm flag of that proof only, E stays exact
    y = y0.copy()
    zc, _ = chain(ctx, "open", [y0, r0, d0])
    v = zc[0] - y0
    pos = np.argwhere(v[2] != 0)
    assert len(pos) >= 4
    for n_, (j, i) in enumerate(pos[:4]):               # two that wrap (y at the end v points to), two that do not
        sign = 1 if v[2, j, i] > 0 else -1
        y[2, j, i] = sign * P.half if n_ < 2 else -sign * P.half
    want, acc, _ = check(torch_mod, ctx, P, "open", [y, r0, d0], coin0, max_undecidable=0)
    assert [w[1] for w in want] == [0, 0, RR.NORM, 0, 0] and acc.tolist() == [1, 1, 0, 1, 1]
    zf, _, _ = fused(ctx, "open", [y, r0, d0], coin0, R62, LNM)
    assert (np.abs(zf[0][2] - y[2]) > P.q - 100).any()      # the wrap is in the data
    # coins 0, R - 1, R
    for R in (1000, R62):
        coin = np.array([0, R - 1, R, 0, R - 1], np.int64)
        want, acc, _ = check(torch_mod, ctx, P, "open", [y0, r0, d0], coin, R=R, max_undecidable=0)
        assert [w[1] for w in want] == [0, 0, RR.COIN, 0, 0] and acc.tolist() == [1, 0, 0, 1, 0]
    # a non-canonical y, r, d, each in a proof of its own: accept = 0 there, the fault is reported, the others are unaffected
    _, acc_ok, E_ok = fused(ctx, "open", [y0, r0, d0], coin0, R62, LNM)
    for which, where, bad in ((0, (1, 2, 7), P.half + 1), (1, (3, 0, 511), (1 << 32) + 1), (2, (4, 100), -P.half - 1),
                              (0, (0, 1, 64), -(1 << 40))):
        ins = [y0.copy(), r0.copy(), d0.copy()]
        ins[which][where] = bad
        with pytest.raises(RzkError) as e:
            fused(ctx, "open", ins, coin0, R62, LNM)
        assert e.value.status == _lib.RZK_E_ARG
        _, dacc, dE = fused(ctx, "open", [dev(torch_mod, a) for a in ins], dev(torch_mod, coin0), R62, LNM)
        with pytest.raises(RzkError) as e:
            ctx.synchronize()                   # rzk_ctx_check_inputs' word, reported once
        assert e.value.status == _lib.RZK_E_ARG
        ctx.synchronize()
        victim = where[0]
        assert dacc.cpu().numpy().tolist() == [int(b != victim) for b in range(B)]
        others = [b for b in range(B) if b != victim]
        assert np.array_equal(dE.cpu().numpy()[others], E_ok[others])
    _, acc, _ = fused(ctx, "open", [y0, r0, d0], coin0, R62, LNM)   # the fault does not leak into the next call
    assert acc.tolist() == [1] * B


def test_trusted_mode_gives_identical_bytes(torch_mod):
    ctx, P = ctx_of(1024)
    rng = np.random.default_rng(6)
    ins, coin = inputs(rng, ctx, P, "open", 5), RR.coins(rng, 5, R62)
    zs, acc, E = fused_both(torch_mod, ctx, "open", ins, coin, R62, LNM)
    ctx.trust_device_outputs(True)
    names = [n for n, _ in launches(ctx, lambda: fused(ctx, "open", ins, coin, R62, LNM))]
    assert names == ["response_stat_kernel<10, true>", "reject_decide_kernel"]
    want, acc_t, E_t = check(torch_mod, ctx, P, "open", ins, coin, trusted=True)
    zs_t, _, _ = fused(ctx, "open", ins, coin, R62, LNM)
    ctx.trust_device_outputs(False)
    assert acc_t.tobytes() == acc.tobytes() and E_t.tobytes() == E.tobytes() and zs_t[0].tobytes() == zs[0].tobytes()


@pytest.mark.parametrize("kind,V", [("open", 1), ("sum", 3)])
def test_grid_stride_trips(torch_mod, kind, V):
    """B = 100 with the grid sized for one CU (16 workgroups of 4 wavefronts): 300 / 900 + 300 rows, several trips per team"""
    ctx1, P = ctx_of(512, env={"RZK_GRID_CUS": 1})
    ctx, _ = ctx_of(512)
    B = 100
    rng = np.random.default_rng(177 + V)
    ins, coin = inputs(rng, ctx, P, kind, B, V), RR.coins(rng, B, R62)
    lnM = FS.zk_lnm(V + 1 if kind == "sum" else 1)
    zs1, acc1, E1 = fused_both(torch_mod, ctx1, kind, ins, coin, R62, lnM)
    want, acc, E = check(torch_mod, ctx, P, kind, ins, coin, lnM=lnM)
    zs, _, _ = fused(ctx, kind, ins, coin, R62, lnM)
    assert np.array_equal(acc1, acc) and np.array_equal(E1, E) and all(np.array_equal(a, b) for a, b in zip(zs1, zs))


def test_threshold_flip(torch_mod):
    """as test_gpu_reject.py::test_threshold_flip, through the fused entry point: c* - delta accepts, c* + delta rejects"""
    ctx, P = ctx_of(1024)
    R = R62
    rng = np.random.default_rng(12 + 1024)
    y, r, d = inputs(rng, ctx, P, "open", 1)
    (z,), _ = chain(ctx, "open", [y, r, d])
    E, flags = RR.proof_stats(P, list(zip(z[0].tolist(), y[0].tolist())))
    c = RR.largest_accepted_coin(P, E, LNM, R)
    delta = -(-R // (1 << 40))
    assert flags == 0 and 0 <= c - delta and c + delta < R
    coin = np.array([c - delta, c + delta], np.int64)
    ins = [np.repeat(a, 2, 0) for a in (y, r, d)]
    want, acc, _ = check(torch_mod, ctx, P, "open", ins, coin, R=R, max_undecidable=0)
    assert [w[2] for w in want] == [True, False] and acc.tolist() == [1, 0]


def ptr(a):
    return C.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data) if a is not None else None


def test_argument_rules(torch_mod):
    ctx, P = ctx_of(1024)
    L = ctx._L
    B = 2
    rng = np.random.default_rng(3)
    y, r, d = inputs(rng, ctx, P, "open", B)
    coin, acc, E, z = np.zeros(B, np.int64), np.zeros(B, np.uint8), np.zeros(B, np.int64), np.zeros_like(y)
    ctx._bind_torch_stream()
    host = dict(y=y, r=r, d=d, coin=coin, z=z, acc=acc, E=E)
    devs = {key: dev(torch_mod, a) for key, a in host.items()}
    for fn, a in ((L.rzk_open_response_reject_batch, host), (L.rzk_open_response_reject_batch_dev, devs)):
        def call(R=R62, lnM=LNM, B_=B, **null):
            g = lambda key: None if key in null else ptr(a[key])
            return fn(ctx._h, g("y"), g("r"), g("d"), g("coin"), R, lnM, g("z"), g("acc"), g("E"), B_)
        assert call() == _lib.RZK_OK
        assert call(E=1) == _lib.RZK_OK                            # E may be NULL
        for key in ("y", "r", "d", "coin", "z", "acc"):
            assert call(**{key: 1}) == _lib.RZK_E_ARG, key
        assert call(R=2) == _lib.RZK_OK and call(R=R62) == _lib.RZK_OK
        assert call(R=1) == _lib.RZK_E_ARG and call(R=0) == _lib.RZK_E_ARG and call(R=R62 + 1) == _lib.RZK_E_ARG
        assert call(lnM=0.0) == _lib.RZK_OK
        assert call(lnM=-1e-9) == _lib.RZK_E_ARG and call(lnM=float("nan")) == _lib.RZK_E_ARG
        assert call(lnM=float("inf")) == _lib.RZK_E_ARG
        assert call(B_=0, y=1, z=1) == _lib.RZK_OK                 # B == 0 is a no-op
        ctx.synchronize()
    # Linear and Sum: NULL pointers, V = 0
    lin = [ptr(devs[key]) for key in ("y", "y", "r", "r", "d", "coin")]
    zp = torch_mod.zeros_like(devs["z"])
    out = [ptr(devs["z"]), ptr(zp), ptr(devs["acc"]), ptr(devs["E"])]
    assert L.rzk_linear_response_reject_batch_dev(ctx._h, *lin, R62, LNM, *out, B) == _lib.RZK_OK
    for i in range(6):
        bad = list(lin)
        bad[i] = None
        assert L.rzk_linear_response_reject_batch_dev(ctx._h, *bad, R62, LNM, *out, B) == _lib.RZK_E_ARG
    ys = devs["y"].reshape(B, 1, ctx.k, ctx.N)
    sm = [ptr(ys), ptr(devs["y"]), ptr(ys), ptr(devs["r"]), ptr(devs["d"]), ptr(devs["coin"])]
    assert L.rzk_sum_response_reject_batch_dev(ctx._h, 1, *sm, R62, LNM, *out, B) == _lib.RZK_OK
    assert L.rzk_sum_response_reject_batch_dev(ctx._h, 0, *sm, R62, LNM, *out, B) == _lib.RZK_E_ARG
    assert L.rzk_sum_response_reject_batch(ctx._h, 0, *sm, R62, LNM, *out, B) == _lib.RZK_E_ARG
    assert L.rzk_sum_response_reject_batch_dev(ctx._h, 1, *sm, R62 + 1, LNM, *out, B) == _lib.RZK_E_ARG
    ctx.synchronize()
    # rows N 2^24 kappa b < 2^52 at its edge: (V + 1) k 1024 x 36 < 2^28 <=> (V + 1) k <= 7281 = 2427 x 3
    zeros = lambda *shape: torch_mod.zeros(shape, dtype=torch_mod.int64, device="cuda")
    for V, rc in ((2426, _lib.RZK_OK), (2427, _lib.RZK_E_ARG)):
        ys_, rs_, zs_, one, zp_ = zeros(1, V, ctx.k, ctx.N), zeros(1, V, ctx.k, ctx.N), zeros(1, V, ctx.k, ctx.N), zeros(1, ctx.k, ctx.N), zeros(1, ctx.k, ctx.N)
        d_, coin_ = zeros(1, ctx.N), zeros(1)
        args = [ptr(ys_), ptr(one), ptr(rs_), ptr(one), ptr(d_), ptr(coin_)]
        res = [ptr(zs_), ptr(zp_), ptr(devs["acc"]), ptr(devs["E"])]
        assert L.rzk_sum_response_reject_batch_dev(ctx._h, V, *args, R62, LNM, *res, 1) == rc, V
        ctx.synchronize()
    big = make_ctx(1024, 1, 3, 1, b=1 << 10)                        # verify_bound >= 2^24
    assert big.verify_bound >= 1 << 24
    assert big._L.rzk_open_response_reject_batch(big._h, ptr(y), ptr(r), ptr(d), ptr(coin), R62, LNM, ptr(z), ptr(acc), ptr(E),
                                                 B) == _lib.RZK_E_ARG
    with pytest.raises(ValueError):
        ctx.open_response_reject(y, r[:, :2], d, coin, R62, LNM)


# ---- the zero-knowledge provers: bit for bit the parent's loop (*_prove, then Context.reject) ---------------------------
def test_open_prove_zk_replays_and_retries_without_commit(torch_mod):
    T = torch_mod
    N, B, seed = 512, 64, 131
    ctx, A = keyed_ctx(N, 1, 3, 1, 36, seed=141)
    k = ctx.k
    x = ctx.sample_uniform(9, 0, ctx.half, (B, 1))
    # what a commit launch of this batch looks like, from a run of its own: (name, bytes per proof)
    s0 = SeededSampler(ctx, 7)
    r0, y0 = s0.uniform(ctx.b, (B, k)), s0.gauss(ctx.sigma, (B, k))
    commit_sig = [(n, nb // B) for n, nb in launches(ctx, lambda: ctx.open_commit(x, r0, y0))]
    assert commit_sig
    ctx.prof_enable(True)
    ctx.prof_reset()
    c, t, z, ok, r, rounds = FS.open_prove_zk(ctx, x, SeededSampler(ctx, seed), aux=AUX, max_rounds=64)
    ctx.synchronize()
    recs = ctx.prof_read_kernels()
    ctx.prof_enable(False)
    s2 = SeededSampler(ctx, seed)
    r2 = s2.uniform(ctx.b, (B, k))
    assert T.equal(r, r2)

    def prove(idx):
        xs, rs = (x, r2) if idx is None else (x[T.from_numpy(idx).cuda()], r2[T.from_numpy(idx).cuda()])
        y = s2.gauss(ctx.sigma, (xs.shape[0], k))
        cc, tt, zz, okk = FS.open_prove(ctx, xs, rs, y, aux=AUX)
        return (cc, tt, zz), okk, [(zz, y)]

    acc_round, kept, okn = replay(ctx, B, 1, 64, s2, prove)
    check_zk((c, t, z), ok, rounds, acc_round, kept, okn, (1, 2), 64)
    assert T.equal(c, FS.open_prove_sampled(ctx, x, SeededSampler(ctx, seed), aux=AUX)[0])
    assert bool(ok.all()) and int(rounds.max()) >= 1
    # the recorded launches, one segment per round (each ends with the decision)
    segments, cur = [], []
    for rec in recs:
        cur.append(rec)
        if rec[0] == "reject_decide_kernel":
            segments.append(cur)
            cur = []
    assert not cur and len(segments) == int(rounds.max()) + 1
    seg0 = [(n, nb // B) for n, nb in segments[0]]
    assert any(seg0[i:i + len(commit_sig)] == commit_sig for i in range(len(seg0)))     # round 0 commits
    resp0 = [nb for n, nb in segments[0] if n.startswith("response_stat_kernel")]
    assert len(resp0) == 1 and resp0[0] % B == 0
    assert not any(n.startswith("reject_stat_kernel") for n, _ in recs)
    for seg in segments[1:]:
        resp = [nb for n, nb in seg if n.startswith("response_stat_kernel")]
        assert len(resp) == 1 and resp[0] % (resp0[0] // B) == 0
        pending = resp[0] // (resp0[0] // B)                  # proofs of this round
        assert 0 < pending < B
        commit_like = {(n, per * pending) for n, per in commit_sig}
        assert not [rec for rec in seg if rec in commit_like], seg


def test_linear_prove_zk_replays(torch_mod):
    T = torch_mod
    N, B, seed = 512, 64, 132
    ctx, A = keyed_ctx(N, 1, 3, 1, 36, seed=142)
    g, x = ctx.sample_uniform(9, 0, ctx.half, (B,)), ctx.sample_uniform(9, 1, ctx.half, (B, 1))
    out = FS.linear_prove_zk(ctx, g, x, SeededSampler(ctx, seed), aux=AUX, max_rounds=64)
    ok, rounds = out[7], out[10]
    s2 = SeededSampler(ctx, seed)
    r2, rp2 = s2.uniform(ctx.b, (B, ctx.k)), s2.uniform(ctx.b, (B, ctx.k))
    assert T.equal(out[8], r2) and T.equal(out[9], rp2)

    def prove(idx):
        sel = (lambda a: a) if idx is None else (lambda a: a[T.from_numpy(idx).cuda()])
        n = B if idx is None else len(idx)
        y, yp = s2.gauss(ctx.sigma, (n, ctx.k)), s2.gauss(ctx.sigma, (n, ctx.k))
        o = FS.linear_prove(ctx, sel(g), sel(x), sel(r2), sel(rp2), y, yp, aux=AUX)
        return o[:7], o[7], [(o[5], y), (o[6], yp)]

    acc_round, kept, okn = replay(ctx, B, 2, 64, s2, prove)
    check_zk(out[:7], ok, rounds, acc_round, kept, okn, (2, 3, 4, 5, 6), 64)
    assert bool(ok.all()) and int(rounds.max()) >= 1


def test_sum_prove_zk_replays(torch_mod):
    T = torch_mod
    N, B, V, seed = 512, 64, 2, 133
    ctx, A = keyed_ctx(N, 1, 3, 1, 36, seed=143)
    gs, xs = ctx.sample_uniform(9, 0, ctx.half, (B, V)), ctx.sample_uniform(9, 1, ctx.half, (B, V, 1))
    out = FS.sum_prove_zk(ctx, gs, xs, SeededSampler(ctx, seed), aux=AUX, max_rounds=64)
    ok, rounds = out[7], out[10]
    s2 = SeededSampler(ctx, seed)
    rs2, rp2 = s2.uniform(ctx.b, (B, V, ctx.k)), s2.uniform(ctx.b, (B, ctx.k))
    assert T.equal(out[8], rs2) and T.equal(out[9], rp2)

    def prove(idx):
        sel = (lambda a: a) if idx is None else (lambda a: a[T.from_numpy(idx).cuda()])
        n = B if idx is None else len(idx)
        ys, yp = s2.gauss(ctx.sigma, (n, V, ctx.k)), s2.gauss(ctx.sigma, (n, ctx.k))
        o = FS.sum_prove(ctx, sel(gs), sel(xs), sel(rs2), sel(rp2), ys, yp, aux=AUX)
        return o[:7], o[7], [(o[5], ys), (o[6], yp)]

    acc_round, kept, okn = replay(ctx, B, V + 1, 64, s2, prove)
    check_zk(out[:7], ok, rounds, acc_round, kept, okn, (2, 3, 4, 5, 6), 64)
    assert bool(ok.all()) and int(rounds.max()) >= 1
