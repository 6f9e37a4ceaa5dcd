"""Packed-byte rotations of shift_row_kernel (GPU): response rows whose operands satisfy |d|_1 * 2 |v|_inf <= 255 rotate
bytes instead of words (ByteGeo, ring_zk_amd/csrc/rzk_core.h; RZK_SHIFT_BYTES, default 1).  Every result is compared
byte for byte with the oracle AND with the same call on a context created under RZK_SHIFT_BYTES=0, checked and trusted:

  * the Open, Linear and Sum responses at N = 512 / 1024 with an odd and a multiple batch (part-filled last workgroup);
  * the edge of the condition for |v|_inf = 1, 2, 3: floor(255 / (2 |v|_inf)) non-zeros and one more (which the kernel
    hands to the word path), with every byte sum at its extreme (v = +b everywhere, d all +1, and the mirror image);
  * rotations by 0..3 (every byte alignment), N-1, N/2 and next to the boundaries of a lane's outputs;
  * a zero multiplier, a dense +-3 multiplier, entries of magnitude 2;
  * non-canonical coefficients in r, y or d fail the call as before.
Which path a term takes is a per-wavefront decision invisible from outside; the predicate itself is pinned on the CPU
(tests/test_emul_shift_bytes.py).  Reference: z = y + r (.) d, src/prove/open.rs:113-115, linear.rs:135-150,
sum.rs:182-200.
"""
import numpy as np
import pytest

from oracle import oracle as O
from ring_zk_amd import synth

from test_gpu_baseline_shapes import P_of, dev, make_ctx, sum_inputs, torch_mod  # noqa: F401

pytestmark = pytest.mark.gpu

_ctxs = {}


def ctx_pair(N):
    """(default context, the same under RZK_SHIFT_BYTES=0) at (1,3,1), with one key loaded into both."""
    if N not in _ctxs:
        on, off = make_ctx(N, 1, 3, 1, env={"RZK_SHIFT_BYTES": 1}), make_ctx(N, 1, 3, 1, env={"RZK_SHIFT_BYTES": 0})
        A = synth.key(np.random.default_rng(7000 + N), N, 1, 3, 1)
        on.load_key(A)
        off.load_key(A)
        _ctxs[N] = (on, off)
    return _ctxs[N]


def every_way(N, call):
    """call(ctx) on both contexts, checked and trusted; asserts four identical results and returns one."""
    outs = []
    for ctx in ctx_pair(N):
        for trusted in (False, True):
            ctx.trust_device_outputs(trusted)
            try:
                out = call(ctx)
            finally:
                ctx.trust_device_outputs(False)
            outs.append(out if isinstance(out, tuple) else (out,))
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert np.array_equal(a, b)
    return outs[0]


def open_case(N, r, d, seed):
    """z = y + r (.) d for hand-made r [B, N] (used for all three columns, shifted) and d [B, N]."""
    on, _ = ctx_pair(N)
    P = P_of(on)
    B = d.shape[0]
    r3 = np.ascontiguousarray(np.stack([r, np.roll(r, 1, axis=-1), r[:, ::-1]], axis=1))
    y = synth.gauss(np.random.default_rng(seed), (B, 3, N), P.sigma)
    (z,) = every_way(N, lambda ctx: ctx.open_response(y, r3, d))
    for b in range(B):
        assert np.array_equal(z[b], O.open_response(P, y[b], r3[b], d[b])), b
    return y, z


@pytest.mark.parametrize("B", [5, 64])
@pytest.mark.parametrize("N", [512, 1024])
def test_open_linear_sum_responses(torch_mod, N, B):
    on, off = ctx_pair(N)
    P = P_of(on)
    rng = np.random.default_rng(7100 + N + B)
    k, V = 3, 2
    r, rp = synth.small(rng, (B, k, N)), synth.small(rng, (B, k, N))
    y, yp = synth.gauss(rng, (B, k, N), P.sigma), synth.gauss(rng, (B, k, N), P.sigma)
    d = synth.challenge(rng, (B,), N, P.kappa)
    (z,) = every_way(N, lambda ctx: ctx.open_response(y, r, d))
    lz, lzp = every_way(N, lambda ctx: ctx.linear_response(y, yp, r, rp, d))
    gs, xs, rs, rp2, ys, yp2, d2 = sum_inputs(rng, P, B, V)
    sz, szp = every_way(N, lambda ctx: ctx.sum_response(ys, yp2, rs, rp2, d2))
    for b in range(B):
        assert np.array_equal(z[b], O.open_response(P, y[b], r[b], d[b])), b
        zr, zpr = O.linear_response(P, y[b], yp[b], r[b], rp[b], d[b])
        assert np.array_equal(lz[b], zr) and np.array_equal(lzp[b], zpr), b
        zr, zpr = O.sum_response(P, ys[b], yp2[b], rs[b], rp2[b], d2[b])
        assert np.array_equal(sz[b], zr) and np.array_equal(szp[b], zpr), b


@pytest.mark.parametrize("N", [512, 1024])
def test_the_switch_selects_the_instantiation(torch_mod, N):
    on, off = ctx_pair(N)
    P = P_of(on)
    rng = np.random.default_rng(7200 + N)
    D = lambda a: dev(torch_mod, a)
    y, r, d = synth.gauss(rng, (2, 3, N), P.sigma), synth.small(rng, (2, 3, N)), synth.challenge(rng, (2,), N, P.kappa)
    logn = N.bit_length() - 1
    for ctx, trusted, want in ((on, False, f"shift_row_kernel<{logn}, false>"), (on, True, f"shift_row_kernel<{logn}, true>"),
                               (off, False, f"shift_row_kernel<{logn}, false, WaveTeam, false>"),
                               (off, True, f"shift_row_kernel<{logn}, true, WaveTeam, false>")):
        ctx.trust_device_outputs(trusted)
        ctx.prof_enable(True)
        ctx.prof_reset()
        try:
            ctx.open_response(D(y), D(r), D(d))
            names = ctx.prof_read_kernels()
        finally:
            ctx.prof_enable(False)
            ctx.trust_device_outputs(False)
        assert [nm for nm, _ in names] == [want]
        assert [nb for _, nb in names] == [10 * 8 * N * 2]   # reads d, y(3), r(3), stores z(3): the same accounting on both


@pytest.mark.parametrize("m", [1, 2, 3])
@pytest.mark.parametrize("N", [512, 1024])
def test_edge_of_the_condition(torch_mod, N, m):
    fit = 255 // (2 * m)
    rng = np.random.default_rng(7300 + N + m)
    pos = rng.permutation(N)[:fit + 1]
    rows = []
    for sign in (1, -1):
        for nnz in (fit, fit + 1):
            d = np.zeros(N, dtype=np.int64)
            d[pos[:nnz]] = sign
            rows.append((np.full(N, sign * m, dtype=np.int64), d))                   # every byte sum at 0 or at 2 |d|_1 m
            rows.append((np.full(N, -sign * m, dtype=np.int64), d))
            rv = rng.integers(-m, m + 1, N)
            rv[rng.integers(N)] = m
            d2 = d.copy()
            d2[pos[:nnz]] = rng.choice([-1, 1], nnz)
            rows.append((rv, d2))
    r = np.stack([a for a, _ in rows])
    d = np.stack([b for _, b in rows])
    y, z = open_case(N, r, d, 7350 + N + m)
    # the extreme itself, spelled out: v = m everywhere, `fit` entries +1 at positions p: z - y = m (#{p <= j} - #{p > j})
    want = np.array([m * (2 * np.sum(pos[:fit] <= j) - fit) for j in range(N)])
    assert abs(want).max() == m * fit and not np.any((z[0, 0] - y[0, 0] - want) % O.Q_DEFAULT)


@pytest.mark.parametrize("N", [512, 1024])
def test_rotation_extremes_zero_and_dense_multipliers(torch_mod, N):
    E = N // 64
    single = [0, 1, 2, 3, 4, 5, E - 1, E, E + 1, 4 * 64 - 1, 4 * 64, 4 * 64 + 1, N // 2 - 1, N // 2, N // 2 + 1, N - 2, N - 1]
    rng = np.random.default_rng(7400 + N)
    ds = []
    for p in single:
        for val in (1, -1):
            d = np.zeros(N, dtype=np.int64)
            d[p] = val
            ds.append(d)
    d = np.zeros(N, dtype=np.int64)
    d[[0, 1, 2, 3, N // 2, N - 1]] = [1, -1, 1, -1, 1, -1]
    ds.append(d)
    ds.append(np.zeros(N, dtype=np.int64))                       # zero multiplier: z = y
    ds.append(rng.choice([-3, 3], N))                            # dense +-3: the word path
    d = np.zeros(N, dtype=np.int64)
    d[[5, 300, 77]] = [2, -3, 1]                                 # short, but entries beyond +-1
    ds.append(d)
    d = np.stack(ds)
    r = rng.integers(-1, 2, (d.shape[0], N))
    r[-1] = rng.integers(-2, 3, N)
    y, z = open_case(N, r, d, 7450 + N)
    zero = len(single) * 2 + 1
    assert np.array_equal(z[zero], y[zero])


@pytest.mark.parametrize("N", [512, 1024])
def test_noncanonical_inputs_still_fail_the_call(torch_mod, N):
    from ring_zk_amd.backend import RzkError

    rng = np.random.default_rng(7500 + N)
    B = 5
    for ctx in ctx_pair(N):
        P = P_of(ctx)
        y, r, d = synth.gauss(rng, (B, 3, N), P.sigma), synth.small(rng, (B, 3, N)), synth.challenge(rng, (B,), N, P.kappa)
        good = ctx.open_response(y, r, d)
        for which, where, bad in (("r", (4, 2, N - 1), 1 << 32), ("r", (0, 0, 0), -(1 << 32) + 1), ("y", (1, 1, 7), 3 << 32),
                                  ("d", (2, 9), 1 << 32), ("r", (3, 1, 5), 1 << 31)):
            args = dict(y=y.copy(), r=r.copy(), d=d.copy())
            args[which][where] += bad
            with pytest.raises(RzkError):
                ctx.open_response(args["y"], args["r"], args["d"])
        assert np.array_equal(ctx.open_response(y, r, d), good)   # the failing calls cleared the sticky condition
