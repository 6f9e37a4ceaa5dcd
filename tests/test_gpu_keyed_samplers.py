"""Keyed device samplers (include/rzk.h "keyed device-side samplers"): ChaCha20 blocks under a 256-bit key.

The uniform and challenge kernels are compared bit for bit with tests/chacha_ref.py (a numpy restatement of the stream
and the maps) at the shapes where the quad layout can go wrong: a block wider than the polynomial (N = 4), one block
per polynomial pair of quads, several grid-stride trips, an output that is only 8-byte aligned.  The Gaussian kernel
goes through floating point, so it is checked like the seeded one (tests/test_gpu_samplers.py, same properties, sizes
and tolerances: the project's own, at 6 standard errors) and for determinism against itself.  Then the argument rules,
the provers of ring_zk_amd.fiat_shamir that draw their own randomness, and the kernel names.

Every test but the first needs the GPU; the first shows on the CPU that an ideal normal sample of the same size passes
the Gaussian tolerances, so a failure of the GPU test is the sampler's."""
import ctypes as C
from math import erf, sqrt

import numpy as np
import pytest

import chacha_ref
import fs_ref
from oracle import oracle as O
from test_gpu_baseline_shapes import P_of, make_ctx, torch_mod  # noqa: F401

gpu = pytest.mark.gpu
Q = O.Q_DEFAULT
HALF = (Q - 1) // 2
KEY = bytes((11 * i + 5) & 0xFF for i in range(32))
KEY2 = KEY[:31] + bytes([KEY[31] ^ 0x80])
NONCE = bytes((3 * i + 1) & 0xFF for i in range(16))


def keyed(N, kappa=None, env=None, key=KEY):
    ctx = make_ctx(N, 1, 3, 1, env=env, kappa=min(36, N) if kappa is None else kappa)
    ctx.set_sampler_key(key)
    return ctx


def host(t):
    return t.cpu().numpy()


# ---- Gaussian tolerances: the checks of test_gauss_matches_truncated_normal ---------------------------------------------
def check_gauss(y, sigma):
    """y: int64 samples of (i64) N(0, sigma), shape (256, 3, 1024)."""
    assert y.dtype == np.int64 and y.shape == (256, 3, 1024)
    f = y.astype(np.float64)
    n = f.size
    assert abs(f.mean()) < 6 * sigma / np.sqrt(n)
    assert abs(f.std() / sigma - 1) < 0.01
    assert abs(((f / sigma) ** 4).mean() - 3.0) < 0.1
    assert abs((np.abs(f) < sigma).mean() - 0.6827) < 0.005
    assert np.abs(f).max() < 8 * sigma


def check_truncation(small):
    """small: int64 samples at sigma = 3, shape (512, 1024): |trunc(x)| has P(0) = P(|x| < 1)."""
    assert small.shape == (512, 1024)
    p0 = (small == 0).mean()
    want = erf(1 / (3.0 * sqrt(2)))
    assert abs(p0 - want) < 6 * np.sqrt(want * (1 - want) / small.size)


@pytest.mark.parametrize("sigma", [21780.0, float(1 << 20)])
def test_an_ideal_normal_sample_passes_the_gauss_tolerances(sigma):
    rng = np.random.default_rng(int(sigma))
    check_gauss(np.trunc(rng.normal(0.0, sigma, (256, 3, 1024))).astype(np.int64), sigma)
    check_truncation(np.trunc(rng.normal(0.0, 3.0, (512, 1024))).astype(np.int64))


# ---- bit for bit against chacha_ref --------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("N,bound,count", [(4, 1, 37), (4, HALF, 37), (16, 12345, 9), (512, HALF, 5), (2048, 1, 3)])
def test_uniform_matches_reference_across_ring_degrees(torch_mod, N, bound, count):
    ctx = keyed(N)
    got = host(ctx.sample_uniform_keyed(NONCE, 7, bound, (count,)))
    assert got.shape == (count, N)
    assert np.array_equal(got, chacha_ref.uniform(KEY, NONCE, 7, N, bound, range(count)))


@gpu
@pytest.mark.parametrize("count", [1, 3, 67])
@pytest.mark.parametrize("bound", [1, HALF])
def test_uniform_matches_reference_at_1024(torch_mod, bound, count):
    ctx = keyed(1024)
    got = host(ctx.sample_uniform_keyed(NONCE, 0x80000001, bound, (count,)))
    assert np.array_equal(got, chacha_ref.uniform(KEY, NONCE, 0x80000001, 1024, bound, range(count)))
    assert got.min() >= -bound and got.max() <= bound


# kappa = N at N = 4; a full 64-step round (blocks 0 .. 7) at N = 64; two rounds of the lane loop at kappa = 100
@gpu
@pytest.mark.parametrize("N,kappa,count", [(4, 4, 9), (64, 64, 9), (128, 100, 9), (1024, 36, 70)])
def test_challenge_matches_reference(torch_mod, N, kappa, count):
    ctx = keyed(N, kappa)
    got = host(ctx.sample_challenge_keyed(NONCE, 3, (count,)))
    assert np.array_equal(got, chacha_ref.challenge(KEY, NONCE, 3, N, kappa, range(count)))
    assert (np.abs(got).sum(axis=1) == kappa).all() and np.abs(got).max() == 1   # challenge_space.rs:56-82


@gpu
def test_unaligned_output_takes_the_8_byte_path(torch_mod):
    """out = one int64 into a tensor: 8-byte aligned only.  Same values, and the words around the output stay untouched."""
    torch = torch_mod
    N, cnt, guard = 1024, 3, -0x0123456789ABCDEF
    ctx = keyed(N)
    L = ctx._L
    nonce = (C.c_uint8 * 16).from_buffer_copy(NONCE)
    want_u = chacha_ref.uniform(KEY, NONCE, 1, N, HALF, range(cnt))
    want_c = chacha_ref.challenge(KEY, NONCE, 2, N, ctx.kappa, range(cnt))
    want_g = host(ctx.sample_gauss_keyed(NONCE, 4, 1000.0, (cnt,)))
    want_g2 = host(ctx.sample_gauss_keyed(NONCE, 4, float(1 << 20), (cnt,)))
    calls = [
        (lambda p: L.rzk_sample_uniform_keyed_dev(ctx._h, nonce, 1, HALF, p, cnt), want_u),
        (lambda p: L.rzk_sample_challenge_keyed_dev(ctx._h, nonce, 2, p, cnt), want_c),
        (lambda p: L.rzk_sample_gauss_keyed_dev(ctx._h, nonce, 4, C.c_double(1000.0), p, cnt), want_g),
        (lambda p: L.rzk_sample_gauss_keyed_dev(ctx._h, nonce, 4, C.c_double(float(1 << 20)), p, cnt), want_g2),
    ]
    ctx._bind_torch_stream()
    for call, want in calls:
        buf = torch.full((cnt * N + 3,), guard, dtype=torch.int64, device="cuda")
        view = buf[1:1 + cnt * N]
        assert view.data_ptr() % 16 == 8
        assert call(C.c_void_p(view.data_ptr())) == 0
        got = host(buf)
        assert np.array_equal(got[1:1 + cnt * N].reshape(cnt, N), want)
        assert got[0] == guard and got[-2] == guard and got[-1] == guard


@gpu
def test_grid_stride_trips(torch_mod):
    """Grids sized for one CU: 16 blocks of 64 quads = 8192 coefficients per trip of the uniform and Gaussian kernels,
    16 blocks of 4 wavefronts = 64 polynomials per trip of the challenge kernel."""
    N, kappa = 1024, 36
    one = keyed(N, kappa, env={"RZK_GRID_CUS": 1})
    full = keyed(N, kappa)
    cnt = 27   # 27648 coefficients: 4 trips, the last one partial
    assert np.array_equal(host(one.sample_uniform_keyed(NONCE, 5, HALF, (cnt,))),
                          chacha_ref.uniform(KEY, NONCE, 5, N, HALF, range(cnt)))
    for sigma in (float(one.sigma), float(1 << 20)):
        assert np.array_equal(host(one.sample_gauss_keyed(NONCE, 6, sigma, (cnt,))),
                              host(full.sample_gauss_keyed(NONCE, 6, sigma, (cnt,))))
    cnt = 150   # 3 trips, the last one partial
    assert np.array_equal(host(one.sample_challenge_keyed(NONCE, 7, (cnt,))),
                          chacha_ref.challenge(KEY, NONCE, 7, N, kappa, range(cnt)))


@gpu
def test_separation_and_prefix(torch_mod):
    ctx = keyed(1024)
    first = bytes([NONCE[0] ^ 1]) + NONCE[1:]
    last = NONCE[:15] + bytes([NONCE[15] ^ 0x80])
    draws = {
        "uniform": lambda n, s, cnt: ctx.sample_uniform_keyed(n, s, HALF, (cnt,)),
        "gauss": lambda n, s, cnt: ctx.sample_gauss_keyed(n, s, 100.0, (cnt,)),
        "challenge": lambda n, s, cnt: ctx.sample_challenge_keyed(n, s, (cnt,)),
    }
    for name, draw in draws.items():
        a = host(draw(NONCE, 2, 64))
        assert np.array_equal(a, host(draw(NONCE, 2, 64))), name            # same triple -> same bytes
        others = [host(draw(first, 2, 64)), host(draw(last, 2, 64)), host(draw(NONCE, 3, 64))]
        ctx.set_sampler_key(KEY2)
        others.append(host(draw(NONCE, 2, 64)))
        ctx.set_sampler_key(KEY)
        seen = {a.tobytes()}
        for o in others:
            assert not np.array_equal(a, o), name
            assert not any(np.array_equal(a[i], o[i]) for i in range(64)), name   # every polynomial differs
            seen.add(o.tobytes())
        assert len(seen) == 5, name
        assert np.array_equal(host(draw(NONCE, 2, 16)), a[:16]), name        # polynomial i does not depend on count


# ---- Gaussian: the distribution ------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("form", ["f32", "f64"])
def test_gauss_matches_truncated_normal(torch_mod, form):
    ctx = keyed(1024)
    sigma = float(ctx.sigma) if form == "f32" else float(1 << 20)
    assert (sigma < 524288.0) == (form == "f32")
    y = host(ctx.sample_gauss_keyed(NONCE, 0, sigma, (256, 3)))
    check_gauss(y, sigma)
    check_truncation(host(ctx.sample_gauss_keyed(NONCE, 1, 3.0, (512,))))
    if form == "f32":   # honest responses built from sampled y pass the verifier's norm predicate (open.rs:167-169)
        assert all(O.check_norm(y[b], ctx.verify_bound) for b in range(16))


# ---- argument rules ---------------------------------------------------------------------------------------------------------
@gpu
def test_errors(torch_mod):
    from ring_zk_amd import _lib
    from ring_zk_amd.backend import RzkError

    ctx = make_ctx(1024, 1, 3, 1)
    for draw in (lambda: ctx.sample_uniform_keyed(NONCE, 0, 1, (4,)), lambda: ctx.sample_gauss_keyed(NONCE, 0, 100.0, (4,)),
                 lambda: ctx.sample_challenge_keyed(NONCE, 0, (4,))):
        with pytest.raises(RzkError) as e:   # no key set
            draw()
        assert e.value.status == _lib.RZK_E_ARG
    ctx.set_sampler_key(KEY)
    with pytest.raises(RzkError):
        ctx.sample_uniform_keyed(NONCE, 0, 0, (4,))
    with pytest.raises(RzkError):
        ctx.sample_uniform_keyed(NONCE, 0, HALF + 1, (4,))
    with pytest.raises(RzkError):
        ctx.sample_gauss_keyed(NONCE, 0, 0.0, (4,))
    out = torch_mod.empty(1024, dtype=torch_mod.int64, device="cuda")
    assert ctx._L.rzk_sample_uniform_keyed_dev(ctx._h, None, 0, 1, C.c_void_p(out.data_ptr()), 1) == _lib.RZK_E_ARG   # NULL nonce
    assert ctx._L.rzk_sample_uniform_keyed_dev(ctx._h, None, 0, 1, None, 0) == _lib.RZK_OK                          # count == 0
    with pytest.raises(ValueError):
        ctx.set_sampler_key(b"short")
    with pytest.raises(ValueError):
        ctx.sample_uniform_keyed(NONCE[:8], 0, 1, (4,))
    assert host(ctx.sample_uniform_keyed(NONCE, 0, 1, (4,))).shape == (4, 1024)
    ctx.set_sampler_key(None)
    with pytest.raises(RzkError):
        ctx.sample_uniform_keyed(NONCE, 0, 1, (4,))


# ---- the provers that draw their own randomness ------------------------------------------------------------------------------
@gpu
def test_keyed_sampler_counts_nonces(torch_mod):
    from ring_zk_amd.backend import KeyedSampler

    ctx = make_ctx(1024, 1, 3, 1)
    s = KeyedSampler(ctx, KEY, nonce0=(1 << 64) - 1)   # the counter carries into the upper half of the nonce
    n0, n1, n2 = [((1 << 64) - 1 + i).to_bytes(16, "little") for i in range(3)]
    assert np.array_equal(host(s.uniform(1, (2, 3))).reshape(6, 1024), chacha_ref.uniform(KEY, n0, 0, 1024, 1, range(6)))
    g = host(s.gauss(100.0, (2,)))
    assert np.array_equal(host(s.challenge((5,))), chacha_ref.challenge(KEY, n2, 0, 1024, ctx.kappa, range(5)))
    assert np.array_equal(g, host(ctx.sample_gauss_keyed(n1, 0, 100.0, (2,))))
    u1 = host(KeyedSampler(ctx).uniform(HALF, (1,)))        # key = None: os.urandom, a fresh key per sampler
    assert not np.array_equal(u1, host(KeyedSampler(ctx).uniform(HALF, (1,))))


@gpu
def test_open_prove_sampled_end_to_end(torch_mod):
    from ring_zk_amd import fiat_shamir as FS
    from ring_zk_amd import synth
    from ring_zk_amd.backend import KeyedSampler

    N, B = 1024, 64
    ctx = make_ctx(N, 1, 3, 1)
    A = synth.key(np.random.default_rng(31), N, 1, 3, 1)
    ctx.load_key(A)
    sampler = KeyedSampler(ctx, KEY, nonce0=5)
    x = torch_mod.from_numpy(synth.uniform(np.random.default_rng(32), (B, 1, N))).cuda()
    c, t, z, ok, r = FS.open_prove_sampled(ctx, x, sampler)
    acc = FS.open_verify(ctx, c, t, z)
    assert host(ok).tolist() == [1] * B and host(acc).tolist() == [1] * B
    assert np.array_equal(host(r).reshape(B * 3, N), chacha_ref.uniform(KEY, (5).to_bytes(16, "little"), 0, N, ctx.b, range(3 * B)))
    c2, t2, z2, ok2, r2 = FS.open_prove_sampled(ctx, x, sampler)
    assert not np.array_equal(host(r2), host(r)) and not np.array_equal(host(z2), host(z))
    assert sampler.counter == 9
    P = P_of(ctx)
    c, t, z = host(c), host(t), host(z)
    kd = fs_ref.key_digest(A, ctx.q, N, 1, 3, 1, ctx.kappa, ctx.b)
    for b in (0, B - 1):
        d, _ = fs_ref.challenge_one(fs_ref.OPEN_COMMITMENT, 0, kd, bytes(32), [c[b], t[b]], N, ctx.kappa)
        assert O.open_verify(P, A, z[b], t[b], c[b], d) == 1


@gpu
def test_linear_and_sum_prove_sampled(torch_mod):
    from ring_zk_amd import fiat_shamir as FS
    from ring_zk_amd import synth
    from ring_zk_amd.backend import KeyedSampler

    N, B, V = 512, 8, 2
    ctx = make_ctx(N, 1, 3, 1)
    ctx.load_key(synth.key(np.random.default_rng(33), N, 1, 3, 1))
    sampler = KeyedSampler(ctx, KEY)
    rng = np.random.default_rng(34)
    D = lambda a: torch_mod.from_numpy(a).cuda()
    aux = bytes(range(32))
    g, x = D(synth.uniform(rng, (B, N))), D(synth.uniform(rng, (B, 1, N)))
    c, cp, t, tp, u, z, zp, ok, r, rp = FS.linear_prove_sampled(ctx, g, x, sampler, aux=aux)
    assert r.shape == (B, 3, N) and not np.array_equal(host(r), host(rp))
    assert host(ok).tolist() == [1] * B
    assert host(FS.linear_verify(ctx, c, cp, g, t, tp, u, z, zp, aux=aux)).tolist() == [1] * B
    gs, xs = D(synth.uniform(rng, (B, V, N))), D(synth.uniform(rng, (B, V, 1, N)))
    cs, cp, ts, tp, u, zs, zp, ok, rs, rp = FS.sum_prove_sampled(ctx, gs, xs, sampler, aux=aux)
    assert rs.shape == (B, V, 3, N) and rp.shape == (B, 3, N)
    assert host(ok).tolist() == [1] * B
    assert host(FS.sum_verify(ctx, cs, cp, gs, ts, tp, u, zs, zp, aux=aux)).tolist() == [1] * B
    assert sampler.counter == 8


@gpu
def test_profiler_names_the_kernels(torch_mod):
    ctx = keyed(1024)
    ctx.prof_enable(True)
    ctx.prof_reset()
    ctx.sample_uniform_keyed(NONCE, 0, 1, (4,))
    ctx.sample_gauss_keyed(NONCE, 1, 100.0, (4,))
    ctx.sample_gauss_keyed(NONCE, 2, float(1 << 20), (4,))
    ctx.sample_challenge_keyed(NONCE, 3, (4,))
    names = ctx.prof_read_kernels()
    ctx.prof_enable(False)
    assert names == [("sample_uniform_chacha_kernel", 4 * 8192), ("sample_gauss_chacha_kernel<true>", 4 * 8192),
                     ("sample_gauss_chacha_kernel<false>", 4 * 8192), ("sample_challenge_chacha_kernel", 4 * 8192)]
