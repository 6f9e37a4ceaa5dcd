"""The exact discrete Gaussian sampler on the GPU (rzk_sample_dgauss_keyed_dev, rzk_debug_dgauss_trial_dev,
Context.sample_dgauss_keyed, backend.ExactKeyedSampler) against tests/dgauss_ref.py (Python integers), bit
for bit: the sampler is integer-only, so every comparison with the restatement is an equality.  Shapes are those at which
the tiled queue kernel can go wrong: fewer pairs than one round of quads (N = 4, 1 polynomial), a tile that is cut by
the end of the call, tiles that span polynomials (N <= 128), several tiles per polynomial (N >= 512), several grid-stride
trips, an output that is only 8-byte aligned.  The distribution itself is shown on the CPU (tests/test_dgauss_host.py);
here P(0) at sigma = 3 puts the defect of the truncated sampler and its absence on record."""
import ctypes as C
from math import sqrt

import mpmath
import numpy as np
import pytest

import dgauss_ref as D
from test_dgauss_host import build_driver, host_trials
from test_gpu_baseline_shapes import make_ctx, torch_mod  # noqa: F401
from test_gpu_fiat_shamir import keyed_ctx

pytestmark = pytest.mark.gpu

KEY = bytes((11 * i + 5) & 0xFF for i in range(32))
KEY2 = KEY[:31] + bytes([KEY[31] ^ 0x80])
NONCE = bytes((3 * i + 1) & 0xFF for i in range(16))
SIGMAS = (3, 21780, 1 << 26)


def keyed(N, env=None, key=KEY):
    ctx = make_ctx(N, 1, 3, 1, env=env, kappa=min(36, N))
    ctx.set_sampler_key(key)
    return ctx


def host(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory, sanitize=False)   # the sanitized build belongs to the CPU tier


# ---- bit for bit against the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("N", [4, 8, 64, 1024, 2048])
def test_device_matches_reference(torch_mod, N, sigma):
    """Every N x (1, 3, 5 polynomials) x sigma.  The restatement is computed once per (N, sigma), for 5 polynomials: its
    polynomial i does not depend on how many are asked for (dgauss_ref.sample takes a list of indices), so a call of
    `count` polynomials must equal its first `count` rows."""
    ctx = keyed(N)
    want = D.sample(KEY, NONCE, 7, N, sigma, range(5))
    for count in (1, 3, 5):
        got = host(ctx.sample_dgauss_keyed(NONCE, 7, sigma, (count,)))
        assert got.shape == (count, N)
        assert np.array_equal(got, want[:count]), (N, count, sigma)


@pytest.mark.parametrize("count", [1, 3, 5])
@pytest.mark.parametrize("sigma", SIGMAS)
def test_device_matches_reference_at_every_sigma(torch_mod, count, sigma):
    """N = 64: 32 pairs per polynomial, so 1, 3 and 5 polynomials are 32, 96 and 160 pairs: less than a tile, a cut tile,
    and two tiles of which the first spans 4 polynomials."""
    ctx = keyed(64)
    got = host(ctx.sample_dgauss_keyed(NONCE, 0x80000001, sigma, (count,)))
    assert np.array_equal(got, D.sample(KEY, NONCE, 0x80000001, 64, sigma, range(count)))
    assert np.abs(got).max() < 8 * D.params(sigma)[1]


def test_unaligned_output_takes_the_8_byte_path(torch_mod):
    torch = torch_mod
    N, cnt, guard = 64, 5, -0x0123456789ABCDEF
    ctx = keyed(N)
    want = D.sample(KEY, NONCE, 4, N, 21780, range(cnt))
    nonce = (C.c_uint8 * 16).from_buffer_copy(NONCE)
    ctx._bind_torch_stream()
    buf = torch.full((cnt * N + 3,), guard, dtype=torch.int64, device="cuda")
    view = buf[1:1 + cnt * N]
    assert view.data_ptr() % 16 == 8
    assert ctx._L.rzk_sample_dgauss_keyed_dev(ctx._h, nonce, 4, 21780, C.c_void_p(view.data_ptr()), cnt * N) == 0
    got = host(buf)
    assert np.array_equal(got[1:1 + cnt * N].reshape(cnt, N), want)
    assert got[0] == guard and got[-2] == guard and got[-1] == guard


def test_grid_stride_trips_and_prefix(torch_mod):
    """A grid sized for one CU: 8 blocks of 4 wavefronts = 32 tiles = 4096 pairs per trip; 300 polynomials at N = 64 are
    9600 pairs = 75 tiles: three trips, the last one partial, every tile spanning 4 polynomials.  The output does not
    depend on the grid or on count: polynomial i of a longer call is polynomial i of a shorter one."""
    N, cnt = 64, 300
    one = keyed(N, env={"RZK_GRID_CUS": 1})
    full = keyed(N)
    want = D.sample(KEY, NONCE, 6, N, 21780, range(cnt))
    assert np.array_equal(host(one.sample_dgauss_keyed(NONCE, 6, 21780, (cnt,))), want)
    assert np.array_equal(host(full.sample_dgauss_keyed(NONCE, 6, 21780, (cnt,))), want)
    for m in (1, 3, 7):
        assert np.array_equal(host(full.sample_dgauss_keyed(NONCE, 6, 21780, (m,))), want[:m])
        assert np.array_equal(host(one.sample_dgauss_keyed(NONCE, 6, 21780, (m,))), want[:m])


def test_stream_separation(torch_mod):
    ctx = keyed(1024)
    sigma, cnt = 21780, 8
    a = host(ctx.sample_dgauss_keyed(NONCE, 2, sigma, (cnt,)))
    assert np.array_equal(a, host(ctx.sample_dgauss_keyed(NONCE, 2, sigma, (cnt,))))        # same triple -> same bytes
    # every block the restatement reads has bit 31 of word 12 set (the other samplers' blocks have it clear: their
    # word 12 is the block index within a polynomial, below 2^13), and the restatement is what the device computed
    used = set()
    assert np.array_equal(a[:2], D.sample(KEY, NONCE, 2, 1024, sigma, range(2), used=used))
    assert used and all(w >> 31 == 1 for w in used)
    box = host(ctx.sample_gauss_keyed(NONCE, 2, float(sigma), (cnt,)))
    assert not any(np.array_equal(a[i], box[i]) for i in range(cnt))
    assert (a == box).mean() < 0.01
    first = bytes([NONCE[0] ^ 1]) + NONCE[1:]
    last = NONCE[:15] + bytes([NONCE[15] ^ 0x80])
    others = [host(ctx.sample_dgauss_keyed(first, 2, sigma, (cnt,))), host(ctx.sample_dgauss_keyed(last, 2, sigma, (cnt,))),
              host(ctx.sample_dgauss_keyed(NONCE, 3, sigma, (cnt,)))]
    ctx.set_sampler_key(KEY2)
    others.append(host(ctx.sample_dgauss_keyed(NONCE, 2, sigma, (cnt,))))
    ctx.set_sampler_key(KEY)
    for o in others:
        assert not any(np.array_equal(a[i], o[i]) for i in range(cnt))
    assert len({a.tobytes()} | {o.tobytes() for o in others}) == 5


# ---- the debug entry ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [1, 3, 21780, 1 << 26])
def test_debug_trial_matches_the_host_driver(torch_mod, driver, tmp_path, sigma):
    """The host test's edge words and 4000 random tuples: the device's trial equals the restatement's and the host
    driver's (a plain build here; tests/test_dgauss_host.py runs the same words through the sanitized one)."""
    ctx = keyed(64)
    edge = np.array([w for _, w in D.edge_words(sigma)], dtype=np.uint32)
    rnd = np.random.default_rng(sigma + 1).integers(0, 1 << 32, (4000, 8), dtype=np.uint64).astype(np.uint32)
    words = np.concatenate([edge, rnd])
    C_, k = D.params(sigma)
    want = np.array([[int(ok), v] for ok, v in (D.trial(C_, k, [int(x) for x in w]) for w in words)], dtype=np.int64)
    got = ctx.debug_dgauss_trial(words, sigma)
    assert np.array_equal(got, want)
    assert np.array_equal(got, host_trials(driver, tmp_path, sigma, words))


# ---- argument rules ------------------------------------------------------------------------------------------------------------
def test_errors(torch_mod):
    from ring_zk_amd import _lib
    from ring_zk_amd.backend import RzkError

    N = 64
    ctx = make_ctx(N, 1, 3, 1, kappa=36)
    L, h = ctx._L, ctx._h
    ctx._bind_torch_stream()
    out = torch_mod.zeros(2 * N, dtype=torch_mod.int64, device="cuda")
    p = C.c_void_p(out.data_ptr())
    nonce = (C.c_uint8 * 16).from_buffer_copy(NONCE)
    with pytest.raises(RzkError) as e:   # no key set
        ctx.sample_dgauss_keyed(NONCE, 0, 3, (2,))
    assert e.value.status == _lib.RZK_E_ARG
    ctx.set_sampler_key(KEY)
    assert L.rzk_sample_dgauss_keyed_dev(h, nonce, 0, 0, p, 2 * N) == _lib.RZK_E_ARG                 # sigma = 0
    assert L.rzk_sample_dgauss_keyed_dev(h, nonce, 0, (1 << 26) + 1, p, 2 * N) == _lib.RZK_E_ARG     # sigma > 2^26
    assert L.rzk_sample_dgauss_keyed_dev(h, None, 0, 3, p, 2 * N) == _lib.RZK_E_ARG                  # NULL nonce
    assert L.rzk_sample_dgauss_keyed_dev(h, nonce, 0, 3, p, 2 * N - 1) == _lib.RZK_E_ARG             # count not a multiple of N
    assert L.rzk_sample_dgauss_keyed_dev(h, nonce, 0, 3, None, 2 * N) == _lib.RZK_E_ARG
    assert not host(out).any()
    assert L.rzk_sample_dgauss_keyed_dev(h, None, 0, 0, None, 0) == _lib.RZK_OK                      # count == 0
    assert L.rzk_sample_dgauss_keyed_dev(h, nonce, 0, 1 << 26, p, 2 * N) == _lib.RZK_OK
    assert host(out).any()
    assert L.rzk_debug_dgauss_trial_dev(h, 0, p, p, 1) == _lib.RZK_E_ARG
    assert L.rzk_debug_dgauss_trial_dev(h, (1 << 26) + 1, p, p, 1) == _lib.RZK_E_ARG
    assert L.rzk_debug_dgauss_trial_dev(h, 3, None, None, 0) == _lib.RZK_OK
    with pytest.raises(ValueError):
        ctx.sample_dgauss_keyed(NONCE, 0, 2.5, (2,))
    with pytest.raises(ValueError):
        ctx.debug_dgauss_trial(np.zeros((3, 4), dtype=np.uint32), 3)
    ctx.set_sampler_key(None)
    with pytest.raises(RzkError):
        ctx.sample_dgauss_keyed(NONCE, 0, 3, (2,))


def test_profiler_names_the_kernel(torch_mod):
    ctx = keyed(1024)
    ctx.prof_enable(True)
    ctx.prof_reset()
    ctx.sample_dgauss_keyed(NONCE, 0, 21780, (4,))
    names = ctx.prof_read_kernels()
    ctx.prof_enable(False)
    assert names == [("sample_dgauss_chacha_kernel", 4 * 8192)]


# ---- P(0) at sigma = 3: the defect of the truncated sampler, and its absence --------------------------------------------------------
def test_p0_at_sigma_3(torch_mod):
    mpmath.mp.prec = 100
    p0 = float(1 / (1 + 2 * mpmath.nsum(lambda z: mpmath.exp(-mpmath.mpf(z * z) / 18), [1, mpmath.inf])))
    assert abs(p0 - 0.13298) < 1e-5
    n = 1 << 17
    width = 6 * sqrt(p0 * (1 - p0) / n)
    ctx = keyed(1024)
    exact = (host(ctx.sample_dgauss_keyed(NONCE, 1, 3, (n // 1024,))) == 0).mean()
    trunc = (host(ctx.sample_gauss_keyed(NONCE, 1, 3.0, (n // 1024,))) == 0).mean()
    print("P(0) at sigma = 3 over %d coefficients: exact sampler %.5f, truncated Box-Muller %.5f, D_3(0) = %.5f +- %.5f"
          % (n, exact, trunc, p0, width))
    assert abs(exact - p0) < width
    assert abs(trunc - p0) > width          # about 0.261: the interval (-1, 1) goes to 0


# ---- end to end: the zero-knowledge provers over the exact sampler --------------------------------------------------------------------
class Recording:
    """An ExactKeyedSampler that keeps what gauss returned, in order."""

    def __new__(cls, ctx, key, nonce0):
        from ring_zk_amd.backend import ExactKeyedSampler

        class _Rec(ExactKeyedSampler):
            def __init__(self, *a, **kw):
                super().__init__(*a, **kw)
                self.draws = []

            def gauss(self, sigma, lead):
                nonce = self.counter
                y = super().gauss(sigma, lead)
                self.draws.append((nonce, tuple(lead), y.clone()))
                return y

        return _Rec(ctx, key, nonce0)


AUX = bytes(range(50, 82))


def check_draw(ctx, draw, N):
    nonce, lead, y = draw
    want = D.sample(KEY, nonce.to_bytes(16, "little"), 0, N, ctx.sigma, range(int(np.prod(lead))))
    assert np.array_equal(host(y).reshape(-1, N), want)


def test_zero_knowledge_provers_over_the_exact_sampler(torch_mod):
    from ring_zk_amd import fiat_shamir as FS
    from ring_zk_amd.backend import ExactKeyedSampler, KeyedSampler

    N, B, V = 64, 8, 2
    ctx, _ = keyed_ctx(N, 1, 3, 1, 36, seed=41)
    assert issubclass(ExactKeyedSampler, KeyedSampler) and int(ctx.sigma) == ctx.sigma
    x = ctx.sample_uniform(9, 0, ctx.half, (B, 1))
    s = Recording(ctx, KEY, 100)
    c, t, z, ok, r, rounds = FS.open_prove_zk(ctx, x, s, aux=AUX)
    okh = host(ok).astype(bool)
    assert okh.all() and host(FS.open_verify(ctx, c, t, z, aux=AUX)).astype(bool)[okh].all()
    assert s.draws[0][:2] == (101, (B, 3))                  # nonce 100 is r's
    check_draw(ctx, s.draws[0], N)
    # the same round 0 from the one-shot prover: z = y + d r with the restatement's y
    c1, t1, z1, ok1, r1 = FS.open_prove_sampled(ctx, x, ExactKeyedSampler(ctx, KEY, 100), aux=AUX)
    first = host(rounds) == 0
    assert np.array_equal(host(z1)[first], host(z)[first]) and torch_mod.equal(r1, r)

    g = ctx.sample_uniform(9, 1, ctx.half, (B,))
    s = Recording(ctx, KEY, 200)
    c, cp, t, tp, u, z, zp, ok, r, rp, rounds = FS.linear_prove_zk(ctx, g, x, s, aux=AUX)
    okh = host(ok).astype(bool)
    assert okh.all() and host(FS.linear_verify(ctx, c, cp, g, t, tp, u, z, zp, aux=AUX)).astype(bool)[okh].all()
    assert [d[:2] for d in s.draws[:2]] == [(202, (B, 3)), (203, (B, 3))]
    check_draw(ctx, s.draws[0], N)
    check_draw(ctx, s.draws[1], N)

    gs, xs = ctx.sample_uniform(9, 2, ctx.half, (B, V)), ctx.sample_uniform(9, 3, ctx.half, (B, V, 1))
    s = Recording(ctx, KEY, 300)
    cs, cp, ts, tp, u, zs, zp, ok, rs, rp, rounds = FS.sum_prove_zk(ctx, gs, xs, s, aux=AUX)
    okh = host(ok).astype(bool)
    assert okh.any() and host(FS.sum_verify(ctx, cs, cp, gs, ts, tp, u, zs, zp, aux=AUX)).astype(bool)[okh].all()
    assert [d[:2] for d in s.draws[:2]] == [(302, (B, V, 3)), (303, (B, 3))]
    check_draw(ctx, s.draws[0], N)
    check_draw(ctx, s.draws[1], N)
