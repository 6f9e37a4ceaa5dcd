"""The Gaussian samplers, coefficient by coefficient, against an extended-precision statement of what they draw.

Four kernels draw y: sample_gauss_kernel<true / false> (Philox words, rzk_sample.h) and sample_gauss_chacha_kernel<true /
false> (ChaCha20 words, rzk_csprng_dev.hip), all through the one word-to-pair map of rzk_gauss.h.  The moment checks of
tests/test_gpu_samplers.py and tests/test_gpu_keyed_samplers.py cannot see a wrong word, a swapped pair, a repeated
block or a sigma off by half a percent.  Here every coefficient is held to

    |got - ref| < 1 + delta      always
    got == trunc(ref)            wherever delta decides the truncation

(tests/gauss_ref.py: the map in np.longdouble, delta32 / delta64 and their derivation), with the words from
tests/philox_ref.py and tests/chacha_ref.py.  Bit equality is not asked of a floating-point path; before it looks at the
device's output, every case asserts from the reference alone that the bound decides at least 90 % of its coefficients
in the F32 form (sigma up to the parameter sets' own; at 2^19 - 1, the last F32 sigma, almost nothing is decidable and
only the first line binds) and 99.9 % in the F64 form.

  * chosen words through Context.debug_gauss_map: the ends of both uniforms and of the angle and the region where log2 u0
    cancels (__log2f at m = 2 - 2^-23, sincospif(2.0f)), which no seed or key produces in a test-sized draw, and 10^5
    random quadruples;
  * the streams of both families at N = 4 (a ChaCha block is wider than the polynomial, a Philox polynomial is two
    threads), 16, 512, 2048; several grid-stride trips on one CU; the 8-byte store path;
  * the form at the dispatch edge 2^19 - 1 | 2^19, by the profiler's kernel names;
  * the first two draws of SeededSampler and KeyedSampler (stream and nonce counters).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import chacha_ref
import gauss_ref
import philox_ref
from test_gpu_baseline_shapes import make_ctx, torch_mod  # noqa: F401
from test_gpu_keyed_samplers import KEY, NONCE

pytestmark = pytest.mark.gpu

SEED, STREAM = 77, 3
LAST_F32 = float((1 << 19) - 1)
FIRST_F64 = float(1 << 19)
WIDEST = float(1 << 26)


def form_of(sigma):
    return sigma < gauss_ref.F32_SIGMA_LIMIT


def least_share(f32, sigma):
    """Share of coefficients the bound must decide (module docstring); None: no share is asked."""
    if not f32:
        return 0.999
    return 0.9 if sigma < LAST_F32 else None


@functools.lru_cache(maxsize=None)
def stream_words(family, N, count):
    if family == "philox":
        return philox_ref.gauss_words(SEED, STREAM, N, range(count))
    return chacha_ref.gauss_words(KEY, NONCE, STREAM, N, range(count))


@functools.lru_cache(maxsize=None)
def reference(family, N, count, sigma):
    """(v [count, N], delta [count, N]) of a stream case, computed once and shared; read-only."""
    v, d = gauss_ref.real(form_of(sigma), stream_words(family, N, count), sigma)
    v, d = v.reshape(count, N), np.broadcast_to(d, d.shape[:-1] + (2,)).reshape(count, N)
    v.setflags(write=False)
    return v, d


_ctxs = {}


def ctx_of(N, one_cu=False):
    """One keyed context per (N, grid) for the module."""
    if (N, one_cu) not in _ctxs:
        ctx = make_ctx(N, 1, 3, 1, env={"RZK_GRID_CUS": 1} if one_cu else None, kappa=min(36, N))
        ctx.set_sampler_key(KEY)
        _ctxs[(N, one_cu)] = ctx
    return _ctxs[(N, one_cu)]


def draw(family, ctx, sigma, count):
    if family == "philox":
        return ctx.sample_gauss(SEED, STREAM, sigma, (count,)).cpu().numpy()
    return ctx.sample_gauss_keyed(NONCE, STREAM, sigma, (count,)).cpu().numpy()


def sigma_of(ctx, which):
    return float(ctx.sigma) if which == "ctx" else float(which)


def hold(what, f32, sigma, v, d, get):
    """The share from the reference alone, then the device's output (get()) under gauss_ref.check."""
    least = least_share(f32, sigma)
    share = gauss_ref.decidable_share(v, d)
    if least is not None:
        assert share >= least, (what, share)
    st = gauss_ref.check(get(), v, d, what)
    print("PIN %s %s sigma %g: n %d, decidable %.5f, differ from trunc(ref) %d (share %.2e), worst (|got - ref| - 1) / delta %.4f"
          % (what, "f32" if f32 else "f64", sigma, st.n, share, st.differ, st.differ / st.n, st.worst))
    return st


# ---- chosen words ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [3.0, 21780.0, LAST_F32, FIRST_F64, WIDEST])
def test_map_on_edge_and_random_words(torch_mod, sigma):
    f32 = form_of(sigma)
    ctx = ctx_of(512)
    edge = gauss_ref.edge_words_f32() if f32 else gauss_ref.edge_words_f64()
    rnd = gauss_ref.random_words(4242, 100000)
    v, d = gauss_ref.real(f32, rnd, sigma)
    hold("random words", f32, sigma, v, d, lambda: ctx.debug_gauss_map(f32, rnd, sigma))
    v, d = gauss_ref.real(f32, edge, sigma)
    got = ctx.debug_gauss_map(f32, edge, sigma)
    st = gauss_ref.check(got, v, d, "edge words")     # no share asked: these words sit where the bound is widest
    print("PIN edge words %s sigma %g: n %d, undecidable %d, differ %d, worst %.4f" % ("f32" if f32 else "f64", sigma, st.n, st.undecidable, st.differ, st.worst))
    if not f32:
        zero = (edge[:, 0] == 0xFFFFFFFF) & (edge[:, 1] >= 0xFFFFF800)      # X >> 11 = 2^53 - 1: u0 = 1, radius 0
        assert zero.sum() == 32 and not got[zero].any()


def test_map_entry_point_arguments(torch_mod):
    from ring_zk_amd import _lib
    from ring_zk_amd.backend import RzkError

    ctx = ctx_of(512)
    w = gauss_ref.random_words(1, 5)
    assert ctx.debug_gauss_map(True, w[:0], 3.0).shape == (0, 2)         # pairs == 0
    assert ctx.debug_gauss_map(True, w, 3.0).shape == (5, 2)
    for f32, sigma in ((True, FIRST_F64), (True, 0.0), (False, 0.0), (False, 2 * WIDEST)):
        with pytest.raises(RzkError) as e:
            ctx.debug_gauss_map(f32, w, sigma)
        assert e.value.status == _lib.RZK_E_ARG
    # one thread per pair, 256 per block: a count that is no multiple of the block, and the same pairs whatever the count
    a = ctx.debug_gauss_map(True, gauss_ref.random_words(2, 1000), 100.0)
    assert np.array_equal(ctx.debug_gauss_map(True, gauss_ref.random_words(2, 1000)[:257], 100.0), a[:257])


# ---- the streams -----------------------------------------------------------------------------------------------------------------
SHAPES = [(4, 37), (16, 9), (512, 5), (2048, 3)]
STREAM_CASES = [(N, count, s) for N, count in SHAPES for s in ("ctx", 3.0, FIRST_F64, WIDEST)] + [(512, 3, LAST_F32)]


@pytest.mark.parametrize("family", ["philox", "chacha"])
@pytest.mark.parametrize("N,count,which", STREAM_CASES)
def test_stream_matches_reference(torch_mod, family, N, count, which):
    ctx = ctx_of(N)
    sigma = sigma_of(ctx, which)
    v, d = reference(family, N, count, sigma)
    hold("%s N %d x %d" % (family, N, count), form_of(sigma), sigma, v, d, lambda: draw(family, ctx, sigma, count))


@pytest.mark.parametrize("family", ["philox", "chacha"])
@pytest.mark.parametrize("which", ["ctx", 3.0, FIRST_F64, WIDEST])
def test_stream_on_one_cu_makes_several_trips(torch_mod, family, which):
    """Grids sized for one CU hold 16 blocks: 8192 coefficients per trip of either family; 67 polynomials of 512 make 5."""
    N, count = 512, 67
    ctx = ctx_of(N, one_cu=True)
    sigma = sigma_of(ctx, which)
    v, d = reference(family, N, count, sigma)
    hold("%s one CU" % family, form_of(sigma), sigma, v, d, lambda: draw(family, ctx, sigma, count))


@pytest.mark.parametrize("family", ["philox", "chacha"])
@pytest.mark.parametrize("which", ["ctx", 3.0, FIRST_F64, WIDEST])
def test_stream_into_an_8_byte_aligned_buffer(torch_mod, family, which):
    """out = one int64 into a tensor: the 8-byte store path.  Same reference, and the words around the output stay."""
    torch = torch_mod
    N, count, guard = 512, 5, -0x0123456789ABCDEF
    ctx = ctx_of(N)
    sigma = sigma_of(ctx, which)
    v, d = reference(family, N, count, sigma)
    buf = torch.full((count * N + 3,), guard, dtype=torch.int64, device="cuda")
    view = buf[1:1 + count * N]
    assert view.data_ptr() % 16 == 8
    ctx._bind_torch_stream()

    def get():
        p = C.c_void_p(view.data_ptr())
        if family == "philox":
            rc = ctx._L.rzk_sample_gauss_dev(ctx._h, SEED, STREAM, C.c_double(sigma), p, count)
        else:
            rc = ctx._L.rzk_sample_gauss_keyed_dev(ctx._h, (C.c_uint8 * 16).from_buffer_copy(NONCE), STREAM, C.c_double(sigma), p, count)
        assert rc == 0
        return buf.cpu().numpy()[1:1 + count * N].reshape(count, N)

    hold("%s 8-byte aligned" % family, form_of(sigma), sigma, v, d, get)
    got = buf.cpu().numpy()
    assert got[0] == guard and got[-2] == guard and got[-1] == guard
    assert np.array_equal(got[1:1 + count * N].reshape(count, N), draw(family, ctx, sigma, count))   # as the 16-byte path


# ---- dispatch and the samplers' counters ---------------------------------------------------------------------------------------
def test_form_at_the_dispatch_edge(torch_mod):
    ctx = ctx_of(512)
    ctx.prof_enable(True)
    ctx.prof_reset()
    for sigma in (LAST_F32, FIRST_F64):
        ctx.sample_gauss(SEED, STREAM, sigma, (3,))
        ctx.sample_gauss_keyed(NONCE, STREAM, sigma, (3,))
    names = ctx.prof_read_kernels()
    ctx.prof_enable(False)
    nbytes = 3 * 512 * 8
    assert names == [("sample_gauss_kernel<true>", nbytes), ("sample_gauss_chacha_kernel<true>", nbytes),
                     ("sample_gauss_kernel<false>", nbytes), ("sample_gauss_chacha_kernel<false>", nbytes)]


def test_samplers_first_two_draws(torch_mod):
    """SeededSampler counts streams under its seed, KeyedSampler nonces under its key (stream 0): draw i of either is the
    reference's polynomials at that stream / nonce."""
    from ring_zk_amd.backend import KeyedSampler, SeededSampler

    N, count = 512, 3
    ctx = make_ctx(N, 1, 3, 1)
    sigma = float(ctx.sigma)
    s = SeededSampler(ctx, SEED, stream0=STREAM)
    for i in range(2):
        v, d = gauss_ref.real(True, philox_ref.gauss_words(SEED, STREAM + i, N, range(count)), sigma)
        got = s.gauss(sigma, (count,)).cpu().numpy()
        hold("SeededSampler draw %d" % i, True, sigma, v.reshape(count, N), np.repeat(d, 2, axis=-1).reshape(count, N), lambda: got)
    nonce0 = (1 << 64) - 1                                   # the counter carries into the upper half of the nonce
    k = KeyedSampler(ctx, KEY, nonce0=nonce0)
    for i in range(2):
        nonce = (nonce0 + i).to_bytes(16, "little")
        v, d = gauss_ref.real(True, chacha_ref.gauss_words(KEY, nonce, 0, N, range(count)), sigma)
        got = k.gauss(sigma, (count,)).cpu().numpy()
        hold("KeyedSampler draw %d" % i, True, sigma, v.reshape(count, N), np.repeat(d, 2, axis=-1).reshape(count, N), lambda: got)
