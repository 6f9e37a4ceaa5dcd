"""Extended-precision statement of the Gaussian samplers' word-to-pair map (ring_zk_amd/csrc/rzk_gauss.h)
and the bound within which an implementation must agree with it.  Test infrastructure: shares no code with the library.

Both generators feed the same map with four 32-bit words (w0, w1, w2, w3) per coefficient pair — the four words of a
Philox block (tests/philox_ref.py) or quarter i = w[4i .. 4i+3] of a ChaCha20 block (tests/chacha_ref.py):

    F32 form (sigma < 2^19)   X = w0:w1 (0 is taken as 1), lz = clz(X), top = the 24 leading bits of X << lz,
                              u0 = top 2^-(24+lz): only those 24 bits count;
                              a = float32(w2) 2^-31 half turns: the rounding of w2 to 24 bits (nearest even) is part of
                              the definition, w2 = 2^32 - 1 gives a full turn;
                              R = float32(sigma) sqrt(-2 ln u0)
    F64 form                  u0 = ((w0:w1 >> 11) + 1) 2^-53, u1 = (w2:w3 >> 11) 2^-53, a = 2 u1 half turns,
                              R = sigma sqrt(-2 ln u0)
    both                      (v0, v1) = (R cos pi a, R sin pi a), and the coefficients are trunc(v0), trunc(v1)

real_f32 / real_f64 return the REAL values v before the truncation, in np.longdouble (64 mantissa bits on x86), formed
so that nothing cancels: ln u0 = log1p(u0' - 1) - lz ln 2 with u0' in [1/2, 1] and u0' - 1 exact, and the angle reduced
exactly to a quadrant plus |r| <= 1/4 half turns before pi enters.  Their own error is a few 2^-63 relative.

The bound (delta32, delta64) is what an implementation in the form's own precision may be off by before it truncates.

delta32 = 2^-24 (1.4 sigma^2 / max(R, 2^-24 sigma) + 16 R), term by term:
  * the logarithm.  log2 u0 is formed as log2f(m) - (lz + 1), m = top 2^-23 in [1, 2).  An absolute error of one ulp of
    log2f on [0.5, 1), 2^-24, in log2 u0 is 0.69 2^-24 in ln u0; R^2 = -2 sigma^2 ln u0, so dR = sigma^2 / R * 0.69 2^-24.
    Where u0 is close to 1 (lz = 0, m close to 2) the difference cancels and this term is all there is: R is far below
    sigma and the error of a sample reaches 0.47 at sigma = 21780 (measured on a float32 restatement of the map).  R >=
    sigma sqrt(-2 ln(1 - 2^-24)) = 3.4e-4 sigma there, so the floor 2^-24 sigma in the denominator only guards R = 0.
  * everything else is relative: half an ulp each for the subtraction, the product with 2 ln 2 = 1.386..., the correctly
    rounded square root, the product with sigma and the final product, and 2 ulp for sincospif: about 8 2^-24 R.
  * both constants carry a factor 2 over that count (0.69 -> 1.4, 8 -> 16).
delta64 = 2^-50 max(R, 1): the same count in double precision (8 2^-53 R = 2^-50 R), with an absolute floor.
The ulp figures of the device intrinsics (__log2f, __fsqrt_rn, sincospif, log, sqrt, sincospi) are those of the ROCm
documentation, not measurements.

check() holds an integer output to a reference under that bound:
  always            |got - ref| < 1 + delta                    (whatever truncation does, it moves a value by < 1)
  where decidable   got == trunc(ref) wherever |ref| is further than delta from the nearest integer at which trunc
                    steps (1, 2, ...: a reference within delta of 0 still decides, the coefficient is 0)
and counts the rest as undecidable, as reject_ref.count_undecidable does for the rejection step."""
from collections import namedtuple

import numpy as np

LD = np.longdouble
if np.finfo(LD).nmant < 63:
    raise AssertionError("tests/gauss_ref.py needs np.longdouble with at least 64 mantissa bits (x86 extended precision); "
                         "this platform's has %d" % (np.finfo(LD).nmant + 1))

_PI = LD("3.14159265358979323846264338327950288")
_LN2 = LD("0.693147180559945309417232121458176568")
F32_SIGMA_LIMIT = 524288.0   # 2^19: the samplers take the F32 form below it


def _u64(hi, lo):
    return (np.asarray(hi, dtype=np.uint64) << np.uint64(32)) | np.asarray(lo, dtype=np.uint64)


def _clz64(x):
    """Leading zeros of uint64 values >= 1, exactly."""
    x = x.copy()
    n = np.zeros(x.shape, dtype=np.uint64)
    for s in (32, 16, 8, 4, 2, 1):
        small = x < (np.uint64(1) << np.uint64(64 - s))
        n = np.where(small, n + np.uint64(s), n)
        x = np.where(small, x << np.uint64(s), x)
    return n


def _cos_sin_half_turns(a):
    """(cos pi a, sin pi a) for longdouble a >= 0 that are exact multiples of 2^-60 or coarser: quadrant k = round(2 a),
    rest r = a - k / 2 (exact), |r| <= 1/4."""
    k = np.rint(2 * a)
    r = a - k / 2
    c, s = np.cos(_PI * r), np.sin(_PI * r)
    q = k.astype(np.int64) & 3
    cos = np.select([q == 0, q == 1, q == 2], [c, -s, -c], s)
    sin = np.select([q == 0, q == 1, q == 2], [s, c, -s], -c)
    return cos, sin


def _pair(R, a, swap):
    c, s = _cos_sin_half_turns(a)
    v = np.stack([R * s, R * c] if swap else [R * c, R * s], axis=-1)
    return v, R


def real_f32(words, sigma, *, angle_word=2, swap=False):
    """words: uint32 [..., 4] -> (v longdouble [..., 2], R longdouble [...]).  angle_word / swap exist for the mutation
    test only (tests/test_chacha.py): the definition is angle_word = 2, swap = False."""
    w = np.asarray(words, dtype=np.uint32)
    X = _u64(w[..., 0], w[..., 1])
    X = np.where(X == 0, np.uint64(1), X)
    lz = _clz64(X)
    top = (X << lz) >> np.uint64(40)                                  # 24 bits, top bit set
    frac = (top.astype(np.int64) - (1 << 24)).astype(LD) / LD(1 << 24)   # u0 2^lz - 1 in [-1/2, 0), exact
    ln_u0 = np.log1p(frac) - lz.astype(LD) * _LN2
    R = LD(np.float32(sigma)) * np.sqrt(-2 * ln_u0)
    a = w[..., angle_word].astype(np.float32).astype(LD) / LD(1 << 31)   # uint32 -> float32 rounds to nearest even
    return _pair(R, a, swap)


def real_f64(words, sigma, *, angle_words=(2, 3), swap=False):
    """The double-precision form; angle_words / swap as in real_f32."""
    w = np.asarray(words, dtype=np.uint32)
    n0 = (_u64(w[..., 0], w[..., 1]) >> np.uint64(11)) + np.uint64(1)      # 1 .. 2^53
    frac = (n0.astype(np.int64) - (1 << 53)).astype(LD) / LD(1 << 53)      # u0 - 1, exact
    # ln u0 without cancellation at either end: log1p near 1, log elsewhere
    ln_u0 = np.where(n0 >= np.uint64(1 << 52), np.log1p(frac), np.log(n0.astype(LD)) - 53 * _LN2)
    R = LD(np.float64(sigma)) * np.sqrt(-2 * ln_u0)
    n1 = _u64(w[..., angle_words[0]], w[..., angle_words[1]]) >> np.uint64(11)
    a = n1.astype(LD) / LD(1 << 52)                                        # 2 u1 half turns
    return _pair(R, a, swap)


def delta32(R, sigma):
    s = LD(np.float32(sigma))
    return LD(2) ** -24 * (LD("1.4") * s * s / np.maximum(R, LD(2) ** -24 * s) + 16 * R)


def delta64(R):
    return LD(2) ** -50 * np.maximum(R, LD(1))


def real(f32, words, sigma, **kw):
    """(v [..., 2], delta [..., 1]) of the chosen form."""
    v, R = (real_f32 if f32 else real_f64)(words, sigma, **kw)
    d = delta32(R, sigma) if f32 else delta64(R)
    return v, d[..., None]


def decidable(v, delta):
    """Where the bound decides the truncation: |v| further than delta from every integer at which trunc steps — the
    integers from 1 on (trunc is 0 on all of (-1, 1), so a reference at or next to 0 decides: the coefficient is 0)."""
    a = np.abs(v)
    return np.abs(a - np.maximum(np.rint(a), 1)) > delta


def decidable_share(v, delta):
    return float(decidable(v, delta).mean())


Stats = namedtuple("Stats", "n undecidable differ worst")   # differ: got != trunc(ref); worst: max (|got - ref| - 1) / delta


def check(got, v, delta, what=""):
    """The two assertions of the module docstring; got: integers of v's shape.  Returns the Stats of the comparison."""
    got = np.asarray(got)
    assert got.shape == v.shape and got.dtype == np.int64, (what, got.shape, v.shape, got.dtype)
    g = got.astype(LD)                                  # exact: |got| < 2^63
    err = np.abs(g - v)
    over = err >= 1 + delta
    assert not over.any(), "%s: %d of %d coefficients off by 1 + delta or more; first at %s: got %s, reference %s, delta %s" % (
        what, int(over.sum()), over.size, np.argwhere(over)[0].tolist(), got[over][0], v[over][0], np.broadcast_to(delta, v.shape)[over][0])
    dec = decidable(v, delta)
    want = np.trunc(v)
    wrong = dec & (g != want)
    assert not wrong.any(), "%s: %d decidable coefficients differ from trunc(reference); first at %s: got %s, reference %s" % (
        what, int(wrong.sum()), np.argwhere(wrong)[0].tolist(), got[wrong][0], v[wrong][0])
    return Stats(v.size, int((~dec).sum()), int((g != want).sum()), float(((err - 1) / delta).max()))


def violates(got, v, delta):
    """True where check() would fail (for the mutation test)."""
    try:
        check(got, v, delta)
    except AssertionError:
        return True
    return False


# ---- the words of the tests (tests/test_chacha.py on the host functions, tests/test_gpu_gauss_pin.py on the device) -------
W2_EDGES = (0, 1, 1 << 29, 1 << 30, (1 << 30) - (1 << 7), (1 << 30) + (1 << 7), 1 << 31, 3 << 30, (1 << 32) - 129,
            (1 << 32) - 128, (1 << 32) - 1)   # quadrants; 2^32 - 129 rounds down, 2^32 - 128 (a tie) and 2^32 - 1 up to a full turn


def x_edges_f32():
    """X = w0:w1 at the ends of the F32 form: 0 (taken as 1), 1 (lz = 63), both sides of lz 0 / 1, all ones, the largest
    24-bit top alone, and the cancellation region — lz = 0 with top = 2^24 - 1 .. 2^24 - 20, once with the 40 bits below
    the top clear and once with all of them set (they do not count)."""
    xs = [0, 1, 1 << 63, (1 << 63) - 1, (1 << 64) - 1, ((1 << 24) - 1) << 40]
    for t in range(1, 21):
        top = (1 << 24) - t
        xs += [top << 40, (top << 40) | ((1 << 40) - 1)]
    return xs


def edge_words_f32():
    """uint32 [len(x_edges_f32()) * len(W2_EDGES), 4]: every edge X with every edge w2 (w3 is not read)."""
    rows = [(x >> 32, x & 0xFFFFFFFF, w2, 0xDEADBEEF) for x in x_edges_f32() for w2 in W2_EDGES]
    return np.array(rows, dtype=np.uint64).astype(np.uint32)


def edge_words_f64():
    """uint32 [n, 4]: X >> 11 in {0, 2^53 - 1} (u0 = 2^-53, the largest radius, and u0 = 1, radius 0: both outputs 0), with
    and without the 11 bits that do not count, and two radii in between, each with u1 in {0, 1/4, 1/2, 3/4}, again with
    and without the dropped bits, and one step to either side of each quadrant."""
    xs = [0, (1 << 11) - 1, ((1 << 53) - 1) << 11, (1 << 64) - 1, 1 << 63, 0x0123456789ABCDEF]
    ys = []
    for q in range(4):
        y = q << 62
        ys += [y, y | ((1 << 11) - 1), y + (1 << 11), (y - (1 << 11)) % (1 << 64)]
    rows = [(x >> 32, x & 0xFFFFFFFF, y >> 32, y & 0xFFFFFFFF) for x in xs for y in ys]
    return np.array(rows, dtype=np.uint64).astype(np.uint32)


def random_words(seed, pairs):
    return np.random.default_rng(seed).integers(0, 1 << 32, (pairs, 4), dtype=np.uint64).astype(np.uint32)
