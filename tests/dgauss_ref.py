"""Python-integer restatement of the exact discrete Gaussian sampler (the library's statement is
ring_zk_amd/csrc/rzk_dgauss.h): the parameters of sigma, one trial on 8 words, and the word stream of a call.  Test
infrastructure: shares no code with the library; the ChaCha20 blocks come from tests/chacha_ref.py.  The constants
below are data (tools/gen_dgauss_consts.py prints them); K is asserted against mpmath by tests/test_dgauss_host.py.

    K = floor(2^127 log2 e), C = K div sigma^2, k = least integer with k^2 C >= 2^128
    trial(w[0..7]):  X = w0:w1, m = X W; m mod 2^64 < 2^64 mod W rejects; u = m >> 64; x = #{i : u >= CUM[i]}
                     m = w2 k; m mod 2^32 < 2^32 mod k rejects; y = m >> 32;  z = k x + y
                     E = z^2 C >> 64;  a = (E >> 64) - x^2, f = E mod 2^64
                     a >= 64 rejects; (a, f) = (0, 0) accepts; else w4:w5 < T accepts, T = 2^(64-a) if f = 0 else exp2m(f) >> a
                     z = 0 and w3 bit 1 rejects; value = -z if w3 bit 0 else z
    stream:          trial t of pair j of polynomial p: block(subkey, 0x80000000 | t << 16 | j, p lo, p hi, stream),
                     words 0..7 -> coefficient 2j, words 8..15 -> coefficient 2j + 1; first accepted trial, t < T_MAX,
                     else 0
"""
from math import isqrt

import numpy as np

import chacha_ref

M64 = (1 << 64) - 1
K = 0xB8AA3B295C17F0BBBE87FED0691D3E88
W = sum(1 << (49 - x * x) for x in range(8))
CUM = [sum(1 << (49 - i * i) for i in range(x + 1)) for x in range(7)]
COEF = [0xB17217F7D1CF79AC, 0x3D7F7BFF058B1D51, 0x0E35846B82505FC6, 0x0276556DF749CEE5, 0x005761FF9E299CC4,
        0x000A184897C363C4, 0x0000FFE5FE2C4586, 0x0000162C0223A5C8, 0x000001B5253D395E, 0x0000001E4CF5158C,
        0x00000001E8CAC735, 0x000000001C3BD651, 0x0000000001816193, 0x0000000000131496, 0x000000000000E1B7]   # c_1 .. c_15
R = 0xB504F333F9DE6484
T_MAX = 160
SIGMA_MAX = 1 << 26
EPS_B = 2.0 ** -61   # documented bound of the acceptance probability's absolute error
REJECT, THRESHOLD, ALWAYS = 0, 1, 2


def params(sigma):
    """(C, k) of an integer sigma in [1, 2^26]."""
    assert 1 <= sigma <= SIGMA_MAX
    C = K // (sigma * sigma)
    k = isqrt(((1 << 128) + C - 1) // C - 1) + 1   # least k with k^2 >= ceil(2^128 / C)
    assert k * k * C >= 1 << 128 > (k - 1) * (k - 1) * C
    return C, k


def exp2m(f):
    """2^64 2^(-f / 2^64) in fixed point, f in [1, 2^64)."""
    g = f & ((1 << 63) - 1)
    p = COEF[14]
    for c in COEF[13::-1]:
        p = c - (g * p >> 64)
    v = M64 - (g * p >> 64)
    return v * R >> 64 if f >> 63 else v


def threshold(a, f):
    if a >= 64:
        return REJECT, 0
    if f == 0:
        return (ALWAYS, 0) if a == 0 else (THRESHOLD, 1 << (64 - a))
    return THRESHOLD, exp2m(f) >> a


def exponent(C, k, x, y):
    z = k * x + y
    E = z * z * C >> 64
    return (E >> 64) - x * x, E & M64


def trial(C, k, w):
    """w: 8 words -> (accepted, value)."""
    m = ((w[0] << 32) | w[1]) * W
    ok = (m & M64) >= (1 << 64) % W
    u = m >> 64
    x = sum(u >= c for c in CUM)
    m = w[2] * k
    ok = ok and (m & 0xFFFFFFFF) >= (1 << 32) % k
    y = m >> 32
    a, f = exponent(C, k, x, y)
    assert a >= 0
    kind, T = threshold(a, f)
    ok = ok and (kind == ALWAYS or (kind == THRESHOLD and ((w[4] << 32) | w[5]) < T))
    z = k * x + y
    ok = ok and not (z == 0 and w[3] & 2)
    return bool(ok), (-z if w[3] & 1 else z)


def w12_of(t, j):
    return 0x80000000 | (t << 16) | j


def sample(key, nonce, stream, N, sigma, polys, t_max=T_MAX, used=None):
    """int64 [len(polys), N]: the polynomials with the given indices of a draw.  `used`, a set, collects the w12 of every
    block read."""
    C, k = params(sigma)
    sub = chacha_ref.le_words(chacha_ref.hchacha20(key, nonce))
    polys = [int(p) for p in polys]
    out = np.zeros((len(polys), N), dtype=np.int64)
    pend = [(i, j, 3 if 2 * j + 1 < N else 1) for i in range(len(polys)) for j in range((N + 1) // 2)]   # bit c: coefficient 2j + c is open
    for t in range(t_max):
        if not pend:
            break
        w12 = np.array([w12_of(t, j) for _, j, _ in pend], dtype=np.uint64)
        pp = np.array([polys[i] for i, _, _ in pend], dtype=np.uint64)
        blocks = chacha_ref.block_words(sub, w12, pp & np.uint64(0xFFFFFFFF), pp >> np.uint64(32), stream).tolist()
        if used is not None:
            used.update(int(v) for v in w12)
        nxt = []
        for (i, j, mask), w in zip(pend, blocks):
            for c in (0, 1):
                if mask >> c & 1:
                    ok, v = trial(C, k, w[8 * c:8 * c + 8])
                    if ok:
                        out[i, 2 * j + c] = v
                        mask &= ~(1 << c)
            if mask:
                nxt.append((i, j, mask))
        pend = nxt
    return out


# ---- words at the edges of a trial (shared by the host and the GPU test) -------------------------------------------------
def x_words(u):
    """(w0, w1) whose Lemire draw gives exactly u in [0, W) and is not rejected (the least such X)."""
    X = ((u << 64) + W - 1) // W
    while (X * W & M64) < (1 << 64) % W:
        X += 1
    assert X <= M64 and X * W >> 64 == u
    return X >> 32, X & 0xFFFFFFFF


def y_word(k, y):
    """w2 that gives y in [0, k) and is not rejected (the least one)."""
    w2 = ((y << 32) + k - 1) // k
    while (w2 * k & 0xFFFFFFFF) < (1 << 32) % k:
        w2 += 1
    assert w2 < 1 << 32 and w2 * k >> 32 == y
    return w2


def words_for(k, x, y, r=0, bits=0, w6=0x6A09E667, w7=0xBB67AE85):
    w0, w1 = x_words(CUM[x - 1] if x else 0)
    return [w0, w1, y_word(k, y), bits, r >> 32, r & 0xFFFFFFFF, w6, w7]


def edge_words(sigma):
    """List of (label, 8 words) at the edges of one trial for this sigma; every tuple is valid input."""
    C, k = params(sigma)
    inv = pow(W, -1, 1 << 64)
    out = []
    # x: the largest X (x = 7), both sides of every cumulative sum, both sides of the Lemire rejection
    out.append(("x=7 largest X", [0xFFFFFFFF, 0xFFFFFFFF, y_word(k, k - 1), 0, 0, 0, 1, 2]))
    for i, c in enumerate(CUM):
        for u in (c - 1, c):
            w0, w1 = x_words(u)
            out.append(("x cum %d u=%d" % (i, u), [w0, w1, y_word(k, 0), 0, 0, 0, 3, 4]))
    for lo in ((1 << 64) % W - 1, (1 << 64) % W, 0):
        X = lo * inv & M64
        assert X * W & M64 == lo
        out.append(("x lemire lo=%d" % lo, [X >> 32, X & 0xFFFFFFFF, y_word(k, 1 % k), 0, 0, 0, 5, 6]))
    # y: the words whose low product is closest to 2^32 mod k from below and from above, and the last word
    rej = (1 << 32) % k
    cand = {}
    for y in range(min(k, 1 << 16)):
        w2 = ((y << 32) + k - 1) // k
        for d in (0, 1):
            if (w2 + d) * k >> 32 == y:
                cand[(w2 + d) * k & 0xFFFFFFFF] = w2 + d
    below = [lo for lo in cand if lo < rej]
    assert bool(below) == (rej != 0)   # k a power of two rejects no word; every other k of the tests has a candidate
    if below:
        out.append(("y below the edge", words_for(k, 0, 0)[:2] + [cand[max(below)], 0, 0, 0, 7, 8]))
    out.append(("y at the edge", words_for(k, 0, 0)[:2] + [cand[min(lo for lo in cand if lo >= rej)], 0, 0, 0, 9, 10]))
    out.append(("y last word", words_for(k, 1, 0)[:2] + [0xFFFFFFFF, 1, 0xFFFFFFFF, 0xFFFFFFFF, 11, 12]))
    # z = 0: both coins, both signs
    for bits in range(4):
        out.append(("z=0 bits=%d" % bits, words_for(k, 0, 0, r=M64, bits=bits)))
    # the random word at threshold - 1 and at threshold, for a few candidates; and the largest a of this sigma
    zs = [(0, 1 % k), (1, 0), (1, k - 1), (2, k // 2), (5, 1 % k), (6, 0), (7, 0), (7, k - 1)]   # sigma = 1: a = 62 at z = 11, 67 at z = 12
    for x, y in zs:
        a, f = exponent(C, k, x, y)
        kind, T = threshold(a, f)
        if kind == THRESHOLD:
            for r in (T - 1, T):
                if 0 <= r <= M64:
                    out.append(("x=%d y=%d a=%d r=T%+d" % (x, y, a, r - T), words_for(k, x, y, r=r, bits=1)))
        else:
            out.append(("x=%d y=%d a=%d kind=%d" % (x, y, a, kind), words_for(k, x, y, r=0, bits=1)))
    return out
