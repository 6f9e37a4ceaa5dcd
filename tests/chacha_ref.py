"""Python / numpy restatement of the keyed samplers' generator: the ChaCha20 block function (RFC 8439
§2.3), HChaCha20 (draft-irtf-cfrg-xchacha §2.2), the counter layout, the uniform and challenge samplers, and the words
behind every coefficient pair of the Gaussian sampler (the map from words to a pair is tests/gauss_ref.py).  Test
infrastructure: shares no code with the library; tests/test_chacha.py (CPU), tests/test_gpu_keyed_samplers.py and
tests/test_gpu_gauss_pin.py compare against it.

    subkey                   = HChaCha20(key[32], nonce[16])
    block(stream, poly, blk) = ChaCha20_block(subkey, w12 = blk, w13 = poly & 0xffffffff, w14 = poly >> 32, w15 = stream)
    uniform    coefficient 8 blk + j = ((w[2j] : w[2j+1]) * (2 bound + 1) >> 64) - bound
    challenge  Floyd step t (block t >> 3, s = t & 7): pick = ((w[2s] : w[2s+1] & ~1) * (j + 1)) >> 64 with
               j = N - kappa + t, sign +1 if w[2s+1] & 1 else -1; position = pick if it is free, else j
    gauss      coefficients 8 blk + 2i, 8 blk + 2i + 1 from quarter i of the block, w[4i .. 4i+3]

All block arithmetic is vectorised over a leading axis of blocks (uint32 numpy arrays, wrap-around adds).
"""
import numpy as np

SIGMA = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)   # "expand 32-byte k"
M32 = 0xFFFFFFFF


def _rotl(x, n):
    return (x << np.uint32(n)) | (x >> np.uint32(32 - n))


def _quarter(x, a, b, c, d):
    x[a] = x[a] + x[b]; x[d] = _rotl(x[d] ^ x[a], 16)
    x[c] = x[c] + x[d]; x[b] = _rotl(x[b] ^ x[c], 12)
    x[a] = x[a] + x[b]; x[d] = _rotl(x[d] ^ x[a], 8)
    x[c] = x[c] + x[d]; x[b] = _rotl(x[b] ^ x[c], 7)


def _rounds(state):
    """state: list of 16 uint32 arrays of one shape -> the state after 20 rounds (new list)."""
    x = [s.copy() for s in state]
    with np.errstate(over="ignore"):
        for _ in range(10):
            _quarter(x, 0, 4, 8, 12); _quarter(x, 1, 5, 9, 13); _quarter(x, 2, 6, 10, 14); _quarter(x, 3, 7, 11, 15)
            _quarter(x, 0, 5, 10, 15); _quarter(x, 1, 6, 11, 12); _quarter(x, 2, 7, 8, 13); _quarter(x, 3, 4, 9, 14)
    return x


def _state(key_words, w12, w13, w14, w15):
    w = [np.asarray(v, dtype=np.uint64) for v in (w12, w13, w14, w15)]
    shape = np.broadcast(*w).shape
    full = lambda v: np.broadcast_to(np.asarray(v, dtype=np.uint64) & M32, shape).astype(np.uint32)
    return [full(v) for v in SIGMA] + [full(v) for v in key_words] + [full(v) for v in w]


def block_words(key_words, w12, w13, w14, w15):
    """ChaCha20 blocks for (broadcast) arrays of the words 12..15 -> uint32 [..., 16]."""
    s = _state(key_words, w12, w13, w14, w15)
    x = _rounds(s)
    with np.errstate(over="ignore"):
        return np.stack([a + b for a, b in zip(x, s)], axis=-1)


def le_words(data: bytes):
    return [int.from_bytes(data[i:i + 4], "little") for i in range(0, len(data), 4)]


def block_bytes(key: bytes, w12, w13, w14, w15) -> bytes:
    return block_words(le_words(key), w12, w13, w14, w15).astype("<u4").tobytes()


def hchacha20(key: bytes, nonce: bytes) -> bytes:
    assert len(key) == 32 and len(nonce) == 16
    x = _rounds(_state(le_words(key), *le_words(nonce)))
    return b"".join(int(x[i]).to_bytes(4, "little") for i in (0, 1, 2, 3, 12, 13, 14, 15))


def sampler_blocks(key: bytes, nonce: bytes, stream: int, polys, nblk: int):
    """Blocks 0 .. nblk-1 of every polynomial index in `polys` -> uint32 [len(polys), nblk, 16]."""
    sub = le_words(hchacha20(key, nonce))
    polys = np.asarray(polys, dtype=np.uint64).reshape(-1, 1)
    blk = np.arange(nblk, dtype=np.uint64).reshape(1, -1)
    return block_words(sub, blk, polys & np.uint64(M32), polys >> np.uint64(32), stream)


def _mulhi64(hi, lo, rng):
    """floor(((hi << 32) | lo) * rng / 2^64) for uint32 arrays hi, lo and 0 < rng <= 2^32, in exact integer arithmetic."""
    hi, lo = hi.astype(np.uint64), lo.astype(np.uint64)
    r = np.uint64(rng)
    return (hi * r + ((lo * r) >> np.uint64(32))) >> np.uint64(32)   # hi * r + carry < 2^64: no overflow


def uniform(key: bytes, nonce: bytes, stream: int, N: int, bound: int, polys):
    """int64 [len(polys), N]: the polynomials with the given indices of a uniform draw in [-bound, bound]."""
    nblk = max(N // 8, 1)
    w = sampler_blocks(key, nonce, stream, polys, nblk)                       # [P, nblk, 16]
    v = _mulhi64(w[..., 0::2], w[..., 1::2], 2 * bound + 1).astype(np.int64) - bound   # [P, nblk, 8]
    return v.reshape(len(w), nblk * 8)[:, :N]


def challenge(key: bytes, nonce: bytes, stream: int, N: int, kappa: int, polys):
    """int64 [len(polys), N]: kappa coefficients +-1 per polynomial (Floyd's subset, one step per word pair)."""
    kap = min(kappa, N)
    nblk = (kap + 7) // 8
    w = sampler_blocks(key, nonce, stream, polys, nblk).reshape(len(polys), nblk * 16)
    out = np.zeros((len(polys), N), dtype=np.int64)
    for p in range(len(polys)):
        for t in range(kap):
            w0, w1 = int(w[p, 2 * t]), int(w[p, 2 * t + 1])
            j = N - kap + t
            pick = ((((w0 << 32) | (w1 & ~1 & M32)) * (j + 1)) >> 64)
            pos = j if out[p, pick] else pick
            out[p, pos] = 1 if (w1 & 1) else -1
    return out


def gauss_words(key: bytes, nonce: bytes, stream: int, N: int, polys, quarter_xor: int = 0):
    """uint32 [len(polys), N / 2, 4]: the word quadruple behind every coefficient pair of a Gaussian draw, quarter i of
    block blk for the pair 4 blk + i.  quarter_xor != 0 exists for the mutation test only (pair i reads quarter
    i ^ quarter_xor)."""
    nblk = max(N // 8, 1)
    w = sampler_blocks(key, nonce, stream, polys, nblk).reshape(len(polys), nblk, 4, 4)
    if quarter_xor:
        w = w[:, :, np.arange(4) ^ quarter_xor, :]
    return w.reshape(len(polys), nblk * 4, 4)[:, :N // 2]
