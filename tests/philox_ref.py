"""numpy restatement of the seeded samplers' generator (ring_zk_amd/csrc/rzk_rng.h): Philox4x32-10 (Salmon et al., SC'11)
with the samplers' counter layout.  Test infrastructure: shares no code with the library; tests/test_chacha.py checks it
against the Random123 known answers and the CPU emulator's uniform sampler, tests/test_gpu_gauss_pin.py feeds its words
to tests/gauss_ref.py.

    block(seed, stream, poly, blk) = Philox4x32-10(counter = (blk, poly & 0xffffffff, poly >> 32, stream),
                                                   key = (seed & 0xffffffff, seed >> 32))
    block blk of a polynomial gives its coefficients 2 blk and 2 blk + 1

All arithmetic is vectorised over broadcast uint64 arrays holding 32-bit values."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57       # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85       # key schedule (Weyl sequence)
M32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(ctr, key):
    """ctr: 4 and key: 2 (broadcastable) integer arrays of 32-bit values -> uint32 [..., 4]."""
    c = [np.asarray(v, dtype=np.uint64) & M32 for v in ctr]
    k0, k1 = (np.asarray(v, dtype=np.uint64) & M32 for v in key)
    c = list(np.broadcast_arrays(*c, k0, k1)[:4])
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]          # 32 x 32 -> 64 bits: no overflow
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> S32) ^ c[1] ^ k0, p1 & M32, (p0 >> S32) ^ c[3] ^ k1, p0 & M32]
        k0 = (k0 + np.uint64(W0)) & M32
        k1 = (k1 + np.uint64(W1)) & M32
    return np.stack(c, axis=-1).astype(np.uint32)


def sampler_blocks(seed: int, stream: int, polys, nblk: int):
    """Blocks 0 .. nblk-1 of every polynomial index in `polys` -> uint32 [len(polys), nblk, 4]."""
    polys = np.asarray(list(polys), dtype=np.uint64).reshape(-1, 1)
    blk = np.arange(nblk, dtype=np.uint64).reshape(1, -1)
    return philox4x32_10((blk, polys & M32, polys >> S32, np.uint64(stream)), (np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)))


def gauss_words(seed: int, stream: int, N: int, polys):
    """The word quadruple behind every coefficient pair of a Gaussian draw -> uint32 [len(polys), N / 2, 4]."""
    return sampler_blocks(seed, stream, polys, N // 2)


def uniform(seed: int, stream: int, N: int, bound: int, polys):
    """int64 [len(polys), N]: sample_uniform_kernel's polynomials (floor(w:w' (2 bound + 1) / 2^64) - bound per word pair)."""
    w = sampler_blocks(seed, stream, polys, N // 2).astype(np.uint64)
    r = np.uint64(2 * bound + 1)

    def below(hi, lo):
        return (hi * r + ((lo * r) >> S32)) >> S32     # hi r + carry < 2^64

    v = np.stack([below(w[..., 0], w[..., 1]), below(w[..., 2], w[..., 3])], axis=-1).astype(np.int64) - bound
    return v.reshape(len(w), N)
