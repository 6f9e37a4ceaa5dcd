"""The "XP1" seed expansion restated with hashlib.shake_256 and Python integers; shares no code with
the library (ring_zk_amd/csrc/rzk_xof.h is the other statement).

    CH        = min(N, 256), C = N / CH; W = bitlen(q - 1), mask = 2^W - 1
    msg(p, c) = "RZKXP1\\0U" | le64(q) | le32(N) | le32(domain) | seed[0:32] | le32(p) | le32(c)          64 bytes
    stream    = SHAKE256(msg(p, c)) as little-endian 32-bit words
    a word w gives the candidate v = w & mask, accepted iff v < q, value v - (q - 1) / 2
    chunk c of polynomial p = the first CH accepted values -> coefficients c CH .. c CH + CH - 1
"""
import hashlib
import struct

import numpy as np

TAG = b"RZKXP1\x00U"
DOMAIN_KEY = 0
RATE_WORDS32 = 34   # 32-bit words per SHAKE256 rate block


def chunk_len(N):
    return min(N, 256)


def message(q, N, domain, seed, p, c):
    seed = bytes(seed)
    assert len(seed) == 32
    return TAG + struct.pack("<QII", q, N, domain) + seed + struct.pack("<II", p, c)


def chunk(q, N, domain, seed, p, c):
    """(values, words used) of chunk c of polynomial p."""
    ch = chunk_len(N)
    W = (q - 1).bit_length()
    mask = (1 << W) - 1
    half = (q - 1) // 2
    msg = message(q, N, domain, seed, p, c)
    nwords = 2 * ch + 64
    while True:
        stream = hashlib.shake_256(msg).digest(4 * nwords)
        vals = []
        for i in range(nwords):
            v = int.from_bytes(stream[4 * i:4 * i + 4], "little") & mask
            if v < q:
                vals.append(v - half)
                if len(vals) == ch:
                    return vals, i + 1
        nwords *= 2   # (a prefix of the same stream: SHAKE output does not depend on the length asked for)


def poly(q, N, domain, seed, p):
    out = []
    for c in range(N // chunk_len(N)):
        out += chunk(q, N, domain, seed, p, c)[0]
    return np.array(out, dtype=np.int64)


def uniform(q, N, domain, seeds, rows):
    """[B][rows][N]: out[b][r] = polynomial r under seeds[b] and `domain`."""
    return np.stack([np.stack([poly(q, N, domain, s, r) for r in range(rows)]) for s in seeds])


def key(q, N, n, k, l, seed):
    """CommitmentKey::new with a1 = [I_n | a1'], a2 = [0 | I_l | a2']; general entry (i, j) is polynomial i k + j, domain 0."""
    a = np.zeros((n + l, k, N), dtype=np.int64)
    for i in range(n + l):
        a[i, i, 0] = 1
        for j in range(n if i < n else n + l, k):
            a[i, j] = poly(q, N, DOMAIN_KEY, seed, i * k + j)
    return a


def sha256_of(coefs):
    return hashlib.sha256(np.ascontiguousarray(coefs, dtype="<i8").tobytes()).hexdigest()


def seed_of(i):
    """Seed i of the search for the edge conditions: sha256(le32(i))."""
    return hashlib.sha256(struct.pack("<I", i)).digest()
