"""Python restatement of the FS1 Fiat-Shamir transcript over hashlib's SHAKE256.  Test infrastructure:
shares no code with the library; tests/test_fs_transcript.py (CPU) and tests/test_gpu_fiat_shamir.py compare against it.

    leaf(p,c)  = SHAKE256( b"RZKFS1\\0L" | le32(p) | le32(c) | coefficients of P_p[c*LEAF : (c+1)*LEAF] )[0:32]
    keydigest  = SHAKE256( b"RZKFS1\\0K" | le64(q) | le32(N) le32(n) le32(k) le32(l) le32(kappa) le32(0) | le64(b)
                           | leaf(p,c) of the (n+l)*k key polynomials row-major, all c )[0:32]
    stream     = SHAKE256( b"RZKFS1\\0R" | le32(kind) | le32(V) | keydigest | aux[32] | leaf(p,c), p in 0..M-1, c in 0..C-1 )

LEAF = min(N, 256), C = N / LEAF; a coefficient is the little-endian two's-complement int32 of its centred value; the
message polynomials P_0..P_{M-1} are the fields in declaration order, each slab flattened row-major.  stream[0:32] is
the transcript digest; the challenge comes from stream[32:] read as little-endian 16-bit words.
"""
import hashlib
import struct

import numpy as np

OPEN_COMMITMENT, LINEAR_COMMITMENT, SUM_COMMITMENT = 3, 5, 6   # RZK_MSG_* (include/rzk.h)


def shake256(data: bytes, outlen: int) -> bytes:
    return hashlib.shake_256(data).digest(outlen)


def leaf_len(N):
    return min(N, 256)


def leaves(polys, N, first=0):
    """Concatenated leaf digests of polynomials [M][N] (numbered from `first`)."""
    polys = np.asarray(polys, dtype=np.int64).reshape(-1, N)
    L = leaf_len(N)
    out = b""
    for p, poly in enumerate(polys):
        for c in range(N // L):
            chunk = poly[c * L:(c + 1) * L].astype("<i4").tobytes()
            out += shake256(b"RZKFS1\0L" + struct.pack("<II", first + p, c) + chunk, 32)
    return out


def key_digest(A, q, N, n, k, l, kappa, b):
    A = np.asarray(A, dtype=np.int64).reshape((n + l) * k, N)
    head = b"RZKFS1\0K" + struct.pack("<QIIIIIIQ", q, N, n, k, l, kappa, 0, b)
    return shake256(head + leaves(A, N), 32)


def sample(stream: bytes, N, kappa):
    """(challenge [N] int64, 16-bit words consumed) from stream[32:]."""
    pos = 32
    c = [0] * N
    for i in range(N - kappa, N):
        mask = (1 << i.bit_length()) - 1
        while True:
            w = stream[pos] | (stream[pos + 1] << 8)
            pos += 2
            j = w & mask
            if j <= i:
                break
        c[i] = c[j]
        c[j] = 1 - 2 * (w >> 15)
    return np.array(c, dtype=np.int64), (pos - 32) // 2


def challenge_one(kind, V, keydig, aux, fields, N, kappa):
    """(d [N], digest bytes) of one proof; fields: its slabs in declaration order, each [..., N]."""
    polys = np.concatenate([np.asarray(f, dtype=np.int64).reshape(-1, N) for f in fields])
    msg = b"RZKFS1\0R" + struct.pack("<II", kind, V) + keydig + aux + leaves(polys, N)
    stream = shake256(msg, 32 + 2 * 40 * max(kappa, 8))   # far more words than the sampler reads (a word is accepted with probability > 1/2)
    d, _ = sample(stream, N, kappa)
    return d, stream[:32]


def challenge(kind, V, keydig, aux, fields, N, kappa):
    """Batched: fields [B, ..., N] each -> (d [B][N] int64, digest [B][32] uint8)."""
    aux = bytes(32) if aux is None else bytes(aux)
    B = fields[0].shape[0]
    ds, digs = [], []
    for b in range(B):
        d, dig = challenge_one(kind, V, keydig, aux, [f[b] for f in fields], N, kappa)
        ds.append(d)
        digs.append(np.frombuffer(dig, dtype=np.uint8))
    return np.stack(ds), np.stack(digs)
