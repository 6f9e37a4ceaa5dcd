"""The packed proof format "RZKP1" restated in Python integers (include/rzk.h "fixed-width packed records").

Shares no code with the library: a polynomial is packed through ONE big integer, sum raw_i << (i W), written out as
ceil(N W / 64) little-endian 64-bit words.  Used by tests/test_packed_host.py (against ring_zk_amd/csrc/rzk_packed.h under
g++) and tests/test_gpu_packed.py (against the GPU codec)."""
import math
from collections import namedtuple

import numpy as np

(COMMITMENT, OPENING, CHALLENGE, OPEN_COMMITMENT, OPEN_RESPONSE, LINEAR_COMMITMENT, SUM_COMMITMENT, SUM_RESPONSE,
 LINEAR_RESPONSE, OPEN_SHORT) = range(10)
KINDS = (COMMITMENT, CHALLENGE, OPEN_COMMITMENT, OPEN_RESPONSE, LINEAR_COMMITMENT, SUM_COMMITMENT, SUM_RESPONSE,
         LINEAR_RESPONSE, OPEN_SHORT)
SUM_KINDS = (SUM_COMMITMENT, SUM_RESPONSE)

Cls = namedtuple("Cls", "W bias limit")
Ctx = namedtuple("Ctx", "N n k l q verify_bound")


def verify_bound(N, k, kappa, b):
    """2 sigma floor(sqrt N), sigma = 11 kappa b floor(sqrt(k N)) (params.rs:94-98, 114)."""
    return 2 * (11 * kappa * b * math.isqrt(k * N)) * math.isqrt(N)


def make_ctx(N, n, k, l, q, kappa=36, b=1):
    return Ctx(N, n, k, l, q, verify_bound(N, k, kappa, b))


def cls_of(bias, limit):
    W = int(limit).bit_length()
    assert (1 << W) - 1 > limit, "all-ones must lie above the limit"
    return Cls(W, bias, limit)


def classes(ctx):
    return {"Q": cls_of((ctx.q - 1) // 2, ctx.q - 1), "Z": cls_of(ctx.verify_bound, 2 * ctx.verify_bound), "D": cls_of(1, 2)}


def fields(ctx, kind, V=None):
    """[(name, class letter, polynomials per record)] in declaration order."""
    n, k, l = ctx.n, ctx.k, ctx.l
    if kind in SUM_KINDS:
        assert V and 1 <= V <= 65535
    return {
        COMMITMENT: [("c", "Q", n + l)],
        CHALLENGE: [("d", "D", 1)],
        OPEN_COMMITMENT: [("c", "Q", n + l), ("t", "Q", n)],
        OPEN_RESPONSE: [("z", "Z", k)],
        LINEAR_COMMITMENT: [("c", "Q", n + l), ("cp", "Q", n + l), ("g", "Q", 1), ("t", "Q", n), ("tp", "Q", n), ("u", "Q", l)],
        SUM_COMMITMENT: [("cp", "Q", n + l), ("cs", "Q", (V or 0) * (n + l)), ("gs", "Q", V or 0), ("tp", "Q", n),
                         ("ts", "Q", (V or 0) * n), ("u", "Q", l)],
        SUM_RESPONSE: [("zp", "Z", k), ("zs", "Z", (V or 0) * k)],
        LINEAR_RESPONSE: [("z", "Z", k), ("zp", "Z", k)],
        OPEN_SHORT: [("c", "Q", n + l), ("d", "D", 1), ("z", "Z", k)],
    }[kind]


def poly_bytes(N, W):
    return 8 * ((N * W + 63) // 64)


def record_bytes(ctx, kind, V=None):
    cl = classes(ctx)
    return 8 + sum(rows * poly_bytes(ctx.N, cl[c].W) for _, c, rows in fields(ctx, kind, V))


def header(kind, V):
    return b"RZKP" + bytes([1, kind]) + int(V).to_bytes(2, "little")


def pack_poly(coefs, cls):
    """(bytes, ok): one big integer; a coefficient outside [-bias, limit - bias] becomes all-ones and clears ok."""
    big, ok = 0, True
    for i, c in enumerate(coefs):
        raw = int(c) + cls.bias
        if not 0 <= raw <= cls.limit:
            raw, ok = (1 << cls.W) - 1, False
        big |= raw << (i * cls.W)
    return big.to_bytes(poly_bytes(len(coefs), cls.W), "little"), ok


def unpack_poly(data, N, cls):
    """(coefficients, ok): ok = every raw <= limit and no bit set above N W."""
    big = int.from_bytes(data, "little")
    mask = (1 << cls.W) - 1
    raws = [(big >> (i * cls.W)) & mask for i in range(N)]
    ok = all(r <= cls.limit for r in raws) and (big >> (N * cls.W)) == 0
    return [r - cls.bias for r in raws], ok


def encode(ctx, kind, slabs, V=None):
    """slabs: one int64 array [B, ..., N] per field -> (records uint8 [B][record_bytes], ok uint8 [B])."""
    cl, fl = classes(ctx), fields(ctx, kind, V)
    assert len(slabs) == len(fl)
    B = slabs[0].shape[0]
    hv = V if kind in SUM_KINDS else 0
    recs, oks = [], []
    for b in range(B):
        out, ok = [header(kind, hv)], True
        for (_, c, rows), slab in zip(fl, slabs):
            flat = np.asarray(slab[b]).reshape(rows, ctx.N)
            for r in range(rows):
                data, good = pack_poly(flat[r].tolist(), cl[c])
                out.append(data)
                ok = ok and good
        recs.append(b"".join(out))
        oks.append(int(ok))
    size = record_bytes(ctx, kind, V)
    assert all(len(r) == size for r in recs)
    return np.frombuffer(b"".join(recs), dtype=np.uint8).reshape(B, size).copy(), np.array(oks, dtype=np.uint8)


def decode(ctx, kind, records, shapes, V=None):
    """records uint8 [B][record_bytes] -> (slabs with the per-message shapes given, ok)."""
    cl, fl = classes(ctx), fields(ctx, kind, V)
    B = records.shape[0]
    hv = V if kind in SUM_KINDS else 0
    slabs = [np.zeros((B,) + tuple(sh), dtype=np.int64) for sh in shapes]
    oks = []
    for b in range(B):
        raw = records[b].tobytes()
        ok = raw[:8] == header(kind, hv)
        pos = 8
        for (_, c, rows), slab in zip(fl, slabs):
            flat = slab[b].reshape(rows, ctx.N)
            nb = poly_bytes(ctx.N, cl[c].W)
            for r in range(rows):
                coefs, good = unpack_poly(raw[pos:pos + nb], ctx.N, cl[c])
                flat[r] = coefs
                ok = ok and good
                pos += nb
        assert pos == len(raw)
        oks.append(int(ok))
    return slabs, np.array(oks, dtype=np.uint8)
