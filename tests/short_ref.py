"""The two short-proof kinds of the packed format "RZKP1" (include/rzk.h: RZK_MSG_LINEAR_SHORT, RZK_MSG_SUM_SHORT; DESIGN.md
§16) restated on top of tests/packed_ref.py's polynomial rules (one big integer per polynomial, classes Q / Z / D).

A short record is the full commitment kind's fields in their declaration order with t / tp / ts / u removed, then d
(class D), then the response kind's fields.  Used by tests/test_short_host.py (against rzk_packed.h under g++) and
tests/test_gpu_short.py (against the GPU codec)."""
import numpy as np

import packed_ref as PR

LINEAR_SHORT, SUM_SHORT = 11, 12
KINDS = (LINEAR_SHORT, SUM_SHORT)
DROPPED = ("t", "tp", "ts", "u")


def fields(ctx, kind, V=None):
    """[(name, class letter, polynomials per record)]: derived from the full kinds, not written out again."""
    if kind == LINEAR_SHORT:
        full, resp, V = PR.LINEAR_COMMITMENT, PR.LINEAR_RESPONSE, None
    elif kind == SUM_SHORT:
        assert V and 1 <= V <= 65535
        full, resp = PR.SUM_COMMITMENT, PR.SUM_RESPONSE
    else:
        raise KeyError(kind)
    kept = [f for f in PR.fields(ctx, full, V) if f[0] not in DROPPED]
    return kept + [("d", "D", 1)] + PR.fields(ctx, resp, V)


def header_v(kind, V):
    return V if kind == SUM_SHORT else 0


def record_bytes(ctx, kind, V=None):
    cl = PR.classes(ctx)
    return 8 + sum(rows * PR.poly_bytes(ctx.N, cl[c].W) for _, c, rows in fields(ctx, kind, V))


def field_byte_ranges(ctx, kind, V=None):
    """[(first byte, last byte)] of every field inside a record."""
    cl, out, pos = PR.classes(ctx), [], 8
    for _, c, rows in fields(ctx, kind, V):
        size = rows * PR.poly_bytes(ctx.N, cl[c].W)
        out.append((pos, pos + size - 1))
        pos += size
    return out


def encode(ctx, kind, slabs, V=None):
    """slabs: one int64 array [B, ..., N] per field -> (records uint8 [B][record_bytes], ok uint8 [B])."""
    cl, fl = PR.classes(ctx), fields(ctx, kind, V)
    assert len(slabs) == len(fl)
    B = slabs[0].shape[0]
    recs, oks = [], []
    for b in range(B):
        out, ok = [PR.header(kind, header_v(kind, V))], True
        for (_, c, rows), slab in zip(fl, slabs):
            flat = np.asarray(slab[b]).reshape(rows, ctx.N)
            for r in range(rows):
                data, good = PR.pack_poly(flat[r].tolist(), cl[c])
                out.append(data)
                ok = ok and good
        recs.append(b"".join(out))
        oks.append(int(ok))
    size = record_bytes(ctx, kind, V)
    assert all(len(r) == size for r in recs)
    return np.frombuffer(b"".join(recs), dtype=np.uint8).reshape(B, size).copy(), np.array(oks, dtype=np.uint8)


def decode(ctx, kind, records, V=None):
    """records uint8 [B][record_bytes] -> (slabs [B][rows][N] per field, ok)."""
    cl, fl = PR.classes(ctx), fields(ctx, kind, V)
    B = records.shape[0]
    slabs = [np.zeros((B, rows, ctx.N), dtype=np.int64) for _, _, rows in fl]
    oks = []
    for b in range(B):
        raw = records[b].tobytes()
        ok = raw[:8] == PR.header(kind, header_v(kind, V))
        pos = 8
        for (_, c, rows), slab in zip(fl, slabs):
            nb = PR.poly_bytes(ctx.N, cl[c].W)
            for r in range(rows):
                coefs, good = PR.unpack_poly(raw[pos:pos + nb], ctx.N, cl[c])
                slab[b, r] = coefs
                ok = ok and good
                pos += nb
        assert pos == len(raw)
        oks.append(int(ok))
    return slabs, np.array(oks, dtype=np.uint8)
