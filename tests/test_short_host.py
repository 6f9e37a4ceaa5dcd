"""CPU tier of the short-proof record kinds (RZK_MSG_LINEAR_SHORT = 11, RZK_MSG_SUM_SHORT = 12): the schema
of ring_zk_amd/csrc/rzk_packed.h, compiled with g++ under -fsanitize=address,undefined into the stand-alone
tests/packed/packed_driver.cpp, against tests/short_ref.py (the two kinds restated over packed_ref's polynomial rules):
record sizes with the literals the format's description pins, encode and decode bit for bit, both ends of every class
and one past, every header byte, and a kind or V mismatch that rejects its own record."""
import struct

import numpy as np
import pytest

import packed_ref as PR
import short_ref as SR
from test_packed_host import Q, WIDTH_CASES, ctx_of, driver, head, run_driver, set_coef  # noqa: F401

SIZES = [4, 64, 128]


def v_of(kind, V):
    return V if kind == SR.SUM_SHORT else None


def drv_encode(exe, tmp_path, ctx, kind, slabs, V=None):
    B = slabs[0].shape[0]
    rec = head(2, ctx, kind, V) + struct.pack("<I", B) + b"".join(np.ascontiguousarray(s, np.int64).tobytes() for s in slabs)
    got = run_driver(exe, tmp_path, [rec])
    assert len(got) == B
    recs = np.frombuffer(bytes.fromhex("".join(g[1] for g in got)), dtype=np.uint8).reshape(B, SR.record_bytes(ctx, kind, V))
    return recs, np.array([int(g[0]) for g in got], dtype=np.uint8)


def drv_decode(exe, tmp_path, ctx, kind, records, V=None):
    B = records.shape[0]
    got = run_driver(exe, tmp_path, [head(3, ctx, kind, V) + struct.pack("<I", B) + records.tobytes()])
    assert len(got) == B
    slabs = [np.zeros((B, rows, ctx.N), np.int64) for _, _, rows in SR.fields(ctx, kind, V)]
    for b, g in enumerate(got):
        flat = np.frombuffer(bytes.fromhex(g[1]), dtype=np.int64)
        pos = 0
        for s in slabs:
            s[b] = flat[pos:pos + s[b].size].reshape(s[b].shape)
            pos += s[b].size
        assert pos == flat.size
    return slabs, np.array([int(g[0]) for g in got], dtype=np.uint8)


def random_fields(rng, ctx, kind, V, B):
    """Random in-range slabs with the extreme values of every class planted: -bias, limit - bias and 0."""
    cl = PR.classes(ctx)
    out = []
    for _, c, rows in SR.fields(ctx, kind, V):
        lo, hi = -cl[c].bias, cl[c].limit - cl[c].bias
        a = rng.integers(lo, hi + 1, (B, rows, ctx.N), dtype=np.int64)
        a[0, 0, 0], a[0, -1, -1], a[-1, 0, ctx.N // 2], a[-1, -1, 1] = lo, hi, 0, lo
        a[B // 2, rows // 2, ctx.N - 2] = hi
        out.append(a)
    return out


def test_field_lists_are_the_full_kinds_without_the_recomputed_fields():
    ctx = PR.make_ctx(64, 1, 3, 1, Q)
    assert [f[0] for f in SR.fields(ctx, SR.LINEAR_SHORT)] == ["c", "cp", "g", "d", "z", "zp"]
    assert [f[0] for f in SR.fields(ctx, SR.SUM_SHORT, 2)] == ["cp", "cs", "gs", "d", "zp", "zs"]
    assert [f[1] for f in SR.fields(ctx, SR.SUM_SHORT, 2)] == ["Q", "Q", "Q", "D", "Z", "Z"]


def test_literal_sizes(driver, tmp_path):
    """N = 1024, (1,3,1), verify_bound as the context computes it (W_Z = 22): 37 640 and 58 376 (V = 2) bytes, against
    49 680 and 74 512 for the full proofs."""
    ctx = PR.make_ctx(1024, 1, 3, 1, Q)
    assert PR.classes(ctx)["Z"].W == 22
    cases = [(SR.LINEAR_SHORT, 0, 37640), (SR.SUM_SHORT, 2, 58376)]
    got = run_driver(driver, tmp_path, [head(1, ctx, kind, V) for kind, V, _ in cases])
    assert [int(g[1]) for g in got] == [size for _, _, size in cases]
    assert [SR.record_bytes(ctx, kind, V or None) for kind, V, _ in cases] == [size for _, _, size in cases]
    full_lin = PR.record_bytes(ctx, PR.LINEAR_COMMITMENT) + PR.record_bytes(ctx, PR.LINEAR_RESPONSE)
    full_sum = PR.record_bytes(ctx, PR.SUM_COMMITMENT, 2) + PR.record_bytes(ctx, PR.SUM_RESPONSE, 2)
    assert (full_lin, full_sum) == (49680, 74512)


def test_record_sizes_and_bad_arguments(driver, tmp_path):
    cases = []
    for q, vb, wq, wz in WIDTH_CASES:
        for N in SIZES + [1024]:
            for nkl in ((1, 3, 1), (2, 5, 2)):
                ctx = ctx_of(N, q, vb, nkl)
                cases.append((ctx, SR.LINEAR_SHORT, 0, wq, wz))
                for V in (1, 3, 65535):
                    cases.append((ctx, SR.SUM_SHORT, V, wq, wz))
    got = run_driver(driver, tmp_path, [head(1, c, kind, V) for c, kind, V, _, _ in cases])
    for (ctx, kind, V, wq, wz), g in zip(cases, got):
        assert [int(v) for v in g] == [1, SR.record_bytes(ctx, kind, V or None), wq, wz, 2], (ctx, kind, V)
    ctx = ctx_of(64, Q, 100)
    bad = [(ctx, 10, 0), (ctx, 13, 0), (ctx, SR.SUM_SHORT, 0), (ctx, SR.SUM_SHORT, 65536),
           (ctx_of(64, Q - 1, 100), SR.LINEAR_SHORT, 0), (ctx_of(64, Q, 0), SR.SUM_SHORT, 1)]
    got = run_driver(driver, tmp_path, [head(1, c, kind, V) for c, kind, V in bad])
    assert [g[0] for g in got] == ["0"] * len(bad)
    # V is ignored by the kind without summands, as for the other such kinds: its header holds 0
    g = run_driver(driver, tmp_path, [head(1, ctx, SR.LINEAR_SHORT, 7)])[0]
    assert [int(g[0]), int(g[1])] == [1, SR.record_bytes(ctx, SR.LINEAR_SHORT)]


@pytest.mark.parametrize("q,vb,wq,wz", [WIDTH_CASES[0], WIDTH_CASES[1], WIDTH_CASES[4]])
@pytest.mark.parametrize("N", SIZES)
def test_both_kinds_against_reference(driver, tmp_path, N, q, vb, wq, wz):
    ctx = ctx_of(N, q, vb)
    rng = np.random.default_rng(N * 1000 + wz + wq + 16)
    for kind, V in ((SR.LINEAR_SHORT, None), (SR.SUM_SHORT, 1), (SR.SUM_SHORT, 3)):
        B = 3
        slabs = random_fields(rng, ctx, kind, V, B)
        want, wok = SR.encode(ctx, kind, slabs, V)
        assert wok.tolist() == [1] * B
        got, gok = drv_encode(driver, tmp_path, ctx, kind, slabs, V)
        assert gok.tolist() == [1] * B and np.array_equal(got, want), (kind, V)
        assert bytes(got[0, :8]) == b"RZKP" + bytes([1, kind]) + struct.pack("<H", V if kind == SR.SUM_SHORT else 0)
        back, bok = drv_decode(driver, tmp_path, ctx, kind, want, V)
        ref_back, rok = SR.decode(ctx, kind, want, V)
        assert bok.tolist() == [1] * B and rok.tolist() == [1] * B
        for a, b, c in zip(back, slabs, ref_back):
            assert np.array_equal(a, b) and np.array_equal(c, b), (kind, V)


@pytest.mark.parametrize("N", SIZES)
def test_one_past_the_range_writes_the_marker(driver, tmp_path, N):
    """bias + 1 on either side of every class, in every field: the all-ones marker in that coefficient's place, ok
    cleared for that message only, and the record does not decode."""
    ctx = ctx_of(N, Q, 100000)
    cl = PR.classes(ctx)
    rng = np.random.default_rng(N + 77)
    for kind, V in ((SR.LINEAR_SHORT, None), (SR.SUM_SHORT, 3)):
        fl = SR.fields(ctx, kind, V)
        B = 2 * len(fl) + 1
        slabs = random_fields(rng, ctx, kind, V, B)
        for f, (_, c, rows) in enumerate(fl):
            slabs[f][2 * f, rows - 1, N - 1] = cl[c].limit - cl[c].bias + 1
            slabs[f][2 * f + 1, 0, 0] = -cl[c].bias - 1
        want, wok = SR.encode(ctx, kind, slabs, V)
        assert wok.tolist() == [0] * (B - 1) + [1]
        got, gok = drv_encode(driver, tmp_path, ctx, kind, slabs, V)
        assert np.array_equal(gok, wok) and np.array_equal(got, want), kind
        _, dok = drv_decode(driver, tmp_path, ctx, kind, got, V)
        _, rok = SR.decode(ctx, kind, got, V)
        assert np.array_equal(dok, wok) and np.array_equal(rok, wok), kind
        # field 3 is d: its marker is the two bits 11 at the coefficient's own place
        lo, _ = SR.field_byte_ranges(ctx, kind, V)[3]
        big = int.from_bytes(got[6, lo:lo + PR.poly_bytes(N, 2)].tobytes(), "little")
        assert (big >> (2 * (N - 1))) & 3 == 3


@pytest.mark.parametrize("N", [4, 64])
def test_decode_rejections(driver, tmp_path, N):
    """limit + 1 and all-ones in every field, each header byte, a kind or V that belongs to another record, one padding
    bit: each rejects exactly its own record, and the restatement agrees."""
    ctx = ctx_of(N, Q, 100)   # W_Z = 8: N = 4 leaves 32 padding bits in a z polynomial, 56 in d
    cl = PR.classes(ctx)
    for kind, V in ((SR.LINEAR_SHORT, None), (SR.SUM_SHORT, 3)):
        fl = SR.fields(ctx, kind, V)
        base, _ = SR.encode(ctx, kind, random_fields(np.random.default_rng(N + kind), ctx, kind, V, 1), V)
        starts = [lo for lo, _ in SR.field_byte_ranges(ctx, kind, V)]
        mods = []
        for f, (_, c, rows) in enumerate(fl):
            for raw in (cl[c].limit + 1, (1 << cl[c].W) - 1):
                r = base.copy()
                set_coef(r, 0, starts[f] + (rows - 1) * PR.poly_bytes(N, cl[c].W), N, cl[c].W, N - 1, raw)
                mods.append(r)
        for byte in range(8):
            r = base.copy()
            r[0, byte] ^= 1
            mods.append(r)
        other = SR.SUM_SHORT if kind == SR.LINEAR_SHORT else SR.LINEAR_SHORT
        for byte, val in ((5, other), (5, 10), (5, PR.OPEN_SHORT), (6, (V or 0) + 1), (6, (V or 0) ^ 2), (7, 1)):
            r = base.copy()
            r[0, byte] = val
            mods.append(r)
        if N == 4:
            for f, bit in ((3, 8), (3, 63), (4, 32), (5, 63)):   # d: bits 8 .. 63 are padding; z (W = 8): bits 32 .. 63
                r = base.copy()
                r[0, starts[f] + bit // 8] |= 1 << (bit % 8)
                mods.append(r)
        recs = np.concatenate([base] + mods + [base])
        _, ok = drv_decode(driver, tmp_path, ctx, kind, recs, V)
        _, rok = SR.decode(ctx, kind, recs, V)
        assert ok.tolist() == [1] + [0] * len(mods) + [1] and np.array_equal(ok, rok), kind
