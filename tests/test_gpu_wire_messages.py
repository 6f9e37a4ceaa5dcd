"""Batched GPU codec of the reference's serialized protocol messages (rzk_wire_{decode,encode}_batch[_dev],
ring_zk_amd/wire.py) against the independent struct-based encoder of tests/test_wire_walk.py (the serde rules of
bincode with the reference's default options; nothing here is produced by the library under test):

  1. a known-answer OpenProofCommitment / OpenProofResponse at N = 16 (the reference's test ring, tests/test.rs:8),
     written out byte by byte for widths 8 and 4; the Mat-form t the project used before is rejected;
  2. round trips of every message kind at the BASELINE shapes, real proofs from the library's commit / response
     entry points, mixed trimmed lengths in one batch;
  3. verification from the wire equals the oracle's verdicts, tampered proofs and damaged messages reject exactly
     their own proofs;
  4. full batches (Open B = 4096 at N = 1024, a config-5 chunk) byte-equal to the test encoder, host and device
     entry points alike.
"""
import struct

import numpy as np
import pytest

from oracle import oracle as O
from ring_zk_amd import synth, wire
from test_gpu_baseline_shapes import P_of, _open_proof, dev, make_ctx, sum_inputs, torch_mod  # noqa: F401
from test_wire_walk import (CHALLENGE, COMMITMENT, LINEAR_COMMITMENT, OPEN_COMMITMENT, OPEN_RESPONSE, OPENING,
                            SUM_COMMITMENT, SUM_RESPONSE, enc_poly, encode_message, py_walk, random_fields)

pytestmark = pytest.mark.gpu

Q = O.Q_DEFAULT
HALF = (Q - 1) // 2


def ref_batch(ctx, kind, slabs, V=1, cb=8):
    """Test-encoder bytes of B messages from [B]-leading slabs (None = Option None)."""
    B = next(s for s in slabs if s is not None).shape[0]
    return [encode_message(kind, [None if s is None else s[b] for s in slabs], ctx.n, ctx.k, ctx.l, V, cb)
            for b in range(B)]


def check_round_trip(torch, ctx, kind, slabs, V=None, cb=8, device=True):
    """encode == test encoder, decode(test bytes) == slabs with ok = 1, on the host and (device=True) on the GPU."""
    want = ref_batch(ctx, kind, slabs, V or 1, cb)
    data, offsets = wire.encode_batch(ctx, kind, *slabs, V=V, coef_bytes=cb)
    assert wire.split(data, offsets) == want
    out = wire.decode_batch(ctx, kind, *wire.pack(want), V=V, coef_bytes=cb)
    assert out[-1].tolist() == [1] * len(want)
    for got, s in zip(out[:-1], slabs):
        if s is None:   # Option None decodes to the constant polynomial 1
            one = np.zeros_like(got)
            one[:, 0] = 1
            assert np.array_equal(got, one)
        else:
            assert np.array_equal(got, s)
    if device:
        D = [None if s is None else dev(torch, s) for s in slabs]
        dd, do = wire.encode_batch(ctx, kind, *D, V=V, coef_bytes=cb)
        assert wire.split(dd, do) == want
        pd, po = wire.pack(want)
        outd = wire.decode_batch(ctx, kind, dev(torch, pd), dev(torch, po.astype(np.int64)), V=V, coef_bytes=cb)
        for g, h in zip(outd, out):
            assert np.array_equal(g.cpu().numpy(), h)
    return want


# ---- 1. known answer at N = 16 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cb", [8, 4])
def test_kat_open_messages_n16(torch_mod, cb):
    ctx = make_ctx(16, 1, 3, 1, kappa=8)
    N = 16
    co = "<%d" + ("q" if cb == 8 else "i")
    Qd = lambda v: struct.pack("<Q", v)
    cf = lambda *v: struct.pack(co % len(v), *v)
    # OpenProofCommitment { c: Commitment { c: Mat 2x1 }, t: Vec<Polynomial> of 1 }  (open.rs:190-197, commit.rs:134)
    commitment = (Qd(2) + Qd(1) + Qd(3) + cf(1, -2, 3) + Qd(1) + Qd(0)
                  + Qd(1) + Qd(4) + cf(5, 0, 0, -7))
    # OpenProofResponse { z: Mat 3x1 } (open.rs:222-228)
    response = Qd(3) + Qd(1) + Qd(1) + cf(HALF) + Qd(1) + Qd(16) + cf(*range(-8, 8)) + Qd(1) + Qd(2) + cf(0, -HALF)
    c = np.zeros((1, 2, N), np.int64)
    c[0, 0, :3] = [1, -2, 3]
    t = np.zeros((1, 1, N), np.int64)
    t[0, 0, :4] = [5, 0, 0, -7]
    z = np.zeros((1, 3, N), np.int64)
    z[0, 0, 0] = HALF
    z[0, 1] = np.arange(-8, 8)
    z[0, 2, 1] = -HALF
    cg, tg, ok = wire.decode_batch(ctx, wire.MSG_OPEN_COMMITMENT, *wire.pack([commitment]), coef_bytes=cb)
    assert ok.tolist() == [1] and np.array_equal(cg, c) and np.array_equal(tg, t)
    zg, ok = wire.decode_batch(ctx, wire.MSG_OPEN_RESPONSE, *wire.pack([response]), coef_bytes=cb)
    assert ok.tolist() == [1] and np.array_equal(zg, z)
    assert wire.split(*wire.encode_batch(ctx, wire.MSG_OPEN_COMMITMENT, c, t, coef_bytes=cb)) == [commitment]
    assert wire.split(*wire.encode_batch(ctx, wire.MSG_OPEN_RESPONSE, z, coef_bytes=cb)) == [response]
    # the Mat-form t (a 1 x 1 Mat: 8 bytes more per row than Vec<Polynomial>) is not an OpenProofCommitment
    mat_form = wire.mat_encode(c[0][:, None, :], cb) + wire.mat_encode(t[0][:, None, :], cb)
    assert len(mat_form) == len(commitment) + 8
    assert wire.decode_batch(ctx, wire.MSG_OPEN_COMMITMENT, *wire.pack([mat_form]), coef_bytes=cb)[-1].tolist() == [0]
    assert wire.max_bytes(ctx, wire.MSG_OPEN_COMMITMENT, coef_bytes=cb) == 8 + 2 * 8 + 8 + 3 * (8 + 16 * cb)


# ---- 2. round trips of every kind at the BASELINE shapes ---------------------------------------------------------------
def _linear_proof(ctx, B, seed, short_g=True):
    P = P_of(ctx)
    rng = np.random.default_rng(seed)
    A = synth.key(rng, ctx.N, ctx.n, ctx.k, ctx.l)
    ctx.load_key(A)
    N, k, l = ctx.N, ctx.k, ctx.l
    g = synth.uniform(rng, (B, N))
    if short_g:
        g[0, 7:] = 0          # short g
        g[-1, 1:] = 0         # a constant
    x = synth.uniform(rng, (B, l, N))
    r, rp = synth.small(rng, (B, k, N), P.b), synth.small(rng, (B, k, N), P.b)
    y, yp = synth.gauss(rng, (B, k, N), P.sigma), synth.gauss(rng, (B, k, N), P.sigma)
    d = synth.challenge(rng, (B,), N, P.kappa)
    c, cp, t, tp, u, ok = ctx.linear_commit(g, x, r, rp, y, yp)
    z, zp = ctx.linear_response(y, yp, r, rp, d)
    return A, dict(g=g, x=x, r=r, rp=rp, d=d, c=c, cp=cp, t=t, tp=tp, u=u, z=z, zp=zp)


def _sum_proof(ctx, B, V, seed):
    P = P_of(ctx)
    rng = np.random.default_rng(seed)
    A = synth.key(rng, ctx.N, ctx.n, ctx.k, ctx.l)
    ctx.load_key(A)
    gs, xs, rs, rp, ys, yp, d = sum_inputs(rng, P, B, V)
    gs[0, 0, 3:] = 0          # short g_i
    gs[-1, V - 1] = 0         # a zero polynomial
    gs[-1, 0, 1:] = 0
    cs, cp, ts, tp, u, ok = ctx.sum_commit(gs, xs, rs, rp, ys, yp)
    zs, zp = ctx.sum_response(ys, yp, rs, rp, d)
    return A, dict(gs=gs, d=d, cs=cs, cp=cp, ts=ts, tp=tp, u=u, zs=zs, zp=zp)


@pytest.mark.parametrize("cb", [8, 4])
def test_round_trip_open_and_commitment_kinds(torch_mod, cb):
    ctx = make_ctx(1024, 1, 3, 1)
    B = 4
    A, x, r, y, d, c, t, z = _open_proof(ctx, B, 31)
    c[1, 1] = 0                               # a zero polynomial in a Mat
    c[2, 0, 100:] = 0                         # a short one
    check_round_trip(torch_mod, ctx, OPEN_COMMITMENT, [c, t], cb=cb)
    check_round_trip(torch_mod, ctx, OPEN_RESPONSE, [z], cb=cb)
    check_round_trip(torch_mod, ctx, CHALLENGE, [d], cb=cb)       # sparse: trimmed at the last +-1
    check_round_trip(torch_mod, ctx, COMMITMENT, [c], cb=cb)
    f = d.copy()
    f[0] = 0
    f[0, 0] = 1                               # Some(1)
    check_round_trip(torch_mod, ctx, OPENING, [x, r, f], cb=cb)
    check_round_trip(torch_mod, ctx, OPENING, [x, r, None], cb=cb)
    # random canonical fields with full / short / sparse / zero polynomials, every kind
    rng = np.random.default_rng(32 + cb)
    for kind, V in ((COMMITMENT, None), (OPENING, None), (CHALLENGE, None), (OPEN_COMMITMENT, None),
                    (OPEN_RESPONSE, None), (LINEAR_COMMITMENT, None), (SUM_COMMITMENT, 3), (SUM_RESPONSE, 3)):
        msgs = [random_fields(rng, kind, 1024, 1, 3, 1, V or 1, cb, lim=HALF) for _ in range(5)]
        slabs = [np.stack([m[i] for m in msgs]) for i in range(len(msgs[0]))]
        check_round_trip(torch_mod, ctx, kind, slabs, V=V, cb=cb, device=cb == 8)


def test_round_trip_linear(torch_mod):
    ctx = make_ctx(1024, 1, 3, 1)
    _, p = _linear_proof(ctx, 4, 41)
    for cb in (8, 4):
        check_round_trip(torch_mod, ctx, LINEAR_COMMITMENT, [p[k] for k in ("c", "cp", "g", "t", "tp", "u")], cb=cb)


@pytest.mark.parametrize("shape", [(1024, 4, 9, 4, 8), (2048, 8, 17, 8, 32)])
def test_round_trip_sum(torch_mod, shape):
    N, n, k, l, V = shape
    ctx = make_ctx(N, n, k, l)
    _, p = _sum_proof(ctx, 2, V, 51 + n)
    for cb in (8, 4):
        check_round_trip(torch_mod, ctx, SUM_COMMITMENT, [p[k] for k in ("cp", "cs", "gs", "tp", "ts", "u")], V=V,
                         cb=cb, device=cb == 8)
        check_round_trip(torch_mod, ctx, SUM_RESPONSE, [p["zp"], p["zs"]], V=V, cb=cb, device=cb == 8)


# ---- 3. verification from the wire ------------------------------------------------------------------------------------
def _damage(msgs, cb, coef_pos, count_pos):
    """Damaged copies of msgs[1..6] + a byte layout with a misaligned start; returns (data, offsets).
    [0] intact, [1] coefficient HALF+1, [2] k*2^32 + v (8-byte) / -(HALF+1) (4-byte), [3] truncated by one coefficient,
    [4] wrong Vec count, [5] trailing bytes, [6] starts at an unaligned offset, [7..] intact."""
    m = [bytearray(x) for x in msgs]
    p = coef_pos
    if cb == 8:
        m[1][p:p + 8] = struct.pack("<q", HALF + 1)
        v = struct.unpack_from("<q", m[2], p)[0]
        m[2][p:p + 8] = struct.pack("<q", v + 3 * 2 ** 32)
    else:
        m[1][p:p + 4] = struct.pack("<i", HALF + 1)
        m[2][p:p + 4] = struct.pack("<i", -(HALF + 1))
    del m[3][-cb:]
    v = struct.unpack_from("<Q", m[4], count_pos)[0]
    m[4][count_pos:count_pos + 8] = struct.pack("<Q", v + 1)
    parts, offs = [], [0]
    for b, x in enumerate(m):
        if b == 5:
            x = x + b"\0" * cb                    # trailing bytes, message end stays aligned
        if b == 6:
            parts.append(b"\0")                   # misaligned start ...
            offs[-1] += 1
            x = x + b"\0" * (cb - 1)              # ... and realigned for the messages after it
        parts.append(bytes(x))
        offs.append(offs[-1] + len(x))
    return np.frombuffer(b"".join(parts), np.uint8).copy(), np.array(offs, np.uint64)


def _first_coef_pos(msg, kind, ctx, V=1, cb=8):
    ok, ents = py_walk(msg, kind, ctx.N, ctx.n, ctx.k, ctx.l, V, cb)
    assert ok
    pos, ln = next(e for e in ents if 0 < e[1] < 0xFFFF)
    return pos


@pytest.mark.parametrize("cb", [8, 4])
def test_verify_open_from_wire_matches_oracle(torch_mod, cb):
    ctx = make_ctx(1024, 1, 3, 1)
    P = P_of(ctx)
    B = 9
    A, x, r, y, d, c, t, z = _open_proof(ctx, B, 61)
    zt = z.copy()
    zt[8, 2, 5] = O.center(int(zt[8, 2, 5]) + 1)              # proof 8 is tampered (decodes fine, does not verify)
    com = ref_batch(ctx, OPEN_COMMITMENT, [c, t], cb=cb)
    cha = ref_batch(ctx, CHALLENGE, [d], cb=cb)
    res = ref_batch(ctx, OPEN_RESPONSE, [zt], cb=cb)
    want = [int(O.open_verify(P, A, zt[b], t[b], c[b], d[b]) == 1) for b in range(B)]
    assert want == [1] * 8 + [0]
    assert wire.verify_open(ctx, com, cha, res, coef_bytes=cb).tolist() == want
    # damaged commitments reject exactly their own proofs; t is the Vec<Polynomial> field (count at 8 + 2*(8+8+len))
    count_pos = 8 + sum(16 + len(np.trim_zeros(c[0, i], "b")) * cb for i in range(2))
    bad = _damage(com, cb, _first_coef_pos(com[0], OPEN_COMMITMENT, ctx, cb=cb), count_pos)
    got = wire.verify_open(ctx, bad, cha, res, coef_bytes=cb)
    assert got.tolist() == [1, 0, 0, 0, 0, 0, 0, 1, 0]
    # device entry points: same verdicts
    D = lambda pair: (dev(torch_mod, pair[0]), dev(torch_mod, pair[1].astype(np.int64)))
    gotd = wire.verify_open(ctx, D(bad), D(wire.pack(cha)), D(wire.pack(res)), coef_bytes=cb)
    assert gotd.cpu().tolist() == got.tolist()


def test_verify_linear_from_wire_matches_oracle(torch_mod):
    ctx = make_ctx(1024, 1, 3, 1)
    P = P_of(ctx)
    B = 9
    A, p = _linear_proof(ctx, B, 71)
    zp = p["zp"].copy()
    zp[8, 0, 0] = O.center(int(zp[8, 0, 0]) - 1)
    com = ref_batch(ctx, LINEAR_COMMITMENT, [p[k] for k in ("c", "cp", "g", "t", "tp", "u")])
    cha = ref_batch(ctx, CHALLENGE, [p["d"]])
    want = [int(O.linear_verify(P, A, p["z"][b], zp[b], p["c"][b], p["cp"][b], p["g"][b], p["t"][b], p["tp"][b],
                                p["u"][b], p["d"][b]) == 1) for b in range(B)]
    assert want[8] == 0
    assert wire.verify_linear(ctx, com, cha, p["z"], zp).tolist() == want
    # damage: the t field (Vec<Polynomial> of n) follows c, cp, g
    m0 = com[0]
    n_l = ctx.n + ctx.l
    pos = 0
    for key in ("c", "cp"):
        pos += 8 + sum(16 + len(np.trim_zeros(p[key][0, i], "b")) * 8 for i in range(n_l))
    pos += 8 + len(np.trim_zeros(p["g"][0], "b")) * 8
    assert struct.unpack_from("<Q", m0, pos)[0] == ctx.n
    bad = _damage(com, 8, _first_coef_pos(m0, LINEAR_COMMITMENT, ctx), pos)
    assert wire.verify_linear(ctx, bad, cha, p["z"], zp).tolist() == [want[0], 0, 0, 0, 0, 0, 0, want[7], 0]


def test_verify_sum_from_wire_matches_oracle(torch_mod):
    N, n, k, l, V = 1024, 4, 9, 4, 8
    ctx = make_ctx(N, n, k, l)
    P = P_of(ctx)
    B = 3
    A, p = _sum_proof(ctx, B, V, 81)
    zs = p["zs"].copy()
    zs[2, V - 1, k - 1, 9] = O.center(int(zs[2, V - 1, k - 1, 9]) + 1)
    com = ref_batch(ctx, SUM_COMMITMENT, [p[k_] for k_ in ("cp", "cs", "gs", "tp", "ts", "u")], V=V)
    cha = ref_batch(ctx, CHALLENGE, [p["d"]])
    res = ref_batch(ctx, SUM_RESPONSE, [p["zp"], zs], V=V)
    want = [int(O.sum_verify(P, A, zs[b], p["zp"][b], p["cs"][b], p["cp"][b], p["gs"][b], p["ts"][b], p["tp"][b],
                             p["u"][b], p["d"][b]) == 1) for b in range(B)]
    assert want == [1, 1, 0]
    assert wire.verify_sum(ctx, V, com, cha, res).tolist() == want
    # a response whose Vec<Mat> has V - 1 entries is rejected (zs count sits right after zp)
    r0 = bytearray(res[0])
    pos = 8 + sum(16 + len(np.trim_zeros(p["zp"][0, i], "b")) * 8 for i in range(k))
    assert struct.unpack_from("<Q", r0, pos)[0] == V
    r0[pos:pos + 8] = struct.pack("<Q", V - 1)
    assert wire.verify_sum(ctx, V, com, cha, [bytes(r0)] + res[1:]).tolist() == [0, 1, 0]


def test_verify_commitment_from_wire_none_and_some(torch_mod):
    ctx = make_ctx(1024, 1, 3, 1)
    P = P_of(ctx)
    B = 4
    A, x, r, y, d, c, t, z = _open_proof(ctx, B, 91)
    xt = x.copy()
    xt[3, 0, 0] = O.center(int(xt[3, 0, 0]) + 1)               # opening 3 does not open c
    com = ref_batch(ctx, COMMITMENT, [c])
    # Some(f): f * c == a.r' + f * [0;x] holds for r' = f * r (commit.rs:200-209); a small f keeps r' short
    f = np.zeros((B, ctx.N), dtype=np.int64)
    f[:, 0] = 2
    f[:, 5] = -1
    rf = np.stack([O.mat_cmul(r[b][:, None, :], f[b])[:, 0, :] for b in range(B)])
    for fv, rv in ((None, r), (f, rf)):
        ope = ref_batch(ctx, OPENING, [xt, rv, fv])
        want = [int(bool(O.commitment_verify(P, A, c[b], xt[b], rv[b], None if fv is None else fv[b])))
                for b in range(B)]
        assert want == [1, 1, 1, 0]
        assert wire.verify_commitment(ctx, com, ope).tolist() == want
        bad = list(ope)                                          # opening 1 gets Option tag 2
        tag = len(bad[1]) - (0 if fv is None else len(enc_poly(fv[1], 8))) - 1
        assert bad[1][tag] == (0 if fv is None else 1)
        bad[1] = bad[1][:tag] + bytes([2]) + bad[1][tag + 1:]
        assert wire.verify_commitment(ctx, com, bad).tolist() == [1, 0, 1, 0]


# ---- 4. full batches -------------------------------------------------------------------------------------------------
def test_full_batch_open_b4096(torch_mod):
    ctx = make_ctx(1024, 1, 3, 1)
    B = 4096
    A, x, r, y, d, c, t, z = _open_proof(ctx, B, 101)
    for cb in (8, 4):
        for kind, slabs in ((OPEN_COMMITMENT, [c, t]), (OPEN_RESPONSE, [z]), (CHALLENGE, [d])):
            check_round_trip(torch_mod, ctx, kind, slabs, cb=cb)
    acc = wire.verify_open(ctx, ref_batch(ctx, OPEN_COMMITMENT, [c, t]), ref_batch(ctx, CHALLENGE, [d]),
                           ref_batch(ctx, OPEN_RESPONSE, [z]))
    assert acc.tolist() == [1] * B


def test_full_batch_config5_chunk(torch_mod):
    N, n, k, l, V = 2048, 8, 17, 8, 32
    ctx = make_ctx(N, n, k, l)
    B = 8
    A, p = _sum_proof(ctx, B, V, 111)
    T = torch_mod
    com = check_round_trip(T, ctx, SUM_COMMITMENT, [p[k_] for k_ in ("cp", "cs", "gs", "tp", "ts", "u")], V=V)
    res = check_round_trip(T, ctx, SUM_RESPONSE, [p["zp"], p["zs"]], V=V)
    cha = ref_batch(ctx, CHALLENGE, [p["d"]])
    D = lambda pair: (dev(T, pair[0]), dev(T, pair[1].astype(np.int64)))
    acc = wire.verify_sum(ctx, V, D(wire.pack(com)), D(wire.pack(cha)), D(wire.pack(res)))
    assert acc.cpu().tolist() == ctx.sum_verify(p["zs"], p["zp"], p["cs"], p["cp"], p["gs"], p["ts"], p["tp"], p["u"],
                                                p["d"]).tolist() == [1] * B
