"""The packed proof format "RZKP1" on the GPU (rzk_packed_{encode,decode}_batch[_dev], ring_zk_amd/packed.py and the
packed / short verifiers of ring_zk_amd/fiat_shamir.py) against tests/packed_ref.py, the big-integer restatement of the
format: records and ok bit for bit, host and device entry points, every kind, at the shapes where the lane arithmetic
can go wrong (one partial word, idle lanes, coefficients that straddle words, several 128-coefficient trips); grid-stride
trips; faults and rejections that stay with their own record; stores that stay inside their buffers; the argument rules;
and the stored proofs end to end, the short Open proof against the oracle's verifier with the reference transcript."""
import ctypes as C
import functools

import numpy as np
import pytest

import fs_ref
import packed_ref as PR
from oracle import oracle as O
from ring_zk_amd import fiat_shamir as FS
from ring_zk_amd import packed, synth, wire
from test_gpu_baseline_shapes import P_of, dev, make_ctx, torch_mod  # noqa: F401

pytestmark = pytest.mark.gpu

Q = O.Q_DEFAULT
AUX = bytes(range(50, 82))
SUM_KINDS = (packed.MSG_SUM_COMMITMENT, packed.MSG_SUM_RESPONSE)

# name -> (N, n, k, l, kappa): N = 4 is one partial word (56 padding bits in d, W_Z = 8); N = 64 leaves half of the lanes
# idle (W_Z = 15 and 18); N = 128 is one full trip; N = 1024 (W_Z = 22) and 2048 (23) straddle words over 8 / 16 trips
CONTEXTS = {
    "n4": (4, 1, 2, 1, 1),
    "n64k4": (64, 1, 3, 1, 4),
    "n64": (64, 1, 3, 1, 36),
    "n128": (128, 1, 3, 1, 36),
    "n1024": (1024, 1, 3, 1, 36),
    "n2048": (2048, 1, 3, 1, 36),
}
EXPECT_WZ = {"n4": 8, "n64k4": 15, "n64": 18, "n1024": 22, "n2048": 23}


@functools.lru_cache(maxsize=None)
def ctx_named(name, grid_cus=None):
    N, n, k, l, kappa = CONTEXTS[name]
    return make_ctx(N, n, k, l, env={"RZK_GRID_CUS": grid_cus} if grid_cus else None, kappa=kappa)


def ref_ctx(ctx):
    return PR.Ctx(ctx.N, ctx.n, ctx.k, ctx.l, ctx.q, ctx.verify_bound)


def kinds_and_v():
    for kind in packed.KINDS:
        for V in ((1, 3) if kind in SUM_KINDS else (None,)):
            yield kind, V


def rand_fields(rng, ctx, kind, V, B, extremes=True):
    """Random slabs inside every field's class range, with both ends of the range and zero planted."""
    cl = PR.classes(ref_ctx(ctx))
    out = []
    for (_, sh), (_, c, _) in zip(packed.field_shapes(ctx, kind, V), PR.fields(ref_ctx(ctx), kind, V)):
        lo, hi = -cl[c].bias, cl[c].limit - cl[c].bias
        a = rng.integers(lo, hi + 1, (B,) + sh, dtype=np.int64)
        if extremes:
            flat = a.reshape(B, -1, ctx.N)
            flat[0, 0, 0], flat[0, -1, -1], flat[-1, 0, ctx.N // 2], flat[-1, -1, 1] = lo, hi, 0, lo
            flat[B // 2, flat.shape[1] // 2, ctx.N - 2] = hi
        out.append(a)
    return out


def shapes_of(ctx, kind, V):
    return [sh for _, sh in packed.field_shapes(ctx, kind, V)]


def encode_both(torch, ctx, kind, slabs, V=None):
    """(records, ok) of the host entry point, after checking that the device entry point gives the same bytes."""
    rec, ok = packed.encode_batch(ctx, kind, *slabs, V=V)
    drec, dok = packed.encode_batch(ctx, kind, *[dev(torch, s) for s in slabs], V=V)
    assert np.array_equal(drec.cpu().numpy(), rec) and np.array_equal(dok.cpu().numpy(), ok)
    return rec, ok


def decode_both(torch, ctx, kind, records, V=None):
    """(slabs, ok) of the host entry point; the device entry point agrees on ok and on the slabs of accepted records."""
    *slabs, ok = packed.decode_batch(ctx, kind, records, V=V)
    *dslabs, dok = packed.decode_batch(ctx, kind, dev(torch, records), V=V)
    assert np.array_equal(dok.cpu().numpy(), ok)
    good = ok.astype(bool)
    for a, b in zip(slabs, dslabs):
        assert np.array_equal(b.cpu().numpy()[good], a[good])
    return slabs, ok


# ---- 1, 2: bit-exact against the reference; round trip ------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("name", list(CONTEXTS))
def test_records_match_reference_and_round_trip(torch_mod, name, B):
    ctx = ctx_named(name)
    wq, wz = packed.widths(ctx)
    cl = PR.classes(ref_ctx(ctx))
    assert (wq, wz) == (cl["Q"].W, cl["Z"].W) and wq == 32
    if name in EXPECT_WZ:
        assert wz == EXPECT_WZ[name]
    rng = np.random.default_rng(ctx.N * 10 + B + ctx.kappa)
    for kind, V in kinds_and_v():
        assert packed.record_bytes(ctx, kind, V) == PR.record_bytes(ref_ctx(ctx), kind, V)
        slabs = rand_fields(rng, ctx, kind, V, B)
        want, wok = PR.encode(ref_ctx(ctx), kind, slabs, V)
        rec, ok = encode_both(torch_mod, ctx, kind, slabs, V)
        assert wok.tolist() == [1] * B and np.array_equal(ok, wok), (kind, V)
        assert np.array_equal(rec, want), (kind, V)
        back, bok = decode_both(torch_mod, ctx, kind, rec, V)
        assert bok.tolist() == [1] * B, (kind, V)
        for a, b in zip(back, slabs):
            assert np.array_equal(a, b), (kind, V)


def test_pinned_sizes(torch_mod):
    ctx = ctx_named("n1024")
    sizes = [packed.record_bytes(ctx, k) for k in (packed.MSG_OPEN_COMMITMENT, packed.MSG_OPEN_RESPONSE, packed.MSG_OPEN_SHORT,
                                                  packed.MSG_CHALLENGE)]
    assert sizes == [12296, 8456, 16904, 264]
    assert wire.max_bytes(ctx, wire.MSG_OPEN_COMMITMENT) + wire.max_bytes(ctx, wire.MSG_OPEN_RESPONSE) == 49264


# ---- 3: grid-stride trips ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,V", [(packed.MSG_OPEN_SHORT, None), (packed.MSG_SUM_COMMITMENT, 3)])
def test_grid_stride_trips(torch_mod, kind, V):
    """B = 100 at N = 64 with every grid sized for one CU (32 wavefronts): 600 .. 1600 polynomials make many trips."""
    capped, free = ctx_named("n64", 1), ctx_named("n64")
    B = 100
    slabs = rand_fields(np.random.default_rng(100 + kind), free, kind, V, B)
    slabs[0][17].reshape(-1)[3] = (Q - 1) // 2 + 1   # one failed message, to see ok[] make the trips too
    rec, ok = encode_both(torch_mod, capped, kind, slabs, V)
    rec2, ok2 = encode_both(torch_mod, free, kind, slabs, V)
    want, wok = PR.encode(ref_ctx(free), kind, slabs, V)
    assert np.array_equal(rec, rec2) and np.array_equal(ok, ok2)
    assert np.array_equal(rec, want) and np.array_equal(ok, wok) and ok.sum() == B - 1
    back, bok = decode_both(torch_mod, capped, kind, rec, V)
    back2, bok2 = decode_both(torch_mod, free, kind, rec, V)
    assert np.array_equal(bok, ok) and np.array_equal(bok2, ok)
    good = ok.astype(bool)
    for a, b, c in zip(back, back2, slabs):
        assert np.array_equal(a[good], c[good]) and np.array_equal(b[good], c[good])


# ---- 4: faults stay local ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n64", "n1024"])
@pytest.mark.parametrize("trusted", [False, True])
def test_encode_faults_stay_local(torch_mod, name, trusted):
    """A response coefficient of verify_bound + 1 and a non-canonical commitment coefficient clear their own ok flags
    only; the other records are the reference's; the failed records do not decode.  The same in trusted-producer mode:
    the range test decides whether a value fits, so it is never skipped."""
    N, n, k, l, kappa = CONTEXTS[name]
    ctx = make_ctx(N, n, k, l, kappa=kappa)
    if trusted:
        ctx.trust_device_outputs(True)
    kind, B = packed.MSG_OPEN_SHORT, 5
    c, d, z = rand_fields(np.random.default_rng(N + 4), ctx, kind, None, B)
    z[1, k - 1, N - 1] = ctx.verify_bound + 1
    c[3, 0, N // 2 + 1] = (1 << 32) + 5          # never packed as 5
    want, wok = PR.encode(ref_ctx(ctx), kind, [c, d, z])
    rec, ok = encode_both(torch_mod, ctx, kind, [c, d, z])
    assert ok.tolist() == [1, 0, 1, 0, 1] and np.array_equal(ok, wok)
    assert np.array_equal(rec, want)              # the failed records too: the marker sits in the coefficient's place
    back, bok = decode_both(torch_mod, ctx, kind, rec)
    assert bok.tolist() == [1, 0, 1, 0, 1]
    for a, b in zip(back, (c, d, z)):
        assert np.array_equal(a[[0, 2, 4]], b[[0, 2, 4]])
    ctx.synchronize()   # a failed message is a verdict, not an input fault of the call


# ---- 5: decode rejections ------------------------------------------------------------------------------------------------
def set_coef(records, b, byte0, N, W, i, raw):
    nb = PR.poly_bytes(N, W)
    big = int.from_bytes(records[b, byte0:byte0 + nb].tobytes(), "little")
    big = (big & ~(((1 << W) - 1) << (i * W))) | (raw << (i * W))
    records[b, byte0:byte0 + nb] = np.frombuffer(big.to_bytes(nb, "little"), dtype=np.uint8)


@pytest.mark.parametrize("name", ["n4", "n1024"])
def test_decode_rejections(torch_mod, name):
    """limit + 1 in each class, a wrong magic / version / kind / V, and at N = 4 a padding bit: each rejects exactly its
    own record, and the reference agrees on every one."""
    ctx = ctx_named(name)
    rc = ref_ctx(ctx)
    cl = PR.classes(rc)
    kind, N = packed.MSG_OPEN_SHORT, ctx.N
    fl = PR.fields(rc, kind)
    base, _ = PR.encode(rc, kind, rand_fields(np.random.default_rng(N + 5), ctx, kind, None, 1))
    starts, pos = [], 8
    for _, c, rows in fl:
        starts.append(pos)
        pos += rows * PR.poly_bytes(N, cl[c].W)
    mods = []
    for f, (_, c, rows) in enumerate(fl):                      # limit + 1 in the last / first coefficient of a polynomial
        for r, i in ((rows - 1, N - 1), (0, 0), (0, N // 2 + 1)):
            m = base.copy()
            set_coef(m, 0, starts[f] + r * PR.poly_bytes(N, cl[c].W), N, cl[c].W, i, cl[c].limit + 1)
            mods.append(m)
    for byte, val in ((0, ord("S")), (3, ord("Q")), (4, 2), (5, packed.MSG_OPEN_COMMITMENT), (5, 10), (6, 1), (7, 1)):
        m = base.copy()
        m[0, byte] = val
        mods.append(m)
    if N == 4:
        for f, bit in ((1, 8), (1, 63), (2, 32), (2, 63)):     # d: bits 8 .. 63 are padding; z (W = 8): bits 32 .. 63
            m = base.copy()
            m[0, starts[f] + bit // 8] |= 1 << (bit % 8)
            mods.append(m)
    recs = np.concatenate([base] + mods + [base])
    _, ok = decode_both(torch_mod, ctx, kind, recs)
    _, rok = PR.decode(rc, kind, recs, shapes_of(ctx, kind, None))
    assert ok.tolist() == [1] + [0] * len(mods) + [1] and np.array_equal(ok, rok)


def test_kind_and_v_mismatch(torch_mod):
    """Records of one kind offered as another of the same size, and Sum records under another V in the header."""
    ctx = ctx_named("n64")
    rng = np.random.default_rng(77)
    z, zp = rand_fields(rng, ctx, packed.MSG_LINEAR_RESPONSE, None, 3)
    rec, ok = packed.encode_batch(ctx, packed.MSG_LINEAR_RESPONSE, z, zp)
    assert packed.record_bytes(ctx, packed.MSG_SUM_RESPONSE, 1) == rec.shape[1] and ok.all()
    *_, bad = decode_both(torch_mod, ctx, packed.MSG_SUM_RESPONSE, rec, V=1)
    assert bad.tolist() == [0, 0, 0]
    rec2, _ = packed.encode_batch(ctx, packed.MSG_SUM_RESPONSE, z, zp[:, None], V=1)
    rec2[1, 6] = 2                                            # V = 2 in the header of a record with one summand
    *_, ok2 = decode_both(torch_mod, ctx, packed.MSG_SUM_RESPONSE, rec2, V=1)
    assert ok2.tolist() == [1, 0, 1]


# ---- 6: bounds -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n4", "n64", "n1024"])
def test_stores_stay_inside_their_buffers(torch_mod, name):
    """Encode from slabs that end where their allocation ends into records between guard bytes; decode from a tensor of
    exactly B record_bytes into slabs between guard rows.  Every guard byte is unchanged afterwards.  (This checks the
    stores; that no load leaves a polynomial's own words is established by reading the kernels)"""
    torch = torch_mod
    ctx = ctx_named(name)
    ctx._bind_torch_stream()
    L, N, GUARD = ctx._L, ctx.N, 512
    for kind, V in ((packed.MSG_OPEN_SHORT, None), (packed.MSG_SUM_RESPONSE, 3), (packed.MSG_CHALLENGE, None)):
        B = 5
        slabs = rand_fields(np.random.default_rng(N + kind), ctx, kind, V, B)
        want, _ = PR.encode(ref_ctx(ctx), kind, slabs, V)
        size = want.shape[1]
        views = []
        for s in slabs:                                        # a view that ends at the end of its allocation
            buf = torch.full((64 + s.size,), 7, dtype=torch.int64, device="cuda")
            buf[64:] = dev(torch, s.reshape(-1))
            views.append(buf[64:])
        out = torch.full((GUARD + B * size + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        ok = torch.full((GUARD + B + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        fields = (C.c_void_p * len(views))(*[v.data_ptr() for v in views])
        assert L.rzk_packed_encode_batch_dev(ctx._h, kind, V or 0, fields, C.c_void_p(out.data_ptr() + GUARD),
                                             C.c_void_p(ok.data_ptr() + GUARD), B) == 0
        ctx.synchronize()
        o, k = out.cpu().numpy(), ok.cpu().numpy()
        assert (o[:GUARD] == 0xA5).all() and (o[-GUARD:] == 0xA5).all() and (k[:GUARD] == 0xA5).all() and (k[-GUARD:] == 0xA5).all()
        assert np.array_equal(o[GUARD:-GUARD].reshape(B, size), want) and k[GUARD:-GUARD].tolist() == [1] * B
        recs = dev(torch, want.reshape(-1))                    # exactly B * record_bytes
        assert recs.numel() == B * size
        outs = [torch.full((B + 2,) + tuple(s.shape[1:]), -99, dtype=torch.int64, device="cuda") for s in slabs]
        ok.fill_(0xA5)
        fields = (C.c_void_p * len(outs))(*[t[1:].data_ptr() for t in outs])
        assert L.rzk_packed_decode_batch_dev(ctx._h, kind, V or 0, C.c_void_p(recs.data_ptr()), fields,
                                             C.c_void_p(ok.data_ptr() + GUARD), B) == 0
        ctx.synchronize()
        k = ok.cpu().numpy()
        assert (k[:GUARD] == 0xA5).all() and (k[-GUARD:] == 0xA5).all() and k[GUARD:-GUARD].tolist() == [1] * B
        for t, s in zip(outs, slabs):
            t = t.cpu().numpy()
            assert (t[0] == -99).all() and (t[-1] == -99).all() and np.array_equal(t[1:-1], s)


# ---- 7: argument rules, B == 0, profiling names ---------------------------------------------------------------------------
def test_argument_rules_and_empty_batch(torch_mod):
    from ring_zk_amd import _lib

    ctx = ctx_named("n64")
    L, h = ctx._L, ctx._h
    z = np.zeros((2, 3, 64), np.int64)
    rec = np.zeros((2, packed.record_bytes(ctx, packed.MSG_OPEN_RESPONSE) // 8), np.uint64).view(np.uint8)
    ok = np.zeros(2, np.uint8)
    F = (C.c_void_p * 2)(z.ctypes.data, z.ctypes.data)
    p = lambda a: C.c_void_p(a.ctypes.data)
    enc, dec = L.rzk_packed_encode_batch, L.rzk_packed_decode_batch
    RESP = packed.MSG_OPEN_RESPONSE
    assert enc(h, RESP, 0, F, p(rec), p(ok), 2) == 0 and dec(h, RESP, 0, p(rec), F, p(ok), 2) == 0
    for kind in (packed.MSG_OPENING, 10, -1, 99):
        assert enc(h, kind, 1, F, p(rec), p(ok), 2) == _lib.RZK_E_ARG and dec(h, kind, 1, p(rec), F, p(ok), 2) == _lib.RZK_E_ARG
        assert L.rzk_packed_record_bytes(h, kind, 1) == 0
    for V in (0, 65536):
        assert enc(h, packed.MSG_SUM_RESPONSE, V, F, p(rec), p(ok), 2) == _lib.RZK_E_ARG
        assert dec(h, packed.MSG_SUM_RESPONSE, V, p(rec), F, p(ok), 2) == _lib.RZK_E_ARG
        assert L.rzk_packed_record_bytes(h, packed.MSG_SUM_COMMITMENT, V) == 0
    assert L.rzk_packed_record_bytes(h, packed.MSG_SUM_RESPONSE, 65535) == 8 + 65536 * 3 * PR.poly_bytes(64, 18)
    none = C.c_void_p(0)
    assert enc(h, RESP, 0, None, p(rec), p(ok), 2) == _lib.RZK_E_ARG
    assert enc(h, RESP, 0, (C.c_void_p * 1)(None), p(rec), p(ok), 2) == _lib.RZK_E_ARG
    assert enc(h, RESP, 0, F, none, p(ok), 2) == _lib.RZK_E_ARG and enc(h, RESP, 0, F, p(rec), none, 2) == _lib.RZK_E_ARG
    assert dec(h, RESP, 0, none, F, p(ok), 2) == _lib.RZK_E_ARG and dec(h, RESP, 0, p(rec), F, none, 2) == _lib.RZK_E_ARG
    mis = C.c_void_p(rec.ctypes.data + 4)
    assert enc(h, RESP, 0, F, mis, p(ok), 1) == _lib.RZK_E_ARG and dec(h, RESP, 0, mis, F, p(ok), 1) == _lib.RZK_E_ARG
    # the wire entry points keep rejecting the two kinds of the packed format
    for kind in (packed.MSG_LINEAR_RESPONSE, packed.MSG_OPEN_SHORT):
        assert L.rzk_wire_max_bytes(h, kind, 1, 8) == 0
    with pytest.raises(ValueError):
        packed.record_bytes(ctx, packed.MSG_OPENING)
    with pytest.raises(ValueError):
        packed.field_shapes(ctx, packed.MSG_OPENING)
    # B == 0: a successful no-op, host and device
    ok[:] = 9
    assert enc(h, RESP, 0, F, p(rec), p(ok), 0) == 0 and dec(h, RESP, 0, p(rec), F, p(ok), 0) == 0 and ok.tolist() == [9, 9]
    r0, k0 = packed.encode_batch(ctx, RESP, z[:0])
    assert r0.shape == (0, rec.shape[1]) and k0.shape == (0,)
    r0, k0 = packed.encode_batch(ctx, RESP, dev(torch_mod, z)[:0])
    assert tuple(r0.shape) == (0, rec.shape[1])
    zz, k0 = packed.decode_batch(ctx, RESP, r0)
    assert tuple(zz.shape) == (0, 3, 64) and tuple(k0.shape) == (0,)


def test_kernel_names_in_the_profiling_table(torch_mod):
    N, n, k, l, kappa = CONTEXTS["n64"]
    ctx = make_ctx(N, n, k, l, kappa=kappa)
    ctx.prof_enable(True)
    ctx.prof_reset()
    z = dev(torch_mod, rand_fields(np.random.default_rng(1), ctx, packed.MSG_OPEN_RESPONSE, None, 4)[0])
    rec, _ = packed.encode_batch(ctx, packed.MSG_OPEN_RESPONSE, z)
    packed.decode_batch(ctx, packed.MSG_OPEN_RESPONSE, rec)
    ctx.synchronize()
    nbytes = 4 * (packed.record_bytes(ctx, packed.MSG_OPEN_RESPONSE) + 3 * 64 * 8)
    assert ctx.prof_read_kernels() == [("packed_encode_kernel", nbytes), ("packed_decode_kernel", nbytes)]
    assert all(us > 0 for us in ctx.prof_read_all())


# ---- 8, 9: stored proofs end to end ---------------------------------------------------------------------------------------
def keyed_ctx(N, seed):
    ctx = make_ctx(N, 1, 3, 1, kappa=36)
    A = synth.key(np.random.default_rng(seed), N, 1, 3, 1)
    ctx.load_key(A)
    return ctx, A


def flip_bit(records, b, byte, bit=0):
    m = records.copy()
    m[b, byte] ^= 1 << bit
    return m


def field_byte_ranges(ctx, kind, V=None):
    """[(first byte, end byte)] of every field inside a record."""
    rc = ref_ctx(ctx)
    cl = PR.classes(rc)
    out, pos = [], 8
    for _, c, rows in PR.fields(rc, kind, V):
        nb = rows * PR.poly_bytes(ctx.N, cl[c].W)
        out.append((pos, pos + nb))
        pos += nb
    return out


def check_flips(verify, recs_c, recs_z, ranges_c, ranges_z, acc):
    """One flipped bit inside any field's bytes, of the commitment or the response record, rejects exactly that proof."""
    B = acc.shape[0]
    assert acc.tolist() == [1] * B
    for i, (lo, hi) in enumerate(ranges_c + ranges_z):
        victim = i % B
        byte = lo + ((hi - lo) * (i + 1)) // (len(ranges_c) + len(ranges_z) + 1)
        if i < len(ranges_c):
            got = verify(flip_bit(recs_c, victim, byte, i % 8), recs_z)
        else:
            got = verify(recs_c, flip_bit(recs_z, victim, byte, i % 8))
        assert got.tolist() == [int(b != victim) for b in range(B)], (i, byte)


@pytest.mark.parametrize("N", [64, 1024])
def test_stored_proofs_end_to_end(torch_mod, N):
    ctx, A = keyed_ctx(N, seed=31)
    P, B, V, k = P_of(ctx), 5, 2, 3
    rng = np.random.default_rng(N + 8)
    small, gauss = (lambda *lead: synth.small(rng, lead + (k, N), P.b)), (lambda *lead: synth.gauss(rng, lead + (k, N), P.sigma))
    # Open
    c, t, z, _ = FS.open_prove(ctx, synth.uniform(rng, (B, 1, N)), small(B), gauss(B), aux=AUX)
    rc_, ok1 = packed.encode_batch(ctx, packed.MSG_OPEN_COMMITMENT, c, t)
    rz_, ok2 = packed.encode_batch(ctx, packed.MSG_OPEN_RESPONSE, z)
    assert ok1.all() and ok2.all()
    acc = FS.open_verify(ctx, c, t, z, aux=AUX)
    assert np.array_equal(FS.open_verify_packed(ctx, rc_, rz_, aux=AUX), acc)
    assert np.array_equal(FS.open_verify_packed(ctx, dev(torch_mod, rc_), dev(torch_mod, rz_), aux=AUX).cpu().numpy(), acc)
    assert not FS.open_verify_packed(ctx, rc_, rz_, aux=None).any()
    check_flips(lambda a, b: FS.open_verify_packed(ctx, a, b, aux=AUX), rc_, rz_,
                field_byte_ranges(ctx, packed.MSG_OPEN_COMMITMENT), field_byte_ranges(ctx, packed.MSG_OPEN_RESPONSE), acc)
    # Linear
    g = synth.uniform(rng, (B, N))
    c, cp, t, tp, u, z, zp, _ = FS.linear_prove(ctx, g, synth.uniform(rng, (B, 1, N)), small(B), small(B), gauss(B), gauss(B), aux=AUX)
    rc_, ok1 = packed.encode_batch(ctx, packed.MSG_LINEAR_COMMITMENT, c, cp, g, t, tp, u)
    rz_, ok2 = packed.encode_batch(ctx, packed.MSG_LINEAR_RESPONSE, z, zp)
    assert ok1.all() and ok2.all()
    acc = FS.linear_verify(ctx, c, cp, g, t, tp, u, z, zp, aux=AUX)
    assert np.array_equal(FS.linear_verify_packed(ctx, rc_, rz_, aux=AUX), acc)
    check_flips(lambda a, b: FS.linear_verify_packed(ctx, a, b, aux=AUX), rc_, rz_,
                field_byte_ranges(ctx, packed.MSG_LINEAR_COMMITMENT), field_byte_ranges(ctx, packed.MSG_LINEAR_RESPONSE), acc)
    # Sum, V = 2
    gs, xs = synth.uniform(rng, (B, V, N)), synth.uniform(rng, (B, V, 1, N))
    cs, cp, ts, tp, u, zs, zp, _ = FS.sum_prove(ctx, gs, xs, small(B, V), small(B), gauss(B, V), gauss(B), aux=AUX)
    rc_, ok1 = packed.encode_batch(ctx, packed.MSG_SUM_COMMITMENT, cp, cs, gs, tp, ts, u, V=V)
    rz_, ok2 = packed.encode_batch(ctx, packed.MSG_SUM_RESPONSE, zp, zs, V=V)
    assert ok1.all() and ok2.all()
    acc = FS.sum_verify(ctx, cs, cp, gs, ts, tp, u, zs, zp, aux=AUX)
    assert np.array_equal(FS.sum_verify_packed(ctx, rc_, rz_, V, aux=AUX), acc)
    check_flips(lambda a, b: FS.sum_verify_packed(ctx, a, b, V, aux=AUX), rc_, rz_,
                field_byte_ranges(ctx, packed.MSG_SUM_COMMITMENT, V), field_byte_ranges(ctx, packed.MSG_SUM_RESPONSE, V), acc)


def oracle_short(ctx, P, A, c, d, z, aux):
    """The reference verdict of a short proof: t' from the oracle's Mat operations, d' from the hashlib transcript,
    the norm rule and the equation from the oracle's interactive verifier."""
    n = ctx.n
    kd = fs_ref.key_digest(A, ctx.q, ctx.N, ctx.n, ctx.k, ctx.l, ctx.kappa, ctx.b)
    out = []
    for b in range(c.shape[0]):
        t = O.mat_sub(O.mat_dot(A[:n], z[b][:, None, :]), O.mat_cmul(c[b][:n][:, None, :], d[b]))[:, 0, :]
        d2, _ = fs_ref.challenge(packed.MSG_OPEN_COMMITMENT, 0, kd, aux, [c[b:b + 1], t[None]], ctx.N, ctx.kappa)
        out.append(int(np.array_equal(d2[0], d[b]) and O.open_verify(P, A, z[b], t, c[b], d[b]) == 1))
    return np.array(out, dtype=np.uint8)


@pytest.mark.parametrize("N", [64, 1024])
def test_short_open_proofs(torch_mod, N):
    ctx, A = keyed_ctx(N, seed=41)
    P, B = P_of(ctx), 5
    rng = np.random.default_rng(N + 9)
    x, r, y = synth.uniform(rng, (B, 1, N)), synth.small(rng, (B, 3, N), P.b), synth.gauss(rng, (B, 3, N), P.sigma)
    c, t, z, _ = FS.open_prove(ctx, x, r, y, aux=AUX)
    d = FS.open_short(ctx, c, t, z, aux=AUX)
    acc = FS.open_verify_short(ctx, c, d, z, aux=AUX)
    assert acc.tolist() == [1] * B                                   # every honest proof
    assert np.array_equal(acc, oracle_short(ctx, P, A, c, d, z, AUX))
    assert np.array_equal(FS.open_verify_short(ctx, *[dev(torch_mod, a) for a in (c, d, z)], aux=AUX).cpu().numpy(), acc)

    def tamper(a, idx):
        m = a.copy()
        m[idx] = O.center(int(m[idx]) + 1)
        return m

    cases = [(tamper(c, (1, 0, 3)), d, z, 1), (tamper(c, (4, 1, N - 1)), d, z, 4), (c, tamper(d, (2, N // 2)), z, 2),
             (c, d, tamper(z, (0, 2, N - 1)), 0), (c, d, tamper(z, (3, 0, 0)), 3)]
    for cc, dd, zz, victim in cases:
        got = FS.open_verify_short(ctx, cc, dd, zz, aux=AUX)
        assert got.tolist() == [int(b != victim) for b in range(B)], victim
        assert np.array_equal(got, oracle_short(ctx, P, A, cc, dd, zz, AUX))
        rec, ok = packed.encode_batch(ctx, packed.MSG_OPEN_SHORT, cc, dd, zz)
        if ok.all():                                                  # d + 1 may leave class D: then the record itself fails
            assert np.array_equal(FS.open_verify_short_packed(ctx, rec, aux=AUX), got)
        else:
            assert ok.tolist() == got.tolist() and np.array_equal(FS.open_verify_short_packed(ctx, rec, aux=AUX), got)
    other = FS.open_verify_short(ctx, c, d, z, aux=None)
    assert not other.any() and np.array_equal(other, oracle_short(ctx, P, A, c, d, z, None))
    rec, ok = packed.encode_batch(ctx, packed.MSG_OPEN_SHORT, c, d, z)
    assert ok.all() and rec.shape[1] == packed.record_bytes(ctx, packed.MSG_OPEN_SHORT)
    assert np.array_equal(FS.open_verify_short_packed(ctx, rec, aux=AUX), acc)
    assert np.array_equal(FS.open_verify_short_packed(ctx, dev(torch_mod, rec), aux=AUX).cpu().numpy(), acc)
    assert not FS.open_verify_short_packed(ctx, rec, aux=bytes(32)).any()
    # a non-canonical coefficient from elsewhere rejects its own proof, it does not fail the call
    zz = z.copy()
    zz[2, 1, 5] += ctx.q
    assert FS.open_verify_short(ctx, c, d, zz, aux=AUX).tolist() == [1, 1, 0, 1, 1]
    lo, hi = field_byte_ranges(ctx, packed.MSG_OPEN_SHORT)[1]
    for b, byte in ((1, 8 + 5), (2, lo + 1), (3, hi + 7)):            # one bit in c, in d, in z
        got = FS.open_verify_short_packed(ctx, flip_bit(rec, b, byte, 3), aux=AUX)
        assert got.tolist() == [int(i != b) for i in range(B)]
