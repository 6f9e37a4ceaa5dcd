"""The transcript hash, the packed codec and the short verifier's compare on 32-bit slabs (include/rzk.h "32-bit slabs:
messages"), on the GPU.

  * hash parity: challenge32(narrow(fields)) gives the digest and ok of challenge(fields) and narrow() of its d, and both
    equal tests/fs_ref.py, at every leaf shape (one short leaf, 2, 4, 8 leaves per polynomial), with dead lanes at the end of
    the last wavefront, for Open, Linear and Sum messages, with and without aux; two grid-stride trips under RZK_GRID_CUS=1.
  * hash verdict edges: the one unsigned compare of the 32-bit leaf kernel at the first and last coefficient of the first
    and last leaf of every field, for the four violations an int32 can hold; +-h stays valid; trusted mode; ok = NULL.
  * codec parity: records and ok of encode_batch32 are those of encode_batch; decode_batch32 is narrow(decode_batch);
    records cross between the widths; every kind, the lane shapes N = 4, 64, 128, 2048, several grid-stride trips.
  * codec edges: both ends of every class's range, the values next to them and the int32 extremes; decode rejections.
  * eq32, and the Open flows of fiat_shamir on int32 slabs against their 64-bit namesakes.
Every 32-bit *_dev call made by pointer here writes into device buffers with guard words on both sides of each output.
All equalities are exact."""
import ctypes as C

import numpy as np
import pytest

import fs_ref
from oracle import oracle as O
from ring_zk_amd import fiat_shamir as FS
from ring_zk_amd import packed, synth, wire
from ring_zk_amd.backend import RzkError
from test_gpu_baseline_shapes import P_of, dev, make_ctx, torch_mod  # noqa: F401
from test_gpu_slab32 import Guarded, kernel_names, n32, w64

pytestmark = pytest.mark.gpu

Q = O.Q_DEFAULT
HALF = (Q - 1) // 2
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
RANGE_FAULTS = [HALF + 1, -HALF - 1, I32_MAX, I32_MIN]
AUX = bytes(range(90, 122))
ALL_KINDS = tuple(packed.KINDS) + tuple(packed.SHORT_KINDS)
V_KINDS = (packed.MSG_SUM_COMMITMENT, packed.MSG_SUM_RESPONSE, packed.MSG_SUM_SHORT)


def keyed(N, env=None, seed=7, **kw):
    ctx = make_ctx(N, 1, 3, 1, env=env, **kw)
    A = synth.key(np.random.default_rng(seed), N, 1, 3, 1)
    ctx.load_key(A)
    return ctx, A


def key_digest_ref(ctx, A):
    return fs_ref.key_digest(A, ctx.q, ctx.N, ctx.n, ctx.k, ctx.l, ctx.kappa, ctx.b)


def ptr_table(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def run_dev(ctx, fn, *args):
    """One *_dev call with the profiler on: the kernel names it launched (an input fault surfaces in synchronize())."""
    ctx._bind_torch_stream()
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        ctx._check(getattr(ctx._L, fn)(ctx._h, *args))
        ctx.synchronize()
        return kernel_names(ctx)
    finally:
        ctx.prof_enable(False)


def challenge32_dev(T, ctx, kind, slabs, V=None, aux=None, with_ok=True):
    """rzk_fs_challenge32_batch_dev on guarded outputs: (d, digest, ok or None, kernel names)."""
    B = slabs[0].shape[0]
    ins = [dev(T, np.ascontiguousarray(s)) for s in slabs]
    assert all(t.dtype == T.int32 for t in ins)
    d, dig, ok = Guarded(T, (B, ctx.N), T.int32), Guarded(T, (B, 32), T.uint8), Guarded(T, (B,), T.uint8)
    names = run_dev(ctx, "rzk_fs_challenge32_batch_dev", kind, V or 0, ptr_table(ins), FS._aux(aux), C.c_void_p(d.ptr()),
                    C.c_void_p(dig.ptr()), C.c_void_p(ok.ptr()) if with_ok else None, B)
    okv = ok.take()
    if not with_ok:
        assert (okv == 0x5A).all(), "ok was NULL: nothing may be written"
    return d.take(), dig.take(), okv if with_ok else None, names


def encode32_dev(T, ctx, kind, slabs, V=None):
    B = slabs[0].shape[0]
    ins = [dev(T, np.ascontiguousarray(s)) for s in slabs]
    assert all(t.dtype == T.int32 for t in ins)
    rec, ok = Guarded(T, (B, packed.record_bytes(ctx, kind, V)), T.uint8), Guarded(T, (B,), T.uint8)
    names = run_dev(ctx, "rzk_packed_encode32_batch_dev", kind, V or 0, ptr_table(ins), C.c_void_p(rec.ptr()), C.c_void_p(ok.ptr()), B)
    return rec.take(), ok.take(), names


def decode32_dev(T, ctx, kind, records, V=None):
    B = records.shape[0]
    outs = [Guarded(T, (B,) + sh, T.int32) for _, sh in packed.field_shapes(ctx, kind, V)]
    ok = Guarded(T, (B,), T.uint8)
    rec = dev(T, np.ascontiguousarray(records))
    names = run_dev(ctx, "rzk_packed_decode32_batch_dev", kind, V or 0, C.c_void_p(rec.data_ptr()),
                    (C.c_void_p * len(outs))(*[o.ptr() for o in outs]), C.c_void_p(ok.ptr()), B)
    return [o.take() for o in outs], ok.take(), names


def field_classes(ctx, kind, V=None):
    """[(name, shape, bias, limit)] of the kind's fields: class Z for the responses, D for d, Q for everything else."""
    out = []
    for name, sh in packed.field_shapes(ctx, kind, V):
        if name in ("z", "zp", "zs"):
            bias = ctx.verify_bound
        elif name == "d":
            bias = 1
        else:
            bias = (ctx.q - 1) // 2
        out.append((name, sh, bias, 2 * bias))
    return out


def rand_fields(rng, ctx, kind, V, B):
    """Random int64 slabs inside every field's class range, both ends of the range planted at polynomial edges."""
    out = []
    for _, sh, bias, limit in field_classes(ctx, kind, V):
        a = rng.integers(-bias, limit - bias + 1, (B,) + sh, dtype=np.int64)
        flat = a.reshape(B, -1, ctx.N)
        flat[0, 0, 0], flat[0, -1, -1], flat[-1, 0, ctx.N // 2], flat[-1, -1, 1] = -bias, limit - bias, 0, -bias
        out.append(a)
    return out


def open_message(rng, ctx, B):
    """Canonical (c, t) of an Open commitment message with +-h where leaves and rate blocks meet."""
    N = ctx.N
    c, t = synth.uniform(rng, (B, ctx.n + ctx.l, N)), synth.uniform(rng, (B, ctx.n, N))
    for a in (c, t):
        for j, v in ((0, HALF), (N - 1, -HALF), (min(29, N - 1), -HALF), (min(30, N - 1), HALF), (N // 2, HALF)):
            a[0, 0, j] = v
            a[-1, -1, j] = -v
    return c, t


# ---- hash parity --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,B", [(64, 5), (512, 70), (1024, 5), (1024, 70), (2048, 5)])
def test_hash_parity_open(torch_mod, N, B):
    ctx, A = keyed(N)
    kd = key_digest_ref(ctx, A)
    leaves = B * (2 * ctx.n + ctx.l) * (N // fs_ref.leaf_len(N))
    assert leaves % 64 != 0, "the last wavefront has dead lanes"
    c, t = open_message(np.random.default_rng(71000 + N + B), ctx, B)
    for aux in (None, AUX):
        d64, dig64, ok64 = FS.challenge(ctx, wire.MSG_OPEN_COMMITMENT, c, t, aux=aux)
        dref, digref = fs_ref.challenge(fs_ref.OPEN_COMMITMENT, 0, kd, aux, [c, t], N, ctx.kappa)
        d32, dig32, ok32, names = challenge32_dev(torch_mod, ctx, wire.MSG_OPEN_COMMITMENT, [n32(c), n32(t)], aux=aux)
        assert names == ["fs_leaf_kernel<i32>", "fs_root_kernel<i32>"]
        assert ok32.tolist() == [1] * B == ok64.tolist()
        assert np.array_equal(dig32, dig64) and np.array_equal(dig32, digref)
        assert d32.dtype == np.int32 and np.array_equal(d32, n32(d64)) and np.array_equal(w64(d32), dref)
        # the Python layer: host arrays and device tensors
        dh, digh, okh = FS.challenge32(ctx, wire.MSG_OPEN_COMMITMENT, n32(c), n32(t), aux=aux)
        assert dh.dtype == np.int32 and np.array_equal(dh, d32) and np.array_equal(digh, dig32) and okh.all()
        dd, digd, okd = FS.challenge32(ctx, wire.MSG_OPEN_COMMITMENT, dev(torch_mod, n32(c)), dev(torch_mod, n32(t)), aux=aux)
        assert dd.dtype == torch_mod.int32 and np.array_equal(dd.cpu().numpy(), d32) and np.array_equal(digd.cpu().numpy(), dig32)
        assert bool(okd.all())
    ctx.prof_enable(True)
    ctx.prof_reset()
    FS.challenge(ctx, wire.MSG_OPEN_COMMITMENT, dev(torch_mod, c), dev(torch_mod, t))
    ctx.synchronize()
    assert kernel_names(ctx) == ["fs_leaf_kernel", "fs_root_kernel"], "the 64-bit names are unchanged"
    ctx.prof_enable(False)


@pytest.mark.parametrize("kind,V", [(wire.MSG_LINEAR_COMMITMENT, None), (wire.MSG_SUM_COMMITMENT, 2)], ids=["linear", "sum-v2"])
def test_hash_is_kind_generic(torch_mod, kind, V):
    N, B = 512, 3
    ctx, A = keyed(N)
    rng = np.random.default_rng(72000 + kind)
    fields = [synth.uniform(rng, (B,) + sh) for _, sh in wire.field_shapes(ctx, kind, V)]
    for aux in (None, AUX):
        d64, dig64, ok64 = FS.challenge(ctx, kind, *fields, V=V, aux=aux)
        dref, digref = fs_ref.challenge(kind, V or 0, key_digest_ref(ctx, A), aux, fields, N, ctx.kappa)
        d32, dig32, ok32, names = challenge32_dev(torch_mod, ctx, kind, [n32(f) for f in fields], V=V, aux=aux)
        assert names == ["fs_leaf_kernel<i32>", "fs_root_kernel<i32>"]
        assert ok32.all() and ok64.all() and np.array_equal(dig32, dig64) and np.array_equal(dig32, digref)
        assert np.array_equal(d32, n32(d64)) and np.array_equal(w64(d32), dref)


def test_hash_two_trips(torch_mod):
    """N = 1024, B = 100 with every grid sized for one CU: 12 leaves per proof, 1200 leaves against 16 workgroups of 64
    lanes per trip.  Two trips; the second is partly live and its last block partly dead."""
    N, B = 1024, 100
    ctx, A = keyed(N, env={"RZK_GRID_CUS": 1})
    free, _ = keyed(N)
    leaves, per_trip = B * 3 * (N // 256), 16 * 64
    assert leaves == 1200 and -(-leaves // per_trip) == 2 and (leaves - per_trip) % 64 != 0
    c, t = open_message(np.random.default_rng(73000), ctx, B)
    d64, dig64, ok64 = FS.challenge(free, wire.MSG_OPEN_COMMITMENT, c, t, aux=AUX)
    dref, digref = fs_ref.challenge(fs_ref.OPEN_COMMITMENT, 0, key_digest_ref(ctx, A), AUX, [c, t], N, ctx.kappa)
    d32, dig32, ok32, names = challenge32_dev(torch_mod, ctx, wire.MSG_OPEN_COMMITMENT, [n32(c), n32(t)], aux=AUX)
    assert names == ["fs_leaf_kernel<i32>", "fs_root_kernel<i32>"]
    assert ok32.tolist() == [1] * B and ok64.all()
    assert np.array_equal(dig32, dig64) and np.array_equal(dig32, digref)
    assert np.array_equal(d32, n32(d64)) and np.array_equal(w64(d32), dref)


# ---- hash verdict edges -------------------------------------------------------------------------------------------------------
def edge_places(ctx):
    """(field index, row, coefficient): first and last coefficient of the first and last leaf of c and of t."""
    N, L = ctx.N, fs_ref.leaf_len(ctx.N)
    out = []
    for f, rows in ((0, ctx.n + ctx.l), (1, ctx.n)):
        out += [(f, 0, 0), (f, 0, L - 1), (f, rows - 1, N - L), (f, rows - 1, N - 1)]
    return out


@pytest.mark.parametrize("N", [64, 1024])
def test_hash_verdict_edges(torch_mod, N):
    ctx, A = keyed(N)
    kd = key_digest_ref(ctx, A)
    places = edge_places(ctx)
    cases = [(pl, v) for pl in places for v in RANGE_FAULTS]
    B = len(cases) + 8
    c, t = open_message(np.random.default_rng(74000 + N), ctx, B)
    c32, t32 = n32(c), n32(t)
    for e, ((f, row, j), v) in enumerate(cases):
        (c32, t32)[f][e, row, j] = v
    want = [0] * len(cases) + [1] * 8
    d32, dig32, ok32, _ = challenge32_dev(torch_mod, ctx, wire.MSG_OPEN_COMMITMENT, [c32, t32], aux=AUX)
    d64, dig64, ok64 = FS.challenge(ctx, wire.MSG_OPEN_COMMITMENT, w64(c32), w64(t32), aux=AUX)
    assert ok32.tolist() == want, "each violation clears ok of its own proof only"
    assert np.array_equal(ok32, ok64)
    good = np.array(want, dtype=bool)
    dref, digref = fs_ref.challenge(fs_ref.OPEN_COMMITMENT, 0, kd, AUX, [c[good], t[good]], N, ctx.kappa)
    assert np.array_equal(dig32[good], digref) and np.array_equal(w64(d32[good]), dref)
    assert np.array_equal(dig32[good], dig64[good]) and np.array_equal(d32[good], n32(d64[good]))
    # +-h at the same places: still valid, and the digest is the reference's
    ce, te = c[:len(places) * 2].copy(), t[:len(places) * 2].copy()
    for e, (f, row, j) in enumerate(places):
        (ce, te)[f][2 * e, row, j] = HALF
        (ce, te)[f][2 * e + 1, row, j] = -HALF
    d32, dig32, ok32, _ = challenge32_dev(torch_mod, ctx, wire.MSG_OPEN_COMMITMENT, [n32(ce), n32(te)], aux=AUX)
    dref, digref = fs_ref.challenge(fs_ref.OPEN_COMMITMENT, 0, kd, AUX, [ce, te], N, ctx.kappa)
    assert ok32.all() and np.array_equal(dig32, digref) and np.array_equal(w64(d32), dref)
    # ok = NULL: the violation is an input fault of the call, as in the sibling
    for slabs in ([c32, t32],):
        with pytest.raises(RzkError) as ei:
            challenge32_dev(torch_mod, ctx, wire.MSG_OPEN_COMMITMENT, slabs, aux=AUX, with_ok=False)
        assert ei.value.status == -1
    ctx._bind_torch_stream()
    dd = torch_mod.empty((B, N), dtype=torch_mod.int64, device="cuda")
    ins = [dev(torch_mod, w64(c32)), dev(torch_mod, w64(t32))]
    ctx._check(ctx._L.rzk_fs_challenge_batch_dev(ctx._h, wire.MSG_OPEN_COMMITMENT, 0, ptr_table(ins), FS._aux(AUX),
                                                 C.c_void_p(dd.data_ptr()), None, None, B))
    with pytest.raises(RzkError):
        ctx.synchronize()
    d32, dig32, none, _ = challenge32_dev(torch_mod, ctx, wire.MSG_OPEN_COMMITMENT, [n32(ce), n32(te)], aux=AUX, with_ok=False)
    assert none is None and np.array_equal(dig32, digref)       # the sticky word was consumed: a clean call succeeds
    # trusted-producer mode: no test; what is hashed is the int32 itself
    ctx.trust_device_outputs(True)
    d32, dig32, ok32, _ = challenge32_dev(torch_mod, ctx, wire.MSG_OPEN_COMMITMENT, [c32, t32], aux=AUX)
    d64, dig64, ok64 = FS.challenge(ctx, wire.MSG_OPEN_COMMITMENT, w64(c32), w64(t32), aux=AUX)
    dref, digref = fs_ref.challenge(fs_ref.OPEN_COMMITMENT, 0, kd, AUX, [w64(c32), w64(t32)], N, ctx.kappa)
    assert ok32.all() and ok64.all() and np.array_equal(dig32, dig64) and np.array_equal(dig32, digref)
    assert np.array_equal(d32, n32(d64)) and np.array_equal(w64(d32), dref)


# ---- codec parity -------------------------------------------------------------------------------------------------------------
def check_codec_parity(torch, ctx, kind, V, B, rng):
    slabs = rand_fields(rng, ctx, kind, V, B)
    rec64, ok64 = packed.encode_batch(ctx, kind, *slabs, V=V)
    rec32, ok32, names = encode32_dev(torch, ctx, kind, [n32(s) for s in slabs], V)
    assert names == ["packed_encode_kernel<i32>"]
    assert ok64.tolist() == [1] * B and np.array_equal(ok32, ok64) and np.array_equal(rec32, rec64), (kind, V)
    back32, bok32, names = decode32_dev(torch, ctx, kind, rec64, V)          # a 64-bit record into 32-bit slabs
    assert names == ["packed_decode_kernel<i32>"]
    *back64, bok64 = packed.decode_batch(ctx, kind, rec32, V=V)              # a 32-bit record into 64-bit slabs
    assert bok32.tolist() == [1] * B == bok64.tolist()
    for a32, a64, s in zip(back32, back64, slabs):
        assert a32.dtype == np.int32 and np.array_equal(a32, n32(a64)) and np.array_equal(a64, s), (kind, V)
    return slabs, rec64


@pytest.mark.parametrize("N", [512, 1024])
def test_codec_parity_every_kind(torch_mod, N):
    ctx = make_ctx(N, 1, 3, 1)
    rng = np.random.default_rng(75000 + N)
    for kind in ALL_KINDS:
        check_codec_parity(torch_mod, ctx, kind, 2 if kind in V_KINDS else None, 5, rng)


@pytest.mark.parametrize("N,k,kappa", [(4, 2, 1), (64, 3, 36), (128, 3, 36), (2048, 3, 36)])
def test_codec_parity_lane_shapes(torch_mod, N, k, kappa):
    """MSG_OPEN_SHORT (all three classes) where the lane arithmetic changes: N = 4 has two active lanes, N = 64 one short
    trip, N = 128 exactly one full trip, N = 2048 sixteen."""
    ctx = make_ctx(N, 1, k, 1, kappa=kappa)
    slabs, rec = check_codec_parity(torch_mod, ctx, packed.MSG_OPEN_SHORT, None, 5, np.random.default_rng(76000 + N))
    # the Python layer, host and device
    r2, ok2 = packed.encode_batch32(ctx, packed.MSG_OPEN_SHORT, *[n32(s) for s in slabs])
    assert np.array_equal(r2, rec) and ok2.all()
    r3, ok3 = packed.encode_batch32(ctx, packed.MSG_OPEN_SHORT, *[dev(torch_mod, n32(s)) for s in slabs])
    assert np.array_equal(r3.cpu().numpy(), rec) and bool(ok3.all())
    *back, bok = packed.decode_batch32(ctx, packed.MSG_OPEN_SHORT, rec)
    *backd, bokd = packed.decode_batch32(ctx, packed.MSG_OPEN_SHORT, dev(torch_mod, rec))
    assert bok.all() and bool(bokd.all())
    for a, b, s in zip(back, backd, slabs):
        assert a.dtype == np.int32 and b.dtype == torch_mod.int32
        assert np.array_equal(a, n32(s)) and np.array_equal(b.cpu().numpy(), a)
    with pytest.raises(ValueError):
        packed.encode_batch32(ctx, packed.MSG_OPEN_SHORT, *slabs)           # int64 slabs: not coerced
    with pytest.raises(ValueError):
        packed.encode_batch(ctx, packed.MSG_OPEN_SHORT, *[dev(torch_mod, n32(s)) for s in slabs])


def test_codec_grid_stride_trips(torch_mod):
    """B = 100 MSG_OPEN_SHORT records at N = 1024 under RZK_GRID_CUS=1: 500 polynomials against 32 wavefronts per trip; one
    failed message, to see ok[] make the trips too."""
    N, B = 1024, 100
    ctx, free = make_ctx(N, 1, 3, 1, env={"RZK_GRID_CUS": 1}), make_ctx(N, 1, 3, 1)
    kind = packed.MSG_OPEN_SHORT
    assert B * 5 > 32 * 4
    slabs = rand_fields(np.random.default_rng(77000), ctx, kind, None, B)
    s32 = [n32(s) for s in slabs]
    s32[2][61, 1, 700] = ctx.verify_bound + 1
    rec64, ok64 = packed.encode_batch(free, kind, *[w64(s) for s in s32])
    rec32, ok32, _ = encode32_dev(torch_mod, ctx, kind, s32)
    assert np.array_equal(rec32, rec64) and np.array_equal(ok32, ok64) and int(ok32.sum()) == B - 1 and ok32[61] == 0
    back32, bok32, _ = decode32_dev(torch_mod, ctx, kind, rec64)
    *back64, bok64 = packed.decode_batch(free, kind, rec64)
    assert np.array_equal(bok32, bok64) and np.array_equal(bok32, ok64)
    good = bok32.astype(bool)
    for a32, a64, s in zip(back32, back64, s32):
        assert np.array_equal(a32[good], n32(a64[good])) and np.array_equal(a32[good], s[good])


# ---- codec edges --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [64, 1024])
def test_encode_edges(torch_mod, N):
    """Per class: limit - bias and -bias round-trip; limit - bias + 1, -bias - 1, INT32_MAX and INT32_MIN clear ok, at the
    first coefficient and at the last; the record carries the all-ones marker and never decodes as valid."""
    ctx = make_ctx(N, 1, 3, 1)
    kind = packed.MSG_OPEN_SHORT
    fc = field_classes(ctx, kind)
    cases = []
    for f, (_, _, bias, limit) in enumerate(fc):
        for j in (0, N - 1):
            cases += [(f, j, limit - bias, 1), (f, j, -bias, 1), (f, j, limit - bias + 1, 0), (f, j, -bias - 1, 0),
                      (f, j, I32_MAX, 0), (f, j, I32_MIN, 0)]
    B = len(cases)
    s32 = [n32(s) for s in rand_fields(np.random.default_rng(78000 + N), ctx, kind, None, B)]
    for e, (f, j, v, _) in enumerate(cases):
        flat = s32[f].reshape(B, -1, N)
        flat[e, 0 if j == 0 else -1, j] = v
    want = [w for *_, w in cases]
    rec32, ok32, _ = encode32_dev(torch_mod, ctx, kind, s32)
    rec64, ok64 = packed.encode_batch(ctx, kind, *[w64(s) for s in s32])
    assert ok32.tolist() == want and np.array_equal(ok32, ok64) and np.array_equal(rec32, rec64)
    # the marker sits in the coefficient's place: all W bits set
    starts, pos = [], 8
    for _, sh, bias, limit in fc:
        W = int(limit).bit_length()
        rows = int(np.prod(sh[:-1], dtype=np.int64)) if len(sh) > 1 else 1
        starts.append((pos, W, rows))
        pos += rows * 8 * ((N * W + 63) // 64)
    for e, (f, j, v, w) in enumerate(cases):
        if w:
            continue
        p0, W, rows = starts[f]
        nb = 8 * ((N * W + 63) // 64)
        p0 += 0 if j == 0 else (rows - 1) * nb
        big = int.from_bytes(rec32[e, p0:p0 + nb].tobytes(), "little")
        assert (big >> (j * W)) & ((1 << W) - 1) == (1 << W) - 1, (f, j, v)
    back32, bok32, _ = decode32_dev(torch_mod, ctx, kind, rec32)
    *back64, bok64 = packed.decode_batch(ctx, kind, rec32)
    assert bok32.tolist() == want and np.array_equal(bok32, bok64)
    good = bok32.astype(bool)
    for a32, a64, s in zip(back32, back64, s32):
        assert np.array_equal(a32[good], s[good]) and np.array_equal(a32[good], n32(a64[good]))
    ctx.synchronize()       # a failed message is a verdict, not an input fault of the call


def set_raw(records, b, byte0, nb, W, i, raw):
    big = int.from_bytes(records[b, byte0:byte0 + nb].tobytes(), "little")
    big = (big & ~(((1 << W) - 1) << (i * W))) | (raw << (i * W))
    records[b, byte0:byte0 + nb] = np.frombuffer(big.to_bytes(nb, "little"), dtype=np.uint8)


@pytest.mark.parametrize("N,k,kappa", [(4, 2, 1), (1024, 3, 36)])
def test_decode_rejections(torch_mod, N, k, kappa):
    """A flipped header byte, a raw value of limit + 1 in every class, and at N = 4 a set padding bit of d (class D: bits
    8 .. 63 of its word are padding): each rejects its own record only, as in the 64-bit decoder."""
    ctx = make_ctx(N, 1, k, 1, kappa=kappa)
    kind = packed.MSG_OPEN_SHORT
    fc = field_classes(ctx, kind)
    base, ok = packed.encode_batch(ctx, kind, *rand_fields(np.random.default_rng(79000 + N), ctx, kind, None, 1))
    assert ok.all()
    mods, pos = [], 8
    for byte in (0, 4, 5, 6):
        m = base.copy()
        m[0, byte] ^= 1
        mods.append(m)
    for _, sh, bias, limit in fc:
        W = int(limit).bit_length()
        rows = int(np.prod(sh[:-1], dtype=np.int64)) if len(sh) > 1 else 1
        nb = 8 * ((N * W + 63) // 64)
        for r, i in ((0, 0), (rows - 1, N - 1)):
            m = base.copy()
            set_raw(m, 0, pos + r * nb, nb, W, i, limit + 1)
            mods.append(m)
        if N == 4 and bias == 1:
            for bit in (8, 63):
                m = base.copy()
                m[0, pos + bit // 8] |= 1 << (bit % 8)
                mods.append(m)
        pos += rows * nb
    recs = np.concatenate([base] + mods + [base])
    _, ok32, _ = decode32_dev(torch_mod, ctx, kind, recs)
    *_, ok64 = packed.decode_batch(ctx, kind, recs)
    assert ok32.tolist() == [1] + [0] * len(mods) + [1] and np.array_equal(ok32, ok64)


# ---- eq32 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,rows", [(4, 1), (64, 3), (1024, 1), (1024, 2)])
def test_eq32(torch_mod, N, rows):
    T = torch_mod
    ctx = make_ctx(N, 1, 3 if N > 4 else 2, 1, kappa=36 if N > 4 else 1)
    B = 70
    rng = np.random.default_rng(80000 + N + rows)
    a = rng.integers(I32_MIN, I32_MAX + 1, (B, rows, N), dtype=np.int64).astype(np.int32)   # no range test: any int32
    b = a.copy()
    want = np.ones(B, dtype=np.uint8)
    for e, (r, j) in {3: (0, 0), 17: (rows - 1, N - 1), 64: (0, N // 2), 69: (rows - 1, N - 1)}.items():
        b[e, r, j] ^= np.int32(1 << (e % 31))
        want[e] = 0
    b[5, 0, 0], a[5, 0, 0] = I32_MIN, I32_MIN                                            # equal extremes stay equal
    eq = Guarded(T, (B,), T.uint8)
    da, db = dev(T, a), dev(T, b)
    names = run_dev(ctx, "rzk_eq32_batch_dev", C.c_void_p(da.data_ptr()), C.c_void_p(db.data_ptr()), rows, C.c_void_p(eq.ptr()), B)
    assert names == ["eq32_kernel"]
    assert np.array_equal(eq.take(), want)
    assert np.array_equal(ctx.eq32(a, b), want) and np.array_equal(ctx.eq32(da, db).cpu().numpy(), want)
    assert ctx.eq32(a, a).all()
    L, h = ctx._L, ctx._h
    assert L.rzk_eq32_batch_dev(h, None, None, rows, None, 0) == 0
    assert L.rzk_eq32_batch_dev(h, None, C.c_void_p(db.data_ptr()), rows, C.c_void_p(eq.ptr()), B) == -1
    assert L.rzk_eq32_batch_dev(h, C.c_void_p(da.data_ptr() + 8), C.c_void_p(db.data_ptr()), rows, C.c_void_p(eq.ptr()), B) == -1
    with pytest.raises(ValueError):
        ctx.eq32(w64(a), w64(b))


def test_argument_rules(torch_mod):
    T = torch_mod
    N, B = 512, 2
    ctx, _ = keyed(N)
    L, h = ctx._L, ctx._h
    buf = T.zeros(B * 3 * N + 16, dtype=T.int32, device="cuda")
    out = T.zeros(B * 20000, dtype=T.uint8, device="cuda")
    p, o = buf.data_ptr(), out.data_ptr()
    okp = C.c_void_p(o + B * 20000 - 64)           # behind the records
    kind = wire.MSG_OPEN_COMMITMENT
    assert B * packed.record_bytes(ctx, kind) <= B * 20000 - 64
    tab = lambda *ptrs: (C.c_void_p * len(ptrs))(*ptrs)
    assert L.rzk_fs_challenge32_batch_dev(h, kind, 0, None, None, None, None, None, 0) == 0
    assert L.rzk_fs_challenge32_batch_dev(h, kind, 0, tab(p, p), None, None, None, None, B) == -1          # d NULL
    assert L.rzk_fs_challenge32_batch_dev(h, kind, 0, tab(p, None), None, C.c_void_p(p), None, None, B) == -1
    assert L.rzk_fs_challenge32_batch_dev(h, kind, 0, tab(p + 8, p), None, C.c_void_p(p), None, None, B) == -1   # alignment
    assert L.rzk_fs_challenge32_batch_dev(h, wire.MSG_OPEN_RESPONSE, 0, tab(p), None, C.c_void_p(p), None, None, B) == -1
    for fn in (L.rzk_packed_encode32_batch_dev, L.rzk_packed_decode32_batch_dev):
        enc = fn is L.rzk_packed_encode32_batch_dev
        args = (lambda f, r, k: (tab(*f), r, k)) if enc else (lambda f, r, k: (r, tab(*f), k))
        assert fn(h, kind, 0, None, None, None, 0) == 0
        assert fn(h, kind, 0, *args((p, p), C.c_void_p(o), okp), B) == 0
        assert fn(h, kind, 0, *args((p, None), C.c_void_p(o), okp), B) == -1
        assert fn(h, kind, 0, *args((p, p + 8), C.c_void_p(o), okp), B) == -1                                    # alignment
        assert fn(h, kind, 0, *args((p, p), C.c_void_p(o + 4), okp), B) == -1                                    # records: 8 bytes
        assert fn(h, kind, 0, *args((p, p), C.c_void_p(o), None), B) == -1                                       # ok NULL
        assert fn(h, packed.MSG_OPENING, 0, *args((p, p), C.c_void_p(o), okp), B) == -1
    ctx.synchronize()
    c = np.zeros((B, 2, N), dtype=np.int32)
    t = np.zeros((B, 1, N), dtype=np.int32)
    with pytest.raises(ValueError):
        FS.challenge32(ctx, kind, w64(c), w64(t))                       # the 32-bit form does not coerce int64
    with pytest.raises(ValueError):
        FS.challenge(ctx, kind, dev(T, c), dev(T, t))                   # the 64-bit form keeps rejecting int32 tensors


# ---- the Open flows ---------------------------------------------------------------------------------------------------------
def bump(a, idx):
    m = a.copy()
    m[idx] += 1 if int(m[idx]) < HALF else -1
    return m


def flip(records, b, byte, bit):
    m = records.copy()
    m[b, byte] ^= 1 << bit
    return m


def byte_ranges(ctx, kind):
    out, pos = [], 8
    for _, sh, bias, limit in field_classes(ctx, kind):
        W = int(limit).bit_length()
        rows = int(np.prod(sh[:-1], dtype=np.int64)) if len(sh) > 1 else 1
        nb = rows * 8 * ((ctx.N * W + 63) // 64)
        out.append((pos, pos + nb))
        pos += nb
    return out


@pytest.mark.parametrize("N", [64, 512, 1024])
def test_open_flows(torch_mod, N):
    """open_prove32 = narrow(open_prove); the four 32-bit verifiers accept the honest batch and give the verdict vector of
    their 64-bit namesakes on the widened inputs for every tampering; records cross between the widths.  N = 64 runs the
    Open calls on the convert path, the hash, the codec and the compare natively."""
    T = torch_mod
    ctx, A = keyed(N)
    P, B = P_of(ctx), 5
    rng = np.random.default_rng(81000 + N)
    x, r, y = synth.uniform(rng, (B, 1, N)), synth.small(rng, (B, 3, N), P.b), synth.gauss(rng, (B, 3, N), P.sigma)
    c, t, z, ok = FS.open_prove(ctx, x, r, y, aux=AUX)
    c32, t32, z32, ok32 = FS.open_prove32(ctx, n32(x), n32(r), n32(y), aux=AUX)
    assert ok.all() and np.array_equal(ok32, ok)
    assert all(a.dtype == np.int32 for a in (c32, t32, z32))
    assert np.array_equal(c32, n32(c)) and np.array_equal(t32, n32(t)) and np.array_equal(z32, n32(z))
    dc, dt, dz, dok = FS.open_prove32(ctx, *[dev(T, n32(a)) for a in (x, r, y)], aux=AUX)      # device tensors: the same bytes
    assert dc.dtype == T.int32 and np.array_equal(dc.cpu().numpy(), c32) and np.array_equal(dt.cpu().numpy(), t32)
    assert np.array_equal(dz.cpu().numpy(), z32) and bool(dok.all())
    d = FS.open_short(ctx, c, t, z, aux=AUX)
    d32 = FS.open_short32(ctx, c32, t32, z32, aux=AUX)
    assert d32.dtype == np.int32 and np.array_equal(d32, n32(d))

    def same(v32, v64, honest=False):
        v32 = v32.cpu().numpy() if hasattr(v32, "cpu") else v32
        assert np.array_equal(v32, v64), (v32.tolist(), v64.tolist())
        if honest:
            assert v64.tolist() == [1] * B
        return v64

    # honest, host and device
    same(FS.open_verify32(ctx, c32, t32, z32, aux=AUX), FS.open_verify(ctx, c, t, z, aux=AUX), True)
    same(FS.open_verify32(ctx, dc, dt, dz, aux=AUX), FS.open_verify(ctx, c, t, z, aux=AUX), True)
    same(FS.open_verify_short32(ctx, c32, d32, z32, aux=AUX), FS.open_verify_short(ctx, c, d, z, aux=AUX), True)
    same(FS.open_verify_short32(ctx, dc, dev(T, d32), dz, aux=AUX), FS.open_verify_short(ctx, c, d, z, aux=AUX), True)
    # one tampered coefficient per field
    for victim, (cc, tt, zz) in enumerate([(bump(c32, (0, 0, 3)), t32, z32), (c32, bump(t32, (1, 0, N - 1)), z32),
                                           (c32, t32, bump(z32, (2, 2, N // 2)))]):
        got = same(FS.open_verify32(ctx, cc, tt, zz, aux=AUX), FS.open_verify(ctx, w64(cc), w64(tt), w64(zz), aux=AUX))
        assert got.tolist() == [int(b != victim) for b in range(B)]
    for victim, (cc, dd, zz) in enumerate([(bump(c32, (0, 1, N - 1)), d32, z32), (c32, bump(d32, (1, N // 2)), z32),
                                           (c32, d32, bump(z32, (2, 0, 0)))]):
        got = same(FS.open_verify_short32(ctx, cc, dd, zz, aux=AUX), FS.open_verify_short(ctx, w64(cc), w64(dd), w64(zz), aux=AUX))
        assert got.tolist() == [int(b != victim) for b in range(B)]
    # a wrong aux
    assert not same(FS.open_verify32(ctx, c32, t32, z32, aux=None), FS.open_verify(ctx, c, t, z, aux=None)).any()
    assert not same(FS.open_verify_short32(ctx, c32, d32, z32, aux=None), FS.open_verify_short(ctx, c, d, z, aux=None)).any()
    # a foreign d with -h - 1 in one coefficient: the recompute step's verdict rejects that proof, the call succeeds
    df = d32.copy()
    df[3, 7] = -HALF - 1
    got = same(FS.open_verify_short32(ctx, c32, df, z32, aux=AUX), FS.open_verify_short(ctx, c, w64(df), z, aux=AUX))
    assert got.tolist() == [1, 1, 1, 0, 1]
    got = same(FS.open_verify_short32(ctx, dc, dev(T, df), dz, aux=AUX), got)
    ctx.synchronize()
    # packed records, in both directions between the widths
    rc64, o1 = packed.encode_batch(ctx, packed.MSG_OPEN_COMMITMENT, c, t)
    rz64, o2 = packed.encode_batch(ctx, packed.MSG_OPEN_RESPONSE, z)
    rs64, o3 = packed.encode_batch(ctx, packed.MSG_OPEN_SHORT, c, d, z)
    rc32, p1 = packed.encode_batch32(ctx, packed.MSG_OPEN_COMMITMENT, c32, t32)
    rz32, p2 = packed.encode_batch32(ctx, packed.MSG_OPEN_RESPONSE, z32)
    rs32, p3 = packed.encode_batch32(ctx, packed.MSG_OPEN_SHORT, c32, d32, z32)
    assert all(o.all() for o in (o1, o2, o3, p1, p2, p3))
    assert np.array_equal(rc32, rc64) and np.array_equal(rz32, rz64) and np.array_equal(rs32, rs64)
    same(FS.open_verify_packed32(ctx, rc64, rz64, aux=AUX), FS.open_verify_packed(ctx, rc32, rz32, aux=AUX), True)
    same(FS.open_verify_short_packed32(ctx, rs64, aux=AUX), FS.open_verify_short_packed(ctx, rs32, aux=AUX), True)
    same(FS.open_verify_short_packed32(ctx, dev(T, rs64), aux=AUX), FS.open_verify_short_packed(ctx, rs32, aux=AUX), True)
    assert not same(FS.open_verify_short_packed32(ctx, rs64, aux=None), FS.open_verify_short_packed(ctx, rs64, aux=None)).any()
    # one flipped record bit per field
    for i, (lo, hi) in enumerate(byte_ranges(ctx, packed.MSG_OPEN_SHORT)):
        m = flip(rs64, i + 1, lo + (hi - lo) // 3, i % 8)
        got = same(FS.open_verify_short_packed32(ctx, m, aux=AUX), FS.open_verify_short_packed(ctx, m, aux=AUX))
        assert got.tolist() == [int(b != i + 1) for b in range(B)]
    for i, (lo, hi) in enumerate(byte_ranges(ctx, packed.MSG_OPEN_COMMITMENT)):
        m = flip(rc64, i, lo + (hi - lo) // 2, 5)
        got = same(FS.open_verify_packed32(ctx, m, rz64, aux=AUX), FS.open_verify_packed(ctx, m, rz64, aux=AUX))
        assert got.tolist() == [int(b != i) for b in range(B)]
    (lo, hi), = byte_ranges(ctx, packed.MSG_OPEN_RESPONSE)
    m = flip(rz64, 4, hi - 9, 2)
    got = same(FS.open_verify_packed32(ctx, rc64, m, aux=AUX), FS.open_verify_packed(ctx, rc64, m, aux=AUX))
    assert got.tolist() == [1, 1, 1, 1, 0]


@pytest.mark.parametrize("N", [512, 1024])
def test_device_resident_cycle_touches_no_int64_slab(torch_mod, N):
    """Operands -> packed short records -> verdicts on device tensors: every slab the caller holds or receives is int32,
    and no convert, canonicalize or 64-bit compare launch runs between record and verdict."""
    T = torch_mod
    ctx, A = keyed(N)
    P, B = P_of(ctx), 5
    rng = np.random.default_rng(82000 + N)
    x, r, y = (dev(T, n32(a)) for a in (synth.uniform(rng, (B, 1, N)), synth.small(rng, (B, 3, N), P.b),
                                         synth.gauss(rng, (B, 3, N), P.sigma)))
    ctx.prof_enable(True)
    ctx.prof_reset()
    c, t, z, ok = FS.open_prove32(ctx, x, r, y, aux=AUX)
    d = FS.open_short32(ctx, c, t, z, aux=AUX)
    records, eok = packed.encode_batch32(ctx, packed.MSG_OPEN_SHORT, c, d, z)
    ctx.synchronize()
    prove_names = kernel_names(ctx)
    ctx.prof_reset()
    acc = FS.open_verify_short_packed32(ctx, records, aux=AUX)
    ctx.synchronize()
    verify_names = kernel_names(ctx)
    ctx.prof_enable(False)
    assert all(a.dtype == T.int32 for a in (c, t, z, d)) and records.dtype == T.uint8
    assert bool(ok.all()) and bool(eok.all()) and acc.cpu().numpy().tolist() == [1] * B
    for names in (prove_names, verify_names):
        assert not any(nm in ("widen_kernel", "narrow_kernel") or nm.startswith(("canonicalize", "eq_kernel")) for nm in names), names
    assert verify_names[0] == "packed_decode_kernel<i32>" and verify_names[-3:] == ["fs_leaf_kernel<i32>", "fs_root_kernel<i32>", "eq32_kernel"]
    assert all(nm.endswith("i32>") or nm == "eq32_kernel" for nm in verify_names), verify_names
    assert "packed_encode_kernel<i32>" in prove_names
    # the oracle's interactive verifier accepts what the records hold
    cc, dd, zz = (w64(a.cpu().numpy()) for a in (c, d, z))
    tt = w64(t.cpu().numpy())
    for e in range(B):
        assert O.open_verify(P, A, zz[e], tt[e], cc[e], dd[e]) == 1
