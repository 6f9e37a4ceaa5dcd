"""Fiat-Shamir challenges on the GPU (rzk_fs_challenge_batch[_dev], rzk_fs_key_digest, ring_zk_amd/fiat_shamir.py)
against tests/fs_ref.py, the hashlib restatement of the FS1 transcript: d, digest and ok bit for bit, host and device
entry points, at the shapes where the absorption can go wrong; sensitivity of the transcript to every field, to aux
and to the key; per-proof rejection of non-canonical coefficients; and the non-interactive proofs end to end against
the oracle's interactive verifier run with the reference transcript's challenge."""
import numpy as np
import pytest

import fs_ref
from oracle import oracle as O
from ring_zk_amd import fiat_shamir as FS
from ring_zk_amd import synth, wire
from test_gpu_baseline_shapes import P_of, dev, make_ctx, torch_mod  # noqa: F401

pytestmark = pytest.mark.gpu

Q = O.Q_DEFAULT
HALF = (Q - 1) // 2
OPEN, LINEAR, SUM = wire.MSG_OPEN_COMMITMENT, wire.MSG_LINEAR_COMMITMENT, wire.MSG_SUM_COMMITMENT
AUX = bytes(range(100, 132))


def rand_fields(rng, ctx, kind, V, B):
    """Canonical random slabs of B commitment messages (strictly inside the range, so that +-1 stays canonical)."""
    return [rng.integers(-HALF + 1, HALF, (B,) + sh, dtype=np.int64) for _, sh in wire.field_shapes(ctx, kind, V)]


def ref_challenge(ctx, A, kind, V, fields, aux=None):
    kd = fs_ref.key_digest(A, ctx.q, ctx.N, ctx.n, ctx.k, ctx.l, ctx.kappa, ctx.b)
    return fs_ref.challenge(kind, V if kind == SUM else 0, kd, aux, fields, ctx.N, ctx.kappa)


def keyed_ctx(N, n, k, l, kappa, seed, env=None):
    ctx = make_ctx(N, n, k, l, env=env, kappa=kappa)
    A = synth.key(np.random.default_rng(seed), N, n, k, l)
    ctx.load_key(A)
    return ctx, A


def both(torch, ctx, kind, fields, V=None, aux=None):
    """(d, digest, ok) from the host entry point, after checking that the device entry point gives the same bytes."""
    d, dig, ok = FS.challenge(ctx, kind, *fields, V=V, aux=aux)
    dd, ddig, dok = FS.challenge(ctx, kind, *[dev(torch, f) for f in fields], V=V, aux=aux)
    okn = dok.cpu().numpy()
    assert np.array_equal(okn, ok)
    good = ok.astype(bool)   # d and digest of a rejected proof are unspecified
    assert np.array_equal(dd.cpu().numpy()[good], d[good]) and np.array_equal(ddig.cpu().numpy()[good], dig[good])
    return d, dig, ok


# N = 4: a leaf shorter than one rate block; N = 64: leaf input 272 = 2 x 136 bytes, the padding in an extra block;
# N = 256: one full leaf; N = 512 (1,3,1) Open: root input 80 + 6 x 32 = 272 bytes, the same edge at the root;
# N = 2048: eight chunks.  kappa = N at N = 4, kappa = 64 at N = 64 (the squeeze crosses a block), kappa = 1, default 36.
SHAPES = [
    (4, (1, 3, 1), OPEN, None, 4),
    (64, (1, 3, 1), OPEN, None, 64),
    (256, (1, 3, 1), OPEN, None, 36),
    (512, (1, 3, 1), OPEN, None, 36),
    (1024, (1, 3, 1), OPEN, None, 36),
    (2048, (1, 3, 1), OPEN, None, 36),
    (16, (1, 3, 1), LINEAR, None, 8),
    (16, (2, 5, 2), SUM, 3, 1),
]


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("N,nkl,kind,V,kappa", SHAPES)
def test_challenge_matches_reference(torch_mod, N, nkl, kind, V, kappa, B):
    ctx, A = keyed_ctx(N, *nkl, kappa, seed=N + kind)
    assert FS.key_digest(ctx) == fs_ref.key_digest(A, Q, N, *nkl, kappa, ctx.b)
    rng = np.random.default_rng(1000 * N + 10 * kind + B)
    fields = rand_fields(rng, ctx, kind, V, B)
    fields[0][0, 0, 0], fields[-1][-1, -1, -1] = HALF, -HALF   # both ends of the range
    for aux in (None, AUX):
        d, dig, ok = both(torch_mod, ctx, kind, fields, V, aux)
        dr, digr = ref_challenge(ctx, A, kind, V, fields, aux)
        assert ok.tolist() == [1] * B
        assert np.array_equal(dig, digr)
        assert np.array_equal(d, dr)
        assert np.abs(d).sum(axis=1).tolist() == [kappa] * B


@pytest.mark.parametrize("kind,nkl,V", [(OPEN, (1, 3, 1), None), (LINEAR, (1, 3, 1), None), (SUM, (2, 5, 2), 3)])
def test_grid_stride_trips(torch_mod, kind, nkl, V):
    """B = 300 at N = 16 with every grid sized for one CU: the leaf kernel (Linear, Sum: more than 16 x 64 leaves) and
    the root kernel (more than 4 x 64 proofs) make several trips."""
    ctx, A = keyed_ctx(16, *nkl, 8, seed=3, env={"RZK_GRID_CUS": 1})
    B = 300
    fields = rand_fields(np.random.default_rng(300 + kind), ctx, kind, V, B)
    d, dig, ok = both(torch_mod, ctx, kind, fields, V, AUX)
    dr, digr = ref_challenge(ctx, A, kind, V, fields, AUX)
    assert ok.tolist() == [1] * B and np.array_equal(dig, digr) and np.array_equal(d, dr)


def test_key_digest_needs_a_key_and_bad_kinds(torch_mod):
    from ring_zk_amd import RzkError, _lib

    ctx = make_ctx(16, 1, 3, 1, kappa=8)
    with pytest.raises(RzkError) as e:
        FS.key_digest(ctx)
    assert e.value.status == _lib.RZK_E_STATE
    ctx.load_key(synth.key(np.random.default_rng(0), 16, 1, 3, 1))
    z = np.zeros((1, 3, 16), np.int64)
    with pytest.raises(ValueError):
        FS.challenge(ctx, wire.MSG_OPEN_RESPONSE, z)
    import ctypes as C

    fields = (C.c_void_p * 1)(z.ctypes.data)
    d = np.zeros((1, 16), np.int64)
    for kind in (wire.MSG_OPEN_RESPONSE, wire.MSG_COMMITMENT, wire.MSG_SUM_RESPONSE, 99):
        assert ctx._L.rzk_fs_challenge_batch(ctx._h, kind, 1, fields, None, C.c_void_p(d.ctypes.data), None, None,
                                             1) == _lib.RZK_E_ARG


@pytest.mark.parametrize("kind,nkl,V", [(OPEN, (1, 3, 1), None), (LINEAR, (1, 3, 1), None), (SUM, (2, 5, 2), 3)])
def test_sensitivity(torch_mod, kind, nkl, V):
    """Flipping the lowest bit of the first / last coefficient of the first / last polynomial of any field changes the
    digest and d of that proof only; aux and one key coefficient change every proof."""
    N, B, victim = 16, 3, 1
    ctx, A = keyed_ctx(N, *nkl, 8, seed=11)
    fields = rand_fields(np.random.default_rng(50 + kind), ctx, kind, V, B)
    d0, dig0, _ = both(torch_mod, ctx, kind, fields, V, AUX)
    for f in range(len(fields)):
        flat = fields[f].reshape(B, -1, N)
        for poly in {0, flat.shape[1] - 1}:
            for coef in (0, N - 1):
                mod = [a.copy() for a in fields]
                mod[f].reshape(B, -1, N)[victim, poly, coef] ^= 1
                d, dig, ok = both(torch_mod, ctx, kind, mod, V, AUX)
                dr, digr = ref_challenge(ctx, A, kind, V, mod, AUX)
                assert ok.tolist() == [1] * B and np.array_equal(dig, digr) and np.array_equal(d, dr)
                for b in range(B):
                    same = np.array_equal(dig[b], dig0[b]), np.array_equal(d[b], d0[b])
                    assert same == ((b != victim,) * 2), (f, poly, coef, b)
    aux2 = bytes([AUX[0] ^ 1]) + AUX[1:]
    d, dig, _ = both(torch_mod, ctx, kind, fields, V, aux2)
    assert all(not np.array_equal(dig[b], dig0[b]) and not np.array_equal(d[b], d0[b]) for b in range(B))
    A2 = A.copy()
    A2[-1, -1, -1] ^= 1
    ctx.load_key(A2)
    d, dig, _ = both(torch_mod, ctx, kind, fields, V, AUX)
    dr, digr = ref_challenge(ctx, A2, kind, V, fields, AUX)
    assert np.array_equal(dig, digr) and np.array_equal(d, dr)
    assert all(not np.array_equal(dig[b], dig0[b]) and not np.array_equal(d[b], d0[b]) for b in range(B))


@pytest.mark.parametrize("N", [16, 1024])
def test_non_canonical_coefficient_rejects_its_own_proof(torch_mod, N):
    """(q-1)/2 + 1 and 2^32 + s clear ok of their own proof only (never read as s); the other proofs are unaffected."""
    ctx, A = keyed_ctx(N, 1, 3, 1, min(N, 36), seed=5)
    B = 4
    fields = rand_fields(np.random.default_rng(N), ctx, OPEN, None, B)
    dr, digr = ref_challenge(ctx, A, OPEN, None, fields)
    for f, victim, where, bad in ((0, 2, (1, N - 1), HALF + 1), (1, 0, (0, 0), 2 ** 32 + 7), (0, 3, (0, N // 2), -HALF - 1),
                                  (1, 1, (0, N - 1), -(2 ** 32) + 3)):
        mod = [a.copy() for a in fields]
        mod[f][(victim,) + where] = bad
        d, dig, ok = both(torch_mod, ctx, OPEN, mod)
        assert ok.tolist() == [int(b != victim) for b in range(B)]
        keep = [b for b in range(B) if b != victim]
        assert np.array_equal(d[keep], dr[keep]) and np.array_equal(dig[keep], digr[keep])
    ctx.synchronize()   # a rejected proof is a verdict, not an input fault of the call


def test_non_canonical_coefficient_without_ok_is_an_input_fault(torch_mod):
    """With ok == NULL there is no verdict to clear: 2^32 + s is reported as an input fault of the call (host variant:
    RZK_E_ARG; device variant: the sticky word, at the next synchronize), never hashed as s without a signal."""
    import ctypes as C

    from ring_zk_amd import RzkError, _lib

    N, B = 16, 3
    ctx, _ = keyed_ctx(N, 1, 3, 1, 8, seed=6)
    good = rand_fields(np.random.default_rng(6), ctx, OPEN, None, B)
    bad = [a.copy() for a in good]
    bad[1][2, 0, N - 1] = 2 ** 32 + 7

    def call(fn, slabs, d):
        fields = (C.c_void_p * len(slabs))(*[wire._ptr(s).value for s in slabs])
        return fn(ctx._h, OPEN, 0, fields, None, wire._ptr(d), None, None, B)

    d = np.empty((B, N), np.int64)
    assert call(ctx._L.rzk_fs_challenge_batch, good, d) == _lib.RZK_OK
    assert call(ctx._L.rzk_fs_challenge_batch, bad, d) == _lib.RZK_E_ARG
    assert call(ctx._L.rzk_fs_challenge_batch, good, d) == _lib.RZK_OK   # the fault does not leak into the next call
    ctx._bind_torch_stream()
    dd = dev(torch_mod, d)
    assert call(ctx._L.rzk_fs_challenge_batch_dev, [dev(torch_mod, a) for a in good], dd) == _lib.RZK_OK
    ctx.synchronize()
    assert np.array_equal(dd.cpu().numpy(), d)
    assert call(ctx._L.rzk_fs_challenge_batch_dev, [dev(torch_mod, a) for a in bad], dd) == _lib.RZK_OK
    with pytest.raises(RzkError) as e:
        ctx.synchronize()
    assert e.value.status == _lib.RZK_E_ARG
    ctx.synchronize()   # reported once, then cleared


# ---- end to end ----------------------------------------------------------------------------------------------------------
def tamper(a, idx):
    t = a.copy()
    t[idx] = O.center(int(t[idx]) + 1)
    return t


def expect_single_reject(acc, base, victim):
    assert acc.tolist() == [int(v and b != victim) for b, v in enumerate(base.tolist())]


@pytest.mark.parametrize("N", [16, 512])
def test_open_end_to_end(torch_mod, N):
    ctx, A = keyed_ctx(N, 1, 3, 1, min(N, 36) if N > 16 else 8, seed=21)
    P, B = P_of(ctx), 4
    rng = np.random.default_rng(N + 1)
    x, r, y = synth.uniform(rng, (B, 1, N)), synth.small(rng, (B, 3, N), P.b), synth.gauss(rng, (B, 3, N), P.sigma)
    c, t, z, ok = FS.open_prove(ctx, x, r, y, aux=AUX)
    d, _ = ref_challenge(ctx, A, OPEN, None, [c, t], AUX)
    assert np.array_equal(z, ctx.open_response(y, r, d))

    def oracle(zz, tt, cc, aux=AUX):
        dd, _ = ref_challenge(ctx, A, OPEN, None, [cc, tt], aux)
        return np.array([O.open_verify(P, A, zz[b], tt[b], cc[b], dd[b]) == 1 for b in range(B)], dtype=np.uint8)

    acc = FS.open_verify(ctx, c, t, z, aux=AUX)
    assert np.array_equal(acc, oracle(z, t, c)) and acc.any()
    cases = [(tamper(z, (1, 2, N - 1)), t, c, 1), (z, tamper(t, (2, 0, 0)), c, 2), (z, t, tamper(c, (0, 1, 3)), 0)]
    for zz, tt, cc, victim in cases:
        got = FS.open_verify(ctx, cc, tt, zz, aux=AUX)
        assert np.array_equal(got, oracle(zz, tt, cc))
        expect_single_reject(got, acc, victim)
        msgs_c = wire.split(*wire.encode_batch(ctx, OPEN, cc, tt))
        msgs_z = wire.split(*wire.encode_batch(ctx, wire.MSG_OPEN_RESPONSE, zz))
        assert np.array_equal(FS.verify_open_wire(ctx, msgs_c, msgs_z, aux=AUX), got)
    other = FS.open_verify(ctx, c, t, z, aux=None)
    assert np.array_equal(other, oracle(z, t, c, None)) and not other.any()
    msgs_c = wire.split(*wire.encode_batch(ctx, OPEN, c, t))
    msgs_z = wire.split(*wire.encode_batch(ctx, wire.MSG_OPEN_RESPONSE, z))
    assert np.array_equal(FS.verify_open_wire(ctx, msgs_c, msgs_z, aux=AUX), acc)
    msgs_z[1] = msgs_z[1][:-8]   # a damaged response message rejects its own proof
    expect_single_reject(FS.verify_open_wire(ctx, msgs_c, msgs_z, aux=AUX), acc, 1)
    # device path: nothing leaves the GPU between commit, challenge and response
    D = lambda a: dev(torch_mod, a)
    cd, td, zd, okd = FS.open_prove(ctx, D(x), D(r), D(y), aux=AUX)
    for got, want in zip((cd, td, zd, okd), (c, t, z, ok)):
        assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(FS.open_verify(ctx, cd, td, zd, aux=AUX).cpu().numpy(), acc)


@pytest.mark.parametrize("N", [16, 512])
def test_linear_end_to_end(torch_mod, N):
    ctx, A = keyed_ctx(N, 1, 3, 1, min(N, 36) if N > 16 else 8, seed=22)
    P, B = P_of(ctx), 3
    rng = np.random.default_rng(N + 2)
    g, x = synth.uniform(rng, (B, N)), synth.uniform(rng, (B, 1, N))
    r, rp = synth.small(rng, (B, 3, N), P.b), synth.small(rng, (B, 3, N), P.b)
    y, yp = synth.gauss(rng, (B, 3, N), P.sigma), synth.gauss(rng, (B, 3, N), P.sigma)
    c, cp, t, tp, u, z, zp, ok = FS.linear_prove(ctx, g, x, r, rp, y, yp, aux=AUX)

    msg = dict(c=c, cp=cp, g=g, t=t, tp=tp, u=u)   # the commitment message, in the transcript's field order

    def oracle(m, zz, aux=AUX):
        dd, _ = ref_challenge(ctx, A, LINEAR, None, list(m.values()), aux)
        return np.array([O.linear_verify(P, A, zz[b], zp[b], m["c"][b], m["cp"][b], m["g"][b], m["t"][b], m["tp"][b],
                                         m["u"][b], dd[b]) == 1 for b in range(B)], dtype=np.uint8)

    def verify(m, zz, aux=AUX):
        return FS.linear_verify(ctx, m["c"], m["cp"], m["g"], m["t"], m["tp"], m["u"], zz, zp, aux=aux)

    acc = verify(msg, z)
    assert np.array_equal(acc, oracle(msg, z)) and acc.any()
    got = verify(msg, tamper(z, (0, 0, 0)))
    assert np.array_equal(got, oracle(msg, tamper(z, (0, 0, 0))))
    expect_single_reject(got, acc, 0)
    # every field that enters the transcript rejects exactly its own proof
    for name, idx in (("c", (1, 0, N - 1)), ("cp", (0, 1, 0)), ("g", (2, 5)), ("t", (1, 0, 2)), ("tp", (2, 0, N - 1)),
                      ("u", (0, 0, 0))):
        m = dict(msg, **{name: tamper(msg[name], idx)})
        got = verify(m, z)
        assert np.array_equal(got, oracle(m, z)), name
        expect_single_reject(got, acc, idx[0])
    other = verify(msg, z, aux=bytes(32))
    assert np.array_equal(other, oracle(msg, z, None)) and not other.any()
    D = lambda a: dev(torch_mod, a)
    outs = FS.linear_prove(ctx, D(g), D(x), D(r), D(rp), D(y), D(yp), aux=AUX)
    for got, want in zip(outs, (c, cp, t, tp, u, z, zp, ok)):
        assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("N,nkl,V", [(16, (2, 5, 2), 3), (512, (1, 3, 1), 4)])   # 512: BASELINE config 1
def test_sum_end_to_end(torch_mod, N, nkl, V):
    ctx, A = keyed_ctx(N, *nkl, min(N, 36) if N > 16 else 8, seed=23)
    P, B = P_of(ctx), 2
    n, k, l = nkl
    rng = np.random.default_rng(N + 3)
    gs, xs = synth.uniform(rng, (B, V, N)), synth.uniform(rng, (B, V, l, N))
    rs, rp = synth.small(rng, (B, V, k, N), P.b), synth.small(rng, (B, k, N), P.b)
    ys, yp = synth.gauss(rng, (B, V, k, N), P.sigma), synth.gauss(rng, (B, k, N), P.sigma)
    cs, cp, ts, tp, u, zs, zp, ok = FS.sum_prove(ctx, gs, xs, rs, rp, ys, yp, aux=AUX)

    msg = dict(cp=cp, cs=cs, gs=gs, tp=tp, ts=ts, u=u)   # the commitment message, in the transcript's field order

    def oracle(m, zz, aux=AUX):
        dd, _ = ref_challenge(ctx, A, SUM, V, list(m.values()), aux)
        return np.array([O.sum_verify(P, A, zz[b], zp[b], m["cs"][b], m["cp"][b], m["gs"][b], m["ts"][b], m["tp"][b],
                                      m["u"][b], dd[b]) == 1 for b in range(B)], dtype=np.uint8)

    def verify(m, zz, aux=AUX):
        return FS.sum_verify(ctx, m["cs"], m["cp"], m["gs"], m["ts"], m["tp"], m["u"], zz, zp, aux=aux)

    acc = verify(msg, zs)
    assert np.array_equal(acc, oracle(msg, zs)) and acc.any()
    zt = tamper(zs, (1, V - 1, k - 1, 7))
    got = verify(msg, zt)
    assert np.array_equal(got, oracle(msg, zt))
    expect_single_reject(got, acc, 1)
    # every field that enters the transcript rejects exactly its own proof
    for name, idx in (("cp", (1, 0, 0)), ("cs", (0, 0, 0, 0)), ("gs", (1, V - 1, N - 1)), ("tp", (0, n - 1, 1)),
                      ("ts", (1, V - 1, 0, N - 1)), ("u", (0, l - 1, 3))):
        m = dict(msg, **{name: tamper(msg[name], idx)})
        got = verify(m, zs)
        assert np.array_equal(got, oracle(m, zs)), name
        expect_single_reject(got, acc, idx[0])
    other = verify(msg, zs, aux=None)
    assert np.array_equal(other, oracle(msg, zs, None)) and not other.any()
    D = lambda a: dev(torch_mod, a)
    outs = FS.sum_prove(ctx, D(gs), D(xs), D(rs), D(rp), D(ys), D(yp), aux=AUX)
    for got, want in zip(outs, (cs, cp, ts, tp, u, zs, zp, ok)):
        assert np.array_equal(got.cpu().numpy(), want)
