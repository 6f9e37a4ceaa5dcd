"""What a context carries from one call to the next (GPU; DESIGN.md section 5, "Context walk").

Every other GPU file creates a context, loads one key, runs one batch size and drops the context.  Here a context lives as a
caller's does: keys are refused and replaced, batches grow past every arena and shrink again, Sum's V changes, and the
sticky input-fault word, trusted mode, the bound stream and the profiling slots change between calls.  What survives a
call — the plan cache, the key stores and digest, the grow-only arenas with the marks and per-call pointers inside them,
the first-use allocations — is only right if every step still equals its reference.

Oracle rule of every step: B <= 9 compares every entry bit for bit with the oracle (oracle/rzk_oracle.c) or the family's
Python reference, B > 9 the first entry, the last one and four seeded ones; the verdict vector is always exact.

  (a) a refused key (include/rzk.h, "key": RZK_E_ARG changes nothing): digest, the cached program and every program
      first planned after the refusal are the previous key's;
  (b) key replacement: regular -> dense -> a zero column that takes an identity entry with it -> only 0 / 1 entries ->
      regular;
  (c) workspace walk: batch sizes 2, 1, 9, 3, 40, 5, 1, 64 with V = 1, 3, 2, 5, 1, ... through every family, and Sum under a
      key whose a1 transforms nothing at every size;
  (d) three contexts of one shape alive at once under RZK_TW_LDS = 0, 1, 2.
"""
import time

import numpy as np
import pytest

import fs_ref
from oracle import oracle as O
from ring_zk_amd import _lib, RzkError, packed, synth, wire
from ring_zk_amd import fiat_shamir as FS
from ring_zk_amd.backend import KeyedSampler
from test_gpu_baseline_shapes import P_of, check_key_products_and_open, check_sum_cycle, dev, make_ctx, torch_mod  # noqa: F401
from test_gpu_random_shapes import check_linear_cycle
from test_gpu_slab32 import Slab32, assert_path, kernel_names, n32, w64

pytestmark = pytest.mark.gpu

Q = O.Q_DEFAULT
HALF = (Q - 1) // 2
E_ARG = _lib.RZK_E_ARG
OPEN = wire.MSG_OPEN_COMMITMENT
KEY = bytes(range(100, 132))
AUX = bytes(range(60, 92))


# ---- the oracle rule ------------------------------------------------------------------------------------------------------
def entries_of(B, seed):
    if B <= 9:
        return list(range(B))
    mid = np.random.default_rng(seed).choice(np.arange(1, B - 1), 4, replace=False)
    return sorted({0, B - 1} | {int(v) for v in mid})


# ---- steps that have no shared checker yet ------------------------------------------------------------------------------------
def check_digest(ctx, A):
    assert FS.key_digest(ctx) == fs_ref.key_digest(A, ctx.q, ctx.N, ctx.n, ctx.k, ctx.l, ctx.kappa, ctx.b)


def check_matvec_addend(ctx, A, B, seed, entries=None):
    """out = KEY(which) . v + addend for A1, A2 and A vs the oracle (commit.rs:125)."""
    rng = np.random.default_rng(seed)
    n, l, q = ctx.n, ctx.l, ctx.q
    v = synth.uniform(rng, (B, ctx.k, ctx.N), q)
    for which, sl in ((0, slice(0, n)), (1, slice(n, n + l)), (2, slice(0, n + l))):
        add = synth.uniform(rng, (B, sl.stop - sl.start, ctx.N), q)
        out = ctx.matvec(which, v, add)
        for b in range(B) if entries is None else entries:
            want = O.mat_add(O.mat_dot(A[sl], v[b][:, None, :], q), add[b][:, None, :], q)[:, 0, :]
            assert np.array_equal(out[b], want), ("matvec + addend", which, b)


def open_inputs(ctx, B, seed):
    P = P_of(ctx)
    rng = np.random.default_rng(seed)
    return (synth.uniform(rng, (B, ctx.l, ctx.N), ctx.q), synth.small(rng, (B, ctx.k, ctx.N), ctx.b),
            synth.gauss(rng, (B, ctx.k, ctx.N), P.sigma), synth.challenge(rng, (B,), ctx.N, P.kappa))


def open_reference(ctx, A, ins, entries):
    """{b: (c, t, ok, z)} of the oracle."""
    P = P_of(ctx)
    x, r, y, d = ins
    return {b: O.open_commit(P, A, x[b], r[b], y[b]) + (O.open_response(P, y[b], r[b], d[b]),) for b in entries}


def assert_open(ref, c, t, ok, z=None):
    for b, (c_ref, t_ref, ok_ref, z_ref) in ref.items():
        assert np.array_equal(c[b], c_ref) and np.array_equal(t[b], t_ref) and bool(ok[b]) == ok_ref, ("open commit", b)
        assert z is None or np.array_equal(z[b], z_ref), ("open response", b)


def check_open32(torch, ctx, A, B, seed, entries=None, native=None):
    """The 32-bit Open cycle on guarded device slabs vs the oracle; the last proof tampered.  native (True / False): every
    call ran on the 32-bit kernels / on the convert path, by the names of its launches."""
    entries = range(B) if entries is None else entries
    P = P_of(ctx)
    ins = open_inputs(ctx, B, seed)
    x, r, y, d = (n32(a) for a in ins)
    s = Slab32(torch, ctx)

    def path(outputs=True):
        if native is not None:
            assert_path(s.names, native, outputs=outputs)

    c, t, ok = s.commit(x, r, y)
    path()
    z = s.response(y, r, d)
    path()
    assert_open(open_reference(ctx, A, ins, entries), c, t, ok, z)
    for b in entries:
        assert O.open_verify(P, A, w64(z[b]), w64(t[b]), w64(c[b]), ins[3][b]) == 1
    zt = z.copy()
    zt[B - 1, ctx.k - 1, ctx.N - 1] += 1
    assert s.verify(z, t, c, d).tolist() == [1] * B
    path(outputs=False)
    assert s.verify(zt, t, c, d).tolist() == [1] * (B - 1) + [0]
    tr, accr = s.recover(z, c, d)
    path()
    assert accr.tolist() == [1] * B and all(np.array_equal(tr[b], t[b]) for b in entries)   # (t is the oracle's at `entries`)


def check_open_recover(ctx, A, B, seed, entries=None):
    """open_recover (64-bit): t = a1.z - c1 (.) d of an honest proof is the oracle's t, and every proof is accepted."""
    ins = open_inputs(ctx, B, seed)
    ref = open_reference(ctx, A, ins, range(B) if entries is None else entries)
    c, t, ok = ctx.open_commit(*ins[:3])
    z = ctx.open_response(ins[2], ins[1], ins[3])
    assert_open(ref, c, t, ok, z)
    tr, accr = ctx.open_recover(z, c, ins[3])
    assert accr.tolist() == [1] * B
    for b, (_, t_ref, _, _) in ref.items():
        assert np.array_equal(tr[b], t_ref), ("open recover", b)


def check_open_dev(torch, ctx, ins, ref, tamper=0):
    """The Open cycle through the device-pointer forms on torch's current stream; ref: open_reference of some entries."""
    B = ins[0].shape[0]
    x, r, y, d = (dev(torch, a) for a in ins)
    c, t, ok = ctx.open_commit(x, r, y)
    z = ctx.open_response(y, r, d)
    zt = z.clone()
    zt[tamper, 0, 0] += 1
    acc, acct = ctx.open_verify(z, t, c, d), ctx.open_verify(zt, t, c, d)
    ctx.synchronize()
    assert_open(ref, *(a.cpu().numpy() for a in (c, t, ok, z)))
    assert acc.cpu().numpy().tolist() == [1] * B
    assert acct.cpu().numpy().tolist() == [int(b != tamper) for b in range(B)]
    return c, t, z


def check_protocols(torch, ctx, A, B, V, seed, entries=None, recover=False, device_too=False):
    """Key products with and without an addend, the Open (with recover), Linear and Sum cycles and the 32-bit Open cycle
    under key A."""
    check_key_products_and_open(ctx, A, B, seed, entries=entries)
    check_open_recover(ctx, A, B, seed + 5, entries=entries)
    check_matvec_addend(ctx, A, B, seed + 1, entries=entries)
    check_linear_cycle(ctx, A, B, seed + 2, entries=entries, recover=recover, torch=torch if device_too else None)
    check_sum_cycle(torch, ctx, A, B, V, seed + 3, device_too=device_too, entries=entries, recover=recover)
    check_open32(torch, ctx, A, B, seed + 4, entries=entries)


# ---- (a) a refused key changes nothing ----------------------------------------------------------------------------------------
def other_key(rng, N, n, k, l):
    """Other values and another classification than synth.key: the first general entry of a1 is the constant 1, and the
    identity entry of a2's first row is general."""
    A = synth.key(rng, N, n, k, l)
    A[0, n] = 0
    A[0, n, 0] = 1
    A[n, n] = synth.uniform(rng, (N,))
    return A


REFUSALS = {   # where the coefficient outside the range sits: (row, column, coefficient, value)
    "last": lambda n, k, l, N: (n + l - 1, k - 1, N - 1, HALF + 1),
    "first": lambda n, k, l, N: (0, 0, 0, -(HALF + 1)),
}


def refuse(torch, ctx, A, where, via):
    bad = A.copy()
    row, col, j, value = REFUSALS[where](ctx.n, ctx.k, ctx.l, ctx.N)
    bad[row, col, j] = value
    with pytest.raises(RzkError) as e:
        ctx.load_key(dev(torch, bad) if via == "dev" else bad)
    assert e.value.status == E_ARG


@pytest.mark.parametrize("N,shape,where,via", [
    (512, (1, 3, 1), "last", "host"), (512, (1, 3, 1), "first", "host"), (512, (1, 3, 1), "last", "dev"), (512, (1, 3, 1), "first", "dev"),
    (64, (1, 3, 1), "last", "host"), (64, (1, 3, 1), "first", "host"),          # small rings: d_key_mont
    (1024, (2, 5, 2), "last", "host"), (1024, (2, 5, 2), "first", "host"),
])
def test_refused_key_changes_nothing(torch_mod, N, shape, where, via):
    n, k, l = shape
    B = 2
    ctx = make_ctx(N, n, k, l)
    K0 = synth.key(np.random.default_rng(7000 + N), N, n, k, l)
    K1 = other_key(np.random.default_rng(7100 + N), N, n, k, l)
    ctx.load_key(K0)
    ins = open_inputs(ctx, B, 7200 + N)
    ref0 = open_reference(ctx, K0, ins, range(B))
    assert_open(ref0, *ctx.open_commit(*ins[:3]))                      # one program is cached
    refuse(torch_mod, ctx, K1, where, via)
    check_digest(ctx, K0)
    assert_open(ref0, *ctx.open_commit(*ins[:3]))                      # the cached program, under K0
    check_protocols(torch_mod, ctx, K0, B, 2, 7300 + N)                # programs first planned after the refusal, under K0
    # every program is cached now; the other refusal
    refuse(torch_mod, ctx, K1, "first" if where == "last" else "last", "host")
    check_digest(ctx, K0)
    assert_open(ref0, *ctx.open_commit(*ins[:3]))
    check_key_products_and_open(ctx, K0, B, 7400 + N)
    # a valid load takes effect: other values, another classification
    ctx.load_key(dev(torch_mod, K1) if via == "dev" else K1)
    check_digest(ctx, K1)
    assert_open(open_reference(ctx, K1, ins, range(B)), *ctx.open_commit(*ins[:3]))
    check_protocols(torch_mod, ctx, K1, B, 2, 7500 + N)


# ---- (b) key replacement ------------------------------------------------------------------------------------------------------
def key_sequence(N, n, k, l, seed):
    rng = np.random.default_rng(seed)
    regular = synth.key(rng, N, n, k, l)
    dense = synth.uniform(rng, (n + l, k, N))
    dense[:, :, 1] = np.where(dense[:, :, 1] == 0, 1, dense[:, :, 1])   # no entry is the constant 0 or 1
    holes = synth.key(rng, N, n, k, l)
    assert k == n + l + 1 and holes[n + l - 1, k - 2, 0] == 1
    holes[:, k - 2, :] = 0                                            # a zero column, and with it a2's last row loses its identity entry
    bits = np.zeros((n + l, k, N), dtype=np.int64)
    bits[:, :, 0] = rng.integers(0, 2, (n + l, k))
    bits[0, 0, 0], bits[0, k - 1, 0], bits[n + l - 1, k - 1, 0] = 1, 1, 0
    keys = [("regular", regular), ("dense", dense), ("zero column", holes), ("only 0 / 1", bits),
            ("regular again", synth.key(rng, N, n, k, l))]
    for _, A in keys:   # the shared checkers tamper with columns 0 and k - 1 of a response: a1 must read both
        assert A[:n, 0].any() and A[:n, k - 1].any()
    return keys


def check_prover(torch, ctx, A, prev, B, seed):
    """open_prove_zk_native: every proof verifies in the oracle under A (challenge from the reference transcript, c opens
    to x with r), and not every one under the previous key."""
    P = P_of(ctx)
    x = ctx.sample_uniform(9, seed, ctx.half, (B, ctx.l))
    out = FS.open_prove_zk_native(ctx, x, KeyedSampler(ctx, KEY, seed), aux=AUX)
    ctx.synchronize()
    c, t, z, ok, r, rounds = (a.cpu().numpy() for a in out)
    x = x.cpu().numpy()
    assert ok.tolist() == [1] * B

    def verdicts(key):
        kd = fs_ref.key_digest(key, ctx.q, ctx.N, ctx.n, ctx.k, ctx.l, ctx.kappa, ctx.b)
        d, _ = fs_ref.challenge(OPEN, 0, kd, AUX, [c, t], ctx.N, ctx.kappa)
        return [int(O.open_verify(P, key, z[b], t[b], c[b], d[b]) == 1) for b in range(B)]

    assert verdicts(A) == [1] * B
    for b in range(B):
        c_ref, ok_ref = O.commit(P, A, x[b], r[b])
        assert ok_ref and np.array_equal(c[b], c_ref)
    if prev is not None:
        assert 0 in verdicts(prev)


@pytest.mark.parametrize("N,shape,env", [(64, (2, 5, 2), None), (512, (2, 5, 2), None),
                                         (1024, (2, 5, 2), {"RZK_DKEY": 2, "RZK_SUM_D": 1}),   # multiplier and operand images on
                                         (2048, (1, 3, 1), None)])
def test_key_replacement_walk(torch_mod, N, shape, env):
    n, k, l = shape
    B = 2
    ctx = make_ctx(N, n, k, l, env=env)
    prev = None
    for step, (name, A) in enumerate(key_sequence(N, n, k, l, 8000 + N)):
        ctx.load_key(dev(torch_mod, A) if step % 2 else A)
        classes = {("zero" if not p.any() else "one" if p[0] == 1 and not p[1:].any() else "general") for p in A.reshape(-1, N)}
        assert classes == {"regular": {"zero", "one", "general"}, "dense": {"general"}, "zero column": {"zero", "one", "general"},
                           "only 0 / 1": {"zero", "one"}, "regular again": {"zero", "one", "general"}}[name]
        check_digest(ctx, A)
        # every protocol runs under every key: from the second key on, a stale plan or image would be in the cache
        check_protocols(torch_mod, ctx, A, B, 2, 8100 + N + 10 * step, device_too=(step in (0, 3)))
        if N == 512:
            check_prover(torch_mod, ctx, A, prev, 8, 8200 + step)
        prev = A


# ---- (c) workspace walk ---------------------------------------------------------------------------------------------------------
SIZES = [2, 1, 9, 3, 40, 5, 1, 64]        # every new maximum exceeds 1.25 x the last: each arena is reallocated, then reused
SUM_V = [1, 3, 2, 5, 1]


def check_response_reject(torch, ctx, B, seed, entries):
    import reject_ref as RR
    from test_gpu_response_reject import LNM, R62, compare, fused_both

    P = RR.params_of(ctx)
    rng = np.random.default_rng(seed)
    y, r = synth.gauss(rng, (B, ctx.k, ctx.N), P.sigma), synth.small(rng, (B, ctx.k, ctx.N), ctx.b)
    d = synth.challenge(rng, (B,), ctx.N, ctx.kappa)
    coin = RR.coins(rng, B, R62)
    (z,), acc, E = fused_both(torch, ctx, "open", [y, r, d], coin, R62, LNM)
    sel = list(entries)
    Pz = P_of(ctx)
    for b in sel:
        assert np.array_equal(z[b], O.open_response(Pz, y[b], r[b], d[b])), b
    want = RR.run(P, [(z[sel], y[sel])], coin[sel], R62, LNM)
    compare(want, acc[sel], E[sel])


def check_fs_challenge(torch, ctx, A, B, seed, entries):
    from test_gpu_fiat_shamir import both, rand_fields, ref_challenge

    fields = rand_fields(np.random.default_rng(seed), ctx, OPEN, None, B)
    d, dig, ok = both(torch, ctx, OPEN, fields, None, AUX)
    sel = list(entries)
    dr, digr = ref_challenge(ctx, A, OPEN, None, [f[sel] for f in fields], AUX)
    assert ok.tolist() == [1] * B and np.array_equal(d[sel], dr) and np.array_equal(dig[sel], digr)


def check_packed(torch, ctx, B, V, seed, entries):
    import packed_ref as PR
    from test_gpu_packed import decode_both, encode_both, rand_fields, ref_ctx

    rng = np.random.default_rng(seed)
    sel = list(entries)
    for kind, v in ((packed.MSG_OPEN_SHORT, None), (packed.MSG_SUM_RESPONSE, V)):
        slabs = rand_fields(rng, ctx, kind, v, B, extremes=B >= 2)
        rec, ok = encode_both(torch, ctx, kind, slabs, v)
        want, wok = PR.encode(ref_ctx(ctx), kind, [s[sel] for s in slabs], v)
        assert ok.tolist() == [1] * B and wok.tolist() == [1] * len(sel) and np.array_equal(rec[sel], want), kind
        back, bok = decode_both(torch, ctx, kind, rec, v)
        assert bok.tolist() == [1] * B and all(np.array_equal(a, b) for a, b in zip(back, slabs)), kind


def check_wire(torch, ctx, B, seed, entries):
    """encode of the whole batch, its messages at `entries` against the struct-based test encoder; decode of the whole batch"""
    from test_gpu_wire_messages import ref_batch

    rng = np.random.default_rng(seed)
    slabs = [rng.integers(-HALF, HALF + 1, (B,) + sh, dtype=np.int64) for _, sh in wire.field_shapes(ctx, OPEN)]
    slabs[1][0, 0, 5:] = 0                                             # a trimmed polynomial: message lengths differ
    sel = list(entries)
    want = ref_batch(ctx, OPEN, [s[sel] for s in slabs])
    for D in (lambda a: a, lambda a: dev(torch, a)):
        data, offsets = wire.encode_batch(ctx, OPEN, *[D(s) for s in slabs])
        msgs = wire.split(data, offsets)
        assert [msgs[b] for b in sel] == want
    pd, po = wire.pack(msgs)
    out = wire.decode_batch(ctx, OPEN, pd, po)
    outd = wire.decode_batch(ctx, OPEN, dev(torch, pd), dev(torch, po.astype(np.int64)))
    assert out[-1].tolist() == [1] * B
    for got, gotd, s in zip(out[:-1], outd[:-1], slabs):
        assert np.array_equal(got, s) and np.array_equal(gotd.cpu().numpy(), s)


def check_xof(torch, ctx, B, rows, seed, entries):
    import xof_ref
    from test_gpu_xof import both, ref_uniform

    seeds = [xof_ref.seed_of(seed + i) for i in range(B)]
    out = both(torch, ctx, seeds, rows, 1)
    sel = list(entries)
    assert np.array_equal(out[sel], ref_uniform(ctx.N, 1, [seeds[b] for b in sel], rows))


class Walk:
    """One long-lived context and a valid Open and Sum proof of it, verified by the oracle once, for the interleaved checks."""

    def __init__(self, torch, ctx, A):
        self.torch, self.ctx, self.A = torch, ctx, A
        P = P_of(ctx)
        self.open_ins = open_inputs(ctx, 3, 9100)
        self.open_ref = open_reference(ctx, A, self.open_ins, range(3))
        self.c, self.t, ok = ctx.open_commit(*self.open_ins[:3])
        self.z = ctx.open_response(self.open_ins[2], self.open_ins[1], self.open_ins[3])
        assert_open(self.open_ref, self.c, self.t, ok, self.z)
        assert all(O.open_verify(P, A, self.z[b], self.t[b], self.c[b], self.open_ins[3][b]) == 1 for b in range(3))
        from test_gpu_baseline_shapes import sum_inputs

        gs, xs, rs, rp, ys, yp, d = sum_inputs(np.random.default_rng(9101), P, 2, 2)
        cs, cp, ts, tp, u, _ = ctx.sum_commit(gs, xs, rs, rp, ys, yp)
        zs, zp = ctx.sum_response(ys, yp, rs, rp, d)
        self.sum = (zs, zp, cs, cp, gs, ts, tp, u, d)
        assert all(O.sum_verify(P, A, zs[b], zp[b], cs[b], cp[b], gs[b], ts[b], tp[b], u[b], d[b]) == 1 for b in range(2))
        self.profile = None

    def open_verify(self):
        d = self.open_ins[3]
        assert self.ctx.open_verify(self.z, self.t, self.c, d).tolist() == [1, 1, 1]

    # -- the interleaved events ---------------------------------------------------------------------------------------------
    def prover_fault(self, step):
        """One c -+ q input: the call fails once, through the host form or (odd steps) as the sticky word of the device form;
        the next call is clean and its outputs are the oracle's."""
        ctx, T = self.ctx, self.torch
        x, r, y, d = (a.copy() for a in self.open_ins)
        x[1, 0, ctx.N - 1] += -Q if x[1, 0, ctx.N - 1] > 0 else Q
        if step % 2:
            ctx.open_commit(dev(T, x), dev(T, r), dev(T, y))
            with pytest.raises(RzkError) as e:
                ctx.synchronize()
        else:
            with pytest.raises(RzkError) as e:
                ctx.open_commit(x, r, y)
        assert e.value.status == E_ARG
        ctx.synchronize()                                              # reported once
        c, t, ok = ctx.open_commit(*self.open_ins[:3])
        assert_open(self.open_ref, c, t, ok)

    def sum_fault(self):
        """A non-canonical g_i rejects its own proof; the following Open verify is unaffected."""
        zs, zp, cs, cp, gs, ts, tp, u, d = self.sum
        bad = gs.copy()
        bad[1, 1, 3] += -Q if bad[1, 1, 3] > 0 else Q
        assert self.ctx.sum_verify(zs, zp, cs, cp, bad, ts, tp, u, d).tolist() == [1, 0]
        self.open_verify()
        assert self.ctx.sum_verify(*self.sum).tolist() == [1, 1]

    def trusted(self):
        """Trusted mode on: identical bytes; off again: s + 2^32 is rejected again."""
        ctx = self.ctx
        zb = self.z.copy()
        zb[2, 0, 7] += 1 << 32
        d = self.open_ins[3]
        ctx.trust_device_outputs(True)
        try:
            c, t, ok = ctx.open_commit(*self.open_ins[:3])
            z = ctx.open_response(self.open_ins[2], self.open_ins[1], d)
            assert_open(self.open_ref, c, t, ok, z)
            self.open_verify()
        finally:
            ctx.trust_device_outputs(False)
        assert ctx.open_verify(zb, self.t, self.c, d).tolist() == [1, 1, 0]
        self.open_verify()

    def streams(self, step):
        """The Open cycle on torch's current stream, on a side stream, on the context's own stream, and back."""
        T, ctx = self.torch, self.ctx
        check_open_dev(T, ctx, self.open_ins, self.open_ref, tamper=step % 3)
        side = T.cuda.Stream()
        T.cuda.synchronize()
        with T.cuda.stream(side):
            check_open_dev(T, ctx, self.open_ins, self.open_ref, tamper=(step + 1) % 3)
        side.synchronize()
        ctx._check(ctx._L.rzk_ctx_use_own_stream(ctx._h))
        ctx._stream = None                                              # (the next device-pointer call binds torch's stream again)
        c, t, ok = ctx.open_commit(*self.open_ins[:3])
        assert_open(self.open_ref, c, t, ok)
        check_open_dev(T, ctx, self.open_ins, self.open_ref, tamper=(step + 2) % 3)

    def profiled_step(self):
        """Profiling on for one Open verify: the names of that call alone, as many as rzk_prof_count, the same every time.
        (The 32-bit steps record their own launches too, to name their path: each resets the slots first, as this does.)"""
        ctx = self.ctx
        ctx.prof_enable(True)
        ctx.prof_reset()
        try:
            self.open_verify()
            ctx.synchronize()
            names = kernel_names(ctx)
            assert names and len(names) == ctx.prof_count()
        finally:
            ctx.prof_enable(False)
        assert len(names) <= 3, names                                  # one call: the steps before it launched hundreds
        assert self.profile in (None, names)
        self.profile = names
        self.open_verify()                                             # not recorded
        assert ctx.prof_count() == len(names)


@pytest.mark.parametrize("N,shape,env", [(512, (1, 3, 1), {}), (1024, (2, 5, 2), {"RZK_DKEY": 2, "RZK_SUM_D": 1}),
                                         (2048, (1, 3, 1), {})])
def test_workspace_walk(torch_mod, N, shape, env):
    n, k, l = shape
    ctx = make_ctx(N, n, k, l, env=dict(env, RZK_GRID_CUS=2))
    A = synth.key(np.random.default_rng(9000 + N), N, n, k, l)
    ctx.load_key(A)
    walk = Walk(torch_mod, ctx, A)
    T = torch_mod
    native32 = N in (512, 1024) and shape == (1, 3, 1)                 # else the 32-bit calls take the convert path (ws32)
    # a key whose a1 has 0 / 1 entries only: its products transform nothing, so where Sum keeps operand images none is
    # stored and every "nothing stored yet" mark must come from this call, not from what the arena held before
    A0 = A.copy()
    A0[:n] = 0
    A0[:n, :, 0] = np.random.default_rng(9001 + N).integers(0, 2, (n, k))
    A0[0, 0, 0] = A0[0, k - 1, 0] = 1                                   # (the checkers tamper with columns 0 and k - 1)
    times = []
    for step, B in enumerate(SIZES):
        t0 = time.perf_counter()
        V = SUM_V[step % len(SUM_V)]
        seed = 9200 + 100 * step + N
        ent = entries_of(B, seed)
        families = [
            ("open", lambda: check_key_products_and_open(ctx, A, B, seed, entries=ent)),
            ("open, device form", lambda: check_open_dev(T, ctx, open_inputs(ctx, B, seed + 1),
                                                         open_reference(ctx, A, open_inputs(ctx, B, seed + 1), ent), tamper=B - 1)),
            ("linear", lambda: check_linear_cycle(ctx, A, B, seed + 2, entries=ent, recover=True, torch=T)),
            ("sum", lambda: check_sum_cycle(T, ctx, A, B, V, seed + 3, device_too=True, entries=ent, recover=True)),
            ("open recover", lambda: check_open_recover(ctx, A, B, seed + 11, entries=ent)),
            ("open32", lambda: check_open32(T, ctx, A, B, seed + 4, entries=ent, native=native32)),
            ("response + reject", lambda: check_response_reject(T, ctx, B, seed + 5, ent)),
            ("fs_challenge", lambda: check_fs_challenge(T, ctx, A, B, seed + 6, ent)),
            ("packed", lambda: check_packed(T, ctx, B, V, seed + 7, ent)),
            ("wire", lambda: check_wire(T, ctx, B, seed + 8, ent)),
            ("xof", lambda: check_xof(T, ctx, B, V, seed + 9, ent)),
        ]
        if N == 512:
            families.append(("prover loop", lambda: check_prover(T, ctx, A, None, B, seed + 10)))
        events = [lambda: walk.prover_fault(step), walk.sum_fault, walk.trusted, lambda: walk.streams(step)]
        if step == len(SIZES) // 2:
            events.append(walk.profiled_step)                           # profiling for one step in the middle ...
        order = np.random.default_rng(seed).permutation(len(families))
        for i, f in enumerate(order):
            name, run = families[int(f)]
            try:
                run()
            except AssertionError as exc:
                raise AssertionError("B = %d, V = %d, step %d, %s: %s" % (B, V, step, name, exc)) from exc
            if i < len(events):
                events[(i + step) % len(events)]()
        # Sum at this size under the key without a1 transforms, in the arenas the calls above left, then back
        ctx.load_key(A0)
        check_sum_cycle(T, ctx, A0, B, V, seed + 12, device_too=False, entries=ent, recover=True)
        ctx.load_key(A)
        walk.open_verify()
        times.append((B, V, round(time.perf_counter() - t0, 2)))
    walk.profiled_step()                                               # ... and once more at the end: the same names
    print("workspace walk N = %d %s: (B, V, seconds) %s" % (N, shape, times))


# ---- (d) several contexts of one shape alive at once ------------------------------------------------------------------------------
def test_three_contexts_round_robin(torch_mod):
    N, shape, B = 1024, (1, 3, 1), 5
    ctxs = []
    for tw in (0, 1, 2):
        ctx = make_ctx(N, *shape, env={"RZK_TW_LDS": tw})
        A = synth.key(np.random.default_rng(9800 + tw), N, *shape)
        ctx.load_key(A)
        ins = open_inputs(ctx, B, 9810 + tw)
        ctxs.append((ctx, A, ins, open_reference(ctx, A, ins, range(B))))
    digests = {FS.key_digest(ctx) for ctx, _, _, _ in ctxs}
    assert len(digests) == 3
    for rnd in range(3):
        for ctx, A, ins, ref in ctxs:                                   # device-pointer forms: all on torch's current stream
            c, t, z = check_open_dev(torch_mod, ctx, ins, ref, tamper=rnd)
            if rnd == 0:
                P, cn, tn, zn = P_of(ctx), c.cpu().numpy(), t.cpu().numpy(), z.cpu().numpy()
                assert all(O.open_verify(P, A, zn[b], tn[b], cn[b], ins[3][b]) == 1 for b in range(B))
    for ctx, A, _, _ in ctxs:
        check_digest(ctx, A)
