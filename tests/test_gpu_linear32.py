"""The Linear proof on 32-bit slabs (include/rzk.h "slab32 Linear").

  * parity: the six calls on narrow(inputs) equal narrow() of their 64-bit siblings' outputs bit for bit, both equal the
    oracle, ok / accept / E are identical - on the native kernels ((1,3,1), N = 512 / 1024: the fused two-bit commit at
    B = 8, the norm-kernel fallback at B = 5, several grid-stride trips of row_kernel under RZK_GRID_CUS=1, trusted mode)
    and on the convert path (N = 64, N = 2048, (2,5,2), RZK_DKEY=2, RZK_LIN_E=0).  The profiler's kernel names say which
    path ran: "row_kernel<9, false, i32, false>", "norm_kernel_i32<9>", "unit_io_kernel<9, false, i32>", ...
  * verdict edges of the new instantiations: the range test in both operand loads of a vector x vector term and in the
    epilogue's additions, the zero test, the prover side's input fault, the norm rule at L - 1, L, L + 1 in the fused and
    in the stand-alone form.  Expected verdicts come from the 64-bit call on the widened data and from the oracle.
  * bounds: every 32-bit call of the parity and edge tests runs on device buffers with guard words around each output.
  * argument rules, one device-resident cycle, the short form through packed records, the zero-knowledge prover.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from ring_zk_amd import fiat_shamir as fs
from ring_zk_amd import packed, synth
from ring_zk_amd._lib import MSG_LINEAR_SHORT
from ring_zk_amd.backend import ExactKeyedSampler, ExactKeyedSampler32, KeyedSampler, KeyedSampler32, RzkError
from test_gpu_baseline_shapes import P_of, dev, make_ctx, torch_mod  # noqa: F401
from test_gpu_slab32 import HALF, I32_MAX, I32_MIN, Q, RZK_E_ARG, Guarded, assert_path, n32, raw, w64

pytestmark = pytest.mark.gpu

RANGE_FAULTS = [HALF + 1, -HALF - 1, I32_MAX, I32_MIN, HALF - Q]   # the last: an alias of the canonical HALF
COIN_R = 1 << 40


class Lin32:
    """The seven 32-bit calls on device buffers with guarded outputs; inputs are numpy int32 arrays (coin: int64)."""

    def __init__(self, torch, ctx):
        self.T, self.ctx = torch, ctx
        self.names = []

    def _call(self, name, ins, outs, B, mid=()):
        """ins, outs in the C argument order; mid: plain arguments between them (the reject call's R and lnM)."""
        d_in = [dev(self.T, a) for a in ins]
        self.names = raw(self.ctx, name, [a.data_ptr() for a in d_in] + [o.ptr() for o in outs], B) if not mid else \
            self._raw_mid(name, d_in, mid, outs, B)
        return [o.take() for o in outs]

    def _raw_mid(self, name, d_in, mid, outs, B):
        c = self.ctx
        c._bind_torch_stream()
        c.prof_enable(True)
        c.prof_reset()
        st = getattr(c._L, name + "_dev")(c._h, *[C.c_void_p(a.data_ptr()) for a in d_in], *mid,
                                          *[C.c_void_p(o.ptr()) for o in outs], B)
        c._check(st)
        c.synchronize()
        names = [nm for nm, _ in c.prof_read_kernels()]
        c.prof_enable(False)
        return names

    def _g(self, B, rows, dt=None):
        return Guarded(self.T, (B, rows, self.ctx.N) if rows else (B,), dt or self.T.int32)

    def commit(self, g, x, r, rp, y, yp):
        c, B = self.ctx, x.shape[0]
        outs = [self._g(B, c.n + c.l), self._g(B, c.n + c.l), self._g(B, c.n), self._g(B, c.n), self._g(B, c.l),
                self._g(B, 0, self.T.uint8)]
        return self._call("rzk_linear_commit32_batch", (g, x, r, rp, y, yp), outs, B)

    def mask(self, g, y, yp):
        c, B = self.ctx, y.shape[0]
        return self._call("rzk_linear_mask32_batch", (g, y, yp), [self._g(B, c.n), self._g(B, c.n), self._g(B, c.l)], B)

    def response(self, y, yp, r, rp, d):
        c, B = self.ctx, y.shape[0]
        return self._call("rzk_linear_response32_batch", (y, yp, r, rp, d), [self._g(B, c.k), self._g(B, c.k)], B)

    def response_reject(self, y, yp, r, rp, d, coin, lnM):
        c, B = self.ctx, y.shape[0]
        outs = [self._g(B, c.k), self._g(B, c.k), self._g(B, 0, self.T.uint8), self._g(B, 0, self.T.int64)]
        return self._call("rzk_linear_response_reject32_batch", (y, yp, r, rp, d, coin), outs, B,
                          mid=(C.c_uint64(COIN_R), C.c_double(lnM)))

    def verify(self, z, zp, c, cp, g, t, tp, u, d):
        B = z.shape[0]
        return self._call("rzk_linear_verify32_batch", (z, zp, c, cp, g, t, tp, u, d), [self._g(B, 0, self.T.uint8)], B)[0]

    def recover(self, z, zp, c, cp, g, d):
        cx, B = self.ctx, z.shape[0]
        outs = [self._g(B, cx.n), self._g(B, cx.n), self._g(B, cx.l), self._g(B, 0, self.T.uint8)]
        return self._call("rzk_linear_recover32_batch", (z, zp, c, cp, g, d), outs, B)

    def norm2(self, v, bound):
        c = self.ctx
        B, rows = v.shape[0], v.shape[1]
        ok = self._g(B, 0, self.T.uint8)
        dv = dev(self.T, v)
        c._bind_torch_stream()
        c.prof_enable(True)
        c.prof_reset()
        c._check(c._L.rzk_norm2_le32_batch_dev(c._h, C.c_void_p(dv.data_ptr()), rows, bound, C.c_void_p(ok.ptr()), B))
        c.synchronize()
        self.names = [nm for nm, _ in c.prof_read_kernels()]
        c.prof_enable(False)
        return ok.take()


def honest(rng, P, B):
    g = synth.uniform(rng, (B, P.N))
    x = synth.uniform(rng, (B, P.l, P.N))
    r, rp = synth.small(rng, (B, P.k, P.N), P.b), synth.small(rng, (B, P.k, P.N), P.b)
    y, yp = synth.gauss(rng, (B, P.k, P.N), P.sigma), synth.gauss(rng, (B, P.k, P.N), P.sigma)
    d = synth.challenge(rng, (B,), P.N, P.kappa)
    return g, x, r, rp, y, yp, d


WIDTH_FREE = ("reject_decide_kernel",)    # reads the partials of the response rows: no slab, no width


def assert_native(names, must=(), never=()):
    """Every launch is an i32 instantiation: no widen / narrow, no 64-bit kernel."""
    assert names, "the call launched nothing"
    assert all("i32" in nm or nm in WIDTH_FREE for nm in names), names
    for m in must:
        assert m in names, (m, names)
    for m in never:
        assert m not in names, (m, names)


def check_cycle(torch, ctx, A, B, rng, native, fused=None, entries=None):
    """The six calls in both widths on the same values, against each other and the oracle."""
    P, N = P_of(ctx), ctx.N
    L = N.bit_length() - 1
    row = f"row_kernel<{L}, false, i32, false>"
    norm = f"norm_kernel_i32<{L}>"
    s = Lin32(torch, ctx)
    ents = list(range(B)) if entries is None else entries
    g, x, r, rp, y, yp, d = honest(rng, P, B)
    g3, x3, r3, rp3, y3, yp3, d3 = (n32(a) for a in (g, x, r, rp, y, yp, d))

    def path(outputs=True, must=(), never=()):
        if native:
            assert_native(s.names, must, never)
        else:
            assert_path(s.names, False, outputs=outputs)

    # commit
    w = ctx.linear_commit(g, x, r, rp, y, yp)
    got = s.commit(g3, x3, r3, rp3, y3, yp3)
    path(must=(row,) + ((norm,) if fused is False else ()), never=(norm,) if fused else ())
    if native and fused is False:
        assert s.names.count(norm) == 2, s.names     # r, then r'
    for a, b in zip(got[:5], w[:5]):
        assert np.array_equal(a, n32(b))
    assert np.array_equal(got[5], w[5]) and (w[5] == 3).all()
    for e in ents:
        ref = O.linear_commit(P, A, g[e], x[e], r[e], rp[e], y[e], yp[e])
        assert all(np.array_equal(w64(a[e]), b) for a, b in zip(got[:5], ref[:5])) and int(got[5][e]) == int(ref[5]), e
    c, cp, t, tp, u = w[:5]
    c3, cp3, t3, tp3, u3 = got[:5]
    # mask: the y-only half gives the same t, t', u
    m = s.mask(g3, y3, yp3)
    path(must=(row,))
    assert np.array_equal(m[0], t3) and np.array_equal(m[1], tp3) and np.array_equal(m[2], u3)
    # response, and response with the rejection test
    z, zp = ctx.linear_response(y, yp, r, rp, d)
    z3, zp3 = s.response(y3, yp3, r3, rp3, d3)
    path()
    assert np.array_equal(z3, n32(z)) and np.array_equal(zp3, n32(zp))
    for e in ents:
        zr, zpr = O.linear_response(P, y[e], yp[e], r[e], rp[e], d[e])
        assert np.array_equal(w64(z3[e]), zr) and np.array_equal(w64(zp3[e]), zpr), e
    coin = rng.integers(0, COIN_R, B, dtype=np.int64)
    lnM = fs.zk_lnm(2)
    wz, wzp, wacc, wE = ctx.linear_response_reject(y, yp, r, rp, d, coin, COIN_R, lnM)
    rz, rzp, racc, rE = s.response_reject(y3, yp3, r3, rp3, d3, coin, lnM)
    path()
    assert np.array_equal(rz, z3) and np.array_equal(rzp, zp3) and np.array_equal(wz, z)
    assert np.array_equal(racc, wacc) and np.array_equal(rE, wE)
    # verify: honest proofs, then every second proof with one coefficient of u off by one
    acc = ctx.linear_verify(z, zp, c, cp, g, t, tp, u, d)
    acc3 = s.verify(z3, zp3, c3, cp3, g3, t3, tp3, u3, d3)
    path(outputs=False, must=(row,))
    assert np.array_equal(acc3, acc) and acc.all()
    for e in ents:
        assert O.linear_verify(P, A, z[e], zp[e], c[e], cp[e], g[e], t[e], tp[e], u[e], d[e]) == 1, e
    ub = u3.copy()
    odd = np.arange(1, B, 2)
    ub[odd, 0, (37 * odd + 5) % N] ^= 1
    acc3 = s.verify(z3, zp3, c3, cp3, g3, t3, tp3, ub, d3)
    assert np.array_equal(acc3, ctx.linear_verify(z, zp, c, cp, g, t, tp, w64(ub), d))
    assert acc3[0::2].all() and not acc3[1::2].any()
    # recover: an honest proof recovers its own t, t', u
    wt, wtp, wu, wacc = ctx.linear_recover(z, zp, c, cp, g, d)
    rt, rtp, ru, racc = s.recover(z3, zp3, c3, cp3, g3, d3)
    if native:
        assert_native(s.names, must=(row,))
    assert np.array_equal(rt, t3) and np.array_equal(rtp, tp3) and np.array_equal(ru, u3)
    assert np.array_equal(rt, n32(wt)) and np.array_equal(ru, n32(wu)) and np.array_equal(racc, wacc) and racc.all()


# ---- parity on the native kernels ----------------------------------------------------------------------------------------
NATIVE = {
    "fused-8": ({}, False, 8, True),           # ok is four-byte aligned and B % 4 == 0: the fused two-bit commit
    "fallback-5": ({}, False, 5, False),       # B % 4 != 0: norm_kernel_i32 for r and r', then the plain commit rows
    "grid1-100": ({"RZK_GRID_CUS": 1}, False, 100, True),   # several grid-stride trips of row_kernel, its row rotation included
    "trusted-8": ({}, True, 8, True),
}


@pytest.mark.parametrize("kind", list(NATIVE))
@pytest.mark.parametrize("N", [512, 1024])
def test_parity_native(torch_mod, N, kind):
    env, trusted, B, fused = NATIVE[kind]
    ctx = make_ctx(N, 1, 3, 1, env=env)
    rng = np.random.default_rng(61000 + N + B)
    A = synth.key(rng, N, 1, 3, 1)
    ctx.load_key(A)
    if trusted:
        ctx.trust_device_outputs(True)
    check_cycle(torch_mod, ctx, A, B, rng, native=True, fused=fused, entries=None if B <= 8 else [0, 1, 49, 98, 99])


# ---- the convert path --------------------------------------------------------------------------------------------------------
CONVERT = {
    "small-64": (64, (1, 3, 1), {}),
    "pair-2048": (2048, (1, 3, 1), {}),
    "groups-1024": (1024, (2, 5, 2), {}),
    "dkey2-512": (512, (1, 3, 1), {"RZK_DKEY": 2}),
    "lin_e0-1024": (1024, (1, 3, 1), {"RZK_LIN_E": 0}),
}


@pytest.mark.parametrize("cid", list(CONVERT))
def test_convert_path(torch_mod, cid):
    """Contexts without native kernels for some program of the call: the same bytes through widen, the sibling, narrow.
    (RZK_DKEY=2 leaves the response rows native: they multiply by no g.  RZK_LIN_E=0 converts the verifier alone.)"""
    N, (n, k, l), env = CONVERT[cid]
    ctx = make_ctx(N, n, k, l, env=env)
    rng = np.random.default_rng(62000 + N + n + len(env))
    A = synth.key(rng, N, n, k, l)
    ctx.load_key(A)
    P, B = P_of(ctx), 3
    s = Lin32(torch_mod, ctx)
    g, x, r, rp, y, yp, d = honest(rng, P, B)
    g3, x3, r3, rp3, y3, yp3, d3 = (n32(a) for a in (g, x, r, rp, y, yp, d))
    whole = cid not in ("dkey2-512", "lin_e0-1024")     # every call of the context converts
    row = f"row_kernel<{N.bit_length() - 1}, false, i32, false>"

    def path(converts, outputs=True, must=()):
        """This call converts, or (the rule is per call, not per context) it stays native."""
        if converts:
            assert_path(s.names, False, outputs=outputs)
        else:
            assert_native(s.names, must=must)

    w = ctx.linear_commit(g, x, r, rp, y, yp)
    got = s.commit(g3, x3, r3, rp3, y3, yp3)
    path(cid != "lin_e0-1024", must=(row,))
    assert all(np.array_equal(a, n32(b)) for a, b in zip(got[:5], w[:5])) and np.array_equal(got[5], w[5])
    c, cp, t, tp, u = w[:5]
    m = s.mask(g3, y3, yp3)
    path(cid != "lin_e0-1024", must=(row,))
    assert all(np.array_equal(a, n32(b)) for a, b in zip(m, (t, tp, u)))
    z, zp = ctx.linear_response(y, yp, r, rp, d)
    z3, zp3 = s.response(y3, yp3, r3, rp3, d3)
    path(whole)
    assert np.array_equal(z3, n32(z)) and np.array_equal(zp3, n32(zp))
    coin = rng.integers(0, COIN_R, B, dtype=np.int64)
    wr = ctx.linear_response_reject(y, yp, r, rp, d, coin, COIN_R, fs.zk_lnm(2))
    rr = s.response_reject(y3, yp3, r3, rp3, d3, coin, fs.zk_lnm(2))
    path(whole)
    assert np.array_equal(rr[0], z3) and np.array_equal(rr[1], zp3) and np.array_equal(rr[2], wr[2]) and np.array_equal(rr[3], wr[3])
    args = [n32(a) for a in (z, zp, c, cp, g, t, tp, u, d)]
    acc3 = s.verify(*args)
    assert_path(s.names, False, outputs=False)
    assert np.array_equal(acc3, ctx.linear_verify(z, zp, c, cp, g, t, tp, u, d)) and acc3.all()
    rt, rtp, ru, racc = s.recover(*[n32(a) for a in (z, zp, c, cp, g, d)])
    path(cid != "lin_e0-1024", must=(row,))
    assert np.array_equal(rt, n32(t)) and np.array_equal(rtp, n32(tp)) and np.array_equal(ru, n32(u)) and racc.all()
    v = n32(np.concatenate([r, rp], axis=1))
    ok = s.norm2(v, P.commit_bound)
    if N in (64, 2048):
        assert s.names == ["widen_kernel"], s.names     # (the 64-bit norm kernel takes no profiling slot)
    else:
        assert s.names == [f"norm_kernel_i32<{N.bit_length() - 1}>"], s.names
    assert np.array_equal(ok, ctx.norm2_le(w64(v), P.commit_bound)) and ok.all()


# ---- verdict edges in the new instantiations ---------------------------------------------------------------------------------
def valid_proof(ctx, A, rng, g_half_at=()):
    """One honest proof from the 64-bit calls, accepted by the oracle; g holds HALF at the given coefficients."""
    P = P_of(ctx)
    g, x, r, rp, y, yp, d = honest(rng, P, 1)
    g[0, list(g_half_at)] = HALF
    c, cp, t, tp, u, ok = ctx.linear_commit(g, x, r, rp, y, yp)
    z, zp = ctx.linear_response(y, yp, r, rp, d)
    assert int(ok[0]) == 3 and O.linear_verify(P, A, z[0], zp[0], c[0], cp[0], g[0], t[0], tp[0], u[0], d[0]) == 1
    return dict(z=z[0], zp=zp[0], c=c[0], cp=cp[0], g=g[0], t=t[0], tp=tp[0], u=u[0], d=d[0])


ORDER = ("z", "zp", "c", "cp", "g", "t", "tp", "u", "d")


@pytest.mark.parametrize("trusted", [False, True], ids=["checked", "trusted"])
@pytest.mark.parametrize("N", [512, 1024])
def test_verifier_range_and_zero_tests(torch_mod, N, trusted):
    """One fault per proof: every range violation an int32 can hold (and HALF - q) at the first, a middle and the last
    coefficient of g (an operand load of the vector x vector term), u (an addition of the epilogue) and c' (which reaches
    row_kernel as e'); then +-1 on u, t, t' (the zero tests).  Only the faulted proofs reject, the call succeeds, the
    verdicts are the 64-bit call's on the widened data.  g holds HALF at the three positions, so HALF - q there is an alias
    of the honest value: only the range test can reject it, and trusted mode, which skips that test, accepts it (every
    other fault changes a residue and fails a relation in either mode)."""
    ctx = make_ctx(N, 1, 3, 1)
    rng = np.random.default_rng(63000 + N)
    A = synth.key(rng, N, 1, 3, 1)
    ctx.load_key(A)
    s = Lin32(torch_mod, ctx)
    proof = valid_proof(ctx, A, rng, g_half_at=(0, N // 2 + 1, N - 1))
    faults = [(op, pos, val) for op in ("g", "u", "cp") for pos in (0, N // 2 + 1, N - 1) for val in RANGE_FAULTS]
    zeros = [(op, pos, sgn) for op, pos in (("u", 0), ("u", N - 1), ("t", 65), ("tp", N - 2)) for sgn in (1, -1)]
    B = len(faults) + len(zeros) + 3
    slabs = {key: np.broadcast_to(n32(v), (B,) + v.shape).copy() for key, v in proof.items()}
    for e, (op, pos, val) in enumerate(faults):
        slabs[op].reshape(B, -1)[e, -N + pos if op == "cp" else pos] = val       # c': its last row (the a2 part)
    for i, (op, pos, sgn) in enumerate(zeros):
        e = len(faults) + i
        cur = int(slabs[op].reshape(B, -1)[e, pos])
        slabs[op].reshape(B, -1)[e, pos] = cur + sgn if abs(cur + sgn) <= HALF else cur - sgn
    if trusted:
        ctx.trust_device_outputs(True)
    want = ctx.linear_verify(*[w64(slabs[key]) for key in ORDER])
    got = s.verify(*[slabs[key] for key in ORDER])
    assert_native(s.names, must=(f"row_kernel<{N.bit_length() - 1}, false, i32, false>",))
    assert np.array_equal(got, want), np.flatnonzero(got != want)
    assert got[-3:].all() and not got[len(faults):-3].any()
    if not trusted:
        assert not got[:len(faults)].any()
    else:
        alias = np.array([op == "g" and val == HALF - Q for op, _, val in faults])
        assert got[:len(faults)][alias].all() and not got[:len(faults)][~alias].any()
    # recover decides the range test of its inputs with the same loads
    _, _, _, acc64 = ctx.linear_recover(*[w64(slabs[key]) for key in ("z", "zp", "c", "cp", "g", "d")])
    _, _, _, acc32 = s.recover(*[slabs[key] for key in ("z", "zp", "c", "cp", "g", "d")])
    assert np.array_equal(acc32, acc64)
    if not trusted:
        in_rec = np.array([op in ("g", "cp") for op, _, _ in faults])
        assert not acc32[:len(faults)][in_rec].any() and acc32[:len(faults)][~in_rec].all() and acc32[len(faults):].all()


@pytest.mark.parametrize("N", [512, 1024])
def test_prover_side_faults_fail_the_call(torch_mod, N):
    """A non-canonical g or x (both operand loads of gx = g . x), at the first, a middle and the last coefficient: the host
    form returns RZK_E_ARG, the device form raises the sticky fault; the next clean call succeeds.  Trusted mode: no test,
    the low word is what the kernels compute with, as in the 64-bit call."""
    ctx = make_ctx(N, 1, 3, 1)
    rng = np.random.default_rng(64000 + N)
    A = synth.key(rng, N, 1, 3, 1)
    ctx.load_key(A)
    P, B = P_of(ctx), 3
    s = Lin32(torch_mod, ctx)
    ops = [n32(a) for a in honest(rng, P, B)[:6]]
    trial = 0
    for i in (0, 1):                         # g, x
        for pos in (0, N // 2 + 1, N - 1):
            for val in RANGE_FAULTS:
                args = [a.copy() for a in ops]
                args[i].reshape(B, -1)[trial % B, pos] = val
                trial += 1
                with pytest.raises(RzkError) as ei:
                    ctx.linear_commit32(*args)                   # host form
                assert ei.value.status == RZK_E_ARG, (i, pos, val)
                if trial % 5 == 0:
                    with pytest.raises(RzkError) as ei:
                        s.commit(*args)                          # device form: synchronize reports the sticky word
                    assert ei.value.status == RZK_E_ARG
                    assert (s.commit(*ops)[5] == 3).all()        # ... and consumed it
    bad = [a.copy() for a in ops]
    bad[0][1, 65] = HALF - Q
    with pytest.raises(RzkError):
        ctx.linear_mask32(bad[0], bad[4], bad[5])
    ctx.trust_device_outputs(True)
    got = s.commit(*bad)
    want = ctx.linear_commit(*[w64(a) for a in bad])
    assert all(np.array_equal(a, n32(b)) for a, b in zip(got[:5], want[:5])) and np.array_equal(got[5], want[5])


def edge_polys(P, N, bound, rng):
    plan = synth.norm_plan((bound + 1) ** 2)
    out = []
    for name in ("below", "at", "above"):
        for style, pos in (("point", 63), ("point", N - 3), ("spread", 0)):
            p = synth.norm_edge(N, plan[name], style, pos, rng)
            out.append((f"{name}/{style}@{pos}", p, int(O.check_norm(p[None], bound))))
    assert [w for _, _, w in out] == [1] * 3 + [0] * 6
    return out


@pytest.mark.parametrize("form", ["fused", "fallback"])
@pytest.mark.parametrize("N", [512, 1024])
def test_commit_norm_bits(torch_mod, N, form):
    """Sum of squares L - 1, L, L + 1 in every row of r (bit 0 of ok) and of r' (bit 1), in the fused form (B % 4 == 0) and
    through norm_kernel_i32 (B % 4 != 0): the byte is the oracle's and the 64-bit call's."""
    ctx = make_ctx(N, 1, 3, 1)
    P = P_of(ctx)
    rng = np.random.default_rng(65000 + N)
    A = synth.key(rng, N, 1, 3, 1)
    ctx.load_key(A)
    polys = edge_polys(P, N, P.commit_bound, rng)
    places = [(vec, i, j) for vec in (0, 1) for i in range(len(polys)) for j in range(ctx.k)]
    B = len(places) + (2 if form == "fused" else 1)
    assert (B % 4 == 0) == (form == "fused")
    g, x, r, rp, y, yp, _ = honest(rng, P, B)
    want = np.full(B, 3, dtype=np.uint8)
    for e, (vec, i, j) in enumerate(places):
        (rp if vec else r)[e, j] = polys[i][1]
        if not polys[i][2]:
            want[e] = 3 & ~(1 << vec)
    assert set(want.tolist()) == {1, 2, 3}
    s = Lin32(torch_mod, ctx)
    got = s.commit(*[n32(a) for a in (g, x, r, rp, y, yp)])
    norm = f"norm_kernel_i32<{N.bit_length() - 1}>"
    assert_native(s.names, must=(norm,) if form == "fallback" else (), never=(norm,) if form == "fused" else ())
    bad = [(polys[places[e][1]][0], places[e], int(got[5][e]), int(want[e])) for e in range(len(places)) if got[5][e] != want[e]]
    assert not bad, bad
    w = ctx.linear_commit(g, x, r, rp, y, yp)
    assert np.array_equal(got[5], w[5]) and all(np.array_equal(a, n32(b)) for a, b in zip(got[:5], w[:5]))
    for e in (0, len(places) // 2, len(places) - 1):
        assert int(O.linear_commit(P, A, g[e], x[e], r[e], rp[e], y[e], yp[e])[5]) == int(want[e])


@pytest.mark.parametrize("N", [512, 1024])
def test_verify_norm_edge_on_z_and_zp(torch_mod, N):
    """The same three sums in every row of z and of z'; c = c' = 0 and t, t', u are what linear_recover computes for the
    crafted vectors, so the relations hold and the verdict is the oracle's check_norm of the crafted row."""
    ctx = make_ctx(N, 1, 3, 1)
    P = P_of(ctx)
    rng = np.random.default_rng(66000 + N)
    A = synth.key(rng, N, 1, 3, 1)
    ctx.load_key(A)
    polys = edge_polys(P, N, P.verify_bound, rng)
    places = [(vec, i, j) for vec in (0, 1) for i in range(len(polys)) for j in range(ctx.k)]
    B = len(places) + 1
    g = synth.uniform(rng, (B, N))
    z, zp = synth.gauss(rng, (B, ctx.k, N), P.sigma), synth.gauss(rng, (B, ctx.k, N), P.sigma)
    d = synth.challenge(rng, (B,), N, P.kappa)
    want = np.ones(B, dtype=np.uint8)
    for e, (vec, i, j) in enumerate(places):
        (zp if vec else z)[e, j] = polys[i][1]
        want[e] = polys[i][2]
    c = np.zeros((B, ctx.n + ctx.l, N), dtype=np.int64)
    t, tp, u, acc = ctx.linear_recover(z, zp, c, c, g, d)
    assert np.array_equal(acc, want)
    s = Lin32(torch_mod, ctx)
    args = [n32(a) for a in (z, zp, c, c, g, t, tp, u, d)]
    got = s.verify(*args)
    assert_native(s.names)
    bad = [(polys[places[e][1]][0], places[e]) for e in range(len(places)) if got[e] != want[e]]
    assert not bad, bad
    assert np.array_equal(got, ctx.linear_verify(z, zp, c, c, g, t, tp, u, d))
    for e in (0, len(places) // 2, len(places) - 1, B - 1):
        assert int(O.linear_verify(P, A, z[e], zp[e], c[e], c[e], g[e], t[e], tp[e], u[e], d[e]) == 1) == int(want[e])
    rt, rtp, ru, racc = s.recover(*[n32(a) for a in (z, zp, c, c, g, d)])
    assert np.array_equal(racc, want) and np.array_equal(rt, n32(t)) and np.array_equal(ru, n32(u))


@pytest.mark.parametrize("N", [512, 1024])
def test_norm2_le32(torch_mod, N):
    """The stand-alone predicate at L - 1, L, L + 1 in either row of a two-row block, and on a non-canonical input."""
    ctx = make_ctx(N, 1, 3, 1)
    P = P_of(ctx)
    rng = np.random.default_rng(67000 + N)
    polys = edge_polys(P, N, P.commit_bound, rng)
    B = 2 * len(polys) + 1
    v = synth.small(rng, (B, 2, N), P.b)
    want = np.ones(B, dtype=np.uint8)
    for e in range(B - 1):
        v[e, e % 2] = polys[e // 2][1]
        want[e] = polys[e // 2][2]
    s = Lin32(torch_mod, ctx)
    got = s.norm2(n32(v), P.commit_bound)
    assert s.names == [f"norm_kernel_i32<{N.bit_length() - 1}>"], s.names
    assert np.array_equal(got, want) and np.array_equal(got, ctx.norm2_le(v, P.commit_bound))
    assert np.array_equal(ctx.norm2_le32(n32(v), P.commit_bound), want)          # host form
    for val in RANGE_FAULTS:
        bad = n32(v)
        bad[B - 1, 1, N - 1] = val
        with pytest.raises(RzkError) as ei:
            ctx.norm2_le32(bad, P.commit_bound)
        assert ei.value.status == RZK_E_ARG
        with pytest.raises(RzkError):
            ctx.norm2_le(w64(bad), P.commit_bound)
        ok = ctx.norm2_le32(dev(torch_mod, bad), 1 << 40)        # device form: the verdict is cleared whatever the bound
        assert int(ok.cpu()[B - 1]) == 0 and bool(ok.cpu()[:B - 1].all())
        with pytest.raises(RzkError):
            ctx.synchronize()


# ---- argument rules ----------------------------------------------------------------------------------------------------------
def test_argument_rules(torch_mod):
    torch = torch_mod
    N = 512
    ctx = make_ctx(N, 1, 3, 1)
    rng = np.random.default_rng(68000)
    ctx.load_key(synth.key(rng, N, 1, 3, 1))
    L, h = ctx._L, ctx._h
    B = 2
    buf = torch.zeros(B * 3 * N + 16, dtype=torch.int32, device="cuda")
    coin = torch.zeros(16, dtype=torch.int64, device="cuda")
    flags = torch.zeros(16, dtype=torch.uint8, device="cuda")
    p, f, cn = C.c_void_p(buf.data_ptr()), C.c_void_p(flags.data_ptr()), C.c_void_p(coin.data_ptr())
    R, lnM = C.c_uint64(COIN_R), C.c_double(1.0)
    # (arguments, indices of the int32 slabs, indices of the other pointers that must not be NULL)
    calls = {
        "rzk_linear_commit32_batch_dev": ([p] * 11 + [f], range(11), ()),          # ok may be NULL
        "rzk_linear_mask32_batch_dev": ([p] * 6, range(6), ()),
        "rzk_linear_response32_batch_dev": ([p] * 7, range(7), ()),
        "rzk_linear_response_reject32_batch_dev": ([p] * 5 + [cn, R, lnM, p, p, f, cn], [0, 1, 2, 3, 4, 8, 9], (5, 10)),
        "rzk_linear_verify32_batch_dev": ([p] * 9 + [f], range(9), (9,)),
        "rzk_linear_recover32_batch_dev": ([p] * 9 + [f], range(9), (9,)),
        "rzk_norm2_le32_batch_dev": ([p, C.c_uint32(1), C.c_uint64(5), f], [0], (3,)),
    }
    for name, (args, slabs, others) in calls.items():
        fn = getattr(L, name)
        empty = [None if isinstance(a, C.c_void_p) else a for a in args]
        assert fn(h, *empty, 0) == 0, name                                  # B == 0: a no-op, pointers may be NULL
        for i in list(slabs) + list(others):
            nul = list(args)
            nul[i] = None
            assert fn(h, *nul, B) == RZK_E_ARG, (name, "NULL", i)
        for i in slabs:
            off = list(args)
            off[i] = C.c_void_p(buf.data_ptr() + 8)                         # element-aligned, not 16-byte aligned
            assert fn(h, *off, B) == RZK_E_ARG, (name, "misaligned", i)
    ctx.synchronize()
    # the 64-bit methods keep rejecting int32, the 32-bit ones int64
    y = np.zeros((B, 3, N), dtype=np.int32)
    d = np.zeros((B, N), dtype=np.int32)
    with pytest.raises(ValueError):
        ctx.linear_response(y, y, y, y, d)
    with pytest.raises(ValueError):
        ctx.linear_response32(w64(y), w64(y), w64(y), w64(y), w64(d))
    with pytest.raises(ValueError):
        ctx.norm2_le(y, 5)


# ---- whole cycles on the device ----------------------------------------------------------------------------------------------
def test_device_resident_cycle_and_short_form(torch_mod):
    """linear_commit32 -> challenge32 -> linear_response_reject32 -> linear_verify32 on device tensors, every launch an i32
    instantiation; then linear_short32 -> packed records -> linear_verify_short_packed32 accepts every proof, and one
    record tampered in z' rejects exactly that proof."""
    torch = torch_mod
    N, B = 1024, 8
    ctx = make_ctx(N, 1, 3, 1)
    P = P_of(ctx)
    rng = np.random.default_rng(69000)
    A = synth.key(rng, N, 1, 3, 1)
    ctx.load_key(A)
    g, x, r, rp, y, yp, _ = (dev(torch, n32(a)) for a in honest(rng, P, B))
    coin = dev(torch, rng.integers(0, COIN_R, B, dtype=np.int64))
    ctx._bind_torch_stream()
    ctx.prof_enable(True)
    ctx.prof_reset()
    c, cp, t, tp, u, ok = ctx.linear_commit32(g, x, r, rp, y, yp)
    d, _, okf = fs.challenge32(ctx, fs.MSG_LINEAR_COMMITMENT, c, cp, g, t, tp, u)
    z, zp, _, _ = ctx.linear_response_reject32(y, yp, r, rp, d, coin, COIN_R, fs.zk_lnm(2))
    acc = ctx.linear_verify32(z, zp, c, cp, g, t, tp, u, d)
    ctx.synchronize()
    names = [nm for nm, _ in ctx.prof_read_kernels()]
    ctx.prof_enable(False)
    assert_native(names, must=("row_kernel<10, false, i32, false>", "fs_leaf_kernel<i32>"))
    assert all(v.dtype == torch.int32 for v in (c, cp, t, tp, u, d, z, zp))
    assert bool((ok == 3).all()) and bool(okf.all()) and bool(acc.all())
    assert bool(fs.linear_verify32(ctx, c, cp, g, t, tp, u, z, zp).all())
    # the same proof verifies in the other width: the transcript is one
    wide = [ctx.widen(v) for v in (c, cp, g, t, tp, u, z, zp)]
    assert bool(fs.linear_verify(ctx, *wide).all())
    for e in (0, B - 1):
        hv = [w64(v[e].cpu().numpy()) for v in (z, zp, c, cp, g, t, tp, u, d)]
        assert O.linear_verify(P, A, *hv) == 1
    # short form through packed records
    ds = fs.linear_short32(ctx, c, cp, g, t, tp, u, z, zp)
    assert bool((ds == d).all())
    records, okr = packed.encode_batch32(ctx, MSG_LINEAR_SHORT, c, cp, g, ds, z, zp)
    assert bool(okr.all())
    assert bool(fs.linear_verify_short_packed32(ctx, records).all())
    assert bool(fs.linear_verify_short_packed(ctx, records).all())
    zt = zp.clone()
    zt[5, 2, 700] += 1
    rec_t, okt = packed.encode_batch32(ctx, MSG_LINEAR_SHORT, c, cp, g, ds, z, zt)
    assert bool(okt.all())
    got = fs.linear_verify_short_packed32(ctx, rec_t).cpu().numpy()
    assert [int(v) for v in got] == [int(e != 5) for e in range(B)]


@pytest.mark.parametrize("exact", [False, True], ids=["box-muller", "dgauss"])
def test_prove_zk32_equals_narrowed_prove_zk(torch_mod, exact):
    """linear_prove_zk32 under a fixed key and nonce: every slab is narrow() of linear_prove_zk's, ok and rounds are the
    same, and the sampler's counter ends where the 64-bit loop leaves it."""
    torch = torch_mod
    N, B = 512, 8
    ctx = make_ctx(N, 1, 3, 1)
    P = P_of(ctx)
    rng = np.random.default_rng(70000)
    ctx.load_key(synth.key(rng, N, 1, 3, 1))
    g, x = synth.uniform(rng, (B, N)), synth.uniform(rng, (B, P.l, N))
    key = bytes(range(32))
    S64, S32 = (ExactKeyedSampler, ExactKeyedSampler32) if exact else (KeyedSampler, KeyedSampler32)
    s64 = S64(ctx, key, nonce0=11)
    out64 = fs.linear_prove_zk(ctx, dev(torch, g), dev(torch, x), s64, max_rounds=32)
    s32 = S32(ctx, key, nonce0=11)
    out32 = fs.linear_prove_zk32(ctx, dev(torch, n32(g)), dev(torch, n32(x)), s32, max_rounds=32)
    ctx.synchronize()
    assert s32.counter == s64.counter
    names = ("c", "cp", "t", "tp", "u", "z", "zp", "ok", "r", "rp", "rounds")
    assert len(out32) == len(out64) == len(names)
    for nm, a, b in zip(names, out32, out64):
        if nm in ("ok", "rounds"):
            assert bool((a == b).all()), nm
        else:
            assert a.dtype == torch.int32 and bool((a == ctx.narrow(b)).all()), nm
    assert bool(out32[7].all())
    with pytest.raises(ValueError):
        fs.linear_prove_zk32(ctx, dev(torch, g), dev(torch, x), s32)
