"""The 32-bit coefficient slabs on the GPU (include/rzk.h "32-bit slabs").

  * parity: the four Open calls on narrow(inputs) equal narrow() of their 64-bit siblings' outputs bit for bit, both equal
    the oracle, verdict bytes are identical — on the native kernels (N = 512 / 1024, (1,3,1); default context, one team
    per proof with and without the in-kernel flag preset, trusted mode, several grid-stride trips) and on the convert
    path (N = 64, N = 2048, (2,5,2)).  The profiler's kernel names say which path ran.
  * verdict edges of the new instantiations: the range test at every coefficient position (one unsigned compare now),
    the zero test, the prover side's input fault, trusted mode, the fused norm predicate at L - 1, L, L + 1.  Expected
    verdicts come from the 64-bit call on the widened data, and from the oracle's check_norm where the norm decides.
  * bounds: every 32-bit call here runs on device buffers with guard words on both sides of each output.
  * narrow / widen round trip and the argument rules; a whole commit32 -> response32 -> verify32 cycle.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from ring_zk_amd import synth
from ring_zk_amd.backend import RzkError
from test_gpu_baseline_shapes import P_of, dev, make_ctx, torch_mod  # noqa: F401
from test_gpu_verdict_edges import open_entries

pytestmark = pytest.mark.gpu

Q = O.Q_DEFAULT
HALF = (Q - 1) // 2
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
RZK_E_ARG = -1
GUARD = 64             # guard elements on either side of an output (int32: 256 bytes, so the slab stays 16-byte aligned)
PATTERN = 0x5A


class Guarded:
    """A device output with guard elements on both sides, all bytes PATTERN before the call."""

    def __init__(self, torch, shape, dtype):
        self.n = int(np.prod(shape))
        self.shape = shape
        self.buf = torch.empty(GUARD + self.n + GUARD, dtype=dtype, device="cuda")
        self.buf.view(torch.uint8).fill_(PATTERN)
        self.fill = self.buf[:1].clone()

    @property
    def data(self):
        return self.buf[GUARD:GUARD + self.n].view(self.shape)

    def ptr(self):
        return self.data.data_ptr()

    def take(self):
        """The output as numpy, after checking that no guard element changed."""
        assert bool((self.buf[:GUARD] == self.fill).all()) and bool((self.buf[GUARD + self.n:] == self.fill).all()), \
            "a store went outside the output slab"
        return self.data.cpu().numpy()


def kernel_names(ctx):
    return [nm for nm, _ in ctx.prof_read_kernels()]


def raw(ctx, name, ptrs, B):
    """One *_dev call by pointer; the sticky input fault of a prover-side call surfaces in synchronize()."""
    ctx._bind_torch_stream()
    ctx.prof_enable(True)
    ctx.prof_reset()
    st = getattr(ctx._L, name + "_dev")(ctx._h, *[None if p is None else C.c_void_p(p) for p in ptrs], B)
    ctx._check(st)
    ctx.synchronize()
    names = kernel_names(ctx)
    ctx.prof_enable(False)
    return names


class Slab32:
    """The four 32-bit Open calls on device buffers with guarded outputs; inputs are numpy int32 arrays."""

    def __init__(self, torch, ctx):
        self.T, self.ctx = torch, ctx
        self.names = []

    def commit(self, x, r, y):
        T, c = self.T, self.ctx
        B = x.shape[0]
        cm, t = Guarded(T, (B, c.n + c.l, c.N), T.int32), Guarded(T, (B, c.n, c.N), T.int32)
        ok = Guarded(T, (B,), T.uint8)
        ins = [dev(T, a) for a in (x, r, y)]
        self.names = raw(c, "rzk_open_commit32_batch", [a.data_ptr() for a in ins] + [cm.ptr(), t.ptr(), ok.ptr()], B)
        return cm.take(), t.take(), ok.take()

    def response(self, y, r, d):
        T, c = self.T, self.ctx
        B = y.shape[0]
        z = Guarded(T, (B, c.k, c.N), T.int32)
        ins = [dev(T, a) for a in (y, r, d)]
        self.names = raw(c, "rzk_open_response32_batch", [a.data_ptr() for a in ins] + [z.ptr()], B)
        return z.take()

    def verify(self, z, t, cm, d):
        T, c = self.T, self.ctx
        B = z.shape[0]
        acc = Guarded(T, (B,), T.uint8)
        ins = [dev(T, a) for a in (z, t, cm, d)]
        self.names = raw(c, "rzk_open_verify32_batch", [a.data_ptr() for a in ins] + [acc.ptr()], B)
        return acc.take()

    def recover(self, z, cm, d):
        T, c = self.T, self.ctx
        B = z.shape[0]
        t = Guarded(T, (B, c.n, c.N), T.int32)
        acc = Guarded(T, (B,), T.uint8)
        ins = [dev(T, a) for a in (z, cm, d)]
        self.names = raw(c, "rzk_open_recover32_batch", [a.data_ptr() for a in ins] + [t.ptr(), acc.ptr()], B)
        return t.take(), acc.take()


def n32(a):
    """narrow on the host for canonical test data (the library's narrow is tested against it below)."""
    assert int(np.abs(a).max(initial=0)) <= HALF
    return np.ascontiguousarray(a.astype(np.int32))


def w64(a):
    return np.ascontiguousarray(a.astype(np.int64))


def honest(rng, P, B):
    """The usual honest inputs: x uniform, r small, y Gaussian at sigma, d a challenge."""
    x = synth.uniform(rng, (B, P.l, P.N))
    r = synth.small(rng, (B, P.k, P.N), P.b)
    y = synth.gauss(rng, (B, P.k, P.N), P.sigma)
    d = synth.challenge(rng, (B,), P.N, P.kappa)
    return x, r, y, d


def assert_path(names, native, family=None, outputs=True):
    """native: every launch of the call is a 32-bit instantiation (of `family`); convert: widen launches, then the 64-bit
    kernels, then (calls with slab outputs) narrow launches."""
    assert names, "the call launched nothing"
    if native:
        assert all(nm.endswith(", i32>") for nm in names), names
        if family:
            assert all(nm.startswith(family + "<") for nm in names), names
        return
    assert names[0] == "widen_kernel" and not any("i32" in nm for nm in names), names
    inner = [nm for nm in names if nm not in ("widen_kernel", "narrow_kernel")]
    assert inner, names
    first, last = names.index(inner[0]), len(names) - 1 - names[::-1].index(inner[-1])
    assert all(nm == "widen_kernel" for nm in names[:first]), names
    assert all(nm == "narrow_kernel" for nm in names[last + 1:]), names
    assert (len(names) - 1 - last > 0) == outputs, names


def check_cycle(torch, ctx, A, B, rng, native, oracle_entries=None):
    """commit, response, verify, recover in both widths on the same values, against each other and the oracle."""
    P = P_of(ctx)
    N = ctx.N
    fam_units = "unit_io_kernel" if N == 512 else "unit_kernel"
    s32 = Slab32(torch, ctx)
    ents = list(range(B)) if oracle_entries is None else oracle_entries
    x, r, y, d = honest(rng, P, B)
    # commit
    c, t, ok = ctx.open_commit(x, r, y)
    c32, t32, ok32 = s32.commit(n32(x), n32(r), n32(y))
    assert_path(s32.names, native, fam_units)
    assert np.array_equal(c32, n32(c)) and np.array_equal(t32, n32(t)) and np.array_equal(ok32, ok)
    for e in ents:
        c_ref, t_ref, ok_ref = O.open_commit(P, A, x[e], r[e], y[e])
        assert np.array_equal(w64(c32[e]), c_ref) and np.array_equal(w64(t32[e]), t_ref) and int(ok32[e]) == int(ok_ref), e
    # response
    z = ctx.open_response(y, r, d)
    z32 = s32.response(n32(y), n32(r), n32(d))
    assert_path(s32.names, native, "shift_row_kernel")
    assert np.array_equal(z32, n32(z))
    for e in ents:
        assert np.array_equal(w64(z32[e]), O.open_response(P, y[e], r[e], d[e])), e
    # verify: honest proofs, then one batch whose c and t hold +-HALF.  Even entries: c1 gets +-HALF and t is recomputed for
    # it (accepted); odd entries: t gets +-HALF (rejected).
    acc = ctx.open_verify(z, t, c, d)
    acc32 = s32.verify(z32, t32, c32, n32(d))
    assert_path(s32.names, native, fam_units, outputs=False)
    assert np.array_equal(acc32, acc) and acc.all()
    for e in ents:
        assert O.open_verify(P, A, z[e], t[e], c[e], d[e]) == 1, e
    ce, te = c.copy(), t.copy()
    for e in range(B):
        j = (37 * e + 5) % N
        if e % 2 == 0:
            ce[e, 0, j], ce[e, 0, (j + 64) % N] = HALF, -HALF
        else:
            te[e, 0, j], te[e, 0, (j + 64) % N] = HALF, -HALF
    te_rec, _ = ctx.open_recover(z, ce, d)
    te[0::2] = te_rec[0::2]
    acc_e = ctx.open_verify(z, te, ce, d)
    acc_e32 = s32.verify(z32, n32(te), n32(ce), n32(d))
    assert np.array_equal(acc_e32, acc_e)
    assert acc_e[0::2].all() and not acc_e[1::2].any()
    for e in ents:
        assert int(O.open_verify(P, A, z[e], te[e], ce[e], d[e]) == 1) == int(acc_e32[e]), e
    # recover
    tr, accr = ctx.open_recover(z, ce, d)
    tr32, accr32 = s32.recover(z32, n32(ce), n32(d))
    assert_path(s32.names, native, fam_units)
    assert np.array_equal(tr32, n32(tr)) and np.array_equal(accr32, accr) and accr.all()
    t0, _ = s32.recover(z32, c32, n32(d))
    assert np.array_equal(t0, t32), "an honest proof recovers its own t"


# ---- parity on the native kernels ----------------------------------------------------------------------------------------
NATIVE_CTX = {
    "default": ({}, False, (1, 5)),
    "upt64": ({"RZK_UPT": 64}, False, (1, 5)),                                     # all units of a proof on one wavefront
    "upt64-fill": ({"RZK_UPT": 64, "RZK_PRESET_IN_KERNEL": 0}, False, (1, 5)),     # ... with the flags preset by a fill launch
    "trusted": ({}, True, (1, 5)),
    "grid1": ({"RZK_GRID_CUS": 1}, False, (100,)),                                 # several grid-stride trips
}


@pytest.mark.parametrize("kind", list(NATIVE_CTX))
@pytest.mark.parametrize("N", [512, 1024])
def test_parity_native(torch_mod, N, kind):
    env, trusted, batches = NATIVE_CTX[kind]
    ctx = make_ctx(N, 1, 3, 1, env=env)
    rng = np.random.default_rng(51000 + N + len(kind))
    A = synth.key(rng, N, 1, 3, 1)
    ctx.load_key(A)
    if trusted:
        ctx.trust_device_outputs(True)
    for B in batches:
        check_cycle(torch_mod, ctx, A, B, rng, native=True, oracle_entries=None if B <= 5 else [0, 1, 49, 98, 99])


# ---- the convert path --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,shape,B", [(64, (1, 3, 1), 3), (2048, (1, 3, 1), 3), (1024, (2, 5, 2), 3)],
                         ids=["small-64", "pair-2048", "groups-1024"])
def test_convert_path(torch_mod, N, shape, B):
    n, k, l = shape
    ctx = make_ctx(N, n, k, l)
    rng = np.random.default_rng(52000 + N + n)
    A = synth.key(rng, N, n, k, l)
    ctx.load_key(A)
    check_cycle(torch_mod, ctx, A, B, rng, native=False)


# ---- verdict edges in the new kernels ---------------------------------------------------------------------------------------
def valid_proof(ctx, A, rng):
    """One honest proof (z, t, c, d) from the 64-bit calls, accepted by the oracle."""
    P = P_of(ctx)
    x, r, y, d = honest(rng, P, 1)
    c, t, ok = ctx.open_commit(x, r, y)
    z = ctx.open_response(y, r, d)
    assert ok.all() and O.open_verify(P, A, z[0], t[0], c[0], d[0]) == 1
    return z[0], t[0], c[0], d[0]


RANGE_FAULTS = [HALF + 1, -HALF - 1, I32_MAX, I32_MIN]


@pytest.mark.parametrize("N", [512, 1024])
def test_verifier_position_sweep(torch_mod, N):
    """B = N entries, entry i with one fault at coefficient i, the carrying row cycling, one entry in eight clean, two
    passes that together fault every coefficient; the faults cycle through the four range violations an int32 can hold.
    Then +-1 on t: the zero test.  Only the faulted proofs reject, the call succeeds, and the verdicts are those of the
    64-bit call on the widened data."""
    ctx = make_ctx(N, 1, 3, 1)
    rng = np.random.default_rng(53000 + N)
    A = synth.key(rng, N, 1, 3, 1)
    ctx.load_key(A)
    s32 = Slab32(torch_mod, ctx)
    z0, t0, c0, d0 = valid_proof(ctx, A, rng)
    base = {"z": z0, "t": t0, "c": c0, "d": d0}
    rows = {"z": ctx.k, "t": ctx.n, "c": ctx.n}     # Open's verifier reads only the first n rows of c
    for op, pass_ in [(o, p) for o in ("z", "t", "c") for p in (0, 1)] + [("t1", 0), ("t1", 1)]:
        zero_test = op == "t1"
        name = "t" if zero_test else op
        slabs = {key: np.broadcast_to(n32(v), (N,) + v.shape).copy() for key, v in base.items()}
        ent, row, coef = synth.sweep_faults(N, rows[name], pass_)
        if zero_test:
            vals = slabs[name][ent, row, coef].astype(np.int64) + np.where(ent % 2 == 0, 1, -1)
            vals = np.clip(vals, I32_MIN, I32_MAX)
        else:
            vals = np.array([RANGE_FAULTS[i % 4] for i in range(len(ent))], dtype=np.int64)
        slabs[name][ent, row, coef] = vals.astype(np.int32)
        want = ctx.open_verify(*[w64(slabs[key]) for key in ("z", "t", "c", "d")])
        got = s32.verify(slabs["z"], slabs["t"], slabs["c"], slabs["d"])
        assert_path(s32.names, True, outputs=False)
        assert np.array_equal(got, want), (op, pass_, np.flatnonzero(got != want)[:8])
        clean = np.ones(N, dtype=bool)
        clean[ent] = False
        assert got[clean].all() and not got[ent].any(), (op, pass_)
        if not zero_test:   # recover decides the range test (not the relation) with the same loads: t is its output
            if name != "t":
                _, acc64 = ctx.open_recover(w64(slabs["z"]), w64(slabs["c"]), w64(slabs["d"]))
                _, acc32 = s32.recover(slabs["z"], slabs["c"], slabs["d"])
                assert np.array_equal(acc32, acc64) and acc32[clean].all() and not acc32[ent].any(), (op, pass_)


@pytest.mark.parametrize("N", [512, 1024])
def test_alias_of_half_is_rejected_unless_trusted(torch_mod, N):
    """A coefficient first set to HALF, then replaced by HALF - q: the same residue, an int32 value, not canonical.  t is
    recomputed for the HALF, so the relation holds for both: only the range test can tell them apart.  Trusted mode skips
    the range test and accepts."""
    for trusted in (False, True):
        ctx = make_ctx(N, 1, 3, 1)
        rng = np.random.default_rng(54000 + N)
        A = synth.key(rng, N, 1, 3, 1)
        ctx.load_key(A)
        s32 = Slab32(torch_mod, ctx)
        z0, t0, c0, d0 = valid_proof(ctx, A, rng)
        B = 64
        z, c, d = (np.broadcast_to(v, (B,) + v.shape).copy() for v in (z0, c0, d0))
        pos = [(17 * e + (e // 8) * 64) % N for e in range(B)]
        c[np.arange(B), 0, pos] = HALF
        t, acc = ctx.open_recover(z, c, d)
        assert acc.all() and ctx.open_verify(z, t, c, d).all()
        z32, t32, c32, d32 = n32(z), n32(t), n32(c), n32(d)
        faulted = np.arange(B) % 4 != 3
        c32[np.flatnonzero(faulted), 0, np.array(pos)[faulted]] = HALF - Q
        assert HALF - Q >= I32_MIN
        if trusted:
            ctx.trust_device_outputs(True)
        want = ctx.open_verify(z, t, w64(c32), d)
        got = s32.verify(z32, t32, c32, d32)
        assert_path(s32.names, True, outputs=False)
        assert np.array_equal(got, want)
        assert got.all() if trusted else (got[~faulted].all() and not got[faulted].any())
        tr, accr = s32.recover(z32, c32, d32)
        assert np.array_equal(accr, got)
        if trusted:
            assert np.array_equal(tr, t32)


@pytest.mark.parametrize("N", [512, 1024])
def test_prover_side_faults_fail_the_call(torch_mod, N):
    ctx = make_ctx(N, 1, 3, 1)
    rng = np.random.default_rng(55000 + N)
    A = synth.key(rng, N, 1, 3, 1)
    ctx.load_key(A)
    P = P_of(ctx)
    s32 = Slab32(torch_mod, ctx)
    B = 3
    x, r, y, d = (n32(a) for a in honest(rng, P, B))
    trial = 0
    for call, ops in (("commit", (x, r, y)), ("response", (y, r, d))):
        for i in range(len(ops)):
            for val in RANGE_FAULTS + [HALF - Q]:
                args = [a.copy() for a in ops]
                flat = args[i].reshape(B, -1)
                flat[trial % B, (trial * 67 + (0, 63, 64, N - 1)[trial % 4]) % flat.shape[1]] = val
                trial += 1
                with pytest.raises(RzkError) as ei:
                    getattr(s32, call)(*args)
                assert ei.value.status == RZK_E_ARG, (call, i, val)
                getattr(s32, call)(*ops)   # the sticky word was consumed: the next clean call succeeds
    ctx.trust_device_outputs(True)
    bad = y.copy()
    bad[1, 2, 65] = HALF - Q
    z = s32.response(bad, r, d)          # trusted mode: no test; the low word is what the kernel computes with
    assert np.array_equal(z, n32(ctx.open_response(w64(bad), w64(r), w64(d))))


@pytest.mark.parametrize("N", [512, 1024])
def test_norm_edge_on_z(torch_mod, N):
    """synth.norm_edge at L - 1, L, L + 1 (synth.norm_plan), weight at a point (positions 0, 63, 64, N - 3) and spread over
    all coefficients, in every row of z in turn; the relation holds (c = 0, t = a1.z), so the verdict is the oracle's
    check_norm of the crafted row."""
    ctx = make_ctx(N, 1, 3, 1)
    P = P_of(ctx)
    rng = np.random.default_rng(56000 + N)
    A = synth.key(rng, N, 1, 3, 1)
    ctx.load_key(A)
    plan = synth.norm_plan((P.verify_bound + 1) ** 2)
    polys = []
    for name in ("below", "at", "above"):
        for style, pos in [("point", p) for p in (0, 63, 64, N - 3)] + [("spread", 0)]:
            p = synth.norm_edge(N, plan[name], style, pos, rng)
            polys.append((f"{name}/{style}@{pos}", p, int(O.check_norm(p[None], P.verify_bound))))
    assert [w for _, _, w in polys] == [1] * 5 + [0] * 10
    places = [(i, j) for i in range(len(polys)) for j in range(ctx.k)]
    z, t, c, d, want = open_entries(ctx, A, polys, places, rng)
    s32 = Slab32(torch_mod, ctx)
    got = s32.verify(n32(z), n32(t), n32(c), n32(d))
    assert_path(s32.names, True, outputs=False)
    bad = [(polys[places[e][0]][0], places[e][1]) for e in range(len(places)) if int(got[e]) != want[e]]
    assert not bad, bad
    assert np.array_equal(got, ctx.open_verify(z, t, c, d))
    tr, accr = s32.recover(n32(z), n32(c), n32(d))
    assert np.array_equal(accr, got) and np.array_equal(tr[got == 1], n32(t)[got == 1])


# ---- narrow / widen, argument rules -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [64, 1024])
def test_narrow_widen_round_trip(torch_mod, N):
    torch = torch_mod
    ctx = make_ctx(N, 1, 3, 1)
    rng = np.random.default_rng(57000 + N)
    a = synth.uniform(rng, (7, 3, N))
    a[0, 0, :4] = [HALF, -HALF, 0, -1]
    for arr in (a, dev(torch, a)):                      # host and device forms
        nar = ctx.narrow(arr)
        back = ctx.widen(nar)
        ctx.synchronize()
        nar_h, back_h = (v.cpu().numpy() if hasattr(v, "cpu") else v for v in (nar, back))
        assert nar_h.dtype == np.int32 and np.array_equal(nar_h, a.astype(np.int32)) and np.array_equal(back_h, a)
    for val in (HALF + 1, -HALF - 1, 2 ** 32 + 5, HALF - Q):
        bad = a.copy()
        bad[3, 1, N - 1] = val
        with pytest.raises(RzkError) as ei:
            ctx.narrow(bad)                              # host form: reports its own input fault
        assert ei.value.status == RZK_E_ARG
        ctx.narrow(dev(torch, bad))                      # device form: the sticky condition
        with pytest.raises(RzkError):
            ctx.synchronize()
    ctx.trust_device_outputs(True)                       # trusted-producer mode: no test
    bad = a.copy()
    bad[3, 1, N - 1] = 2 ** 32 + 5
    assert int(ctx.narrow(bad)[3, 1, N - 1]) == 5


def test_argument_rules(torch_mod):
    torch = torch_mod
    N = 512
    ctx = make_ctx(N, 1, 3, 1)
    rng = np.random.default_rng(58000)
    ctx.load_key(synth.key(rng, N, 1, 3, 1))
    L, h = ctx._L, ctx._h
    B = 2
    buf = torch.zeros(B * 3 * N + 16, dtype=torch.int32, device="cuda")
    wide = torch.zeros(B * 3 * N + 16, dtype=torch.int64, device="cuda")
    flags = torch.zeros(16, dtype=torch.uint8, device="cuda")
    p, w, f = buf.data_ptr(), wide.data_ptr(), flags.data_ptr()
    calls = {
        "rzk_narrow_batch_dev": [w, p],
        "rzk_widen_batch_dev": [p, w],
        "rzk_open_commit32_batch_dev": [p, p, p, p, p, f],
        "rzk_open_response32_batch_dev": [p, p, p, p],
        "rzk_open_verify32_batch_dev": [p, p, p, p, f],
        "rzk_open_recover32_batch_dev": [p, p, p, p, f],
    }
    for name, ptrs in calls.items():
        fn = getattr(L, name)
        slabs = len(ptrs) - (1 if ptrs[-1] == f else 0)
        assert fn(h, *[None] * len(ptrs), 0) == 0, name                     # B == 0: a no-op, pointers may be NULL
        for i in range(slabs):
            nul = [C.c_void_p(q) for q in ptrs]
            nul[i] = None
            assert fn(h, *nul, B) == RZK_E_ARG, (name, "NULL", i)
            off = [C.c_void_p(q) for q in ptrs]
            off[i] = C.c_void_p(ptrs[i] + 8)                                 # element-aligned for both widths, not 16-byte
            assert fn(h, *off, B) == RZK_E_ARG, (name, "misaligned", i)
    ctx.synchronize()
    # the 64-bit methods keep rejecting int32, the 32-bit ones int64
    y = np.zeros((B, 3, N), dtype=np.int32)
    d = np.zeros((B, N), dtype=np.int32)
    with pytest.raises(ValueError):
        ctx.open_response(y, y, d)
    with pytest.raises(ValueError):
        ctx.open_response32(w64(y), w64(y), w64(d))


# ---- a whole cycle through the Python methods ----------------------------------------------------------------------------------
def test_whole_cycle_32(torch_mod):
    """commit32 -> response32 -> verify32 on device tensors accepts every honest proof at N = 1024, B = 5 (the outputs of
    one call feed the next, nothing is widened); flipping one coefficient of z, t or c1 rejects that proof alone.  The
    host-pointer forms give the same bytes."""
    torch = torch_mod
    N, B = 1024, 5
    ctx = make_ctx(N, 1, 3, 1)
    P = P_of(ctx)
    rng = np.random.default_rng(59000)
    A = synth.key(rng, N, 1, 3, 1)
    ctx.load_key(A)
    x, r, y, d = (n32(a) for a in honest(rng, P, B))
    dx, dr, dy, dd = (dev(torch, a) for a in (x, r, y, d))
    c, t, ok = ctx.open_commit32(dx, dr, dy)
    z = ctx.open_response32(dy, dr, dd)
    acc = ctx.open_verify32(z, t, c, dd)
    t2, acc2 = ctx.open_recover32(z, c, dd)
    ctx.synchronize()
    assert c.dtype == torch.int32 and z.dtype == torch.int32
    assert bool(ok.all()) and bool(acc.all()) and bool(acc2.all()) and bool((t2 == t).all())
    for e in range(B):
        assert O.open_verify(P, A, w64(z[e].cpu().numpy()), w64(t[e].cpu().numpy()), w64(c[e].cpu().numpy()), w64(d[e])) == 1
    for which, e, idx in (("z", 1, (2, 700)), ("t", 2, (0, 63)), ("c", 4, (0, 1023))):
        zz, tt, cc = z.clone(), t.clone(), c.clone()
        tgt = {"z": zz, "t": tt, "c": cc}[which]
        tgt[(e,) + idx] += 1 if int(tgt[(e,) + idx]) < HALF else -1
        got = ctx.open_verify32(zz, tt, cc, dd).cpu().numpy()
        assert [int(v) for v in got] == [int(i != e) for i in range(B)], which
    # host-pointer forms
    ch, th, okh = ctx.open_commit32(x, r, y)
    zh = ctx.open_response32(y, r, d)
    assert np.array_equal(ch, c.cpu().numpy()) and np.array_equal(th, t.cpu().numpy()) and np.array_equal(zh, z.cpu().numpy())
    assert ctx.open_verify32(zh, th, ch, d).all() and okh.all()
    th2, acch = ctx.open_recover32(zh, ch, d)
    assert np.array_equal(th2, th) and acch.all()
