"""The zero-knowledge Open prover on 32-bit slabs (include/rzk.h "slab32 prover") on the GPU.

  * samplers: rzk_sample_*_keyed32_dev equals its 64-bit sibling converted, exactly, under the same key, nonce and stream:
    partly idle last workgroups, the challenge kernel past one trip, dgauss tiles cut by the end of the call and spanning
    polynomials, two grid-stride trips, the extremes of every accepted argument, the argument rules, the kernel names;
  * matvec32: narrow(matvec) and the oracle, native (N = 512 / 1024) and converted, the prover-side input faults;
  * open_response_reject32: z, accept, E byte for byte the sibling's, and tests/reject_ref.py through the helpers of
    test_gpu_response_reject.py; native and converted; trusted mode; one cause per edge case;
  * the prover: open_prove_zk32 under KeyedSampler32 equals open_prove_zk under KeyedSampler converted, every proof verifies,
    and the 32-bit run launches no convert kernel and no kernel without the i32 mark.
Every 32-bit output lives in a device buffer with guard words on both sides (Guarded, test_gpu_slab32.py)."""
import ctypes as C

import numpy as np
import pytest

import reject_ref as RR
from oracle import oracle as O
from ring_zk_amd import _lib, RzkError, synth
from ring_zk_amd import fiat_shamir as FS
from ring_zk_amd.backend import ExactKeyedSampler, ExactKeyedSampler32, KeyedSampler, KeyedSampler32
from test_gpu_baseline_shapes import P_of, dev, make_ctx, torch_mod  # noqa: F401
from test_gpu_fiat_shamir import keyed_ctx
from test_gpu_response_reject import LNM, R62, compare, ctx_of, inputs
from test_gpu_slab32 import Guarded, I32_MAX, I32_MIN, kernel_names

pytestmark = pytest.mark.gpu

Q_MAX = 4294606851
KEY = bytes(range(100, 132))
AUX = bytes(range(60, 92))
RZK_E_ARG = _lib.RZK_E_ARG


def nonce_of(i):
    return (C.c_uint8 * 16).from_buffer_copy(int(i).to_bytes(16, "little"))


def profiled(ctx, call):
    """names of the launches of call(); the sticky input fault of a prover-side call surfaces in synchronize()"""
    ctx._bind_torch_stream()
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        call()
        ctx.synchronize()
        return kernel_names(ctx)
    finally:
        ctx.prof_enable(False)


def n32(a):
    return np.ascontiguousarray(a.astype(np.int32))


def w64(a):
    return np.ascontiguousarray(a.astype(np.int64))


# ---- samplers -------------------------------------------------------------------------------------------------------------
SAMPLER_NAMES = {"uniform": "sample_uniform_chacha_kernel", "dgauss": "sample_dgauss_chacha_kernel",
                 "challenge": "sample_challenge_chacha_kernel"}


def sampler_pair(torch, ctx, kind, arg, npoly, nonce=7, stream=3):
    """(64-bit output, 32-bit output, names of the 64-bit launch, names of the 32-bit launch) of one draw in both widths"""
    N = ctx.N
    wide, nar = Guarded(torch, (npoly, N), torch.int64), Guarded(torch, (npoly, N), torch.int32)
    count = npoly * N if kind == "dgauss" else npoly
    head = (ctx._h, nonce_of(nonce), stream) + (() if kind == "challenge" else (arg,))
    f64 = getattr(ctx._L, "rzk_sample_%s_keyed_dev" % kind)
    f32 = getattr(ctx._L, "rzk_sample_%s_keyed32_dev" % kind)
    names64 = profiled(ctx, lambda: ctx._check(f64(*head, C.c_void_p(wide.ptr()), count)))
    names32 = profiled(ctx, lambda: ctx._check(f32(*head, C.c_void_p(nar.ptr()), count)))
    return wide.take(), nar.take(), names64, names32


def check_sampler(torch, ctx, kind, arg, npoly, **kw):
    a64, a32, names64, names32 = sampler_pair(torch, ctx, kind, arg, npoly, **kw)
    assert int(np.abs(a64).max()) < 2 ** 31
    assert np.array_equal(w64(a32), a64), (kind, arg, npoly, np.argwhere(w64(a32) != a64)[:4])
    if kind == "gauss":
        form = "true" if arg < 524288.0 else "false"
        assert names64 == ["sample_gauss_chacha_kernel<%s>" % form] and names32 == ["sample_gauss_chacha_kernel_i32<%s>" % form]
    else:
        assert names64 == [SAMPLER_NAMES[kind]] and names32 == [SAMPLER_NAMES[kind] + "_i32"]
    return a64


def sampler_ctx(N, env=None, q=O.Q_DEFAULT):
    ctx = make_ctx(N, 1, 3, 1, env=env, kappa=min(N, 36), q=q)
    ctx.set_sampler_key(KEY)
    return ctx


@pytest.mark.parametrize("N", [4, 64, 512, 1024])
def test_samplers_equal_their_siblings(torch_mod, N):
    """5 and 70 polynomials: the last workgroup is partly idle in both, 70 is more than the 64 polynomials of one trip of the
    challenge kernel; N = 64 x 5 is a dgauss tile spanning polynomials (160 pairs, tiles of 128)."""
    ctx = sampler_ctx(N)
    for npoly in (5, 70):
        u = check_sampler(torch_mod, ctx, "uniform", ctx.half, npoly)
        assert int(np.abs(u).max()) > ctx.half // 2 or N * npoly < 64
        check_sampler(torch_mod, ctx, "uniform", 1, npoly, nonce=8)
        check_sampler(torch_mod, ctx, "gauss", float(ctx.sigma), npoly)            # the single-precision form
        check_sampler(torch_mod, ctx, "gauss", 3.0e6, npoly, nonce=9)              # the double-precision form
        check_sampler(torch_mod, ctx, "dgauss", int(ctx.sigma), npoly)
        d = check_sampler(torch_mod, ctx, "challenge", None, npoly)
        assert (np.abs(d).sum(axis=-1) == ctx.kappa).all() and int(np.abs(d).max()) == 1


def test_dgauss_tile_cut_by_the_end_of_the_call(torch_mod):
    ctx = sampler_ctx(4)
    check_sampler(torch_mod, ctx, "dgauss", 1000, 3)      # 6 pairs of a 128-pair tile


def test_challenge_shapes(torch_mod):
    ctx = sampler_ctx(64)
    assert ctx.kappa == 36
    check_sampler(torch_mod, ctx, "challenge", None, 5)
    ctx4 = sampler_ctx(4)
    assert ctx4.kappa == 4
    check_sampler(torch_mod, ctx4, "challenge", None, 5)


def test_samplers_two_grid_stride_trips(torch_mod):
    """One CU's grid: 16 workgroups of 64 quads = 8192 coefficients per trip of uniform / gauss, 32 tiles of 256 coefficients
    per trip of dgauss, 64 polynomials per trip of challenge."""
    ctx = sampler_ctx(1024, env={"RZK_GRID_CUS": 1})
    check_sampler(torch_mod, ctx, "uniform", ctx.half, 20)
    check_sampler(torch_mod, ctx, "gauss", float(ctx.sigma), 20)
    check_sampler(torch_mod, ctx, "dgauss", int(ctx.sigma), 20)
    ctx64 = sampler_ctx(64, env={"RZK_GRID_CUS": 1})
    check_sampler(torch_mod, ctx64, "challenge", None, 70)


def test_sampler_extremes(torch_mod):
    big = sampler_ctx(512, q=Q_MAX)
    u = check_sampler(torch_mod, big, "uniform", (Q_MAX - 1) // 2, 70)
    assert int(np.abs(u).max()) > 2 ** 30                                   # values that need bit 30 of an int32
    ctx = sampler_ctx(512)
    g = check_sampler(torch_mod, ctx, "gauss", 67108864.0, 70)
    assert int(np.abs(g).max()) > 2 ** 27
    check_sampler(torch_mod, ctx, "gauss", 524287.96875, 70)               # the largest float below 2^19
    ctx4 = sampler_ctx(4)
    g = check_sampler(torch_mod, ctx4, "dgauss", 1 << 26, 70)
    assert int(np.abs(g).max()) > 2 ** 26


def test_sampler_argument_rules(torch_mod):
    torch = torch_mod
    ctx = sampler_ctx(64)
    L, h, N = ctx._L, ctx._h, ctx.N
    out = Guarded(torch, (2, N), torch.int32)
    p, nn = C.c_void_p(out.ptr()), nonce_of(1)
    calls = {
        "uniform": lambda o, n_, cnt=2: L.rzk_sample_uniform_keyed32_dev(h, n_, 0, 5, o, cnt),
        "gauss": lambda o, n_, cnt=2: L.rzk_sample_gauss_keyed32_dev(h, n_, 0, 100.0, o, cnt),
        "dgauss": lambda o, n_, cnt=2 * N: L.rzk_sample_dgauss_keyed32_dev(h, n_, 0, 100, o, cnt),
        "challenge": lambda o, n_, cnt=2: L.rzk_sample_challenge_keyed32_dev(h, n_, 0, o, cnt),
    }
    ctx._bind_torch_stream()
    for kind, call in calls.items():
        assert call(p, nn) == 0, kind
        assert call(C.c_void_p(out.ptr() + 8), nn) == RZK_E_ARG, (kind, "misaligned out")
        assert call(None, nn) == RZK_E_ARG, (kind, "NULL out")
        assert call(p, None) == RZK_E_ARG, (kind, "NULL nonce")
        before = out.take().copy()
        assert call(None, None, 0) == 0, (kind, "count == 0 is a no-op")
        ctx.synchronize()
        assert np.array_equal(out.take(), before)
    # the siblings' range rules
    assert L.rzk_sample_uniform_keyed32_dev(h, nn, 0, ctx.half + 1, p, 2) == RZK_E_ARG
    assert L.rzk_sample_uniform_keyed32_dev(h, nn, 0, 0, p, 2) == RZK_E_ARG
    assert L.rzk_sample_gauss_keyed32_dev(h, nn, 0, 67108865.0, p, 2) == RZK_E_ARG
    assert L.rzk_sample_gauss_keyed32_dev(h, nn, 0, 0.0, p, 2) == RZK_E_ARG
    assert L.rzk_sample_dgauss_keyed32_dev(h, nn, 0, (1 << 26) + 1, p, 2 * N) == RZK_E_ARG
    assert L.rzk_sample_dgauss_keyed32_dev(h, nn, 0, 100, p, 2 * N - 1) == RZK_E_ARG
    ctx.set_sampler_key(None)
    for kind, call in calls.items():
        assert call(p, nn) == RZK_E_ARG, (kind, "no key set")
    ctx.synchronize()
    out.take()


def test_keyed_sampler32_consumes_nonces_like_keyed_sampler(torch_mod):
    ctx = sampler_ctx(64)
    for cls64, cls32 in ((KeyedSampler, KeyedSampler32), (ExactKeyedSampler, ExactKeyedSampler32)):
        a, b = cls64(ctx, KEY, 40), cls32(ctx, KEY, 40)
        for draw in (lambda s: s.uniform(5, (3, 2)), lambda s: s.gauss(ctx.sigma, (3,)), lambda s: s.challenge((2,)),
                     lambda s: s.uniform(ctx.half, (1,))):
            x64, x32 = draw(a), draw(b)
            assert a.counter == b.counter
            assert x32.dtype == torch_mod.int32 and torch_mod.equal(x32.to(torch_mod.int64), x64)


# ---- matvec32 ---------------------------------------------------------------------------------------------------------------
def matvec32(torch, ctx, which, v, addend):
    """rzk_matvec32_batch_dev on guarded device buffers: (out, names)"""
    B = v.shape[0]
    rows = ctx._rows(which)
    out = Guarded(torch, (B, rows, ctx.N), torch.int32)
    dv, da = dev(torch, v), None if addend is None else dev(torch, addend)
    names = profiled(ctx, lambda: ctx._check(ctx._L.rzk_matvec32_batch_dev(
        ctx._h, which, C.c_void_p(dv.data_ptr()), None if da is None else C.c_void_p(da.data_ptr()), C.c_void_p(out.ptr()), B)))
    return out.take(), names


def check_matvec(torch, ctx, A, rng, B, native, oracle=True):
    P = P_of(ctx)
    N, n, k = ctx.N, ctx.n, ctx.k
    for which in (0, 1, 2):
        rows = ctx._rows(which)
        key = {0: A[:n], 1: A[n:], 2: A}[which]
        for with_add in (False, True):
            v = synth.uniform(rng, (B, k, N))
            v[0, 0, 0], v[B - 1, k - 1, N - 1] = ctx.half, -ctx.half          # +-h stays valid
            add = synth.uniform(rng, (B, rows, N)) if with_add else None
            if with_add:
                add[0, 0, 0], add[B - 1, rows - 1, N - 1] = -ctx.half, ctx.half
            want = ctx.matvec(which, v, add)
            got, names = matvec32(torch, ctx, which, n32(v), None if add is None else n32(add))
            assert np.array_equal(got, n32(want)), (which, with_add)
            if native:
                assert names and all(nm.endswith("i32>") for nm in names), names
            else:
                assert "widen_kernel" in names and "narrow_kernel" in names and not any("i32" in nm for nm in names), names
            if oracle:
                for e in sorted({0, B - 1}):
                    ref = O.mat_dot(key, v[e][:, None, :], P.q)[:, 0, :]
                    if with_add:
                        ref = O.mat_add(ref[:, None, :], add[e][:, None, :], P.q)[:, 0, :]
                    assert np.array_equal(w64(got[e]), ref), (which, with_add, e)


@pytest.mark.parametrize("N", [512, 1024])
def test_matvec32_native(torch_mod, N):
    ctx, A = keyed_ctx(N, 1, 3, 1, 36, seed=61000 + N)
    rng = np.random.default_rng(61100 + N)
    for B in (1, 5):
        check_matvec(torch_mod, ctx, A, rng, B, native=True)
    ctx1, A1 = keyed_ctx(N, 1, 3, 1, 36, seed=61000 + N, env={"RZK_GRID_CUS": 1})
    check_matvec(torch_mod, ctx1, A1, rng, 100, native=True)


@pytest.mark.parametrize("N,shape", [(64, (1, 3, 1)), (2048, (1, 3, 1)), (1024, (2, 5, 2))], ids=["small-64", "pair-2048", "groups-1024"])
def test_matvec32_convert(torch_mod, N, shape):
    ctx, A = keyed_ctx(N, *shape, 36, seed=62000 + N)
    check_matvec(torch_mod, ctx, A, np.random.default_rng(62100 + N), 5, native=False)


@pytest.mark.parametrize("N", [512, 64])
def test_matvec32_input_faults(torch_mod, N):
    """Prover side and sticky, as the sibling: a coefficient outside [-h, h] at the first or last position of v or of the addend
    fails the call (reported by the next synchronising call), in both widths."""
    ctx, A = keyed_ctx(N, 1, 3, 1, 36, seed=63000 + N)
    rng = np.random.default_rng(63100 + N)
    B, k = 3, ctx.k
    v0, add0 = n32(synth.uniform(rng, (B, k, N))), n32(synth.uniform(rng, (B, 1, N)))
    h = ctx.half
    for which_op in ("v", "add"):
        for pos in ("first", "last"):
            for val in (h + 1, -h - 1, I32_MAX, I32_MIN):
                v, add = v0.copy(), add0.copy()
                tgt = v if which_op == "v" else add
                tgt[(0, 0, 0) if pos == "first" else (B - 1, tgt.shape[1] - 1, N - 1)] = val
                with pytest.raises(RzkError) as e32:
                    matvec32(torch_mod, ctx, 0, v, add)
                assert e32.value.status == RZK_E_ARG, (which_op, pos, val)
                ctx.matvec(0, dev(torch_mod, w64(v)), dev(torch_mod, w64(add)))
                with pytest.raises(RzkError) as e64:
                    ctx.synchronize()
                assert e64.value.status == RZK_E_ARG
                matvec32(torch_mod, ctx, 0, v0, add0)       # the sticky word was consumed: the next clean call succeeds


# ---- open_response_reject32 -----------------------------------------------------------------------------------------------
def reject32(torch, ctx, ins, coin, R=R62, lnM=LNM):
    """rzk_open_response_reject32_batch_dev on guarded device buffers; ins = int32 (y, r, d): (z, accept, E, names)"""
    B = ins[0].shape[0]
    z = Guarded(torch, (B, ctx.k, ctx.N), torch.int32)
    acc, E = Guarded(torch, (B,), torch.uint8), Guarded(torch, (B,), torch.int64)
    d_in = [dev(torch, a) for a in ins] + [dev(torch, coin)]
    names = profiled(ctx, lambda: ctx._check(ctx._L.rzk_open_response_reject32_batch_dev(
        ctx._h, *[C.c_void_p(a.data_ptr()) for a in d_in], R, lnM, C.c_void_p(z.ptr()), C.c_void_p(acc.ptr()), C.c_void_p(E.ptr()), B)))
    return z.take(), acc.take(), E.take(), names


def sibling(torch, ctx, ins, coin, R=R62, lnM=LNM):
    z, acc, E = ctx.open_response_reject(*[dev(torch, w64(a)) for a in ins], dev(torch, coin), R, lnM)
    ctx.synchronize()
    return z.cpu().numpy(), acc.cpu().numpy(), E.cpu().numpy()


def check_reject32(torch, ctx, P, ins64, coin, R=R62, lnM=LNM, trusted=False, max_undecidable=2):
    """32-bit call == sibling byte for byte, and both against the reference; returns (reference, accept, E, names)"""
    ins32 = [n32(a) for a in ins64]
    z64, acc64, E64 = sibling(torch, ctx, ins32, coin, R, lnM)
    z, acc, E, names = reject32(torch, ctx, ins32, coin, R, lnM)
    assert np.array_equal(z, n32(z64)) and acc.tobytes() == acc64.tobytes() and E.tobytes() == E64.tobytes()
    want = RR.run(P, [(w64(z), ins64[0])], coin, R, lnM, trusted=trusted)
    compare(want, acc, E, max_undecidable)
    return want, acc, E, names


@pytest.mark.parametrize("N", [512, 1024])
def test_response_reject32_native(torch_mod, N):
    ctx, P = ctx_of(N)
    for B in (1, 3, 5):
        rng = np.random.default_rng(2000 * N + B)               # the seeds of test_open_matches_chain_and_reference
        ins, coin = inputs(rng, ctx, P, "open", B), RR.coins(rng, B, R62)
        want, _, _, names = check_reject32(torch_mod, ctx, P, ins, coin)
        assert all(w[1] == 0 for w in want)
        assert names == ["response_stat_kernel<%d, false, i32>" % (N.bit_length() - 1), "reject_decide_kernel"]


@pytest.mark.parametrize("N,env", [(64, None), (2048, None), (1024, {"RZK_SHIFT": 0}), (1024, {"RZK_SHIFT_BYTES": 0})],
                         ids=["small-64", "pair-2048", "shift0", "shift-bytes0"])
def test_response_reject32_convert(torch_mod, N, env):
    ctx, P = ctx_of(N, env=env)
    B = 3
    rng = np.random.default_rng(2000 * N + B)
    ins, coin = inputs(rng, ctx, P, "open", B), RR.coins(rng, B, R62)
    _, _, _, names = check_reject32(torch_mod, ctx, P, ins, coin)
    fused64 = env == {"RZK_SHIFT_BYTES": 0}                     # the sibling still runs its fused word kernel there
    inner = (["response_stat_kernel<10, false, false>"] if fused64 else None)
    assert names[:3] == ["widen_kernel"] * 3 and names[-1] == "narrow_kernel" and names[-2] == "reject_decide_kernel", names
    assert not any("i32" in nm for nm in names), names
    mid = names[3:-2]
    if inner:
        assert mid == inner, names
    else:
        assert len(mid) >= 2 and mid[-1].startswith("reject_stat_kernel") and not any(nm.startswith("response_stat") for nm in mid), names


def test_response_reject32_grid_stride_trips(torch_mod):
    ctx1, P = ctx_of(512, env={"RZK_GRID_CUS": 1})
    B = 100
    rng = np.random.default_rng(177 + 1)                         # the seed of test_grid_stride_trips[open]
    ins, coin = inputs(rng, ctx1, P, "open", B), RR.coins(rng, B, R62)
    _, _, _, names = check_reject32(torch_mod, ctx1, P, ins, coin)
    assert names[0] == "response_stat_kernel<9, false, i32>"


def test_response_reject32_trusted_mode_gives_identical_bytes(torch_mod):
    ctx, P = ctx_of(1024)
    rng = np.random.default_rng(6)
    ins, coin = inputs(rng, ctx, P, "open", 5), RR.coins(rng, 5, R62)
    ins32 = [n32(a) for a in ins]
    z, acc, E, _ = reject32(torch_mod, ctx, ins32, coin)
    ctx.trust_device_outputs(True)
    _, acc_t, E_t, names = check_reject32(torch_mod, ctx, P, ins, coin, trusted=True)
    z_t, _, _, _ = reject32(torch_mod, ctx, ins32, coin)
    ctx.trust_device_outputs(False)
    assert names == ["response_stat_kernel<10, true, i32>", "reject_decide_kernel"]
    assert acc_t.tobytes() == acc.tobytes() and E_t.tobytes() == E.tobytes() and z_t.tobytes() == z.tobytes()


@pytest.mark.parametrize("N", [512, 1024])
def test_response_reject32_edges_one_cause_each(torch_mod, N):
    ctx, P = ctx_of(N)
    k, B = ctx.k, 5
    rng = np.random.default_rng(99)
    y0, r0, d0 = inputs(rng, ctx, P, "open", B)
    coin0 = np.zeros(B, np.int64)                                # u = 1 / R: every honest proof is accepted
    _, acc, _, _ = check_reject32(torch_mod, ctx, P, [y0, r0, d0], coin0, max_undecidable=0)
    assert acc.tolist() == [1] * B
    # the norm rule at its edge (r = 0: z = y)
    y, r = y0.copy(), r0.copy()
    r[1], r[3] = 0, 0
    y[1, 2], y[3, 0] = RR.norm_edge_poly(P, 0), RR.norm_edge_poly(P, 1)
    want, acc, _, _ = check_reject32(torch_mod, ctx, P, [y, r, d0], coin0, max_undecidable=0)
    assert [w[1] for w in want] == [0, 0, 0, RR.NORM, 0] and acc.tolist() == [1, 1, 1, 0, 1]
    # |v| > kappa b from an r beyond b: through the word rotation (|r| = 200) and on packed bytes (a coefficient 2 of d)
    y, r, d = y0.copy(), r0.copy(), d0.copy()
    r[1] = synth.small(rng, r[1].shape, 1) * 200
    r[2], d[2] = 1, np.where(d[2] != 0, 1, 0)
    d[2, np.nonzero(d[2])[0][0]] = 2
    want, acc, _, _ = check_reject32(torch_mod, ctx, P, [y, r, d], coin0, max_undecidable=0)
    assert [w[1] for w in want] == [0, RR.VMAX, RR.VMAX, 0, 0] and acc.tolist() == [1, 0, 0, 1, 1]
    # a non-canonical coefficient at the first and last position of y, r and d: what the 64-bit call gives on the widened input
    h = P.half
    _, acc_ok, E_ok, _ = reject32(torch_mod, ctx, [n32(a) for a in (y0, r0, d0)], coin0)
    trial = 0
    for which in range(3):
        for last in (False, True):
            for val in (h + 1, -h - 1, I32_MAX, I32_MIN, h - P.q):
                ins = [n32(y0), n32(r0), n32(d0)]
                victim = trial % B
                trial += 1
                where = (victim, k - 1, N - 1) if last else (victim, 0, 0)
                if which == 2:
                    where = (victim, N - 1) if last else (victim, 0)
                ins[which][where] = val
                dz, dacc, dE = ctx.open_response_reject(*[dev(torch_mod, w64(a)) for a in ins], dev(torch_mod, coin0), R62, LNM)
                with pytest.raises(RzkError) as e64:
                    ctx.synchronize()
                assert e64.value.status == RZK_E_ARG
                z = Guarded(torch_mod, (B, k, N), torch_mod.int32)
                a8, E = Guarded(torch_mod, (B,), torch_mod.uint8), Guarded(torch_mod, (B,), torch_mod.int64)
                d_in = [dev(torch_mod, a) for a in ins] + [dev(torch_mod, coin0)]
                ctx._check(ctx._L.rzk_open_response_reject32_batch_dev(
                    ctx._h, *[C.c_void_p(a.data_ptr()) for a in d_in], R62, LNM, C.c_void_p(z.ptr()), C.c_void_p(a8.ptr()),
                    C.c_void_p(E.ptr()), B))
                with pytest.raises(RzkError) as e32:
                    ctx.synchronize()                            # the sticky word, reported once
                assert e32.value.status == RZK_E_ARG, (which, last, val)
                ctx.synchronize()
                got_acc, got_E = a8.take(), E.take()
                z.take()
                assert got_acc.tolist() == dacc.cpu().numpy().tolist() == [int(b != victim) for b in range(B)], (which, last, val)
                others = [b for b in range(B) if b != victim]
                assert np.array_equal(got_E[others], E_ok[others]) and np.array_equal(dE.cpu().numpy()[others], E_ok[others])
    _, acc, _, _ = reject32(torch_mod, ctx, [n32(a) for a in (y0, r0, d0)], coin0)   # the fault does not leak into the next call
    assert acc.tolist() == [1] * B


def test_response_reject32_argument_rules(torch_mod):
    torch = torch_mod
    ctx, P = ctx_of(512)
    L, B, N, k = ctx._L, 2, ctx.N, ctx.k
    rng = np.random.default_rng(3)
    y, r, d = (n32(a) for a in inputs(rng, ctx, P, "open", B))
    coin, acc, E, z = np.zeros(B, np.int64), np.zeros(B, np.uint8), np.zeros(B, np.int64), np.zeros_like(y)
    ctx._bind_torch_stream()
    pad = lambda a: dev(torch, np.concatenate([a.reshape(-1), np.zeros(4, a.dtype)]))   # room for the misaligned view
    host = dict(y=y, r=r, d=d, coin=coin, z=z, acc=acc, E=E)
    devs = {key: pad(a) for key, a in host.items()}
    ptr = lambda a: C.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)
    for fn, a in ((L.rzk_open_response_reject32_batch, host), (L.rzk_open_response_reject32_batch_dev, devs)):
        def call(R=R62, lnM=LNM, B_=B, shift=None, **null):
            g = lambda key: None if key in null else (C.c_void_p(ptr(a[key]).value + 8) if key == shift else ptr(a[key]))
            return fn(ctx._h, g("y"), g("r"), g("d"), g("coin"), R, lnM, g("z"), g("acc"), g("E"), B_)
        assert call() == _lib.RZK_OK
        assert call(E=1) == _lib.RZK_OK                            # E may be NULL
        for key in ("y", "r", "d", "coin", "z", "acc"):
            assert call(**{key: 1}) == RZK_E_ARG, key
        assert call(R=1) == RZK_E_ARG and call(R=R62 + 1) == RZK_E_ARG and call(R=2) == _lib.RZK_OK
        assert call(lnM=-1e-9) == RZK_E_ARG and call(lnM=float("nan")) == RZK_E_ARG and call(lnM=0.0) == _lib.RZK_OK
        assert call(B_=0, y=1, z=1) == _lib.RZK_OK                 # B == 0 is a no-op
        ctx.synchronize()
    for key in ("y", "r", "d", "z"):                               # the slab32 rule of the device form
        assert call(shift=key) == RZK_E_ARG, key
    ctx.synchronize()
    with pytest.raises(ValueError):
        ctx.open_response_reject32(w64(y), w64(r), w64(d), coin, R62, LNM)
    with pytest.raises(ValueError):
        ctx.open_response_reject(y, r, d, coin, R62, LNM)            # the 64-bit method keeps rejecting int32


# ---- the prover ------------------------------------------------------------------------------------------------------------
MARKED = ("unit_", "shift_row", "row_", "response_stat", "sample_", "fs_")


def check_prover(torch, N, B, exact, native, seed):
    ctx, A = keyed_ctx(N, 1, 3, 1, 36, seed=seed)
    x = ctx.sample_uniform(9, 0, ctx.half, (B, 1))
    x32 = ctx.narrow(x)
    S64, S32 = (ExactKeyedSampler, ExactKeyedSampler32) if exact else (KeyedSampler, KeyedSampler32)
    c, t, z, ok, r, rounds = FS.open_prove_zk(ctx, ctx.widen(x32), S64(ctx, KEY, 1000), aux=AUX)
    ctx.synchronize()
    ctx.prof_enable(True)
    ctx.prof_reset()
    s32 = S32(ctx, KEY, 1000)
    c32, t32, z32, ok32, r32, rounds32 = FS.open_prove_zk32(ctx, x32, s32, aux=AUX)
    ctx.synchronize()
    names = kernel_names(ctx)
    ctx.prof_enable(False)
    for a32, a64 in ((c32, c), (t32, t), (z32, z), (r32, r)):
        assert a32.dtype == torch.int32 and torch.equal(a32.to(torch.int64), a64)
    assert torch.equal(ok32, ok) and torch.equal(rounds32, rounds)
    assert bool(ok32.all())
    assert bool(FS.open_verify32(ctx, c32, t32, z32, aux=AUX).all())
    if native:
        assert "widen_kernel" not in names and "narrow_kernel" not in names, names
        bad = [nm for nm in names if nm.startswith(MARKED) and "i32" not in nm]
        assert not bad, bad
        assert any(nm.startswith("response_stat_kernel<") for nm in names) and any(nm.startswith("sample_") for nm in names)
    else:
        assert "widen_kernel" in names and "narrow_kernel" in names
    return rounds32, names


def test_open_prove_zk32_equals_open_prove_zk(torch_mod):
    rounds, names = check_prover(torch_mod, 512, 64, exact=False, native=True, seed=141)
    assert int(rounds.max()) >= 1                                # a retry ran: t = a1.y alone, through matvec32
    assert sum(nm == "reject_decide_kernel" for nm in names) == int(rounds.max()) + 1


def test_open_prove_zk32_exact_sampler(torch_mod):
    _, names = check_prover(torch_mod, 512, 64, exact=True, native=True, seed=142)
    assert "sample_dgauss_chacha_kernel_i32" in names


def test_open_prove_zk32_n1024(torch_mod):
    check_prover(torch_mod, 1024, 8, exact=False, native=True, seed=143)


def test_open_prove_zk32_convert_path(torch_mod):
    check_prover(torch_mod, 64, 8, exact=False, native=False, seed=144)


def test_open_prove_sampled32(torch_mod):
    ctx, A = keyed_ctx(512, 1, 3, 1, 36, seed=145)
    x = ctx.sample_uniform(9, 0, ctx.half, (5, 1))
    out64 = FS.open_prove_sampled(ctx, x, KeyedSampler(ctx, KEY, 7), aux=AUX)
    out32 = FS.open_prove_sampled32(ctx, ctx.narrow(x), KeyedSampler32(ctx, KEY, 7), aux=AUX)
    ctx.synchronize()
    for a32, a64 in zip(out32, out64):
        assert torch_mod.equal(a32.to(a64.dtype), a64)
