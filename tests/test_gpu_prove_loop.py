"""The zero-knowledge Open prover with its rejection loop inside the library (include/rzk.h "prover loop", DESIGN.md
section 21) on the GPU.  The reference is the Python loop, fiat_shamir.open_prove_zk / open_prove_zk32, under the same key
and first nonce: the native entry point must give the same bytes.

  * compaction: rzk_debug_compact_dev against numpy.nonzero at the tile, wavefront and lane edges, and past one tile;
  * the prover: c, t, z, r, ok, rounds byte for byte, equal sampler counters, every proof verifies; both widths, both
    Gaussian samplers, N = 512 / 1024 / 64 (the convert path) and (2,5,2), several grid-stride trips;
  * max_rounds, input faults, argument rules, the launches of a native run by name, the host-pointer form.
Every output of a raw call lives in a device buffer with guard words on both sides (Guarded, test_gpu_slab32.py)."""
import ctypes as C

import numpy as np
import pytest

from ring_zk_amd import _lib, RzkError
from ring_zk_amd import fiat_shamir as FS
from ring_zk_amd.backend import ExactKeyedSampler, ExactKeyedSampler32, KeyedSampler, KeyedSampler32, SeededSampler
from test_gpu_baseline_shapes import dev, make_ctx, torch_mod  # noqa: F401
from test_gpu_fiat_shamir import keyed_ctx
from test_gpu_slab32 import Guarded, PATTERN, kernel_names

pytestmark = pytest.mark.gpu

KEY = bytes(range(100, 132))
AUX = bytes(range(60, 92))
RZK_E_ARG, RZK_E_STATE = _lib.RZK_E_ARG, _lib.RZK_E_STATE
SAMPLERS = {(64, False): KeyedSampler, (64, True): ExactKeyedSampler, (32, False): KeyedSampler32, (32, True): ExactKeyedSampler32}
FILL32 = int.from_bytes(bytes([PATTERN]) * 4, "little")
LOOP_KERNELS = ("pending_compact_kernel", "coin_kernel", "gather_rows_kernel", "accept_scatter_kernel")
EDGE_KERNELS = ("prove_first_kernel", "prove_last_kernel")


def nonce_of(i):
    return (C.c_uint8 * 16).from_buffer_copy(int(i).to_bytes(16, "little"))


# ---- 1. compaction ----------------------------------------------------------------------------------------------------------
def compact(torch, ctx, live, done):
    """rzk_debug_compact_dev on guarded idx and count: (idx[:count], count) after checking that idx past count is untouched"""
    B = live.shape[0]
    idx, count = Guarded(torch, (max(B, 1),), torch.int32), Guarded(torch, (1,), torch.int32)
    dl, dd = dev(torch, live), dev(torch, done)
    ctx._bind_torch_stream()
    ctx._check(ctx._L.rzk_debug_compact_dev(ctx._h, C.c_void_p(dl.data_ptr()), C.c_void_p(dd.data_ptr()), B, C.c_void_p(idx.ptr()),
                                            C.c_void_p(count.ptr())))
    ctx.synchronize()
    n = int(count.take()[0])
    got = idx.take().view(np.uint32)
    assert 0 <= n <= B and (got[n:] == FILL32).all(), "idx past count was written"
    return got[:n], n


def flag_patterns(rng, B):
    b = np.arange(B)
    yield "clear", np.zeros(B, bool)
    yield "set", np.ones(B, bool)
    yield "even", b % 2 == 0
    yield "odd", b % 2 == 1
    yield "first", b == 0
    yield "last", b == B - 1
    yield "random", rng.integers(0, 2, B).astype(bool)
    yield "sparse", rng.integers(0, 16, B) == 0


def check_compaction(torch, ctx, rng, B):
    for name, pend in flag_patterns(rng, B):
        for mask in range(3):   # not pending: done under a live flag / live clear / live clear and done set
            live = np.where(pend, np.where(np.arange(B) % 3 == 0, 0xff, 1), 0 if mask else 1).astype(np.uint8)
            done = np.where(pend, 0, (0, 1)[mask != 1]).astype(np.uint8)
            if mask == 0:
                done[(~pend) & (np.arange(B) % 5 == 0)] = 0x80            # any non-zero byte is a set flag
            want = np.nonzero((live != 0) & (done == 0))[0]
            assert np.array_equal(want, np.nonzero(pend)[0])
            got, n = compact(torch, ctx, live, done)
            assert n == want.size and np.array_equal(got, want.astype(np.uint32)), (B, name, mask)


@pytest.mark.parametrize("B", [1, 63, 64, 65, 1023, 1024, 1025, 4097])
def test_compaction_equals_nonzero(torch_mod, B):
    ctx = make_ctx(64, 1, 3, 1)
    check_compaction(torch_mod, ctx, np.random.default_rng(70000 + B), B)


def test_compaction_under_one_cu(torch_mod):
    ctx = make_ctx(64, 1, 3, 1, env={"RZK_GRID_CUS": 1})
    check_compaction(torch_mod, ctx, np.random.default_rng(75000), 5000)


def test_compaction_argument_rules(torch_mod):
    torch = torch_mod
    ctx = make_ctx(64, 1, 3, 1)
    L, h = ctx._L, ctx._h
    buf = torch.zeros(16, dtype=torch.uint8, device="cuda")
    idx = torch.zeros(16, dtype=torch.int32, device="cuda")
    p, pi = C.c_void_p(buf.data_ptr()), C.c_void_p(idx.data_ptr())
    ctx._bind_torch_stream()
    assert L.rzk_debug_compact_dev(h, None, p, 4, pi, pi) == RZK_E_ARG
    assert L.rzk_debug_compact_dev(h, p, None, 4, pi, pi) == RZK_E_ARG
    assert L.rzk_debug_compact_dev(h, p, p, 4, None, pi) == RZK_E_ARG
    assert L.rzk_debug_compact_dev(h, p, p, 4, pi, None) == RZK_E_ARG
    assert L.rzk_debug_compact_dev(h, p, p, 1 << 32, pi, pi) == RZK_E_ARG     # indices are uint32
    got, n = compact(torch, ctx, np.zeros(0, np.uint8), np.zeros(0, np.uint8))   # B == 0: count = 0, nothing else
    assert n == 0


# ---- 2. the prover ------------------------------------------------------------------------------------------------------------
def inputs(ctx, B, width):
    x = ctx.sample_uniform(9, 0, ctx.half, (B, ctx.l))
    return ctx.narrow(x) if width == 32 else x


def reference(ctx, x, width, exact, nonce0, max_rounds=64):
    """the Python loop: ((c, t, z, ok, r, rounds) as numpy, the sampler's counter afterwards)"""
    s = SAMPLERS[(width, exact)](ctx, KEY, nonce0)
    prove = FS.open_prove_zk32 if width == 32 else FS.open_prove_zk
    out = prove(ctx, x, s, aux=AUX, max_rounds=max_rounds)
    return tuple(a.cpu().numpy() for a in out), s.counter


def native_raw(torch, ctx, x, width, exact, nonce0, max_rounds=64, aux=AUX, gauss_kind=None, shift=None):
    """rzk_open_prove_zk[32]_batch_dev on guarded outputs: (status, outputs as Guarded by name, rounds_run).
    shift: the name of one slab whose pointer is moved by 8 bytes (the alignment rule)"""
    dt = torch.int32 if width == 32 else torch.int64
    B, N, n, k, l = int(x.shape[0]), ctx.N, ctx.n, ctx.k, ctx.l
    out = {"c": Guarded(torch, (B, n + l, N), dt), "t": Guarded(torch, (B, n, N), dt), "z": Guarded(torch, (B, k, N), dt),
           "r": Guarded(torch, (B, k, N), dt), "ok": Guarded(torch, (B,), torch.uint8), "rounds": Guarded(torch, (B,), torch.uint8)}
    ptr = {name: g.ptr() for name, g in out.items()}
    ptr["x"] = x.data_ptr()
    if shift:
        ptr[shift] += 8
    ran = C.c_uint32(0xffff)
    fn = ctx._L.rzk_open_prove_zk32_batch_dev if width == 32 else ctx._L.rzk_open_prove_zk_batch_dev
    ctx._bind_torch_stream()
    auxb = None if aux is None else (C.c_uint8 * 32).from_buffer_copy(aux)
    st = fn(ctx._h, C.c_void_p(ptr["x"]), nonce_of(nonce0), 0, int(exact) if gauss_kind is None else gauss_kind, auxb, max_rounds,
            *[C.c_void_p(ptr[name]) for name in ("c", "t", "z", "r", "ok", "rounds")], C.byref(ran), B)
    return st, out, int(ran.value)


def take(out):
    return tuple(out[name].take() for name in ("c", "t", "z", "ok", "r", "rounds"))


def assert_same(got, want, what):
    for name, a, b in zip(("c", "t", "z", "ok", "r", "rounds"), got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name)
        assert a.tobytes() == b.tobytes(), (what, name, np.argwhere(a != b)[:4])


def verify(ctx, torch, width, c, t, z):
    fn = FS.open_verify32 if width == 32 else FS.open_verify
    return fn(ctx, dev(torch, c), dev(torch, t), dev(torch, z), aux=AUX).cpu().numpy()


def check_prover(torch, ctx, B, width, exact, nonce0, max_rounds=64):
    """open_prove_zk_native and the raw entry point against the Python loop; returns (outputs, rounds_run)"""
    x = inputs(ctx, B, width)
    want, counter = reference(ctx, x, width, exact, nonce0, max_rounds)
    ctx.synchronize()
    s = SAMPLERS[(width, exact)](ctx, KEY, nonce0)
    got = tuple(a.cpu().numpy() for a in FS.open_prove_zk_native(ctx, x, s, aux=AUX, max_rounds=max_rounds))
    ctx.synchronize()
    assert_same(got, want, "open_prove_zk_native")
    assert s.counter == counter, "the sampler's counter ends where open_prove_zk's does"
    st, out, ran = native_raw(torch, ctx, x, width, exact, nonce0, max_rounds)
    assert st == 0, ctx._L.rzk_last_error(ctx._h)
    ctx.synchronize()
    assert_same(take(out), want, "rzk_open_prove_zk_batch_dev")
    assert 1 + 3 * ran == counter - nonce0, "rounds_run counts the rounds that drew"
    c, t, z, ok, r, rounds = want
    assert verify(ctx, torch, width, c, t, z).tolist() == ok.tolist()
    assert (rounds[ok == 0] == 0).all() and not t[ok == 0].any() and not z[ok == 0].any()
    assert int(rounds.max()) < ran <= max_rounds
    return want, ran


@pytest.mark.parametrize("width", [64, 32])
@pytest.mark.parametrize("exact", [False, True], ids=["box-muller", "exact"])
def test_prover_n512(torch_mod, width, exact):
    ctx, _ = keyed_ctx(512, 1, 3, 1, 36, seed=151)
    (c, t, z, ok, r, rounds), ran = check_prover(torch_mod, ctx, 64, width, exact, nonce0=2000 + width + exact)
    assert ok.all()
    assert int(rounds.max()) >= 2                                # several retry rounds ran on shrinking sub-batches


@pytest.mark.parametrize("width", [64, 32])
def test_prover_n1024(torch_mod, width):
    ctx, _ = keyed_ctx(1024, 1, 3, 1, 36, seed=152)
    (_, _, _, ok, _, _), _ = check_prover(torch_mod, ctx, 8, width, False, nonce0=(1 << 64) - 3)   # the nonce carries into byte 8
    assert ok.all()


def test_prover_convert_path(torch_mod):
    ctx, _ = keyed_ctx(64, 1, 3, 1, 36, seed=153)
    (_, _, _, ok, _, _), _ = check_prover(torch_mod, ctx, 8, 32, False, nonce0=5)
    assert ok.all()


def test_prover_2_5_2(torch_mod):
    ctx, _ = keyed_ctx(1024, 2, 5, 2, 36, seed=154)
    (_, _, _, ok, _, _), _ = check_prover(torch_mod, ctx, 4, 64, False, nonce0=6)
    assert ok.all()


def test_prover_under_one_cu(torch_mod):
    ctx, _ = keyed_ctx(512, 1, 3, 1, 36, seed=155, env={"RZK_GRID_CUS": 1})
    (_, _, _, ok, _, rounds), _ = check_prover(torch_mod, ctx, 100, 32, False, nonce0=7)
    assert ok.all() and int(rounds.max()) >= 2


# ---- 3. max_rounds ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_rounds", [1, 2])
def test_max_rounds(torch_mod, max_rounds):
    ctx, _ = keyed_ctx(512, 1, 3, 1, 36, seed=156)
    (c, t, z, ok, r, rounds), ran = check_prover(torch_mod, ctx, 64, 32, False, nonce0=3000, max_rounds=max_rounds)
    assert ran == max_rounds                                      # 64 proofs at acceptance 1/3: some are still pending
    assert 0 < int(ok.sum()) < 64 and int(rounds.max()) == max_rounds - 1
    assert not t[ok == 0].any() and not z[ok == 0].any()


# ---- 4. input faults ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [64, 32])
def test_input_faults(torch_mod, width):
    """A non-canonical coefficient in the first and in the last proof of x: their ok bytes are cleared, the call raises the
    sticky word once, and the other proofs are what the Python loop gives."""
    torch = torch_mod
    ctx, _ = keyed_ctx(512, 1, 3, 1, 36, seed=157)
    B = 8
    x = inputs(ctx, B, width)
    x[0, 0, 0] = ctx.half + 1
    x[B - 1, ctx.l - 1, ctx.N - 1] = -(ctx.half + 1)
    want, _ = reference(ctx, x, width, False, 4000)
    with pytest.raises(RzkError) as e_ref:
        ctx.synchronize()
    assert e_ref.value.status == RZK_E_ARG
    ctx.synchronize()
    st, out, ran = native_raw(torch, ctx, x, width, False, 4000)
    assert st == 0
    with pytest.raises(RzkError) as e_nat:
        ctx.synchronize()                                          # the sticky word, reported once
    assert e_nat.value.status == RZK_E_ARG
    ctx.synchronize()
    got = take(out)
    assert got[3].tolist() == want[3].tolist() == [0] + [1] * (B - 2) + [0]
    good = slice(1, B - 1)
    for name, a, b in zip(("c", "t", "z", "ok", "r", "rounds"), got, want):
        assert np.array_equal(a[good], b[good]), name
    assert not got[1][[0, B - 1]].any() and not got[2][[0, B - 1]].any()   # t, z of the refused proofs are zero
    st, out, _ = native_raw(torch, ctx, inputs(ctx, B, width), width, False, 4100)   # the fault does not leak into the next call
    assert st == 0
    ctx.synchronize()
    assert take(out)[3].all()


# ---- 5. argument rules ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [64, 32])
def test_argument_rules(torch_mod, width):
    torch = torch_mod
    ctx, _ = keyed_ctx(512, 1, 3, 1, 36, seed=158)
    ctx.set_sampler_key(KEY)
    x = inputs(ctx, 4, width)

    def refused(code, **kw):
        st, out, ran = native_raw(torch, ctx, x, width, False, kw.pop("nonce0", 10), **kw)
        assert st == code, (kw, st)
        ctx.synchronize()                                          # nothing was launched: no fault, and every output keeps its fill
        for name, g in out.items():
            assert (g.take().view(np.uint8) == PATTERN).all(), (kw, name)
        assert ran == 0

    refused(RZK_E_ARG, gauss_kind=2)
    refused(RZK_E_ARG, gauss_kind=-1)
    refused(RZK_E_ARG, max_rounds=0)
    refused(RZK_E_ARG, max_rounds=256)
    refused(RZK_E_ARG, nonce0=(1 << 128) - 1 - 3 * 64, max_rounds=64)          # nonce0 + 1 + 3 max_rounds = 2^128
    refused(RZK_E_ARG, nonce0=(1 << 128) - 1, max_rounds=1)
    for name in ("x", "c", "t", "z", "r"):
        refused(RZK_E_ARG, shift=name)
    st, out, ran = native_raw(torch, ctx, x, width, False, (1 << 128) - 2 - 3 * 64, max_rounds=64)   # the last span that fits
    assert st == 0 and ran >= 1
    ctx.synchronize()
    assert take(out)[3].all()
    st, out, ran = native_raw(torch, ctx, x, width, False, 11, aux=None)                              # aux32 may be NULL
    assert st == 0
    ctx.synchronize()
    c, t, z, ok, r, rounds = take(out)
    fn = FS.open_verify32 if width == 32 else FS.open_verify
    assert fn(ctx, dev(torch, c), dev(torch, t), dev(torch, z)).cpu().numpy().all()
    ctx.set_sampler_key(None)
    refused(RZK_E_STATE)                                                                               # no sampler key
    ctx.set_sampler_key(KEY)
    with pytest.raises(ValueError):
        FS.open_prove_zk_native(ctx, x, SeededSampler(ctx, 1))                                         # Philox has no keyed entry point
    nokey = make_ctx(512, 1, 3, 1, kappa=36)
    nokey.set_sampler_key(KEY)
    st, _, _ = native_raw(torch, nokey, inputs(nokey, 2, width), width, False, 10)
    assert st == RZK_E_STATE                                                                           # no commitment key


# ---- 6. the launches of a native run ------------------------------------------------------------------------------------------
def test_profile_of_a_native_run(torch_mod):
    torch = torch_mod
    ctx, _ = keyed_ctx(512, 1, 3, 1, 36, seed=159)
    ctx.set_sampler_key(KEY)
    x = inputs(ctx, 64, 32)
    ctx._bind_torch_stream()
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        st, out, ran = native_raw(torch, ctx, x, 32, False, 5000)
        assert st == 0
        ctx.synchronize()
        names = kernel_names(ctx)
    finally:
        ctx.prof_enable(False)
    c, t, z, ok, r, rounds = take(out)
    assert ok.all() and int(rounds.max()) >= 2
    assert "widen_kernel" not in names and "narrow_kernel" not in names, names
    assert sum(nm == "reject_decide_kernel" for nm in names) == int(rounds.max()) + 1 == ran
    new = [nm.split("<")[0] for nm in names]
    assert all(nm.endswith("<i32>") for nm in names if nm.split("<")[0] in LOOP_KERNELS[1:] + EDGE_KERNELS[1:]), names
    # a segment per pending_compact_kernel launch: round 0 in front, then one per retry round, then the empty compaction
    cuts = [i for i, nm in enumerate(new) if nm == "pending_compact_kernel"] + [len(new)]
    head = new[:cuts[0]]
    assert [nm for nm in head if nm in LOOP_KERNELS + EDGE_KERNELS] == ["coin_kernel", "prove_first_kernel"]
    segments = [new[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    assert len(segments) == ran                                   # ran - 1 retry rounds and the compaction that found nothing
    for seg in segments[:-1]:
        ours = [nm for nm in seg if nm in LOOP_KERNELS]
        assert len(ours) <= 4 and sorted(ours) == sorted(LOOP_KERNELS), seg
        assert sum(nm == "reject_decide_kernel" for nm in seg) == 1
    assert [nm for nm in segments[-1] if nm in LOOP_KERNELS + EDGE_KERNELS] == ["pending_compact_kernel", "prove_last_kernel"]


# ---- 7. the host-pointer form --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [64, 32])
def test_host_pointer_form(torch_mod, width):
    ctx, _ = keyed_ctx(512, 1, 3, 1, 36, seed=160)
    ctx.set_sampler_key(KEY)
    x = inputs(ctx, 8, width)
    prove = ctx.open_prove_zk32 if width == 32 else ctx.open_prove_zk
    nonce0 = (6000).to_bytes(16, "little")
    d_out = prove(x, nonce0, 0, 0, AUX, 64)
    ctx.synchronize()
    h_out = prove(x.cpu().numpy(), nonce0, 0, 0, AUX, 64)
    assert h_out[-1] == d_out[-1] >= 1
    for a, b in zip(h_out[:-1], d_out[:-1]):
        assert isinstance(a, np.ndarray) and a.dtype == b.cpu().numpy().dtype and np.array_equal(a, b.cpu().numpy())
    assert h_out[3].all()
