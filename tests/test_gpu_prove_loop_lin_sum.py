"""The zero-knowledge Linear and Sum provers with their rejection loop inside the library (include/rzk.h "prover loop: Linear
and Sum") on the GPU.  The reference is the Python loop, fiat_shamir.linear_prove_zk / sum_prove_zk, under
the same key, stream, aux and first nonce: the native entry points must give the same bytes.

  * the provers: every output byte for byte, equal sampler counters, 2 + 4 rounds_run nonces, every accepted proof verifies;
    both Gaussian samplers, N = 64 / 512 / 1024 / 2048, (2,5,2) under one CU, V = 1, 2, 3, a nonce that carries into byte 8;
  * truncated runs (max_rounds 1 and 2), input faults in x and g, the argument rules, the launches of a native run by name,
    the host-pointer form.
The conditions a case needs of its key and nonce (every proof accepted, at least two retry rounds, or a partly accepted batch)
are asserted on the REFERENCE's output.  Every output of a raw call lives in a device buffer with guard words on both sides
(Guarded, test_gpu_slab32.py)."""
import ctypes as C

import numpy as np
import pytest

from ring_zk_amd import _lib, RzkError
from ring_zk_amd import fiat_shamir as FS
from ring_zk_amd.backend import ExactKeyedSampler, KeyedSampler, SeededSampler
from test_gpu_baseline_shapes import dev, make_ctx, torch_mod  # noqa: F401
from test_gpu_fiat_shamir import keyed_ctx
from test_gpu_slab32 import Guarded, PATTERN, kernel_names

pytestmark = pytest.mark.gpu

KEY = bytes(range(100, 132))
AUX = bytes(range(60, 92))
RZK_E_ARG, RZK_E_STATE = _lib.RZK_E_ARG, _lib.RZK_E_STATE
# the tuple of fiat_shamir.*_prove_zk, and the output arguments of the C call in their order
NAMES = {"linear": ("c", "cp", "t", "tp", "u", "z", "zp", "ok", "r", "rp", "rounds"),
         "sum": ("cs", "cp", "ts", "tp", "u", "zs", "zp", "ok", "rs", "rp", "rounds")}
C_ORDER = {"linear": ("c", "cp", "t", "tp", "u", "z", "zp", "r", "rp", "ok", "rounds"),
           "sum": ("cs", "cp", "ts", "tp", "u", "zs", "zp", "rs", "rp", "ok", "rounds")}
FRESH = {"linear": ("t", "tp", "u", "z", "zp"), "sum": ("ts", "tp", "u", "zs", "zp")}
LOOP_KERNELS = ("pending_compact_kernel", "coin_kernel", "gather_fields_kernel", "accept_scatter_fields_kernel")
EDGE_KERNELS = ("prove_first_want_kernel", "prove_last_fields_kernel")
OPEN_ONLY = ("gather_rows_kernel", "accept_scatter_kernel", "prove_first_kernel", "prove_last_kernel")


def nonce_of(i):
    return (C.c_uint8 * 16).from_buffer_copy(int(i).to_bytes(16, "little"))


def inputs(ctx, B, V=None):
    """(g, x) for Linear (V None), (gs, xs) for Sum: uniform, canonical, on the device"""
    lead = (B,) if V is None else (B, V)
    return ctx.sample_uniform(11, 0, ctx.half, lead), ctx.sample_uniform(12, 0, ctx.half, lead + (ctx.l,))


def shapes(ctx, B, V=None):
    N, n, k, l = ctx.N, ctx.n, ctx.k, ctx.l
    v = () if V is None else (V,)
    kind = "linear" if V is None else "sum"
    sh = dict(zip(C_ORDER[kind], [(B,) + v + (n + l, N), (B, n + l, N), (B,) + v + (n, N), (B, n, N), (B, l, N), (B,) + v + (k, N),
                                  (B, k, N), (B,) + v + (k, N), (B, k, N), (B,), (B,)]))
    return kind, sh


def reference(ctx, g, x, exact, nonce0, max_rounds=64, V=None):
    """the Python loop: ({name: numpy}, the sampler's counter afterwards)"""
    s = (ExactKeyedSampler if exact else KeyedSampler)(ctx, KEY, nonce0)
    kind = "linear" if V is None else "sum"
    out = (FS.linear_prove_zk if V is None else FS.sum_prove_zk)(ctx, g, x, s, aux=AUX, max_rounds=max_rounds)
    return {name: a.cpu().numpy() for name, a in zip(NAMES[kind], out)}, s.counter


def native_raw(torch, ctx, g, x, exact, nonce0, max_rounds=64, aux=AUX, gauss_kind=None, shift=None, V=None, raw_V=None):
    """rzk_linear / rzk_sum_prove_zk_batch_dev on guarded outputs: (status, {name: Guarded}, rounds_run).  shift: the name of
    one slab whose pointer is moved by 8 bytes (the alignment rule); raw_V: the V passed to the C call in place of the slabs'"""
    B = int(x.shape[0])
    kind, sh = shapes(ctx, B, V)
    out = {name: Guarded(torch, sh[name], torch.uint8 if name in ("ok", "rounds") else torch.int64) for name in C_ORDER[kind]}
    ptr = {name: o.ptr() for name, o in out.items()}
    ptr["g"], ptr["x"] = g.data_ptr(), x.data_ptr()
    if shift:
        ptr[shift] += 8
    ran = C.c_uint32(0xffff)
    ctx._bind_torch_stream()
    auxb = None if aux is None else (C.c_uint8 * 32).from_buffer_copy(aux)
    fn = ctx._L.rzk_linear_prove_zk_batch_dev if V is None else ctx._L.rzk_sum_prove_zk_batch_dev
    lead = [] if V is None else [V if raw_V is None else raw_V]
    st = fn(ctx._h, *lead, C.c_void_p(ptr["g"]), C.c_void_p(ptr["x"]), nonce_of(nonce0), 0, int(exact) if gauss_kind is None else gauss_kind,
            auxb, max_rounds, *[C.c_void_p(ptr[name]) for name in C_ORDER[kind]], C.byref(ran), B)
    return st, out, int(ran.value)


def take(out):
    return {name: o.take() for name, o in out.items()}


def assert_same(got, want, what):
    for name, b in want.items():
        a = got[name]
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), (what, name, np.argwhere(a != b)[:4])


def verify(ctx, torch, o, g, V=None):
    d = {name: dev(torch, a) for name, a in o.items()}
    if V is None:
        acc = FS.linear_verify(ctx, d["c"], d["cp"], g, d["t"], d["tp"], d["u"], d["z"], d["zp"], aux=AUX)
    else:
        acc = FS.sum_verify(ctx, d["cs"], d["cp"], g, d["ts"], d["tp"], d["u"], d["zs"], d["zp"], aux=AUX)
    return acc.cpu().numpy()


def check_prover(torch, ctx, B, exact, nonce0, max_rounds=64, V=None, complete=True):
    """*_prove_zk_native and the raw entry point against the Python loop; returns (the reference's outputs, rounds_run).
    complete: the case needs a key and nonce under which every proof is accepted after at least two retry rounds."""
    kind = "linear" if V is None else "sum"
    g, x = inputs(ctx, B, V)
    want, counter = reference(ctx, g, x, exact, nonce0, max_rounds, V)
    ctx.synchronize()
    if complete:   # facts of the key and the nonce (the draws are deterministic), asserted on the reference
        assert want["ok"].all() and int(want["rounds"].max()) >= 2, (want["ok"].tolist(), want["rounds"].tolist())
    s = (ExactKeyedSampler if exact else KeyedSampler)(ctx, KEY, nonce0)
    native = FS.linear_prove_zk_native if V is None else FS.sum_prove_zk_native
    got = {name: a.cpu().numpy() for name, a in zip(NAMES[kind], native(ctx, g, x, s, aux=AUX, max_rounds=max_rounds))}
    ctx.synchronize()
    assert_same(got, want, kind + "_prove_zk_native")
    assert s.counter == counter, "the sampler's counter ends where the Python loop's does"
    st, out, ran = native_raw(torch, ctx, g, x, exact, nonce0, max_rounds, V=V)
    assert st == 0, ctx._L.rzk_last_error(ctx._h)
    ctx.synchronize()
    assert_same(take(out), want, "rzk_%s_prove_zk_batch_dev" % kind)
    assert 2 + 4 * ran == counter - nonce0, "rounds_run counts the rounds that drew"
    ok, rounds = want["ok"], want["rounds"]
    acc = verify(ctx, torch, want, g, V)
    assert (acc[ok != 0] == 1).all(), "every proof with ok is accepted by the verifier"
    assert (rounds[ok == 0] == 0).all() and all(not want[name][ok == 0].any() for name in FRESH[kind])
    assert int(rounds.max()) < ran <= max_rounds
    return want, ran


# ---- 1. Linear ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [False, True], ids=["box-muller", "exact"])
def test_linear_n512(torch_mod, exact):
    ctx, _ = keyed_ctx(512, 1, 3, 1, 36, seed=251)
    check_prover(torch_mod, ctx, 64, exact, nonce0=7000 + exact)


def test_linear_n1024_nonce_carry(torch_mod):
    ctx, _ = keyed_ctx(1024, 1, 3, 1, 36, seed=252)
    check_prover(torch_mod, ctx, 8, False, nonce0=(1 << 64) - 3)              # the nonce carries into byte 8


def test_linear_n64(torch_mod):
    ctx, _ = keyed_ctx(64, 1, 3, 1, 36, seed=253)
    check_prover(torch_mod, ctx, 16, False, nonce0=5)


def test_linear_n2048(torch_mod):
    ctx, _ = keyed_ctx(2048, 1, 3, 1, 36, seed=254)
    check_prover(torch_mod, ctx, 4, False, nonce0=6)


def test_linear_2_5_2_under_one_cu(torch_mod):
    ctx, _ = keyed_ctx(1024, 2, 5, 2, 36, seed=255, env={"RZK_GRID_CUS": 1})
    check_prover(torch_mod, ctx, 100, False, nonce0=7)


# ---- 2. Sum ------------------------------------------------------------------------------------------------------------------
def test_sum_v2_n512(torch_mod):
    ctx, _ = keyed_ctx(512, 1, 3, 1, 36, seed=261)
    check_prover(torch_mod, ctx, 32, False, nonce0=8000, V=2)


def test_sum_v3_n1024_128_rounds(torch_mod):
    ctx, _ = keyed_ctx(1024, 1, 3, 1, 36, seed=262)
    check_prover(torch_mod, ctx, 8, False, nonce0=8100, V=3, max_rounds=128)


def test_sum_v1_n64(torch_mod):
    ctx, _ = keyed_ctx(64, 1, 3, 1, 36, seed=263)
    check_prover(torch_mod, ctx, 8, False, nonce0=8200, V=1)


# ---- 3. truncated runs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_rounds", [1, 2])
def test_max_rounds(torch_mod, max_rounds):
    ctx, _ = keyed_ctx(512, 1, 3, 1, 36, seed=256)
    B = 64
    want, ran = check_prover(torch_mod, ctx, B, False, nonce0=9000, max_rounds=max_rounds, complete=False)
    ok = want["ok"]
    assert 0 < int(ok.sum()) < B                                              # on the reference: some proofs are still pending
    assert ran == max_rounds and int(want["rounds"].max()) <= max_rounds - 1
    assert all(not want[name][ok == 0].any() for name in FRESH["linear"])     # (and, by assert_same, of the native call)
    for name in ("c", "cp", "r", "rp"):                                       # written for every proof, accepted or not
        assert all(want[name][b].any() for b in range(B)), name


# ---- 4. input faults -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["x", "g"])
def test_input_faults(torch_mod, which):
    """A non-canonical coefficient in the first and in the last proof of x or g: their ok bytes are cleared, the call raises
    the sticky word once, and the other proofs are what the Python loop gives."""
    torch = torch_mod
    ctx, _ = keyed_ctx(512, 1, 3, 1, 36, seed=257)
    B = 8
    g, x = inputs(ctx, B)
    bad = x if which == "x" else g
    bad.reshape(B, -1)[0, 0] = ctx.half + 1
    bad.reshape(B, -1)[B - 1, -1] = -(ctx.half + 1)
    want, _ = reference(ctx, g, x, False, 4000)
    with pytest.raises(RzkError) as e_ref:
        ctx.synchronize()
    assert e_ref.value.status == RZK_E_ARG
    ctx.synchronize()
    st, out, ran = native_raw(torch, ctx, g, x, False, 4000)
    assert st == 0
    with pytest.raises(RzkError) as e_nat:
        ctx.synchronize()                                                     # the sticky word, reported once
    assert e_nat.value.status == RZK_E_ARG
    ctx.synchronize()
    got = take(out)
    assert got["ok"].tolist() == want["ok"].tolist() == [0] + [1] * (B - 2) + [0]
    good = slice(1, B - 1)
    for name in NAMES["linear"]:
        assert np.array_equal(got[name][good], want[name][good]), name
    for name in FRESH["linear"]:                                              # nothing y-dependent of a refused proof is released
        assert not got[name][[0, B - 1]].any(), name
    st, out, _ = native_raw(torch, ctx, *inputs(ctx, B), False, 4100)         # the fault does not leak into the next call
    assert st == 0
    ctx.synchronize()
    assert take(out)["ok"].all()


# ---- 5. argument rules ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [None, 2], ids=["linear", "sum"])
def test_argument_rules(torch_mod, V):
    torch = torch_mod
    ctx, _ = keyed_ctx(512, 1, 3, 1, 36, seed=258)
    ctx.set_sampler_key(KEY)
    g, x = inputs(ctx, 4, V)
    kind = "linear" if V is None else "sum"

    def refused(code, **kw):
        ctx._bind_torch_stream()
        ctx.prof_enable(True)
        ctx.prof_reset()
        try:
            st, out, ran = native_raw(torch, ctx, g, x, False, kw.pop("nonce0", 10), V=V, **kw)
            assert st == code, (kw, st)
            ctx.synchronize()                                                 # nothing was launched: no fault, no kernel, every fill kept
            assert kernel_names(ctx) == [], kw
        finally:
            ctx.prof_enable(False)
        for name, o in out.items():
            assert (o.take().view(np.uint8) == PATTERN).all(), (kw, name)
        assert ran == 0

    refused(RZK_E_ARG, gauss_kind=2)
    refused(RZK_E_ARG, max_rounds=0)
    refused(RZK_E_ARG, max_rounds=256)
    refused(RZK_E_ARG, nonce0=(1 << 128) - 2 - 4 * 64, max_rounds=64)         # nonce0 + 2 + 4 max_rounds = 2^128
    refused(RZK_E_ARG, nonce0=(1 << 128) - 1, max_rounds=1)
    for name in ("g", "x") + C_ORDER[kind][:9]:
        refused(RZK_E_ARG, shift=name)                                        # a misaligned slab
    if V is not None:
        refused(RZK_E_ARG, raw_V=0)
    st, out, ran = native_raw(torch, ctx, g, x, False, (1 << 128) - 3 - 4 * 64, max_rounds=64, V=V)   # the last span that fits
    assert st == 0 and ran >= 1
    ctx.synchronize()
    st, out, ran = native_raw(torch, ctx, g, x, False, 11, aux=None, V=V)    # aux32 may be NULL
    assert st == 0
    ctx.synchronize()
    ctx.set_sampler_key(None)
    refused(RZK_E_STATE)                                                      # no sampler key
    ctx.set_sampler_key(KEY)
    native = FS.linear_prove_zk_native if V is None else FS.sum_prove_zk_native
    with pytest.raises(ValueError):
        native(ctx, g, x, SeededSampler(ctx, 1))                              # Philox has no keyed entry point
    st, out, ran = native_raw(torch, ctx, g[:0], x[:0], False, 12, V=V)      # B == 0: a no-op
    assert st == 0 and ran == 0


# ---- 6. the launches of a native run ------------------------------------------------------------------------------------------
def profiled(ctx, call):
    ctx._bind_torch_stream()
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        out = call()
        ctx.synchronize()
        return out, kernel_names(ctx)
    finally:
        ctx.prof_enable(False)


@pytest.mark.parametrize("V", [None, 2], ids=["linear", "sum"])
def test_profile_of_a_native_run(torch_mod, V):
    torch = torch_mod
    ctx, _ = keyed_ctx(512, 1, 3, 1, 36, seed=259)
    ctx.set_sampler_key(KEY)
    B = 64 if V is None else 32
    g, x = inputs(ctx, B, V)
    want, _ = reference(ctx, g, x, False, 5000, V=V)
    ctx.synchronize()
    assert want["ok"].all() and int(want["rounds"].max()) >= 2               # on the reference: several retry rounds
    (st, out, ran), names = profiled(ctx, lambda: native_raw(torch, ctx, g, x, False, 5000, V=V))
    assert st == 0
    assert_same(take(out), want, "profiled run")
    # the launches of the commit call and of the mask call at this shape
    k = ctx.k
    lead = (B,) if V is None else (B, V)
    r, rp = ctx.sample_uniform(13, 0, ctx.b, lead + (k,)), ctx.sample_uniform(14, 0, ctx.b, (B, k))
    y, yp = ctx.sample_uniform(15, 0, ctx.b, lead + (k,)), ctx.sample_uniform(16, 0, ctx.b, (B, k))
    if V is None:
        _, commit = profiled(ctx, lambda: ctx.linear_commit(g, x, r, rp, y, yp))
        _, mask = profiled(ctx, lambda: ctx.linear_mask(g, y, yp))
    else:
        _, commit = profiled(ctx, lambda: ctx.sum_commit(g, x, r, rp, y, yp))
        _, mask = profiled(ctx, lambda: ctx.sum_mask(g, y, yp))
    assert len(mask) < len(commit)
    new = [nm.split("<")[0] for nm in names]
    assert not any(nm in OPEN_ONLY for nm in new), new                        # the Open loop's kernels stay the Open loop's
    assert sum(nm == "reject_decide_kernel" for nm in new) == int(want["rounds"].max()) + 1 == ran
    # a segment per pending_compact_kernel launch: round 0 in front, then one per retry round, then the empty compaction
    cuts = [i for i, nm in enumerate(new) if nm == "pending_compact_kernel"] + [len(new)]
    head = new[:cuts[0]]
    assert [nm for nm in head if nm in LOOP_KERNELS + EDGE_KERNELS] == ["coin_kernel", "prove_first_want_kernel"]
    segments = [new[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    assert len(segments) == ran
    rows0 = sum(nm == "row_kernel" for nm in head)
    for seg in segments[:-1]:
        # exactly one compaction, one coin kernel, one field gather and one field scatter beyond the library calls
        assert sorted(nm for nm in seg if nm in LOOP_KERNELS) == sorted(LOOP_KERNELS), seg
        assert sum(nm == "reject_decide_kernel" for nm in seg) == 1
        # No commit program after round 0.  The commit call's first launch is a row_kernel over the statement (gx = g x for
        # Linear, xp = sum_i x_i g_i for Sum); the mask call keeps only the row_kernel of the u rows: a retry has one
        # row_kernel launch fewer than round 0 ...
        assert sum(nm == "row_kernel" for nm in seg) == rows0 - 1 == 1, seg
        # ... and as many launches as round 0 without the two draws of r, the first kernel and the launches the mask call
        # saves, plus the compaction, the gather and the scatter
        assert len(seg) == len(head) - 2 - 1 - (len(commit) - len(mask)) + 3, (seg, head)
    assert [nm for nm in segments[-1] if nm in LOOP_KERNELS + EDGE_KERNELS] == ["pending_compact_kernel", "prove_last_fields_kernel"]


# ---- 7. the host-pointer form --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [None, 2], ids=["linear", "sum"])
def test_host_pointer_form(torch_mod, V):
    ctx, _ = keyed_ctx(512, 1, 3, 1, 36, seed=260)
    ctx.set_sampler_key(KEY)
    g, x = inputs(ctx, 8, V)
    prove = ctx.linear_prove_zk if V is None else ctx.sum_prove_zk
    nonce0 = (6000).to_bytes(16, "little")
    d_out = prove(g, x, nonce0, 0, 0, AUX, 64)
    ctx.synchronize()
    h_out = prove(g.cpu().numpy(), x.cpu().numpy(), nonce0, 0, 0, AUX, 64)
    assert h_out[-1] == d_out[-1] >= 1
    for a, b in zip(h_out[:-1], d_out[:-1]):
        assert isinstance(a, np.ndarray) and a.dtype == b.cpu().numpy().dtype and np.array_equal(a, b.cpu().numpy())
    assert h_out[7].any()
