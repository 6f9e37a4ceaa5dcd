"""The y-only half of the Linear and Sum commit steps (rzk_linear_mask_batch / rzk_sum_mask_batch, include/rzk.h "mask calls",
DESIGN.md section 24) on the GPU.

  * linear_mask / sum_mask give, byte for byte, the t, tp, u (ts, tp, u) that linear_commit / sum_commit write for the same
    g, y, yp, and those of the oracle's commit: N = 64 / 512 / 1024 / 2048 at (1,3,1), (2,5,2) at N = 1024, several grid-stride
    trips under RZK_GRID_CUS=1 at B = 40; Sum with V = 1, 2, 3 on both sides of sum_uses_d;
  * a non-canonical coefficient of g (gs) or y is reported as matvec reports it; the host form equals the device form; B == 0;
  * a mask call starts fewer launches than the commit call at the same shape.
Every output of a raw call lives in a device buffer with guard words on both sides (Guarded, test_gpu_slab32.py)."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from ring_zk_amd import RzkError, synth
from test_gpu_baseline_shapes import P_of, dev, make_ctx, torch_mod  # noqa: F401
from test_gpu_fiat_shamir import keyed_ctx
from test_gpu_slab32 import Guarded, kernel_names

pytestmark = pytest.mark.gpu

RZK_E_ARG = -1
S131, S252 = (1, 3, 1), (2, 5, 2)
IMAGES = {"RZK_SUM_D": 1, "RZK_DKEY": 2}   # the a2.(sum_i g_i y_i - y') side with the multiplier images (test_gpu_launch_names.py)
# (N, shape, knobs, B)
SHAPES = [(64, S131, {}, 3), (512, S131, {}, 3), (1024, S131, {}, 3), (2048, S131, {}, 3), (1024, S252, {}, 3),
          (512, S131, {"RZK_GRID_CUS": 1}, 40)]


def shape_id(N, shape, knobs, B):
    return f"{N}-{''.join(map(str, shape))}-B{B}" + "".join(f"-{k[4:]}={v}" for k, v in knobs.items())


def profiled(ctx, call):
    """(status, kernel names) of one raw call"""
    ctx._bind_torch_stream()
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        st = call()
        ctx._check(st)
        ctx.synchronize()
        return kernel_names(ctx)
    finally:
        ctx.prof_enable(False)


def raw_linear_mask(torch, ctx, g, y, yp):
    B = g.shape[0]
    out = [Guarded(torch, (B, ctx.n, ctx.N), torch.int64), Guarded(torch, (B, ctx.n, ctx.N), torch.int64),
           Guarded(torch, (B, ctx.l, ctx.N), torch.int64)]
    ins = [dev(torch, a) for a in (g, y, yp)]
    names = profiled(ctx, lambda: ctx._L.rzk_linear_mask_batch_dev(
        ctx._h, *[C.c_void_p(a.data_ptr()) for a in ins], *[C.c_void_p(o.ptr()) for o in out], B))
    return [o.take() for o in out], names


def raw_sum_mask(torch, ctx, gs, ys, yp):
    B, V = gs.shape[0], gs.shape[1]
    out = [Guarded(torch, (B, V, ctx.n, ctx.N), torch.int64), Guarded(torch, (B, ctx.n, ctx.N), torch.int64),
           Guarded(torch, (B, ctx.l, ctx.N), torch.int64)]
    ins = [dev(torch, a) for a in (gs, ys, yp)]
    names = profiled(ctx, lambda: ctx._L.rzk_sum_mask_batch_dev(
        ctx._h, V, *[C.c_void_p(a.data_ptr()) for a in ins], *[C.c_void_p(o.ptr()) for o in out], B))
    return [o.take() for o in out], names


def commit_names(ctx, call):
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        out = call()
        ctx.synchronize()
        return out, kernel_names(ctx)
    finally:
        ctx.prof_enable(False)


def same_bytes(got, want, what):
    for name, a, b in zip(("t", "tp", "u"), got, want):
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name)
        assert a.tobytes() == b.tobytes(), (what, name, np.argwhere(a != b)[:4])


def linear_inputs(ctx, rng, B):
    N, k, l, sig = ctx.N, ctx.k, ctx.l, ctx.sigma
    return dict(g=synth.uniform(rng, (B, N)), x=synth.uniform(rng, (B, l, N)), r=synth.small(rng, (B, k, N)),
                rp=synth.small(rng, (B, k, N)), y=synth.gauss(rng, (B, k, N), sig), yp=synth.gauss(rng, (B, k, N), sig))


def sum_inputs(ctx, rng, B, V):
    N, k, l, sig = ctx.N, ctx.k, ctx.l, ctx.sigma
    return dict(gs=synth.uniform(rng, (B, V, N)), xs=synth.uniform(rng, (B, V, l, N)), rs=synth.small(rng, (B, V, k, N)),
                rp=synth.small(rng, (B, k, N)), ys=synth.gauss(rng, (B, V, k, N), sig), yp=synth.gauss(rng, (B, k, N), sig))


# ---- 1. Linear ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,shape,knobs,B", SHAPES, ids=[shape_id(*s) for s in SHAPES])
def test_linear_mask_equals_the_commit_call(torch_mod, N, shape, knobs, B):
    torch = torch_mod
    ctx, A = keyed_ctx(N, *shape, 36, seed=2300 + N + shape[0], env=knobs)
    i = linear_inputs(ctx, np.random.default_rng(2310 + N + B), B)
    d = {key: dev(torch, a) for key, a in i.items()}
    (c, cp, t, tp, u, ok), names_commit = commit_names(ctx, lambda: ctx.linear_commit(d["g"], d["x"], d["r"], d["rp"], d["y"], d["yp"]))
    want = [a.cpu().numpy() for a in (t, tp, u)]
    got, names_mask = raw_linear_mask(torch, ctx, i["g"], i["y"], i["yp"])
    same_bytes(got, want, "rzk_linear_mask_batch_dev")
    same_bytes(ctx.linear_mask(i["g"], i["y"], i["yp"]), want, "rzk_linear_mask_batch (host form)")
    same_bytes([a.cpu().numpy() for a in ctx.linear_mask(d["g"], d["y"], d["yp"])], want, "Context.linear_mask on tensors")
    P = P_of(ctx)
    for b in sorted({0, B // 2, B - 1}):                       # the oracle's Linear commit (linear.rs:118-129)
        ref = O.linear_commit(P, A, i["g"][b], i["x"][b], i["r"][b], i["rp"][b], i["y"][b], i["yp"][b])
        same_bytes([a[b] for a in got], ref[2:5], ("oracle", b))
    assert 0 < len(names_mask) < len(names_commit), (names_mask, names_commit)


# ---- 2. Sum ------------------------------------------------------------------------------------------------------------------
# (small rings have no a2.(sum) rearrangement and no multiplier images: one side only)
SUM_CASES = [s + (side,) for s in SHAPES for side in ("default", "images") if not (side == "images" and s[0] < 512)]


@pytest.mark.parametrize("N,shape,knobs,B,side", SUM_CASES, ids=[shape_id(*s[:4]) + "-" + s[4] for s in SUM_CASES])
def test_sum_mask_equals_the_commit_call(torch_mod, N, shape, knobs, B, side):
    torch = torch_mod
    env = dict(knobs, **(IMAGES if side == "images" else {}))
    ctx, A = keyed_ctx(N, *shape, 36, seed=2400 + N + shape[0], env=env)
    P = P_of(ctx)
    for V in (1, 2, 3):
        i = sum_inputs(ctx, np.random.default_rng(2410 + N + B + V), B, V)
        d = {key: dev(torch, a) for key, a in i.items()}
        (cs, cp, ts, tp, u, ok), names_commit = commit_names(
            ctx, lambda: ctx.sum_commit(d["gs"], d["xs"], d["rs"], d["rp"], d["ys"], d["yp"]))
        want = [a.cpu().numpy() for a in (ts, tp, u)]
        got, names_mask = raw_sum_mask(torch, ctx, i["gs"], i["ys"], i["yp"])
        same_bytes(got, want, ("rzk_sum_mask_batch_dev", V))
        same_bytes(ctx.sum_mask(i["gs"], i["ys"], i["yp"]), want, ("rzk_sum_mask_batch (host form)", V))
        for b in sorted({0, B - 1}):                           # the oracle's Sum commit (sum.rs:145-160)
            ref = O.sum_commit(P, A, i["gs"][b], i["xs"][b], i["rs"][b], i["rp"][b], i["ys"][b], i["yp"][b])
            same_bytes([a[b] for a in got], ref[2:5], ("oracle", V, b))
        assert 0 < len(names_mask) < len(names_commit), (V, names_mask, names_commit)
        if side == "images":                                   # the forced side: multiplier images in both calls
            assert any(nm.startswith("dkey_transform_kernel") for nm in names_mask), names_mask
            assert any(nm.startswith("dkey_transform_kernel") for nm in names_commit), names_commit


# ---- 3. faults and modes -----------------------------------------------------------------------------------------------------
def sticky(ctx):
    """the sticky input-error word of the device forms: reported once by synchronize()"""
    try:
        ctx.synchronize()
    except RzkError as e:
        assert e.status == RZK_E_ARG
        ctx.synchronize()   # reported once
        return True
    return False


@pytest.mark.parametrize("N", [64, 1024])
def test_non_canonical_inputs_are_reported_as_matvec_reports_them(torch_mod, N):
    torch = torch_mod
    ctx, _ = keyed_ctx(N, *S131, 36, seed=2500 + N)
    B, V = 4, 2
    rng = np.random.default_rng(2510 + N)
    lin, summ = linear_inputs(ctx, rng, B), sum_inputs(ctx, rng, B, V)
    bad_v = lin["y"].copy()
    bad_v[0, 0, 0] = ctx.half + 1
    # the rule of matvec: the host form fails with RZK_E_ARG, the device form raises the sticky word
    with pytest.raises(RzkError) as e:
        ctx.matvec(0, bad_v)
    assert e.value.status == RZK_E_ARG
    ctx.matvec(0, dev(torch, bad_v))
    assert sticky(ctx)

    def planted(a, where):
        a = a.copy()
        a.reshape(-1)[0 if where == "first" else -1] = (ctx.half + 1) * (1 if where == "first" else -1)
        return a

    for where in ("first", "last"):
        for name in ("g", "y"):
            i = dict(lin, **{name: planted(lin[name], where)})
            with pytest.raises(RzkError) as e:
                ctx.linear_mask(i["g"], i["y"], i["yp"])
            assert e.value.status == RZK_E_ARG, (where, name)
            ctx.linear_mask(*[dev(torch, i[key]) for key in ("g", "y", "yp")])
            assert sticky(ctx), ("linear", where, name)
        for name in ("gs", "ys"):
            i = dict(summ, **{name: planted(summ[name], where)})
            with pytest.raises(RzkError) as e:
                ctx.sum_mask(i["gs"], i["ys"], i["yp"])
            assert e.value.status == RZK_E_ARG, (where, name)
            ctx.sum_mask(*[dev(torch, i[key]) for key in ("gs", "ys", "yp")])
            assert sticky(ctx), ("sum", where, name)
    # the fault does not leak into the next call, and clean inputs raise nothing
    ctx.linear_mask(*[dev(torch, lin[key]) for key in ("g", "y", "yp")])
    ctx.sum_mask(*[dev(torch, summ[key]) for key in ("gs", "ys", "yp")])
    assert not sticky(ctx)
    # trusted-producer mode is matvec's too: the transform kernels skip the canonical test, the schoolbook kernels of the
    # small rings keep it
    ctx.trust_device_outputs(True)
    ctx.matvec(0, dev(torch, bad_v))
    matvec_reports = sticky(ctx)
    assert matvec_reports == (N < 512)
    ctx.linear_mask(dev(torch, lin["g"]), dev(torch, bad_v), dev(torch, lin["yp"]))
    assert sticky(ctx) == matvec_reports
    ctx.trust_device_outputs(False)


def test_empty_batch_and_null_rules(torch_mod):
    ctx, _ = keyed_ctx(512, *S131, 36, seed=2600)
    L, h, null = ctx._L, ctx._h, C.c_void_p(None)
    ctx._bind_torch_stream()
    ctx.prof_enable(True)
    ctx.prof_reset()
    for dev_form in ("", "_dev"):                              # B == 0: a no-op, pointers may be NULL
        assert getattr(L, "rzk_linear_mask_batch" + dev_form)(h, *[null] * 6, 0) == 0
        assert getattr(L, "rzk_sum_mask_batch" + dev_form)(h, 2, *[null] * 6, 0) == 0
        assert getattr(L, "rzk_sum_mask_batch" + dev_form)(h, 0, *[null] * 6, 0) == 0        # (as the commit call)
    buf = torch_mod.zeros(4 * 3 * 512, dtype=torch_mod.int64, device="cuda")
    p = C.c_void_p(buf.data_ptr())
    assert L.rzk_sum_mask_batch_dev(h, 0, *[p] * 6, 1) == RZK_E_ARG                           # V == 0
    for hole in range(6):                                      # a NULL slab
        args = [p] * 6
        args[hole] = null
        assert L.rzk_linear_mask_batch_dev(h, *args, 1) == RZK_E_ARG
        assert L.rzk_sum_mask_batch_dev(h, 1, *args, 1) == RZK_E_ARG
    ctx.synchronize()
    assert kernel_names(ctx) == []                             # none of these launched anything
    ctx.prof_enable(False)
