"""Grid-stride trips against the oracle (GPU).

Every kernel walks its tasks in a grid-stride loop whose grid is capped by the device's CU count, so at the batch sizes
the other files use a team never makes a second trip.  RZK_GRID_CUS (include/rzk.h) sizes every grid cap, and the
scratch behind it, for fewer CUs; at 1 - 3 CUs batches of tens of proofs make several trips, and what only runs on a
later trip (row_kernel's row rotation, per-team scratch lines and parked sums reused from one task to the next, the
verdict flags a team presets, the XCD-class dealing of row_slots_kernel, the wire codec's loops) is compared with
oracle/rzk_oracle.c entry by entry.

Trip counts: the unit and row kernels run at most 32 one-wavefront teams per CU (8 two-wavefront teams at N = 2048), so
with c CUs the task stride is 32 c; a launch of T tasks makes ceil(T / 32 c) trips.  Unit kernels take one task per
batch entry once the batch is >= 16 c (RZK_UPT's default), row kernels one task per row of the program.  Each case
states the trips it reaches in its test id or in a comment.

  a. the knob takes effect and clamps;
  b. a seeded sweep (protocols x knobs x 1, 2, 3 CUs) at batches where every unit launch makes >= 3 trips;
  c. row_kernel's row rotation (stride % rows == 0) on and off, tampered proofs on later trips;
  d. BASELINE config 4 (Linear, N = 1024, B = 8192) at the device's own grid, as benchmarked and with RZK_LIN_E=0, where
     the 4-row verifier runs on row_kernel with 4 trips and the rotation on;
  e. every row-program kernel reached at 1 CU, oracle-equal;
  f. results do not depend on the grid: the Open cycle, the samplers, and the primitives at 1 CU vs the oracle;
  g. the wire codec at 1 CU: 16 walk trips, hundreds of copy trips, damaged messages on the last trips.
"""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

from oracle import oracle as O
from ring_zk_amd import synth, wire
from test_gpu_baseline_shapes import (P_of, _open_proof, check_key_products_and_open, check_sum_cycle, dev,  # noqa: F401
                                      make_ctx, torch_mod)
from test_gpu_random_shapes import KNOBS, check_linear_cycle
from test_gpu_wire_messages import _first_coef_pos, _sum_proof, check_round_trip, ref_batch
from test_wire_walk import CHALLENGE, OPEN_COMMITMENT, OPEN_RESPONSE, SUM_COMMITMENT, SUM_RESPONSE

pytestmark = pytest.mark.gpu

Q = O.Q_DEFAULT
HALF = (Q - 1) // 2
LINES = 32   # one-wavefront teams per CU of the unit / row kernels (the row scratch holds that many lines per CU)


def trips(ntasks, stride):
    return -(-ntasks // stride)


def boundary_entries(B, stride, nrows):
    """Batch entries on both sides of every trip boundary of a launch of B x nrows tasks with the given task stride."""
    out = set()
    t = stride
    while t < B * nrows:
        e = t // nrows
        out.update(x for x in (e - 1, e, e + 1 if t % nrows else e) if 0 <= x < B)
        t += stride
    return out


def team_stride(N, cus, env):
    """Task stride of the unit / row kernels: 32 one-wavefront teams per CU, 8 two-wavefront teams per CU at N = 2048
    (RZK_PAIR_POLY, default 1)."""
    pairs = N == 2048 and int(env.get("RZK_PAIR_POLY", 1)) != 0
    return (8 if pairs else LINES) * cus


def sample_entries(B, stride, seed, rows=(1, 4), extra=4):
    """First, last, both sides of each trip boundary at the given task stride (one task per entry and four rows per
    entry), a few drawn ones."""
    s = {0, B - 1}
    for r in rows:
        s |= boundary_entries(B, stride, r)
    rng = np.random.default_rng(seed)
    s |= set(int(v) for v in rng.integers(0, B, extra))
    return sorted(s)


def device_cus(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


def kernel_family(name):
    return re.sub(r"<[^<>]*>", "", name)


# ---- a. the knob -------------------------------------------------------------------------------------------------------
def scratch_bytes(ctx):
    total = C.c_size_t(0)
    assert ctx._L.rzk_debug_read_scratch(ctx._h, None, 0, C.byref(total)) == 0
    return total.value


def test_grid_cus_knob_sizes_the_scratch(torch_mod):
    cus = device_cus(torch_mod)
    full = scratch_bytes(make_ctx(1024, 1, 3, 1))
    one = scratch_bytes(make_ctx(1024, 1, 3, 1, env={"RZK_GRID_CUS": 1}))
    assert one > 0 and one * cus == full
    assert scratch_bytes(make_ctx(1024, 1, 3, 1, env={"RZK_GRID_CUS": 3})) == 3 * one
    # clamped to [1, multiProcessorCount]: 0 (and anything that is not a number) is 1, too many is the device's count
    assert scratch_bytes(make_ctx(1024, 1, 3, 1, env={"RZK_GRID_CUS": 0})) == one
    assert scratch_bytes(make_ctx(1024, 1, 3, 1, env={"RZK_GRID_CUS": "x"})) == one
    assert scratch_bytes(make_ctx(1024, 1, 3, 1, env={"RZK_GRID_CUS": cus + 1})) == full
    assert scratch_bytes(make_ctx(1024, 1, 3, 1, env={"RZK_GRID_CUS": 1 << 40})) == full


# ---- b. seeded sweep ---------------------------------------------------------------------------------------------------
def draw_trip_case(seed):
    rng = np.random.default_rng(13000 + seed)
    N = int(rng.choice([512, 1024, 1024, 2048]))
    nl = int(rng.choice([1, 1, 2, 3]))
    if N == 2048:
        nl = min(nl, 2)
    k = 2 * nl + int(rng.choice([1, 1, 2]))
    V = int(rng.choice([1, 2, 3] if N < 2048 else [1, 2]))
    env = dict(KNOBS[int(rng.integers(0, len(KNOBS)))])
    if seed < 3:
        # 1 CU, B = 15 / 16 / 17: one unit per task below 16 x CUs, all units of an entry per task from there on
        cus, B = 1, 15 + seed
    else:
        cus = 1 + seed % 3   # 3: a stride that is not a power of two
        # > 2 x 32 x cus entries: >= 3 trips even where a launch has one task per entry; row kernels make more
        B = 2 * LINES * cus + 1 + int(rng.integers(0, LINES * cus // 2))
    env["RZK_GRID_CUS"] = cus
    return dict(N=N, n=nl, k=k, l=nl, B=B, V=V, cus=cus, env=env)


# RZK_SWEEP_CASES / RZK_SWEEP_FIRST: a longer soak over other seeds
_SWEEP_N = int(os.environ.get("RZK_SWEEP_CASES", "24"))
_SWEEP_0 = int(os.environ.get("RZK_SWEEP_FIRST", "0"))
_SWEEP = list(range(_SWEEP_0, _SWEEP_0 + _SWEEP_N))


def _sweep_id(seed):
    cs = draw_trip_case(seed)
    return "s{}-N{}-{}{}{}-cus{}-B{}-entry_trips{}".format(seed, cs["N"], cs["n"], cs["k"], cs["l"], cs["cus"], cs["B"],
                                                            trips(cs["B"], team_stride(cs["N"], cs["cus"], cs["env"])))


def check_open_tamper_on_every_trip(ctx, B, stride, seed):
    """Open proofs tampered at the first entry of every trip (one task per entry) and at the last entry: exactly
    those reject, and the oracle agrees."""
    P = P_of(ctx)
    A, x, r, y, d, c, t, z = _open_proof(ctx, B, seed)
    bad = sorted(set(range(0, B, stride)) | {B - 1})
    zt = z.copy()
    for b in bad:
        zt[b, ctx.k - 1, ctx.N - 1] = O.center(int(zt[b, ctx.k - 1, ctx.N - 1]) + 1)
    want = np.ones(B, dtype=np.uint8)
    for b in bad:
        want[b] = int(O.open_verify(P, A, zt[b], t[b], c[b], d[b]) == 1)
    assert not want[bad].any()
    assert np.array_equal(ctx.open_verify(zt, t, c, d), want)


@pytest.mark.parametrize("seed", _SWEEP, ids=[_sweep_id(s) for s in _SWEEP])
def test_multi_trip_sweep_vs_oracle(torch_mod, seed):
    cs = draw_trip_case(seed)
    N, n, k, l, B, V, cus = (cs[key] for key in ("N", "n", "k", "l", "B", "V", "cus"))
    ctx = make_ctx(N, n, k, l, env=cs["env"])
    A = synth.key(np.random.default_rng(13100 + seed), N, n, k, l)
    ctx.load_key(A)
    # every entry at 1 CU; at 2 and 3 CUs the ends, both sides of every trip boundary and a few drawn entries
    stride = team_stride(N, cus, cs["env"])
    ent = None if cus == 1 else sample_entries(B, stride, 13500 + seed)
    check_key_products_and_open(ctx, A, B, 13200 + seed, entries=ent)
    check_linear_cycle(ctx, A, B, 13300 + seed, entries=ent)
    check_sum_cycle(torch_mod, ctx, A, B, V, 13400 + seed, device_too=seed % 4 == 0, entries=ent)
    check_open_tamper_on_every_trip(ctx, B, stride, 13600 + seed)


# ---- c. row_kernel's row rotation on and off ---------------------------------------------------------------------------
def linear_inputs(rng, P, B):
    N, k, l = P.N, P.k, P.l
    g = synth.uniform(rng, (B, N))
    x = synth.uniform(rng, (B, l, N))
    r, rp = synth.small(rng, (B, k, N)), synth.small(rng, (B, k, N))
    y, yp = synth.gauss(rng, (B, k, N), P.sigma), synth.gauss(rng, (B, k, N), P.sigma)
    d = synth.challenge(rng, (B,), N, P.kappa)
    return g, x, r, rp, y, yp, d


def bump(a, pos, delta=1):
    a[pos] = O.center(int(a[pos]) + delta)


@pytest.mark.parametrize("shape,cus,B,rotate", [
    # PG_LIN_V1 (the verifier with RZK_LIN_E=0) has n + n + l + l rows: n relation rows a1.z - c1(.)d - t, n for z',
    # l rows a2.z, l rows c2(.)g - c2'.  RZK_DKEY=2 puts the products by g on prepared images, so it runs on row_kernel.
    ((1, 3, 1), 1, 40, True),    # 4 rows, stride 32: 32 % 4 == 0, rotation; 160 tasks = 5 trips
    ((3, 7, 3), 1, 16, False),   # 12 rows, stride 32: no rotation; 192 tasks = 6 trips
    ((3, 7, 3), 3, 40, True),    # 12 rows, stride 96: rotation; 480 tasks = 5 trips
], ids=["131-cus1-rot", "373-cus1-norot", "373-cus3-rot"])
def test_row_rotation_linear_vs_oracle(torch_mod, shape, cus, B, rotate):
    n, k, l = shape
    N = 1024
    nrows, stride = 2 * n + 2 * l, LINES * cus
    assert (stride % nrows == 0) == rotate and trips(B * nrows, stride) >= 5
    ctx = make_ctx(N, n, k, l, env={"RZK_LIN_E": 0, "RZK_DKEY": 2, "RZK_GRID_CUS": cus})
    P = P_of(ctx)
    rng = np.random.default_rng(14000 + 10 * n + cus)
    A = synth.key(rng, N, n, k, l)
    ctx.load_key(A)
    g, x, r, rp, y, yp, d = linear_inputs(rng, P, B)
    c, cp, t, tp, u, ok = ctx.linear_commit(g, x, r, rp, y, yp)
    z, zp = ctx.linear_response(y, yp, r, rp, d)
    for b in range(B):
        ref = O.linear_commit(P, A, g[b], x[b], r[b], rp[b], y[b], yp[b])
        for got, want, name in zip((c, cp, t, tp, u), ref[:5], ("c", "cp", "t", "tp", "u")):
            assert np.array_equal(got[b], want), (name, b)
        assert int(ok[b]) == ref[5]
        zr, zpr = O.linear_response(P, y[b], yp[b], r[b], rp[b], d[b])
        assert np.array_equal(z[b], zr) and np.array_equal(zp[b], zpr), b
    # tampered z, z', u, g at the first entry of trips 1, 2, 3 (and one entry further on) and at the last entry
    first = lambda trip: trip * stride // nrows
    zt, zpt, ut, gt = z.copy(), zp.copy(), u.copy(), g.copy()
    bump(zt, (first(1), k - 1, N - 1))
    bump(zpt, (first(2), 0, 0))
    bump(ut, (first(3), l - 1, 5), -1)
    bump(gt, (first(3) + 1, 3))
    bump(zt, (B - 1, 0, 7))
    tampered = {first(1), first(2), first(3), first(3) + 1, B - 1}
    assert len(tampered) == 5 and all(first(1) <= b for b in tampered)
    ctx.prof_enable(True)
    ctx.prof_reset()
    acc = ctx.linear_verify(zt, zpt, c, cp, gt, t, tp, ut, d)
    names = [nm for nm, _ in ctx.prof_read_kernels()]
    ctx.prof_enable(False)
    want = [int(O.linear_verify(P, A, zt[b], zpt[b], c[b], cp[b], gt[b], t[b], tp[b], ut[b], d[b]) == 1)
            for b in range(B)]
    assert [i for i, v in enumerate(want) if not v] == sorted(tampered)
    assert acc.tolist() == want
    assert any(nm.startswith("row_kernel<10,") for nm in names), names


# ---- d. config 4 at its real batch -------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{}, {"RZK_LIN_E": 0}], ids=["default", "lin_e0"])
def test_config4_full_batch_vs_oracle(torch_mod, env):
    """Linear, N = 1024, (1,3,1), B = 8192 at the device's own grid, inputs from the device generators.

    default: config 4 as bench.py runs it.  The 4-row verifier is PG_LIN_V1B on unit_kernel, one task per entry; the
    row_kernel programs (PG_CMUL, PG_LIN_U, PG_LIN_V2B) have l = 1 row, so there is no rotation, and at 256 CUs
    (stride 8192) only shift_row_kernel makes more than one trip.  This pins the full batch as benchmarked.
    lin_e0: RZK_LIN_E=0.  The verifier's first program is PG_LIN_V1 with 2n + 2l = 4 rows on row_kernel (its product by
    g is a vector or prepared-image term): 32768 tasks, 4 trips at stride 8192, and the rotation on (8192 % 4 == 0)."""
    T = torch_mod
    N, n, k, l, B = 1024, 1, 3, 1, 8192
    cus = device_cus(T)
    stride = LINES * cus
    nrows = 2 * n + 2 * l                 # PG_LIN_V1 (lin_e0)
    rows_v1 = bool(env)
    if rows_v1:
        assert stride % nrows == 0 and trips(B * nrows, stride) >= 2   # 4 at 256 CUs
    ctx = make_ctx(N, n, k, l, env=env)
    P = P_of(ctx)
    dv = T.device("cuda", 0)
    gen = T.Generator(device=dv)
    gen.manual_seed(15000)
    A = synth.t_key(gen, N, n, k, l, dv)
    ctx.load_key(A)
    g, x = synth.t_uniform(gen, (B, N), dv), synth.t_uniform(gen, (B, l, N), dv)
    r, rp = synth.t_small(gen, (B, k, N), dv), synth.t_small(gen, (B, k, N), dv)
    y, yp = synth.t_gauss(gen, (B, k, N), dv, P.sigma), synth.t_gauss(gen, (B, k, N), dv, P.sigma)
    d = synth.t_challenge(gen, B, N, P.kappa, dv)
    c, cp, t, tp, u, ok = ctx.linear_commit(g, x, r, rp, y, yp)
    z, zp = ctx.linear_response(y, yp, r, rp, d)
    ctx.prof_enable(True)
    ctx.prof_reset()
    acc = ctx.linear_verify(z, zp, c, cp, g, t, tp, u, d)
    names = [nm for nm, _ in ctx.prof_read_kernels()]
    ctx.prof_enable(False)
    if rows_v1:
        assert names[0].startswith("row_kernel<10,"), names     # PG_LIN_V1 ran on row_kernel
    else:
        assert names[0].startswith("unit_kernel<10,"), names    # PG_LIN_V1B ran on unit_kernel
    H = lambda a: a.cpu().numpy()
    Ah = H(A)
    # entries: first, last, both sides of every trip boundary a launch with 1 - 4 rows per entry has at this stride
    # (for lin_e0 those of PG_LIN_V1 at entries 2048, 4096, 6144 at 256 CUs), the rest drawn
    ent = {0, B - 1}
    for rows in (1, 2, 3, 4):
        ent |= boundary_entries(B, stride, rows)
    rng = np.random.default_rng(15001)
    while len(ent) < 72:
        ent.add(int(rng.integers(0, B)))
    ent = sorted(ent)
    hs = {name: H(a) for name, a in dict(g=g, x=x, r=r, rp=rp, y=y, yp=yp, d=d, c=c, cp=cp, t=t, tp=tp, u=u, z=z,
                                         zp=zp).items()}
    okh, acch = H(ok), H(acc)
    for b in ent:
        ref = O.linear_commit(P, Ah, hs["g"][b], hs["x"][b], hs["r"][b], hs["rp"][b], hs["y"][b], hs["yp"][b])
        for name, want in zip(("c", "cp", "t", "tp", "u"), ref[:5]):
            assert np.array_equal(hs[name][b], want), (name, b)
        assert int(okh[b]) == ref[5], b
        zr, zpr = O.linear_response(P, hs["y"][b], hs["yp"][b], hs["r"][b], hs["rp"][b], hs["d"][b])
        assert np.array_equal(hs["z"][b], zr) and np.array_equal(hs["zp"][b], zpr), b
        want = O.linear_verify(P, Ah, hs["z"][b], hs["zp"][b], hs["c"][b], hs["cp"][b], hs["g"][b], hs["t"][b],
                               hs["tp"][b], hs["u"][b], hs["d"][b]) == 1
        assert int(acch[b]) == int(want), b
    assert int(acch.sum()) == B
    # tampered entries in each quarter of the batch (for lin_e0: on trips 0 .. 3 of PG_LIN_V1) and the last entry:
    # the exact verdict vector
    per_trip = stride // nrows
    bad = [5, per_trip + 7, 2 * per_trip + 11, 3 * per_trip + 13, B - 1]
    bad = sorted(set(b for b in bad if b < B))
    zt, zpt, ut, gt = z.clone(), zp.clone(), u.clone(), g.clone()
    for i, b in enumerate(bad):
        arr, pos = [(zt, (b, k - 1, N - 1)), (zpt, (b, 0, 0)), (ut, (b, l - 1, 5)), (gt, (b, 3))][i % 4]
        v = int(arr[pos])
        arr[pos] = v - 1 if v > 0 else v + 1
    got = H(ctx.linear_verify(zt, zpt, c, cp, gt, t, tp, ut, d))
    zth, zpth, uth, gth = H(zt), H(zpt), H(ut), H(gt)
    want = np.ones(B, dtype=np.uint8)
    for b in bad:
        want[b] = int(O.linear_verify(P, Ah, zth[b], zpth[b], hs["c"][b], hs["cp"][b], gth[b], hs["t"][b], hs["tp"][b],
                                      uth[b], hs["d"][b]) == 1)
    assert not want[bad].any()
    assert np.array_equal(got, want)


# ---- e. every row-program kernel on several trips ------------------------------------------------------------------------
E_CASES = [
    # (N, (n, k, l), V, B, env): all at 1 CU (stride 32 one-wavefront teams, 8 pairs at N = 2048)
    # N = 512 key products: unit_io_kernel, one team per entry from B = 16 on: 70 entries = 3 trips; shift_row_kernel
    (512, (1, 3, 1), 2, 70, {}),
    # N = 1024: unit_kernel; with RZK_DKEY=2 the products by g run on row_kernel (B x 4 rows = 9 trips)
    (1024, (1, 3, 1), 2, 70, {"RZK_DKEY": 2, "RZK_LIN_E": 0}),
    # row groups of two a1 rows (row_group_kernel, 4 waves per workgroup, 32 per CU): 70 x groups tasks >= 3 trips
    (1024, (2, 5, 2), 2, 70, {}),
    # shared-operand path: fwd_slots_kernel, then row_slots_kernel with 8 workgroups, one per XCD class; class 0
    # holds proofs 0, 8, 16 and its one workgroup walks their row groups in turn
    (1024, (2, 5, 2), 2, 20, {"RZK_ROW_GROUPS": 0, "RZK_BLOCK_MIN_LOGN": 12, "RZK_SLOT_SHARE_MIN": 1}),
    # row blocks at N = 1024: two workgroups per CU, OPEN_COMMIT at (4,9,4) takes two blocks per proof: 4 trips at B = 4
    (1024, (4, 9, 4), 2, 4, {"RZK_BLOCK_MIN_LOGN": 10}),
    # BASELINE config 3 and config 5 at B = 1 - 2 (row groups / row blocks at their own shapes)
    (1024, (4, 9, 4), 8, 2, {}),
    (2048, (8, 17, 8), 32, 1, {}),
]


def test_every_row_kernel_on_several_trips(torch_mod):
    seen = {}
    for i, (N, (n, k, l), V, B, env) in enumerate(E_CASES):
        ctx = make_ctx(N, n, k, l, env=dict(env, RZK_GRID_CUS=1))
        A = synth.key(np.random.default_rng(16000 + i), N, n, k, l)
        ctx.load_key(A)
        ent = sample_entries(B, team_stride(N, 1, env), 16100 + i) if B > 16 else None
        ctx.prof_enable(True)
        ctx.prof_reset()
        check_key_products_and_open(ctx, A, B, 16200 + i, entries=ent)
        if n <= 4:   # Linear commit at (8,17,8) has more rows than a row program holds (kMaxRows)
            check_linear_cycle(ctx, A, B, 16300 + i, entries=ent)
        check_sum_cycle(torch_mod, ctx, A, B, V, 16400 + i, device_too=False, entries=ent)
        for nm, _ in ctx.prof_read_kernels():
            seen.setdefault(kernel_family(nm), set()).add(i)
        ctx.prof_enable(False)
    # path selection that drifts away from a kernel fails here
    need = {"unit_kernel", "unit_io_kernel", "row_kernel", "shift_row_kernel", "row_group_kernel", "row_block_kernel",
            "fwd_slots_kernel + row_slots_kernel"}
    assert need <= set(seen), (sorted(need - set(seen)), sorted(seen))
    assert 3 in seen["fwd_slots_kernel + row_slots_kernel"] and 4 in seen["row_block_kernel"], seen


# ---- f. the grid does not change results ---------------------------------------------------------------------------------
def test_open_cycle_independent_of_grid(torch_mod):
    """Open, N = 1024, B = 4096: one team per entry, 128 trips at 1 CU, bit-equal to the device's own grid."""
    N, n, k, l, B = 1024, 1, 3, 1, 4096
    outs = []
    for env in ({"RZK_GRID_CUS": 1}, {}):
        ctx = make_ctx(N, n, k, l, env=env)
        P = P_of(ctx)
        rng = np.random.default_rng(17000)
        A = synth.key(rng, N, n, k, l)
        ctx.load_key(A)
        x = synth.uniform(rng, (B, l, N))
        r = synth.small(rng, (B, k, N))
        y = synth.gauss(rng, (B, k, N), P.sigma)
        d = synth.challenge(rng, (B,), N, P.kappa)
        c, t, ok = ctx.open_commit(x, r, y)
        z = ctx.open_response(y, r, d)
        zt = z.copy()
        bad = [0, 31, 32, 2047, 4064, B - 1]
        for b in bad:
            bump(zt, (b, b % k, b % N))
        acc, acct = ctx.open_verify(z, t, c, d), ctx.open_verify(zt, t, c, d)
        outs.append((c, t, ok, z, acc, acct))
    for name, a, b in zip(("c", "t", "ok", "z", "acc", "acc_tampered"), *outs):
        assert np.array_equal(a, b), name
    c, t, ok, z, acc, acct = outs[0]
    want = np.ones(B, dtype=np.uint8)
    want[bad] = 0
    assert np.array_equal(acc, np.ones(B, dtype=np.uint8)) and np.array_equal(acct, want)
    for b in (0, 31, 32, 4095):
        c_ref, t_ref, ok_ref = O.open_commit(P, A, x[b], r[b], y[b])
        assert np.array_equal(c[b], c_ref) and np.array_equal(t[b], t_ref) and bool(ok[b]) == ok_ref
        assert np.array_equal(z[b], O.open_response(P, y[b], r[b], d[b]))


def test_samplers_independent_of_grid(torch_mod):
    T = torch_mod
    cus = device_cus(T)
    N = 512
    one, full = make_ctx(N, 1, 3, 1, env={"RZK_GRID_CUS": 1}), make_ctx(N, 1, 3, 1)
    # uniform / gauss: 2 coefficients per thread, 16 x 256 threads per CU; challenge: 64 polynomials per CU
    coef_trip = 2 * 16 * 256 * cus
    npoly = 2 * coef_trip // N + 3              # > 2 trips at the device's grid, hundreds at 1 CU
    nchal = 2 * 64 * cus + 5
    for seed, stream in ((18000, 0), (18001, 7)):
        a, b = one.sample_uniform(seed, stream, HALF, (npoly,)), full.sample_uniform(seed, stream, HALF, (npoly,))
        assert T.equal(a, b) and int(a.abs().max()) <= HALF
        a, b = one.sample_gauss(seed, stream, 1000.0, (npoly,)), full.sample_gauss(seed, stream, 1000.0, (npoly,))
        assert T.equal(a, b)
        a, b = one.sample_challenge(seed, stream, (nchal,)), full.sample_challenge(seed, stream, (nchal,))
        assert T.equal(a, b) and T.equal((a != 0).sum(dim=1), T.full((nchal,), one.kappa, device=a.device))
    T.cuda.synchronize()


def test_primitives_one_cu_vs_oracle(torch_mod):
    """NTT, polymul, matvec, cmul, add / sub, norm2_le, eq and canonicalize at 1 CU on batches of several trips."""
    N, n, k, l = 1024, 1, 3, 1
    ctx = make_ctx(N, n, k, l, env={"RZK_GRID_CUS": 1})
    rng = np.random.default_rng(19000)
    A = synth.key(rng, N, n, k, l)
    ctx.load_key(A)
    B = 100                                        # 32 polynomials / entries per trip: 4 trips
    perm = ctx.ntt_layout()
    for prime in range(3):
        p, psi = ctx.ntt_prime(prime), ctx.ntt_psi(prime)
        x = rng.integers(0, p, (B, N), dtype=np.uint32)
        f = ctx.ntt_forward(prime, x)
        ref = O.ntt_forward_batch(x, p, psi)
        assert np.array_equal(f[:, perm], ref)
        assert np.array_equal(ctx.ntt_inverse(prime, f), x)
    a, b = synth.uniform(rng, (B, N)), synth.uniform(rng, (B, N))
    prod = ctx.polymul(a, b)
    for i in range(B):
        assert np.array_equal(prod[i], O.poly_mul(a[i], b[i])), i
    v = synth.uniform(rng, (B, k, N))
    mv = ctx.matvec(2, v)
    m, pm = synth.uniform(rng, (B, k, N)), synth.uniform(rng, (B, N))
    cm = ctx.cmul(m, pm)
    for i in range(B):
        assert np.array_equal(mv[i], O.mat_dot(A, v[i][:, None, :])[:, 0, :]), i
        assert np.array_equal(cm[i], O.mat_cmul(m[i][:, None, :], pm[i])[:, 0, :]), i
    # add / sub: 2 coefficients per thread, 8 workgroups of 256 threads at 1 CU = 4096 per trip: 75 trips
    s, df = ctx.add(v, m), ctx.sub(v, m)
    center = lambda w: np.where(w > HALF, w - Q, np.where(w < -HALF, w + Q, w))
    assert np.array_equal(s, center(v + m)) and np.array_equal(df, center(v - m))
    # norm2_le: one bound for the batch, every entry on its own side of it
    y = synth.gauss(rng, (B, k, N), 1000)
    norms = [max(O.norm2(y[i, j]) for j in range(k)) for i in range(B)]
    bound = int(np.median(norms))
    want = [int(O.check_norm(y[i], bound)) for i in range(B)]
    assert 0 < sum(want) < B
    assert ctx.norm2_le(y, bound).tolist() == want
    # eq: entries differing in one coefficient on every trip
    e2 = v.copy()
    diff = [0, 31, 32, 63, 64, 99]
    for i in diff:
        e2[i, i % k, (7 * i) % N] ^= 1
    want = [0 if i in diff else 1 for i in range(B)]
    assert ctx.eq(v, e2).tolist() == want
    # canonicalize: 32 workgroups of 256 threads at 1 CU: 13 trips
    raw = rng.integers(-2 ** 62, 2 ** 62, (B, N), dtype=np.int64)
    rem = np.mod(raw, Q)
    assert np.array_equal(ctx.canonicalize(raw), np.where(rem > HALF, rem - Q, rem))


# ---- g. the wire codec on later trips ------------------------------------------------------------------------------------
def _damage_late(msgs, cb, idx, ctx, c):
    """Copies of msgs with messages idx[0..3] damaged: coefficient HALF + 1, one coefficient short, the Vec count of t
    off by one, trailing bytes."""
    m = [bytes(x) for x in msgs]
    i0, i1, i2, i3 = idx
    x = bytearray(m[i0])
    p = _first_coef_pos(m[i0], OPEN_COMMITMENT, ctx, cb=cb)
    x[p:p + 8] = struct.pack("<q", HALF + 1)
    m[i0] = bytes(x)
    m[i1] = m[i1][:-cb]
    x = bytearray(m[i2])
    pos = 8 + sum(16 + len(np.trim_zeros(c[i2, j], "b")) * cb for j in range(ctx.n + ctx.l))
    assert struct.unpack_from("<Q", x, pos)[0] == ctx.n
    x[pos:pos + 8] = struct.pack("<Q", ctx.n + 1)
    m[i2] = bytes(x)
    m[i3] = m[i3] + b"\0" * cb
    return m


def test_wire_open_one_cu(torch_mod):
    """Open at B = 4096 under RZK_GRID_CUS=1: the walk makes 16 trips (256 messages each), copy / len / write 64
    polynomials per trip (192 trips for the 12288 polynomials of the commitments), the message scan 16 workgroups."""
    ctx = make_ctx(1024, 1, 3, 1, env={"RZK_GRID_CUS": 1})
    P = P_of(ctx)
    B = 4096
    A, x, r, y, d, c, t, z = _open_proof(ctx, B, 20000)
    com = check_round_trip(torch_mod, ctx, OPEN_COMMITMENT, [c, t])
    res = check_round_trip(torch_mod, ctx, OPEN_RESPONSE, [z])
    cha = check_round_trip(torch_mod, ctx, CHALLENGE, [d], device=False)
    assert wire.verify_open(ctx, com, cha, res).tolist() == [1] * B
    # damaged commitments on the last walk trip and the last copy trips, a tampered response on the last trip
    idx = [3841, 4000, 4094, B - 1]
    bad = _damage_late(com, 8, idx, ctx, c)
    ok = wire.decode_batch(ctx, OPEN_COMMITMENT, *wire.pack(bad))[-1]
    want = np.ones(B, dtype=np.uint8)
    want[idx] = 0
    assert np.array_equal(ok, want)
    zt = z.copy()
    bump(zt, (4093, 2, 5))
    assert O.open_verify(P, A, zt[4093], t[4093], c[4093], d[4093]) != 1
    want[4093] = 0
    res_t = ref_batch(ctx, OPEN_RESPONSE, [zt])
    assert np.array_equal(wire.verify_open(ctx, bad, cha, res_t), want)
    # the same from device buffers
    D = lambda pair: (dev(torch_mod, pair[0]), dev(torch_mod, pair[1].astype(np.int64)))
    gotd = wire.verify_open(ctx, D(wire.pack(bad)), D(wire.pack(cha)), D(wire.pack(res_t)))
    assert np.array_equal(gotd.cpu().numpy(), want)


def test_wire_sum_one_cu(torch_mod):
    """Sum, config 3 shape (4,9,4), V = 8, B = 40 under RZK_GRID_CUS=1: 120 polynomials per commitment (75 copy trips),
    the message scan over 40 messages with 16 workgroups (3 trips)."""
    N, n, k, l, V = 1024, 4, 9, 4, 8
    ctx = make_ctx(N, n, k, l, env={"RZK_GRID_CUS": 1})
    B = 40
    A, p = _sum_proof(ctx, B, V, 20100)
    com = check_round_trip(torch_mod, ctx, SUM_COMMITMENT, [p[k_] for k_ in ("cp", "cs", "gs", "tp", "ts", "u")], V=V)
    res = check_round_trip(torch_mod, ctx, SUM_RESPONSE, [p["zp"], p["zs"]], V=V)
    cha = ref_batch(ctx, CHALLENGE, [p["d"]])
    zs = p["zs"].copy()
    bump(zs, (B - 2, V - 1, k - 1, 9))
    res_t = ref_batch(ctx, SUM_RESPONSE, [p["zp"], zs], V=V)
    bad = list(com)
    bad[B - 1] = bad[B - 1][:-8]                     # truncated commitment: the last message
    want = ctx.sum_verify(zs, p["zp"], p["cs"], p["cp"], p["gs"], p["ts"], p["tp"], p["u"], p["d"]).tolist()
    assert want == [1] * (B - 2) + [0, 1]
    want[B - 1] = 0
    assert wire.verify_sum(ctx, V, bad, cha, res_t).tolist() == want
    assert wire.verify_sum(ctx, V, com, cha, res).tolist() == [1] * B
