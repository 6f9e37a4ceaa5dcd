"""Every kernel family against the oracle at the edges of the supported modulus range.

include/rzk.h: q odd, 1073692673 < q <= 4294606851; q reaches every kernel as a run-time value (DevTables::crt: about
twenty derived constants, 32-bit add / sub with wrap-around, Montgomery steps mod q, the one-add lift x + 2p).  The
modulus set is test_emul_modq.MODULI (Q_MIN, Q_B30, Q_A30, Q_A31, Q_DEF, Q_MAX; tests/test_emul_modq.py says why each).

A case is (ring degree, key shape, knobs, context parameters, helpers, kernel families).  The routes are those of the
table in tests/test_gpu_launch_names.py.  The helpers are the shared ones (check_key_products_and_open, check_sum_cycle of
test_gpu_baseline_shapes, check_linear_cycle of test_gpu_random_shapes) with edges=True: batch 3, V = 2, every result
compared with oracle/rzk_oracle.c for equality (norm flags included), one tampered proof per cycle, and
  * +-h, h = (q-1)/2, planted at coefficients 0, 63, 64, N-1, one polynomial all +h and one alternating -h, +h in every
    operand a kernel lifts and transforms: v of matvec, both factors of polymul, g / g_i, x, one entry of a1' and two of
    a2', and c, t on the verifier's side (plant_edges / plant_key_edges assert the planted values before the GPU runs);
  * below 2^30, r (.) d and c1 (.) d computed in numpy are asserted to hold sums in [-(2^32 - 4q), -1], whose low words
    lie past 4q (assert_rotation_band): the band in which the parent of this test's commit reduced a 64-bit rotation sum
    to [q, 2q) instead of [0, q) (zq_from_i64, rzk_core.h).
After the helpers of a case have run, the kernel names the context recorded (Context.prof_read_kernels) must include
every family the case names: a case cannot fall onto another kernel unnoticed.  FAMILY_CASES run at Q_MIN and Q_MAX,
ROTATION_CASES at all six moduli.  The element-wise kernels (add / sub / eq / norm / canonicalize) do not report names
and are compared with numpy only.

The side families that read the modulus (XP1 expansion, rejection step, 32-bit slabs, packed and wire codecs, the FS key
digest, the uniform samplers) run at Q_MIN, Q_A30 and Q_MAX against the project's Python references, which take q.
"""
import math

import numpy as np
import pytest

import fs_ref
import packed_ref as PR
import reject_ref as RR
import xof_ref
from oracle import oracle as O
from ring_zk_amd import fiat_shamir as FS
from ring_zk_amd import packed, synth, wire
from ring_zk_amd.backend import RzkError
from test_emul_modq import MODULI
from test_gpu_baseline_shapes import (assert_rotation_band, check_key_products_and_open, check_sum_cycle, dev, make_ctx,  # noqa: F401
                                      plant_edges, plant_key_edges, torch_mod)
from test_gpu_random_shapes import check_linear_cycle

pytestmark = pytest.mark.gpu

B, V = 3, 2
S131, S252 = (1, 3, 1), (2, 5, 2)
IMAGES = {"RZK_SUM_D": 1, "RZK_DKEY": 2}
R62 = 1 << 62
LNM = 12 / 11 + 1 / 242


def has_family(names, fam):
    """fam ending in '>' is a whole instantiation name, anything else a prefix."""
    return any(nm == fam if fam.endswith(">") else nm.startswith(fam) for nm in names)


def check_polymul(ctx, seed):
    q, N = ctx.q, ctx.N
    rng = np.random.default_rng(seed)
    a, b = synth.uniform(rng, (B, N), q), synth.uniform(rng, (B, N), q)
    plant_edges(a, ctx.half), plant_edges(b, ctx.half)
    b[1] = a[1]                                   # (-h, +h, ...)^2: every term of a coefficient's sum has one sign
    prod = ctx.polymul(a, b)
    for i in range(B):
        assert np.array_equal(prod[i], O.poly_mul(a[i], b[i], q)), i


def check_elementwise(ctx, seed):
    """add / sub / eq / norm2_le / canonicalize against numpy at the ends of the centred range."""
    q, N, h = ctx.q, ctx.N, ctx.half
    rng = np.random.default_rng(seed)
    a, b = synth.uniform(rng, (B, N), q), synth.uniform(rng, (B, N), q)
    plant_edges(a, h), plant_edges(b, h)
    b[2] = -a[2]                                  # h + h, -h - h, h - (-h): the sums furthest outside the range

    def centre(v):
        v = v % q
        return np.where(v > h, v - q, v)

    assert np.array_equal(ctx.add(a, b), centre(a + b)) and np.array_equal(ctx.sub(a, b), centre(a - b))
    assert np.array_equal(ctx.add(a, a), centre(2 * a)) and np.array_equal(ctx.sub(a, -a), centre(2 * a))
    wide = a.copy()
    wide[0, 1], wide[1, 2], wide[2, 3] = h + 1, -h - 1, q - 1          # any int64: canonicalize reduces it
    wide[0, 2], wide[1, 3], wide[2, 0] = (1 << 62) - 1, -(1 << 62), -q
    assert np.array_equal(ctx.canonicalize(wide), centre(wide))
    a3, b3 = a[:, None, :], a[:, None, :].copy()
    b3[1, 0, N - 1] = O.center(int(b3[1, 0, N - 1]) + 1, q)
    assert ctx.eq(a3, a3.copy()).tolist() == [1, 1, 1] and ctx.eq(a3, b3).tolist() == [1, 0, 1]
    sq = [sum(int(c) * int(c) for c in a[i]) for i in range(B)]       # up to N h^2 < 2^73: beyond 64 bits
    assert max(sq) == N * h * h and 8 * min(sq) < 7 * max(sq)          # the all +-h polynomials against the random one
    for bound in (math.isqrt(min(sq)) // 2, math.isqrt((min(sq) + max(sq)) // 2), 2 * math.isqrt(max(sq))):
        want = [int(s < (bound + 1) ** 2) for s in sq]                 # far from the limit: none, some, all
        assert ctx.norm2_le(a3, bound).tolist() == want


def check_response_reject(torch, ctx, seed):
    """open_response_reject: z against the oracle, accept and E against tests/reject_ref.py (the fused statistic runs in
    response_stat_kernel at N = 512 / 1024)."""
    from test_gpu_response_reject import check, inputs

    P = RR.params_of(ctx)
    rng = np.random.default_rng(seed)
    ins, coin = inputs(rng, ctx, P, "open", B), RR.coins(rng, B, R62)
    assert_rotation_band(ins[1], ins[2], ctx.q)
    want, acc, E = check(torch, ctx, P, "open", ins, coin)
    z, _, _ = ctx.open_response_reject(*ins, coin, R62, LNM)
    Po = O.Params(N=ctx.N, n=ctx.n, k=ctx.k, l=ctx.l, kappa=ctx.kappa, b=ctx.b, q=ctx.q)
    for i in range(B):
        assert np.array_equal(z[i], O.open_response(Po, ins[0][i], ins[1][i], ins[2][i])), i
    assert all(w[1] == 0 for w in want)


HELPERS = {
    "open": lambda T, ctx, A, s: check_key_products_and_open(ctx, A, B, s, edges=True),
    "linear": lambda T, ctx, A, s: check_linear_cycle(ctx, A, B, s + 1, edges=True),
    "sum": lambda T, ctx, A, s: check_sum_cycle(T, ctx, A, B, V, s + 2, device_too=False, edges=True),
    "polymul": lambda T, ctx, A, s: check_polymul(ctx, s + 3),
    "stat": lambda T, ctx, A, s: check_response_reject(T, ctx, s + 4),
    "elementwise": lambda T, ctx, A, s: check_elementwise(ctx, s + 5),
}


def run_case(torch, q, N, shape, env, kw, helpers, families):
    n, k, l = shape
    ctx = make_ctx(N, n, k, l, env=env, q=q, **kw)
    try:
        assert ctx.q == q and ctx.half == (q - 1) // 2
        seed = 88000 + N + 7 * n + q % 1000
        A = plant_key_edges(synth.key(np.random.default_rng(seed), N, n, k, l, q), n, l, ctx.half)
        ctx.load_key(A)
        ctx.prof_enable(True)
        ctx.prof_reset()
        for name in helpers:
            HELPERS[name](torch, ctx, A, seed)
        ctx.synchronize()
        names = sorted({nm for nm, _ in ctx.prof_read_kernels()})
        for fam in families:
            assert has_family(names, fam), (fam, names)
    finally:
        ctx.close()


def case_id(c):
    N, shape, env, kw = c[:4]
    knobs = "+".join(f"{k[4:]}={v}" for k, v in env.items()) or "default"
    return f"{N}-{''.join(map(str, shape))}-{knobs}" + "".join(f"-{k}{v}" for k, v in kw.items())


ALL3 = ["open", "linear", "sum", "polymul"]
# (N, shape, knobs, context parameters, helpers, families that must have run)
FAMILY_CASES = [
    # unit_io_kernel: the default at 512, forced at 1024 and on the two-wavefront teams of 2048
    (512, S131, {}, {}, ALL3 + ["elementwise"],
     ["unit_io_kernel<9, false>", "unit_io_kernel<9, true>", "row_kernel<9, false, WaveTeam, false>", "row_kernel<9, true, WaveTeam, false>"]),
    (1024, S131, {"RZK_UNIT_IO": 1}, {}, ["open", "linear"], ["unit_io_kernel<10, false>", "unit_io_kernel<10, true>"]),
    (2048, S131, {"RZK_UNIT_IO": 1}, {}, ["open"], ["unit_io_kernel<11, false, PairTeam>"]),
    # unit_kernel: with and without the twiddle image at 1024, two- and one-wavefront teams at 2048, the vector x vector
    # variants, and the longer lane-level forms behind their knobs
    (1024, S131, {}, {}, ALL3,
     ["unit_kernel<10, false, false>", "unit_kernel<10, false, true>", "row_kernel<10, false, WaveTeam, false>", "row_kernel<10, true, WaveTeam, false>"]),
    (1024, S131, {"RZK_TW_LDS": 0}, {}, ["open"], ["unit_kernel<10, false, false>", "unit_kernel<10, false, true>"]),
    (2048, S131, {}, {}, ["open", "sum", "polymul"],
     ["unit_kernel<11, false, false, PairTeam>", "unit_kernel<11, false, true, PairTeam>", "row_kernel<11, false, PairTeam, false>",
      "row_kernel<11, true, PairTeam, false>"]),
    (2048, S131, {"RZK_PAIR_POLY": 0}, {}, ["open", "polymul"], ["unit_kernel<11, false, false>", "row_kernel<11, false, WaveTeam, false>"]),
    (1024, S131, {"RZK_VEC_ROWS": 0}, {}, ["linear", "sum", "polymul"], ["unit_kernel<10, true, false>", "unit_kernel<10, true, true>"]),
    (1024, S131, {"RZK_ROT_LAST": 0}, {}, ["open"], ["unit_kernel<10, false, true>"]),
    (1024, S131, {"RZK_DOT2": 0, "RZK_CRT2_SHORT": 0}, {}, ["open", "linear"], ["unit_kernel<10, false, false>", "unit_kernel<10, false, true>"]),
    # rows that read the call's operand images (TERM_DD) and the prepared multiplier images
    (1024, S131, IMAGES, {}, ["sum"], ["row_kernel<10, false, WaveTeam, true>", "dkey_transform_kernel<10>"]),
    (512, S131, IMAGES, {}, ["linear", "sum"], ["row_kernel<9, false, WaveTeam, true>", "dkey_transform_kernel<9>"]),
    # rows that share operands: groups, blocks, slots (key-only programs store two primes; the full-range v of matvec
    # needs the third: the slots' more-primes-than-stored fallback)
    (1024, S252, {}, {}, ["open", "sum"], ["row_group_kernel<10"]),
    (1024, S252, IMAGES, {}, ["sum"], ["row_group_kernel<10", "dkey_transform_kernel<10>"]),   # (operand images produced by the group kernel)
    (2048, S252, {}, {}, ["open"], ["row_block_kernel<11, BlockPairTeam>"]),
    (1024, S252, {"RZK_BLOCK_MIN_LOGN": 10}, {}, ["open", "sum"], ["row_block_kernel<10>"]),
    (1024, S252, {"RZK_ROW_GROUPS": 0, "RZK_BLOCK_MIN_LOGN": 12}, {}, ["open", "sum"], ["fwd_slots_kernel<10> + row_slots_kernel<10>"]),
    (2048, S252, {"RZK_BLOCK_MIN_LOGN": 12}, {}, ["open"], ["fwd_slots_kernel<11> + row_slots_kernel<11>"]),
    # the schoolbook kernel of small rings
    (64, S131, {}, {}, ALL3 + ["elementwise", "stat"], ["row_kernel_small"]),
    (4, S131, {}, {"kappa": 2}, ["open", "polymul", "elementwise"], ["row_kernel_small"]),
]

# the rotation paths: every route through shift_product / shift_product_bytes and the statistic kernel
ROTATION_CASES = [
    (512, S131, {}, {}, ["open", "stat"], ["shift_row_kernel<9, false>", "response_stat_kernel<9, false>", "unit_io_kernel<9, true>"]),
    (1024, S131, {}, {}, ["open", "stat"], ["shift_row_kernel<10, false>", "response_stat_kernel<10, false>", "unit_kernel<10, false, true>"]),
    (512, S131, {"RZK_SHIFT_BYTES": 0}, {}, ["open", "stat"], ["shift_row_kernel<9, false, WaveTeam, false>", "response_stat_kernel<9, false, false>"]),
    (1024, S131, {"RZK_SHIFT_BYTES": 0}, {}, ["open", "stat", "linear"],
     ["shift_row_kernel<10, false, WaveTeam, false>", "response_stat_kernel<10, false, false>"]),
    # |d|_1 2 |r|_inf = 360 > 255: the packed-byte kernels take the word path term by term
    (1024, S131, {}, {"kappa": 60, "b": 3}, ["open", "stat"], ["shift_row_kernel<10, false>", "response_stat_kernel<10, false>"]),
    (2048, S131, {}, {}, ["open", "stat"], ["shift_row_kernel<11, false, PairTeam>", "unit_kernel<11, false, true, PairTeam>"]),
    (1024, S252, {}, {}, ["open"], ["shift_row_kernel<10"]),
    # control: the same products by transforms
    (1024, S131, {"RZK_SHIFT": 0}, {}, ["open", "stat"], ["row_kernel<10", "reject_stat_kernel"]),
]


@pytest.mark.parametrize("qname", ["Q_MIN", "Q_MAX"])
@pytest.mark.parametrize("case", FAMILY_CASES, ids=[case_id(c) for c in FAMILY_CASES])
def test_kernel_family_at_the_ends_of_the_modulus_range(torch_mod, case, qname):
    N, shape, env, kw, helpers, families = case
    run_case(torch_mod, MODULI[qname], N, shape, env, kw, helpers, families)


@pytest.mark.parametrize("qname", sorted(MODULI))
@pytest.mark.parametrize("case", ROTATION_CASES, ids=[case_id(c) for c in ROTATION_CASES])
def test_rotation_paths_at_every_edge_modulus(torch_mod, case, qname):
    N, shape, env, kw, helpers, families = case
    run_case(torch_mod, MODULI[qname], N, shape, env, kw, helpers, families)


# ---- side families that read the modulus ----------------------------------------------------------------------------------
SIDE = ["Q_MIN", "Q_A30", "Q_MAX"]


@pytest.mark.parametrize("qname", SIDE)
@pytest.mark.parametrize("N", [64, 512])
def test_xp1_expansion(torch_mod, N, qname):
    """xof_uniform (domain 5) and expand_key (domain 0) bit for bit against tests/xof_ref.py.  At Q_A30 the 31-bit mask
    accepts barely half of the candidates: the squeeze loop's extra blocks."""
    q = MODULI[qname]
    ctx = make_ctx(N, 1, 3, 1, q=q, kappa=min(N, 36))
    seeds = [xof_ref.seed_of(3000 + N + i) for i in range(3)]
    sa = np.frombuffer(b"".join(seeds), dtype=np.uint8).reshape(3, 32).copy()
    want = xof_ref.uniform(q, N, 5, seeds, 2)
    assert int(np.abs(want).max()) <= ctx.half
    assert np.array_equal(ctx.xof_uniform(sa, 2, 5), want)
    assert np.array_equal(ctx.xof_uniform(dev(torch_mod, sa), 2, 5).cpu().numpy(), want)
    assert np.array_equal(ctx.expand_key(seeds[0]), xof_ref.key(q, N, 1, 3, 1, seeds[0]))


@pytest.mark.parametrize("qname", SIDE)
def test_rejection_step(torch_mod, qname):
    """reject against tests/reject_ref.py: honest parts, then z and y at +-h, so that z - y spans (-q, q) and its centring
    wraps 32 bits above 2^31."""
    q = MODULI[qname]
    ctx = make_ctx(512, 1, 3, 1, q=q)
    P = RR.params_of(ctx)
    h = ctx.half
    rng = np.random.default_rng(q % 9973)
    z, y = RR.honest(rng, P, 4, 3)
    coin = RR.coins(rng, 4, R62)
    # a coefficient of magnitude h always breaks the norm rule, so these proofs are rejected; what is compared is E, the
    # exact statistic over v = centred(z - y), which the library must wrap the same way
    z[1, 0, :4], y[1, 0, :4] = [h, -h, h, -h], [-h, h, h - 5, 3 - h]   # v = 2h - q = -1, +1 (wrapped), 5, -3
    z[2, 1, 63], y[2, 1, 63] = h, -h + 40                              # v = -41 (wrapped): beyond vmax = 36
    z[3, 2, 511], y[3, 2, 511] = -h, 0                                 # v = -h
    want = RR.run(P, [(z, y)], coin, R62, LNM)
    assert [w[1] for w in want] == [0, RR.NORM, RR.VMAX | RR.NORM, RR.VMAX | RR.NORM]
    acc, E = ctx.reject([(z, y)], coin, R62, LNM)
    for i, w in enumerate(want):
        assert int(E[i]) == w[0], i
        if w[3]:
            assert int(acc[i]) == int(w[2]), i
        assert not (w[1] and acc[i]), i
    dacc, dE = ctx.reject([(dev(torch_mod, z), dev(torch_mod, y))], dev(torch_mod, coin), R62, LNM)
    assert np.array_equal(dacc.cpu().numpy(), acc) and np.array_equal(dE.cpu().numpy(), E)


@pytest.mark.parametrize("qname", SIDE)
def test_slab32_calls(torch_mod, qname):
    """narrow / widen and the 32-bit Open calls at N = 512 with +-h planted, against the 64-bit calls and the oracle;
    h + 1 as an int32 is refused (at Q_MAX it lies 180221 below the int32 limit)."""
    q = MODULI[qname]
    N, n, k, l = 512, 1, 3, 1
    ctx = make_ctx(N, n, k, l, q=q)
    h = ctx.half
    P = O.Params(N=N, n=n, k=k, l=l, q=q)
    rng = np.random.default_rng(q % 7919)
    A = plant_key_edges(synth.key(rng, N, n, k, l, q), n, l, h)
    ctx.load_key(A)
    x = plant_edges(synth.uniform(rng, (B, l, N), q), h)
    r, y, d = synth.small(rng, (B, k, N)), synth.gauss(rng, (B, k, N), P.sigma), synth.challenge(rng, (B,), N, P.kappa)
    assert_rotation_band(r, d, q)
    x32 = ctx.narrow(x)
    assert x32.dtype == np.int32 and np.array_equal(x32, x) and np.array_equal(ctx.widen(x32), x)
    assert h + 1 < 2 ** 31
    bad = x.copy()
    bad[1, 0, 64] = h + 1
    with pytest.raises(RzkError):
        ctx.narrow(bad)
    n32 = lambda *arrs: [np.ascontiguousarray(a.astype(np.int32)) for a in arrs]
    ctx.prof_enable(True)
    ctx.prof_reset()
    c32, t32, ok32 = ctx.open_commit32(*n32(x, r, y))
    z32 = ctx.open_response32(*n32(y, r, d))
    acc32 = ctx.open_verify32(z32, t32, c32, *n32(d))
    names = sorted({nm for nm, _ in ctx.prof_read_kernels()})
    for fam in ("unit_io_kernel<9, false, i32>", "unit_io_kernel<9, true, i32>", "shift_row_kernel<9, false, i32>"):
        assert has_family(names, fam), (fam, names)
    c, t, ok = ctx.open_commit(x, r, y)
    z = ctx.open_response(y, r, d)
    assert np.array_equal(c32, c) and np.array_equal(t32, t) and np.array_equal(z32, z) and np.array_equal(ok32, ok)
    for i in range(B):
        c_ref, t_ref, ok_ref = O.open_commit(P, A, x[i], r[i], y[i])
        assert np.array_equal(c32[i], c_ref) and np.array_equal(t32[i], t_ref) and bool(ok32[i]) == ok_ref
        assert np.array_equal(z32[i], O.open_response(P, y[i], r[i], d[i]))
    assert acc32.tolist() == [1] * B
    xb = x32.copy()
    xb[2, 0, 0] = h + 1                                                # int32, outside the centred range
    with pytest.raises(RzkError):
        ctx.open_commit32(xb, *n32(r, y))
    cb = c32.copy()
    cb[1, 0, 5] = -h - 1
    assert ctx.open_verify32(z32, t32, cb, *n32(d)).tolist() == [1, 0, 1]


@pytest.mark.parametrize("qname", SIDE)
def test_packed_codec(torch_mod, qname):
    """The packed format against tests/packed_ref.py: field widths from the modulus and the verify bound, record sizes,
    records bit for bit with both ends of every class planted, round trip."""
    from test_gpu_packed import decode_both, encode_both, rand_fields, ref_ctx

    q = MODULI[qname]
    ctx = make_ctx(512, 1, 3, 1, q=q)
    ref = ref_ctx(ctx)
    assert ref == PR.make_ctx(512, 1, 3, 1, q)
    cl = PR.classes(ref)
    assert packed.widths(ctx) == (cl["Q"].W, cl["Z"].W) and cl["Q"].W == (q - 1).bit_length()
    rng = np.random.default_rng(q % 6007)
    for kind in (packed.MSG_OPEN_COMMITMENT, packed.MSG_OPEN_RESPONSE, packed.MSG_OPEN_SHORT):
        assert packed.record_bytes(ctx, kind) == PR.record_bytes(ref, kind)
        slabs = rand_fields(rng, ctx, kind, None, B)
        want, wok = PR.encode(ref, kind, slabs, None)
        rec, ok = encode_both(torch_mod, ctx, kind, slabs, None)
        assert wok.tolist() == [1] * B and np.array_equal(ok, wok) and np.array_equal(rec, want), kind
        back, bok = decode_both(torch_mod, ctx, kind, rec, None)
        assert bok.tolist() == [1] * B and all(np.array_equal(a, b) for a, b in zip(back, slabs)), kind


@pytest.mark.parametrize("coef_bytes", [8, 4])
@pytest.mark.parametrize("qname", SIDE)
def test_wire_codec_range_test(torch_mod, qname, coef_bytes):
    """The wire codec's decode on the GPU: +-h accepted, +-(h+1) clears ok of that message only; encode -> decode round trip."""
    q = MODULI[qname]
    N, n, k, l = 512, 1, 3, 1
    ctx = make_ctx(N, n, k, l, q=q)
    h = ctx.half
    rng = np.random.default_rng(q % 5003 + coef_bytes)
    z = plant_edges(synth.uniform(rng, (4, k, N), q), h)
    data, offsets = wire.encode_batch(ctx, wire.MSG_OPEN_RESPONSE, z, coef_bytes=coef_bytes)
    back, ok = wire.decode_batch(ctx, wire.MSG_OPEN_RESPONSE, data, offsets, coef_bytes=coef_bytes)
    assert ok.tolist() == [1] * 4 and np.array_equal(back, z)
    msgs = wire.split(data, offsets)
    for b in range(4):
        assert msgs[b] == wire.mat_encode(z[b][:, None, :], coef_bytes)
    zb = z.copy()
    zb[2, 1, 64], zb[3, 2, N - 1] = h + 1, -h - 1
    bad = [wire.mat_encode(zb[b][:, None, :], coef_bytes) for b in range(4)]
    pd, po = wire.pack(bad)
    _, okb = wire.decode_batch(ctx, wire.MSG_OPEN_RESPONSE, pd, po, coef_bytes=coef_bytes)
    assert okb.tolist() == [1, 1, 0, 0]
    _, okd = wire.decode_batch(ctx, wire.MSG_OPEN_RESPONSE, dev(torch_mod, pd), dev(torch_mod, po.astype(np.int64)), coef_bytes=coef_bytes)
    assert okd.cpu().numpy().tolist() == [1, 1, 0, 0]


@pytest.mark.parametrize("qname", SIDE)
def test_key_digest(torch_mod, qname):
    """The FS1 key digest carries q in its header, and its leaves hold key coefficients up to +-h."""
    q = MODULI[qname]
    N, n, k, l = 512, 2, 5, 2
    ctx = make_ctx(N, n, k, l, q=q)
    A = plant_key_edges(synth.key(np.random.default_rng(q % 4001), N, n, k, l, q), n, l, ctx.half)
    ctx.load_key(A)
    assert FS.key_digest(ctx) == fs_ref.key_digest(A, q, N, n, k, l, ctx.kappa, ctx.b)
    other = make_ctx(N, n, k, l)
    other.load_key(np.where(np.abs(A) > other.half, 0, A))
    assert FS.key_digest(other) != FS.key_digest(ctx)


@pytest.mark.parametrize("qname", SIDE)
def test_uniform_samplers_cover_the_centred_range(torch_mod, qname):
    q = MODULI[qname]
    ctx = make_ctx(512, 1, 3, 1, q=q)
    h = ctx.half
    u = ctx.sample_uniform(1, 0, h, (16,)).cpu().numpy()
    assert u.min() >= -h and u.max() <= h and u.max() > 0.99 * h and u.min() < -0.99 * h
    ctx.set_sampler_key(bytes(range(32)))
    uk = ctx.sample_uniform_keyed(bytes(16), 0, h, (16,)).cpu().numpy()
    assert uk.min() >= -h and uk.max() <= h and uk.max() > 0.99 * h and uk.min() < -0.99 * h
