"""All vector twiddles of the N = 1024 unit kernels from one LDS image per sixteen-team workgroup (RZK_TW_LDS=2, include/rzk.h; GPU).

The image holds the same table entries the global tables hold, so a context created with RZK_TW_LDS=2 must give the bytes
and verdicts of one created with RZK_TW_LDS=1 (phase-2 image, four-team workgroups) and of one with RZK_TW_LDS=0 (global
tables), all kernels of the same library, and all must match the oracle:
  * Open commit / response / verify at N = 1024, (1,3,1), B = 5, with z tampered at one coefficient and a non-canonical
    coefficient of c1: the exact reject pattern;
  * B = 1 and B = 17 with every unit of a proof in one task (RZK_UPT=16: one task per proof): one workgroup with fifteen
    teams that have no task — they fill their share of the image, meet the barrier and leave —, then a second workgroup
    with one busy team;
  * the same cycle at B = 101 on a grid sized for one CU (RZK_GRID_CUS=1: ONE workgroup of 16 teams, one task per proof):
    teams 0 .. 4 make seven trips, every other team six, over one fill of the image.  The contexts are compared on every
    proof, the oracle on both sides of trip boundaries and the last proof;
  * a matvec with full-range operands, whose bound asks for the third prime and with it the third pair of images;
  * the 32-bit entry points open_commit32 / open_response32 / open_verify32 at B = 5 (the i32 instantiations share the body);
  * one Linear cycle at B = 3, whose launches mix kernels with the image (unit_kernel, the HAS_VEC instantiations among
    them) and without it (row_kernel, shift_row_kernel).
All three paths report the same kernel names.  What the image holds and which words a lane reads is pinned on the CPU
(tests/test_emul_tw3_lds.py).  Reference: src/prove/open.rs:80-174, src/mat.rs:95-115, src/prove/linear.rs:82-250.
"""
import numpy as np
import pytest

from oracle import oracle as O
from ring_zk_amd import synth

from test_gpu_baseline_shapes import P_of, make_ctx, torch_mod  # noqa: F401
from test_gpu_random_shapes import check_linear_cycle

pytestmark = pytest.mark.gpu

N, SHAPE = 1024, (1, 3, 1)
MODES = (2, 1, 0)
_ctxs, _memo = {}, {}


def key():
    if "key" not in _memo:
        _memo["key"] = synth.key(np.random.default_rng(9960), N, *SHAPE)
    return _memo["key"]


def ctx_of(tw, **extra):
    ident = (tw, tuple(sorted(extra.items())))
    if ident not in _ctxs:
        ctx = make_ctx(N, *SHAPE, env=dict(extra, RZK_TW_LDS=tw))
        ctx.load_key(key())
        _ctxs[ident] = ctx
    return _ctxs[ident]


def open_inputs(B, seed):
    P = P_of(ctx_of(2))
    rng = np.random.default_rng(seed)
    return (synth.uniform(rng, (B, 1, N)), synth.small(rng, (B, 3, N)), synth.gauss(rng, (B, 3, N), P.sigma),
            synth.challenge(rng, (B,), N, P.kappa))


def same(outs, other):
    for a, b in zip(outs, other):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def names_of(ctx, call):
    ctx.prof_enable(True)
    ctx.prof_reset()
    out = call()
    names = [nm for nm, _ in ctx.prof_read_kernels()]
    ctx.prof_enable(False)
    return out, names


def test_open_cycle_three_paths_vs_oracle_and_reject_pattern(torch_mod):
    B = 5
    full = ctx_of(2)
    P, A = P_of(full), key()
    x, r, y, d = open_inputs(B, 9961)
    (c, t, ok), names_c = names_of(full, lambda: full.open_commit(x, r, y))
    assert "unit_kernel<10, false, false>" in names_c, names_c
    z = full.open_response(y, r, d)
    for b in range(B):
        c_ref, t_ref, ok_ref = O.open_commit(P, A, x[b], r[b], y[b])
        assert np.array_equal(c[b], c_ref) and np.array_equal(t[b], t_ref) and bool(ok[b]) == ok_ref, b
        assert np.array_equal(z[b], O.open_response(P, y[b], r[b], d[b])), b
    zt = z.copy()
    zt[1, 2, N - 1] = O.center(int(zt[1, 2, N - 1]) + 1)       # tampered z: proof 1
    zt[4, 0, 0] = O.center(int(zt[4, 0, 0]) - 1)               # ... and proof 4
    cb = c.copy()
    cb[3, 0, 7] += 1 << 32                                     # non-canonical c1: proof 3, never read as its low word
    acc, names_v = names_of(full, lambda: full.open_verify(z, t, c, d))
    assert "unit_kernel<10, false, true>" in names_v, names_v
    assert acc.tolist() == [1] * B == [int(O.open_verify(P, A, z[b], t[b], c[b], d[b]) == 1) for b in range(B)]
    acct, accb = full.open_verify(zt, t, c, d), full.open_verify(z, t, cb, d)
    assert acct.tolist() == [1, 0, 1, 1, 0] == [int(O.open_verify(P, A, zt[b], t[b], c[b], d[b]) == 1) for b in range(B)]
    assert accb.tolist() == [1, 1, 1, 0, 1]
    for tw in MODES[1:]:
        other = ctx_of(tw)
        (c0, t0, ok0), names_c0 = names_of(other, lambda: other.open_commit(x, r, y))
        acc0, names_v0 = names_of(other, lambda: other.open_verify(z, t, c, d))
        assert names_c0 == names_c and names_v0 == names_v, (tw, names_c0, names_v0)
        same((c, t, ok, z), (c0, t0, ok0, other.open_response(y, r, d)))
        same((acc, acct, accb), (acc0, other.open_verify(zt, t, c, d), other.open_verify(z, t, cb, d)))


@pytest.mark.parametrize("B", [1, 17])
def test_idle_teams_reach_the_barrier(torch_mod, B):
    # One task per proof: B = 1 is one workgroup with fifteen idle teams, B = 17 adds a second workgroup with one busy team.
    ctxs = [ctx_of(tw, RZK_UPT=16) for tw in MODES]
    full = ctxs[0]
    P, A = P_of(full), key()
    x, r, y, d = open_inputs(B, 9962 + B)
    c, t, ok = full.open_commit(x, r, y)
    z = full.open_response(y, r, d)
    zt = z.copy()
    zt[B - 1, 1, 3] = O.center(int(zt[B - 1, 1, 3]) + 1)       # the last proof: the second workgroup's only task at B = 17
    acc, acct = full.open_verify(z, t, c, d), full.open_verify(zt, t, c, d)
    assert acc.tolist() == [1] * B and acct.tolist() == [1] * (B - 1) + [0]
    for b in sorted({0, B - 1}):
        c_ref, t_ref, ok_ref = O.open_commit(P, A, x[b], r[b], y[b])
        assert np.array_equal(c[b], c_ref) and np.array_equal(t[b], t_ref) and bool(ok[b]) == ok_ref, b
        assert np.array_equal(z[b], O.open_response(P, y[b], r[b], d[b])), b
        assert O.open_verify(P, A, z[b], t[b], c[b], d[b]) == 1 and (O.open_verify(P, A, zt[b], t[b], c[b], d[b]) == 1) == (b != B - 1), b
    for other in ctxs[1:]:
        same((c, t, ok, z), other.open_commit(x, r, y) + (other.open_response(y, r, d),))
        same((acc, acct), (other.open_verify(z, t, c, d), other.open_verify(zt, t, c, d)))


def test_the_image_survives_six_and_seven_trips_per_team(torch_mod):
    # One CU: the grid of the sixteen-team workgroups is ONE workgroup, and from B >= 16 on a task is one proof: team i
    # evaluates proofs i, i + 16, ...  B = 101: teams 0 .. 4 make seven trips, teams 5 .. 15 six.
    B, teams = 101, 16
    assert sorted({len(range(i, B, teams)) for i in range(teams)}) == [6, 7]
    ctxs = [ctx_of(tw, RZK_GRID_CUS=1) for tw in MODES]
    full = ctxs[0]
    P, A = P_of(full), key()
    x, r, y, d = open_inputs(B, 9970)
    c, t, ok = full.open_commit(x, r, y)
    z = full.open_response(y, r, d)
    zt = z.copy()
    bad = [teams - 1, teams, 3 * teams - 1, 3 * teams, 6 * teams - 1, 6 * teams, B - 1]   # both sides of trip boundaries (first, middle, last), the last proof
    for b in bad:
        zt[b, b % 3, (17 * b) % N] = O.center(int(zt[b, b % 3, (17 * b) % N]) + 1)
    acc, acct = full.open_verify(z, t, c, d), full.open_verify(zt, t, c, d)
    assert acc.tolist() == [1] * B and acct.tolist() == [0 if b in bad else 1 for b in range(B)]
    for b in [0] + bad:
        c_ref, t_ref, ok_ref = O.open_commit(P, A, x[b], r[b], y[b])
        assert np.array_equal(c[b], c_ref) and np.array_equal(t[b], t_ref) and bool(ok[b]) == ok_ref, b
        assert np.array_equal(z[b], O.open_response(P, y[b], r[b], d[b])), b
        assert O.open_verify(P, A, z[b], t[b], c[b], d[b]) == 1 and (O.open_verify(P, A, zt[b], t[b], c[b], d[b]) == 1) == (b not in bad), b
    for other in ctxs[1:]:
        same((c, t, ok, z), other.open_commit(x, r, y) + (other.open_response(y, r, d),))
        same((acc, acct), (other.open_verify(z, t, c, d), other.open_verify(zt, t, c, d)))


def test_full_range_matvec_takes_the_third_primes_images(torch_mod):
    B = 3
    full = ctx_of(2)
    A = key()
    v = synth.uniform(np.random.default_rng(9980), (B, 3, N))
    # |a|_2 |v|_2 of one product alone (a1 = [1 | a1']: column 1 is a full-range entry) is beyond what two primes hold (P/2 < 2^59)
    assert float(np.sqrt((A[0, 1].astype(np.float64) ** 2).sum())) * float(np.sqrt((v[0, 1].astype(np.float64) ** 2).sum())) > 2.0 ** 60
    out, names = names_of(full, lambda: full.matvec(2, v))
    assert any(nm.startswith("unit_kernel<10,") for nm in names), names
    for b in range(B):
        assert np.array_equal(out[b], O.mat_dot(A, v[b][:, None, :])[:, 0, :]), b
    for tw in MODES[1:]:
        same((out,), (ctx_of(tw).matvec(2, v),))


def test_open32_entry_points(torch_mod):
    B = 5
    full = ctx_of(2)
    P, A = P_of(full), key()
    x, r, y, d = open_inputs(B, 9990)
    n32 = lambda a: np.ascontiguousarray(a.astype(np.int32))
    w64 = lambda a: np.ascontiguousarray(a.astype(np.int64))
    (c, t, ok), names = names_of(full, lambda: full.open_commit32(n32(x), n32(r), n32(y)))
    assert "unit_kernel<10, false, false, i32>" in names, names
    z = full.open_response32(n32(y), n32(r), n32(d))
    zt = z.copy()
    zt[2, 1, 5] += 1
    acc, acct = full.open_verify32(z, t, c, n32(d)), full.open_verify32(zt, t, c, n32(d))
    for b in range(B):
        c_ref, t_ref, ok_ref = O.open_commit(P, A, x[b], r[b], y[b])
        assert np.array_equal(w64(c[b]), c_ref) and np.array_equal(w64(t[b]), t_ref) and bool(ok[b]) == ok_ref, b
        assert np.array_equal(w64(z[b]), O.open_response(P, y[b], r[b], d[b])), b
    assert acc.tolist() == [1] * B and acct.tolist() == [1, 1, 0, 1, 1]
    assert [int(O.open_verify(P, A, w64(zt[b]), w64(t[b]), w64(c[b]), d[b]) == 1) for b in range(B)] == [1, 1, 0, 1, 1]
    for tw in MODES[1:]:
        other = ctx_of(tw)
        same((c, t, ok, z), other.open_commit32(n32(x), n32(r), n32(y)) + (other.open_response32(n32(y), n32(r), n32(d)),))
        same((acc, acct), (other.open_verify32(z, t, c, n32(d)), other.open_verify32(zt, t, c, n32(d))))


def test_linear_cycle_with_vector_products(torch_mod):
    A = key()
    check_linear_cycle(ctx_of(2), A, 3, 9995)    # the default paths: unit_kernel for the key products, row_kernel for vector x vector
    # RZK_VEC_ROWS=0: the vector x vector programs on unit_kernel too (the HAS_VEC instantiations)
    full = ctx_of(2, RZK_VEC_ROWS=0)
    rng = np.random.default_rng(9996)
    a, b = synth.uniform(rng, (2, N)), synth.uniform(rng, (2, N))
    prod, names = names_of(full, lambda: full.polymul(a, b))
    assert names == ["unit_kernel<10, true, false>"], names
    for tw in MODES:     # all oracle-equal at every entry, hence equal to each other
        check_linear_cycle(ctx_of(tw, RZK_VEC_ROWS=0), A, 3, 9995)
        same((prod,), (ctx_of(tw, RZK_VEC_ROWS=0).polymul(a, b),))
