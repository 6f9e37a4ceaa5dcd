"""The unit kernels' shorter forms (GPU): rotation terms last with their sums in registers (RZK_ROT_LAST), two-product key
rows with one reduction (RZK_DOT2), the two-prime reconstruction with one reduction mod q (RZK_CRT2_SHORT); all default 1
(include/rzk.h).  Every form computes the same values as the path it replaces, so every result is compared bit for bit
with the oracle AND with the same call on contexts created with each knob switched off on its own (and all three off):

  * the Open commit and verify at N = 512 / 1024, (1,3,1), B = 1 / 5 — N = 512 also under RZK_UNIT_IO=0, where the
    key-product programs run on unit_kernel as at N = 1024 instead of unit_io_kernel; and at N = 2048 on teams of two
    and (RZK_PAIR_POLY=0) of one wavefront, where only the shorter reconstruction applies: rotation terms at N = 2048
    exist on teams of two only, which run them first, and two-product rows keep one reduction per product;
  * the relation row a1.z - c1 (.) d with ANY multiplier d through the rotation-last path, stored (open_recover) and
    tested against zero (open_verify): d all zeros, dense ternary, and dense full-range against a full-range c1, whose
    sums exceed 2^62 and take the two-pass 16-bit fallback;
  * z, t or c1 tampered at one coefficient: the reject pattern of the oracle, whatever the knobs;
  * a non-canonical coefficient of c1 or d clears exactly that proof's verdict;
  * 101 proofs on a grid sized for one CU (32 teams, one task per proof): teams 0 .. 4 make four trips, every other
    team three (its slab, P and registers reused);
  * the paths that keep the old forms: a Linear cycle at (1,3,1), whose commit program has pair units and whose verifier
    rows carry one key product in front of their rotation term (the planner never pairs a row that has rotation terms:
    plan_units, rzk_plan.h), and one at (1,4,1), whose rows have three key products.
Which form a unit takes is invisible from outside; the lane-level arithmetic is pinned on the CPU
(tests/test_emul_unit_diet.py).  Reference: src/prove/open.rs:80-174, src/prove/linear.rs:82-250.
"""
import numpy as np
import pytest

from oracle import oracle as O
from ring_zk_amd import synth

from test_gpu_baseline_shapes import P_of, make_ctx, torch_mod  # noqa: F401
from test_gpu_random_shapes import check_linear_cycle

pytestmark = pytest.mark.gpu

KNOBS = ("RZK_ROT_LAST", "RZK_DOT2", "RZK_CRT2_SHORT")
ALL_ON = {k: 1 for k in KNOBS}
ALL_OFF = {k: 0 for k in KNOBS}
ONE_OFF = [dict(ALL_ON, **{k: 0}) for k in KNOBS]

_ctxs, _keys = {}, {}


def key_of(N, shape):
    if (N, shape) not in _keys:
        _keys[N, shape] = synth.key(np.random.default_rng(8100 + N + sum(shape)), N, *shape)
    return _keys[N, shape]


def ctx_of(N, knobs, shape=(1, 3, 1), **extra):
    ident = (N, shape, tuple(sorted(knobs.items())), tuple(sorted(extra.items())))
    if ident not in _ctxs:
        ctx = make_ctx(N, *shape, env=dict(knobs, **extra))
        ctx.load_key(key_of(N, shape))
        _ctxs[ident] = ctx
    return _ctxs[ident]


def open_inputs(N, B, seed):
    P = P_of(ctx_of(N, ALL_ON))
    rng = np.random.default_rng(seed)
    return (synth.uniform(rng, (B, 1, N)), synth.small(rng, (B, 3, N)), synth.gauss(rng, (B, 3, N), P.sigma),
            synth.challenge(rng, (B,), N, P.kappa))


def same(outs, other):
    for a, b in zip(outs, other):
        assert a.dtype == b.dtype and np.array_equal(a, b)


def ref_verdicts(N, z, t, c, d):
    P, A = P_of(ctx_of(N, ALL_ON)), key_of(N, (1, 3, 1))
    return [int(O.open_verify(P, A, z[b], t[b], c[b], d[b]) == 1) for b in range(z.shape[0])]


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("N,extra", [(512, {}), (512, {"RZK_UNIT_IO": 0}), (1024, {}), (2048, {}), (2048, {"RZK_PAIR_POLY": 0})],
                         ids=["512", "512-unit_kernel", "1024", "2048-teams-of-two", "2048-one-wavefront"])
def test_open_commit_and_verify_vs_oracle_and_each_knob_off(torch_mod, N, extra, B):
    on = ctx_of(N, ALL_ON, **extra)
    P, A = P_of(on), key_of(N, (1, 3, 1))
    x, r, y, d = open_inputs(N, B, 8200 + N + B)
    c, t, ok = on.open_commit(x, r, y)
    z = on.open_response(y, r, d)
    zt = z.copy()
    zt[B - 1, 2, N - 1] = O.center(int(zt[B - 1, 2, N - 1]) + 1)   # the last proof once more, tampered
    acc, acct = on.open_verify(z, t, c, d), on.open_verify(zt, t, c, d)
    for b in range(B):
        c_ref, t_ref, ok_ref = O.open_commit(P, A, x[b], r[b], y[b])
        assert np.array_equal(c[b], c_ref) and np.array_equal(t[b], t_ref) and bool(ok[b]) == ok_ref, b
    assert acc.tolist() == ref_verdicts(N, z, t, c, d) == [1] * B
    assert acct.tolist() == ref_verdicts(N, zt, t, c, d) == [1] * (B - 1) + [0]
    for knobs in ONE_OFF + [ALL_OFF]:
        off = ctx_of(N, knobs, **extra)
        same((c, t, ok), off.open_commit(x, r, y))
        same((acc, acct), (off.open_verify(z, t, c, d), off.open_verify(zt, t, c, d)))


@pytest.mark.parametrize("N,extra", [(512, {"RZK_UNIT_IO": 0}), (1024, {})], ids=["512-unit_kernel", "1024"])
def test_any_multiplier_through_the_rotation_last_path(torch_mod, N, extra):
    on = ctx_of(N, ALL_ON, **extra)
    P, A = P_of(on), key_of(N, (1, 3, 1))
    rng = np.random.default_rng(8300 + N)
    ds = [np.zeros(N, dtype=np.int64), rng.integers(-1, 2, N), synth.uniform(rng, (N,)), synth.challenge(rng, (1,), N, P.kappa)[0]]
    d = np.ascontiguousarray(np.stack(ds))
    B = d.shape[0]
    z = synth.gauss(rng, (B, 3, N), P.sigma)
    c = synth.uniform(rng, (B, 2, N))         # full-range c1: |d|_1 |c1|_inf > 2^62 for the dense full-range d
    assert float(np.abs(d[2]).sum()) * float(np.abs(c[2, 0]).max()) > 2.0 ** 62
    t, acc = on.open_recover(z, c, d)
    for b in range(B):                        # t = a1.z - c1 (.) d, the relation row stored instead of tested
        w = O.mat_dot(A[:1], z[b][:, None, :])[:, 0, :]
        assert np.array_equal(t[b, 0], O.poly_sub(w[0], O.poly_mul(c[b, 0], d[b]))), b
    tt = t.copy()
    tt[1, 0, 5] = O.center(int(tt[1, 0, 5]) - 1)
    tt[2, 0, N - 1] = O.center(int(tt[2, 0, N - 1]) + 1)
    v, vt = on.open_verify(z, t, c, d), on.open_verify(z, tt, c, d)
    assert v.tolist() == ref_verdicts(N, z, t, c, d) == acc.tolist()
    assert vt.tolist() == ref_verdicts(N, z, tt, c, d) and vt.tolist()[1:3] == [0, 0] and vt[0] == v[0] and vt[3] == v[3]
    for knobs in ONE_OFF + [ALL_OFF]:
        off = ctx_of(N, knobs, **extra)
        same((t, acc), off.open_recover(z, c, d))
        same((v, vt), (off.open_verify(z, t, c, d), off.open_verify(z, tt, c, d)))


@pytest.mark.parametrize("N", [512, 1024])
def test_tampered_and_noncanonical_coefficients(torch_mod, N):
    extra = {"RZK_UNIT_IO": 0} if N == 512 else {}
    on, off = ctx_of(N, ALL_ON, **extra), ctx_of(N, ALL_OFF, **extra)
    B = 6
    x, r, y, d = open_inputs(N, B, 8400 + N)
    c, t, _ = on.open_commit(x, r, y)
    z = on.open_response(y, r, d)
    zt, tt, ct = z.copy(), t.copy(), c.copy()
    zt[0, 1, 3] = O.center(int(zt[0, 1, 3]) + 1)
    tt[2, 0, N // 2] = O.center(int(tt[2, 0, N // 2]) - 1)
    ct[4, 0, N - 1] = O.center(int(ct[4, 0, N - 1]) + 1)            # c1 enters through the rotation term
    ct[5, 1, 0] = O.center(int(ct[5, 1, 0]) + 1)                    # c2 is not part of the relation: still accepted
    for zz, ts, cc, want in ((zt, t, c, [0, 1, 1, 1, 1, 1]), (z, tt, c, [1, 1, 0, 1, 1, 1]), (z, t, ct, [1, 1, 1, 1, 0, 1]),
                             (zt, tt, ct, [0, 1, 0, 1, 0, 1])):
        got = on.open_verify(zz, ts, cc, d)
        assert got.tolist() == want == ref_verdicts(N, zz, ts, cc, d)
        same((got,), (off.open_verify(zz, ts, cc, d),))
    # a coefficient outside the centred range is never read as its low word: exactly that proof is rejected
    cb, db = c.copy(), d.copy()
    cb[1, 0, 7] += 1 << 32
    db[3, int(np.flatnonzero(d[3] == 0)[0])] = 1 << 32
    for ctx in (on, off):
        assert ctx.open_verify(z, t, cb, d).tolist() == [1, 0, 1, 1, 1, 1]
        assert ctx.open_verify(z, t, c, db).tolist() == [1, 1, 1, 0, 1, 1]
        assert ctx.open_verify(z, t, c, d).tolist() == [1] * B


def test_at_least_three_trips_per_team(torch_mod):
    # One CU: the unit kernels' grid is 8 workgroups of 4 one-wavefront teams = 32 teams, and from B >= 16 on a task is
    # one proof: team i evaluates proofs i, i + 32, i + 64, i + 96.  B = 101: teams 0 .. 4 make four trips (the last
    # trip is partial), teams 5 .. 31 three.
    N, B, teams = 1024, 101, 32
    assert min(len(range(i, B, teams)) for i in range(teams)) == 3
    on, off = ctx_of(N, ALL_ON, RZK_GRID_CUS=1), ctx_of(N, ALL_OFF, RZK_GRID_CUS=1)
    P, A = P_of(on), key_of(N, (1, 3, 1))
    x, r, y, d = open_inputs(N, B, 8500)
    c, t, ok = on.open_commit(x, r, y)
    z = on.open_response(y, r, d)
    zt = z.copy()
    bad = [teams - 1, teams, 2 * teams - 1, 2 * teams, 3 * teams - 1, 3 * teams, B - 1]   # both sides of every trip boundary, the last proof
    for b in bad:
        zt[b, b % 3, (17 * b) % N] = O.center(int(zt[b, b % 3, (17 * b) % N]) + 1)
    acc, acct = on.open_verify(z, t, c, d), on.open_verify(zt, t, c, d)
    assert acc.tolist() == [1] * B and acct.tolist() == [0 if b in bad else 1 for b in range(B)]
    for b in [0, teams + 1, 2 * teams + 1, 3 * teams + 1] + bad:
        c_ref, t_ref, ok_ref = O.open_commit(P, A, x[b], r[b], y[b])
        assert np.array_equal(c[b], c_ref) and np.array_equal(t[b], t_ref) and bool(ok[b]) == ok_ref, b
        assert O.open_verify(P, A, z[b], t[b], c[b], d[b]) == 1 and (O.open_verify(P, A, zt[b], t[b], c[b], d[b]) == 1) == (b not in bad)
    same((c, t, ok), off.open_commit(x, r, y))
    same((acc, acct), (off.open_verify(z, t, c, d), off.open_verify(zt, t, c, d)))


@pytest.mark.parametrize("shape", [(1, 3, 1), (1, 4, 1)], ids=["pairs-and-one-product-rotation-rows", "three-product-rows"])
def test_linear_cycles_on_the_old_paths(torch_mod, shape):
    N, B = 1024, 3
    A = key_of(N, shape)
    for knobs in (ALL_ON, ALL_OFF):     # both oracle-equal, hence equal to each other
        check_linear_cycle(ctx_of(N, knobs, shape=shape), A, B, 8600 + sum(shape))
