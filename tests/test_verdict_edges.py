"""Verdict edges, CPU tier: the generators behind tests/test_gpu_verdict_edges.py, in Python integers.

norm_edge must hit its sum of squares exactly, stay below the clamp of the exact sum (2^24), put its weight where the
style says, and flip the oracle's norm predicate exactly between L - 1 and L, L = (bound + 1)^2.  Which path of the
kernels a planned sum exercises (exact re-sum inside the band L (1 +- 2^-16), float total outside) is derived here from
rational arithmetic on S and L alone, never from the library.  fault_positions must reach every coefficient once and every
(row, lane) and (row, register) pair; the two passes of sweep_faults together must fault every coefficient.
"""
import numpy as np
import pytest

from oracle import oracle as O
from ring_zk_amd import synth

SIZES = (512, 1024, 2048)
STYLE_POS = [("point", 0), ("point", 63), ("point", 64), ("point", "half-3"), ("point", "N-3"), ("spread", 0),
             ("upper", 0), ("lower", 0), ("lastreg", 0), ("wave2", 0)]


def position(N, pos):
    return {"half-3": N // 2 - 3, "N-3": N - 3}.get(pos, pos)


def bounds(N):
    """(bound, L) of every norm predicate the GPU tier meets at this N."""
    out = set()
    for n, k, l in ((1, 3, 1), (2, 5, 2)):
        P = O.Params(N=N, n=n, k=k, l=l, kappa=36, b=1)
        out |= {P.verify_bound, P.commit_bound}
    return sorted(out)


def sq(p):
    return sum(int(v) * int(v) for v in p)


@pytest.mark.parametrize("N", SIZES)
def test_norm_edge_hits_every_planned_sum_exactly(N):
    rng = np.random.default_rng(N)
    half = N // 2
    for bound in bounds(N):
        L = (bound + 1) ** 2
        assert L < 1 << 48
        for name, S in synth.norm_plan(L).items():
            for style, pos in STYLE_POS:
                at = position(N, pos)
                p = synth.norm_edge(N, S, style, at, rng)
                assert p.shape == (N,) and sq(p) == S, (bound, name, style, pos)
                assert max(abs(int(v)) for v in p) < 1 << 24
                nz = {i for i in range(N) if p[i]}
                if style == "point":
                    assert nz <= {(at + i) % N for i in range(5)} and p[at] == synth.isqrt(S)
                elif style == "spread":
                    assert len(nz) == N
                elif style == "upper":
                    assert nz == set(range(half, N))
                elif style == "lower":
                    assert nz == set(range(half))
                elif style == "lastreg":
                    assert nz == set(range(N - 64, N))
                else:
                    assert nz == {i for i in range(N) if i & 64}
                if style != "point":
                    assert {int(v) < 0 for v in p if v} == {True, False}     # both signs occur
    # the two point positions that matter most really straddle / wrap
    p = synth.norm_edge(N, (bounds(N)[0] + 1) ** 2 - 1, "point", N // 2 - 3, rng)
    assert p[half - 1] and p[half] and p[half + 1]
    p = synth.norm_edge(N, (bounds(N)[0] + 1) ** 2 - 1, "point", N - 3, rng)
    assert p[N - 1] and p[0] and p[1]


@pytest.mark.parametrize("N", SIZES)
def test_oracle_predicate_flips_between_below_and_at(N):
    rng = np.random.default_rng(100 + N)
    for bound in bounds(N):
        L = (bound + 1) ** 2
        plan = synth.norm_plan(L)
        for style, pos in STYLE_POS:
            below = synth.norm_edge(N, plan["below"], style, position(N, pos), rng)
            at = synth.norm_edge(N, plan["at"], style, position(N, pos), rng)
            assert O.norm2(below) == bound and O.norm2(at) == bound + 1
            assert O.check_norm(below[None], bound) and not O.check_norm(at[None], bound)
        for name, S in plan.items():
            p = synth.norm_edge(N, S, "spread", 0, rng)
            assert O.check_norm(p[None], bound) == (S < L), name


@pytest.mark.parametrize("N", SIZES)
def test_planned_sums_take_their_intended_path(N):
    for bound in bounds(N):
        L = (bound + 1) ** 2
        plan = synth.norm_plan(L)
        assert len(set(plan.values())) == len(plan) == 9
        assert (plan["below"], plan["at"], plan["above"]) == (L - 1, L, L + 1)
        # in band by more than the float total's documented error (2^-18): only the exact sum can decide
        for name in ("below", "at", "above"):
            assert abs(plan[name] - L) * 2 ** 17 <= L and synth.norm_path(plan[name], L) == "exact", name
        # far outside the band L (1 +- 2^-16): the float total decides
        for name in ("far_lo", "far_hi"):
            assert abs(plan[name] - L) * 2 ** 15 >= L and synth.norm_path(plan[name], L) == "float", name
        assert plan["far_lo"] < L < plan["far_hi"]
        # the band's own edges, ceil(L 2^-19) to either side: either path may run (float total within 2^-18 of S)
        step = -(-L // 2 ** 19)
        for name, edge, side in (("lo_out", -1, -1), ("lo_in", -1, 1), ("hi_in", 1, -1), ("hi_out", 1, 1)):
            S = plan[name]
            centre = L * (2 ** 16 + edge)          # 2^16 x the band edge
            assert abs(S * 2 ** 16 - (centre + side * step * 2 ** 16)) <= 2 ** 15, name   # rounding of the edge only
            assert synth.norm_path(S, L) == "edge", name
        assert plan["lo_out"] < plan["lo_in"] < L < plan["hi_in"] < plan["hi_out"]


def test_four_squares():
    for m in list(range(0, 400)) + [2 * 4 ** 9, 6 * 4 ** 5, 14 * 4 ** 3, 2 * 679536, 2 ** 22 + 12345]:
        a, b, c, d = synth.four_squares(m)
        assert a * a + b * b + c * c + d * d == m and a >= b >= c >= d >= 0
        four = synth.four_squares(m, nonzero=True)
        brute = any(m - a * a - b * b - c * c > 0 and synth.isqrt(m - a * a - b * b - c * c) ** 2 == m - a * a - b * b - c * c
                    for a in range(1, 21) for b in range(1, a + 1) for c in range(1, b + 1)) if m < 400 else None
        if four is None:
            assert not brute
        else:
            assert all(v > 0 for v in four) and sum(v * v for v in four) == m
            assert brute in (None, True)


ROWS = (1, 2, 3, 4, 5, 6, 9, 10)          # the row counts of the operands the GPU sweeps fault


@pytest.mark.parametrize("N", SIZES)
def test_fault_positions_cover_lanes_and_registers(N):
    for rows in ROWS:
        for offset in (0, 1):
            fp = synth.fault_positions(N, rows, offset)
            assert [c for _, c in fp] == list(range(N)) and {r for r, _ in fp} == set(range(rows))
            # a 64-lane team (coefficient e * 64 + lane): every (row, register), and every (row, lane) once rows <= N / 64
            assert {(r, c // 64) for r, c in fp} == {(r, e) for r in range(rows) for e in range(N // 64)}
            if rows <= N // 64:
                assert {(r, c % 64) for r, c in fp} == {(r, ln) for r in range(rows) for ln in range(64)}
    # three rows (z, z', r, y at k = 3) also meet every thread of a two-wavefront team (coefficient e * 128 + t)
    fp = synth.fault_positions(N, 3)
    assert {(r, c % 128) for r, c in fp} == {(r, t) for r in range(3) for t in range(128)}


@pytest.mark.parametrize("N", SIZES)
def test_sweep_faults_reach_every_coefficient(N):
    """The two passes of a position sweep: clean entries (i + i // 64) % 8 == 0, then == 4, rows stepped by one in between."""
    for rows in ROWS:
        seen, pairs64, pairs128 = set(), set(), set()
        for pass_ in (0, 1):
            ent, rr, cc = synth.sweep_faults(N, rows, pass_)
            assert len(ent) == N - N // 8 and set(ent.tolist()) == {i for i in range(N) if (i + i // 64) % 8 != 4 * pass_}
            assert cc.tolist() == ent.tolist() and int(rr.max()) < rows
            seen |= set(cc.tolist())
            pairs64 |= {(int(r), int(c) % 64) for r, c in zip(rr, cc)}
            pairs128 |= {(int(r), int(c) % 128) for r, c in zip(rr, cc)}
        assert seen == set(range(N))
        if rows <= N // 64:
            assert pairs64 == {(r, ln) for r in range(rows) for ln in range(64)}, rows
        if N == 2048 and rows in (1, 2, 3, 5, 6):    # what the sweeps fault in two-wavefront teams
            assert pairs128 == {(r, t) for r in range(rows) for t in range(128)}, rows
