"""Verdict edges on the GPU: every decision a row-program kernel takes from its own loads, at its edge.

Three verdicts never pass through the products that the rest of the suite pins: the fused norm predicate
sum c^2 < (bound + 1)^2 (float total outside the band L (1 +- 2^-16), exact integer re-sum inside: load_lift,
load_measure / norm_below, checked_add_verdicts, each over WaveTeam / PairTeam sums), the canonical-range test of every
loaded coefficient, and the zero test of a relation row.  Honest responses are far below the bound and tampered proofs
fail the relation, so a sum that lost a lane, a register or a wavefront would pass everything else.

  * norm cases: polynomials from synth.norm_edge at the sums of synth.norm_plan (L - 1, L, L + 1; either side of the
    band's own edges; L (1 -+ 2^-15)), weight at a point (positions 0, 63, 64, N/2 - 3, N - 3), over all coefficients,
    one half, the last 64 or the second wavefront's share, in one carrying row at a time among honest rows; a coefficient
    above the clamp and a full-range one (92 polynomials per limit; every one runs in Open, Commitment::verify,
    Linear and Sum; where an operand has 9 rows, and in Sum, the L - 1 / L pairs go to every row and the rest to one
    cycling row).  The relation stays true (commitments zero, t / u / c solved with the
    oracle's Mat operations), so the expected verdict is the oracle's check_norm of the crafted polynomial; the
    oracle's verifier confirms it on a sample of entries.
  * position sweeps: one valid proof from the oracle, B = N entries, entry i with one fault at coefficient i, the row
    cycling (synth.fault_positions), one entry in eight clean, in two passes that together fault every coefficient
    (synth.sweep_faults): c -+ q (same residue, only the range test can reject), c + 2^32, +-2^31, and +-1
    (the zero test); trusted-producer mode; the prover side.  Open's verifier reads only the first n rows of c
    (a1.z = t + c1 (.) d), so the sweep of c covers those.

Batches: 40 entries per call in the norm cases; 72 (24 in two-wavefront teams) where one team has to make three trips.
The whole file takes about 5 s on an MI355X; DESIGN.md section 5 has the figures and the mutants it was checked against.

Kernel names come from the profiler, so a routing change cannot quietly empty a case.
"""
import functools
import time

import numpy as np
import pytest

from oracle import oracle as O
from ring_zk_amd import synth
from ring_zk_amd.backend import RzkError
from test_gpu_baseline_shapes import P_of, dev, make_ctx, torch_mod  # noqa: F401
from test_gpu_prime_count_edges import KEY_CASES, VEC_CASES, run_prof, sum_mod

pytestmark = pytest.mark.gpu

Q = O.Q_DEFAULT
HALF = (Q - 1) // 2
CHUNK = 40               # batch entries per call of a norm case
SAMPLE = 16              # entries per case confirmed by the oracle's own verifier


def styles(N):
    return [("point", p) for p in (0, 63, 64, N // 2 - 3, N - 3)] + [(s, 0) for s in synth.NORM_STYLES[1:]]


@functools.lru_cache(maxsize=None)
def edge_polys(N, bound):
    """[(label, polynomial, oracle's check_norm)] for one limit: the whole plan x every style, one coefficient above the
    clamp of the exact sum, one full-range coefficient at N - 1.  Built once per (N, bound) and shared."""
    rng = np.random.default_rng(41000 + N + bound % 1000)
    out = []
    for name, S in synth.norm_plan((bound + 1) ** 2).items():
        for style, pos in styles(N):
            out.append((f"{name}/{style}@{pos}", synth.norm_edge(N, S, style, pos, rng)))
    huge = np.zeros(N, dtype=np.int64)
    huge[int(rng.integers(65, N))] = (1 << 24) + 5
    full = np.zeros(N, dtype=np.int64)
    full[N - 1] = HALF
    out += [("huge", huge), ("full", full)]
    res = []
    for lab, p in out:
        p.setflags(write=False)
        res.append((lab, p, int(O.check_norm(p[None], bound))))
    assert {w for _, _, w in res} == {0, 1}
    return res


def placements(polys, k, thin=False):
    """(polynomial index, carrying row): every row for every polynomial; thin (many rows): every row for the L - 1 / L
    pairs, one cycling row for the rest."""
    out = []
    for i, (lab, _, _) in enumerate(polys):
        every = not thin or lab.startswith(("below", "at"))
        out += [(i, j) for j in range(k) if every or j == i % k]
    return out


def col_dot(A, rows, j, p):
    """A[rows, j] (.) p as [len(rows)][N] (oracle)."""
    return O.mat_dot(A[rows, j:j + 1], np.ascontiguousarray(p)[None, None, :])[:, 0, :]


def madd(a, b):
    return O.mat_add(a[:, None, :], b[:, None, :])[:, 0, :]


def msub(a, b):
    return O.mat_sub(a[:, None, :], b[:, None, :])[:, 0, :]


def dot(A, v):
    return O.mat_dot(A, v[:, None, :])[:, 0, :]


def cmul(m, p):
    return O.mat_cmul(m[:, None, :], p)[:, 0, :]


class Swap:
    """A . v for vectors that differ from a base vector v0 in one row: A.v = A.v0 - A[:, j] v0_j + A[:, j] p."""

    def __init__(self, A, v0):
        self.A, self.v0 = A, v0
        self.rows = np.arange(A.shape[0])
        self.base = dot(A, v0)
        self.cols = {}

    def __call__(self, j, p):
        if j not in self.cols:
            self.cols[j] = col_dot(self.A, self.rows, j, self.v0[j])
        return madd(msub(self.base, self.cols[j]), col_dot(self.A, self.rows, j, p))


def chunks(n, size=CHUNK):
    return [range(s, min(s + size, n)) for s in range(0, n, size)]


def sample(n, m=SAMPLE):
    return sorted({(i * n) // m for i in range(m)})


# ---- Open verify ---------------------------------------------------------------------------------------------------------
# Shapes and knob sets are those of test_gpu_prime_count_edges.py (KEY_CASES: id, N, shape, env, batch, family of the key
# products; VEC_CASES: id, N, env, family), so the two files cannot drift apart.
_KEY = {c[0]: c for c in KEY_CASES}
_VEC = {c[0]: c for c in VEC_CASES}
SHIFT0 = dict(_VEC["1024-shift0"][2])          # the challenge product by transforms instead of rotations


def key_case(cid, fam=None, extra=None, name=None):
    """(id, N, shape, env, family) of KEY_CASES[cid]; fam where this file's entry point runs on another family."""
    _, N, shape, env, _, kfam = _KEY[cid]
    return (name or cid, N, shape, dict(env, **(extra or {})), fam or kfam)


OPEN_NORM_CASES = [
    # (id, N, (n, k, l), env, kernel family that loads z and decides its norm)
    key_case("unit_io-512"),
    key_case("unit-1024"),
    key_case("unit-2048-pair"),
    # one wavefront per polynomial at N = 2048: the verifier's rows run on row_kernel, whose loads bound the norm by
    # |v|_1 |v|_inf and sum the float squares of the registers for the predicate (LL_L1INF)
    key_case("unit-2048-nopair", fam="row_kernel", name="row-2048-nopair"),
    key_case("group-1024"),
    key_case("block-1024"),
    key_case("block-2048"),
    # the shared-operand path takes no rotation terms: the challenge product by transforms
    key_case("slots-1024", extra=SHIFT0),
    key_case("unit-1024", fam="row_kernel", extra=SHIFT0, name="row-1024-shift0"),
]


def open_entries(ctx, A, polys, places, rng):
    """z (one crafted row among honest Gaussian rows), t = a1.z, c = 0, d: the relation holds, so the verdict is the
    crafted row's norm predicate."""
    P = P_of(ctx)
    n, k, l, N = ctx.n, ctx.k, ctx.l, ctx.N
    z0 = synth.gauss(rng, (k, N), P.sigma)
    assert O.check_norm(z0, P.verify_bound)
    a1z = Swap(A[:n], z0)
    B = len(places)
    z = np.broadcast_to(z0, (B, k, N)).copy()
    t = np.empty((B, n, N), dtype=np.int64)
    for e, (i, j) in enumerate(places):
        z[e, j] = polys[i][1]
        t[e] = a1z(j, polys[i][1])
    c = np.zeros((B, n + l, N), dtype=np.int64)
    d = synth.challenge(rng, (B,), N, ctx.kappa)
    want = [polys[i][2] for i, _ in places]
    return z, t, c, d, want


@pytest.mark.parametrize("cid,N,shape,env,fam", OPEN_NORM_CASES, ids=[c[0] for c in OPEN_NORM_CASES])
def test_open_verify_norm_edges(torch_mod, cid, N, shape, env, fam):
    t0 = time.time()
    n, k, l = shape
    ctx = make_ctx(N, n, k, l, env=env)
    P = P_of(ctx)
    assert ctx.verify_bound == P.verify_bound
    rng = np.random.default_rng(42000 + N + 10 * n + len(env))
    A = synth.key(rng, N, n, k, l)
    ctx.load_key(A)
    check_open_verify(ctx, A, fam, rng, cid, t0)


def check_open_verify(ctx, A, fam, rng, cid, t0):
    P = P_of(ctx)
    N, k = ctx.N, ctx.k
    polys = edge_polys(N, P.verify_bound)
    places = placements(polys, k, thin=k > 5)
    z, t, c, d, want = open_entries(ctx, A, polys, places, rng)
    for e in sample(len(places)):
        assert int(O.open_verify(P, A, z[e], t[e], c[e], d[e]) == 1) == want[e], polys[places[e][0]][0]
    sites = set()
    for ch in chunks(len(places)):
        sl = slice(ch.start, ch.stop)
        acc, names = run_prof(ctx, lambda: ctx.open_verify(z[sl], t[sl], c[sl], d[sl]))
        bad = [(polys[places[e][0]][0], places[e][1], want[e]) for e in ch if int(acc[e - ch.start]) != want[e]]
        assert not bad, bad
        assert fam in names, names
        sites.update(names)
    print(f"[open-verify {cid}] {len(places)} entries, {time.time() - t0:.1f}s, kernels {sorted(sites)}")


# ---- Open commit: the predicate on r with the commit bound ----------------------------------------------------------------
COMMIT_NORM_CASES = [key_case(cid) for cid in ("unit_io-512", "unit-1024", "unit-2048-pair", "group-1024", "slots-1024")]


@pytest.mark.parametrize("cid,N,shape,env,fam", COMMIT_NORM_CASES, ids=[c[0] for c in COMMIT_NORM_CASES])
def test_open_commit_norm_edges(torch_mod, cid, N, shape, env, fam):
    """r with one crafted column: identity columns of [a1; a2] are checked additions, the others products."""
    t0 = time.time()
    n, k, l = shape
    ctx = make_ctx(N, n, k, l, env=env)
    P = P_of(ctx)
    assert ctx.commit_bound == P.commit_bound
    rng = np.random.default_rng(43000 + N + 10 * n)
    A = synth.key(rng, N, n, k, l)
    ctx.load_key(A)
    check_open_commit(ctx, A, fam, rng, cid, t0)


def check_open_commit(ctx, A, fam, rng, cid, t0):
    P = P_of(ctx)
    N, k, l = ctx.N, ctx.k, ctx.l
    polys = edge_polys(N, P.commit_bound)
    places = placements(polys, k)
    B = len(places)
    r = np.broadcast_to(synth.small(rng, (k, N)), (B, k, N)).copy()
    for e, (i, j) in enumerate(places):
        r[e, j] = polys[i][1]
    x = np.broadcast_to(synth.uniform(rng, (l, N)), (B, l, N)).copy()
    y = np.broadcast_to(synth.gauss(rng, (k, N), P.sigma), (B, k, N)).copy()
    want = [polys[i][2] for i, _ in places]
    picked = set(sample(B))
    sites = set()
    for ch in chunks(B):
        sl = slice(ch.start, ch.stop)
        (c, t, ok), names = run_prof(ctx, lambda: ctx.open_commit(x[sl], r[sl], y[sl]))
        bad = [(polys[places[e][0]][0], places[e][1], want[e]) for e in ch if int(ok[e - ch.start]) != want[e]]
        assert not bad, bad
        for e in ch:
            if e in picked:
                c_ref, t_ref, ok_ref = O.open_commit(P, A, x[e], r[e], y[e])
                assert int(ok_ref) == want[e]
                assert np.array_equal(c[e - ch.start], c_ref) and np.array_equal(t[e - ch.start], t_ref), e
        assert fam in names, names
        sites.update(names)
    print(f"[open-commit {cid}] {B} entries, {time.time() - t0:.1f}s, kernels {sorted(sites)}")


@pytest.mark.parametrize("N,fam", [(512, "unit_io_kernel"), (1024, "unit_kernel"), (2048, "unit_kernel")])
def test_checked_additions_in_later_slots(torch_mod, N, fam):
    """A key whose first row is [1 | 1 | general]: row 0 adds r_0 and r_1 (z_0 and z_1), so the checked addition of column 1
    sits in the second slot of the row's per-addition sums while the first slot holds an honest column's."""
    t0 = time.time()
    n, k, l = 1, 3, 1
    ctx = make_ctx(N, n, k, l)
    rng = np.random.default_rng(43500 + N)
    A = synth.key(rng, N, n, k, l)
    A[0, 1] = 0
    A[0, 1, 0] = 1
    ctx.load_key(A)
    check_open_commit(ctx, A, fam, rng, f"two-ones-{N}", t0)
    check_open_verify(ctx, A, fam, rng, f"two-ones-{N}", t0)


# ---- Commitment::verify, both f branches ----------------------------------------------------------------------------------
@pytest.mark.parametrize("N,fam", [(512, "unit_io_kernel"), (1024, "unit_kernel")])
def test_commitment_verify_norm_edges(torch_mod, N, fam):
    """c = a.r + [0; x] (f = None) and c = f^-1 (a.r) + [0; x] for the unit f = +-X^s, f^-1 = -+X^(N - s): the opening
    holds, so the verdict is the commit constraint on r."""
    t0 = time.time()
    n, k, l = 1, 3, 1
    ctx = make_ctx(N, n, k, l)
    P = P_of(ctx)
    rng = np.random.default_rng(44000 + N)
    A = synth.key(rng, N, n, k, l)
    ctx.load_key(A)
    polys = edge_polys(N, P.commit_bound)
    places = placements(polys, k)
    B = len(places)
    r0 = synth.small(rng, (k, N))
    ar = Swap(A, r0)
    x0 = synth.uniform(rng, (l, N))
    zx = np.concatenate([np.zeros((n, N), dtype=np.int64), x0])
    r = np.broadcast_to(r0, (B, k, N)).copy()
    x = np.broadcast_to(x0, (B, l, N)).copy()
    f = np.zeros((B, N), dtype=np.int64)
    c = np.empty((B, n + l, N), dtype=np.int64)
    cf = np.empty((B, n + l, N), dtype=np.int64)
    for e, (i, j) in enumerate(places):
        r[e, j] = polys[i][1]
        prod = ar(j, polys[i][1])
        c[e] = madd(prod, zx)
        s, sg = 1 + (7 * e) % (N - 1), 1 if e % 2 else -1
        f[e, s] = sg
        finv = np.zeros(N, dtype=np.int64)
        finv[N - s] = -sg
        cf[e] = madd(cmul(prod, finv), zx)
    want = [polys[i][2] for i, _ in places]
    for e in sample(B):
        assert int(O.commitment_verify(P, A, c[e], x[e], r[e])) == want[e]
        assert int(O.commitment_verify(P, A, cf[e], x[e], r[e], f[e])) == want[e]
    sites = set()
    for ch in chunks(B):
        sl = slice(ch.start, ch.stop)
        # f = None: key products plus additions on the unit kernels; with f the products c (.) f and [0; x] (.) f are
        # vector x vector terms, which the planner sends to row_kernel
        for label, cm, ff, want_fam in (("plain", c, None, fam), ("f", cf, f[sl], "row_kernel")):
            ok, names = run_prof(ctx, lambda: ctx.commitment_verify(cm[sl], x[sl], r[sl], ff))
            bad = [(label, polys[places[e][0]][0], places[e][1], want[e]) for e in ch if int(ok[e - ch.start]) != want[e]]
            assert not bad, bad
            assert want_fam in names, (label, names)
            sites.update(names)
    print(f"[commitment-verify {N}] {B} entries x 2, {time.time() - t0:.1f}s, kernels {sorted(sites)}")


# ---- Linear ---------------------------------------------------------------------------------------------------------------
def pair_plan(polys, k):
    """Entries (polynomial index or None, row) for the first vector and for the second: every polynomial in every row of
    the first vector alone, then of the second alone; every polynomial in the first vector together with another one in
    the second (rows offset from each other, both cycling); and one entry with neither."""
    m = len(polys)
    out = [((None, 0), (None, 0))]
    for i in range(m):
        for j in range(k):
            out += [((i, j), (None, 0)), ((None, 0), (i, j))]
        out.append(((i, (i // 7) % k), ((i + 7) % m, (i // 7 + 1 + i % 2) % k)))
    return out


def check_pair_coverage(plan, polys, k):
    """Every (vector, row) carries an over-edge and an under-edge polynomial at least once, alone and together with a
    crafted polynomial in the other vector."""
    for vec in (0, 1):
        for both in (False, True):
            seen = {(ent[vec][1], polys[ent[vec][0]][2]) for ent in plan
                    if ent[vec][0] is not None and (ent[1 - vec][0] is not None) == both}
            assert seen == {(j, w) for j in range(k) for w in (0, 1)}, (vec, both)


def pair_label(polys, ent):
    return tuple((polys[i][0], j) if i is not None else None for i, j in ent)


@pytest.mark.parametrize("N", [512, 1024])
@pytest.mark.parametrize("env,fam", [({}, "unit"), ({"RZK_LIN_E": 0}, "row_kernel")], ids=["default", "lin_e0"])
def test_linear_verify_norm_edges(torch_mod, N, env, fam):
    """The whole plan in every row of z alone, of z' alone, in both, in neither; c = c' = 0, t = a1.z, t' = a1.z',
    u = g (.) (a2.z) - a2.z'.  The entry point returns one bit: accept iff both norms pass."""
    t0 = time.time()
    n, k, l = 1, 3, 1
    if fam == "unit":
        fam = "unit_io_kernel" if N == 512 else "unit_kernel"
    ctx = make_ctx(N, n, k, l, env=env)
    P = P_of(ctx)
    rng = np.random.default_rng(45000 + N + len(env))
    A = synth.key(rng, N, n, k, l)
    ctx.load_key(A)
    polys = edge_polys(N, P.verify_bound)
    plan = pair_plan(polys, k)
    check_pair_coverage(plan, polys, k)
    B = len(plan)
    z0, zp0 = synth.gauss(rng, (k, N), P.sigma), synth.gauss(rng, (k, N), P.sigma)
    a1z, a2z, a1zp, a2zp = Swap(A[:n], z0), Swap(A[n:], z0), Swap(A[:n], zp0), Swap(A[n:], zp0)
    g0 = synth.uniform(rng, (N,))
    a2zg = cmul(a2z.base, g0)
    z, zp = np.broadcast_to(z0, (B, k, N)).copy(), np.broadcast_to(zp0, (B, k, N)).copy()
    t, tp = np.broadcast_to(a1z.base, (B, n, N)).copy(), np.broadcast_to(a1zp.base, (B, n, N)).copy()
    u = np.empty((B, l, N), dtype=np.int64)
    g = np.broadcast_to(g0, (B, N)).copy()
    want = []
    for e, ((i, j), (ip, jp)) in enumerate(plan):
        left, right = a2zg, a2zp.base
        if i is not None:
            z[e, j], t[e] = polys[i][1], a1z(j, polys[i][1])
            left = cmul(a2z(j, polys[i][1]), g0)
        if ip is not None:
            zp[e, jp], tp[e] = polys[ip][1], a1zp(jp, polys[ip][1])
            right = a2zp(jp, polys[ip][1])
        u[e] = msub(left, right)
        want.append((polys[i][2] if i is not None else 1) & (polys[ip][2] if ip is not None else 1))
    c = np.zeros((B, n + l, N), dtype=np.int64)
    d = synth.challenge(rng, (B,), N, ctx.kappa)
    for e in sample(B):
        assert int(O.linear_verify(P, A, z[e], zp[e], c[e], c[e], g[e], t[e], tp[e], u[e], d[e]) == 1) == want[e], plan[e]
    sites = set()
    for ch in chunks(B):
        sl = slice(ch.start, ch.stop)
        acc, names = run_prof(ctx, lambda: ctx.linear_verify(z[sl], zp[sl], c[sl], c[sl], g[sl], t[sl], tp[sl], u[sl],
                                                             d[sl]))
        bad = [(pair_label(polys, plan[e]), want[e]) for e in ch if int(acc[e - ch.start]) != want[e]]
        assert not bad, bad
        assert fam in names, names
        sites.update(names)
    print(f"[linear-verify {N} {env}] {B} entries, {time.time() - t0:.1f}s, kernels {sorted(sites)}")


@pytest.mark.parametrize("N,fam", [(512, "unit_io_kernel"), (1024, "unit_kernel")])
def test_linear_commit_verdict_bits(torch_mod, N, fam):
    """linear_commit exposes both verdict bits: bit 0 the constraint on r, bit 1 on r'.  The whole plan in every column of
    r alone, of r' alone, in both, in neither (identity columns are checked additions marked ADD_CHECK / ADD_CHECK2, the
    last column a product): the byte equals the oracle's, so an r' that fails alone is never reported as r failing."""
    t0 = time.time()
    n, k, l = 1, 3, 1
    ctx = make_ctx(N, n, k, l)
    P = P_of(ctx)
    rng = np.random.default_rng(46000 + N)
    A = synth.key(rng, N, n, k, l)
    ctx.load_key(A)
    polys = edge_polys(N, P.commit_bound)
    plan = pair_plan(polys, k)
    check_pair_coverage(plan, polys, k)
    B = len(plan)
    r, rp = synth.small(rng, (B, k, N)), synth.small(rng, (B, k, N))
    want = []
    for e, ((i, j), (ip, jp)) in enumerate(plan):
        if i is not None:
            r[e, j] = polys[i][1]
        if ip is not None:
            rp[e, jp] = polys[ip][1]
        want.append((polys[i][2] if i is not None else 1) | (polys[ip][2] if ip is not None else 1) << 1)
    assert set(want) == {0, 1, 2, 3}
    g, x = synth.uniform(rng, (B, N)), synth.uniform(rng, (B, l, N))
    y, yp = synth.gauss(rng, (B, k, N), P.sigma), synth.gauss(rng, (B, k, N), P.sigma)
    picked = set(sample(B))
    sites = set()
    for ch in chunks(B):
        sl = slice(ch.start, ch.stop)
        outs, names = run_prof(ctx, lambda: ctx.linear_commit(g[sl], x[sl], r[sl], rp[sl], y[sl], yp[sl]))
        ok = outs[5]
        bad = [(pair_label(polys, plan[e]), want[e], int(ok[e - ch.start])) for e in ch if int(ok[e - ch.start]) != want[e]]
        assert not bad, bad
        for e in ch:
            if e in picked:
                ref = O.linear_commit(P, A, g[e], x[e], r[e], rp[e], y[e], yp[e])
                assert int(ref[5]) == want[e]
                for got, ref_a in zip(outs[:5], ref[:5]):
                    assert np.array_equal(got[e - ch.start], ref_a), e
        assert fam in names, names
        sites.update(names)
    print(f"[linear-commit {N}] {B} entries, {time.time() - t0:.1f}s, kernels {sorted(sites)}")


# ---- Sum ------------------------------------------------------------------------------------------------------------------
def test_sum_verify_norm_edges(torch_mod):
    """(2,5,2), V = 2: the whole plan in z_0, then z_1, then z' (one vector at a time; the carrying row cycles with the
    polynomial and the vector, the L - 1 / L pairs go to every row), commitments zero, t_i = a1.z_i, t' = a1.z',
    u = sum_i g_i (.) (a2.z_i) - a2.z'."""
    t0 = time.time()
    N, n, k, l, V = 1024, 2, 5, 2, 2
    ctx = make_ctx(N, n, k, l)
    P = P_of(ctx)
    rng = np.random.default_rng(47000)
    A = synth.key(rng, N, n, k, l)
    ctx.load_key(A)
    polys = edge_polys(N, P.verify_bound)
    v0 = synth.gauss(rng, (V + 1, k, N), P.sigma)          # z_0 .. z_{V-1}, z'
    a1v = [Swap(A[:n], v0[s]) for s in range(V + 1)]
    a2v = [Swap(A[n:], v0[s]) for s in range(V + 1)]
    g0 = synth.uniform(rng, (V, N))
    a2g = [cmul(a2v[s].base, g0[s]) for s in range(V)]
    places = []                                            # (polynomial, vector, row)
    for i, (lab, _, _) in enumerate(polys):
        for s in range(V + 1):
            rows = range(k) if lab.startswith(("below", "at")) else [(i + s) % k]
            places += [(i, s, j) for j in rows]
    for s in range(V + 1):                                 # every (vector, row) meets both verdicts
        assert {(j, polys[i][2]) for i, s_, j in places if s_ == s} == {(j, w) for j in range(k) for w in (0, 1)}
    B = len(places)
    zs, zp = np.broadcast_to(v0[:V], (B, V, k, N)).copy(), np.broadcast_to(v0[V], (B, k, N)).copy()
    ts = np.broadcast_to(np.stack([a1v[s].base for s in range(V)]), (B, V, n, N)).copy()
    tp = np.broadcast_to(a1v[V].base, (B, n, N)).copy()
    u = np.empty((B, l, N), dtype=np.int64)
    for e, (i, s, j) in enumerate(places):
        p = polys[i][1]
        terms, right = list(a2g), a2v[V].base
        if s < V:
            zs[e, s, j], ts[e, s] = p, a1v[s](j, p)
            terms[s] = cmul(a2v[s](j, p), g0[s])
        else:
            zp[e, j], tp[e] = p, a1v[V](j, p)
            right = a2v[V](j, p)
        acc_u = terms[0]
        for term in terms[1:]:
            acc_u = madd(acc_u, term)
        u[e] = msub(acc_u, right)
    gs = np.broadcast_to(g0, (B, V, N)).copy()
    cs, cp = np.zeros((B, V, n + l, N), dtype=np.int64), np.zeros((B, n + l, N), dtype=np.int64)
    d = synth.challenge(rng, (B,), N, ctx.kappa)
    want = [polys[i][2] for i, _, _ in places]
    for e in sample(B):
        assert int(O.sum_verify(P, A, zs[e], zp[e], cs[e], cp[e], gs[e], ts[e], tp[e], u[e], d[e]) == 1) == want[e]
    sites = set()
    for ch in chunks(B):
        sl = slice(ch.start, ch.stop)
        acc, names = run_prof(ctx, lambda: ctx.sum_verify(zs[sl], zp[sl], cs[sl], cp[sl], gs[sl], ts[sl], tp[sl], u[sl],
                                                          d[sl]))
        bad = [(polys[places[e][0]][0], places[e][1:], want[e]) for e in ch if int(acc[e - ch.start]) != want[e]]
        assert not bad, bad
        assert "row_group_kernel" in names, names
        sites.update(names)
    print(f"[sum-verify] {B} entries, {time.time() - t0:.1f}s, kernels {sorted(sites)}")


# ---- three trips of one team: the exact path re-reads src on a later trip --------------------------------------------------
@pytest.mark.parametrize("N,stride,fam", [(1024, 32, "unit_kernel"), (2048, 8, "unit_kernel"), (512, 32, "unit_io_kernel")])
def test_norm_edges_on_later_trips(torch_mod, N, stride, fam):
    """RZK_GRID_CUS=1, a batch of 2 strides + 8 (three trips, one task per entry): the L entries (reject) at offset 5 of
    trips 0, 1, 2 and the L - 1 entries (accept) at offset 7, honest entries on either side of each."""
    n, k, l = 1, 3, 1
    ctx = make_ctx(N, n, k, l, env={"RZK_GRID_CUS": 1})
    P = P_of(ctx)
    rng = np.random.default_rng(48000 + N)
    A = synth.key(rng, N, n, k, l)
    ctx.load_key(A)
    B = 2 * stride + 8
    by = {lab: (lab, p, w) for lab, p, w in edge_polys(N, P.verify_bound)}
    for style in ("point@0", "spread@0"):
        polys = [by[f"at/{style}"], by[f"below/{style}"]]
        z0 = synth.gauss(rng, (k, N), P.sigma)
        a1z = Swap(A[:n], z0)
        z = np.broadcast_to(z0, (B, k, N)).copy()
        t = np.broadcast_to(a1z.base, (B, n, N)).copy()
        want = [1] * B
        for trip in range(3):
            for off, (lab, p, w) in ((5, polys[0]), (7, polys[1])):
                e, j = trip * stride + off, trip % k
                z[e, j], t[e], want[e] = p, a1z(j, p), w
        assert sum(want) == B - 3
        c = np.zeros((B, n + l, N), dtype=np.int64)
        d = synth.challenge(rng, (B,), N, ctx.kappa)
        for e in (4, 5, 7, stride + 5, 2 * stride + 5, 2 * stride + 7):
            assert int(O.open_verify(P, A, z[e], t[e], c[e], d[e]) == 1) == want[e]
        acc, names = run_prof(ctx, lambda: ctx.open_verify(z, t, c, d))
        assert acc.tolist() == want, style
        assert fam in names, names


# ---- position sweeps ------------------------------------------------------------------------------------------------------
def center_np(v):
    v = np.mod(v, Q)
    return np.where(v > HALF, v - Q, v)


def fault_values(old, kind):
    """q: the same residue outside the centred range (only the range test can reject); 2^32: the same low word;
    2^31: +-2^31 in place of the coefficient; pm1: the neighbouring residue (the zero test must see it)."""
    if kind == "q":
        return np.where(old > 0, old - Q, old + Q)
    if kind == "2^32":
        return old + (1 << 32)
    if kind == "2^31":
        return np.where(np.arange(len(old)) % 2 == 0, 1 << 31, -(1 << 31))
    assert kind == "pm1"
    return center_np(old + np.where(np.arange(len(old)) % 2 == 0, 1, -1))


def sweep(torch, call, arrays, name, rows, kinds, N, trusted_too=None, total=None):
    """Runs call(**arrays) with arrays[name] faulted as synth.sweep_faults says (over the first `rows` of its `total`
    rows), two passes per kind: the clean entries move and the rows step by one, so that together the passes fault every
    coefficient position.  Exact verdict vectors."""
    arr = arrays[name]
    lead = arr.reshape(N, total or rows, N)
    for pass_ in (0, 1):
        ent, rr, cc = synth.sweep_faults(N, rows, pass_)
        expect = np.ones(N, dtype=np.uint8)
        expect[ent] = 0
        E, R, Cc = (torch.from_numpy(a).cuda() for a in (ent, rr, cc))
        old = lead[E, R, Cc].clone()
        for kind in kinds:
            lead[E, R, Cc] = torch.from_numpy(fault_values(old.cpu().numpy(), kind)).cuda()
            acc = call(**arrays).cpu().numpy()
            lead[E, R, Cc] = old
            if trusted_too is not None and kind == "q":      # the range test is off: only the clean entries are pinned
                assert acc[expect == 1].tolist() == [1] * int(expect.sum()), (name, kind)
                continue
            wrong = np.flatnonzero(acc != expect)
            assert wrong.size == 0, (name, kind, pass_, [(int(i), int(acc[i])) for i in wrong[:12]], int(wrong.size))


def oracle_open_proof(P, A, rng):
    N, k, l = P.N, P.k, P.l
    x, r, y = synth.uniform(rng, (l, N)), synth.small(rng, (k, N)), synth.gauss(rng, (k, N), P.sigma)
    d = synth.challenge(rng, (1,), N, P.kappa)[0]
    c, t, ok = O.open_commit(P, A, x, r, y)
    z = O.open_response(P, y, r, d)
    assert ok and O.open_verify(P, A, z, t, c, d) == 1
    return dict(z=z, t=t, c=c, d=d)


def replicate(torch, proof, B):
    return {key: torch.from_numpy(np.broadcast_to(a, (B,) + a.shape).copy()).cuda() for key, a in proof.items()}


# the norm cases' configurations plus row_kernel in two-wavefront teams
OPEN_SWEEP_CASES = OPEN_NORM_CASES + [key_case("unit-2048-pair", fam="row_kernel", extra=SHIFT0, name="row-2048-shift0")]


@pytest.mark.parametrize("trusted", [False, True], ids=["checked", "trusted"])
@pytest.mark.parametrize("cid,N,shape,env,fam", OPEN_SWEEP_CASES, ids=[c[0] for c in OPEN_SWEEP_CASES])
def test_open_verify_position_sweeps(torch_mod, cid, N, shape, env, fam, trusted):
    """Open's z, t, c: range test (c -+ q, c + 2^32; +-2^31 in t and c, which carry no norm mark) and zero test
    (z +- 1, t +- 1) at every coefficient position.  Trusted-producer mode: clean entries accept, +-1 entries reject."""
    t0 = time.time()
    n, k, l = shape
    ctx = make_ctx(N, n, k, l, env=env)
    P = P_of(ctx)
    rng = np.random.default_rng(49000 + N + n + len(env))
    A = synth.key(rng, N, n, k, l)
    ctx.load_key(A)
    proof = oracle_open_proof(P, A, rng)
    arrays = replicate(torch_mod, proof, N)
    if trusted:
        ctx.trust_device_outputs(True)
    call = lambda z, t, c, d: ctx.open_verify(z, t, c, d)
    acc, names = run_prof(ctx, lambda: call(**arrays))
    assert acc.cpu().numpy().tolist() == [1] * N
    assert fam in names, names
    tr = True if trusted else None
    kinds = ("q", "pm1") if trusted else ("q", "2^32", "pm1")
    sweep(torch_mod, call, arrays, "z", k, kinds, N, tr)
    sweep(torch_mod, call, arrays, "t", n, kinds if trusted else ("q", "2^32", "2^31", "pm1"), N, tr)
    if not trusted:
        # Open's relation a1.z = t + c1 (.) d reads the first n rows of c only (open.rs:167-173, as the oracle): the rest is
        # no input of this verifier, so there is no load that could test it
        sweep(torch_mod, call, arrays, "c", n, ("q", "2^32", "2^31"), N, total=n + l)
    # the oracle agrees on a +-1 entry of each operand (its relation is what the zero test decides)
    for name, pos in (("z", (k - 1, N - 1)), ("t", (0, N // 2 + 64))):
        m = {key: a.copy() for key, a in proof.items()}
        m[name][pos] = O.center(int(m[name][pos]) + 1)
        assert O.open_verify(P, A, m["z"], m["t"], m["c"], m["d"]) != 1
    ctx.synchronize()
    print(f"[open-sweep {cid} trusted={trusted}] {time.time() - t0:.1f}s, kernels {sorted(set(names))}")


@pytest.mark.parametrize("N,env,fam", [(512, {}, "unit_io_kernel"), (1024, {}, "unit_kernel"),
                                       (1024, {"RZK_LIN_E": 0}, "row_kernel"), (2048, {}, "unit_kernel")],
                         ids=["512", "1024", "1024-lin_e0", "2048-pair"])
def test_linear_verify_position_sweeps(torch_mod, N, env, fam):
    """Linear's z', u, g at every coefficient position."""
    t0 = time.time()
    n, k, l = 1, 3, 1
    ctx = make_ctx(N, n, k, l, env=env)
    P = P_of(ctx)
    rng = np.random.default_rng(50000 + N + len(env))
    A = synth.key(rng, N, n, k, l)
    ctx.load_key(A)
    g, x = synth.uniform(rng, (N,)), synth.uniform(rng, (l, N))
    r, rp = synth.small(rng, (k, N)), synth.small(rng, (k, N))
    y, yp = synth.gauss(rng, (k, N), P.sigma), synth.gauss(rng, (k, N), P.sigma)
    d = synth.challenge(rng, (1,), N, P.kappa)[0]
    c, cp, t, tp, u, ok = O.linear_commit(P, A, g, x, r, rp, y, yp)
    z, zp = O.linear_response(P, y, yp, r, rp, d)
    assert ok == 3 and O.linear_verify(P, A, z, zp, c, cp, g, t, tp, u, d) == 1
    arrays = replicate(torch_mod, dict(z=z, zp=zp, c=c, cp=cp, g=g, t=t, tp=tp, u=u, d=d), N)
    call = lambda **a: ctx.linear_verify(*(a[key] for key in ("z", "zp", "c", "cp", "g", "t", "tp", "u", "d")))
    acc, names = run_prof(ctx, lambda: call(**arrays))
    assert acc.cpu().numpy().tolist() == [1] * N
    assert fam in names, names
    sweep(torch_mod, call, arrays, "zp", k, ("q", "2^32", "pm1"), N)
    sweep(torch_mod, call, arrays, "u", l, ("q", "2^32", "2^31", "pm1"), N)
    sweep(torch_mod, call, arrays, "g", 1, ("q", "2^32", "2^31", "pm1"), N)
    print(f"[linear-sweep {N} {env}] {time.time() - t0:.1f}s, kernels {sorted(set(names))}")


@pytest.mark.parametrize("N,shape,fam", [(512, (1, 3, 1), "unit_io_kernel"), (1024, (1, 3, 1), "unit_kernel"),
                                         (2048, (1, 3, 1), "unit_kernel"), (1024, (2, 5, 2), "row_group_kernel")],
                         ids=["512-131", "1024-131", "2048-131-pair", "1024-252"])
def test_sum_verify_position_sweeps(torch_mod, N, shape, fam):
    """Sum's zs (V k rows) and gs (V rows) at every coefficient position, V = 2; the products by g_i run on row_kernel."""
    t0 = time.time()
    n, k, l = shape
    V = 2
    ctx = make_ctx(N, n, k, l)
    P = P_of(ctx)
    rng = np.random.default_rng(51000 + N + n)
    A = synth.key(rng, N, n, k, l)
    ctx.load_key(A)
    gs, xs = synth.uniform(rng, (V, N)), synth.uniform(rng, (V, l, N))
    rs, rp = synth.small(rng, (V, k, N)), synth.small(rng, (k, N))
    ys, yp = synth.gauss(rng, (V, k, N), P.sigma), synth.gauss(rng, (k, N), P.sigma)
    d = synth.challenge(rng, (1,), N, P.kappa)[0]
    cs, cp, ts, tp, u, ok = O.sum_commit(P, A, gs, xs, rs, rp, ys, yp)
    zs, zp = O.sum_response(P, ys, yp, rs, rp, d)
    assert ok and O.sum_verify(P, A, zs, zp, cs, cp, gs, ts, tp, u, d) == 1
    arrays = replicate(torch_mod, dict(zs=zs, zp=zp, cs=cs, cp=cp, gs=gs, ts=ts, tp=tp, u=u, d=d), N)
    call = lambda **a: ctx.sum_verify(*(a[key] for key in ("zs", "zp", "cs", "cp", "gs", "ts", "tp", "u", "d")))
    acc, names = run_prof(ctx, lambda: call(**arrays))
    assert acc.cpu().numpy().tolist() == [1] * N
    assert fam in names and "row_kernel" in names, names
    sweep(torch_mod, call, arrays, "zs", V * k, ("q", "2^32", "pm1"), N)
    sweep(torch_mod, call, arrays, "gs", V, ("q", "2^32", "2^31", "pm1"), N)
    print(f"[sum-sweep {N} {shape}] {time.time() - t0:.1f}s, kernels {sorted(set(names))}")


# ---- the prover side: a non-canonical input fails the call --------------------------------------------------------------
@pytest.mark.parametrize("N,fam", [(512, "unit_io_kernel"), (1024, "unit_kernel"), (2048, "unit_kernel")])
def test_prover_inputs_fail_the_call_at_spread_positions(torch_mod, N, fam):
    """x, r or y of open_commit with c -+ q at 16 positions spread over lanes, registers and rows: RZK_E_ARG, the faulted
    entries' flags cleared, and the clean entries' outputs bit-equal to a clean call's."""
    n, k, l = 1, 3, 1
    ctx = make_ctx(N, n, k, l)
    P = P_of(ctx)
    rng = np.random.default_rng(52000 + N)
    A = synth.key(rng, N, n, k, l)
    ctx.load_key(A)
    B, F = 24, 16
    x, r, y = synth.uniform(rng, (B, l, N)), synth.small(rng, (B, k, N)), synth.gauss(rng, (B, k, N), P.sigma)
    (c0, t0, ok0), names = run_prof(ctx, lambda: ctx.open_commit(x, r, y))
    assert ok0.tolist() == [1] * B and fam in names, names
    for e in (0, B - 1):
        c_ref, t_ref, _ = O.open_commit(P, A, x[e], r[e], y[e])
        assert np.array_equal(c0[e], c_ref) and np.array_equal(t0[e], t_ref)
    for name, rows in (("x", l), ("r", k), ("y", k)):
        fp = synth.fault_positions(N, rows)
        arrs = dict(x=x.copy(), r=r.copy(), y=y.copy())
        for e in range(F):
            row, coef = fp[(e * N) // F + (5 * e) % 64]       # every register block, lanes 0, 5, 10, ..
            v = int(arrs[name][e, row, coef])
            arrs[name][e, row, coef] = v - Q if v > 0 else v + Q
        with pytest.raises(RzkError) as err:
            ctx.open_commit(arrs["x"], arrs["r"], arrs["y"])
        assert err.value.status == -1                          # RZK_E_ARG
        c1, t1, ok1 = ctx.open_commit(*(dev(torch_mod, arrs[key]) for key in ("x", "r", "y")))
        with pytest.raises(RzkError) as err:
            ctx.synchronize()
        assert err.value.status == -1
        assert ok1.cpu().numpy().tolist() == [0] * F + [1] * (B - F), name
        assert np.array_equal(c1.cpu().numpy()[F:], c0[F:]) and np.array_equal(t1.cpu().numpy()[F:], t0[F:]), name
    # the context keeps working
    c2, t2, ok2 = ctx.open_commit(x, r, y)
    assert np.array_equal(c2, c0) and np.array_equal(t2, t0) and ok2.tolist() == [1] * B
