"""Prime-count edges on the GPU: Cauchy-Schwarz-tight operands at every kernel that picks 1, 2 or 3 auxiliary primes.

Every NTT-path product is reconstructed from as many auxiliary primes as the kernel's bound sum_terms |a|_2 |b|_2
asks for (primes_for in rzk_rowprog.h).  A bound that drops a term, a row or a factor makes the CRT reconstruct a
value modulo the wrong product of primes: a wrong answer mod q, or a flipped verdict, with no error.  Random
protocol data sits bits away from a capacity, so these cases build exact results just below and just above
(P_np - 1) / 2 on purpose (ring_zk_amd/synth.py, tight_terms / conj; tests/test_crt_edges.py checks the identities
and that too few primes give a wrong value).  Everything is compared bit for bit with oracle/rzk_oracle.c, an
__int128 schoolbook that uses no CRT.

  * key products (matvec A1 / A2 / A with an addend) with a key whose tight row is first or last of its block, every
    other row tiny: unit_io_kernel (N = 512), unit_kernel (N = 1024, paired rows; N = 2048 with RZK_PAIR_POLY on and
    off), row_group_kernel, row_block_kernel, fwd_slots_kernel + row_slots_kernel;
  * polymul and cmul: vector x vector terms with unequal factor norms (a = 16 w, b = conj(w)) on row_kernel, under
    RZK_SHIFT=0, and on row_slots_kernel's vector-term branch (RZK_SLOT_SHARE_MIN=1);
  * a dense aligned-sign full-range matvec at (8,17,8), N = 2048: rows of +-17 N ((q-1)/2)^2, about 2^76.5;
  * Open, Commitment::verify, Linear (RZK_LIN_E=0 and the default nested g (.) e with e a chosen e*) and Sum (output
    images and prepared multiplier images) at b = 2^22, every canonical norm passing, with t / c / u solved by the
    oracle, so a miscounted prime flips accept to reject; one tampered entry per call must reject;
  * batches at RZK_GRID_CUS=1 with tight and tiny entries on consecutive trips of one team.

Kernel names come from the profiler (prof_read_kernels), so a routing change cannot quietly empty a case.
"""
import time

import numpy as np
import pytest

from oracle import oracle as O
from ring_zk_amd import synth
from test_gpu_baseline_shapes import make_ctx, torch_mod  # noqa: F401
from test_gpu_multi_trip import kernel_family

pytestmark = pytest.mark.gpu

Q = O.Q_DEFAULT
HALF = (Q - 1) // 2
BIG_B = 1 << 22          # every canonical norm is below the verify bound (test_norm_bounds_beyond_32_bits)
LAM = 16                 # vector x vector terms: a = LAM w, b = conj(w), so |a|_2 != |b|_2
FAMILIES = [(np_, name) for np_ in (1, 2) for name in ("under", "below", "just", "near", "far")]


def run_prof(ctx, fn):
    ctx.prof_enable(True)
    ctx.prof_reset()
    out = fn()
    names = [kernel_family(nm) for nm, _ in ctx.prof_read_kernels()]
    ctx.prof_enable(False)
    return out, names


def tiny_entry(N, rng):
    """A general key entry of norm sqrt(2) (never the constant 1)."""
    return synth.spread(N, [1, 1], rng)


def edge_key(N, n, k, l, rng):
    """[a1; a2] with the usual identity entries and every general entry tiny (load_tight_row then sets one row)."""
    A = np.zeros((n + l, k, N), dtype=np.int64)
    for i in range(n + l):
        A[i, i, 0] = 1
        for c in general_cols(n, k, l, i):
            A[i, c] = tiny_entry(N, rng)
    return A


def general_cols(n, k, l, row):
    return list(range(n, k)) if row < n else list(range(n + l, k))


def load_tight_row(ctx, A, row, target, rng):
    """Makes `row` of A tight for `target` (sum of its general entries' squared norms == target) and loads A."""
    n, k, l, N = ctx.n, ctx.k, ctx.l, ctx.N
    cols = general_cols(n, k, l, row)
    Ks = synth.tight_terms(N, target, len(cols), rng)
    for c, K in zip(cols, Ks):
        A[row, c] = K
    ctx.load_key(A)
    return A


def tight_vector(A, row, n, k, l, sign, rng):
    """v with v_c = sign conj(A[row, c]) on the row's general columns, ternary elsewhere, and coefficient 0 of the
    row's identity column zero: (A[row] . v)_0 == sign * sum_c |A[row, c]|^2 exactly, the Cauchy-Schwarz bound of
    the kernels."""
    N = A.shape[-1]
    v = synth.small(rng, (k, N))
    v[row, 0] = 0
    for c in general_cols(n, k, l, row):
        v[c] = sign * synth.conj(A[row, c])
    return v


def dot_row_exact(A, row, v):
    """Exact integer value of coefficient 0 of A[row] . v over the general columns (Python integers)."""
    return sum(synth.negacyclic_coef0(A[row, c], v[c]) for c in range(A.shape[1]) if synth.sq_norm(A[row, c]) > 1)


# ---- key products ------------------------------------------------------------------------------------------------------
KEY_CASES = [
    # (id, N, (n, k, l), env, B, kernel family the key products must run on)
    ("unit_io-512", 512, (1, 3, 1), {}, 40, "unit_io_kernel"),
    ("unit-1024", 1024, (1, 3, 1), {}, 40, "unit_kernel"),
    ("unit-2048-pair", 2048, (1, 3, 1), {}, 20, "unit_kernel"),
    ("unit-2048-nopair", 2048, (1, 3, 1), {"RZK_PAIR_POLY": 0}, 40, "unit_kernel"),
    ("group-1024", 1024, (2, 5, 2), {}, 40, "row_group_kernel"),
    ("block-1024", 1024, (4, 9, 4), {"RZK_BLOCK_MIN_LOGN": 10}, 6, "row_block_kernel"),
    ("block-2048", 2048, (2, 5, 2), {}, 6, "row_block_kernel"),
    ("slots-1024", 1024, (2, 5, 2), {"RZK_ROW_GROUPS": 0, "RZK_BLOCK_MIN_LOGN": 12, "RZK_SLOT_SHARE_MIN": 1}, 20,
     "fwd_slots_kernel + row_slots_kernel"),
]


def batch_plan(B):
    """Per entry: None (tiny) or a sign (tight).  Tight entries every third slot, so at 32 teams per CU one team meets
    tight and tiny entries on consecutive trips; signs alternate."""
    return [None if b % 3 != 1 else (1 if (b // 3) % 2 == 0 else -1) for b in range(B)]


# (np, family) per loaded key, alternating between the rows of a configuration
LOADS = [[(1, "near"), (2, "just"), (1, "under"), (2, "far")],
         [(2, "near"), (1, "just"), (2, "under"), (1, "far")]]


def check_key_products(ctx, A, row, plan, rng, fam, sites):
    """matvec A1, A2, A (with an addend) over a batch that follows `plan`; every entry vs the oracle."""
    n, k, l, N = ctx.n, ctx.k, ctx.l, ctx.N
    B = len(plan)
    v = synth.small(rng, (B, k, N))
    rowsum = sum(synth.sq_norm(A[row, c]) for c in general_cols(n, k, l, row))
    for b, sign in enumerate(plan):
        if sign is not None:
            v[b] = tight_vector(A, row, n, k, l, sign, rng)
            assert dot_row_exact(A, row, v[b]) == sign * rowsum
    want = [O.mat_dot(A, v[b][:, None, :])[:, 0, :] for b in range(B)]
    for which, sl in ((0, slice(0, n)), (1, slice(n, n + l)), (2, slice(0, n + l))):
        add = synth.uniform(rng, (B, ctx._rows(which), N))
        out, names = run_prof(ctx, lambda: ctx.matvec(which, v, add))
        assert fam in names, (which, names)
        sites.update(names)
        for b in range(B):
            assert np.array_equal(out[b], O.mat_add(want[b][sl, None, :], add[b][:, None, :])[:, 0, :]), \
                (which, b, plan[b])


@pytest.mark.parametrize("cid,N,shape,env,B,fam", KEY_CASES, ids=[c[0] for c in KEY_CASES])
def test_key_products_at_prime_edges(torch_mod, cid, N, shape, env, B, fam):
    """One tight row per loaded key (the first row, the last a1 row, the last row), the other rows tiny; each load
    puts the tight row on one side of one capacity, the batch mixes tight entries of both signs with tiny ones."""
    t0 = time.time()
    n, k, l = shape
    ctx = make_ctx(N, n, k, l, env=dict(env, RZK_GRID_CUS=1), b=BIG_B)
    rng = np.random.default_rng(31000 + N + 100 * n)
    rows = sorted({0, n - 1, n + l - 1})
    big = N * k * (n + l) > 1024 * 3 * 2 * 2    # the oracle's schoolbook dominates: two loads per row
    sites = set()
    for ri, row in enumerate(rows):
        for np_, name in LOADS[ri % 2][:2 if big else 4]:
            A = edge_key(N, n, k, l, rng)
            load_tight_row(ctx, A, row, synth.edge_targets(np_)[name], rng)
            check_key_products(ctx, A, row, batch_plan(B), rng, fam, sites)
    print(f"[{cid}] {time.time() - t0:.1f}s, kernels {sorted(sites)}")


# ---- vector x vector products ------------------------------------------------------------------------------------------
def vec_pair(N, X, rng, lam_on_a):
    """(a, b) with (a*b)_0 = |a|_2 |b|_2 just at or above X: a = LAM w, b = conj(w) (or w, LAM conj(w)), w four equal
    magnitudes, so |v|_1 |v|_inf = |v|_2^2 for both factors."""
    c = synth.isqrt(-(-X // (4 * LAM)))
    while 4 * LAM * c * c < X:
        c += 1
    w = synth.spread(N, [c] * 4, rng)
    a, b = (LAM * w, synth.conj(w)) if lam_on_a else (w, LAM * synth.conj(w))
    assert max(int(np.abs(a).max()), int(np.abs(b).max())) <= HALF
    return a, b


VEC_CASES = [
    # (id, N, env, kernel family of polymul and of the three-row cmul)
    ("512", 512, {}, "row_kernel"),
    ("1024", 1024, {}, "row_kernel"),
    ("2048-pair", 2048, {}, "row_kernel"),
    ("2048-nopair", 2048, {"RZK_PAIR_POLY": 0}, "row_kernel"),
    ("1024-shift0", 1024, {"RZK_SHIFT": 0}, "row_kernel"),
    # every operand its own slot (polymul), the three cmul rows share p: the shared-operand path, vector x vector
    # terms of row_slots_kernel with both norms read from the slots
    ("1024-slots", 1024, {"RZK_SLOT_SHARE_MIN": 1}, "fwd_slots_kernel + row_slots_kernel"),
]


@pytest.mark.parametrize("cid,N,env,fam", VEC_CASES, ids=[c[0] for c in VEC_CASES])
def test_polymul_cmul_at_prime_edges(torch_mod, cid, N, env, fam):
    """Vector x vector products (both factors measured by the kernel) on every family of both capacities, both signs,
    the larger factor on either side; cmul with the tight row first or last among tiny rows."""
    t0 = time.time()
    ctx = make_ctx(N, 1, 3, 1, env=dict(env, RZK_GRID_CUS=1), b=BIG_B)
    rng = np.random.default_rng(32000 + N + len(env))
    plan = batch_plan(40)
    B = len(plan)
    a, b = synth.small(rng, (B, N)), synth.small(rng, (B, N))
    for i, sign in enumerate(plan):
        if sign is None:
            continue
        np_, name = FAMILIES[(i // 3) % len(FAMILIES)]
        X = synth.edge_targets(np_)[name]
        if name == "near" and sign > 0:     # exact target: lam = 1, greedy squares
            a[i], b[i] = synth.tight_pair(synth.spread(N, synth.squares_to(X, HALF), rng))
            assert synth.negacyclic_coef0(a[i], b[i]) == X
        else:
            a[i], b[i] = vec_pair(N, X, rng, lam_on_a=(i // 3) % 2 == 0)
            b[i] *= sign
            assert abs(synth.negacyclic_coef0(a[i], b[i])) >= X
    # an aligned-sign full-range product near the 3-prime maximum N (q-1)^2 / 4
    a[0] = HALF
    b[0] = -HALF * np.ones(N, dtype=np.int64)
    b[0, 0] = HALF
    prod, names = run_prof(ctx, lambda: ctx.polymul(a, b))
    for i in range(B):
        assert np.array_equal(prod[i], O.poly_mul(a[i], b[i])), (i, plan[i])
    assert names == [fam], names
    sites = set(names)
    # cmul: three rows, the tight one first or last, the others tiny
    rows = 3
    m = synth.small(rng, (B, rows, N))
    for i, sign in enumerate(plan):
        if sign is not None:
            r = 0 if (i // 3) % 2 == 0 else rows - 1
            m[i, r] = a[i]
            m[i, rows - 1 - r] = synth.small(rng, N)
    cm, names = run_prof(ctx, lambda: ctx.cmul(m, b))
    for i in range(B):
        assert np.array_equal(cm[i], O.mat_cmul(m[i][:, None, :], b[i])[:, 0, :]), (i, plan[i])
    assert names == [fam], names
    sites.update(names)
    print(f"[{cid}] {time.time() - t0:.1f}s, kernels {sorted(sites)}")


def test_aligned_sign_full_range_matvec(torch_mod):
    """Every key entry and every vector entry full range with aligned signs at (8,17,8), N = 2048: coefficient 0 of
    each tight row is +-17 N ((q-1)/2)^2, about 2^76.5, the largest exact result a key row can have; 17 float terms
    sum to the bound and three primes rebuild it."""
    N, n, k, l = 2048, 8, 17, 8
    ctx = make_ctx(N, n, k, l, b=BIG_B)
    A = np.full((n + l, k, N), HALF, dtype=np.int64)
    A[n + l - 1, :, 1::2] = -HALF
    ctx.load_key(A)
    v = np.stack([synth.conj(A[0]), -synth.conj(A[n + l - 1])])
    assert synth.negacyclic_coef0(A[0, 0], v[0, 0]) * k == k * N * HALF * HALF
    out, names = run_prof(ctx, lambda: ctx.matvec(2, v))
    for b in range(2):
        assert np.array_equal(out[b], O.mat_dot(A, v[b][:, None, :])[:, 0, :]), b
    assert names, names


# ---- verifiers: a miscounted prime flips accept to reject ----------------------------------------------------------------
def solve_open_t(A, n, z, c, d):
    return O.mat_sub(O.mat_dot(A[:n], z[:, None, :]), O.mat_cmul(c[:n, None, :], d))[:, 0, :]


OPEN_CASES = [
    ("512", 512, (1, 3, 1), {}, "unit_io_kernel"),
    ("1024", 1024, (1, 3, 1), {}, "unit_kernel"),
    ("2048-pair", 2048, (1, 3, 1), {}, "unit_kernel"),
    ("group-1024", 1024, (2, 5, 2), {}, "row_group_kernel"),
    ("block-1024", 1024, (4, 9, 4), {"RZK_BLOCK_MIN_LOGN": 10}, "row_block_kernel"),
]


@pytest.mark.parametrize("cid,N,shape,env,fam", OPEN_CASES, ids=[c[0] for c in OPEN_CASES])
def test_open_verify_at_prime_edges(torch_mod, cid, N, shape, env, fam):
    """z tight against an a1 row, t solved by the oracle: the oracle accepts, so must the GPU; one tampered t rejects.
    The same z as the opening r of Commitment::verify, c from the oracle's commit, one tampered c."""
    t0 = time.time()
    n, k, l = shape
    ctx = make_ctx(N, n, k, l, env=dict(env, RZK_GRID_CUS=1), b=BIG_B)
    P = O.Params(N=N, n=n, k=k, l=l, kappa=ctx.kappa, b=BIG_B)
    rng = np.random.default_rng(33000 + N + n)
    sites = set()
    for row in sorted({0, n - 1}):
        for np_ in (1, 2):
            A = edge_key(N, n, k, l, rng)
            load_tight_row(ctx, A, row, synth.edge_targets(np_)["just" if row == 0 else "near"], rng)
            B = 8
            z = synth.small(rng, (B, k, N))
            for b in range(1, B, 2):
                z[b] = tight_vector(A, row, n, k, l, 1 if b % 4 == 1 else -1, rng)
            c = synth.uniform(rng, (B, n + l, N))
            d = synth.challenge(rng, (B,), N, ctx.kappa)
            t = np.stack([solve_open_t(A, n, z[b], c[b], d[b]) for b in range(B)])
            t[B - 2, 0, 5] = O.center(int(t[B - 2, 0, 5]) + 1)
            want = [int(O.open_verify(P, A, z[b], t[b], c[b], d[b]) == 1) for b in range(B)]
            assert want == [1] * (B - 2) + [0, 1]
            acc, names = run_prof(ctx, lambda: ctx.open_verify(z, t, c, d))
            assert acc.tolist() == want, (row, np_)
            sites.update(names)
            # Commitment::verify with r = z: c solved by the oracle's commit, one tampered c rejects
            x = synth.uniform(rng, (B, l, N))
            cm = np.stack([O.commit(P, A, x[b], z[b])[0] for b in range(B)])
            cm[B - 1, n + l - 1, 3] = O.center(int(cm[B - 1, n + l - 1, 3]) - 1)
            want = [int(O.commitment_verify(P, A, cm[b], x[b], z[b])) for b in range(B)]
            assert want == [1] * (B - 1) + [0]
            ok, names = run_prof(ctx, lambda: ctx.commitment_verify(cm, x, z))
            assert ok.tolist() == want, (row, np_)
            sites.update(names)
    assert fam in sites, sites
    print(f"[{cid}] {time.time() - t0:.1f}s, kernels {sorted(sites)}")


def check_linear(ctx, P, A, z, zp, c, cp, g, d):
    """Solves t, t', u with the oracle (every entry then accepts), tampers u of entry B - 2, and compares the GPU's
    verdicts with the oracle's: all accept except that one."""
    n, l, N = ctx.n, ctx.l, ctx.N
    B = len(z)
    A2 = A[n:]
    t = np.stack([solve_open_t(A, n, z[b], c[b], d[b]) for b in range(B)])
    tp = np.stack([solve_open_t(A, n, zp[b], cp[b], d[b]) for b in range(B)])
    u = np.empty((B, l, N), dtype=np.int64)
    for b in range(B):
        lhs = O.mat_sub(O.mat_cmul(O.mat_dot(A2, z[b][:, None, :]), g[b]), O.mat_dot(A2, zp[b][:, None, :]))
        rhs = O.mat_cmul(O.mat_sub(O.mat_cmul(c[b][n:, None, :], g[b]), cp[b][n:, None, :]), d[b])
        u[b] = O.mat_sub(lhs, rhs)[:, 0, :]
    u[B - 2, l - 1, 9] = O.center(int(u[B - 2, l - 1, 9]) + 1)
    want = [int(O.linear_verify(P, A, z[b], zp[b], c[b], cp[b], g[b], t[b], tp[b], u[b], d[b]) == 1)
            for b in range(B)]
    assert want == [1] * (B - 2) + [0, 1]
    acc, names = run_prof(ctx, lambda: ctx.linear_verify(z, zp, c, cp, g, t, tp, u, d))
    assert acc.tolist() == want
    return acc, names


LIN_CASES = [
    # the verifier's rows on row_kernel, products by g on g's prepared image (dkey_transform_kernel)
    ("dkey-row", (1, 3, 1), {"RZK_LIN_E": 0, "RZK_DKEY": 2}, "row_kernel"),
    # products by g as vector x vector terms of row_kernel (both factors measured), two rows of each block
    ("vec-row", (2, 5, 2), {"RZK_LIN_E": 0, "RZK_DKEY": 0}, "row_kernel"),
]


@pytest.mark.parametrize("cid,shape,env,fam", LIN_CASES, ids=[c[0] for c in LIN_CASES])
def test_linear_verify_at_prime_edges(torch_mod, cid, shape, env, fam):
    """Linear under RZK_LIN_E=0 (the reference's grouping, c2 (.) g a product of its own): z tight against a1, and
    (g, c2) = (16 w, conj(w)) or (w, 16 conj(w)) so that c2 (.) g sits on a capacity edge with unequal factor norms;
    t, t', u solved by the oracle.  Batch entry 0 is tiny, so a norm read from the wrong entry is too small."""
    t0 = time.time()
    N = 1024
    n, k, l = shape
    ctx = make_ctx(N, n, k, l, env=dict(env, RZK_GRID_CUS=1), b=BIG_B)
    P = O.Params(N=N, n=n, k=k, l=l, kappa=ctx.kappa, b=BIG_B)
    rng = np.random.default_rng(34000 + n)
    sites = set()
    for np_ in (1, 2):
        A = edge_key(N, n, k, l, rng)
        load_tight_row(ctx, A, 0, synth.edge_targets(np_)["near"], rng)
        B = 8
        z, zp = synth.small(rng, (B, k, N)), synth.small(rng, (B, k, N))
        g = synth.small(rng, (B, N))
        c, cp = synth.small(rng, (B, n + l, N)), synth.small(rng, (B, n + l, N))
        d = synth.challenge(rng, (B,), N, ctx.kappa)
        for b in range(1, B):
            X = synth.edge_targets(np_)[("just", "near", "far")[b % 3]]
            if b % 2:
                z[b] = tight_vector(A, 0, n, k, l, 1, rng)
            else:
                g[b], c[b, n] = vec_pair(N, X, rng, lam_on_a=b % 4 == 0)
        acc, names = check_linear(ctx, P, A, z, zp, c, cp, g, d)
        sites.update(names)
    assert fam in sites, sites
    print(f"[linear-{cid}] {time.time() - t0:.1f}s, kernels {sorted(sites)}")


def test_linear_verify_nested_e(torch_mod):
    """Linear with the default rearrangement (RZK_LIN_E=1): the verifier forms e = a2.z - c2 (.) d mod q, then
    multiplies g (.) e.  The identity column of a2 is solved so that e is a test-chosen e*, and (g, e*) =
    (16 w, conj(w)) or (w, 16 conj(w)) puts g (.) e on a capacity edge.  Entry 0 is tiny."""
    t0 = time.time()
    N, n, k, l = 1024, 1, 3, 1
    ctx = make_ctx(N, n, k, l, env={"RZK_GRID_CUS": 1}, b=BIG_B)
    P = O.Params(N=N, n=n, k=k, l=l, kappa=ctx.kappa, b=BIG_B)
    rng = np.random.default_rng(35000)
    A = edge_key(N, n, k, l, rng)
    ctx.load_key(A)
    sites = set()
    for np_ in (1, 2):
        B = 8
        z, zp = synth.small(rng, (B, k, N)), synth.small(rng, (B, k, N))
        g = synth.small(rng, (B, N))
        c, cp = synth.small(rng, (B, n + l, N)), synth.small(rng, (B, n + l, N))
        d = synth.challenge(rng, (B,), N, ctx.kappa)
        for b in range(1, B):
            X = synth.edge_targets(np_)[("under", "just", "near", "far")[b % 4]]
            g[b], estar = vec_pair(N, X, rng, lam_on_a=b % 2 == 0)
            # a2 = [0 | 1 | a2']: e = z_n + a2'.z_rest - c2 (.) d, so z_n = e* + c2 (.) d - a2'.z_rest
            z[b, n] = 0
            rest = O.mat_dot(A[n:], z[b][:, None, :])[0, 0]
            z[b, n] = O.mat_sub(O.mat_add(estar[None, None, :], O.mat_cmul(c[b][n:, None, :], d[b])),
                                rest[None, None, :])[0, 0]
            e = O.mat_sub(O.mat_dot(A[n:], z[b][:, None, :]), O.mat_cmul(c[b][n:, None, :], d[b]))[0, 0]
            assert np.array_equal(e, estar)
            assert abs(synth.negacyclic_coef0(g[b], e)) >= X
        acc, names = check_linear(ctx, P, A, z, zp, c, cp, g, d)
        sites.update(names)
    assert "unit_kernel" in sites and "row_kernel" in sites, sites
    print(f"[linear-nested-e] {time.time() - t0:.1f}s, kernels {sorted(sites)}")


SUM_ENV = {"RZK_DKEY": 2, "RZK_SUM_D": 1, "RZK_OIMG": 1}


def test_sum_verify_output_images_at_prime_edges(torch_mod):
    """Sum at (2,5,2), V = 2, as a2.(sum_i g_i z_i - z') (RZK_SUM_D=1): the rows of D multiply g_i's prepared image
    (dkey_transform_kernel measures its norm, l2[]) by the transform of z_{i,c} that a1.z_i on row_group_kernel left
    behind (oimg_l2).  (g_i, z_{i,c}) = (16 w, conj(w)) or (w, 16 conj(w)) on an a2 column; t_i, t', u solved by the
    oracle, u of one entry tampered.  Entry 0 is tiny."""
    t0 = time.time()
    N, n, k, l, V = 1024, 2, 5, 2, 2
    ctx = make_ctx(N, n, k, l, env=dict(SUM_ENV, RZK_GRID_CUS=1), b=BIG_B)
    P = O.Params(N=N, n=n, k=k, l=l, kappa=ctx.kappa, b=BIG_B)
    rng = np.random.default_rng(36000)
    A = edge_key(N, n, k, l, rng)
    ctx.load_key(A)
    A2 = A[n:]
    raw, sites = [], set()
    for np_ in (1, 2):
        B = 6
        zs, zp = synth.small(rng, (B, V, k, N)), synth.small(rng, (B, k, N))
        gs = synth.small(rng, (B, V, N))
        cs, cp = synth.small(rng, (B, V, n + l, N)), synth.small(rng, (B, n + l, N))
        d = synth.challenge(rng, (B,), N, ctx.kappa)
        for b in range(1, B):
            X = synth.edge_targets(np_)[("under", "just", "near", "far")[b % 4]]
            i, col = b % V, (n, k - 1)[(b // V) % 2]       # an identity column of a2 and a general one
            gs[b, i], zs[b, i, col] = vec_pair(N, X, rng, lam_on_a=b % 3 == 0)
        ts = np.stack([np.stack([solve_open_t(A, n, zs[b, i], cs[b, i], d[b]) for i in range(V)]) for b in range(B)])
        tp = np.stack([solve_open_t(A, n, zp[b], cp[b], d[b]) for b in range(B)])
        u = np.empty((B, l, N), dtype=np.int64)
        for b in range(B):
            lhs = O.mat_sub(sum_mod([O.mat_cmul(O.mat_dot(A2, zs[b, i][:, None, :]), gs[b, i]) for i in range(V)]),
                            O.mat_dot(A2, zp[b][:, None, :]))
            inner = O.mat_sub(sum_mod([O.mat_cmul(cs[b, i][n:, None, :], gs[b, i]) for i in range(V)]),
                              cp[b][n:, None, :])
            u[b] = O.mat_sub(lhs, O.mat_cmul(inner, d[b]))[:, 0, :]
        u[B - 2, 0, 4] = O.center(int(u[B - 2, 0, 4]) - 1)
        want = [int(O.sum_verify(P, A, zs[b], zp[b], cs[b], cp[b], gs[b], ts[b], tp[b], u[b], d[b]) == 1)
                for b in range(B)]
        assert want == [1] * (B - 2) + [0, 1]
        ctx.prof_enable(True)
        ctx.prof_reset()
        acc = ctx.sum_verify(zs, zp, cs, cp, gs, ts, tp, u, d)
        raw += [nm for nm, _ in ctx.prof_read_kernels()]
        ctx.prof_enable(False)
        assert acc.tolist() == want, np_
    sites = {kernel_family(nm) for nm in raw}
    # the D rows read operand images: row_kernel's last template flag (DD) is on
    assert {"dkey_transform_kernel", "row_group_kernel"} <= sites, raw
    assert any(nm.startswith("row_kernel<") and nm.endswith(", true>") for nm in raw), raw
    print(f"[sum-oimg] {time.time() - t0:.1f}s, kernels {sorted(raw)}")


def sum_mod(mats):
    out = mats[0]
    for m in mats[1:]:
        out = O.mat_add(out, m)
    return out
