"""Short Linear and Sum proofs and the recompute ("recover") entry points behind all three short forms.

  * rzk_{open,linear,sum}_recover_batch[_dev] against the oracle's Mat operations (mat_dot, mat_cmul, mat_sub), bit for
    bit, host and device entry points, at the shapes that select the different launch paths: N = 64 (schoolbook rows),
    N = 512 / 1024 (1,3,1) (one unit-kernel launch with a rotation term), N = 1024 (4,9,4) (row groups, then rotations
    only), N = 2048 (1,3,1) and (2,5,2) (two-wavefront teams; row blocks, then transform products), and a context with
    RZK_LIN_E=0 RZK_SHIFT=0 (recover calls stay on the rearranged Linear pair; challenge products as transforms).  The
    kernels each shape ran are printed from the profiling table and their union must cover Small, Shift, Units and
    Groups or Blocks;
  * grid-stride trips: B = 100 with every grid sized for one CU against the uncapped context;
  * accept: the norm rule at its exact edge, a non-canonical coefficient in every input field, guard polynomials either
    side of every output slab;
  * d as foreign data: kappa + 1 non-zeros, a coefficient 2, a dense d;
  * the proofs: prove -> short -> verify_short, the recovered fields against the prover's, the verdicts against a
    reference built from the oracle's Mat operations, the hashlib transcript (fs_ref) and the oracle's verifiers, one
    tampered coefficient per field, a wrong aux, and the packed kinds 11 / 12 (round trip against short_ref, one
    flipped bit per field, device tensors, the wire entry points' refusal)."""
import ctypes as C
import functools

import numpy as np
import pytest

import fs_ref
import short_ref as SR
from oracle import oracle as O
from ring_zk_amd import _lib
from ring_zk_amd import fiat_shamir as FS
from ring_zk_amd import packed, synth
from test_gpu_baseline_shapes import P_of, dev, make_ctx, torch_mod  # noqa: F401
from test_gpu_packed import flip_bit, ref_ctx

pytestmark = pytest.mark.gpu

Q = O.Q_DEFAULT
AUX = bytes(range(70, 102))
B = 5
GUARD = -0x0123456789ABCDEF

# name -> (N, n, k, l, knobs)
CONFIGS = {
    "n64": (64, 1, 3, 1, None),
    "n512": (512, 1, 3, 1, None),
    "n1024": (1024, 1, 3, 1, None),
    "n1024split": (1024, 4, 9, 4, None),
    "n2048": (2048, 1, 3, 1, None),
    "n2048split": (2048, 2, 5, 2, None),
    "n512knobs": (512, 1, 3, 1, {"RZK_LIN_E": 0, "RZK_SHIFT": 0}),
}
SUM_VS = (1, 3)
PATH_OF_KERNEL = {"row_kernel_small": "Small", "shift_row_kernel": "Shift", "unit_kernel": "Units", "unit_io_kernel": "Units",
                  "row_group_kernel": "Groups", "row_block_kernel": "Blocks", "row_kernel": "Rows",
                  "fwd_slots_kernel": "Slots", "row_slots_kernel": "Slots", "dkey_transform_kernel": None}


@functools.lru_cache(maxsize=None)
def ctx_named(name, grid_cus=None):
    N, n, k, l, env = CONFIGS[name]
    env = dict(env or {})
    if grid_cus:
        env["RZK_GRID_CUS"] = grid_cus
    ctx = make_ctx(N, n, k, l, env=env or None)
    A = synth.key(np.random.default_rng(N + 13 * n), N, n, k, l)
    ctx.load_key(A)
    return ctx, A


# ---- the reference: the verification equations solved for t, t', u with the oracle's Mat operations ---------------------
def col(v):
    return np.ascontiguousarray(v)[:, None, :]


def ref_t(A, n, z, c, d):
    """open.rs:171-173, linear.rs:225-235, sum.rs:278-298: t = a1.z - c1 (.) d"""
    return O.mat_sub(O.mat_dot(A[:n], col(z)), O.mat_cmul(col(c[:n]), d))[:, 0, :]


def ref_open(A, n, z, c, d):
    return (ref_t(A, n, z, c, d),)


def ref_linear(A, n, z, zp, c, cp, g, d):
    """linear.rs:237-249: (a2.z) (.) g - a2.z' == (c2 (.) g - c2') (.) d + u"""
    lhs = O.mat_sub(O.mat_cmul(O.mat_dot(A[n:], col(z)), g), O.mat_dot(A[n:], col(zp)))
    w2 = O.mat_sub(O.mat_cmul(col(c[n:]), g), col(cp[n:]))
    return ref_t(A, n, z, c, d), ref_t(A, n, zp, cp, d), O.mat_sub(lhs, O.mat_cmul(w2, d))[:, 0, :]


def ref_sum(A, n, zs, zp, cs, cp, gs, d):
    """sum.rs:301-319: sum_i (a2.z_i) (.) g_i - a2.z' == (sum_i c2_i (.) g_i - c2') (.) d + u"""
    V = zs.shape[0]
    lhs = O.mat_cmul(O.mat_dot(A[n:], col(zs[0])), gs[0])
    w2 = O.mat_cmul(col(cs[0][n:]), gs[0])
    for i in range(1, V):
        lhs = O.mat_add(lhs, O.mat_cmul(O.mat_dot(A[n:], col(zs[i])), gs[i]))
        w2 = O.mat_add(w2, O.mat_cmul(col(cs[i][n:]), gs[i]))
    lhs = O.mat_sub(lhs, O.mat_dot(A[n:], col(zp)))
    w2 = O.mat_sub(w2, col(cp[n:]))
    ts = np.stack([ref_t(A, n, zs[i], cs[i], d) for i in range(V)])
    return ts, ref_t(A, n, zp, cp, d), O.mat_sub(lhs, O.mat_cmul(w2, d))[:, 0, :]


PROOFS = {   # proof -> (Context method, reference, names of the inputs in call order)
    "open": ("open_recover", ref_open, ("z", "c", "d")),
    "linear": ("linear_recover", ref_linear, ("z", "zp", "c", "cp", "g", "d")),
    "sum": ("sum_recover", ref_sum, ("zs", "zp", "cs", "cp", "gs", "d")),
}


def draw_inputs(ctx, proof, V, nb, seed):
    """Canonical inputs of a recover call: responses that pass the norm rule, everything else uniform; d a challenge."""
    P = P_of(ctx)
    N, n, k, l = ctx.N, ctx.n, ctx.k, ctx.l
    rng = np.random.default_rng(seed)
    lead = {"z": (k,), "zp": (k,), "zs": (V, k), "c": (n + l,), "cp": (n + l,), "cs": (V, n + l), "g": (), "gs": (V,)}
    out = []
    for name in PROOFS[proof][2]:
        if name == "d":
            out.append(synth.challenge(rng, (nb,), N, P.kappa))
        elif name.startswith("z"):
            out.append(synth.gauss(rng, (nb,) + lead[name] + (N,), P.sigma))
        else:
            out.append(synth.uniform(rng, (nb,) + lead[name] + (N,)))
    return out


def reference(A, n, proof, ins):
    """The reference outputs of a batch, one array per output."""
    per = [PROOFS[proof][1](A, n, *[a[b] for a in ins]) for b in range(ins[0].shape[0])]
    return [np.stack([p[i] for p in per]) for i in range(len(per[0]))]


def proofs_and_v():
    return [("open", None), ("linear", None)] + [("sum", V) for V in SUM_VS]


@functools.lru_cache(maxsize=None)
def honest_case(name, proof, V):
    """(inputs, reference outputs) of the B proofs every test of a configuration starts from; treated as read-only."""
    ctx, A = ctx_named(name)
    ins = draw_inputs(ctx, proof, V, B, seed=ctx.N + 7 * ctx.n + (V or 0))
    return ins, reference(A, ctx.n, proof, ins)


def recover(ctx, proof, ins):
    *outs, acc = getattr(ctx, PROOFS[proof][0])(*ins)
    return outs, acc


def to_np(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def kernels_of(torch, name):
    """Kernel names of the open, linear and sum (V = 3) recover calls of a configuration, from the profiling table."""
    ctx, _ = ctx_named(name)
    ctx.prof_enable(True)
    names = {}
    try:
        for proof, V in (("open", None), ("linear", None), ("sum", 3)):
            ins, _ = honest_case(name, proof, V)
            ctx.prof_reset()
            recover(ctx, proof, [dev(torch, a) for a in ins])
            ctx.synchronize()
            names[proof] = [k for k, _ in ctx.prof_read_kernels()]
    finally:
        ctx.prof_enable(False)
    return names


def paths_of(names):
    out = set()
    for ks in names.values():
        for k in ks:
            for part in k.split(" + "):
                path = PATH_OF_KERNEL[part.split("<")[0]]
                if path:
                    out.add(path)
    return out


# ---- 3: recompute against the oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CONFIGS))
def test_recover_matches_the_oracle(torch_mod, name):
    ctx, A = ctx_named(name)
    for proof, V in proofs_and_v():
        ins, want = honest_case(name, proof, V)
        outs, acc = recover(ctx, proof, ins)
        assert acc.tolist() == [1] * B, (proof, V)
        for got, ref in zip(outs, want):
            assert got.shape == ref.shape and np.array_equal(got, ref), (proof, V)
        douts, dacc = recover(ctx, proof, [dev(torch_mod, a) for a in ins])
        assert to_np(dacc).tolist() == [1] * B
        for got, ref in zip(douts, want):
            assert np.array_equal(to_np(got), ref), (proof, V, "device")
    names = kernels_of(torch_mod, name)
    print("%s: %s -> %s" % (name, names, sorted(paths_of(names))))


def test_the_shapes_cover_the_launch_paths(torch_mod):
    per = {name: paths_of(kernels_of(torch_mod, name)) for name in CONFIGS}
    print(per)
    union = set().union(*per.values())
    assert {"Small", "Shift", "Units"} <= union and ({"Groups", "Blocks"} & union), per
    assert per["n64"] == {"Small"}
    assert "Shift" in per["n1024split"] and "Groups" in per["n1024split"]     # a1.z grouped, then rotations only
    assert "Blocks" in per["n2048split"]
    assert "Units" in per["n1024"] and "Units" in per["n2048"]
    assert "Shift" not in per["n512knobs"]                                     # RZK_SHIFT=0: no rotation kernel
    # n == 1: the Open recompute is ONE launch
    for name in ("n512", "n1024", "n2048"):
        assert len(kernels_of(torch_mod, name)["open"]) == 1, name
    names = kernels_of(torch_mod, "n2048")
    assert all("PairTeam" in k for k in names["open"]), names                  # two-wavefront teams at N = 2048


def test_grid_stride_trips(torch_mod):
    """B = 100 at N = 1024 (4,9,4) with every grid sized for one CU: the capped context makes many trips per
    workgroup (and owns a whole proof per team), the uncapped one few; same bytes."""
    (capped, _), (free, _) = ctx_named("n1024split", 1), ctx_named("n1024split")
    for proof, V in (("open", None), ("linear", None), ("sum", 3)):
        ins = [dev(torch_mod, a) for a in draw_inputs(free, proof, V, 100, seed=900 + (V or 0))]
        o1, a1 = recover(capped, proof, ins)
        o2, a2 = recover(free, proof, ins)
        assert to_np(a1).tolist() == [1] * 100 and to_np(a2).tolist() == [1] * 100
        for x, y in zip(o1, o2):
            assert torch_mod.equal(x, y), proof
    # the first and the last proof against the oracle
    ins, A = draw_inputs(free, "sum", 3, 100, seed=903), ctx_named("n1024split")[1]
    outs, _ = recover(capped, "sum", [dev(torch_mod, a) for a in ins])
    for b in (0, 99):
        for got, ref in zip(outs, ref_sum(A, free.n, *[a[b] for a in ins])):
            assert np.array_equal(to_np(got[b]), ref), b


# ---- accept ---------------------------------------------------------------------------------------------------------------
EDGE_CONFIGS = ["n64", "n512", "n1024split", "n2048"]


def response_names(proof):
    return [nm for nm in PROOFS[proof][2] if nm.startswith("z")]


@pytest.mark.parametrize("name", EDGE_CONFIGS)
def test_accept_is_the_norm_rule_at_its_exact_edge(torch_mod, name):
    """One polynomial of a response vector with sum of squares (verify_bound + 1)^2 - 1 (accepted, and its outputs still
    the oracle's) and one with (verify_bound + 1)^2 (rejected); the expectation is the oracle's check_norm."""
    ctx, A = ctx_named(name)
    P = P_of(ctx)
    L = (P.verify_bound + 1) ** 2
    rng = np.random.default_rng(ctx.N + 3)
    for proof, V in (("open", None), ("linear", None), ("sum", 3)):
        ins0, _ = honest_case(name, proof, V)
        for which in response_names(proof):
            ins = [a.copy() for a in ins0]
            zv = ins[PROOFS[proof][2].index(which)]
            flat = zv.reshape(B, -1, ctx.N)
            flat[1, 0] = synth.norm_edge(ctx.N, L - 1, "spread", 0, rng)
            flat[3, flat.shape[1] - 1] = synth.norm_edge(ctx.N, L, "spread", 0, rng)
            want_acc = [int(all(O.check_norm(a[b], P.verify_bound) for a, nm in zip(ins, PROOFS[proof][2]) if nm.startswith("z")))
                        for b in range(B)]
            assert want_acc == [1, 1, 1, 0, 1]
            outs, acc = recover(ctx, proof, ins)
            assert acc.tolist() == want_acc, (proof, which)
            dacc = recover(ctx, proof, [dev(torch_mod, a) for a in ins])[1]
            assert to_np(dacc).tolist() == want_acc, (proof, which, "device")
            for got, ref in zip(outs, PROOFS[proof][1](A, ctx.n, *[a[1] for a in ins])):
                assert np.array_equal(got[1], ref), (proof, which)


@pytest.mark.parametrize("name", EDGE_CONFIGS)
def test_a_non_canonical_coefficient_clears_its_own_proof(torch_mod, name):
    """q added to (or the value 2^32 + s put in place of) one coefficient of each input field: the call returns OK, exactly
    that proof's verdict is cleared, the other proofs' outputs are untouched.  Open does not read the rows c2 of c (the
    transcript hash range-tests them): its coefficient sits in c1."""
    ctx, _ = ctx_named(name)
    for proof, V in (("open", None), ("linear", None), ("sum", 3)):
        ins0, want = honest_case(name, proof, V)
        for f, nm in enumerate(PROOFS[proof][2]):
            victim = (f + 1) % B
            ins = [a.copy() for a in ins0]
            flat = ins[f].reshape(B, -1, ctx.N)
            row = 0 if (proof == "open" and nm == "c") else flat.shape[1] - 1
            pos = (17 * f + 5) % ctx.N
            flat[victim, row, pos] = flat[victim, row, pos] + ctx.q if f % 2 else (1 << 32) + int(flat[victim, row, pos]) % 1000
            expect = [int(b != victim) for b in range(B)]
            outs, acc = recover(ctx, proof, ins)                       # host entry point: the call itself succeeds
            assert acc.tolist() == expect, (proof, nm)
            douts, dacc = recover(ctx, proof, [dev(torch_mod, a) for a in ins])
            assert to_np(dacc).tolist() == expect, (proof, nm, "device")
            keep = [b for b in range(B) if b != victim]
            for got, dgot, ref in zip(outs, douts, want):
                assert np.array_equal(got[keep], ref[keep]) and np.array_equal(to_np(dgot)[keep], ref[keep]), (proof, nm)


@pytest.mark.parametrize("name", EDGE_CONFIGS)
def test_guard_polynomials_round_every_output_stay_untouched(torch_mod, name):
    """The device entry points write ts / t / tp / u into the middle of buffers with one guard polynomial either side."""
    ctx, _ = ctx_named(name)
    L, h, N = ctx._L, ctx._h, ctx.N
    for proof, V in (("open", None), ("linear", None), ("sum", 3)):
        ins0, want = honest_case(name, proof, V)
        ins = [dev(torch_mod, a) for a in ins0]
        bufs = [torch_mod.full((w[0].size * B + 2 * N,), GUARD, dtype=torch_mod.int64, device="cuda") for w in want]
        acc = torch_mod.full((B + 2,), 7, dtype=torch_mod.uint8, device="cuda")
        ctx._bind_torch_stream()
        p = [C.c_void_p(a.data_ptr()) for a in ins] + [C.c_void_p(b.data_ptr() + 8 * N) for b in bufs] + [C.c_void_p(acc.data_ptr() + 1)]
        fn = getattr(L, "rzk_%s_recover_batch_dev" % proof)
        st = fn(h, V, *p, B) if proof == "sum" else fn(h, *p, B)
        assert st == 0, ctx._L.rzk_last_error(h)
        torch_mod.cuda.synchronize()
        assert acc.cpu().tolist() == [7] + [1] * B + [7]
        for buf, ref in zip(bufs, want):
            got = buf.cpu().numpy()
            assert (got[:N] == GUARD).all() and (got[-N:] == GUARD).all(), proof
            assert np.array_equal(got[N:-N].reshape(ref.shape), ref), proof


# ---- d is foreign data ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EDGE_CONFIGS + ["n512knobs"])
def test_foreign_d_is_multiplied_exactly(torch_mod, name):
    """d with kappa + 1 non-zeros, with a coefficient 2, and dense over the whole centred range: the recompute is still
    the oracle's Mat arithmetic, and accept does not depend on d's shape."""
    ctx, A = ctx_named(name)
    half = (ctx.q - 1) // 2
    rng = np.random.default_rng(ctx.N + 99)
    for proof, V in (("open", None), ("linear", None), ("sum", 3)):
        ins0, _ = honest_case(name, proof, V)
        ins = [a.copy() for a in ins0]
        d = ins[-1]
        zero = np.flatnonzero(d[0] == 0)
        d[0, zero[len(zero) // 2]] = -1                                  # kappa + 1 non-zeros
        d[1, np.flatnonzero(d[1])[3]] = 2                                # a coefficient 2
        d[2] = rng.integers(-half, half + 1, ctx.N, dtype=np.int64)      # dense
        d[2, 0], d[2, ctx.N - 1] = half, -half
        assert np.count_nonzero(d[0]) == ctx.kappa + 1 and d[1].max() == 2
        want = reference(A, ctx.n, proof, ins)
        outs, acc = recover(ctx, proof, ins)
        assert acc.tolist() == [1] * B, proof
        for got, ref in zip(outs, want):
            assert np.array_equal(got, ref), proof
        douts, dacc = recover(ctx, proof, [dev(torch_mod, a) for a in ins])
        assert to_np(dacc).tolist() == [1] * B
        for got, ref in zip(douts, want):
            assert np.array_equal(to_np(got), ref), (proof, "device")


def test_argument_rules(torch_mod):
    ctx, _ = ctx_named("n64")
    L, h = ctx._L, ctx._h
    ins, _ = honest_case("n64", "open", None)
    z, c, d = ins
    t, acc = np.zeros((B, 1, 64), np.int64), np.full(B, 9, np.uint8)
    p = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    assert L.rzk_open_recover_batch(h, p(z), p(c), p(d), p(t), p(acc), 0) == 0 and acc.tolist() == [9] * B   # B == 0: a no-op
    assert L.rzk_open_recover_batch(h, None, None, None, None, None, 0) == 0
    assert L.rzk_open_recover_batch(h, p(z), p(c), p(d), None, p(acc), B) == _lib.RZK_E_ARG
    assert L.rzk_open_recover_batch(h, p(z), p(c), p(d), p(t), None, B) == _lib.RZK_E_ARG
    assert L.rzk_sum_recover_batch(h, 0, *[p(z)] * 9, p(acc), B) == _lib.RZK_E_ARG                           # V == 0
    # n != l: the c1 / c2 split does not exist (as in the verifiers)
    odd = make_ctx(64, 2, 4, 1)
    odd.load_key(synth.key(np.random.default_rng(5), 64, 2, 4, 1))
    zz, cc = np.zeros((B, 4, 64), np.int64), np.zeros((B, 3, 64), np.int64)
    tt = np.zeros((B, 2, 64), np.int64)
    assert odd._L.rzk_open_recover_batch(odd._h, p(zz), p(cc), p(d), p(tt), p(acc), B) == _lib.RZK_E_ARG
    assert odd._L.rzk_linear_recover_batch(odd._h, p(zz), p(zz), p(cc), p(cc), p(d), p(d), p(tt), p(tt), p(tt), p(acc),
                                           B) == _lib.RZK_E_ARG
    assert _lib.ABI_VERSION >= 12 and int(L.rzk_abi_version()) == _lib.ABI_VERSION


# ---- 4: the proofs ------------------------------------------------------------------------------------------------------------
def keyed_ctx(N):
    return ctx_named({64: "n64", 1024: "n1024"}[N])


@functools.lru_cache(maxsize=None)
def honest_proof(kind, N):
    """(c, cp, g, t, tp, u, z, zp) / (cs, cp, gs, ts, tp, u, zs, zp) of B honest proofs under AUX, V = 2 for Sum."""
    ctx, _ = keyed_ctx(N)
    P, k = P_of(ctx), ctx.k
    rng = np.random.default_rng(N + 21 + len(kind))
    small = lambda *lead: synth.small(rng, lead + (k, N), P.b)        # noqa: E731
    gauss = lambda *lead: synth.gauss(rng, lead + (k, N), P.sigma)    # noqa: E731
    if kind == "linear":
        g = synth.uniform(rng, (B, N))
        c, cp, t, tp, u, z, zp, ok = FS.linear_prove(ctx, g, synth.uniform(rng, (B, 1, N)), small(B), small(B), gauss(B), gauss(B), aux=AUX)
        assert ok.all()
        return c, cp, g, t, tp, u, z, zp
    gs, xs = synth.uniform(rng, (B, 2, N)), synth.uniform(rng, (B, 2, 1, N))
    cs, cp, ts, tp, u, zs, zp, ok = FS.sum_prove(ctx, gs, xs, small(B, 2), small(B), gauss(B, 2), gauss(B), aux=AUX)
    assert ok.all()
    return cs, cp, gs, ts, tp, u, zs, zp


def oracle_short_linear(ctx, A, c, cp, g, d, z, zp, aux):
    """The reference verdict of a short Linear proof: t', tp', u' from the oracle's Mat operations, d' from the hashlib
    transcript under the FULL commitment kind, the norm rule and the equations from the oracle's interactive verifier."""
    P = P_of(ctx)
    kd = fs_ref.key_digest(A, ctx.q, ctx.N, ctx.n, ctx.k, ctx.l, ctx.kappa, ctx.b)
    out = []
    for b in range(c.shape[0]):
        t, tp, u = ref_linear(A, ctx.n, z[b], zp[b], c[b], cp[b], g[b], d[b])
        fields = [a[None] for a in (c[b], cp[b], g[b], t, tp, u)]
        d2, _ = fs_ref.challenge(packed.MSG_LINEAR_COMMITMENT, 0, kd, aux, fields, ctx.N, ctx.kappa)
        ok = O.linear_verify(P, A, z[b], zp[b], c[b], cp[b], g[b], t, tp, u, d[b]) == 1
        out.append(int(np.array_equal(d2[0], d[b]) and ok))
    return np.array(out, dtype=np.uint8)


def oracle_short_sum(ctx, A, cs, cp, gs, d, zs, zp, aux):
    P, V = P_of(ctx), cs.shape[1]
    kd = fs_ref.key_digest(A, ctx.q, ctx.N, ctx.n, ctx.k, ctx.l, ctx.kappa, ctx.b)
    out = []
    for b in range(cs.shape[0]):
        ts, tp, u = ref_sum(A, ctx.n, zs[b], zp[b], cs[b], cp[b], gs[b], d[b])
        fields = [a[None] for a in (cp[b], cs[b], gs[b], tp, ts, u)]
        d2, _ = fs_ref.challenge(packed.MSG_SUM_COMMITMENT, V, kd, aux, fields, ctx.N, ctx.kappa)
        ok = O.sum_verify(P, A, zs[b], zp[b], cs[b], cp[b], gs[b], ts, tp, u, d[b]) == 1
        out.append(int(np.array_equal(d2[0], d[b]) and ok))
    return np.array(out, dtype=np.uint8)


def tamper(a, idx):
    m = a.copy()
    m[idx] = O.center(int(m[idx]) + 1)
    return m


def short_api(kind, ctx, A):
    """(short fields of a full proof, verify_short, recover + full verify, reference verdict, packed kind, V)."""
    if kind == "linear":
        def split(c, cp, g, t, tp, u, z, zp):
            return [c, cp, g, FS.linear_short(ctx, c, cp, g, t, tp, u, z, zp, aux=AUX), z, zp], (t, tp, u)

        def full_on_recovered(c, cp, g, d, z, zp, aux):
            t, tp, u, _ = ctx.linear_recover(z, zp, c, cp, g, d)
            return (t, tp, u), FS.linear_verify(ctx, c, cp, g, t, tp, u, z, zp, aux=aux)

        return (split, lambda f, aux: FS.linear_verify_short(ctx, *f, aux=aux), full_on_recovered,
                lambda f, aux: oracle_short_linear(ctx, A, *f, aux), packed.MSG_LINEAR_SHORT, None,
                lambda r, aux: FS.linear_verify_short_packed(ctx, r, aux=aux))

    def split(cs, cp, gs, ts, tp, u, zs, zp):
        return [cs, cp, gs, FS.sum_short(ctx, cs, cp, gs, ts, tp, u, zs, zp, aux=AUX), zs, zp], (ts, tp, u)

    def full_on_recovered(cs, cp, gs, d, zs, zp, aux):
        ts, tp, u, _ = ctx.sum_recover(zs, zp, cs, cp, gs, d)
        return (ts, tp, u), FS.sum_verify(ctx, cs, cp, gs, ts, tp, u, zs, zp, aux=aux)

    return (split, lambda f, aux: FS.sum_verify_short(ctx, *f, aux=aux), full_on_recovered,
            lambda f, aux: oracle_short_sum(ctx, A, *f, aux), packed.MSG_SUM_SHORT, 2,
            lambda r, aux: FS.sum_verify_short_packed(ctx, r, 2, aux=aux))


def record_order(kind, f):
    """The short fields in the record's declaration order: Linear as they are; Sum { cp, cs, gs, d, zp, zs }."""
    return f if kind == "linear" else [f[1], f[0], f[2], f[3], f[5], f[4]]


@pytest.mark.parametrize("N", [64, 1024])
@pytest.mark.parametrize("kind", ["linear", "sum"])
def test_short_proofs(torch_mod, kind, N):
    ctx, A = keyed_ctx(N)
    split, verify, full_on_recovered, oracle_verdict, _, _, _ = short_api(kind, ctx, A)
    f, prover_fields = split(*honest_proof(kind, N))
    acc = verify(f, AUX)
    assert acc.tolist() == [1] * B                                        # every honest proof
    recovered, full = full_on_recovered(*f, AUX)
    for got, ref in zip(recovered, prover_fields):                        # the recovered fields are the prover's
        assert np.array_equal(got, ref)
    assert np.array_equal(full, acc) and np.array_equal(oracle_verdict(f, AUX), acc)
    assert np.array_equal(to_np(verify([dev(torch_mod, a) for a in f], AUX)), acc)
    # one tampered coefficient in each field of the short proof
    for i in range(len(f)):
        victim = (i + 2) % B
        idx = (victim,) + tuple((3 * i + j) % s for j, s in enumerate(f[i].shape[1:]))
        g2 = list(f)
        g2[i] = tamper(f[i], idx)
        got = verify(g2, AUX)
        assert got.tolist() == [int(b != victim) for b in range(B)], (kind, i)
        assert np.array_equal(got, oracle_verdict(g2, AUX)), (kind, i)
        assert np.array_equal(got, full_on_recovered(*g2, AUX)[1]), (kind, i)
    # a wrong aux rejects all, and the reference agrees
    for aux in (None, bytes(32)):
        other = verify(f, aux)
        assert not other.any() and np.array_equal(other, oracle_verdict(f, aux))
    # foreign data rejects its proof and does not fail the call: a non-canonical d, a non-canonical response
    for i in (3, 4):
        g2 = list(f)
        g2[i] = f[i].copy()
        g2[i].reshape(B, -1)[2, 5] += ctx.q
        assert verify(g2, AUX).tolist() == [1, 1, 0, 1, 1], (kind, i)
        assert to_np(verify([dev(torch_mod, a) for a in g2], AUX)).tolist() == [1, 1, 0, 1, 1], (kind, i)


@pytest.mark.parametrize("N", [64, 1024])
@pytest.mark.parametrize("kind", ["linear", "sum"])
def test_short_proofs_packed(torch_mod, kind, N):
    ctx, A = keyed_ctx(N)
    split, verify, _, _, pk, V, verify_packed = short_api(kind, ctx, A)
    f, _ = split(*honest_proof(kind, N))
    acc = verify(f, AUX)
    slabs = record_order(kind, f)
    rec, ok = packed.encode_batch(ctx, pk, *slabs, V=V)
    rc = ref_ctx(ctx)
    want, wok = SR.encode(rc, pk, slabs, V)
    assert ok.all() and wok.all() and np.array_equal(rec, want)
    assert rec.shape[1] == packed.record_bytes(ctx, pk, V) == SR.record_bytes(rc, pk, V)
    *back, bok = packed.decode_batch(ctx, pk, rec, V=V)                   # round trip
    assert bok.all() and all(np.array_equal(a, b) for a, b in zip(back, slabs))
    drec, dok = packed.encode_batch(ctx, pk, *[dev(torch_mod, a) for a in slabs], V=V)
    assert np.array_equal(to_np(drec), rec) and to_np(dok).all()
    assert np.array_equal(verify_packed(rec, AUX), acc) and acc.all()
    assert np.array_equal(to_np(verify_packed(dev(torch_mod, rec), AUX)), acc)
    assert not verify_packed(rec, bytes(32)).any()
    # one flipped bit inside each field's byte range rejects exactly its record's proof; device tensors agree
    for i, (lo, hi) in enumerate(SR.field_byte_ranges(rc, pk, V)):
        victim = (i + 1) % B
        byte = lo + ((hi - lo) * (i + 1)) // 7
        bad = flip_bit(rec, victim, byte, i % 8)
        got = verify_packed(bad, AUX)
        assert got.tolist() == [int(b != victim) for b in range(B)], (kind, i, byte)
        assert np.array_equal(to_np(verify_packed(dev(torch_mod, bad), AUX)), got), (kind, i)
    # a record of the other V / kind does not decode; the header's kind byte is checked
    bad = rec.copy()
    bad[1, 5] = packed.MSG_OPEN_SHORT
    assert verify_packed(bad, AUX).tolist() == [1, 0, 1, 1, 1]
    # a short proof and a full proof are one proof in two encodings: the full records verify too
    if kind == "linear":
        c, cp, g, t, tp, u, z, zp = honest_proof(kind, N)
        assert FS.linear_verify(ctx, c, cp, g, t, tp, u, z, zp, aux=AUX).all()
    if N == 1024:
        assert rec.shape[1] == {"linear": 37640, "sum": 58376}[kind]
    for k in (packed.MSG_LINEAR_SHORT, packed.MSG_SUM_SHORT):             # the wire entry points reject both kinds
        assert ctx._L.rzk_wire_max_bytes(ctx._h, k, 2, 8) == 0
    assert ctx._L.rzk_packed_record_bytes(ctx._h, 10, 0) == 0             # kind 10 stays unassigned


@pytest.mark.parametrize("N", [64, 1024])
def test_rebased_open_short_verifier_agrees_with_recover_then_verify(torch_mod, N):
    """open_verify_short is recover + transcript + compare; open_verify on the recovered t gives the same verdicts."""
    ctx, A = keyed_ctx(N)
    P = P_of(ctx)
    rng = np.random.default_rng(N + 55)
    c, t, z, _ = FS.open_prove(ctx, synth.uniform(rng, (B, 1, N)), synth.small(rng, (B, 3, N), P.b), synth.gauss(rng, (B, 3, N), P.sigma),
                               aux=AUX)
    d = FS.open_short(ctx, c, t, z, aux=AUX)
    t2, acc = ctx.open_recover(z, c, d)
    assert np.array_equal(t2, t) and acc.all()
    for cc, dd, zz in ((c, d, z), (tamper(c, (1, 1, 7)), d, z), (c, tamper(d, (2, 9)), z), (c, d, tamper(z, (4, 2, 63)))):
        got = FS.open_verify_short(ctx, cc, dd, zz, aux=AUX)
        tt, _ = ctx.open_recover(zz, cc, dd)
        assert np.array_equal(got, FS.open_verify(ctx, cc, tt, zz, aux=AUX))
    assert FS.open_verify_short(ctx, c, d, z, aux=AUX).all()
