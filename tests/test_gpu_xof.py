"""The XP1 seed expansion on the GPU (rzk_xof_uniform_batch[_dev], rzk_key_expand; Context.xof_uniform / expand_key,
fiat_shamir.multipliers) bit for bit against tests/xof_ref.py (hashlib): host and device entry points at
every chunk shape, the places where a chunk can end put into one wavefront, the grid cap, guard bytes round the output,
domain / seed / index separation, the argument rules, the expanded key with its structure and digest, and a Linear proof
whose key and multiplier both come from seeds."""
import ctypes as C
import functools

import numpy as np
import pytest

import xof_ref
from ring_zk_amd import RzkError
from ring_zk_amd import fiat_shamir as FS
from ring_zk_amd import synth
from test_gpu_baseline_shapes import P_of, dev, make_ctx, torch_mod  # noqa: F401
from test_xof_host import EDGE_NAMES, edge_seeds

pytestmark = pytest.mark.gpu

Q = 3515337053
GUARD = 0x5a5a5a5a5a5a5a5a


@functools.lru_cache(maxsize=None)
def ref_poly(N, domain, seed, p):
    a = xof_ref.poly(Q, N, domain, seed, p)
    a.setflags(write=False)
    return a


def ref_uniform(N, domain, seeds, rows):
    return np.stack([np.stack([ref_poly(N, domain, s, r) for r in range(rows)]) for s in seeds])


def seed_array(seeds):
    return np.frombuffer(b"".join(seeds), dtype=np.uint8).reshape(len(seeds), 32).copy()


def ctx_of(N, env=None, nkl=(1, 3, 1)):
    return make_ctx(N, *nkl, env=env, kappa=min(N, 36))


def both(torch, ctx, seeds, rows, domain):
    """[B][rows][N] from the host entry point after checking that the device entry point gives the same bytes."""
    sa = seed_array(seeds)
    out = ctx.xof_uniform(sa, rows, domain)
    dout = ctx.xof_uniform(dev(torch, sa), rows, domain)
    ctx.synchronize()
    assert out.shape == (len(seeds), rows, ctx.N) and out.dtype == np.int64
    assert np.array_equal(dout.cpu().numpy(), out)
    return out


@pytest.mark.parametrize("N", [4, 256, 512, 1024, 2048])
def test_matches_reference(torch_mod, N):
    """N = 4: four values per lane and 32 rows per drain step; 256: one full chunk; 512 .. 2048: 2, 4, 8 chunks per
    polynomial.  (5, 7) at N = 512 is 70 chunks: one full wavefront and a partial one."""
    ctx = ctx_of(N)
    for B, rows in ((1, 1), (3, 2), (5, 7)):
        seeds = [xof_ref.seed_of(1000 * N + 10 * B + i) for i in range(B)]
        for domain in (1, 0x80000001):
            out = both(torch_mod, ctx, seeds, rows, domain)
            assert np.array_equal(out, ref_uniform(N, domain, seeds, rows)), (B, rows, domain)
            assert int(out.max()) <= ctx.half and int(out.min()) >= -ctx.half


def test_chunk_ends_share_a_wavefront(torch_mod):
    """The seeds of the host tier's edge conditions in different lanes of one launch: at N = 256 a chunk that ends on the
    last word of a rate block, on a low and on a high half, the 11-block chunk and the shortest of the first 2000 seeds
    sit between ordinary lanes of one wavefront; at N = 4 lanes with and without a rejection."""
    edges = edge_seeds()
    assert sorted(edges) == sorted(EDGE_NAMES)
    used = {i: xof_ref.chunk(Q, 256, 1, xof_ref.seed_of(i), 0, 0)[1] for i in range(2000)}
    shortest = min(used, key=used.get)
    assert used[shortest] <= 9 * xof_ref.RATE_WORDS32 < 10 * xof_ref.RATE_WORDS32 < edges["most_words"][2]   # 9 against 11 blocks
    lanes = {5: edges["block_end"][1], 17: edges["low_half"][1], 18: edges["high_half"][1], 40: edges["most_words"][1],
             41: shortest, 63: edges["most_words"][1]}
    idx = [lanes.get(b, 3000 + b) for b in range(64)]
    seeds = [xof_ref.seed_of(i) for i in idx]
    ctx = ctx_of(256)
    out = both(torch_mod, ctx, seeds, 1, 1)
    for b in range(64):
        assert np.array_equal(out[b, 0], ref_poly(256, 1, seeds[b], 0)), (b, idx[b])
    ctx4 = ctx_of(4)
    seeds4 = [xof_ref.seed_of(i) for i in range(64)]
    assert edges["n4_no_rejection"][1] < 64 and edges["n4_rejection"][1] < 64
    assert np.array_equal(both(torch_mod, ctx4, seeds4, 1, 1), ref_uniform(4, 1, seeds4, 1))


def test_grid_cap_gives_the_same_result(torch_mod):
    """600 chunks are ten wavefronts of tasks; a context made for one CU runs at most eight workgroups, so some make a
    second trip through the kernel's grid-stride loop."""
    seeds = seed_array([xof_ref.seed_of(7000 + i) for i in range(100)])
    want = ctx_of(512).xof_uniform(seeds, 3, 2)
    capped = ctx_of(512, env={"RZK_GRID_CUS": 1})
    got = capped.xof_uniform(seeds, 3, 2)
    assert np.array_equal(got, want)
    for b in (0, 21, 99):   # lanes of the first and of the second trip
        assert np.array_equal(want[b], ref_uniform(512, 2, [bytes(seeds[b])], 3)[0])
    dgot = capped.xof_uniform(dev(torch_mod, seeds), 3, 2)
    capped.synchronize()
    assert np.array_equal(dgot.cpu().numpy(), want)


@pytest.mark.parametrize("N,B,rows", [(4, 3, 1), (512, 5, 7), (256, 1, 1)])
def test_guard_words_stay_untouched(torch_mod, N, B, rows):
    torch = torch_mod
    ctx = ctx_of(N)
    seeds = seed_array([xof_ref.seed_of(i) for i in range(B)])
    n = B * rows * N
    pad = 64   # int64 words either side; the slab itself stays 16-byte aligned
    want = ref_uniform(N, 3, [bytes(s) for s in seeds], rows).reshape(-1)
    hbuf = np.full(n + 2 * pad, GUARD, dtype=np.int64)
    st = ctx._L.rzk_xof_uniform_batch(ctx._h, C.c_void_p(seeds.ctypes.data), 3, rows, C.c_void_p(hbuf.ctypes.data + 8 * pad), B)
    assert st == 0
    dbuf = torch.full((n + 2 * pad,), GUARD, dtype=torch.int64, device="cuda")
    dseeds = dev(torch, seeds)
    ctx._bind_torch_stream()
    st = ctx._L.rzk_xof_uniform_batch_dev(ctx._h, C.c_void_p(dseeds.data_ptr()), 3, rows, C.c_void_p(dbuf.data_ptr() + 8 * pad), B)
    assert st == 0
    ctx.synchronize()
    for buf in (hbuf, dbuf.cpu().numpy()):
        assert (buf[:pad] == GUARD).all() and (buf[pad + n:] == GUARD).all()
        assert np.array_equal(buf[pad:pad + n], want)


def test_domains_seeds_and_indices_are_separate(torch_mod):
    ctx = ctx_of(512)
    s0, s1 = xof_ref.seed_of(1), xof_ref.seed_of(2)
    a = both(torch_mod, ctx, [s0, s1], 2, 1)
    b = both(torch_mod, ctx, [s0], 2, 2)
    assert not np.array_equal(a[0], b[0])           # same seed, two domains
    assert not np.array_equal(a[0], a[1])           # two seeds, one domain
    assert not np.array_equal(a[0, 0], a[0, 1])     # p = 0 against p = 1
    assert not np.array_equal(a[0, 0, :256], a[0, 0, 256:])   # c = 0 against c = 1
    assert np.array_equal(a, ref_uniform(512, 1, [s0, s1], 2)) and np.array_equal(b, ref_uniform(512, 2, [s0], 2))


def test_argument_rules_and_profile_name(torch_mod):
    torch = torch_mod
    ctx = ctx_of(512)
    L, h = ctx._L, ctx._h
    seeds = seed_array([xof_ref.seed_of(i) for i in range(3)])
    out = np.empty((3, 2, 512), dtype=np.int64)
    sp, op = C.c_void_p(seeds.ctypes.data), C.c_void_p(out.ctypes.data)
    dseeds = torch.zeros(3 * 32 + 8, dtype=torch.uint8, device="cuda")
    dout = torch.empty(3 * 2 * 512 + 2, dtype=torch.int64, device="cuda")
    dsp, dop = dseeds.data_ptr(), dout.data_ptr()
    assert dsp % 8 == 0 and dop % 16 == 0
    ctx._bind_torch_stream()
    for fn, s, o in ((L.rzk_xof_uniform_batch, sp, op), (L.rzk_xof_uniform_batch_dev, C.c_void_p(dsp), C.c_void_p(dop))):
        assert fn(h, s, 0, 2, o, 3) == -1          # domain 0 belongs to the keys
        assert fn(h, s, 1, 0, o, 3) == -1          # rows == 0
        assert fn(h, None, 1, 2, o, 3) == -1
        assert fn(h, s, 1, 2, None, 3) == -1
        assert fn(None, s, 1, 2, o, 3) == -1
        assert fn(h, None, 1, 2, None, 0) == 0     # B == 0: a no-op
        assert fn(h, s, 1, 2, o, 3) == 0
    assert L.rzk_xof_uniform_batch_dev(h, C.c_void_p(dsp + 4), 1, 2, C.c_void_p(dop), 3) == -1    # seeds not 8-byte aligned
    assert L.rzk_xof_uniform_batch_dev(h, C.c_void_p(dsp), 1, 2, C.c_void_p(dop + 8), 3) == -1    # out not 16-byte aligned
    assert L.rzk_xof_uniform_batch_dev(h, C.c_void_p(dsp + 8), 1, 2, C.c_void_p(dop + 16), 3) == 0
    ctx.synchronize()
    with pytest.raises(RzkError):
        ctx.xof_uniform(seeds, 2, 0)
    with pytest.raises(ValueError):
        ctx.xof_uniform(seeds[:, :31], 2, 1)
    with pytest.raises(ValueError):
        ctx.expand_key(bytes(31))
    assert ctx.xof_uniform(seeds[:0], 2, 1).shape == (0, 2, 512)
    # needs no loaded key; the launch is named in the profile
    ctx.prof_enable(True)
    ctx.prof_reset()
    ctx.xof_uniform(seeds, 2, 1)
    ctx.xof_uniform(dev(torch, seeds), 2, 1)
    ctx.synchronize()
    nbytes = 3 * 2 * 512 * 8
    assert ctx.prof_read_kernels() == [("xof_uniform_kernel", nbytes)] * 2
    ctx.prof_enable(False)


KEY_SEED = bytes(range(32))


@pytest.mark.parametrize("N", [64, 1024])
@pytest.mark.parametrize("nkl", [(1, 3, 1), (2, 5, 2), (1, 2, 1)])
def test_expand_key(torch_mod, N, nkl):
    """(1, 2, 1): a2' has no columns, so the last key row starts no launch."""
    n, k, l = nkl
    ctx = ctx_of(N, nkl=nkl)
    A = ctx.expand_key(KEY_SEED)
    assert A.shape == (n + l, k, N) and A.dtype == np.int64
    one = np.zeros(N, dtype=np.int64)
    one[0] = 1
    for i in range(n + l):
        first_general = n if i < n else n + l
        for j in range(k):
            if j >= first_general:
                assert np.array_equal(A[i, j], ref_poly(N, 0, KEY_SEED, i * k + j)), (i, j)
            else:
                assert np.array_equal(A[i, j], one if j == i else 0 * one), (i, j)
    assert np.array_equal(A, xof_ref.key(Q, N, n, k, l, KEY_SEED))
    digest = FS.key_digest(ctx)
    second = ctx_of(N, nkl=nkl)
    assert np.array_equal(second.expand_key(KEY_SEED), A) and FS.key_digest(second) == digest
    loaded = ctx_of(N, nkl=nkl)
    loaded.load_key(xof_ref.key(Q, N, n, k, l, KEY_SEED))
    assert FS.key_digest(loaded) == digest
    assert not np.array_equal(second.expand_key(bytes(32)), A) and FS.key_digest(second) != digest
    # the expanded key is the loaded key: a commitment under it equals one under the reference-built matrix
    rng = np.random.default_rng(N + k)
    x, r = synth.uniform(rng, (2, l, N)), synth.small(rng, (2, k, N), ctx.b)
    c1, ok1 = ctx.commit(x, r)
    c2, ok2 = loaded.commit(x, r)
    assert np.array_equal(c1, c2) and np.array_equal(ok1, ok2)


def test_linear_proof_from_seeds(torch_mod):
    """Key from a seed, g from per-proof seeds: the verifier who derives g from the same seeds accepts, one who derives
    it from other seeds rejects every proof."""
    N, B = 512, 3
    ctx = ctx_of(N)
    ctx.expand_key(KEY_SEED)
    P = P_of(ctx)
    seeds = seed_array([xof_ref.seed_of(500 + b) for b in range(B)])
    g = FS.multipliers(ctx, seeds)
    assert g.shape == (B, N) and np.array_equal(g, ref_uniform(N, 1, [bytes(s) for s in seeds], 1)[:, 0])
    gs = FS.multipliers(ctx, seeds, V=2)
    assert gs.shape == (B, 2, N) and np.array_equal(gs[:, 0], g)
    rng = np.random.default_rng(77)
    x = synth.uniform(rng, (B, 1, N))
    r, rp = synth.small(rng, (B, 3, N), P.b), synth.small(rng, (B, 3, N), P.b)
    y, yp = synth.gauss(rng, (B, 3, N), P.sigma), synth.gauss(rng, (B, 3, N), P.sigma)
    c, cp, t, tp, u, z, zp, ok = FS.linear_prove(ctx, g, x, r, rp, y, yp)
    assert ok.all()
    verifier = ctx_of(N)
    verifier.expand_key(KEY_SEED)
    assert FS.linear_verify(verifier, c, cp, FS.multipliers(verifier, seeds), t, tp, u, z, zp).all()
    other = FS.multipliers(verifier, seed_array([xof_ref.seed_of(600 + b) for b in range(B)]))
    assert not FS.linear_verify(verifier, c, cp, other, t, tp, u, z, zp).any()
    # the device path: seeds on the GPU give the same multipliers
    dg = FS.multipliers(ctx, dev(torch_mod, seeds))
    ctx.synchronize()
    assert np.array_equal(dg.cpu().numpy(), g)
