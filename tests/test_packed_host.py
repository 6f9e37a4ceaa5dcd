"""CPU tier of the packed proof format "RZKP1": ring_zk_amd/csrc/rzk_packed.h (schema, widths, record sizes, header, the
scalar put / get forms and the kernels' division by W), compiled with g++ under -fsanitize=address,undefined into
tests/packed/packed_driver.cpp and run as a process, against tests/packed_ref.py (one big integer per polynomial)."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import packed_ref as PR

HERE = os.path.dirname(os.path.abspath(__file__))
Q = 3515337053

# (q, verify_bound) -> (W_Q, W_Z); class D is always 2 bits: together W in {2, 8, 15, 18, 22, 23, 32}
WIDTH_CASES = [
    (Q, 100, 32, 8),
    (32749, 100, 15, 8),
    (Q, 10000, 32, 15),
    (Q, 100000, 32, 18),
    (Q, 1393920, 32, 22),     # N = 1024, (1,3,1), kappa = 36
    (Q, 3000000, 32, 23),
]
SIZES = [4, 32, 64, 128]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build the packed driver")
    exe = str(tmp_path_factory.mktemp("packed") / "packed_driver")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-o", exe,
                           os.path.join(HERE, "packed", "packed_driver.cpp")])
    return exe


def run_driver(exe, tmp_path, records):
    path = tmp_path / ("packed_cases_%d.bin" % os.getpid())
    with open(path, "wb") as f:
        f.write(b"".join(records))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    res = subprocess.run([exe, str(path)], capture_output=True, text=True, env=env)
    assert res.returncode == 0, res.stderr[-4000:]
    return [line.split() for line in res.stdout.splitlines()]


def head(op, ctx, kind, V):
    return struct.pack("<7IqQ", op, kind, ctx.N, ctx.n, ctx.k, ctx.l, V or 0, ctx.q, ctx.verify_bound)


def ctx_of(N, q, vb, nkl=(1, 3, 1)):
    return PR.Ctx(N, *nkl, q, vb)


def shapes_of(ctx, kind, V):
    return [(rows, ctx.N) for _, _, rows in PR.fields(ctx, kind, V)]


def drv_encode(exe, tmp_path, ctx, kind, slabs, V=None):
    B = slabs[0].shape[0]
    rec = head(2, ctx, kind, V) + struct.pack("<I", B) + b"".join(np.ascontiguousarray(s, np.int64).tobytes() for s in slabs)
    got = run_driver(exe, tmp_path, [rec])
    assert len(got) == B
    size = PR.record_bytes(ctx, kind, V)
    recs = np.frombuffer(bytes.fromhex("".join(g[1] for g in got)), dtype=np.uint8).reshape(B, size)
    return recs, np.array([int(g[0]) for g in got], dtype=np.uint8)


def drv_decode(exe, tmp_path, ctx, kind, records, V=None):
    B = records.shape[0]
    got = run_driver(exe, tmp_path, [head(3, ctx, kind, V) + struct.pack("<I", B) + records.tobytes()])
    assert len(got) == B
    shapes = shapes_of(ctx, kind, V)
    slabs = [np.zeros((B,) + sh, np.int64) for sh in shapes]
    for b, g in enumerate(got):
        flat = np.frombuffer(bytes.fromhex(g[1]), dtype=np.int64)
        pos = 0
        for s in slabs:
            n = s[b].size
            s[b] = flat[pos:pos + n].reshape(s[b].shape)
            pos += n
        assert pos == flat.size
    return slabs, np.array([int(g[0]) for g in got], dtype=np.uint8)


def random_fields(rng, ctx, kind, V, B):
    """Random in-range slabs with the extreme values of every class planted: -bias, limit - bias and 0."""
    cl = PR.classes(ctx)
    out = []
    for _, c, rows in PR.fields(ctx, kind, V):
        lo, hi = -cl[c].bias, cl[c].limit - cl[c].bias
        a = rng.integers(lo, hi + 1, (B, rows, ctx.N), dtype=np.int64)
        a[0, 0, 0], a[0, -1, -1], a[-1, 0, ctx.N // 2], a[-1, -1, 1] = lo, hi, 0, lo
        a[B // 2, rows // 2, ctx.N - 2] = hi
        out.append(a)
    return out


def test_division_by_the_width(driver, tmp_path):
    assert run_driver(driver, tmp_path, [struct.pack("<I", 4)]) == [["1"]]


def test_literal_sizes_and_widths(driver, tmp_path):
    """The sizes the format's description pins for Open N = 1024, (1,3,1), and W_Z at the three NTT sizes."""
    ctx = PR.make_ctx(1024, 1, 3, 1, Q)
    want = {PR.OPEN_COMMITMENT: 12296, PR.OPEN_RESPONSE: 8456, PR.OPEN_SHORT: 16904, PR.CHALLENGE: 264}
    got = run_driver(driver, tmp_path, [head(1, ctx, kind, 0) for kind in want])
    assert [int(g[1]) for g in got] == list(want.values())
    assert [PR.record_bytes(ctx, kind) for kind in want] == list(want.values())
    for N, wz in ((512, 21), (1024, 22), (2048, 23)):
        c = PR.make_ctx(N, 1, 3, 1, Q)
        g = run_driver(driver, tmp_path, [head(1, c, PR.OPEN_RESPONSE, 0)])[0]
        assert (int(g[2]), int(g[3]), int(g[4])) == (32, wz, 2)
        assert PR.classes(c)["Z"].W == wz


def test_record_sizes_and_bad_arguments(driver, tmp_path):
    cases = []
    for q, vb, wq, wz in WIDTH_CASES:
        for N in SIZES + [1024]:
            for nkl in ((1, 3, 1), (2, 5, 2)):
                ctx = ctx_of(N, q, vb, nkl)
                for kind in PR.KINDS:
                    for V in ((1, 3, 65535) if kind in PR.SUM_KINDS else (0,)):
                        cases.append((ctx, kind, V, wq, wz))
    got = run_driver(driver, tmp_path, [head(1, c, kind, V) for c, kind, V, _, _ in cases])
    for (ctx, kind, V, wq, wz), g in zip(cases, got):
        assert [int(v) for v in g] == [1, PR.record_bytes(ctx, kind, V or None), wq, wz, 2], (ctx, kind, V)
    ctx = ctx_of(64, Q, 100)
    bad = [(ctx, PR.OPENING, 0), (ctx, 10, 0), (ctx, 99, 0), (ctx, PR.SUM_COMMITMENT, 0), (ctx, PR.SUM_RESPONSE, 65536),
           (ctx_of(64, Q - 1, 100), PR.COMMITMENT, 0), (ctx_of(64, Q, (Q - 1) // 2 + 1), PR.COMMITMENT, 0),
           (ctx_of(64, Q, 0), PR.COMMITMENT, 0)]
    got = run_driver(driver, tmp_path, [head(1, c, kind, V) for c, kind, V in bad])
    assert [g[0] for g in got] == ["0"] * len(bad)


@pytest.mark.parametrize("q,vb,wq,wz", WIDTH_CASES)
@pytest.mark.parametrize("N", SIZES)
def test_every_kind_against_reference(driver, tmp_path, N, q, vb, wq, wz):
    ctx = ctx_of(N, q, vb)
    rng = np.random.default_rng(N * 1000 + wz + wq)
    for kind in PR.KINDS:
        V = 3 if kind in PR.SUM_KINDS else None
        B = 3
        slabs = random_fields(rng, ctx, kind, V, B)
        want, wok = PR.encode(ctx, kind, slabs, V)
        assert wok.tolist() == [1] * B
        got, gok = drv_encode(driver, tmp_path, ctx, kind, slabs, V)
        assert gok.tolist() == [1] * B and np.array_equal(got, want), kind
        back, bok = drv_decode(driver, tmp_path, ctx, kind, want, V)
        assert bok.tolist() == [1] * B
        ref_back, rok = PR.decode(ctx, kind, want, shapes_of(ctx, kind, V), V)
        assert rok.tolist() == [1] * B
        for a, b, c in zip(back, slabs, ref_back):
            assert np.array_equal(a, b) and np.array_equal(c, b), kind


@pytest.mark.parametrize("q,vb,wq,wz", WIDTH_CASES)
@pytest.mark.parametrize("N", SIZES)
def test_one_past_the_range_writes_the_marker(driver, tmp_path, N, q, vb, wq, wz):
    """bias + 1 on either side of every class: the all-ones marker in that coefficient's place, ok cleared for that
    message only, and the record does not decode."""
    ctx = ctx_of(N, q, vb)
    cl = PR.classes(ctx)
    rng = np.random.default_rng(N + wz)
    for kind in (PR.OPEN_SHORT, PR.LINEAR_COMMITMENT, PR.SUM_RESPONSE):
        V = 2 if kind in PR.SUM_KINDS else None
        fl = PR.fields(ctx, kind, V)
        B = 2 * len(fl) + 1
        slabs = random_fields(rng, ctx, kind, V, B)
        for f, (_, c, rows) in enumerate(fl):
            slabs[f][2 * f, rows - 1, N - 1] = cl[c].limit - cl[c].bias + 1
            slabs[f][2 * f + 1, 0, 0] = -cl[c].bias - 1
        want, wok = PR.encode(ctx, kind, slabs, V)
        assert wok.tolist() == [0] * (B - 1) + [1]
        got, gok = drv_encode(driver, tmp_path, ctx, kind, slabs, V)
        assert np.array_equal(gok, wok) and np.array_equal(got, want), kind
        _, dok = drv_decode(driver, tmp_path, ctx, kind, got, V)
        assert np.array_equal(dok, wok), kind
        # the marker is all-ones at the coefficient's own bits
        f, (_, c, rows) = 0, fl[0]
        big = int.from_bytes(got[0, 8 + (rows - 1) * PR.poly_bytes(N, cl[c].W):][:PR.poly_bytes(N, cl[c].W)].tobytes(), "little")
        assert (big >> ((N - 1) * cl[c].W)) & ((1 << cl[c].W) - 1) == (1 << cl[c].W) - 1


def test_non_canonical_64_bit_values_never_pack_as_their_low_bits(driver, tmp_path):
    ctx = ctx_of(64, Q, 1000)
    slabs = random_fields(np.random.default_rng(3), ctx, PR.OPEN_SHORT, None, 4)
    slabs[0][0, 0, 5], slabs[1][1, 0, 9], slabs[2][2, 1, 63] = (1 << 32) + 7, -(1 << 40), (1 << 63) - 1
    want, wok = PR.encode(ctx, PR.OPEN_SHORT, slabs)
    got, gok = drv_encode(driver, tmp_path, ctx, PR.OPEN_SHORT, slabs)
    assert gok.tolist() == [0, 0, 0, 1] and np.array_equal(gok, wok) and np.array_equal(got, want)


def set_coef(records, b, byte0, N, W, i, raw):
    """Overwrite coefficient i of the polynomial whose words start at byte0 of record b."""
    nb = PR.poly_bytes(N, W)
    big = int.from_bytes(records[b, byte0:byte0 + nb].tobytes(), "little")
    big = (big & ~(((1 << W) - 1) << (i * W))) | (raw << (i * W))
    records[b, byte0:byte0 + nb] = np.frombuffer(big.to_bytes(nb, "little"), dtype=np.uint8)


@pytest.mark.parametrize("N", [4, 64])
def test_decode_rejections(driver, tmp_path, N):
    """limit + 1 and all-ones in every class, each header byte, one padding bit: each rejects exactly its own record,
    and the reference agrees."""
    ctx = ctx_of(N, Q, 100)   # W_Z = 8: N = 4 leaves 32 padding bits in z, 56 in d
    cl = PR.classes(ctx)
    kind = PR.OPEN_SHORT
    fl = PR.fields(ctx, kind)
    base, _ = PR.encode(ctx, kind, random_fields(np.random.default_rng(N), ctx, kind, None, 1))
    starts, pos = [], 8
    for _, c, rows in fl:
        starts.append(pos)
        pos += rows * PR.poly_bytes(N, cl[c].W)
    mods = []
    for f, (_, c, rows) in enumerate(fl):
        for raw in (cl[c].limit + 1, (1 << cl[c].W) - 1):
            r = base.copy()
            set_coef(r, 0, starts[f] + (rows - 1) * PR.poly_bytes(N, cl[c].W), N, cl[c].W, N - 1, raw)
            mods.append(r)
    for byte in range(8):
        r = base.copy()
        r[0, byte] ^= 1
        mods.append(r)
    if N == 4:
        for f, bit in ((1, 8), (1, 63), (2, 32), (2, 63)):   # d: bits 8 .. 63 are padding; z (W = 8): bits 32 .. 63
            r = base.copy()
            r[0, starts[f] + bit // 8] |= 1 << (bit % 8)
            mods.append(r)
    recs = np.concatenate([base] + mods + [base])
    _, ok = drv_decode(driver, tmp_path, ctx, kind, recs)
    _, rok = PR.decode(ctx, kind, recs, shapes_of(ctx, kind, None))
    assert ok.tolist() == [1] + [0] * len(mods) + [1] and np.array_equal(ok, rok)
