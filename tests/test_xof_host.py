"""CPU tier of the XP1 seed expansion: the scalar form of ring_zk_amd/csrc/rzk_xof.h, compiled with g++
under -fsanitize=address,undefined into tests/xof/xof_driver.cpp and run as a process, against tests/xof_ref.py
(hashlib).  Three polynomials are pinned as SHA-256 literals so that the format cannot drift in both restatements at
once; the seeds of the edge conditions found here are the ones tests/test_gpu_xof.py places in one wavefront."""
import os
import shutil
import struct
import subprocess

import pytest

import xof_ref

HERE = os.path.dirname(os.path.abspath(__file__))
Q = 3515337053
SEED = bytes(range(32))

# (q, N, domain, p, first coefficients, SHA-256 of the coefficients as little-endian int64); seed = bytes 0x00 .. 0x1f
PINNED = (
    (Q, 4, 0, 0, [1515073418, -1093657056, -1471467796, 45713935],
     "ec8a6f289e1ad0590821b4b78eb9444add16cc92e0dfbc1643a3b6d6be3bede5"),
    (Q, 1024, 1, 5, [-1348283605, 177552371], "c93e43fd3799a92453c54aff43304152fa0cb2ca1a840f7ab18943ad7b41b792"),
    (257, 64, 1, 0, [-61, -70, -88, -82], "f50d591d39be948cb7d6727973bc7e0e0288ce3d4945707425178bde9e8e3a25"),
)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build the XP1 driver")
    exe = str(tmp_path_factory.mktemp("xof") / "xof_driver")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Werror", "-o", exe,
                           os.path.join(HERE, "xof", "xof_driver.cpp")])
    return exe


def run_driver(exe, tmp_path, records):
    path = tmp_path / ("xof_cases_%d.bin" % os.getpid())
    with open(path, "wb") as f:
        f.write(b"".join(records))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    res = subprocess.run([exe, str(path)], capture_output=True, text=True, env=env)
    assert res.returncode == 0, res.stderr[-4000:]
    return [line.split() for line in res.stdout.splitlines()]


def chunk_record(q, N, domain, p, c, seed):
    return struct.pack("<IQIIII", 1, q, N, domain, p, c) + seed


def poly_record(q, N, domain, p, seed):
    return struct.pack("<IQIII", 2, q, N, domain, p) + seed


def want_chunk(q, N, domain, p, c, seed):
    vals, words = xof_ref.chunk(q, N, domain, seed, p, c)
    return ["chunk", str(words)] + [str(v) for v in vals]


def test_pinned_polynomials(driver, tmp_path):
    for q, N, domain, p, first, digest in PINNED:
        ref = xof_ref.poly(q, N, domain, SEED, p)
        assert ref[:len(first)].tolist() == first
        assert xof_ref.sha256_of(ref) == digest
    got = run_driver(driver, tmp_path, [poly_record(q, N, domain, p, SEED) for q, N, domain, p, _, _ in PINNED])
    for g, (q, N, domain, p, first, digest) in zip(got, PINNED):
        assert g[0] == "poly" and len(g) == 1 + N
        coefs = [int(v) for v in g[1:]]
        assert coefs[:len(first)] == first
        assert xof_ref.sha256_of(coefs) == digest


@pytest.mark.parametrize("q", [Q, 257])
@pytest.mark.parametrize("N", [4, 64, 256, 512])
def test_chunks_against_reference(driver, tmp_path, q, N):
    """Every chunk of a few polynomials, bit for bit and with the same number of stream words.  q = 257 has W = 9 and an
    acceptance rate of 0.502, the worst a modulus can have."""
    cases = [(domain, p, c, xof_ref.seed_of(100 * N + t))
             for t, (domain, p) in enumerate(((0, 0), (1, 0), (1, 3), (0xfffffffe, 0x01020304)))
             for c in range(N // xof_ref.chunk_len(N))]
    got = run_driver(driver, tmp_path, [chunk_record(q, N, d, p, c, s) for d, p, c, s in cases])
    assert got == [want_chunk(q, N, d, p, c, s) for d, p, c, s in cases]


def edge_seeds():
    """Smallest i, seed = sha256(le32(i)), domain 1, p = 0, c = 0, q = Q, for every place a chunk can end; found by the
    reference.  name -> (N, i, words used)."""
    found = {}
    for i in range(64):
        words = xof_ref.chunk(Q, 4, 1, xof_ref.seed_of(i), 0, 0)[1]
        found.setdefault("n4_no_rejection" if words == 4 else "n4_rejection", (4, i, words))
    used = [xof_ref.chunk(Q, 256, 1, xof_ref.seed_of(i), 0, 0)[1] for i in range(2000)]
    for i, words in enumerate(used):
        if words % xof_ref.RATE_WORDS32 == 0:
            found.setdefault("block_end", (256, i, words))
        found.setdefault("low_half" if words % 2 == 1 else "high_half", (256, i, words))
    most = max(used)
    found["most_words"] = (256, used.index(most), most)
    return found


EDGE_NAMES = ("n4_no_rejection", "n4_rejection", "block_end", "low_half", "high_half", "most_words")


def test_edge_seeds_found_and_reproduced(driver, tmp_path):
    edges = edge_seeds()
    assert sorted(edges) == sorted(EDGE_NAMES)
    assert edges["n4_no_rejection"] == (4, 0, 4)
    assert edges["n4_rejection"][2] > 4
    assert edges["block_end"] == (256, 4, 306)
    assert edges["low_half"][2] % 2 == 1 and edges["high_half"][2] % 2 == 0
    assert edges["most_words"][2] == 346   # 11 blocks: ceil(346 / 34)
    cases = [edges[name] for name in EDGE_NAMES]
    got = run_driver(driver, tmp_path, [chunk_record(Q, N, 1, 0, 0, xof_ref.seed_of(i)) for N, i, _ in cases])
    assert got == [want_chunk(Q, N, 1, 0, 0, xof_ref.seed_of(i)) for N, i, _ in cases]
    assert [int(g[1]) for g in got] == [w for _, _, w in cases]
