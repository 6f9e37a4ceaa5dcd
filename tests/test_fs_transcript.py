"""CPU tier of the Fiat-Shamir transcript: ring_zk_amd/csrc/rzk_keccak.h (Keccak-f[1600], the SHAKE256 sponge, the
FS1 leaf / key / root streams and the challenge sampler), compiled with g++ under -fsanitize=address,undefined into
tests/fs/fs_driver.cpp, against tests/fs_ref.py (hashlib).  Three digests are pinned as hex literals so that the
format cannot drift in both restatements at once."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import fs_ref

HERE = os.path.dirname(os.path.abspath(__file__))
Q = 3515337053
HALF = (Q - 1) // 2
KINDS = (fs_ref.OPEN_COMMITMENT, fs_ref.LINEAR_COMMITMENT, fs_ref.SUM_COMMITMENT)


def message_polys(kind, n, l, V):
    """Polynomials per message: the fields of the RZK_MSG_* table in declaration order (include/rzk.h)."""
    return {fs_ref.OPEN_COMMITMENT: (n + l) + n,
            fs_ref.LINEAR_COMMITMENT: 2 * (n + l) + 1 + 2 * n + l,
            fs_ref.SUM_COMMITMENT: (n + l) + V * (n + l) + V + n + V * n + l}[kind]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build the transcript driver")
    exe = str(tmp_path_factory.mktemp("fs") / "fs_driver")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Werror", "-o", exe,
                           os.path.join(HERE, "fs", "fs_driver.cpp")])
    return exe


def run_driver(exe, tmp_path, records):
    path = tmp_path / ("fs_cases_%d.bin" % os.getpid())
    with open(path, "wb") as f:
        f.write(b"".join(records))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    res = subprocess.run([exe, str(path)], capture_output=True, text=True, env=env)
    assert res.returncode == 0, res.stderr[-4000:]
    return [line.split() for line in res.stdout.splitlines()]


def shake_record(msg, outlen):
    return struct.pack("<III", 1, len(msg), outlen) + msg


def fs_record(kind, V, N, n, k, l, kappa, q, b, aux, key, polys):
    return (struct.pack("<9I", 2, kind, V, N, n, k, l, kappa, polys.shape[0]) + struct.pack("<qQ", q, b) + aux
            + np.ascontiguousarray(key, dtype="<i8").tobytes() + np.ascontiguousarray(polys, dtype="<i8").tobytes())


def test_shake256_against_hashlib(driver, tmp_path):
    rng = np.random.default_rng(1)
    cases = [(rng.integers(0, 256, ln, dtype=np.uint8).tobytes(), out)
             for ln in (0, 1, 135, 136, 137, 271, 272, 1040) for out in (32, 300)]
    got = run_driver(driver, tmp_path, [shake_record(m, o) for m, o in cases])
    assert [g[0] for g in got] == ["shake"] * len(cases)
    assert [g[1] for g in got] == [fs_ref.shake256(m, o).hex() for m, o in cases]


def random_case(rng, kind, N, n, k, l, V, kappa):
    key = rng.integers(-HALF, HALF + 1, ((n + l) * k, N), dtype=np.int64)
    polys = rng.integers(-HALF, HALF + 1, (message_polys(kind, n, l, V), N), dtype=np.int64)
    polys[0, 0], polys[-1, -1] = HALF, -HALF   # both ends of the centred range (int32 sign bit set / clear)
    aux = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
    return key, polys, aux


@pytest.mark.parametrize("N", [4, 64, 256, 512])
@pytest.mark.parametrize("kind", KINDS)
def test_leaf_root_sampler_against_reference(driver, tmp_path, kind, N):
    rng = np.random.default_rng(100 * kind + N)
    recs, want = [], []
    for (n, k, l), V, kappa in (((1, 3, 1), 2, min(N, 36)), ((2, 5, 2), 3, 1), ((1, 3, 1), 1, N if N <= 64 else 60)):
        Vh = V if kind == fs_ref.SUM_COMMITMENT else 0
        key, polys, aux = random_case(rng, kind, N, n, k, l, V, kappa)
        recs.append(fs_record(kind, Vh, N, n, k, l, kappa, Q, 1, aux, key, polys))
        kd = fs_ref.key_digest(key, Q, N, n, k, l, kappa, 1)
        d, dig = fs_ref.challenge_one(kind, Vh, kd, aux, [polys], N, kappa)
        assert int(np.abs(d).sum()) == kappa and set(np.unique(d)) <= {-1, 0, 1}
        want.append(["fs", kd.hex(), fs_ref.leaves(polys, N).hex(), dig.hex()] + [str(v) for v in d])
    assert run_driver(driver, tmp_path, recs) == want


# produced once from tests/fs_ref.py; a change of either restatement that alters the format fails here
PINNED = {
    "leaf": "686fe805fe05e1b00ed7cff021b0609ccd9c85684b1c2e24d7c31bab995bd8fb",
    "key": "7f344f7521fe0bffddb357018c7b9f413fcf82b2dfb3e85b7e0ceb24f74a8153",
    "root": "2aa06fa500688d4d7fc4ecf968d0771ef45e1034b4ca249f19f4d41d86de7014",
}


def pinned_inputs():
    N, n, k, l, kappa = 16, 1, 3, 1, 8
    key = (np.arange((n + l) * k * N, dtype=np.int64).reshape((n + l) * k, N) * 7919) % 2001 - 1000
    polys = (np.arange(3 * N, dtype=np.int64).reshape(3, N) * 104729) % 20001 - 10000
    return N, n, k, l, kappa, key, polys


def test_pinned_digests(driver, tmp_path):
    N, n, k, l, kappa, key, polys = pinned_inputs()
    aux = bytes(range(32))
    kd = fs_ref.key_digest(key, Q, N, n, k, l, kappa, 1)
    d, dig = fs_ref.challenge_one(fs_ref.OPEN_COMMITMENT, 0, kd, aux, [polys], N, kappa)
    assert fs_ref.leaves(polys[:1], N).hex() == PINNED["leaf"]
    assert kd.hex() == PINNED["key"]
    assert dig.hex() == PINNED["root"]
    got = run_driver(driver, tmp_path, [fs_record(fs_ref.OPEN_COMMITMENT, 0, N, n, k, l, kappa, Q, 1, aux, key, polys)])
    assert got[0][1] == PINNED["key"] and got[0][2][:64] == PINNED["leaf"] and got[0][3] == PINNED["root"]
    assert [int(v) for v in got[0][4:]] == d.tolist()


SAMPLER_PAIRS = ((1024, 36), (4, 4), (16, 8), (2048, 36), (512, 36), (64, 64), (2048, 2048))


def word_budget(kappa):
    """Words that kappa draws need with probability >= 1 - 2^-40: every word is accepted with probability >= 1/2
    (j = w & mask <= i, mask < 2 (i + 1)), so P(more than m words) <= P(Bin(m, 1/2) < kappa) <= exp(-(m - 2 kappa)^2 /
    (2 m)) by Hoeffding, which is 2^-40 at m = 2 kappa + x with x^2 = 56 m, i.e. x = 28 + sqrt(784 + 112 kappa)."""
    return int(2 * kappa + 28 + (784 + 112 * kappa) ** 0.5) + 1


@pytest.mark.parametrize("N,kappa", SAMPLER_PAIRS)
def test_sampler_weight_and_word_budget(driver, tmp_path, N, kappa):
    """200 streams per (N, kappa): the reference sampler gives exactly kappa coefficients +-1 from no more words than
    its acceptance probability allows, and the library's sampler (record 3 of the driver) gives the same challenge
    from the same SHAKE256 stream."""
    seeds = [struct.pack("<III", N, kappa, t) for t in range(200)]
    want = []
    for seed in seeds:
        d, words = fs_ref.sample(fs_ref.shake256(seed, 32 + 2 * word_budget(kappa)), N, kappa)
        assert int(np.abs(d).sum()) == kappa and set(np.unique(d)) <= {-1, 0, 1}
        assert words <= word_budget(kappa)
        want.append(["sample"] + [str(v) for v in d])
    recs = [struct.pack("<IIII", 3, N, kappa, len(seed)) + seed for seed in seeds]
    assert run_driver(driver, tmp_path, recs) == want
