"""CPU tier of the rejection-sampling step: ring_zk_amd/csrc/rzk_reject.h (the per-coefficient step, the lnM helper,
the argument rule and the decision), compiled with g++ under -fsanitize=address,undefined into
tests/reject/reject_driver.cpp, against tests/reject_ref.py (Python integers, 50-digit decimal threshold).  E and the
flags are compared exactly, the decision on every decidable case (reject_ref: |E - T| > 2 sigma^2 2^-44)."""
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import reject_ref as RR

HERE = os.path.dirname(os.path.abspath(__file__))
Q = 3515337053
R62 = 1 << 62


def params(N, k=3, kappa=36, b=1, q=Q):
    """Params::standard_deviation and check_verify_constraint's bound (params.rs:94-98, 114), floor square roots."""
    sigma = 11 * kappa * b * math.isqrt(k * N)
    return RR.Params(q, N, sigma, kappa * b, 2 * sigma * math.isqrt(N))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build the reject driver")
    exe = str(tmp_path_factory.mktemp("reject") / "reject_driver")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-o", exe,
                           os.path.join(HERE, "reject", "reject_driver.cpp")])
    return exe


def run_driver(exe, tmp_path, records):
    path = tmp_path / ("reject_cases_%d.bin" % os.getpid())
    with open(path, "wb") as f:
        f.write(b"".join(records))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    res = subprocess.run([exe, str(path)], capture_output=True, text=True, env=env)
    assert res.returncode == 0, res.stderr[-4000:]
    return [line.split() for line in res.stdout.splitlines()]


def case_record(P, z, y, coin, R, lnM, trusted=False):
    B, rows = z.shape[0], z.shape[1]
    head = struct.pack("<I4qdQ4I", 1, P.q, P.vmax, P.verify_bound, P.sigma, lnM, R, P.N, rows, B, int(trusted))
    return head + np.ascontiguousarray(z, np.int64).tobytes() + np.ascontiguousarray(y, np.int64).tobytes() + \
        np.ascontiguousarray(coin, np.int64).tobytes()


def check(exe, tmp_path, P, z, y, coin, R, lnM, trusted=False, max_undecidable=2):
    """Driver against the reference on one batch; returns the reference's results."""
    want = RR.run(P, [(z, y)], coin, R, lnM, trusted=trusted)
    assert RR.count_undecidable(want) <= max_undecidable   # from the reference alone
    got = run_driver(exe, tmp_path, [case_record(P, z, y, coin, R, lnM, trusted)])
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        if w[1] & RR.NONCANON:                    # E (and with it which other rules fire) is unspecified for non-canonical input
            assert int(g[1]) & RR.NONCANON, b
        else:
            assert (int(g[0]), int(g[1])) == (w[0], w[1]), b
        if w[3]:
            assert int(g[2]) == int(w[2]), b
    return want


def test_lnm_helper(driver, tmp_path):
    got = run_driver(driver, tmp_path, [struct.pack("<Id", 2, a) for a in (11.0, 11.0 / math.sqrt(2.0), 1.0)])
    assert float.fromhex(got[0][1]) == 12 / 11 + 1 / 242
    a = 11.0 / math.sqrt(2.0)
    assert float.fromhex(got[1][1]) == 12.0 / a + 1.0 / (2.0 * a * a)
    assert float.fromhex(got[2][1]) == 12.5
    assert abs(math.exp(float.fromhex(got[0][1])) - 2.99) < 0.01     # M of the Open proof


def test_argument_rule(driver, tmp_path):
    """rows N 2^24 vmax < 2^52, at the edge; verify_bound below 2^24."""
    cases = [(3, 1024, 36, 1393920, 1), (1 << 8, 1 << 10, 1 << 10, 100, 0), (1 << 8, 1 << 10, (1 << 10) - 1, 100, 1),
             ((1 << 18) - 1, 1 << 10, 1, 100, 1), (1 << 18, 1 << 10, 1, 100, 0), (3, 1024, 36, (1 << 24) - 1, 1),
             (3, 1024, 36, 1 << 24, 0), (0, 1024, 36, 100, 0), (3, 1024, 0, 100, 1)]
    got = run_driver(driver, tmp_path, [struct.pack("<IQIQQ", 3, r, N, v, vb) for r, N, v, vb, _ in cases])
    assert [int(g[1]) for g in got] == [c[4] for c in cases]
    for r, N, v, vb, ok in cases:
        assert ok == int(r > 0 and r * N * (1 << 24) * v < 1 << 52 and vb < 1 << 24)


@pytest.mark.parametrize("N,rows,B", [(4, 1, 7), (64, 3, 5), (64, 130, 2), (1024, 3, 4), (2048, 6, 2)])
def test_random_honest_data(driver, tmp_path, N, rows, B):
    P = params(N, kappa=min(N, 36))
    rng = np.random.default_rng(100 * N + rows)
    z, y = RR.honest(rng, P, B, rows)
    lnM = 12 / 11 + 1 / 242
    want = check(driver, tmp_path, P, z, y, RR.coins(rng, B, R62), R62, lnM)
    assert all(w[1] == 0 for w in want)
    check(driver, tmp_path, P, z, y, RR.coins(rng, B, 1000), 1000, lnM, trusted=True)


def test_wrap_around_folds(driver, tmp_path):
    """z - y near +-q: z and y at opposite ends of the range, v small after one conditional add / subtract."""
    P = params(64)
    rng = np.random.default_rng(7)
    B, rows = 4, 2
    v = rng.integers(-P.vmax, P.vmax + 1, (B, rows, P.N), dtype=np.int64)
    y = np.where(v >= 0, P.half - rng.integers(0, 5, v.shape), -P.half + rng.integers(0, 5, v.shape)).astype(np.int64)
    z = y + v
    z = np.where(z > P.half, z - P.q, np.where(z < -P.half, z + P.q, z))
    assert (np.abs(z - y) > P.q - 100).any() and (np.abs(z) <= P.half).all()
    want = check(driver, tmp_path, P, z, y, RR.coins(rng, B, R62), R62, 1.0)
    # |z| is near (q-1)/2: the norm rule fires, nothing else, and E is still the exact integer
    assert all(w[1] == RR.NORM for w in want)


def test_vmax_edge(driver, tmp_path):
    P = params(64)
    rng = np.random.default_rng(8)
    z, y = RR.honest(rng, P, 4, 3)
    for b, (j, i, dv) in enumerate([(0, 0, P.vmax), (2, 63, -P.vmax), (1, 5, P.vmax + 1), (2, 0, -P.vmax - 1)]):
        z[b, j, i] = y[b, j, i] + dv
    want = check(driver, tmp_path, P, z, y, RR.coins(rng, 4, R62), R62, 1.0)
    assert [w[1] for w in want] == [0, 0, RR.VMAX, RR.VMAX]


def test_norm_edge(driver, tmp_path):
    P = params(64)
    rng = np.random.default_rng(9)
    z, y = RR.honest(rng, P, 3, 3)
    z[0, 1], z[1, 2] = RR.norm_edge_poly(P, 0), RR.norm_edge_poly(P, 1)
    y[0, 1], y[1, 2] = z[0, 1] - 1, z[1, 2] + 1
    want = check(driver, tmp_path, P, z, y, RR.coins(rng, 3, R62), R62, 1.0)
    assert [w[1] for w in want] == [0, RR.NORM, 0]


def test_non_canonical(driver, tmp_path):
    P = params(64)
    rng = np.random.default_rng(10)
    z, y = RR.honest(rng, P, 6, 2)
    z[1, 0, 0], y[2, 1, 63], z[3, 1, 1], y[4, 0, 7] = P.half + 1, -P.half - 1, (1 << 32) + 5, -(1 << 40)
    z[5, 0, 0], y[5, 0, 0] = P.half, P.half - 1                      # the ends of the range are canonical
    want = check(driver, tmp_path, P, z, y, RR.coins(rng, 6, R62), R62, 1.0)
    assert [bool(w[1] & RR.NONCANON) for w in want] == [False, True, True, True, True, False]
    assert not any(w[2] for w in want[1:5])


def test_coin_range(driver, tmp_path):
    P = params(64)
    rng = np.random.default_rng(11)
    z1, y1 = RR.honest(rng, P, 1, 3)
    for R in (2, 1000, R62):
        coin = np.array([0, R - 1, R, -1, R + 1], np.int64)
        z, y = np.repeat(z1, 5, 0), np.repeat(y1, 5, 0)
        want = check(driver, tmp_path, P, z, y, coin, R, 12 / 11 + 1 / 242)
        assert [w[1] for w in want] == [0, 0, RR.COIN, RR.COIN, RR.COIN]
        # coin R - 1 (u = 1) needs E >= 2 sigma^2 lnM; coin 0 (u = 1 / R) is accepted once ln R exceeds lnM - E / 2 sigma^2
        assert not want[1][2] and want[0][2] == (R > 2)


@pytest.mark.parametrize("N,R", [(64, R62), (1024, R62), (64, (1 << 31) - 1)])
def test_threshold_flip(driver, tmp_path, N, R):
    """For fixed (z, y) the reference computes the largest accepted coin c*; c* - delta accepts and c* + delta rejects,
    delta = ceil(R 2^-40): a relative step of 2^-40 in u, i.e. 2 sigma^2 2^-40 in T, sixteen times the margin."""
    P = params(N)
    lnM = 12 / 11 + 1 / 242
    z, y = RR.honest(np.random.default_rng(12 + N), P, 1, 3)
    E, flags = RR.proof_stats(P, [(zz, yy) for zz, yy in zip(z[0].tolist(), y[0].tolist())])
    assert flags == 0
    c = RR.largest_accepted_coin(P, E, lnM, R)
    delta = -(-R // (1 << 40))
    assert 0 <= c - delta and c + delta < R
    coin = np.array([c - delta, c + delta], np.int64)
    want = check(driver, tmp_path, P, np.repeat(z, 2, 0), np.repeat(y, 2, 0), coin, R, lnM, max_undecidable=0)
    assert [w[2] for w in want] == [True, False]
