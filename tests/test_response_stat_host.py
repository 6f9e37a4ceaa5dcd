"""CPU tier of the fused response rows: reject_step_v (ring_zk_amd/csrc/rzk_reject.h), the per-coefficient
step that takes the centred product sum v the kernel holds, against reject_step, which derives v from z - y, and against
Python integers.  Compiled with g++ under -fsanitize=address,undefined into tests/reject/response_stat_driver.cpp, a
stand-alone program; nothing is loaded into Python.  Wherever y is canonical the two steps must leave identical s1, s2,
zsq and flags; for a non-canonical y only the flag is defined."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import reject_ref as RR

HERE = os.path.dirname(os.path.abspath(__file__))
Q = 3515337053
HALF = (Q - 1) // 2
VMAX = 36
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build the response-stat driver")
    exe = str(tmp_path_factory.mktemp("response_stat") / "response_stat_driver")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-o", exe,
                           os.path.join(HERE, "reject", "response_stat_driver.cpp")])
    return exe


def centred(a):
    return np.array([RR.centred(int(c), Q) for c in a], np.int64)


def run(exe, tmp_path, y, v, check=True, vmax=VMAX):
    """y, v: int64 arrays (v the centred product sum); z = centred(y + v).  Returns (per-coefficient rows, total row) of
    eight integers each: s1, s2, zsq, flags of reject_step, then of reject_step_v."""
    y, v = np.asarray(y, np.int64), np.asarray(v, np.int64)
    z = centred(y.astype(object) + v.astype(object))
    path = tmp_path / ("response_stat_%d.bin" % os.getpid())
    with open(path, "wb") as f:
        f.write(struct.pack("<I2q2I", 1, Q, vmax, len(y), int(check)) + z.tobytes() + v.tobytes() + y.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    res = subprocess.run([exe, str(path)], capture_output=True, text=True, env=env)
    assert res.returncode == 0, res.stderr[-4000:]
    lines = [line.split() for line in res.stdout.splitlines()]
    assert len(lines) == len(y) + 1 and lines[-1][0] == "total"
    return z, [[int(t) for t in line] for line in lines[:-1]], [int(t) for t in lines[-1][1:]]


def expect(z, v, vmax=VMAX):
    """(s1, s2, zsq, flags) of canonical coefficients in Python integers, sums mod 2^64"""
    s1 = sum(int(a) * int(b) for a, b in zip(z, v)) & M64
    s2 = sum(int(b) * int(b) for b in v) & M64
    zsq = sum(min(abs(int(a)), 1 << 24) ** 2 for a in z) & M64
    return [s1, s2, zsq, RR.VMAX if any(abs(int(b)) > vmax for b in v) else 0]


def same_and_right(z, v, rows, total, vmax=VMAX):
    for i, row in enumerate(rows):
        assert row[:4] == row[4:], (i, row)
        assert row[:4] == expect(z[i:i + 1], v[i:i + 1], vmax), (i, row)
    assert total[:4] == total[4:] == expect(z, v, vmax)


@pytest.mark.parametrize("check", [True, False])
def test_random_honest_triples(driver, tmp_path, check):
    rng = np.random.default_rng(1700 + check)
    n = 4096
    sigma = 11 * 36 * 55     # sigma of (1,3,1) at N = 1024
    y = np.rint(rng.normal(0.0, sigma, n)).astype(np.int64)
    v = rng.integers(-VMAX, VMAX + 1, n, dtype=np.int64)
    z, rows, total = run(driver, tmp_path, y, v, check)
    assert all(r[3] == 0 for r in rows)
    same_and_right(z, v, rows, total)


def test_wrap_in_z(driver, tmp_path):
    """y = +-(q-1)/2 with v of either sign: z = y + v wraps where they point the same way."""
    y = np.array([HALF, HALF, -HALF, -HALF, HALF - 3, -HALF + 3, HALF, -HALF], np.int64)
    v = np.array([5, -5, 5, -5, 36, -36, 0, 0], np.int64)
    z, rows, total = run(driver, tmp_path, y, v)
    assert z[0] == -HALF + 4 and z[3] == HALF - 4 and z[1] == HALF - 5 and z[2] == -HALF + 5   # the wrap is in the data
    assert all(r[3] == 0 for r in rows)
    same_and_right(z, v, rows, total)


def test_vmax_edge(driver, tmp_path):
    y = np.array([100, -100, 7, -7, 0, 0], np.int64)
    v = np.array([VMAX, -VMAX, VMAX + 1, -VMAX - 1, VMAX - 1, 1000], np.int64)
    z, rows, total = run(driver, tmp_path, y, v)
    assert [r[3] for r in rows] == [0, 0, RR.VMAX, RR.VMAX, 0, RR.VMAX]
    same_and_right(z, v, rows, total)


def test_clamp_of_z(driver, tmp_path):
    """|z| at 2^24 - 1, 2^24 and above: the square is clamped at 2^48."""
    t = 1 << 24
    zs = [t - 1, t, t + 1, -(t - 1), -t, -(t + 1), HALF, -HALF, 1 << 30]
    v = np.array([3, -3, 1, 2, -2, 36, -36, 0, 5], np.int64)
    y = centred(np.array(zs, object) - v.astype(object))
    z, rows, total = run(driver, tmp_path, y, v)
    assert z.tolist() == zs
    assert [r[2] for r in rows] == [(t - 1) ** 2, t * t, t * t, (t - 1) ** 2, t * t, t * t, t * t, t * t, t * t]
    same_and_right(z, v, rows, total)


def test_wide_products_wrap_alike(driver, tmp_path):
    """v far above vmax (a non-challenge multiplier): flagged, and s1, s2 are still the same sums mod 2^64."""
    rng = np.random.default_rng(1711)
    n = 512
    y = rng.integers(-HALF, HALF + 1, n, dtype=np.int64)
    v = rng.integers(-HALF, HALF + 1, n, dtype=np.int64)
    z, rows, total = run(driver, tmp_path, y, v)
    assert total[3] == RR.VMAX
    same_and_right(z, v, rows, total)


def test_non_canonical_y_flag_only(driver, tmp_path):
    """A y outside the centred range: both steps raise kRejNonCanon (the sums are unspecified); without the test
    (trusted producer) neither does."""
    y = np.array([HALF + 1, -HALF - 1, (1 << 32) + 5, -(1 << 40), HALF, -HALF], np.int64)
    v = np.array([1, -1, 2, -2, 0, 0], np.int64)
    _, rows, total = run(driver, tmp_path, y, v, check=True)
    assert [bool(r[3] & RR.NONCANON) for r in rows] == [True, True, True, True, False, False]
    assert [bool(r[7] & RR.NONCANON) for r in rows] == [True, True, True, True, False, False]
    assert total[3] & RR.NONCANON and total[7] & RR.NONCANON
    _, rows, _ = run(driver, tmp_path, y[4:], v[4:], check=False)
    assert all(r[3] == 0 and r[7] == 0 for r in rows)
