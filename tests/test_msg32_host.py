"""CPU tier of the 32-bit message calls: the host forms of what the new kernels compute, compiled
with g++ under -fsanitize=address,undefined into tests/msg32/msg32_driver.cpp and run as a process.

  * the leaf hash of rzk_keccak.h on int32 coefficients gives the digest of the int64 form and of tests/fs_ref.py;
  * the 32-bit raw rule of the packed codec (packed_raw32, rzk_packed.h) equals the 64-bit rule and Python integers for
    every class, the default, smallest and largest modulus, the values at and next to every edge, and a seeded sweep.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import fs_ref

HERE = os.path.dirname(os.path.abspath(__file__))
Q_DEFAULT = 3515337053
Q_MAX = 4294606851      # the largest modulus rzk_ctx_create takes
Q_MIN = 3               # ... and the smallest
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
PK_Q, PK_Z, PK_D = 0, 1, 2


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build the msg32 driver")
    exe = str(tmp_path_factory.mktemp("msg32") / "msg32_driver")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-o", exe,
                           os.path.join(HERE, "msg32", "msg32_driver.cpp")])
    return exe


def run_driver(exe, tmp_path, mode, lines):
    path = tmp_path / ("msg32_%s.txt" % mode)
    path.write_text("".join(line + "\n" for line in lines))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    res = subprocess.run([exe, mode, str(path)], capture_output=True, text=True, env=env)
    assert res.returncode == 0, (res.returncode, res.stderr[-4000:])
    out = [line.split() for line in res.stdout.splitlines()]
    assert len(out) == len(lines)
    return out


# ---- the leaf hash ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [4, 64, 256, 512, 1024])
def test_leaf_digest_is_the_same_at_both_widths(driver, tmp_path, N):
    """Every leaf of three polynomials: random canonical values, one holding +-h and the int32 extremes (the hash takes any
    int32; the range test is the kernel's), one alternating sign."""
    rng = np.random.default_rng(61000 + N)
    half = (Q_DEFAULT - 1) // 2
    polys = rng.integers(-half, half + 1, size=(3, N), dtype=np.int64)
    polys[1, :4] = [half, -half, I32_MAX, I32_MIN]
    polys[1, N - 1] = -1
    polys[2] = np.where(np.arange(N) % 2 == 0, half, -half)
    L = fs_ref.leaf_len(N)
    cases, want = [], []
    for p in range(3):
        ref = fs_ref.leaves(polys[p:p + 1], N, first=7 + p)
        for c in range(N // L):
            cases.append("%d %d %d %s" % (N, 7 + p, c, " ".join(str(int(v)) for v in polys[p])))
            want.append(ref[32 * c:32 * c + 32].hex())
    got = run_driver(driver, tmp_path, "leaf", cases)
    for g, w, case in zip(got, want, cases):
        assert g[0] == g[1] == w, case[:32]


# ---- the raw rule of the packed codec -------------------------------------------------------------------------------------
def classes(q, vb):
    half = (q - 1) // 2
    return {PK_Q: (half, q - 1), PK_Z: (vb, 2 * vb), PK_D: (1, 2)}


def check_raw(exe, tmp_path, q, vb, values):
    cls_of = classes(q, vb)
    cases = [(cls, c) for cls in (PK_Q, PK_Z, PK_D) for c in values[cls]]
    got = run_driver(exe, tmp_path, "raw", ["%d %d %d %d" % (q, vb, cls, c) for cls, c in cases])
    for (cls, c), g in zip(cases, got):
        bias, limit = cls_of[cls]
        ok = -bias <= c <= limit - bias
        marker = 2 ** limit.bit_length() - 1
        assert marker > limit
        want = [int(ok), c + bias if ok else marker]
        assert [int(v) for v in g[:2]] == want, (q, vb, cls, c, "32-bit rule")
        assert [int(v) for v in g[2:]] == want, (q, vb, cls, c, "64-bit rule")


def bounds_for(q):
    """verify_bound values: the one of a default context at N = 1024, k = 3 (when it fits), the smallest, the largest."""
    half = (q - 1) // 2
    default = 2 * 11 * 36 * 1 * 3 * 1024     # 2 sigma sqrt(N) with sigma = 11 kappa b sqrt(k N), kappa = 36, b = 1
    return sorted({min(default, half), 1, half})


@pytest.mark.parametrize("q", [Q_DEFAULT, Q_MIN, Q_MAX])
def test_raw_rule_at_the_edges(driver, tmp_path, q):
    for vb in bounds_for(q):
        values = {}
        for cls, (bias, limit) in classes(q, vb).items():
            assert limit == 2 * bias and bias < 2 ** 31
            vals = [0, bias, -bias, limit - bias, limit - bias + 1, -bias - 1, I32_MAX, I32_MIN]
            values[cls] = [v for v in vals if I32_MIN <= v <= I32_MAX]
            assert len(values[cls]) == len(vals)
        check_raw(driver, tmp_path, q, vb, values)


@pytest.mark.parametrize("q", [Q_DEFAULT, Q_MIN, Q_MAX])
def test_raw_rule_on_a_seeded_sweep(driver, tmp_path, q):
    rng = np.random.default_rng(62000 + q % 1000)
    for vb in bounds_for(q):
        values = {}
        for cls, (bias, limit) in classes(q, vb).items():
            near = [e + s for e in (0, bias, -bias, I32_MIN + 4, I32_MAX - 4) for s in range(-4, 5)]
            wide = rng.integers(I32_MIN, I32_MAX + 1, size=300, dtype=np.int64).tolist()
            inside = rng.integers(-bias, bias + 1, size=100, dtype=np.int64).tolist()
            values[cls] = [int(v) for v in near + wide + inside if I32_MIN <= v <= I32_MAX]
        check_raw(driver, tmp_path, q, vb, values)
