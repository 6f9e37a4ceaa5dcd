"""CPU tier of the exact discrete Gaussian sampler: ring_zk_amd/csrc/rzk_dgauss.h with rzk_chacha.h, compiled
with g++ under -fsanitize=address,undefined into tests/dgauss/dgauss_driver.cpp, against tests/dgauss_ref.py (Python
integers) bit for bit, against mpmath for exp2m and for the law itself, and a chi-square of one stream draw.

The sampler is integer-only, so every comparison with the restatement is an equality.  The distribution is shown by
test_law_is_the_discrete_gaussian: the probability of every value follows from the integer thresholds, and is compared
with rho_sigma from mpmath at 200 bits; that test is not statistical."""
import os
import shutil
import struct
import subprocess
from math import log, sqrt

import mpmath
import numpy as np
import pytest

import dgauss_ref as D

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = (bytes(range(32)), bytes((7 * i + 3) & 0xFF for i in range(32)))
NONCES = (bytes.fromhex("000000090000004a0000000031415927"), bytes((0xF1 - 5 * i) & 0xFF for i in range(16)))
STREAMS = (0, 0x80000001)
POLYS = (0, 1, (1 << 32) - 1, 1 << 32, (0xABCDEF01 << 32) | 0xFFFFFFFF)   # either side of 2^32: words 13 and 14


SANITIZE = ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer")


def build_driver(tmp_path_factory, sanitize=True):
    """The stand-alone driver.  The CPU tier builds it under ASan/UBSan; a test that runs next to the GPU (the debug entry of
    tests/test_gpu_dgauss.py) takes the plain build: sanitizers stay with the CPU tier."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build the dgauss driver")
    exe = str(tmp_path_factory.mktemp("dgauss") / "dgauss_driver")
    subprocess.check_call([gxx, "-std=c++17", "-O1", *(SANITIZE if sanitize else ()), "-Wall", "-Werror",
                           "-Wno-unknown-pragmas", "-o", exe, os.path.join(HERE, "dgauss", "dgauss_driver.cpp")])
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory)


def run_driver(exe, tmp_path, records):
    path = tmp_path / ("dgauss_cases_%d.bin" % os.getpid())
    with open(path, "wb") as f:
        f.write(b"".join(records))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    res = subprocess.run([exe, str(path)], capture_output=True, text=True, env=env)
    assert res.returncode == 0, res.stderr[-4000:]
    return [line.split() for line in res.stdout.splitlines()]


def trial_record(sigma, words):
    w = np.ascontiguousarray(words, dtype="<u4")
    assert w.ndim == 2 and w.shape[1] == 8
    return struct.pack("<III", 3, sigma, len(w)) + w.tobytes()


def host_trials(exe, tmp_path, sigma, words):
    """int64 [n][2]: (accepted, value) of every 8-word tuple, from the driver."""
    (got,) = run_driver(exe, tmp_path, [trial_record(sigma, words)])
    assert got[0] == "trial" and len(got) == 1 + 2 * len(words)
    return np.array([int(v) for v in got[1:]], dtype=np.int64).reshape(len(words), 2)


def ref_trials(sigma, words):
    C, k = D.params(sigma)
    return np.array([[int(ok), v] for ok, v in (D.trial(C, k, [int(x) for x in w]) for w in words)], dtype=np.int64)


def sample_record(key, nonce, stream, N, sigma, poly):
    return struct.pack("<I", 4) + key + nonce + struct.pack("<3IQ", stream, N, sigma, poly)


def host_sample(exe, tmp_path, key, nonce, stream, N, sigma, polys):
    got = run_driver(exe, tmp_path, [sample_record(key, nonce, stream, N, sigma, p) for p in polys])
    assert len(got) == len(polys) and all(g[0] == "sample" and len(g) == N + 1 for g in got)
    return np.array([[int(v) for v in g[1:]] for g in got], dtype=np.int64)


# ---- parameters -------------------------------------------------------------------------------------------------------------
def test_parameters(driver, tmp_path):
    mpmath.mp.prec = 400
    assert D.K == 0xB8AA3B295C17F0BBBE87FED0691D3E88 == int(mpmath.floor(mpmath.mpf(2) ** 127 / mpmath.log(2)))
    assert D.W == 880717420568577
    assert [D.params(s)[1] for s in (1, 3, 21780, 1 << 26)] == [2, 4, 25644, 79014650]
    sigmas = (1, 2, 3, 132, 15444, 21780, 30888, (1 << 19) - 1, 1 << 26)
    got = run_driver(driver, tmp_path, [struct.pack("<II", 1, s) for s in sigmas])
    for s, g in zip(sigmas, got):
        C, k = D.params(s)
        assert g == ["params", "%032x" % C, str(k), str((1 << 32) % k)], s
        assert k < 1 << 27 and 8 * k >= 9.4 * s


# ---- exp2m ------------------------------------------------------------------------------------------------------------------
def test_exp2m_against_mpmath(driver, tmp_path):
    mpmath.mp.prec = 200
    rng = np.random.default_rng(61)
    fs = [1, 2, 1 << 63, (1 << 63) - 1, (1 << 63) + 1, (1 << 64) - 1] + [int(v) for v in rng.integers(1, 1 << 64, 10000, dtype=np.uint64)]
    (got,) = run_driver(driver, tmp_path, [struct.pack("<II", 2, len(fs)) + b"".join(struct.pack("<Q", f) for f in fs)])
    have = [int(v) for v in got[1:]]
    assert have == [D.exp2m(f) for f in fs]
    worst = 0
    for f, v in zip(fs, have):
        real = mpmath.mpf(2) ** 64 * mpmath.power(2, -mpmath.mpf(f) / mpmath.mpf(2) ** 64)
        worst = max(worst, abs(float(v - real)))
    print("exp2m: worst |error| = %.3f units of 2^-64 over %d arguments (bound %g)" % (worst, len(fs), D.EPS_B * 2.0 ** 64))
    assert worst * 2.0 ** -64 <= D.EPS_B
    # f = 0 is exact: probability 2^-a, with a = 0 "always"
    pairs = [(0, 0), (1, 0), (63, 0), (64, 0), (63, 12345), (64, 12345), (63, (1 << 64) - 1), (200, 7)]
    (got,) = run_driver(driver, tmp_path, [struct.pack("<II", 6, len(pairs)) + b"".join(struct.pack("<IQ", a, f) for a, f in pairs)])
    have = [(int(got[1 + 2 * i]), int(got[2 + 2 * i])) for i in range(len(pairs))]
    assert have == [D.threshold(a, f) for a, f in pairs]
    assert have[:4] == [(D.ALWAYS, 0), (D.THRESHOLD, 1 << 63), (D.THRESHOLD, 2), (D.REJECT, 0)]
    assert have[4] == (D.THRESHOLD, 1) and have[5] == (D.REJECT, 0)   # a = 63 and a = 64


# ---- one trial, bit for bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [3, 21780, 1 << 26])
def test_trial_on_random_words(driver, tmp_path, sigma):
    words = np.random.default_rng(sigma).integers(0, 1 << 32, (100000, 8), dtype=np.uint64).astype(np.uint32)
    want = ref_trials(sigma, words)
    share = want[:, 0].mean()
    print("sigma %d: %.4f of the trials accept (%.3f trials per sample)" % (sigma, share, 1 / share))
    assert 0.55 < share < 0.70
    assert np.array_equal(host_trials(driver, tmp_path, sigma, words), want)


@pytest.mark.parametrize("sigma", [1, 3, 21780, 1 << 26])
def test_trial_on_edge_words(driver, tmp_path, sigma):
    """The edges listed in dgauss_ref.edge_words.  a = 63 and a = 64 are reached by no candidate of any sigma (the exponent
    passes 64 only at sigma = 1, where it goes 47, 62, 67: z = 10, 11, 12), so the trial is taken to a = 62 and a = 67
    there and the threshold function to 63 and 64 directly (test_exp2m_against_mpmath)."""
    edges = D.edge_words(sigma)
    labels = [e[0] for e in edges]
    words = np.array([e[1] for e in edges], dtype=np.uint32)
    want = ref_trials(sigma, words)
    at = {lab: tuple(int(v) for v in row) for lab, row in zip(labels, want)}
    C, k = D.params(sigma)
    # the restatement behaves at the edges as the definition says, before the driver is looked at
    assert at["x=7 largest X"][1] == 8 * k - 1
    assert at["x lemire lo=%d" % ((1 << 64) % D.W - 1)][0] == 0 and at["x lemire lo=0"][0] == 0
    assert [at["z=0 bits=%d" % b] for b in range(4)] == [(1, 0), (1, 0), (0, 0), (0, 0)]
    for lab in labels:
        if lab.endswith("r=T-1"):
            assert at[lab][0] == 1 and at[lab[:-3] + "T+0"][0] == 0, lab
    # 2^32 mod k = 0 at sigma = 1 and 3 (k = 2, 4): no word of y is rejected there; at the other two some word is
    assert ("y below the edge" in at) == ((1 << 32) % k != 0) == (sigma in (21780, 1 << 26))
    if (1 << 32) % k:
        assert at["y below the edge"][0] == 0
    assert at["y at the edge"][0] == 1
    if sigma == 1:
        assert "x=5 y=1 a=62 r=T-1" in at and at["x=6 y=0 a=67 kind=0"][0] == 0
    assert np.array_equal(host_trials(driver, tmp_path, sigma, words), want)


# ---- the stream sampler, bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 4, 8, 64])
def test_stream_sampler_matches_reference(driver, tmp_path, N):
    combos = [(k, n, s) for k in KEYS for n in NONCES for s in STREAMS]
    have = []
    for sigma, (k, n, s) in zip((3, 21780, 1 << 26, 1, 3, 21780, 1 << 26, 2), combos):
        used = set()
        want = D.sample(k, n, s, N, sigma, POLYS, used=used)
        got = host_sample(driver, tmp_path, k, n, s, N, sigma, POLYS)
        assert np.array_equal(got, want), (N, sigma)
        assert all(w >> 31 == 1 and (w & 0xFFFF) < (N + 1) // 2 for w in used)
        have.append(host_sample(driver, tmp_path, k, n, s, N, 21780, POLYS))
    assert len({h.tobytes() for h in have}) == len(combos)                       # key, nonce and stream all matter
    assert len({have[0][p].tobytes() for p in range(len(POLYS))}) == len(POLYS)  # and so do both halves of poly


def test_a_source_that_always_rejects_gives_zero_after_t_max_trials(driver, tmp_path):
    assert D.T_MAX == 160
    for N in (2, 5, 8):
        (got,) = run_driver(driver, tmp_path, [struct.pack("<III", 7, 3, N)])
        assert got[0] == "exhaust" and int(got[1]) == D.T_MAX * ((N + 1) // 2)
        assert [int(v) for v in got[2:]] == [0] * N
    # the restatement's loop ends the same way: no accepted trial within t_max leaves 0
    assert D.trial(*D.params(3), [0] * 8) == (False, 0)
    # and T_MAX is enough: a trial of the worst sigma (1: k = 2 against 1.18) accepts with probability > 0.40
    C, k = D.params(1)
    acc = sum((1 << (49 - (z // k) ** 2)) / D.W / k * (0.5 if z == 0 else 1.0) *
              (lambda kt: 1.0 if kt[0] == D.ALWAYS else kt[1] / 2.0 ** 64)(D.threshold(*D.exponent(C, k, z // k, z % k)))
              for z in range(8 * k))
    assert 0.40 < acc < 0.41 and D.T_MAX * log(1 - acc, 2) < -100


# ---- the law, exactly ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [3, 10])
def test_law_is_the_discrete_gaussian(driver, tmp_path, sigma):
    """P(value = v) = P(x) P(y) P(accept z) / 2 for every v = +-z (the sign), and for v = 0 (the coin): weight(x) / k *
    T(z) / 2^64 / 2 with the driver's integer thresholds.  Normalised at z = 1 it must be rho_sigma(z) / rho_sigma(1) within
    2 eps_B 2^a relative: the threshold is within eps_B of 2^-a 2^-t absolutely, t < 1.  Without the coin, 0 would
    carry the mass of both signs: twice rho(0)."""
    mpmath.mp.prec = 200
    C, k = D.params(sigma)
    (got,) = run_driver(driver, tmp_path, [struct.pack("<II", 5, sigma)])
    assert got[0] == "law" and len(got) == 1 + 3 * 8 * k
    law, a_of = [], []
    for z in range(8 * k):
        a, kind, T = (int(v) for v in got[1 + 3 * z:4 + 3 * z])
        assert (a, (kind, T)) == (D.exponent(C, k, z // k, z % k)[0], D.threshold(*D.exponent(C, k, z // k, z % k)))
        acc = mpmath.mpf(1) if kind == D.ALWAYS else mpmath.mpf(T) / mpmath.mpf(2) ** 64
        law.append(mpmath.mpf(1 << (49 - (z // k) ** 2)) / D.W / k * acc / 2)    # the sign bit, or the coin at z = 0
        a_of.append(a)
    rho = lambda z: mpmath.exp(-mpmath.mpf(z * z) / (2 * sigma * sigma))
    worst = 0.0
    for z in range(8 * k):
        dev = abs(law[z] / law[1] * rho(1) / rho(z) - 1)
        worst = max(worst, float(dev / (2 * D.EPS_B * 2.0 ** a_of[z])))
        assert dev <= 2 * D.EPS_B * 2.0 ** a_of[z], (z, float(dev))
    print("sigma %d: worst relative deviation of the law = %.3f of its bound, over z = 0 .. %d" % (sigma, worst, 8 * k - 1))
    assert a_of[0] == 0 and abs(law[0] / law[1] * rho(1) - 1) <= 2 * D.EPS_B          # P(0) is rho(0), not 2 rho(0)
    # the tail cut: mass beyond 8k, relative to the whole
    total = 1 + 2 * mpmath.nsum(rho, [1, mpmath.inf])
    assert 2 * mpmath.nsum(rho, [8 * k, mpmath.inf]) / total < mpmath.mpf(2) ** -63


# ---- chi-square of one stream draw at sigma = 3 ----------------------------------------------------------------------------------------
CHI_N, CHI_NU = 1 << 17, 25
CHI_BOUND = CHI_NU + 2 * sqrt(CHI_NU * log(1e9)) + 2 * log(1e9)   # Laurent-Massart at a false-alarm rate of 1e-9: 112


def chi_square(values):
    mpmath.mp.prec = 100
    rho = lambda z: mpmath.exp(-mpmath.mpf(z * z) / 18)
    total = 1 + 2 * mpmath.nsum(rho, [1, mpmath.inf])
    p = [float(rho(z) / total) for z in range(-12, 13)]
    p.append(1.0 - sum(p))
    v = np.asarray(values).ravel()
    assert v.size == CHI_N
    obs = [int((v == z).sum()) for z in range(-12, 13)] + [int((np.abs(v) > 12).sum())]
    assert 3.5 < CHI_N * p[-1] < 4                                                   # the tail cell (|v| >= 13) expects 3.7
    return sum((o - CHI_N * q) ** 2 / (CHI_N * q) for o, q in zip(obs, p))


def test_chi_square_at_sigma_3(driver, tmp_path):
    assert 111 < CHI_BOUND < 113
    polys = range(CHI_N // 64)
    want = D.sample(KEYS[1], NONCES[1], 5, 64, 3, polys)
    stat = chi_square(want)
    print("chi-square of %d coefficients at sigma = 3: %.1f on %d degrees of freedom (bound %.1f)" % (CHI_N, stat, CHI_NU, CHI_BOUND))
    assert stat < CHI_BOUND                                                           # from the restatement alone
    assert np.array_equal(host_sample(driver, tmp_path, KEYS[1], NONCES[1], 5, 64, 3, polys), want)
