"""CPU tier of the keyed samplers' generator: ring_zk_amd/csrc/rzk_chacha.h (ChaCha20 block, HChaCha20, the counter
layout and the word-to-coefficient maps), compiled with g++ under -fsanitize=address,undefined into
tests/chacha/chacha_driver.cpp, against tests/chacha_ref.py (numpy).  The RFC 8439 block and the XChaCha draft's
HChaCha20 vector are pinned as hex literals so that the two restatements cannot drift together."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import chacha_ref
import gauss_ref

HERE = os.path.dirname(os.path.abspath(__file__))
Q = 3515337053
HALF = (Q - 1) // 2
KEY_RFC = bytes(range(32))
# RFC 8439 §2.3.2: key 00..1f, block counter 1, nonce 00 00 00 09 00 00 00 4a 00 00 00 00
BLOCK_RFC = ("10f1e7e4d13b5915500fdd1fa32071c4" "c7d1f4c733c068030422aa9ac3d46c4e"
             "d2826446079faa0914c2d705d98b02a2" "b5129cd1de164eb9cbd083e8a2503c4e")
# draft-irtf-cfrg-xchacha §2.2.1: key 00..1f, nonce 00 00 00 09 00 00 00 4a 00 00 00 00 31 41 59 27
NONCE_X = bytes.fromhex("000000090000004a0000000031415927")
SUBKEY_X = "82413b4227b27bfed30e42508a877d73a0f9e4d58a74a853c12ec41326d3ecdc"

KEYS = (KEY_RFC, bytes((7 * i + 3) & 0xFF for i in range(32)))
NONCES = (NONCE_X, bytes((0xF1 - 5 * i) & 0xFF for i in range(16)))
STREAMS = (0, 0x80000001)
POLYS = (0, 1, 5, (1 << 32) + 3, (0xABCDEF01 << 32) | 0xFFFFFFFF)   # word 14 (poly >> 32) is exercised


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build the ChaCha driver")
    exe = str(tmp_path_factory.mktemp("chacha") / "chacha_driver")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-o", exe,
                           os.path.join(HERE, "chacha", "chacha_driver.cpp")])
    return exe


def run_driver(exe, tmp_path, records):
    path = tmp_path / ("chacha_cases_%d.bin" % os.getpid())
    with open(path, "wb") as f:
        f.write(b"".join(records))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    res = subprocess.run([exe, str(path)], capture_output=True, text=True, env=env)
    assert res.returncode == 0, res.stderr[-4000:]
    return [line.split() for line in res.stdout.splitlines()]


def block_record(key, w):
    return struct.pack("<I", 1) + key + struct.pack("<4I", *w)


def hchacha_record(key, nonce):
    return struct.pack("<I", 2) + key + nonce


def sampler_record(kind, key, nonce, stream, N, par, poly):
    return struct.pack("<I", kind) + key + nonce + struct.pack("<3IQ", stream, N, par, poly)


def test_rfc8439_block(driver, tmp_path):
    w = (1, 0x09000000, 0x4A000000, 0)
    assert len(BLOCK_RFC) == 128 and BLOCK_RFC.startswith("10f1e7e4d13b5915500fdd1fa32071c4") and BLOCK_RFC.endswith("a2503c4e")
    assert chacha_ref.block_bytes(KEY_RFC, *w).hex() == BLOCK_RFC
    got = run_driver(driver, tmp_path, [block_record(KEY_RFC, w)])
    assert got == [["block", BLOCK_RFC]]


def test_blocks_agree_on_random_inputs(driver, tmp_path):
    rng = np.random.default_rng(5)
    cases = [(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), tuple(int(v) for v in rng.integers(0, 1 << 32, 4)))
             for _ in range(16)]
    cases.append((bytes([0xFF] * 32), (0xFFFFFFFF,) * 4))
    got = run_driver(driver, tmp_path, [block_record(k, w) for k, w in cases])
    assert [g[1] for g in got] == [chacha_ref.block_bytes(k, *w).hex() for k, w in cases]


def test_hchacha20_draft_vector(driver, tmp_path):
    assert chacha_ref.hchacha20(KEY_RFC, NONCE_X).hex() == SUBKEY_X
    recs = [hchacha_record(k, n) for k in KEYS for n in NONCES]
    got = run_driver(driver, tmp_path, recs)
    assert got[0] == ["hchacha", SUBKEY_X]
    assert [g[1] for g in got] == [chacha_ref.hchacha20(k, n).hex() for k in KEYS for n in NONCES]
    assert len({g[1] for g in got}) == 4


def test_reference_multiply_shift_is_exact():
    """chacha_ref's vectorised floor(X * range / 2^64) against Python integers, at the ends of every operand."""
    rng = np.random.default_rng(6)
    hi = np.concatenate([rng.integers(0, 1 << 32, 500, dtype=np.uint64), [0, 0xFFFFFFFF, 0xFFFFFFFF]]).astype(np.uint32)
    lo = np.concatenate([rng.integers(0, 1 << 32, 500, dtype=np.uint64), [0, 0xFFFFFFFF, 0]]).astype(np.uint32)
    for r in (1, 3, 1025, Q, (1 << 32) - 1):
        want = [((int(h) << 32 | int(l)) * r) >> 64 for h, l in zip(hi, lo)]
        assert chacha_ref._mulhi64(hi, lo, r).tolist() == want


@pytest.mark.parametrize("N", [4, 16, 1024])
@pytest.mark.parametrize("bound", [1, HALF])
def test_uniform_sampler_matches_reference(driver, tmp_path, N, bound):
    combos = [(k, n, s) for k in KEYS for n in NONCES for s in STREAMS]
    recs = [sampler_record(3, k, n, s, N, bound, p) for k, n, s in combos for p in POLYS]
    got = run_driver(driver, tmp_path, recs)
    assert len(got) == len(recs) and all(g[0] == "uniform" and len(g) == N + 1 for g in got)
    have = np.array([[int(v) for v in g[1:]] for g in got], dtype=np.int64).reshape(len(combos), len(POLYS), N)
    for i, (k, n, s) in enumerate(combos):
        assert np.array_equal(have[i], chacha_ref.uniform(k, n, s, N, bound, POLYS)), (i, N, bound)
    assert have.min() >= -bound and have.max() <= bound
    assert len({have[i].tobytes() for i in range(len(combos))}) == len(combos)   # key, nonce and stream all matter
    assert len({have[0, p].tobytes() for p in range(len(POLYS))}) == len(POLYS)  # and so do both halves of poly


@pytest.mark.parametrize("N,kappa", [(4, 4), (64, 64), (1024, 36)])
def test_challenge_sampler_matches_reference(driver, tmp_path, N, kappa):
    combos = [(k, n, s) for k in KEYS for n in NONCES for s in STREAMS]
    recs = [sampler_record(4, k, n, s, N, kappa, p) for k, n, s in combos for p in POLYS]
    got = run_driver(driver, tmp_path, recs)
    assert len(got) == len(recs) and all(g[0] == "challenge" and len(g) == N + 1 for g in got)
    have = np.array([[int(v) for v in g[1:]] for g in got], dtype=np.int64).reshape(len(combos), len(POLYS), N)
    for i, (k, n, s) in enumerate(combos):
        assert np.array_equal(have[i], chacha_ref.challenge(k, n, s, N, kappa, POLYS)), (i, N, kappa)
    assert (np.abs(have).sum(axis=-1) == kappa).all() and np.abs(have).max() == 1   # challenge_space.rs:56-82
    if kappa < N:
        assert len({have[i].tobytes() for i in range(len(combos))}) == len(combos)


# ---- the Gaussian word-to-pair map on the host (rzk_gauss.h with libm) against tests/gauss_ref.py ---------------------------
# Assertions and bounds are those of the GPU pin (tests/test_gpu_gauss_pin.py): gauss_ref.check.  The F32 form takes
# sigma < 2^19, the last one being 2^19 - 1, where almost no truncation is decidable and only |got - ref| < 1 + delta
# binds; the F64 form is held at every sigma.
def gauss_record(f32, sigma, words):
    w = np.ascontiguousarray(words, dtype="<u4")
    assert w.ndim == 2 and w.shape[1] == 4
    return struct.pack("<IIdI", 5, 1 if f32 else 0, float(sigma), len(w)) + w.tobytes()


def host_gauss(driver, tmp_path, f32, sigma, words):
    (got,) = run_driver(driver, tmp_path, [gauss_record(f32, sigma, words)])
    assert got[0] == "gauss" and len(got) == 1 + 2 * len(words)
    return np.array([int(v) for v in got[1:]], dtype=np.int64).reshape(len(words), 2)


GAUSS_CASES = [(True, 3.0, 0.9), (True, 100.0, 0.9), (True, 21780.0, 0.9), (True, float((1 << 19) - 1), None),
               (False, 3.0, 0.999), (False, 21780.0, 0.999), (False, float(1 << 19), 0.999), (False, float(1 << 26), 0.999)]
GAUSS_IDS = ["%s-%g" % ("f32" if f else "f64", s) for f, s, _ in GAUSS_CASES]


@pytest.mark.parametrize("f32,sigma,least", GAUSS_CASES, ids=GAUSS_IDS)
def test_host_gauss_map_on_random_words(driver, tmp_path, f32, sigma, least):
    case = GAUSS_CASES.index((f32, sigma, least))
    words = gauss_ref.random_words(1000 + case, 100000)
    v, d = gauss_ref.real(f32, words, sigma)
    share = gauss_ref.decidable_share(v, d)
    if least is not None:   # from the reference alone, before the output is looked at
        assert share >= least, share
    st = gauss_ref.check(host_gauss(driver, tmp_path, f32, sigma, words), v, d, GAUSS_IDS[case])
    print("host %s sigma %g: decidable %.5f, differ from trunc(ref) %d of %d, worst (|got - ref| - 1) / delta %.3f"
          % ("f32" if f32 else "f64", sigma, share, st.differ, st.n, st.worst))
    assert st.undecidable == round((1 - share) * st.n)


@pytest.mark.parametrize("f32,sigma,least", GAUSS_CASES, ids=GAUSS_IDS)
def test_host_gauss_map_on_edge_words(driver, tmp_path, f32, sigma, least):
    """The ends of both uniforms and of the angle, and the region where log2 u0 cancels (gauss_ref.x_edges_f32).  No
    decidable share is asked of these words: they are chosen where the bound is at its widest."""
    words = gauss_ref.edge_words_f32() if f32 else gauss_ref.edge_words_f64()
    v, d = gauss_ref.real(f32, words, sigma)
    got = host_gauss(driver, tmp_path, f32, sigma, words)
    gauss_ref.check(got, v, d, "edge words")
    if not f32:
        zero = (words[:, 0] == 0xFFFFFFFF) & (words[:, 1] >= 0xFFFFF800)    # X >> 11 = 2^53 - 1: u0 = 1
        assert zero.sum() == 32 and not got[zero].any()
