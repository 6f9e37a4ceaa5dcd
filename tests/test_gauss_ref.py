"""CPU checks of the references behind the Gaussian pin (tests/test_gpu_gauss_pin.py, tests/test_chacha.py):

  * tests/philox_ref.py against the Random123 known answers (the vectors tests/test_emul_core.py pins for the library's
    own generator) and against the CPU emulator's uniform sampler, so that the word source of the seeded pin is not new
    ground;
  * the comparison of tests/gauss_ref.py can fail: mutations of the reference itself — each one a bug that leaves
    the marginal distribution and the determinism of a sampler untouched — violate it against the unmutated reference;
  * the share of coefficients whose truncation the bound decides, from the reference alone."""
import ctypes as C

import numpy as np
import pytest

import chacha_ref
import gauss_ref
import philox_ref
from test_emul_core import load_emul

KEY = bytes((11 * i + 5) & 0xFF for i in range(32))      # as tests/test_gpu_keyed_samplers.py
NONCE = bytes((3 * i + 1) & 0xFF for i in range(16))
Q = 3515337053
HALF = (Q - 1) // 2

# Random123 kat_vectors, philox4x32 10 rounds: (counter, key, output)
KATS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_philox_ref_known_answers():
    for ctr, key, want in KATS:
        assert tuple(int(v) for v in philox_ref.philox4x32_10(ctr, key)) == want
    ctr = [np.array([k[0][i] for k in KATS]) for i in range(4)]          # and vectorised, all three at once
    key = [np.array([k[1][i] for k in KATS]) for i in range(2)]
    assert philox_ref.philox4x32_10(ctr, key).tolist() == [list(k[2]) for k in KATS]


@pytest.mark.parametrize("N,bound", [(4, 1), (1024, HALF)])
def test_philox_ref_matches_the_emulators_uniform_sampler(N, bound):
    """Counter layout and word order: block blk of polynomial poly gives coefficients 2 blk, 2 blk + 1 (rzk_rng.h:41)."""
    L = load_emul()
    polys = (5, (0xABCDEF01 << 32) | 0xFFFFFFFE)                         # both halves of the polynomial index
    seed, stream = (0x9E3779B9 << 32) | 77, 0x80000003                   # and of the seed
    got = philox_ref.uniform(seed, stream, N, bound, polys)
    want = np.empty(N, dtype=np.int64)
    for i, poly in enumerate(polys):
        L.emul_sample_uniform(C.c_uint64(seed), C.c_uint32(stream), C.c_uint64(poly), C.c_uint32(N), C.c_uint32(bound),
                              want.ctypes.data_as(C.POINTER(C.c_int64)))
        assert np.array_equal(got[i], want), poly
    assert not np.array_equal(got[0], got[1])


def test_reference_pieces_are_exact_where_they_claim_to_be():
    x = np.array([1, 2, 3, (1 << 63) - 1, 1 << 63, (1 << 64) - 1, 1 << 40], dtype=np.uint64)
    assert gauss_ref._clz64(x).tolist() == [63, 62, 62, 1, 0, 0, 23]
    a = np.array([0, 0.25, 0.5, 1, 1.5, 2], dtype=gauss_ref.LD)
    c, s = gauss_ref._cos_sin_half_turns(a)
    assert c.tolist() == [1, np.sqrt(gauss_ref.LD(2)) / 2, 0, -1, 0, 1] and s.tolist()[2:] == [1, 0, -1, 0]
    # u0 = 1 in the F64 form: radius 0; X = 0 in the F32 form is X = 1: u0 = 2^-64
    v, R = gauss_ref.real_f64(np.array([[0xFFFFFFFF, 0xFFFFFFFF, 1, 2]], dtype=np.uint32), 1000.0)
    assert R.tolist() == [0] and v.tolist() == [[0, 0]]
    _, R0 = gauss_ref.real_f32(np.array([[0, 0, 0, 0], [0, 1, 0, 0]], dtype=np.uint32), 1.0)
    assert R0[0] == R0[1] and abs(float(R0[0]) - np.sqrt(2 * 64 * np.log(2))) < 1e-12
    # float32(w2): 2^32 - 129 rounds down to 2^32 - 256, the tie 2^32 - 128 and 2^32 - 1 round up to a full turn
    w = np.array([[1, 0, w2, 0] for w2 in ((1 << 32) - 129, (1 << 32) - 128, (1 << 32) - 1)], dtype=np.uint64).astype(np.uint32)
    v, R = gauss_ref.real_f32(w, 100.0)
    assert v[1, 0] == R[1] and v[1, 1] == 0 and v[2, 0] == R[2] and v[2, 1] == 0
    assert v[0, 1] < 0 and abs(float(v[0, 1] / R[0]) + np.sin(np.pi * 256 / 2.0 ** 31)) < 1e-15


# ---- the comparison can fail -------------------------------------------------------------------------------------------------
SIGMA = 21780.0
POLYS, N = range(8), 512


@pytest.fixture(scope="module")
def words():
    return chacha_ref.gauss_words(KEY, NONCE, 3, N, POLYS)


def trunc_i64(v):
    return np.trunc(v).astype(np.int64)


@pytest.mark.parametrize("f32", [True, False], ids=["f32", "f64"])
def test_unmutated_reference_passes_its_own_comparison(words, f32):
    v, d = gauss_ref.real(f32, words, SIGMA)
    assert v.shape == (8, N // 2, 2) and d.shape == (8, N // 2, 1)
    st = gauss_ref.check(trunc_i64(v), v, d)
    assert st.n == 8 * N and st.differ == 0 and st.worst < 0
    # rounding to nearest instead of truncating toward zero is caught too
    assert gauss_ref.violates(np.rint(v).astype(np.int64), v, d)


def _xor1(w):
    return chacha_ref.gauss_words(KEY, NONCE, 3, N, POLYS, quarter_xor=1)


# name -> (form, mutated reference (words, sigma) -> real values).  Every mutation runs at sigma = 21780; those of the F64
# form also at 2^26, where that form runs in the samplers.
MUTATIONS = {
    "sine and cosine swapped, f32": (True, lambda w, s: gauss_ref.real_f32(w, s, swap=True)[0]),
    "sine and cosine swapped, f64": (False, lambda w, s: gauss_ref.real_f64(w, s, swap=True)[0]),
    "angle from w1, f32": (True, lambda w, s: gauss_ref.real_f32(w, s, angle_word=1)[0]),
    "pair i reads quarter i ^ 1, f32": (True, lambda w, s: gauss_ref.real_f32(_xor1(w), s)[0]),
    "pair i reads quarter i ^ 1, f64": (False, lambda w, s: gauss_ref.real_f64(_xor1(w), s)[0]),
    "sigma scaled by 1.005, f32": (True, lambda w, s: gauss_ref.real_f32(w, s * 1.005)[0]),
    "sigma scaled by 1.005, f64": (False, lambda w, s: gauss_ref.real_f64(w, s * 1.005)[0]),
}
CASES = [(name, SIGMA) for name in sorted(MUTATIONS)] + [(name, float(1 << 26)) for name in sorted(MUTATIONS) if not MUTATIONS[name][0]]


@pytest.mark.parametrize("name,sigma", CASES)
def test_each_mutation_violates_the_comparison(words, name, sigma):
    f32, mutated = MUTATIONS[name]
    v, d = gauss_ref.real(f32, words, sigma)
    got = trunc_i64(mutated(words, sigma))
    assert got.shape == v.shape
    assert gauss_ref.violates(got, v, d), name
    # and by far more than a marginal case: most coefficients are off by 1 + delta or more (1.005 sigma: those beyond
    # |v| = 200 or so, i.e. nearly all at these sigmas)
    assert (np.abs(got.astype(gauss_ref.LD) - v) >= 1 + d).mean() > 0.5, name


def test_f64_angle_from_w2_twice_violates_the_comparison_where_the_form_runs(words):
    """The F64 angle is (w2:w3 >> 11) 2^-53 turns; with w2 in place of w3 it moves by (w2 - w3) 2^-64 of a turn, a sample
    by 2 pi |w2 - w3| 2^-64 |v'| with v' the other coefficient of the pair.  A truncated sample changes where one lies
    that close to an integer: with E|w2 - w3| = 2^32 / 3 and E|v'| = 0.8 sigma a share of 1.67 2^-32 sigma of them —
    2.6 % at sigma = 2^26 (107 of this test's 4096; at least half of that is asserted), 2e-4 at 2^19, and 8.5e-6 at sigma
    = 21780: 0.03 coefficients of 4096, so there the integer output of the mutated map IS the correct output and no
    comparison of outputs can see the mutation.  It is therefore held at 2^26, the sigma at which the samplers run this
    form at its widest and the GPU pin draws it, not at 21780."""
    sigma = float(1 << 26)
    v, d = gauss_ref.real(False, words, sigma)
    got = trunc_i64(gauss_ref.real_f64(words, sigma, angle_words=(2, 2))[0])
    assert gauss_ref.violates(got, v, d)
    differ = int(((got != trunc_i64(v)) & gauss_ref.decidable(v, d)).sum())
    print("f64 angle from w2:w2 at sigma 2^26: %d of %d decidable coefficients differ" % (differ, v.size))
    assert differ >= 53


def test_a_mutation_of_one_pair_is_caught(words):
    """One swapped pair among 2048, one repeated block: the comparison is per coefficient, not a share."""
    v, d = gauss_ref.real(True, words, SIGMA)
    got = trunc_i64(v)
    got[5, 17] = got[5, 17, ::-1].copy()
    assert gauss_ref.violates(got, v, d)
    got = trunc_i64(v)
    got[6, :4] = got[2, :4]                       # polynomial 6 repeats the first block of polynomial 2
    assert gauss_ref.violates(got, v, d)


# ---- the decidable share, from the reference alone -----------------------------------------------------------------------------
@pytest.mark.parametrize("sigma,least", [(3.0, 0.9), (100.0, 0.9), (21780.0, 0.9)])
def test_decidable_share_f32(sigma, least):
    v, d = gauss_ref.real(True, gauss_ref.random_words(int(sigma), 100000), sigma)
    share = gauss_ref.decidable_share(v, d)
    print("f32 sigma %g: decidable share %.5f" % (sigma, share))
    assert share >= least


@pytest.mark.parametrize("sigma", [3.0, 21780.0, float(1 << 19), float(1 << 26)])
def test_decidable_share_f64(sigma):
    v, d = gauss_ref.real(False, gauss_ref.random_words(int(sigma), 100000), sigma)
    share = gauss_ref.decidable_share(v, d)
    print("f64 sigma %g: decidable share %.7f" % (sigma, share))
    assert share >= 0.999
