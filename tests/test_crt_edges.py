"""CRT prime-count edges on the CPU: the tight-operand generator and the lane emulator's reconstruction.

ring_zk_amd/synth.py builds operands whose exact product attains the Cauchy-Schwarz bound the kernels use to pick 1, 2
or 3 auxiliary primes (tests/test_gpu_prime_count_edges.py feeds them to every kernel that makes that choice).  Here:

  * the generator's claims, checked in Python integers for every family the GPU tests use;
  * with the prime count forced (tests/emul/emul.cpp, the g++ build of the kernels' core), results of exactly
    +-H_np, +-(H_np - 1) and +-H_np (1 - 2^-10), H_np = (P_np - 1) / 2, reconstruct exactly for np = 1 and 2 (the
    centring constants);
  * every "above" family gives a wrong result at np primes and the right one at np + 1, so a GPU case that picks too
    few primes cannot pass by luck.
"""
import numpy as np
import pytest

from oracle import oracle as O
from ring_zk_amd import synth
from test_emul_core import _polymul, load_emul

Q = O.Q_DEFAULT
HALF = (Q - 1) // 2


@pytest.fixture(scope="module")
def emul():
    return load_emul()


def test_crt_half_matches_the_library_tables(emul):
    for np_ in (1, 2, 3):
        P = 1
        for i in range(np_):
            assert synth.AUX_PRIMES[i] == emul.emul_prime(i)
            P *= synth.AUX_PRIMES[i]
        H = synth.crt_half(np_)
        assert H == (P - 1) // 2
        # crt_capacity rounds down by 2^-40 at most: the capacity lies in (H (1 - 2^-39), H]
        cap = emul.emul_capacity(np_)
        assert H * (1 - 2.0 ** -39) < cap <= H


@pytest.mark.parametrize("N", [512, 1024, 2048])
def test_conj_pair_attains_the_bound(N):
    rng = np.random.default_rng(N)
    a = synth.uniform(rng, (N,))
    a2, b = synth.tight_pair(a)
    assert np.array_equal(a2, a)
    assert b[0] == a[0] and all(b[N - i] == -a[i] for i in (1, 2, N - 1))
    assert synth.sq_norm(a) == synth.sq_norm(b)
    assert synth.negacyclic_coef0(a, b) == synth.sq_norm(a)
    assert np.array_equal(synth.conj(synth.conj(a)), a)
    # the whole product mod q agrees at coefficient 0 (the oracle reduces; Python integers do not)
    assert int(O.poly_mul(a, b)[0]) == O.center(synth.sq_norm(a) % Q)


@pytest.mark.parametrize("np_", [1, 2])
@pytest.mark.parametrize("nterms", [1, 2, 3, 8, 16])
def test_tight_terms_identity(np_, nterms):
    """sum_t (K_t * conj(K_t))_0 == sum_t |K_t|_2 |conj(K_t)|_2 == target, exactly; the equal-magnitude terms are also
    tight for |v|_1 |v|_inf; dropping any one term leaves the total below the capacity the kernel compares with."""
    N = 1024
    rng = np.random.default_rng(100 * np_ + nterms)
    for name, target in synth.edge_targets(np_).items():
        Ks = synth.tight_terms(N, target, nterms, rng)
        assert all(int(np.abs(K).max()) <= HALF for K in Ks)
        total = sum(synth.negacyclic_coef0(K, synth.conj(K)) for K in Ks)
        assert total == target == sum(synth.sq_norm(K) for K in Ks)
        for K in Ks[:-1]:
            assert int(np.abs(K).sum()) * int(np.abs(K).max()) == synth.sq_norm(K)
        if nterms > 1 and name in ("just", "near", "far"):
            cap = synth.crt_half(np_) * (1 - 2.0 ** -12)      # primes_for's safety factor is 1 + 2^-12
            for K in Ks:
                assert target - synth.sq_norm(K) < cap, (name, nterms)


def _single(N, X, rng, sign=1):
    """(a, b) with (a*b)_0 == sign * X exactly: a a greedy sum of squares, b = +-conj(a)."""
    a = synth.spread(N, synth.squares_to(abs(X), HALF), rng)
    return a, sign * synth.conj(a)


@pytest.mark.parametrize("logn", [9, 10, 11])
@pytest.mark.parametrize("np_", [1, 2])
def test_forced_prime_count_reconstructs_the_centre_exactly(emul, logn, np_):
    N = 1 << logn
    H = synth.crt_half(np_)
    rng = np.random.default_rng(7 * logn + np_)
    for X in (H, H - 1, synth.edge_targets(np_)["under"]):
        for sign in (1, -1):
            a, b = _single(N, X, rng, sign)
            assert synth.negacyclic_coef0(a, b) == sign * X
            want = O.poly_mul(a, b)
            assert np.array_equal(_polymul(emul, logn, np_, a, b), want), (X, sign)
            assert np.array_equal(_polymul(emul, logn, np_ + 1, a, b), want)


@pytest.mark.parametrize("logn", [9, 10, 11])
@pytest.mark.parametrize("np_", [1, 2])
def test_above_capacity_is_wrong_with_too_few_primes(emul, logn, np_):
    N = 1 << logn
    rng = np.random.default_rng(50 + 7 * logn + np_)
    for name, X in synth.edge_targets(np_).items():
        if name in ("under", "below", "at"):
            continue
        for sign in (1, -1):
            a, b = _single(N, X, rng, sign)
            want = O.poly_mul(a, b)
            got = _polymul(emul, logn, np_, a, b)
            assert int(got[0]) != int(want[0]), (name, sign)
            assert np.array_equal(_polymul(emul, logn, np_ + 1, a, b), want), (name, sign)
