"""Seeded synthetic inputs with the reference's distributions.

  key entries U, message x, scalars g : uniform over [-(q-1)/2, (q-1)/2]  (commit.rs:41,53; params.rs:126;
                                         benches/bench.rs:354-358 — full length N, the worst case)
  r                                   : uniform in [-b, b]                 (commit.rs:101)
  y                                   : trunc(Normal(0, sigma))            (open.rs:88-94, polynomial.rs:28-44)
  d                                   : exactly kappa coefficients +-1     (challenge_space.rs:12-33)

numpy versions feed the parity tests; torch versions build the bench inputs directly in HBM.
"""
from __future__ import annotations

import numpy as np

Q_DEFAULT = 3515337053


def isqrt(x: int) -> int:
    import math

    return math.isqrt(x)


def sigma(b: int, kappa: int, k: int, N: int) -> int:
    return b * (11 * kappa) * isqrt(k * N)  # params.rs:94-98


def key(rng: np.random.Generator, N, n, k, l, q=Q_DEFAULT) -> np.ndarray:
    """[a1;a2] with a1 = [I_n | a1'], a2 = [0 | I_l | a2'] (commit.rs:33-60)."""
    half = (q - 1) // 2
    A = np.zeros((n + l, k, N), dtype=np.int64)
    for i in range(n):
        A[i, i, 0] = 1
        A[i, n:, :] = rng.integers(-half, half + 1, (k - n, N), dtype=np.int64)
    for i in range(l):
        A[n + i, n + i, 0] = 1
        if k - n - l > 0:
            A[n + i, n + l:, :] = rng.integers(-half, half + 1, (k - n - l, N), dtype=np.int64)
    return A


def uniform(rng, shape, q=Q_DEFAULT) -> np.ndarray:
    half = (q - 1) // 2
    return rng.integers(-half, half + 1, shape, dtype=np.int64)


def small(rng, shape, b=1) -> np.ndarray:
    return rng.integers(-b, b + 1, shape, dtype=np.int64)


def gauss(rng, shape, sig) -> np.ndarray:
    return np.trunc(rng.normal(0.0, float(sig), shape)).astype(np.int64)


def challenge(rng, batch_shape, N, kappa) -> np.ndarray:
    kap = min(kappa, N)
    B = int(np.prod(batch_shape, dtype=np.int64)) if len(batch_shape) else 1
    d = np.zeros((B, N), dtype=np.int64)
    for i in range(B):
        pos = rng.choice(N, kap, replace=False)
        d[i, pos] = rng.choice(np.array([-1, 1], dtype=np.int64), kap)
    return d.reshape(tuple(batch_shape) + (N,))


# ---- Cauchy-Schwarz-tight operands (prime-count edges) ----------------------------------------------------
# Every NTT-path product picks 1 - 3 auxiliary primes from the bound sum_terms |a|_2 |b|_2 of its exact result.  For the
# negacyclic conjugate b = conj(a) (b_0 = a_0, b_{N-i} = -a_i) coefficient 0 of a*b is exactly |a|_2^2 = |a|_2 |b|_2, so
# the bound is attained and an exact result can be placed on either side of a prime count's capacity.
AUX_PRIMES = (1073692673, 1073668097, 1073651713)   # rzk_core.h kPrimes


def crt_half(np_: int) -> int:
    """(P_np - 1) / 2: the largest |exact result| np auxiliary primes reconstruct."""
    P = 1
    for p in AUX_PRIMES[:np_]:
        P *= p
    return (P - 1) // 2


def conj(a) -> np.ndarray:
    """Negacyclic conjugate along the last axis: b_0 = a_0, b_{N-i} = -a_i."""
    a = np.asarray(a, dtype=np.int64)
    b = -a[..., ::-1]
    return np.concatenate([a[..., :1], b[..., :-1]], axis=-1)


def tight_pair(a):
    """(a, conj(a)): (a*b)_0 = |a|_2^2 = |a|_2 |b|_2."""
    return np.asarray(a, dtype=np.int64), conj(a)


def squares_to(target: int, cmax: int) -> list:
    """Greedy sum-of-squares decomposition: magnitudes c_i <= cmax with sum c_i^2 == target."""
    out = []
    rest = int(target)
    while rest:
        c = min(isqrt(rest), cmax)
        out.append(c)
        rest -= c * c
    return out


def spread(N: int, mags, rng, sign=True) -> np.ndarray:
    """Polynomial with the given magnitudes on distinct non-constant positions (random signs if sign), so it is never
    the key's constant 1."""
    a = np.zeros(N, dtype=np.int64)
    assert len(mags) < N
    pos = rng.choice(np.arange(1, N), len(mags), replace=False)
    sg = rng.choice(np.array([-1, 1]), len(mags)) if sign else np.ones(len(mags), dtype=np.int64)
    a[pos] = np.asarray(mags, dtype=np.int64) * sg
    return a


def sq_norm(a) -> int:
    return sum(int(v) * int(v) for v in np.asarray(a).ravel())


def tight_terms(N: int, target: int, nterms: int, rng, q=Q_DEFAULT, nz=4) -> list:
    """nterms polynomials K_t with sum_t |K_t|_2^2 == target exactly and every |K_t|_2^2 close to target / nterms.
    All but the last have nz non-zeros of one magnitude (|v|_1 |v|_inf = |v|_2^2: tight for kernels that measure
    that product); the last takes the exact remainder as a greedy sum of squares."""
    half = (q - 1) // 2
    out = []
    for _ in range(nterms - 1):
        c = isqrt(target // (nterms * nz))
        assert 1 < c <= half
        out.append(spread(N, [c] * nz, rng))
    rest = target - sum(sq_norm(K) for K in out)
    assert rest > 0
    out.append(spread(N, squares_to(rest, half), rng))
    assert sum(sq_norm(K) for K in out) == target
    return out


def edge_targets(np_: int) -> dict:
    """Exact results around the capacity H = (P_np - 1) / 2 of np_ primes.  'under' (H (1 - 2^-10)), 'below' (H - 1)
    and 'at' (H) fit np_ primes, but only 'under' lies outside the kernels' 2^-12 safety margin, so it is the one that
    the kernels reconstruct with np_ primes; 'below' and 'at' take np_ + 1.  'just', 'near' (within 2^-20 relative)
    and 'far' (2^-9) need np_ + 1."""
    H = crt_half(np_)
    return {"under": H - (H >> 10), "below": H - 1, "at": H, "just": H + 1, "near": H + (H >> 21),
            "far": H + (H >> 9)}


def negacyclic_coef0(a, b) -> int:
    """Coefficient 0 of a*b in Z[x]/(x^N + 1), in Python integers."""
    a = [int(v) for v in a]
    b = [int(v) for v in b]
    N = len(a)
    return a[0] * b[0] - sum(a[i] * b[N - i] for i in range(1, N))


# ---- device-side generators (torch: plumbing for synthetic bench data only) -----------------------------
def t_uniform(gen, shape, device, q=Q_DEFAULT):
    import torch

    half = (q - 1) // 2
    return torch.randint(-half, half + 1, shape, dtype=torch.int64, device=device, generator=gen)


def t_small(gen, shape, device, b=1):
    import torch

    return torch.randint(-b, b + 1, shape, dtype=torch.int64, device=device, generator=gen)


def t_gauss(gen, shape, device, sig):
    import torch

    return torch.trunc(torch.randn(shape, dtype=torch.float64, device=device, generator=gen) * float(sig)).to(torch.int64)


def t_challenge(gen, B, N, kappa, device):
    import torch

    kap = min(kappa, N)
    keys = torch.rand((B, N), device=device, generator=gen)
    pos = keys.argsort(dim=1)[:, :kap]
    signs = torch.randint(0, 2, (B, kap), device=device, generator=gen, dtype=torch.int64) * 2 - 1
    d = torch.zeros((B, N), dtype=torch.int64, device=device)
    d.scatter_(1, pos, signs)
    return d


def t_key(gen, N, n, k, l, device, q=Q_DEFAULT):
    import torch

    half = (q - 1) // 2
    A = torch.zeros((n + l, k, N), dtype=torch.int64, device=device)
    for i in range(n):
        A[i, i, 0] = 1
        A[i, n:, :] = torch.randint(-half, half + 1, (k - n, N), dtype=torch.int64, device=device, generator=gen)
    for i in range(l):
        A[n + i, n + i, 0] = 1
        if k - n - l > 0:
            A[n + i, n + l:, :] = torch.randint(-half, half + 1, (k - n - l, N), dtype=torch.int64, device=device,
                                                generator=gen)
    return A
