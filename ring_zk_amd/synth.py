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


# ---- norm-predicate edges (verdict edges) ------------------------------------------------------------------------
# The fused norm predicate sum c^2 < L, L = (bound + 1)^2, is decided by a float total outside the band
# L (1 +- 2 kNormSlack) = L (1 +- 2^-16) (rzk_wave.h) and by an exact integer sum inside it.  norm_edge builds one
# polynomial with a chosen exact sum of squares and a chosen placement of the weight over lanes, registers and halves.
NORM_STYLES = ("point", "spread", "upper", "lower", "lastreg", "wave2")
NORM_CLAMP = 1 << 24          # lane_sum_sq_exact clamps magnitudes here; norm_edge stays below it
NORM_BAND_IN = 2.0 ** -17     # |S / L - 1| <= this: inside the band by more than the float total's 2^-18
NORM_BAND_OUT = 2.0 ** -15    # |S / L - 1| >= this: the float total decides


def four_squares(m: int, nonzero: bool = False):
    """(a, b, c, d), a >= b >= c >= d >= 0, a^2 + b^2 + c^2 + d^2 == m (Lagrange), by search from the largest a; with
    nonzero every part is positive (None where m has no such split: 1, 3, 5, 9, 11, 17, 29, 41 and 4^j {2, 6, 14})."""
    if nonzero:
        odd = m
        while odd and odd % 4 == 0:
            odd //= 4
        if m < 4 or m in (5, 9, 11, 17, 29, 41) or odd in (2, 6, 14):
            return None
    a = isqrt(m)
    while a >= 0 and 4 * a * a >= m:
        r1 = m - a * a
        b = min(isqrt(r1), a)
        while b >= 0 and 3 * b * b >= r1:
            r2 = r1 - b * b
            c = min(isqrt(r2), b)
            while c >= 0 and 2 * c * c >= r2:
                d = isqrt(r2 - c * c)
                if d * d == r2 - c * c and (d > 0 or not nonzero):
                    return a, b, c, d
                c -= 1
            b -= 1
        a -= 1
    assert nonzero, m
    return None


def _filled(count: int, S: int, rng) -> np.ndarray:
    """count non-zero coefficients with random signs and sum of squares exactly S: count - 5 of magnitude
    floor(sqrt(S / count)), the last five absorb the remainder (one free magnitude + a four-squares split with every
    part positive)."""
    assert count > 5 and S >= 9 * count
    base = isqrt(S // count)
    rest = S - (count - 5) * base * base
    e = isqrt(rest - 4)
    while True:
        assert e > 0
        four = four_squares(rest - e * e, nonzero=True)
        if four is not None:
            break
        e -= 1
    mags = np.array([base] * (count - 5) + [e] + list(four), dtype=np.int64)
    return mags * rng.choice(np.array([-1, 1], dtype=np.int64), count)


def norm_edge(N: int, S: int, style: str, pos: int, rng) -> np.ndarray:
    """One polynomial with sum of squares exactly S and every |c| < 2^24.

      point    [m, a, b, c, d], m = floor(sqrt(S)), a^2 + b^2 + c^2 + d^2 = S - m^2, from coefficient pos on, wrapping
               past N - 1 (pos is ignored by the other styles)
      spread   all N coefficients non-zero, random signs: every lane and register carries weight
      upper    the same over coefficients >= N / 2 only (the second wavefront of a two-wavefront team, the second rolled
               half of a load)
      lower    over coefficients < N / 2 only
      lastreg  over coefficients >= N - 64 only
      wave2    over coefficients with bit 6 set only: thread t of a team holds coefficients e * LANES + t (Geo::j_p1), so
               with 128 threads these are exactly the second wavefront's, with 64 the odd registers
    """
    out = np.zeros(N, dtype=np.int64)
    if style == "point":
        m = isqrt(S)
        vals = [m] + list(four_squares(S - m * m))
        for i, v in enumerate(vals):
            out[(pos + i) % N] = v
    elif style == "spread":
        out[:] = _filled(N, S, rng)
    elif style == "upper":
        out[N // 2:] = _filled(N // 2, S, rng)
    elif style == "lower":
        out[:N // 2] = _filled(N // 2, S, rng)
    elif style == "lastreg":
        out[N - 64:] = _filled(64, S, rng)
    elif style == "wave2":
        out[(np.arange(N) & 64) != 0] = _filled(N // 2, S, rng)
    else:
        raise ValueError(style)
    assert sq_norm(out) == S and int(np.abs(out).max()) < NORM_CLAMP
    return out


def norm_plan(L: int) -> dict:
    """Sums of squares around the limit L = (bound + 1)^2 of a norm predicate.  'below' / 'at' / 'above' (L - 1, L,
    L + 1) lie inside the band, where only the exact sum can decide; lo_in .. hi_out sit ceil(L 2^-19) on either side of
    the band's own edges L (1 -+ 2^-16), where either path may run; 'far_lo' / 'far_hi' (L (1 -+ 2^-15)) are decided by
    the float total."""
    step = -(-L // (1 << 19))
    lo, hi = L - (L + (1 << 15)) // (1 << 16), L + (L + (1 << 15)) // (1 << 16)
    return {"below": L - 1, "at": L, "above": L + 1,
            "lo_out": lo - step, "lo_in": lo + step, "hi_in": hi - step, "hi_out": hi + step,
            "far_lo": L - -(-L // (1 << 15)), "far_hi": L + -(-L // (1 << 15))}


def norm_path(S: int, L: int) -> str:
    """'exact' / 'float' / 'edge' from exact rational arithmetic: which path must (or, 'edge', may) decide S against L."""
    dev = abs(S - L)
    if dev * (1 << 17) <= L:
        return "exact"
    if dev * (1 << 15) >= L:
        return "float"
    return "edge"


def fault_positions(N: int, rows: int, offset: int = 0):
    """One (row, coefficient) per coefficient position, the row cycling and stepping once more per 64 coefficients:
    row = (i % 64 + i // 64 + offset) % rows.  A thread of a 64-lane team holds coefficients e * 64 + lane, so every row
    meets every register index e, and every lane as soon as rows <= N / 64, whatever rows has in common with 64.  In a
    two-wavefront team (coefficients e * 128 + t) that holds for odd rows; an even number of rows ties the row's parity
    to the thread, which a second pass with offset 1 undoes."""
    return [((i % 64 + i // 64 + offset) % rows, i) for i in range(N)]


def sweep_faults(N: int, rows: int, pass_: int):
    """Position sweep over a batch of N entries, pass 0 or 1: entry i carries one fault at fault_positions[i] (offset =
    pass), except the clean entries, (i + i // 64) % 8 == 4 * pass: one in eight, on other lanes in the next register.
    Returns (entries, rows, coefficients) of the faulted entries; the two passes together reach every coefficient."""
    fp = fault_positions(N, rows, pass_)
    ent = [i for i in range(N) if (i + i // 64) % 8 != 4 * pass_]
    return (np.array(ent, dtype=np.int64), np.array([fp[i][0] for i in ent], dtype=np.int64),
            np.array([fp[i][1] for i in ent], dtype=np.int64))


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
