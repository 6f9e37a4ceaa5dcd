"""Reference statement of the prover's rejection-sampling step (include/rzk.h "rejection sampling").
It shares no code with the library: v, S1, S2, E and the fail flags are computed in Python integers, the threshold

    T = 2 sigma^2 (lnM + ln((coin + 1) / R))

with `decimal` at 50 digits.  The library evaluates T in double precision, so its decision is pinned only where the
exact E is not too close to the exact T.  A case is DECIDABLE when |E - T| > 2 sigma^2 2^-44: |ln| <= 44 (R <= 2^62,
lnM small), the quotient (coin + 1) / R and the logarithm are each correct to a few ulp (2^-53 relative, so about
44 x 2^-51 < 2^-45 absolute on the sum), and the two remaining operations (the sum with lnM, the product with
2 sigma^2) add two more roundings of a value below 45: the double T is within 2 sigma^2 2^-44 of the exact one, with
room.  E and the flags are always compared exactly; accept exactly on decidable cases."""
import decimal
from decimal import Decimal

NONCANON, VMAX, NORM, COIN = 1, 2, 4, 8
CTX50 = decimal.Context(prec=50)


class Params:
    def __init__(self, q, N, sigma, vmax, verify_bound):
        self.q, self.N, self.sigma, self.vmax, self.verify_bound = int(q), int(N), int(sigma), int(vmax), int(verify_bound)
        self.half = (self.q - 1) // 2


def params_of(ctx):
    """Params of a ring_zk_amd.Context (its numbers only)."""
    return Params(ctx.q, ctx.N, ctx.sigma, ctx.kappa * ctx.b, ctx.verify_bound)


def centred(a, q):
    a %= q
    return a - q if a > (q - 1) // 2 else a


def wrap64(a):
    a &= (1 << 64) - 1
    return a - (1 << 64) if a >> 63 else a


def proof_stats(P, polys):
    """polys: [(z coefficients, y coefficients)] of one proof, Python ints -> (E, flags) in exact integers."""
    S1 = S2 = 0
    flags = 0
    for z, y in polys:
        assert len(z) == len(y) == P.N
        if any(abs(c) > P.half for c in z) or any(abs(c) > P.half for c in y):
            flags |= NONCANON
        v = [centred(a - b, P.q) for a, b in zip(z, y)]
        if any(abs(c) > P.vmax for c in v):
            flags |= VMAX
        if sum(c * c for c in z) >= (P.verify_bound + 1) ** 2:
            flags |= NORM
        S1 += sum(a * b for a, b in zip(z, v))
        S2 += sum(c * c for c in v)
    return S2 - 2 * S1, flags


def threshold(P, lnM, coin, R):
    """T as a 50-digit Decimal (lnM: the double the library is given, taken exactly)."""
    u = CTX50.divide(Decimal(coin + 1), Decimal(R))
    return CTX50.multiply(Decimal(2 * P.sigma * P.sigma), CTX50.add(Decimal(lnM), CTX50.ln(u)))


def margin(P):
    return Decimal(2 * P.sigma * P.sigma) / Decimal(1 << 44)


def decide(P, E, flags, coin, R, lnM):
    """(accept, decidable)."""
    if not 0 <= coin < R:
        flags |= COIN
    if flags:
        return False, True
    T = threshold(P, lnM, coin, R)
    return Decimal(E) >= T, abs(Decimal(E) - T) > margin(P)


def largest_accepted_coin(P, E, lnM, R):
    """c* = the largest coin in [0, R) that the exact rule accepts for this E (-1: none)."""
    x = CTX50.subtract(CTX50.divide(Decimal(E), Decimal(2 * P.sigma * P.sigma)), Decimal(lnM))
    c = int(CTX50.multiply(Decimal(R), CTX50.exp(x)).to_integral_value(rounding=decimal.ROUND_FLOOR)) - 1
    c = min(c, R - 1)
    while c + 1 < R and Decimal(E) >= threshold(P, lnM, c + 1, R):   # the floor of a 50-digit product: settle the last unit
        c += 1
    while c >= 0 and Decimal(E) < threshold(P, lnM, c, R):
        c -= 1
    return c


def run(P, parts, coin, R, lnM, trusted=False):
    """parts: [(z, y)] numpy slabs [B][...][N]; coin: [B].  Per proof: E (as the int64 the library stores), flags,
    accept, decidable."""
    B = len(coin)
    flat = [(z.reshape(B, -1, P.N).tolist(), y.reshape(B, -1, P.N).tolist()) for z, y in parts]
    out = []
    for b in range(B):
        polys = [(zz, yy) for zs, ys in flat for zz, yy in zip(zs[b], ys[b])]
        E, flags = proof_stats(P, polys)
        if trusted:
            assert not flags & NONCANON, "trusted-producer mode is defined on canonical data only"
        acc, dec = decide(P, E, flags, int(coin[b]), R, lnM)
        out.append((wrap64(E), flags | (0 if 0 <= int(coin[b]) < R else COIN), acc, dec))
    return out


# ---- test data (numpy; shared by the CPU and the GPU tier) ---------------------------------------------------------------
def honest(rng, P, B, rows):
    """(z, y) [B][rows][N]: y ~ round(N(0, sigma)), z = centred(y + v) with v uniform in [-vmax, vmax] (|d r|_inf <= vmax)."""
    import numpy as np

    y = np.rint(rng.normal(0.0, P.sigma, (B, rows, P.N))).astype(np.int64)
    v = rng.integers(-P.vmax, P.vmax + 1, (B, rows, P.N), dtype=np.int64)
    z = y + v
    z = np.where(z > P.half, z - P.q, np.where(z < -P.half, z + P.q, z))
    return z, y


def coins(rng, B, R):
    import numpy as np

    return rng.integers(0, R, B, dtype=np.int64)


def norm_edge_poly(P, over):
    """A polynomial with sum c^2 = (verify_bound + 1)^2 - 1 + over: (vb + 1)^2 - 1 = vb^2 + 2 vb, as vb, then 2 vb as a
    greedy sum of squares."""
    import math

    import numpy as np

    z = np.zeros(P.N, np.int64)
    z[0] = P.verify_bound
    rest = 2 * P.verify_bound + over
    i = 1
    while rest:
        c = math.isqrt(rest)
        z[i], rest, i = c, rest - c * c, i + 1
    assert i <= P.N and int((z.astype(object) ** 2).sum()) == (P.verify_bound + 1) ** 2 - 1 + over
    return z


def count_undecidable(results):
    return sum(1 for r in results if not r[3])
