#!/usr/bin/env python3
"""Constants of the exact discrete Gaussian sampler (ring_zk_amd/csrc/rzk_dgauss.h), from Python integers
alone: no floating point, no library.  Prints the literals that the header and tests/dgauss_ref.py carry.

    K      = floor(2^127 log2 e)
    W      = sum over x = 0 .. 7 of 2^(49 - x^2), and the cumulative sums behind the 7 compares
    c_i    = round(2^64 (ln 2)^i / i!), i = 1 .. 15: 2^-t = sum c_i (-t)^i on t in [0, 1/2)
    R      = floor(2^64 / sqrt 2)

ln 2 = sum over k >= 1 of 1 / (k 2^k), summed in 320-bit fixed point (truncation of each term: < 2^-310 in all)."""
from math import isqrt

PREC = 320
DEGREE = 15


def ln2_fixed():
    one, s, k = 1 << PREC, 0, 1
    while (one >> k) // k:
        s += (one >> k) // k
        k += 1
    return s


def main():
    ln2 = ln2_fixed()
    one = 1 << PREC
    print("K      = 0x%x" % ((one << 127) // ln2))                       # log2 e = 1 / ln 2
    cum, acc = [], 0
    for x in range(8):
        acc += 1 << (49 - x * x)
        cum.append(acc)
    print("W      = %d" % acc)
    print("cum    = " + ", ".join("%dull" % c for c in cum[:7]))
    power, fact = one, 1
    coef = []
    for i in range(1, DEGREE + 1):
        power = power * ln2 >> PREC
        fact *= i
        coef.append(((power << 64) // fact + (one >> 1)) >> PREC)        # round to nearest
    print("c[1..] = " + ", ".join("0x%016xull" % c for c in coef))
    print("R      = 0x%016xull" % isqrt(1 << 127))
    # remainder of the degree-15 series on t < 1/2: (ln 2 / 2)^16 / 16!, in units of 2^-64
    power = power * ln2 >> PREC
    print("series remainder, units of 2^-64: < 1 / %d" % (((fact * (DEGREE + 1)) << (DEGREE + 1)) * one // (power << 64)))


if __name__ == "__main__":
    main()
