// rzk_dgauss.h — the exact discrete Gaussian sampler D_sigma over the integers, in integer operations alone: the one
// statement of its parameters, of one trial and of its word stream.  Shared by the kernels
// (rzk_csprng_dev.hip), the host side of the entry point (rzk_samplers.cpp: the parameters) and the CPU test
// (tests/test_dgauss_host.py, g++).  Host + device, plain C++; the same function of its words on every machine, so
// tests/dgauss_ref.py (Python integers) is compared with it bit for bit.
//
// The binary-Gaussian rejection sampler of Ducas, Durmus, Lepoint, Lyubashevsky ("Lattice signatures and bimodal
// Gaussians", CRYPTO 2013, Alg. 10-12) for any integer sigma in [1, 2^26], every restart folded into "the trial fails".
//
// Parameters of sigma (integers, computed on the host: dgauss_params)
//   K = floor(2^127 log2 e),  C = K div sigma^2 = floor(2^128 c) for c = log2 e / (2 sigma^2) up to 2^-75 relative,
//   k = the least integer with k^2 C >= 2^128 (k >= sigma sqrt(2 ln 2); k < 2^27),  y_rej = 2^32 mod k
//
// One trial: 8 words w[0..7] -> "reject" or a signed value (dgauss_trial)
//   x   X = w0:w1; m = X W with W = sum_{x=0..7} 2^(49 - x^2); m mod 2^64 < 2^64 mod W fails the trial (Lemire: what
//       remains is exactly uniform, probability of failing < 2^-14); u = m >> 64 in [0, W); x = the number of cumulative
//       sums sum_{i<=x} 2^(49 - i^2) that u has reached, so P(x) = 2^(49 - x^2) / W exactly, x in 0 .. 7
//   y   m = w2 k; m mod 2^32 < y_rej fails the trial; y = m >> 32, exactly uniform in [0, k)
//   z   = k x + y < 2^30
//   E64 = z^2 (C >> 64) + mulhi64(z^2, C mod 2^64) = floor(z^2 C / 2^64);  a = (E64 >> 64) - x^2 >= 0 (by the choice of
//       k), f = E64 mod 2^64: the exponent a + f 2^-64 = z^2 c - x^2 in bits
//   accept with probability 2^-(a + f 2^-64): a >= 64 fails the trial; f = 0 and a = 0 accepts; else w4:w5 < T with
//       T = 2^(64-a) for f = 0 and T = exp2m(f) >> a otherwise (dgauss_threshold)
//   sign, zero   w3 bit 0 is the sign, bit 1 the coin: z = 0 with the coin set fails the trial (0 would otherwise have
//       twice its mass); the value is -z if the sign is set, else z.  w3 bits 2 .. 31, w6 and w7 are not used.
//
// exp2m(f), f in [1, 2^64): 2^64 2^(-f 2^-64) in fixed point.  f = b 2^63 + g: p = c_15; p = c_i - mulhi64(g, p) for
// i = 14 .. 1 (the alternating series of 2^-t, t = g 2^-64 < 1/2: every p stays positive); v = 2^64 - 1 - mulhi64(g, p);
// b set: v = mulhi64(v, R), R = floor(2^64 / sqrt 2).  Coefficients: tools/gen_dgauss_consts.py.
// Error: a Horner step adds at most 1/2 (the coefficient) + 1 (the floor) and halves what it carries, so p_1 is off by
// at most 7/3; v by at most 1 + 1 + 7/6 + 1/26 (series remainder) before and 0.71 3.3 + 1.5 after the product with R;
// the shift by a adds 1; the floor in E64 moves f by 1, the probability by 0.7 2^-a.  In all the acceptance
// probability is within 6 2^-64 of 2^-(z^2 c' - x^2), c' = C 2^-128: eps_B = 2^-61 is the documented bound (the tests
// hold exp2m to it against mpmath).
//
// Stream: trial t of coefficient pair j of polynomial p of a call reads
//   ChaCha20_block(subkey, w12 = 0x80000000 | t << 16 | j, w13 = p & 0xffffffff, w14 = p >> 32, w15 = stream)
// words 0 .. 7 for coefficient 2j, words 8 .. 15 for coefficient 2j + 1 (subkey as in rzk_chacha.h; bit 31 of w12 keeps
// these blocks apart from every other stream's).  A coefficient takes its first accepted trial, t = 0 .. kDgaussTMax - 1,
// and is 0 if there is none: a trial accepts with probability >= 0.40 (sigma = 1: k = 2 against 1.18; 0.68 for large
// sigma), so that happens with probability < 0.6^160 < 2^-117.
#pragma once
#include <stdint.h>

#include "rzk_core.h"

namespace rzk {

constexpr uint32_t kDgaussSigmaMax = 1u << 26;
constexpr uint32_t kDgaussTMax = 160;   // < 2^15: t << 16 stays below bit 31 of w12
constexpr uint64_t kDgaussKHi = 0xb8aa3b295c17f0bbull, kDgaussKLo = 0xbe87fed0691d3e88ull;   // K = floor(2^127 log2 e)
constexpr uint64_t kDgaussW = 880717420568577ull;                                           // sum 2^(49 - x^2)
constexpr uint64_t kDgaussWRej = 117699900706351ull;                                           // 2^64 mod W
constexpr uint64_t kDgaussInvSqrt2 = 0xb504f333f9de6484ull;                                  // floor(2^64 / sqrt 2)

struct DgaussParams {
  uint64_t c_hi, c_lo;   // C = K div sigma^2
  uint32_t k, y_rej;     // y_rej = 2^32 mod k
};

RZK_HD uint64_t dgauss_mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// host only (128-bit division); sigma in [1, 2^26]
inline DgaussParams dgauss_params(uint32_t sigma) {
  typedef unsigned __int128 u128;
  const u128 K = ((u128)kDgaussKHi << 64) | kDgaussKLo;
  const u128 C = K / ((u128)sigma * sigma);
  // k^2 C >= 2^128  <=>  k^2 >= ceil(2^128 / C) = floor((2^128 - 1) / C) + 1 (C does not divide 2^128 unless it is a
  // power of two, and then the formula still holds: (2^128 - 1) div C = 2^128 / C - 1)
  const u128 need = ~(u128)0 / C + 1;   // < 2^54
  uint64_t k = 1;
  while ((u128)k * k < need) k <<= 1;
  for (uint64_t bit = k >> 1; bit; bit >>= 1)
    if ((u128)(k - bit) * (k - bit) >= need) k -= bit;
  DgaussParams p;
  p.c_hi = (uint64_t)(C >> 64), p.c_lo = (uint64_t)C;
  p.k = (uint32_t)k, p.y_rej = (uint32_t)((1ull << 32) % k);
  return p;
}

// 2^64 2^(-f 2^-64) for f in [1, 2^64), within 5 of the real value (the file comment)
RZK_HD uint64_t dgauss_exp2m(uint64_t f) {
  const uint64_t g = f & 0x7fffffffffffffffull;
  uint64_t p = 0x000000000000e1b7ull;
  p = 0x0000000000131496ull - dgauss_mulhi64(g, p);
  p = 0x0000000001816193ull - dgauss_mulhi64(g, p);
  p = 0x000000001c3bd651ull - dgauss_mulhi64(g, p);
  p = 0x00000001e8cac735ull - dgauss_mulhi64(g, p);
  p = 0x0000001e4cf5158cull - dgauss_mulhi64(g, p);
  p = 0x000001b5253d395eull - dgauss_mulhi64(g, p);
  p = 0x0000162c0223a5c8ull - dgauss_mulhi64(g, p);
  p = 0x0000ffe5fe2c4586ull - dgauss_mulhi64(g, p);
  p = 0x000a184897c363c4ull - dgauss_mulhi64(g, p);
  p = 0x005761ff9e299cc4ull - dgauss_mulhi64(g, p);
  p = 0x0276556df749cee5ull - dgauss_mulhi64(g, p);
  p = 0x0e35846b82505fc6ull - dgauss_mulhi64(g, p);
  p = 0x3d7f7bff058b1d51ull - dgauss_mulhi64(g, p);
  p = 0xb17217f7d1cf79acull - dgauss_mulhi64(g, p);
  const uint64_t v = ~dgauss_mulhi64(g, p);
  return (f >> 63) ? dgauss_mulhi64(v, kDgaussInvSqrt2) : v;
}

// acceptance of the exponent a + f 2^-64: 0 = never (a >= 64), 2 = always (a = 0, f = 0), 1 = a word below T accepts
RZK_HD int dgauss_threshold(uint32_t a, uint64_t f, uint64_t& T) {
  T = 0;
  if (a >= 64u) return 0;
  if (f == 0) {
    if (a == 0) return 2;
    T = 1ull << (64u - a);
    return 1;
  }
  T = dgauss_exp2m(f) >> a;
  return 1;
}

// exponent of the candidate z = k x + y: a, f (the file comment)
RZK_HD void dgauss_exponent(const DgaussParams& P, uint32_t x, uint32_t y, uint32_t& a, uint64_t& f) {
  const uint64_t z = (uint64_t)P.k * x + y;
  const uint64_t zz = z * z;                               // < 2^60
  const uint64_t lo = zz * P.c_hi;                         // E64 = zz c_hi + mulhi64(zz, c_lo), as hi:f
  const uint64_t add = dgauss_mulhi64(zz, P.c_lo);
  f = lo + add;
  const uint32_t hi = (uint32_t)dgauss_mulhi64(zz, P.c_hi) + (f < lo ? 1u : 0u);   // < 2^8
  a = hi - x * x;
}

// one trial on the words w0 .. w5 (w6, w7 are not used): true = accepted, value in `out`
RZK_HD bool dgauss_trial(const DgaussParams& P, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t w4, uint32_t w5,
                         int64_t& out) {
  const uint64_t X = ((uint64_t)w0 << 32) | w1;
  const uint64_t u = dgauss_mulhi64(X, kDgaussW);
  bool ok = X * kDgaussW >= kDgaussWRej;
  const uint32_t x = (u >= 562949953421312ull) + (u >= 844424930131968ull) + (u >= 879609302220800ull) +
                     (u >= 880708813848576ull) + (u >= 880717403783168ull) + (u >= 880717420560384ull) +
                     (u >= 880717420568576ull);
  const uint64_t m = (uint64_t)w2 * P.k;
  ok = ok && (uint32_t)m >= P.y_rej;
  const uint32_t y = (uint32_t)(m >> 32);
  uint32_t a;
  uint64_t f, T;
  dgauss_exponent(P, x, y, a, f);
  const int kind = dgauss_threshold(a, f, T);
  const uint64_t r = ((uint64_t)w4 << 32) | w5;
  ok = ok && (kind == 2 || (kind == 1 && r < T));
  const int64_t z = (int64_t)((uint64_t)P.k * x + y);
  ok = ok && !(z == 0 && (w3 & 2u));
  out = (w3 & 1u) ? -z : z;
  return ok;
}

// word 12 of the block of trial t of coefficient pair j
RZK_HD uint32_t dgauss_w12(uint32_t t, uint32_t j) { return 0x80000000u | (t << 16) | j; }

}  // namespace rzk
