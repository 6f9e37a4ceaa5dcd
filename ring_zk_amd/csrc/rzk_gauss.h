// rzk_gauss.h — the word-to-pair map of the Gaussian samplers: Box-Muller from four 32-bit words to two coefficients.
// One statement for both generators: sample_gauss_kernel (rzk_sample.h) feeds it the four words of a Philox block,
// sample_gauss_chacha_kernel (rzk_csprng_dev.hip) quarter i = w[4i .. 4i+3] of a ChaCha20 block (rzk_chacha.h), and
// debug_gauss_map_kernel (rzk_sample.h) words chosen by the caller.  Host + device, plain C++: the host side is what
// tests/test_chacha.py compiles with g++ (libm instead of the device intrinsics).
//
// The definition (tests/gauss_ref.py states it in extended precision), before the truncation toward zero:
//   F32 (sigma < 2^19)  X = w0:w1 (0 is taken as 1), lz = clz(X), top = the 24 leading bits of X << lz,
//                       u0 = top 2^-(24+lz) — only those 24 bits count;  a = float(w2) 2^-31 half turns — the rounding
//                       of w2 to 24 bits (nearest even) counts, w2 = 2^32 - 1 gives a full turn;
//                       R = float(sigma) sqrt(-2 ln u0);  (v0, v1) = (R cos pi a, R sin pi a)
//   F64                 u0 = ((w0:w1 >> 11) + 1) 2^-53 in (0, 1],  u1 = (w2:w3 >> 11) 2^-53 in [0, 1),
//                       R = sigma sqrt(-2 ln u0);  (v0, v1) = (R cos 2 pi u1, R sin 2 pi u1)
// Error of a sample before the truncation, against that definition:
//   F32  < 2^-24 (1.4 sigma^2 / max(R, 2^-24 sigma) + 16 R).  The first term is the logarithm: log2 u0 is formed as
//        log2(m) - (lz + 1) with m = top 2^-23 in [1, 2), and one ulp of log2f on [0.5, 1) — 2^-24 absolute — moves R by
//        0.69 2^-24 sigma^2 / R.  It dominates where u0 is close to 1 (lz = 0, m close to 2: the difference cancels, a
//        radius far below sigma, probability about 1e-5): there a sample can be off by 0.47 at sigma = 21780.  The
//        second term is half an ulp each for the subtraction, the product with 2 ln 2, the square root, the product with
//        sigma and the final product, and 2 ulp for sincospif: about 8 2^-24 R.  Both constants carry a factor 2 over
//        that count.  At sigma = 21780 and a typical radius this is 0.02; in the tail (R = 8 sigma) 0.17.
//   F64  < 2^-50 max(R, 1).
// The ulp figures of the device intrinsics are those of the ROCm documentation; tests/test_gpu_gauss_pin.py holds the
// kernels to these bounds coefficient by coefficient.
#pragma once
#include <math.h>
#include <stdint.h>

#include "rzk_core.h"

namespace rzk {

// single precision (sigma < 2^19): the radius from the 64-bit uniform w0:w1 through exponent + log2 of the 24-bit
// mantissa, the angle from w2.  The conversion truncates toward zero, like I::from_f64.
RZK_HD void gauss_pair_f32(uint32_t w0, uint32_t w1, uint32_t w2, float sigf, int64_t& v0, int64_t& v1) {
  uint64_t X = ((uint64_t)w0 << 32) | w1;   // u0 = X 2^-64 (X = 0, probability 2^-64, is taken as 1)
  X = X ? X : 1ull;
  const int lz = __builtin_clzll(X);
  const uint32_t top = (uint32_t)((X << lz) >> 40);            // 24 bits, top bit set
  const float m = (float)top * (1.0f / 8388608.0f);            // exact: [1, 2)
  float sn, cs;
#if defined(__HIP_DEVICE_COMPILE__)
  const float l2 = __log2f(m) - (float)(lz + 1);               // log2 u0 <= -2^-24 (m = 2 - 2^-23, lz = 0)
  const float r = sigf * __fsqrt_rn(-1.3862943611198906f * l2);   // sigma sqrt(-2 ln u0)
  sincospif((float)w2 * (2.0f / 4294967296.0f), &sn, &cs);     // angle 2 pi u1, in half turns
#else
  const float l2 = log2f(m) - (float)(lz + 1);
  const float r = sigf * sqrtf(-1.3862943611198906f * l2);
  const float ang = (float)w2 * (2.0f / 4294967296.0f);
  sn = sinf(3.14159265358979323846f * ang), cs = cosf(3.14159265358979323846f * ang);
#endif
  v0 = (int64_t)(r * cs);
  v1 = (int64_t)(r * sn);
}

// the double-precision form (sigma up to 2^26, whose samples need more than 24 bits): 53-bit uniforms from w0:w1, w2:w3
RZK_HD void gauss_pair_f64(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, double sigma, int64_t& v0, int64_t& v1) {
  const double k = 1.0 / 9007199254740992.0;   // 2^-53: u0 in (0, 1]
  const double u0 = ((double)((((uint64_t)w0 << 32) | w1) >> 11) + 1.0) * k;
  const double u1 = (double)((((uint64_t)w2 << 32) | w3) >> 11) * k;
  const double r0 = sigma * sqrt(-2.0 * log(u0));
  double s0, c0;
#if defined(__HIP_DEVICE_COMPILE__)
  sincospi(2.0 * u1, &s0, &c0);
#else
  s0 = sin(6.283185307179586476925 * u1), c0 = cos(6.283185307179586476925 * u1);
#endif
  v0 = (int64_t)(r0 * c0);
  v1 = (int64_t)(r0 * s0);
}

}  // namespace rzk
