// rzk_reject.h — the prover's rejection-sampling step (BDLOP, eprint 2016/997, Fig. 2; Lyubashevsky 2012, Thm 4.6;
// DESIGN.md §12), shared by the GPU kernels (rzk_reject_dev.hip), the entry points (rzk_codec.cpp: the argument rules)
// and the CPU test (tests/test_reject_host.py, g++).  Plain C++.
//
// A response z = y + v, v = d r, is released only with probability min(1, D_sigma(z) / (M D_{v,sigma}(z))) =
// min(1, exp((|v|^2 - 2 <z, v>) / (2 sigma^2)) / M).  The step, fixed to the bit:
//   per coefficient   v  = centred((z - y) mod q)         z - y lies in (-q, q): one conditional add or subtract
//   per proof         S1 = sum z v,  S2 = sum v^2,  E = S2 - 2 S1   exact integers over all rows and coefficients;
//                     what is stored is E mod 2^64 as an int64, which IS E whenever no fail flag is set (argument
//                     rule below) and in every flagged case with |E| < 2^63
//   fail              a z or y coefficient outside [-(q-1)/2, (q-1)/2]      (kRejNonCanon; skipped by trusted producers)
//                     | some |v| > vmax = kappa b, the honest bound on |d r|_inf               (kRejVmax)
//                     | a z polynomial with sum c^2 >= (verify_bound + 1)^2                     (kRejNorm)
//                     | coin outside [0, R)                                                     (kRejCoin)
//   accept            !fail && (double)E >= 2 sigma^2 (lnM + log((coin + 1) / R))   evaluated in double precision:
//                     coin / R < min(1, exp(E / 2 sigma^2) / M) in the log domain, coin uniform in [0, R)
// Argument rule (the entry points return RZK_E_ARG otherwise): rows N 2^24 vmax < 2^52.  An unflagged proof has
// |z| <= verify_bound < 2^24 and |v| <= vmax, so |S1| and S2 stay below 2^52 and |E| below 2^53: (double)E is exact.
// The norm test clamps |c| to 2^24 before squaring (as the fused norm predicate does, rzk_wave.h): a polynomial's sum
// stays below 2^59 and is exact whenever it is below 2^48 >= (verify_bound + 1)^2, hence the verdict is exact.
#pragma once
#include <math.h>
#include <stdint.h>

#include "rzk_core.h"

namespace rzk {

enum : uint32_t { kRejNonCanon = 1u, kRejVmax = 2u, kRejNorm = 4u, kRejCoin = 8u };
constexpr int kRejectMaxParts = 4;
constexpr uint64_t kRejectMaxR = 1ull << 62;

// M = exp(12 / alpha + 1 / (2 alpha^2)) for sigma = alpha |v| (Lyubashevsky 2012, Thm 4.6 with |<z,v>| < 12 sigma |v|)
RZK_HD double reject_lnm(double alpha) { return 12.0 / alpha + 1.0 / (2.0 * alpha * alpha); }

// rows N 2^24 vmax < 2^52 (and verify_bound + 1 <= 2^24, which the clamp of the norm test needs)
RZK_HD bool reject_args_ok(uint64_t rows, uint32_t N, uint64_t vmax, uint64_t verify_bound) {
  if (rows == 0 || rows > (1ull << 28) || vmax >= (1ull << 28) || verify_bound >= (1ull << 24)) return false;
  const uint64_t rn = rows * (uint64_t)N;   // < 2^40
  return vmax == 0 || rn < ((1ull << 28) + vmax - 1) / vmax;   // rn vmax < 2^28
}

struct RejectAcc {   // running sums of one lane / one polynomial; all arithmetic wraps mod 2^64
  uint64_t s1, s2, zsq;
  uint32_t flags;
};

// One coefficient pair.  CHECK = false: trusted producer, no canonical test.  The products take the low 32 bits of
// z and v as signed factors (v_mad_i64_i32 on the device): exact for canonical data, where |z|, |v| <= (q-1)/2 < 2^31.
template <bool CHECK>
RZK_HD void reject_step(RejectAcc& a, int64_t z, int64_t y, int64_t q, int64_t half, int64_t vmax) {
  if (CHECK && (z > half || z < -half || y > half || y < -half)) a.flags |= kRejNonCanon;
  int64_t v = (int64_t)((uint64_t)z - (uint64_t)y);
  if (v > half) v -= q;
  else if (v < -half) v += q;
  if (v > vmax || v < -vmax) a.flags |= kRejVmax;
  const int32_t zl = (int32_t)(uint32_t)(uint64_t)z, vl = (int32_t)(uint32_t)(uint64_t)v;
  a.s1 += (uint64_t)((int64_t)zl * vl);
  a.s2 += (uint64_t)((int64_t)vl * vl);
  uint32_t m = zl < 0 ? 0u - (uint32_t)zl : (uint32_t)zl;
  m = m < (1u << 24) ? m : (1u << 24);
  a.zsq += (uint64_t)m * m;
}

// The same step for a producer that still holds v: the response rows fused with the statistic (rzk_response_stat_dev.hip,
// DESIGN.md §17) have the centred product sum v = d r and the centred z = y + v in registers and take both from there
// instead of deriving v from z - y.  For a canonical y, centred((z - y) mod q) IS the centred product sum, so the two
// steps add the same s1, s2, zsq and flags; z is canonical by construction, y_noncanon is the producer's own test of y
// (and of the other coefficients it loaded), vmax as above.
template <bool CHECK>
RZK_HD void reject_step_v(RejectAcc& a, int64_t z, int64_t v, bool y_noncanon, int64_t vmax) {
  if (CHECK && y_noncanon) a.flags |= kRejNonCanon;
  if (v > vmax || v < -vmax) a.flags |= kRejVmax;
  const int32_t zl = (int32_t)(uint32_t)(uint64_t)z, vl = (int32_t)(uint32_t)(uint64_t)v;
  a.s1 += (uint64_t)((int64_t)zl * vl);
  a.s2 += (uint64_t)((int64_t)vl * vl);
  uint32_t m = zl < 0 ? 0u - (uint32_t)zl : (uint32_t)zl;
  m = m < (1u << 24) ? m : (1u << 24);
  a.zsq += (uint64_t)m * m;
}

// what one polynomial hands to the decision: e = S2 - 2 S1 of its coefficients, flags with the norm verdict folded in
struct alignas(16) RejectPartial {
  int64_t e;
  uint32_t flags, pad;
};
RZK_HD uint64_t reject_e(const RejectAcc& a) { return a.s2 - 2 * a.s1; }
// e, zsq, flags: the polynomial's totals of reject_e, RejectAcc::zsq and RejectAcc::flags; norm_limit = (verify_bound + 1)^2
RZK_HD RejectPartial reject_partial(uint64_t e, uint64_t zsq, uint32_t flags, uint64_t norm_limit) {
  RejectPartial p;
  p.e = (int64_t)e;
  p.flags = flags | (zsq < norm_limit ? 0u : kRejNorm);
  p.pad = 0;
  return p;
}

RZK_HD uint32_t reject_coin_flags(int64_t coin, uint64_t R) { return coin >= 0 && (uint64_t)coin < R ? 0u : kRejCoin; }

// the decision of one proof from E, the flags of all its polynomials and its coin; two_sigma_sq = 2 sigma^2 < 2^53
RZK_HD bool reject_decide(int64_t E, uint32_t flags, int64_t coin, uint64_t R, double lnM, double two_sigma_sq) {
  if (flags | reject_coin_flags(coin, R)) return false;
  const double u = (double)((uint64_t)coin + 1) / (double)R;
  return (double)E >= two_sigma_sq * (lnM + log(u));
}

}  // namespace rzk
