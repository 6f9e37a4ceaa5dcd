// rzk_norm.h - the body of the stand-alone norm kernels (norm_kernel, rzk_xform.h; norm_kernel_i32, rzk_slab32_dev.hip).
// Device code only, templates only: a translation unit that includes it gets no kernel by doing so.
#pragma once
#include "rzk_slab32.h"
#include "rzk_wave.h"

namespace rzk {

// One wavefront per proof: all `rows` polynomials must satisfy sum c^2 < limit (= (bound+1)^2),
// i.e. floor(sqrt(sum c^2)) <= bound (src/polynomial.rs:60-73, src/params.rs:105-107).
// The sum is exact: c^2 split into 32-bit halves, accumulated in two 64-bit lane sums.
// C: the coefficient type of the slab.  int32_t takes the canonical test of rzk_slab32.h, one unsigned compare, and
// |c| as a 32-bit value (slab32_abs); sum, limit compare and the three modes are the same code.
template <int LOGN, class C>
__device__ __forceinline__ void norm_rows(const C* __restrict__ v, uint32_t rows, uint64_t limit_hi, uint64_t limit_lo,
                                          uint8_t* __restrict__ ok, uint64_t B, int and_mode, int shift, uint32_t qhalf,
                                          uint32_t* __restrict__ bad_word) {
  using G = Geo<LOGN>;
  constexpr int E = G::E;
  constexpr int N = G::N;
  const int lane = threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (uint64_t b = (uint64_t)blockIdx.x * 4 + wave; b < B; b += (uint64_t)gridDim.x * 4) {
    int good = 1;
    for (uint32_t r = 0; r < rows; ++r) {
      const C* __restrict__ p = v + (b * rows + r) * N;
      uint64_t slo = 0, shi = 0;
      int huge = 0;   // a coefficient outside the centred range: not a ZqI64 value, the predicate fails
#pragma unroll
      for (int e = 0; e < E; ++e) {
        uint64_t al;
        if constexpr (sizeof(C) == 8) {
          const int64_t c = p[G::j_p1(lane, e)];
          const uint64_t a = c < 0 ? 0ull - (uint64_t)c : (uint64_t)c;
          huge |= a > (uint64_t)qhalf;
          al = a & 0xffffffffu;
        } else {
          const int32_t c = p[G::j_p1(lane, e)];
          huge |= !slab32_canonical(c, qhalf);
          al = slab32_abs(c);
        }
        const uint64_t ll = al * al;
        slo += ll & 0xffffffffu;
        shi += ll >> 32;
      }
      slo = wave_sum_u64(slo);
      shi = wave_sum_u64(shi);
      // total = shi * 2^32 + slo  (shi, slo < 2^50)
      const uint64_t t_lo32 = slo & 0xffffffffu;
      const uint64_t mid = shi + (slo >> 32);
      const uint64_t tot_lo = (mid << 32) | t_lo32;
      const uint64_t tot_hi = mid >> 32;
      const int lt = (tot_hi < limit_hi) || (tot_hi == limit_hi && tot_lo < limit_lo);
      const int any_huge = __any(huge);
      good &= lt && !any_huge;
      if (any_huge && bad_word && lane == 0) *bad_word = 1u;
    }
    if (lane == 0) {
      if (and_mode == 0)
        ok[b] = (uint8_t)good;
      else if (and_mode == 1)
        ok[b] = (uint8_t)(ok[b] & good);
      else
        ok[b] = (uint8_t)(ok[b] | (good << shift));
    }
  }
}

}  // namespace rzk
