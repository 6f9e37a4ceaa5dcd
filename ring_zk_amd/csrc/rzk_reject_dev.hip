// rzk_reject_dev.hip — the prover's rejection-sampling step on the device (definition: rzk_reject.h).
// Two launches per call, no atomics, grid-stride loops under the context's grid cap, so results do not depend on the grid:
//   reject_stat_kernel<TRUSTED>   one wavefront per polynomial pair (z, y), four independent wavefronts per workgroup.
//                                 Lane l of trip t loads coefficients 2 (64 t + l), 2 (64 t + l) + 1 of both operands
//                                 as one 16-byte piece each (lane-consecutive: 1 KiB per wave instruction and operand;
//                                 N < 128 leaves lanes idle, N = 4 is one load in two lanes), folds v = z - y, range-
//                                 tests and accumulates S1, S2 and the clamped sum z^2 in 64-bit registers
//                                 (v_mad_i64_i32 / v_mad_u64_u32), reduces the wave with the DPP sums of rzk_wave.h
//                                 and lets lane 0 store one 16-byte RejectPartial per polynomial.  No LDS, no scratch.
//   reject_decide_kernel          one wavefront per proof: the lanes stride over the proof's partials, reduce, and
//                                 lane 0 evaluates the decision in double precision and writes accept[b] and E[b].
#include <hip/hip_runtime.h>

#include <string>

#include "rzk_dev.h"
#include "rzk_reject.h"
#include "rzk_wave.h"

namespace rzk {

namespace {

constexpr uint32_t kWavesPerBlock = 4;
constexpr uint32_t kBlocksPerCu = 8;   // 32 wavefronts per CU: eight per SIMD, what the register count allows

struct Pair16 {   // two consecutive coefficients, loaded as one 16-byte piece
  int64_t c0, c1;
};
__device__ __forceinline__ Pair16 load_pair(const int64_t* p) {
  typedef long v2l __attribute__((ext_vector_type(2)));
  const v2l t = *reinterpret_cast<const v2l*>(p);
  return Pair16{(int64_t)t.x, (int64_t)t.y};
}

__device__ __forceinline__ uint32_t wave_index() {   // wave-uniform, in scalar registers
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
}
__device__ __forceinline__ bool wave_any(bool p) { return __builtin_amdgcn_ballot_w64(p) != 0; }

template <bool TRUSTED>
__global__ void __launch_bounds__(64 * kWavesPerBlock) reject_stat_kernel(RejectParts m, int64_t q, int64_t vmax,
                                                                          uint64_t norm_limit, RejectPartial* __restrict__ part,
                                                                          uint64_t npolys) {
  const uint32_t lane = threadIdx.x & 63u;
  const int64_t half = (q - 1) / 2;
  const uint32_t trips = (m.N + 127u) / 128u;   // 16-byte pieces per lane and operand
  for (uint64_t p = (uint64_t)blockIdx.x * kWavesPerBlock + wave_index(); p < npolys;
       p += (uint64_t)gridDim.x * kWavesPerBlock) {
    const uint64_t b = p / m.rows;
    const uint32_t j = (uint32_t)(p - b * m.rows);
    uint32_t f = 0;
    while (f + 1 < m.nparts && j >= m.first[f + 1]) ++f;
    const uint64_t off = (b * (uint64_t)(m.first[f + 1] - m.first[f]) + (j - m.first[f])) * (uint64_t)m.N;
    const int64_t* z = m.z[f] + off;
    const int64_t* y = m.y[f] + off;
    RejectAcc a{0, 0, 0, 0};
#pragma unroll 4
    for (uint32_t t = 0; t < trips; ++t) {
      const uint32_t c = 2u * (t * 64u + lane);
      if (c < m.N) {   // (N >= 4 is even: a piece never straddles the end)
        const Pair16 zz = load_pair(z + c), yy = load_pair(y + c);
        reject_step<!TRUSTED>(a, zz.c0, yy.c0, q, half, vmax);
        reject_step<!TRUSTED>(a, zz.c1, yy.c1, q, half, vmax);
      }
    }
    // a lane's clamped sum z^2 is at most 32 x 2^48 = 2^53: wave_sum_u56 is exact; S2 - 2 S1 is any 64-bit value
    const uint64_t e = wave_sum_u64(reject_e(a));
    const uint64_t zsq = wave_sum_u56(a.zsq);
    const uint32_t flags = (wave_any(a.flags & kRejNonCanon) ? (uint32_t)kRejNonCanon : 0u) |
                           (wave_any(a.flags & kRejVmax) ? (uint32_t)kRejVmax : 0u);
    if (lane == 0) part[p] = reject_partial(e, zsq, flags, norm_limit);
  }
}

__global__ void __launch_bounds__(64 * kWavesPerBlock) reject_decide_kernel(const RejectPartial* __restrict__ part, uint32_t rows,
                                                                            const int64_t* __restrict__ coin, uint64_t R, double lnM,
                                                                            double two_sigma_sq, uint8_t* accept, int64_t* E,
                                                                            uint32_t* bad_word, uint64_t B) {
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t b = (uint64_t)blockIdx.x * kWavesPerBlock + wave_index(); b < B; b += (uint64_t)gridDim.x * kWavesPerBlock) {
    const RejectPartial* row = part + b * rows;
    uint64_t e = 0;
    uint32_t flags = 0;
    for (uint32_t j = lane; j < rows; j += 64u) {
      const RejectPartial p = row[j];
      e += (uint64_t)p.e;
      flags |= p.flags;
    }
    e = wave_sum_u64(e);
    const bool noncanon = wave_any(flags & kRejNonCanon);
    const bool other = wave_any(flags & (kRejVmax | kRejNorm));
    if (lane == 0) {
      const uint32_t fl = (noncanon ? (uint32_t)kRejNonCanon : 0u) | (other ? (uint32_t)kRejVmax : 0u);
      accept[b] = reject_decide((int64_t)e, fl, coin[b], R, lnM, two_sigma_sq) ? 1 : 0;
      if (E) E[b] = (int64_t)e;
      if (noncanon && bad_word) *bad_word = 1u;   // every writer stores the same value
    }
  }
}

uint64_t capped(uint64_t tasks, int num_cus) {   // workgroups of kWavesPerBlock tasks under the grid cap
  uint64_t blocks = (tasks + kWavesPerBlock - 1) / kWavesPerBlock;
  const uint64_t cap = (uint64_t)num_cus * kBlocksPerCu;
  return blocks < cap ? blocks : cap;
}

}  // namespace

int launch_reject_stat(const LaunchCfg& cfg, const RejectParts& m, int64_t q, uint64_t vmax, uint64_t norm_limit, bool trusted,
                       RejectPartial* part, uint64_t B) {
  const uint64_t npolys = B * m.rows;
  if (npolys == 0) return 0;
  const dim3 grid((unsigned)capped(npolys, cfg.num_cus)), block(64 * kWavesPerBlock);
  if (trusted)
    hipLaunchKernelGGL(reject_stat_kernel<true>, grid, block, 0, (hipStream_t)cfg.stream, m, q, (int64_t)vmax, norm_limit, part, npolys);
  else
    hipLaunchKernelGGL(reject_stat_kernel<false>, grid, block, 0, (hipStream_t)cfg.stream, m, q, (int64_t)vmax, norm_limit, part, npolys);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = trusted ? "reject_stat_kernel<true>" : "reject_stat_kernel<false>";
  return 0;
}

int launch_reject_decide(const LaunchCfg& cfg, const RejectPartial* part, uint32_t rows, const int64_t* coin, uint64_t R,
                         double lnM, double two_sigma_sq, uint8_t* accept, int64_t* E, uint32_t* bad_word, uint64_t B) {
  if (B == 0) return 0;
  hipLaunchKernelGGL(reject_decide_kernel, dim3((unsigned)capped(B, cfg.num_cus)), dim3(64 * kWavesPerBlock), 0,
                     (hipStream_t)cfg.stream, part, rows, coin, R, lnM, two_sigma_sq, accept, E, bad_word, B);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = "reject_decide_kernel";
  return 0;
}

}  // namespace rzk
