// rzk_response_stat_dev.hip — the response rows z = y + r (.) d fused with the rejection statistic.
//   response_stat_kernel<LOGN, TRUSTED, BYTES>   what shift_row_kernel<LOGN, TRUSTED, WaveTeam, BYTES> does for the rows of
//                                 PG_RESPONSE (rzk_row.h: one wavefront per row, four independent wavefronts per workgroup,
//                                 the product as signed rotations of packed bytes or words in LDS, the same grid-stride
//                                 loop under the context's grid cap), and in the epilogue, where the rolled loop holds the
//                                 product sum v, the addend y and z = y + v of GC coefficient pairs in registers, what
//                                 reject_stat_kernel computes from (z, y) read back from memory: S1 = sum z v, S2 = sum v^2,
//                                 the clamped sum z^2 and the |v| <= kappa b test (reject_step_v, rzk_reject.h).  Wave totals
//                                 with the DPP sums of rzk_wave.h; lane 0 stores one RejectPartial per row where
//                                 reject_decide_kernel expects it.  No atomics, no LDS beyond the image, no scratch.
// One-wavefront teams only (N = 512, 1024); every other shape runs the response launch and reject_stat_kernel
// (rzk_protocols.cpp, response_reject).
// The kernel exists for int64_t slabs and, in its packed-byte form, for the 32-bit slabs of DESIGN.md §18 (reported as
// response_stat_kernel<LOGN, TRUSTED, i32>), from one text (rzk_response_stat_kernel.inc).
#include <hip/hip_runtime.h>

#include <string>
#include <type_traits>

#include "rzk_dev.h"
#include "rzk_reject.h"
#include "rzk_rowprog.h"
#include "rzk_launch.h"   // (templates only: this file instantiates none of the kernels it names)

namespace rzk {

namespace {

constexpr int kTeams = 4;   // wavefronts per workgroup, one 8 N-byte image each (ShiftCfg<LOGN, WaveTeam>)

template <class C>
using P2Out = std::conditional_t<sizeof(C) == 8, int4, int2>;   // the store of one result pair: 16 / 8 bytes
__device__ __forceinline__ void store_result_pair(int4* p, int64_t c0, int64_t c1) {
  st_stream(p, make_int4((int32_t)c0, (int32_t)(c0 >> 32), (int32_t)c1, (int32_t)(c1 >> 32)));
}
__device__ __forceinline__ void store_result_pair(int2* p, int64_t c0, int64_t c1) {   // (centred: below 2^31 in magnitude, the cast is exact)
  st_stream(p, make_int2((int32_t)c0, (int32_t)c1));
}

// The kernel's text, once per coefficient width (see the head of rzk_response_stat_kernel.inc).
#define RZK_RS_KERNEL(name) name
#define RZK_RS_COEF int64_t
#define RZK_RS_TEAM WaveTeam
#include "rzk_response_stat_kernel.inc"
#undef RZK_RS_KERNEL
#undef RZK_RS_COEF
#undef RZK_RS_TEAM
#define RZK_RS_KERNEL(name) name##_i32
#define RZK_RS_COEF int32_t
#define RZK_RS_TEAM WaveTeam32
#include "rzk_response_stat_kernel.inc"
#undef RZK_RS_KERNEL
#undef RZK_RS_COEF
#undef RZK_RS_TEAM

template <int LOGN, bool BYTES>
int launch_t(const LaunchCfg& cfg, const RowArgs& a, const Operands& ops, uint32_t ntasks, const ResponseStat& so) {
  // the workgroup of shift_row_kernel<LOGN, ., WaveTeam, BYTES>, so its LDS request and grid cap (shift_launch, rzk_launch.h)
  static_assert(ShiftCfg<LOGN, WaveTeam>::TPB == kTeams && ShiftCfg<LOGN, WaveTeam>::WORDS == ShiftGeo<LOGN, true, 6>::WORDS,
                "response_stat_kernel lays its images out as shift_row_kernel does");
  constexpr ShiftLaunch g = shift_launch<LOGN, WaveTeam, BYTES>();
  const dim3 grid(grid_for(ntasks, cfg.num_cus, kTeams, g.blocks_per_cu)), block(64 * kTeams);
  if (ops.trusted)
    hipLaunchKernelGGL((response_stat_kernel<LOGN, true, BYTES>), grid, block, g.lds, (hipStream_t)cfg.stream, a.prog, ops, a.T, ntasks, so);
  else
    hipLaunchKernelGGL((response_stat_kernel<LOGN, false, BYTES>), grid, block, g.lds, (hipStream_t)cfg.stream, a.prog, ops, a.T, ntasks, so);
  RZK_LAUNCH_CHECK();
  if (cfg.launched)
    *cfg.launched = "response_stat_kernel<" + std::to_string(LOGN) + ", " + tf(ops.trusted) + (BYTES ? "" : ", false") + ">";
  return 0;
}

// the packed-byte form on 32-bit slabs: the sibling's workgroup, LDS request and grid
template <int LOGN>
int launch32_t(const LaunchCfg& cfg, const RowArgs& a, const Operands& ops, uint32_t ntasks, const ResponseStat& so) {
  static_assert(ShiftCfg<LOGN, WaveTeam32>::TPB == kTeams && ShiftCfg<LOGN, WaveTeam32>::WORDS == ShiftGeo<LOGN, true, 6>::WORDS,
                "response_stat_kernel_i32 lays its images out as shift_row_kernel does");
  constexpr ShiftLaunch g = shift_launch<LOGN, WaveTeam32, true>();
  static_assert(g.lds <= 48 * 1024, "below the opt-in for large dynamic LDS");
  const dim3 grid(grid_for(ntasks, cfg.num_cus, kTeams, g.blocks_per_cu)), block(64 * kTeams);
  if (ops.trusted)
    hipLaunchKernelGGL((response_stat_kernel_i32<LOGN, true, true>), grid, block, g.lds, (hipStream_t)cfg.stream, a.prog, ops, a.T, ntasks, so);
  else
    hipLaunchKernelGGL((response_stat_kernel_i32<LOGN, false, true>), grid, block, g.lds, (hipStream_t)cfg.stream, a.prog, ops, a.T, ntasks, so);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = "response_stat_kernel<" + std::to_string(LOGN) + ", " + tf(ops.trusted) + ", " + WaveTeam32::kName + ">";
  return 0;
}

}  // namespace

int launch_response_stat(int logn, const LaunchCfg& cfg, const RowArgs& a, const Operands& ops, uint32_t nrows, uint64_t batch,
                         const ResponseStat& so) {
  uint32_t ntasks;
  if (const int rc = task_count(batch, nrows, ntasks); rc <= 0) return rc;
  switch (logn) {
    case 9: return cfg.shift_bytes ? launch_t<9, true>(cfg, a, ops, ntasks, so) : launch_t<9, false>(cfg, a, ops, ntasks, so);
    case 10: return cfg.shift_bytes ? launch_t<10, true>(cfg, a, ops, ntasks, so) : launch_t<10, false>(cfg, a, ops, ntasks, so);
  }
  return -1;   // two-wavefront teams and small rings: the caller runs the chain (response_stat_fused, rzk_run.cpp)
}

int launch_response_stat32(int logn, const LaunchCfg& cfg, const RowArgs& a, const Operands& ops, uint32_t nrows, uint64_t batch,
                           const ResponseStat& so) {
  uint32_t ntasks;
  if (const int rc = task_count(batch, nrows, ntasks); rc <= 0) return rc;
  if (!cfg.shift_bytes) return -1;   // the packed-byte kernel only
  switch (logn) {
    case 9: return launch32_t<9>(cfg, a, ops, ntasks, so);
    case 10: return launch32_t<10>(cfg, a, ops, ntasks, so);
  }
  return -1;   // every other shape: the caller converts (slab32_native, rzk_slab32.h)
}

}  // namespace rzk
