// rzk_response_stat_dev.hip — the response rows z = y + r (.) d fused with the rejection statistic.
//   response_stat_kernel<LOGN, TRUSTED, BYTES, TM>   what shift_row_kernel<LOGN, TRUSTED, TM, BYTES> does for the rows of
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
// The kernel takes its team last, response_stat_kernel<LOGN, TRUSTED, BYTES, TM>: WaveTeam for int64_t slabs and, in the
// packed-byte form only, WaveTeam32 for the 32-bit slabs of DESIGN.md §18 (reported as response_stat_kernel<LOGN, TRUSTED, i32>;
// DESIGN.md §20, §23).
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

// The coefficient type of the slabs y, r, d, z comes with the team (TeamCoef, rzk_wave.h), as in unit_kernel and
// shift_row_kernel: int64_t for WaveTeam, int32_t for WaveTeam32 (Operands carries addresses).  The operand loads are the
// coefficient-typed load_pairs / operand_ptr / shift_product_bytes of the rotation kernels (rzk_rowprog.h); the addend is one
// 16- / 8-byte ld_stream per pair (CoefPair) with the canonical test of its width (canon_pair); z leaves as one 16- / 8-byte
// non-temporal store per pair.  TM is also the team of the word-image fallback shift_product.  The statistic, the partial
// layout, the flags, the DPP sums and the LDS image do not depend on the width.
template <int LOGN, bool TRUSTED, bool BYTES, class TM>
__global__ void __launch_bounds__(64 * kTeams, (BYTES ? RZK_SHIFT_BYTES_WAVES : 1))
response_stat_kernel(const Program* __restrict__ prog, const Operands ops, const DevTables* __restrict__ Tp, const uint32_t ntasks,
                     const ResponseStat so) {
  using S = ShiftGeo<LOGN, true, 6>;
  using C = typename TeamCoef<TM>::type;   // coefficient type of the slabs
  constexpr int E = S::E;
  constexpr int N = S::N;
  constexpr int LANES = S::LANES;
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int lane = threadIdx.x & (LANES - 1);
  const uint32_t team = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int32_t* slab = reinterpret_cast<int32_t*>(smem) + team * S::WORDS;
  const DevTables& T = *Tp;
  const uint32_t q = T.crt.q;
  const uint32_t nrows = prog->nrows;

  for (uint32_t task = blockIdx.x * kTeams + team; task < ntasks; task += gridDim.x * kTeams) {
    const uint32_t b = task / nrows;
    const uint32_t rowi = task - b * nrows;
    const uint32_t bo = ops.group > 1 ? b / ops.group : b;
    const Row row = prog->rows[rowi];
    const uint32_t qhalf = T.crt.qhalf;
    constexpr bool trusted = TRUSTED;
    bool fault = false;
    {
      uint32_t res[E];
#pragma unroll
      for (int i = 0; i < E; ++i) res[i] = 0;
#pragma unroll 1
      for (uint32_t t = 0; t < row.nterms; ++t) {
        const Term tm = prog->terms[row.term0 + t];
        int32_t a[E];
        uint32_t abad = 0, amx = 0;
        load_pairs<LOGN, 6, C>(a, operand_ptr<C>(ops, tm.a_op, tm.a_off, b, bo, N), lane, qhalf, abad, amx, trusted);
        if (!trusted) fault = fault || canon_fail(abad, amx, qhalf);
        const C* __restrict__ pv = operand_ptr<C>(ops, tm.b_op, tm.b_off, b, bo, N);
        bool done = false;
        if constexpr (BYTES) done = shift_product_bytes<LOGN, C>(res, tm.sign < 0, a, pv, lane, slab, T, fault, trusted);
        if (!done) shift_product<LOGN, true, false, TM, kShiftH, C>(res, false, tm.sign < 0, a, pv, lane, slab, T, fault, trusted);
      }
      // the sums move to the idle image, each thread's pairs in its own 8-byte slots (as shift_row_kernel)
      wave_sync();
      uint2* own = reinterpret_cast<uint2*>(slab) + lane;
#pragma unroll
      for (int g = 0; g < S::G; ++g) own[g * LANES] = make_uint2(res[2 * g], res[2 * g + 1]);
    }
    constexpr int GC = S::G < 4 ? S::G : 4;   // pairs per trip
    uint32_t in_bad = 0, in_mx = 0;
    RejectAcc acc{0, 0, 0, 0};
#pragma unroll 1
    for (int g0 = 0; g0 < S::G; g0 += GC) {
      uint32_t r[2 * GC], vq[2 * GC];   // vq: the product sum mod q, r: with the additions
      const uint2* own = reinterpret_cast<const uint2*>(slab) + lane + g0 * LANES;
#pragma unroll
      for (int g = 0; g < GC; ++g) {
        const uint2 v = own[g * LANES];
        r[2 * g] = vq[2 * g] = v.x, r[2 * g + 1] = vq[2 * g + 1] = v.y;
      }
#pragma unroll 1
      for (uint32_t ai = 0; ai < row.nadds; ++ai) {
        const AddTerm ad = prog->adds[row.add0 + ai];
        using P2 = typename CoefPair<C>::type;
        const P2* __restrict__ p =
            reinterpret_cast<const P2*>(operand_ptr<C>(ops, ad.op & ADD_OP_MASK, ad.off, b, bo, N)) + g0 * LANES + lane;
        int32_t av[2 * GC];
        if (trusted) {
#pragma unroll
          for (int g = 0; g < GC; ++g) {
            const P2 t = ld_stream(p + g * LANES);
            pair_words(t, av[2 * g], av[2 * g + 1]);
          }
        } else {
#pragma unroll
          for (int g = 0; g < GC; ++g) canon_pair(ld_stream(p + g * LANES), qhalf, in_bad, in_mx, av[2 * g], av[2 * g + 1]);
        }
        if (ad.sign >= 0) {
#pragma unroll
          for (int i = 0; i < 2 * GC; ++i) r[i] = addq(r[i], zq_from_centered(av[i], q), q);
        } else {
#pragma unroll
          for (int i = 0; i < 2 * GC; ++i) r[i] = subq(r[i], zq_from_centered(av[i], q), q);
        }
      }
      P2Out<C>* __restrict__ dst =
          reinterpret_cast<P2Out<C>*>(const_cast<C*>(operand_ptr<C>(ops, row.out_op, row.out_off, b, bo, N))) + g0 * LANES + lane;
#pragma unroll
      for (int g = 0; g < GC; ++g) {
        const int64_t c0 = center_from_zq(r[2 * g], T.crt), c1 = center_from_zq(r[2 * g + 1], T.crt);
        store_result_pair(dst + g * LANES, c0, c1);
        // the statistic of the pair (the canonical verdict of y, r and d is wave-uniform and joins the flags below)
        reject_step_v<false>(acc, c0, center_from_zq(vq[2 * g], T.crt), false, so.vmax);
        reject_step_v<false>(acc, c1, center_from_zq(vq[2 * g + 1], T.crt), false, so.vmax);
      }
    }
    const bool noncanon = fault || canon_fail(in_bad, in_mx, qhalf);   // (both false in trusted mode)
    if (noncanon) input_fault(ops, nullptr, bo, lane);
    // a lane's clamped sum z^2 is at most 32 x 2^48 = 2^53: wave_sum_u56 is exact; S2 - 2 S1 is any 64-bit value
    const uint64_t e = wave_sum_u64(reject_e(acc));
    const uint64_t zsq = wave_sum_u56(acc.zsq);
    const uint32_t flags = (noncanon ? (uint32_t)kRejNonCanon : 0u) | (__any(acc.flags & kRejVmax) ? (uint32_t)kRejVmax : 0u);
    if (lane == 0)
      so.part[(size_t)bo * so.rows_total + so.part_off + (b - bo * ops.group) * nrows + rowi] =
          reject_partial(e, zsq, flags, so.norm_limit);
    wave_sync();   // the next task's image overwrites the slots read above
  }
}

// the workgroup, LDS request and grid of shift_row_kernel<LOGN, ., TM, BYTES> (shift_launch, rzk_launch.h)
template <int LOGN, bool BYTES, class TM>
int launch_t(const LaunchCfg& cfg, const RowArgs& a, const Operands& ops, uint32_t ntasks, const ResponseStat& so) {
  static_assert(ShiftCfg<LOGN, TM>::TPB == kTeams && ShiftCfg<LOGN, TM>::WORDS == ShiftGeo<LOGN, true, 6>::WORDS,
                "response_stat_kernel lays its images out as shift_row_kernel does");
  constexpr ShiftLaunch g = shift_launch<LOGN, TM, BYTES>();
  static_assert(g.lds <= 48 * 1024, "below the opt-in for large dynamic LDS");
  const dim3 grid(grid_for(ntasks, cfg.num_cus, kTeams, g.blocks_per_cu)), block(64 * kTeams);
  if (ops.trusted)
    hipLaunchKernelGGL((response_stat_kernel<LOGN, true, BYTES, TM>), grid, block, g.lds, (hipStream_t)cfg.stream, a.prog, ops, a.T, ntasks, so);
  else
    hipLaunchKernelGGL((response_stat_kernel<LOGN, false, BYTES, TM>), grid, block, g.lds, (hipStream_t)cfg.stream, a.prog, ops, a.T, ntasks, so);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) {
    const std::string form = std::is_same<TM, WaveTeam32>::value ? std::string(", ") + TM::kName : BYTES ? "" : ", false";
    *cfg.launched = "response_stat_kernel<" + std::to_string(LOGN) + ", " + tf(ops.trusted) + form + ">";
  }
  return 0;
}

}  // namespace

int launch_response_stat(int logn, const LaunchCfg& cfg, const RowArgs& a, const Operands& ops, uint32_t nrows, uint64_t batch,
                         const ResponseStat& so) {
  uint32_t ntasks;
  if (const int rc = task_count(batch, nrows, ntasks); rc <= 0) return rc;
  switch (logn) {
    case 9: return cfg.shift_bytes ? launch_t<9, true, WaveTeam>(cfg, a, ops, ntasks, so) : launch_t<9, false, WaveTeam>(cfg, a, ops, ntasks, so);
    case 10: return cfg.shift_bytes ? launch_t<10, true, WaveTeam>(cfg, a, ops, ntasks, so) : launch_t<10, false, WaveTeam>(cfg, a, ops, ntasks, so);
  }
  return -1;   // two-wavefront teams and small rings: the caller runs the chain (response_stat_fused, rzk_run.cpp)
}

int launch_response_stat32(int logn, const LaunchCfg& cfg, const RowArgs& a, const Operands& ops, uint32_t nrows, uint64_t batch,
                           const ResponseStat& so) {
  uint32_t ntasks;
  if (const int rc = task_count(batch, nrows, ntasks); rc <= 0) return rc;
  if (!cfg.shift_bytes) return -1;   // the packed-byte kernel only
  switch (logn) {
    case 9: return launch_t<9, true, WaveTeam32>(cfg, a, ops, ntasks, so);
    case 10: return launch_t<10, true, WaveTeam32>(cfg, a, ops, ntasks, so);
  }
  return -1;   // every other shape: the caller converts (slab32_native, rzk_slab32.h)
}

}  // namespace rzk
