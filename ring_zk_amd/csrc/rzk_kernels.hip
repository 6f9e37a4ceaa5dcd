// rzk_kernels.hip — gfx950 (MI355X) kernels of the ring-zk polynomial-ring backend.
//
// Execution model: one 64-lane wavefront owns one polynomial-sized unit of work (one output row of
// one proof, or one transform); workgroups are 4 independent wavefronts (no workgroup barriers),
// each with a private LDS slab of N + N/32 words for the two transpositions of the wave NTT
// (rzk_core.h).  Global accesses are coalesced: coefficient slabs are read/written with lane-
// consecutive 8-byte accesses (512 B per wave instruction), NTT-domain data (resident key, transform
// output) with 16-byte accesses (1 KiB per wave instruction).  No MFMA: the work is 32-bit integer
// modular arithmetic (v_mad_u64_u32 / v_mul_lo_u32), bounded by HBM traffic and integer VALU rate.
//
// One translation unit: the kernels live in family headers, in the order they are defined; this file includes them
// and holds the launchers (the host side of every <<<>>>).  The launch rules of the unit and rotation kernels, which the
// 32-bit slabs and the fused response rows start from translation units of their own, are in rzk_launch.h.
#include <hip/hip_runtime.h>

#include <string>

#include "rzk_wave.h"
#include "rzk_rowprog.h"
#include "rzk_unit.h"
#include "rzk_row.h"
#include "rzk_group.h"
#include "rzk_xform.h"
#include "rzk_sample.h"
#include "rzk_launch.h"

namespace rzk {

// =============================================================================================
// Launchers
// =============================================================================================
size_t row_scratch_words(int logn, int num_cus) { return (size_t)num_cus * 8 * 4 * (((size_t)kScratchLines << logn) + 16); }

int launch_rows(int logn, const LaunchCfg& cfg, const RowArgs& a, const Operands& ops, uint32_t nrows, bool has_shift, uint64_t batch,
                bool has_dd) {
  uint32_t ntasks;
  if (const int rc = task_count(batch, nrows, ntasks); rc <= 0) return rc;
  if (has_dd && !has_shift) {   // rows whose operand transforms may come from the call's operand images (TERM_DD)
    switch (logn) {
      case 9: return launch_rows_t<9, false, WaveTeam, true>(cfg, a, ops, ntasks);
      case 10: return launch_rows_t<10, false, WaveTeam, true>(cfg, a, ops, ntasks);
      case 11:
        return cfg.pair_poly ? launch_rows_t<11, false, PairTeam, true>(cfg, a, ops, ntasks)
                             : launch_rows_t<11, false, WaveTeam, true>(cfg, a, ops, ntasks);
    }
    return -1;
  }
  switch (logn) {
    case 9: return has_shift ? launch_rows_t<9, true>(cfg, a, ops, ntasks) : launch_rows_t<9, false>(cfg, a, ops, ntasks);
    case 10: return has_shift ? launch_rows_t<10, true>(cfg, a, ops, ntasks) : launch_rows_t<10, false>(cfg, a, ops, ntasks);
    case 11:   // rotation terms at N = 2048: teams of two only (rzk_run.cpp, shift_ok)
      if (has_shift) return cfg.pair_poly ? launch_rows_t<11, true, PairTeam>(cfg, a, ops, ntasks) : -1;
      return cfg.pair_poly ? launch_rows_t<11, false, PairTeam>(cfg, a, ops, ntasks) : launch_rows_t<11, false>(cfg, a, ops, ntasks);
  }
  return -1;
}

int launch_units(int logn, const LaunchCfg& cfg, const RowArgs& a, const Operands& ops, const UnitShape& u, uint64_t batch) {
  UnitTasks t;
  if (const int rc = unit_tasks(u, batch, t); rc <= 0) return rc;
  const bool pair = logn == 11 && cfg.pair_poly;
  if (logn == 11 && u.has_shift && !pair) return -1;   // rotation terms at N = 2048: teams of two only (rzk_run.cpp, shift_ok)
  if (!u.has_vec && cfg.unit_io && !(logn == 11 && u.has_shift)) {   // key-product programs: every operand read once (unit_io_kernel)
    switch (logn) {
      case 9: return with_flag(u.has_shift, [&](auto S) { return launch_units_io_t<9, S>(cfg, a, ops, t); });
      case 10: return with_flag(u.has_shift, [&](auto S) { return launch_units_io_t<10, S>(cfg, a, ops, t); });
      case 11: return pair ? launch_units_io_t<11, false, PairTeam>(cfg, a, ops, t) : launch_units_io_t<11, false>(cfg, a, ops, t);
    }
    return -1;
  }
  return with_flag(u.has_vec, [&](auto V) {
    return with_flag(u.has_shift, [&](auto S) -> int {
      constexpr bool kVec = decltype(V)::value;
      switch (logn) {
        case 9: return launch_units_t<9, kVec, S>(cfg, a, ops, t);
        case 10:   // twiddles from LDS (RZK_TW_LDS): N = 1024, one-wavefront teams; 1: phase 2, 2: phases 2 and 3 on sixteen-team workgroups
          if (cfg.tw_lds >= 2) return launch_units_t<10, kVec, S, WaveTeamTw3>(cfg, a, ops, t);
          return cfg.tw_lds ? launch_units_t<10, kVec, S, WaveTeamTw>(cfg, a, ops, t) : launch_units_t<10, kVec, S>(cfg, a, ops, t);
        case 11:
          if (pair) return launch_units_t<11, kVec, S, PairTeam>(cfg, a, ops, t);
          if constexpr (!S) return launch_units_t<11, kVec, false>(cfg, a, ops, t);   // (one wavefront: no rotation terms, above)
      }
      return -1;
    });
  });
}

template <int LOGN>
static int launch_dkey_t(const LaunchCfg& cfg, const int64_t* g, uint64_t count, uint32_t dkey_n, uint32_t* img, double* l2,
                         const DevTables* T, const uint32_t* d_tw, uint8_t* d_flags, uint32_t* d_bad, bool two_bit, bool trusted) {
  using G = Geo<LOGN>;
  hipLaunchKernelGGL(dkey_transform_kernel<LOGN>, dim3(grid_for(count, cfg.num_cus)), dim3(256), 4 * G::LDS_WORDS * sizeof(uint32_t),
                     (hipStream_t)cfg.stream, g, count, dkey_n, img, l2, T, d_tw, d_flags, d_bad, two_bit ? 1u : 0u,
                     trusted ? 1u : 0u);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = "dkey_transform_kernel<" + std::to_string(LOGN) + ">";
  return 0;
}
int launch_dkey_transform(int logn, const LaunchCfg& cfg, const int64_t* g, uint64_t count, uint32_t dkey_n, uint32_t* img,
                          double* l2, const DevTables* T, const uint32_t* d_tw, uint8_t* d_flags, uint32_t* d_bad, bool two_bit,
                          bool trusted) {
  if (count == 0) return 0;
  return with_logn(logn,
                   [&](auto L) { return launch_dkey_t<L>(cfg, g, count, dkey_n, img, l2, T, d_tw, d_flags, d_bad, two_bit, trusted); });
}

int launch_shift_rows(int logn, const LaunchCfg& cfg, const RowArgs& a, const Operands& ops, uint32_t nrows, uint64_t batch) {
  uint32_t ntasks;
  if (const int rc = task_count(batch, nrows, ntasks); rc <= 0) return rc;
  switch (logn) {
    case 9: return cfg.shift_bytes ? launch_shift_t<9>(cfg, a, ops, ntasks) : launch_shift_t<9, WaveTeam, false>(cfg, a, ops, ntasks);
    case 10: return cfg.shift_bytes ? launch_shift_t<10>(cfg, a, ops, ntasks) : launch_shift_t<10, WaveTeam, false>(cfg, a, ops, ntasks);
    case 11: return cfg.pair_poly ? launch_shift_t<11, PairTeam>(cfg, a, ops, ntasks) : -1;   // (rzk_run.cpp, shift_ok)
  }
  return -1;
}

size_t group_scratch_words(int logn, int num_cus) {
  return (size_t)num_cus * 8 * 4 * (size_t)(2 * kGroupMax) * ((size_t)1 << logn);
}

template <int LOGN>
static int launch_groups_t(const LaunchCfg& cfg, const RowArgs& a, const Operands& ops, uint32_t ntasks) {
  using G = Geo<LOGN>;
  constexpr int GM = group_accumulators(LOGN);   // accumulators per wave (N = 2048 is never grouped by the host)
  hipLaunchKernelGGL((row_group_kernel<LOGN, GM>), dim3(grid_for(ntasks, cfg.num_cus)), dim3(256),
                     4 * G::LDS_WORDS * sizeof(uint32_t), (hipStream_t)cfg.stream, a.prog, ops, a.key_ntt, a.key_l2, a.T,
                     a.tw, a.scratch, a.flags, ntasks);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = "row_group_kernel<" + std::to_string(LOGN) + ", " + std::to_string(GM) + ">";
  return 0;
}

int launch_row_groups(int logn, const LaunchCfg& cfg, const RowArgs& a, const Operands& ops, uint32_t ngroups, uint64_t batch) {
  uint32_t ntasks;
  if (const int rc = task_count(batch, ngroups, ntasks); rc <= 0) return rc;
  return with_logn(logn, [&](auto L) { return launch_groups_t<L>(cfg, a, ops, ntasks); });
}

size_t block_scratch_words(int logn, int num_cus) {
  return (size_t)num_cus * 2 * (size_t)(2 * kBlockMaxRows) * ((size_t)1 << logn);
}

template <int LOGN, class TM = WaveTeam>
static int launch_blocks_t(const LaunchCfg& cfg, const RowArgs& a, const Operands& ops, const BlockPlan* d_plan, uint32_t ntasks) {
  using G = Geo<LOGN, TM::LL>;
  const size_t lds = ((size_t)kBlockMaxSlots * G::N + (size_t)kBlockWaves * G::LDS_WORDS) * sizeof(uint32_t) +
                     kBlockMaxSlots * sizeof(double);
  // > 64 KiB of dynamic LDS needs an explicit opt-in.  The attribute is kept per device and contexts may live on
  // several devices / host threads, so it is set (idempotently, a host-side call of ~1 us) before every launch
  // rather than behind a process-wide "done" flag.
  {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&row_block_kernel<LOGN, TM>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  uint32_t grid = ntasks < (uint32_t)cfg.num_cus * 2 ? ntasks : (uint32_t)cfg.num_cus * 2;   // scratch: num_cus * 2 lines
  hipLaunchKernelGGL((row_block_kernel<LOGN, TM>), dim3(grid), dim3(kBlockWaves << TM::LL), lds, (hipStream_t)cfg.stream, a.prog,
                     d_plan, ops, a.key_ntt, a.key_l2, a.T, a.tw, a.scratch, a.flags, ntasks);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = "row_block_kernel<" + std::to_string(LOGN) + team_arg<TM>() + ">";
  return 0;
}

int launch_row_blocks(int logn, const LaunchCfg& cfg, const RowArgs& a, const Operands& ops, const BlockPlan* d_plan, uint32_t nblocks,
                      uint64_t batch) {
  uint32_t ntasks;
  if (const int rc = task_count(batch, nblocks, ntasks); rc <= 0) return rc;
  switch (logn) {
    case 10: return launch_blocks_t<10>(cfg, a, ops, d_plan, ntasks);
    case 11:
      if (cfg.pair_poly)   // eight two-wavefront teams: 16 coefficients per thread, 4 waves per SIMD beside 138 KiB of LDS
        return launch_blocks_t<11, BlockPairTeam>(cfg, a, ops, d_plan, ntasks);
      return launch_blocks_t<11>(cfg, a, ops, d_plan, ntasks);
  }
  return -1;
}

template <int LOGN>
static int launch_slots_t(const LaunchCfg& cfg, const RowArgs& a, const Operands& ops, const SlotTable* d_slots, uint32_t nslots,
                          const SlotStore& st, uint32_t batch) {
  using G = Geo<LOGN>;
  const uint32_t ftasks = batch * nslots;
  hipLaunchKernelGGL(fwd_slots_kernel<LOGN>, dim3(grid_for(ftasks, cfg.num_cus)), dim3(256),
                     4 * G::LDS_WORDS * sizeof(uint32_t), (hipStream_t)cfg.stream, d_slots, ops, a.T, a.tw, st.ws, st.norms,
                     a.flags, ftasks, st.np_store);
  RZK_LAUNCH_CHECK();
  unsigned grid = (unsigned)cfg.num_cus * 8;   // multiple of 8: the XCD-class dealing needs whole classes
  grid -= grid % 8;
  hipLaunchKernelGGL(row_slots_kernel<LOGN>, dim3(grid), dim3(256), 4 * (G::LDS_WORDS + G::N) * sizeof(uint32_t),
                     (hipStream_t)cfg.stream, a.prog, d_slots, ops, a.key_ntt, a.key_l2, a.T, a.tw, st.ws, st.norms,
                     a.scratch, a.flags, batch, st.np_store);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = "fwd_slots_kernel<" + std::to_string(LOGN) + "> + row_slots_kernel<" + std::to_string(LOGN) + ">";
  return 0;
}

int launch_row_program_slots(int logn, const LaunchCfg& cfg, const RowArgs& a, const Operands& ops, const SlotTable* d_slots,
                             uint32_t nslots, const SlotStore& st, uint64_t batch) {
  if (batch == 0) return 0;   // (not task_count: two launches, and the rows run even without slots)
  if (batch * nslots >= (1ull << 32) || batch >= (1ull << 31)) return -2;
  return with_logn(logn, [&](auto L) { return launch_slots_t<L>(cfg, a, ops, d_slots, nslots, st, (uint32_t)batch); });
}

template <int LOGN>
static int launch_key_t(const LaunchCfg& cfg, const int64_t* d_key, uint32_t entries, uint32_t* d_key_ntt,
                        const DevTables* T, const uint32_t* d_tw) {
  using G = Geo<LOGN>;
  const size_t lds = 4 * G::LDS_WORDS * sizeof(uint32_t);
  const unsigned grid = grid_for((uint64_t)entries * kKeyImages, cfg.num_cus);
  hipLaunchKernelGGL(key_transform_kernel<LOGN>, dim3(grid), dim3(256), lds, (hipStream_t)cfg.stream,
                     d_key, entries, d_key_ntt, T, d_tw);
  RZK_LAUNCH_CHECK();
  return 0;
}

int launch_key_transform(int logn, const LaunchCfg& cfg, const int64_t* d_key, uint32_t entries,
                         uint32_t* d_key_ntt, const DevTables* T, const uint32_t* d_tw) {
  if (entries == 0) return 0;
  return with_logn(logn, [&](auto L) { return launch_key_t<L>(cfg, d_key, entries, d_key_ntt, T, d_tw); });
}

template <int LOGN>
static int launch_ntt_t(bool inverse, const LaunchCfg& cfg, int prime, const uint32_t* d_in, uint32_t* d_out,
                        uint64_t count, const DevTables* T, const uint32_t* d_tw) {
  using G = Geo<LOGN>;
  const size_t lds = 4 * G::LDS_WORDS * sizeof(uint32_t);
  const unsigned grid = grid_for(count, cfg.num_cus);
  if (inverse)
    hipLaunchKernelGGL(ntt_inv_kernel<LOGN>, dim3(grid), dim3(256), lds, (hipStream_t)cfg.stream, d_in,
                       d_out, count, prime, T, d_tw);
  else
    hipLaunchKernelGGL(ntt_fwd_kernel<LOGN>, dim3(grid), dim3(256), lds, (hipStream_t)cfg.stream, d_in,
                       d_out, count, prime, T, d_tw);
  RZK_LAUNCH_CHECK();
  return 0;
}

int launch_ntt(int logn, bool inverse, const LaunchCfg& cfg, int prime, const uint32_t* d_in,
               uint32_t* d_out, uint64_t count, const DevTables* T, const uint32_t* d_tw) {
  if (count == 0) return 0;
  return with_logn(logn, [&](auto L) { return launch_ntt_t<L>(inverse, cfg, prime, d_in, d_out, count, T, d_tw); });
}

// flags[i] = value: one small launch (hipMemsetAsync's fill kernel takes ~4.5 us for 4 KiB on this stack)
__global__ void __launch_bounds__(256) fill_u8_kernel(uint8_t* __restrict__ p, uint8_t value, uint64_t n) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) p[i] = value;
}
int launch_fill_u8(const LaunchCfg& cfg, uint8_t* p, uint8_t value, uint64_t n) {
  if (n == 0) return 0;
  uint64_t blocks = (n + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(fill_u8_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)cfg.stream, p, value, n);
  RZK_LAUNCH_CHECK();
  return 0;
}

static inline uint32_t log2_u32(uint32_t v) {
  uint32_t l = 0;
  while ((1u << l) < v) ++l;
  return l;
}
int launch_sample_uniform(const LaunchCfg& cfg, int64_t* out, uint64_t npoly, uint32_t n_ring, uint64_t seed,
                          uint32_t stream, uint32_t bound) {
  if (npoly == 0) return 0;
  if (n_ring < 2 || (n_ring & (n_ring - 1))) return -1;
  const uint64_t ncoef = npoly * n_ring;
  hipLaunchKernelGGL(sample_uniform_kernel, dim3(grid_for((ncoef + 1) / 2, cfg.num_cus, 256, 16)), dim3(256), 0,
                     (hipStream_t)cfg.stream, out, ncoef, log2_u32(n_ring), seed, stream, bound);
  RZK_LAUNCH_CHECK();
  return 0;
}
int launch_sample_gauss(const LaunchCfg& cfg, int64_t* out, uint64_t npoly, uint32_t n_ring, uint64_t seed,
                        uint32_t stream, double sigma) {
  if (npoly == 0) return 0;
  if (n_ring < 2 || (n_ring & (n_ring - 1))) return -1;
  const uint64_t ncoef = npoly * n_ring;
  const dim3 grid(grid_for((ncoef + 1) / 2, cfg.num_cus, 256, 16));
  if (sigma < 524288.0)   // 9.4 sigma < 2^23: single precision carries every sample within the bound of rzk_gauss.h
    hipLaunchKernelGGL(sample_gauss_kernel<true>, grid, dim3(256), 0, (hipStream_t)cfg.stream, out, ncoef, log2_u32(n_ring), seed,
                       stream, sigma);
  else
    hipLaunchKernelGGL(sample_gauss_kernel<false>, grid, dim3(256), 0, (hipStream_t)cfg.stream, out, ncoef, log2_u32(n_ring), seed,
                       stream, sigma);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = sigma < 524288.0 ? "sample_gauss_kernel<true>" : "sample_gauss_kernel<false>";
  return 0;
}
int launch_debug_gauss_map(const LaunchCfg& cfg, bool f32, const uint32_t* words, double sigma, int64_t* out, uint64_t pairs) {
  if (pairs == 0) return 0;
  const dim3 grid(grid_for(pairs, cfg.num_cus, 256, 16));
  if (f32)
    hipLaunchKernelGGL(debug_gauss_map_kernel<true>, grid, dim3(256), 0, (hipStream_t)cfg.stream, words, out, pairs, sigma);
  else
    hipLaunchKernelGGL(debug_gauss_map_kernel<false>, grid, dim3(256), 0, (hipStream_t)cfg.stream, words, out, pairs, sigma);
  RZK_LAUNCH_CHECK();
  return 0;
}
int launch_sample_challenge(const LaunchCfg& cfg, int64_t* out, uint64_t npoly, uint32_t n_ring, uint64_t seed,
                            uint32_t stream, uint32_t kappa) {
  if (npoly == 0) return 0;
  hipLaunchKernelGGL(sample_challenge_kernel, dim3(grid_for(npoly, cfg.num_cus, 4, 16)), dim3(256), 4 * n_ring,
                     (hipStream_t)cfg.stream, out, npoly, n_ring, seed, stream, kappa);
  RZK_LAUNCH_CHECK();
  return 0;
}

// any int64 -> centred representative mod q (utility for data that does not come from a ZqI64: the hot kernels
// assume canonical inputs and read only the low word of every coefficient)
__global__ void __launch_bounds__(256) canonicalize_kernel(const int64_t* __restrict__ in, int64_t* __restrict__ out,
                                                          uint64_t ncoef, int64_t q) {
  const int64_t half = (q - 1) / 2;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < ncoef; i += (uint64_t)gridDim.x * 256) {
    int64_t r = in[i] % q;          // sign of the dividend, |r| < q
    if (r > half) r -= q;
    if (r < -half) r += q;
    out[i] = r;
  }
}
int launch_canonicalize(const LaunchCfg& cfg, const int64_t* in, int64_t* out, uint64_t ncoef, int64_t q) {
  if (ncoef == 0) return 0;
  uint64_t blocks = (ncoef + 255) / 256;
  const uint64_t cap = (uint64_t)cfg.num_cus * 32;
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(canonicalize_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)cfg.stream, in, out, ncoef, q);
  RZK_LAUNCH_CHECK();
  return 0;
}

int launch_addsub(const LaunchCfg& cfg, bool sub, const int64_t* a, const int64_t* b, int64_t* out,
                  uint64_t ncoef, const DevTables* T, uint32_t* bad_word) {
  if (ncoef == 0) return 0;
  const uint64_t n2 = ncoef / 2;   // ncoef is a multiple of N >= 512
  uint64_t blocks = (n2 + 255) / 256;
  const uint64_t cap = (uint64_t)cfg.num_cus * 8;
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(addsub_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)cfg.stream, a, b,
                     out, n2, sub ? 1 : 0, T, bad_word);
  RZK_LAUNCH_CHECK();
  return 0;
}

int launch_norm(int logn, const LaunchCfg& cfg, const int64_t* v, uint32_t rows, uint64_t limit_hi,
                uint64_t limit_lo, uint8_t* ok, uint64_t B, int and_mode, int shift, uint32_t qhalf,
                uint32_t* bad_word) {
  if (B == 0) return 0;
  const unsigned grid = grid_for(B, cfg.num_cus);
  const int rc = with_logn(logn, [&](auto L) {
    hipLaunchKernelGGL(norm_kernel<L>, dim3(grid), dim3(256), 0, (hipStream_t)cfg.stream, v, rows,
                       limit_hi, limit_lo, ok, B, and_mode, shift, qhalf, bad_word);
    return 0;
  });
  if (rc != 0) return rc;
  RZK_LAUNCH_CHECK();
  return 0;
}

int launch_eq(int logn, const LaunchCfg& cfg, const int64_t* a, const int64_t* b, uint32_t rows,
              uint8_t* eq, uint64_t B, uint32_t qhalf, uint32_t* bad_word) {
  if (B == 0) return 0;
  const unsigned grid = grid_for(B, cfg.num_cus);
  const int rc = with_logn(logn, [&](auto L) {
    hipLaunchKernelGGL(eq_kernel<L>, dim3(grid), dim3(256), 0, (hipStream_t)cfg.stream, a, b, rows, eq, B, qhalf,
                       bad_word);
    return 0;
  });
  if (rc != 0) return rc;
  RZK_LAUNCH_CHECK();
  return 0;
}

// ---- small ring degrees ------------------------------------------------------------------------------------------
int launch_row_program_small(uint32_t N, const LaunchCfg& cfg, const Program* d_prog, uint32_t nrows,
                             const Operands& ops, const uint32_t* d_key_mont, const DevTables* T, uint32_t r2q,
                             uint8_t* d_flags, uint64_t batch) {
  uint32_t ntasks;
  if (const int rc = task_count(batch, nrows, ntasks); rc <= 0) return rc;
  const unsigned grid = grid_for(ntasks, cfg.num_cus);
  hipLaunchKernelGGL(row_kernel_small, dim3(grid), dim3(256), 4 * 2 * N * sizeof(uint32_t), (hipStream_t)cfg.stream,
                     d_prog, ops, d_key_mont, T, d_flags, ntasks, N, r2q);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = "row_kernel_small";
  return 0;
}

int launch_key_mont(const LaunchCfg& cfg, const int64_t* d_key, uint32_t* d_key_mont, uint64_t ncoef,
                    const DevTables* T, uint32_t r2q) {
  if (ncoef == 0) return 0;
  uint64_t blocks = (ncoef + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(key_mont_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)cfg.stream, d_key,
                     d_key_mont, ncoef, T, r2q);
  RZK_LAUNCH_CHECK();
  return 0;
}

int launch_norm_small(uint32_t N, const LaunchCfg& cfg, const int64_t* v, uint32_t rows, uint64_t limit_hi,
                      uint64_t limit_lo, uint8_t* ok, uint64_t B, int and_mode, int shift, uint32_t qhalf,
                      uint32_t* bad_word) {
  if (B == 0) return 0;
  hipLaunchKernelGGL(norm_kernel_small, dim3(grid_for(B, cfg.num_cus)), dim3(256), 0, (hipStream_t)cfg.stream, v,
                     rows, limit_hi, limit_lo, ok, B, and_mode, shift, N, qhalf, bad_word);
  RZK_LAUNCH_CHECK();
  return 0;
}

int launch_eq_small(uint32_t N, const LaunchCfg& cfg, const int64_t* a, const int64_t* b, uint32_t rows,
                    uint8_t* eq, uint64_t B, uint32_t qhalf, uint32_t* bad_word) {
  if (B == 0) return 0;
  hipLaunchKernelGGL(eq_kernel_small, dim3(grid_for(B, cfg.num_cus)), dim3(256), 0, (hipStream_t)cfg.stream, a, b,
                     rows, eq, B, N, qhalf, bad_word);
  RZK_LAUNCH_CHECK();
  return 0;
}

}  // namespace rzk
