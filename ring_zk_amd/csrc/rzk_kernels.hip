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
// and holds the launchers (the host side of every <<<>>>).
#include <hip/hip_runtime.h>

#include <string>
#include <type_traits>

#include "rzk_wave.h"
#include "rzk_rowprog.h"
#include "rzk_unit.h"
#include "rzk_row.h"
#include "rzk_group.h"
#include "rzk_xform.h"
#include "rzk_sample.h"

namespace rzk {

// =============================================================================================
// Launchers
// =============================================================================================
static inline unsigned grid_for(uint64_t tasks, int num_cus, int waves_per_block = 4, int blocks_per_cu = 8) {
  uint64_t blocks = (tasks + waves_per_block - 1) / waves_per_block;
  const uint64_t cap = (uint64_t)num_cus * blocks_per_cu;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  return (unsigned)blocks;
}

#define RZK_LAUNCH_CHECK()                      \
  do {                                          \
    hipError_t e_ = hipGetLastError();          \
    if (e_ != hipSuccess) return (int)e_;       \
  } while (0)

// f(std::integral_constant<int, LOGN>) for the ring degrees the transform kernels are compiled for
template <class F>
static int with_logn(int logn, F&& f) {
  switch (logn) {
    case 9: return f(std::integral_constant<int, 9>{});
    case 10: return f(std::integral_constant<int, 10>{});
    case 11: return f(std::integral_constant<int, 11>{});
  }
  return -1;
}

// The launchers of the row-program kernels report which instantiation they started (LaunchCfg::launched, read back
// through rzk_prof_read_kernels): its name as a profiler prints it, without "void rzk::" and the argument list.  Tests,
// bench.py and tools/pmc_traffic.py match these strings, so they keep their habits: a default WaveTeam is left out
// (team_arg) by every kernel but row_kernel, which always names its team.
static const char* tf(bool v) { return v ? "true" : "false"; }
template <class TM>
static std::string team_arg() {   // (the teams with the twiddle image report as the teams they derive from)
  return std::is_same<TM, WaveTeam>::value || std::is_same<TM, WaveTeamTw>::value ? std::string() : std::string(", ") + TM::kName;
}

size_t row_scratch_words(int logn, int num_cus) { return (size_t)num_cus * 8 * 4 * (((size_t)kScratchLines << logn) + 16); }

// LDS words of one team in unit_kernel / row_kernel: transposition slab + one N-word buffer; a rotation term's image
// (2N words) fits inside that, the non-zero list of a two-wavefront team comes on top.  Teams with the phase-2 twiddles in
// LDS (TeamTwLds) share one set of images per workgroup behind the teams' buffers: block_tw_words.
template <int LOGN, class TM, bool HAS_SHIFT>
constexpr size_t team_lds_words() {
  using G = Geo<LOGN, TM::LL>;
  constexpr size_t base = G::LDS_WORDS + G::N;
  constexpr size_t rot = (HAS_SHIFT && TM::LL != 6) ? 2 * (size_t)G::N + kShiftListWords : 0;
  static_assert(!(HAS_SHIFT && TM::LL != 6) || TM::kTeamsPerBlock == 1, "the list lies behind the team's own buffers");
  return (((base > rot ? base : rot) + 3) / 4) * 4;
}

template <int LOGN, class TM>
constexpr size_t block_tw_words() {
  return TeamTwLds<TM>::value ? (size_t)Tw2Img<LOGN, TM::LL>::TABLES * Tw2Img<LOGN, TM::LL>::WORDS : 0;
}
// N = 1024, four one-wavefront teams: 4 x 8 320 + 6 144 = 39 424 bytes, four workgroups (4 waves per SIMD) in 157 696 of the
// CU's 163 840
static_assert(4 * (WaveTeamTw::kTeamsPerBlock * team_lds_words<10, WaveTeamTw, true>() + block_tw_words<10, WaveTeamTw>()) * sizeof(uint32_t) <= 160 * 1024,
              "the twiddle images must leave room for four workgroups per CU");

template <int LOGN, bool HAS_VEC, bool HAS_SHIFT, class TM = WaveTeam>
static int launch_units_t(const LaunchCfg& cfg, const Program* d_prog, const WaveProgram* d_wp, const Operands& ops,
                          const uint32_t* d_key_ntt, const double* d_key_l2, const DevTables* T, const uint32_t* d_tw,
                          uint32_t* d_scratch, uint8_t* d_flags, uint32_t ntasks, uint32_t upt, uint32_t tpe, uint32_t wpt) {
  using G = Geo<LOGN, TM::LL>;
  constexpr int TPB = TM::kTeamsPerBlock;
  // per team: transposition slab + P; per workgroup: the twiddle images
  const size_t lds = (TPB * team_lds_words<LOGN, TM, HAS_SHIFT>() + block_tw_words<LOGN, TM>()) * sizeof(uint32_t);
  static_assert(!TeamTwLds<TM>::value || team_lds_words<LOGN, TM, HAS_SHIFT>() == (size_t)(G::LDS_WORDS + G::N),
                "unit_kernel puts the images right behind the teams' slab + P");
  if (lds > 48 * 1024) {   // large dynamic LDS needs an opt-in; per device, so set before every launch (cheap, idempotent)
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&unit_kernel<LOGN, HAS_VEC, HAS_SHIFT, TM>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  // scratch sizing: at most num_cus * 32 team lines; every team walks its tasks with a grid stride
  const unsigned grid = grid_for(ntasks, cfg.num_cus, TPB, TM::LL == 6 ? 32 / TPB : 8);
  hipLaunchKernelGGL((unit_kernel<LOGN, HAS_VEC, HAS_SHIFT, TM>), dim3(grid), dim3(TPB << TM::LL), lds, (hipStream_t)cfg.stream,
                     d_prog, d_wp, ops, d_key_ntt, d_key_l2, T, d_tw, d_scratch, d_flags, ntasks, upt, tpe, wpt);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = "unit_kernel<" + std::to_string(LOGN) + ", " + tf(HAS_VEC) + ", " + tf(HAS_SHIFT) + team_arg<TM>() + ">";
  return 0;
}

template <int LOGN, bool HAS_SHIFT, class TM = WaveTeam>
static int launch_units_io_t(const LaunchCfg& cfg, const Program* d_prog, const WaveProgram* d_wp, const Operands& ops,
                             const uint32_t* d_key_ntt, const double* d_key_l2, const DevTables* T, const uint32_t* d_tw,
                             uint32_t* d_scratch, uint8_t* d_flags, uint32_t ntasks, uint32_t upt, uint32_t tpe, uint32_t wpt) {
  using G = Geo<LOGN, TM::LL>;
  constexpr int TPB = TM::kTeamsPerBlock;
  const size_t lds = TPB * (size_t)IoCfg<LOGN, TM::LL>::WORDS * sizeof(uint32_t);   // per team: slab + parking buffers
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&unit_io_kernel<LOGN, HAS_SHIFT, TM>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  const unsigned grid = grid_for(ntasks, cfg.num_cus, TPB, TM::LL == 6 ? 32 / TPB : 8);
  hipLaunchKernelGGL((unit_io_kernel<LOGN, HAS_SHIFT, TM>), dim3(grid), dim3(TPB << TM::LL), lds, (hipStream_t)cfg.stream,
                     d_prog, d_wp, ops, d_key_ntt, d_key_l2, T, d_tw, d_scratch, d_flags, ntasks, upt, tpe, wpt);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = "unit_io_kernel<" + std::to_string(LOGN) + ", " + tf(HAS_SHIFT) + team_arg<TM>() + ">";
  return 0;
}

template <int LOGN, bool HAS_SHIFT, class TM = WaveTeam, bool DD = false>
static int launch_rows_t(const LaunchCfg& cfg, const Program* d_prog, const Operands& ops, const uint32_t* d_key_ntt,
                         const double* d_key_l2, const DevTables* T, const uint32_t* d_tw, uint32_t* d_scratch,
                         uint8_t* d_flags, uint32_t ntasks) {
  using G = Geo<LOGN, TM::LL>;
  constexpr int TPB = TM::kTeamsPerBlock;
  const size_t lds = TPB * team_lds_words<LOGN, TM, HAS_SHIFT>() * sizeof(uint32_t);   // per team: transposition slab + state word A
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&row_kernel<LOGN, HAS_SHIFT, TM, DD>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  const unsigned grid = grid_for(ntasks, cfg.num_cus, TPB, TM::LL == 6 ? 32 / TPB : 8);   // <= 32 team lines per CU (scratch sizing)
  hipLaunchKernelGGL((row_kernel<LOGN, HAS_SHIFT, TM, DD>), dim3(grid), dim3(TPB << TM::LL), lds, (hipStream_t)cfg.stream, d_prog, ops,
                     d_key_ntt, d_key_l2, T, d_tw, d_scratch, d_flags, ntasks);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = "row_kernel<" + std::to_string(LOGN) + ", " + tf(HAS_SHIFT) + ", " + TM::kName + ", " + tf(DD) + ">";
  return 0;
}

int launch_rows(int logn, const LaunchCfg& cfg, const Program* d_prog, uint32_t nrows, bool has_shift, const Operands& ops,
                const uint32_t* d_key_ntt, const double* d_key_l2, const DevTables* T, const uint32_t* d_tw,
                uint32_t* d_scratch, uint8_t* d_flags, uint64_t batch, bool has_dd) {
  if (batch == 0 || nrows == 0) return 0;
  if (batch * nrows >= (1ull << 32)) return -2;
  const uint32_t ntasks = (uint32_t)(batch * nrows);
#define RZK_ROWS_ARGS cfg, d_prog, ops, d_key_ntt, d_key_l2, T, d_tw, d_scratch, d_flags, ntasks
  if (has_dd && !has_shift) {   // rows whose operand transforms may come from the call's operand images (TERM_DD)
    switch (logn) {
      case 9: return launch_rows_t<9, false, WaveTeam, true>(RZK_ROWS_ARGS);
      case 10: return launch_rows_t<10, false, WaveTeam, true>(RZK_ROWS_ARGS);
      case 11: return cfg.pair_poly ? launch_rows_t<11, false, PairTeam, true>(RZK_ROWS_ARGS) : launch_rows_t<11, false, WaveTeam, true>(RZK_ROWS_ARGS);
    }
    return -1;
  }
  switch (logn) {
    case 9: return has_shift ? launch_rows_t<9, true>(RZK_ROWS_ARGS) : launch_rows_t<9, false>(RZK_ROWS_ARGS);
    case 10: return has_shift ? launch_rows_t<10, true>(RZK_ROWS_ARGS) : launch_rows_t<10, false>(RZK_ROWS_ARGS);
    case 11:   // rotation terms at N = 2048: teams of two only (rzk_api.cpp, shift_ok)
      if (has_shift) return cfg.pair_poly ? launch_rows_t<11, true, PairTeam>(RZK_ROWS_ARGS) : -1;
      return cfg.pair_poly ? launch_rows_t<11, false, PairTeam>(RZK_ROWS_ARGS) : launch_rows_t<11, false>(RZK_ROWS_ARGS);
  }
#undef RZK_ROWS_ARGS
  return -1;
}

int launch_units(int logn, const LaunchCfg& cfg, const Program* d_prog, const WaveProgram* d_wp, uint32_t nunits,
                 uint32_t units_per_task, uint32_t work_per_entry, bool has_vec, bool has_shift, const Operands& ops,
                 const uint32_t* d_key_ntt, const double* d_key_l2, const DevTables* T, const uint32_t* d_tw,
                 uint32_t* d_scratch, uint8_t* d_flags, uint64_t batch) {
  if (batch == 0 || nunits == 0) return 0;
  if (units_per_task == 0) units_per_task = 1;
  const uint32_t tpe = (nunits + units_per_task - 1) / units_per_task;   // tasks per batch entry
  if (batch * tpe >= (1ull << 32)) return -2;   // task index is 32-bit
  const uint32_t ntasks = (uint32_t)(batch * tpe);
  const uint32_t wpt = (work_per_entry + tpe - 1) / tpe;   // transforms per task (estimate, for the progress priorities)
#define RZK_UNIT_ARGS cfg, d_prog, d_wp, ops, d_key_ntt, d_key_l2, T, d_tw, d_scratch, d_flags, ntasks, units_per_task, tpe, wpt
  if (!has_vec && cfg.unit_io && !(logn == 11 && has_shift)) {   // key-product programs: every operand read once (unit_io_kernel)
    switch (logn) {
      case 9: return has_shift ? launch_units_io_t<9, true>(RZK_UNIT_ARGS) : launch_units_io_t<9, false>(RZK_UNIT_ARGS);
      case 10: return has_shift ? launch_units_io_t<10, true>(RZK_UNIT_ARGS) : launch_units_io_t<10, false>(RZK_UNIT_ARGS);
      case 11:
        if (has_shift) return -1;
        return cfg.pair_poly ? launch_units_io_t<11, false, PairTeam>(RZK_UNIT_ARGS) : launch_units_io_t<11, false>(RZK_UNIT_ARGS);
    }
    return -1;
  }
  if (logn == 10 && cfg.tw_lds) {   // phase-2 twiddles from LDS (RZK_TW_LDS): N = 1024, one-wavefront teams
    if (has_shift)
      return has_vec ? launch_units_t<10, true, true, WaveTeamTw>(RZK_UNIT_ARGS) : launch_units_t<10, false, true, WaveTeamTw>(RZK_UNIT_ARGS);
    return has_vec ? launch_units_t<10, true, false, WaveTeamTw>(RZK_UNIT_ARGS) : launch_units_t<10, false, false, WaveTeamTw>(RZK_UNIT_ARGS);
  }
#define RZK_UNIT_CASE(L)                                                                                            \
  case L:                                                                                                           \
    if (has_shift)                                                                                                  \
      return has_vec ? launch_units_t<L, true, true>(RZK_UNIT_ARGS) : launch_units_t<L, false, true>(RZK_UNIT_ARGS); \
    return has_vec ? launch_units_t<L, true, false>(RZK_UNIT_ARGS) : launch_units_t<L, false, false>(RZK_UNIT_ARGS);
  switch (logn) {
    RZK_UNIT_CASE(9)
    RZK_UNIT_CASE(10)
    case 11:   // rotation terms at N = 2048: teams of two only (rzk_api.cpp, shift_ok)
      if (has_shift) {
        if (!cfg.pair_poly) return -1;
        return has_vec ? launch_units_t<11, true, true, PairTeam>(RZK_UNIT_ARGS) : launch_units_t<11, false, true, PairTeam>(RZK_UNIT_ARGS);
      }
      if (cfg.pair_poly)
        return has_vec ? launch_units_t<11, true, false, PairTeam>(RZK_UNIT_ARGS) : launch_units_t<11, false, false, PairTeam>(RZK_UNIT_ARGS);
      return has_vec ? launch_units_t<11, true, false>(RZK_UNIT_ARGS) : launch_units_t<11, false, false>(RZK_UNIT_ARGS);
  }
#undef RZK_UNIT_ARGS
#undef RZK_UNIT_CASE
  return -1;
}

template <int LOGN, class TM = WaveTeam, bool BYTES = (TM::LL == 6)>
static int launch_shift_t(const LaunchCfg& cfg, const Program* d_prog, const Operands& ops, const DevTables* T,
                          uint8_t* d_flags, uint32_t ntasks) {
  constexpr int TPB = ShiftCfg<LOGN, TM>::TPB;
  static_assert(!BYTES || TM::LL == 6, "packed-byte rotations: one wavefront per polynomial");
  // One team's image is 8 N bytes.  The workgroup asks for at least 40 KiB so that a CU holds four workgroups = 4 waves per
  // SIMD: with the 79 VGPRs the kernel needs, five or six would fit, and measured slower (response rows at N = 1024:
  // 86.7 us against 77.5 us at four — the kernel is co-bound by the LDS pipe, more waves only add contention).
  // Teams of two (N = 2048): 18 KiB per 128-thread workgroup, eight workgroups = 4 waves per SIMD.
  // BYTES: the packed image is 3 N bytes, but a term that fails the condition still builds the word image, so the request
  // stays at 8 N bytes per team.  The floor stays too while the kernel is compiled for four waves per SIMD
  // (RZK_SHIFT_BYTES_WAVES, rzk_row.h: at five it needs 96 VGPRs and spills; measured no gain).
  size_t lds = (size_t)TPB * ShiftCfg<LOGN, TM>::WORDS * sizeof(uint32_t);
  if ((!BYTES || RZK_SHIFT_BYTES_WAVES < 5) && TM::LL == 6 && LOGN >= 10 && lds < 40 * 1024) lds = 40 * 1024;   // (N = 512 keeps its 6 waves per SIMD: 4-KiB images, measured fine in round 2)
  const void* fn = ops.trusted ? reinterpret_cast<const void*>(&shift_row_kernel<LOGN, true, TM, BYTES>)
                               : reinterpret_cast<const void*>(&shift_row_kernel<LOGN, false, TM, BYTES>);
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  const unsigned grid = grid_for(ntasks, cfg.num_cus, TPB, TM::LL == 6 ? 16 : 64);
  if (ops.trusted)
    hipLaunchKernelGGL((shift_row_kernel<LOGN, true, TM, BYTES>), dim3(grid), dim3(TPB << TM::LL), lds, (hipStream_t)cfg.stream, d_prog,
                       ops, T, d_flags, ntasks);
  else
    hipLaunchKernelGGL((shift_row_kernel<LOGN, false, TM, BYTES>), dim3(grid), dim3(TPB << TM::LL), lds, (hipStream_t)cfg.stream, d_prog,
                       ops, T, d_flags, ntasks);
  RZK_LAUNCH_CHECK();
  // template defaults are left out, as everywhere: BYTES defaults to "one wavefront per polynomial", so the short name is
  // the packed-byte kernel at N <= 1024 and the word kernel of the two-wavefront teams; RZK_SHIFT_BYTES=0 spells it out
  constexpr bool kDefault = BYTES == (TM::LL == 6);
  if (cfg.launched)
    *cfg.launched = "shift_row_kernel<" + std::to_string(LOGN) + ", " + tf(ops.trusted) +
                    (kDefault ? team_arg<TM>() : std::string(", ") + TM::kName + ", " + tf(BYTES)) + ">";
  return 0;
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

int launch_shift_rows(int logn, const LaunchCfg& cfg, const Program* d_prog, uint32_t nrows, const Operands& ops,
                      const DevTables* T, uint8_t* d_flags, uint64_t batch) {
  if (batch == 0 || nrows == 0) return 0;
  if (batch * nrows >= (1ull << 32)) return -2;
  const uint32_t ntasks = (uint32_t)(batch * nrows);
  switch (logn) {
    case 9:
      return cfg.shift_bytes ? launch_shift_t<9>(cfg, d_prog, ops, T, d_flags, ntasks)
                             : launch_shift_t<9, WaveTeam, false>(cfg, d_prog, ops, T, d_flags, ntasks);
    case 10:
      return cfg.shift_bytes ? launch_shift_t<10>(cfg, d_prog, ops, T, d_flags, ntasks)
                             : launch_shift_t<10, WaveTeam, false>(cfg, d_prog, ops, T, d_flags, ntasks);
    case 11: return cfg.pair_poly ? launch_shift_t<11, PairTeam>(cfg, d_prog, ops, T, d_flags, ntasks) : -1;   // (rzk_api.cpp, shift_ok)
  }
  return -1;
}

size_t group_scratch_words(int logn, int num_cus) {
  return (size_t)num_cus * 8 * 4 * (size_t)(2 * kGroupMax) * ((size_t)1 << logn);
}

template <int LOGN>
static int launch_groups_t(const LaunchCfg& cfg, const Program* d_prog, const Operands& ops, const uint32_t* d_key_ntt,
                           const double* d_key_l2, const DevTables* T, const uint32_t* d_tw, uint32_t* d_scratch,
                           uint8_t* d_flags, uint32_t ntasks) {
  using G = Geo<LOGN>;
  constexpr int GM = group_accumulators(LOGN);   // accumulators per wave (N = 2048 is never grouped by the host)
  hipLaunchKernelGGL((row_group_kernel<LOGN, GM>), dim3(grid_for(ntasks, cfg.num_cus)), dim3(256),
                     4 * G::LDS_WORDS * sizeof(uint32_t), (hipStream_t)cfg.stream, d_prog, ops, d_key_ntt, d_key_l2, T,
                     d_tw, d_scratch, d_flags, ntasks);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = "row_group_kernel<" + std::to_string(LOGN) + ", " + std::to_string(GM) + ">";
  return 0;
}

int launch_row_groups(int logn, const LaunchCfg& cfg, const Program* d_prog, uint32_t ngroups, const Operands& ops,
                      const uint32_t* d_key_ntt, const double* d_key_l2, const DevTables* T, const uint32_t* d_tw,
                      uint32_t* d_scratch, uint8_t* d_flags, uint64_t batch) {
  if (batch == 0 || ngroups == 0) return 0;
  if (batch * ngroups >= (1ull << 32)) return -2;
  const uint32_t ntasks = (uint32_t)(batch * ngroups);
  return with_logn(logn,
                   [&](auto L) { return launch_groups_t<L>(cfg, d_prog, ops, d_key_ntt, d_key_l2, T, d_tw, d_scratch, d_flags, ntasks); });
}

size_t block_scratch_words(int logn, int num_cus) {
  return (size_t)num_cus * 2 * (size_t)(2 * kBlockMaxRows) * ((size_t)1 << logn);
}

template <int LOGN, class TM = WaveTeam>
static int launch_blocks_t(const LaunchCfg& cfg, const Program* d_prog, const BlockPlan* d_plan, const Operands& ops,
                           const uint32_t* d_key_ntt, const double* d_key_l2, const DevTables* T, const uint32_t* d_tw,
                           uint32_t* d_scratch, uint8_t* d_flags, uint32_t ntasks) {
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
  hipLaunchKernelGGL((row_block_kernel<LOGN, TM>), dim3(grid), dim3(kBlockWaves << TM::LL), lds, (hipStream_t)cfg.stream, d_prog,
                     d_plan, ops, d_key_ntt, d_key_l2, T, d_tw, d_scratch, d_flags, ntasks);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = "row_block_kernel<" + std::to_string(LOGN) + team_arg<TM>() + ">";
  return 0;
}

int launch_row_blocks(int logn, const LaunchCfg& cfg, const Program* d_prog, const BlockPlan* d_plan, uint32_t nblocks,
                      const Operands& ops, const uint32_t* d_key_ntt, const double* d_key_l2, const DevTables* T,
                      const uint32_t* d_tw, uint32_t* d_scratch, uint8_t* d_flags, uint64_t batch) {
  if (batch == 0 || nblocks == 0) return 0;
  if (batch * nblocks >= (1ull << 32)) return -2;
  const uint32_t ntasks = (uint32_t)(batch * nblocks);
  switch (logn) {
    case 10: return launch_blocks_t<10>(cfg, d_prog, d_plan, ops, d_key_ntt, d_key_l2, T, d_tw, d_scratch, d_flags, ntasks);
    case 11:
      if (cfg.pair_poly)   // eight two-wavefront teams: 16 coefficients per thread, 4 waves per SIMD beside 138 KiB of LDS
        return launch_blocks_t<11, BlockPairTeam>(cfg, d_prog, d_plan, ops, d_key_ntt, d_key_l2, T, d_tw, d_scratch, d_flags, ntasks);
      return launch_blocks_t<11>(cfg, d_prog, d_plan, ops, d_key_ntt, d_key_l2, T, d_tw, d_scratch, d_flags, ntasks);
  }
  return -1;
}

template <int LOGN>
static int launch_slots_t(const LaunchCfg& cfg, const Program* d_prog, const SlotTable* d_slots, uint32_t nslots,
                          const Operands& ops, const uint32_t* d_key_ntt, const double* d_key_l2, const DevTables* T,
                          const uint32_t* d_tw, uint32_t* d_ws, double* d_norms, uint32_t* d_scratch, uint8_t* d_flags,
                          uint32_t batch, uint32_t np_store) {
  using G = Geo<LOGN>;
  const uint32_t ftasks = batch * nslots;
  hipLaunchKernelGGL(fwd_slots_kernel<LOGN>, dim3(grid_for(ftasks, cfg.num_cus)), dim3(256),
                     4 * G::LDS_WORDS * sizeof(uint32_t), (hipStream_t)cfg.stream, d_slots, ops, T, d_tw, d_ws, d_norms,
                     d_flags, ftasks, np_store);
  RZK_LAUNCH_CHECK();
  unsigned grid = (unsigned)cfg.num_cus * 8;   // multiple of 8: the XCD-class dealing needs whole classes
  grid -= grid % 8;
  hipLaunchKernelGGL(row_slots_kernel<LOGN>, dim3(grid), dim3(256), 4 * (G::LDS_WORDS + G::N) * sizeof(uint32_t),
                     (hipStream_t)cfg.stream, d_prog, d_slots, ops, d_key_ntt, d_key_l2, T, d_tw, d_ws, d_norms,
                     d_scratch, d_flags, batch, np_store);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = "fwd_slots_kernel<" + std::to_string(LOGN) + "> + row_slots_kernel<" + std::to_string(LOGN) + ">";
  return 0;
}

int launch_row_program_slots(int logn, const LaunchCfg& cfg, const Program* d_prog, const SlotTable* d_slots,
                             uint32_t nslots, const Operands& ops, const uint32_t* d_key_ntt,
                             const double* d_key_l2, const DevTables* T, const uint32_t* d_tw, uint32_t* d_ws,
                             double* d_norms, uint32_t* d_scratch, uint8_t* d_flags, uint64_t batch,
                             uint32_t np_store) {
  if (batch == 0) return 0;
  if (batch * nslots >= (1ull << 32) || batch >= (1ull << 31)) return -2;
  return with_logn(logn, [&](auto L) {
    return launch_slots_t<L>(cfg, d_prog, d_slots, nslots, ops, d_key_ntt, d_key_l2, T, d_tw, d_ws, d_norms, d_scratch, d_flags,
                             (uint32_t)batch, np_store);
  });
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
  if (batch == 0 || nrows == 0) return 0;
  if (batch * nrows >= (1ull << 32)) return -2;
  const uint32_t ntasks = (uint32_t)(batch * nrows);
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
