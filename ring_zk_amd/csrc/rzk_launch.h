// rzk_launch.h — the launch rules of the row-program kernels: grids, dynamic LDS requests, task arithmetic and the names the
// launchers report.  Host code of the device translation units (rzk_kernels.hip, rzk_slab32_dev.hip,
// rzk_response_stat_dev.hip), included after the kernel headers.  Everything here is a template or an inline function: a
// translation unit gets exactly the kernels its own dispatchers name, nothing by including this file.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <type_traits>

#include "rzk_row.h"
#include "rzk_unit.h"

namespace rzk {

static inline unsigned grid_for(uint64_t tasks, int num_cus, int waves_per_block = 4, int blocks_per_cu = 8) {
  uint64_t blocks = (tasks + waves_per_block - 1) / waves_per_block;
  const uint64_t cap = (uint64_t)num_cus * blocks_per_cu;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  return (unsigned)blocks;
}

// Tasks of a launch, `per_entry` for each of `batch` entries.  1: launch ntasks of them; 0: nothing to do; -2: the kernels'
// 32-bit task index cannot hold the count.  A launcher returns every answer but 1 as it is.
static inline int task_count(uint64_t batch, uint64_t per_entry, uint32_t& ntasks) {
  if (batch == 0 || per_entry == 0) return 0;
  if (batch * per_entry >= (1ull << 32)) return -2;
  ntasks = (uint32_t)(batch * per_entry);
  return 1;
}
// The task arithmetic of the unit kernels (their last four arguments); answers as task_count
struct UnitTasks {
  uint32_t ntasks, upt, tpe, wpt;
};
static inline int unit_tasks(const UnitShape& u, uint64_t batch, UnitTasks& t) {
  t.upt = u.units_per_task ? u.units_per_task : 1;
  t.tpe = (u.nunits + t.upt - 1) / t.upt;   // tasks per batch entry
  const int rc = task_count(batch, t.tpe, t.ntasks);
  if (rc > 0) t.wpt = (u.work_per_entry + t.tpe - 1) / t.tpe;   // transforms per task (estimate, for the progress priorities)
  return rc;
}

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
// f(std::true_type / std::false_type) for a run-time flag that is a template argument of the kernel
template <class F>
static int with_flag(bool v, F&& f) {
  return v ? f(std::true_type{}) : f(std::false_type{});
}

// The launchers of the row-program kernels report which instantiation they started (LaunchCfg::launched, read back
// through rzk_prof_read_kernels): its name as a profiler prints it, without "void rzk::" and the argument list.  Tests,
// bench.py and tools/pmc_traffic.py match these strings, so they keep their habits: a default WaveTeam is left out
// (team_arg) by every kernel but row_kernel, which always names its team.
static inline const char* tf(bool v) { return v ? "true" : "false"; }
template <class TM>
static std::string team_arg() {   // (the teams with the twiddle image report as the teams they derive from)
  return std::is_same<TM, WaveTeam>::value || std::is_same<TM, WaveTeamTw>::value || std::is_same<TM, WaveTeamTw3>::value
             ? std::string()
             : std::string(", ") + TM::kName;
}

// ---- unit kernels ------------------------------------------------------------------------------------------------------
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
  using I = typename TeamTwImg<LOGN, TM>::type;
  return TeamTwLds<TM>::value ? (size_t)I::TABLES * I::WORDS : 0;
}
// bytes per workgroup of unit_kernel (and, for the teams without the image, row_kernel) / of unit_io_kernel
template <int LOGN, class TM, bool HAS_SHIFT>
constexpr size_t unit_lds_bytes() {
  return (TM::kTeamsPerBlock * team_lds_words<LOGN, TM, HAS_SHIFT>() + block_tw_words<LOGN, TM>()) * sizeof(uint32_t);
}
template <int LOGN, class TM>
constexpr size_t unit_io_lds_bytes() {   // per team: slab + parking buffers
  return TM::kTeamsPerBlock * (size_t)IoCfg<LOGN, TM::LL>::WORDS * sizeof(uint32_t);
}
// workgroups per CU under the grid cap: at most num_cus * 32 team lines of scratch; every team walks its tasks with a grid stride.
// A sixteen-team workgroup is all a CU holds (LDS), and a second one would only start when all sixteen teams of the first
// are done: one per CU, so that every team fills its image once and walks on.
template <class TM>
constexpr int unit_blocks_per_cu() {
  return TM::LL == 6 ? (TM::kTeamsPerBlock >= 16 ? 1 : 32 / TM::kTeamsPerBlock) : 8;
}
static_assert(unit_blocks_per_cu<WaveTeam>() * WaveTeam::kTeamsPerBlock <= 32 && unit_blocks_per_cu<WaveTeamTw3>() * WaveTeamTw3::kTeamsPerBlock <= 32 &&
                  unit_blocks_per_cu<WaveTeam32Tw3>() * WaveTeam32Tw3::kTeamsPerBlock <= 32,
              "row_scratch_words: 32 team lines per CU");

template <int LOGN, bool HAS_VEC, bool HAS_SHIFT, class TM = WaveTeam>
static int launch_units_t(const LaunchCfg& cfg, const RowArgs& a, const Operands& ops, const UnitTasks& t) {
  using G = Geo<LOGN, TM::LL>;
  constexpr int TPB = TM::kTeamsPerBlock;
  constexpr size_t lds = unit_lds_bytes<LOGN, TM, HAS_SHIFT>();
  static_assert(!TeamTwLds<TM>::value || team_lds_words<LOGN, TM, HAS_SHIFT>() == (size_t)(G::LDS_WORDS + G::N),
                "unit_kernel puts the images right behind the teams' slab + P");
  if (lds > 48 * 1024) {   // large dynamic LDS needs an opt-in; per device, so set before every launch (cheap, idempotent)
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&unit_kernel<LOGN, HAS_VEC, HAS_SHIFT, TM>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  const unsigned grid = grid_for(t.ntasks, cfg.num_cus, TPB, unit_blocks_per_cu<TM>());
  hipLaunchKernelGGL((unit_kernel<LOGN, HAS_VEC, HAS_SHIFT, TM>), dim3(grid), dim3(TPB << TM::LL), lds, (hipStream_t)cfg.stream,
                     a.prog, a.wp, ops, a.key_ntt, a.key_l2, a.T, a.tw, a.scratch, a.flags, t.ntasks, t.upt, t.tpe, t.wpt);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = "unit_kernel<" + std::to_string(LOGN) + ", " + tf(HAS_VEC) + ", " + tf(HAS_SHIFT) + team_arg<TM>() + ">";
  return 0;
}

template <int LOGN, bool HAS_SHIFT, class TM = WaveTeam>
static int launch_units_io_t(const LaunchCfg& cfg, const RowArgs& a, const Operands& ops, const UnitTasks& t) {
  constexpr int TPB = TM::kTeamsPerBlock;
  constexpr size_t lds = unit_io_lds_bytes<LOGN, TM>();
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&unit_io_kernel<LOGN, HAS_SHIFT, TM>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  const unsigned grid = grid_for(t.ntasks, cfg.num_cus, TPB, unit_blocks_per_cu<TM>());
  hipLaunchKernelGGL((unit_io_kernel<LOGN, HAS_SHIFT, TM>), dim3(grid), dim3(TPB << TM::LL), lds, (hipStream_t)cfg.stream,
                     a.prog, a.wp, ops, a.key_ntt, a.key_l2, a.T, a.tw, a.scratch, a.flags, t.ntasks, t.upt, t.tpe, t.wpt);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = "unit_io_kernel<" + std::to_string(LOGN) + ", " + tf(HAS_SHIFT) + team_arg<TM>() + ">";
  return 0;
}

// ---- row_kernel ---------------------------------------------------------------------------------------------------------
// The LDS request, grid and scratch lines of unit_kernel's teams.  The name always carries the team: "row_kernel<9, false,
// WaveTeam, false>", and "row_kernel<9, false, i32, false>" on 32-bit slabs.
template <int LOGN, bool HAS_SHIFT, class TM = WaveTeam, bool DD = false>
static int launch_rows_t(const LaunchCfg& cfg, const RowArgs& a, const Operands& ops, uint32_t ntasks) {
  constexpr int TPB = TM::kTeamsPerBlock;
  constexpr size_t lds = unit_lds_bytes<LOGN, TM, HAS_SHIFT>();   // per team: transposition slab + state word A
  static_assert(!TeamTwLds<TM>::value, "row_kernel reads its twiddles from the global tables");
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&row_kernel<LOGN, HAS_SHIFT, TM, DD>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  const unsigned grid = grid_for(ntasks, cfg.num_cus, TPB, unit_blocks_per_cu<TM>());   // <= 32 team lines per CU (scratch sizing)
  hipLaunchKernelGGL((row_kernel<LOGN, HAS_SHIFT, TM, DD>), dim3(grid), dim3(TPB << TM::LL), lds, (hipStream_t)cfg.stream, a.prog, ops,
                     a.key_ntt, a.key_l2, a.T, a.tw, a.scratch, a.flags, ntasks);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = "row_kernel<" + std::to_string(LOGN) + ", " + tf(HAS_SHIFT) + ", " + TM::kName + ", " + tf(DD) + ">";
  return 0;
}

// ---- rotation kernels (shift_row_kernel, response_stat_kernel) -------------------------------------------------------------
// One team's image is 8 N bytes.  The workgroup asks for at least 40 KiB so that a CU holds four workgroups = 4 waves per
// SIMD: with the 79 VGPRs the kernel needs, five or six would fit, and measured slower (response rows at N = 1024:
// 86.7 us against 77.5 us at four — the kernel is co-bound by the LDS pipe, more waves only add contention).
// N = 512 keeps its 6 waves per SIMD: 4-KiB images, measured fine.
// Teams of two (N = 2048): 18 KiB per 128-thread workgroup, eight workgroups = 4 waves per SIMD.
// BYTES: the packed image is 3 N bytes, but a term that fails the condition still builds the word image, so the request
// stays at 8 N bytes per team.  The floor stays too while the kernel is compiled for four waves per SIMD
// (RZK_SHIFT_BYTES_WAVES, rzk_row.h: at five it needs 96 VGPRs and spills; measured no gain).
// The grid cap is 16 workgroups per CU (64 of the one-team workgroups of N = 2048).
struct ShiftLaunch {
  size_t lds;          // bytes of dynamic LDS per workgroup
  int blocks_per_cu;   // grid cap
};
template <int LOGN, class TM, bool BYTES>
constexpr ShiftLaunch shift_launch() {
  static_assert(!BYTES || TM::LL == 6, "packed-byte rotations: one wavefront per polynomial");
  size_t lds = (size_t)ShiftCfg<LOGN, TM>::TPB * ShiftCfg<LOGN, TM>::WORDS * sizeof(uint32_t);
  if ((!BYTES || RZK_SHIFT_BYTES_WAVES < 5) && TM::LL == 6 && LOGN >= 10 && lds < 40 * 1024) lds = 40 * 1024;
  return {lds, TM::LL == 6 ? 16 : 64};
}

template <int LOGN, class TM = WaveTeam, bool BYTES = (TM::LL == 6)>
static int launch_shift_t(const LaunchCfg& cfg, const RowArgs& a, const Operands& ops, uint32_t ntasks) {
  constexpr int TPB = ShiftCfg<LOGN, TM>::TPB;
  constexpr ShiftLaunch g = shift_launch<LOGN, TM, BYTES>();
  const void* fn = ops.trusted ? reinterpret_cast<const void*>(&shift_row_kernel<LOGN, true, TM, BYTES>)
                               : reinterpret_cast<const void*>(&shift_row_kernel<LOGN, false, TM, BYTES>);
  if (g.lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds);
    if (e != hipSuccess) return (int)e;
  }
  const unsigned grid = grid_for(ntasks, cfg.num_cus, TPB, g.blocks_per_cu);
  if (ops.trusted)
    hipLaunchKernelGGL((shift_row_kernel<LOGN, true, TM, BYTES>), dim3(grid), dim3(TPB << TM::LL), g.lds, (hipStream_t)cfg.stream, a.prog,
                       ops, a.T, a.flags, ntasks);
  else
    hipLaunchKernelGGL((shift_row_kernel<LOGN, false, TM, BYTES>), dim3(grid), dim3(TPB << TM::LL), g.lds, (hipStream_t)cfg.stream, a.prog,
                       ops, a.T, a.flags, ntasks);
  RZK_LAUNCH_CHECK();
  // template defaults are left out, as everywhere: BYTES defaults to "one wavefront per polynomial", so the short name is
  // the packed-byte kernel at N <= 1024 and the word kernel of the two-wavefront teams; RZK_SHIFT_BYTES=0 spells it out
  constexpr bool kDefault = BYTES == (TM::LL == 6);
  if (cfg.launched)
    *cfg.launched = "shift_row_kernel<" + std::to_string(LOGN) + ", " + tf(ops.trusted) +
                    (kDefault ? team_arg<TM>() : std::string(", ") + TM::kName + ", " + tf(BYTES)) + ">";
  return 0;
}

// ---- the geometry, pinned: bytes of dynamic LDS per workgroup of every instantiation the dispatchers start ---------------
// (the tests see kernel names, not grids or LDS sizes; a retuning changes the number here on purpose)
// unit_kernel, without and with rotation terms (the 32-bit teams: key-product programs only)
static_assert(unit_lds_bytes<9, WaveTeam, false>() == 16640 && unit_lds_bytes<9, WaveTeam, true>() == 16640, "");
static_assert(unit_lds_bytes<9, WaveTeam32, false>() == 16640 && unit_lds_bytes<9, WaveTeam32, true>() == 16640, "");
static_assert(unit_lds_bytes<10, WaveTeam, false>() == 33280 && unit_lds_bytes<10, WaveTeam, true>() == 33280, "");
static_assert(unit_lds_bytes<10, WaveTeam32, false>() == 33280 && unit_lds_bytes<10, WaveTeam32, true>() == 33280, "");
static_assert(unit_lds_bytes<10, WaveTeamTw, false>() == 39424 && unit_lds_bytes<10, WaveTeamTw, true>() == 39424, "");   // 4 x 8 320 + 6 144
static_assert(unit_lds_bytes<10, WaveTeam32Tw, false>() == 39424 && unit_lds_bytes<10, WaveTeam32Tw, true>() == 39424, "");
static_assert(unit_lds_bytes<10, WaveTeamTw3, false>() == 157696 && unit_lds_bytes<10, WaveTeamTw3, true>() == 157696, "");   // 16 x 8 320 + 24 576
static_assert(unit_lds_bytes<10, WaveTeam32Tw3, false>() == 157696 && unit_lds_bytes<10, WaveTeam32Tw3, true>() == 157696, "");
static_assert(unit_lds_bytes<11, WaveTeam, false>() == 66560, "");   // (above 48 KiB: the opt-in branch; no rotation terms on one wavefront)
static_assert(unit_lds_bytes<11, PairTeam, false>() == 16640 && unit_lds_bytes<11, PairTeam, true>() == 18448, "");
// row_kernel: unit_kernel's request for the same team, in either width (pinned above for WaveTeam / WaveTeam32)
// unit_io_kernel
static_assert(unit_io_lds_bytes<9, WaveTeam>() == 33024 && unit_io_lds_bytes<9, WaveTeam32>() == 33024, "");
static_assert(unit_io_lds_bytes<10, WaveTeam>() == 33280 && unit_io_lds_bytes<10, WaveTeam32>() == 33280, "");
static_assert(unit_io_lds_bytes<11, WaveTeam>() == 66560 && unit_io_lds_bytes<11, PairTeam>() == 16640, "");
// the rotation kernels, with their workgroups per CU
#define RZK_PIN_SHIFT(LOGN, TM, BYTES, LDS, CAP)                                                                            \
  static_assert(shift_launch<LOGN, TM, BYTES>().lds == LDS && shift_launch<LOGN, TM, BYTES>().blocks_per_cu == CAP, \
                "rotation kernels: LDS per workgroup, workgroups per CU")
constexpr size_t kPinBytes1024 = RZK_SHIFT_BYTES_WAVES < 5 ? 40960 : 32768;   // (the tuning build for five waves per SIMD drops the floor)
RZK_PIN_SHIFT(9, WaveTeam, true, 16384, 16);
RZK_PIN_SHIFT(9, WaveTeam, false, 16384, 16);
RZK_PIN_SHIFT(9, WaveTeam32, true, 16384, 16);
RZK_PIN_SHIFT(10, WaveTeam, true, kPinBytes1024, 16);
RZK_PIN_SHIFT(10, WaveTeam, false, 40960, 16);
RZK_PIN_SHIFT(10, WaveTeam32, true, kPinBytes1024, 16);
RZK_PIN_SHIFT(11, PairTeam, false, 18448, 64);
#undef RZK_PIN_SHIFT
// N = 1024, four one-wavefront teams with the twiddle image: four workgroups (4 waves per SIMD) in 157 696 of the CU's 163 840
static_assert(4 * unit_lds_bytes<10, WaveTeamTw, true>() <= 160 * 1024, "the twiddle images must leave room for four workgroups per CU");
// ... and sixteen teams with every vector twiddle in LDS: one workgroup, the same 4 waves per SIMD in the same 157 696 B
static_assert(unit_lds_bytes<10, WaveTeamTw3, true>() == 4 * unit_lds_bytes<10, WaveTeamTw, true>() && (WaveTeamTw3::kTeamsPerBlock << 6) == 1024,
              "the full image: one 1024-thread workgroup in the LDS of four 256-thread ones");

}  // namespace rzk
