// rzk_slab32_dev.hip — the kernels of the 32-bit coefficient slabs (format and routing: rzk_slab32.h).
//   unit_kernel / unit_io_kernel / shift_row_kernel <.., WaveTeam32>
//                    the kernels of rzk_unit.h and rzk_row.h instantiated for the team whose slabs hold int32_t
//                    coefficients (TeamCoef, rzk_wave.h): the same programs, LDS requests, grids and register budgets;
//                    every operand load moves 4 bytes per coefficient, the canonical test is one unsigned compare on
//                    the max-ed word (canon_lo_mx(int32_t), rzk_rowprog.h), results are stored as int32_t,
//                    non-temporally.  One-wavefront teams at N = 512 and N = 1024, key-product programs only
//                    (slab32_native).  The launchers report them as "unit_kernel<10, false, true, i32>" etc.
//   narrow_kernel    int64 slab -> int32 slab (the low words), with the canonical test of the 64-bit kernels or without
//   widen_kernel     int32 slab -> int64 slab (sign extension)
//                    plain streaming kernels, two coefficients per thread and trip: 16-byte accesses on the wide side,
//                    8-byte on the narrow one, grid-stride under the context's grid cap.
#include <hip/hip_runtime.h>

#include <string>

#include "rzk_dev.h"
#include "rzk_row.h"
#include "rzk_rowprog.h"
#include "rzk_unit.h"

namespace rzk {

#define RZK_LAUNCH_CHECK()                      \
  do {                                          \
    hipError_t e_ = hipGetLastError();          \
    if (e_ != hipSuccess) return (int)e_;       \
  } while (0)

namespace {

// bad == NULL: no test (the producer is this library: outputs of the convert path, trusted mode)
__global__ void __launch_bounds__(256) narrow_kernel(const longlong2* __restrict__ in, int2* __restrict__ out, uint64_t npairs,
                                                     uint32_t qhalf, uint32_t* __restrict__ bad) {
  uint32_t hi = 0, mx = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < npairs; i += (uint64_t)gridDim.x * 256) {
    const longlong2 t = ld_stream(in + i);
    int32_t a, b;
    if (bad) canon_pair(t, qhalf, hi, mx, a, b);
    else pair_words(t, a, b);
    st_stream(out + i, make_int2(a, b));
  }
  if (bad && ((hi != 0) | (mx > 2u * qhalf))) *bad = 1u;
}

__global__ void __launch_bounds__(256) widen_kernel(const int2* __restrict__ in, longlong2* __restrict__ out, uint64_t npairs) {
  int4* __restrict__ o4 = reinterpret_cast<int4*>(out);
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < npairs; i += (uint64_t)gridDim.x * 256) {
    const int2 t = ld_stream(in + i);
    st_stream(o4 + i, make_int4(t.x, t.x >> 31, t.y, t.y >> 31));
  }
}

// the grids, LDS requests and task arithmetic of launch_units_t / launch_units_io_t / launch_shift_t (rzk_kernels.hip)
unsigned grid_for(uint64_t tasks, int num_cus, int waves_per_block, int blocks_per_cu) {
  uint64_t blocks = (tasks + waves_per_block - 1) / waves_per_block;
  const uint64_t cap = (uint64_t)num_cus * blocks_per_cu;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  return (unsigned)blocks;
}
const char* tf(bool v) { return v ? "true" : "false"; }

struct UnitArgs {
  const Program* d_prog;
  const WaveProgram* d_wp;
  const uint32_t* d_key_ntt;
  const double* d_key_l2;
  const DevTables* T;
  const uint32_t* d_tw;
  uint32_t* d_scratch;
  uint8_t* d_flags;
  uint32_t ntasks, upt, tpe, wpt;
};

template <int LOGN, bool HAS_SHIFT, class TM = WaveTeam32>
int launch_units32_t(const LaunchCfg& cfg, const Operands& ops, const UnitArgs& a) {
  using G = Geo<LOGN, 6>;
  constexpr int TPB = WaveTeam::kTeamsPerBlock;
  // per team: transposition slab + P; per workgroup of a team with the phase-2 twiddles in LDS (TeamTwLds): the images
  constexpr size_t kTwWords = TeamTwLds<TM>::value ? (size_t)Tw2Img<LOGN, 6>::TABLES * Tw2Img<LOGN, 6>::WORDS : 0;
  const size_t lds = (TPB * (size_t)(((G::LDS_WORDS + G::N + 3) / 4) * 4) + kTwWords) * sizeof(uint32_t);
  static_assert((TPB * (((G::LDS_WORDS + G::N + 3) / 4) * 4) + kTwWords) * 4 <= 48 * 1024, "no opt-in for large dynamic LDS needed");
  const unsigned grid = grid_for(a.ntasks, cfg.num_cus, TPB, 32 / TPB);
  hipLaunchKernelGGL((unit_kernel<LOGN, false, HAS_SHIFT, TM>), dim3(grid), dim3(TPB << 6), lds, (hipStream_t)cfg.stream, a.d_prog, a.d_wp, ops,
                     a.d_key_ntt, a.d_key_l2, a.T, a.d_tw, a.d_scratch, a.d_flags, a.ntasks, a.upt, a.tpe, a.wpt);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = "unit_kernel<" + std::to_string(LOGN) + ", false, " + tf(HAS_SHIFT) + ", i32>";
  return 0;
}

template <int LOGN, bool HAS_SHIFT>
int launch_units_io32_t(const LaunchCfg& cfg, const Operands& ops, const UnitArgs& a) {
  constexpr int TPB = WaveTeam::kTeamsPerBlock;
  const size_t lds = TPB * (size_t)IoCfg<LOGN, 6>::WORDS * sizeof(uint32_t);   // per team: slab + parking buffers
  static_assert(TPB * IoCfg<LOGN, 6>::WORDS * 4 <= 48 * 1024, "no opt-in for large dynamic LDS needed");
  const unsigned grid = grid_for(a.ntasks, cfg.num_cus, TPB, 32 / TPB);
  hipLaunchKernelGGL((unit_io_kernel<LOGN, HAS_SHIFT, WaveTeam32>), dim3(grid), dim3(TPB << 6), lds, (hipStream_t)cfg.stream, a.d_prog, a.d_wp,
                     ops, a.d_key_ntt, a.d_key_l2, a.T, a.d_tw, a.d_scratch, a.d_flags, a.ntasks, a.upt, a.tpe, a.wpt);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = "unit_io_kernel<" + std::to_string(LOGN) + ", " + tf(HAS_SHIFT) + ", i32>";
  return 0;
}

template <int LOGN>
int launch_shift32_t(const LaunchCfg& cfg, const Program* d_prog, const Operands& ops, const DevTables* T, uint8_t* d_flags,
                     uint32_t ntasks) {
  constexpr int TPB = ShiftCfg<LOGN, WaveTeam32>::TPB;
  size_t lds = (size_t)TPB * ShiftCfg<LOGN, WaveTeam32>::WORDS * sizeof(uint32_t);
  if (RZK_SHIFT_BYTES_WAVES < 5 && LOGN >= 10 && lds < 40 * 1024) lds = 40 * 1024;   // four workgroups per CU, as launch_shift_t
  const unsigned grid = grid_for(ntasks, cfg.num_cus, TPB, 16);
  if (ops.trusted)
    hipLaunchKernelGGL((shift_row_kernel<LOGN, true, WaveTeam32, true>), dim3(grid), dim3(TPB << 6), lds, (hipStream_t)cfg.stream, d_prog, ops, T,
                       d_flags, ntasks);
  else
    hipLaunchKernelGGL((shift_row_kernel<LOGN, false, WaveTeam32, true>), dim3(grid), dim3(TPB << 6), lds, (hipStream_t)cfg.stream, d_prog, ops, T,
                       d_flags, ntasks);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = "shift_row_kernel<" + std::to_string(LOGN) + ", " + tf(ops.trusted) + ", i32>";
  return 0;
}

unsigned stream_grid(uint64_t npairs, int num_cus) {
  uint64_t blocks = (npairs + 255) / 256;
  const uint64_t cap = (uint64_t)num_cus * 8;
  if (blocks > cap) blocks = cap;
  return (unsigned)(blocks < 1 ? 1 : blocks);
}

}  // namespace

int launch_units32(int logn, const LaunchCfg& cfg, const Program* d_prog, const WaveProgram* d_wp, uint32_t nunits,
                   uint32_t units_per_task, uint32_t work_per_entry, bool has_shift, const Operands& ops,
                   const uint32_t* d_key_ntt, const double* d_key_l2, const DevTables* T, const uint32_t* d_tw,
                   uint32_t* d_scratch, uint8_t* d_flags, uint64_t batch) {
  if (batch == 0 || nunits == 0) return 0;
  if (units_per_task == 0) units_per_task = 1;
  const uint32_t tpe = (nunits + units_per_task - 1) / units_per_task;   // tasks per batch entry
  if (batch * tpe >= (1ull << 32)) return -2;
  const uint32_t ntasks = (uint32_t)(batch * tpe);
  const uint32_t wpt = (work_per_entry + tpe - 1) / tpe;
  const UnitArgs a{d_prog, d_wp, d_key_ntt, d_key_l2, T, d_tw, d_scratch, d_flags, ntasks, units_per_task, tpe, wpt};
  if (cfg.unit_io) {
    switch (logn) {
      case 9: return has_shift ? launch_units_io32_t<9, true>(cfg, ops, a) : launch_units_io32_t<9, false>(cfg, ops, a);
      case 10: return has_shift ? launch_units_io32_t<10, true>(cfg, ops, a) : launch_units_io32_t<10, false>(cfg, ops, a);
    }
    return -1;
  }
  switch (logn) {
    case 9: return has_shift ? launch_units32_t<9, true>(cfg, ops, a) : launch_units32_t<9, false>(cfg, ops, a);
    case 10:
      if (cfg.tw_lds) return has_shift ? launch_units32_t<10, true, WaveTeam32Tw>(cfg, ops, a) : launch_units32_t<10, false, WaveTeam32Tw>(cfg, ops, a);
      return has_shift ? launch_units32_t<10, true>(cfg, ops, a) : launch_units32_t<10, false>(cfg, ops, a);
  }
  return -1;   // (slab32_native, rzk_slab32.h: every other shape takes the convert path)
}

int launch_shift_rows32(int logn, const LaunchCfg& cfg, const Program* d_prog, uint32_t nrows, const Operands& ops,
                        const DevTables* T, uint8_t* d_flags, uint64_t batch) {
  if (batch == 0 || nrows == 0) return 0;
  if (batch * nrows >= (1ull << 32)) return -2;
  const uint32_t ntasks = (uint32_t)(batch * nrows);
  if (!cfg.shift_bytes) return -1;
  switch (logn) {
    case 9: return launch_shift32_t<9>(cfg, d_prog, ops, T, d_flags, ntasks);
    case 10: return launch_shift32_t<10>(cfg, d_prog, ops, T, d_flags, ntasks);
  }
  return -1;
}

int launch_narrow(const LaunchCfg& cfg, const int64_t* in, int32_t* out, uint64_t ncoef, uint32_t qhalf, uint32_t* bad_word) {
  if (ncoef == 0) return 0;
  const uint64_t npairs = ncoef / 2;   // ncoef is a multiple of N >= 4
  hipLaunchKernelGGL(narrow_kernel, dim3(stream_grid(npairs, cfg.num_cus)), dim3(256), 0, (hipStream_t)cfg.stream,
                     reinterpret_cast<const longlong2*>(in), reinterpret_cast<int2*>(out), npairs, qhalf, bad_word);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = "narrow_kernel";
  return 0;
}

int launch_widen(const LaunchCfg& cfg, const int32_t* in, int64_t* out, uint64_t ncoef) {
  if (ncoef == 0) return 0;
  const uint64_t npairs = ncoef / 2;
  hipLaunchKernelGGL(widen_kernel, dim3(stream_grid(npairs, cfg.num_cus)), dim3(256), 0, (hipStream_t)cfg.stream,
                     reinterpret_cast<const int2*>(in), reinterpret_cast<longlong2*>(out), npairs);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = "widen_kernel";
  return 0;
}

}  // namespace rzk
