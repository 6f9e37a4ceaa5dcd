// rzk_slab32_dev.hip — the kernels of the 32-bit coefficient slabs (format and routing: rzk_slab32.h).
//   unit_kernel / unit_io_kernel / shift_row_kernel <.., WaveTeam32>
//                    the kernels of rzk_unit.h and rzk_row.h instantiated for the team whose slabs hold int32_t
//                    coefficients (TeamCoef, rzk_wave.h): the same programs, LDS requests, grids and register budgets;
//                    every operand load moves 4 bytes per coefficient, the canonical test is one unsigned compare on
//                    the max-ed word (canon_lo_mx(int32_t), rzk_rowprog.h), results are stored as int32_t,
//                    non-temporally.  One-wavefront teams at N = 512 and N = 1024, key-product programs only
//                    (slab32_native).  Started by the launchers of the 64-bit kernels (launch_units_t, launch_units_io_t,
//                    launch_shift_t, rzk_launch.h) with WaveTeam32 / WaveTeam32Tw as the team; only the dispatchers
//                    launch_units32 / launch_shift_rows32 are here.  Reported as "unit_kernel<10, false, true, i32>" etc.
//   row_kernel<LOGN, false, WaveTeam32, false>
//                    the vector x vector programs of Linear (gx = g.x, u, the verifier's last program) on 32-bit slabs:
//                    the kernel of rzk_row.h with the 32-bit team, without rotation terms, started by launch_rows_t
//                    (rzk_launch.h) from launch_rows32.  Reported as "row_kernel<9, false, i32, false>".
//   norm_kernel_i32  the stand-alone norm predicate (norm_rows, rzk_norm.h) on an int32_t slab: where a checked program's
//                    fused form cannot run (two-bit verdicts on a flag array that is not made of whole aligned words)
//                    and behind rzk_norm2_le32_batch.  Reported as "norm_kernel_i32<9>".
//   narrow_kernel    int64 slab -> int32 slab (the low words), with the canonical test of the 64-bit kernels or without
//   widen_kernel     int32 slab -> int64 slab (sign extension)
//                    plain streaming kernels, two coefficients per thread and trip: 16-byte accesses on the wide side,
//                    8-byte on the narrow one, grid-stride under the context's grid cap.
//   eq32_kernel      eq[b] = (two blocks of int32 words are equal word for word): the compare of the short verifier on
//                    32-bit slabs.  One wavefront per batch entry, 16-byte loads, lane-consecutive, four
//                    wavefronts per workgroup, grid-stride; every entry's byte is written, so there is no preset.
#include <hip/hip_runtime.h>

#include <string>

#include "rzk_dev.h"
#include "rzk_norm.h"
#include "rzk_row.h"
#include "rzk_rowprog.h"
#include "rzk_unit.h"
#include "rzk_launch.h"

namespace rzk {

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

constexpr uint32_t kEqWaves = 4;

__global__ void __launch_bounds__(64 * kEqWaves) eq32_kernel(const int4* __restrict__ a, const int4* __restrict__ b, uint64_t quads,
                                                             uint8_t* __restrict__ eq, uint64_t B) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  for (uint64_t e = (uint64_t)blockIdx.x * kEqWaves + wave; e < B; e += (uint64_t)gridDim.x * kEqWaves) {
    const int4* pa = a + e * quads;
    const int4* pb = b + e * quads;
    uint32_t diff = 0;
    for (uint64_t i = lane; i < quads; i += 64) {
      const int4 x = ld_stream(pa + i), y = ld_stream(pb + i);
      diff |= (uint32_t)((x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w));
    }
    const bool any = __builtin_amdgcn_ballot_w64(diff != 0) != 0;
    if (lane == 0) eq[e] = any ? 0 : 1;
  }
}

template <int LOGN>
__global__ void __launch_bounds__(256)
norm_kernel_i32(const int32_t* __restrict__ v, uint32_t rows, uint64_t limit_hi, uint64_t limit_lo, uint8_t* __restrict__ ok,
                uint64_t B, int and_mode, int shift, uint32_t qhalf, uint32_t* __restrict__ bad_word) {
  norm_rows<LOGN, int32_t>(v, rows, limit_hi, limit_lo, ok, B, and_mode, shift, qhalf, bad_word);
}

unsigned stream_grid(uint64_t npairs, int num_cus) {
  uint64_t blocks = (npairs + 255) / 256;
  const uint64_t cap = (uint64_t)num_cus * 8;
  if (blocks > cap) blocks = cap;
  return (unsigned)(blocks < 1 ? 1 : blocks);
}

}  // namespace

// The shared launchers (rzk_launch.h) on the 32-bit teams.  Dispatchers of this file's own, so that the instantiations stay
// in this translation unit; every shape without a native 32-bit kernel answers -1 (slab32_native, rzk_slab32.h: the
// caller takes the convert path).
static_assert(unit_lds_bytes<10, WaveTeam32Tw, true>() <= 48 * 1024 && unit_io_lds_bytes<10, WaveTeam32>() <= 48 * 1024 &&
                  unit_io_lds_bytes<9, WaveTeam32>() <= 48 * 1024 && shift_launch<10, WaveTeam32, true>().lds <= 48 * 1024,
              "the 32-bit instantiations with four teams per workgroup stay below the opt-in for large dynamic LDS");

int launch_units32(int logn, const LaunchCfg& cfg, const RowArgs& a, const Operands& ops, const UnitShape& u, uint64_t batch) {
  UnitTasks t;
  if (const int rc = unit_tasks(u, batch, t); rc <= 0) return rc;
  if (u.has_vec) return -1;   // key-product programs only
  return with_flag(u.has_shift, [&](auto S) -> int {
    if (cfg.unit_io) {
      switch (logn) {
        case 9: return launch_units_io_t<9, S, WaveTeam32>(cfg, a, ops, t);
        case 10: return launch_units_io_t<10, S, WaveTeam32>(cfg, a, ops, t);
      }
      return -1;
    }
    switch (logn) {
      case 9: return launch_units_t<9, false, S, WaveTeam32>(cfg, a, ops, t);
      case 10:
        if (cfg.tw_lds >= 2) return launch_units_t<10, false, S, WaveTeam32Tw3>(cfg, a, ops, t);   // (the one instantiation here with the large-LDS opt-in)
        return cfg.tw_lds ? launch_units_t<10, false, S, WaveTeam32Tw>(cfg, a, ops, t) : launch_units_t<10, false, S, WaveTeam32>(cfg, a, ops, t);
    }
    return -1;
  });
}

int launch_shift_rows32(int logn, const LaunchCfg& cfg, const RowArgs& a, const Operands& ops, uint32_t nrows, uint64_t batch) {
  uint32_t ntasks;
  if (const int rc = task_count(batch, nrows, ntasks); rc <= 0) return rc;
  if (!cfg.shift_bytes) return -1;   // the packed-byte kernel only
  switch (logn) {
    case 9: return launch_shift_t<9, WaveTeam32>(cfg, a, ops, ntasks);
    case 10: return launch_shift_t<10, WaveTeam32>(cfg, a, ops, ntasks);
  }
  return -1;
}

// row_kernel on 32-bit slabs: no rotation terms, no operand images (slab32_native)
int launch_rows32(int logn, const LaunchCfg& cfg, const RowArgs& a, const Operands& ops, uint32_t nrows, bool has_shift, uint64_t batch,
                  bool has_dd) {
  uint32_t ntasks;
  if (const int rc = task_count(batch, nrows, ntasks); rc <= 0) return rc;
  if (has_shift || has_dd) return -1;
  switch (logn) {
    case 9: return launch_rows_t<9, false, WaveTeam32>(cfg, a, ops, ntasks);
    case 10: return launch_rows_t<10, false, WaveTeam32>(cfg, a, ops, ntasks);
  }
  return -1;
}

// launch_norm (rzk_kernels.hip) on an int32_t slab: the same grid, one wavefront per proof
int launch_norm32(int logn, const LaunchCfg& cfg, const int32_t* v, uint32_t rows, uint64_t limit_hi, uint64_t limit_lo, uint8_t* ok,
                  uint64_t B, int and_mode, int shift, uint32_t qhalf, uint32_t* bad_word) {
  if (B == 0) return 0;
  const unsigned grid = grid_for(B, cfg.num_cus);
  switch (logn) {
    case 9:
      hipLaunchKernelGGL(norm_kernel_i32<9>, dim3(grid), dim3(256), 0, (hipStream_t)cfg.stream, v, rows, limit_hi, limit_lo, ok, B,
                         and_mode, shift, qhalf, bad_word);
      break;
    case 10:
      hipLaunchKernelGGL(norm_kernel_i32<10>, dim3(grid), dim3(256), 0, (hipStream_t)cfg.stream, v, rows, limit_hi, limit_lo, ok, B,
                         and_mode, shift, qhalf, bad_word);
      break;
    default: return -1;
  }
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = "norm_kernel_i32<" + std::to_string(logn) + ">";
  return 0;
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

int launch_eq32(const LaunchCfg& cfg, const int32_t* a, const int32_t* b, uint64_t words, uint8_t* eq, uint64_t B) {
  if (B == 0) return 0;
  uint64_t blocks = (B + kEqWaves - 1) / kEqWaves;
  const uint64_t cap = (uint64_t)cfg.num_cus * 8;
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(eq32_kernel, dim3((unsigned)blocks), dim3(64 * kEqWaves), 0, (hipStream_t)cfg.stream,
                     reinterpret_cast<const int4*>(a), reinterpret_cast<const int4*>(b), words / 4, eq, B);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = "eq32_kernel";
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
