// rzk_prove_loop_dev.hip — the kernels between the library calls of the in-library prover loops (host loops:
// rzk_prove_loop.cpp; arithmetic: rzk_prove_loop.h).  All of them move flags, indices and whole rows; none
// computes on a coefficient, so T (i64 / i32) only sets how many 16-byte quads a row has.
//   pending_compact_kernel      idx[0 .. count) = the ascending b with live[b] && !done[b], *count.  ONE workgroup of 16
//                               wavefronts (an ordered scan, not an atomic append: the order is the oracle's): per tile of
//                               1024 flags one ballot and popcount per wavefront, the 16 totals through LDS, a running base.
//   coin_kernel<T>              coin[i] = prove_coin(a[i][0], b[i][1]) from the two uniform draws of N coefficients each
//   gather_rows_kernel<T>       dst[i] = src[idx[i]] for up to two slabs (r: k rows, c: n + l rows) in one launch; one
//                               workgroup per entry and trip, 16-byte loads and stores, lane-consecutive
//   accept_scatter_kernel<T>    accept[i] != 0: rows of t[i], z[i] -> t_out[idx[i]], z_out[idx[i]]; rounds[idx[i]] = rnd,
//                               done[idx[i]] = 1.  idx has no duplicates, so no two workgroups write one proof.
//   prove_first_kernel          after round 0: live = ok_commit & ok_hash (as 0 / 1), done = live & accept, rounds = 0
//   prove_last_kernel<T>        after the last round: t, z rows of every proof with done == 0 are zeroed, ok = done
// and, for the five slabs per direction of the Linear and Sum loops, the same moves over a field list (FieldList):
//   gather_fields_kernel, accept_scatter_fields_kernel, prove_last_fields_kernel; prove_first_want_kernel compares the
//   commit flag against a wanted value (prove_live).  64-bit slabs only, so they are no templates.
// Grids follow the context's cap (LaunchCfg::num_cus, RZK_GRID_CUS) with grid-stride loops.
#include <hip/hip_runtime.h>

#include <string>
#include <type_traits>

#include "rzk_dev.h"
#include "rzk_prove_loop.h"
#include "rzk_wave.h"

namespace rzk {

namespace {

__global__ void __launch_bounds__(kCompactTile) pending_compact_kernel(const uint8_t* __restrict__ live, const uint8_t* __restrict__ done,
                                                                       uint64_t B, uint32_t* __restrict__ idx, uint32_t* __restrict__ count) {
  __shared__ uint32_t totals[kCompactWaves];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint32_t base = 0;
  for (uint64_t tile0 = 0; tile0 < B; tile0 += kCompactTile) {
    const uint64_t i = tile0 + threadIdx.x;
    const bool pend = i < B && compact_pending(live[i], done[i]);
    const uint64_t ballot = __builtin_amdgcn_ballot_w64(pend);
    if (lane == 0) totals[wave] = compact_wave_total(ballot);
    __syncthreads();
    if (pend) idx[base + compact_wave_base(totals, wave) + compact_lane_rank(ballot, lane)] = (uint32_t)i;
    base += compact_wave_base(totals, kCompactWaves);
    __syncthreads();   // the totals are read before the next tile overwrites them
  }
  if (threadIdx.x == 0) *count = base;
}

template <class T>
__global__ void __launch_bounds__(256) coin_kernel(const T* __restrict__ a, const T* __restrict__ b, uint32_t N, int64_t* __restrict__ coin,
                                                   uint64_t count) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (uint64_t)gridDim.x * 256)
    coin[i] = prove_coin((int64_t)a[i * N], (int64_t)b[i * N + 1]);
}

struct GatherJob {   // dst[s][i] = src[s][idx[i]], quads[s] 16-byte quads per entry; quads[1] == 0: one slab
  const int4* src[2];
  int4* dst[2];
  uint32_t quads[2];
};

template <class T>
__global__ void __launch_bounds__(256) gather_rows_kernel(GatherJob job, const uint32_t* __restrict__ idx, uint32_t count) {
  for (uint32_t i = blockIdx.x; i < count; i += gridDim.x) {
    const uint64_t from = idx[i];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int4* __restrict__ src = job.src[s] + from * job.quads[s];
      int4* __restrict__ dst = job.dst[s] + (uint64_t)i * job.quads[s];
      for (uint32_t q = threadIdx.x; q < job.quads[s]; q += 256) dst[q] = ld_stream(src + q);
    }
  }
}

struct ScatterJob {   // the sub-batch's t, z and the caller's; quads per entry of each
  const int4 *t, *z;
  int4 *t_out, *z_out;
  uint32_t t_quads, z_quads;
};

template <class T>
__global__ void __launch_bounds__(256) accept_scatter_kernel(ScatterJob job, const uint8_t* __restrict__ accept, const uint32_t* __restrict__ idx,
                                                             uint32_t count, uint8_t rnd, uint8_t* __restrict__ rounds,
                                                             uint8_t* __restrict__ done) {
  for (uint32_t i = blockIdx.x; i < count; i += gridDim.x) {
    if (accept[i] == 0) continue;   // uniform over the workgroup
    const uint64_t to = idx[i];
    const int4* __restrict__ ts = job.t + (uint64_t)i * job.t_quads;
    int4* __restrict__ td = job.t_out + to * job.t_quads;
    for (uint32_t q = threadIdx.x; q < job.t_quads; q += 256) st_stream(td + q, ld_stream(ts + q));
    const int4* __restrict__ zs = job.z + (uint64_t)i * job.z_quads;
    int4* __restrict__ zd = job.z_out + to * job.z_quads;
    for (uint32_t q = threadIdx.x; q < job.z_quads; q += 256) st_stream(zd + q, ld_stream(zs + q));
    if (threadIdx.x == 0) {
      rounds[to] = rnd;
      done[to] = 1;
    }
  }
}

__global__ void __launch_bounds__(256) prove_first_kernel(const uint8_t* __restrict__ ok_commit, const uint8_t* __restrict__ ok_hash,
                                                          const uint8_t* __restrict__ accept, uint8_t* __restrict__ live,
                                                          uint8_t* __restrict__ done, uint8_t* __restrict__ rounds, uint64_t B) {
  for (uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x; b < B; b += (uint64_t)gridDim.x * 256) {
    const uint8_t l = (ok_commit[b] & ok_hash[b]) != 0 ? 1 : 0;
    live[b] = l;
    done[b] = (l && accept[b] != 0) ? 1 : 0;
    rounds[b] = 0;
  }
}

template <class T>
__global__ void __launch_bounds__(256) prove_last_kernel(const uint8_t* __restrict__ done, int4* __restrict__ t_out, int4* __restrict__ z_out,
                                                         uint32_t t_quads, uint32_t z_quads, uint8_t* __restrict__ ok, uint64_t B) {
  const int4 zero = make_int4(0, 0, 0, 0);
  for (uint64_t b = blockIdx.x; b < B; b += gridDim.x) {
    const uint8_t dn = done[b];   // uniform over the workgroup
    if (threadIdx.x == 0) ok[b] = dn;
    if (dn) continue;
    for (uint32_t q = threadIdx.x; q < t_quads; q += 256) st_stream(t_out + b * t_quads + q, zero);
    for (uint32_t q = threadIdx.x; q < z_quads; q += 256) st_stream(z_out + b * z_quads + q, zero);
  }
}

// ---- the field-list kernels of the Linear and Sum loops: the same moves over up to kMaxFields slabs with
// per-field entry sizes, one launch per direction and round.  The list arrives by value (kernel arguments: scalar loads);
// the loop over it is unrolled so that no field is indexed at run time.
__global__ void __launch_bounds__(256) gather_fields_kernel(FieldList fl, const uint32_t* __restrict__ idx, uint32_t count) {
  for (uint32_t i = blockIdx.x; i < count; i += gridDim.x) {
    const uint64_t from = idx[i];
#pragma unroll
    for (uint32_t f = 0; f < kMaxFields; ++f) {
      if (f >= fl.n) break;
      const uint32_t quads = fl.quads[f];
      const int4* __restrict__ src = (const int4*)fl.src[f] + field_offset(from, quads);
      int4* __restrict__ dst = (int4*)fl.dst[f] + field_offset(i, quads);
      for (uint32_t q = threadIdx.x; q < quads; q += 256) dst[q] = ld_stream(src + q);
    }
  }
}

__global__ void __launch_bounds__(256) accept_scatter_fields_kernel(FieldList fl, const uint8_t* __restrict__ accept,
                                                                    const uint32_t* __restrict__ idx, uint32_t count, uint8_t rnd,
                                                                    uint8_t* __restrict__ rounds, uint8_t* __restrict__ done) {
  for (uint32_t i = blockIdx.x; i < count; i += gridDim.x) {
    if (accept[i] == 0) continue;   // uniform over the workgroup
    const uint64_t to = idx[i];
#pragma unroll
    for (uint32_t f = 0; f < kMaxFields; ++f) {
      if (f >= fl.n) break;
      const uint32_t quads = fl.quads[f];
      const int4* __restrict__ src = (const int4*)fl.src[f] + field_offset(i, quads);
      int4* __restrict__ dst = (int4*)fl.dst[f] + field_offset(to, quads);
      for (uint32_t q = threadIdx.x; q < quads; q += 256) st_stream(dst + q, ld_stream(src + q));
    }
    if (threadIdx.x == 0) {
      rounds[to] = rnd;
      done[to] = 1;
    }
  }
}

// prove_first_kernel with the commit flag compared against a wanted value (prove_live)
__global__ void __launch_bounds__(256) prove_first_want_kernel(const uint8_t* __restrict__ ok_commit, uint8_t wanted,
                                                               const uint8_t* __restrict__ ok_hash, const uint8_t* __restrict__ accept,
                                                               uint8_t* __restrict__ live, uint8_t* __restrict__ done,
                                                               uint8_t* __restrict__ rounds, uint64_t B) {
  for (uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x; b < B; b += (uint64_t)gridDim.x * 256) {
    const uint8_t l = prove_live(ok_commit[b], wanted, ok_hash[b]);
    live[b] = l;
    done[b] = (l && accept[b] != 0) ? 1 : 0;
    rounds[b] = 0;
  }
}

__global__ void __launch_bounds__(256) prove_last_fields_kernel(FieldList fl, const uint8_t* __restrict__ done, uint8_t* __restrict__ ok,
                                                                uint64_t B) {
  const int4 zero = make_int4(0, 0, 0, 0);
  for (uint64_t b = blockIdx.x; b < B; b += gridDim.x) {
    const uint8_t dn = done[b];   // uniform over the workgroup
    if (threadIdx.x == 0) ok[b] = dn;
    if (dn) continue;
#pragma unroll
    for (uint32_t f = 0; f < kMaxFields; ++f) {
      if (f >= fl.n) break;
      const uint32_t quads = fl.quads[f];
      int4* __restrict__ dst = (int4*)fl.dst[f] + field_offset(b, quads);
      for (uint32_t q = threadIdx.x; q < quads; q += 256) st_stream(dst + q, zero);
    }
  }
}

unsigned entry_grid(uint64_t entries, int num_cus) {   // one workgroup per entry under the cap
  const uint64_t cap = (uint64_t)num_cus * 8;
  const uint64_t blocks = entries < cap ? entries : cap;
  return (unsigned)(blocks < 1 ? 1 : blocks);
}
unsigned flat_grid(uint64_t items, int num_cus) {   // 256 items per workgroup under the cap
  return entry_grid((items + 255) / 256, num_cus);
}

template <class T>
const char* width_mark() {
  return std::is_same<T, int32_t>::value ? "<i32>" : "<i64>";
}
template <class C>
uint32_t quads_of(uint32_t rows, uint32_t N) { return rows * N * sizeof(C) / 16; }   // N >= 4: a whole number

}  // namespace

int launch_pending_compact(const LaunchCfg& cfg, const uint8_t* live, const uint8_t* done, uint64_t B, uint32_t* idx, uint32_t* count) {
  if (B >> 32) return -2;   // indices are uint32
  hipLaunchKernelGGL(pending_compact_kernel, dim3(1), dim3(kCompactTile), 0, (hipStream_t)cfg.stream, live, done, B, idx, count);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = "pending_compact_kernel";
  return 0;
}

template <class C>
int launch_prove_coins(const LaunchCfg& cfg, const C* a, const C* b, uint32_t N, int64_t* coin, uint64_t count) {
  if (count == 0) return 0;
  hipLaunchKernelGGL(coin_kernel<C>, dim3(flat_grid(count, cfg.num_cus)), dim3(256), 0, (hipStream_t)cfg.stream, a, b, N, coin, count);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = std::string("coin_kernel") + width_mark<C>();
  return 0;
}
RZK_BOTH_WIDTHS(launch_prove_coins)

template <class C>
int launch_gather_rows(const LaunchCfg& cfg, const C* src0, C* dst0, uint32_t rows0, const C* src1, C* dst1, uint32_t rows1, uint32_t N,
                       const uint32_t* idx, uint32_t count) {
  if (count == 0) return 0;
  GatherJob job{};
  job.src[0] = (const int4*)src0, job.dst[0] = (int4*)dst0, job.quads[0] = quads_of<C>(rows0, N);
  job.src[1] = (const int4*)src1, job.dst[1] = (int4*)dst1, job.quads[1] = src1 ? quads_of<C>(rows1, N) : 0;
  hipLaunchKernelGGL(gather_rows_kernel<C>, dim3(entry_grid(count, cfg.num_cus)), dim3(256), 0, (hipStream_t)cfg.stream, job, idx, count);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = std::string("gather_rows_kernel") + width_mark<C>();
  return 0;
}
RZK_BOTH_WIDTHS(launch_gather_rows)

template <class C>
int launch_accept_scatter(const LaunchCfg& cfg, const C* t, const C* z, C* t_out, C* z_out, uint32_t t_rows, uint32_t z_rows, uint32_t N,
                          const uint8_t* accept, const uint32_t* idx, uint32_t count, uint8_t rnd, uint8_t* rounds, uint8_t* done) {
  if (count == 0) return 0;
  const ScatterJob job{(const int4*)t, (const int4*)z, (int4*)t_out, (int4*)z_out, quads_of<C>(t_rows, N), quads_of<C>(z_rows, N)};
  hipLaunchKernelGGL(accept_scatter_kernel<C>, dim3(entry_grid(count, cfg.num_cus)), dim3(256), 0, (hipStream_t)cfg.stream, job, accept, idx,
                     count, rnd, rounds, done);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = std::string("accept_scatter_kernel") + width_mark<C>();
  return 0;
}
RZK_BOTH_WIDTHS(launch_accept_scatter)

int launch_prove_first(const LaunchCfg& cfg, const uint8_t* ok_commit, const uint8_t* ok_hash, const uint8_t* accept, uint8_t* live,
                       uint8_t* done, uint8_t* rounds, uint64_t B) {
  if (B == 0) return 0;
  hipLaunchKernelGGL(prove_first_kernel, dim3(flat_grid(B, cfg.num_cus)), dim3(256), 0, (hipStream_t)cfg.stream, ok_commit, ok_hash, accept,
                     live, done, rounds, B);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = "prove_first_kernel";
  return 0;
}

template <class C>
int launch_prove_last(const LaunchCfg& cfg, const uint8_t* done, C* t_out, C* z_out, uint32_t t_rows, uint32_t z_rows, uint32_t N,
                      uint8_t* ok, uint64_t B) {
  if (B == 0) return 0;
  hipLaunchKernelGGL(prove_last_kernel<C>, dim3(entry_grid(B, cfg.num_cus)), dim3(256), 0, (hipStream_t)cfg.stream, done, (int4*)t_out,
                     (int4*)z_out, quads_of<C>(t_rows, N), quads_of<C>(z_rows, N), ok, B);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = std::string("prove_last_kernel") + width_mark<C>();
  return 0;
}
RZK_BOTH_WIDTHS(launch_prove_last)

// a list the kernels can walk: 1 .. kMaxFields fields, every slab present and 16-byte aligned, no empty entry
static bool field_list_ok(const FieldList& fl, bool with_src) {
  if (fl.n < 1 || fl.n > kMaxFields) return false;
  uintptr_t bits = 0;
  for (uint32_t f = 0; f < fl.n; ++f) {
    if (!fl.dst[f] || (with_src && !fl.src[f]) || fl.quads[f] == 0) return false;
    bits |= (uintptr_t)fl.dst[f] | (with_src ? (uintptr_t)fl.src[f] : 0);
  }
  return (bits & 15u) == 0;
}

int launch_gather_fields(const LaunchCfg& cfg, const FieldList& fl, const uint32_t* idx, uint32_t count) {
  if (count == 0) return 0;
  if (!field_list_ok(fl, true)) return -2;
  hipLaunchKernelGGL(gather_fields_kernel, dim3(entry_grid(count, cfg.num_cus)), dim3(256), 0, (hipStream_t)cfg.stream, fl, idx, count);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = "gather_fields_kernel";
  return 0;
}

int launch_accept_scatter_fields(const LaunchCfg& cfg, const FieldList& fl, const uint8_t* accept, const uint32_t* idx, uint32_t count,
                                 uint8_t rnd, uint8_t* rounds, uint8_t* done) {
  if (count == 0) return 0;
  if (!field_list_ok(fl, true)) return -2;
  hipLaunchKernelGGL(accept_scatter_fields_kernel, dim3(entry_grid(count, cfg.num_cus)), dim3(256), 0, (hipStream_t)cfg.stream, fl, accept,
                     idx, count, rnd, rounds, done);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = "accept_scatter_fields_kernel";
  return 0;
}

int launch_prove_first_want(const LaunchCfg& cfg, const uint8_t* ok_commit, uint8_t wanted, const uint8_t* ok_hash, const uint8_t* accept,
                            uint8_t* live, uint8_t* done, uint8_t* rounds, uint64_t B) {
  if (B == 0) return 0;
  hipLaunchKernelGGL(prove_first_want_kernel, dim3(flat_grid(B, cfg.num_cus)), dim3(256), 0, (hipStream_t)cfg.stream, ok_commit, wanted,
                     ok_hash, accept, live, done, rounds, B);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = "prove_first_want_kernel";
  return 0;
}

int launch_prove_last_fields(const LaunchCfg& cfg, const FieldList& fl, const uint8_t* done, uint8_t* ok, uint64_t B) {
  if (B == 0) return 0;
  if (!field_list_ok(fl, false)) return -2;
  hipLaunchKernelGGL(prove_last_fields_kernel, dim3(entry_grid(B, cfg.num_cus)), dim3(256), 0, (hipStream_t)cfg.stream, fl, done, ok, B);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = "prove_last_fields_kernel";
  return 0;
}

}  // namespace rzk
