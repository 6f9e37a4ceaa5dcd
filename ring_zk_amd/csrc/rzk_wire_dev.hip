// rzk_wire_dev.hip — batched GPU codec of the reference's serialized protocol messages (include/rzk.h "protocol
// messages on the wire"; schema and walk in rzk_wire_walk.h).
//
// Decode, two launches:
//   wire_walk_kernel   one lane per message: checks the span, walks the length prefixes (latency bound: a few
//                      dependent loads per polynomial) and writes one (position << 16 | len) entry per polynomial
//                      into the context's scratch table, and ok[b].
//   wire_copy_kernel   one wavefront per polynomial, grid-stride over B x polys: widens the coefficients to int64,
//                      range-checks them, zero-fills len .. N-1 (bandwidth bound); a bad coefficient clears ok[b].
// Encode, four launches:
//   wire_len_kernel        one wavefront per polynomial: trimmed length (last non-zero index, wave max) and the
//                          canonical test of every coefficient (raises the context's input-fault word).
//   wire_msg_scan_kernel   one workgroup per message: exclusive scan of the polynomials' sizes -> the position of
//                          every polynomial's len prefix inside its message, and the message size.
//   wire_batch_scan_kernel one workgroup: exclusive scan of the message sizes -> offsets[0 .. B].
//   wire_write_kernel      one wavefront per polynomial: the structural prefixes in front of it (lane 0), its len
//                          prefix and its coefficients.
// Every store is an ordinary vector store from C++.  Message starts are multiples of coef_bytes (checked) and every
// field is 8 or coef_bytes bytes wide, so coefficient and prefix accesses are naturally aligned, except behind the
// 1-byte Option tag of an Opening: those go byte by byte.
#include <hip/hip_runtime.h>

#include "rzk_dev.h"
#include "rzk_wire_walk.h"

namespace rzk {

namespace {

constexpr int kWaves = 4;   // wavefronts per workgroup of the per-polynomial kernels

unsigned wave_grid(uint64_t tasks, int num_cus) {
  uint64_t blocks = (tasks + kWaves - 1) / kWaves;
  const uint64_t cap = (uint64_t)num_cus * 16;
  if (blocks > cap) blocks = cap;
  return (unsigned)(blocks ? blocks : 1);
}

struct WalkEmit {
  uint64_t* tab;   // this message's entries
  uint64_t base;   // message start in the byte buffer
  __device__ void operator()(uint32_t j, uint64_t pos, uint32_t len) { tab[j] = ((base + pos) << 16) | len; }
};

__device__ inline void wire_store_u64(uint8_t* p, uint64_t v) {
  if (((uintptr_t)p & 3u) == 0) {
    uint32_t* w = (uint32_t*)p;
    w[0] = (uint32_t)v;
    w[1] = (uint32_t)(v >> 32);
  } else {
    for (int i = 0; i < 8; ++i) p[i] = (uint8_t)(v >> (8 * i));
  }
}

__device__ inline int64_t wire_load_coef(const uint8_t* p, uint32_t cb, bool aligned) {
  if (aligned) return cb == 8 ? *(const int64_t*)p : (int64_t)*(const int32_t*)p;
  uint64_t v = 0;
  for (uint32_t i = 0; i < cb; ++i) v |= (uint64_t)p[i] << (8 * i);
  return cb == 8 ? (int64_t)v : (int64_t)(int32_t)(uint32_t)v;
}

__device__ inline void wire_store_coef(uint8_t* p, int64_t v, uint32_t cb, bool aligned) {
  if (aligned) {
    if (cb == 8) *(int64_t*)p = v;
    else *(int32_t*)p = (int32_t)v;
    return;
  }
  for (uint32_t i = 0; i < cb; ++i) p[i] = (uint8_t)((uint64_t)v >> (8 * i));
}

// slab row of polynomial j of message b
__device__ inline int64_t* wire_row(const WireSchema& s, const WireSlabs& sl, uint64_t b, uint32_t j, uint32_t* fout) {
  const uint32_t f = wire_field_of(s, j);
  *fout = f;
  int64_t* base = sl.ptr[f];
  if (!base) return nullptr;
  const uint64_t rows = s.first[f + 1] - s.first[f];
  return base + (b * rows + (j - s.first[f])) * (uint64_t)s.N;
}

__global__ void __launch_bounds__(256) wire_walk_kernel(const uint8_t* __restrict__ bytes, uint64_t total,
                                                        const uint64_t* __restrict__ offsets, WireSchema s,
                                                        int need_align, uint64_t* __restrict__ tab,
                                                        uint8_t* __restrict__ ok, uint64_t B) {
  for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < B; b += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t o0 = offsets[b], o1 = offsets[b + 1];
    bool good = o0 <= o1 && o1 <= total && (!need_align || o0 % s.coef_bytes == 0);
    if (good) {   // a message outside the buffer, inverted or misaligned is not read at all
      WalkEmit e{tab + b * s.polys, o0};
      good = wire_walk(bytes + o0, o1 - o0, s, e);
    }
    ok[b] = good ? 1 : 0;
  }
}

__global__ void __launch_bounds__(256) wire_copy_kernel(const uint8_t* __restrict__ bytes,
                                                        const uint64_t* __restrict__ tab, WireSchema s, WireSlabs sl,
                                                        int64_t half, uint8_t* ok, uint64_t npoly) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t nw = (uint64_t)gridDim.x * kWaves;
  const uint32_t N = s.N, cb = s.coef_bytes;
  for (uint64_t i = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); i < npoly; i += nw) {
    const uint64_t b = i / s.polys;
    const uint32_t j = (uint32_t)(i - b * s.polys);
    if (!ok[b]) continue;   // rejected by the walk (its table entries are not valid) or by another wave
    const uint64_t e = tab[i];
    const uint32_t len = (uint32_t)(e & 0xffffu);
    uint32_t f;
    int64_t* dst = wire_row(s, sl, b, j, &f);
    if (len == kWireNone) {   // Option None: the constant 1 (Commitment::verify with Some(1) == None)
      for (uint32_t t = lane; t < N; t += 64) dst[t] = t == 0 ? 1 : 0;
      continue;
    }
    const uint8_t* src = bytes + (e >> 16);
    const bool aligned = ((uintptr_t)src % cb) == 0;
    bool bad = false;
#pragma unroll 4
    for (uint32_t t = lane; t < N; t += 64) {
      int64_t v = 0;
      if (t < len) {
        v = wire_load_coef(src + (uint64_t)t * cb, cb, aligned);
        bad |= v > half || v < -half;
      }
      dst[t] = v;
    }
    if (bad) ok[b] = 0;   // every writer stores the same 0
  }
}

__global__ void __launch_bounds__(256) wire_len_kernel(WireSchema s, WireSlabs sl, int64_t half,
                                                       uint32_t* __restrict__ lens, uint32_t* bad_word,
                                                       uint64_t npoly) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t nw = (uint64_t)gridDim.x * kWaves;
  const uint32_t N = s.N;
  for (uint64_t i = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); i < npoly; i += nw) {
    const uint64_t b = i / s.polys;
    const uint32_t j = (uint32_t)(i - b * s.polys);
    uint32_t f;
    const int64_t* src = wire_row(s, sl, b, j, &f);
    if (!src) {   // Option with no slab: None
      if (lane == 0) lens[i] = kWireNone;
      continue;
    }
    int last = -1;
    bool bad = false;
#pragma unroll 4
    for (uint32_t t = lane; t < N; t += 64) {
      const int64_t v = src[t];
      if (v != 0) last = (int)t;
      bad |= v > half || v < -half;
    }
    for (int m = 32; m > 0; m >>= 1) last = max(last, __shfl_xor(last, m));
    if (lane == 0) lens[i] = (uint32_t)(last + 1);
    if (bad && bad_word) *bad_word = 1u;
  }
}

// exclusive scan of one value per thread of a workgroup of T threads; *total = sum over the workgroup
template <int T>
__device__ uint64_t block_exscan(uint64_t v, uint64_t* sh, uint64_t* total) {
  const int tid = threadIdx.x;
  sh[tid] = v;
  __syncthreads();
  for (int d = 1; d < T; d <<= 1) {
    const uint64_t a = tid >= d ? sh[tid - d] : 0;
    __syncthreads();
    sh[tid] += a;
    __syncthreads();
  }
  const uint64_t incl = sh[tid];
  *total = sh[T - 1];
  __syncthreads();
  return incl - v;
}

__global__ void __launch_bounds__(256) wire_msg_scan_kernel(WireSchema s, const uint32_t* __restrict__ lens,
                                                            uint64_t* __restrict__ rel, uint64_t* __restrict__ msize,
                                                            uint64_t B) {
  __shared__ uint64_t sh[256];
  const uint64_t st = wire_struct_total(s);
  for (uint64_t b = blockIdx.x; b < B; b += gridDim.x) {
    uint64_t carry = 0;
    for (uint32_t j0 = 0; j0 < s.polys; j0 += 256) {
      const uint32_t j = j0 + threadIdx.x;
      uint64_t sz = 0;
      if (j < s.polys) {
        const uint32_t len = lens[b * s.polys + j];
        sz = len == kWireNone ? 0 : 8 + (uint64_t)len * s.coef_bytes;
      }
      uint64_t tot;
      const uint64_t ex = block_exscan<256>(sz, sh, &tot);
      if (j < s.polys) rel[b * s.polys + j] = carry + ex + wire_struct_before(s, j);
      carry += tot;
    }
    if (threadIdx.x == 0) msize[b] = carry + st;
  }
}

__global__ void __launch_bounds__(1024) wire_batch_scan_kernel(const uint64_t* __restrict__ msize,
                                                               uint64_t* __restrict__ offsets, uint64_t B) {
  __shared__ uint64_t sh[1024];
  uint64_t carry = 0;
  for (uint64_t b0 = 0; b0 < B; b0 += 1024) {
    const uint64_t b = b0 + threadIdx.x;
    uint64_t tot;
    const uint64_t ex = block_exscan<1024>(b < B ? msize[b] : 0, sh, &tot);
    if (b < B) offsets[b] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) offsets[B] = carry;
}

struct PrefixPut {
  uint8_t* p;
  __device__ void operator()(uint64_t v, int nb) {
    if (nb == 8) wire_store_u64(p, v);
    else *p = (uint8_t)v;
    p += nb;
  }
};
struct PrefixCount {
  __device__ void operator()(uint64_t, int) {}
};

__global__ void __launch_bounds__(256) wire_write_kernel(WireSchema s, WireSlabs sl, const uint32_t* __restrict__ lens,
                                                         const uint64_t* __restrict__ rel,
                                                         const uint64_t* __restrict__ offsets,
                                                         uint8_t* __restrict__ bytes, uint64_t npoly) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t nw = (uint64_t)gridDim.x * kWaves;
  const uint32_t cb = s.coef_bytes;
  for (uint64_t i = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); i < npoly; i += nw) {
    const uint64_t b = i / s.polys;
    const uint32_t j = (uint32_t)(i - b * s.polys);
    const uint32_t len = lens[i];
    uint8_t* dst = bytes + offsets[b] + rel[i];   // this polynomial's len prefix
    if (lane == 0) {
      PrefixCount cnt;
      const uint32_t nb = wire_prefixes(s, j, len != kWireNone, cnt);
      PrefixPut put{dst - nb};
      wire_prefixes(s, j, len != kWireNone, put);
      if (len != kWireNone) wire_store_u64(dst, len);
    }
    if (len == kWireNone) continue;
    uint32_t f;
    const int64_t* src = wire_row(s, sl, b, j, &f);
    uint8_t* out = dst + 8;
    const bool aligned = ((uintptr_t)out % cb) == 0;
#pragma unroll 4
    for (uint32_t t = lane; t < len; t += 64) wire_store_coef(out + (uint64_t)t * cb, src[t], cb, aligned);
  }
}

}  // namespace

int launch_wire_walk(const LaunchCfg& cfg, const uint8_t* bytes, uint64_t total, const uint64_t* offsets,
                     const WireSchema& s, int need_align, uint64_t* tab, uint8_t* ok, uint64_t B) {
  if (B == 0) return 0;
  uint64_t blocks = (B + 63) / 64;
  const uint64_t cap = (uint64_t)cfg.num_cus * 4;
  if (blocks > cap) blocks = cap;
  // 64-thread workgroups: one message per lane, spread over as many CUs as there are
  hipLaunchKernelGGL(wire_walk_kernel, dim3((unsigned)blocks), dim3(64), 0, (hipStream_t)cfg.stream, bytes, total,
                     offsets, s, need_align, tab, ok, B);
  RZK_LAUNCH_CHECK();
  return 0;
}

int launch_wire_copy(const LaunchCfg& cfg, const uint8_t* bytes, const uint64_t* tab, const WireSchema& s,
                     const WireSlabs& sl, int64_t half, uint8_t* ok, uint64_t B) {
  const uint64_t npoly = B * s.polys;
  if (npoly == 0) return 0;
  hipLaunchKernelGGL(wire_copy_kernel, dim3(wave_grid(npoly, cfg.num_cus)), dim3(64 * kWaves), 0,
                     (hipStream_t)cfg.stream, bytes, tab, s, sl, half, ok, npoly);
  RZK_LAUNCH_CHECK();
  return 0;
}

int launch_wire_encode(const LaunchCfg& cfg, const WireSchema& s, const WireSlabs& sl, int64_t half, uint32_t* lens,
                       uint64_t* rel, uint64_t* msize, uint8_t* bytes, uint64_t* offsets, uint32_t* bad_word,
                       uint64_t B) {
  const uint64_t npoly = B * s.polys;
  if (B == 0) return 0;
  const hipStream_t st = (hipStream_t)cfg.stream;
  const dim3 grid(wave_grid(npoly, cfg.num_cus));
  hipLaunchKernelGGL(wire_len_kernel, grid, dim3(64 * kWaves), 0, st, s, sl, half, lens, bad_word, npoly);
  RZK_LAUNCH_CHECK();
  const uint64_t mb = B < (uint64_t)cfg.num_cus * 16 ? B : (uint64_t)cfg.num_cus * 16;
  hipLaunchKernelGGL(wire_msg_scan_kernel, dim3((unsigned)mb), dim3(256), 0, st, s, lens, rel, msize, B);
  RZK_LAUNCH_CHECK();
  hipLaunchKernelGGL(wire_batch_scan_kernel, dim3(1), dim3(1024), 0, st, msize, offsets, B);
  RZK_LAUNCH_CHECK();
  hipLaunchKernelGGL(wire_write_kernel, grid, dim3(64 * kWaves), 0, st, s, sl, lens, rel, offsets, bytes, npoly);
  RZK_LAUNCH_CHECK();
  return 0;
}

}  // namespace rzk
