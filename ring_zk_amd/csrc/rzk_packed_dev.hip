// rzk_packed_dev.hip — the fixed-width packed proof format on the device (format: rzk_packed.h).
// Every record of a kind has the same size, so both directions are one launch: no walk, no scan, no host
// synchronisation, no atomics.  One wavefront per polynomial, four independent wavefronts per workgroup, grid-stride
// loops under the context's grid cap.  A polynomial is handled in trips of 128 coefficients = 2 W whole 64-bit words
// (128 W bits), so a trip never shares a word with its neighbour; N < 128 is one shorter trip.
//   packed_encode_kernel   lane l of trip t loads coefficients 128 t + 2 l, + 1 as one 16-byte piece (lane-consecutive,
//                          as reject_stat_kernel does), range-tests and biases them (packed_raw: the all-ones marker for
//                          a coefficient out of range) and leaves the two raw values in the wavefront's 512-byte LDS tile;
//                          lane m < 2 W then assembles output word m from the 2 .. 5 tile entries it draws on (33 for
//                          class D) and stores it: 8-byte stores, lane-consecutive, every word written once by one lane.
//   packed_decode_kernel   lane m < 2 W of trip t loads word m of the trip (8 bytes, lane-consecutive) into the tile — no
//                          lane reads past the polynomial's own words — and lane l extracts coefficients 2 l, 2 l + 1 from
//                          the one or two tile words they span, tests them against the limit, removes the bias and stores
//                          one 16-byte piece.  The lane that loaded the last word tests the padding bits.
// The wavefront of a record's first polynomial also writes / checks the header word.  ok[] is preset to 1 by the entry
// point; a wavefront that meets a fault stores 0 (every writer stores the same value).  No scratch memory.
// Both kernels are templates over the coefficient type of the slabs, int64_t or the 32-bit slabs' int32_t (reported as
// packed_encode_kernel<i32>, packed_decode_kernel<i32>): there a lane's piece of two coefficients is one
// 8-byte access (int2) and the raw rule runs in 32-bit arithmetic (packed_raw32).  Records carry no width.
#include <hip/hip_runtime.h>

#include <string>

#include "rzk_dev.h"
#include "rzk_packed.h"
#include "rzk_wave.h"

namespace rzk {

namespace {

constexpr uint32_t kWavesPerBlock = 4;
constexpr uint32_t kBlocksPerCu = 8;     // 32 wavefronts per CU
constexpr uint32_t kTripCoefs = 128;     // coefficients per trip: two per lane

typedef long v2l __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t wave_index() {   // wave-uniform, in scalar registers
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
}
__device__ __forceinline__ bool wave_any(bool p) { return __builtin_amdgcn_ballot_w64(p) != 0; }

struct PolyTask {   // where polynomial p of the batch lives; wave-uniform
  uint64_t b;       // record
  uint32_t j;       // polynomial of the record
  uint32_t f;       // its field
  uint64_t coef;    // index of its first coefficient in the field's slab
  uint64_t word;    // index of its first word in the record buffer
};
__device__ __forceinline__ PolyTask poly_task(const PackedSchema& s, uint64_t p) {
  PolyTask t;
  t.b = p / s.polys;
  t.j = (uint32_t)(p - t.b * s.polys);
  t.f = packed_field_of(s, t.j);
  const PackedField& F = s.f[t.f];
  const uint32_t r = t.j - s.first[t.f];
  t.coef = (t.b * F.rows + r) * (uint64_t)s.N;
  t.word = t.b * s.rec_words + F.woff + (uint64_t)r * F.wpp;
  return t;
}

// What the kernels take from the coefficient type C of the slabs (PackedSlabs carries addresses):
//   Pair           a lane's piece of two coefficients: v2l, one 16-byte access / int2, one 8-byte access.  Slabs are 16-byte
//                  aligned and a piece starts at an even coefficient, so both are naturally aligned
//   raw            packed_raw / packed_raw32 (rzk_packed.h)
//   unbias(r, b)   the decoded coefficient r - b in the slab's type (a valid r is at most 2 b, so it fits an int32_t; the
//                  value of a rejected record is unspecified at either width)
template <class C>
struct PackedCoef;
template <>
struct PackedCoef<int64_t> {
  using Pair = v2l;
  static __device__ __forceinline__ bool raw(int64_t v, const PackedWidth& w, uint32_t* r) { return packed_raw(v, w, r); }
  static __device__ __forceinline__ long unbias(uint32_t r, uint32_t b) { return ((long)(r) - (long)(b)); }
};
template <>
struct PackedCoef<int32_t> {
  using Pair = int2;
  static __device__ __forceinline__ bool raw(int32_t v, const PackedWidth& w, uint32_t* r) { return packed_raw32(v, w, r); }
  static __device__ __forceinline__ int unbias(uint32_t r, uint32_t b) { return ((int)((r) - (b))); }
};
template <class C>
using PackedPair = typename PackedCoef<C>::Pair;

template <class C>
__global__ void __launch_bounds__(64 * kWavesPerBlock) packed_encode_kernel(PackedSchema s, PackedSlabs sl, uint64_t* __restrict__ rec,
                                                                            uint8_t* __restrict__ ok, uint64_t npolys) {
  __shared__ uint32_t tile_all[kWavesPerBlock][kTripCoefs];
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t* tile = tile_all[wave_index()];
  const uint32_t trips = (s.N + kTripCoefs - 1) / kTripCoefs;
  const uint32_t ncoef = s.N < kTripCoefs ? s.N : kTripCoefs;   // coefficients per trip (N is a power of two)
  for (uint64_t p = (uint64_t)blockIdx.x * kWavesPerBlock + wave_index(); p < npolys;
       p += (uint64_t)gridDim.x * kWavesPerBlock) {
    const PolyTask t = poly_task(s, p);
    const PackedWidth w = s.w[s.f[t.f].cls];
    const C* src = reinterpret_cast<const C*>(sl.ptr[t.f]) + t.coef;
    uint64_t* dst = rec + t.word;
    if (t.j == 0 && lane == 0) rec[t.b * s.rec_words] = packed_header(s.kind, s.V);
    bool bad = false;
    const bool active = 2u * lane < ncoef;   // (N >= 4 is even: a piece never straddles the end)
    const uint32_t nw = (ncoef * w.W + 63u) / 64u;   // words of one trip, at most 2 W <= 64
    // Loads are unconditional, so that the next trip's piece stays in flight while this one is packed (a load under a
    // branch makes the compiler wait for everything outstanding): an idle lane (N < 128) re-reads the polynomial's first
    // piece and the last trip re-reads itself; both stay inside the polynomial and their values are not used (the indices
    // count coefficients, so this holds at either width).
    const uint32_t at = active ? 2u * lane : 0u;
    PackedPair<C> cc = *reinterpret_cast<const PackedPair<C>*>(src + at);
    for (uint32_t tr = 0; tr < trips; ++tr) {
      const uint32_t tn = tr + 1 < trips ? tr + 1 : tr;
      const PackedPair<C> next = *reinterpret_cast<const PackedPair<C>*>(src + tn * kTripCoefs + at);
      uint32_t r0 = 0, r1 = 0;
      if (active) {
        bad |= !PackedCoef<C>::raw((C)cc.x, w, &r0);
        bad |= !PackedCoef<C>::raw((C)cc.y, w, &r1);
      }
      wave_sync();   // the previous trip's reads of the tile are over
      *reinterpret_cast<uint2*>(tile + 2u * lane) = make_uint2(r0, r1);   // lanes past the end store zeros: the padding
      wave_sync();
      if (lane < nw) {
        const uint32_t bit0 = 64u * lane;
        uint64_t word = 0;
        for (uint32_t i = packed_div(bit0, w); i < kTripCoefs && i * w.W < bit0 + 64u; ++i) {
          const int32_t sh = (int32_t)(i * w.W) - (int32_t)bit0;   // -W < sh < 64
          const uint64_t v = tile[i];
          word |= sh >= 0 ? v << sh : v >> (-sh);
        }
        dst[(uint64_t)tr * 2u * w.W + lane] = word;
      }
      cc = next;
    }
    if (wave_any(bad) && lane == 0) ok[t.b] = 0;
  }
}

template <class C>
__global__ void __launch_bounds__(64 * kWavesPerBlock) packed_decode_kernel(PackedSchema s, PackedSlabs sl, const uint64_t* __restrict__ rec,
                                                                            uint8_t* __restrict__ ok, uint64_t npolys) {
  __shared__ uint64_t tile_all[kWavesPerBlock][64];
  const uint32_t lane = threadIdx.x & 63u;
  uint64_t* tile = tile_all[wave_index()];
  const uint32_t trips = (s.N + kTripCoefs - 1) / kTripCoefs;
  const uint32_t ncoef = s.N < kTripCoefs ? s.N : kTripCoefs;   // coefficients per trip (N is a power of two)
  for (uint64_t p = (uint64_t)blockIdx.x * kWavesPerBlock + wave_index(); p < npolys;
       p += (uint64_t)gridDim.x * kWavesPerBlock) {
    const PolyTask t = poly_task(s, p);
    const PackedWidth w = s.w[s.f[t.f].cls];
    const uint64_t* src = rec + t.word;
    C* dst = reinterpret_cast<C*>(sl.ptr[t.f]) + t.coef;
    const uint64_t mask = (1ull << w.W) - 1;
    bool bad = false;
    if (t.j == 0 && lane == 0) bad = rec[t.b * s.rec_words] != packed_header(s.kind, s.V);
    const uint32_t bits = ncoef * w.W;
    const uint32_t nw = (bits + 63u) / 64u;   // words of one trip, at most 2 W <= 64
    // unconditional loads, as in the encoder: a lane past the trip's words re-reads word 0, the last trip itself
    const uint32_t at = lane < nw ? lane : 0u;
    uint64_t word = src[at];
    for (uint32_t tr = 0; tr < trips; ++tr) {
      const uint32_t tn = tr + 1 < trips ? tr + 1 : tr;
      const uint64_t next = src[(uint64_t)tn * 2u * w.W + at];
      wave_sync();   // the previous trip's reads of the tile are over
      if (lane < nw) {
        tile[lane] = word;
        if (lane == nw - 1 && (bits & 63u)) bad |= (word >> (bits & 63u)) != 0;   // padding bits
      }
      wave_sync();
      if (2u * lane < ncoef) {
        uint32_t raw[2];
#pragma unroll
        for (uint32_t e = 0; e < 2; ++e) {
          const uint32_t bit = (2u * lane + e) * w.W;
          const uint32_t sh = bit & 63u;
          uint64_t v = tile[bit >> 6] >> sh;
          if (sh + w.W > 64u) v |= tile[(bit >> 6) + 1] << (64u - sh);   // the next word exists: the coefficient ends inside the trip
          raw[e] = (uint32_t)(v & mask);
          bad |= raw[e] > w.limit;
        }
        PackedPair<C> out;
        out.x = PackedCoef<C>::unbias(raw[0], w.bias);
        out.y = PackedCoef<C>::unbias(raw[1], w.bias);
        *reinterpret_cast<PackedPair<C>*>(dst + tr * kTripCoefs + 2u * lane) = out;
      }
      word = next;
    }
    if (wave_any(bad) && lane == 0) ok[t.b] = 0;
  }
}

uint64_t capped(uint64_t tasks, int num_cus) {   // workgroups of kWavesPerBlock tasks under the grid cap
  uint64_t blocks = (tasks + kWavesPerBlock - 1) / kWavesPerBlock;
  const uint64_t cap = (uint64_t)num_cus * kBlocksPerCu;
  return blocks < cap ? blocks : cap;
}

}  // namespace

template <class C>
int launch_packed_encode(const LaunchCfg& cfg, const PackedSchema& s, const PackedSlabs& sl, uint64_t* rec, uint8_t* ok, uint64_t B) {
  const uint64_t npolys = B * s.polys;
  if (npolys == 0) return 0;
  hipLaunchKernelGGL(packed_encode_kernel<C>, dim3((unsigned)capped(npolys, cfg.num_cus)), dim3(64 * kWavesPerBlock), 0,
                     (hipStream_t)cfg.stream, s, sl, rec, ok, npolys);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = sizeof(C) == 4 ? "packed_encode_kernel<i32>" : "packed_encode_kernel";
  return 0;
}
RZK_BOTH_WIDTHS(launch_packed_encode)

template <class C>
int launch_packed_decode(const LaunchCfg& cfg, const PackedSchema& s, const PackedSlabs& sl, const uint64_t* rec, uint8_t* ok, uint64_t B) {
  const uint64_t npolys = B * s.polys;
  if (npolys == 0) return 0;
  hipLaunchKernelGGL(packed_decode_kernel<C>, dim3((unsigned)capped(npolys, cfg.num_cus)), dim3(64 * kWavesPerBlock), 0,
                     (hipStream_t)cfg.stream, s, sl, rec, ok, npolys);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = sizeof(C) == 4 ? "packed_decode_kernel<i32>" : "packed_decode_kernel";
  return 0;
}
RZK_BOTH_WIDTHS(launch_packed_decode)

}  // namespace rzk
