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
// Both kernels exist for int64_t slabs and for 32-bit slabs (reported as packed_encode_kernel<i32>, packed_decode_kernel<i32>;
// DESIGN.md §19) from one text (rzk_packed_kernels.inc): there a lane's piece of two coefficients is one 8-byte access (int2) and the raw rule
// runs in 32-bit arithmetic (packed_raw32).  Records carry no width.
#include <hip/hip_runtime.h>

#include <string>

#include "rzk_dev.h"
#include "rzk_packed.h"
#include "rzk_wave.h"

namespace rzk {

#define RZK_LAUNCH_CHECK()                      \
  do {                                          \
    hipError_t e_ = hipGetLastError();          \
    if (e_ != hipSuccess) return (int)e_;       \
  } while (0)

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

// The kernels' text, once per coefficient width (see the head of rzk_packed_kernels.inc).
#define RZK_PK_KERNEL(name) name
#define RZK_PK_COEF int64_t
#define RZK_PK_PAIR v2l
#define RZK_PK_RAW packed_raw
#define RZK_PK_UNBIAS(r, b) ((long)(r) - (long)(b))
#include "rzk_packed_kernels.inc"
#undef RZK_PK_KERNEL
#undef RZK_PK_COEF
#undef RZK_PK_PAIR
#undef RZK_PK_RAW
#undef RZK_PK_UNBIAS
#define RZK_PK_KERNEL(name) name##_i32
#define RZK_PK_COEF int32_t
#define RZK_PK_PAIR int2
#define RZK_PK_RAW packed_raw32
#define RZK_PK_UNBIAS(r, b) ((int)((r) - (b)))
#include "rzk_packed_kernels.inc"
#undef RZK_PK_KERNEL
#undef RZK_PK_COEF
#undef RZK_PK_PAIR
#undef RZK_PK_RAW
#undef RZK_PK_UNBIAS

uint64_t capped(uint64_t tasks, int num_cus) {   // workgroups of kWavesPerBlock tasks under the grid cap
  uint64_t blocks = (tasks + kWavesPerBlock - 1) / kWavesPerBlock;
  const uint64_t cap = (uint64_t)num_cus * kBlocksPerCu;
  return blocks < cap ? blocks : cap;
}

}  // namespace

int launch_packed_encode(const LaunchCfg& cfg, const PackedSchema& s, const PackedSlabs& sl, uint64_t* rec, uint8_t* ok, uint64_t B,
                         uint32_t width) {
  const uint64_t npolys = B * s.polys;
  if (npolys == 0) return 0;
  hipLaunchKernelGGL(width == 4 ? packed_encode_kernel_i32 : packed_encode_kernel, dim3((unsigned)capped(npolys, cfg.num_cus)), dim3(64 * kWavesPerBlock), 0,
                     (hipStream_t)cfg.stream, s, sl, rec, ok, npolys);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = width == 4 ? "packed_encode_kernel<i32>" : "packed_encode_kernel";
  return 0;
}

int launch_packed_decode(const LaunchCfg& cfg, const PackedSchema& s, const PackedSlabs& sl, const uint64_t* rec, uint8_t* ok,
                         uint64_t B, uint32_t width) {
  const uint64_t npolys = B * s.polys;
  if (npolys == 0) return 0;
  hipLaunchKernelGGL(width == 4 ? packed_decode_kernel_i32 : packed_decode_kernel, dim3((unsigned)capped(npolys, cfg.num_cus)), dim3(64 * kWavesPerBlock), 0,
                     (hipStream_t)cfg.stream, s, sl, rec, ok, npolys);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = width == 4 ? "packed_decode_kernel<i32>" : "packed_decode_kernel";
  return 0;
}

}  // namespace rzk
