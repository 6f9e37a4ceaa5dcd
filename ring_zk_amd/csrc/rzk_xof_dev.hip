// rzk_xof_dev.hip — batched "XP1" expansion of 32-byte seeds into uniform polynomials (format and scalar form: rzk_xof.h,
// DESIGN.md §14).  One launch:
//   xof_uniform_kernel   one lane per chunk (min(N, 256) coefficients of one polynomial), Keccak state in registers; a
//                        workgroup is one wavefront, task t = (b * rows + r) * C + c writes out[t * CH .. (t + 1) * CH).
//                        The lanes of a wavefront reject different words, so they fill their chunks at different speeds:
//                        the squeeze loop runs wave-uniformly while any lane is short of its chunk, and a lane that has
//                        it takes no further word.  A lane's chunk is up to 2 KiB of contiguous int64, so lane-private
//                        stores would touch 64 cache lines per instruction: every lane appends the accepted candidates
//                        of the current block (at most 34) to a 64-entry ring of its own in LDS (odd row stride), and
//                        after each block the wavefront drains whole segments of SEG = min(CH, 16) values from all
//                        rows together, SEG / 2 consecutive lanes per row and one 16-byte piece (two centred values)
//                        per lane: 128 contiguous bytes per row.  A row holds fewer than SEG values before a block and
//                        at most SEG - 1 + 34 <= 49 after it; CH is a multiple of SEG, so a finished chunk is drained
//                        completely and every coefficient is stored exactly once.
// Grid-stride over wavefront-sized groups of tasks under the context's grid cap: results do not depend on the grid.
#include <hip/hip_runtime.h>

#include "rzk_dev.h"
#include "rzk_xof.h"

namespace rzk {

namespace {

constexpr uint32_t kRing = 64;               // ring entries per row (power of two, >= 15 + 34)
constexpr uint32_t kRingStride = kRing + 1;  // odd: the 64 rows start on distinct banks
constexpr uint32_t kSegMax = 16;             // values per drained segment: 128 bytes of output
constexpr uint32_t kBlocksPerCu = 8;
static_assert(kSegMax - 1 + kXofBlockWords32 <= kRing, "a row's ring holds what one block can add to an undrained rest");
static_assert(kXofChunkMax % kSegMax == 0, "a finished chunk drains completely");

__device__ __forceinline__ bool wave_any(bool p) { return __builtin_amdgcn_ballot_w64(p) != 0; }

struct RingPut {   // the lane's row of the ring
  uint32_t* row;
  __host__ __device__ void operator()(uint32_t i, uint32_t raw) const { row[i & (kRing - 1)] = raw; }
};

typedef long v2l __attribute__((ext_vector_type(2)));

__global__ void __launch_bounds__(64) xof_uniform_kernel(XofJob j, const uint64_t* __restrict__ seeds, int64_t* __restrict__ out,
                                                         uint64_t ntasks) {
  __shared__ uint32_t ring[64 * kRingStride];
  __shared__ uint32_t s_cnt[64], s_done[64];   // values appended to / drained from every row so far
  const uint32_t lane = threadIdx.x;
  const uint32_t ch = xof_chunk_len(j.N);
  const uint32_t seg = ch < kSegMax ? ch : kSegMax;
  const uint32_t lpr_log = (uint32_t)__builtin_ctz(seg) - 1;   // lanes per row of a drain step = seg / 2 (N >= 4: seg >= 4)
  const uint32_t lpr = 1u << lpr_log, rows_per_step = 64u >> lpr_log;
  const uint64_t per_seed = (uint64_t)j.rows * j.chunks;
  const int64_t half = (int64_t)((j.q - 1) / 2);
  const uint32_t q32 = (uint32_t)j.q;
  RingPut put{ring + lane * kRingStride};
  for (uint64_t t0 = (uint64_t)blockIdx.x * 64; t0 < ntasks; t0 += (uint64_t)gridDim.x * 64) {
    const uint64_t t = t0 + lane;
    const bool live = t < ntasks;
    const uint32_t need = live ? ch : 0;   // a lane past the end takes no word and owns no output
    const uint64_t b = live ? t / per_seed : 0;
    const uint32_t rc = (uint32_t)(live ? t - b * per_seed : 0);
    const uint32_t r = rc / j.chunks, c = rc - r * j.chunks;
    uint64_t s[25];
    {
      const uint64_t* sp = seeds + b * 4;
      const uint64_t sw[4] = {sp[0], sp[1], sp[2], sp[3]};
      xof_start(s, j.q, j.N, j.domain, sw, j.p0 + r, c);
    }
    uint32_t cnt = 0, done = 0;
    for (;;) {
      // the 34 words of the block in s[0 .. 16]: constant state indices, a finished lane appends nothing
#pragma unroll
      for (uint32_t w = 0; w < kShakeRateWords; ++w) {
        xof_take((uint32_t)s[w], q32, j.mask, need, cnt, put);
        xof_take((uint32_t)(s[w] >> 32), q32, j.mask, need, cnt, put);
      }
      s_cnt[lane] = cnt;
      s_done[lane] = done;
      __syncthreads();
      // drain: pass k stores segment k of every row's undrained values, while any row has one
      for (uint32_t pass = 0;; ++pass) {
        bool more = false;
        for (uint32_t step = 0; step < lpr; ++step) {
          const uint32_t row = step * rows_per_step + (lane >> lpr_log), piece = lane & (lpr - 1);
          const uint32_t at = s_done[row] + pass * seg, have = s_cnt[row];
          if (at + seg <= have) {   // (rows of lanes past the end have 0: they store nothing)
            const uint32_t* rr = ring + row * kRingStride;
            const uint32_t i = at + 2 * piece;   // even, so i and i + 1 do not straddle the ring's end
            v2l v;
            v.x = (int64_t)rr[i & (kRing - 1)] - half;
            v.y = (int64_t)rr[(i + 1) & (kRing - 1)] - half;
            *reinterpret_cast<v2l*>(out + (t0 + row) * ch + i) = v;
            more |= at + 2 * seg <= have;
          }
        }
        if (!wave_any(more)) break;
      }
      done = cnt - (cnt & (seg - 1));
      __syncthreads();   // the rows are drained before the next block (or the next trip) appends to them
      if (!wave_any(cnt < need)) break;
      keccak_f1600(s);
    }
  }
}

}  // namespace

int launch_xof_uniform(const LaunchCfg& cfg, const XofJob& j, const uint64_t* seeds, int64_t* out, uint64_t B) {
  const uint64_t ntasks = B * j.rows * j.chunks;
  if (ntasks == 0) return 0;
  uint64_t blocks = (ntasks + 63) / 64;
  const uint64_t cap = (uint64_t)cfg.num_cus * kBlocksPerCu;
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(xof_uniform_kernel, dim3((unsigned)blocks), dim3(64), 0, (hipStream_t)cfg.stream, j, seeds, out, ntasks);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = "xof_uniform_kernel";
  return 0;
}

}  // namespace rzk
