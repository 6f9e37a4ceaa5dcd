// rzk_csprng_dev.hip — the keyed device samplers: uniform, Gaussian and challenge polynomials drawn from ChaCha20 blocks
// (stream definition and word-to-coefficient maps: rzk_chacha.h), and the exact discrete Gaussian
// (rzk_dgauss.h; its kernel is described where it stands).  Same distributions, launch shapes and
// store discipline as the seeded samplers (rzk_sample.h); only the source of the words differs.
//
// Layout: a QUAD of lanes computes one ChaCha20 block.  Lane c = lane & 3 holds column c of the 4 x 4 state
// (a, b, c, d) = (x[c], x[4+c], x[8+c], x[12+c]), so a column round is one quarter round in every lane, and a diagonal
// round is the same quarter round after rotating the rows b, c, d by 1, 2, 3 lanes inside the quad (DPP quad_perm: no
// LDS, no memory).  The state is 4 registers per lane (+ 4 for the feed-forward), indexed with constants only: no
// scratch.  After the rounds the quad transposes its 4 x 4 words, so that lane c holds "quarter" c = words 4c .. 4c+3 —
// the two coefficients 8 blk + 2c, 8 blk + 2c + 1 — and a wave instruction stores 64 lane-consecutive 16-byte pieces,
// exactly as store_pair (rzk_sample.h) does for one Philox block per lane.
#include <hip/hip_runtime.h>

#include <string>

#include "rzk_chacha.h"
#include "rzk_dev.h"
#include "rzk_dgauss.h"

namespace rzk {

#define RZK_LAUNCH_CHECK()                      \
  do {                                          \
    hipError_t e_ = hipGetLastError();          \
    if (e_ != hipSuccess) return (int)e_;       \
  } while (0)

namespace {

struct ChaChaKey {   // the call's subkey, passed by value (kernel arguments: scalar registers)
  uint32_t w[8];
};

// value of lane quad_perm[lane & 3] of the same quad, CTRL = p0 | p1 << 2 | p2 << 4 | p3 << 6
template <int CTRL>
__device__ __forceinline__ uint32_t quad_perm(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xf, 0xf, true);
}
constexpr int kQuadFrom1 = 0x39;   // [1, 2, 3, 0]: lane c reads lane c + 1
constexpr int kQuadFrom2 = 0x4E;   // [2, 3, 0, 1]: lane c reads lane c + 2
constexpr int kQuadFrom3 = 0x93;   // [3, 0, 1, 2]: lane c reads lane c + 3

__device__ __forceinline__ uint32_t sel4(uint32_t i, uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3) {   // v[i], i in 0 .. 3
  return (i & 2u) ? ((i & 1u) ? v3 : v2) : ((i & 1u) ? v1 : v0);
}

struct Quarter {   // words 4c .. 4c+3 of a block, in lane c of its quad
  uint32_t w0, w1, w2, w3;
};

// block (w12, w13, w14, w15) under `key`, computed by the four lanes of a quad (all four must be active; c = lane & 3)
__device__ __forceinline__ Quarter chacha_quad_block(const ChaChaKey& key, uint32_t c, uint32_t w12, uint32_t w13,
                                                     uint32_t w14, uint32_t w15) {
  const uint32_t a0 = sel4(c, chacha_sigma(0), chacha_sigma(1), chacha_sigma(2), chacha_sigma(3));
  const uint32_t b0 = sel4(c, key.w[0], key.w[1], key.w[2], key.w[3]);
  const uint32_t c0 = sel4(c, key.w[4], key.w[5], key.w[6], key.w[7]);
  const uint32_t d0 = sel4(c, w12, w13, w14, w15);
  uint32_t xa = a0, xb = b0, xc = c0, xd = d0;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    chacha_quarter_round(xa, xb, xc, xd);                                                    // columns
    xb = quad_perm<kQuadFrom1>(xb), xc = quad_perm<kQuadFrom2>(xc), xd = quad_perm<kQuadFrom3>(xd);
    chacha_quarter_round(xa, xb, xc, xd);                                                    // diagonals
    xb = quad_perm<kQuadFrom3>(xb), xc = quad_perm<kQuadFrom2>(xc), xd = quad_perm<kQuadFrom1>(xd);
  }
  xa += a0, xb += b0, xc += c0, xd += d0;   // lane c: words c, 4 + c, 8 + c, 12 + c
  // transpose: lane l sends its word of row (l - s) & 3 to the lane s places below it, s = 0 .. 3, so lane c receives
  // word 4c + ((c + s) & 3) from lane (c + s) & 3; the four words are then put in order
  const uint32_t q0 = sel4(c, xa, xb, xc, xd);
  const uint32_t q1 = quad_perm<kQuadFrom1>(sel4((c - 1u) & 3u, xa, xb, xc, xd));
  const uint32_t q2 = quad_perm<kQuadFrom2>(sel4((c - 2u) & 3u, xa, xb, xc, xd));
  const uint32_t q3 = quad_perm<kQuadFrom3>(sel4((c - 3u) & 3u, xa, xb, xc, xd));
  return Quarter{sel4((0u - c) & 3u, q0, q1, q2, q3), sel4((1u - c) & 3u, q0, q1, q2, q3),
                 sel4((2u - c) & 3u, q0, q1, q2, q3), sel4((3u - c) & 3u, q0, q1, q2, q3)};
}

// two coefficients at a lane-consecutive address: one non-temporal 16-byte store (full lines per wave instruction)
// where `out` is 16-byte aligned, two 8-byte stores otherwise
__device__ __forceinline__ void store_two(int64_t* __restrict__ p, int64_t v0, int64_t v1, bool pair16) {
  if (pair16) {
    typedef int v4i __attribute__((ext_vector_type(4)));
    v4i t;
    t.x = (int32_t)v0, t.y = (int32_t)(v0 >> 32), t.z = (int32_t)v1, t.w = (int32_t)(v1 >> 32);
    __builtin_nontemporal_store(t, reinterpret_cast<v4i*>(p));
  } else {
    p[0] = v0;
    p[1] = v1;
  }
}
// ... of a 32-bit slab: one non-temporal 8-byte store (a quad writes 32 contiguous bytes, a wavefront 512).  The pair starts
// at an even coefficient of a 16-byte aligned slab (the entry points insist), so the store is aligned whatever the flag says.
__device__ __forceinline__ void store_two(int32_t* __restrict__ p, int64_t v0, int64_t v1, bool) {
  typedef int v2i __attribute__((ext_vector_type(2)));
  v2i t;
  t.x = (int32_t)v0, t.y = (int32_t)v1;
  __builtin_nontemporal_store(t, reinterpret_cast<v2i*>(p));
}

// Work of the uniform and Gaussian kernels: quad g of the call is block g & (Q - 1) of polynomial g >> log_q, Q =
// max(N / 8, 1) blocks per polynomial; lane c of the quad owns coefficients 8 blk + 2c, 8 blk + 2c + 1 (N = 4: lanes
// 0 and 1 only — the block is wider than the polynomial, N = 2: lane 0).  Thread u is lane u & 3 of quad u >> 2: the
// grid strides by multiples of 256, so whole quads enter and leave the loop together.
struct QuadTask {
  uint64_t poly;
  uint32_t blk, c;
  __device__ __forceinline__ QuadTask(uint64_t u, uint32_t log_q) : poly((u >> 2) >> log_q), blk((uint32_t)(u >> 2) & ((1u << log_q) - 1u)), c((uint32_t)u & 3u) {}
  __device__ __forceinline__ uint32_t coef() const { return 8u * blk + 2u * c; }
};

__device__ __forceinline__ void wave_sync() {   // orders a wavefront's LDS accesses (as in rzk_wave.h)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- the exact discrete Gaussian (rzk_dgauss.h) -----------------------------------------------------------
// A trial round of one coefficient pair is one block, so one quad computes it; its two trials are one lane each.  A pair g
// of the call (polynomial g >> log_h, pair g & (N / 2 - 1)) writes out[2g], out[2g + 1], so a TILE of kDgaussTile
// consecutive pairs is a contiguous piece of the output, whatever N is, and may span polynomials or be cut by the end of
// the call.
//
// A wavefront owns a tile and walks it in generations: generation t is the list of the tile's pairs that still have an
// open coefficient after t trials — every item of a generation is at the same trial number, so an item is (pair within
// the tile, 2-bit mask of open coefficients) and the queue is two lists in LDS, the one being read and the one being
// filled.  A round takes up to 32 items, two per quad: the quad computes block A, then block B, and then every lane
// runs one trial — lanes 0, 1 the coefficients 2j, 2j + 1 of A (words 0 .. 7, 8 .. 15), lanes 2, 3 those of B.  Accepted
// values go to the tile in LDS, items with a coefficient still open are appended to the next list at ballot / mbcnt
// positions.  The loops end by their counters (t < kDgaussTMax, the list length): no exit depends on the random words
// alone.  The tile leaves as lane-consecutive 16-byte pieces (store_two).
constexpr uint32_t kDgaussTile = 128;   // pairs per tile: 2 KiB of results + 512 B of lists per wavefront

// Words 8 coef .. 8 coef + 5 of the lane's item, of block A (quarters qa) in lanes 0, 1 of the quad and of block B (qb) in
// lanes 2, 3: the quarter of lane 2 coef ([0, 2, 0, 2]) and two words of lane 2 coef + 1 ([1, 3, 1, 3]).
// CALL WITH ALL 64 LANES ACTIVE: a quad permutation reads 0 from a lane that is masked off.  That is why A and B are
// both permuted in every lane before ?: chooses, and why the choice lives in here and not with the caller.
struct DgaussWords {
  uint32_t w0, w1, w2, w3, w4, w5;
};
__device__ __forceinline__ DgaussWords dgauss_lane_words(const Quarter& qa, const Quarter& qb, bool second) {
  const Quarter lo_a = {quad_perm<0x88>(qa.w0), quad_perm<0x88>(qa.w1), quad_perm<0x88>(qa.w2), quad_perm<0x88>(qa.w3)};
  const Quarter lo_b = {quad_perm<0x88>(qb.w0), quad_perm<0x88>(qb.w1), quad_perm<0x88>(qb.w2), quad_perm<0x88>(qb.w3)};
  const uint32_t hi_a0 = quad_perm<0xDD>(qa.w0), hi_a1 = quad_perm<0xDD>(qa.w1);
  const uint32_t hi_b0 = quad_perm<0xDD>(qb.w0), hi_b1 = quad_perm<0xDD>(qb.w1);
  return {second ? lo_b.w0 : lo_a.w0, second ? lo_b.w1 : lo_a.w1, second ? lo_b.w2 : lo_a.w2,
          second ? lo_b.w3 : lo_a.w3, second ? hi_b0 : hi_a0,     second ? hi_b1 : hi_a1};
}

// The four sampler kernels, once per coefficient width of `out` (see the head of rzk_csprng_kernels.inc): int64_t slabs, and
// the 32-bit slabs of DESIGN.md §18 (reported as sample_*_chacha_kernel_i32).
#define RZK_CS_KERNEL(name) name
#define RZK_CS_COEF int64_t
#include "rzk_csprng_kernels.inc"
#undef RZK_CS_KERNEL
#undef RZK_CS_COEF
#define RZK_CS_KERNEL(name) name##_i32
#define RZK_CS_COEF int32_t
#include "rzk_csprng_kernels.inc"
#undef RZK_CS_KERNEL
#undef RZK_CS_COEF

// Diagnostic (rzk_debug_dgauss_trial_dev): the trial on words the caller chose, one thread per trial
__global__ void __launch_bounds__(256)
debug_dgauss_trial_kernel(const uint32_t* __restrict__ words, int64_t* __restrict__ out, uint64_t trials, DgaussParams P) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < trials; i += (uint64_t)gridDim.x * 256) {
    const uint32_t* w = words + 8 * i;
    int64_t v;
    const bool acc = dgauss_trial(P, w[0], w[1], w[2], w[3], w[4], w[5], v);
    out[2 * i] = acc ? 1 : 0;
    out[2 * i + 1] = v;
  }
}

unsigned grid_for(uint64_t tasks, int num_cus, uint32_t per_block, uint32_t blocks_per_cu) {
  uint64_t blocks = (tasks + per_block - 1) / per_block;
  const uint64_t cap = (uint64_t)num_cus * blocks_per_cu;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  return (unsigned)blocks;
}

bool ring_ok(uint32_t n_ring) { return n_ring >= 2 && !(n_ring & (n_ring - 1)); }

uint32_t log_quads(uint32_t n_ring) {   // log2 of the blocks per polynomial, max(N / 8, 1)
  uint32_t l = 0;
  while ((8u << l) < n_ring) ++l;
  return l;
}

ChaChaKey key_of(const uint32_t subkey[8]) {
  ChaChaKey k;
  for (int i = 0; i < 8; ++i) k.w[i] = subkey[i];
  return k;
}

}  // namespace

int launch_sample_uniform_chacha(const LaunchCfg& cfg, int64_t* out, uint64_t npoly, uint32_t n_ring, const uint32_t subkey[8],
                                 uint32_t stream, uint32_t bound, uint32_t width) {
  if (npoly == 0) return 0;
  if (!ring_ok(n_ring)) return -1;
  const uint32_t lq = log_quads(n_ring);
  const uint64_t nquads = npoly << lq;
  const dim3 grid(grid_for(nquads, cfg.num_cus, 64, 16));
  if (width == 4)
    hipLaunchKernelGGL(sample_uniform_chacha_kernel_i32, grid, dim3(256), 0, (hipStream_t)cfg.stream, reinterpret_cast<int32_t*>(out),
                       nquads, n_ring, lq, key_of(subkey), stream, bound);
  else
    hipLaunchKernelGGL(sample_uniform_chacha_kernel, grid, dim3(256), 0, (hipStream_t)cfg.stream, out, nquads, n_ring, lq,
                       key_of(subkey), stream, bound);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = width == 4 ? "sample_uniform_chacha_kernel_i32" : "sample_uniform_chacha_kernel";
  return 0;
}

int launch_sample_gauss_chacha(const LaunchCfg& cfg, int64_t* out, uint64_t npoly, uint32_t n_ring, const uint32_t subkey[8],
                               uint32_t stream, double sigma, uint32_t width) {
  if (npoly == 0) return 0;
  if (!ring_ok(n_ring)) return -1;
  const uint32_t lq = log_quads(n_ring);
  const uint64_t nquads = npoly << lq;
  const dim3 grid(grid_for(nquads, cfg.num_cus, 64, 16));
  const bool f32 = sigma < 524288.0;   // as launch_sample_gauss: 9.4 sigma < 2^23
  int32_t* out32 = reinterpret_cast<int32_t*>(out);
  if (width == 4 && f32)
    hipLaunchKernelGGL(sample_gauss_chacha_kernel_i32<true>, grid, dim3(256), 0, (hipStream_t)cfg.stream, out32, nquads, n_ring, lq,
                       key_of(subkey), stream, sigma);
  else if (width == 4)
    hipLaunchKernelGGL(sample_gauss_chacha_kernel_i32<false>, grid, dim3(256), 0, (hipStream_t)cfg.stream, out32, nquads, n_ring, lq,
                       key_of(subkey), stream, sigma);
  else if (f32)
    hipLaunchKernelGGL(sample_gauss_chacha_kernel<true>, grid, dim3(256), 0, (hipStream_t)cfg.stream, out, nquads, n_ring, lq,
                       key_of(subkey), stream, sigma);
  else
    hipLaunchKernelGGL(sample_gauss_chacha_kernel<false>, grid, dim3(256), 0, (hipStream_t)cfg.stream, out, nquads, n_ring, lq,
                       key_of(subkey), stream, sigma);
  RZK_LAUNCH_CHECK();
  if (cfg.launched)
    *cfg.launched = std::string(width == 4 ? "sample_gauss_chacha_kernel_i32<" : "sample_gauss_chacha_kernel<") + (f32 ? "true>" : "false>");
  return 0;
}

int launch_sample_dgauss_chacha(const LaunchCfg& cfg, int64_t* out, uint64_t npoly, uint32_t n_ring, const uint32_t subkey[8],
                                uint32_t stream, uint32_t sigma, uint32_t width) {
  if (npoly == 0) return 0;
  if (!ring_ok(n_ring) || n_ring > (1u << 16) || sigma == 0 || sigma > kDgaussSigmaMax) return -1;   // the pair index has 16 bits of w12
  uint32_t log_h = 0;
  while ((2u << log_h) < n_ring) ++log_h;
  const uint64_t npairs = npoly << log_h;
  const uint64_t ntiles = (npairs + kDgaussTile - 1) / kDgaussTile;
  const dim3 grid(grid_for(ntiles, cfg.num_cus, 4, 8));
  if (width == 4)
    hipLaunchKernelGGL(sample_dgauss_chacha_kernel_i32, grid, dim3(256), 0, (hipStream_t)cfg.stream, reinterpret_cast<int32_t*>(out),
                       npairs, log_h, key_of(subkey), stream, dgauss_params(sigma));
  else
    hipLaunchKernelGGL(sample_dgauss_chacha_kernel, grid, dim3(256), 0, (hipStream_t)cfg.stream, out, npairs, log_h, key_of(subkey),
                       stream, dgauss_params(sigma));
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = width == 4 ? "sample_dgauss_chacha_kernel_i32" : "sample_dgauss_chacha_kernel";
  return 0;
}

int launch_debug_dgauss_trial(const LaunchCfg& cfg, uint32_t sigma, const uint32_t* words, int64_t* out, uint64_t trials) {
  if (trials == 0) return 0;
  if (sigma == 0 || sigma > kDgaussSigmaMax) return -1;
  hipLaunchKernelGGL(debug_dgauss_trial_kernel, dim3(grid_for(trials, cfg.num_cus, 256, 16)), dim3(256), 0, (hipStream_t)cfg.stream,
                     words, out, trials, dgauss_params(sigma));
  RZK_LAUNCH_CHECK();
  return 0;
}

int launch_sample_challenge_chacha(const LaunchCfg& cfg, int64_t* out, uint64_t npoly, uint32_t n_ring, const uint32_t subkey[8],
                                   uint32_t stream, uint32_t kappa, uint32_t width) {
  if (npoly == 0) return 0;
  if (n_ring < 4 || (n_ring & 3u)) return -1;   // the byte map is cleared and read in words
  const dim3 grid(grid_for(npoly, cfg.num_cus, 4, 16));
  if (width == 4)
    hipLaunchKernelGGL(sample_challenge_chacha_kernel_i32, grid, dim3(256), 4 * n_ring, (hipStream_t)cfg.stream,
                       reinterpret_cast<int32_t*>(out), npoly, n_ring, key_of(subkey), stream, kappa);
  else
    hipLaunchKernelGGL(sample_challenge_chacha_kernel, grid, dim3(256), 4 * n_ring, (hipStream_t)cfg.stream, out, npoly, n_ring,
                       key_of(subkey), stream, kappa);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = width == 4 ? "sample_challenge_chacha_kernel_i32" : "sample_challenge_chacha_kernel";
  return 0;
}

}  // namespace rzk
