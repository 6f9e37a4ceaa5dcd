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

// The four sampler kernels, templates over C = int64_t / int32_t, what `out` holds (the 32-bit slabs of DESIGN.md §18; reported
// as sample_*_chacha_kernel_i32).  The word streams, block counters and maps are the same; a value is narrowed
// where it is stored (store_two) or parked (the dgauss tile), and every value an accepted argument can produce lies inside
// int32.  `pair16` means "one vector store per coefficient pair": 16 bytes of int64_t, 8 bytes of int32_t.

// Work of the uniform and Gaussian kernels: QuadTask (above).
template <class C>
__global__ void __launch_bounds__(256)
sample_uniform_chacha_kernel(C* __restrict__ out, uint64_t nquads, uint32_t n_ring, uint32_t log_q, ChaChaKey key,
                             uint32_t stream, uint32_t bound) {
  const bool pair16 = (reinterpret_cast<uintptr_t>(out) & 15u) == 0;
  for (uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x; (u >> 2) < nquads; u += (uint64_t)gridDim.x * 256) {
    const QuadTask t(u, log_q);
    const Quarter w = chacha_quad_block(key, t.c, t.blk, (uint32_t)t.poly, (uint32_t)(t.poly >> 32), stream);
    if (t.coef() < n_ring)
      store_two(out + t.poly * n_ring + t.coef(), chacha_uniform_coef(w.w0, w.w1, bound), chacha_uniform_coef(w.w2, w.w3, bound),
                pair16);
  }
}

template <bool F32, class C>
__global__ void __launch_bounds__(256)
sample_gauss_chacha_kernel(C* __restrict__ out, uint64_t nquads, uint32_t n_ring, uint32_t log_q, ChaChaKey key,
                           uint32_t stream, double sigma) {
  const bool pair16 = (reinterpret_cast<uintptr_t>(out) & 15u) == 0;
  const float sigf = (float)sigma;
  for (uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x; (u >> 2) < nquads; u += (uint64_t)gridDim.x * 256) {
    const QuadTask t(u, log_q);
    const Quarter w = chacha_quad_block(key, t.c, t.blk, (uint32_t)t.poly, (uint32_t)(t.poly >> 32), stream);
    int64_t v0, v1;
    if (F32) gauss_pair_f32(w.w0, w.w1, w.w2, sigf, v0, v1);
    else gauss_pair_f64(w.w0, w.w1, w.w2, w.w3, sigma, v0, v1);
    if (t.coef() < n_ring) store_two(out + t.poly * n_ring + t.coef(), v0, v1, pair16);
  }
}

// One wavefront per polynomial, Floyd's kappa-subset walked over an LDS byte map: sample_challenge_kernel (rzk_sample.h)
// with the candidates of 64 steps drawn from 8 ChaCha20 blocks.  Lane t & 63 needs words 2s, 2s + 1 (s = t & 7) of
// block t >> 3: the two quads of lanes 8m .. 8m + 7 both compute block (t0 >> 3) + m, and lane s takes its pair from
// quarter s >> 1, which lane s >> 1 of its own quad holds.
template <class C>
__global__ void __launch_bounds__(256)
sample_challenge_chacha_kernel(C* __restrict__ out, uint64_t npoly, uint32_t n_ring, ChaChaKey key, uint32_t stream,
                               uint32_t kappa) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int8_t* mark = reinterpret_cast<int8_t*>(smem) + (size_t)wave * n_ring;
  uint32_t* mark_w = reinterpret_cast<uint32_t*>(mark);   // n_ring is a multiple of 4
  const uint32_t kap = kappa < n_ring ? kappa : n_ring;
  const bool pair16 = (reinterpret_cast<uintptr_t>(out) & 15u) == 0;
  for (uint64_t poly = (uint64_t)blockIdx.x * 4 + wave; poly < npoly; poly += (uint64_t)gridDim.x * 4) {
    for (uint32_t i = lane; i < n_ring / 4; i += 64) mark_w[i] = 0;
    wave_sync();
    for (uint32_t t0 = 0; t0 < kap; t0 += 64) {
      const uint32_t t = t0 + lane;
      const Quarter q = chacha_quad_block(key, lane & 3u, t >> 3, (uint32_t)poly, (uint32_t)(poly >> 32), stream);
      // quarter (t & 7) >> 1: from lane [0, 0, 1, 1] of the quad in the lower half of an 8-lane group, [2, 2, 3, 3] in the upper
      const bool up = (lane & 4u) != 0;
      const uint32_t x0 = up ? quad_perm<0xFA>(q.w0) : quad_perm<0x50>(q.w0);
      const uint32_t x1 = up ? quad_perm<0xFA>(q.w1) : quad_perm<0x50>(q.w1);
      const uint32_t x2 = up ? quad_perm<0xFA>(q.w2) : quad_perm<0x50>(q.w2);
      const uint32_t x3 = up ? quad_perm<0xFA>(q.w3) : quad_perm<0x50>(q.w3);
      const uint32_t w0 = (lane & 1u) ? x2 : x0, w1 = (lane & 1u) ? x3 : x1;
      const uint32_t j = n_ring - kap + t;                               // (lanes beyond kap: unused)
      uint32_t pick;
      int32_t sign;
      chacha_challenge_step(w0, w1, j, pick, sign);
      const uint32_t m = kap - t0 < 64u ? kap - t0 : 64u;
#pragma unroll 1
      for (uint32_t e = 0; e < m; ++e) {
        const uint32_t pk = (uint32_t)__builtin_amdgcn_readlane((int)pick, (int)e);
        const uint32_t jj = (uint32_t)__builtin_amdgcn_readlane((int)j, (int)e);
        const int32_t sg = __builtin_amdgcn_readlane(sign, (int)e);
        const uint32_t pos = mark[pk] ? jj : pk;
        wave_sync();
        if (lane == 0) mark[pos] = (int8_t)sg;
        wave_sync();
      }
    }
    C* dst = out + poly * n_ring;
    if (pair16) {
      for (uint32_t i = 2 * lane; i < n_ring; i += 128) {
        const int32_t a0 = mark[i], a1 = mark[i + 1];
        store_two(dst + i, (int64_t)a0, (int64_t)a1, true);
      }
    } else {
      for (uint32_t i = lane; i < n_ring; i += 64) dst[i] = (C)mark[i];
    }
    wave_sync();
  }
}

// The exact discrete Gaussian: the tile walk described above.  The tile in LDS holds C (2 KiB or 1 KiB of results per
// wavefront).
template <class C>
__global__ void __launch_bounds__(256)
sample_dgauss_chacha_kernel(C* __restrict__ out, uint64_t npairs, uint32_t log_h, ChaChaKey key, uint32_t stream,
                            DgaussParams P) {
  __shared__ __attribute__((aligned(16))) C s_tile[4][2 * kDgaussTile];
  __shared__ uint16_t s_list[4][2][kDgaussTile];
  const uint32_t lane = threadIdx.x & 63u, c = lane & 3u, quad = lane >> 2, coef = c & 1u;
  const bool second = (c & 2u) != 0;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  C* tile = s_tile[wave];
  const bool pair16 = (reinterpret_cast<uintptr_t>(out) & 15u) == 0;
  const uint64_t ntiles = (npairs + kDgaussTile - 1) / kDgaussTile;
  for (uint64_t tl = (uint64_t)blockIdx.x * 4 + wave; tl < ntiles; tl += (uint64_t)gridDim.x * 4) {
    const uint64_t base = tl * kDgaussTile;
    const uint32_t cnt0 = npairs - base < kDgaussTile ? (uint32_t)(npairs - base) : kDgaussTile;
    for (uint32_t i = lane; i < kDgaussTile; i += 64) {
      tile[2 * i] = 0, tile[2 * i + 1] = 0;                     // a coefficient that runs out of trials is 0
      s_list[wave][0][i] = (uint16_t)(i | (3u << 8));
    }
    wave_sync();
    uint32_t cnt = cnt0, cur = 0;
    for (uint32_t t = 0; t < kDgaussTMax && cnt != 0; ++t) {
      const uint16_t* list = s_list[wave][cur];
      uint16_t* next = s_list[wave][cur ^ 1u];
      uint32_t ncnt = 0;
      const auto block_of = [&](uint32_t item) {                 // the block of trial t of the item's pair
        const uint64_t g = base + (item & 0xffu);
        const uint64_t poly = g >> log_h;
        const uint32_t j = (uint32_t)g & ((1u << log_h) - 1u);
        return chacha_quad_block(key, c, dgauss_w12(t, j), (uint32_t)poly, (uint32_t)(poly >> 32), stream);
      };
      for (uint32_t b0 = 0; b0 < cnt; b0 += 32) {
        const uint32_t idx_a = b0 + quad, idx_b = idx_a + 16;
        uint32_t item_a = 0, item_b = 0;                         // mask 0: nothing open
        Quarter qa = {0, 0, 0, 0}, qb = {0, 0, 0, 0};
        if (idx_a < cnt) item_a = list[idx_a], qa = block_of(item_a);   // whole quads
        if (idx_b < cnt) item_b = list[idx_b], qb = block_of(item_b);
        // reconverged: the two fetches above diverge on whole quads only, and every lane of the wavefront is in this loop
        // (b0 and cnt are uniform), so all 64 lanes are active here, as dgauss_lane_words and the permutations of `still`
        // below need
        const uint32_t item = second ? item_b : item_a, pi = item & 0xffu;   // pi < kDgaussTile
        const DgaussWords w = dgauss_lane_words(qa, qb, second);
        int64_t v;
        const bool acc = dgauss_trial(P, w.w0, w.w1, w.w2, w.w3, w.w4, w.w5, v);
        const bool open = ((item >> (8u + coef)) & 1u) != 0;
        if (open && acc) tile[2 * pi + coef] = (C)v;
        const uint32_t still = open && !acc ? 1u : 0u;
        const uint32_t mask_a = quad_perm<0x00>(still) | (quad_perm<0x55>(still) << 1);   // from lanes 0 and 1
        const uint32_t mask_b = quad_perm<0xAA>(still) | (quad_perm<0xFF>(still) << 1);   // from lanes 2 and 3
        const uint32_t mask = second ? mask_b : mask_a;
        const bool push = coef == 0 && mask != 0;                // lane 0 for A, lane 2 for B
        const uint64_t bal = __ballot(push);
        const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
        if (push) next[ncnt + before] = (uint16_t)(pi | (mask << 8));
        ncnt += (uint32_t)__popcll(bal);                         // <= the items read: the list cannot overflow
      }
      wave_sync();
      cnt = __builtin_amdgcn_readfirstlane(ncnt), cur ^= 1u;
    }
    wave_sync();
    for (uint32_t i = lane; i < cnt0; i += 64) store_two(out + 2 * (base + i), tile[2 * i], tile[2 * i + 1], pair16);
    wave_sync();
  }
}

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

template <class C>
const char* i32_mark() {   // the reported names of the 32-bit kernels end in _i32
  return sizeof(C) == 4 ? "_i32" : "";
}

}  // namespace

template <class C>
int launch_sample_uniform_chacha(const LaunchCfg& cfg, C* out, uint64_t npoly, uint32_t n_ring, const uint32_t subkey[8],
                                 uint32_t stream, uint32_t bound) {
  if (npoly == 0) return 0;
  if (!ring_ok(n_ring)) return -1;
  const uint32_t lq = log_quads(n_ring);
  const uint64_t nquads = npoly << lq;
  const dim3 grid(grid_for(nquads, cfg.num_cus, 64, 16));
  hipLaunchKernelGGL(sample_uniform_chacha_kernel<C>, grid, dim3(256), 0, (hipStream_t)cfg.stream, out, nquads, n_ring, lq,
                     key_of(subkey), stream, bound);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = std::string("sample_uniform_chacha_kernel") + i32_mark<C>();
  return 0;
}
RZK_BOTH_WIDTHS(launch_sample_uniform_chacha)

template <class C>
int launch_sample_gauss_chacha(const LaunchCfg& cfg, C* out, uint64_t npoly, uint32_t n_ring, const uint32_t subkey[8],
                               uint32_t stream, double sigma) {
  if (npoly == 0) return 0;
  if (!ring_ok(n_ring)) return -1;
  const uint32_t lq = log_quads(n_ring);
  const uint64_t nquads = npoly << lq;
  const dim3 grid(grid_for(nquads, cfg.num_cus, 64, 16));
  const bool f32 = sigma < 524288.0;   // as launch_sample_gauss: 9.4 sigma < 2^23
  if (f32)
    hipLaunchKernelGGL((sample_gauss_chacha_kernel<true, C>), grid, dim3(256), 0, (hipStream_t)cfg.stream, out, nquads, n_ring, lq,
                       key_of(subkey), stream, sigma);
  else
    hipLaunchKernelGGL((sample_gauss_chacha_kernel<false, C>), grid, dim3(256), 0, (hipStream_t)cfg.stream, out, nquads, n_ring, lq,
                       key_of(subkey), stream, sigma);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = std::string("sample_gauss_chacha_kernel") + i32_mark<C>() + (f32 ? "<true>" : "<false>");
  return 0;
}
RZK_BOTH_WIDTHS(launch_sample_gauss_chacha)

template <class C>
int launch_sample_dgauss_chacha(const LaunchCfg& cfg, C* out, uint64_t npoly, uint32_t n_ring, const uint32_t subkey[8],
                                uint32_t stream, uint32_t sigma) {
  if (npoly == 0) return 0;
  if (!ring_ok(n_ring) || n_ring > (1u << 16) || sigma == 0 || sigma > kDgaussSigmaMax) return -1;   // the pair index has 16 bits of w12
  uint32_t log_h = 0;
  while ((2u << log_h) < n_ring) ++log_h;
  const uint64_t npairs = npoly << log_h;
  const uint64_t ntiles = (npairs + kDgaussTile - 1) / kDgaussTile;
  const dim3 grid(grid_for(ntiles, cfg.num_cus, 4, 8));
  hipLaunchKernelGGL(sample_dgauss_chacha_kernel<C>, grid, dim3(256), 0, (hipStream_t)cfg.stream, out, npairs, log_h, key_of(subkey),
                     stream, dgauss_params(sigma));
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = std::string("sample_dgauss_chacha_kernel") + i32_mark<C>();
  return 0;
}
RZK_BOTH_WIDTHS(launch_sample_dgauss_chacha)

int launch_debug_dgauss_trial(const LaunchCfg& cfg, uint32_t sigma, const uint32_t* words, int64_t* out, uint64_t trials) {
  if (trials == 0) return 0;
  if (sigma == 0 || sigma > kDgaussSigmaMax) return -1;
  hipLaunchKernelGGL(debug_dgauss_trial_kernel, dim3(grid_for(trials, cfg.num_cus, 256, 16)), dim3(256), 0, (hipStream_t)cfg.stream,
                     words, out, trials, dgauss_params(sigma));
  RZK_LAUNCH_CHECK();
  return 0;
}

template <class C>
int launch_sample_challenge_chacha(const LaunchCfg& cfg, C* out, uint64_t npoly, uint32_t n_ring, const uint32_t subkey[8],
                                   uint32_t stream, uint32_t kappa) {
  if (npoly == 0) return 0;
  if (n_ring < 4 || (n_ring & 3u)) return -1;   // the byte map is cleared and read in words
  const dim3 grid(grid_for(npoly, cfg.num_cus, 4, 16));
  hipLaunchKernelGGL(sample_challenge_chacha_kernel<C>, grid, dim3(256), 4 * n_ring, (hipStream_t)cfg.stream, out, npoly, n_ring,
                     key_of(subkey), stream, kappa);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = std::string("sample_challenge_chacha_kernel") + i32_mark<C>();
  return 0;
}
RZK_BOTH_WIDTHS(launch_sample_challenge_chacha)

}  // namespace rzk
