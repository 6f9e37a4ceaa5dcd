// rzk_csprng_kernels.inc — the text of the four keyed sampler kernels, included by rzk_csprng_dev.hip once per coefficient
// width (inside namespace rzk, behind the file's helpers); as text and not as a template over a shared body for the reason
// given at the head of rzk_packed_kernels.inc: the 64-bit kernels stay token for token what they were (DESIGN.md §20).  The
// including file defines
//   RZK_CS_KERNEL(name)   the kernel's symbol (name, name_i32)
//   RZK_CS_COEF           int64_t / int32_t: what `out` holds.  The word streams, block counters and maps are the same; a
//                         value is narrowed where it is stored (store_two) or parked (the dgauss tile), and every value an
//                         accepted argument can produce lies inside int32 (DESIGN.md §20).  `pair16` means "one vector
//                         store per coefficient pair": 16 bytes of int64_t, 8 bytes of int32_t.

// Work of the uniform and Gaussian kernels: QuadTask (rzk_csprng_dev.hip).
__global__ void __launch_bounds__(256)
RZK_CS_KERNEL(sample_uniform_chacha_kernel)(RZK_CS_COEF* __restrict__ out, uint64_t nquads, uint32_t n_ring, uint32_t log_q, ChaChaKey key,
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

template <bool F32>
__global__ void __launch_bounds__(256)
RZK_CS_KERNEL(sample_gauss_chacha_kernel)(RZK_CS_COEF* __restrict__ out, uint64_t nquads, uint32_t n_ring, uint32_t log_q, ChaChaKey key,
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
__global__ void __launch_bounds__(256)
RZK_CS_KERNEL(sample_challenge_chacha_kernel)(RZK_CS_COEF* __restrict__ out, uint64_t npoly, uint32_t n_ring, ChaChaKey key, uint32_t stream,
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
    RZK_CS_COEF* dst = out + poly * n_ring;
    if (pair16) {
      for (uint32_t i = 2 * lane; i < n_ring; i += 128) {
        const int32_t a0 = mark[i], a1 = mark[i + 1];
        store_two(dst + i, (int64_t)a0, (int64_t)a1, true);
      }
    } else {
      for (uint32_t i = lane; i < n_ring; i += 64) dst[i] = (RZK_CS_COEF)mark[i];
    }
    wave_sync();
  }
}

// The exact discrete Gaussian: the tile walk described in rzk_csprng_dev.hip.  The tile in LDS holds RZK_CS_COEF (2 KiB or
// 1 KiB of results per wavefront).
__global__ void __launch_bounds__(256)
RZK_CS_KERNEL(sample_dgauss_chacha_kernel)(RZK_CS_COEF* __restrict__ out, uint64_t npairs, uint32_t log_h, ChaChaKey key, uint32_t stream,
                            DgaussParams P) {
  __shared__ __attribute__((aligned(16))) RZK_CS_COEF s_tile[4][2 * kDgaussTile];
  __shared__ uint16_t s_list[4][2][kDgaussTile];
  const uint32_t lane = threadIdx.x & 63u, c = lane & 3u, quad = lane >> 2, coef = c & 1u;
  const bool second = (c & 2u) != 0;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  RZK_CS_COEF* tile = s_tile[wave];
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
        if (open && acc) tile[2 * pi + coef] = (RZK_CS_COEF)v;
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
