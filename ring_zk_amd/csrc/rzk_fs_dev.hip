// rzk_fs_dev.hip — batched SHAKE256 transcript hash of the non-interactive (Fiat-Shamir) proofs; the "FS1" format and
// the sponge are in rzk_keccak.h.  Two launches per call:
//   fs_leaf_kernel   one lane per leaf (min(N, 256) coefficients of one polynomial), Keccak state in registers.  A
//                    lane's leaf is up to 2 KiB of contiguous int64, so lane-private loads would touch 64 cache lines
//                    per instruction: the wavefront loads one rate block (34 coefficients) of each of its 64 leaves
//                    together, along the leaves, range-tests the coefficients on the way (a violation clears ok[b],
//                    or raises the sticky bad-input word where the caller passed no ok), and parks their low halves
//                    in an LDS tile of 64 rows with an odd row stride, from which every lane reads its own row.
//   fs_root_kernel   one lane per proof: absorbs the header and the proof's leaf digests, writes the transcript digest,
//                    squeezes and samples the challenge into d (zeroed beforehand by the caller).
// Leaf j of proof b is hashed by lane j * B + b and its digest word w is stored at dig[(j * 4 + w) * B + b]: the lanes
// of a wavefront write, and the root lanes read, consecutive addresses.
// Both kernels are templates over the coefficient type of the slabs: int64_t (reported as fs_leaf_kernel, fs_root_kernel)
// and the 32-bit slabs (reported as fs_leaf_kernel<i32>, fs_root_kernel<i32>); the staging, the tile and
// the grids are the same.
#include <hip/hip_runtime.h>

#include "rzk_dev.h"
#include "rzk_keccak.h"

namespace rzk {

namespace {

constexpr uint32_t kBlockCoefs = 2 * kShakeRateWords;   // coefficients of one rate block
constexpr uint32_t kTileStride = kBlockCoefs + 1;       // odd: the 64 rows start on distinct banks

struct LeafTileWords {   // word i of the lane's leaf, rate block blk staged in the tile
  const uint32_t* row;
  uint32_t blk;
  uint64_t id;           // le32(p) | le32(c)
  __device__ uint64_t operator()(uint32_t i) const {
    if (i == 0) return kFsTagLeaf;
    if (i == 1) return id;
    const uint32_t col = 2 * (i - kShakeRateWords * blk);   // coefficient 2 (i - 2) sits at column 2 (i - 2) - (34 blk - 4)
    return (uint64_t)row[col] | ((uint64_t)row[col + 1] << 32);
  }
};

// The range test |v| > h of a coefficient as it is loaded: two signed compares on an int64_t; on an int32_t the single
// unsigned compare of the slab32 kernels, (uint32_t)(v + h) > 2h (h < 2^31: v > h gives at most 2^31 - 1 + h < 2^32,
// v < -h wraps to at least 2^31 + h > 2h)
__device__ __forceinline__ bool out_of_range(int64_t v, int64_t h) { return ((v) > (h) || (v) < -(h)); }
__device__ __forceinline__ bool out_of_range(int32_t v, int64_t h) { return ((uint32_t)(v) + (uint32_t)(h) > 2u * (uint32_t)(h)); }

// C = int64_t / int32_t: what the slabs of FsMsg and the challenge slab d hold (FsMsg carries addresses).  A slab32 is the
// hash's input format: a row's 34 coefficients are 136 contiguous bytes instead of 272, and the tile store is the word itself.
template <class C>
__global__ void __launch_bounds__(64) fs_leaf_kernel(FsMsg m, int64_t half, int check, uint64_t* __restrict__ dig,
                                                     uint8_t* ok, uint32_t* bad_word, uint64_t B, uint64_t nleaves) {
  __shared__ uint32_t tile[64 * kTileStride];
  __shared__ const C* base[64];   // first coefficient of every lane's leaf (NULL past the end)
  const uint32_t lane = threadIdx.x;
  const uint32_t leaf = fs_leaf_len(m.N), chunks = m.N / leaf;
  const uint32_t W = fs_leaf_words(m.N);
  for (uint64_t t0 = (uint64_t)blockIdx.x * 64; t0 < nleaves; t0 += (uint64_t)gridDim.x * 64) {
    const uint64_t t = t0 + lane;
    const bool live = t < nleaves;
    const uint64_t j = live ? t / B : 0, b = live ? t - j * B : 0;
    const uint32_t p = (uint32_t)(j / chunks), ch = (uint32_t)(j - (uint64_t)p * chunks);
    const C* src = nullptr;
    if (live) {
      uint32_t f = 0;
      while (f + 1 < m.nfields && p >= m.first[f + 1]) ++f;
      const uint64_t rows = m.first[f + 1] - m.first[f];
      src = reinterpret_cast<const C*>(m.ptr[f]) + (b * rows + (p - m.first[f])) * (uint64_t)m.N + (uint64_t)ch * leaf;
    }
    base[lane] = src;   // (the previous trip's last read of base[] lies before its last barrier)
    uint64_t s[25];
#pragma unroll
    for (int i = 0; i < 25; ++i) s[i] = 0;
    for (uint32_t blk = 0; blk <= W / kShakeRateWords; ++blk) {
      __syncthreads();   // base[] written; the previous block's tile consumed
      const int first = (int)(blk * kBlockCoefs) - 4;   // coefficient at tile column 0 (two header words lead the leaf)
      for (uint32_t it = 0; it < kBlockCoefs; ++it) {
        const uint32_t e = it * 64 + lane, row = e / kBlockCoefs, col = e - row * kBlockCoefs;
        const int coef = first + (int)col;
        const C* bp = base[row];
        if (bp && coef >= 0 && coef < (int)leaf) {
          const C v = bp[coef];
          if (check && out_of_range(v, half)) {   // every writer stores the same value
            if (ok) ok[(t0 + row) % B] = 0;
            else if (bad_word) *bad_word = 1u;
          }
          tile[row * kTileStride + col] = (uint32_t)v;
        }
      }
      __syncthreads();
      LeafTileWords word{tile + lane * kTileStride, blk, (uint64_t)p | ((uint64_t)ch << 32)};
      shake256_absorb_block(s, word, blk, W, 0x1Full);
    }
    if (live) {
#pragma unroll
      for (uint32_t w = 0; w < kFsDigestWords; ++w) dig[(j * kFsDigestWords + w) * B + b] = s[w];
    }
  }
}

template <class C>
__global__ void __launch_bounds__(64) fs_root_kernel(FsRoot r, const uint64_t* __restrict__ dig, C* d,
                                                     uint8_t* digest, uint64_t B) {
  const uint32_t W = r.nhdr + kFsDigestWords * r.leaves;
  for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < B; b += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t s[25];
    FsRootWords word{r.hdr, r.nhdr, dig, B, b};
    shake256_absorb(s, word, W, 0, 0);
    if (digest) {
      uint8_t* out = digest + b * 32;
      if (((uintptr_t)digest & 7u) == 0) {
#pragma unroll
        for (uint32_t w = 0; w < kFsDigestWords; ++w) ((uint64_t*)out)[w] = s[w];
      } else {
#pragma unroll
        for (uint32_t w = 0; w < kFsDigestWords; ++w)
          for (int i = 0; i < 8; ++i) out[8 * w + i] = (uint8_t)(s[w] >> (8 * i));
      }
    }
    if (d) fs_sample_challenge(s, d + b * (uint64_t)r.N, r.N, r.kappa);
  }
}

}  // namespace

template <class C>
int launch_fs_leaves(const LaunchCfg& cfg, const FsMsg& m, int64_t half, int check, uint64_t* dig, uint8_t* ok,
                     uint32_t* bad_word, uint64_t B) {
  const uint64_t nleaves = B * m.polys * (m.N / fs_leaf_len(m.N));
  if (nleaves == 0) return 0;
  uint64_t blocks = (nleaves + 63) / 64;
  const uint64_t cap = (uint64_t)cfg.num_cus * 16;
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(fs_leaf_kernel<C>, dim3((unsigned)blocks), dim3(64), 0, (hipStream_t)cfg.stream, m, half, check, dig, ok, bad_word,
                     B, nleaves);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = sizeof(C) == 4 ? "fs_leaf_kernel<i32>" : "fs_leaf_kernel";
  return 0;
}
RZK_BOTH_WIDTHS(launch_fs_leaves)

template <class C>
int launch_fs_roots(const LaunchCfg& cfg, const FsRoot& r, const uint64_t* dig, C* d, uint8_t* digest, uint64_t B) {
  if (B == 0) return 0;
  uint64_t blocks = (B + 63) / 64;
  const uint64_t cap = (uint64_t)cfg.num_cus * 4;
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(fs_root_kernel<C>, dim3((unsigned)blocks), dim3(64), 0, (hipStream_t)cfg.stream, r, dig, d, digest, B);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = sizeof(C) == 4 ? "fs_root_kernel<i32>" : "fs_root_kernel";
  return 0;
}
RZK_BOTH_WIDTHS(launch_fs_roots)

}  // namespace rzk
