// rzk_fs_kernels.inc — the text of fs_leaf_kernel and fs_root_kernel, included by rzk_fs_dev.hip once per coefficient width
// (inside namespace rzk, behind the file's helpers); as text and not as a template over a shared body for the reason given
// at the head of rzk_packed_kernels.inc: the 64-bit kernels stay token for token what they were.  The including file defines
//   RZK_FS_KERNEL(name)          the kernel's symbol (name, name_i32)
//   RZK_FS_COEF                  int64_t / int32_t: what the slabs of FsMsg and the challenge slab d hold (FsMsg carries
//                                addresses).  A slab32 is the hash's input format: a row's 34 coefficients are 136 contiguous
//                                bytes instead of 272, and the tile store is the word itself
//   RZK_FS_OUT_OF_RANGE(v, h)    the range test |v| > h: two signed compares on an int64_t; on an int32_t the single unsigned
//                                compare of the slab32 kernels, (uint32_t)(v + h) > 2h (h < 2^31: v > h gives at most
//                                2^31 - 1 + h < 2^32, v < -h wraps to at least 2^31 + h > 2h)
__global__ void __launch_bounds__(64) RZK_FS_KERNEL(fs_leaf_kernel)(FsMsg m, int64_t half, int check, uint64_t* __restrict__ dig,
                                                     uint8_t* ok, uint32_t* bad_word, uint64_t B, uint64_t nleaves) {
  __shared__ uint32_t tile[64 * kTileStride];
  __shared__ const RZK_FS_COEF* base[64];   // first coefficient of every lane's leaf (NULL past the end)
  const uint32_t lane = threadIdx.x;
  const uint32_t leaf = fs_leaf_len(m.N), chunks = m.N / leaf;
  const uint32_t W = fs_leaf_words(m.N);
  for (uint64_t t0 = (uint64_t)blockIdx.x * 64; t0 < nleaves; t0 += (uint64_t)gridDim.x * 64) {
    const uint64_t t = t0 + lane;
    const bool live = t < nleaves;
    const uint64_t j = live ? t / B : 0, b = live ? t - j * B : 0;
    const uint32_t p = (uint32_t)(j / chunks), ch = (uint32_t)(j - (uint64_t)p * chunks);
    const RZK_FS_COEF* src = nullptr;
    if (live) {
      uint32_t f = 0;
      while (f + 1 < m.nfields && p >= m.first[f + 1]) ++f;
      const uint64_t rows = m.first[f + 1] - m.first[f];
      src = reinterpret_cast<const RZK_FS_COEF*>(m.ptr[f]) + (b * rows + (p - m.first[f])) * (uint64_t)m.N + (uint64_t)ch * leaf;
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
        const RZK_FS_COEF* bp = base[row];
        if (bp && coef >= 0 && coef < (int)leaf) {
          const RZK_FS_COEF v = bp[coef];
          if (check && RZK_FS_OUT_OF_RANGE(v, half)) {   // every writer stores the same value
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

__global__ void __launch_bounds__(64) RZK_FS_KERNEL(fs_root_kernel)(FsRoot r, const uint64_t* __restrict__ dig, RZK_FS_COEF* d,
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
