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
// Both kernels exist for int64_t slabs (fs_leaf_kernel, fs_root_kernel) and for 32-bit slabs (reported as
// fs_leaf_kernel<i32>, fs_root_kernel<i32>) from one text (rzk_fs_kernels.inc); the staging, the tile and the
// grids are the same.
#include <hip/hip_runtime.h>

#include "rzk_dev.h"
#include "rzk_keccak.h"

namespace rzk {

#define RZK_LAUNCH_CHECK()                      \
  do {                                          \
    hipError_t e_ = hipGetLastError();          \
    if (e_ != hipSuccess) return (int)e_;       \
  } while (0)

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

// The kernels' text, once per coefficient width (see the head of rzk_fs_kernels.inc).
#define RZK_FS_KERNEL(name) name
#define RZK_FS_COEF int64_t
#define RZK_FS_OUT_OF_RANGE(v, h) ((v) > (h) || (v) < -(h))
#include "rzk_fs_kernels.inc"
#undef RZK_FS_KERNEL
#undef RZK_FS_COEF
#undef RZK_FS_OUT_OF_RANGE
#define RZK_FS_KERNEL(name) name##_i32
#define RZK_FS_COEF int32_t
#define RZK_FS_OUT_OF_RANGE(v, h) ((uint32_t)(v) + (uint32_t)(h) > 2u * (uint32_t)(h))
#include "rzk_fs_kernels.inc"
#undef RZK_FS_KERNEL
#undef RZK_FS_COEF
#undef RZK_FS_OUT_OF_RANGE

}  // namespace

int launch_fs_leaves(const LaunchCfg& cfg, const FsMsg& m, int64_t half, int check, uint64_t* dig, uint8_t* ok,
                     uint32_t* bad_word, uint64_t B, uint32_t width) {
  const uint64_t nleaves = B * m.polys * (m.N / fs_leaf_len(m.N));
  if (nleaves == 0) return 0;
  uint64_t blocks = (nleaves + 63) / 64;
  const uint64_t cap = (uint64_t)cfg.num_cus * 16;
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(width == 4 ? fs_leaf_kernel_i32 : fs_leaf_kernel, dim3((unsigned)blocks), dim3(64), 0,
                     (hipStream_t)cfg.stream, m, half, check, dig, ok, bad_word, B, nleaves);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = width == 4 ? "fs_leaf_kernel<i32>" : "fs_leaf_kernel";
  return 0;
}

int launch_fs_roots(const LaunchCfg& cfg, const FsRoot& r, const uint64_t* dig, int64_t* d, uint8_t* digest,
                    uint64_t B, uint32_t width) {
  if (B == 0) return 0;
  uint64_t blocks = (B + 63) / 64;
  const uint64_t cap = (uint64_t)cfg.num_cus * 4;
  if (blocks > cap) blocks = cap;
  if (width == 4)
    hipLaunchKernelGGL(fs_root_kernel_i32, dim3((unsigned)blocks), dim3(64), 0, (hipStream_t)cfg.stream, r, dig,
                       reinterpret_cast<int32_t*>(d), digest, B);
  else
    hipLaunchKernelGGL(fs_root_kernel, dim3((unsigned)blocks), dim3(64), 0, (hipStream_t)cfg.stream, r, dig, d, digest, B);
  RZK_LAUNCH_CHECK();
  if (cfg.launched) *cfg.launched = width == 4 ? "fs_root_kernel<i32>" : "fs_root_kernel";
  return 0;
}

}  // namespace rzk
