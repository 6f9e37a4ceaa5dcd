// rzk_prove_loop.h — the arithmetic of the in-library prover loops (include/rzk.h "prover loop") that
// can be wrong, shared by the kernels (rzk_prove_loop_dev.hip), the host loops (rzk_prove_loop.cpp) and the CPU tests
// (tests/test_prove_loop_host.py, tests/test_prove_loop_fields_host.py, g++).  Plain C++.
//
//   nonces      nonce i of a call is nonce0 + i as a 128-bit little-endian integer (backend.KeyedSampler._next_nonce); a
//               call that may use `span` nonces is refused when nonce0 + span leaves 128 bits.
//   flags       which proofs are worth another y after round 0 (prove_live), with the commit flag a proof must show.
//   field lists the slabs the Linear and Sum loops move per round, with per-field entry sizes: the quad count of an entry and
//               its range guard (field_quads), the 64-bit entry offset (field_offset), and the three moves as host loops.
//   coins       coin = (a + half) R0 + (b + half), a = coefficient 0 of one uniform(half) polynomial, b = coefficient 1 of
//               another, R0 = 2^31 - 1, half = 2^30 - 1: uniform in [0, R0^2) (fiat_shamir.draw_coins).
//   compaction  idx[0 .. count) = the ascending b with live[b] && !done[b]: the order torch.nonzero gives, which the
//               sampler's polynomial index of a retry depends on.  One workgroup of kCompactWaves wavefronts walks the flags
//               in tiles of one flag per lane; a lane's slot is
//                   base (pending flags of earlier tiles) + wave_base (of earlier wavefronts of the tile) + rank (of
//                   earlier lanes of the wavefront: the popcount of the ballot below the lane)
//               compact_emulate runs exactly that with loops in place of lanes, through the same three functions.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RZK_PL_HD __host__ __device__ inline
#else
#define RZK_PL_HD inline
#endif

namespace rzk {

// ---- nonces --------------------------------------------------------------------------------------------------------------
// out = nonce0 + inc (128-bit little-endian); false when the sum leaves 128 bits (out then holds the wrapped value)
inline bool nonce_add(const uint8_t nonce0[16], uint64_t inc, uint8_t out[16]) {
  uint64_t carry = inc;
  for (int i = 0; i < 16; ++i) {
    const uint64_t s = (uint64_t)nonce0[i] + (carry & 0xffu);
    out[i] = (uint8_t)s;
    carry = (carry >> 8) + (s >> 8);
  }
  return carry == 0;
}
// nonces a call with this round limit may consume: r, then (y, coin draw a, coin draw b) per round
inline uint64_t prove_nonce_span(uint32_t max_rounds) { return 1ull + 3ull * max_rounds; }

// ... of the Linear and Sum loops: r, r' (rs, r'), then (y, y', coin draw a, coin draw b) per round
inline uint64_t prove_nonce_span_lin_sum(uint32_t max_rounds) { return 2ull + 4ull * max_rounds; }

// ---- flags ---------------------------------------------------------------------------------------------------------------
// Is a proof worth another y after round 0?  Its commit flag must have every bit of `wanted` (1: the one-bit verdicts of the
// Open and Sum commit calls; 3: both bits of rzk_linear_commit_batch, r and r') and its transcript hash must be ok.
RZK_PL_HD uint8_t prove_live(uint8_t ok_commit, uint8_t wanted, uint8_t ok_hash) {
  return ((ok_commit & wanted) == wanted && ok_hash != 0) ? 1 : 0;
}

// ---- field lists ---------------------------------------------------------------------------------------------------------
// The Linear and Sum loops move up to six slabs per direction and round, each with its own entry size, in ONE launch: the
// kernels take the list by value.  An entry of field f is quads[f] 16-byte quads; entry e starts field_offset(e, quads[f])
// quads into the slab.  fields_*_emulate are the kernels with loops in place of workgroups and lanes, through the same
// functions (tests/prove_loop/fields_driver.cpp).
constexpr uint32_t kMaxFields = 6;
struct FieldList {
  const void* src[kMaxFields];   // gather: the caller's slab; scatter: the sub-batch's; zero: unused
  void* dst[kMaxFields];         // gather: the sub-batch's slab; scatter, zero: the caller's
  uint32_t quads[kMaxFields];
  uint32_t n;
};
// quads per entry of a field of `rows` polynomials (V k for zs) of N coefficients of coef_bytes bytes each; false when the
// count leaves uint32 or B entries of it leave what a 64-bit byte offset holds (rows N coef_bytes is a multiple of 16 for
// N >= 4 at either width, N >= 2 at 8 bytes)
inline bool field_quads(uint64_t rows, uint32_t N, uint32_t coef_bytes, uint64_t B, uint32_t* quads) {
  const unsigned __int128 bytes = (unsigned __int128)rows * N * coef_bytes;
  const unsigned __int128 q = bytes / 16;
  if (bytes % 16 != 0 || q == 0 || q > 0xffffffffull) return false;
  if ((unsigned __int128)B * q > (unsigned __int128)0x7fffffffffffffffull / 16) return false;
  *quads = (uint32_t)q;
  return true;
}
RZK_PL_HD uint64_t field_offset(uint64_t entry, uint32_t quads) { return entry * (uint64_t)quads; }

struct FieldQuad { uint64_t w[2]; };   // 16 bytes, as the kernels' int4
inline void fields_gather_emulate(const FieldList& fl, const uint32_t* idx, uint32_t count) {
  for (uint32_t i = 0; i < count; ++i)
    for (uint32_t f = 0; f < fl.n; ++f) {
      const FieldQuad* src = (const FieldQuad*)fl.src[f] + field_offset(idx[i], fl.quads[f]);
      FieldQuad* dst = (FieldQuad*)fl.dst[f] + field_offset(i, fl.quads[f]);
      for (uint32_t q = 0; q < fl.quads[f]; ++q) dst[q] = src[q];
    }
}
inline void fields_scatter_emulate(const FieldList& fl, const uint8_t* accept, const uint32_t* idx, uint32_t count, uint8_t rnd,
                                   uint8_t* rounds, uint8_t* done) {
  for (uint32_t i = 0; i < count; ++i) {
    if (accept[i] == 0) continue;
    for (uint32_t f = 0; f < fl.n; ++f) {
      const FieldQuad* src = (const FieldQuad*)fl.src[f] + field_offset(i, fl.quads[f]);
      FieldQuad* dst = (FieldQuad*)fl.dst[f] + field_offset(idx[i], fl.quads[f]);
      for (uint32_t q = 0; q < fl.quads[f]; ++q) dst[q] = src[q];
    }
    rounds[idx[i]] = rnd;
    done[idx[i]] = 1;
  }
}
inline void fields_zero_emulate(const FieldList& fl, const uint8_t* done, uint8_t* ok, uint64_t B) {
  for (uint64_t b = 0; b < B; ++b) {
    ok[b] = done[b];
    if (done[b]) continue;
    for (uint32_t f = 0; f < fl.n; ++f) {
      FieldQuad* dst = (FieldQuad*)fl.dst[f] + field_offset(b, fl.quads[f]);
      for (uint32_t q = 0; q < fl.quads[f]; ++q) dst[q] = FieldQuad{{0, 0}};
    }
  }
}

// ---- coins ---------------------------------------------------------------------------------------------------------------
constexpr int64_t kCoinR0 = (1ll << 31) - 1;
constexpr int64_t kCoinHalf = (kCoinR0 - 1) / 2;   // 2^30 - 1: the bound of the two uniform draws
constexpr uint64_t kCoinR = (uint64_t)kCoinR0 * (uint64_t)kCoinR0;
RZK_PL_HD int64_t prove_coin(int64_t a, int64_t b) { return (a + kCoinHalf) * kCoinR0 + (b + kCoinHalf); }

// ---- compaction ----------------------------------------------------------------------------------------------------------
constexpr uint32_t kCompactWaves = 16;
constexpr uint32_t kCompactTile = 64 * kCompactWaves;   // flags per trip of the workgroup

RZK_PL_HD bool compact_pending(uint8_t live, uint8_t done) { return live != 0 && done == 0; }
// pending lanes below `lane` in a wavefront whose pending lanes are the set bits of `ballot`
RZK_PL_HD uint32_t compact_lane_rank(uint64_t ballot, uint32_t lane) {
  const uint64_t below = ballot & ((1ull << lane) - 1ull);   // lane < 64
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__popcll(below);
#else
  return (uint32_t)__builtin_popcountll(below);
#endif
}
RZK_PL_HD uint32_t compact_wave_total(uint64_t ballot) { return compact_lane_rank(ballot, 63) + (uint32_t)(ballot >> 63); }
// pending flags of the wavefronts below `wave` in a tile with these totals per wavefront
RZK_PL_HD uint32_t compact_wave_base(const uint32_t* totals, uint32_t wave) {
  uint32_t s = 0;
  for (uint32_t w = 0; w < wave; ++w) s += totals[w];
  return s;
}

// the kernel, lane by lane on the host; idx past *count is not written
inline void compact_emulate(const uint8_t* live, const uint8_t* done, uint64_t B, uint32_t* idx, uint32_t* count) {
  uint32_t base = 0;
  for (uint64_t tile0 = 0; tile0 < B; tile0 += kCompactTile) {
    uint64_t ballots[kCompactWaves];
    uint32_t totals[kCompactWaves];
    for (uint32_t w = 0; w < kCompactWaves; ++w) {
      ballots[w] = 0;
      for (uint32_t lane = 0; lane < 64; ++lane) {
        const uint64_t i = tile0 + w * 64 + lane;
        if (i < B && compact_pending(live[i], done[i])) ballots[w] |= 1ull << lane;
      }
      totals[w] = compact_wave_total(ballots[w]);
    }
    for (uint32_t w = 0; w < kCompactWaves; ++w)
      for (uint32_t lane = 0; lane < 64; ++lane)
        if ((ballots[w] >> lane) & 1ull)
          idx[base + compact_wave_base(totals, w) + compact_lane_rank(ballots[w], lane)] = (uint32_t)(tile0 + w * 64 + lane);
    base += compact_wave_base(totals, kCompactWaves);
  }
  *count = base;
}

}  // namespace rzk
