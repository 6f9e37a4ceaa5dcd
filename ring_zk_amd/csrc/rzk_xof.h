// rzk_xof.h — the "XP1" expansion of 32-byte seeds into uniform elements of R_q with SHAKE256, shared by
// the GPU kernel (rzk_xof_dev.hip), the C-ABI host code and the CPU test (tests/test_xof_host.py, g++).  Plain C++; the
// sponge is the one of rzk_keccak.h.  Every input is public: commitment keys (domain 0) and the public multipliers of
// Linear / Sum proofs (any other domain) come from here, secrets never do (they stay with the keyed samplers).
//
//   CH        = min(N, 256)                      coefficients per chunk (the FS1 leaf length); C = N / CH chunks per polynomial
//   W         = bitlen(q - 1), mask = 2^W - 1    (q <= 2^32)
//   msg(p, c) = "RZKXP1\0U" | le64(q) | le32(N) | le32(domain) | seed[0:32] | le32(p) | le32(c)      64 bytes = 8 whole words
//   stream    = SHAKE256(msg(p, c)), read as little-endian 32-bit words w_0, w_1, ...
//               (w_2i is the low half and w_2i+1 the high half of the i-th squeezed 64-bit word)
//   candidate   v = w & mask; accepted iff v < q; value = v - (q - 1) / 2      (the centred canonical residue)
//   chunk c of polynomial p = the first CH accepted values of stream, in order -> coefficients c CH .. c CH + CH - 1
//
// Every coefficient is exactly uniform over the q residues; a word is accepted with probability q / 2^W > 1/2.  The
// message fills less than one rate block, so a chunk is one absorbed block and then as many squeezed blocks of 34 words
// as its rejections ask for (no fixed count: not constant time, which is harmless here).  Chunks are independent sponge
// instances: a polynomial is C parallel lanes, and any chunk can be recomputed alone.
#pragma once
#include <stdint.h>

#include "rzk_keccak.h"

namespace rzk {

constexpr uint64_t kXofTag = 0x55003150584b5a52ull;   // "RZKXP1\0U" as a little-endian word
constexpr uint32_t kXofMsgWords = 8;
constexpr uint32_t kXofChunkMax = kFsLeafMax;         // coefficients per chunk: min(N, 256)
constexpr uint32_t kXofBlockWords32 = 2 * kShakeRateWords;   // 32-bit stream words per squeezed block
constexpr uint32_t kXofDomainKey = 0;                 // RZK_XOF_DOMAIN_KEY: commitment keys

RZK_FS_HD uint32_t xof_chunk_len(uint32_t N) { return N < kXofChunkMax ? N : kXofChunkMax; }
RZK_FS_HD uint32_t xof_mask(uint64_t q) {   // 2^bitlen(q - 1) - 1, 2 <= q <= 2^32
  uint32_t m = (uint32_t)(q - 1);
  m |= m >> 1;
  m |= m >> 2;
  m |= m >> 4;
  m |= m >> 8;
  m |= m >> 16;
  return m;
}
RZK_FS_HD void xof_seed_words(const uint8_t seed[32], uint64_t w[4]) {
  for (uint32_t i = 0; i < 4; ++i) w[i] = shake256_load_le(seed + 8 * i, 8);
}

struct XofMsgWords {   // word i of msg(p, c); i is a compile-time constant wherever the sponge asks (rzk_keccak.h)
  uint64_t q, nd;      // le64(q); le32(N) | le32(domain)
  uint64_t s0, s1, s2, s3;   // seed[0:32]
  uint64_t pc;         // le32(p) | le32(c)
  RZK_FS_HD uint64_t operator()(uint32_t i) const {
    switch (i) {
      case 0: return kXofTag;
      case 1: return q;
      case 2: return nd;
      case 3: return s0;
      case 4: return s1;
      case 5: return s2;
      case 6: return s3;
      default: return pc;
    }
  }
};

// state whose s[0 .. 16] is the first squeezed block of stream(p, c)
RZK_FS_HD void xof_start(uint64_t (&s)[25], uint64_t q, uint32_t N, uint32_t domain, const uint64_t seed[4], uint32_t p,
                         uint32_t c) {
  XofMsgWords word{q, (uint64_t)N | ((uint64_t)domain << 32), seed[0], seed[1], seed[2], seed[3], (uint64_t)p | ((uint64_t)c << 32)};
  RZK_FS_UNROLL
  for (int i = 0; i < 25; ++i) s[i] = 0;
  shake256_absorb_block(s, word, 0, kXofMsgWords, 0x1Full);
}

// One stream word: appends its value to the chunk when there is room and the candidate is below q.  put(i, raw) stores
// the i-th accepted candidate (the kernel parks raw values in LDS, the scalar form writes the centred value).
template <class Put>
RZK_FS_HD void xof_take(uint32_t w, uint32_t q32, uint32_t mask, uint32_t need, uint32_t& cnt, Put& put) {
  const uint32_t v = w & mask;
  if (cnt < need && (q32 == 0 || v < q32)) {   // (q32 == 0: q = 2^32, every word is a residue)
    put(cnt, v);
    ++cnt;
  }
}

// ---- scalar reference form: chunk c of polynomial p into out[0 .. CH); returns the 32-bit words consumed -----------------
struct XofPutCentred {
  int64_t* out;
  int64_t half;
  RZK_FS_HD void operator()(uint32_t i, uint32_t raw) const { out[i] = (int64_t)raw - half; }
};
RZK_FS_HD uint32_t xof_chunk(uint64_t q, uint32_t N, uint32_t domain, const uint8_t seed[32], uint32_t p, uint32_t c,
                             int64_t* out) {
  uint64_t sw[4], s[25];
  xof_seed_words(seed, sw);
  xof_start(s, q, N, domain, sw, p, c);
  const uint32_t need = xof_chunk_len(N), mask = xof_mask(q), q32 = (uint32_t)q;
  XofPutCentred put{out, (int64_t)((q - 1) / 2)};
  uint32_t cnt = 0, words = 0;
  for (;;) {
    for (uint32_t j = 0; j < kShakeRateWords; ++j) {
      const uint64_t x = shake256_pick(s, j);
      for (uint32_t h = 0; h < 2; ++h) {
        xof_take((uint32_t)(x >> (32 * h)), q32, mask, need, cnt, put);
        ++words;
        if (cnt == need) return words;
      }
    }
    keccak_f1600(s);
  }
}
// polynomial p under (seed, domain): out[0 .. N)
RZK_FS_HD void xof_poly(uint64_t q, uint32_t N, uint32_t domain, const uint8_t seed[32], uint32_t p, int64_t* out) {
  const uint32_t ch = xof_chunk_len(N);
  for (uint32_t c = 0; c < N / ch; ++c) xof_chunk(q, N, domain, seed, p, c, out + (uint64_t)c * ch);
}

}  // namespace rzk
