// rzk_keccak.h — SHAKE256 and the "FS1" Fiat–Shamir transcript of the non-interactive proofs, shared by
// the GPU kernels (rzk_fs_dev.hip) and the CPU transcript test (tests/test_fs_transcript.py, g++).  Plain C++.
//
// Every FS1 hash input is a whole number of little-endian 64-bit words (the tags are 8 bytes, a leaf is 2 + LEAF/2
// words, a digest 4), so the sponge below absorbs words: word(i) is the i-th 64-bit word of the message, and only the
// byte-oriented wrapper for arbitrary messages needs the `tail` of 0 .. 7 bytes.  The state is indexed with
// compile-time constants only (unrolled lane loops, select chains where a position is a run-time value), so a kernel
// keeps it in registers.
//
//   leaf(p,c) = SHAKE256( "RZKFS1\0L" | le32(p) | le32(c) | le32 coefficients of P_p[c*LEAF .. (c+1)*LEAF) )[0:32]
//   keydigest = SHAKE256( "RZKFS1\0K" | le64(q) | le32(N) le32(n) le32(k) le32(l) le32(kappa) le32(0) | le64(b)
//                         | leaf(p,c) of the (n+l)*k key polynomials row-major, all c )[0:32]
//   stream    = SHAKE256( "RZKFS1\0R" | le32(kind) | le32(V) | keydigest | aux[32] | leaf(p,c), p = 0..M-1, c = 0..C-1 )
//   LEAF = min(N, 256), C = N / LEAF; stream[0:32] is the transcript digest, the challenge is sampled from stream[32:].
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RZK_FS_HD __host__ __device__ inline
#define RZK_FS_UNROLL _Pragma("unroll")
#define RZK_FS_NO_UNROLL _Pragma("unroll 1")
#else
#define RZK_FS_HD inline
#define RZK_FS_UNROLL
#define RZK_FS_NO_UNROLL
#endif

namespace rzk {

constexpr uint32_t kShakeRateWords = 17;   // SHAKE256: rate 136 bytes
constexpr uint32_t kFsDigestWords = 4;     // 32-byte digests
constexpr uint32_t kFsLeafMax = 256;       // coefficients per leaf: min(N, 256)
constexpr uint64_t kFsTagLeaf = 0x4c003153464b5a52ull;   // "RZKFS1\0L" as a little-endian word
constexpr uint64_t kFsTagKey = 0x4b003153464b5a52ull;    // "RZKFS1\0K"
constexpr uint64_t kFsTagRoot = 0x52003153464b5a52ull;   // "RZKFS1\0R"
constexpr uint32_t kFsKeyHeaderWords = 6;
constexpr uint32_t kFsRootHeaderWords = 10;

RZK_FS_HD uint64_t keccak_rotl(uint64_t x, int n) { return (x << n) | (x >> (64 - n)); }   // n in 1 .. 63

// Keccak-f[1600] (FIPS 202 §3.3), lane (x, y) at s[5 y + x].  The round loop stays a loop on the device (24 x ~330
// vector instructions unrolled would not fit the instruction cache); everything inside a round has constant indices.
RZK_FS_HD void keccak_f1600(uint64_t (&s)[25]) {
  static constexpr uint64_t kRC[24] = {
      0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull,
      0x000000000000808bull, 0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull,
      0x000000000000008aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000aull,
      0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull, 0x8000000000008003ull,
      0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800aull, 0x800000008000000aull,
      0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
  constexpr int kRot[24] = {1, 3, 6, 10, 15, 21, 28, 36, 45, 55, 2, 14, 27, 41, 56, 8, 25, 43, 62, 18, 39, 61, 20, 44};
  constexpr int kPi[24] = {10, 7, 11, 17, 18, 3, 5, 16, 8, 21, 24, 4, 15, 23, 19, 13, 12, 2, 20, 14, 22, 9, 6, 1};
  RZK_FS_NO_UNROLL
  for (int r = 0; r < 24; ++r) {
    uint64_t bc[5];
    RZK_FS_UNROLL
    for (int x = 0; x < 5; ++x) bc[x] = s[x] ^ s[x + 5] ^ s[x + 10] ^ s[x + 15] ^ s[x + 20];   // theta
    RZK_FS_UNROLL
    for (int x = 0; x < 5; ++x) {
      const uint64_t t = bc[(x + 4) % 5] ^ keccak_rotl(bc[(x + 1) % 5], 1);
      RZK_FS_UNROLL
      for (int y = 0; y < 25; y += 5) s[y + x] ^= t;
    }
    uint64_t t = s[1];   // rho and pi
    RZK_FS_UNROLL
    for (int i = 0; i < 24; ++i) {
      const uint64_t keep = s[kPi[i]];
      s[kPi[i]] = keccak_rotl(t, kRot[i]);
      t = keep;
    }
    RZK_FS_UNROLL
    for (int y = 0; y < 25; y += 5) {   // chi
      RZK_FS_UNROLL
      for (int x = 0; x < 5; ++x) bc[x] = s[y + x];
      RZK_FS_UNROLL
      for (int x = 0; x < 5; ++x) s[y + x] ^= ~bc[(x + 1) % 5] & bc[(x + 2) % 5];
    }
    s[0] ^= kRC[r];   // iota
  }
}

// Absorbs rate block `blk` of a message of `nwords` whole words followed by `last` — the 0 .. 7 trailing message bytes
// with the SHAKE domain byte 0x1F behind them, as one little-endian word — and permutes.  blk runs over
// 0 .. nwords / 17; the block that holds `last` also gets the closing 0x80 of the pad10*1 rule.
template <class Word>
RZK_FS_HD void shake256_absorb_block(uint64_t (&s)[25], Word& word, uint32_t blk, uint32_t nwords, uint64_t last) {
  const uint32_t base = blk * kShakeRateWords;
  RZK_FS_UNROLL
  for (uint32_t j = 0; j < kShakeRateWords; ++j) {
    const uint32_t i = base + j;
    if (i < nwords) s[j] ^= word(i);
    else if (i == nwords) s[j] ^= last;
  }
  if (nwords - base < kShakeRateWords) s[kShakeRateWords - 1] ^= 0x8000000000000000ull;
  keccak_f1600(s);
}

// State after absorbing the whole message: s[0 .. 16] is the first squeezed block.
template <class Word>
RZK_FS_HD void shake256_absorb(uint64_t (&s)[25], Word& word, uint32_t nwords, uint64_t tail, uint32_t tail_bytes) {
  RZK_FS_UNROLL
  for (int i = 0; i < 25; ++i) s[i] = 0;
  const uint64_t last = tail | (0x1Full << (8 * tail_bytes));
  for (uint32_t blk = 0; blk <= nwords / kShakeRateWords; ++blk) shake256_absorb_block(s, word, blk, nwords, last);
}

// s[w] for a run-time w < 17 without indexing the state dynamically
RZK_FS_HD uint64_t shake256_pick(const uint64_t (&s)[25], uint32_t w) {
  uint64_t v = 0;
  RZK_FS_UNROLL
  for (uint32_t j = 0; j < kShakeRateWords; ++j)
    if (j == w) v = s[j];
  return v;
}

// Reader of the squeezed stream as little-endian 16-bit words, from a byte offset that is a multiple of 8.
struct ShakeWords16 {
  uint32_t w;     // next state word
  uint32_t left;  // 16-bit words left in cur
  uint64_t cur;
};
RZK_FS_HD uint32_t shake256_next16(uint64_t (&s)[25], ShakeWords16& r) {
  if (r.left == 0) {
    if (r.w == kShakeRateWords) {
      keccak_f1600(s);
      r.w = 0;
    }
    r.cur = shake256_pick(s, r.w++);
    r.left = 4;
  }
  const uint32_t v = (uint32_t)r.cur & 0xffffu;
  r.cur >>= 16;
  --r.left;
  return v;
}

// The FS1 challenge from stream[32:]: exactly kappa coefficients +-1, uniform over positions and signs (an inside-out
// Fisher-Yates over the last kappa indices; a draw j = w & mask is accepted when j <= i, with probability > 1/2; bit 15
// of the accepted word is the sign, free because N <= 2048).  c[0 .. N) must be zero on entry; kappa <= N.
// Coef: int64_t, or int32_t for a 32-bit slab (the values are 0 and +-1 either way).
template <class Coef>
RZK_FS_HD void fs_sample_challenge(uint64_t (&s)[25], Coef* c, uint32_t N, uint32_t kappa) {
  ShakeWords16 r{kFsDigestWords, 0, 0};
  for (uint32_t i = N - kappa; i < N; ++i) {
    uint32_t mask = i;   // (1 << bit_length(i)) - 1
    mask |= mask >> 1;
    mask |= mask >> 2;
    mask |= mask >> 4;
    mask |= mask >> 8;
    uint32_t w, j;
    do {
      w = shake256_next16(s, r);
      j = w & mask;
    } while (j > i);
    c[i] = c[j];
    c[j] = 1 - 2 * (Coef)(w >> 15);
  }
}

// ---- byte-oriented SHAKE256 (any message length; the CPU test's known answers) ---------------------------------------
RZK_FS_HD uint64_t shake256_load_le(const uint8_t* p, uint32_t nbytes) {
  uint64_t v = 0;
  for (uint32_t i = 0; i < nbytes; ++i) v |= (uint64_t)p[i] << (8 * i);
  return v;
}
struct ShakeByteWords {
  const uint8_t* p;
  RZK_FS_HD uint64_t operator()(uint32_t i) const { return shake256_load_le(p + 8 * (uint64_t)i, 8); }
};
RZK_FS_HD void shake256(const uint8_t* msg, uint32_t len, uint8_t* out, uint32_t outlen) {
  uint64_t s[25];
  ShakeByteWords word{msg};
  shake256_absorb(s, word, len / 8, shake256_load_le(msg + (len & ~7u), len & 7u), len & 7u);
  uint32_t w = 0;
  for (uint32_t o = 0; o < outlen; o += 8) {
    if (w == kShakeRateWords) {
      keccak_f1600(s);
      w = 0;
    }
    const uint64_t v = shake256_pick(s, w++);
    for (uint32_t i = 0; i < 8 && o + i < outlen; ++i) out[o + i] = (uint8_t)(v >> (8 * i));
  }
}

// ---- FS1 word streams -------------------------------------------------------------------------------------------------
RZK_FS_HD uint32_t fs_leaf_len(uint32_t N) { return N < kFsLeafMax ? N : kFsLeafMax; }
RZK_FS_HD uint32_t fs_leaf_words(uint32_t N) { return 2 + fs_leaf_len(N) / 2; }
// word i >= 2 of a leaf: coefficients 2(i-2) and 2(i-2)+1 as little-endian two's-complement int32
RZK_FS_HD uint64_t fs_pack_coefs(int64_t lo, int64_t hi) { return (uint64_t)(uint32_t)lo | ((uint64_t)(uint32_t)hi << 32); }

// leaf (p, c) over coefficients that sit in memory as int64, or as the int32 of a 32-bit slab: the word the hash takes is
// the int32 itself (the CPU form; the kernel stages them)
template <class Coef>
struct FsLeafWordsT {
  const Coef* coef;   // P_p + c * LEAF
  uint32_t p, c;
  RZK_FS_HD uint64_t operator()(uint32_t i) const {
    if (i == 0) return kFsTagLeaf;
    if (i == 1) return (uint64_t)p | ((uint64_t)c << 32);
    return fs_pack_coefs(coef[2 * (i - 2)], coef[2 * (i - 2) + 1]);
  }
};
using FsLeafWords = FsLeafWordsT<int64_t>;
template <class Coef>
RZK_FS_HD void fs_leaf(const Coef* poly, uint32_t N, uint32_t p, uint32_t c, uint64_t out[kFsDigestWords]) {
  uint64_t s[25];
  FsLeafWordsT<Coef> word{poly + (uint64_t)c * fs_leaf_len(N), p, c};
  shake256_absorb(s, word, fs_leaf_words(N), 0, 0);
  for (uint32_t i = 0; i < kFsDigestWords; ++i) out[i] = s[i];
}

// header words of the key digest and of a proof's root
RZK_FS_HD void fs_key_header(int64_t q, uint32_t N, uint32_t n, uint32_t k, uint32_t l, uint32_t kappa, uint64_t b,
                             uint64_t h[kFsKeyHeaderWords]) {
  h[0] = kFsTagKey;
  h[1] = (uint64_t)q;
  h[2] = (uint64_t)N | ((uint64_t)n << 32);
  h[3] = (uint64_t)k | ((uint64_t)l << 32);
  h[4] = (uint64_t)kappa;
  h[5] = b;
}
RZK_FS_HD void fs_root_header(uint32_t kind, uint32_t V, const uint64_t keydigest[kFsDigestWords],
                              const uint64_t aux[kFsDigestWords], uint64_t h[kFsRootHeaderWords]) {
  h[0] = kFsTagRoot;
  h[1] = (uint64_t)kind | ((uint64_t)V << 32);
  for (uint32_t i = 0; i < kFsDigestWords; ++i) {
    h[2 + i] = keydigest[i];
    h[6 + i] = aux[i];
  }
}

// header (nhdr <= 10 words) followed by leaf digests; digest word w of leaf j at dig[(j * 4 + w) * stride + at]
struct FsRootWords {
  const uint64_t* hdr;
  uint32_t nhdr;
  const uint64_t* dig;
  uint64_t stride, at;
  RZK_FS_HD uint64_t operator()(uint32_t i) const {
    if (i < nhdr) {
      uint64_t v = 0;
      RZK_FS_UNROLL
      for (uint32_t j = 0; j < kFsRootHeaderWords; ++j)
        if (j == i) v = hdr[j];
      return v;
    }
    return dig[(uint64_t)(i - nhdr) * stride + at];
  }
};

}  // namespace rzk
