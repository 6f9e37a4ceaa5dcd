// rzk_chacha.h — ChaCha20 (RFC 8439) as the generator of the keyed device samplers, shared by the GPU
// kernels (rzk_csprng_dev.hip), the host side of the entry points (rzk_samplers.cpp: the subkey) and the CPU test
// (tests/test_chacha.py, g++).  Plain C++.
//
// Stream of one call (fixed to the byte):
//   subkey                   = HChaCha20(key[32], nonce[16])          on the host, once per call (the XChaCha construction)
//   block(stream, poly, blk) = ChaCha20_block(subkey, w12 = blk, w13 = poly & 0xffffffff, w14 = poly >> 32, w15 = stream)
// poly is the index of the polynomial within the call, blk counts 64-byte blocks inside that polynomial.  One block
// (16 words w[0..15]) serves 8 coefficients, or 8 steps of the challenge sampler; a block never spans two polynomials
// (at N = 4 a polynomial uses the first 4 coefficients of its block 0 and drops the rest).
//
// Word-to-coefficient maps (the functions at the end; the distributions are those of rzk_sample.h, only the source of
// the words differs):
//   uniform    coefficient 8 blk + j            = uniform_below(w[2j], w[2j+1], 2 bound + 1) - bound
//   gauss      Box-Muller pair i = 0..3 of a block gives coefficients 8 blk + 2i, 8 blk + 2i + 1 from w[4i .. 4i+3]
//   challenge  Floyd step t uses block t >> 3, w0 = w[2 (t & 7)], w1 = w[2 (t & 7) + 1]
// so "quarter" i of a block (words 4i .. 4i+3) is what one Philox block is to the seeded samplers: two coefficients.
#pragma once
#include <stdint.h>

#include "rzk_gauss.h"
#include "rzk_rng.h"

namespace rzk {

// "expand 32-byte k": words 0 .. 3 of every state
RZK_HD uint32_t chacha_sigma(int i) { return i == 0 ? 0x61707865u : i == 1 ? 0x3320646eu : i == 2 ? 0x79622d32u : 0x6b206574u; }

RZK_HD uint32_t chacha_rotl(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }   // n in 1 .. 31

RZK_HD void chacha_quarter_round(uint32_t& a, uint32_t& b, uint32_t& c, uint32_t& d) {
  a += b, d ^= a, d = chacha_rotl(d, 16);
  c += d, b ^= c, b = chacha_rotl(b, 12);
  a += b, d ^= a, d = chacha_rotl(d, 8);
  c += d, b ^= c, b = chacha_rotl(b, 7);
}

// the 20 rounds (10 column + diagonal double rounds) on a 4 x 4 state, row-major
RZK_HD void chacha20_rounds(uint32_t (&x)[16]) {
  for (int r = 0; r < 10; ++r) {
    chacha_quarter_round(x[0], x[4], x[8], x[12]);
    chacha_quarter_round(x[1], x[5], x[9], x[13]);
    chacha_quarter_round(x[2], x[6], x[10], x[14]);
    chacha_quarter_round(x[3], x[7], x[11], x[15]);
    chacha_quarter_round(x[0], x[5], x[10], x[15]);
    chacha_quarter_round(x[1], x[6], x[11], x[12]);
    chacha_quarter_round(x[2], x[7], x[8], x[13]);
    chacha_quarter_round(x[3], x[4], x[9], x[14]);
  }
}

// RFC 8439 §2.3 with the words 12 .. 15 (counter and nonce there) passed directly; out = rounds(state) + state
RZK_HD void chacha20_block(const uint32_t key[8], uint32_t w12, uint32_t w13, uint32_t w14, uint32_t w15, uint32_t out[16]) {
  uint32_t s[16], x[16];
  for (int i = 0; i < 4; ++i) s[i] = chacha_sigma(i);
  for (int i = 0; i < 8; ++i) s[4 + i] = key[i];
  s[12] = w12, s[13] = w13, s[14] = w14, s[15] = w15;
  for (int i = 0; i < 16; ++i) x[i] = s[i];
  chacha20_rounds(x);
  for (int i = 0; i < 16; ++i) out[i] = x[i] + s[i];
}

// HChaCha20 (draft-irtf-cfrg-xchacha §2.2): the same rounds without the feed-forward; words 0 .. 3 and 12 .. 15
RZK_HD void hchacha20(const uint32_t key[8], const uint32_t nonce[4], uint32_t subkey[8]) {
  uint32_t x[16];
  for (int i = 0; i < 4; ++i) x[i] = chacha_sigma(i);
  for (int i = 0; i < 8; ++i) x[4 + i] = key[i];
  for (int i = 0; i < 4; ++i) x[12 + i] = nonce[i];
  chacha20_rounds(x);
  for (int i = 0; i < 4; ++i) subkey[i] = x[i], subkey[4 + i] = x[12 + i];
}

RZK_HD uint32_t chacha_load_le32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// subkey of a call from the key and nonce bytes (words are little-endian, as in the RFC)
RZK_HD void chacha_sampler_subkey(const uint8_t key[32], const uint8_t nonce[16], uint32_t subkey[8]) {
  uint32_t k[8], n[4];
  for (int i = 0; i < 8; ++i) k[i] = chacha_load_le32(key + 4 * i);
  for (int i = 0; i < 4; ++i) n[i] = chacha_load_le32(nonce + 4 * i);
  hchacha20(k, n, subkey);
}

// block blk of polynomial poly of the call's stream
RZK_HD void chacha_sampler_block(const uint32_t subkey[8], uint32_t stream, uint64_t poly, uint32_t blk, uint32_t out[16]) {
  chacha20_block(subkey, blk, (uint32_t)poly, (uint32_t)(poly >> 32), stream, out);
}

// ---- word-to-coefficient maps ----------------------------------------------------------------------------------------
// uniform in [-bound, bound] from the word pair (w[2j], w[2j+1]); bias <= (2 bound + 1) / 2^64
RZK_HD int64_t chacha_uniform_coef(uint32_t w_even, uint32_t w_odd, uint32_t bound) {
  return (int64_t)uniform_below(w_even, w_odd, 2u * bound + 1u) - (int64_t)bound;
}

// gauss: quarter i = w[4i .. 4i+3] goes through gauss_pair_f32 (w[4i .. 4i+2]) or gauss_pair_f64 of rzk_gauss.h, the one
// statement of the Box-Muller map that the seeded kernel (rzk_sample.h) uses on the four words of a Philox block.

// Floyd step t of a kappa-subset of N positions, j = N - kappa + t: the candidate position in [0, j] and the sign
// (random_bool(0.5): +1 / -1) from the word pair (w0, w1) = (w[2 (t & 7)], w[2 (t & 7) + 1]) of block t >> 3.  The
// caller applies Floyd's rule: the candidate if it is still free, else j.
RZK_HD void chacha_challenge_step(uint32_t w0, uint32_t w1, uint32_t j, uint32_t& pick, int32_t& sign) {
  pick = uniform_below(w0, w1 & ~1u, j + 1);
  sign = (w1 & 1u) ? 1 : -1;
}

}  // namespace rzk
