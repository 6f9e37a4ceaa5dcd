// CPU driver of ring_zk_amd/csrc/rzk_chacha.h for tests/test_chacha.py (g++ -fsanitize=address,undefined).
// Reads records from the file named on the command line and prints one line of results per record:
//   u32 1, key[32], u32 w12 w13 w14 w15                                   -> "block <hex of the 64 bytes>"
//   u32 2, key[32], nonce[16]                                             -> "hchacha <hex of the 32 bytes>"
//   u32 3, key[32], nonce[16], u32 stream, u32 N, u32 bound, u64 poly     -> "uniform <N coefficients>"
//   u32 4, key[32], nonce[16], u32 stream, u32 N, u32 kappa, u64 poly     -> "challenge <N coefficients>"
//   u32 5, u32 f32, f64 sigma, u32 pairs, pairs x u32 w0 w1 w2 w3         -> "gauss <2 pairs coefficients>": the Gaussian
//          word-to-pair map (rzk_gauss.h) on the given words, gauss_pair_f32 for f32 != 0, else gauss_pair_f64
// The samplers are the sequential statement of what the kernels draw in parallel: one block per 8 coefficients / 8
// Floyd steps, through the header's own word-to-coefficient maps.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../ring_zk_amd/csrc/rzk_chacha.h"

using namespace rzk;

static bool rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

static void hex_words(const uint32_t* w, size_t n) {
  for (size_t i = 0; i < n; ++i)
    for (int b = 0; b < 4; ++b) printf("%02x", (unsigned)((w[i] >> (8 * b)) & 0xffu));   // little-endian words
}

static std::vector<int64_t> sample_uniform(const uint32_t sub[8], uint32_t stream, uint64_t poly, uint32_t N, uint32_t bound) {
  std::vector<int64_t> out(N);
  for (uint32_t blk = 0; 8 * blk < N; ++blk) {
    uint32_t w[16];
    chacha_sampler_block(sub, stream, poly, blk, w);
    for (uint32_t j = 0; j < 8 && 8 * blk + j < N; ++j) out[8 * blk + j] = chacha_uniform_coef(w[2 * j], w[2 * j + 1], bound);
  }
  return out;
}

static std::vector<int64_t> sample_challenge(const uint32_t sub[8], uint32_t stream, uint64_t poly, uint32_t N, uint32_t kappa) {
  std::vector<int64_t> out(N, 0);
  const uint32_t kap = kappa < N ? kappa : N;
  uint32_t w[16] = {};
  for (uint32_t t = 0; t < kap; ++t) {
    if ((t & 7u) == 0) chacha_sampler_block(sub, stream, poly, t >> 3, w);
    const uint32_t j = N - kap + t;
    uint32_t pick;
    int32_t sign;
    chacha_challenge_step(w[2 * (t & 7u)], w[2 * (t & 7u) + 1], j, pick, sign);
    out[out[pick] ? j : pick] = sign;
  }
  return out;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t type;
  while (rd(f, &type, 4)) {
    if (type == 5) {
      uint32_t f32, pairs;
      double sigma;
      if (!rd(f, &f32, 4) || !rd(f, &sigma, 8) || !rd(f, &pairs, 4) || pairs > (1u << 24)) return 3;
      std::vector<uint32_t> w(4 * (size_t)pairs);
      if (!rd(f, w.data(), 4 * w.size())) return 3;
      printf("gauss");
      for (size_t i = 0; i < pairs; ++i) {
        int64_t v0, v1;
        if (f32) gauss_pair_f32(w[4 * i], w[4 * i + 1], w[4 * i + 2], (float)sigma, v0, v1);
        else gauss_pair_f64(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3], sigma, v0, v1);
        printf(" %lld %lld", (long long)v0, (long long)v1);
      }
      printf("\n");
      continue;
    }
    uint8_t key[32], nonce[16];
    if (!rd(f, key, 32)) return 3;
    if (type == 1) {
      uint32_t k[8], c[4], out[16];
      if (!rd(f, c, 16)) return 3;
      for (int i = 0; i < 8; ++i) k[i] = chacha_load_le32(key + 4 * i);
      chacha20_block(k, c[0], c[1], c[2], c[3], out);
      printf("block ");
      hex_words(out, 16);
      printf("\n");
      continue;
    }
    if (!rd(f, nonce, 16)) return 3;
    uint32_t sub[8];
    chacha_sampler_subkey(key, nonce, sub);
    if (type == 2) {
      printf("hchacha ");
      hex_words(sub, 8);
      printf("\n");
      continue;
    }
    uint32_t a[3];
    uint64_t poly;
    if (!rd(f, a, 12) || !rd(f, &poly, 8)) return 3;
    if (type != 3 && type != 4) return 4;
    if (a[1] == 0 || a[1] > (1u << 16)) return 4;
    const std::vector<int64_t> v = type == 3 ? sample_uniform(sub, a[0], poly, a[1], a[2]) : sample_challenge(sub, a[0], poly, a[1], a[2]);
    printf(type == 3 ? "uniform" : "challenge");
    for (int64_t x : v) printf(" %lld", (long long)x);
    printf("\n");
  }
  fclose(f);
  return 0;
}
