// CPU driver of ring_zk_amd/csrc/rzk_dgauss.h (with rzk_chacha.h for the blocks) for tests/test_dgauss_host.py
// (g++ -fsanitize=address,undefined).  Reads records from the file named on the command line and prints one line per record:
//   u32 1, u32 sigma                                            -> "params <C as 32 hex digits> <k> <y_rej>"
//   u32 2, u32 n, n x u64 f                                     -> "exp2m <n values>"
//   u32 3, u32 sigma, u32 n, n x u32 w[8]                       -> "trial <n x (accepted value)>"
//   u32 4, key[32], nonce[16], u32 stream, u32 N, u32 sigma, u64 poly -> "sample <N coefficients>"
//   u32 5, u32 sigma                                            -> "law <8k x (a kind T)>": the acceptance of every z = 0 .. 8k - 1
//   u32 6, u32 n, n x (u32 a, u64 f)                            -> "threshold <n x (kind T)>"
//   u32 7, u32 sigma, u32 N                                     -> "exhaust <blocks read> <N coefficients>": the stream
//          sampler over a block source whose words always fail the trial (all zero: the Lemire rejection of x)
// The stream sampler is the sequential statement of what the kernel draws in parallel.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../ring_zk_amd/csrc/rzk_chacha.h"
#include "../../ring_zk_amd/csrc/rzk_dgauss.h"

using namespace rzk;

static bool rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

struct ChaChaSource {
  const uint32_t* sub;
  uint32_t stream;
  uint64_t poly, blocks = 0;
  void operator()(uint32_t w12, uint32_t out[16]) {
    ++blocks;
    chacha20_block(sub, w12, (uint32_t)poly, (uint32_t)(poly >> 32), stream, out);
  }
};

struct ZeroSource {
  uint64_t blocks = 0;
  void operator()(uint32_t, uint32_t out[16]) {
    ++blocks;
    for (int i = 0; i < 16; ++i) out[i] = 0;
  }
};

template <class Source>
static std::vector<int64_t> sample_poly(Source& src, const DgaussParams& P, uint32_t N) {
  std::vector<int64_t> out(N, 0);
  for (uint32_t j = 0; 2 * j < N; ++j) {
    bool open[2] = {true, 2 * j + 1 < N};
    for (uint32_t t = 0; t < kDgaussTMax && (open[0] || open[1]); ++t) {
      uint32_t w[16];
      src(dgauss_w12(t, j), w);
      for (int c = 0; c < 2; ++c) {
        int64_t v;
        if (open[c] && dgauss_trial(P, w[8 * c], w[8 * c + 1], w[8 * c + 2], w[8 * c + 3], w[8 * c + 4], w[8 * c + 5], v))
          out[2 * j + c] = v, open[c] = false;
      }
    }
  }
  return out;
}

static void print_coefs(const std::vector<int64_t>& v) {
  for (int64_t x : v) printf(" %lld", (long long)x);
  printf("\n");
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t type;
  while (rd(f, &type, 4)) {
    if (type == 2 || type == 6) {
      uint32_t n;
      if (!rd(f, &n, 4) || n > (1u << 24)) return 3;
      printf(type == 2 ? "exp2m" : "threshold");
      for (uint32_t i = 0; i < n; ++i) {
        uint32_t a = 0;
        uint64_t v, T;
        if ((type == 6 && !rd(f, &a, 4)) || !rd(f, &v, 8)) return 3;
        if (type == 2) {
          if (v == 0) return 4;
          printf(" %" PRIu64, dgauss_exp2m(v));
        } else {
          const int kind = dgauss_threshold(a, v, T);
          printf(" %d %" PRIu64, kind, T);
        }
      }
      printf("\n");
      continue;
    }
    if (type == 4) {
      uint8_t key[32], nonce[16];
      uint32_t a[3], sub[8];
      uint64_t poly;
      if (!rd(f, key, 32) || !rd(f, nonce, 16) || !rd(f, a, 12) || !rd(f, &poly, 8)) return 3;
      if (a[1] == 0 || a[1] > (1u << 16) || a[2] == 0 || a[2] > kDgaussSigmaMax) return 4;
      chacha_sampler_subkey(key, nonce, sub);
      ChaChaSource src{sub, a[0], poly};
      printf("sample");
      print_coefs(sample_poly(src, dgauss_params(a[2]), a[1]));
      continue;
    }
    uint32_t sigma;
    if (!rd(f, &sigma, 4) || sigma == 0 || sigma > kDgaussSigmaMax) return 3;
    const DgaussParams P = dgauss_params(sigma);
    if (type == 1) {
      printf("params %016" PRIx64 "%016" PRIx64 " %u %u\n", P.c_hi, P.c_lo, P.k, P.y_rej);
    } else if (type == 3) {
      uint32_t n;
      if (!rd(f, &n, 4) || n > (1u << 24)) return 3;
      std::vector<uint32_t> w(8 * (size_t)n);
      if (!rd(f, w.data(), 4 * w.size())) return 3;
      printf("trial");
      for (size_t i = 0; i < n; ++i) {
        int64_t v;
        const bool ok = dgauss_trial(P, w[8 * i], w[8 * i + 1], w[8 * i + 2], w[8 * i + 3], w[8 * i + 4], w[8 * i + 5], v);
        printf(" %d %lld", ok ? 1 : 0, (long long)v);
      }
      printf("\n");
    } else if (type == 5) {
      if (P.k > 4096) return 4;
      printf("law");
      for (uint32_t z = 0; z < 8 * P.k; ++z) {
        uint32_t a;
        uint64_t fr, T;
        dgauss_exponent(P, z / P.k, z % P.k, a, fr);
        const int kind = dgauss_threshold(a, fr, T);
        printf(" %u %d %" PRIu64, a, kind, T);
      }
      printf("\n");
    } else if (type == 7) {
      uint32_t N;
      if (!rd(f, &N, 4) || N == 0 || N > 4096) return 3;
      ZeroSource src;
      const std::vector<int64_t> v = sample_poly(src, P, N);
      printf("exhaust %" PRIu64, src.blocks);
      print_coefs(v);
    } else {
      return 4;
    }
  }
  fclose(f);
  return 0;
}
