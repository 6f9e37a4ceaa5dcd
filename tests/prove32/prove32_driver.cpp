// CPU driver of tests/test_prove32_host.py (g++ -fsanitize=address,undefined): the word-to-coefficient maps of the keyed
// samplers (rzk_chacha.h, rzk_gauss.h, rzk_dgauss.h) at the extremes of the arguments the 32-bit entry points accept and on
// a seeded sweep, to establish that every value they can produce is an int32_t (rzk_slab32.h: what narrow keeps).
// Prints one line per map: "<name> <max |v|> <values evaluated> <values with (int32_t)v != v>".
//   usage: prove32_driver <seed> <sweep length>
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../ring_zk_amd/csrc/rzk_chacha.h"
#include "../../ring_zk_amd/csrc/rzk_dgauss.h"
#include "../../ring_zk_amd/csrc/rzk_gauss.h"
#include "../../ring_zk_amd/csrc/rzk_slab32.h"

using namespace rzk;

namespace {

struct Stat {
  uint64_t max_abs = 0, n = 0, misfit = 0;
  void take(int64_t v) {
    const uint64_t a = v < 0 ? 0 - (uint64_t)v : (uint64_t)v;
    if (a > max_abs) max_abs = a;
    ++n;
    if ((int64_t)(int32_t)(uint32_t)(uint64_t)v != v) ++misfit;   // the low word, sign-extended again (slab32_narrow / slab32_widen)
  }
  void print(const char* name) const { printf("%s %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", name, max_abs, n, misfit); }
};

uint64_t splitmix(uint64_t& s) {
  uint64_t z = (s += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  uint64_t seed = strtoull(argv[1], nullptr, 10);
  const uint64_t sweep = strtoull(argv[2], nullptr, 10);
  const uint32_t kAll = 0xffffffffu;

  // uniform(h) for the smallest, the default and the largest modulus: all-zero and all-one words, then the sweep
  const uint64_t moduli[3] = {3ull, 3515337053ull, 4294606851ull};
  const char* const names[3] = {"uniform_qmin", "uniform_qdefault", "uniform_qmax"};
  for (int i = 0; i < 3; ++i) {
    const uint32_t h = slab32_half(moduli[i]);
    Stat s;
    s.take(chacha_uniform_coef(0, 0, h));
    s.take(chacha_uniform_coef(kAll, kAll, h));
    s.take(chacha_uniform_coef(0, kAll, h));
    s.take(chacha_uniform_coef(kAll, 0, h));
    for (uint64_t j = 0; j < sweep; ++j) {
      const uint64_t w = splitmix(seed);
      s.take(chacha_uniform_coef((uint32_t)w, (uint32_t)(w >> 32), h));
    }
    s.print(names[i]);
  }

  // Box-Muller, double precision, sigma = 2^26 (the largest accepted): w0:w1 < 2^11 gives the smallest u0 = 2^-53 and so the
  // largest radius; the angle sweeps the turn, its extremes included
  {
    Stat s;
    const double sigma = 67108864.0;
    int64_t v0, v1;
    for (uint32_t low = 0; low < 2048; low += 2047) {   // both ends of the words that give u0 = 2^-53
      for (uint64_t j = 0; j <= 4096; ++j) {
        const uint64_t ang = j == 4096 ? ~0ull : j << 52;
        gauss_pair_f64(0, low, (uint32_t)(ang >> 32), (uint32_t)ang, sigma, v0, v1);
        s.take(v0), s.take(v1);
      }
    }
    for (uint64_t j = 0; j < sweep; ++j) {
      const uint64_t a = splitmix(seed), b = splitmix(seed);
      gauss_pair_f64((j & 1) ? 0 : (uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32), sigma, v0, v1);
      s.take(v0), s.take(v1);
    }
    s.print("gauss_f64_sigma_2p26");
  }

  // Box-Muller, single precision, the largest sigma below 2^19: X = 0 (taken as 1) and X = 1 give the largest radius
  {
    Stat s;
    const float sigf = 524287.96875f;   // 2^19 - 2^-5, the float below 2^19
    int64_t v0, v1;
    for (uint32_t x = 0; x < 2; ++x) {
      for (uint64_t j = 0; j <= 4096; ++j) {
        const uint32_t w2 = j == 4096 ? kAll : (uint32_t)(j << 20);
        gauss_pair_f32(0, x, w2, sigf, v0, v1);
        s.take(v0), s.take(v1);
      }
    }
    for (uint64_t j = 0; j < sweep; ++j) {
      const uint64_t a = splitmix(seed), b = splitmix(seed);
      gauss_pair_f32((j & 1) ? 0 : (uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, sigf, v0, v1);
      s.take(v0), s.take(v1);
    }
    s.print("gauss_f32_sigma_below_2p19");
  }

  // the exact discrete Gaussian at sigma = 2^26: every candidate is z = k x + y with x <= 7 and y < k, so |v| <= 8 k - 1
  // whatever the words are; the sweep runs the trial itself
  {
    const DgaussParams P = dgauss_params(kDgaussSigmaMax);
    Stat bound;
    bound.take((int64_t)(8ull * P.k - 1));
    bound.take(-(int64_t)(8ull * P.k - 1));
    bound.print("dgauss_tail_bound_sigma_2p26");
    Stat s;
    int64_t v;
    (void)dgauss_trial(P, kAll, kAll, kAll, 1u, 0, 0, v);   // x = 7, the largest y, negative: the extreme candidate
    s.take(v);
    (void)dgauss_trial(P, kAll, kAll, kAll, 0u, 0, 0, v);
    s.take(v);
    for (uint64_t j = 0; j < sweep; ++j) {
      const uint64_t a = splitmix(seed), b = splitmix(seed), c = splitmix(seed);
      (void)dgauss_trial(P, (uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32), (uint32_t)c, (uint32_t)(c >> 32), v);
      s.take(v);   // accepted or not: a rejected candidate is never stored, an accepted one is one of these
    }
    s.print("dgauss_trial_sigma_2p26");
  }
  return 0;
}
