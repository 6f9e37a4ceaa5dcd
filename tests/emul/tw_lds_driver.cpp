// CPU statement of the phase-2 twiddle image of the N = 1024 unit kernels (Tw2Img, ring_zk_amd/csrc/rzk_core.h; TEST
// INFRASTRUCTURE — not part of the product), through the very functions the kernels compile:
//   * the image of every prime and direction is built word by word as the kernels' fill loop builds it (thread t of the
//     256 copies table entry Tw2Img::src(t)), each image in an allocation of its own, so that a
//     read past its 256 words is an error under AddressSanitizer;
//   * every index phase 2 forms, 2^(LE+sp) + (hi << sp) + k, lies in [16, 256) — the condition under which the image is
//     enough — and the image word that (sp, hi, k) reads holds exactly that entry; every entry of [16, 256) is held once;
//   * all 64 lanes of the forward and the inverse transform at LOGN = 10 are replayed phase by phase, phase 2 reading
//     the image, and compared word for word with the run that reads the global table: three primes, seeded random
//     polynomials over the whole lazy range, and the all-maximum polynomial.
// Stand-alone: builds with g++ alone (also under -fsanitize=address,undefined), takes no input, prints one line per group
// of cases and exits non-zero when any case fails.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../ring_zk_amd/csrc/rzk_tables.h"

using namespace rzk;

namespace {

constexpr int LOGN = 10;
using G = Geo<LOGN>;
using I = Tw2Img<LOGN>;
static_assert(I::kFits && I::FIRST == 16 && I::END == 256 && I::WORDS == 256 && I::TABLES == 6, "the layout this driver states");

int failures = 0;
void report(const char* name, uint64_t cases, uint64_t bad) {
  std::printf("%s %s: %llu cases\n", bad ? "FAIL" : "ok  ", name, (unsigned long long)cases);
  if (bad) ++failures;
}

uint64_t rng_state = 0x243F6A8885A308D3ull;
uint64_t rnd64() {   // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the global tables as rzk_ctx_create uploads them: [prime][forward, inverse][kTableLen]
std::vector<uint32_t> global_tables() {
  std::vector<uint32_t> all((size_t)2 * kMaxPrimes * kTableLen);
  for (int i = 0; i < kMaxPrimes; ++i) {
    std::vector<uint32_t> f, v;
    host::make_twiddles(i, f, v);
    std::memcpy(&all[(size_t)(2 * i) * kTableLen], f.data(), sizeof(uint32_t) * kTableLen);
    std::memcpy(&all[(size_t)(2 * i + 1) * kTableLen], v.data(), sizeof(uint32_t) * kTableLen);
  }
  return all;
}

// unit_kernel's fill loop: 256 threads, one word per thread and table
std::vector<std::vector<uint32_t>> fill_images(const std::vector<uint32_t>& tw_all) {
  std::vector<std::vector<uint32_t>> img(I::TABLES, std::vector<uint32_t>(I::WORDS, 0xdeadbeefu));
  for (int thread = 0; thread < 256; ++thread) {
    const int src = I::src(thread);
    for (int t = 0; t < I::TABLES; ++t) img[t][thread] = tw_all[(size_t)t * kTableLen + src];
  }
  return img;
}

void check_indices(const std::vector<uint32_t>& tw_all, const std::vector<std::vector<uint32_t>>& img) {
  uint64_t cases = 0, bad = 0;
  int held[I::END] = {0};
  int pads = 0;
  for (int w = 0; w < I::WORDS; ++w) {
    const int s = I::src(w);
    if (s == 0) ++pads;   // a pad copies entry 0, outside the range and never read
    else if (s < I::FIRST || s >= I::END) ++bad;
    else ++held[s];
  }
  for (int e = I::FIRST; e < I::END; ++e) bad += held[e] != 1;
  bad += pads != I::WORDS - (I::END - I::FIRST);
  report("image holds entries 16..255 once each, 16 pads", I::WORDS, bad);

  bad = 0;
  for (int lane = 0; lane < 64; ++lane) {
    const int hi = G::p2_hi(lane);
    uint32_t w[16];
    for (int t = 0; t < I::TABLES; ++t) {
      I::load(w, img[t].data(), hi);
      for (int sp = 0; sp < G::LE; ++sp)
        for (int k = 0; k < (1 << sp); ++k) {
          const int idx = (1 << (G::LE + sp)) + (hi << sp) + k;   // what fwd_phase2 / inv_phase2 index the global table with
          const int slot = I::slot(sp, k);
          const int word = I::base(hi) + 64 * (slot >> 2) + (slot & 3);
          ++cases;
          if (idx < I::FIRST || idx >= I::END || slot < 0 || slot > 15 || word >= I::WORDS || I::src(word) != idx ||
              w[slot] != tw_all[(size_t)t * kTableLen + idx])
            ++bad;
        }
    }
  }
  report("phase-2 indices inside [16, 256) and served by the image", cases, bad);
}

struct Wave {
  uint32_t x[64][G::E];
  uint32_t lds[G::LDS_WORDS];
  template <bool IMG>
  void forward(const uint32_t* tw, const uint32_t* tw2, const PrimeConsts& pc) {
    for (int l = 0; l < 64; ++l) { fwd_phase1<LOGN>(x[l], tw, pc); lds_put_p1<LOGN>(x[l], l, lds); }
    for (int l = 0; l < 64; ++l) { lds_get_p2<LOGN>(x[l], l, lds); fwd_phase2<LOGN, 6, IMG>(x[l], l, tw2, pc); }
    for (int l = 0; l < 64; ++l) lds_put_p2<LOGN>(x[l], l, lds);
    for (int l = 0; l < 64; ++l) { lds_get_p3<LOGN>(x[l], l, lds); fwd_phase3<LOGN>(x[l], l, tw, pc); }
  }
  template <bool IMG>
  void inverse(const uint32_t* tw, const uint32_t* tw2, const PrimeConsts& pc) {
    for (int l = 0; l < 64; ++l) { inv_phase3<LOGN>(x[l], l, tw, pc); lds_put_p3<LOGN>(x[l], l, lds); }
    for (int l = 0; l < 64; ++l) { lds_get_p2<LOGN>(x[l], l, lds); inv_phase2<LOGN, 6, IMG>(x[l], l, tw2, pc); }
    for (int l = 0; l < 64; ++l) lds_put_p2<LOGN>(x[l], l, lds);
    for (int l = 0; l < 64; ++l) { lds_get_p1<LOGN>(x[l], l, lds); inv_phase1<LOGN>(x[l], tw, pc); }
  }
};

void check_transforms(const std::vector<uint32_t>& tw_all, const std::vector<std::vector<uint32_t>>& img) {
  static Wave a, b;
  constexpr int kPolys = 5;   // four random ones and the all-maximum one
  for (int pi = 0; pi < kMaxPrimes; ++pi) {
    const PrimeConsts pc = host::make_prime_consts(pi, G::N);
    const uint32_t* twf = &tw_all[(size_t)(2 * pi) * kTableLen];
    const uint32_t* twi = &tw_all[(size_t)(2 * pi + 1) * kTableLen];
    uint64_t bad_f = 0, bad_i = 0, same = 0;
    for (int poly = 0; poly < kPolys; ++poly) {
      for (int dir = 0; dir < 2; ++dir) {
        const uint32_t range = dir == 0 ? 4u * pc.p : 2u * pc.p;   // lazy ranges of the forward / inverse inputs (4p < 2^32)
        for (int l = 0; l < 64; ++l)
          for (int e = 0; e < G::E; ++e) a.x[l][e] = b.x[l][e] = poly == kPolys - 1 ? range - 1u : (uint32_t)(rnd64() % range);
        if (dir == 0) {
          a.forward<false>(twf, twf, pc);
          b.forward<true>(twf, img[2 * pi].data(), pc);
        } else {
          a.inverse<false>(twi, twi, pc);
          b.inverse<true>(twi, img[2 * pi + 1].data(), pc);
        }
        for (int l = 0; l < 64; ++l)
          for (int e = 0; e < G::E; ++e) (dir == 0 ? bad_f : bad_i) += a.x[l][e] != b.x[l][e];
      }
      // the two directions still invert each other through the image (guards against comparing two equal mistakes)
      for (int l = 0; l < 64; ++l)
        for (int e = 0; e < G::E; ++e) a.x[l][e] = b.x[l][e] = (uint32_t)(rnd64() % pc.p);
      b.forward<true>(twf, img[2 * pi].data(), pc);
      uint32_t std_order[G::N];
      for (int l = 0; l < 64; ++l)
        for (int c = 0; c < G::E; ++c) std_order[G::j_p3(l, c)] = csub(csub(b.x[l][c], pc.twop), pc.p);
      for (int l = 0; l < 64; ++l)
        for (int c = 0; c < G::E; ++c) b.x[l][c] = std_order[G::j_p3(l, c)];
      b.inverse<true>(twi, img[2 * pi + 1].data(), pc);
      for (int l = 0; l < 64; ++l)
        for (int e = 0; e < G::E; ++e) same += csub(mont_lazy(b.x[l][e], pc.ninv_r, pc.p, pc.npinv), pc.p) != a.x[l][e];
    }
    char name[96];
    std::snprintf(name, sizeof name, "prime %d forward, image against global table", pi);
    report(name, (uint64_t)kPolys * G::N, bad_f);
    std::snprintf(name, sizeof name, "prime %d inverse, image against global table", pi);
    report(name, (uint64_t)kPolys * G::N, bad_i);
    std::snprintf(name, sizeof name, "prime %d inverse(forward(x)) == x through the image", pi);
    report(name, (uint64_t)kPolys * G::N, same);
  }
}

}  // namespace

int main() {
  const std::vector<uint32_t> tw_all = global_tables();
  const std::vector<std::vector<uint32_t>> img = fill_images(tw_all);
  check_indices(tw_all, img);
  check_transforms(tw_all, img);
  if (failures) {
    std::printf("%d groups failed\n", failures);
    return 1;
  }
  std::printf("all cases passed\n");
  return 0;
}
