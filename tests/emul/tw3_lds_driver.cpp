// CPU statement of the full vector-twiddle image of the N = 1024 unit kernels on sixteen-team workgroups (TwAllImg = Tw2Img +
// Tw3Img, ring_zk_amd/csrc/rzk_core.h; RZK_TW_LDS=2; TEST INFRASTRUCTURE — not part of the product), through the very
// functions the kernels compile:
//   * the image of every prime and direction is built word by word as the kernels' fill loop builds it (thread t of the
//     1024 copies table entry TwAllImg::src(t)), each image in an allocation of its own, so that a read past its 1024
//     words is an error under AddressSanitizer;
//   * every index phase 3 forms, 2^(2 LE + sq) + lane (E >> (R3 - sq)) + k, lies in [256, 1024) — the condition under
//     which the image is enough — and the image word that (sq, lane, k) reads holds exactly that entry; every entry of
//     [256, 1024) is held once, and the first 256 words are the phase-2 image unchanged;
//   * no two of sixteen consecutive lanes share a bank (64 banks of 4 bytes) in any of a lane's 16-byte reads, phase 2 and
//     phase 3, whatever 16-byte-aligned address the workgroup's images begin at;
//   * all 64 lanes of wave_fwd / wave_inv at LOGN = 10 are replayed phase by phase, phases 2 and 3 reading the image, and
//     compared word for word with the run that reads the global table: three primes, seeded random polynomials over the
//     whole lazy range, and the all-maximum polynomial.
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
using I2 = Tw2Img<LOGN>;
using I3 = Tw3Img<LOGN>;
using IA = TwAllImg<LOGN>;
static_assert(IA::kFits && I3::FIRST == 256 && I3::END == 1024 && I3::WORDS == 768 && IA::P3 == 256 && IA::WORDS == 1024 && IA::TABLES == 6,
              "the layout this driver states");
constexpr int kThreads = 1024;          // sixteen one-wavefront teams
constexpr int kTeams = 16;
static_assert(kThreads == IA::WORDS, "one image word per thread and table");
// bytes of LDS per workgroup as the launcher asks for them: the teams' slab + P, then the images
static_assert(kTeams * (G::LDS_WORDS + G::N) * 4 + IA::TABLES * IA::WORDS * 4 == 157696, "LDS per workgroup");

int failures = 0;
void report(const char* name, uint64_t cases, uint64_t bad) {
  std::printf("%s %s: %llu cases\n", bad ? "FAIL" : "ok  ", name, (unsigned long long)cases);
  if (bad) ++failures;
}

uint64_t rng_state = 0x13198A2E03707344ull;
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

// unit_kernel's fill loop: 1024 threads, one word per thread and table
std::vector<std::vector<uint32_t>> fill_images(const std::vector<uint32_t>& tw_all) {
  std::vector<std::vector<uint32_t>> img(IA::TABLES, std::vector<uint32_t>(IA::WORDS, 0xdeadbeefu));
  for (int thread = 0; thread < kThreads; ++thread) {
    const int src = IA::src(thread);
    for (int t = 0; t < IA::TABLES; ++t) img[t][thread] = tw_all[(size_t)t * kTableLen + src];
  }
  return img;
}

void check_indices(const std::vector<uint32_t>& tw_all, const std::vector<std::vector<uint32_t>>& img) {
  uint64_t cases = 0, bad = 0;
  int held[I3::END] = {0};
  for (int w = 0; w < IA::WORDS; ++w) {
    const int s = IA::src(w);
    if (w < IA::P3) {   // the phase-2 image as it was
      bad += s != I2::src(w);
      continue;
    }
    if (s < I3::FIRST || s >= I3::END) ++bad;
    else ++held[s];
  }
  for (int e = I3::FIRST; e < I3::END; ++e) bad += held[e] != 1;
  report("image holds the phase-2 image, then entries 256..1023 once each", IA::WORDS, bad);

  bad = 0;
  for (int lane = 0; lane < 64; ++lane) {
    uint32_t w[16];
    for (int t = 0; t < IA::TABLES; ++t) {
      I3::load(w, img[t].data() + IA::P3, lane);
      for (int sq = 0; sq < G::R3; ++sq) {
        const int sh = G::R3 - sq;
        for (int k = 0; k < (G::E >> sh); ++k) {
          const int idx = (1 << (2 * G::LE + sq)) + lane * (G::E >> sh) + k;   // what fwd_phase3 / inv_phase3 index the global table with
          const int slot = I3::slot(sq, k);
          const int word = I3::base(lane) + 256 * (slot >> 2) + (slot & 3);
          ++cases;
          if (idx < I3::FIRST || idx >= I3::END || slot < 0 || slot > 11 || word >= I3::WORDS || I3::src(word) != idx ||
              w[slot] != tw_all[(size_t)t * kTableLen + idx])
            ++bad;
        }
      }
    }
  }
  report("phase-3 indices inside [256, 1024) and served by the image", cases, bad);
}

// ds_read_b128: 64 banks of 4 bytes, sixteen consecutive lanes per pass.  A lane's read covers four consecutive banks from
// (byte address / 4) mod 64; sixteen lanes must cover the 64 banks once.
void check_banks() {
  uint64_t cases = 0, bad = 0;
  const int img0 = kTeams * (G::LDS_WORDS + G::N);   // word address of the first image in the workgroup's LDS
  for (int t = 0; t < IA::TABLES; ++t)
    for (int rd = 0; rd < 4 + 3; ++rd)               // four phase-2 reads, three phase-3 reads
      for (int grp = 0; grp < 4; ++grp) {
        int used[64] = {0};
        for (int l = 16 * grp; l < 16 * grp + 16; ++l) {
          const int word = rd < 4 ? img0 + t * IA::WORDS + I2::base(G::p2_hi(l)) + 64 * rd
                                  : img0 + t * IA::WORDS + IA::P3 + I3::base(l) + 256 * (rd - 4);
          bad += (word & 3) != 0;                    // 16-byte aligned
          for (int c = 0; c < 4; ++c) ++used[(word + c) & 63];
        }
        ++cases;
        for (int bk = 0; bk < 64; ++bk) bad += used[bk] != 1;
      }
  report("sixteen consecutive lanes cover the 64 banks once in every 16-byte read", cases, bad);
}

struct Wave {
  uint32_t x[64][G::E];
  uint32_t lds[G::LDS_WORDS];
  // the phases in wave_fwd's / wave_inv's order (rzk_wave.h); img = the table's TwAllImg, or null for the global table
  template <bool IMG>
  void forward(const uint32_t* tw, const uint32_t* img, const PrimeConsts& pc) {
    for (int l = 0; l < 64; ++l) { fwd_phase1<LOGN>(x[l], tw, pc); lds_put_p1<LOGN>(x[l], l, lds); }
    for (int l = 0; l < 64; ++l) { lds_get_p2<LOGN>(x[l], l, lds); fwd_phase2<LOGN, 6, IMG>(x[l], l, IMG ? img : tw, pc); }
    for (int l = 0; l < 64; ++l) lds_put_p2<LOGN>(x[l], l, lds);
    for (int l = 0; l < 64; ++l) { lds_get_p3<LOGN>(x[l], l, lds); fwd_phase3<LOGN, 6, IMG>(x[l], l, IMG ? img + IA::P3 : tw, pc); }
  }
  template <bool IMG>
  void inverse(const uint32_t* tw, const uint32_t* img, const PrimeConsts& pc) {
    for (int l = 0; l < 64; ++l) { inv_phase3<LOGN, 6, IMG>(x[l], l, IMG ? img + IA::P3 : tw, pc); lds_put_p3<LOGN>(x[l], l, lds); }
    for (int l = 0; l < 64; ++l) { lds_get_p2<LOGN>(x[l], l, lds); inv_phase2<LOGN, 6, IMG>(x[l], l, IMG ? img : tw, pc); }
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
          a.forward<false>(twf, nullptr, pc);
          b.forward<true>(twf, img[2 * pi].data(), pc);
        } else {
          a.inverse<false>(twi, nullptr, pc);
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
  check_banks();
  check_transforms(tw_all, img);
  if (failures) {
    std::printf("%d groups failed\n", failures);
    return 1;
  }
  std::printf("all cases passed\n");
  return 0;
}
