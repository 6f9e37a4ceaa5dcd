// CPU statement of the two shorter lane-level forms the unit kernels take (ring_zk_amd/csrc/rzk_core.h; TEST
// INFRASTRUCTURE — not part of the product), through the very functions the kernels compile:
//   crt2_zq_short   two-prime reconstruction with digit compares and one reduction mod q, against crt_center, the
//                   two-reduction form crt2_zq and an independent 128-bit computation;
//   dot2_lazy       x1 k1 + x2 k2 with one Montgomery reduction, against the two mont_lazy / mac_add / mac_sub steps it
//                   replaces and an independent 128-bit computation.
// Stand-alone: builds with g++ alone (also under -fsanitize=address,undefined), takes no input, prints one line per group
// of cases and exits non-zero when any case fails.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../ring_zk_amd/csrc/rzk_tables.h"

using namespace rzk;

namespace {

typedef unsigned __int128 u128;
int failures = 0;

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd64() {   // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
uint32_t below(uint32_t n) { return (uint32_t)(rnd64() % n); }

void report(const char* name, uint64_t cases, uint64_t bad) {
  std::printf("%s %s: %llu cases\n", bad ? "FAIL" : "ok  ", name, (unsigned long long)cases);
  if (bad) ++failures;
}

// ---- crt2_zq_short ------------------------------------------------------------------------------------------------
struct Crt2 {
  PrimeConsts pc[kMaxPrimes];
  CrtConsts C;
  uint64_t q;
  // one pair of digits, both lazy representatives of the prime-1 residue
  bool check(uint32_t d1, uint32_t d0) const {
    const uint64_t p0 = pc[0].p, p1 = pc[1].p;
    const uint64_t xp = (uint64_t)d1 * p0 + d0;                       // X' = X mod p0 p1
    const bool neg = xp >= C.half2;
    // independent: X = X' - [neg] P, reduced mod q and centred
    const u128 P = (u128)p0 * p1;
    const uint64_t mag = neg ? (uint64_t)(P - xp) : xp;               // |X|
    uint64_t want_zq = mag % q;
    if (neg && want_zq) want_zq = q - want_zq;
    const int64_t want = want_zq > C.qhalf ? (int64_t)want_zq - (int64_t)q : (int64_t)want_zq;
    const uint32_t r1c = (uint32_t)(xp % p1);
    bool ok = true;
    for (int rep = 0; rep < 2; ++rep) {
      const uint32_t r1 = r1c + (rep ? pc[1].p : 0u);                 // [0, 2 p1)
      const uint32_t got = crt2_zq_short(r1, d0, pc, C);
      ok = ok && got < q && got == want_zq;
      ok = ok && got == crt2_zq(r1, d0, pc, C);
      ok = ok && center_from_zq(got, C) == crt_center(d0, r1, 0u, 2, pc, C) && center_from_zq(got, C) == want;
      ok = ok && center_from_zq(got, C) == crt_center(d0 + pc[0].p, r1, 0u, 2, pc, C);   // (lazy first residue: the same digit)
    }
    return ok;
  }
};

void crt2_cases(uint64_t q, uint64_t nrandom) {
  Crt2 t;
  t.q = q;
  for (int i = 0; i < kMaxPrimes; ++i) t.pc[i] = host::make_prime_consts(i, 1024);
  char name[96];
  if (!host::make_crt_consts(q, t.C)) {
    std::snprintf(name, sizeof name, "crt2 q=%llu: constants", (unsigned long long)q);
    report(name, 1, 1);
    return;
  }
  const uint32_t p0 = t.pc[0].p, p1 = t.pc[1].p, h1 = t.C.half2_d1, h0 = t.C.half2_d0;
  uint64_t bad = (uint64_t)h1 * p0 + h0 != t.C.half2 || h0 >= p0 || h1 + 1 >= p1 || h0 == 0 || h1 == 0;
  std::snprintf(name, sizeof name, "crt2 q=%llu: (h1, h0) = divmod((P+1)/2, p0), both inside their ranges", (unsigned long long)q);
  report(name, 1, bad);
  const uint32_t d1s[] = {0u, 1u, h1 - 1u, h1, h1 + 1u, p1 - 1u};
  const uint32_t d0s[] = {0u, h0 - 1u, h0, h0 + 1u, p0 - 1u};
  bad = 0;
  uint64_t n = 0;
  for (uint32_t d1 : d1s)
    for (uint32_t d0 : d0s) {
      ++n;
      if (!t.check(d1, d0)) {
        ++bad;
        std::printf("     mismatch at d1=%u d0=%u\n", d1, d0);
      }
    }
  std::snprintf(name, sizeof name, "crt2 q=%llu: digit edges, both lazy residues", (unsigned long long)q);
  report(name, n, bad);
  bad = 0;
  for (uint64_t i = 0; i < nrandom; ++i) {
    // every fourth pair next to the sign boundary in its high digit, so that the low-digit compare decides
    const uint32_t d1 = (i & 3) == 3 ? h1 : below(p1);
    const uint32_t d0 = below(p0);
    if (!t.check(d1, d0)) {
      if (bad < 5) std::printf("     mismatch at d1=%u d0=%u\n", d1, d0);
      ++bad;
    }
  }
  std::snprintf(name, sizeof name, "crt2 q=%llu: seeded random pairs, both lazy residues", (unsigned long long)q);
  report(name, nrandom, bad);
}

// ---- dot2_lazy ------------------------------------------------------------------------------------------------------
void dot2_cases(int pi) {
  const PrimeConsts pc = host::make_prime_consts(pi, 1024);
  const uint32_t p = pc.p;
  std::vector<uint32_t> xs = {0u, 1u, 4u * p - 1u, 0xffffffffu};
  std::vector<uint32_t> ks = {0u, 1u, p - 1u};
  for (int i = 0; i < 12; ++i) xs.push_back((uint32_t)rnd64());
  for (int i = 0; i < 12; ++i) ks.push_back(below(p));
  uint64_t n = 0, bad = 0;
  for (uint32_t x1 : xs)
    for (uint32_t x2 : xs)
      for (uint32_t k1 : ks)
        for (uint32_t k2 : ks)
          for (int s = 0; s < 4; ++s) {
            const bool m1 = s & 1, m2 = s & 2;
            // the two steps it replaces: first product of a sum, then multiply-accumulate
            uint32_t ref = m1 ? mac_sub(0u, x1, k1, pc) : mont_lazy(x1, k1, pc.p, pc.npinv);
            ref = m2 ? mac_sub(ref, x2, k2, pc) : mac_add(ref, x2, k2, pc);
            const uint32_t got = dot2_lazy(x1, m1 ? p - k1 : k1, x2, m2 ? p - k2 : k2, pc);
            // independent: got * 2^32 = +-x1 k1 +- x2 k2 (mod p)
            const uint64_t t1 = (uint64_t)((u128)x1 * k1 % p), t2 = (uint64_t)((u128)x2 * k2 % p);
            const uint64_t want = ((m1 ? p - t1 : t1) + (m2 ? p - t2 : t2)) % p;
            const bool ok = got < 2u * p && ref < 2u * p && got % p == ref % p && (uint64_t)(((u128)got << 32) % p) == want;
            ++n;
            if (!ok) {
              if (bad < 5) std::printf("     mismatch at x1=%u k1=%u x2=%u k2=%u signs %d\n", x1, k1, x2, k2, s);
              ++bad;
            }
          }
  char name[96];
  std::snprintf(name, sizeof name, "dot2 p%d=%u: edges and random, both signs, in [0,2p) and equal mod p", pi, p);
  report(name, n, bad);
}

}  // namespace

int main() {
  crt2_cases(3515337053ull, 1000000);               // the ring modulus of the protocols
  crt2_cases((uint64_t)kPrimes[0] + 2, 100000);     // the smallest and the largest modulus make_crt_consts accepts
  crt2_cases(4ull * kPrimes[2] - 1, 100000);
  for (int pi = 0; pi < kMaxPrimes; ++pi) dot2_cases(pi);
  if (failures) {
    std::printf("%d group(s) failed\n", failures);
    return 1;
  }
  std::printf("all cases passed\n");
  return 0;
}
