// CPU statement of every lane-level helper that depends on the ring modulus q (ring_zk_amd/csrc/rzk_core.h; TEST
// INFRASTRUCTURE — not part of the product), through the very functions the kernels compile, against 128-bit arithmetic,
// at the edges of the supported modulus range (include/rzk.h: q odd, p0 < q <= 4 p2 - 1):
//   addq, subq, montq_u, montq + center_rounds, zq_from_centered, center_from_zq
//   zq_from_i64            the rotation sums' reduction (its low word is below 5q, not 4q, when q < 2^30: 4q < 2^32 there)
//   crt_center, crt_fold0/1/2 + crt_finish, crt1_zq, crt2_zq, crt2_zq_short     for np = 1, 2, 3
//   lift                   the one-add lift x + 2p into the lazy range [0, 4p) of every auxiliary prime
//   the canonical test     (uint64)(c + h) <= 2h and its 32-bit form, as rzk_slab32.h states them for the host
//                          (the kernels' canon_lo_mx / canon_fail are device code: a wavefront vote over the same compare)
// Stand-alone: builds with g++ alone (also under -fsanitize=address,undefined), takes no input, prints one line per group
// of cases and exits non-zero when any case fails.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../ring_zk_amd/csrc/rzk_slab32.h"
#include "../../ring_zk_amd/csrc/rzk_tables.h"

using namespace rzk;

namespace {

typedef unsigned __int128 u128;
typedef __int128 i128;
int failures = 0;

uint64_t rng_state = 0x243F6A8885A308D3ull;
uint64_t rnd64() {   // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
uint32_t below(uint32_t n) { return (uint32_t)(rnd64() % n); }

struct Group {   // one printed line: "ok   <name> q=<q>: <cases> cases"
  const char* name;
  uint64_t q, cases = 0, bad = 0;
  Group(const char* n, uint64_t q_) : name(n), q(q_) {}
  void check(bool ok, i128 at) {
    ++cases;
    if (ok) return;
    if (bad < 4) {
      const bool neg = at < 0;
      const u128 m = neg ? (u128)(-at) : (u128)at;
      std::printf("     %s q=%llu: mismatch at %s0x%llx%016llx\n", name, (unsigned long long)q, neg ? "-" : "",
                  (unsigned long long)(uint64_t)(m >> 64), (unsigned long long)(uint64_t)m);
    }
    ++bad;
  }
  ~Group() {
    std::printf("%s %s q=%llu: %llu cases\n", bad ? "FAIL" : "ok  ", name, (unsigned long long)q, (unsigned long long)cases);
    if (bad) ++failures;
  }
};

uint32_t mod_q(i128 a, uint64_t q) {   // a mod q in [0, q)
  i128 r = a % (i128)q;
  if (r < 0) r += (i128)q;
  return (uint32_t)r;
}
int64_t centred(i128 a, uint64_t q) {   // the representative in [-(q-1)/2, (q-1)/2]
  const int64_t r = mod_q(a, q), h = (int64_t)((q - 1) / 2);
  return r > h ? r - (int64_t)q : r;
}

struct Ctx {
  uint64_t q;
  uint32_t h;
  PrimeConsts pc[kMaxPrimes];
  CrtConsts C;
};

// ---- 32-bit arithmetic mod q ------------------------------------------------------------------------------------------
void arith_cases(const Ctx& t) {
  const uint64_t q = t.q;
  const uint32_t qq = (uint32_t)q, h = t.h;
  std::vector<uint32_t> res = {0u, 1u, 2u, h - 1u, h, h + 1u, qq - 2u, qq - 1u};   // residues in [0, q)
  for (uint32_t v : {0x3fffffffu, 0x40000000u, 0x7fffffffu, 0x80000000u, 0x80000001u, 0xc0000000u})
    if (v < qq) res.push_back(v), res.push_back(qq - 1u - v);
  for (int i = 0; i < 200; ++i) res.push_back(below(qq));
  std::vector<uint32_t> words = {0u, 1u, qq - 1u, qq, qq + 1u, 0x7fffffffu, 0x80000000u, 0xfffffffeu, 0xffffffffu};   // any 32-bit word
  for (int i = 0; i < 200; ++i) words.push_back((uint32_t)rnd64());
  {
    Group g("addq / subq", q);
    for (uint32_t a : res)
      for (uint32_t b : res) {
        g.check(addq(a, b, qq) == mod_q((i128)a + b, q), ((i128)a << 32) | b);
        g.check(subq(a, b, qq) == mod_q((i128)a - b, q), ((i128)a << 32) | b);
      }
  }
  {
    Group g("montq_u / montq: a c 2^-32 mod q", q);
    for (uint32_t a : words)
      for (uint32_t c : res) {
        const uint32_t want = mod_q((i128)a * c, q);
        const uint32_t u = montq_u(a, c, t.C);
        g.check(u < q && mod_q((i128)u << 32, q) == want, ((i128)a << 32) | c);
        const int64_t s = montq(a, c, t.C);
        g.check(s > -(int64_t)q && s < (int64_t)q && mod_q((i128)s * ((i128)1 << 32), q) == want, ((i128)a << 32) | c);
      }
  }
  {
    Group g("center_rounds<3>: |s| < 3q", q);
    const int64_t Q = (int64_t)q;
    std::vector<int64_t> ss;
    for (int64_t k = -3; k <= 3; ++k)
      for (int64_t e : {(int64_t)-h - 1, (int64_t)-h, (int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)h, (int64_t)h + 1}) {
        const int64_t s = k * Q + e;
        if (s > -3 * Q && s < 3 * Q) ss.push_back(s);
      }
    for (int i = 0; i < 100000; ++i) ss.push_back((int64_t)(rnd64() % (uint64_t)(6 * Q - 1)) - (3 * Q - 1));
    for (int64_t s : ss) g.check(center_rounds<3>(s, t.C) == centred(s, q), s);
  }
  {
    Group g("zq_from_centered / center_from_zq", q);
    std::vector<int64_t> xs = {-(int64_t)h, -(int64_t)h + 1, -1, 0, 1, (int64_t)h - 1, (int64_t)h};
    for (int i = 0; i < 100000; ++i) xs.push_back((int64_t)(rnd64() % q) - (int64_t)h);
    for (int64_t x : xs) {
      const uint32_t u = zq_from_centered((int32_t)x, (uint32_t)q);
      g.check((int64_t)(int32_t)x == x && u == mod_q(x, q) && center_from_zq(u, t.C) == x, x);
    }
  }
}

// ---- zq_from_i64 --------------------------------------------------------------------------------------------------------
// Contract: |a| < 2^62 and |a| < q 2^32; the callers keep |a| < 4.0e18 (the pass split of shift_product).
constexpr int64_t kPassEdge = 4000000000000000000ll;
void i64_cases(const Ctx& t) {
  const uint64_t q = t.q;
  auto ok = [&](int64_t a) { return zq_from_i64(a, t.C) == mod_q(a, q); };
  {
    Group g("zq_from_i64: every a in [-2^20, 2^20]", q);
    for (int64_t a = -(1 << 20); a <= (1 << 20); ++a) g.check(ok(a), a);
  }
  {
    // low words past the last multiple of q below 2^32 (for 4q < 2^32: everything from 4q - 8 on), next to every multiple
    // of q, and the top of the word; under high words 0, +-1 and the passes' edge on both sides
    Group g("zq_from_i64: low-word edges under several high words", q);
    std::vector<uint32_t> los;
    const uint64_t top = (((uint64_t)1 << 32) / q) * q;   // largest multiple of q that fits the word
    for (uint64_t lo = top - 8; lo < ((uint64_t)1 << 32); ++lo) {
      los.push_back((uint32_t)lo);
      if (los.size() >= 400000) break;   // (q just above 2^30 or 2^31 leaves almost a whole q of them: the first 400000 ...)
    }
    for (uint64_t lo = ((uint64_t)1 << 32) - 4096; lo < ((uint64_t)1 << 32); ++lo) los.push_back((uint32_t)lo);   // (... and the last)
    for (uint64_t k = 0; k * q < ((uint64_t)1 << 32); ++k)
      for (int64_t e = -2; e <= 2; ++e) {
        const int64_t lo = (int64_t)(k * q) + e;
        if (lo >= 0 && lo < ((int64_t)1 << 32)) los.push_back((uint32_t)lo);
      }
    const int64_t his[] = {0, 1, -1, -2, kPassEdge >> 32, (-kPassEdge) >> 32, (kPassEdge >> 32) - 1, ((-kPassEdge) >> 32) + 1};
    for (int64_t hi : his)
      for (uint32_t lo : los) {
        const int64_t a = hi * ((int64_t)1 << 32) + (int64_t)lo;
        g.check(ok(a), a);
      }
  }
  {
    Group g("zq_from_i64: |a| just below 4.0e18", q);
    for (int64_t k = 1; k <= 4096; ++k) {
      g.check(ok(kPassEdge - k), kPassEdge - k);
      g.check(ok(k - kPassEdge), k - kPassEdge);
    }
  }
  {
    Group g("zq_from_i64: seeded random |a| < 4.0e18", q);
    for (int i = 0; i < 1000000; ++i) {
      const int64_t a = (int64_t)(rnd64() % (uint64_t)(2 * kPassEdge - 1)) - (kPassEdge - 1);
      g.check(ok(a), a);
    }
  }
  if (q > ((uint64_t)1 << 30)) {   // |a| < 2^62 <= q 2^32
    Group g("zq_from_i64: seeded random |a| < 2^62", q);
    for (int i = 0; i < 1000000; ++i) {
      const int64_t a = (int64_t)(rnd64() >> 1) >> 1;   // 62 bits and a sign
      const int64_t b = (rnd64() & 1) ? a : -a;
      g.check(ok(b), b);
    }
  }
}

// ---- CRT reconstruction -----------------------------------------------------------------------------------------------
void crt_one(const Ctx& t, int np, i128 X, Group& g, Group& g2) {
  const int64_t want = centred(X, t.q);
  uint32_t rc[kMaxPrimes] = {0, 0, 0};
  for (int i = 0; i < np; ++i) {
    i128 r = X % (i128)t.pc[i].p;
    if (r < 0) r += t.pc[i].p;
    rc[i] = (uint32_t)r;
  }
  bool ok = true, ok2 = true;
  for (int rep = 0; rep < (1 << np); ++rep) {   // every mix of the two lazy representatives [0, p) and [p, 2p)
    uint32_t r[kMaxPrimes];
    for (int i = 0; i < kMaxPrimes; ++i) r[i] = rc[i] + ((rep >> i) & 1 ? t.pc[i].p : 0u);
    ok = ok && crt_center(r[0], r[1], r[2], np, t.pc, t.C) == want;
    uint32_t stA = crt_fold0(r[0], np, t.pc, t.C), stB = 0;
    if (np >= 2) crt_fold1(r[1], np, t.pc, t.C, stA, stB);
    if (np >= 3) crt_fold2(r[2], t.pc, t.C, stA, stB);
    const uint32_t z = crt_finish_zq(stA, np, t.C);
    ok = ok && z < t.q && z == mod_q(X, t.q) && crt_finish(stA, np, t.C) == want;
    if (np == 1) {
      const uint32_t u = crt1_zq(r[0], t.pc, t.C);
      ok = ok && u < t.q && center_from_zq(u, t.C) == want;
    }
    if (np == 2) {
      const uint32_t d0 = crt2_digit0(r[0], t.pc);
      const uint32_t a = crt2_zq(r[1], d0, t.pc, t.C), b = crt2_zq_short(r[1], d0, t.pc, t.C);
      ok2 = ok2 && a == b && a < t.q && a == mod_q(X, t.q);
    }
  }
  g.check(ok, X);
  if (np == 2) g2.check(ok2, X);
}

void crt_cases(const Ctx& t) {
  for (int np = 1; np <= kMaxPrimes; ++np) {
    u128 P = 1;
    for (int i = 0; i < np; ++i) P *= kPrimes[i];
    const i128 H = (i128)((P - 1) / 2);
    char n1[96], n2[96];
    std::snprintf(n1, sizeof n1, "crt np=%d: crt_center, fold chain%s", np, np == 1 ? ", crt1_zq" : "");
    std::snprintf(n2, sizeof n2, "crt np=%d: crt2_zq == crt2_zq_short", np);
    Group g(n1, t.q), g2(n2, t.q);
    const i128 edges[] = {0, 1, -1, H, -H, H - 1, -H + 1, (i128)t.h, -(i128)t.h, (i128)t.q, -(i128)t.q};
    for (i128 X : edges)
      if (X <= H && X >= -H) crt_one(t, np, X, g, g2);
    for (int i = 0; i < 100000; ++i) {
      const u128 w = ((u128)rnd64() << 64) | rnd64();
      crt_one(t, np, (i128)(w % (u128)(2 * H + 1)) - H, g, g2);
    }
    if (np != 2) g2.check(true, 0);   // (keeps the line's format; the pair exists for np = 2 only)
  }
}

// ---- lift and the canonical test ------------------------------------------------------------------------------------------
void lift_cases(const Ctx& t) {
  const int64_t h = t.h;
  {
    Group g("lift: x + 2p in [0, 4p) and = x mod p", t.q);
    const int64_t xs[] = {-h, -h + 1, -1, 0, 1, h - 1, h};
    for (int pi = 0; pi < kMaxPrimes; ++pi)
      for (int64_t x : xs) {
        const int64_t p = t.pc[pi].p, exact = x + 2 * p;
        const uint32_t got = lift((int32_t)x, t.pc[pi]);
        g.check((int64_t)(int32_t)x == x && exact >= 0 && exact < 4 * p && exact < ((int64_t)1 << 32) && (int64_t)got == exact &&
                    (int64_t)(got % (uint32_t)p) == (int64_t)mod_q(x, (uint64_t)p),
                x);
      }
  }
  {
    Group g("canonical test: +-h pass; +-(h+1), +-(h + 2^32) fail", t.q);
    const uint32_t hh = t.h;
    const int64_t two32 = (int64_t)1 << 32;
    for (int64_t c : {h, -h, (int64_t)0, h - 1, -h + 1}) {
      g.check(slab64_canonical(c, hh), c);
      g.check(slab32_canonical((int32_t)c, hh) && slab32_test_word((int32_t)c, hh) <= 2u * hh, c);
    }
    for (int64_t c : {h + 1, -h - 1, h + two32, -h - two32, two32, -two32, h - two32, (int64_t)t.q, (int64_t)1 << 62})
      g.check(!slab64_canonical(c, hh), c);
    // h + 1 and -h - 1 fit an int32 for every supported modulus (h <= 2^31 - 180223) and are refused there as well
    g.check(h + 1 <= INT32_MAX && !slab32_canonical((int32_t)(h + 1), hh), h + 1);
    g.check(!slab32_canonical((int32_t)(-h - 1), hh), -h - 1);
    g.check(!slab32_canonical(INT32_MAX, hh) && !slab32_canonical(INT32_MIN, hh), INT32_MAX);
  }
}

void modulus(uint64_t q) {
  Ctx t;
  t.q = q;
  t.h = (uint32_t)((q - 1) / 2);
  for (int i = 0; i < kMaxPrimes; ++i) t.pc[i] = host::make_prime_consts(i, 1024);
  {
    Group g("constants accepted", q);
    const bool ok = host::make_crt_consts(q, t.C);
    g.check(ok && t.C.q == q && t.C.qhalf == t.h && (uint32_t)(t.C.q * t.C.qinv) == 1u, (i128)q);
    if (!ok) return;
  }
  arith_cases(t);
  i64_cases(t);
  crt_cases(t);
  lift_cases(t);
}

}  // namespace

int main() {
  const uint64_t p0 = kPrimes[0], p2 = kPrimes[kMaxPrimes - 1];
  // the modulus set of tests/test_emul_modq.py (MODULI): Q_MIN, Q_B30, Q_A30, Q_A31, Q_DEF, Q_MAX
  const uint64_t qs[] = {p0 + 2, (1ull << 30) - 1, 1073741827ull, (1ull << 31) + 1, 3515337053ull, 4 * p2 - 1};
  for (uint64_t q : qs) modulus(q);
  {
    // the range itself: one step outside on either side, and an even modulus, are refused
    Group g("constants refused outside (p0, 4 p2 - 1] and for even q", 0);
    CrtConsts C;
    const uint64_t outside[] = {p0, p0 - 2, p0 + 1, 4 * p2 + 1, 4 * p2, ((uint64_t)1 << 32) + 1, 2, 1};
    for (uint64_t q : outside)
      g.check(!host::make_crt_consts(q, C), (i128)q);
  }
  if (failures) {
    std::printf("%d group(s) failed\n", failures);
    return 1;
  }
  std::printf("all cases passed\n");
  return 0;
}
