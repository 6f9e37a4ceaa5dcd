// CPU driver of tests/test_prove_loop_fields_host.py (g++ -fsanitize=address,undefined): what the Linear and Sum prover loops
// add to ring_zk_amd/csrc/rzk_prove_loop.h.
//   fields    fields_gather_emulate / fields_scatter_emulate / fields_zero_emulate — the field-list kernels with loops in place
//             of workgroups and lanes, through the kernels' own field_offset — against plain byte copies, for 1 .. 6 fields,
//             entry sizes of V x k rows, index sets first / last / all / ascending subsets, accept all / none / alternating;
//             every destination lives between guard words and is compared whole, guards included
//   live      prove_live for every (ok_commit, wanted, ok_hash), printed for the Python side to compare
//   nonces    prove_nonce_span_lin_sum and nonce_add of it across every byte carry and at the 128-bit edge, printed likewise
//   quads     field_quads at the edges of its two guards, printed likewise
// Prints "fields <cases> <failures>", then "live", "span", "edge" and "quads" lines.
//   usage: fields_driver <seed>
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../ring_zk_amd/csrc/rzk_prove_loop.h"

using namespace rzk;

namespace {

uint64_t splitmix(uint64_t& s) {
  uint64_t z = (s += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

constexpr uint8_t kGuardByte = 0xa5;
constexpr size_t kPad = 64;   // guard bytes on either side (keeps the slab 16-byte aligned inside its buffer)

// a slab of `entries` entries of `bytes` bytes between guards; 16-byte aligned storage
struct Slab {
  std::vector<FieldQuad> store;
  size_t bytes_total;
  Slab(size_t entries, size_t bytes, uint64_t& seed, bool random) : store((2 * kPad + entries * bytes) / 16), bytes_total(entries * bytes) {
    uint8_t* p = (uint8_t*)store.data();
    memset(p, kGuardByte, store.size() * 16);
    if (random)
      for (size_t i = 0; i < bytes_total; ++i) p[kPad + i] = (uint8_t)splitmix(seed);
  }
  uint8_t* data() { return (uint8_t*)store.data() + kPad; }
  const uint8_t* whole() const { return (const uint8_t*)store.data(); }
  size_t whole_bytes() const { return store.size() * 16; }
};

bool same(const Slab& a, const Slab& b) { return a.whole_bytes() == b.whole_bytes() && memcmp(a.whole(), b.whole(), a.whole_bytes()) == 0; }

// rows of field f of a proof with V summands and k columns: the entry sizes of the Sum loop's slabs (zs: V k; z': k; ts-like,
// t'-like, gs, g)
uint32_t rows_of(uint32_t f, uint32_t V, uint32_t k) {
  const uint32_t r[kMaxFields] = {V * k, k, V * 2, 2, V, 1};
  return r[f];
}

struct Case {
  uint32_t nf, N, V, k;
  uint64_t B;
  std::vector<uint32_t> idx;     // ascending, no duplicates
  std::vector<uint8_t> accept;   // one per idx entry
};

// the three moves of one case; returns the number of moves that differ from the plain copies
int run_case(const Case& cs, uint64_t& seed) {
  int bad = 0;
  const uint32_t count = (uint32_t)cs.idx.size();
  uint32_t quads[kMaxFields];
  size_t bytes[kMaxFields];
  for (uint32_t f = 0; f < cs.nf; ++f) {
    if (!field_quads(rows_of(f, cs.V, cs.k), cs.N, 8, cs.B, &quads[f])) return 3;
    bytes[f] = (size_t)quads[f] * 16;
    if (bytes[f] != (size_t)rows_of(f, cs.V, cs.k) * cs.N * 8) return 3;
  }
  // ---- gather: caller's slab [B] -> sub-batch [count]
  {
    std::vector<Slab> src, dst, want;
    FieldList fl{};
    fl.n = cs.nf;
    for (uint32_t f = 0; f < cs.nf; ++f) {
      src.emplace_back(cs.B, bytes[f], seed, true);
      dst.emplace_back(count, bytes[f], seed, false);
      want.emplace_back(count, bytes[f], seed, false);
    }
    for (uint32_t f = 0; f < cs.nf; ++f) {
      fl.src[f] = src[f].data(), fl.dst[f] = dst[f].data(), fl.quads[f] = quads[f];
      for (uint32_t i = 0; i < count; ++i) memcpy(want[f].data() + (size_t)i * bytes[f], src[f].data() + (size_t)cs.idx[i] * bytes[f], bytes[f]);
    }
    fields_gather_emulate(fl, cs.idx.data(), count);
    bool ok = true;
    for (uint32_t f = 0; f < cs.nf; ++f) ok = ok && same(dst[f], want[f]);
    bad += !ok;
  }
  // ---- scatter: sub-batch [count] -> caller's slab [B], with rounds and done
  std::vector<uint8_t> done(cs.B + 2, kGuardByte), rounds(cs.B + 2, kGuardByte), done_want, rounds_want;
  for (uint64_t b = 0; b < cs.B; ++b) done[1 + b] = 0, rounds[1 + b] = 0;
  done_want = done, rounds_want = rounds;
  std::vector<Slab> out, out_want;
  {
    std::vector<Slab> src;
    FieldList fl{};
    fl.n = cs.nf;
    for (uint32_t f = 0; f < cs.nf; ++f) {
      src.emplace_back(count, bytes[f], seed, true);
      uint64_t s2 = seed;
      out.emplace_back(cs.B, bytes[f], seed, true);
      out_want.emplace_back(cs.B, bytes[f], s2, true);   // the same bytes
    }
    for (uint32_t f = 0; f < cs.nf; ++f) {
      fl.src[f] = src[f].data(), fl.dst[f] = out[f].data(), fl.quads[f] = quads[f];
      for (uint32_t i = 0; i < count; ++i)
        if (cs.accept[i]) memcpy(out_want[f].data() + (size_t)cs.idx[i] * bytes[f], src[f].data() + (size_t)i * bytes[f], bytes[f]);
    }
    for (uint32_t i = 0; i < count; ++i)
      if (cs.accept[i]) done_want[1 + cs.idx[i]] = 1, rounds_want[1 + cs.idx[i]] = 7;
    fields_scatter_emulate(fl, cs.accept.data(), cs.idx.data(), count, 7, rounds.data() + 1, done.data() + 1);
    bool ok = done == done_want && rounds == rounds_want;
    for (uint32_t f = 0; f < cs.nf; ++f) ok = ok && same(out[f], out_want[f]);
    bad += !ok;
  }
  // ---- zero: the caller's slabs of every proof that is not done, ok = done
  {
    FieldList fl{};
    fl.n = cs.nf;
    std::vector<uint8_t> okv(cs.B + 2, kGuardByte), ok_want(cs.B + 2, kGuardByte);
    for (uint32_t f = 0; f < cs.nf; ++f) {
      fl.dst[f] = out[f].data(), fl.quads[f] = quads[f];
      for (uint64_t b = 0; b < cs.B; ++b)
        if (!done[1 + b]) memset(out_want[f].data() + (size_t)b * bytes[f], 0, bytes[f]);
    }
    for (uint64_t b = 0; b < cs.B; ++b) ok_want[1 + b] = done[1 + b];
    fields_zero_emulate(fl, done.data() + 1, okv.data() + 1, cs.B);
    bool ok = okv == ok_want;
    for (uint32_t f = 0; f < cs.nf; ++f) ok = ok && same(out[f], out_want[f]);
    bad += !ok;
  }
  return bad;
}

void print_hex(const uint8_t* p) {
  for (int i = 0; i < 16; ++i) printf("%02x", p[i]);
}
void edge_case(const uint8_t* n0, uint32_t max_rounds) {
  uint8_t out[16];
  const bool ok = nonce_add(n0, prove_nonce_span_lin_sum(max_rounds), out);
  printf("edge ");
  print_hex(n0);
  printf(" %u ", max_rounds);
  print_hex(out);
  printf(" %d\n", ok ? 1 : 0);
}
void quads_case(uint64_t rows, uint32_t N, uint32_t coef, uint64_t B) {
  uint32_t q = 0;
  const bool ok = field_quads(rows, N, coef, B, &q);
  printf("quads %" PRIu64 " %u %u %" PRIu64 " %d %u\n", rows, N, coef, B, ok ? 1 : 0, ok ? q : 0u);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  uint64_t seed = strtoull(argv[1], nullptr, 10);

  // ---- the three moves
  uint64_t cases = 0, failures = 0;
  const uint32_t Ns[] = {4, 64, 1024}, Vs[] = {1, 2, 3}, ks[] = {3, 5};
  for (uint32_t nf = 1; nf <= kMaxFields; ++nf)
    for (const uint32_t N : Ns)
      for (const uint32_t V : Vs)
        for (const uint32_t k : ks) {
          const uint64_t B = N == 1024 ? 5 : 9;
          // index sets: first only, last only, all, two ascending random subsets; accept: all, none, alternating
          for (int set = 0; set < 5; ++set)
            for (int acc = 0; acc < 3; ++acc) {
              Case cs{nf, N, V, k, B, {}, {}};
              for (uint64_t b = 0; b < B; ++b) {
                const bool in = set == 0 ? b == 0 : set == 1 ? b == B - 1 : set == 2 ? true : (splitmix(seed) & 1) != 0;
                if (in) cs.idx.push_back((uint32_t)b);
              }
              for (size_t i = 0; i < cs.idx.size(); ++i) cs.accept.push_back(acc == 0 ? 1 : acc == 1 ? 0 : (uint8_t)((i & 1) ? 0x80 : 0));
              ++cases;
              const int bad = run_case(cs, seed);
              if (bad) {
                ++failures;
                fprintf(stderr, "fields: nf %u N %u V %u k %u set %d accept %d: %d moves differ\n", nf, N, V, k, set, acc, bad);
              }
            }
        }
  printf("fields %" PRIu64 " %" PRIu64 "\n", cases, failures);

  // ---- the live rule
  for (int okc = 0; okc < 4; ++okc)
    for (const int wanted : {1, 3})
      for (int okh = 0; okh < 2; ++okh) printf("live %d %d %d %d\n", okc, wanted, okh, (int)prove_live((uint8_t)okc, (uint8_t)wanted, (uint8_t)okh));
  printf("live 1 1 255 %d\n", (int)prove_live(1, 1, 0xff));   // any non-zero hash byte is a set flag

  // ---- the nonce span: its value, a carry out of every byte, the 128-bit edge
  printf("span %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", prove_nonce_span_lin_sum(1), prove_nonce_span_lin_sum(64), prove_nonce_span_lin_sum(255));
  for (int i = 0; i < 16; ++i) {
    uint8_t n0[16] = {};
    for (int j = 0; j <= i; ++j) n0[j] = 0xff;
    edge_case(n0, 1);     // + 6: carries out of bytes 0 .. i (i == 15: leaves 128 bits)
    edge_case(n0, 255);   // + 1022: a two-byte increment
  }
  {
    uint8_t top[16];
    memset(top, 0xff, sizeof(top));
    for (const uint32_t mr : {1u, 64u, 255u}) {
      const uint64_t span = prove_nonce_span_lin_sum(mr);
      for (int d = -1; d <= 1; ++d) {   // nonce0 = 2^128 - span + d: d < 0 fits, d >= 0 leaves 128 bits
        uint8_t n0[16];
        memcpy(n0, top, 16);            // 2^128 - 1
        const uint64_t sub = span - 1 - (uint64_t)d;   // (2^128 - 1) - sub = 2^128 - span + d; sub < 2^16
        n0[0] = (uint8_t)(0xff - (sub & 0xff)), n0[1] = (uint8_t)(0xff - (sub >> 8));
        edge_case(n0, mr);
      }
    }
  }

  // ---- the quad count and its two guards
  quads_case(15, 1024, 8, 5);                               // zs at V = 3, k = 5
  quads_case(3, 4, 8, 1);                                   // the smallest entry of the sweep
  quads_case(1, 2, 8, 1);                                   // one quad
  quads_case(1, 2, 4, 1);                                   // half a quad: refused
  quads_case(0, 1024, 8, 1);                                // an empty entry: refused
  quads_case(0xffffffffull * 2, 1, 8, 1);                   // 2^32 - 1 quads: the last count that fits
  quads_case(0x100000000ull * 2, 1, 8, 1);                  // 2^32 quads: refused
  quads_case((1ull << 20) * 32, 2048, 8, 1);                // V = 2^20, k = 32 at N = 2048: 2^35 quads, refused
  quads_case(0xffffffffull * 2, 1, 8, 0x7ffffffull);        // B quads 16 = (2^32 - 1)(2^27 - 1) 16 < 2^63: fits
  quads_case(0xffffffffull * 2, 1, 8, 0x8000001ull);        // ... past 2^63: refused
  quads_case(2, 1, 8, 0x7ffffffffffffffull);                // one quad, B = 2^59 - 1: the last batch that fits
  quads_case(2, 1, 8, 0x800000000000000ull);                // B = 2^59: refused
  return failures == 0 ? 0 : 1;
}
