// CPU driver of tests/test_prove_loop_host.py (g++ -fsanitize=address,undefined): the arithmetic of the in-library prover loop
// that can be wrong (ring_zk_amd/csrc/rzk_prove_loop.h).
//   compaction   compact_emulate — the kernel lane by lane — against a plain loop for every batch size and flag pattern the
//                tiles, wavefronts and lanes can disagree on; idx lives between guard words and past count it is untouched
//   nonces       nonce_add across every byte carry and at the wrap of 128 bits, printed for the Python side to compare
//   coins        prove_coin at the extremes of the two draws, printed likewise
// Prints "compact <cases> <failures>", then "nonce <hex nonce0> <inc> <hex sum> <ok>" and "coin <a> <b> <coin>" lines.
//   usage: prove_loop_driver <seed>
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

constexpr uint32_t kGuard = 0xdeadbeefu;
constexpr size_t kPad = 8;

// one case: returns true when the emulation equals the plain loop and wrote nothing else
bool check(const std::vector<uint8_t>& live, const std::vector<uint8_t>& done) {
  const size_t B = live.size();
  std::vector<uint32_t> want;
  for (size_t b = 0; b < B; ++b)
    if (live[b] != 0 && done[b] == 0) want.push_back((uint32_t)b);
  std::vector<uint32_t> buf(kPad + B + kPad, kGuard);
  uint32_t count = kGuard;
  compact_emulate(live.data(), done.data(), B, buf.data() + kPad, &count);
  if (count != want.size()) return false;
  for (size_t i = 0; i < kPad; ++i)
    if (buf[i] != kGuard || buf[kPad + B + i] != kGuard) return false;
  for (size_t i = 0; i < B; ++i)
    if (buf[kPad + i] != (i < want.size() ? want[i] : kGuard)) return false;   // past count: untouched
  return true;
}

void print_hex(const uint8_t* p) {
  for (int i = 0; i < 16; ++i) printf("%02x", p[i]);
}

void nonce_case(const uint8_t* n0, uint64_t inc) {
  uint8_t out[16];
  const bool ok = nonce_add(n0, inc, out);
  printf("nonce ");
  print_hex(n0);
  printf(" %" PRIu64 " ", inc);
  print_hex(out);
  printf(" %d\n", ok ? 1 : 0);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  uint64_t seed = strtoull(argv[1], nullptr, 10);

  // ---- compaction
  const size_t sizes[] = {1, 63, 64, 65, 1023, 1024, 1025, 4097};
  uint64_t cases = 0, failures = 0;
  for (const size_t B : sizes) {
    // patterns of the pending set: all clear, all set, alternating (both phases), first only, last only, random at three densities
    for (int pat = 0; pat < 9; ++pat) {
      std::vector<uint8_t> pend(B, 0);
      for (size_t b = 0; b < B; ++b) {
        switch (pat) {
          case 0: break;
          case 1: pend[b] = 1; break;
          case 2: pend[b] = (b & 1) == 0; break;
          case 3: pend[b] = (b & 1) == 1; break;
          case 4: pend[b] = b == 0; break;
          case 5: pend[b] = b == B - 1; break;
          case 6: pend[b] = (splitmix(seed) & 1) != 0; break;
          case 7: pend[b] = (splitmix(seed) & 15) == 0; break;
          case 8: pend[b] = (splitmix(seed) & 15) != 0; break;
        }
      }
      // three ways to say "not pending": done set under a live flag, live clear, live clear AND done set (a set entry the
      // live mask excludes); flag bytes other than 1 count as set
      for (int mask = 0; mask < 3; ++mask) {
        std::vector<uint8_t> live(B), done(B);
        for (size_t b = 0; b < B; ++b) {
          if (pend[b]) {
            live[b] = (b % 3 == 0) ? 0xff : 1;
            done[b] = 0;
          } else if (mask == 0) {
            live[b] = 1, done[b] = (b % 5 == 0) ? 0x80 : 1;
          } else if (mask == 1) {
            live[b] = 0, done[b] = 0;
          } else {
            live[b] = 0, done[b] = 1;
          }
        }
        ++cases;
        if (!check(live, done)) {
          ++failures;
          fprintf(stderr, "compact: B = %zu pattern %d mask %d differs\n", B, pat, mask);
        }
      }
    }
  }
  // no flags at all: count = 0 and nothing is written
  {
    std::vector<uint8_t> none;
    ++cases;
    if (!check(none, none)) ++failures;
  }
  printf("compact %" PRIu64 " %" PRIu64 "\n", cases, failures);

  // ---- nonces: a carry out of every byte (0xff.. in bytes 0 .. i, inc 1), a multi-byte increment, and the wrap rule
  for (int i = 0; i < 16; ++i) {
    uint8_t n0[16] = {};
    for (int j = 0; j <= i; ++j) n0[j] = 0xff;
    nonce_case(n0, 1);   // i == 15: 2^128 - 1 + 1 leaves 128 bits
    nonce_case(n0, 0);
  }
  {
    uint8_t n0[16];
    for (int j = 0; j < 16; ++j) n0[j] = (uint8_t)(0x10 * j + 7);
    nonce_case(n0, 766);                        // 1 + 3 * 255
    nonce_case(n0, 0xffffffffffffffffull);      // the increment's own eight bytes all carry
    uint8_t top[16];
    memset(top, 0xff, sizeof(top));
    top[0] = 0x00, top[1] = 0xfd;               // 2^128 - 768
    nonce_case(top, 766);
    nonce_case(top, 767);
    nonce_case(top, 768);                       // exactly 2^128: leaves 128 bits
    nonce_case(top, 769);
  }
  printf("span %" PRIu64 " %" PRIu64 "\n", prove_nonce_span(1), prove_nonce_span(255));

  // ---- coins at the extremes of the two draws
  const int64_t ext[] = {-kCoinHalf, -kCoinHalf + 1, -1, 0, 1, kCoinHalf - 1, kCoinHalf};
  for (const int64_t a : ext)
    for (const int64_t b : ext) printf("coin %" PRId64 " %" PRId64 " %" PRId64 "\n", a, b, prove_coin(a, b));
  printf("consts %" PRId64 " %" PRId64 " %" PRIu64 "\n", kCoinR0, kCoinHalf, kCoinR);
  return failures == 0 ? 0 : 1;
}
