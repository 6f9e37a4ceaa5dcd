// CPU statement of the packed-byte rotations of shift_row_kernel (ByteGeo in ring_zk_amd/csrc/rzk_core.h; TEST
// INFRASTRUCTURE — not part of the product).  Replays the 64 lanes of one wavefront through the very functions the
// kernel calls — condition, byte-image build, window fetch, realign, add, park, take — with the LDS image as a plain
// array, and compares with the schoolbook negacyclic product.  Stand-alone: builds with g++ alone (also under
// -fsanitize=address,undefined), takes no input, prints one line per case and exits non-zero on the first mismatch.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../ring_zk_amd/csrc/rzk_core.h"

using namespace rzk;

namespace {

int failures = 0;

std::vector<int64_t> schoolbook(const std::vector<int32_t>& d, const std::vector<int32_t>& v) {
  const int N = (int)v.size();
  std::vector<int64_t> out(N, 0);
  for (int s = 0; s < N; ++s) {
    if (!d[s]) continue;
    for (int t = 0; t < N; ++t) {
      const int j = s + t;
      if (j < N) out[j] += (int64_t)d[s] * v[t];
      else out[j - N] -= (int64_t)d[s] * v[t];
    }
  }
  return out;
}

// the wavefront, lane by lane; every loop over the lanes ends where the kernel has a wave_sync
template <int LOGN>
bool bytes_product(const std::vector<int32_t>& d, const std::vector<int32_t>& v, std::vector<int64_t>& out) {
  using S = ShiftGeo<LOGN, true>;
  using B = ByteGeo<LOGN>;
  static int32_t a[64][S::E], vr[64][S::E];
  uint32_t maxv = 0;
  uint64_t suma = 0;
  for (int l = 0; l < 64; ++l)
    for (int i = 0; i < S::E; ++i) {
      a[l][i] = d[S::j(l, i)];
      vr[l][i] = v[S::j(l, i)];
      const uint32_t av = vr[l][i] < 0 ? 0u - (uint32_t)vr[l][i] : (uint32_t)vr[l][i];
      const uint32_t aa = a[l][i] < 0 ? 0u - (uint32_t)a[l][i] : (uint32_t)a[l][i];
      maxv = av > maxv ? av : maxv;
      suma += aa < 256u ? aa : 256u;   // (saturated per entry, as the kernel's 32-bit sum)
    }
  if (!shift_bytes_ok(suma, maxv)) return false;
  // exactly the image, so that the sanitizer sees every access a lane makes; poisoned, so that a byte the fill left
  // out would show in the result
  std::vector<uint32_t> img(B::IMG_WORDS, 0xA5A5A5A5u);
  for (int l = 0; l < 64; ++l)
    for (int g = 0; g < S::G; ++g) shift_bytes_put_raw<LOGN>(vr[l][2 * g], vr[l][2 * g + 1], l, g, img.data());
  for (int l = 0; l < 64; ++l) shift_bytes_bias<LOGN>(l, maxv, img.data());
  static uint32_t acc[64][B::W];
  for (int l = 0; l < 64; ++l) {
    for (int k = 0; k < B::W; ++k) acc[l][k] = 0;
    for (int i = 0; i < S::E; ++i)        // the ballot / readlane walk: registers in order, lanes in order
      for (int src = 0; src < 64; ++src)
        if (a[src][i] != 0) shift_bytes_accum<LOGN>(acc[l], l, S::off(i) + 2 * src, a[src][i], img.data());
  }
  for (int l = 0; l < 64; ++l) shift_bytes_park<LOGN>(acc[l], l, img.data());
  out.assign(S::N, 0);
  for (int l = 0; l < 64; ++l) {
    int32_t r[S::E];
    shift_bytes_take<LOGN>(r, l, (uint32_t)suma * maxv, img.data());
    for (int i = 0; i < S::E; ++i) out[S::j(l, i)] = r[i];
  }
  return true;
}

template <int LOGN>
void run(const char* name, const std::vector<int32_t>& d, const std::vector<int32_t>& v, bool want_bytes) {
  std::vector<int64_t> got;
  const bool took = bytes_product<LOGN>(d, v, got);
  bool ok = took == want_bytes;
  if (took) ok = ok && got == schoolbook(d, v);
  std::printf("%s N=%d %s %s\n", ok ? "ok  " : "FAIL", 1 << LOGN, took ? "bytes" : "words", name);
  if (!ok) ++failures;
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {   // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (uint32_t)((z ^ (z >> 31)) >> 16);
}
std::vector<int32_t> uniform(int N, int b) {
  std::vector<int32_t> v(N);
  for (auto& c : v) c = (int32_t)(rnd() % (2 * b + 1)) - b;
  v[rnd() % N] = b;   // the bound is attained
  return v;
}
std::vector<int32_t> challenge(int N, int kappa) {
  std::vector<int32_t> d(N, 0);
  for (int n = 0; n < kappa;) {
    const int p = (int)(rnd() % N);
    if (d[p]) continue;
    d[p] = (rnd() & 1) ? 1 : -1;
    ++n;
  }
  return d;
}
std::vector<int32_t> at(int N, std::initializer_list<int> pos, int val) {
  std::vector<int32_t> d(N, 0);
  for (int p : pos) d[p] = val;
  return d;
}

template <int LOGN>
void cases() {
  constexpr int N = 1 << LOGN;
  char name[96];
  for (int rep = 0; rep < 4; ++rep) {
    std::snprintf(name, sizeof name, "ternary x challenge(36) #%d", rep);
    run<LOGN>(name, challenge(N, 36), uniform(N, 1), true);
  }
  // the edge of the condition, every byte sum at 0 or at its maximum
  for (int m = 1; m <= 3; ++m) {
    const int fit = 255 / (2 * m);
    for (int sign : {1, -1}) {
      std::vector<int32_t> d(N, 0), d1(N, 0), v(N, m * sign);
      for (int i = 0; i < fit; ++i) d[(i * 7) % N] = sign;
      d1 = d;
      for (int p = N - 1; p >= 0; --p)
        if (!d1[p]) {
          d1[p] = sign;
          break;
        }
      std::snprintf(name, sizeof name, "edge |v|=%d sign %+d: %d non-zeros", m, sign, fit);
      run<LOGN>(name, d, v, true);
      std::snprintf(name, sizeof name, "edge |v|=%d sign %+d: %d non-zeros", m, sign, fit + 1);
      run<LOGN>(name, d1, v, false);
      std::snprintf(name, sizeof name, "edge |v|=%d sign %+d: random v, %d non-zeros", m, sign, fit);
      run<LOGN>(name, d, uniform(N, m), true);
    }
  }
  // rotation extremes: every byte alignment, the wrap, the boundaries of a lane's 16 outputs and of the 64-dword rows
  for (int val : {1, -1}) {
    for (int p : {0, 1, 2, 3, 4, 5, 15, 16, 17, 127, 128, 129, 255, 256, 257, N / 2 - 1, N / 2, N / 2 + 1, N - 3, N - 2, N - 1}) {
      std::snprintf(name, sizeof name, "single %+d at %d", val, p);
      run<LOGN>(name, at(N, {p}, val), uniform(N, 1), true);
    }
    run<LOGN>("positions 0 1 2 3 N/2 N-1 together", at(N, {0, 1, 2, 3, N / 2, N - 1}, val), uniform(N, 3), true);
  }
  run<LOGN>("zero multiplier", std::vector<int32_t>(N, 0), uniform(N, 1), true);
  run<LOGN>("zero multiplier, wide operand", std::vector<int32_t>(N, 0), uniform(N, 1000), false);
  run<LOGN>("zero operand", challenge(N, 36), std::vector<int32_t>(N, 0), true);
  run<LOGN>("entries of magnitude 2 and 3", [] { auto d = at(N, {5, 300}, 2); d[77] = -3; d[78] = 1; return d; }(), uniform(N, 2), true);
  run<LOGN>("dense +-3 multiplier", uniform(N, 3), uniform(N, 1), false);
  run<LOGN>("one entry of 256", at(N, {9}, 256), std::vector<int32_t>(N, 0), false);
  run<LOGN>("INT32_MIN in the operand", at(N, {1}, 1), [] { std::vector<int32_t> v(N, 0); v[3] = INT32_MIN; return v; }(), false);
}

}  // namespace

int main() {
  cases<9>();
  cases<10>();
  if (failures) {
    std::printf("%d case(s) failed\n", failures);
    return 1;
  }
  std::printf("all cases passed\n");
  return 0;
}
