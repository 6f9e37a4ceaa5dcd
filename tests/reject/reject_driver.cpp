// CPU driver of ring_zk_amd/csrc/rzk_reject.h for tests/test_reject_host.py (g++, ASan + UBSan).
// Input: records, little-endian.
//   u32 1 | i64 q, vmax, verify_bound, sigma | f64 lnM | u64 R | u32 N, rows, B, trusted | z [B][rows][N] i64 | y likewise |
//           coin [B] i64                 -> B lines "E flags accept"
//   u32 2 | f64 alpha                    -> "lnm <hex float>"
//   u32 3 | u64 rows | u32 N | u64 vmax | u64 verify_bound   -> "args <0|1>"
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../ring_zk_amd/csrc/rzk_reject.h"

using namespace rzk;

namespace {

struct Reader {
  std::vector<uint8_t> buf;
  size_t pos = 0;
  bool ok = true;
  template <class T>
  T get() {
    T v{};
    if (pos + sizeof(T) > buf.size()) {
      ok = false;
      return v;
    }
    std::memcpy(&v, buf.data() + pos, sizeof(T));
    pos += sizeof(T);
    return v;
  }
  void get_i64(std::vector<int64_t>& out, size_t n) {
    out.assign(n, 0);
    if (n > (buf.size() - pos) / sizeof(int64_t)) {
      ok = false;
      return;
    }
    if (n) std::memcpy(out.data(), buf.data() + pos, n * sizeof(int64_t));
    pos += n * sizeof(int64_t);
  }
};

template <bool CHECK>
RejectPartial poly_partial(const int64_t* z, const int64_t* y, uint32_t N, int64_t q, int64_t vmax, uint64_t limit) {
  RejectAcc a{0, 0, 0, 0};
  for (uint32_t i = 0; i < N; ++i) reject_step<CHECK>(a, z[i], y[i], q, (q - 1) / 2, vmax);
  return reject_partial(reject_e(a), a.zsq, a.flags, limit);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  Reader r;
  uint8_t chunk[1 << 16];
  size_t got;
  while ((got = std::fread(chunk, 1, sizeof(chunk), f)) > 0) r.buf.insert(r.buf.end(), chunk, chunk + got);
  std::fclose(f);
  while (r.pos < r.buf.size()) {
    const uint32_t kind = r.get<uint32_t>();
    if (kind == 2) {
      const double alpha = r.get<double>();
      if (!r.ok) return 3;
      std::printf("lnm %a\n", reject_lnm(alpha));
    } else if (kind == 3) {
      const uint64_t rows = r.get<uint64_t>();
      const uint32_t N = r.get<uint32_t>();
      const uint64_t vmax = r.get<uint64_t>();
      const uint64_t vb = r.get<uint64_t>();
      if (!r.ok) return 3;
      std::printf("args %d\n", reject_args_ok(rows, N, vmax, vb) ? 1 : 0);
    } else if (kind == 1) {
      const int64_t q = r.get<int64_t>(), vmax = r.get<int64_t>(), vb = r.get<int64_t>(), sigma = r.get<int64_t>();
      const double lnM = r.get<double>();
      const uint64_t R = r.get<uint64_t>();
      const uint32_t N = r.get<uint32_t>(), rows = r.get<uint32_t>(), B = r.get<uint32_t>(), trusted = r.get<uint32_t>();
      if (!r.ok || !reject_args_ok(rows, N, (uint64_t)vmax, (uint64_t)vb)) return 3;
      std::vector<int64_t> z, y, coin;
      r.get_i64(z, (size_t)B * rows * N);
      r.get_i64(y, (size_t)B * rows * N);
      r.get_i64(coin, B);
      if (!r.ok) return 3;
      const uint64_t limit = (uint64_t)(vb + 1) * (uint64_t)(vb + 1);
      const double s = (double)sigma;
      for (uint32_t b = 0; b < B; ++b) {
        uint64_t e = 0;
        uint32_t flags = 0;
        for (uint32_t j = 0; j < rows; ++j) {
          const size_t off = ((size_t)b * rows + j) * N;
          const RejectPartial p = trusted ? poly_partial<false>(&z[off], &y[off], N, q, vmax, limit)
                                          : poly_partial<true>(&z[off], &y[off], N, q, vmax, limit);
          e += (uint64_t)p.e;
          flags |= p.flags;
        }
        const bool acc = reject_decide((int64_t)e, flags, coin[b], R, lnM, 2.0 * s * s);
        std::printf("%lld %u %d\n", (long long)(int64_t)e, flags | reject_coin_flags(coin[b], R), acc ? 1 : 0);
      }
    } else {
      return 4;
    }
  }
  return 0;
}
