// CPU driver of reject_step_v (ring_zk_amd/csrc/rzk_reject.h) for tests/test_response_stat_host.py (g++, ASan + UBSan):
// the per-coefficient step of the fused response rows, which takes the centred product sum v the kernel holds, next to
// reject_step, which derives v from z - y.
// Input: records, little-endian.
//   u32 1 | i64 q, vmax | u32 n, check | z [n] i64 | v [n] i64 | y [n] i64
//       -> n lines "s1 s2 zsq flags s1v s2v zsqv flagsv" (each coefficient into accumulators of its own, unsigned decimal)
//          and one line "total ..." of the same eight numbers with all n coefficients in one accumulator each
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../ring_zk_amd/csrc/rzk_reject.h"

using namespace rzk;

namespace {

bool read_i64(const std::vector<uint8_t>& buf, size_t& pos, std::vector<int64_t>& out, size_t n) {
  out.assign(n, 0);
  if (n > (buf.size() - pos) / sizeof(int64_t)) return false;
  if (n) std::memcpy(out.data(), buf.data() + pos, n * sizeof(int64_t));
  pos += n * sizeof(int64_t);
  return true;
}

template <bool CHECK>
void both(RejectAcc& a, RejectAcc& av, int64_t z, int64_t v, int64_t y, int64_t q, int64_t vmax) {
  const int64_t half = (q - 1) / 2;
  reject_step<CHECK>(a, z, y, q, half, vmax);
  reject_step_v<CHECK>(av, z, v, y > half || y < -half, vmax);
}

void print(const char* head, const RejectAcc& a, const RejectAcc& av) {
  std::printf("%s%llu %llu %llu %u %llu %llu %llu %u\n", head, (unsigned long long)a.s1, (unsigned long long)a.s2,
              (unsigned long long)a.zsq, a.flags, (unsigned long long)av.s1, (unsigned long long)av.s2, (unsigned long long)av.zsq,
              av.flags);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> buf;
  uint8_t chunk[1 << 16];
  size_t got;
  while ((got = std::fread(chunk, 1, sizeof(chunk), f)) > 0) buf.insert(buf.end(), chunk, chunk + got);
  std::fclose(f);
  size_t pos = 0;
  while (pos < buf.size()) {
    struct {
      uint32_t kind;
      int64_t q, vmax;
      uint32_t n, check;
    } __attribute__((packed)) h;
    if (buf.size() - pos < sizeof(h)) return 3;
    std::memcpy(&h, buf.data() + pos, sizeof(h));
    pos += sizeof(h);
    if (h.kind != 1) return 4;
    std::vector<int64_t> z, v, y;
    if (!read_i64(buf, pos, z, h.n) || !read_i64(buf, pos, v, h.n) || !read_i64(buf, pos, y, h.n)) return 3;
    RejectAcc t{0, 0, 0, 0}, tv{0, 0, 0, 0};
    for (uint32_t i = 0; i < h.n; ++i) {
      RejectAcc a{0, 0, 0, 0}, av{0, 0, 0, 0};
      if (h.check) {
        both<true>(a, av, z[i], v[i], y[i], h.q, h.vmax);
        both<true>(t, tv, z[i], v[i], y[i], h.q, h.vmax);
      } else {
        both<false>(a, av, z[i], v[i], y[i], h.q, h.vmax);
        both<false>(t, tv, z[i], v[i], y[i], h.q, h.vmax);
      }
      print("", a, av);
    }
    print("total ", t, tv);
  }
  return 0;
}
