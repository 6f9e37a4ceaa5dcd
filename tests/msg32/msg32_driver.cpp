// Host driver of the 32-bit message rules for tests/test_msg32_host.py: the leaf hash of the FS1 transcript on int32
// coefficients (ring_zk_amd/csrc/rzk_keccak.h) and the 32-bit form of the packed codec's raw rule (rzk_packed.h).
//   msg32_driver leaf CASES   per line "N p c v_0 .. v_{N-1}" (int32 values): the digest of leaf (p, c) of the polynomial as
//                             hex, from int32_t coefficients and from the same values as int64_t
//   msg32_driver raw CASES    per line "q verify_bound class c" (c an int32 value): ok32 raw32 ok64 raw64
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../ring_zk_amd/csrc/rzk_keccak.h"
#include "../../ring_zk_amd/csrc/rzk_packed.h"

using namespace rzk;

namespace {

void print_digest(const uint64_t d[kFsDigestWords]) {
  for (uint32_t w = 0; w < kFsDigestWords; ++w)
    for (int i = 0; i < 8; ++i) std::printf("%02x", (unsigned)((d[w] >> (8 * i)) & 0xffu));
}

int run_leaf(const char* path) {
  std::ifstream in(path);
  if (!in) return 2;
  std::string line;
  while (std::getline(in, line)) {
    if (line.empty()) continue;
    std::istringstream ss(line);
    uint32_t N, p, c;
    if (!(ss >> N >> p >> c)) return 2;
    std::vector<int32_t> v32(N);   // exactly N elements: a read past the polynomial is a sanitizer report
    std::vector<int64_t> v64(N);
    for (uint32_t i = 0; i < N; ++i) {
      long long v;
      if (!(ss >> v)) return 2;
      v32[i] = (int32_t)v;
      v64[i] = (int64_t)v;
    }
    if (c >= N / fs_leaf_len(N)) return 2;
    uint64_t d32[kFsDigestWords], d64[kFsDigestWords];
    fs_leaf(v32.data(), N, p, c, d32);
    fs_leaf(v64.data(), N, p, c, d64);
    print_digest(d32);
    std::printf(" ");
    print_digest(d64);
    std::printf("\n");
  }
  return 0;
}

int run_raw(const char* path) {
  std::ifstream in(path);
  if (!in) return 2;
  std::string line;
  while (std::getline(in, line)) {
    if (line.empty()) continue;
    std::istringstream ss(line);
    long long q, c;
    unsigned long long vb;
    unsigned cls;
    if (!(ss >> q >> vb >> cls >> c) || cls >= PK_NCLASSES) return 2;
    PackedWidth w[PK_NCLASSES];
    if (!packed_widths((int64_t)q, vb, w)) return 3;
    uint32_t r32 = 0, r64 = 0;
    const bool ok32 = packed_raw32((int32_t)c, w[cls], &r32);
    const bool ok64 = packed_raw((int64_t)c, w[cls], &r64);
    std::printf("%d %u %d %u\n", (int)ok32, r32, (int)ok64, r64);
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const std::string mode = argv[1];
  if (mode == "leaf") return run_leaf(argv[2]);
  if (mode == "raw") return run_raw(argv[2]);
  return 2;
}
