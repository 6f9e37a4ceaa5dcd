// Host driver of the per-coefficient arithmetic of the 32-bit norm kernel (norm_rows<., int32_t>, ring_zk_amd/csrc/rzk_norm.h,
// which takes it from ring_zk_amd/csrc/rzk_slab32.h) for tests/test_linear32_host.py.
//   norm32_driver CASES   per line "q c" (c any int32): canonical, |c| as the kernel squares it, and the two 32-bit halves
//                         of its square as the kernel adds them to its lane sums
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

#include "../../ring_zk_amd/csrc/rzk_slab32.h"

using namespace rzk;

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: norm32_driver CASES\n");
    return 2;
  }
  std::ifstream in(argv[1]);
  if (!in) return 2;
  std::string line;
  while (std::getline(in, line)) {
    if (line.empty()) continue;
    std::istringstream ss(line);
    unsigned long long q;
    long long c;
    if (!(ss >> q >> c) || c < INT32_MIN || c > INT32_MAX) return 2;
    const uint32_t half = slab32_half(q);
    const uint64_t al = slab32_abs((int32_t)c);
    const uint64_t ll = al * al;
    std::printf("%d %llu %llu %llu\n", (int)slab32_canonical((int32_t)c, half), (unsigned long long)al,
                (unsigned long long)(ll & 0xffffffffu), (unsigned long long)(ll >> 32));
  }
  return 0;
}
