// CPU driver of ring_zk_amd/csrc/rzk_xof.h for tests/test_xof_host.py (g++ -fsanitize=address,undefined).
// Reads records from the file named on the command line and prints one line of results per record:
//   u32 1, u64 q, u32 N, u32 domain, u32 p, u32 c, seed[32]   -> "chunk <words used> <CH coefficients ...>"
//   u32 2, u64 q, u32 N, u32 domain, u32 p, seed[32]          -> "poly <N coefficients ...>"
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../ring_zk_amd/csrc/rzk_xof.h"

using namespace rzk;

static bool rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t type;
  while (fread(&type, 4, 1, f) == 1) {
    uint64_t q;
    uint32_t N, domain, p, c = 0;
    uint8_t seed[32];
    if (type != 1 && type != 2) return 4;
    if (!rd(f, &q, 8) || !rd(f, &N, 4) || !rd(f, &domain, 4) || !rd(f, &p, 4) || (type == 1 && !rd(f, &c, 4)) || !rd(f, seed, 32))
      return 3;
    // exact sizes: the sanitizer sees any coefficient written beyond them
    std::vector<int64_t> out(type == 1 ? xof_chunk_len(N) : N);
    if (type == 1) {
      printf("chunk %u", xof_chunk(q, N, domain, seed, p, c, out.data()));
    } else {
      xof_poly(q, N, domain, seed, p, out.data());
      printf("poly");
    }
    for (int64_t v : out) printf(" %lld", (long long)v);
    printf("\n");
  }
  fclose(f);
  return 0;
}
