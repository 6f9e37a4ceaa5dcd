// Host driver for ring_zk_amd/csrc/rzk_slabs.h: prints every call's slab list for a shape.  tests/test_slabs_host.py
// builds it with g++ under -fsanitize=address,undefined and holds the output against the declarations of include/rzk.h.
//   slabs_driver n k l V rows
// One line per slab:  <call> <both_widths> <name> <coef|bytes> <in|out> <req|opt> <count>
// count: polynomials per proof of a coefficient slab, bytes per proof of a companion.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../../ring_zk_amd/csrc/rzk_slabs.h"

using namespace rzk;

int main(int argc, char** argv) {
  if (argc != 6) {
    std::fprintf(stderr, "usage: slabs_driver n k l V rows\n");
    return 2;
  }
  const SlabDims dm = {std::strtoull(argv[1], nullptr, 10), std::strtoull(argv[2], nullptr, 10), std::strtoull(argv[3], nullptr, 10),
                       std::strtoull(argv[4], nullptr, 10), std::strtoull(argv[5], nullptr, 10)};
  for (const CallSlabs* call : kAllCallSlabs)
    for (size_t i = 0; i < slab_len(*call); ++i) {
      const Slab& s = call->s[i];
      std::printf("%s %d %s %s %s %s %llu\n", call->call, (int)call->both_widths, s.name, slab_is_coef(s.kind) ? "coef" : "bytes",
                  slab_reads(s.role) ? "in" : "out", slab_optional(s.role) ? "opt" : "req", (unsigned long long)slab_count(s.kind, dm));
    }
  // the key rows a selector names, for 0, 1, 2 and two values that are none
  std::printf("key_rows");
  for (int which : {0, 1, 2, -1, 3}) std::printf(" %u", key_row_count(which, (uint32_t)dm.n, (uint32_t)dm.l));
  std::printf("\n");
  return 0;
}
