// CPU driver of the message walker (ring_zk_amd/csrc/rzk_wire_walk.h), built by tests/test_wire_walk.py with g++ and
// -fsanitize=address,undefined.  Every message is copied into a heap block of exactly its own size (after `shift`
// leading bytes), so any read outside the message span is reported by the sanitizer.
//
// stdin-free: reads the case file named by argv[1]:
//   u32 kind, N, n, k, l, V, coef_bytes, ncases ; ncases x { u32 shift ; u64 len ; len bytes }
// writes one line per case to stdout:  ok polys j:pos:len ...   (pos relative to the message start)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../ring_zk_amd/csrc/rzk_wire_walk.h"

namespace {

struct Rec {
  std::vector<uint64_t> pos;
  std::vector<uint32_t> len;
  void operator()(uint32_t j, uint64_t p, uint32_t l) {
    if (j >= pos.size()) {
      std::fprintf(stderr, "emit index %u out of range\n", j);
      std::abort();
    }
    pos[j] = p;
    len[j] = l;
  }
};

bool rd(FILE* f, void* p, size_t n) { return std::fread(p, 1, n, f) == n; }

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t hdr[8];
  if (!rd(f, hdr, sizeof hdr)) return 2;
  rzk::WireSchema s;
  if (!rzk::wire_schema((int)hdr[0], hdr[1], hdr[2], hdr[3], hdr[4], hdr[5], hdr[6], &s)) {
    std::printf("schema-rejected\n");
    return 0;
  }
  std::printf("schema %u %llu %llu\n", s.polys, (unsigned long long)rzk::wire_struct_total(s),
              (unsigned long long)rzk::wire_max_bytes(s));
  for (uint32_t j = 0; j < s.polys; ++j) std::printf("%llu ", (unsigned long long)rzk::wire_struct_before(s, j));
  std::printf("\n");
  for (uint32_t c = 0; c < hdr[7]; ++c) {
    uint32_t shift;
    uint64_t len;
    if (!rd(f, &shift, 4) || !rd(f, &len, 8)) return 2;
    uint8_t* block = (uint8_t*)std::malloc(shift + len ? shift + len : 1);
    if (!rd(f, block + shift, len)) return 2;
    Rec rec;
    rec.pos.assign(s.polys, 0);
    rec.len.assign(s.polys, 0);
    const bool ok = rzk::wire_walk(block + shift, len, s, rec);
    std::printf("%d", ok ? 1 : 0);
    if (ok)
      for (uint32_t j = 0; j < s.polys; ++j) std::printf(" %llu:%u", (unsigned long long)rec.pos[j], rec.len[j]);
    std::printf("\n");
    std::free(block);
  }
  std::fclose(f);
  return 0;
}
