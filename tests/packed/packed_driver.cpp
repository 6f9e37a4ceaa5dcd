// CPU driver over ring_zk_amd/csrc/rzk_packed.h for tests/test_packed_host.py (g++ -fsanitize=address,undefined).
// Reads a file of cases, each starting with a u32 op, and prints one line per result:
//   op 1  sizes    u32 kind N n k l V, i64 q, u64 verify_bound            -> "<valid> <record bytes> <W_Q> <W_Z> <W_D>"
//   op 2  encode   the same header, u32 B, then every field's slab [B][rows][N] i64   -> per record "<ok> <hex of the record>"
//   op 3  decode   the same header, u32 B, then B records                 -> per record "<ok> <hex of its slabs, field after field>"
//   op 4  division packed_div against / for every W in 2 .. 32 and x < 2^13 -> "<all equal>"
// Encode writes into a buffer of exactly B * record_bytes and decode into slabs of exactly their size, so that the
// sanitizer sees any access outside a polynomial's own words.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../ring_zk_amd/csrc/rzk_packed.h"

using namespace rzk;

namespace {

struct Reader {
  std::vector<uint8_t> buf;
  size_t pos = 0;
  bool take(void* dst, size_t n) {
    if (buf.size() - pos < n) return false;
    if (n) memcpy(dst, buf.data() + pos, n);
    pos += n;
    return true;
  }
};

void print_hex(const void* p, size_t n) {
  const uint8_t* b = (const uint8_t*)p;
  for (size_t i = 0; i < n; ++i) printf("%02x", b[i]);
}

struct Head {
  uint32_t kind, N, n, k, l, V;
  int64_t q;
  uint64_t vb;
};

bool read_head(Reader& r, Head& h) { return r.take(&h, 6 * sizeof(uint32_t)) && r.take(&h.q, 8) && r.take(&h.vb, 8); }

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  Reader r;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint8_t tmp[4096];
  size_t got;
  while ((got = fread(tmp, 1, sizeof(tmp), f)) > 0) r.buf.insert(r.buf.end(), tmp, tmp + got);
  fclose(f);
  uint32_t op;
  while (r.take(&op, 4)) {
    if (op == 4) {
      bool same = true;
      for (uint32_t W = 2; W <= 32; ++W) {
        PackedWidth w;
        if (!packed_width(1, (1ull << W) - 2, &w) || w.W != W) return 3;
        for (uint32_t x = 0; x < (1u << 13); ++x) same = same && packed_div(x, w) == x / W;
      }
      printf("%d\n", same ? 1 : 0);
      continue;
    }
    Head h;
    if (!read_head(r, h)) return 3;
    PackedSchema s;
    const bool valid = packed_schema((int)h.kind, h.N, h.n, h.k, h.l, h.V, h.q, h.vb, &s);
    if (op == 1) {
      if (valid)
        printf("1 %llu %u %u %u\n", (unsigned long long)packed_record_bytes(s), s.w[PK_Q].W, s.w[PK_Z].W, s.w[PK_D].W);
      else
        printf("0 0 0 0 0\n");
      continue;
    }
    uint32_t B;
    if (!valid || !r.take(&B, 4)) return 3;
    // every slab and the record buffer in an allocation of exactly its size
    std::vector<std::vector<int64_t>> slabs(s.nfields);
    for (uint32_t fi = 0; fi < s.nfields; ++fi) slabs[fi].resize((size_t)B * s.f[fi].rows * s.N);
    std::vector<uint64_t> recs((size_t)B * s.rec_words);
    if (op == 2) {
      for (uint32_t fi = 0; fi < s.nfields; ++fi)
        if (!r.take(slabs[fi].data(), slabs[fi].size() * 8)) return 3;
      for (uint32_t b = 0; b < B; ++b) {
        const int64_t* fp[kPackedMaxFields] = {};
        for (uint32_t fi = 0; fi < s.nfields; ++fi) fp[fi] = slabs[fi].data() + (size_t)b * s.f[fi].rows * s.N;
        uint64_t* rec = recs.data() + (size_t)b * s.rec_words;
        const bool ok = packed_encode_record(s, fp, rec);
        printf("%d ", ok ? 1 : 0);
        print_hex(rec, 8 * (size_t)s.rec_words);
        printf("\n");
      }
    } else if (op == 3) {
      if (!r.take(recs.data(), recs.size() * 8)) return 3;
      for (uint32_t b = 0; b < B; ++b) {
        int64_t* fp[kPackedMaxFields] = {};
        for (uint32_t fi = 0; fi < s.nfields; ++fi) fp[fi] = slabs[fi].data() + (size_t)b * s.f[fi].rows * s.N;
        const bool ok = packed_decode_record(s, recs.data() + (size_t)b * s.rec_words, fp);
        printf("%d ", ok ? 1 : 0);
        for (uint32_t fi = 0; fi < s.nfields; ++fi) print_hex(fp[fi], 8 * (size_t)s.f[fi].rows * s.N);
        printf("\n");
      }
    } else {
      return 3;
    }
  }
  return r.pos == r.buf.size() ? 0 : 3;
}
