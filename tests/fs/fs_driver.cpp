// CPU driver of ring_zk_amd/csrc/rzk_keccak.h for tests/test_fs_transcript.py (g++ -fsanitize=address,undefined).
// Reads records from the file named on the command line and prints one line of results per record:
//   u32 1, u32 len, u32 outlen, len bytes                     -> "shake <hex>"
//   u32 2, u32 kind V N n k l kappa M, i64 q, u64 b, aux[32], (n+l)*k*N i64 key, M*N i64 message polynomials
//                                                             -> "fs <keydigest hex> <leaf digests hex> <digest hex> <d ...>"
//   u32 3, u32 N, u32 kappa, u32 len, len bytes               -> "sample <d ...>", d from SHAKE256(bytes)[32:]
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../ring_zk_amd/csrc/rzk_keccak.h"

using namespace rzk;

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

static void hex(const uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; ++i) printf("%02x", p[i]);
}

static void words_to_bytes(const uint64_t* w, size_t nw, uint8_t* out) {
  for (size_t i = 0; i < nw; ++i)
    for (int b = 0; b < 8; ++b) out[8 * i + b] = (uint8_t)(w[i] >> (8 * b));
}

// leaf digests of `count` polynomials, word w of leaf j at dig[j * 4 + w] (stride 1)
static std::vector<uint64_t> leaf_digests(const int64_t* polys, uint32_t count, uint32_t N) {
  const uint32_t C = N / fs_leaf_len(N);
  std::vector<uint64_t> dig((size_t)count * C * kFsDigestWords);
  for (uint32_t p = 0; p < count; ++p)
    for (uint32_t c = 0; c < C; ++c) fs_leaf(polys + (size_t)p * N, N, p, c, &dig[((size_t)p * C + c) * kFsDigestWords]);
  return dig;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t type;
  while (fread(&type, 4, 1, f) == 1) {
    if (type == 1) {
      uint32_t len, outlen;
      if (!rd(f, &len, 4) || !rd(f, &outlen, 4)) return 3;
      std::vector<uint8_t> msg(len), out(outlen);   // exact sizes: the sanitizer sees any byte touched beyond them
      if (!rd(f, msg.data(), len)) return 3;
      shake256(msg.data(), len, out.data(), outlen);
      printf("shake ");
      hex(out.data(), outlen);
      printf("\n");
    } else if (type == 2) {
      uint32_t h[8];
      int64_t q;
      uint64_t b;
      uint8_t auxb[32];
      if (!rd(f, h, sizeof h) || !rd(f, &q, 8) || !rd(f, &b, 8) || !rd(f, auxb, 32)) return 3;
      const uint32_t kind = h[0], V = h[1], N = h[2], n = h[3], k = h[4], l = h[5], kappa = h[6], M = h[7];
      std::vector<int64_t> key((size_t)(n + l) * k * N), polys((size_t)M * N);
      if (!rd(f, key.data(), key.size() * 8) || !rd(f, polys.data(), polys.size() * 8)) return 3;
      uint64_t s[25], kd[kFsDigestWords], aux[kFsDigestWords], hdr[kFsRootHeaderWords];
      // key digest
      const std::vector<uint64_t> kdig = leaf_digests(key.data(), (n + l) * k, N);
      fs_key_header(q, N, n, k, l, kappa, b, hdr);
      FsRootWords kw{hdr, kFsKeyHeaderWords, kdig.data(), 1, 0};
      shake256_absorb(s, kw, kFsKeyHeaderWords + (uint32_t)kdig.size(), 0, 0);
      for (uint32_t i = 0; i < kFsDigestWords; ++i) kd[i] = s[i];
      // root
      const std::vector<uint64_t> dig = leaf_digests(polys.data(), M, N);
      for (uint32_t i = 0; i < kFsDigestWords; ++i) aux[i] = shake256_load_le(auxb + 8 * i, 8);
      fs_root_header(kind, V, kd, aux, hdr);
      FsRootWords rw{hdr, kFsRootHeaderWords, dig.data(), 1, 0};
      shake256_absorb(s, rw, kFsRootHeaderWords + (uint32_t)dig.size(), 0, 0);
      uint8_t out[32];
      std::vector<uint8_t> lb(dig.size() * 8);
      printf("fs ");
      words_to_bytes(kd, kFsDigestWords, out);
      hex(out, 32);
      printf(" ");
      words_to_bytes(dig.data(), dig.size(), lb.data());
      hex(lb.data(), lb.size());
      printf(" ");
      words_to_bytes(s, kFsDigestWords, out);
      hex(out, 32);
      std::vector<int64_t> d(N, 0);
      fs_sample_challenge(s, d.data(), N, kappa);
      for (uint32_t i = 0; i < N; ++i) printf(" %lld", (long long)d[i]);
      printf("\n");
    } else if (type == 3) {
      uint32_t N, kappa, len;
      if (!rd(f, &N, 4) || !rd(f, &kappa, 4) || !rd(f, &len, 4)) return 3;
      std::vector<uint8_t> msg(len);
      if (!rd(f, msg.data(), len)) return 3;
      uint64_t s[25];
      ShakeByteWords word{msg.data()};
      shake256_absorb(s, word, len / 8, shake256_load_le(msg.data() + (len & ~7u), len & 7u), len & 7u);
      std::vector<int64_t> d(N, 0);
      fs_sample_challenge(s, d.data(), N, kappa);
      printf("sample");
      for (uint32_t i = 0; i < N; ++i) printf(" %lld", (long long)d[i]);
      printf("\n");
    } else {
      return 4;
    }
  }
  fclose(f);
  return 0;
}
