// Host driver of the key planner (ring_zk_amd/csrc/rzk_keyplan.h) for tests/test_keyplan_host.py.
//   keyplan_driver Q N ENTRIES NKEYS FILE   FILE: NKEYS keys of ENTRIES * N little-endian int64 coefficients each
// For every key plan_key_tables — the call of rzk_key.cpp — runs into a KeyPlan filled with sentinels and into
// sentinel-filled tables standing for those a context holds from its previous key.  One line per key:
//   ok <n_general> <classes as digits> <entries, comma separated> <sha256 of the general list> <kinf as %a, comma separated | ->
//   refused <status> <1 when the KeyPlan still holds its sentinels, else 0> <the same for the context's tables>
// (ok lines print the classes and entries from the context's tables, where an accepted key has installed them)
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "../../ring_zk_amd/csrc/rzk_keyplan.h"
#include "../plan/sha256.h"

using namespace rzk;

namespace {

constexpr uint8_t kClassMark = 0xab;
constexpr int32_t kEntryMark = 0x5a5a5a5a;
constexpr uint32_t kCountMark = 0xdeadu;
constexpr int64_t kCoefMark = 0x7111111111111111ll;
constexpr double kNormMark = -12345.5;

KeyPlan sentinels(size_t entries, uint32_t N) {
  KeyPlan kp;
  kp.key_class.assign(entries, kClassMark);
  kp.key_entry.assign(entries, kEntryMark);
  kp.n_general = kCountMark;
  kp.general.assign((size_t)3 * N, kCoefMark);
  kp.kinf.assign(3, kNormMark);
  return kp;
}

bool same(const KeyPlan& a, const KeyPlan& b) {
  return a.key_class == b.key_class && a.key_entry == b.key_entry && a.n_general == b.n_general && a.general == b.general &&
         a.kinf == b.kinf;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 6) {
    std::fprintf(stderr, "usage: keyplan_driver Q N ENTRIES NKEYS FILE\n");
    return 2;
  }
  const int64_t q = std::strtoll(argv[1], nullptr, 10);
  const uint32_t N = (uint32_t)std::strtoul(argv[2], nullptr, 10);
  const size_t entries = std::strtoul(argv[3], nullptr, 10), nkeys = std::strtoul(argv[4], nullptr, 10);
  std::ifstream in(argv[5], std::ios::binary);
  if (!in) return 2;
  // exactly the key's size: a read past the last coefficient is a heap overflow under the sanitizer
  std::vector<int64_t> key(entries * N);
  for (size_t i = 0; i < nkeys; ++i) {
    if (!in.read(reinterpret_cast<char*>(key.data()), (std::streamsize)(key.size() * sizeof(int64_t)))) return 2;
    KeyPlan out = sentinels(entries, N);
    const KeyPlan out_before = out;
    // the tables a context holds from its previous key go through the function rzk_key.cpp calls: only an accepted key
    // may replace them
    std::vector<uint8_t> ctx_class(entries, kClassMark);
    std::vector<int32_t> ctx_entry(entries, kEntryMark);
    uint32_t ctx_count = kCountMark;
    const int rc = plan_key_tables(key.data(), entries, N, q, ctx_class, ctx_entry, ctx_count, out);
    if (rc != kPlanOk) {
      bool ctx_intact = ctx_count == kCountMark && ctx_class.size() == entries && ctx_entry.size() == entries;
      for (size_t e = 0; ctx_intact && e < entries; ++e) ctx_intact = ctx_class[e] == kClassMark && ctx_entry[e] == kEntryMark;
      std::printf("refused %d %d %d\n", rc, same(out, out_before) ? 1 : 0, ctx_intact ? 1 : 0);
      continue;
    }
    if (ctx_count != out.n_general) return 3;
    std::string classes, idx, norms;
    for (size_t e = 0; e < ctx_class.size(); ++e) {   // the installed tables
      classes += (char)('0' + ctx_class[e]);
      idx += (e ? "," : "") + std::to_string(ctx_entry[e]);
    }
    char buf[64];
    for (size_t g = 0; g < out.kinf.size(); ++g) {
      std::snprintf(buf, sizeof buf, "%a", out.kinf[g]);
      norms += (g ? "," : "") + std::string(buf);
    }
    std::printf("ok %u %s %s %s %s\n", out.n_general, classes.c_str(), idx.c_str(),
                sha256::hex(out.general.data(), out.general.size() * sizeof(int64_t)).c_str(), norms.empty() ? "-" : norms.c_str());
  }
  return 0;
}
