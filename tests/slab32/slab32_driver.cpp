// Host driver of the 32-bit slab format (ring_zk_amd/csrc/rzk_slab32.h) for tests/test_slab32_host.py.
//   slab32_driver rules CASES   per line "q c" (c any int64): canon64 narrow fault, and, when c is an int32 value,
//                               canon32 widen test_word (else "-")
//   slab32_driver route CASES   per line "n k l logn small rot shift_bytes pair_poly id var key": the planner's status,
//                               the launch path of the plan and slab32_native for it (key as in plan_driver, "-" = none)
#include <cstdio>
#include <fstream>
#include <limits>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../ring_zk_amd/csrc/rzk_plan.h"
#include "../../ring_zk_amd/csrc/rzk_slab32.h"

using namespace rzk;

namespace {

int run_rules(const char* path) {
  std::ifstream in(path);
  if (!in) return 2;
  std::string line;
  while (std::getline(in, line)) {
    if (line.empty()) continue;
    std::istringstream ss(line);
    unsigned long long q;
    long long c;
    if (!(ss >> q >> c)) return 2;
    const uint32_t half = slab32_half(q);
    bool fault = false;
    const int32_t nar = slab32_narrow((int64_t)c, half, &fault);
    std::printf("%d %d %d", (int)slab64_canonical((int64_t)c, half), (int)nar, (int)fault);
    if (c >= std::numeric_limits<int32_t>::min() && c <= std::numeric_limits<int32_t>::max()) {
      const int32_t c32 = (int32_t)c;
      std::printf(" %d %lld %u\n", (int)slab32_canonical(c32, half), (long long)slab32_widen(c32), slab32_test_word(c32, half));
    } else {
      std::printf(" - - -\n");
    }
  }
  return 0;
}

int run_route(const char* path) {
  std::ifstream in(path);
  if (!in) return 2;
  std::unique_ptr<Plan> plan(new Plan);
  std::string line;
  while (std::getline(in, line)) {
    if (line.empty()) continue;
    std::istringstream ss(line);
    PlanEnv e{};
    int small, rot, shift_bytes, pair_poly, id;
    uint32_t var;
    std::string key;
    if (!(ss >> e.n >> e.k >> e.l >> e.logn >> small >> rot >> shift_bytes >> pair_poly >> id >> var >> key)) return 2;
    // the knobs of a default context (rzk_ctx_create)
    e.small = small != 0;
    e.rot = rot != 0;
    e.block_min_logn = 11;
    e.use_groups = true;
    e.group_max = group_max_for((int)e.logn);
    e.use_pairs = true;
    e.slot_share_min = 2.0;
    e.dot2 = true;
    std::vector<uint8_t> key_class;
    std::vector<int32_t> key_entry;
    if (key != "-") {
      if (key.size() != (size_t)(e.n + e.l) * e.k) return 2;
      int32_t general = 0;
      for (char ch : key) {
        key_class.push_back((uint8_t)(ch - '0'));
        key_entry.push_back(ch - '0' == KC_GENERAL ? general++ : -1);
      }
    }
    e.key_class = key_class.data();
    e.key_entry = key_entry.data();
    const int rc = plan_program(e, id, var, *plan);
    if (rc != kPlanOk) {
      std::printf("%d - 0\n", rc);
      continue;
    }
    const Path p = path_of(plan->f, e.small, true);
    const Slab32Facts f = slab32_facts(plan->f, p == Path::Units, p == Path::Shift, e.n, e.rot, shift_bytes != 0);
    const int team_ll = (e.logn >= 11 && pair_poly) ? 7 : 6;
    std::printf("%d %d %d\n", rc, (int)p, (int)slab32_native(f, e.logn, e.small, team_ll));
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "rules" && argc == 3) return run_rules(argv[2]);
  if (mode == "route" && argc == 3) return run_route(argv[2]);
  std::fprintf(stderr, "usage: slab32_driver rules CASES | slab32_driver route CASES\n");
  return 2;
}
