// Host driver of the 32-bit slab format (ring_zk_amd/csrc/rzk_slab32.h) for tests/test_slab32_host.py.
//   slab32_driver rules CASES   per line "q c" (c any int64): canon64 narrow fault, and, when c is an int32 value,
//                               canon32 widen test_word (else "-")
//   slab32_driver route CASES   per line "n k l logn small rot shift_bytes pair_poly id var key": the planner's status,
//                               the launch path of the plan and slab32_native for it (key as in plan_driver, "-" = none)
//   slab32_driver coef CASES    per line "N count": the typed byte count of `count` polynomials (rzk_coef.h) for int64_t and
//                               int32_t slabs, and whether launch_addr kept the address of a slab of each type (1 1)
#include <cstdio>
#include <fstream>
#include <limits>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../ring_zk_amd/csrc/rzk_coef.h"
#include "../../ring_zk_amd/csrc/rzk_plan.h"
#include "../../ring_zk_amd/csrc/rzk_slab32.h"

using namespace rzk;

namespace {

// An operand list has the type of its slabs: Op<C>{p, stride, outer} exists for a const C* only, so a 32-bit list cannot
// be filled from 64-bit slabs or the reverse (the mistake a runtime width argument let through).
template <class O, class P, class = void>
struct OpFrom : std::false_type {};
template <class O, class P>
struct OpFrom<O, P, std::void_t<decltype(O{std::declval<P>(), 0u, 0u})>> : std::true_type {};
static_assert(OpFrom<Op<int32_t>, const int32_t*>::value && OpFrom<Op<int64_t>, const int64_t*>::value, "the detector sees a good list");
static_assert(OpFrom<Op<int32_t>, int32_t*>::value && OpFrom<Op<int64_t>, int64_t*>::value, "output slabs are operands too");
static_assert(!OpFrom<Op<int32_t>, const int64_t*>::value, "no Op<int32_t> from a 64-bit slab");
static_assert(!OpFrom<Op<int64_t>, const int32_t*>::value, "no Op<int64_t> from a 32-bit slab");
static_assert(!OpFrom<Op<int32_t>, const void*>::value && !OpFrom<Op<int64_t>, const void*>::value, "nor from an untyped address");
static_assert(poly_bytes<int64_t>(4, 1) == 32 && poly_bytes<int32_t>(4, 1) == 16, "constexpr byte counts");

int run_coef(const char* path) {
  std::ifstream in(path);
  if (!in) return 2;
  std::string line;
  int64_t wide[2] = {1, 2};
  int32_t narrow[2] = {3, 4};
  while (std::getline(in, line)) {
    if (line.empty()) continue;
    std::istringstream ss(line);
    uint32_t N;
    unsigned long long count;
    if (!(ss >> N >> count)) return 2;
    const bool same64 = (const void*)launch_addr(&wide[1]) == (const void*)&wide[1] && launch_addr(&wide[1])[0] == 2;
    const bool same32 = (const void*)launch_addr(&narrow[1]) == (const void*)&narrow[1];
    std::printf("%zu %zu %d %d\n", poly_bytes<int64_t>(N, (size_t)count), poly_bytes<int32_t>(N, (size_t)count), (int)same64, (int)same32);
  }
  return 0;
}

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
  if (mode == "coef" && argc == 3) return run_coef(argv[2]);
  std::fprintf(stderr, "usage: slab32_driver rules CASES | slab32_driver route CASES | slab32_driver coef CASES\n");
  return 2;
}
