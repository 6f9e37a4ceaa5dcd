// Host driver of the row-program planner (ring_zk_amd/csrc/rzk_plan.h) for tests/test_plan.py.
//   plan_driver sha  TEXT          SHA-256 of TEXT (checks sha256.h against hashlib)
//   plan_driver plan CASES [full]  one JSON line per case: status, facts, path, digests of the tables in use;
//                                  with `full` also the tables themselves
// A case is a line  "n k l logn small rot block_min_logn use_groups group_max use_pairs slot_share_min vec_rows id var key"
// where key is the (n+l)*k KeyClass digits in row-major order, or "-" for a context without a key.  An optional last field
// gives the (n+l)*k key_entry values, comma separated, for tables that no key load numbers (tests/test_keyplan_host.py:
// what a refused load used to leave behind); without it the general entries are numbered as rzk_key_load numbers them.
#include <cstdio>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../ring_zk_amd/csrc/rzk_plan.h"
#include "sha256.h"

using namespace rzk;

namespace {

struct Json {
  std::string s = "{";
  void key(const char* k) {
    if (s.size() > 1) s += ",";
    s += std::string("\"") + k + "\":";
  }
  void num(const char* k, long long v) { key(k); s += std::to_string(v); }
  void str(const char* k, const std::string& v) { key(k); s += "\"" + v + "\""; }
  void null(const char* k) { key(k); s += "null"; }
  template <class T, class F>
  void list(const char* k, const T* a, size_t n, F each) {   // each(record) -> "[...]" or a number
    key(k);
    s += "[";
    for (size_t i = 0; i < n; ++i) s += (i ? "," : "") + each(a[i]);
    s += "]";
  }
};

template <class... Ts>
std::string tup(Ts... v) {
  std::string out = "[";
  bool first = true;
  for (long long x : {(long long)v...}) {
    out += (first ? "" : ",") + std::to_string(x);
    first = false;
  }
  return out + "]";
}

void tables(Json& j, const Plan& pl) {
  const Program& p = pl.prog;
  j.num("prog_ngroups", p.ngroups);
  j.list("rows", p.rows, p.nrows, [](const Row& r) { return tup(r.term0, r.nterms, r.add0, r.nadds, r.out_op, r.mode, r.out_off, r.nshift); });
  j.list("terms", p.terms, p.nterms, [](const Term& t) { return tup(t.kind, t.sign, t.a_op, t.b_op, t.a_off, t.b_off); });
  j.list("adds", p.adds, p.nadds, [](const AddTerm& a) { return tup(a.op, a.sign, a.off); });
  j.list("groups", p.groups, p.ngroups, [](const GroupDesc& g) { return tup(g.row0, g.count); });
  if (pl.use_wave) {
    j.list("units", pl.wave.units, pl.wave.nunits, [](const Unit& u) { return tup(u.rowA, u.rowB, u.item0, u.nitems); });
    j.list("items", pl.wave.items, pl.wave.nitems, [](const Item& i) {
      return tup(i.kind, i.flags, i.b_op, i.a_op, i.b_off, i.a_off, i.keyA, i.keyB, i.signA, i.signB);
    });
  }
  if (pl.use_slots) {
    const SlotTable& st = pl.slots;
    std::vector<uint32_t> idx(st.nslots), tix(p.nterms);
    for (uint32_t i = 0; i < st.nslots; ++i) idx[i] = i;
    for (uint32_t i = 0; i < p.nterms; ++i) tix[i] = i;
    j.list("slots", idx.data(), idx.size(), [&](uint32_t i) { return tup(st.op[i], st.off[i], st.check[i]); });
    j.list("term_ab", tix.data(), tix.size(), [&](uint32_t t) { return tup(st.term_a[t], st.term_b[t]); });
  }
  if (pl.use_blocks) {
    const BlockPlan& bp = pl.blocks;
    std::vector<uint32_t> idx(bp.nslots_total), tix(p.nterms);
    for (uint32_t i = 0; i < bp.nslots_total; ++i) idx[i] = i;
    for (uint32_t i = 0; i < p.nterms; ++i) tix[i] = i;
    j.list("blocks", bp.blk, bp.nblocks, [](const BlockDesc& b) { return tup(b.row0, b.nrows, b.slot0, b.nslots); });
    j.list("block_slots", idx.data(), idx.size(), [&](uint32_t i) { return tup(bp.slot_op[i], bp.slot_off[i], bp.slot_check[i]); });
    j.list("term_slot", tix.data(), tix.size(), [&](uint32_t t) { return std::to_string(bp.term_slot[t]); });
  }
}

int run_cases(const char* path, bool full) {
  std::ifstream in(path);
  if (!in) return 2;
  std::unique_ptr<Plan> plan(new Plan);
  std::string line;
  while (std::getline(in, line)) {
    if (line.empty()) continue;
    std::istringstream ss(line);
    PlanEnv e{};
    int small, rot, use_groups, use_pairs, vec_rows, id;
    uint32_t var;
    std::string key;
    if (!(ss >> e.n >> e.k >> e.l >> e.logn >> small >> rot >> e.block_min_logn >> use_groups >> e.group_max >> use_pairs >>
          e.slot_share_min >> vec_rows >> id >> var >> key)) {
      std::fprintf(stderr, "bad case line: %s\n", line.c_str());
      return 2;
    }
    e.small = small != 0;
    e.rot = rot != 0;
    e.use_groups = use_groups != 0;
    e.use_pairs = use_pairs != 0;
    std::vector<uint8_t> key_class;
    std::vector<int32_t> key_entry;
    if (key != "-") {
      if (key.size() != (size_t)(e.n + e.l) * e.k) {
        std::fprintf(stderr, "key of %zu entries for (%u,%u,%u)\n", key.size(), e.n, e.k, e.l);
        return 2;
      }
      int32_t general = 0;   // as rzk_key_load numbers them: in row-major order
      for (char ch : key) {
        key_class.push_back((uint8_t)(ch - '0'));
        key_entry.push_back(ch - '0' == KC_GENERAL ? general++ : -1);
      }
      std::string given;
      if (ss >> given) {
        std::istringstream es(given);
        std::string tok;
        key_entry.clear();
        while (std::getline(es, tok, ',')) key_entry.push_back((int32_t)std::stol(tok));
        if (key_entry.size() != key_class.size()) {
          std::fprintf(stderr, "%zu key_entry values for %zu entries\n", key_entry.size(), key_class.size());
          return 2;
        }
      }
    }
    e.key_class = key_class.data();
    e.key_entry = key_entry.data();
    const int rc = plan_program(e, id, var, *plan);
    Json j;
    j.num("status", rc);
    if (rc == kPlanOk) {
      const PlanFacts& f = plan->f;
      j.num("nrows", f.nrows); j.num("nunits", f.nunits); j.num("work", f.work); j.num("has_vec", f.has_vec);
      j.num("nslots", f.nslots); j.num("np_store", f.np_store); j.num("ngroups", f.ngroups); j.num("nblocks", f.nblocks);
      j.num("has_dkey", f.has_dkey); j.num("has_dd", f.has_dd); j.num("shift", f.shift); j.num("has_shift", f.has_shift);
      j.num("two_bit", f.two_bit); j.num("polys_out", f.polys_out);
      j.list("polys_in", f.polys_in, (size_t)kMaxOperands, [](uint16_t v) { return std::to_string(v); });
      bool paired = false;
      for (uint32_t u = 0; plan->use_wave && u < plan->wave.nunits; ++u) paired = paired || plan->wave.units[u].rowB != kNoRow;
      j.num("paired", paired);
      j.str("sha_program", sha256::hex(&plan->prog, sizeof(Program)));
      plan->use_wave ? j.str("sha_wave", sha256::hex(&plan->wave, sizeof(WaveProgram))) : j.null("sha_wave");
      plan->use_slots ? j.str("sha_slots", sha256::hex(&plan->slots, sizeof(SlotTable))) : j.null("sha_slots");
      plan->use_blocks ? j.str("sha_blocks", sha256::hex(&plan->blocks, sizeof(BlockPlan))) : j.null("sha_blocks");
      j.num("path", (int)path_of(f, e.small, vec_rows != 0));
      if (full) tables(j, *plan);
    } else {
      j.num("overflow", plan->overflow);
    }
    std::printf("%s}\n", j.s.c_str());
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "sha" && argc == 3) {
    const std::string text = argv[2];
    std::printf("%s\n", sha256::hex(text.data(), text.size()).c_str());
    return 0;
  }
  if (mode == "plan" && argc >= 3) return run_cases(argv[2], argc > 3 && std::string(argv[3]) == "full");
  std::fprintf(stderr, "usage: plan_driver sha TEXT | plan_driver plan CASES [full]\n");
  return 2;
}
