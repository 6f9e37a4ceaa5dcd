// rzk_plan.h — the row-program planner: writes the rows, terms and additions of every protocol phase (ProgId) and
// derives what decides the launch path (flags, row blocks, row groups, units / items / pairs, shared-operand slots,
// traffic counts).  Host-only and pure: a plan is a function of (PlanEnv, id, variant), so it is tested without a GPU
// (tests/test_plan.py).  rzk_run.cpp uploads the tables of a plan and launches what path_of() names.
#pragma once
#include <cstring>
#include <map>
#include <utility>

#include "rzk_dev.h"

namespace rzk {

// table_load (rzk_dev.h) reads these records with scalar loads: they must be naturally aligned inside their tables
static_assert(sizeof(Term) == 8 && sizeof(AddTerm) == 4 && sizeof(Row) == 16 && sizeof(Item) == 16 && sizeof(Unit) == 8,
              "program record sizes");
static_assert(offsetof(Program, rows) % 8 == 0 && offsetof(Program, terms) % 8 == 0 && offsetof(Program, adds) % 4 == 0 &&
                  offsetof(WaveProgram, units) % 8 == 0 && offsetof(WaveProgram, items) % 8 == 0,
              "program record alignment");

enum KeyClass : uint8_t { KC_ZERO = 0, KC_ONE = 1, KC_GENERAL = 2 };

enum ProgId : int {
  PG_MATVEC = 0,      // variant = which*2 + has_addend
  PG_POLYMUL,
  PG_CMUL,            // variant = rows
  PG_OPEN_COMMIT,
  PG_RESPONSE,        // variant = number of (y,r,z) triples sharing d (1 = open, 2 = linear)
  PG_A1_RELATION,     // a1.z - c1(.)d - t == 0   (open / linear / sum verify)
  PG_LIN_COMMIT2,     // variant bit 1 (kMaskVar): the rows that depend on y alone (t, a2.y, t'), no commitment rows
  PG_LIN_U,
  PG_LIN_V1,
  PG_LIN_V2,
  PG_SUM_XP,          // variant = V
  PG_SUM_U,           // variant = V
  PG_SUM_W2,          // variant = V
  PG_SUM_V3,          // variant = V
  PG_COMMIT,          // c = [a1;a2].r + [0;x]                       (commit.rs:88-128)
  PG_COMMIT_VERIFY,   // variant bit 1: opening has a scalar f       (commit.rs:173-210)
  PG_A1Z,             // w = a1.z (n rows), norm predicate on z fused (bit 0)   } the A1 relation in two steps for
  PG_REL_ROT,         // w - c1(.)d - t == 0, all rotations                      } n >= 2: grouped rows + rotations
  PG_SUM_D,           // variant = V: D_c = sum_i g_i(.)v_{i,c} - v'_c for the columns c that a2 uses   } sum_i g_i (a2.v_i) - a2.v'
  PG_SUM_V4,          // a2.D - w2(.)d - u == 0                                                           }   = a2.(sum_i g_i v_i - v')
  PG_LIN_V1B,         // Linear verifier, rearranged: relation rows, e = a2.z - c2(.)d, e' = a2.z' - c2'(.)d   } (a2.z)(.)g - a2.z' - (c2(.)g - c2')(.)d - u
  PG_LIN_V2B,         // g(.)e - e' - u == 0                                                                     }   = g(.)e - e' - u
};

// bit of a program variant: products with the entry's scalar multipliers (g, g_i) take their prepared images (TERM_DKEY)
constexpr uint32_t kDkeyVar = 0x10000u;
constexpr uint32_t kOimgVar = 0x20000u;   // ... and (PG_SUM_D) the other operand's transform from the call's operand images (TERM_DD)
// bit of a program variant: "recover" form of a verifier program.  Every row that tests  lhs - rhs - x == 0  instead stores
// x' = lhs - rhs into the operand the compare form reads x from (the t / t' / u of a short proof, rzk_*_recover_batch);
// the fused norm marks and every other row stay as they are.
constexpr uint32_t kRecoverVar = 0x40000u;
// the verifier programs that have a recover form; any other id with the bit set is kPlanArg.  The non-rearranged Linear
// pair (PG_LIN_V1 / PG_LIN_V2) has none: recover calls run PG_LIN_V1B / PG_LIN_V2B on every context.
inline bool recover_capable(int id) {
  return id == PG_A1_RELATION || id == PG_REL_ROT || id == PG_LIN_V1B || id == PG_LIN_V2B || id == PG_SUM_V3 || id == PG_SUM_V4;
}

// bit of a PG_LIN_COMMIT2 variant: "masks only".  The program keeps the rows of t = a1.y, a2.y and t' = a1.y' (operands 4, 5,
// 8, 9, 10 at their places; 0 .. 3, 6, 7 are not read) and drops the commitment rows: what a prover's retry needs, with y
// transformed once for the a1 and a2 rows.  It has no fused norm check (y carries no norm rule): kMaskVar | 1 is kPlanArg.
constexpr uint32_t kMaskVar = 2u;

constexpr int kPlanOk = 0, kPlanArg = -1, kPlanUnsupported = -4;   // plan_program's status: RZK_OK / RZK_E_ARG / RZK_E_UNSUPPORTED (include/rzk.h)

// everything a plan depends on besides (id, variant)
struct PlanEnv {
  uint32_t n, k, l, logn;
  bool small;                // N < 512: schoolbook kernels, no tables besides the program
  bool rot;                  // challenge products inside mixed rows as rotations, all-challenge programs on shift_row_kernel
  uint32_t block_min_logn;   // row blocks from this ring degree on
  bool use_groups;
  int group_max;             // rows per group of row_group_kernel
  bool use_pairs;            // units may pair rows that share their last operand
  double slot_share_min;     // shared-operand path when (operand transforms) / (distinct operands) >= this
  const uint8_t* key_class;  // (n+l)*k KeyClass values, row-major; only read by programs with key products
  const int32_t* key_entry;  // index into the NTT-domain store, -1 if not GENERAL
  bool dot2 = false;         // units whose row A is exactly two key products are marked ITEM_DOT2 (one reduction for both)
};

struct PlanFacts {
  uint32_t nrows = 0;
  uint32_t nunits = 0;
  uint32_t work = 0;        // steps (item + inverse trips) of one batch entry per prime pass
  bool has_vec = false;
  uint32_t nslots = 0;      // > 0: shared-operand path (fwd_slots_kernel + row_slots_kernel), chosen when rows share enough operands
  uint32_t np_store = 0;
  uint32_t ngroups = 0;     // > 0: row groups (row_group_kernel)
  uint32_t nblocks = 0;     // > 0: row blocks (row_block_kernel): operands of a block staged once in LDS
  bool has_dkey = false;    // products with prepared multiplier images (TERM_DKEY): row_kernel only
  bool has_dd = false;      // ... whose other operand may come from the call's operand images (TERM_DD): row_kernel<.., DD>
  bool shift = false;       // every product has the sparse challenge as multiplier: shift_row_kernel
  bool has_shift = false;   // some rows end with challenge products evaluated by rotations inside row_kernel
  bool two_bit = false;     // two-bit verdict flags (CHECK2 marks)
  // algorithmic traffic of one batch entry (instrumentation): distinct polynomials read per operand index, rows stored
  uint16_t polys_in[kMaxOperands] = {};
  uint32_t polys_out = 0;
};

// About 50 KB: heap-allocate.  A table is meaningful (and uploaded) only when its use_* flag is set; prog always is.
struct Plan {
  Program prog;
  WaveProgram wave;    // units / items of unit_kernel (the default path)
  SlotTable slots;
  BlockPlan blocks;
  bool use_wave, use_slots, use_blocks;
  bool overflow;       // kPlanUnsupported because the shape exceeds the row-program capacity (else: an uncoverable fused check)
  PlanFacts f;
};

// Which launcher evaluates a row program: decided here, once, for the flag preset and for the launch.
enum class Path { Small, Shift, Blocks, Groups, Slots, Rows, Units };
inline Path path_of(const PlanFacts& f, bool small, bool vec_rows) {
  if (small) return Path::Small;
  if (f.shift) return Path::Shift;
  if (f.nblocks) return Path::Blocks;
  if (f.ngroups) return Path::Groups;
  if (f.nslots) return Path::Slots;
  if (f.has_dkey || (f.has_vec && vec_rows)) return Path::Rows;   // row_kernel: vector x vector products, prepared multiplier images
  return Path::Units;
}

// does some row of a2 have an entry in column `col`?  (PG_SUM_D forms, and the operand images keep, only such columns)
inline bool a2_uses_column(const PlanEnv& e, uint32_t col) {
  for (uint32_t j = 0; j < e.l; ++j)
    if (e.key_class[(e.n + j) * e.k + col] != KC_ZERO) return true;
  return false;
}

namespace plan_detail {

using OpOff = std::pair<uint32_t, uint32_t>;   // (operand, offset): one polynomial of a batch entry
inline uint8_t kind_of(const Term& t) { return t.kind & TERM_KIND_MASK; }

// ---- program builder ------------------------------------------------------------------------------------------
struct PB {
  Program& p;
  const PlanEnv& e;
  bool overflow = false;
  bool two_bit = false;      // the program carries CHECK2 marks: two-bit verdict flags (row_kernel only)
  uint32_t sparse_ops = 0;   // bit i: operand i is a challenge (kappa-sparse, +-1): products with it may use shift-add
  int cur = -1;
  void begin_row(uint8_t out_op, uint32_t out_off, uint8_t mode) {
    if (p.nrows >= (uint32_t)kMaxRows) { overflow = true; return; }
    cur = (int)p.nrows++;
    Row& r = p.rows[cur];
    r.term0 = (uint16_t)p.nterms;
    r.add0 = (uint16_t)p.nadds;
    r.nterms = r.nadds = 0;
    r.nshift = r.pad = 0;
    r.out_op = out_op;
    r.out_off = (uint16_t)out_off;
    r.mode = mode;
    if (out_off > 0xffff) overflow = true;
  }
  // sign * A (.) (b_op,b_off), A by kind: TERM_KEY key entry a_off; TERM_DKEY / TERM_DD image a_off of the entry's own
  // multipliers (Operands::dkey_img, row_kernel only); TERM_VEC (a_op,a_off); TERM_SHIFT (a_op,a_off), sparse (the
  // challenge), evaluated as signed rotations inside the row kernel.  Shift terms close a row's term list (stored behind
  // its transform terms, counted in nshift): they may follow other terms and nothing may follow them.
  void term(uint8_t kind, int sign, uint8_t a_op, uint32_t a_off, uint8_t b_op, uint32_t b_off) {
    if (cur < 0 || p.nterms >= (uint32_t)kMaxTerms || a_off > 0xffff || b_off > 0xffff ||
        (kind != TERM_SHIFT && p.rows[cur].nshift)) { overflow = true; return; }
    Term& t = p.terms[p.nterms++];   // (transform terms and shift terms share Program::terms)
    t.kind = kind;
    t.sign = (int8_t)sign;
    t.a_op = a_op;
    t.a_off = (uint16_t)a_off;
    t.b_op = b_op;
    t.b_off = (uint16_t)b_off;
    (kind == TERM_SHIFT ? p.rows[cur].nshift : p.rows[cur].nterms)++;
  }
  // a product with one of the entry's scalar multipliers (operand gop, index idx): its image when the call prepared
  // them (dk), a vector x vector term otherwise; oi: the other operand's transform may come from the call's operand images
  void scalar_term(bool dk, int sign, uint8_t gop, uint32_t idx, uint8_t bop, uint32_t boff, bool oi = false) {
    if (dk) term(oi ? TERM_DD : TERM_DKEY, sign, 0, idx, bop, boff);
    else term(TERM_VEC, sign, bop, boff, gop, idx);
  }
  // product with the challenge: rotations when enabled, transform product otherwise
  void challenge_term(int sign, uint8_t dop, uint8_t bop, uint32_t boff) { term(e.rot ? TERM_SHIFT : TERM_VEC, sign, dop, 0, bop, boff); }
  void add(int sign, uint8_t op, uint32_t off) {
    if (cur < 0 || p.nadds >= (uint32_t)kMaxAdds || off > 0xffff) { overflow = true; return; }
    AddTerm& a = p.adds[p.nadds++];
    a.op = op;
    a.sign = (int8_t)sign;
    a.off = (uint16_t)off;
    p.rows[cur].nadds++;
  }
  // sign * (row `krow` of [a1;a2]) . v, v = operand (vop, voff .. voff+k-1): skips zero entries, turns
  // entries equal to 1 into plain additions (the identity blocks of commit.rs:38-57), products otherwise.
  void key_row(int sign, uint32_t krow, uint8_t vop, uint32_t voff = 0) {
    for (uint32_t j = 0; j < e.k; ++j) {
      const uint32_t idx = krow * e.k + j;
      switch (e.key_class[idx]) {
        case KC_ZERO: break;
        case KC_ONE: add(sign, vop, voff + j); break;
        default: term(TERM_KEY, sign, 0, (uint32_t)e.key_entry[idx], vop, voff + j); break;
      }
    }
  }
  // out[rows] = (rows krow0 .. of [a1;a2]) . v
  void key_rows(uint8_t out_op, uint32_t rows, uint32_t krow0, uint8_t vop) {
    for (uint32_t i = 0; i < rows; ++i) {
      begin_row(out_op, i, MODE_STORE);
      key_row(+1, krow0 + i, vop);
    }
  }
  // out = [a1;a2].r + [0_n ; x]   (commit.rs:109-125)
  void commit_rows(uint8_t out_op, uint8_t r_op, uint8_t x_op) {
    for (uint32_t i = 0; i < e.n + e.l; ++i) {
      begin_row(out_op, i, MODE_STORE);
      key_row(+1, i, r_op);
      if (i >= e.n) add(+1, x_op, i - e.n);
    }
  }
  // a1.z - c1(.)d - t == 0.  c1 = first l rows of c (Commitment::c1_c2 -> split_rows(n), commit.rs:213-218,
  // mat.rs:203-213); Mat::add requires it to have n rows, so n == l is checked by the caller.
  // recover: t_i = (a1.z)_i - (c1(.)d)_i stored instead
  void relation_rows(uint8_t z_op, uint8_t c_op, uint8_t t_op, uint8_t d_op, bool recover = false) {
    for (uint32_t i = 0; i < e.n; ++i) {
      result_row(recover, t_op, i);
      key_row(+1, i, z_op);
      challenge_term(-1, d_op, c_op, i);
      if (!recover) add(-1, t_op, i);
    }
  }
  // a row of a verifier's last step: compared with (x_op, i) by the caller's add(-1, x_op, i), or (recover) stored there
  void result_row(bool recover, uint8_t x_op, uint32_t i) {
    if (recover) begin_row(x_op, i, MODE_STORE);
    else begin_row(0, 0, MODE_ZERO);
  }
  // Fused norm predicate: mark, for each polynomial (vop, 0..count-1), the first load in program order
  // (b operand of a product term, or one of the first four additions of a row).  Returns false when some
  // polynomial is never loaded by the program — the caller then keeps the separate norm kernel.
  bool mark_checks(uint8_t vop, uint32_t count, bool second = false) {
    const uint8_t tmark = second ? TERM_CHECK2 : TERM_CHECK, amark = second ? ADD_CHECK2 : ADD_CHECK;
    if (second) two_bit = true;
    for (uint32_t j = 0; j < count; ++j) {
      bool done = false;
      for (uint32_t r = 0; r < p.nrows && !done; ++r) {
        const Row& row = p.rows[r];
        for (uint32_t t = 0; t < row.nterms && !done; ++t) {
          Term& tm = p.terms[row.term0 + t];
          if (tm.b_op == vop && tm.b_off == j && !(tm.kind & (TERM_CHECK | TERM_CHECK2))) {
            tm.kind |= tmark;
            done = true;
          }
        }
        for (uint32_t a = 0; a < row.nadds && a < 4 && !done; ++a) {
          AddTerm& ad = p.adds[row.add0 + a];
          if ((ad.op & ADD_OP_MASK) == vop && ad.off == j && !(ad.op & (ADD_CHECK | ADD_CHECK2))) {
            ad.op |= amark;
            done = true;
          }
        }
      }
      if (!done) return false;
    }
    return true;
  }
};

inline int build_program(int id, uint32_t var_in, PB& pb) {
  const uint32_t n = pb.e.n, k = pb.e.k, l = pb.e.l;
  const bool dk = (var_in & kDkeyVar) != 0, oi = (var_in & kOimgVar) != 0, rec = (var_in & kRecoverVar) != 0;
  const uint32_t var = var_in & ~(kDkeyVar | kOimgVar | kRecoverVar);
  if (rec && !recover_capable(id)) return kPlanArg;
  bool covered = true;   // a fused-check variant (var & 1) marked every polynomial of its checked vectors
  switch (id) {
    case PG_MATVEC: {   // ops: 0 = v[k], 1 = addend[rows], 2 = out[rows]; which: 0 = a1, 1 = a2, 2 = [a1;a2] (RZK_KEY_*)
      const uint32_t which = var >> 1;
      const bool has_add = var & 1;
      const uint32_t r0 = which == 1 ? n : 0;
      const uint32_t rows = which == 0 ? n : (which == 1 ? l : n + l);
      for (uint32_t i = 0; i < rows; ++i) {
        pb.begin_row(2, i, MODE_STORE);
        pb.key_row(+1, r0 + i, 0);
        if (has_add) pb.add(+1, 1, i);
      }
      break;
    }
    case PG_POLYMUL:   // ops: 0 = a, 1 = b, 2 = out
      pb.begin_row(2, 0, MODE_STORE);
      pb.term(TERM_VEC, +1, 0, 0, 1, 0);
      break;
    case PG_CMUL:      // ops: 0 = m[rows], 1 = p, 2 = out[rows]   (mat.rs:168-178)
      for (uint32_t i = 0; i < var; ++i) {
        pb.begin_row(2, i, MODE_STORE);
        pb.scalar_term(dk, +1, 1, 0, 0, i);
      }
      break;
    case PG_OPEN_COMMIT:   // ops: 0 = x[l], 1 = r[k], 2 = y[k], 3 = c[n+l], 4 = t[n]
      pb.commit_rows(3, 1, 0);    // commit.rs:125: c = [a1;a2].r + [0_n ; x]
      pb.key_rows(4, n, 0, 2);    // open.rs:97: t = a1.y
      if (var & 1) covered = pb.mark_checks(1, k);   // fused check_commit_constraint(r)  (commit.rs:98-107)
      break;
    case PG_COMMIT:   // ops: 0 = x[l], 1 = r[k], 2 = c[n+l]
      pb.commit_rows(2, 1, 0);
      if (var & 1) covered = pb.mark_checks(1, k);   // fused check_commit_constraint(r)  (commit.rs:98-107)
      break;
    case PG_COMMIT_VERIFY:   // ops: 0 = x[l], 1 = r[k], 2 = c[n+l], 3 = f ; flags &= (commit.rs:199-209)
      for (uint32_t i = 0; i < n + l; ++i) {
        pb.begin_row(0, 0, MODE_ZERO);
        pb.key_row(+1, i, 1);
        if (var & 2) {   // a.r + z(.)f - c(.)f == 0
          if (i >= n) pb.term(TERM_VEC, +1, 0, i - n, 3, 0);
          pb.term(TERM_VEC, -1, 2, i, 3, 0);
        } else {         // a.r + z - c == 0
          if (i >= n) pb.add(+1, 0, i - n);
          pb.add(-1, 2, i);
        }
      }
      if (var & 1) covered = pb.mark_checks(1, k);   // fused check_commit_constraint(r)  (commit.rs:183-185)
      break;
    case PG_A1Z:   // ops: 0 = z[k], 1 = w[n]
      pb.key_rows(1, n, 0, 0);
      if (var & 1) covered = pb.mark_checks(0, k);   // fused check_verify_constraint(z)
      break;
    case PG_REL_ROT:   // ops: 0 = w[n] (= a1.z), 1 = t[n], 2 = c[n+l], 3 = d ; flags &= (w == t + c1(.)d)
      pb.sparse_ops = 1u << 3;
      for (uint32_t i = 0; i < n; ++i) {
        pb.result_row(rec, 1, i);
        pb.term(TERM_VEC, -1, 3, 0, 2, i);
        pb.add(+1, 0, i);
        if (!rec) pb.add(-1, 1, i);
      }
      break;
    case PG_RESPONSE:   // ops: 0 = d, then per triple s: 1+3s = y[k], 2+3s = r[k], 3+3s = z[k]
      pb.sparse_ops = 1u << 0;
      for (uint32_t s = 0; s < var; ++s)
        for (uint32_t i = 0; i < k; ++i) {      // open.rs:113-115: z = y + r (.) d
          pb.begin_row((uint8_t)(3 + 3 * s), i, MODE_STORE);
          pb.term(TERM_VEC, +1, 0, 0, (uint8_t)(2 + 3 * s), i);
          pb.add(+1, (uint8_t)(1 + 3 * s), i);
        }
      break;
    case PG_A1_RELATION:   // ops: 0 = z[k], 1 = t[n], 2 = c[n+l], 3 = d ; flags &= (a1.z == t + c1(.)d)
      pb.relation_rows(0, 2, 1, 3, rec);
      if (var & 1) covered = pb.mark_checks(0, k);   // fused check_verify_constraint(z)  (open.rs:167-169)
      break;
    case PG_LIN_COMMIT2:
      // ops: 0 = x[l], 1 = gx[l], 2 = r[k], 3 = rp[k], 4 = y[k], 5 = yp[k],
      //      6 = c[n+l], 7 = cp[n+l], 8 = t[n], 9 = tp[n], 10 = a2y[l]
      if ((var & kMaskVar) && (var & 1)) return kPlanArg;   // no norm rule on y: the masks have no fused-check form
      if (!(var & kMaskVar)) {
        pb.commit_rows(6, 2, 0);   // linear.rs:97: c = commit(x; r)
        pb.commit_rows(7, 3, 1);   // linear.rs:96: cp = commit(g*x; rp)
      }
      pb.key_rows(8, n, 0, 4);     // linear.rs:118
      pb.key_rows(10, l, n, 4);    // a2.y, reduced mod q before it meets g (linear.rs:124-127); next to t = a1.y: the two rows can share the transform of y
      pb.key_rows(9, n, 0, 5);     // linear.rs:121
      if (var & 1) covered = pb.mark_checks(2, k) && pb.mark_checks(3, k, true);   // fused check_commit_constraint: r -> bit 0, rp -> bit 1 of ok (linear.rs:96-97)
      break;
    case PG_LIN_U:   // ops: 0 = a2y[l], 1 = g, 2 = yp[k], 3 = u[l] : u = a2y(.)g - a2.yp (linear.rs:124-129)
      for (uint32_t i = 0; i < l; ++i) {
        pb.begin_row(3, i, MODE_STORE);
        pb.scalar_term(dk, +1, 1, 0, 0, i);
        pb.key_row(-1, n + i, 2);
      }
      break;
    case PG_LIN_V1:
      // ops: 0 = z[k], 1 = zp[k], 2 = t[n], 3 = tp[n], 4 = c[n+l], 5 = cp[n+l], 6 = d, 7 = g,
      //      8 = w1[l] (a2.z), 9 = w2[l] (c2(.)g - c2p)
      pb.relation_rows(0, 4, 2, 6);            // linear.rs:225-229
      pb.relation_rows(1, 5, 3, 6);            // linear.rs:231-235
      pb.key_rows(8, l, n, 0);                 // a2.z (linear.rs:238-241), reduced before (.)g
      for (uint32_t i = 0; i < l; ++i) {       // c2(.)g - c2p (linear.rs:243-246); c2 = last n rows of c
        pb.begin_row(9, i, MODE_STORE);
        pb.scalar_term(dk, +1, 7, 0, 4, l + i);
        pb.add(-1, 5, l + i);
      }
      if (var & 1) covered = pb.mark_checks(0, k) && pb.mark_checks(1, k);   // fused check_verify_constraint(z), (zp)  (linear.rs:218-223)
      break;
    case PG_LIN_V1B:
      // ops: 0 = z[k], 1 = zp[k], 2 = t[n], 3 = tp[n], 4 = c[n+l], 5 = cp[n+l], 6 = d, 7 = e[l], 8 = ep[l]
      // linear.rs:237-249 reads (a2.z)(.)g - a2.z' == (c2(.)g - c2')(.)d + u; in a commutative ring that is
      // g(.)(a2.z - c2(.)d) - (a2.z' - c2'(.)d) - u == 0: one product with g instead of two, and none in this program
      pb.relation_rows(0, 4, 2, 6, rec);       // linear.rs:225-229
      pb.relation_rows(1, 5, 3, 6, rec);       // linear.rs:231-235
      for (uint32_t s = 0; s < 2; ++s)         // e = a2.z - c2(.)d, then e' = a2.z' - c2'(.)d ; c2 = last n rows of c
        for (uint32_t i = 0; i < l; ++i) {
          pb.begin_row((uint8_t)(7 + s), i, MODE_STORE);
          pb.key_row(+1, n + i, (uint8_t)s);
          pb.challenge_term(-1, 6, (uint8_t)(4 + s), l + i);
        }
      if (var & 1) covered = pb.mark_checks(0, k) && pb.mark_checks(1, k);   // fused check_verify_constraint(z), (zp)  (linear.rs:218-223)
      break;
    case PG_LIN_V2B:   // ops: 0 = e[l], 1 = ep[l], 2 = g, 3 = u[l] : g(.)e - e' - u == 0
      for (uint32_t i = 0; i < l; ++i) {
        pb.result_row(rec, 3, i);
        pb.scalar_term(dk, +1, 2, 0, 0, i);
        pb.add(-1, 1, i);
        if (!rec) pb.add(-1, 3, i);
      }
      break;
    case PG_LIN_V2:
      // ops: 0 = w1[l], 1 = w2[l], 2 = g, 3 = d, 4 = zp[k], 5 = u[l]
      // w1(.)g - a2.zp - w2(.)d - u == 0   (linear.rs:237-249)
      for (uint32_t i = 0; i < l; ++i) {
        pb.begin_row(0, 0, MODE_ZERO);
        pb.scalar_term(dk, +1, 2, 0, 0, i);
        pb.key_row(-1, n + i, 4);
        pb.challenge_term(-1, 3, 1, i);
        pb.add(-1, 5, i);
      }
      break;
    case PG_SUM_XP:   // ops: 0 = xs[V*l], 1 = gs[V], 2 = xp[l] : xp = sum_i x_i (.) g_i (sum.rs:107-115)
      for (uint32_t j = 0; j < l; ++j) {
        pb.begin_row(2, j, MODE_STORE);
        for (uint32_t i = 0; i < var; ++i) pb.scalar_term(dk, +1, 1, i, 0, i * l + j);
      }
      break;
    case PG_SUM_U:    // ops: 0 = w[V*l] (a2.y_i), 1 = gs[V], 2 = yp[k], 3 = u[l]   (sum.rs:154-160)
      for (uint32_t j = 0; j < l; ++j) {
        pb.begin_row(3, j, MODE_STORE);
        for (uint32_t i = 0; i < var; ++i) pb.scalar_term(dk, +1, 1, i, 0, i * l + j);
        pb.key_row(-1, n + j, 2);
      }
      break;
    case PG_SUM_W2:   // ops: 0 = cs[V*(n+l)], 1 = gs[V], 2 = cp[n+l], 3 = w2[l] : sum_i c2_i(.)g_i - c2p (sum.rs:309-316)
      for (uint32_t j = 0; j < l; ++j) {
        pb.begin_row(3, j, MODE_STORE);
        for (uint32_t i = 0; i < var; ++i) pb.scalar_term(dk, +1, 1, i, 0, i * (n + l) + l + j);
        pb.add(-1, 2, l + j);
      }
      break;
    case PG_SUM_V3:   // ops: 0 = w1[V*l] (a2.z_i), 1 = gs[V], 2 = zp[k], 3 = w2[l], 4 = d, 5 = u[l]   (sum.rs:301-319)
      for (uint32_t j = 0; j < l; ++j) {
        pb.result_row(rec, 5, j);
        for (uint32_t i = 0; i < var; ++i) pb.scalar_term(dk, +1, 1, i, 0, i * l + j);
        pb.key_row(-1, n + j, 2);
        pb.challenge_term(-1, 4, 3, j);
        if (!rec) pb.add(-1, 5, j);
      }
      break;
    case PG_SUM_D:    // ops: 0 = vs[V*k] (ys or zs), 1 = gs[V], 2 = vp[k] (yp or zp), 3 = D[k]
      // a2 is linear and the ring commutative: sum_i g_i (.) (a2.v_i) - a2.v' = a2.(sum_i g_i (.) v_i - v')
      // (sum.rs:154-160 and 301-308); only the columns a2 has entries in are formed
      for (uint32_t col = 0; col < k; ++col) {
        if (!a2_uses_column(pb.e, col)) continue;
        pb.begin_row(3, col, MODE_STORE);
        for (uint32_t i = 0; i < var; ++i) pb.scalar_term(dk, +1, 1, i, 0, i * k + col, oi);
        pb.add(-1, 2, col);
      }
      break;
    case PG_SUM_V4:   // ops: 0 = D[k], 1 = w2[l], 2 = d, 3 = u[l] : a2.D - w2(.)d - u == 0   (sum.rs:301-319)
      for (uint32_t j = 0; j < l; ++j) {
        pb.result_row(rec, 3, j);
        pb.key_row(+1, n + j, 0);
        pb.challenge_term(-1, 2, 1, j);
        if (!rec) pb.add(-1, 3, j);
      }
      break;
    default: return kPlanArg;
  }
  return covered ? kPlanOk : kPlanUnsupported;
}

// ---- the four table passes: each reads the finished program and fills its table --------------------------------
// Row blocks: consecutive rows of a key-only program are packed into blocks of at most kBlockMaxRows rows and
// kBlockMaxSlots distinct operands.  True when the plan fits and every operand is needed by at least two terms on
// average (otherwise nothing is shared and the plain row kernel is as good).
inline bool plan_blocks(const Program& p, bool key_only, BlockPlan& bp) {
  bool fits = key_only;
  std::map<OpOff, uint32_t> cur;   // (op, off) -> slot of the open block
  auto open_block = [&](uint32_t row) {
    bp.blk[bp.nblocks].row0 = (uint16_t)row;
    bp.blk[bp.nblocks].nrows = 0;
    bp.blk[bp.nblocks].slot0 = (uint16_t)bp.nslots_total;
    bp.blk[bp.nblocks].nslots = 0;
    cur.clear();
  };
  if (fits) open_block(0);
  for (uint32_t r = 0; fits && r < p.nrows; ++r) {
    const Row& row = p.rows[r];
    std::map<OpOff, uint32_t> add;   // operands this row brings that the block lacks
    for (uint32_t t = 0; t < row.nterms; ++t) {
      const Term& tm = p.terms[row.term0 + t];
      if (!cur.count({tm.b_op, tm.b_off})) add[{tm.b_op, tm.b_off}] = 0;
    }
    BlockDesc* bd = &bp.blk[bp.nblocks];
    if (bd->nrows == kBlockMaxRows || bd->nslots + add.size() > (size_t)kBlockMaxSlots) {
      if (bd->nrows == 0) { fits = false; break; }   // a single row needs more operands than LDS holds
      ++bp.nblocks;
      if (bp.nblocks >= (uint32_t)kMaxRows) { fits = false; break; }
      open_block(r);
      bd = &bp.blk[bp.nblocks];
      add.clear();
      for (uint32_t t = 0; t < row.nterms; ++t) add[{p.terms[row.term0 + t].b_op, p.terms[row.term0 + t].b_off}] = 0;
      if (add.size() > (size_t)kBlockMaxSlots) { fits = false; break; }
    }
    for (auto& kv : add) {
      if (bp.nslots_total >= (uint32_t)kMaxSlots) { fits = false; break; }
      const uint32_t sidx = bd->nslots++;
      cur[kv.first] = sidx;
      bp.slot_op[bp.nslots_total] = (uint16_t)kv.first.first;
      bp.slot_off[bp.nslots_total] = (uint16_t)kv.first.second;
      ++bp.nslots_total;
    }
    for (uint32_t t = 0; fits && t < row.nterms; ++t) {
      const Term& tm = p.terms[row.term0 + t];
      const uint32_t sidx = cur[{tm.b_op, tm.b_off}];
      bp.term_slot[row.term0 + t] = (uint16_t)sidx;
      if (tm.kind & TERM_CHECK) bp.slot_check[bd->slot0 + sidx] = 1;
    }
    bd->nrows++;
  }
  if (!fits) return false;
  ++bp.nblocks;
  return bp.nslots_total > 0 && (double)p.nterms / bp.nslots_total >= 2.0;
}

// Row groups: consecutive rows that are key products over the same operand list are evaluated by one wavefront
// (row_group_kernel).  Writes Program::groups; returns their number when grouping at least halves the number of
// tasks, 0 (no groups) otherwise.
inline uint32_t plan_groups(Program& p, uint32_t gmax) {
  uint32_t ng = 0;
  for (uint32_t r = 0; r < p.nrows;) {
    uint32_t cnt = 1;
    const Row& r0 = p.rows[r];
    while (cnt < gmax && r + cnt < p.nrows) {
      const Row& rr = p.rows[r + cnt];
      bool same = rr.nterms == r0.nterms && r0.nterms > 0;
      for (uint32_t t = 0; same && t < r0.nterms; ++t) {
        const Term& a = p.terms[r0.term0 + t];
        const Term& b2 = p.terms[rr.term0 + t];
        same = a.b_op == b2.b_op && a.b_off == b2.b_off;
      }
      if (!same) break;
      ++cnt;
    }
    p.groups[ng].row0 = (uint16_t)r;
    p.groups[ng].count = (uint16_t)cnt;
    ++ng;
    r += cnt;
  }
  return ng * 2 <= p.nrows ? ng : 0;
}

// Wave program of unit_kernel: one unit per row; two consecutive rows become a PAIR when the second has exactly
// one key product and its operand is the last operand of the first (c0 / c1 of a commitment share r_{k-1};
// t = a1.y and a2.y share y_{k-1}): that transform is then computed once for both.  Returns the work per entry.
// dot2: a unit of exactly two items, both key products into row A, is marked ITEM_DOT2 on both (with or without a row B).
inline uint32_t plan_units(const Program& p, bool use_pairs, WaveProgram& wp, bool dot2 = false) {
  auto key_only = [&](const Row& rr) {
    for (uint32_t t = 0; t < rr.nterms; ++t)
      if (kind_of(p.terms[rr.term0 + t]) != TERM_KEY) return false;
    return true;
  };
  uint32_t work = 0;
  for (uint32_t r = 0; r < p.nrows;) {
    const Row& ra = p.rows[r];
    Unit& un = wp.units[wp.nunits++];
    un.rowA = (uint16_t)r;
    un.rowB = kNoRow;
    un.item0 = (uint16_t)wp.nitems;
    un.nitems = ra.nterms;
    for (uint32_t t = 0; t < ra.nterms; ++t) {
      const Term& tm = p.terms[ra.term0 + t];
      Item& im = wp.items[wp.nitems++];
      im.kind = kind_of(tm) == TERM_VEC ? ITEM_VEC : ITEM_KEY;
      im.flags = tm.kind & (TERM_CHECK | TERM_CHECK2);
      im.b_op = tm.b_op;
      im.b_off = tm.b_off;
      im.a_op = tm.a_op;
      im.a_off = tm.a_off;
      im.keyA = im.kind == ITEM_KEY ? tm.a_off : 0;
      im.keyB = kNoKey;
      im.signA = tm.sign;
      im.signB = 0;
    }
    uint32_t step = 1;
    if (use_pairs && r + 1 < p.nrows && ra.nterms >= 1 && ra.nshift == 0 && key_only(ra)) {
      const Row& rb = p.rows[r + 1];
      if (rb.nterms == 1 && rb.nshift == 0 && key_only(rb)) {
        const Term& tb = p.terms[rb.term0];
        const Term& ta = p.terms[ra.term0 + ra.nterms - 1];
        if (tb.b_op == ta.b_op && tb.b_off == ta.b_off) {
          Item& im = wp.items[wp.nitems - 1];
          im.keyB = tb.a_off;
          im.signB = tb.sign;
          im.flags |= tb.kind & (TERM_CHECK | TERM_CHECK2);
          un.rowB = (uint16_t)(r + 1);
          step = 2;
        }
      }
    }
    if (dot2 && un.nitems == 2) {
      Item* two = &wp.items[un.item0];
      if (two[0].kind == ITEM_KEY && two[1].kind == ITEM_KEY && two[0].keyA != kNoKey && two[1].keyA != kNoKey)
        two[0].flags |= ITEM_DOT2, two[1].flags |= ITEM_DOT2;
    }
    work += (un.nitems ? un.nitems : 1u) + (un.rowB != kNoRow ? 2u : 1u);
    r += step;
  }
  return work;
}

// Distinct operands of the product terms ("slots"): when rows share them often enough, each is transformed once per
// proof (shared-operand path) instead of once per row.  True when the table fits and the sharing reaches share_min.
inline bool plan_slots(const Program& p, double share_min, SlotTable& st) {
  std::map<OpOff, uint32_t> index;
  bool fits = true;
  uint32_t transforms = 0;
  auto slot_of = [&](uint8_t op, uint16_t off) -> uint32_t {
    auto it = index.find({op, off});
    if (it != index.end()) return it->second;
    if (st.nslots >= (uint32_t)kMaxSlots) { fits = false; return 0; }
    const uint32_t sidx = st.nslots++;
    st.op[sidx] = op;
    st.off[sidx] = off;
    index[{op, off}] = sidx;
    return sidx;
  };
  for (uint32_t t = 0; t < p.nterms; ++t) {
    const Term& tm = p.terms[t];
    const uint32_t sb = slot_of(tm.b_op, tm.b_off);
    st.term_b[t] = (uint16_t)sb;
    ++transforms;
    if (tm.kind & TERM_CHECK) st.check[sb] = 1;
    if (kind_of(tm) == TERM_VEC) {
      st.term_a[t] = (uint16_t)slot_of(tm.a_op, tm.a_off);
      ++transforms;
    }
  }
  return fits && st.nslots > 0 && (double)transforms / st.nslots >= share_min;
}

// distinct polynomials read per operand index, rows stored
inline void count_traffic(const Program& p, PlanFacts& f) {
  std::map<OpOff, int> seen;
  auto touch = [&](uint32_t op, uint32_t off) {
    if (op < (uint32_t)kMaxOperands && !seen.count({op, off})) {
      seen[{op, off}] = 1;
      f.polys_in[op]++;
    }
  };
  for (uint32_t r = 0; r < p.nrows; ++r) {
    const Row& row = p.rows[r];
    for (uint32_t t = 0; t < (uint32_t)row.nterms + row.nshift; ++t) {
      const Term& tm = p.terms[row.term0 + t];
      touch(tm.b_op, tm.b_off);
      if (kind_of(tm) != TERM_KEY) touch(tm.a_op, tm.a_off);
    }
    for (uint32_t a = 0; a < row.nadds; ++a) touch(p.adds[row.add0 + a].op & ADD_OP_MASK, p.adds[row.add0 + a].off);
    if (row.mode == MODE_STORE) f.polys_out++;
  }
}

}  // namespace plan_detail

// The plan of program (id, var) under env.  kPlanOk; kPlanUnsupported for a fused-check variant that cannot cover every
// polynomial, or (plan.overflow) for a shape beyond the row-program capacity; kPlanArg for an unknown id.
inline int plan_program(const PlanEnv& env, int id, uint32_t var, Plan& plan) {
  using namespace plan_detail;
  std::memset(&plan.prog, 0, sizeof(plan.prog));
  std::memset(&plan.wave, 0, sizeof(plan.wave));
  std::memset(&plan.slots, 0, sizeof(plan.slots));
  std::memset(&plan.blocks, 0, sizeof(plan.blocks));
  plan.use_wave = plan.use_slots = plan.use_blocks = plan.overflow = false;
  plan.f = PlanFacts{};
  Program& p = plan.prog;
  PlanFacts& f = plan.f;
  PB pb{p, env};
  const int rc = build_program(id, var, pb);
  if (rc != kPlanOk) return rc;
  plan.overflow = pb.overflow;
  if (pb.overflow) return kPlanUnsupported;
  // one pass over the terms: what kinds there are, and whether every product is a plain (unchecked) vector x vector
  // term with a sparse multiplier
  bool key_only = p.nterms > 0, all_sparse = p.nterms > 0;
  for (uint32_t t = 0; t < p.nterms; ++t) {
    const Term& tm = p.terms[t];
    const uint8_t kind = kind_of(tm);
    key_only = key_only && kind == TERM_KEY;
    all_sparse = all_sparse && tm.kind == TERM_VEC && ((pb.sparse_ops >> tm.a_op) & 1u);
    f.has_vec = f.has_vec || kind == TERM_VEC;
    f.has_shift = f.has_shift || kind == TERM_SHIFT;
    f.has_dd = f.has_dd || kind == TERM_DD;
    f.has_dkey = f.has_dkey || kind == TERM_DKEY || kind == TERM_DD;
  }
  f.shift = env.rot && pb.sparse_ops && all_sparse;
  f.two_bit = pb.two_bit;
  f.nrows = p.nrows;
  // precedence: blocks before groups before slots
  if (!env.small && env.logn >= 10 && env.logn >= env.block_min_logn && !f.shift && !f.has_shift && !f.two_bit &&
      !f.has_dkey && p.nterms > 0) {
    plan.use_blocks = plan_blocks(p, key_only, plan.blocks);
    if (plan.use_blocks) f.nblocks = plan.blocks.nblocks;
  }
  if (!env.small && env.use_groups && !f.shift && !f.two_bit && !f.nblocks && !f.has_dkey && key_only)
    p.ngroups = f.ngroups = plan_groups(p, (uint32_t)env.group_max);
  if (!env.small) {
    plan.use_wave = true;
    f.work = plan_units(p, env.use_pairs, plan.wave, env.dot2);
    f.nunits = plan.wave.nunits;
  }
  if (!env.small && env.slot_share_min > 0 && p.nterms > 0 && f.ngroups == 0 && !f.shift && !f.has_shift &&
      !f.two_bit && !f.nblocks && !f.has_dkey) {
    plan.use_slots = plan_slots(p, env.slot_share_min, plan.slots);
    if (plan.use_slots) {
      f.nslots = plan.slots.nslots;
      f.np_store = f.has_vec ? 3 : 2;
    }
  }
  count_traffic(p, f);
  return kPlanOk;
}

}  // namespace rzk
