// rzk_slabs.h — what the slabs of a protocol-level entry point of the C ABI are (include/rzk.h), stated once: how many
// polynomials per proof every kind of slab holds, and for every entry point the ordered list of its slabs and byte-sized
// companions — name, kind and role, in the order of the C declaration.  The NULL test, the alignment test, the staging
// plan of the host form and the convert plan of a 32-bit call are derived from a call's list by the glue in rzk_ctx.h;
// the prover loops take their row counts from it.  Host-only and pure (no HIP header): tests/test_slabs_host.py holds
// the table against the declarations of include/rzk.h without a GPU.
#pragma once
#include <cstddef>
#include <cstdint>

namespace rzk {

// rows of the key part a selector names (RZK_KEY_A1 / RZK_KEY_A2 / RZK_KEY_A = 0 / 1 / 2); 0: not a selector
constexpr uint32_t key_row_count(int which, uint32_t n, uint32_t l) {
  return which == 0 ? n : which == 1 ? l : which == 2 ? n + l : 0;
}
constexpr bool is_key_selector(int which) { return which >= 0 && which <= 2; }

// the context's shape and the call's own size arguments: V summands (Sum), `rows` polynomials of a free-size operand
// (the rows argument of cmul / norm2_le / eq / eq32; key_row_count(which) for matvec)
struct SlabDims {
  uint64_t n, k, l, V, rows;
};

enum SlabKind : uint8_t {
  // coefficient slabs: polynomials per proof
  SK_X,      // a message x: l
  SK_RYZ,    // commitment randomness r, mask y, response z: k
  SK_C,      // a commitment c: n + l
  SK_T,      // t = a1.y: n
  SK_U,      // u: l
  SK_GD,     // a multiplier g, a challenge d, the scalar f of an opening, one polynomial of a count-sized call: 1
  SK_ROWS,   // a free-size operand: SlabDims::rows
  SK_SUM = 8,   // | SK_SUM: the V summands of a Sum proof, V times the kind
  // byte-sized companions: bytes per proof
  SK_FLAG = 16,   // ok / accept / eq / rounds: 1
  SK_WORD,        // coin, E: 8
};
constexpr SlabKind sum_of(SlabKind kind) { return (SlabKind)(kind | SK_SUM); }
constexpr bool slab_is_coef(SlabKind kind) { return kind < SK_FLAG; }
// polynomials per proof of a coefficient slab, bytes per proof of a companion
constexpr uint64_t slab_count(SlabKind kind, const SlabDims& d) {
  if (kind == SK_FLAG) return 1;
  if (kind == SK_WORD) return 8;
  const uint64_t one = (kind & 7) == SK_X ? d.l : (kind & 7) == SK_RYZ ? d.k : (kind & 7) == SK_C ? d.n + d.l
                     : (kind & 7) == SK_T ? d.n : (kind & 7) == SK_U ? d.l : (kind & 7) == SK_GD ? 1 : d.rows;
  return (kind & SK_SUM) ? d.V * one : one;
}

enum SlabRole : uint8_t { SR_IN, SR_OUT, SR_IN_OPT, SR_OUT_OPT };   // read / written; _OPT: may be NULL
constexpr bool slab_reads(SlabRole r) { return r == SR_IN || r == SR_IN_OPT; }
constexpr bool slab_optional(SlabRole r) { return r == SR_IN_OPT || r == SR_OUT_OPT; }

struct Slab {
  const char* name;   // the parameter's name in include/rzk.h; NULL ends a list
  SlabKind kind;
  SlabRole role;
};
constexpr Slab rd(const char* name, SlabKind kind) { return {name, kind, SR_IN}; }
constexpr Slab wr(const char* name, SlabKind kind) { return {name, kind, SR_OUT}; }
constexpr Slab rd_opt(const char* name, SlabKind kind) { return {name, kind, SR_IN_OPT}; }
constexpr Slab wr_opt(const char* name, SlabKind kind) { return {name, kind, SR_OUT_OPT}; }

constexpr int kMaxCallSlabs = 14;
struct CallSlabs {
  const char* call;   // rzk_<call>_batch and rzk_<call>_batch_dev
  bool both_widths;   // rzk_<call>32_batch(_dev) exist too: the same list on int32_t coefficient slabs
  Slab s[kMaxCallSlabs];
};
constexpr size_t slab_len(const CallSlabs& c) {
  size_t n = 0;
  while (n < (size_t)kMaxCallSlabs && c.s[n].name) ++n;
  return n;
}

// The lists: constexpr objects of internal linkage (the library exports nothing of them), usable as template arguments.
// ---- ring / Mat primitives (polymul, add, sub, canonicalize, narrow, widen: one polynomial per entry of `count`) ----------
constexpr CallSlabs kSlabsPolymul = {"polymul", false, {rd("a", SK_GD), rd("b", SK_GD), wr("out", SK_GD)}};
constexpr CallSlabs kSlabsAdd = {"add", false, {rd("a", SK_GD), rd("b", SK_GD), wr("out", SK_GD)}};
constexpr CallSlabs kSlabsSub = {"sub", false, {rd("a", SK_GD), rd("b", SK_GD), wr("out", SK_GD)}};
constexpr CallSlabs kSlabsCanonicalize = {"canonicalize", false, {rd("in", SK_GD), wr("out", SK_GD)}};
constexpr CallSlabs kSlabsNarrow = {"narrow", false, {rd("in", SK_GD), wr("out", SK_GD)}};
constexpr CallSlabs kSlabsWiden = {"widen", false, {rd("in", SK_GD), wr("out", SK_GD)}};
constexpr CallSlabs kSlabsMatvec = {"matvec", true, {rd("v", SK_RYZ), rd_opt("addend", SK_ROWS), wr("out", SK_ROWS)}};
constexpr CallSlabs kSlabsCmul = {"cmul", false, {rd("m", SK_ROWS), rd("p", SK_GD), wr("out", SK_ROWS)}};
constexpr CallSlabs kSlabsNorm2Le = {"norm2_le", true, {rd("v", SK_ROWS), wr("ok", SK_FLAG)}};
constexpr CallSlabs kSlabsEq = {"eq", false, {rd("a", SK_ROWS), rd("b", SK_ROWS), wr("eq", SK_FLAG)}};
constexpr CallSlabs kSlabsEq32 = {"eq32", false, {rd("a", SK_ROWS), rd("b", SK_ROWS), wr("eq", SK_FLAG)}};
// ---- commitment scheme ------------------------------------------------------------------------------------------------
constexpr CallSlabs kSlabsCommit = {"commit", false, {rd("x", SK_X), rd("r", SK_RYZ), wr("c", SK_C), wr_opt("ok", SK_FLAG)}};
constexpr CallSlabs kSlabsCommitmentVerify = {
    "commitment_verify", false, {rd("c", SK_C), rd("x", SK_X), rd("r", SK_RYZ), rd_opt("f", SK_GD), wr("ok", SK_FLAG)}};
// ---- Open ---------------------------------------------------------------------------------------------------------------
constexpr CallSlabs kSlabsOpenCommit = {
    "open_commit", true, {rd("x", SK_X), rd("r", SK_RYZ), rd("y", SK_RYZ), wr("c", SK_C), wr("t", SK_T), wr_opt("ok", SK_FLAG)}};
constexpr CallSlabs kSlabsOpenResponse = {"open_response", true, {rd("y", SK_RYZ), rd("r", SK_RYZ), rd("d", SK_GD), wr("z", SK_RYZ)}};
constexpr CallSlabs kSlabsOpenVerify = {
    "open_verify", true, {rd("z", SK_RYZ), rd("t", SK_T), rd("c", SK_C), rd("d", SK_GD), wr("accept", SK_FLAG)}};
constexpr CallSlabs kSlabsOpenRecover = {
    "open_recover", true, {rd("z", SK_RYZ), rd("c", SK_C), rd("d", SK_GD), wr("t_out", SK_T), wr("accept", SK_FLAG)}};
constexpr CallSlabs kSlabsOpenResponseReject = {
    "open_response_reject", true,
    {rd("y", SK_RYZ), rd("r", SK_RYZ), rd("d", SK_GD), rd("coin", SK_WORD), wr("z", SK_RYZ), wr("accept", SK_FLAG), wr_opt("E", SK_WORD)}};
constexpr CallSlabs kSlabsOpenProveZk = {
    "open_prove_zk", true,
    {rd("x", SK_X), wr("c", SK_C), wr("t", SK_T), wr("z", SK_RYZ), wr("r", SK_RYZ), wr("ok", SK_FLAG), wr("rounds", SK_FLAG)}};
// ---- Linear -------------------------------------------------------------------------------------------------------------
constexpr CallSlabs kSlabsLinearCommit = {
    "linear_commit", true,
    {rd("g", SK_GD), rd("x", SK_X), rd("r", SK_RYZ), rd("rp", SK_RYZ), rd("y", SK_RYZ), rd("yp", SK_RYZ), wr("c", SK_C), wr("cp", SK_C),
     wr("t", SK_T), wr("tp", SK_T), wr("u", SK_U), wr_opt("ok", SK_FLAG)}};
constexpr CallSlabs kSlabsLinearMask = {
    "linear_mask", true, {rd("g", SK_GD), rd("y", SK_RYZ), rd("yp", SK_RYZ), wr("t", SK_T), wr("tp", SK_T), wr("u", SK_U)}};
constexpr CallSlabs kSlabsLinearResponse = {
    "linear_response", true,
    {rd("y", SK_RYZ), rd("yp", SK_RYZ), rd("r", SK_RYZ), rd("rp", SK_RYZ), rd("d", SK_GD), wr("z", SK_RYZ), wr("zp", SK_RYZ)}};
constexpr CallSlabs kSlabsLinearVerify = {
    "linear_verify", true,
    {rd("z", SK_RYZ), rd("zp", SK_RYZ), rd("c", SK_C), rd("cp", SK_C), rd("g", SK_GD), rd("t", SK_T), rd("tp", SK_T), rd("u", SK_U),
     rd("d", SK_GD), wr("accept", SK_FLAG)}};
constexpr CallSlabs kSlabsLinearRecover = {
    "linear_recover", true,
    {rd("z", SK_RYZ), rd("zp", SK_RYZ), rd("c", SK_C), rd("cp", SK_C), rd("g", SK_GD), rd("d", SK_GD), wr("t_out", SK_T),
     wr("tp_out", SK_T), wr("u_out", SK_U), wr("accept", SK_FLAG)}};
constexpr CallSlabs kSlabsLinearResponseReject = {
    "linear_response_reject", true,
    {rd("y", SK_RYZ), rd("yp", SK_RYZ), rd("r", SK_RYZ), rd("rp", SK_RYZ), rd("d", SK_GD), rd("coin", SK_WORD), wr("z", SK_RYZ),
     wr("zp", SK_RYZ), wr("accept", SK_FLAG), wr_opt("E", SK_WORD)}};
constexpr CallSlabs kSlabsLinearProveZk = {
    "linear_prove_zk", false,
    {rd("g", SK_GD), rd("x", SK_X), wr("c", SK_C), wr("cp", SK_C), wr("t", SK_T), wr("tp", SK_T), wr("u", SK_U), wr("z", SK_RYZ),
     wr("zp", SK_RYZ), wr("r", SK_RYZ), wr("rp", SK_RYZ), wr("ok", SK_FLAG), wr("rounds", SK_FLAG)}};
// ---- Sum: the Linear lists with V summands where a name ends in s ----------------------------------------------------------
constexpr CallSlabs kSlabsSumCommit = {
    "sum_commit", false,
    {rd("gs", sum_of(SK_GD)), rd("xs", sum_of(SK_X)), rd("rs", sum_of(SK_RYZ)), rd("rp", SK_RYZ), rd("ys", sum_of(SK_RYZ)), rd("yp", SK_RYZ),
     wr("cs", sum_of(SK_C)), wr("cp", SK_C), wr("ts", sum_of(SK_T)), wr("tp", SK_T), wr("u", SK_U), wr_opt("ok", SK_FLAG)}};
constexpr CallSlabs kSlabsSumMask = {
    "sum_mask", false,
    {rd("gs", sum_of(SK_GD)), rd("ys", sum_of(SK_RYZ)), rd("yp", SK_RYZ), wr("ts", sum_of(SK_T)), wr("tp", SK_T), wr("u", SK_U)}};
constexpr CallSlabs kSlabsSumResponse = {
    "sum_response", false,
    {rd("ys", sum_of(SK_RYZ)), rd("yp", SK_RYZ), rd("rs", sum_of(SK_RYZ)), rd("rp", SK_RYZ), rd("d", SK_GD), wr("zs", sum_of(SK_RYZ)),
     wr("zp", SK_RYZ)}};
constexpr CallSlabs kSlabsSumVerify = {
    "sum_verify", false,
    {rd("zs", sum_of(SK_RYZ)), rd("zp", SK_RYZ), rd("cs", sum_of(SK_C)), rd("cp", SK_C), rd("gs", sum_of(SK_GD)), rd("ts", sum_of(SK_T)),
     rd("tp", SK_T), rd("u", SK_U), rd("d", SK_GD), wr("accept", SK_FLAG)}};
constexpr CallSlabs kSlabsSumRecover = {
    "sum_recover", false,
    {rd("zs", sum_of(SK_RYZ)), rd("zp", SK_RYZ), rd("cs", sum_of(SK_C)), rd("cp", SK_C), rd("gs", sum_of(SK_GD)), rd("d", SK_GD),
     wr("ts_out", sum_of(SK_T)), wr("tp_out", SK_T), wr("u_out", SK_U), wr("accept", SK_FLAG)}};
constexpr CallSlabs kSlabsSumResponseReject = {
    "sum_response_reject", false,
    {rd("ys", sum_of(SK_RYZ)), rd("yp", SK_RYZ), rd("rs", sum_of(SK_RYZ)), rd("rp", SK_RYZ), rd("d", SK_GD), rd("coin", SK_WORD),
     wr("zs", sum_of(SK_RYZ)), wr("zp", SK_RYZ), wr("accept", SK_FLAG), wr_opt("E", SK_WORD)}};
constexpr CallSlabs kSlabsSumProveZk = {
    "sum_prove_zk", false,
    {rd("gs", sum_of(SK_GD)), rd("xs", sum_of(SK_X)), wr("cs", sum_of(SK_C)), wr("cp", SK_C), wr("ts", sum_of(SK_T)), wr("tp", SK_T),
     wr("u", SK_U), wr("zs", sum_of(SK_RYZ)), wr("zp", SK_RYZ), wr("rs", sum_of(SK_RYZ)), wr("rp", SK_RYZ), wr("ok", SK_FLAG),
     wr("rounds", SK_FLAG)}};

// every list above (tests/slabs/slabs_driver.cpp prints them)
constexpr const CallSlabs* kAllCallSlabs[] = {
    &kSlabsPolymul, &kSlabsAdd, &kSlabsSub, &kSlabsCanonicalize, &kSlabsNarrow, &kSlabsWiden, &kSlabsMatvec, &kSlabsCmul, &kSlabsNorm2Le,
    &kSlabsEq, &kSlabsEq32, &kSlabsCommit, &kSlabsCommitmentVerify, &kSlabsOpenCommit, &kSlabsOpenResponse, &kSlabsOpenVerify,
    &kSlabsOpenRecover, &kSlabsOpenResponseReject, &kSlabsOpenProveZk, &kSlabsLinearCommit, &kSlabsLinearMask, &kSlabsLinearResponse,
    &kSlabsLinearVerify, &kSlabsLinearRecover, &kSlabsLinearResponseReject, &kSlabsLinearProveZk, &kSlabsSumCommit, &kSlabsSumMask,
    &kSlabsSumResponse, &kSlabsSumVerify, &kSlabsSumRecover, &kSlabsSumResponseReject, &kSlabsSumProveZk};

}  // namespace rzk
