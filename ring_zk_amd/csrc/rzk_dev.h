// rzk_dev.h — structures shared by the kernels (rzk_kernels.hip and the family headers it includes), the host planner (rzk_plan.h) and the C-ABI host code (rzk_ctx.h and the rzk_*.cpp files behind it).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "rzk_core.h"
#include "rzk_packed.h"
#include "rzk_wire_walk.h"

namespace rzk {

// Constants every kernel reads through a pointer to device memory (uniform -> scalar loads).
// The twiddle tables are passed separately as one global pointer: table (2*prime + dir) of kTableLen
// words, dir 0 = psi^{bitrev} * R (forward), dir 1 = psi^{-bitrev} * R (inverse).
struct DevTables {
  PrimeConsts pc[kMaxPrimes];
  CrtConsts crt;
  double cap[kMaxPrimes + 1];           // cap[np] = largest |exact result| np primes can represent
  uint32_t diet;                        // DIET_* bits: which shorter forms the unit kernels take (all compute the same values)
  uint32_t pad;
};
// DevTables::diet (rzk_ctx_create: RZK_ROT_LAST / RZK_CRT2_SHORT, default on)
// (the third knob of the family, RZK_DOT2, reaches the kernel through the plan: ITEM_DOT2 below)
enum : uint32_t {
  DIET_ROT_LAST = 1,   // unit_kernel, single-row units of one wavefront: rotation terms after the last inverse transform, sums in registers
  DIET_CRT2 = 2,       // two-prime reconstruction with one reduction mod q (crt2_zq_short)
};

// ---- row programs ------------------------------------------------------------------------------------
// Every protocol phase is a small "row program": for each proof b of the batch and each output row,
//
//     out_row = sum_terms sign * (KEY[entry]  (*)  V[b][src])        key entry times a per-proof polynomial
//             + sum_terms sign * (U[b][srcA]  (*)  V[b][srcB])        product of two per-proof polynomials
//             + sum_adds  sign *  T[b][src]                           plain additions
//
// evaluated by ONE wavefront: the products are accumulated in the NTT domain of as many auxiliary
// primes as the exact integer result needs (decided per row from the operands' norms), transformed
// back once, CRT-reconstructed, reduced to the centred representative mod q, then the additions are
// applied.  The result is either stored (MODE_STORE) or tested against zero (MODE_ZERO, the
// `lhs == rhs` of the verifiers, e.g. src/prove/open.rs:173).
// Program tables (rows, terms, additions, units, items, plans) are written by the host before a launch and never by
// a kernel, so the kernels may read them through the constant address space: the compiler then uses scalar loads
// (one s_load per record, no vector-memory latency in the control flow).  The records are 4 / 8 / 16 bytes, naturally
// aligned inside their tables (static_asserts in rzk_plan.h).
#if defined(__HIPCC__)
template <class Tp>
__device__ __forceinline__ Tp table_load(const Tp* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef const Tp __attribute__((address_space(4))) * cptr_t;
  return *reinterpret_cast<cptr_t>(reinterpret_cast<uintptr_t>(p));
#else
  return *p;
#endif
}
#endif
constexpr int kMaxOperands = 12;
constexpr int kMaxRows = 48;
constexpr int kMaxTerms = 640;
constexpr int kMaxAdds = 128;

// TERM_SHIFT: (a_op,a_off) (*) (b_op,b_off) with a sparse `a` (the challenge d), evaluated as signed negacyclic
// rotations (ShiftGeo, rzk_core.h) instead of transforms.  A row keeps its shift terms behind its transform
// terms: terms[term0 .. term0+nterms) are KEY / VEC, terms[term0+nterms .. +nshift) are SHIFT.
enum : uint8_t { TERM_KEY = 0, TERM_VEC = 1, TERM_SHIFT = 2, TERM_DKEY = 3, TERM_DD = 4, TERM_KIND_MASK = 0x3f };
enum : uint8_t { MODE_STORE = 0, MODE_ZERO = 1 };
// Fused norm predicate (Params::check_*_constraint, src/params.rs:102-118): a term (its b operand) or an
// addition marked with CHECK also tests sum c^2 < Operands::norm_limit for the polynomial it loads and
// clears flags[proof] on failure.  The host marks, for each polynomial of the checked vector, the first
// load in program order, so every polynomial is tested exactly once and no separate norm pass is needed.
// CHECK2 marks a second checked vector whose failure clears only bit 1 of the flag byte (two-bit verdicts:
// Linear commit reports constraint(r) in bit 0 and constraint(r') in bit 1); it is honoured by row_kernel only.
constexpr uint8_t TERM_CHECK = 0x80;   // in Term::kind
constexpr uint8_t TERM_CHECK2 = 0x40;
constexpr uint8_t ADD_CHECK = 0x80;    // in AddTerm::op
constexpr uint8_t ADD_CHECK2 = 0x40;
constexpr uint8_t ADD_OP_MASK = 0x3f;

struct alignas(8) Term {
  uint8_t kind;     // TERM_KEY: KEY[a_off] (*) operand(b_op, b_off);  TERM_VEC: (a_op,a_off) (*) (b_op,b_off);
                    // TERM_DKEY: image a_off of the batch entry's own multipliers (Operands::dkey_img) (*) operand(b_op, b_off)
                    // TERM_DD: the same, and the operand's transform is taken from Operands::oimg when an earlier launch
                    //          of the call left it there (b_off = summand * oimg_k + column); transformed here otherwise
  int8_t sign;      // +1 / -1
  uint8_t a_op, b_op;
  uint16_t a_off, b_off;
};
struct alignas(4) AddTerm {
  uint8_t op;
  int8_t sign;
  uint16_t off;
};
struct alignas(8) Row {
  uint16_t term0, nterms, add0, nadds;
  uint8_t out_op, mode;
  uint16_t out_off;
  uint16_t nshift, pad;
};
// Row groups: consecutive rows made of key products over the SAME operand list (the n rows of a1 over
// columns n..k-1, the l rows of a2, ...).  One wavefront evaluates a whole group: every shared operand is
// transformed once and multiplied into up to kGroupMax accumulators (row_group_kernel).
constexpr int kGroupMax = 4;
struct GroupDesc {
  uint16_t row0, count;
};
struct Program {
  uint32_t nrows, nterms, nadds, ngroups;
  GroupDesc groups[kMaxRows];
  Row rows[kMaxRows];
  Term terms[kMaxTerms];
  AddTerm adds[kMaxAdds];
};

// ---- wave programs (unit_kernel): the default evaluation of a row program -------------------------------------
// A UNIT is one output row — or a PAIR of rows (A, B) — evaluated by one wavefront over an ordered list of ITEMS;
// an item is one forward-transformed operand together with what is multiplied into the rows with it:
//   ITEM_KEY   acc_A += signA * KEY[keyA] (*) X      and / or      acc_B = signB * KEY[keyB] (*) X
//   ITEM_VEC   acc_A += signA * X(a_op,a_off) (*) X(b_op,b_off)                      (single-row units only)
// Row B of a pair has exactly one product and its operand is the unit's LAST item, so the transform of that operand
// is shared (c0 = r0 + K0 r1 + K1 r2 and c1 = r1 + K2 r2 + x of an Open commitment share r2: commit.rs:109-125).
// While operands are loaded and transformed nothing else is live in registers: the accumulator of row A is parked
// in LDS between items (one N-word buffer per wavefront, the layout of the resident key), the one of row B exists
// only from the last item on.  The Garner state between primes lives in a per-wave global scratch line.
// Rotation terms (TERM_SHIFT), plain additions, the store / zero test and the norm marks stay in Program::rows.
enum : uint8_t { ITEM_KEY = 0, ITEM_VEC = 1 };
constexpr uint16_t kNoKey = 0xffff;
constexpr uint16_t kNoRow = 0xffff;
// Item::flags, on both items of a unit whose row A is exactly two key products (set by plan_units when PlanEnv::dot2):
// unit_kernel parks the first TRANSFORM instead of the first product and forms x1 k1 + x2 k2 with one reduction (dot2_lazy)
constexpr uint8_t ITEM_DOT2 = 0x01;
struct alignas(8) Item {
  uint8_t kind;        // ITEM_KEY / ITEM_VEC
  uint8_t flags;       // TERM_CHECK / TERM_CHECK2: the b operand carries a fused norm mark; ITEM_DOT2 (below)
  uint8_t b_op, a_op;
  uint16_t b_off, a_off;
  uint16_t keyA, keyB;   // key entries (kNoKey = the item does not feed that row)
  int8_t signA, signB;
  uint16_t pad;
};
struct alignas(8) Unit {
  uint16_t rowA, rowB;      // indices into Program::rows; rowB = kNoRow for a single row
  uint16_t item0, nitems;   // nitems items from item0 on
};
struct WaveProgram {
  uint32_t nunits, nitems;
  Unit units[kMaxRows];
  Item items[kMaxTerms];
};

// Shared-operand path: the distinct polynomials ("slots") the product terms of a program read, and for
// each term the slots of its operands.  check[s] != 0: the slot belongs to a norm-checked vector.
constexpr int kMaxSlots = 512;
struct SlotTable {
  uint32_t nslots, pad;
  uint16_t op[kMaxSlots], off[kMaxSlots];
  uint8_t check[kMaxSlots];
  uint16_t term_a[kMaxTerms], term_b[kMaxTerms];
};

// Row blocks (row_block_kernel): consecutive rows of a key-only program whose distinct operands fit in LDS
// together.  One 8-wave workgroup evaluates a block of one proof prime by prime: the waves transform the
// block's operands into LDS (each exactly once), meet at a barrier, then every wave evaluates rows from the
// staged transforms.  For [a1;a2].r at (8,17,8) that is 9 transforms per prime and block instead of 72 + 8.
constexpr int kBlockWaves = 8;     // (9 measured slightly slower in round 1; 10 — no idle wave in the operand phase — +0.7 % in round 2: noise)
constexpr int kBlockMaxSlots = 9;    // staged operand transforms per block: 9 * 4N bytes of LDS (72 KiB at N = 2048)
constexpr int kBlockMaxRows = 16;    // rows per block (two Garner state lines each in the workgroup's scratch)
struct BlockDesc {
  uint16_t row0, nrows, slot0, nslots;
};
struct BlockPlan {
  uint32_t nblocks, nslots_total;
  BlockDesc blk[kMaxRows];
  uint16_t slot_op[kMaxSlots], slot_off[kMaxSlots];   // indexed by BlockDesc::slot0 + s
  uint8_t slot_check[kMaxSlots];
  uint16_t term_slot[kMaxTerms];                      // slot (within its block) of each term's operand
};

// Operand table of one launch.  The batch index b of a task may be a (proof, summand) pair:
// bo = b / group is the proof.  Polynomial (op, off) lives at
// base[op] + ((outer[op] ? bo : b) * stride[op] + off) * N ; verification flags are per proof (flags[bo]).
struct Operands {
  int64_t* base[kMaxOperands];
  uint32_t stride[kMaxOperands];
  uint32_t outer[kMaxOperands];
  uint32_t group;
  uint32_t pad;          // != 0: two-bit verdict flags (TERM_CHECK clears bit 0, TERM_CHECK2 bit 1; row_kernel only)
  uint64_t norm_limit;   // (bound+1)^2 of the fused norm predicate; must be <= 2^48 (0 = unused)
  // Canonical-input test (every coefficient a kernel loads must be the centred representative a ZqI64 holds,
  // src/params.rs:122-127): a violation clears the proof's verdict flag when the launch has flags, and sets this
  // sticky word of the context when it is not NULL (prover-side and Mat-level entry points: the call fails).
  uint32_t* bad;
  // != 0: the caller vouches that every coefficient this launch loads is canonical (written by this library on this
  // device, or validated before): the canonical test is skipped (rzk_ctx_trust_device_outputs).  Norm predicates and
  // the norm measurements that fix the prime count are evaluated as always.
  uint32_t trusted;
  // != 0: the launch itself initialises every verdict flag to this value before its rows can clear it — only set when
  // one team evaluates ALL rows of a batch entry and flags are per entry (unit kernels with units_per_task = all, group 1);
  // otherwise the host presets the flags with a fill launch of its own (rzk_run.cpp, run_program)
  uint32_t preset;
  // Per-entry multiplier images (TERM_DKEY, row_kernel only): the scalar polynomials g_i of the Linear / Sum proofs, which
  // every vector x vector row of a proof multiplies by, transformed ONCE per proof and call (dkey_transform_kernel) into
  // the form of the resident key: [entry][dkey_n][kKeyImages][N] residues x N^-1 x R, NTT-domain layout; dkey_l2 their
  // 2-norms (upper bounds).  Entry = the proof index (b / group).
  const uint32_t* dkey_img;
  const double* dkey_l2;
  uint32_t dkey_n, pad3;
  // Operand images: the key-product kernels that transform the vectors y_i (z_i) of a Sum call anyway — row_group_kernel,
  // row_block_kernel evaluating a1.y_i (a1.z_i) — leave the transforms of the columns a2 uses here (producer: oimg_op =
  // that operand's index, entry = batch entry), and the vector x vector rows of D = sum_i g_i (.) v_i read them back
  // (consumer, TERM_DD: entry = proof * oimg_group + summand) instead of transforming v_{i,c} again.
  // [entry][oimg_n][kKeyImages][N] lazy residues in the NTT-domain layout; oimg_l2 2-norm bounds; oimg_np primes stored.
  uint32_t* oimg;
  double* oimg_l2;
  uint8_t* oimg_np;
  uint32_t oimg_n, oimg_op, oimg_group, oimg_k;
  int8_t oimg_col[32];   // column of the vector -> image index, or -1
};

// ---- launchers (defined in rzk_kernels.hip; their shared launch rules: rzk_launch.h) ----------------------------
// Behind every launch of every .hip file: the launcher returns the HIP error of a launch that did not start.
#define RZK_LAUNCH_CHECK()                      \
  do {                                          \
    hipError_t e_ = hipGetLastError();          \
    if (e_ != hipSuccess) return (int)e_;       \
  } while (0)
// A launcher that exists for both coefficient types of a slab (C = int64_t, int32_t; rzk_coef.h) is declared below as a
// template over C, and defined and instantiated for both in its .hip file: RZK_BOTH_WIDTHS(launch_x) behind the definition.
// The host layer's typed entry points (rzk_ctx.h) use the same macro.
// (an explicit instantiation takes the visibility of where it stands, not of its declaration: hidden is said here, so
// that the library's export list holds none of them)
#define RZK_BOTH_WIDTHS(fn)                                                              \
  template __attribute__((visibility("hidden"))) decltype(fn<int64_t>) fn<int64_t>; \
  template __attribute__((visibility("hidden"))) decltype(fn<int32_t>) fn<int32_t>;

struct LaunchCfg {
  void* stream;   // hipStream_t
  int num_cus;
  int pair_poly;  // N = 2048: two wavefronts per polynomial (PairTeam) in unit_kernel / row_kernel / row_block_kernel
  int unit_io;    // key-product programs through unit_io_kernel (operands read once) instead of unit_kernel
  int shift_bytes;   // shift_row_kernel at N <= 1024: short operands rotate as packed bytes (RZK_SHIFT_BYTES)
  int tw_lds;     // unit_kernel at N = 1024: 1 = phase-2 twiddles from an LDS image per workgroup, 2 = phase 3 too, sixteen teams per workgroup (RZK_TW_LDS)
  std::string* launched = nullptr;   // out: the row-program launchers write the name of the instantiation they started here
};

// The device pointers of a row-program launch: run_program (rzk_run.cpp) fills one per call, only `scratch` differs per path.
struct RowArgs {
  const Program* prog;
  const WaveProgram* wp;      // the unit kernels' view of the program (NULL for a program planned without one)
  const uint32_t* key_ntt;    // resident key images and their 2-norms
  const double* key_l2;
  const DevTables* T;
  const uint32_t* tw;         // twiddle tables
  uint32_t* scratch;          // the path's global scratch lines (row_scratch_words / group_scratch_words / block_scratch_words)
  uint8_t* flags;             // verdict flags, or NULL
};
// What the unit kernels' launchers need to know of the planned program.
// units_per_task: how many consecutive units of one batch entry a wavefront evaluates back to back (all of them =
// one wavefront per proof: equal-cost tasks, no tail)
// work_per_entry: transforms one batch entry costs at two primes (the progress priorities only need an estimate)
struct UnitShape {
  uint32_t nunits, units_per_task, work_per_entry;
  bool has_vec, has_shift;
};
// The shared-operand path's workspace of stored transforms (np_store primes each) and their norms
struct SlotStore {
  uint32_t* ws;
  double* norms;
  uint32_t np_store;
};
// row_kernel: one wavefront per (batch entry, row); programs with vector x vector products
int launch_rows(int logn, const LaunchCfg& cfg, const RowArgs& a, const Operands& ops, uint32_t nrows, bool has_shift, uint64_t batch,
                bool has_dd = false);
int launch_units(int logn, const LaunchCfg& cfg, const RowArgs& a, const Operands& ops, const UnitShape& u, uint64_t batch);
int launch_row_program_slots(int logn, const LaunchCfg& cfg, const RowArgs& a, const Operands& ops, const SlotTable* d_slots,
                             uint32_t nslots, const SlotStore& st, uint64_t batch);
int launch_row_groups(int logn, const LaunchCfg& cfg, const RowArgs& a, const Operands& ops, uint32_t ngroups, uint64_t batch);
size_t group_scratch_words(int logn, int num_cus);
int launch_row_blocks(int logn, const LaunchCfg& cfg, const RowArgs& a, const Operands& ops, const BlockPlan* d_plan, uint32_t nblocks,
                      uint64_t batch);
size_t block_scratch_words(int logn, int num_cus);
// images of `count` scalar multipliers (dkey_n per batch entry) for TERM_DKEY terms; flags / bad as in Operands
int launch_dkey_transform(int logn, const LaunchCfg& cfg, const int64_t* g, uint64_t count, uint32_t dkey_n, uint32_t* img,
                          double* l2, const DevTables* T, const uint32_t* d_tw, uint8_t* d_flags, uint32_t* d_bad, bool two_bit,
                          bool trusted);
// rows whose products all have a sparse multiplier (the challenge) as `a` operand: shift-add kernel, no transforms
int launch_shift_rows(int logn, const LaunchCfg& cfg, const RowArgs& a, const Operands& ops, uint32_t nrows, uint64_t batch);
// Rows per group of row_group_kernel.  Two numbers, on purpose:
//   group_accumulators  how many accumulators (= rows per group, at most kGroupMax) the instantiation launched for this
//                       size is COMPILED with: 4 at N <= 1024, 2 at N = 2048;
//   group_max_for       what the host groups by DEFAULT: the same at N <= 1024, but 1 = no grouping at N = 2048 (the
//                       accumulators cost too many registers there: measured slower).  The RZK_GROUP_MAX knob of
//                       rzk_ctx_create may raise it again, up to group_accumulators (the tests do, to reach the kernel).
constexpr int group_accumulators(int logn) { return logn >= 11 ? 2 : 4; }
inline int group_max_for(int logn) { return logn >= 11 ? 1 : group_accumulators(logn); }
// words of per-wave global scratch of unit_kernel: (max blocks) * 4 waves * 4N (Garner words A, B of rows A, B)
size_t row_scratch_words(int logn, int num_cus);
int launch_key_transform(int logn, const LaunchCfg& cfg, const int64_t* d_key, uint32_t entries,
                         uint32_t* d_key_ntt, const DevTables* d_T, const uint32_t* d_tw);
int launch_ntt(int logn, bool inverse, const LaunchCfg& cfg, int prime, const uint32_t* d_in,
               uint32_t* d_out, uint64_t count, const DevTables* d_T, const uint32_t* d_tw);
int launch_fill_u8(const LaunchCfg& cfg, uint8_t* p, uint8_t value, uint64_t n);
// device-side samplers (rzk_rng.h): npoly polynomials of n_ring coefficients each
int launch_sample_uniform(const LaunchCfg& cfg, int64_t* out, uint64_t npoly, uint32_t n_ring, uint64_t seed,
                          uint32_t stream, uint32_t bound);
int launch_sample_gauss(const LaunchCfg& cfg, int64_t* out, uint64_t npoly, uint32_t n_ring, uint64_t seed,
                        uint32_t stream, double sigma);
int launch_sample_challenge(const LaunchCfg& cfg, int64_t* out, uint64_t npoly, uint32_t n_ring, uint64_t seed,
                            uint32_t stream, uint32_t kappa);
// the Gaussian word-to-pair map (rzk_gauss.h) on chosen words: words [pairs][4] -> out [pairs][2]
int launch_debug_gauss_map(const LaunchCfg& cfg, bool f32, const uint32_t* words, double sigma, int64_t* out, uint64_t pairs);
int launch_canonicalize(const LaunchCfg& cfg, const int64_t* in, int64_t* out, uint64_t ncoef, int64_t q);
int launch_addsub(const LaunchCfg& cfg, bool sub, const int64_t* a, const int64_t* b, int64_t* out,
                  uint64_t ncoef, const DevTables* d_T, uint32_t* bad_word);
// ok[b] = (all `rows` polys of proof b have sum c^2 < limit), limit = (bound+1)^2 given as hi:lo.
// and_mode: 0 = overwrite ok[b], 1 = ok[b] &= result, 2 = ok[b] |= result << shift
// qhalf = (q-1)/2, bad_word: see Operands::bad (a non-canonical coefficient also fails the predicate / equality)
int launch_norm(int logn, const LaunchCfg& cfg, const int64_t* v, uint32_t rows, uint64_t limit_hi,
                uint64_t limit_lo, uint8_t* ok, uint64_t B, int and_mode, int shift, uint32_t qhalf,
                uint32_t* bad_word);
int launch_eq(int logn, const LaunchCfg& cfg, const int64_t* a, const int64_t* b, uint32_t rows,
              uint8_t* eq, uint64_t B, uint32_t qhalf, uint32_t* bad_word);
// ---- batched codec of the serialized protocol messages (rzk_wire_dev.hip; schema in rzk_wire_walk.h) ----------------
struct WireSlabs {
  int64_t* ptr[kWireMaxFields];   // dense slab of every field ([B][rows of the field][N]); encode: NULL Option = None
};
// decode: walk (ok[b], tab[b * polys + j] = (byte position << 16) | len) then copy (widen, range-check, zero-fill)
int launch_wire_walk(const LaunchCfg& cfg, const uint8_t* bytes, uint64_t total, const uint64_t* offsets,
                     const WireSchema& s, int need_align, uint64_t* tab, uint8_t* ok, uint64_t B);
int launch_wire_copy(const LaunchCfg& cfg, const uint8_t* bytes, const uint64_t* tab, const WireSchema& s,
                     const WireSlabs& sl, int64_t half, uint8_t* ok, uint64_t B);
// encode: trimmed lengths + canonical test, per-message scan, batch scan of message sizes, write.
// lens: [B * polys] u32, rel: [B * polys] u64, msize: [B] u64 (scratch); offsets: [B + 1]
int launch_wire_encode(const LaunchCfg& cfg, const WireSchema& s, const WireSlabs& sl, int64_t half, uint32_t* lens,
                       uint64_t* rel, uint64_t* msize, uint8_t* bytes, uint64_t* offsets, uint32_t* bad_word,
                       uint64_t B);
// ---- Fiat-Shamir transcript hash (rzk_fs_dev.hip; format and sponge in rzk_keccak.h) ---------------------------------
struct FsMsg {   // the polynomials P_0 .. P_{polys-1} of one proof: fields in declaration order, slabs row-major
  uint32_t nfields, N, polys;
  uint32_t first[kWireMaxFields + 1];      // first polynomial of every field; first[nfields] = polys
  const int64_t* ptr[kWireMaxFields];      // slab of every field, [B][rows of the field][N]
};
struct FsRoot {
  uint64_t hdr[10];   // header words in front of the leaf digests (rzk_keccak.h: fs_root_header / fs_key_header)
  uint32_t nhdr;
  uint32_t leaves;    // leaf digests per proof
  uint32_t N, kappa;
};
// leaf digests of B proofs: word w of leaf j = p * C + c of proof b at dig[(j * 4 + w) * B + b].  check != 0: every
// coefficient is range-tested while it is loaded; a violation clears ok[b], or with ok == NULL sets *bad_word (the
// context's sticky bad-input word), so that a non-canonical coefficient is never hashed silently as its low 32 bits.
// C: what the slabs of m hold (FsMsg carries addresses, so the caller names it: launch_fs_leaves<C>); int32_t is reported
// as fs_leaf_kernel<i32>
template <class C>
int launch_fs_leaves(const LaunchCfg& cfg, const FsMsg& m, int64_t half, int check, uint64_t* dig, uint8_t* ok,
                     uint32_t* bad_word, uint64_t B);
// root of every proof: digest [B][32] (may be NULL) and, with d != NULL, the challenge into d [B][N] (zeroed before);
// an int32_t slab d is reported as fs_root_kernel<i32>
template <class C>
int launch_fs_roots(const LaunchCfg& cfg, const FsRoot& r, const uint64_t* dig, C* d, uint8_t* digest, uint64_t B);
// ---- keyed samplers (rzk_csprng_dev.hip; stream and maps in rzk_chacha.h): the distributions of launch_sample_*,
// drawn from ChaCha20 blocks under the call's subkey = HChaCha20(key, nonce)
// an int32_t slab `out` (16-byte aligned) is reported as sample_*_chacha_kernel_i32: the same streams, narrowed at the store
template <class C>
int launch_sample_uniform_chacha(const LaunchCfg& cfg, C* out, uint64_t npoly, uint32_t n_ring, const uint32_t subkey[8],
                                 uint32_t stream, uint32_t bound);
template <class C>
int launch_sample_gauss_chacha(const LaunchCfg& cfg, C* out, uint64_t npoly, uint32_t n_ring, const uint32_t subkey[8],
                               uint32_t stream, double sigma);
template <class C>
int launch_sample_challenge_chacha(const LaunchCfg& cfg, C* out, uint64_t npoly, uint32_t n_ring, const uint32_t subkey[8],
                                   uint32_t stream, uint32_t kappa);
// the exact discrete Gaussian D_sigma, integer sigma in [1, 2^26] (definition and stream: rzk_dgauss.h), and its trial
// on chosen words: words [trials][8] -> out [trials][2] = (accepted, value)
template <class C>
int launch_sample_dgauss_chacha(const LaunchCfg& cfg, C* out, uint64_t npoly, uint32_t n_ring, const uint32_t subkey[8],
                                uint32_t stream, uint32_t sigma);
int launch_debug_dgauss_trial(const LaunchCfg& cfg, uint32_t sigma, const uint32_t* words, int64_t* out, uint64_t trials);
// ---- rejection sampling of the provers (rzk_reject_dev.hip; definition in rzk_reject.h) --------------------------------
struct RejectPartial;
struct RejectParts {   // the rows response polynomials of one proof as nparts pairs of slabs (z_f, y_f), each [B][rows of f][N]
  uint32_t nparts, N, rows;
  uint32_t first[4 + 1];   // first polynomial of every part; first[nparts] = rows
  const int64_t* z[4];
  const int64_t* y[4];
};
// part[b * rows + j] = (S2 - 2 S1, flags) of polynomial j of proof b; slabs must be 16-byte aligned
int launch_reject_stat(const LaunchCfg& cfg, const RejectParts& m, int64_t q, uint64_t vmax, uint64_t norm_limit, bool trusted,
                       RejectPartial* part, uint64_t B);
// accept[b], E[b] (may be NULL) from the partials and coin[b]; a non-canonical coefficient also sets *bad_word
int launch_reject_decide(const LaunchCfg& cfg, const RejectPartial* part, uint32_t rows, const int64_t* coin, uint64_t R,
                         double lnM, double two_sigma_sq, uint8_t* accept, int64_t* E, uint32_t* bad_word, uint64_t B);
// ---- response rows fused with the rejection statistic (rzk_response_stat_dev.hip) -----------------------
struct ResponseStat {   // where a launch of response_stat_kernel leaves its partials, and what it tests
  RejectPartial* part;    // [B][rows_total], the layout launch_reject_decide reads
  uint32_t rows_total;    // response polynomials per proof over all launches of the call
  uint32_t part_off;      // first partial of this launch inside a proof's rows_total
  int64_t vmax;           // kappa b
  uint64_t norm_limit;    // (verify_bound + 1)^2
};
// The rows of a PG_RESPONSE program (rzk_plan.h) as launch_shift_rows runs them, one wavefront per row, N = 512 / 1024 only
// (-1 otherwise); the partial of row `rowi` of batch entry b goes to part[(b / group) * rows_total + part_off +
// (b mod group) * nrows + rowi], group = Operands::group.
int launch_response_stat(int logn, const LaunchCfg& cfg, const RowArgs& a, const Operands& ops, uint32_t nrows, uint64_t batch,
                         const ResponseStat& so);
// ... on int32_t slabs (Operands::base address them): the packed-byte form at N = 512 / 1024, response_stat_kernel<., ., i32>
// (-1 otherwise: the caller converts)
int launch_response_stat32(int logn, const LaunchCfg& cfg, const RowArgs& a, const Operands& ops, uint32_t nrows, uint64_t batch,
                           const ResponseStat& so);
// ---- 32-bit coefficient slabs (rzk_slab32_dev.hip; format and routing in rzk_slab32.h) ------------------
// launch_units / launch_shift_rows for a launch whose Operands::base address int32_t slabs: key-product programs, one-wavefront
// teams, N = 512 / 1024, the packed-byte rotation kernel (-1 otherwise: the caller converts, slab32_native)
int launch_units32(int logn, const LaunchCfg& cfg, const RowArgs& a, const Operands& ops, const UnitShape& u, uint64_t batch);
int launch_shift_rows32(int logn, const LaunchCfg& cfg, const RowArgs& a, const Operands& ops, uint32_t nrows, uint64_t batch);
// launch_rows for such a launch: row_kernel<., false, i32, false>, programs with vector x vector items and neither rotation
// terms nor images, N = 512 / 1024 (-1 otherwise)
int launch_rows32(int logn, const LaunchCfg& cfg, const RowArgs& a, const Operands& ops, uint32_t nrows, bool has_shift, uint64_t batch,
                  bool has_dd);
// launch_norm on an int32_t slab: norm_kernel_i32, N = 512 / 1024 (-1 otherwise)
int launch_norm32(int logn, const LaunchCfg& cfg, const int32_t* v, uint32_t rows, uint64_t limit_hi, uint64_t limit_lo, uint8_t* ok,
                  uint64_t B, int and_mode, int shift, uint32_t qhalf, uint32_t* bad_word);
// out = the low words of in (bad_word != NULL: a non-canonical coefficient sets it); out = in sign-extended.  ncoef even,
// both slabs 16-byte aligned
int launch_narrow(const LaunchCfg& cfg, const int64_t* in, int32_t* out, uint64_t ncoef, uint32_t qhalf, uint32_t* bad_word);
int launch_widen(const LaunchCfg& cfg, const int32_t* in, int64_t* out, uint64_t ncoef);
// eq[b] = (the two blocks of `words` int32 words of entry b are equal word for word), no range test; words % 4 == 0, both
// slabs 16-byte aligned
int launch_eq32(const LaunchCfg& cfg, const int32_t* a, const int32_t* b, uint64_t words, uint8_t* eq, uint64_t B);
// ---- the in-library Open prover loop (rzk_prove_loop_dev.hip; arithmetic in rzk_prove_loop.h) ------------
// C: the coefficient type of the slabs; every slab 16-byte aligned.  count == 0 launches nothing.
// idx[0 .. *count) = the ascending b < B with live[b] && !done[b]; entries from *count on are not written.  -2: B >= 2^32
int launch_pending_compact(const LaunchCfg& cfg, const uint8_t* live, const uint8_t* done, uint64_t B, uint32_t* idx, uint32_t* count);
// coin[i] = prove_coin(a[i][0], b[i][1]); a, b: [count][N]
template <class C>
int launch_prove_coins(const LaunchCfg& cfg, const C* a, const C* b, uint32_t N, int64_t* coin, uint64_t count);
// dst0[i] = src0[idx[i]] ([rows0][N] each) and, with src1 != NULL, dst1[i] = src1[idx[i]] ([rows1][N]), i < count
template <class C>
int launch_gather_rows(const LaunchCfg& cfg, const C* src0, C* dst0, uint32_t rows0, const C* src1, C* dst1, uint32_t rows1, uint32_t N,
                       const uint32_t* idx, uint32_t count);
// accept[i] != 0: t[i] -> t_out[idx[i]], z[i] -> z_out[idx[i]], rounds[idx[i]] = rnd, done[idx[i]] = 1, i < count
template <class C>
int launch_accept_scatter(const LaunchCfg& cfg, const C* t, const C* z, C* t_out, C* z_out, uint32_t t_rows, uint32_t z_rows, uint32_t N,
                          const uint8_t* accept, const uint32_t* idx, uint32_t count, uint8_t rnd, uint8_t* rounds, uint8_t* done);
// after round 0: live = (ok_commit & ok_hash) != 0, done = live && accept, rounds = 0
int launch_prove_first(const LaunchCfg& cfg, const uint8_t* ok_commit, const uint8_t* ok_hash, const uint8_t* accept, uint8_t* live,
                       uint8_t* done, uint8_t* rounds, uint64_t B);
// after the last round: rows of t_out, z_out of every proof with done == 0 zeroed; ok = done
template <class C>
int launch_prove_last(const LaunchCfg& cfg, const uint8_t* done, C* t_out, C* z_out, uint32_t t_rows, uint32_t z_rows, uint32_t N,
                      uint8_t* ok, uint64_t B);
// The same moves over a field list (rzk_prove_loop.h: up to kMaxFields slabs, quads per entry of each), for the Linear and
// Sum loops; 64-bit slabs only.  -2: a list the kernels cannot walk (no field, too many, a NULL or
// misaligned slab, an empty entry).
struct FieldList;
// dst[f][i] = src[f][idx[i]] for every field f, i < count
int launch_gather_fields(const LaunchCfg& cfg, const FieldList& fl, const uint32_t* idx, uint32_t count);
// accept[i] != 0: src[f][i] -> dst[f][idx[i]] for every field, rounds[idx[i]] = rnd, done[idx[i]] = 1, i < count
int launch_accept_scatter_fields(const LaunchCfg& cfg, const FieldList& fl, const uint8_t* accept, const uint32_t* idx, uint32_t count,
                                 uint8_t rnd, uint8_t* rounds, uint8_t* done);
// launch_prove_first with live = prove_live(ok_commit, wanted, ok_hash)
int launch_prove_first_want(const LaunchCfg& cfg, const uint8_t* ok_commit, uint8_t wanted, const uint8_t* ok_hash, const uint8_t* accept,
                            uint8_t* live, uint8_t* done, uint8_t* rounds, uint64_t B);
// after the last round: dst[f][b] zeroed for every field of every proof with done == 0; ok = done
int launch_prove_last_fields(const LaunchCfg& cfg, const FieldList& fl, const uint8_t* done, uint8_t* ok, uint64_t B);
// ---- fixed-width packed records (rzk_packed_dev.hip; format in rzk_packed.h) -------------------------------------------
struct PackedSlabs {
  int64_t* ptr[kPackedMaxFields];   // dense slab of every field ([B][rows of the field][N]), 16-byte aligned
};
// rec: [B][s.rec_words] 64-bit words.  ok[b] must hold 1 before the launch; it is cleared for a message with a coefficient
// outside its class's range (encode: the marker is written in its place) / a record that does not decode
// C: what the slabs hold (PackedSlabs carries addresses, so the caller names it: launch_packed_encode<C>); int32_t is
// reported as packed_*_kernel<i32>
template <class C>
int launch_packed_encode(const LaunchCfg& cfg, const PackedSchema& s, const PackedSlabs& sl, uint64_t* rec, uint8_t* ok, uint64_t B);
template <class C>
int launch_packed_decode(const LaunchCfg& cfg, const PackedSchema& s, const PackedSlabs& sl, const uint64_t* rec, uint8_t* ok, uint64_t B);
// ---- seed expansion "XP1" (rzk_xof_dev.hip; format in rzk_xof.h) ---------------------------------------------------------
struct XofJob {
  uint64_t q;
  uint32_t N, domain;
  uint32_t p0, rows;   // out[b][r] is polynomial p0 + r under seeds[b]
  uint32_t chunks;     // N / min(N, 256)
  uint32_t mask;       // 2^bitlen(q - 1) - 1
};
// seeds: [B][4] little-endian 64-bit words (8-byte aligned), out: [B][rows][N] (16-byte aligned), both on the device
int launch_xof_uniform(const LaunchCfg& cfg, const XofJob& j, const uint64_t* seeds, int64_t* out, uint64_t B);
// small ring degrees (N = 4 .. 256): schoolbook products mod q, same row programs
int launch_row_program_small(uint32_t N, const LaunchCfg& cfg, const Program* d_prog, uint32_t nrows,
                             const Operands& ops, const uint32_t* d_key_mont, const DevTables* d_T, uint32_t r2q,
                             uint8_t* d_flags, uint64_t batch);
int launch_key_mont(const LaunchCfg& cfg, const int64_t* d_key, uint32_t* d_key_mont, uint64_t ncoef,
                    const DevTables* d_T, uint32_t r2q);
int launch_norm_small(uint32_t N, const LaunchCfg& cfg, const int64_t* v, uint32_t rows, uint64_t limit_hi,
                      uint64_t limit_lo, uint8_t* ok, uint64_t B, int and_mode, int shift, uint32_t qhalf,
                      uint32_t* bad_word);
int launch_eq_small(uint32_t N, const LaunchCfg& cfg, const int64_t* a, const int64_t* b, uint32_t rows,
                    uint8_t* eq, uint64_t B, uint32_t qhalf, uint32_t* bad_word);

}  // namespace rzk
