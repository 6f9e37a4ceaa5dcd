// rzk_ctx.h — internal to the C-ABI host code (rzk_ctx.cpp, rzk_key.cpp, rzk_run.cpp, rzk_protocols.cpp, rzk_host.cpp,
// rzk_samplers.cpp, rzk_codec.cpp, rzk_slab32.cpp, rzk_prove_loop.cpp): the context behind include/rzk.h and the helpers
// those translation units share.  An entry point that exists for int64_t and int32_t slabs is one template over the
// coefficient type C (rzk_coef.h); its extern "C" symbols forward to it.
// Host-only.  Everything in rzk::api has hidden visibility: the library exports the rzk_* entry points, not these.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <tuple>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/rzk.h"
#include "rzk_chacha.h"
#include "rzk_coef.h"
#include "rzk_core.h"
#include "rzk_dev.h"
#include "rzk_dgauss.h"
#include "rzk_keccak.h"
#include "rzk_packed.h"
#include "rzk_plan.h"
#include "rzk_reject.h"
#include "rzk_slab32.h"
#include "rzk_slabs.h"
#include "rzk_tables.h"
#include "rzk_xof.h"

// plan_program speaks the C ABI's status codes, PG_MATVEC its key selectors
static_assert(rzk::kPlanOk == RZK_OK && rzk::kPlanArg == RZK_E_ARG && rzk::kPlanUnsupported == RZK_E_UNSUPPORTED, "plan status codes");
static_assert(RZK_KEY_A1 == 0 && RZK_KEY_A2 == 1 && RZK_KEY_A == 2, "key selectors");

namespace rzk {
namespace api __attribute__((visibility("hidden"))) {

struct DevProg : PlanFacts {   // a plan's facts and its tables on the device
  Program* d = nullptr;
  WaveProgram* d_wp = nullptr;     // units / items of unit_kernel (the default path)
  SlotTable* d_slots = nullptr;    // shared-operand path (fwd_slots_kernel + row_slots_kernel)
  BlockPlan* d_blocks = nullptr;   // row blocks (row_block_kernel)
};

struct Arena {   // grow-only device buffer
  void* p = nullptr;
  size_t cap = 0;
};

using OpSpec = Op<int64_t>;

struct OpList {   // an operand list as the bodies of rzk_run.cpp take it: lowered addresses and, once, what they point at
  const int64_t* base[kMaxOperands];
  uint32_t stride[kMaxOperands];
  uint32_t outer[kMaxOperands];
  size_t n;         // operands of the list; the bodies refuse more than kMaxOperands (none beyond are held)
  uint32_t width;   // sizeof(C)
};
template <class C>
inline OpList lower(const std::vector<Op<C>>& specs) {
  OpList o;
  o.n = specs.size();
  o.width = sizeof(C);
  for (size_t i = 0; i < o.n && i < (size_t)kMaxOperands; ++i) {
    o.base[i] = launch_addr(specs[i].base);
    o.stride[i] = specs[i].stride;
    o.outer[i] = specs[i].outer;
  }
  return o;
}

}  // namespace api
}  // namespace rzk

using namespace rzk;
using namespace rzk::api;

struct rzk_ctx {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  int num_cus = 256;
  int64_t q = 0;
  uint32_t N = 0, logn = 0, n = 0, k = 0, l = 0, kappa = 0;
  uint64_t b = 0;
  uint64_t sigma = 0, commit_bound = 0, verify_bound = 0;
  DevTables hT{};
  DevTables* dT = nullptr;
  uint32_t* d_tw = nullptr;
  uint32_t* d_row_scratch = nullptr;   // per-wave Garner state of the row kernel (third prime only)
  uint32_t* d_group_scratch = nullptr; // per-wave Garner state of the row-group kernel (allocated on first use)
  uint32_t* d_block_scratch = nullptr; // per-workgroup Garner state of the row-block kernel (allocated on first use)
  uint32_t block_min_logn = 11;        // row blocks from this ring degree on (below it row groups do the sharing)
  bool use_groups = true;
  uint32_t units_per_task = 0;         // 0 = automatic (RZK_UPT overrides, tuning)
  bool vec_rows = true;                // programs with vector x vector products: row_kernel (RZK_VEC_ROWS=0: unit_kernel)
  bool unit_io = false;                // key-product programs through unit_io_kernel (every operand read once): where its sums park in
                                       // LDS (N = 512); RZK_UNIT_IO=0 / 1 forces unit_kernel / unit_io_kernel
  bool pair_poly = true;               // N = 2048: two wavefronts per polynomial (RZK_PAIR_POLY=0: one, the round-2 kernels)
  bool trusted = false;                // rzk_ctx_trust_device_outputs: skip the canonical test of loaded coefficients
  bool use_pairs = true;               // unit_kernel: pair rows that share their last operand (RZK_PAIRS=0 turns it off, tuning)
  bool rot_last = true;                // unit_kernel: rotation terms of single-row units after the transforms, sums in registers (RZK_ROT_LAST=0: first, through the scratch line)
  bool dot2 = true;                    // unit_kernel: two-product key rows park the transform and reduce once (RZK_DOT2=0: one reduction per product)
  bool crt2_short = true;              // two-prime reconstruction with one reduction mod q (RZK_CRT2_SHORT=0: crt2_zq)
  int tw_lds = 0;                      // unit_kernel, one-wavefront teams at N = 1024 (the only size with the images; RZK_TW_LDS): 0 = twiddles from the
                                       // global tables, 1 = phase 2 from an LDS image per four-team workgroup, 2 = phases 2 and 3 from one image per
                                       // sixteen-team workgroup
  int group_max = 1;                   // rows per group of row_group_kernel (group_max_for; RZK_GROUP_MAX overrides, tuning)
  bool use_shift = true;               // challenge products as signed rotations (shift_row_kernel) instead of transforms
  bool shift_bytes = true;             // ... of short operands as packed bytes (shift_row_kernel, N <= 1024; RZK_SHIFT_BYTES=0: words only)
  int use_dkey = 1;                    // the scalar multipliers g_i of Linear / Sum transformed once per proof and call (TERM_DKEY): 0 never (every row
                                       // transforms them itself), 1 when at least kDkeyMinUses rows of the call multiply by each, 2 always (RZK_DKEY)
  Arena ws_dkey;                       // their images + norms
  const uint32_t* dkey_img = nullptr;  // images of the call in progress (set by prepare_dkey, cleared by DkeyScope)
  const double* dkey_l2 = nullptr;
  uint32_t dkey_n = 0;
  bool use_oimg = true;                // Sum proof: the transforms of y_i / z_i that the a1 key products compute anyway are kept for the D rows (RZK_OIMG=0: off)
  Arena ws_oimg;
  Operands oimg_state{};               // oimg* fields of the call in progress (oimg == NULL: none); oimg_op is set per launch
  uint32_t oimg_producer_op = 0xffu;   // != 0xff: the next launches store the images of this operand's columns (OimgProducer)
  bool lin_e = true;                   // Linear verifier: g(.)(a2.z - c2(.)d) - (a2.z' - c2'(.)d) - u == 0 (one product with g; RZK_LIN_E=0: the reference's grouping)
  int sum_d = -1;                      // Sum proof: a2.(sum_i g_i v_i - v') instead of sum_i g_i (a2.v_i) - a2.v' (-1 = by cost, RZK_SUM_D=0|1 forces)
  bool preset_in_kernel = true;        // verdict flags initialised by the unit kernels themselves where one team owns an entry (RZK_PRESET_IN_KERNEL=0: always a fill launch)
  bool small = false;                  // N < 512: schoolbook kernels (rzk_xform.h, "small ring degrees")
  uint32_t r2q = 0;                    // 2^64 mod q
  uint32_t* d_key_mont = nullptr;      // small N: key entries as Montgomery-form residues mod q
  // key
  bool key_loaded = false;
  std::vector<uint8_t> key_class;     // (n+l)*k
  std::vector<int32_t> key_entry;     // index into the NTT-domain store, -1 if not GENERAL
  uint32_t n_general = 0;
  uint32_t* d_key_ntt = nullptr;
  double* d_key_l2 = nullptr;
  std::map<std::pair<int, uint32_t>, DevProg> progs;
  Arena ws, stage, ws_slots;
  Arena ws32;                          // convert path of the 32-bit entry points: the call's slabs widened to int64 (rzk_slab32.cpp)
  Arena ws_wire;                       // message codec: position table (decode) / lengths, positions, sizes (encode)
  Arena ws_fs;                         // Fiat-Shamir transcript: leaf digests of the call (and the key while it is hashed)
  Arena ws_reject;                     // rejection sampling: one RejectPartial per response polynomial of the call
  Arena ws_prove;                      // the prover loops (rzk_prove_loop.cpp): y, retry copies of the masks and responses, d, the gathered
                                       // randomness and commitments, coin draws, flags, idx, count
  uint32_t* h_pending = nullptr;       // ... its pending count of the round, read back once per round (pinned, allocated on first use)
  uint64_t key_digest[kFsDigestWords] = {};   // FS1 digest of the loaded key and the context's parameters (rzk_fs_key_digest)
  bool sampler_key_set = false;                // rzk_sampler_set_key: the key of the keyed (ChaCha20) samplers, host memory only;
  uint8_t sampler_key[32] = {};                // wiped when it is cleared and in rzk_ctx_destroy
  // canonical-input test (rzk_dev.h, Operands::bad): sticky word set by any kernel that loaded a coefficient
  // outside the centred range on behalf of an entry point without per-proof verdicts; read back at every
  // synchronising call (host-pointer variants, rzk_ctx_synchronize, rzk_ctx_check_inputs)
  uint32_t* d_bad = nullptr;
  uint32_t* h_bad = nullptr;   // pinned
  double slot_share_min = 2.0;   // use the shared-operand path when (operand transforms) / (distinct operands) >= this
  std::string err;
  // profiling of the row kernel with HIP events on the launch stream
  bool prof = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_events;
  struct ProfInfo {
    std::string kernel;     // the kernel template instance the launch ran
    uint64_t bytes = 0;     // algorithmic bytes of the launch: (8 or 4) N x (distinct polynomials read + rows stored)
  };
  std::vector<ProfInfo> prof_info;   // parallel to the used part of prof_events
  size_t prof_used = 0;
  double prof_us = 0.0;
  uint64_t prof_launches = 0;
};

#define HIPCHK(ctx, expr)                                                                        \
  do {                                                                                           \
    hipError_t e_ = (expr);                                                                      \
    if (e_ != hipSuccess) {                                                                      \
      (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                            \
      return RZK_E_HIP;                                                                          \
    }                                                                                            \
  } while (0)

namespace rzk {
namespace api __attribute__((visibility("hidden"))) {

// ---- rzk_ctx.cpp ---------------------------------------------------------------------------------------------------
int fail(rzk_ctx* c, int code, const char* msg);
void wipe(void* p, size_t n);   // zeroes secret bytes through a volatile pointer, so that the stores are not removed as dead
LaunchCfg cfg_of(rzk_ctx* c);
int arena_reserve(rzk_ctx* c, Arena& a, size_t bytes);
int check_launch(rzk_ctx* c, int lrc, const char* what);
int take_input_error(rzk_ctx* c);   // synchronises and reports (then clears) the sticky input-error word
template <class C = int64_t>
inline size_t polys(const rzk_ctx* c, size_t count) { return poly_bytes<C>(c->N, count); }   // bytes of `count` polynomials
// 32-bit device slabs are 16-byte aligned (rzk_slab32.h); the 64-bit entry points have no such rule
// (the calls with a slab list: slabs_misaligned below; this form serves the one-output samplers)
inline bool misaligned(std::initializer_list<const void*> slabs) {
  uintptr_t bits = 0;
  for (const void* p : slabs) bits |= reinterpret_cast<uintptr_t>(p);
  return (bits & 15u) != 0;
}
inline int align_fail(rzk_ctx* c) { return fail(c, RZK_E_ARG, "slab32: device slabs must be 16-byte aligned"); }

// ---- rzk_run.cpp: row programs, norm kernels, the images of a call ----------------------------------------------------
void drop_programs(rzk_ctx* c);
int prof_begin(rzk_ctx* c, uint64_t bytes, LaunchCfg& cfg);
int prof_end(rzk_ctx* c);
// one launch in a profiling slot of its own: launch(cfg) returns the launcher's status
template <class L>
int run_profiled(rzk_ctx* c, uint64_t bytes, const char* what, L launch) {
  LaunchCfg cfg;
  int rc = prof_begin(c, bytes, cfg);
  if (rc == RZK_OK) rc = check_launch(c, launch(cfg), what);
  return rc != RZK_OK ? rc : prof_end(c);
}
bool shift_ok(const rzk_ctx* c);
bool response_stat_fused(const rzk_ctx* c);
// The operands' coefficient type says which kernels run.  C defaults to int64_t where the list is written in braces at the
// call (a list of int32_t slabs then does not compile); a named std::vector<Op<C>> brings its own.  int32_t: the program
// must have native 32-bit kernels on this context (program_native32, asked by the entry point before its first launch).
int run_program_lowered(rzk_ctx* c, int id, uint32_t var, const OpList& specs, uint8_t* flags, uint32_t group, uint64_t batch,
                        uint64_t norm_limit, bool sticky, uint8_t preset_value, uint64_t nflags, const ResponseStat* stat);
template <class C = int64_t>
inline int run_program(rzk_ctx* c, int id, uint32_t var, const std::vector<Op<C>>& specs, uint8_t* flags, uint32_t group,
                       uint64_t batch, uint64_t norm_limit = 0, bool sticky = true, uint8_t preset_value = 0, uint64_t nflags = 0,
                       const ResponseStat* stat = nullptr) {
  return run_program_lowered(c, id, var, lower(specs), flags, group, batch, norm_limit, sticky, preset_value, nflags, stat);
}
bool program_native32(rzk_ctx* c, int id, uint32_t var);
// the fused (var | 1) form of a checked program can run on this context with this bound (run_checked then takes no fallback)
bool checked_fuses(rzk_ctx* c, int id, uint32_t var, uint64_t bound);
// run_checked of this program runs natively on 32-bit slabs whichever side it takes: the plain form (the fallback, and the
// call without flags), the stand-alone norm kernel and, where the program has one, the fused form
bool checked_native32(rzk_ctx* c, int id, uint32_t var, uint64_t bound, bool has_flags);
bool norm_native32(const rzk_ctx* c);   // run_norm<int32_t> has a kernel on this context (N = 512 / 1024)
template <class C>
int run_norm(rzk_ctx* c, const C* v, uint32_t rows, uint64_t bound, uint8_t* ok, uint64_t B, int mode, int shift, bool sticky = true);
struct NormSpec {   // one launch of the norm kernel: flags (mode, shift) sum c^2 of v's `rows` polynomials per flag < (bound+1)^2
  const void* v;   // the slab, int64_t or int32_t coefficients: its width is that of the program's operand list
  uint32_t rows;
  int mode, shift;   // launch_norm: 0 = overwrite, 1 = and, 2 = or (result << shift)
};
int run_checked_lowered(rzk_ctx* c, int id, uint32_t var, const OpList& specs, uint8_t* flags, uint32_t group, uint64_t batch,
                        uint64_t nflags, uint64_t bound, bool preset, bool sticky, std::initializer_list<NormSpec> norms);
template <class C = int64_t>
inline int run_checked(rzk_ctx* c, int id, uint32_t var, const std::vector<Op<C>>& specs, uint8_t* flags, uint32_t group,
                       uint64_t batch, uint64_t nflags, uint64_t bound, bool preset, bool sticky,
                       std::initializer_list<NormSpec> norms) {
  return run_checked_lowered(c, id, var, lower(specs), flags, group, batch, nflags, bound, preset, sticky, norms);
}
bool dkey_wanted(const rzk_ctx* c, uint32_t uses);   // prepare_dkey would build images for a call with `uses` rows per multiplier
int prepare_dkey(rzk_ctx* c, const int64_t* g, uint64_t entries, uint32_t per_entry, uint32_t uses, uint8_t* flags, bool sticky);
int prepare_oimg(rzk_ctx* c, uint64_t B, uint32_t V, uint32_t uses);
bool sum_uses_d(const rzk_ctx* c, uint32_t V);
// variant bits of programs that multiply by the call's multiplier images / read its operand images
inline uint32_t dkv(const rzk_ctx* c) { return c->dkey_img ? kDkeyVar : 0u; }
inline uint32_t oiv(const rzk_ctx* c) { return (c->oimg_state.oimg && c->dkey_img) ? kOimgVar : 0u; }

// The images prepare_dkey / prepare_oimg leave in the context belong to one call: the entry point declares the guard
// right after the prepare call, and whichever way it returns the next call starts without images.
struct DkeyScope {
  rzk_ctx* c;
  ~DkeyScope() { c->dkey_img = nullptr; c->dkey_l2 = nullptr; c->dkey_n = 0; }
};
struct OimgScope {
  rzk_ctx* c;
  ~OimgScope() { c->oimg_state = Operands{}; c->oimg_producer_op = 0xffu; }
};
// while it lives, the launches of the call store the images of operand `op`'s columns (prepare_oimg has made room)
struct OimgProducer {
  rzk_ctx* c;
  OimgProducer(rzk_ctx* ctx, uint32_t op) : c(ctx) { c->oimg_producer_op = op; }
  ~OimgProducer() { c->oimg_producer_op = 0xffu; }
};

// ---- a call's slab list (rzk_slabs.h) at work -----------------------------------------------------------------------
// Every entry point passes its pointers as it declares them, with its list S: what follows, and host_run below, are the only
// places that turn a list into a NULL test, an alignment test, a convert plan or a staging plan.  A pointer whose constness
// disagrees with its slab's role, or a list of another length, does not compile.
struct SizeArgs {   // the call's own size arguments (SlabDims) and whether they obey its rule: V >= 1, rows >= 1, a key selector
  uint64_t V = 1, rows = 0;
  int which = -1;   // >= 0: rows = the key rows it selects
  bool ok = true;
};
inline SizeArgs by_V(uint64_t V) { return {V, 0, -1, V != 0}; }
inline SizeArgs by_rows(uint64_t rows) { return {1, rows, -1, rows != 0}; }
inline SizeArgs by_key(int which) { return {1, 0, which, is_key_selector(which)}; }
inline SlabDims dims_of(const rzk_ctx* c, const SizeArgs& a = {}) {
  return {c->n, c->k, c->l, a.V, a.which >= 0 ? key_row_count(a.which, c->n, c->l) : a.rows};
}
template <const CallSlabs& S, class... P>
constexpr bool slab_types_ok() {
  if (sizeof...(P) != slab_len(S)) return false;
  const bool reads[] = {std::is_const_v<P>...};
  for (size_t i = 0; i < sizeof...(P); ++i)
    if (reads[i] != slab_reads(S.s[i].role)) return false;
  return true;
}
template <const CallSlabs& S, class... P>
inline bool slabs_null(P*... p) {   // a required pointer is NULL
  static_assert(slab_types_ok<S, P...>(), "the pointers of the call are not its slab list");
  const void* const a[] = {p...};
  for (size_t i = 0; i < sizeof...(P); ++i)
    if (!a[i] && !slab_optional(S.s[i].role)) return true;
  return false;
}
template <const CallSlabs& S, class... P>
inline bool slabs_misaligned(P*... p) {   // a coefficient slab is not 16-byte aligned (the companions have no such rule)
  static_assert(slab_types_ok<S, P...>(), "the pointers of the call are not its slab list");
  const void* const a[] = {p...};
  uintptr_t bits = 0;
  for (size_t i = 0; i < sizeof...(P); ++i)
    if (slab_is_coef(S.s[i].kind)) bits |= reinterpret_cast<uintptr_t>(a[i]);
  return (bits & 15u) != 0;
}
// The argument rules every call without error texts of its own shares, in the order include/rzk.h gives them: an empty
// batch is a no-op whatever the pointers; a NULL context, a NULL required pointer or a size argument that breaks its rule
// (sz.ok) is RZK_E_ARG.  kGo: the call goes on; it is no status of include/rzk.h, which are RZK_OK = 0 and negative codes.
constexpr int kGo = 1;
static_assert(RZK_OK == 0 && RZK_E_ARG < 0 && RZK_E_UNSUPPORTED < 0 && RZK_E_STATE < 0 && RZK_E_HIP < 0, "kGo is no status code");
template <const CallSlabs& S, class... P>
inline int slab_args(const rzk_ctx* c, const SizeArgs& sz, size_t B, P*... p) {
  if (c && B == 0) return RZK_OK;
  return !c || !sz.ok || slabs_null<S>(p...) ? RZK_E_ARG : kGo;
}
inline int split_check(rzk_ctx* c) {   // the verifiers and recompute steps split c into c1, c2
  return c->n == c->l ? RZK_OK : fail(c, RZK_E_ARG, "c1_c2 split needs n == l (reference panics in Mat::add)");
}

// ---- rzk_slab32.cpp: the convert path of a 32-bit call ----------------------------------------------------------------
// The call's coefficient slabs as int64_t copies in ws32: convert_call reserves the arena and widens every slab the list
// reads, runs body — the call's own body on int64_t, with the pointers of the call in declaration order, every int32_t
// slab replaced by its copy (NULL for an absent one) and every companion as it came — and narrows every slab it writes.
struct Conv {   // one slab of the call, `count` polynomials: read (in), written (out), or absent (neither)
  const int32_t* in;
  int32_t* out;
  size_t count;
};
int convert_begin(rzk_ctx* c, const Conv* slabs, size_t n, int64_t** wide);
int convert_end(rzk_ctx* c, const Conv* slabs, size_t n, int64_t* const* wide);
template <const CallSlabs& S, class F, class... P>
int convert_call(rzk_ctx* c, const SizeArgs& sz, size_t B, F body, P*... p) {
  static_assert(slab_types_ok<S, P...>(), "the pointers of the call are not its slab list");
  constexpr size_t K = sizeof...(P);
  const SlabDims dm = dims_of(c, sz);
  const CallSlabs& list = S;   // (the lambdas index this, not S: hipcc of ROCm 7.2 crashes on S.s[i] inside a generic lambda)
  size_t i = 0;
  auto conv = [&](auto* q) -> Conv {
    const Slab& s = list.s[i++];
    const size_t count = B * slab_count(s.kind, dm);
    if constexpr (std::is_same_v<decltype(q), const int32_t*>) return {q, nullptr, count};
    else if constexpr (std::is_same_v<decltype(q), int32_t*>) return {nullptr, q, count};
    else return {nullptr, nullptr, 0};
  };
  const Conv slabs[K] = {conv(p)...};   // (braces: in the order of the list)
  int64_t* wide[K];
  int rc = convert_begin(c, slabs, K, wide);
  if (rc != RZK_OK) return rc;
  i = 0;
  auto pick = [&](auto* q) {
    using T = std::remove_pointer_t<decltype(q)>;
    int64_t* const w = wide[i++];
    if constexpr (std::is_same_v<T, const int32_t>) return static_cast<const int64_t*>(w);
    else if constexpr (std::is_same_v<T, int32_t>) return w;
    else return q;
  };
  const std::tuple<decltype(pick(p))...> args{pick(p)...};
  rc = std::apply(body, args);
  return rc != RZK_OK ? rc : convert_end(c, slabs, K, wide);
}

// ---- the typed *_dev entry points another translation unit calls (rzk_prove_loop.cpp), C = int64_t or int32_t; the
// siblings' extern "C" symbols forward to them.  Defined, and instantiated for both, in the file named.
// (RZK_BOTH_WIDTHS(fn), rzk_dev.h: the typed launchers are instantiated the same way)
// rzk_protocols.cpp
template <class C> int open_commit_dev(rzk_ctx* c, const C* x, const C* r, const C* y, C* cm, C* t, uint8_t* ok, size_t B);
template <class C> int matvec_dev(rzk_ctx* c, int which, const C* v, const C* addend, C* out, size_t B);
// rzk_samplers.cpp
template <class C> int sample_uniform_keyed_dev(rzk_ctx* c, const uint8_t* nonce, uint32_t stream, uint64_t bound, C* out, size_t count);
template <class C> int sample_gauss_keyed_dev(rzk_ctx* c, const uint8_t* nonce, uint32_t stream, double sigma, C* out, size_t count);
template <class C> int sample_dgauss_keyed_dev(rzk_ctx* c, const uint8_t* nonce, uint32_t stream, uint32_t sigma, C* out, size_t count);
template <class C> int sample_challenge_keyed_dev(rzk_ctx* c, const uint8_t* nonce, uint32_t stream, C* out, size_t count);
// rzk_codec.cpp
template <class C> int fs_challenge_dev(rzk_ctx* c, int kind, uint32_t V, const C* const* fields, const uint8_t* aux32, C* d,
                                        uint8_t* digest, uint8_t* ok, size_t B);
template <class C> int open_response_reject_dev(rzk_ctx* c, const C* y, const C* r, const C* d, const int64_t* coin, uint64_t R,
                                                double lnM, C* z, uint8_t* accept, int64_t* E, size_t B);
// out[b][r] = polynomial p0 + r of XP1 under seeds[b] and `domain`; seeds and out on the device
int run_xof(rzk_ctx* c, uint32_t domain, uint32_t p0, uint32_t rows, const uint64_t* seeds, int64_t* out, size_t B);

// ---- rzk_host.cpp: one host-pointer call ------------------------------------------------------------------------------
// The buffers of the call are declared first (in / out / scratch return typed device pointers that become valid once the
// staging arena is reserved), then run() does, in stream order: clear the sticky input-error word (a fault left by
// earlier *_dev calls whose caller never asked — rzk_ctx_check_inputs — is dropped here, as include/rzk.h documents),
// reserve the arena and copy the inputs in, call the *_dev entry point; when that fails, consume the sticky word so that
// it never leaks into the next call, keep the first error text and return the first status; otherwise copy the outputs
// back, synchronise and report the sticky word: a host-pointer call reports exactly its own input faults.
class HostCall {
 public:
  template <class T>
  class Dev {   // NULL host pointer: no bytes are staged and the device pointer is NULL too
   public:
    Dev() = default;
    operator T*() const { return off_ == kNull ? nullptr : (T*)((char*)arena_->p + off_); }
   private:
    friend class HostCall;
    Dev(const Arena* a, size_t off) : arena_(a), off_(off) {}
    const Arena* arena_ = nullptr;
    size_t off_ = kNull;
  };
  explicit HostCall(rzk_ctx* c) : c_(c) {}
  template <class T> Dev<const T> in(const T* host, size_t bytes) { return {&c_->stage, add(host, nullptr, bytes, !host)}; }
  template <class T> Dev<T> out(T* host, size_t bytes) { return {&c_->stage, add(nullptr, host, bytes, !host)}; }
  template <class T> Dev<T> scratch(size_t bytes) { return {&c_->stage, add(nullptr, nullptr, bytes, false)}; }
  template <class C> Dev<const C> pin(const C* host, size_t count) { return in(host, polys<C>(c_, count)); }   // count polynomials
  template <class C> Dev<C> pout(C* host, size_t count) { return out(host, polys<C>(c_, count)); }
  // for pointer tables (the slabs of a message's fields): *slot receives the device pointer when the arena is staged
  template <class C> void in_to(const C** slot, const C* host, size_t bytes) { add(host, nullptr, bytes, !host, slot, &set_slot<const C>); }
  template <class C> void out_to(C** slot, C* host, size_t bytes) { add(nullptr, host, bytes, !host, slot, &set_slot<C>); }
  int stage();   // reserve and fill the arena only (callers without the sticky-word protocol)
  template <class F>
  int run(F dev_call) {
    int rc = begin();
    return rc != RZK_OK ? rc : end(dev_call());
  }
 private:
  static constexpr size_t kNull = ~size_t(0);
  struct Buf {
    const void* in;   // host source (nullptr for pure outputs)
    void* out;        // host destination (nullptr for pure inputs)
    size_t bytes, off;
    void* slot;                    // in_to / out_to: the caller's T*, written by set(slot, device pointer)
    void (*set)(void*, void*);
  };
  template <class T> static void set_slot(void* slot, void* p) { *static_cast<T**>(slot) = static_cast<T*>(p); }
  size_t add(const void* in, void* out, size_t bytes, bool null, void* slot = nullptr, void (*set)(void*, void*) = nullptr);
  int begin();
  int end(int rc);
  rzk_ctx* c_;
  std::vector<Buf> bufs_;
  size_t total_ = 0;
};

// The host form of a call with the list S: every pointer staged by its slab's role, kind and the pointer's own coefficient
// width, then dev(the staged pointers, typed and in declaration order) under HostCall::run.  The caller has refused what
// the call refuses: nothing here fails before the stream is touched.
template <const CallSlabs& S, class F, class... P>
int host_run(rzk_ctx* c, const SizeArgs& sz, size_t B, F dev, P*... p) {
  static_assert(slab_types_ok<S, P...>(), "the pointers of the call are not its slab list");
  const SlabDims dm = dims_of(c, sz);
  const CallSlabs& list = S;   // (as in convert_call)
  HostCall h(c);
  size_t i = 0;
  auto stage = [&](auto* q) {
    using T = std::remove_pointer_t<decltype(q)>;
    const Slab& s = list.s[i++];
    size_t bytes = B * slab_count(s.kind, dm);   // of a companion; a coefficient slab: polynomials of its pointer's width
    if constexpr (is_coef<std::remove_const_t<T>>) {
      if (slab_is_coef(s.kind)) bytes = polys<std::remove_const_t<T>>(c, bytes);
    }
    if constexpr (std::is_const_v<T>) return h.in(q, bytes);
    else return h.out(q, bytes);
  };
  const std::tuple<HostCall::Dev<P>...> staged{stage(p)...};   // (braces: in the order of the list)
  return h.run([&] { return std::apply([&](const auto&... d) { return dev(static_cast<P*>(d)...); }, staged); });
}
// ... with the argument rules of slab_args in front
template <const CallSlabs& S, class F, class... P>
int host_call(rzk_ctx* c, const SizeArgs& sz, size_t B, F dev, P*... p) {
  const int rc = slab_args<S>(c, sz, B, p...);
  return rc != kGo ? rc : host_run<S>(c, sz, B, dev, p...);
}
// the two common shapes: dev(c, slabs..., B), and dev(c, lead, slabs..., B) with the call's V or key selector in front
template <class T> struct AsGiven { using type = T; };   // (dev's type follows from the pointers: it is not deduced itself)
template <const CallSlabs& S, class... P>
int host_form(rzk_ctx* c, size_t B, typename AsGiven<int (*)(rzk_ctx*, P*..., size_t)>::type dev, P*... p) {
  return host_call<S>(c, {}, B, [&](P*... d) { return dev(c, d..., B); }, p...);
}
template <const CallSlabs& S, class A, class... P>
int host_form(rzk_ctx* c, const SizeArgs& sz, size_t B, A lead, typename AsGiven<int (*)(rzk_ctx*, A, P*..., size_t)>::type dev,
              P*... p) {
  return host_call<S>(c, sz, B, [&](P*... d) { return dev(c, lead, d..., B); }, p...);
}

}  // namespace api
}  // namespace rzk
