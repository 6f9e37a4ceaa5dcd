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

// ---- rzk_slab32.cpp: the convert path of a 32-bit call ----------------------------------------------------------------
// The call's slabs as int64_t copies in ws32: convert_call reserves the arena and widens every `in`, runs body(wide) —
// the call's own body on int64_t, wide[i] the copy of slab i (NULL for an absent one) — and narrows every `out`.
struct Conv {   // one slab of the call, `count` polynomials: read (in), written (out), or absent (neither)
  const int32_t* in;
  int32_t* out;
  size_t count;
};
int convert_begin(rzk_ctx* c, const Conv* slabs, size_t n, int64_t** wide);
int convert_end(rzk_ctx* c, const Conv* slabs, size_t n, int64_t* const* wide);
template <size_t K, class F>
int convert_call(rzk_ctx* c, const Conv (&slabs)[K], F body) {
  int64_t* wide[K];
  int rc = convert_begin(c, slabs, K, wide);
  if (rc == RZK_OK) rc = body(wide);
  return rc != RZK_OK ? rc : convert_end(c, slabs, K, wide);
}

// ---- the *_dev entry points that exist at both widths, C = int64_t or int32_t (the siblings' extern "C" symbols forward
// here; rzk_prove_loop.cpp calls them typed).  Defined, and instantiated for both, in the file named.
// (RZK_BOTH_WIDTHS(fn), rzk_dev.h: the typed launchers are instantiated the same way)
// rzk_protocols.cpp
template <class C> int open_commit_dev(rzk_ctx* c, const C* x, const C* r, const C* y, C* cm, C* t, uint8_t* ok, size_t B);
template <class C> int open_response_dev(rzk_ctx* c, const C* y, const C* r, const C* d, C* z, size_t B);
template <class C> int open_a1_relation_dev(rzk_ctx* c, const C* z, const C* t, const C* cm, const C* d, uint8_t* accept, size_t B,
                                            bool recover);   // verify; recover: t is the output
template <class C> int matvec_dev(rzk_ctx* c, int which, const C* v, const C* addend, C* out, size_t B);
template <class C> int norm2_le_dev(rzk_ctx* c, const C* v, uint32_t rows, uint64_t bound, uint8_t* ok, size_t B);
template <class C> int linear_commit_dev(rzk_ctx* c, const C* g, const C* x, const C* r, const C* rp, const C* y, const C* yp, C* cm, C* cpm,
                                         C* t, C* tp, C* u, uint8_t* ok, size_t B);
template <class C> int linear_mask_dev(rzk_ctx* c, const C* g, const C* y, const C* yp, C* t, C* tp, C* u, size_t B);
template <class C> int linear_response_dev(rzk_ctx* c, const C* y, const C* yp, const C* r, const C* rp, const C* d, C* z, C* zp, size_t B);
template <class C> int linear_verify_dev(rzk_ctx* c, const C* z, const C* zp, const C* cm, const C* cpm, const C* g, const C* t,
                                         const C* tp, const C* u, const C* d, uint8_t* accept, size_t B);
template <class C> int linear_recover_dev(rzk_ctx* c, const C* z, const C* zp, const C* cm, const C* cpm, const C* g, const C* d, C* t_out,
                                          C* tp_out, C* u_out, uint8_t* accept, size_t B);
// rzk_samplers.cpp
template <class C> int sample_uniform_keyed_dev(rzk_ctx* c, const uint8_t* nonce, uint32_t stream, uint64_t bound, C* out, size_t count);
template <class C> int sample_gauss_keyed_dev(rzk_ctx* c, const uint8_t* nonce, uint32_t stream, double sigma, C* out, size_t count);
template <class C> int sample_dgauss_keyed_dev(rzk_ctx* c, const uint8_t* nonce, uint32_t stream, uint32_t sigma, C* out, size_t count);
template <class C> int sample_challenge_keyed_dev(rzk_ctx* c, const uint8_t* nonce, uint32_t stream, C* out, size_t count);
// rzk_codec.cpp
template <class C> int fs_challenge_dev(rzk_ctx* c, int kind, uint32_t V, const C* const* fields, const uint8_t* aux32, C* d,
                                        uint8_t* digest, uint8_t* ok, size_t B);
template <class C> int linear_response_reject_dev(rzk_ctx* c, const C* y, const C* yp, const C* r, const C* rp, const C* d,
                                                  const int64_t* coin, uint64_t R, double lnM, C* z, C* zp, uint8_t* accept, int64_t* E,
                                                  size_t B);
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

}  // namespace api
}  // namespace rzk
