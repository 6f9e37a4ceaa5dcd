// rzk_api.cpp — the C ABI declared in include/rzk.h: context, resident key, row programs of every
// protocol phase, host-pointer wrappers.  Compiled with hipcc together with rzk_kernels.hip into
// ring_zk_amd/librzk_hip.so.  There is no CPU fallback anywhere in this file: every entry point
// launches HIP kernels on the context's device or returns an error status.
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
#include "rzk_core.h"
#include "rzk_dev.h"
#include "rzk_dgauss.h"
#include "rzk_keccak.h"
#include "rzk_packed.h"
#include "rzk_plan.h"
#include "rzk_reject.h"
#include "rzk_tables.h"
#include "rzk_xof.h"

using namespace rzk;

// plan_program speaks the C ABI's status codes, PG_MATVEC its key selectors
static_assert(kPlanOk == RZK_OK && kPlanArg == RZK_E_ARG && kPlanUnsupported == RZK_E_UNSUPPORTED, "plan status codes");
static_assert(RZK_KEY_A1 == 0 && RZK_KEY_A2 == 1 && RZK_KEY_A == 2, "key selectors");

namespace {

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

}  // namespace

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
  int group_max = 1;                   // rows per group of row_group_kernel (group_max_for; RZK_GROUP_MAX overrides, tuning)
  bool use_shift = true;               // challenge products as signed rotations (shift_row_kernel) instead of transforms
  bool shift_bytes = true;             // ... of short operands as packed bytes (shift_row_kernel, N <= 1024; RZK_SHIFT_BYTES=0: words only)
  int use_dkey = 1;                    // the scalar multipliers g_i of Linear / Sum transformed once per proof and call (TERM_DKEY): 0 never (every row
                                       // transforms them itself), 1 when at least kDkeyMinUses rows of the call multiply by each, 2 always (RZK_DKEY)
  Arena ws_dkey;                       // their images + norms
  const uint32_t* dkey_img = nullptr;  // images of the call in progress (set by prepare_dkey, cleared by the entry point)
  const double* dkey_l2 = nullptr;
  uint32_t dkey_n = 0;
  bool use_oimg = true;                // Sum proof: the transforms of y_i / z_i that the a1 key products compute anyway are kept for the D rows (RZK_OIMG=0: off)
  Arena ws_oimg;
  Operands oimg_state{};               // oimg* fields of the call in progress (oimg == NULL: none); oimg_op is set per launch
  uint32_t oimg_producer_op = 0xffu;   // != 0xff: the next launches store the images of this operand's columns
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
  Arena ws_wire;                       // message codec: position table (decode) / lengths, positions, sizes (encode)
  Arena ws_fs;                         // Fiat-Shamir transcript: leaf digests of the call (and the key while it is hashed)
  Arena ws_reject;                     // rejection sampling: one RejectPartial per response polynomial of the call
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
    uint64_t bytes = 0;     // algorithmic bytes of the launch: 8 N x (distinct polynomials read + rows stored)
  };
  std::vector<ProfInfo> prof_info;   // parallel to the used part of prof_events
  size_t prof_used = 0;
  double prof_us = 0.0;
  uint64_t prof_launches = 0;
};

namespace {

#define HIPCHK(ctx, expr)                                                                        \
  do {                                                                                           \
    hipError_t e_ = (expr);                                                                      \
    if (e_ != hipSuccess) {                                                                      \
      (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                            \
      return RZK_E_HIP;                                                                          \
    }                                                                                            \
  } while (0)

std::string g_create_err;   // last rzk_ctx_create failure (no context exists yet to hold it)

int create_fail(int code, const std::string& msg) {
  g_create_err = msg;
  return code;
}

// zeroes secret bytes through a volatile pointer, so that the stores are not removed as dead
void wipe(void* p, size_t n) {
  volatile uint8_t* v = (volatile uint8_t*)p;
  for (size_t i = 0; i < n; ++i) v[i] = 0;
}

int fail(rzk_ctx* c, int code, const char* msg) {
  if (c) c->err = msg;
  return code;
}

uint64_t isqrt_u64(uint64_t x) {
  uint64_t r = (uint64_t)std::sqrt((long double)x);
  while ((unsigned __int128)r * r > x) --r;
  while ((unsigned __int128)(r + 1) * (r + 1) <= x) ++r;
  return r;
}

LaunchCfg cfg_of(rzk_ctx* c) {
  (void)hipSetDevice(c->device);   // the calling thread may have another current device
  return LaunchCfg{(void*)c->stream, c->num_cus, c->pair_poly ? 1 : 0, c->unit_io ? 1 : 0, c->shift_bytes ? 1 : 0};
}

int arena_reserve(rzk_ctx* c, Arena& a, size_t bytes) {
  if (bytes <= a.cap) return RZK_OK;
  // grow-only; happens outside steady state.  The old block may still be in use by queued work.
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (a.p) HIPCHK(c, hipFree(a.p));
  a.p = nullptr;
  a.cap = 0;
  size_t want = bytes + bytes / 4;
  HIPCHK(c, hipMalloc(&a.p, want));
  a.cap = want;
  return RZK_OK;
}

// Challenge products as signed rotations (shift-add) instead of transforms.  At N = 2048 only with two wavefronts
// per polynomial (16 outputs per thread): with one, a lane holds 32 outputs, the rotation kernels need > 200 VGPRs
// (one or two waves per SIMD) and measured slower than the transform path (round 2).
bool shift_ok(const rzk_ctx* c) { return c->use_shift && !c->small && (c->logn <= 10 || c->pair_poly); }

// ---- row programs: planned on the host (rzk_plan.h), uploaded once per (program, shape) --------------------------
PlanEnv plan_env(const rzk_ctx* c) {
  return PlanEnv{c->n, c->k, c->l, c->logn, c->small, shift_ok(c), c->block_min_logn, c->use_groups, c->group_max,
                 c->use_pairs, c->slot_share_min, c->key_class.data(), c->key_entry.data()};
}

template <class T>
int upload(rzk_ctx* c, const T* host, T** dev) {
  HIPCHK(c, hipMalloc((void**)dev, sizeof(T)));
  HIPCHK(c, hipMemcpyAsync(*dev, host, sizeof(T), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));   // the host table goes away with its plan; one-off per (program, shape)
  return RZK_OK;
}

void free_program(DevProg& dp) {
  if (dp.d) (void)hipFree(dp.d);
  if (dp.d_slots) (void)hipFree(dp.d_slots);
  if (dp.d_blocks) (void)hipFree(dp.d_blocks);
  if (dp.d_wp) (void)hipFree(dp.d_wp);
}

int get_program(rzk_ctx* c, int id, uint32_t var, DevProg& out) {
  const bool needs_key = !(id == PG_POLYMUL || id == PG_CMUL || id == PG_RESPONSE || id == PG_SUM_XP ||
                           id == PG_SUM_W2 || id == PG_REL_ROT);   // (PG_SUM_D reads the key's classification)
  if (needs_key && !c->key_loaded) return fail(c, RZK_E_STATE, "commitment key not loaded");
  auto it = c->progs.find({id, var});
  if (it != c->progs.end()) {
    out = it->second;
    return RZK_OK;
  }
  std::unique_ptr<Plan> plan(new Plan);
  int rc = plan_program(plan_env(c), id, var, *plan);
  // (without a message: a fused-check variant that cannot cover every polynomial; the caller keeps the separate norm kernel)
  if (rc == RZK_E_UNSUPPORTED) return plan->overflow ? fail(c, rc, "shape exceeds row-program capacity") : rc;
  if (rc != RZK_OK) return fail(c, rc, "unknown program");
  DevProg dp;
  static_cast<PlanFacts&>(dp) = plan->f;
  if (plan->use_blocks) rc = upload(c, &plan->blocks, &dp.d_blocks);
  if (rc == RZK_OK) rc = upload(c, &plan->prog, &dp.d);
  if (rc == RZK_OK && plan->use_wave) rc = upload(c, &plan->wave, &dp.d_wp);
  if (rc == RZK_OK && plan->use_slots) rc = upload(c, &plan->slots, &dp.d_slots);
  if (rc != RZK_OK) {
    free_program(dp);
    return rc;
  }
  c->progs[{id, var}] = dp;
  out = dp;
  return RZK_OK;
}


void drop_programs(rzk_ctx* c) {
  for (auto& kv : c->progs) free_program(kv.second);
  c->progs.clear();
}

struct OpSpec {
  const int64_t* base;
  uint32_t stride;
  uint32_t outer;   // 0: indexed by the task batch index; otherwise by the proof index b / group
};

// `group` > 1: the batch is B*group (proof, summand) pairs; operands with outer != 0 and the flags are per proof
// sticky: a non-canonical input coefficient fails the CALL (prover-side / Mat-level entry points); verifier-side
// programs pass false — there the offending proof's verdict flag is cleared and the call succeeds.
int check_launch(rzk_ctx* c, int lrc, const char* what);

// Profiling of one launch (rzk_prof_*): prof_begin records the start event and returns a launch configuration whose
// `launched` points at the slot's kernel name, which the launcher fills in; prof_end records the stop event and only
// then counts the slot.  A failed launch returns before prof_end, so rzk_prof_read* never meets a half-recorded slot.
// A launcher that has nothing to do (empty batch, no rows) starts no kernel and writes no name: prof_end does not count
// such a slot either.
int prof_begin(rzk_ctx* c, uint64_t bytes, LaunchCfg& cfg) {
  cfg = cfg_of(c);
  if (!c->prof) return RZK_OK;
  if (c->prof_used == c->prof_events.size()) {
    hipEvent_t a, b;
    // no system-scope fence at the events: a default event flushes the caches to make results visible to the
    // host, which slows the NEXT kernel (measured 138 -> 162 us for the commit rows)
    HIPCHK(c, hipEventCreateWithFlags(&a, hipEventDisableSystemFence));
    const hipError_t eb = hipEventCreateWithFlags(&b, hipEventDisableSystemFence);
    if (eb != hipSuccess) (void)hipEventDestroy(a);
    HIPCHK(c, eb);
    c->prof_events.push_back({a, b});
  }
  if (c->prof_info.size() <= c->prof_used) c->prof_info.resize(c->prof_used + 1);
  rzk_ctx::ProfInfo& pi = c->prof_info[c->prof_used];
  pi.kernel.clear();
  pi.bytes = bytes;
  cfg.launched = &pi.kernel;
  HIPCHK(c, hipEventRecord(c->prof_events[c->prof_used].first, c->stream));
  return RZK_OK;
}
int prof_end(rzk_ctx* c) {
  if (!c->prof || c->prof_info[c->prof_used].kernel.empty()) return RZK_OK;
  HIPCHK(c, hipEventRecord(c->prof_events[c->prof_used].second, c->stream));
  c->prof_used++;
  return RZK_OK;
}

// preset_value != 0: every verdict flag (nflags of them) starts at that value — written by the launch itself when one
// team evaluates all rows of a batch entry (no 5-us fill launch in front of a 75-us kernel), by a fill launch otherwise.
int run_program(rzk_ctx* c, int id, uint32_t var, const std::vector<OpSpec>& specs, uint8_t* flags,
                uint32_t group, uint64_t batch, uint64_t norm_limit = 0, bool sticky = true, uint8_t preset_value = 0,
                uint64_t nflags = 0) {
  DevProg dp;
  int rc = get_program(c, id, var, dp);
  if (rc != RZK_OK) return rc;
  if (specs.size() > (size_t)kMaxOperands) return fail(c, RZK_E_ARG, "too many operands");
  // units of one batch entry per task: all of them (one team per entry: equal-cost tasks, no tail) once the batch alone
  // fills the chip's wave slots; one unit per task below that
  uint32_t upt = batch >= (uint64_t)c->num_cus * 16 ? dp.nunits : 1;
  if (c->units_per_task) upt = c->units_per_task;   // RZK_UPT (tuning)
  const Path path = path_of(dp, c->small, c->vec_rows);
  const bool preset_in_kernel = preset_value && flags && c->preset_in_kernel && path == Path::Units && upt >= dp.nunits && dp.nunits > 0 &&
                                (group ? group : 1) == 1 && nflags == batch;
  if (preset_value && flags && !preset_in_kernel) {
    rc = check_launch(c, launch_fill_u8(cfg_of(c), flags, preset_value, nflags), "flag preset");
    if (rc != RZK_OK) return rc;
  }
  Operands ops{};
  for (size_t i = 0; i < specs.size(); ++i) {
    ops.base[i] = const_cast<int64_t*>(specs[i].base);
    ops.stride[i] = specs[i].stride;
    ops.outer[i] = specs[i].outer ? 1 : 0;
  }
  ops.group = group ? group : 1;
  ops.pad = dp.two_bit ? 1 : 0;
  ops.norm_limit = norm_limit;
  ops.bad = sticky ? c->d_bad : nullptr;
  ops.trusted = c->trusted ? 1u : 0u;
  ops.preset = preset_in_kernel ? preset_value : 0u;
  if (c->oimg_state.oimg) {   // operand images of the call in progress: this launch stores (producer op) and / or reads them
    ops.oimg = c->oimg_state.oimg;
    ops.oimg_l2 = c->oimg_state.oimg_l2;
    ops.oimg_np = c->oimg_state.oimg_np;
    ops.oimg_n = c->oimg_state.oimg_n;
    ops.oimg_group = c->oimg_state.oimg_group;
    ops.oimg_k = c->oimg_state.oimg_k;
    std::memcpy(ops.oimg_col, c->oimg_state.oimg_col, sizeof(ops.oimg_col));
    ops.oimg_op = c->oimg_producer_op;
  } else {
    ops.oimg_op = 0xffu;
  }
  if (dp.has_dkey) {
    if (!c->dkey_img || c->small) return fail(c, RZK_E_STATE, "multiplier images not prepared");
    ops.dkey_img = c->dkey_img;
    ops.dkey_l2 = c->dkey_l2;
    ops.dkey_n = c->dkey_n;
  }
  uint64_t bytes = 0;   // what the launch has to move at least: its operands in, its results out
  for (size_t i = 0; i < specs.size(); ++i)
    bytes += (uint64_t)dp.polys_in[i] * (specs[i].outer ? batch / (group ? group : 1) : batch);
  bytes = (bytes + (uint64_t)dp.polys_out * batch) * 8ull * c->N;
  LaunchCfg cfg;
  rc = prof_begin(c, bytes, cfg);
  if (rc != RZK_OK) return rc;
  int lrc = 0;
  switch (path) {
    case Path::Small:
      lrc = launch_row_program_small(c->N, cfg, dp.d, dp.nrows, ops, c->d_key_mont, c->dT, c->r2q, flags, batch);
      break;
    case Path::Shift:
      lrc = launch_shift_rows((int)c->logn, cfg, dp.d, dp.nrows, ops, c->dT, flags, batch);
      break;
    case Path::Blocks:
      if (!c->d_block_scratch)
        HIPCHK(c, hipMalloc((void**)&c->d_block_scratch, block_scratch_words((int)c->logn, c->num_cus) * sizeof(uint32_t)));
      lrc = launch_row_blocks((int)c->logn, cfg, dp.d, dp.d_blocks, dp.nblocks, ops, c->d_key_ntt, c->d_key_l2, c->dT,
                              c->d_tw, c->d_block_scratch, flags, batch);
      break;
    case Path::Groups:
      if (!c->d_group_scratch)
        HIPCHK(c, hipMalloc((void**)&c->d_group_scratch, group_scratch_words((int)c->logn, c->num_cus) * sizeof(uint32_t)));
      lrc = launch_row_groups((int)c->logn, cfg, dp.d, dp.ngroups, ops, c->d_key_ntt, c->d_key_l2, c->dT, c->d_tw,
                              c->d_group_scratch, flags, batch);
      break;
    case Path::Slots: {
      // shared-operand path; the workspace of stored transforms is bounded, so large batches go in chunks
      const size_t per_item = (size_t)dp.nslots * dp.np_store * c->N * sizeof(uint32_t) + (size_t)dp.nslots * 16;
      const size_t cap = (size_t)6 << 30;
      uint64_t chunk = cap / per_item;
      const uint64_t grp = ops.group;
      chunk -= chunk % grp;
      if (chunk < grp) chunk = grp;
      if (chunk > batch) chunk = batch;
      int rc2 = arena_reserve(c, c->ws_slots, (size_t)chunk * per_item + 256);
      if (rc2 != RZK_OK) return rc2;
      uint32_t* d_ws = (uint32_t*)c->ws_slots.p;
      double* d_norms = (double*)((char*)c->ws_slots.p + (((size_t)chunk * dp.nslots * dp.np_store * c->N * 4 + 255) & ~(size_t)255));
      for (uint64_t b0 = 0; b0 < batch && lrc == 0; b0 += chunk) {
        const uint64_t nb = batch - b0 < chunk ? batch - b0 : chunk;
        Operands o2 = ops;
        for (size_t i = 0; i < specs.size(); ++i) {
          if (!o2.base[i]) continue;
          const uint64_t first = o2.outer[i] ? b0 / grp : b0;
          o2.base[i] += first * o2.stride[i] * c->N;
        }
        lrc = launch_row_program_slots((int)c->logn, cfg, dp.d, dp.d_slots, dp.nslots, o2, c->d_key_ntt,
                                       c->d_key_l2, c->dT, c->d_tw, d_ws, d_norms, c->d_row_scratch,
                                       flags ? flags + b0 / grp : nullptr, nb, dp.np_store);
      }
      break;
    }
    case Path::Rows:
      lrc = launch_rows((int)c->logn, cfg, dp.d, dp.nrows, dp.has_shift, ops, c->d_key_ntt, c->d_key_l2, c->dT, c->d_tw,
                        c->d_row_scratch, flags, batch, dp.has_dd);
      break;
    case Path::Units:
      lrc = launch_units((int)c->logn, cfg, dp.d, dp.d_wp, dp.nunits, upt, 2 * dp.work, dp.has_vec, dp.has_shift, ops,
                         c->d_key_ntt, c->d_key_l2, c->dT, c->d_tw, c->d_row_scratch, flags, batch);
      break;
  }
  if (lrc == -2) return fail(c, RZK_E_UNSUPPORTED, "batch * rows must stay below 2^32");
  if (lrc != 0) {
    c->err = std::string("row kernel launch: ") + (lrc > 0 ? hipGetErrorString((hipError_t)lrc) : "bad ring degree");
    return RZK_E_HIP;
  }
  return prof_end(c);
}

int check_launch(rzk_ctx* c, int lrc, const char* what) {
  if (lrc == 0) return RZK_OK;
  c->err = std::string(what) + ": " + (lrc > 0 ? hipGetErrorString((hipError_t)lrc) : "bad ring degree");
  return RZK_E_HIP;
}

// (bound+1)^2 as hi:lo
void norm_limit(uint64_t bound, uint64_t& hi, uint64_t& lo) {
  unsigned __int128 v = (unsigned __int128)(bound + 1) * (bound + 1);
  hi = (uint64_t)(v >> 64);
  lo = (uint64_t)v;
}

// (bound+1)^2 when the fused predicate applies (NTT kernels only, limit <= 2^48), else 0
uint64_t fused_limit(const rzk_ctx* c, uint64_t bound) {
  if (c->small || bound >= (1ull << 24) - 1) return 0;
  return (bound + 1) * (bound + 1);
}

// Runs the checked variant (var | 1) of a program with the norm predicate fused into it: flags are
// preset to 1 and cleared by failing rows.  Returns RZK_E_UNSUPPORTED when fusion is not possible.
int run_program_checked(rzk_ctx* c, int id, uint32_t var, const std::vector<OpSpec>& specs, uint8_t* flags,
                        uint32_t group, uint64_t batch, uint64_t nflags, uint64_t bound, bool preset = true,
                        bool sticky = true) {
  const uint64_t lim = fused_limit(c, bound);
  if (!lim || !flags) return RZK_E_UNSUPPORTED;
  DevProg dp;
  int rc = get_program(c, id, var | 1, dp);
  if (rc != RZK_OK) return rc;
  // two-bit verdicts are cleared with word atomics: the flag array must be made of whole aligned words
  if (dp.two_bit && ((reinterpret_cast<uintptr_t>(flags) & 3u) || (nflags & 3u))) return RZK_E_UNSUPPORTED;
  const uint8_t all_ok = dp.two_bit ? 3 : 1;
  return run_program(c, id, var | 1, specs, flags, group, batch, lim, sticky, preset ? all_ok : (uint8_t)0, nflags);
}

// The scalar multipliers of a Linear / Sum call (g: one per proof; g_i: V per proof) transformed once into the form of the
// resident key, for the TERM_DKEY terms of the call's row programs (variant bit kDkeyVar).  flags / sticky as in
// run_program: a non-canonical coefficient clears the proof's verdict and / or raises the sticky word.  Leaves
// c->dkey_img NULL when the path is off (RZK_DKEY=0, small rings): the callers then ask for the plain variants.
// uses: rows of this call that multiply by each multiplier.  The forward launch costs three transforms per multiplier and
// a launch of its own; measured: Linear at l = 1 (2 uses) gains nothing, the Sum shapes (9 and 17 uses) 14-15 %.
constexpr uint32_t kDkeyMinUses = 4;
bool dkey_wanted(const rzk_ctx* c, uint32_t uses) {
  return !(c->use_dkey <= 0 || (c->use_dkey == 1 && uses < kDkeyMinUses) || c->small);
}
int prepare_dkey(rzk_ctx* c, const int64_t* g, uint64_t entries, uint32_t per_entry, uint32_t uses, uint8_t* flags, bool sticky) {
  c->dkey_img = nullptr;
  c->dkey_l2 = nullptr;
  c->dkey_n = 0;
  if (!dkey_wanted(c, uses) || entries == 0) return RZK_OK;
  const uint64_t count = entries * per_entry;
  const size_t img_bytes = ((size_t)count * kKeyImages * c->N * sizeof(uint32_t) + 255) & ~(size_t)255;
  int rc = arena_reserve(c, c->ws_dkey, img_bytes + (size_t)count * sizeof(double));
  if (rc != RZK_OK) return rc;
  uint32_t* img = (uint32_t*)c->ws_dkey.p;
  double* l2 = (double*)((char*)c->ws_dkey.p + img_bytes);
  LaunchCfg cfg;
  rc = prof_begin(c, count * 8ull * c->N, cfg);   // the multipliers it reads; the images are derived data
  if (rc != RZK_OK) return rc;
  rc = check_launch(c, launch_dkey_transform((int)c->logn, cfg, g, count, per_entry, img, l2, c->dT, c->d_tw, flags,
                                             sticky ? c->d_bad : nullptr, false, c->trusted), "multiplier images");
  if (rc != RZK_OK) return rc;
  rc = prof_end(c);
  if (rc != RZK_OK) return rc;
  c->dkey_img = img;
  c->dkey_l2 = l2;
  c->dkey_n = per_entry;
  return RZK_OK;
}
// variant bit for programs that multiply by the call's scalar multipliers
uint32_t dkv(const rzk_ctx* c) { return c->dkey_img ? kDkeyVar : 0u; }

// Operand images of a Sum call (Operands::oimg): room for the transforms of the columns a2 uses of every (proof, summand)
// vector, all marked "nothing stored yet".  Leaves c->oimg_state.oimg NULL when the path is off or nothing would be saved.
bool sum_uses_d(const rzk_ctx* c, uint32_t V);   // (below, with the Sum entry points)
int prepare_oimg(rzk_ctx* c, uint64_t B, uint32_t V, uint32_t uses) {
  c->oimg_state = Operands{};
  c->oimg_producer_op = 0xffu;
  if (!c->use_oimg || !dkey_wanted(c, uses) || c->k > 32u || !sum_uses_d(c, V)) return RZK_OK;
  const uint32_t k = c->k;
  const PlanEnv env = plan_env(c);
  uint32_t ncols = 0;
  for (uint32_t col = 0; col < 32u; ++col) c->oimg_state.oimg_col[col] = -1;
  for (uint32_t col = 0; col < k; ++col)
    if (a2_uses_column(env, col)) c->oimg_state.oimg_col[col] = (int8_t)ncols++;
  if (ncols == 0) return RZK_OK;
  const uint64_t slots = B * V * ncols;
  const size_t img_bytes = ((size_t)slots * kKeyImages * c->N * sizeof(uint32_t) + 255) & ~(size_t)255;
  const size_t l2_bytes = ((size_t)slots * sizeof(double) + 255) & ~(size_t)255;
  int rc = arena_reserve(c, c->ws_oimg, img_bytes + l2_bytes + slots);
  if (rc != RZK_OK) return rc;
  char* base = (char*)c->ws_oimg.p;
  HIPCHK(c, hipMemsetAsync(base + img_bytes + l2_bytes, 0, slots, c->stream));
  c->oimg_state.oimg = (uint32_t*)base;
  c->oimg_state.oimg_l2 = (double*)(base + img_bytes);
  c->oimg_state.oimg_np = (uint8_t*)(base + img_bytes + l2_bytes);
  c->oimg_state.oimg_n = ncols;
  c->oimg_state.oimg_group = V;
  c->oimg_state.oimg_k = k;
  return RZK_OK;
}
uint32_t oiv(const rzk_ctx* c) { return (c->oimg_state.oimg && c->dkey_img) ? kOimgVar : 0u; }

bool can_fuse(rzk_ctx* c, int id, uint32_t var, uint64_t bound) {
  DevProg dp;
  return fused_limit(c, bound) != 0 && get_program(c, id, var | 1, dp) == RZK_OK;
}

int run_norm(rzk_ctx* c, const int64_t* v, uint32_t rows, uint64_t bound, uint8_t* ok, uint64_t B, int mode,
             int shift, bool sticky = true) {
  // canonical coefficients are below 2^31 in magnitude, so sum c^2 < 2^73: every bound from 2^37 on holds for
  // all inputs; clamping there keeps (bound+1)^2 inside 128 bits for any u64 bound (sigma grows with b)
  if (bound > (1ull << 40)) bound = 1ull << 40;
  uint64_t hi, lo;
  norm_limit(bound, hi, lo);
  uint32_t* bad = sticky ? c->d_bad : nullptr;
  const uint32_t qh = c->hT.crt.qhalf;
  if (c->small)
    return check_launch(c, launch_norm_small(c->N, cfg_of(c), v, rows, hi, lo, ok, B, mode, shift, qh, bad), "norm kernel");
  return check_launch(c, launch_norm((int)c->logn, cfg_of(c), v, rows, hi, lo, ok, B, mode, shift, qh, bad), "norm kernel");
}

// ---- host-pointer plumbing ---------------------------------------------------------------------------------
struct HostBuf {
  const void* in;   // host source (nullptr for pure outputs)
  void* out;        // host destination (nullptr for pure inputs)
  size_t bytes;
  void* dev;        // filled by stage_in
};

int stage_in(rzk_ctx* c, std::vector<HostBuf>& bufs) {
  size_t total = 0;
  for (auto& b : bufs) total += (b.bytes + 255) & ~size_t(255);
  int rc = arena_reserve(c, c->stage, total);
  if (rc != RZK_OK) return rc;
  size_t off = 0;
  for (auto& b : bufs) {
    b.dev = (char*)c->stage.p + off;
    off += (b.bytes + 255) & ~size_t(255);
    if (b.in && b.bytes) HIPCHK(c, hipMemcpyAsync(b.dev, b.in, b.bytes, hipMemcpyHostToDevice, c->stream));
  }
  return RZK_OK;
}

// Synchronises and reports (then clears) the sticky input-error word.
int take_input_error(rzk_ctx* c) {
  HIPCHK(c, hipMemcpyAsync(c->h_bad, c->d_bad, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (*c->h_bad == 0) return RZK_OK;
  *c->h_bad = 0;
  HIPCHK(c, hipMemsetAsync(c->d_bad, 0, sizeof(uint32_t), c->stream));
  return fail(c, RZK_E_ARG,
              "an input coefficient is not the centred representative in [-(q-1)/2, (q-1)/2] (ZqI64 range); "
              "reduce foreign data with rzk_canonicalize_batch first");
}

int stage_out(rzk_ctx* c, std::vector<HostBuf>& bufs) {
  for (auto& b : bufs)
    if (b.out && b.bytes) HIPCHK(c, hipMemcpyAsync(b.out, b.dev, b.bytes, hipMemcpyDeviceToHost, c->stream));
  return take_input_error(c);
}

size_t polys(const rzk_ctx* c, size_t count) { return count * (size_t)c->N * sizeof(int64_t); }

}  // namespace

// =================================================================================================
// context
// =================================================================================================
extern "C" {

int rzk_ctx_create(rzk_ctx** out, int64_t q, uint32_t N, uint32_t n, uint32_t k, uint32_t l, uint32_t kappa,
                   uint64_t b, int device) {
  if (!out) return RZK_E_ARG;
  *out = nullptr;
  const bool pow2 = N >= 4 && (N & (N - 1)) == 0;
  if (!pow2 || N > 2048) return create_fail(RZK_E_UNSUPPORTED, "ring degree must be a power of two in [4, 2048]");
  if (n < 1 || l < 1 || k <= n || n + l > k)   // params.rs:26-31: k > n >= l ; a2' has k-n-l cols
    return create_fail(RZK_E_ARG, "need k > n >= 1, l >= 1, n + l <= k");
  if (q < 3) return create_fail(RZK_E_ARG, "bad modulus");
  int ndev = 0;
  hipError_t de = hipGetDeviceCount(&ndev);
  if (de != hipSuccess) return create_fail(RZK_E_HIP, std::string("hipGetDeviceCount: ") + hipGetErrorString(de));
  if (ndev <= 0 || device < 0 || device >= ndev) return create_fail(RZK_E_HIP, "no such HIP device");
  rzk_ctx* c = new rzk_ctx();
  c->device = device;
  c->q = q;
  c->N = N;
  c->logn = 0;
  while ((1u << c->logn) < N) ++c->logn;
  c->small = N < 512;
  c->r2q = (uint32_t)((((unsigned __int128)1) << 64) % (unsigned __int128)q);
  c->n = n;
  c->k = k;
  c->l = l;
  c->kappa = kappa;
  c->b = b;
  // params.rs:94-98, 104, 114 (usize floor square roots)
  c->sigma = b * (11ull * kappa) * isqrt_u64((uint64_t)k * N);
  c->commit_bound = 4 * c->sigma * isqrt_u64(N);
  c->verify_bound = 2 * c->sigma * isqrt_u64(N);
  if (!host::make_crt_consts((uint64_t)q, c->hT.crt)) {
    delete c;
    return create_fail(RZK_E_UNSUPPORTED, "modulus must be odd and below 4 * the smallest auxiliary prime");
  }
  if ((de = hipSetDevice(device)) != hipSuccess) {
    delete c;
    return create_fail(RZK_E_HIP, std::string("hipSetDevice: ") + hipGetErrorString(de));
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
    c->num_cus = prop.multiProcessorCount;
  // RZK_GRID_CUS (testing): every grid cap and the scratch sized from it follow this CU count, so that small batches
  // make several grid-stride trips; set before the first allocation sized by num_cus (the row scratch below)
  if (const char* e = std::getenv("RZK_GRID_CUS")) {
    const long v = std::strtol(e, nullptr, 10);
    c->num_cus = v < 1 ? 1 : (v < c->num_cus ? (int)v : c->num_cus);
  }
  if ((de = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking)) != hipSuccess) {
    delete c;
    return create_fail(RZK_E_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(de));
  }
  c->stream = c->own_stream;
  if (const char* e = std::getenv("RZK_SLOT_SHARE_MIN")) c->slot_share_min = std::atof(e);   // tuning knobs
  if (const char* e = std::getenv("RZK_ROW_GROUPS")) c->use_groups = std::atoi(e) != 0;
  c->group_max = group_max_for((int)c->logn);
  if (const char* e = std::getenv("RZK_GROUP_MAX")) {
    const int g = std::atoi(e);
    if (g >= 1 && g <= group_accumulators(c->logn)) c->group_max = g;   // bounded by the compiled accumulators
  }
  if (const char* e = std::getenv("RZK_SHIFT")) c->use_shift = std::atoi(e) != 0;
  if (const char* e = std::getenv("RZK_SHIFT_BYTES")) c->shift_bytes = std::atoi(e) != 0;
  if (const char* e = std::getenv("RZK_SUM_D")) c->sum_d = std::atoi(e) != 0 ? 1 : 0;
  if (const char* e = std::getenv("RZK_DKEY")) c->use_dkey = std::atoi(e);
  if (const char* e = std::getenv("RZK_LIN_E")) c->lin_e = std::atoi(e) != 0;
  if (const char* e = std::getenv("RZK_OIMG")) c->use_oimg = std::atoi(e) != 0;
  if (const char* e = std::getenv("RZK_PRESET_IN_KERNEL")) c->preset_in_kernel = std::atoi(e) != 0;
  if (const char* e = std::getenv("RZK_PAIRS")) c->use_pairs = std::atoi(e) != 0;
  if (const char* e = std::getenv("RZK_UPT")) c->units_per_task = (uint32_t)std::atoi(e);
  if (const char* e = std::getenv("RZK_VEC_ROWS")) c->vec_rows = std::atoi(e) != 0;
  if (const char* e = std::getenv("RZK_PAIR_POLY")) c->pair_poly = std::atoi(e) != 0;
  c->unit_io = c->logn == 9;
  if (const char* e = std::getenv("RZK_UNIT_IO")) c->unit_io = std::atoi(e) != 0;
  if (const char* e = std::getenv("RZK_BLOCK_MIN_LOGN")) c->block_min_logn = (uint32_t)std::atoi(e);   // 12 = never

  // twiddle tables: 3 primes x {fwd, inv} x kTableLen
  std::vector<uint32_t> all((size_t)2 * kMaxPrimes * kTableLen);
  for (int i = 0; i < kMaxPrimes; ++i) {
    std::vector<uint32_t> f, v;
    host::make_twiddles(i, f, v);
    std::memcpy(&all[(size_t)(2 * i) * kTableLen], f.data(), sizeof(uint32_t) * kTableLen);
    std::memcpy(&all[(size_t)(2 * i + 1) * kTableLen], v.data(), sizeof(uint32_t) * kTableLen);
    c->hT.pc[i] = host::make_prime_consts(i, N);
  }
  bool okk = hipMalloc((void**)&c->d_tw, all.size() * sizeof(uint32_t)) == hipSuccess &&
             hipMemcpy(c->d_tw, all.data(), all.size() * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess;
  c->hT.cap[0] = 0.0;
  for (int np = 1; np <= kMaxPrimes; ++np) c->hT.cap[np] = host::crt_capacity(np);
  okk = okk && (c->small || hipMalloc((void**)&c->d_row_scratch,
                                      row_scratch_words((int)c->logn, c->num_cus) * sizeof(uint32_t)) == hipSuccess);
  okk = okk && hipMalloc((void**)&c->dT, sizeof(DevTables)) == hipSuccess &&
        hipMemcpy(c->dT, &c->hT, sizeof(DevTables), hipMemcpyHostToDevice) == hipSuccess;
  okk = okk && hipMalloc((void**)&c->d_bad, sizeof(uint32_t)) == hipSuccess &&
        hipMemset(c->d_bad, 0, sizeof(uint32_t)) == hipSuccess &&
        hipHostMalloc((void**)&c->h_bad, sizeof(uint32_t), hipHostMallocDefault) == hipSuccess;
  if (okk) *c->h_bad = 0;
  if (!okk) {
    rzk_ctx_destroy(c);
    return create_fail(RZK_E_HIP, std::string("table upload: ") + hipGetErrorString(hipGetLastError()));
  }
  *out = c;
  return RZK_OK;
}

void rzk_ctx_destroy(rzk_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  drop_programs(c);
  for (auto& ev : c->prof_events) {
    (void)hipEventDestroy(ev.first);
    (void)hipEventDestroy(ev.second);
  }
  if (c->d_key_ntt) (void)hipFree(c->d_key_ntt);
  if (c->d_key_l2) (void)hipFree(c->d_key_l2);
  if (c->ws.p) (void)hipFree(c->ws.p);
  if (c->ws_slots.p) (void)hipFree(c->ws_slots.p);
  if (c->ws_wire.p) (void)hipFree(c->ws_wire.p);
  if (c->ws_fs.p) (void)hipFree(c->ws_fs.p);
  if (c->ws_reject.p) (void)hipFree(c->ws_reject.p);
  if (c->ws_dkey.p) (void)hipFree(c->ws_dkey.p);
  if (c->ws_oimg.p) (void)hipFree(c->ws_oimg.p);
  if (c->stage.p) (void)hipFree(c->stage.p);
  if (c->dT) (void)hipFree(c->dT);
  if (c->d_tw) (void)hipFree(c->d_tw);
  if (c->d_row_scratch) (void)hipFree(c->d_row_scratch);
  if (c->d_block_scratch) (void)hipFree(c->d_block_scratch);
  if (c->d_group_scratch) (void)hipFree(c->d_group_scratch);
  if (c->d_key_mont) (void)hipFree(c->d_key_mont);
  if (c->d_bad) (void)hipFree(c->d_bad);
  if (c->h_bad) (void)hipHostFree(c->h_bad);
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  wipe(c->sampler_key, sizeof(c->sampler_key));
  delete c;
}

uint32_t rzk_abi_version(void) { return RZK_ABI_VERSION; }

int rzk_ctx_trust_device_outputs(rzk_ctx* c, int on) {
  if (!c) return RZK_E_ARG;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->trusted = on != 0;
  return RZK_OK;
}

int rzk_ctx_set_stream(rzk_ctx* c, void* hip_stream) {
  if (!c) return RZK_E_ARG;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->stream = (hipStream_t)hip_stream;   // NULL = HIP's default stream
  return RZK_OK;
}

int rzk_ctx_use_own_stream(rzk_ctx* c) {
  if (!c) return RZK_E_ARG;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->stream = c->own_stream;
  return RZK_OK;
}

int rzk_ctx_synchronize(rzk_ctx* c) {
  if (!c) return RZK_E_ARG;
  (void)hipSetDevice(c->device);
  return take_input_error(c);   // also the place where the asynchronous *_dev calls report non-canonical inputs
}

int rzk_ctx_check_inputs(rzk_ctx* c) { return rzk_ctx_synchronize(c); }

const char* rzk_last_error(const rzk_ctx* c) { return c ? c->err.c_str() : g_create_err.c_str(); }
uint64_t rzk_sigma(const rzk_ctx* c) { return c ? c->sigma : 0; }
uint64_t rzk_commit_bound(const rzk_ctx* c) { return c ? c->commit_bound : 0; }
uint64_t rzk_verify_bound(const rzk_ctx* c) { return c ? c->verify_bound : 0; }

// =================================================================================================
// key
// =================================================================================================
static int fs_key_digest_dev(rzk_ctx* c, const int64_t* a_host, const int64_t* a_dev);

// a_dev: the same key on the device when the caller has it there (rzk_key_load_dev), else NULL
static int key_load_impl(rzk_ctx* c, const int64_t* a_host, const int64_t* a_dev = nullptr) {
  const uint32_t N = c->N, rows = c->n + c->l, k = c->k;
  const size_t total = (size_t)rows * k;
  const int64_t half = (c->q - 1) / 2;
  c->key_class.assign(total, KC_GENERAL);
  c->key_entry.assign(total, -1);
  std::vector<int64_t> general;
  std::vector<double> kinf;
  c->n_general = 0;
  for (size_t e = 0; e < total; ++e) {
    const int64_t* p = a_host + e * N;
    bool tail_zero = true;
    long double ssq = 0.0L;
    for (uint32_t j = 0; j < N; ++j) {
      const int64_t v = p[j];
      if (v > half || v < -half) return fail(c, RZK_E_ARG, "key coefficient outside the centred range");
      if (j > 0 && v != 0) tail_zero = false;
      ssq += (long double)v * (long double)v;
    }
    if (tail_zero && p[0] == 0)
      c->key_class[e] = KC_ZERO;
    else if (tail_zero && p[0] == 1)
      c->key_class[e] = KC_ONE;
    else {
      c->key_entry[e] = (int32_t)c->n_general++;
      general.insert(general.end(), p, p + N);
      kinf.push_back((double)(std::sqrt(ssq) * (1.0L + 1e-6L)));   // upper bound of the entry's 2-norm (prime-count bound), still one after rounding to float
    }
  }
  drop_programs(c);   // programs depend on the classification
  if (c->d_key_ntt) HIPCHK(c, hipFree(c->d_key_ntt));
  if (c->d_key_l2) HIPCHK(c, hipFree(c->d_key_l2));
  if (c->d_key_mont) HIPCHK(c, hipFree(c->d_key_mont));
  c->d_key_ntt = nullptr;
  c->d_key_l2 = nullptr;
  c->d_key_mont = nullptr;
  if (c->n_general && c->small) {
    const size_t gbytes = general.size() * sizeof(int64_t);
    int rc = arena_reserve(c, c->stage, gbytes);
    if (rc != RZK_OK) return rc;
    HIPCHK(c, hipMalloc((void**)&c->d_key_mont, general.size() * sizeof(uint32_t)));
    HIPCHK(c, hipMemcpyAsync(c->stage.p, general.data(), gbytes, hipMemcpyHostToDevice, c->stream));
    rc = check_launch(c, launch_key_mont(cfg_of(c), (const int64_t*)c->stage.p, c->d_key_mont, general.size(), c->dT,
                                         c->r2q),
                      "key conversion");
    if (rc != RZK_OK) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
  } else if (c->n_general) {
    const size_t gbytes = general.size() * sizeof(int64_t);
    int rc = arena_reserve(c, c->stage, gbytes);
    if (rc != RZK_OK) return rc;
    HIPCHK(c, hipMalloc((void**)&c->d_key_ntt, (size_t)c->n_general * kKeyImages * N * sizeof(uint32_t)));
    HIPCHK(c, hipMalloc((void**)&c->d_key_l2, (size_t)c->n_general * sizeof(double)));
    HIPCHK(c, hipMemcpyAsync(c->stage.p, general.data(), gbytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_key_l2, kinf.data(), kinf.size() * sizeof(double), hipMemcpyHostToDevice,
                             c->stream));
    rc = check_launch(c, launch_key_transform((int)c->logn, cfg_of(c), (const int64_t*)c->stage.p, c->n_general,
                                              c->d_key_ntt, c->dT, c->d_tw),
                      "key transform");
    if (rc != RZK_OK) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));   // `general` / `kinf` are host temporaries
  }
  c->key_loaded = false;   // until the digest of the new key is in place
  int frc = fs_key_digest_dev(c, a_host, a_dev);
  if (frc != RZK_OK) return frc;
  c->key_loaded = true;
  return RZK_OK;
}

// FS1 key digest (rzk_keccak.h): leaf digests of the (n+l)*k key polynomials, then one root lane over the parameter
// header and those digests.  Runs once per key load, on the coefficients the load has at hand.
static int fs_key_digest_dev(rzk_ctx* c, const int64_t* a_host, const int64_t* a_dev) {
  const uint32_t kpolys = (c->n + c->l) * c->k;
  const uint32_t leaves = kpolys * (c->N / fs_leaf_len(c->N));
  const size_t dig_b = ((size_t)leaves * kFsDigestWords * sizeof(uint64_t) + 255) & ~size_t(255);
  const size_t key_b = a_dev ? 0 : (size_t)kpolys * c->N * sizeof(int64_t);
  int rc = arena_reserve(c, c->ws_fs, dig_b + 256 + key_b);
  if (rc != RZK_OK) return rc;
  uint64_t* dig = (uint64_t*)c->ws_fs.p;
  uint8_t* out = (uint8_t*)c->ws_fs.p + dig_b;
  if (!a_dev) {
    int64_t* stage = (int64_t*)((char*)c->ws_fs.p + dig_b + 256);
    HIPCHK(c, hipMemcpyAsync(stage, a_host, key_b, hipMemcpyHostToDevice, c->stream));
    a_dev = stage;
  }
  FsMsg m{};
  m.nfields = 1;
  m.N = c->N;
  m.polys = kpolys;
  m.first[1] = kpolys;
  m.ptr[0] = a_dev;
  const LaunchCfg cfg = cfg_of(c);
  // (the host loop of the load has range-tested every coefficient)
  rc = check_launch(c, launch_fs_leaves(cfg, m, (c->q - 1) / 2, 0, dig, nullptr, nullptr, 1), "key leaf hash");
  if (rc != RZK_OK) return rc;
  FsRoot r{};
  fs_key_header(c->q, c->N, c->n, c->k, c->l, c->kappa, c->b, r.hdr);
  r.nhdr = kFsKeyHeaderWords;
  r.leaves = leaves;
  r.N = c->N;
  r.kappa = c->kappa;
  rc = check_launch(c, launch_fs_roots(cfg, r, dig, nullptr, out, 1), "key root hash");
  if (rc != RZK_OK) return rc;
  HIPCHK(c, hipMemcpyAsync(c->key_digest, out, sizeof c->key_digest, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return RZK_OK;
}

int rzk_key_load(rzk_ctx* c, const int64_t* a_host) {
  if (!c || !a_host) return RZK_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  return key_load_impl(c, a_host);
}

// CommitmentKey::new (commit.rs:33-60) with the device-side sampler: a1 = [I_n | U], a2 = [0_{l x n} | I_l | U],
// U uniform over the centred range (params.rs:126).  The full key goes back to the caller (the reference's
// CommitmentKey is public data) and is loaded like any other key.
int rzk_key_generate(rzk_ctx* c, uint64_t seed, int64_t* a_host_out) {
  if (!c) return RZK_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  const uint32_t N = c->N, n = c->n, k = c->k, l = c->l;
  const size_t n_rand = (size_t)n * (k - n) + (size_t)l * (k - n - l);
  std::vector<int64_t> rnd(n_rand * N);
  if (n_rand) {
    int rc = arena_reserve(c, c->stage, n_rand * N * sizeof(int64_t));
    if (rc != RZK_OK) return rc;
    rc = check_launch(c, launch_sample_uniform(cfg_of(c), (int64_t*)c->stage.p, n_rand, N, seed, 0x6b6579u /* "key" */,
                                               (uint32_t)((c->q - 1) / 2)),
                      "key sampler");
    if (rc != RZK_OK) return rc;
    HIPCHK(c, hipMemcpyAsync(rnd.data(), c->stage.p, rnd.size() * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  std::vector<int64_t> a((size_t)(n + l) * k * N, 0);
  size_t next = 0;
  auto put_random = [&](size_t row, size_t col) {
    std::memcpy(a.data() + (row * k + col) * N, rnd.data() + next * N, (size_t)N * sizeof(int64_t));
    ++next;
  };
  for (uint32_t i = 0; i < n; ++i) {          // a1 = [I_n | a1']   (commit.rs:38-46)
    a[((size_t)i * k + i) * N] = 1;
    for (uint32_t j = n; j < k; ++j) put_random(i, j);
  }
  for (uint32_t i = 0; i < l; ++i) {          // a2 = [0 | I_l | a2']  (commit.rs:48-57)
    a[((size_t)(n + i) * k + n + i) * N] = 1;
    for (uint32_t j = n + l; j < k; ++j) put_random(n + i, j);
  }
  if (a_host_out) std::memcpy(a_host_out, a.data(), a.size() * sizeof(int64_t));
  return key_load_impl(c, a.data());
}

int rzk_key_load_dev(rzk_ctx* c, const int64_t* a_dev) {
  if (!c || !a_dev) return RZK_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t total = (size_t)(c->n + c->l) * c->k * c->N;
  std::vector<int64_t> h(total);
  HIPCHK(c, hipMemcpyAsync(h.data(), a_dev, total * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return key_load_impl(c, h.data(), a_dev);
}

// =================================================================================================
// ring / Mat primitives
// =================================================================================================
int rzk_polymul_batch_dev(rzk_ctx* c, const int64_t* a, const int64_t* b, int64_t* out, size_t count) {
  if (c && count == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !a || !b || !out) return RZK_E_ARG;
  return run_program(c, PG_POLYMUL, 0, {{a, 1, 0}, {b, 1, 0}, {out, 1, 0}}, nullptr, 1, count);
}

int rzk_matvec_batch_dev(rzk_ctx* c, int which, const int64_t* v, const int64_t* addend, int64_t* out, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !v || !out || which < 0 || which > 2) return RZK_E_ARG;
  const uint32_t rows = which == RZK_KEY_A1 ? c->n : (which == RZK_KEY_A2 ? c->l : c->n + c->l);
  return run_program(c, PG_MATVEC, (uint32_t)which * 2 + (addend ? 1 : 0),
                     {{v, c->k, 0}, {addend, rows, 0}, {out, rows, 0}}, nullptr, 1, B);
}

int rzk_cmul_batch_dev(rzk_ctx* c, const int64_t* m, uint32_t rows, const int64_t* p, int64_t* out, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !m || !p || !out || rows == 0) return RZK_E_ARG;
  if (rows > (uint32_t)kMaxRows) {
    // more rows than one program holds: treat every row as its own batch entry sharing p
    return run_program(c, PG_CMUL, 1, {{m, 1, 0}, {p, 1, 1}, {out, 1, 0}}, nullptr, rows, B * rows);
  }
  return run_program(c, PG_CMUL, rows, {{m, rows, 0}, {p, 1, 0}, {out, rows, 0}}, nullptr, 1, B);
}

int rzk_canonicalize_batch_dev(rzk_ctx* c, const int64_t* in, int64_t* out, size_t count) {
  if (c && count == 0) return RZK_OK;
  if (!c || !in || !out) return RZK_E_ARG;
  return check_launch(c, launch_canonicalize(cfg_of(c), in, out, (uint64_t)count * c->N, c->q), "canonicalize kernel");
}

int rzk_add_batch_dev(rzk_ctx* c, const int64_t* a, const int64_t* b, int64_t* out, size_t count) {
  if (c && count == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !a || !b || !out) return RZK_E_ARG;
  return check_launch(c, launch_addsub(cfg_of(c), false, a, b, out, (uint64_t)count * c->N, c->dT, c->d_bad), "add kernel");
}

int rzk_sub_batch_dev(rzk_ctx* c, const int64_t* a, const int64_t* b, int64_t* out, size_t count) {
  if (c && count == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !a || !b || !out) return RZK_E_ARG;
  return check_launch(c, launch_addsub(cfg_of(c), true, a, b, out, (uint64_t)count * c->N, c->dT, c->d_bad), "sub kernel");
}

int rzk_norm2_le_batch_dev(rzk_ctx* c, const int64_t* v, uint32_t rows, uint64_t bound, uint8_t* ok, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !v || !ok || rows == 0) return RZK_E_ARG;
  return run_norm(c, v, rows, bound, ok, B, 0, 0);
}

int rzk_eq_batch_dev(rzk_ctx* c, const int64_t* a, const int64_t* b, uint32_t rows, uint8_t* eq, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !a || !b || !eq || rows == 0) return RZK_E_ARG;
  const uint32_t qh = c->hT.crt.qhalf;
  if (c->small) return check_launch(c, launch_eq_small(c->N, cfg_of(c), a, b, rows, eq, B, qh, c->d_bad), "eq kernel");
  return check_launch(c, launch_eq((int)c->logn, cfg_of(c), a, b, rows, eq, B, qh, c->d_bad), "eq kernel");
}

int rzk_ntt_forward_batch_dev(rzk_ctx* c, int prime, const uint32_t* in, uint32_t* out, size_t count) {
  if (c && count == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !in || !out || prime < 0 || prime >= kMaxPrimes) return RZK_E_ARG;
  if (c->small) return fail(c, RZK_E_UNSUPPORTED, "batched transforms need N >= 512");
  return check_launch(c, launch_ntt((int)c->logn, false, cfg_of(c), prime, in, out, count, c->dT, c->d_tw), "ntt forward");
}

int rzk_ntt_inverse_batch_dev(rzk_ctx* c, int prime, const uint32_t* in, uint32_t* out, size_t count) {
  if (c && count == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !in || !out || prime < 0 || prime >= kMaxPrimes) return RZK_E_ARG;
  if (c->small) return fail(c, RZK_E_UNSUPPORTED, "batched transforms need N >= 512");
  return check_launch(c, launch_ntt((int)c->logn, true, cfg_of(c), prime, in, out, count, c->dT, c->d_tw), "ntt inverse");
}

uint32_t rzk_ntt_prime(int prime) { return prime >= 0 && prime < kMaxPrimes ? kPrimes[prime] : 0; }
uint32_t rzk_ntt_psi(int prime, uint32_t N) {
  if (prime < 0 || prime >= kMaxPrimes || N == 0 || (N & (N - 1)) || N > (uint32_t)kTableLen) return 0;
  return host::psi_for(prime, N);
}
uint32_t rzk_ntt_layout_index(uint32_t N, uint32_t j) {
  if (j >= N || N < 512) return 0xffffffffu;
  const uint32_t E = N / 64;
  const uint32_t lane = j / E, c = j % E;
  return (c >> 2) * 256 + lane * 4 + (c & 3);
}

// =================================================================================================
// Device-side samplers
// =================================================================================================
int rzk_sample_uniform_dev(rzk_ctx* c, uint64_t seed, uint32_t stream, uint64_t bound, int64_t* out, size_t count) {
  if (c && count == 0) return RZK_OK;
  if (!c || !out || bound == 0 || bound > (uint64_t)(c->q - 1) / 2) return RZK_E_ARG;
  return check_launch(c, launch_sample_uniform(cfg_of(c), out, count, c->N, seed, stream, (uint32_t)bound), "sampler");
}
int rzk_sample_gauss_dev(rzk_ctx* c, uint64_t seed, uint32_t stream, double sigma, int64_t* out, size_t count) {
  if (c && count == 0) return RZK_OK;
  // |x| stays far below (q-1)/2 for every sigma the parameters produce; 2^26 keeps 12 sigma inside the range
  if (!c || !out || !(sigma > 0.0) || sigma > 67108864.0) return RZK_E_ARG;
  LaunchCfg cfg;   // a profiling slot when profiling is on: rzk_prof_read_kernels names the form that ran
  int rc = prof_begin(c, (uint64_t)count * c->N * sizeof(int64_t), cfg);
  if (rc != RZK_OK) return rc;
  rc = check_launch(c, launch_sample_gauss(cfg, out, count, c->N, seed, stream, sigma), "sampler");
  return rc != RZK_OK ? rc : prof_end(c);
}
int rzk_sample_challenge_dev(rzk_ctx* c, uint64_t seed, uint32_t stream, int64_t* out, size_t count) {
  if (c && count == 0) return RZK_OK;
  if (!c || !out) return RZK_E_ARG;
  return check_launch(c, launch_sample_challenge(cfg_of(c), out, count, c->N, seed, stream, c->kappa), "sampler");
}

// ---- keyed samplers (v6): the same distributions from ChaCha20 blocks (rzk_chacha.h) ------------------
int rzk_sampler_set_key(rzk_ctx* c, const uint8_t key[32]) {
  if (!c) return RZK_E_ARG;
  wipe(c->sampler_key, sizeof(c->sampler_key));
  c->sampler_key_set = key != nullptr;
  if (key) std::memcpy(c->sampler_key, key, sizeof(c->sampler_key));
  return RZK_OK;
}

namespace {
// subkey of one call = HChaCha20(key, nonce), and the launch configuration (a profiling slot when profiling is on)
int keyed_begin(rzk_ctx* c, const uint8_t* nonce, size_t count, uint32_t subkey[8], LaunchCfg& cfg) {
  if (!c->sampler_key_set) return fail(c, RZK_E_ARG, "keyed sampler: no key set (rzk_sampler_set_key)");
  if (!nonce) return fail(c, RZK_E_ARG, "keyed sampler: NULL nonce");
  const int rc = prof_begin(c, (uint64_t)count * c->N * sizeof(int64_t), cfg);
  if (rc == RZK_OK) chacha_sampler_subkey(c->sampler_key, nonce, subkey);
  return rc;
}
// the launch has copied the subkey into its kernel arguments: wipe the host copy
int keyed_end(rzk_ctx* c, int launch_rc, uint32_t subkey[8]) {
  wipe(subkey, 8 * sizeof(uint32_t));
  const int rc = check_launch(c, launch_rc, "keyed sampler");
  return rc != RZK_OK ? rc : prof_end(c);
}
}  // namespace

int rzk_sample_uniform_keyed_dev(rzk_ctx* c, const uint8_t nonce[16], uint32_t stream, uint64_t bound, int64_t* out,
                                 size_t count) {
  if (c && count == 0) return RZK_OK;
  if (!c || !out || bound == 0 || bound > (uint64_t)(c->q - 1) / 2) return RZK_E_ARG;
  uint32_t sk[8];
  LaunchCfg cfg;
  const int rc = keyed_begin(c, nonce, count, sk, cfg);
  if (rc != RZK_OK) return rc;
  return keyed_end(c, launch_sample_uniform_chacha(cfg, out, count, c->N, sk, stream, (uint32_t)bound), sk);
}
int rzk_sample_gauss_keyed_dev(rzk_ctx* c, const uint8_t nonce[16], uint32_t stream, double sigma, int64_t* out,
                               size_t count) {
  if (c && count == 0) return RZK_OK;
  if (!c || !out || !(sigma > 0.0) || sigma > 67108864.0) return RZK_E_ARG;   // as rzk_sample_gauss_dev
  uint32_t sk[8];
  LaunchCfg cfg;
  const int rc = keyed_begin(c, nonce, count, sk, cfg);
  if (rc != RZK_OK) return rc;
  return keyed_end(c, launch_sample_gauss_chacha(cfg, out, count, c->N, sk, stream, sigma), sk);
}
// v11: the exact discrete Gaussian D_sigma (rzk_dgauss.h); count is in coefficients here
int rzk_sample_dgauss_keyed_dev(rzk_ctx* c, const uint8_t nonce[16], uint32_t stream, uint32_t sigma, int64_t* out,
                                size_t count) {
  if (c && count == 0) return RZK_OK;
  if (!c || !out || sigma == 0 || sigma > kDgaussSigmaMax || count % c->N != 0) return RZK_E_ARG;
  const size_t npoly = count / c->N;
  uint32_t sk[8];
  LaunchCfg cfg;
  const int rc = keyed_begin(c, nonce, npoly, sk, cfg);
  if (rc != RZK_OK) return rc;
  return keyed_end(c, launch_sample_dgauss_chacha(cfg, out, npoly, c->N, sk, stream, sigma), sk);
}
int rzk_sample_challenge_keyed_dev(rzk_ctx* c, const uint8_t nonce[16], uint32_t stream, int64_t* out, size_t count) {
  if (c && count == 0) return RZK_OK;
  if (!c || !out) return RZK_E_ARG;
  uint32_t sk[8];
  LaunchCfg cfg;
  const int rc = keyed_begin(c, nonce, count, sk, cfg);
  if (rc != RZK_OK) return rc;
  return keyed_end(c, launch_sample_challenge_chacha(cfg, out, count, c->N, sk, stream, c->kappa), sk);
}

namespace {

// accept &= check_verify_constraint(z) && (a1.z == t + c1 (.) d)      (open.rs:167-173, sum.rs:262-298)
// specs: z[k], t[n], c[n+l], d.  group / batch / nflags as in run_program; preset: initialise accept.
// n == 1: one launch, the d-product is a rotation term inside the relation row.  n >= 2 (and rotations +
// row groups available): a1.z as ONE grouped launch (each z_j transformed once for the n rows, norm predicate
// fused) into `w`, then the relation rows as pure rotations (shift_row_kernel) — 18 instead of 48 transform
// units per (4,9,4) relation.
int run_a1_relation(rzk_ctx* c, const std::vector<OpSpec>& specs, int64_t* w, uint8_t* accept, uint32_t group,
                    uint64_t batch, uint64_t nflags, bool preset) {
  // (at N = 2048 the first step runs as row blocks and the second as transform products)
  const bool blocks = !c->small && c->logn >= 10 && c->logn >= c->block_min_logn;
  const bool split = w && c->n >= 2 && ((shift_ok(c) && c->use_groups && c->group_max > 1) || blocks);
  int rc;
  if (split) {
    const std::vector<OpSpec> a1z = {specs[0], {w, c->n, 0}};
    // verifier side: non-canonical prover data clears the proof's verdict, the call itself succeeds (sticky = false)
    rc = run_program_checked(c, PG_A1Z, 0, a1z, accept, group, batch, nflags, c->verify_bound, preset, false);
    if (rc == RZK_E_UNSUPPORTED) {
      rc = run_norm(c, specs[0].base, group * c->k, c->verify_bound, accept, nflags, preset ? 0 : 1, 0, false);
      if (rc != RZK_OK) return rc;
      rc = run_program(c, PG_A1Z, 0, a1z, accept, group, batch, 0, false);
    }
    if (rc != RZK_OK) return rc;
    return run_program(c, PG_REL_ROT, 0, {{w, c->n, 0}, specs[1], specs[2], specs[3]}, accept, group, batch, 0, false);
  }
  rc = run_program_checked(c, PG_A1_RELATION, 0, specs, accept, group, batch, nflags, c->verify_bound, preset, false);
  if (rc != RZK_E_UNSUPPORTED) return rc;
  rc = run_norm(c, specs[0].base, group * c->k, c->verify_bound, accept, nflags, preset ? 0 : 1, 0, false);
  if (rc != RZK_OK) return rc;
  return run_program(c, PG_A1_RELATION, 0, specs, accept, group, batch, 0, false);
}

}  // namespace

// =================================================================================================
// Commitment scheme
// =================================================================================================
int rzk_commit_batch_dev(rzk_ctx* c, const int64_t* x, const int64_t* r, int64_t* cm, uint8_t* ok, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !x || !r || !cm) return RZK_E_ARG;
  const std::vector<OpSpec> specs = {{x, c->l, 0}, {r, c->k, 0}, {cm, c->n + c->l, 0}};
  int rc = run_program_checked(c, PG_COMMIT, 0, specs, ok, 1, B, B, c->commit_bound);
  if (rc != RZK_E_UNSUPPORTED) return rc;
  // unfused: the exact norm kernel sets ok, then the rows clear it again for proofs with non-canonical inputs
  if (ok) rc = run_norm(c, r, c->k, c->commit_bound, ok, B, 0, 0);
  if (ok && rc != RZK_OK) return rc;
  return run_program(c, PG_COMMIT, 0, specs, ok, 1, B);
}

int rzk_commitment_verify_batch_dev(rzk_ctx* c, const int64_t* cm, const int64_t* x, const int64_t* r,
                                    const int64_t* f, uint8_t* ok, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !cm || !x || !r || !ok) return RZK_E_ARG;
  const uint32_t var = f ? 2u : 0u;
  const std::vector<OpSpec> specs = {{x, c->l, 0}, {r, c->k, 0}, {cm, c->n + c->l, 0}, {f, 1, 0}};
  // commit.rs:183-185: the norm predicate on r rides on the rows that load r
  int rc = run_program_checked(c, PG_COMMIT_VERIFY, var, specs, ok, 1, B, B, c->commit_bound, true, false);
  if (rc != RZK_E_UNSUPPORTED) return rc;
  rc = run_norm(c, r, c->k, c->commit_bound, ok, B, 0, 0, false);
  if (rc != RZK_OK) return rc;
  return run_program(c, PG_COMMIT_VERIFY, var, specs, ok, 1, B, 0, false);
}

// =================================================================================================
// OpenProof
// =================================================================================================
int rzk_open_commit_batch_dev(rzk_ctx* c, const int64_t* x, const int64_t* r, const int64_t* y, int64_t* cm,
                              int64_t* t, uint8_t* ok, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !x || !r || !y || !cm || !t) return RZK_E_ARG;
  const std::vector<OpSpec> specs = {{x, c->l, 0}, {r, c->k, 0}, {y, c->k, 0}, {cm, c->n + c->l, 0}, {t, c->n, 0}};
  // check_commit_constraint(r) (params.rs:102-108) rides on the loads of r the commit rows do anyway
  int rc = run_program_checked(c, PG_OPEN_COMMIT, 0, specs, ok, 1, B, B, c->commit_bound);
  if (rc != RZK_E_UNSUPPORTED) return rc;
  if (ok) rc = run_norm(c, r, c->k, c->commit_bound, ok, B, 0, 0);
  if (ok && rc != RZK_OK) return rc;
  return run_program(c, PG_OPEN_COMMIT, 0, specs, ok, 1, B);
}

int rzk_open_response_batch_dev(rzk_ctx* c, const int64_t* y, const int64_t* r, const int64_t* d, int64_t* z,
                                size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !y || !r || !d || !z) return RZK_E_ARG;
  return run_program(c, PG_RESPONSE, 1, {{d, 1, 0}, {y, c->k, 0}, {r, c->k, 0}, {z, c->k, 0}}, nullptr, 1, B);
}

int rzk_open_verify_batch_dev(rzk_ctx* c, const int64_t* z, const int64_t* t, const int64_t* cm, const int64_t* d,
                              uint8_t* accept, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !z || !t || !cm || !d || !accept) return RZK_E_ARG;
  if (c->n != c->l) return fail(c, RZK_E_ARG, "c1_c2 split needs n == l (reference panics in Mat::add)");
  const std::vector<OpSpec> specs = {{z, c->k, 0}, {t, c->n, 0}, {cm, c->n + c->l, 0}, {d, 1, 0}};
  int rc = arena_reserve(c, c->ws, polys(c, B * c->n));
  if (rc != RZK_OK) return rc;
  // open.rs:167-173: the norm predicate on z rides on the rows that load z
  return run_a1_relation(c, specs, (int64_t*)c->ws.p, accept, 1, B, B, true);
}

// =================================================================================================
// LinearProof
// =================================================================================================
int rzk_linear_commit_batch_dev(rzk_ctx* c, const int64_t* g, const int64_t* x, const int64_t* r, const int64_t* rp,
                                const int64_t* y, const int64_t* yp, int64_t* cm, int64_t* cpm, int64_t* t,
                                int64_t* tp, int64_t* u, uint8_t* ok, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !g || !x || !r || !rp || !y || !yp || !cm || !cpm || !t || !tp || !u) return RZK_E_ARG;
  const uint32_t n = c->n, k = c->k, l = c->l;
  int rc = arena_reserve(c, c->ws, polys(c, 2 * B * l));
  if (rc != RZK_OK) return rc;
  int64_t* gx = (int64_t*)c->ws.p;
  int64_t* a2y = gx + B * l * c->N;
  // the multiplier g of every proof, transformed once for the rows that multiply by it (gx, u)
  rc = prepare_dkey(c, g, B, 1, 2 * l, nullptr, true);      // l rows of gx, l rows of u
  if (rc != RZK_OK) return rc;
  struct DkeyScope {
    rzk_ctx* c;
    ~DkeyScope() { c->dkey_img = nullptr; c->dkey_l2 = nullptr; c->dkey_n = 0; }
  } dkey_scope{c};
  // linear.rs:91-95: gx = x_i * g
  rc = run_program(c, PG_CMUL, l | dkv(c), {{x, l, 0}, {g, 1, 0}, {gx, l, 0}}, nullptr, 1, B);
  if (rc != RZK_OK) return rc;
  const std::vector<OpSpec> c2 = {{x, l, 0}, {gx, l, 0}, {r, k, 0}, {rp, k, 0}, {y, k, 0}, {yp, k, 0}, {cm, n + l, 0},
                                  {cpm, n + l, 0}, {t, n, 0}, {tp, n, 0}, {a2y, l, 0}};
  // the norm predicates on r (bit 0 of ok) and rp (bit 1) ride on the commit rows when the kernel path allows
  bool fused = false;
  if (ok) {
    rc = run_program_checked(c, PG_LIN_COMMIT2, 0, c2, ok, 1, B, B, c->commit_bound);
    if (rc != RZK_OK && rc != RZK_E_UNSUPPORTED) return rc;
    fused = rc == RZK_OK;
  }
  if (!fused) {
    if (ok) {   // bit 0: constraint(r), bit 1: constraint(rp); the rows below clear the byte on non-canonical inputs
      rc = run_norm(c, r, k, c->commit_bound, ok, B, 0, 0);
      if (rc != RZK_OK) return rc;
      rc = run_norm(c, rp, k, c->commit_bound, ok, B, 2, 1);
      if (rc != RZK_OK) return rc;
    }
    rc = run_program(c, PG_LIN_COMMIT2, 0, c2, ok, 1, B);
    if (rc != RZK_OK) return rc;
  }
  return run_program(c, PG_LIN_U, dkv(c), {{a2y, l, 0}, {g, 1, 0}, {yp, k, 0}, {u, l, 0}}, ok, 1, B);
}

int rzk_linear_response_batch_dev(rzk_ctx* c, const int64_t* y, const int64_t* yp, const int64_t* r,
                                  const int64_t* rp, const int64_t* d, int64_t* z, int64_t* zp, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !y || !yp || !r || !rp || !d || !z || !zp) return RZK_E_ARG;
  const uint32_t k = c->k;
  return run_program(c, PG_RESPONSE, 2, {{d, 1, 0}, {y, k, 0}, {r, k, 0}, {z, k, 0}, {yp, k, 0}, {rp, k, 0}, {zp, k, 0}},
                     nullptr, 1, B);
}

int rzk_linear_verify_batch_dev(rzk_ctx* c, const int64_t* z, const int64_t* zp, const int64_t* cm,
                                const int64_t* cpm, const int64_t* g, const int64_t* t, const int64_t* tp,
                                const int64_t* u, const int64_t* d, uint8_t* accept, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !z || !zp || !cm || !cpm || !g || !t || !tp || !u || !d || !accept) return RZK_E_ARG;
  if (c->n != c->l) return fail(c, RZK_E_ARG, "c1_c2 split needs n == l (reference panics in Mat::add)");
  const uint32_t n = c->n, k = c->k, l = c->l;
  int rc = arena_reserve(c, c->ws, polys(c, 2 * B * l));
  if (rc != RZK_OK) return rc;
  int64_t* w1 = (int64_t*)c->ws.p;
  int64_t* w2 = w1 + B * l * c->N;
  const std::vector<OpSpec> v1 = {{z, k, 0}, {zp, k, 0}, {t, n, 0}, {tp, n, 0}, {cm, n + l, 0}, {cpm, n + l, 0},
                                  {d, 1, 0}, {g, 1, 0}, {w1, l, 0}, {w2, l, 0}};
  if (c->lin_e && !c->small) {
    // rearranged (PG_LIN_V1B / V2B): no product with g in the first program, so it runs on the unit kernel (and
    // initialises the verdicts itself where one team owns a proof); w1 / w2 hold e / e'
    const std::vector<OpSpec> v1b = {{z, k, 0}, {zp, k, 0}, {t, n, 0}, {tp, n, 0}, {cm, n + l, 0}, {cpm, n + l, 0},
                                     {d, 1, 0}, {w1, l, 0}, {w2, l, 0}};
    rc = run_program_checked(c, PG_LIN_V1B, 0, v1b, accept, 1, B, B, c->verify_bound, true, false);
    if (rc == RZK_E_UNSUPPORTED) {
      rc = run_norm(c, z, k, c->verify_bound, accept, B, 0, 0, false);
      if (rc != RZK_OK) return rc;
      rc = run_norm(c, zp, k, c->verify_bound, accept, B, 1, 0, false);
      if (rc != RZK_OK) return rc;
      rc = run_program(c, PG_LIN_V1B, 0, v1b, accept, 1, B, 0, false);
    }
    if (rc != RZK_OK) return rc;
    rc = prepare_dkey(c, g, B, 1, l, accept, false);   // (after the verdicts exist; l rows multiply by g)
    if (rc != RZK_OK) return rc;
    struct DkeyScopeE {
      rzk_ctx* c;
      ~DkeyScopeE() { c->dkey_img = nullptr; c->dkey_l2 = nullptr; c->dkey_n = 0; }
    } dkey_scope_e{c};
    return run_program(c, PG_LIN_V2B, dkv(c), {{w1, l, 0}, {w2, l, 0}, {g, 1, 0}, {u, l, 0}}, accept, 1, B, 0, false);
  }
  // The verdicts are initialised first, then the multiplier's images are prepared (a non-canonical g clears its proof's
  // verdict: nothing may preset the flags after that), then the rows.
  rc = check_launch(c, launch_fill_u8(cfg_of(c), accept, 1, B), "flag preset");
  if (rc != RZK_OK) return rc;
  rc = prepare_dkey(c, g, B, 1, 2 * l, accept, false);
  if (rc != RZK_OK) return rc;
  struct DkeyScope {
    rzk_ctx* c;
    ~DkeyScope() { c->dkey_img = nullptr; c->dkey_l2 = nullptr; c->dkey_n = 0; }
  } dkey_scope{c};
  // linear.rs:218-223: norm predicates on z and zp, fused into the rows that load them when possible
  rc = run_program_checked(c, PG_LIN_V1, dkv(c), v1, accept, 1, B, B, c->verify_bound, false, false);
  if (rc == RZK_E_UNSUPPORTED) {
    rc = run_norm(c, z, k, c->verify_bound, accept, B, 1, 0, false);
    if (rc != RZK_OK) return rc;
    rc = run_norm(c, zp, k, c->verify_bound, accept, B, 1, 0, false);
    if (rc != RZK_OK) return rc;
    rc = run_program(c, PG_LIN_V1, dkv(c), v1, accept, 1, B, 0, false);
  }
  if (rc != RZK_OK) return rc;
  return run_program(c, PG_LIN_V2, dkv(c), {{w1, l, 0}, {w2, l, 0}, {g, 1, 0}, {d, 1, 0}, {zp, k, 0}, {u, l, 0}}, accept, 1, B, 0,
                     false);
}

// =================================================================================================
// SumProof
// =================================================================================================
namespace {
// sum_i g_i (.) (a2.v_i) - a2.v'  (sum.rs:154-160, 301-308) evaluated as a2.(sum_i g_i (.) v_i - v'): V matrix-vector
// products (each with its inverse transforms) become one, for (columns of a2) instead of l rows of V vector x vector
// terms.  Chosen by transform count (forward + inverse, per proof): pays when V is large and a2 has few columns beyond
// its identity block — the reference's key shape; a dense a2 with k > l columns keeps the row-wise form.
bool sum_uses_d(const rzk_ctx* c, uint32_t V) {
  if (c->small) return false;
  if (c->sum_d >= 0) return c->sum_d != 0;
  const uint32_t n = c->n, k = c->k, l = c->l;
  uint32_t cols = 0, fwd = 0, key_terms = 0;   // columns a2 uses; of those with general entries; general entries in all
  for (uint32_t col = 0; col < k; ++col) {
    bool used = false, general = false;
    for (uint32_t j = 0; j < l; ++j) {
      const uint8_t kc = c->key_class[(n + j) * k + col];
      used = used || kc != KC_ZERO;
      general = general || kc == KC_GENERAL;
      key_terms += kc == KC_GENERAL;
    }
    cols += used;
    fwd += general;
  }
  const uint64_t matvec2 = 2ull * (fwd + l), matvec3 = 3ull * (fwd + l);           // a2.v at two / three primes
  const uint64_t rowwise = (uint64_t)V * matvec2 + (uint64_t)l * (6ull * V + 3) + 3ull * key_terms;
  const uint64_t by_d = (uint64_t)cols * (6ull * V + 3) + matvec3;
  return by_d < rowwise && (uint64_t)cols * V <= (uint64_t)kMaxTerms && cols <= (uint32_t)kMaxRows;
}
}  // namespace

int rzk_sum_commit_batch_dev(rzk_ctx* c, uint32_t V, const int64_t* gs, const int64_t* xs, const int64_t* rs,
                             const int64_t* rp, const int64_t* ys, const int64_t* yp, int64_t* cs, int64_t* cpm,
                             int64_t* ts, int64_t* tp, int64_t* u, uint8_t* ok, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || V == 0 || !gs || !xs || !rs || !rp || !ys || !yp || !cs || !cpm || !ts || !tp || !u) return RZK_E_ARG;
  const uint32_t n = c->n, k = c->k, l = c->l;
  const size_t wpolys = (size_t)B * V * l > (size_t)B * k ? (size_t)B * V * l : (size_t)B * k;   // w[B*V][l], or D[B][k]
  int rc = arena_reserve(c, c->ws, polys(c, B * l + wpolys));
  if (rc != RZK_OK) return rc;
  int64_t* xp = (int64_t*)c->ws.p;
  int64_t* w = xp + B * l * c->N;
  // sum.rs:107-115: xp = sum_i x_i (.) g_i
  // (XP runs before ok is preset: a non-canonical x_i / g_i is reported through the sticky word, and again by the
  //  later rows that load the same polynomials with the flags in place)
  // the V multipliers g_i of every proof, transformed once for all the rows that multiply by them (XP, D / U)
  rc = prepare_dkey(c, gs, B, V, 2 * l, nullptr, true);   // l rows of XP, l or (columns of a2) rows of U / D
  if (rc != RZK_OK) return rc;
  struct DkeyScope {   // the images belong to this call
    rzk_ctx* c;
    ~DkeyScope() { c->dkey_img = nullptr; c->dkey_l2 = nullptr; c->dkey_n = 0; }
  } dkey_scope{c};
  rc = run_program(c, PG_SUM_XP, V | dkv(c), {{xs, V * l, 0}, {gs, V, 0}, {xp, l, 0}}, nullptr, 1, B);
  if (rc != RZK_OK) return rc;
  // the a1.y_i key products below leave the transforms of y_i's a2-columns for the D rows (operand 2 of the summand launch)
  rc = prepare_oimg(c, B, V, 2 * l);
  if (rc != RZK_OK) return rc;
  struct OimgScope {
    rzk_ctx* c;
    ~OimgScope() { c->oimg_state = Operands{}; c->oimg_producer_op = 0xffu; }
  } oimg_scope{c};
  // sum.rs:116 and 151: cp = commit(xp; rp), tp = a1.yp
  const std::vector<OpSpec> cp_specs = {{xp, l, 0}, {rp, k, 0}, {yp, k, 0}, {cpm, n + l, 0}, {tp, n, 0}};
  const std::vector<OpSpec> cs_specs = {{xs, l, 0}, {rs, k, 0}, {ys, k, 0}, {cs, n + l, 0}, {ts, n, 0}};
  // ok[b] = constraint(rp_b) && all_i constraint(r_{b,i}): fused into the commit rows when possible
  const bool fused = ok && can_fuse(c, PG_OPEN_COMMIT, 0, c->commit_bound);
  if (fused) {
    rc = run_program_checked(c, PG_OPEN_COMMIT, 0, cp_specs, ok, 1, B, B, c->commit_bound, true);
    if (rc != RZK_OK) return rc;
    // sum.rs:117-120 and 145-148: c_i = commit(x_i; r_i), t_i = a1.y_i — the V summands are extra batch entries
    c->oimg_producer_op = 2;
    rc = run_program_checked(c, PG_OPEN_COMMIT, 0, cs_specs, ok, V, B * V, B, c->commit_bound, false);
    c->oimg_producer_op = 0xffu;
    if (rc != RZK_OK) return rc;
  } else {
    if (ok) {
      rc = run_norm(c, rp, k, c->commit_bound, ok, B, 0, 0);
      if (rc != RZK_OK) return rc;
      rc = run_norm(c, rs, V * k, c->commit_bound, ok, B, 1, 0);
      if (rc != RZK_OK) return rc;
    }
    rc = run_program(c, PG_OPEN_COMMIT, 0, cp_specs, ok, 1, B);
    if (rc != RZK_OK) return rc;
    c->oimg_producer_op = 2;
    rc = run_program(c, PG_OPEN_COMMIT, 0, cs_specs, ok, V, B * V);
    c->oimg_producer_op = 0xffu;
    if (rc != RZK_OK) return rc;
  }
  // sum.rs:154-160: u = sum_i (a2.y_i)(.)g_i - a2.yp
  if (sum_uses_d(c, V)) {   // = a2.(sum_i g_i(.)y_i - yp): D (k polynomials per proof, the columns a2 uses) lives where w would
    int64_t* D = w;
    rc = run_program(c, PG_SUM_D, V | dkv(c) | oiv(c), {{ys, V * k, 0}, {gs, V, 0}, {yp, k, 0}, {D, k, 0}}, ok, 1, B);
    if (rc != RZK_OK) return rc;
    return run_program(c, PG_MATVEC, RZK_KEY_A2 * 2, {{D, k, 0}, {nullptr, l, 0}, {u, l, 0}}, ok, 1, B);
  }
  rc = run_program(c, PG_MATVEC, RZK_KEY_A2 * 2, {{ys, k, 0}, {nullptr, l, 0}, {w, l, 0}}, nullptr, 1, B * V);
  if (rc != RZK_OK) return rc;
  return run_program(c, PG_SUM_U, V | dkv(c), {{w, V * l, 0}, {gs, V, 0}, {yp, k, 0}, {u, l, 0}}, ok, 1, B);
}

int rzk_sum_response_batch_dev(rzk_ctx* c, uint32_t V, const int64_t* ys, const int64_t* yp, const int64_t* rs,
                               const int64_t* rp, const int64_t* d, int64_t* zs, int64_t* zp, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || V == 0 || !ys || !yp || !rs || !rp || !d || !zs || !zp) return RZK_E_ARG;
  const uint32_t k = c->k;
  // sum.rs:188-193: z_i = y_i + r_i (.) d — summands as batch entries, d shared by the V entries of a proof
  int rc = run_program(c, PG_RESPONSE, 1, {{d, 1, 1}, {ys, k, 0}, {rs, k, 0}, {zs, k, 0}}, nullptr, V, B * V);
  if (rc != RZK_OK) return rc;
  // sum.rs:195-197
  return run_program(c, PG_RESPONSE, 1, {{d, 1, 0}, {yp, k, 0}, {rp, k, 0}, {zp, k, 0}}, nullptr, 1, B);
}

int rzk_sum_verify_batch_dev(rzk_ctx* c, uint32_t V, const int64_t* zs, const int64_t* zp, const int64_t* cs,
                             const int64_t* cpm, const int64_t* gs, const int64_t* ts, const int64_t* tp,
                             const int64_t* u, const int64_t* d, uint8_t* accept, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || V == 0 || !zs || !zp || !cs || !cpm || !gs || !ts || !tp || !u || !d || !accept) return RZK_E_ARG;
  if (c->n != c->l) return fail(c, RZK_E_ARG, "c1_c2 split needs n == l (reference panics in Mat::add)");
  const uint32_t n = c->n, k = c->k, l = c->l;
  const bool by_d = sum_uses_d(c, V);
  const size_t w1polys = by_d && (size_t)B * k > (size_t)B * V * l ? (size_t)B * k : (size_t)B * V * l;   // w1[B*V][l], or D[B][k]
  int rc = arena_reserve(c, c->ws, polys(c, w1polys + B * l + B * V * n));
  if (rc != RZK_OK) return rc;
  int64_t* w1 = (int64_t*)c->ws.p;
  int64_t* w2 = w1 + w1polys * c->N;
  int64_t* w0 = w2 + B * l * c->N;   // a1.z of the relation checks (n >= 2 only)
  const std::vector<OpSpec> rel_s = {{zs, k, 0}, {ts, n, 0}, {cs, n + l, 0}, {d, 1, 1}};
  const std::vector<OpSpec> rel_p = {{zp, k, 0}, {tp, n, 0}, {cpm, n + l, 0}, {d, 1, 0}};
  // sum.rs:262-271 norm predicates ride on sum.rs:278-291 (every summand; batch entries B*V, flag per proof)
  // and sum.rs:294-298
  // (the a1.z_i key products leave the transforms of z_i's a2-columns for the D rows: operand 0 of their launch)
  rc = prepare_oimg(c, B, V, 2 * l);
  if (rc != RZK_OK) return rc;
  struct OimgScope {
    rzk_ctx* c;
    ~OimgScope() { c->oimg_state = Operands{}; c->oimg_producer_op = 0xffu; }
  } oimg_scope{c};
  c->oimg_producer_op = 0;
  rc = run_a1_relation(c, rel_s, w0, accept, V, B * V, B, true);
  c->oimg_producer_op = 0xffu;
  if (rc != RZK_OK) return rc;
  rc = run_a1_relation(c, rel_p, w0, accept, 1, B, B, false);
  if (rc != RZK_OK) return rc;
  // sum.rs:301-319.  The multipliers' images are prepared AFTER the relation rows above have initialised accept: a
  // non-canonical g_i must clear the proof's verdict, and nothing presets the flags again from here on.
  rc = prepare_dkey(c, gs, B, V, 2 * l, accept, false);
  if (rc != RZK_OK) return rc;
  struct DkeyScope {
    rzk_ctx* c;
    ~DkeyScope() { c->dkey_img = nullptr; c->dkey_l2 = nullptr; c->dkey_n = 0; }
  } dkey_scope{c};
  if (by_d) {   // lhs = a2.(sum_i g_i(.)z_i - zp): D in w1's place, then one relation row per row of a2
    int64_t* D = w1;
    rc = run_program(c, PG_SUM_D, V | dkv(c) | oiv(c), {{zs, V * k, 0}, {gs, V, 0}, {zp, k, 0}, {D, k, 0}}, accept, 1, B, 0, false);
    if (rc != RZK_OK) return rc;
    rc = run_program(c, PG_SUM_W2, V | dkv(c), {{cs, V * (n + l), 0}, {gs, V, 0}, {cpm, n + l, 0}, {w2, l, 0}}, accept, 1, B, 0, false);
    if (rc != RZK_OK) return rc;
    return run_program(c, PG_SUM_V4, 0, {{D, k, 0}, {w2, l, 0}, {d, 1, 0}, {u, l, 0}}, accept, 1, B, 0, false);
  }
  rc = run_program(c, PG_MATVEC, RZK_KEY_A2 * 2, {{zs, k, 0}, {nullptr, l, 0}, {w1, l, 0}}, accept, V, B * V, 0, false);
  if (rc != RZK_OK) return rc;
  rc = run_program(c, PG_SUM_W2, V | dkv(c), {{cs, V * (n + l), 0}, {gs, V, 0}, {cpm, n + l, 0}, {w2, l, 0}}, accept, 1, B, 0, false);
  if (rc != RZK_OK) return rc;
  return run_program(c, PG_SUM_V3, V | dkv(c), {{w1, V * l, 0}, {gs, V, 0}, {zp, k, 0}, {w2, l, 0}, {d, 1, 0}, {u, l, 0}}, accept,
                     1, B, 0, false);
}

// =================================================================================================
// host-pointer variants
// =================================================================================================
#define IN(ptr, bytes) HostBuf{(ptr), nullptr, (bytes), nullptr}
#define OUT(ptr, bytes) HostBuf{nullptr, (ptr), (bytes), nullptr}
#define DEV(i, T) ((T)bufs[i].dev)
// A host-pointer call reports exactly its own input faults: the sticky word is cleared on the stream before the call's
// work (a fault left by earlier *_dev calls whose caller never asked — rzk_ctx_check_inputs — is dropped here, as
// include/rzk.h documents) and consumed again when the call fails half-way, so it never leaks into the next call.
#define HOST_WRAP(call)                                                                    \
  do {                                                                                     \
    HIPCHK(c, hipMemsetAsync(c->d_bad, 0, sizeof(uint32_t), c->stream));                   \
    int rc_ = stage_in(c, bufs);                                                           \
    if (rc_ != RZK_OK) return rc_;                                                         \
    rc_ = (call);                                                                          \
    if (rc_ != RZK_OK) {                                                                   \
      const std::string keep_ = c->err;                                                    \
      (void)take_input_error(c);                                                           \
      c->err = keep_;                                                                      \
      return rc_;                                                                          \
    }                                                                                      \
    return stage_out(c, bufs);                                                             \
  } while (0)

int rzk_polymul_batch(rzk_ctx* c, const int64_t* a, const int64_t* b, int64_t* out, size_t count) {
  if (c && count == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !a || !b || !out) return RZK_E_ARG;
  std::vector<HostBuf> bufs = {IN(a, polys(c, count)), IN(b, polys(c, count)), OUT(out, polys(c, count))};
  HOST_WRAP(rzk_polymul_batch_dev(c, DEV(0, const int64_t*), DEV(1, const int64_t*), DEV(2, int64_t*), count));
}

int rzk_matvec_batch(rzk_ctx* c, int which, const int64_t* v, const int64_t* addend, int64_t* out, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !v || !out || which < 0 || which > 2) return RZK_E_ARG;
  const uint32_t rows = which == RZK_KEY_A1 ? c->n : (which == RZK_KEY_A2 ? c->l : c->n + c->l);
  std::vector<HostBuf> bufs = {IN(v, polys(c, B * c->k)), IN(addend, addend ? polys(c, B * rows) : 0),
                               OUT(out, polys(c, B * rows))};
  HOST_WRAP(rzk_matvec_batch_dev(c, which, DEV(0, const int64_t*), addend ? DEV(1, const int64_t*) : nullptr,
                                 DEV(2, int64_t*), B));
}

int rzk_cmul_batch(rzk_ctx* c, const int64_t* m, uint32_t rows, const int64_t* p, int64_t* out, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !m || !p || !out || rows == 0) return RZK_E_ARG;
  std::vector<HostBuf> bufs = {IN(m, polys(c, B * rows)), IN(p, polys(c, B)), OUT(out, polys(c, B * rows))};
  HOST_WRAP(rzk_cmul_batch_dev(c, DEV(0, const int64_t*), rows, DEV(1, const int64_t*), DEV(2, int64_t*), B));
}

int rzk_canonicalize_batch(rzk_ctx* c, const int64_t* in, int64_t* out, size_t count) {
  if (c && count == 0) return RZK_OK;
  if (!c || !in || !out) return RZK_E_ARG;
  std::vector<HostBuf> bufs = {IN(in, polys(c, count)), OUT(out, polys(c, count))};
  HOST_WRAP(rzk_canonicalize_batch_dev(c, DEV(0, const int64_t*), DEV(1, int64_t*), count));
}

int rzk_add_batch(rzk_ctx* c, const int64_t* a, const int64_t* b, int64_t* out, size_t count) {
  if (c && count == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !a || !b || !out) return RZK_E_ARG;
  std::vector<HostBuf> bufs = {IN(a, polys(c, count)), IN(b, polys(c, count)), OUT(out, polys(c, count))};
  HOST_WRAP(rzk_add_batch_dev(c, DEV(0, const int64_t*), DEV(1, const int64_t*), DEV(2, int64_t*), count));
}

int rzk_sub_batch(rzk_ctx* c, const int64_t* a, const int64_t* b, int64_t* out, size_t count) {
  if (c && count == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !a || !b || !out) return RZK_E_ARG;
  std::vector<HostBuf> bufs = {IN(a, polys(c, count)), IN(b, polys(c, count)), OUT(out, polys(c, count))};
  HOST_WRAP(rzk_sub_batch_dev(c, DEV(0, const int64_t*), DEV(1, const int64_t*), DEV(2, int64_t*), count));
}

int rzk_norm2_le_batch(rzk_ctx* c, const int64_t* v, uint32_t rows, uint64_t bound, uint8_t* ok, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !v || !ok || rows == 0) return RZK_E_ARG;
  std::vector<HostBuf> bufs = {IN(v, polys(c, B * rows)), OUT(ok, B)};
  HOST_WRAP(rzk_norm2_le_batch_dev(c, DEV(0, const int64_t*), rows, bound, DEV(1, uint8_t*), B));
}

int rzk_eq_batch(rzk_ctx* c, const int64_t* a, const int64_t* b, uint32_t rows, uint8_t* eq, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !a || !b || !eq || rows == 0) return RZK_E_ARG;
  std::vector<HostBuf> bufs = {IN(a, polys(c, B * rows)), IN(b, polys(c, B * rows)), OUT(eq, B)};
  HOST_WRAP(rzk_eq_batch_dev(c, DEV(0, const int64_t*), DEV(1, const int64_t*), rows, DEV(2, uint8_t*), B));
}

int rzk_ntt_forward_batch(rzk_ctx* c, int prime, const uint32_t* in, uint32_t* out, size_t count) {
  if (c && count == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !in || !out) return RZK_E_ARG;
  const size_t bytes = count * c->N * sizeof(uint32_t);
  std::vector<HostBuf> bufs = {IN(in, bytes), OUT(out, bytes)};
  HOST_WRAP(rzk_ntt_forward_batch_dev(c, prime, DEV(0, const uint32_t*), DEV(1, uint32_t*), count));
}

int rzk_ntt_inverse_batch(rzk_ctx* c, int prime, const uint32_t* in, uint32_t* out, size_t count) {
  if (c && count == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !in || !out) return RZK_E_ARG;
  const size_t bytes = count * c->N * sizeof(uint32_t);
  std::vector<HostBuf> bufs = {IN(in, bytes), OUT(out, bytes)};
  HOST_WRAP(rzk_ntt_inverse_batch_dev(c, prime, DEV(0, const uint32_t*), DEV(1, uint32_t*), count));
}

int rzk_commit_batch(rzk_ctx* c, const int64_t* x, const int64_t* r, int64_t* cm, uint8_t* ok, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !x || !r || !cm) return RZK_E_ARG;
  std::vector<HostBuf> bufs = {IN(x, polys(c, B * c->l)), IN(r, polys(c, B * c->k)),
                               OUT(cm, polys(c, B * (c->n + c->l))), OUT(ok, ok ? B : 0)};
  HOST_WRAP(rzk_commit_batch_dev(c, DEV(0, const int64_t*), DEV(1, const int64_t*), DEV(2, int64_t*),
                                 ok ? DEV(3, uint8_t*) : nullptr, B));
}

int rzk_commitment_verify_batch(rzk_ctx* c, const int64_t* cm, const int64_t* x, const int64_t* r, const int64_t* f,
                                uint8_t* ok, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !cm || !x || !r || !ok) return RZK_E_ARG;
  std::vector<HostBuf> bufs = {IN(cm, polys(c, B * (c->n + c->l))), IN(x, polys(c, B * c->l)),
                               IN(r, polys(c, B * c->k)), IN(f, f ? polys(c, B) : 0), OUT(ok, B)};
  HOST_WRAP(rzk_commitment_verify_batch_dev(c, DEV(0, const int64_t*), DEV(1, const int64_t*), DEV(2, const int64_t*),
                                            f ? DEV(3, const int64_t*) : nullptr, DEV(4, uint8_t*), B));
}

int rzk_open_commit_batch(rzk_ctx* c, const int64_t* x, const int64_t* r, const int64_t* y, int64_t* cm, int64_t* t,
                          uint8_t* ok, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !x || !r || !y || !cm || !t) return RZK_E_ARG;
  std::vector<HostBuf> bufs = {IN(x, polys(c, B * c->l)), IN(r, polys(c, B * c->k)), IN(y, polys(c, B * c->k)),
                               OUT(cm, polys(c, B * (c->n + c->l))), OUT(t, polys(c, B * c->n)), OUT(ok, ok ? B : 0)};
  HOST_WRAP(rzk_open_commit_batch_dev(c, DEV(0, const int64_t*), DEV(1, const int64_t*), DEV(2, const int64_t*),
                                      DEV(3, int64_t*), DEV(4, int64_t*), ok ? DEV(5, uint8_t*) : nullptr, B));
}

int rzk_open_response_batch(rzk_ctx* c, const int64_t* y, const int64_t* r, const int64_t* d, int64_t* z, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !y || !r || !d || !z) return RZK_E_ARG;
  std::vector<HostBuf> bufs = {IN(y, polys(c, B * c->k)), IN(r, polys(c, B * c->k)), IN(d, polys(c, B)),
                               OUT(z, polys(c, B * c->k))};
  HOST_WRAP(rzk_open_response_batch_dev(c, DEV(0, const int64_t*), DEV(1, const int64_t*), DEV(2, const int64_t*),
                                        DEV(3, int64_t*), B));
}

int rzk_open_verify_batch(rzk_ctx* c, const int64_t* z, const int64_t* t, const int64_t* cm, const int64_t* d,
                          uint8_t* accept, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !z || !t || !cm || !d || !accept) return RZK_E_ARG;
  std::vector<HostBuf> bufs = {IN(z, polys(c, B * c->k)), IN(t, polys(c, B * c->n)),
                               IN(cm, polys(c, B * (c->n + c->l))), IN(d, polys(c, B)), OUT(accept, B)};
  HOST_WRAP(rzk_open_verify_batch_dev(c, DEV(0, const int64_t*), DEV(1, const int64_t*), DEV(2, const int64_t*),
                                      DEV(3, const int64_t*), DEV(4, uint8_t*), B));
}

int rzk_linear_commit_batch(rzk_ctx* c, const int64_t* g, const int64_t* x, const int64_t* r, const int64_t* rp,
                            const int64_t* y, const int64_t* yp, int64_t* cm, int64_t* cpm, int64_t* t, int64_t* tp,
                            int64_t* u, uint8_t* ok, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !g || !x || !r || !rp || !y || !yp || !cm || !cpm || !t || !tp || !u) return RZK_E_ARG;
  const size_t k = c->k, n = c->n, l = c->l;
  std::vector<HostBuf> bufs = {IN(g, polys(c, B)),          IN(x, polys(c, B * l)),        IN(r, polys(c, B * k)),
                               IN(rp, polys(c, B * k)),     IN(y, polys(c, B * k)),        IN(yp, polys(c, B * k)),
                               OUT(cm, polys(c, B * (n + l))), OUT(cpm, polys(c, B * (n + l))), OUT(t, polys(c, B * n)),
                               OUT(tp, polys(c, B * n)),    OUT(u, polys(c, B * l)),       OUT(ok, ok ? B : 0)};
  HOST_WRAP(rzk_linear_commit_batch_dev(c, DEV(0, const int64_t*), DEV(1, const int64_t*), DEV(2, const int64_t*),
                                        DEV(3, const int64_t*), DEV(4, const int64_t*), DEV(5, const int64_t*),
                                        DEV(6, int64_t*), DEV(7, int64_t*), DEV(8, int64_t*), DEV(9, int64_t*),
                                        DEV(10, int64_t*), ok ? DEV(11, uint8_t*) : nullptr, B));
}

int rzk_linear_response_batch(rzk_ctx* c, const int64_t* y, const int64_t* yp, const int64_t* r, const int64_t* rp,
                              const int64_t* d, int64_t* z, int64_t* zp, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !y || !yp || !r || !rp || !d || !z || !zp) return RZK_E_ARG;
  const size_t kb = polys(c, B * c->k);
  std::vector<HostBuf> bufs = {IN(y, kb), IN(yp, kb), IN(r, kb), IN(rp, kb), IN(d, polys(c, B)), OUT(z, kb), OUT(zp, kb)};
  HOST_WRAP(rzk_linear_response_batch_dev(c, DEV(0, const int64_t*), DEV(1, const int64_t*), DEV(2, const int64_t*),
                                          DEV(3, const int64_t*), DEV(4, const int64_t*), DEV(5, int64_t*),
                                          DEV(6, int64_t*), B));
}

int rzk_linear_verify_batch(rzk_ctx* c, const int64_t* z, const int64_t* zp, const int64_t* cm, const int64_t* cpm,
                            const int64_t* g, const int64_t* t, const int64_t* tp, const int64_t* u, const int64_t* d,
                            uint8_t* accept, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !z || !zp || !cm || !cpm || !g || !t || !tp || !u || !d || !accept) return RZK_E_ARG;
  const size_t k = c->k, n = c->n, l = c->l;
  std::vector<HostBuf> bufs = {IN(z, polys(c, B * k)),   IN(zp, polys(c, B * k)), IN(cm, polys(c, B * (n + l))),
                               IN(cpm, polys(c, B * (n + l))), IN(g, polys(c, B)), IN(t, polys(c, B * n)),
                               IN(tp, polys(c, B * n)),  IN(u, polys(c, B * l)),  IN(d, polys(c, B)),
                               OUT(accept, B)};
  HOST_WRAP(rzk_linear_verify_batch_dev(c, DEV(0, const int64_t*), DEV(1, const int64_t*), DEV(2, const int64_t*),
                                        DEV(3, const int64_t*), DEV(4, const int64_t*), DEV(5, const int64_t*),
                                        DEV(6, const int64_t*), DEV(7, const int64_t*), DEV(8, const int64_t*),
                                        DEV(9, uint8_t*), B));
}

int rzk_sum_commit_batch(rzk_ctx* c, uint32_t V, const int64_t* gs, const int64_t* xs, const int64_t* rs,
                         const int64_t* rp, const int64_t* ys, const int64_t* yp, int64_t* cs, int64_t* cpm,
                         int64_t* ts, int64_t* tp, int64_t* u, uint8_t* ok, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || V == 0 || !gs || !xs || !rs || !rp || !ys || !yp || !cs || !cpm || !ts || !tp || !u) return RZK_E_ARG;
  const size_t k = c->k, n = c->n, l = c->l;
  std::vector<HostBuf> bufs = {IN(gs, polys(c, B * V)),        IN(xs, polys(c, B * V * l)), IN(rs, polys(c, B * V * k)),
                               IN(rp, polys(c, B * k)),        IN(ys, polys(c, B * V * k)), IN(yp, polys(c, B * k)),
                               OUT(cs, polys(c, B * V * (n + l))), OUT(cpm, polys(c, B * (n + l))),
                               OUT(ts, polys(c, B * V * n)),   OUT(tp, polys(c, B * n)),    OUT(u, polys(c, B * l)),
                               OUT(ok, ok ? B : 0)};
  HOST_WRAP(rzk_sum_commit_batch_dev(c, V, DEV(0, const int64_t*), DEV(1, const int64_t*), DEV(2, const int64_t*),
                                     DEV(3, const int64_t*), DEV(4, const int64_t*), DEV(5, const int64_t*),
                                     DEV(6, int64_t*), DEV(7, int64_t*), DEV(8, int64_t*), DEV(9, int64_t*),
                                     DEV(10, int64_t*), ok ? DEV(11, uint8_t*) : nullptr, B));
}

int rzk_sum_response_batch(rzk_ctx* c, uint32_t V, const int64_t* ys, const int64_t* yp, const int64_t* rs,
                           const int64_t* rp, const int64_t* d, int64_t* zs, int64_t* zp, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || V == 0 || !ys || !yp || !rs || !rp || !d || !zs || !zp) return RZK_E_ARG;
  const size_t k = c->k;
  std::vector<HostBuf> bufs = {IN(ys, polys(c, B * V * k)), IN(yp, polys(c, B * k)), IN(rs, polys(c, B * V * k)),
                               IN(rp, polys(c, B * k)),     IN(d, polys(c, B)),      OUT(zs, polys(c, B * V * k)),
                               OUT(zp, polys(c, B * k))};
  HOST_WRAP(rzk_sum_response_batch_dev(c, V, DEV(0, const int64_t*), DEV(1, const int64_t*), DEV(2, const int64_t*),
                                       DEV(3, const int64_t*), DEV(4, const int64_t*), DEV(5, int64_t*),
                                       DEV(6, int64_t*), B));
}

int rzk_sum_verify_batch(rzk_ctx* c, uint32_t V, const int64_t* zs, const int64_t* zp, const int64_t* cs,
                         const int64_t* cpm, const int64_t* gs, const int64_t* ts, const int64_t* tp, const int64_t* u,
                         const int64_t* d, uint8_t* accept, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || V == 0 || !zs || !zp || !cs || !cpm || !gs || !ts || !tp || !u || !d || !accept) return RZK_E_ARG;
  const size_t k = c->k, n = c->n, l = c->l;
  std::vector<HostBuf> bufs = {IN(zs, polys(c, B * V * k)),       IN(zp, polys(c, B * k)),
                               IN(cs, polys(c, B * V * (n + l))), IN(cpm, polys(c, B * (n + l))),
                               IN(gs, polys(c, B * V)),           IN(ts, polys(c, B * V * n)),
                               IN(tp, polys(c, B * n)),           IN(u, polys(c, B * l)),
                               IN(d, polys(c, B)),                OUT(accept, B)};
  HOST_WRAP(rzk_sum_verify_batch_dev(c, V, DEV(0, const int64_t*), DEV(1, const int64_t*), DEV(2, const int64_t*),
                                     DEV(3, const int64_t*), DEV(4, const int64_t*), DEV(5, const int64_t*),
                                     DEV(6, const int64_t*), DEV(7, const int64_t*), DEV(8, const int64_t*),
                                     DEV(9, uint8_t*), B));
}

// =================================================================================================
// instrumentation
// =================================================================================================
double rzk_bench_ntt_forward_dev(rzk_ctx* c, int prime, const uint32_t* in, uint32_t* out, size_t count, int iters) {
  if (!c || !in || !out || iters <= 0 || prime < 0 || prime >= kMaxPrimes) return (double)RZK_E_ARG;
  hipEvent_t e0, e1;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return (double)RZK_E_HIP;
  // warm-up launch, then `iters` back-to-back launches between two events on the launch stream
  int rc = rzk_ntt_forward_batch_dev(c, prime, in, out, count);
  if (rc == RZK_OK && hipEventRecord(e0, c->stream) != hipSuccess) rc = RZK_E_HIP;
  for (int i = 0; i < iters && rc == RZK_OK; ++i) rc = rzk_ntt_forward_batch_dev(c, prime, in, out, count);
  if (rc == RZK_OK && hipEventRecord(e1, c->stream) != hipSuccess) rc = RZK_E_HIP;
  if (rc == RZK_OK && hipEventSynchronize(e1) != hipSuccess) rc = RZK_E_HIP;
  float ms = 0.f;
  if (rc == RZK_OK && hipEventElapsedTime(&ms, e0, e1) != hipSuccess) rc = RZK_E_HIP;
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (rc != RZK_OK) return (double)rc;
  return (double)ms * 1000.0 / iters;
}

// Diagnostic: copy of the row-kernel scratch (per-wave lines; builds with -DRZK_STAMPS=1 leave wave time stamps there).
int rzk_debug_read_scratch(rzk_ctx* c, void* dst, size_t bytes, size_t* total) {
  if (!c) return RZK_E_ARG;
  const size_t all = c->d_row_scratch ? row_scratch_words((int)c->logn, c->num_cus) * sizeof(uint32_t) : 0;
  if (total) *total = all;
  if (!dst || !bytes) return RZK_OK;
  if (bytes > all) bytes = all;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(dst, c->d_row_scratch, bytes, hipMemcpyDeviceToHost));
  return RZK_OK;
}

// Diagnostic: the Gaussian samplers' word-to-pair map on the caller's words (one thread per pair).
int rzk_debug_gauss_map_dev(rzk_ctx* c, int f32, const uint32_t* words, double sigma, int64_t* out, size_t pairs) {
  if (c && pairs == 0) return RZK_OK;
  if (!c || !words || !out || !(sigma > 0.0) || sigma > 67108864.0 || (f32 && !(sigma < 524288.0))) return RZK_E_ARG;
  return check_launch(c, launch_debug_gauss_map(cfg_of(c), f32 != 0, words, sigma, out, pairs), "gauss map kernel");
}

// Diagnostic: one trial of the exact discrete Gaussian sampler on the caller's words (one thread per trial).
int rzk_debug_dgauss_trial_dev(rzk_ctx* c, uint32_t sigma, const uint32_t* words, int64_t* out, size_t trials) {
  if (c && trials == 0) return RZK_OK;
  if (!c || !words || !out || sigma == 0 || sigma > kDgaussSigmaMax) return RZK_E_ARG;
  return check_launch(c, launch_debug_dgauss_trial(cfg_of(c), sigma, words, out, trials), "dgauss trial kernel");
}

int rzk_prof_enable(rzk_ctx* c, int on) {
  if (!c) return RZK_E_ARG;
  c->prof = on != 0;
  return RZK_OK;
}

int rzk_prof_reset(rzk_ctx* c) {
  if (!c) return RZK_E_ARG;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->prof_used = 0;
  c->prof_us = 0.0;
  c->prof_launches = 0;
  return RZK_OK;
}

uint64_t rzk_prof_count(const rzk_ctx* c) { return c ? (uint64_t)c->prof_used : 0; }

int rzk_prof_read_all(rzk_ctx* c, double* us, size_t cap, size_t* count) {
  if (!c || (!us && cap)) return RZK_E_ARG;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (count) *count = c->prof_used;
  for (size_t i = 0; i < c->prof_used && i < cap; ++i) {
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->prof_events[i].first, c->prof_events[i].second));
    us[i] = (double)ms * 1000.0;
  }
  return RZK_OK;
}

// One line per recorded launch, in launch order: "<kernel>\t<algorithmic bytes>\n".  Returns the text's length through
// *needed (without the terminating NUL); copies at most cap - 1 characters.
int rzk_prof_read_kernels(rzk_ctx* c, char* buf, size_t cap, size_t* needed) {
  if (!c || (!buf && cap)) return RZK_E_ARG;
  std::string text;
  for (size_t i = 0; i < c->prof_used && i < c->prof_info.size(); ++i)
    text += c->prof_info[i].kernel + "\t" + std::to_string(c->prof_info[i].bytes) + "\n";
  if (needed) *needed = text.size();
  if (cap) {
    const size_t ncopy = text.size() < cap - 1 ? text.size() : cap - 1;
    std::memcpy(buf, text.data(), ncopy);
    buf[ncopy] = 0;
  }
  return RZK_OK;
}

int rzk_prof_read(rzk_ctx* c, double* row_kernel_us, uint64_t* row_kernel_launches) {
  if (!c) return RZK_E_ARG;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < c->prof_used; ++i) {
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->prof_events[i].first, c->prof_events[i].second));
    c->prof_us += (double)ms * 1000.0;
    c->prof_launches++;
  }
  c->prof_used = 0;
  if (row_kernel_us) *row_kernel_us = c->prof_us;
  if (row_kernel_launches) *row_kernel_launches = c->prof_launches;
  return RZK_OK;
}

// =================================================================================================
// v4: batched codec of the serialized protocol messages (rzk_wire_dev.hip, rzk_wire_walk.h)
// =================================================================================================
namespace {

bool wire_schema_of(const rzk_ctx* c, int kind, uint32_t V, uint32_t coef_bytes, WireSchema* s) {
  return c && wire_schema(kind, c->N, c->n, c->k, c->l, V, coef_bytes, s);
}

// slabs of the fields; only the Option of an Opening may be NULL, and only on encode
bool wire_slabs(const WireSchema& s, int kind, const int64_t* const* fields, bool allow_none, WireSlabs* sl) {
  if (!fields) return false;
  for (int f = 0; f < kWireMaxFields; ++f) sl->ptr[f] = nullptr;
  for (uint32_t f = 0; f < s.nfields; ++f) {
    sl->ptr[f] = const_cast<int64_t*>(fields[f]);
    if (!fields[f] && !(allow_none && kind == WIRE_OPENING && s.f[f].kind == WF_OPT)) return false;
  }
  return true;
}

size_t wire_field_bytes(const rzk_ctx* c, const WireSchema& s, uint32_t f, size_t B) {
  return polys(c, B * (size_t)(s.first[f + 1] - s.first[f]));
}

}  // namespace

size_t rzk_wire_max_bytes(const rzk_ctx* c, int kind, uint32_t V, uint32_t coef_bytes) {
  WireSchema s;
  if (!wire_schema_of(c, kind, V, coef_bytes, &s)) return 0;
  return (size_t)wire_max_bytes(s);
}

int rzk_wire_decode_batch_dev(rzk_ctx* c, int kind, uint32_t V, uint32_t coef_bytes, const uint8_t* bytes,
                              uint64_t total_len, const uint64_t* offsets, int64_t* const* fields, uint8_t* ok,
                              size_t B) {
  WireSchema s;
  if (!wire_schema_of(c, kind, V, coef_bytes, &s)) return fail(c, RZK_E_ARG, "wire decode: bad kind, width or V");
  if (B == 0) return RZK_OK;
  WireSlabs sl;
  if (!bytes || !offsets || !ok || !wire_slabs(s, kind, (const int64_t* const*)fields, false, &sl))
    return fail(c, RZK_E_ARG, "wire decode: NULL pointer");
  if ((uintptr_t)bytes % coef_bytes) return fail(c, RZK_E_ARG, "wire decode: bytes not aligned to coef_bytes");
  if (total_len >> 48) return fail(c, RZK_E_UNSUPPORTED, "wire decode: total_len must stay below 2^48");
  int rc = arena_reserve(c, c->ws_wire, (size_t)B * s.polys * sizeof(uint64_t));
  if (rc != RZK_OK) return rc;
  uint64_t* tab = (uint64_t*)c->ws_wire.p;
  const LaunchCfg cfg = cfg_of(c);
  // an Opening ends with a 1-byte tag, so Openings written back to back start at any byte
  rc = check_launch(c, launch_wire_walk(cfg, bytes, total_len, offsets, s, kind != WIRE_OPENING, tab, ok, B),
                    "wire walk kernel");
  if (rc != RZK_OK) return rc;
  return check_launch(c, launch_wire_copy(cfg, bytes, tab, s, sl, (c->q - 1) / 2, ok, B), "wire copy kernel");
}

int rzk_wire_encode_batch_dev(rzk_ctx* c, int kind, uint32_t V, uint32_t coef_bytes, const int64_t* const* fields,
                              uint8_t* bytes, uint64_t cap, uint64_t* offsets, size_t B) {
  WireSchema s;
  if (!wire_schema_of(c, kind, V, coef_bytes, &s)) return fail(c, RZK_E_ARG, "wire encode: bad kind, width or V");
  if (B == 0) return RZK_OK;
  WireSlabs sl;
  if (!bytes || !offsets || !wire_slabs(s, kind, fields, true, &sl)) return fail(c, RZK_E_ARG, "wire encode: NULL pointer");
  if ((uintptr_t)bytes % coef_bytes) return fail(c, RZK_E_ARG, "wire encode: bytes not aligned to coef_bytes");
  // every message fits its maximum, so the device never writes past cap
  const uint64_t mx = wire_max_bytes(s);
  if (cap / B < mx) return fail(c, RZK_E_ARG, "wire encode: cap < B * rzk_wire_max_bytes");
  const size_t np = (size_t)B * s.polys;
  const size_t lens_b = (np * sizeof(uint32_t) + 255) & ~size_t(255), rel_b = (np * sizeof(uint64_t) + 255) & ~size_t(255);
  int rc = arena_reserve(c, c->ws_wire, lens_b + rel_b + B * sizeof(uint64_t));
  if (rc != RZK_OK) return rc;
  char* w = (char*)c->ws_wire.p;
  return check_launch(c, launch_wire_encode(cfg_of(c), s, sl, (c->q - 1) / 2, (uint32_t*)w, (uint64_t*)(w + lens_b),
                                            (uint64_t*)(w + lens_b + rel_b), bytes, offsets, c->d_bad, B),
                      "wire encode kernels");
}

int rzk_wire_decode_batch(rzk_ctx* c, int kind, uint32_t V, uint32_t coef_bytes, const uint8_t* bytes,
                          uint64_t total_len, const uint64_t* offsets, int64_t* const* fields, uint8_t* ok, size_t B) {
  WireSchema s;
  if (!wire_schema_of(c, kind, V, coef_bytes, &s)) return fail(c, RZK_E_ARG, "wire decode: bad kind, width or V");
  if (B == 0) return RZK_OK;
  WireSlabs sl;
  if (!bytes || !offsets || !ok || !wire_slabs(s, kind, (const int64_t* const*)fields, false, &sl))
    return fail(c, RZK_E_ARG, "wire decode: NULL pointer");
  if ((uintptr_t)bytes % coef_bytes) return fail(c, RZK_E_ARG, "wire decode: bytes not aligned to coef_bytes");
  std::vector<HostBuf> bufs = {IN(bytes, total_len), IN(offsets, (B + 1) * sizeof(uint64_t)), OUT(ok, B)};
  for (uint32_t f = 0; f < s.nfields; ++f) bufs.push_back(OUT(fields[f], wire_field_bytes(c, s, f, B)));
  int64_t* dev_fields[kWireMaxFields] = {};
  HIPCHK(c, hipMemsetAsync(c->d_bad, 0, sizeof(uint32_t), c->stream));
  int rc = stage_in(c, bufs);
  if (rc != RZK_OK) return rc;
  for (uint32_t f = 0; f < s.nfields; ++f) dev_fields[f] = (int64_t*)bufs[3 + f].dev;
  // the staged copy of `bytes` starts on a 256-byte boundary, so alignment and offsets carry over
  rc = rzk_wire_decode_batch_dev(c, kind, V, coef_bytes, DEV(0, const uint8_t*), total_len, DEV(1, const uint64_t*),
                                 dev_fields, DEV(2, uint8_t*), B);
  if (rc != RZK_OK) {
    const std::string keep = c->err;
    (void)take_input_error(c);
    c->err = keep;
    return rc;
  }
  return stage_out(c, bufs);
}

int rzk_wire_encode_batch(rzk_ctx* c, int kind, uint32_t V, uint32_t coef_bytes, const int64_t* const* fields,
                          uint8_t* bytes, uint64_t cap, uint64_t* offsets, size_t B) {
  WireSchema s;
  if (!wire_schema_of(c, kind, V, coef_bytes, &s)) return fail(c, RZK_E_ARG, "wire encode: bad kind, width or V");
  if (B == 0) return RZK_OK;
  WireSlabs sl;
  if (!bytes || !offsets || !wire_slabs(s, kind, fields, true, &sl)) return fail(c, RZK_E_ARG, "wire encode: NULL pointer");
  const uint64_t mx = wire_max_bytes(s);
  if (cap / B < mx) return fail(c, RZK_E_ARG, "wire encode: cap < B * rzk_wire_max_bytes");
  const uint64_t dcap = (uint64_t)B * mx;   // device buffer: what the messages can need, not the caller's whole cap
  std::vector<HostBuf> bufs;
  for (uint32_t f = 0; f < s.nfields; ++f) bufs.push_back(IN(fields[f], fields[f] ? wire_field_bytes(c, s, f, B) : 0));
  bufs.push_back(HostBuf{nullptr, nullptr, (size_t)dcap, nullptr});
  bufs.push_back(OUT(offsets, (B + 1) * sizeof(uint64_t)));
  HIPCHK(c, hipMemsetAsync(c->d_bad, 0, sizeof(uint32_t), c->stream));
  int rc = stage_in(c, bufs);
  if (rc != RZK_OK) return rc;
  const int64_t* dev_fields[kWireMaxFields] = {};
  for (uint32_t f = 0; f < s.nfields; ++f) dev_fields[f] = fields[f] ? (const int64_t*)bufs[f].dev : nullptr;
  uint8_t* dbytes = (uint8_t*)bufs[s.nfields].dev;
  rc = rzk_wire_encode_batch_dev(c, kind, V, coef_bytes, dev_fields, dbytes, dcap, (uint64_t*)bufs[s.nfields + 1].dev, B);
  if (rc == RZK_OK) {
    HIPCHK(c, hipMemcpyAsync(offsets, bufs[s.nfields + 1].dev, (B + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost,
                             c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (offsets[B] > dcap) return fail(c, RZK_E_HIP, "wire encode: message sizes exceed their maximum");
    if (offsets[B]) HIPCHK(c, hipMemcpyAsync(bytes, dbytes, offsets[B], hipMemcpyDeviceToHost, c->stream));
    return take_input_error(c);
  }
  const std::string keep = c->err;
  (void)take_input_error(c);
  c->err = keep;
  return rc;
}

// =================================================================================================
// v5: Fiat-Shamir challenges from the FS1 transcript (rzk_fs_dev.hip, rzk_keccak.h)
// =================================================================================================
int rzk_fs_key_digest(rzk_ctx* c, uint8_t* out) {
  if (!c || !out) return RZK_E_ARG;
  if (!c->key_loaded) return fail(c, RZK_E_STATE, "commitment key not loaded");
  for (uint32_t w = 0; w < kFsDigestWords; ++w)
    for (int i = 0; i < 8; ++i) out[8 * w + i] = (uint8_t)(c->key_digest[w] >> (8 * i));   // little-endian on any host
  return RZK_OK;
}

namespace {
bool fs_kind_ok(int kind) {
  return kind == RZK_MSG_OPEN_COMMITMENT || kind == RZK_MSG_LINEAR_COMMITMENT || kind == RZK_MSG_SUM_COMMITMENT;
}
}  // namespace

int rzk_fs_challenge_batch_dev(rzk_ctx* c, int kind, uint32_t V, const int64_t* const* fields, const uint8_t* aux32,
                               int64_t* d, uint8_t* digest, uint8_t* ok, size_t B) {
  WireSchema s;
  if (!c) return RZK_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));   // the memsets below come before the first cfg_of
  if (!fs_kind_ok(kind) || !wire_schema_of(c, kind, V, 8, &s)) return fail(c, RZK_E_ARG, "fs challenge: bad kind or V");
  if (c->kappa > c->N) return fail(c, RZK_E_ARG, "fs challenge: kappa exceeds the ring degree");
  if (!c->key_loaded) return fail(c, RZK_E_STATE, "commitment key not loaded");
  if (B == 0) return RZK_OK;
  WireSlabs sl;
  if (!d || !wire_slabs(s, kind, fields, false, &sl)) return fail(c, RZK_E_ARG, "fs challenge: NULL pointer");
  FsMsg m{};
  m.nfields = s.nfields;
  m.N = c->N;
  m.polys = s.polys;
  for (uint32_t f = 0; f <= s.nfields; ++f) m.first[f] = s.first[f];
  for (uint32_t f = 0; f < s.nfields; ++f) m.ptr[f] = sl.ptr[f];
  FsRoot r{};
  uint64_t aux[kFsDigestWords] = {};
  if (aux32)
    for (uint32_t w = 0; w < kFsDigestWords; ++w) aux[w] = shake256_load_le(aux32 + 8 * w, 8);
  fs_root_header((uint32_t)kind, kind == RZK_MSG_SUM_COMMITMENT ? V : 0, c->key_digest, aux, r.hdr);
  r.nhdr = kFsRootHeaderWords;
  r.leaves = s.polys * (c->N / fs_leaf_len(c->N));
  r.N = c->N;
  r.kappa = c->kappa;
  int rc = arena_reserve(c, c->ws_fs, (size_t)B * r.leaves * kFsDigestWords * sizeof(uint64_t));
  if (rc != RZK_OK) return rc;
  uint64_t* dig = (uint64_t*)c->ws_fs.p;
  if (ok) HIPCHK(c, hipMemsetAsync(ok, 1, B, c->stream));
  HIPCHK(c, hipMemsetAsync(d, 0, polys(c, B), c->stream));   // the sampler writes the kappa non-zero coefficients only
  const uint64_t hashed = (uint64_t)B * s.polys * c->N * sizeof(int64_t);
  LaunchCfg cfg;
  rc = prof_begin(c, hashed, cfg);
  if (rc != RZK_OK) return rc;
  rc = check_launch(c, launch_fs_leaves(cfg, m, (c->q - 1) / 2, c->trusted ? 0 : 1, dig, ok, c->d_bad, B),
                    "fs leaf kernel");
  if (rc != RZK_OK) return rc;
  rc = prof_end(c);
  if (rc != RZK_OK) return rc;
  rc = prof_begin(c, (uint64_t)B * r.leaves * 32, cfg);
  if (rc != RZK_OK) return rc;
  rc = check_launch(c, launch_fs_roots(cfg, r, dig, d, digest, B), "fs root kernel");
  if (rc != RZK_OK) return rc;
  return prof_end(c);
}

int rzk_fs_challenge_batch(rzk_ctx* c, int kind, uint32_t V, const int64_t* const* fields, const uint8_t* aux32,
                           int64_t* d, uint8_t* digest, uint8_t* ok, size_t B) {
  WireSchema s;
  if (!c) return RZK_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));   // the memsets below come before the first cfg_of
  if (!fs_kind_ok(kind) || !wire_schema_of(c, kind, V, 8, &s)) return fail(c, RZK_E_ARG, "fs challenge: bad kind or V");
  if (B == 0) return RZK_OK;
  WireSlabs sl;
  if (!d || !wire_slabs(s, kind, fields, false, &sl)) return fail(c, RZK_E_ARG, "fs challenge: NULL pointer");
  std::vector<HostBuf> bufs = {OUT(d, polys(c, B)), OUT(digest, digest ? B * 32 : 0), OUT(ok, ok ? B : 0)};
  for (uint32_t f = 0; f < s.nfields; ++f) bufs.push_back(IN(fields[f], wire_field_bytes(c, s, f, B)));
  HIPCHK(c, hipMemsetAsync(c->d_bad, 0, sizeof(uint32_t), c->stream));
  int rc = stage_in(c, bufs);
  if (rc != RZK_OK) return rc;
  const int64_t* dev_fields[kWireMaxFields] = {};
  for (uint32_t f = 0; f < s.nfields; ++f) dev_fields[f] = (const int64_t*)bufs[3 + f].dev;
  rc = rzk_fs_challenge_batch_dev(c, kind, V, dev_fields, aux32, DEV(0, int64_t*), digest ? DEV(1, uint8_t*) : nullptr,
                                  ok ? DEV(2, uint8_t*) : nullptr, B);
  if (rc != RZK_OK) {
    const std::string keep = c->err;
    (void)take_input_error(c);
    c->err = keep;
    return rc;
  }
  return stage_out(c, bufs);
}

// =================================================================================================
// v7: the prover's rejection-sampling step (rzk_reject_dev.hip, rzk_reject.h)
// =================================================================================================
double rzk_reject_lnm(double alpha) { return reject_lnm(alpha); }

namespace {
// argument rules shared by both variants; *total = response polynomials per proof
int reject_args(rzk_ctx* c, uint32_t nparts, const int64_t* const* z, const int64_t* const* y, const uint32_t* rows,
                const int64_t* coin, uint64_t R, double lnM, const uint8_t* accept, uint64_t* total) {
  if (nparts < 1 || nparts > (uint32_t)kRejectMaxParts || !z || !y || !rows || !coin || !accept)
    return fail(c, RZK_E_ARG, "reject: 1 .. 4 parts and non-NULL z, y, rows, coin, accept expected");
  if (R < 2 || R > kRejectMaxR) return fail(c, RZK_E_ARG, "reject: R must lie in [2, 2^62]");
  if (!(lnM >= 0.0) || !std::isfinite(lnM)) return fail(c, RZK_E_ARG, "reject: lnM must be a finite number >= 0");
  uint64_t t = 0;
  for (uint32_t f = 0; f < nparts; ++f) {
    if (!z[f] || !y[f] || rows[f] == 0) return fail(c, RZK_E_ARG, "reject: NULL slab or empty part");
    t += rows[f];
  }
  const uint64_t vmax = c->b < (1ull << 28) ? c->b * c->kappa : ~0ull;
  if (!reject_args_ok(t, c->N, vmax, c->verify_bound))
    return fail(c, RZK_E_ARG, "reject: rows * N * 2^24 * kappa * b must stay below 2^52 (and verify_bound below 2^24)");
  *total = t;
  return RZK_OK;
}
}  // namespace

int rzk_reject_batch_dev(rzk_ctx* c, uint32_t nparts, const int64_t* const* z, const int64_t* const* y, const uint32_t* rows,
                         const int64_t* coin, uint64_t R, double lnM, uint8_t* accept, int64_t* E, size_t B) {
  if (!c) return RZK_E_ARG;
  if (B == 0) return RZK_OK;
  uint64_t total = 0;
  int rc = reject_args(c, nparts, z, y, rows, coin, R, lnM, accept, &total);
  if (rc != RZK_OK) return rc;
  RejectParts m{};
  m.nparts = nparts;
  m.N = c->N;
  m.rows = (uint32_t)total;
  for (uint32_t f = 0; f < nparts; ++f) {
    if (((uintptr_t)z[f] | (uintptr_t)y[f]) & 15u) return fail(c, RZK_E_ARG, "reject: slabs must be 16-byte aligned");
    m.first[f + 1] = m.first[f] + rows[f];
    m.z[f] = z[f];
    m.y[f] = y[f];
  }
  rc = arena_reserve(c, c->ws_reject, (size_t)B * total * sizeof(RejectPartial));
  if (rc != RZK_OK) return rc;
  RejectPartial* part = (RejectPartial*)c->ws_reject.p;
  const uint64_t limit = (c->verify_bound + 1) * (c->verify_bound + 1);   // <= 2^48 (reject_args_ok)
  LaunchCfg cfg;
  rc = prof_begin(c, (uint64_t)B * total * c->N * 2 * sizeof(int64_t), cfg);
  if (rc != RZK_OK) return rc;
  rc = check_launch(c, launch_reject_stat(cfg, m, c->q, c->b * c->kappa, limit, c->trusted, part, B), "reject stat kernel");
  if (rc != RZK_OK) return rc;
  rc = prof_end(c);
  if (rc != RZK_OK) return rc;
  rc = prof_begin(c, (uint64_t)B * total * sizeof(RejectPartial), cfg);
  if (rc != RZK_OK) return rc;
  const double sg = (double)c->sigma;
  rc = check_launch(c, launch_reject_decide(cfg, part, m.rows, coin, R, lnM, 2.0 * sg * sg, accept, E, c->d_bad, B),
                    "reject decide kernel");
  if (rc != RZK_OK) return rc;
  return prof_end(c);
}

int rzk_reject_batch(rzk_ctx* c, uint32_t nparts, const int64_t* const* z, const int64_t* const* y, const uint32_t* rows,
                     const int64_t* coin, uint64_t R, double lnM, uint8_t* accept, int64_t* E, size_t B) {
  if (!c) return RZK_E_ARG;
  if (B == 0) return RZK_OK;
  uint64_t total = 0;
  int rc = reject_args(c, nparts, z, y, rows, coin, R, lnM, accept, &total);
  if (rc != RZK_OK) return rc;
  HIPCHK(c, hipSetDevice(c->device));   // the memset below comes before the first cfg_of
  std::vector<HostBuf> bufs = {IN(coin, B * sizeof(int64_t)), OUT(accept, B), OUT(E, E ? B * sizeof(int64_t) : 0)};
  for (uint32_t f = 0; f < nparts; ++f) {
    bufs.push_back(IN(z[f], polys(c, B * rows[f])));
    bufs.push_back(IN(y[f], polys(c, B * rows[f])));
  }
  HIPCHK(c, hipMemsetAsync(c->d_bad, 0, sizeof(uint32_t), c->stream));
  rc = stage_in(c, bufs);
  if (rc != RZK_OK) return rc;
  const int64_t *dz[kRejectMaxParts] = {}, *dy[kRejectMaxParts] = {};
  for (uint32_t f = 0; f < nparts; ++f) {
    dz[f] = (const int64_t*)bufs[3 + 2 * f].dev;
    dy[f] = (const int64_t*)bufs[4 + 2 * f].dev;
  }
  rc = rzk_reject_batch_dev(c, nparts, dz, dy, rows, DEV(0, const int64_t*), R, lnM, DEV(1, uint8_t*),
                            E ? DEV(2, int64_t*) : nullptr, B);
  if (rc != RZK_OK) {
    const std::string keep = c->err;
    (void)take_input_error(c);
    c->err = keep;
    return rc;
  }
  return stage_out(c, bufs);
}

// =================================================================================================
// v8: fixed-width packed records "RZKP1" (rzk_packed_dev.hip, rzk_packed.h)
// =================================================================================================
static_assert(RZK_MSG_LINEAR_RESPONSE == PK_LINEAR_RESPONSE && RZK_MSG_OPEN_SHORT == PK_OPEN_SHORT &&
                  RZK_MSG_OPENING == PK_OPENING && RZK_MSG_SUM_RESPONSE == PK_SUM_RESPONSE,
              "packed kinds are the RZK_MSG_* values");

namespace {

bool packed_schema_of(const rzk_ctx* c, int kind, uint32_t V, PackedSchema* s) {
  return c && packed_schema(kind, c->N, c->n, c->k, c->l, V, c->q, c->verify_bound, s);
}

// argument rules shared by the four entry points; on RZK_OK *s and *sl are filled
int packed_args(rzk_ctx* c, int kind, uint32_t V, const int64_t* const* fields, const uint8_t* records, const uint8_t* ok,
                size_t B, PackedSchema* s, PackedSlabs* sl) {
  if (!packed_schema_of(c, kind, V, s)) return fail(c, RZK_E_ARG, "packed codec: bad kind or V");
  if (B == 0) return RZK_OK;   // a no-op, whatever the pointers
  if (!fields || !records || !ok) return fail(c, RZK_E_ARG, "packed codec: NULL pointer");
  for (int f = 0; f < kPackedMaxFields; ++f) sl->ptr[f] = nullptr;
  for (uint32_t f = 0; f < s->nfields; ++f) {
    if (!fields[f]) return fail(c, RZK_E_ARG, "packed codec: NULL slab");
    sl->ptr[f] = const_cast<int64_t*>(fields[f]);
  }
  if ((uintptr_t)records % 8) return fail(c, RZK_E_ARG, "packed codec: records must be 8-byte aligned");
  return RZK_OK;
}

size_t packed_field_bytes(const rzk_ctx* c, const PackedSchema& s, uint32_t f, size_t B) { return polys(c, B * (size_t)s.f[f].rows); }

// one launch between preset and profile bookkeeping; decode != 0: records -> slabs
int packed_run(rzk_ctx* c, const PackedSchema& s, const PackedSlabs& sl, uint8_t* records, uint8_t* ok, size_t B, int decode) {
  for (uint32_t f = 0; f < s.nfields; ++f)
    if ((uintptr_t)sl.ptr[f] % 16) return fail(c, RZK_E_ARG, "packed codec: device slabs must be 16-byte aligned");
  HIPCHK(c, hipSetDevice(c->device));   // the memset below comes before the first cfg_of
  HIPCHK(c, hipMemsetAsync(ok, 1, B, c->stream));
  uint64_t slab_bytes = 0;
  for (uint32_t f = 0; f < s.nfields; ++f) slab_bytes += packed_field_bytes(c, s, f, B);
  LaunchCfg cfg;
  int rc = prof_begin(c, slab_bytes + (uint64_t)B * packed_record_bytes(s), cfg);
  if (rc != RZK_OK) return rc;
  rc = decode ? check_launch(c, launch_packed_decode(cfg, s, sl, (const uint64_t*)records, ok, B), "packed decode kernel")
              : check_launch(c, launch_packed_encode(cfg, s, sl, (uint64_t*)records, ok, B), "packed encode kernel");
  if (rc != RZK_OK) return rc;
  return prof_end(c);
}

}  // namespace

size_t rzk_packed_record_bytes(const rzk_ctx* c, int kind, uint32_t V) {
  PackedSchema s;
  if (!packed_schema_of(c, kind, V, &s)) return 0;
  return (size_t)packed_record_bytes(s);
}

int rzk_packed_widths(const rzk_ctx* c, uint32_t* wq, uint32_t* wz) {
  PackedWidth w[PK_NCLASSES];
  if (!c || !wq || !wz) return RZK_E_ARG;
  if (!packed_widths(c->q, c->verify_bound, w)) return RZK_E_UNSUPPORTED;
  *wq = w[PK_Q].W;
  *wz = w[PK_Z].W;
  return RZK_OK;
}

int rzk_packed_encode_batch_dev(rzk_ctx* c, int kind, uint32_t V, const int64_t* const* fields, uint8_t* records, uint8_t* ok,
                                size_t B) {
  PackedSchema s;
  PackedSlabs sl;
  if (!c) return RZK_E_ARG;
  const int rc = packed_args(c, kind, V, fields, records, ok, B, &s, &sl);
  if (rc != RZK_OK || B == 0) return rc;
  return packed_run(c, s, sl, records, ok, B, 0);
}

int rzk_packed_decode_batch_dev(rzk_ctx* c, int kind, uint32_t V, const uint8_t* records, int64_t* const* fields, uint8_t* ok,
                                size_t B) {
  PackedSchema s;
  PackedSlabs sl;
  if (!c) return RZK_E_ARG;
  const int rc = packed_args(c, kind, V, (const int64_t* const*)fields, records, ok, B, &s, &sl);
  if (rc != RZK_OK || B == 0) return rc;
  return packed_run(c, s, sl, const_cast<uint8_t*>(records), ok, B, 1);
}

int rzk_packed_encode_batch(rzk_ctx* c, int kind, uint32_t V, const int64_t* const* fields, uint8_t* records, uint8_t* ok,
                            size_t B) {
  PackedSchema s;
  PackedSlabs sl;
  if (!c) return RZK_E_ARG;
  int rc = packed_args(c, kind, V, fields, records, ok, B, &s, &sl);
  if (rc != RZK_OK || B == 0) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<HostBuf> bufs = {OUT(records, B * (size_t)packed_record_bytes(s)), OUT(ok, B)};
  for (uint32_t f = 0; f < s.nfields; ++f) bufs.push_back(IN(fields[f], packed_field_bytes(c, s, f, B)));
  HIPCHK(c, hipMemsetAsync(c->d_bad, 0, sizeof(uint32_t), c->stream));
  rc = stage_in(c, bufs);
  if (rc != RZK_OK) return rc;
  for (uint32_t f = 0; f < s.nfields; ++f) sl.ptr[f] = (int64_t*)bufs[2 + f].dev;   // staged on 256-byte boundaries
  rc = packed_run(c, s, sl, DEV(0, uint8_t*), DEV(1, uint8_t*), B, 0);
  if (rc != RZK_OK) {
    const std::string keep = c->err;
    (void)take_input_error(c);
    c->err = keep;
    return rc;
  }
  return stage_out(c, bufs);
}

int rzk_packed_decode_batch(rzk_ctx* c, int kind, uint32_t V, const uint8_t* records, int64_t* const* fields, uint8_t* ok,
                            size_t B) {
  PackedSchema s;
  PackedSlabs sl;
  if (!c) return RZK_E_ARG;
  int rc = packed_args(c, kind, V, (const int64_t* const*)fields, records, ok, B, &s, &sl);
  if (rc != RZK_OK || B == 0) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<HostBuf> bufs = {IN(records, B * (size_t)packed_record_bytes(s)), OUT(ok, B)};
  for (uint32_t f = 0; f < s.nfields; ++f) bufs.push_back(OUT(fields[f], packed_field_bytes(c, s, f, B)));
  HIPCHK(c, hipMemsetAsync(c->d_bad, 0, sizeof(uint32_t), c->stream));
  rc = stage_in(c, bufs);
  if (rc != RZK_OK) return rc;
  for (uint32_t f = 0; f < s.nfields; ++f) sl.ptr[f] = (int64_t*)bufs[2 + f].dev;
  rc = packed_run(c, s, sl, DEV(0, uint8_t*), DEV(1, uint8_t*), B, 1);
  if (rc != RZK_OK) {
    const std::string keep = c->err;
    (void)take_input_error(c);
    c->err = keep;
    return rc;
  }
  return stage_out(c, bufs);
}

// =================================================================================================
// v10: commitment keys and public polynomials expanded from 32-byte seeds, "XP1" (rzk_xof_dev.hip, rzk_xof.h)
// =================================================================================================
static_assert(RZK_XOF_DOMAIN_KEY == kXofDomainKey, "the key domain of XP1");

namespace {
// out[b][r] = polynomial p0 + r under seeds[b] and `domain`; seeds and out on the device
int run_xof(rzk_ctx* c, uint32_t domain, uint32_t p0, uint32_t rows, const uint64_t* seeds, int64_t* out, size_t B) {
  const XofJob j{(uint64_t)c->q, c->N, domain, p0, rows, c->N / xof_chunk_len(c->N), xof_mask((uint64_t)c->q)};
  LaunchCfg cfg;
  int rc = prof_begin(c, (uint64_t)B * rows * c->N * sizeof(int64_t), cfg);
  if (rc != RZK_OK) return rc;
  rc = check_launch(c, launch_xof_uniform(cfg, j, seeds, out, B), "xof kernel");
  return rc != RZK_OK ? rc : prof_end(c);
}
}  // namespace

// CommitmentKey::new (commit.rs:33-60) as a public function of the seed: the structure rzk_key_generate builds, with the
// general entry at row i, column j equal to polynomial i * k + j of XP1 under domain 0 (the index is the position, so
// one entry can be recomputed alone).  One launch per key row; the key is then loaded like any other.
int rzk_key_expand(rzk_ctx* c, const uint8_t seed[32], int64_t* a_host_out) {
  if (!c || !seed) return RZK_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  const uint32_t N = c->N, n = c->n, k = c->k, l = c->l;
  const size_t n_rand = (size_t)n * (k - n) + (size_t)l * (k - n - l);
  auto first_general = [&](uint32_t i) { return i < n ? n : n + l; };   // a1 = [I_n | a1'], a2 = [0 | I_l | a2']
  std::vector<int64_t> a((size_t)(n + l) * k * N, 0);
  for (uint32_t i = 0; i < n + l; ++i) a[((size_t)i * k + i) * N] = 1;
  if (n_rand) {
    int rc = arena_reserve(c, c->stage, 256 + polys(c, n_rand));
    if (rc != RZK_OK) return rc;
    int64_t* d_out = (int64_t*)((char*)c->stage.p + 256);
    HIPCHK(c, hipMemcpyAsync(c->stage.p, seed, 32, hipMemcpyHostToDevice, c->stream));
    size_t next = 0;
    for (uint32_t i = 0; i < n + l; ++i) {
      const uint32_t j0 = first_general(i);
      if (j0 == k) continue;
      rc = run_xof(c, kXofDomainKey, i * k + j0, k - j0, (const uint64_t*)c->stage.p, d_out + next * N, 1);
      if (rc != RZK_OK) return rc;
      next += k - j0;
    }
    next = 0;
    for (uint32_t i = 0; i < n + l; ++i) {   // the rows' general entries are contiguous in the matrix as in the staging slab
      const uint32_t j0 = first_general(i);
      if (j0 == k) continue;
      HIPCHK(c, hipMemcpyAsync(a.data() + ((size_t)i * k + j0) * N, d_out + next * N, polys(c, k - j0), hipMemcpyDeviceToHost,
                               c->stream));
      next += k - j0;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  if (a_host_out) std::memcpy(a_host_out, a.data(), a.size() * sizeof(int64_t));
  return key_load_impl(c, a.data());
}

int rzk_xof_uniform_batch_dev(rzk_ctx* c, const uint8_t* seeds, uint32_t domain, uint32_t rows, int64_t* out, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !seeds || !out || rows == 0) return RZK_E_ARG;
  if (domain == RZK_XOF_DOMAIN_KEY) return fail(c, RZK_E_ARG, "xof: domain 0 is reserved for commitment keys (rzk_key_expand)");
  if (((uintptr_t)seeds & 7u) || ((uintptr_t)out & 15u))
    return fail(c, RZK_E_ARG, "xof: seeds must be 8-byte aligned and out 16-byte aligned");
  return run_xof(c, domain, 0, rows, (const uint64_t*)seeds, out, B);
}

int rzk_xof_uniform_batch(rzk_ctx* c, const uint8_t* seeds, uint32_t domain, uint32_t rows, int64_t* out, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !seeds || !out || rows == 0) return RZK_E_ARG;
  if (domain == RZK_XOF_DOMAIN_KEY) return fail(c, RZK_E_ARG, "xof: domain 0 is reserved for commitment keys (rzk_key_expand)");
  HIPCHK(c, hipSetDevice(c->device));   // the memset of HOST_WRAP comes before the first cfg_of
  std::vector<HostBuf> bufs = {IN(seeds, B * 32), OUT(out, polys(c, B * (size_t)rows))};
  HOST_WRAP(rzk_xof_uniform_batch_dev(c, DEV(0, const uint8_t*), domain, rows, DEV(1, int64_t*), B));
}

}  // extern "C"
