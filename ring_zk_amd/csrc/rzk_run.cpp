// rzk_run.cpp — how the host code runs device work: the cache of planned row programs (rzk_plan.h) and run_program, the
// fused norm predicate with its fallback (run_checked), the norm kernel, the images of a Linear / Sum call
// (prepare_dkey, prepare_oimg) and the profiling slots.
#include "rzk_ctx.h"

namespace rzk::api {

// Challenge products as signed rotations (shift-add) instead of transforms.  At N = 2048 only with two wavefronts
// per polynomial (16 outputs per thread): with one, a lane holds 32 outputs, the rotation kernels need > 200 VGPRs
// (one or two waves per SIMD) and measured slower than the transform path (round 2).
bool shift_ok(const rzk_ctx* c) { return c->use_shift && !c->small && (c->logn <= 10 || c->pair_poly); }
// The response rows fused with the rejection statistic (response_stat_kernel): where the rotation kernel
// runs with one wavefront per polynomial.  N = 2048 (two wavefronts), small rings and RZK_SHIFT=0 keep the chain.
bool response_stat_fused(const rzk_ctx* c) { return shift_ok(c) && c->logn <= 10; }

// ---- row programs: planned on the host (rzk_plan.h), uploaded once per (program, shape) --------------------------
namespace {

PlanEnv plan_env(const rzk_ctx* c) {
  return PlanEnv{c->n, c->k, c->l, c->logn, c->small, shift_ok(c), c->block_min_logn, c->use_groups, c->group_max,
                 c->use_pairs, c->slot_share_min, c->key_class.data(), c->key_entry.data(), c->dot2};
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

// routing of a 32-bit launch (slab32_native, rzk_slab32.h) from the plan's facts and the context's knobs
bool native32(const rzk_ctx* c, const DevProg& dp) {
  const Path path = path_of(dp, c->small, c->vec_rows);
  const Slab32Facts f = slab32_facts(dp, path == Path::Units, path == Path::Shift, c->n, shift_ok(c), c->shift_bytes);
  return slab32_native(f, c->logn, c->small, (c->logn >= 11 && c->pair_poly) ? 7 : 6);
}

}  // namespace

bool program_native32(rzk_ctx* c, int id, uint32_t var) {
  DevProg dp;
  if (get_program(c, id, var, dp) != RZK_OK) {
    c->err.clear();   // (the 64-bit call the caller falls back to reports it)
    return false;
  }
  return native32(c, dp);
}

void drop_programs(rzk_ctx* c) {
  for (auto& kv : c->progs) free_program(kv.second);
  c->progs.clear();
}

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

// `group` > 1: the batch is B*group (proof, summand) pairs; operands with outer != 0 and the flags are per proof
// stat != NULL (PG_RESPONSE on the rotation path only, response_stat_fused): the rows also leave their rejection partials
// (in either width: response_stat_kernel<., ., i32> for width 4).
// sticky: a non-canonical input coefficient fails the CALL (prover-side / Mat-level entry points); verifier-side
// programs pass false — there the offending proof's verdict flag is cleared and the call succeeds.
// preset_value != 0: every verdict flag (nflags of them) starts at that value — written by the launch itself when one
// team evaluates all rows of a batch entry (no 5-us fill launch in front of a 75-us kernel), by a fill launch otherwise.
// specs: the list run_program<C> (rzk_ctx.h) lowered; its width is sizeof(C).
int run_program_lowered(rzk_ctx* c, int id, uint32_t var, const OpList& specs, uint8_t* flags, uint32_t group, uint64_t batch,
                        uint64_t norm_limit, bool sticky, uint8_t preset_value, uint64_t nflags, const ResponseStat* stat) {
  const uint32_t width = specs.width;
  DevProg dp;
  int rc = get_program(c, id, var, dp);
  if (rc != RZK_OK) return rc;
  if (width != 8 && (width != 4 || !native32(c, dp))) return fail(c, RZK_E_STATE, "no 32-bit kernels for this program");
  if (specs.n > (size_t)kMaxOperands) return fail(c, RZK_E_ARG, "too many operands");
  // units of one batch entry per task: all of them (one team per entry: equal-cost tasks, no tail) once the batch alone
  // fills the chip's wave slots; one unit per task below that
  uint32_t upt = batch >= (uint64_t)c->num_cus * 16 ? dp.nunits : 1;
  if (c->units_per_task) upt = c->units_per_task;   // RZK_UPT (tuning)
  const Path path = path_of(dp, c->small, c->vec_rows);
  if (stat && (id != PG_RESPONSE || path != Path::Shift || !response_stat_fused(c))) return fail(c, RZK_E_STATE, "fused response rows need the one-wavefront rotation kernel");
  const bool preset_in_kernel = preset_value && flags && c->preset_in_kernel && path == Path::Units && upt >= dp.nunits && dp.nunits > 0 &&
                                (group ? group : 1) == 1 && nflags == batch;
  if (preset_value && flags && !preset_in_kernel) {
    rc = check_launch(c, launch_fill_u8(cfg_of(c), flags, preset_value, nflags), "flag preset");
    if (rc != RZK_OK) return rc;
  }
  // the operand images of the call in progress, if any (all zero otherwise): this launch stores (producer op) and / or reads them
  Operands ops = c->oimg_state;
  ops.oimg_op = ops.oimg ? c->oimg_producer_op : 0xffu;
  for (size_t i = 0; i < specs.n; ++i) {
    ops.base[i] = const_cast<int64_t*>(specs.base[i]);
    ops.stride[i] = specs.stride[i];
    ops.outer[i] = specs.outer[i] ? 1 : 0;
  }
  ops.group = group ? group : 1;
  ops.pad = dp.two_bit ? 1 : 0;
  ops.norm_limit = norm_limit;
  ops.bad = sticky ? c->d_bad : nullptr;
  ops.trusted = c->trusted ? 1u : 0u;
  ops.preset = preset_in_kernel ? preset_value : 0u;
  if (dp.has_dkey) {
    if (!c->dkey_img || c->small) return fail(c, RZK_E_STATE, "multiplier images not prepared");
    ops.dkey_img = c->dkey_img;
    ops.dkey_l2 = c->dkey_l2;
    ops.dkey_n = c->dkey_n;
  }
  uint64_t bytes = 0;   // what the launch has to move at least: its operands in, its results out
  for (size_t i = 0; i < specs.n; ++i)
    bytes += (uint64_t)dp.polys_in[i] * (specs.outer[i] ? batch / (group ? group : 1) : batch);
  bytes = (bytes + (uint64_t)dp.polys_out * batch) * (uint64_t)width * c->N;
  LaunchCfg cfg;
  rc = prof_begin(c, bytes, cfg);
  if (rc != RZK_OK) return rc;
  const int logn = (int)c->logn;
  RowArgs a{dp.d, dp.d_wp, c->d_key_ntt, c->d_key_l2, c->dT, c->d_tw, c->d_row_scratch, flags};   // (scratch: Blocks and Groups have their own)
  int lrc = 0;
  switch (path) {
    case Path::Small:
      lrc = launch_row_program_small(c->N, cfg, dp.d, dp.nrows, ops, c->d_key_mont, c->dT, c->r2q, flags, batch);
      break;
    case Path::Shift:
      lrc = stat ? (width == 4 ? launch_response_stat32(logn, cfg, a, ops, dp.nrows, batch, *stat)
                               : launch_response_stat(logn, cfg, a, ops, dp.nrows, batch, *stat))
            : width == 4 ? launch_shift_rows32(logn, cfg, a, ops, dp.nrows, batch)
                         : launch_shift_rows(logn, cfg, a, ops, dp.nrows, batch);
      break;
    case Path::Blocks:
      if (!c->d_block_scratch)
        HIPCHK(c, hipMalloc((void**)&c->d_block_scratch, block_scratch_words(logn, c->num_cus) * sizeof(uint32_t)));
      a.scratch = c->d_block_scratch;
      lrc = launch_row_blocks(logn, cfg, a, ops, dp.d_blocks, dp.nblocks, batch);
      break;
    case Path::Groups:
      if (!c->d_group_scratch)
        HIPCHK(c, hipMalloc((void**)&c->d_group_scratch, group_scratch_words(logn, c->num_cus) * sizeof(uint32_t)));
      a.scratch = c->d_group_scratch;
      lrc = launch_row_groups(logn, cfg, a, ops, dp.ngroups, batch);
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
        for (size_t i = 0; i < specs.n; ++i) {
          if (!o2.base[i]) continue;
          const uint64_t first = o2.outer[i] ? b0 / grp : b0;
          o2.base[i] += first * o2.stride[i] * c->N;
        }
        a.flags = flags ? flags + b0 / grp : nullptr;
        lrc = launch_row_program_slots(logn, cfg, a, o2, dp.d_slots, dp.nslots, SlotStore{d_ws, d_norms, dp.np_store}, nb);
      }
      break;
    }
    case Path::Rows:
      lrc = width == 4 ? launch_rows32(logn, cfg, a, ops, dp.nrows, dp.has_shift, batch, dp.has_dd)
                       : launch_rows(logn, cfg, a, ops, dp.nrows, dp.has_shift, batch, dp.has_dd);
      break;
    case Path::Units: {
      const UnitShape u{dp.nunits, upt, 2 * dp.work, dp.has_vec, dp.has_shift};
      lrc = width == 4 ? launch_units32(logn, cfg, a, ops, u, batch) : launch_units(logn, cfg, a, ops, u, batch);
      break;
    }
  }
  if (lrc == -2) return fail(c, RZK_E_UNSUPPORTED, "batch * rows must stay below 2^32");
  rc = check_launch(c, lrc, "row kernel launch");
  return rc != RZK_OK ? rc : prof_end(c);
}

namespace {

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
int run_program_checked(rzk_ctx* c, int id, uint32_t var, const OpList& specs, uint8_t* flags, uint32_t group, uint64_t batch,
                        uint64_t nflags, uint64_t bound, bool preset, bool sticky) {
  const uint64_t lim = fused_limit(c, bound);
  if (!lim || !flags) return RZK_E_UNSUPPORTED;
  DevProg dp;
  int rc = get_program(c, id, var | 1, dp);
  if (rc != RZK_OK) return rc;
  // two-bit verdicts are cleared with word atomics: the flag array must be made of whole aligned words
  if (dp.two_bit && ((reinterpret_cast<uintptr_t>(flags) & 3u) || (nflags & 3u))) return RZK_E_UNSUPPORTED;
  const uint8_t all_ok = dp.two_bit ? 3 : 1;
  return run_program_lowered(c, id, var | 1, specs, flags, group, batch, lim, sticky, preset ? all_ok : (uint8_t)0, nflags, nullptr);
}

}  // namespace

bool checked_fuses(rzk_ctx* c, int id, uint32_t var, uint64_t bound) {
  if (!fused_limit(c, bound)) return false;
  DevProg dp;
  if (get_program(c, id, var | 1, dp) != RZK_OK) {
    c->err.clear();
    return false;
  }
  return !dp.two_bit;   // (two-bit verdicts depend on the flag array's alignment: not asked for here)
}

bool checked_native32(rzk_ctx* c, int id, uint32_t var, uint64_t bound, bool has_flags) {
  if (!program_native32(c, id, var)) return false;
  if (!has_flags) return true;
  if (!norm_native32(c)) return false;
  if (!fused_limit(c, bound)) return true;   // never fuses
  DevProg dp;
  if (get_program(c, id, var | 1, dp) != RZK_OK) {   // no fused form: the fallback runs
    c->err.clear();
    return true;
  }
  return native32(c, dp);
}

// The stand-alone norm kernel exists for 32-bit slabs where the native row kernels do (norm_kernel_i32, rzk_slab32_dev.hip)
bool norm_native32(const rzk_ctx* c) { return !c->small && (c->logn == 9 || c->logn == 10); }

// A program whose rows decide a norm predicate of `bound` into `flags` (nflags of them, one per proof): the checked
// variant with the predicate fused into the rows that load the vector anyway; where that cannot run (small rings, a
// bound past 2^24, no flags, a shape or flag array the fused form does not cover) the norm kernels of `norms`, in their
// order, and then the plain program, which clears the verdicts of proofs with non-canonical inputs.  Without flags
// (a prover that does not ask) the norms are skipped.  preset: the fused launch initialises the flags; the first of
// `norms` does so in the fallback (mode 0), or the caller has (mode 1 throughout).
int run_checked_lowered(rzk_ctx* c, int id, uint32_t var, const OpList& specs, uint8_t* flags, uint32_t group, uint64_t batch,
                        uint64_t nflags, uint64_t bound, bool preset, bool sticky, std::initializer_list<NormSpec> norms) {
  int rc = run_program_checked(c, id, var, specs, flags, group, batch, nflags, bound, preset, sticky);
  if (rc != RZK_E_UNSUPPORTED) return rc;
  // (width 4: norm_kernel_i32, on the contexts whose 32-bit calls run natively)
  for (const NormSpec& n : norms) {
    if (!flags) break;
    rc = specs.width == 4 ? run_norm(c, static_cast<const int32_t*>(n.v), n.rows, bound, flags, nflags, n.mode, n.shift, sticky)
                          : run_norm(c, static_cast<const int64_t*>(n.v), n.rows, bound, flags, nflags, n.mode, n.shift, sticky);
    if (rc != RZK_OK) return rc;
  }
  return run_program_lowered(c, id, var, specs, flags, group, batch, 0, sticky, 0, 0, nullptr);
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
  // (bytes: the multipliers it reads; the images are derived data)
  rc = run_profiled(c, count * 8ull * c->N, "multiplier images", [&](const LaunchCfg& cfg) {
    return launch_dkey_transform((int)c->logn, cfg, g, count, per_entry, img, l2, c->dT, c->d_tw, flags,
                                 sticky ? c->d_bad : nullptr, false, c->trusted);
  });
  if (rc != RZK_OK) return rc;
  c->dkey_img = img;
  c->dkey_l2 = l2;
  c->dkey_n = per_entry;
  return RZK_OK;
}

// Operand images of a Sum call (Operands::oimg): room for the transforms of the columns a2 uses of every (proof, summand)
// vector, all marked "nothing stored yet".  Leaves c->oimg_state.oimg NULL when the path is off or nothing would be saved.
int prepare_oimg(rzk_ctx* c, uint64_t B, uint32_t V, uint32_t uses) {
  c->oimg_state = Operands{};
  c->oimg_producer_op = 0xffu;
  if (!c->use_oimg || !dkey_wanted(c, uses) || c->k > 32u || !sum_uses_d(c, V)) return RZK_OK;
  const uint32_t k = c->k;
  const PlanEnv env = plan_env(c);
  Operands st{};   // (c->oimg_state stays all zero unless the images are in place: run_program starts from it)
  uint32_t ncols = 0;
  for (uint32_t col = 0; col < 32u; ++col) st.oimg_col[col] = -1;
  for (uint32_t col = 0; col < k; ++col)
    if (a2_uses_column(env, col)) st.oimg_col[col] = (int8_t)ncols++;
  if (ncols == 0) return RZK_OK;
  const uint64_t slots = B * V * ncols;
  const size_t img_bytes = ((size_t)slots * kKeyImages * c->N * sizeof(uint32_t) + 255) & ~(size_t)255;
  const size_t l2_bytes = ((size_t)slots * sizeof(double) + 255) & ~(size_t)255;
  int rc = arena_reserve(c, c->ws_oimg, img_bytes + l2_bytes + slots);
  if (rc != RZK_OK) return rc;
  char* base = (char*)c->ws_oimg.p;
  HIPCHK(c, hipMemsetAsync(base + img_bytes + l2_bytes, 0, slots, c->stream));
  st.oimg = (uint32_t*)base;
  st.oimg_l2 = (double*)(base + img_bytes);
  st.oimg_np = (uint8_t*)(base + img_bytes + l2_bytes);
  st.oimg_n = ncols;
  st.oimg_group = V;
  st.oimg_k = k;
  c->oimg_state = st;
  return RZK_OK;
}

template <class C>
int run_norm(rzk_ctx* c, const C* v, uint32_t rows, uint64_t bound, uint8_t* ok, uint64_t B, int mode, int shift, bool sticky) {
  // canonical coefficients are below 2^31 in magnitude, so sum c^2 < 2^73: every bound from 2^37 on holds for
  // all inputs; clamping there keeps (bound+1)^2 inside 128 bits for any u64 bound (sigma grows with b)
  if (bound > (1ull << 40)) bound = 1ull << 40;
  uint64_t hi, lo;
  norm_limit(bound, hi, lo);
  uint32_t* bad = sticky ? c->d_bad : nullptr;
  const uint32_t qh = c->hT.crt.qhalf;
  if constexpr (sizeof(C) == 4) {   // in a profiling slot of its own: the tests tell the 32-bit launch by its name
    if (c->small) return fail(c, RZK_E_STATE, "no 32-bit norm kernel for small rings");
    return run_profiled(c, (uint64_t)B * rows * c->N * sizeof(C), "norm kernel", [&](const LaunchCfg& cfg) {
      return launch_norm32((int)c->logn, cfg, v, rows, hi, lo, ok, B, mode, shift, qh, bad);
    });
  } else {
    if (c->small)
      return check_launch(c, launch_norm_small(c->N, cfg_of(c), v, rows, hi, lo, ok, B, mode, shift, qh, bad), "norm kernel");
    return check_launch(c, launch_norm((int)c->logn, cfg_of(c), v, rows, hi, lo, ok, B, mode, shift, qh, bad), "norm kernel");
  }
}
RZK_BOTH_WIDTHS(run_norm)

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

}  // namespace rzk::api
