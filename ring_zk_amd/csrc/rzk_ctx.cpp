// rzk_ctx.cpp — the context of the C ABI (include/rzk.h): create / destroy and the environment knobs, stream and
// synchronising calls, trust mode, profiling and debug entry points, and the small helpers every family file uses.
// Compiled with hipcc together with the kernels into ring_zk_amd/librzk_hip.so.  There is no CPU fallback anywhere in
// the host code: every entry point launches HIP kernels on the context's device or returns an error status.
#include "rzk_ctx.h"

namespace rzk::api {

void wipe(void* p, size_t n) {
  volatile uint8_t* v = (volatile uint8_t*)p;
  for (size_t i = 0; i < n; ++i) v[i] = 0;
}

int fail(rzk_ctx* c, int code, const char* msg) {
  if (c) c->err = msg;
  return code;
}

LaunchCfg cfg_of(rzk_ctx* c) {
  (void)hipSetDevice(c->device);   // the calling thread may have another current device
  return LaunchCfg{(void*)c->stream, c->num_cus, c->pair_poly ? 1 : 0, c->unit_io ? 1 : 0, c->shift_bytes ? 1 : 0, c->tw_lds};
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

int check_launch(rzk_ctx* c, int lrc, const char* what) {
  if (lrc == 0) return RZK_OK;
  c->err = std::string(what) + ": " + (lrc > 0 ? hipGetErrorString((hipError_t)lrc) : "bad ring degree");
  return RZK_E_HIP;
}

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

}  // namespace rzk::api

namespace {

std::string g_create_err;   // last rzk_ctx_create failure (no context exists yet to hold it)

int create_fail(int code, const std::string& msg) {
  g_create_err = msg;
  return code;
}

uint64_t isqrt_u64(uint64_t x) {
  uint64_t r = (uint64_t)std::sqrt((long double)x);
  while ((unsigned __int128)r * r > x) --r;
  while ((unsigned __int128)(r + 1) * (r + 1) <= x) ++r;
  return r;
}

// The environment knobs (tuning and testing), read once by rzk_ctx_create in this order.  Bool: atoi(value) != 0; Flag:
// the same, stored as 0 / 1 in an int whose default means "automatic"; Int / Uint: atoi; Double: atof; Clamped: see
// read_knobs.  A value that does not parse as a number therefore reads as 0.
struct Knob {
  enum Kind { Bool, Flag, Int, Uint, Double, Clamped };
  const char* name;
  Kind kind;
  union {
    bool rzk_ctx::*b;
    int rzk_ctx::*i;
    uint32_t rzk_ctx::*u;
    double rzk_ctx::*d;
  };
  const char* what;
  constexpr Knob(const char* n, bool rzk_ctx::*f, const char* w) : name(n), kind(Bool), b(f), what(w) {}
  constexpr Knob(const char* n, Kind k, int rzk_ctx::*f, const char* w) : name(n), kind(k), i(f), what(w) {}
  constexpr Knob(const char* n, uint32_t rzk_ctx::*f, const char* w) : name(n), kind(Uint), u(f), what(w) {}
  constexpr Knob(const char* n, double rzk_ctx::*f, const char* w) : name(n), kind(Double), d(f), what(w) {}
};
const Knob kKnobs[] = {
    {"RZK_GRID_CUS", Knob::Clamped, &rzk_ctx::num_cus, "testing: CU count behind every grid cap and scratch size, in [1, the device's]"},
    {"RZK_SLOT_SHARE_MIN", &rzk_ctx::slot_share_min, "shared-operand path from this ratio of operand transforms to distinct operands"},
    {"RZK_ROW_GROUPS", &rzk_ctx::use_groups, "0: no row groups"},
    {"RZK_GROUP_MAX", Knob::Clamped, &rzk_ctx::group_max, "rows per group of row_group_kernel, in [1, the compiled accumulators]"},
    {"RZK_SHIFT", &rzk_ctx::use_shift, "0: challenge products as transforms, not rotations"},
    {"RZK_SHIFT_BYTES", &rzk_ctx::shift_bytes, "0: rotations of short operands as words, not packed bytes"},
    {"RZK_SUM_D", Knob::Flag, &rzk_ctx::sum_d, "Sum proof: force a2.(sum_i g_i v_i - v') on (1) or off (0); unset: by cost"},
    {"RZK_DKEY", Knob::Int, &rzk_ctx::use_dkey, "multiplier images: 0 never, 1 from kDkeyMinUses rows per multiplier on, 2 always"},
    {"RZK_LIN_E", &rzk_ctx::lin_e, "0: Linear verifier in the reference's grouping"},
    {"RZK_OIMG", &rzk_ctx::use_oimg, "0: Sum proof without operand images"},
    {"RZK_PRESET_IN_KERNEL", &rzk_ctx::preset_in_kernel, "0: verdict flags always preset by a fill launch"},
    {"RZK_PAIRS", &rzk_ctx::use_pairs, "0: unit_kernel without row pairs"},
    {"RZK_UPT", &rzk_ctx::units_per_task, "units per task of unit_kernel (0: automatic)"},
    {"RZK_VEC_ROWS", &rzk_ctx::vec_rows, "0: vector x vector programs on unit_kernel, not row_kernel"},
    {"RZK_PAIR_POLY", &rzk_ctx::pair_poly, "0: one wavefront per polynomial at N = 2048"},
    {"RZK_UNIT_IO", &rzk_ctx::unit_io, "0 / 1: force unit_kernel / unit_io_kernel for key-product programs (default: N = 512 only)"},
    {"RZK_BLOCK_MIN_LOGN", &rzk_ctx::block_min_logn, "row blocks from this log2 N on (12: never)"},
    {"RZK_ROT_LAST", &rzk_ctx::rot_last, "0: unit_kernel evaluates every row's rotation terms first, through its scratch line"},
    {"RZK_DOT2", &rzk_ctx::dot2, "0: unit_kernel reduces each of a two-product row's products on its own"},
    {"RZK_TW_LDS", Knob::Int, &rzk_ctx::tw_lds, "unit_kernel at N = 1024: 0 twiddles from the global tables, 1 phase 2 from an LDS image, 2 phases 2 and 3 (16-team workgroups)"},
    {"RZK_CRT2_SHORT", &rzk_ctx::crt2_short, "0: two-prime reconstruction with two reductions mod q (crt2_zq)"},
};

constexpr int kTwLdsDefault = 1;   // RZK_TW_LDS at N = 1024 (2 did not pass its A/B — commit gains, verify loses more)

// needs num_cus, group_max, unit_io and tw_lds at their defaults
void read_knobs(rzk_ctx* c) {
  for (const Knob& k : kKnobs) {
    const char* e = std::getenv(k.name);
    if (!e) continue;
    switch (k.kind) {
      case Knob::Bool: c->*k.b = std::atoi(e) != 0; break;
      case Knob::Flag: c->*k.i = std::atoi(e) != 0 ? 1 : 0; break;
      case Knob::Int: c->*k.i = std::atoi(e); break;
      case Knob::Uint: c->*k.u = (uint32_t)std::atoi(e); break;
      case Knob::Double: c->*k.d = std::atof(e); break;
      case Knob::Clamped:
        if (k.i == &rzk_ctx::num_cus) {   // never above the device's count
          const long v = std::strtol(e, nullptr, 10);
          c->num_cus = v < 1 ? 1 : (v < c->num_cus ? (int)v : c->num_cus);
        } else {   // group_max: ignored outside the compiled accumulators
          const int g = std::atoi(e);
          if (g >= 1 && g <= group_accumulators(c->logn)) c->group_max = g;
        }
        break;
    }
  }
}

}  // namespace

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
  // The knobs, over their defaults.  RZK_GRID_CUS: every grid cap and the scratch sized from it follow this CU count, so
  // that small batches make several grid-stride trips; read before the first allocation sized by num_cus (the row scratch)
  c->group_max = group_max_for((int)c->logn);
  c->unit_io = c->logn == 9;
  c->tw_lds = c->logn == 10 ? kTwLdsDefault : 0;
  read_knobs(c);
  c->tw_lds = c->tw_lds < 0 ? 0 : (c->tw_lds > 2 ? 2 : c->tw_lds);
  c->hT.diet = (c->rot_last ? DIET_ROT_LAST : 0u) | (c->crt2_short ? DIET_CRT2 : 0u);   // (RZK_DOT2 goes into the plans: plan_env)
  if ((de = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking)) != hipSuccess) {
    delete c;
    return create_fail(RZK_E_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(de));
  }
  c->stream = c->own_stream;

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
  void* const dev[] = {c->d_key_ntt,  c->d_key_l2, c->ws.p,   c->ws_slots.p,     c->ws_wire.p,       c->ws_fs.p,
                       c->ws_reject.p, c->ws_prove.p, c->ws_dkey.p, c->ws_oimg.p, c->stage.p, c->ws32.p,     c->dT,              c->d_tw,
                       c->d_row_scratch, c->d_block_scratch, c->d_group_scratch, c->d_key_mont, c->d_bad};
  for (void* p : dev)
    if (p) (void)hipFree(p);
  if (c->h_bad) (void)hipHostFree(c->h_bad);
  if (c->h_pending) (void)hipHostFree(c->h_pending);
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

// ---- instrumentation ---------------------------------------------------------------------------------------------
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

}  // extern "C"
