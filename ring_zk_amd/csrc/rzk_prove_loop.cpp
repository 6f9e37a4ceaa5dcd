// rzk_prove_loop.cpp — the zero-knowledge provers with their rejection loop inside the library (include/rzk.h "prover
// loop", DESIGN.md §21 for Open, §24 for Linear and Sum): x -> (commitment, masks, responses, ok, randomness, rounds) in one
// call, every tensor of the loop on the device.  The loop is fiat_shamir._zk_rounds restated over the *_dev entry points,
// which are all asynchronous on the context's stream, with the index bookkeeping of the pending proofs in small kernels
// (rzk_prove_loop_dev.hip):
//   round 0   the commitment randomness, y, the two coin draws, the full commit call, fs_challenge, the response with its
//             test on the dense batch, straight into the caller's slabs; then live = commit flag & ok_hash, done = live & accept
//   retry     idx = the pending proofs in ascending order (the order torch.nonzero gives: the position in the sub-batch is
//             the sampler's polynomial index), their count read back — the one host synchronisation of a round —, then on
//             the dense sub-batch: y and the coin draws under the next nonces, the randomness and the commitments gathered,
//             the masks alone (they are all of the commitment message that depends on y), the hash, the response with its
//             test, and the accepted masks and responses scattered to the caller's slabs
//   end       masks and responses of every proof that never passed are zeroed, ok = done; the secret parts of the
//             workspace are wiped
// ProveLoop is that skeleton, once; OpenLoop, LinearLoop and SumLoop say what a proof draws, calls and moves.  Open moves two
// slabs per direction with its own kernels (their names and launches are pinned by the tests); Linear and Sum move five
// through the field-list kernels.
// Open: one body for both slab widths, over the coefficient type C of the caller's slabs: it calls the typed
// forms of the entry points (rzk_ctx.h); the 32-bit ones convert inside themselves where the context has no native 32-bit
// kernels (ws32 is theirs, within the same call: the loop does not touch it).  Linear and Sum exist on 64-bit slabs only.
// The NULL tests, the alignment test of Open, the staging of the host forms and the row counts of the Linear / Sum fields
// come from the calls' slab lists (rzk_slabs.h, glue in rzk_ctx.h).
#include "rzk_ctx.h"
#include "rzk_prove_loop.h"

namespace {

// ws_prove of one call: every part starts on a 256-byte boundary
struct Workspace {
  size_t total = 0;
  size_t take(size_t bytes) {
    const size_t off = total;
    total += (bytes + 255) & ~size_t(255);
    return off;
  }
};

int pending_word(rzk_ctx* c) {
  if (c->h_pending) return RZK_OK;
  HIPCHK(c, hipHostMalloc((void**)&c->h_pending, sizeof(uint32_t), hipHostMallocDefault));
  return RZK_OK;
}

int compact(rzk_ctx* c, const uint8_t* live, const uint8_t* done, size_t B, uint32_t* idx, uint32_t* count) {
  return run_profiled(c, (uint64_t)B * 2, "pending compact kernel",
                      [&](const LaunchCfg& cfg) { return launch_pending_compact(cfg, live, done, B, idx, count); });
}

int named_fail(rzk_ctx* c, int code, const char* name, const char* what) { return fail(c, code, (std::string(name) + ": " + what).c_str()); }

// span: the nonces the call may consume (prove_nonce_span*); span_text: the same in words
int prove_args(rzk_ctx* c, const char* name, const uint8_t* nonce0, int gauss_kind, uint32_t max_rounds, uint64_t span,
               const char* span_text, size_t B) {
  if (gauss_kind != 0 && gauss_kind != 1)
    return named_fail(c, RZK_E_ARG, name, "gauss_kind must be 0 (Box-Muller) or 1 (exact discrete Gaussian)");
  if (max_rounds < 1 || max_rounds > 255) return named_fail(c, RZK_E_ARG, name, "max_rounds must lie in 1 .. 255");
  if (!nonce0) return named_fail(c, RZK_E_ARG, name, "NULL nonce0");
  if (!c->sampler_key_set) return named_fail(c, RZK_E_STATE, name, "no sampler key set (rzk_sampler_set_key)");
  uint8_t last[16];
  if (!nonce_add(nonce0, span, last)) return named_fail(c, RZK_E_ARG, name, span_text);
  if ((uint64_t)B >> 32) return named_fail(c, RZK_E_ARG, name, "B must stay below 2^32");
  return RZK_OK;
}

// The skeleton of the three loops.  A proof derives from it and says: its parts of the workspace, its draws, what it calls
// on the dense batch and on a sub-batch, which slabs it gathers, scatters and zeroes.
template <class C>
class ProveLoop {
 public:
  ProveLoop(rzk_ctx* ctx, const char* name_, const uint8_t* nonce0_, uint32_t stream_, int gauss_kind_, const uint8_t* aux32_,
            double lnM_, uint8_t* ok_, uint8_t* rounds_, size_t B_)
      : c(ctx), name(name_), nonce0(nonce0_), stream(stream_), gauss_kind(gauss_kind_), aux32(aux32_), lnM(lnM_), ok(ok_),
        rounds(rounds_), B(B_), N(ctx->N), poly(polys<C>(ctx, 1)) {}
  virtual ~ProveLoop() = default;

  // the caller has checked the arguments; rounds_run (host, may be NULL) receives the rounds that ran
  int run(uint32_t max_rounds, uint32_t* rounds_run) {
    HIPCHK(c, hipSetDevice(c->device));
    int rc = pending_word(c);
    if (rc != RZK_OK) return rc;
    // Reserved once, for the full batch, before round 0.  The arenas of the calls below (ws_fs, ws_reject, ws, ws_dkey, and
    // ws32 on the convert path) are sized by the batch of the call, which is largest in round 0: nothing grows in mid-loop.
    Workspace w;
    layout(w);
    const size_t o_d = w.take(B * poly), o_ca = w.take(B * poly), o_cb = w.take(B * poly), o_coin = w.take(B * sizeof(int64_t));
    const size_t o_accept = w.take(B), o_okc = w.take(B), o_okf = w.take(B), o_live = w.take(B), o_done = w.take(B);
    const size_t o_idx = w.take(B * sizeof(uint32_t)), o_count = w.take(sizeof(uint32_t));
    rc = arena_reserve(c, c->ws_prove, w.total);
    if (rc != RZK_OK) return rc;
    char* const base = (char*)c->ws_prove.p;
    bind(base);
    wd = (C*)(base + o_d), wca = (C*)(base + o_ca), wcb = (C*)(base + o_cb);
    coin = (int64_t*)(base + o_coin);
    accept = (uint8_t*)(base + o_accept), okc = (uint8_t*)(base + o_okc), okf = (uint8_t*)(base + o_okf);
    live = (uint8_t*)(base + o_live), done = (uint8_t*)(base + o_done);
    idx = (uint32_t*)(base + o_idx), d_count = (uint32_t*)(base + o_count);

    size_t retry_max = 0;   // the largest sub-batch: how much of the workspace's retry copies was written
    uint32_t ran = 0;
    auto loop = [&]() -> int {
      // ---- round 0: the dense batch, into the caller's slabs
      int st = draw_r();
      if (st == RZK_OK) st = draw(B);
      if (st == RZK_OK) st = first();
      if (st != RZK_OK) return st;
      ran = 1;
      // ---- retry rounds: the pending proofs as a dense sub-batch
      for (uint32_t rnd = 1; rnd < max_rounds; ++rnd) {
        st = compact(c, live, done, B, idx, d_count);
        if (st != RZK_OK) return st;
        // the host sizes the next launches by the count, and stops on 0: the one synchronisation of a round
        HIPCHK(c, hipMemcpyAsync(c->h_pending, d_count, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        const size_t nb = *c->h_pending;
        if (nb == 0) break;
        if (nb > B) return named_fail(c, RZK_E_HIP, name, "pending count exceeds the batch");
        if (nb > retry_max) retry_max = nb;
        st = draw(nb);
        if (st == RZK_OK) st = gather(nb);
        if (st == RZK_OK) st = again(nb);   // the commitments do not depend on y: a retry computes the masks alone
        if (st == RZK_OK) st = scatter(nb, (uint8_t)rnd);
        if (st != RZK_OK) return st;
        ++ran;
      }
      // ---- a rejected attempt never leaves: what is left of round 0 in the caller's masks and responses is overwritten
      return last();
    };
    rc = loop();
    // Rejected responses, and the y and coins behind them, are exactly what must not be released: the y, coin and retry parts
    // of the workspace are zeroed on the stream whichever way the loop ended (memory outside the arena is overwritten, not wiped)
    std::vector<hipError_t> wiped = {hipMemsetAsync(wca, 0, B * poly, c->stream), hipMemsetAsync(wcb, 0, B * poly, c->stream),
                                     hipMemsetAsync(coin, 0, B * sizeof(int64_t), c->stream)};
    wipe(retry_max, wiped);
    if (rounds_run) *rounds_run = ran;
    if (rc != RZK_OK) {   // a failed call releases no response: the last kernel may not have run
      zero_outputs();
      (void)hipMemsetAsync(ok, 0, B, c->stream);
      return rc;
    }
    for (const hipError_t e : wiped)
      if (e != hipSuccess) {
        c->err = std::string(name) + ": hipMemsetAsync: " + hipGetErrorString(e);
        return RZK_E_HIP;
      }
    return RZK_OK;
  }

 protected:
  virtual void layout(Workspace& w) = 0;            // its parts of ws_prove, for the full batch
  virtual void bind(char* base) = 0;                // ... as pointers, once the arena is reserved
  virtual int draw_r() = 0;                         // round 0: the commitment randomness, into the caller's slabs
  virtual int draw_y(size_t nb) = 0;                // y of a round on nb proofs, into the workspace
  virtual int first() = 0;                          // round 0: commit, hash, response with its test, the first kernel
  virtual int gather(size_t nb) = 0;                // the pending proofs' randomness and commitments as a dense sub-batch
  virtual int again(size_t nb) = 0;                 // masks, hash, response with its test on the sub-batch
  virtual int scatter(size_t nb, uint8_t rnd) = 0;  // the accepted masks and responses to the caller's slabs
  virtual int last() = 0;                           // zero what never passed, ok = done
  virtual void wipe(size_t retry_max, std::vector<hipError_t>& e) = 0;   // its secret parts of the workspace
  virtual void zero_outputs() = 0;                  // the caller's y-dependent outputs, after a failure

  const uint8_t* next_nonce() {
    (void)nonce_add(nonce0, used++, nonce);   // inside the span prove_args accepted
    return nonce;
  }
  // `count` polynomials at rzk_sigma(ctx), Box-Muller (0) or the exact discrete Gaussian (1), under the next nonce
  int gauss(C* out, size_t count) {
    const uint8_t* nc = next_nonce();
    if (gauss_kind == 0) return sample_gauss_keyed_dev(c, nc, stream, (double)c->sigma, out, count);
    const uint32_t sg = c->sigma > 0xffffffffull ? 0xffffffffu : (uint32_t)c->sigma;   // (out of range: the sampler says so)
    return sample_dgauss_keyed_dev(c, nc, stream, sg, out, count * N);
  }
  int uniform(uint64_t bound, C* out, size_t count) { return sample_uniform_keyed_dev(c, next_nonce(), stream, bound, out, count); }
  // y and the coins of a round on `nb` proofs, in the order of the Python provers' attempt()
  int draw(size_t nb) {
    int st = draw_y(nb);
    if (st == RZK_OK) st = uniform((uint64_t)kCoinHalf, wca, nb);
    if (st == RZK_OK) st = uniform((uint64_t)kCoinHalf, wcb, nb);
    if (st != RZK_OK) return st;
    return run_profiled(c, (uint64_t)nb * 24, "coin kernel",
                        [&](const LaunchCfg& cfg) { return launch_prove_coins(cfg, wca, wcb, N, coin, nb); });
  }

  rzk_ctx* const c;
  const char* const name;
  const uint8_t* const nonce0;
  const uint32_t stream;
  const int gauss_kind;
  const uint8_t* const aux32;
  const double lnM;
  uint8_t* const ok;
  uint8_t* const rounds;
  const size_t B;
  const uint32_t N;
  const size_t poly;   // bytes of one polynomial
  // the parts of the workspace every proof has
  C *wd = nullptr, *wca = nullptr, *wcb = nullptr;
  int64_t* coin = nullptr;
  uint8_t *accept = nullptr, *okc = nullptr, *okf = nullptr, *live = nullptr, *done = nullptr;
  uint32_t *idx = nullptr, *d_count = nullptr;

 private:
  uint64_t used = 0;   // nonces consumed
  uint8_t nonce[16];
};

// ---- Open ----------------------------------------------------------------------------------------------------------------
template <class C>
class OpenLoop final : public ProveLoop<C> {
  using L = ProveLoop<C>;
  using L::c; using L::B; using L::N; using L::poly; using L::wd; using L::coin; using L::accept; using L::okc; using L::okf;
  using L::live; using L::done; using L::idx; using L::lnM; using L::aux32; using L::ok; using L::rounds;

 public:
  OpenLoop(rzk_ctx* ctx, const C* x_, const uint8_t* nonce0, uint32_t stream, int gauss_kind, const uint8_t* aux32_, C* cm_, C* t_,
           C* z_, C* r_, uint8_t* ok_, uint8_t* rounds_, size_t B_)
      : L(ctx, "open prove zk", nonce0, stream, gauss_kind, aux32_, reject_lnm(11.0), ok_, rounds_, B_),   // one response vector: alpha = 11 (fiat_shamir.zk_lnm(1))
        x(x_), cm(cm_), t(t_), z(z_), r(r_), n(ctx->n), k(ctx->k), l(ctx->l) {}

 protected:
  void layout(Workspace& w) override {
    o_y = w.take(B * k * poly), o_t = w.take(B * n * poly), o_z = w.take(B * k * poly);
    o_rg = w.take(B * k * poly), o_cg = w.take(B * (n + l) * poly);
  }
  void bind(char* base) override {
    wy = (C*)(base + o_y), wt = (C*)(base + o_t), wz = (C*)(base + o_z), wrg = (C*)(base + o_rg), wcg = (C*)(base + o_cg);
  }
  int draw_r() override { return this->uniform(c->b, r, B * k); }
  int draw_y(size_t nb) override { return this->gauss(wy, nb * k); }
  int challenge(const C* cmsg, const C* tmsg, size_t nb) {
    const C* fields[2] = {cmsg, tmsg};
    return fs_challenge_dev(c, RZK_MSG_OPEN_COMMITMENT, 0, fields, aux32, wd, nullptr, okf, nb);
  }
  int first() override {
    int st = open_commit_dev<C>(c, x, r, wy, cm, t, okc, B);
    if (st == RZK_OK) st = challenge(cm, t, B);
    if (st == RZK_OK) st = open_response_reject_dev<C>(c, wy, r, wd, coin, kCoinR, lnM, z, accept, nullptr, B);
    if (st != RZK_OK) return st;
    return run_profiled(c, (uint64_t)B * 6, "prove first kernel",
                        [&](const LaunchCfg& cfg) { return launch_prove_first(cfg, okc, okf, accept, live, done, rounds, B); });
  }
  int gather(size_t nb) override {
    return run_profiled(c, (uint64_t)nb * (2 * k + 2 * (n + l)) * poly, "gather rows kernel", [&](const LaunchCfg& cfg) {
      return launch_gather_rows(cfg, r, wrg, k, cm, wcg, n + l, N, idx, (uint32_t)nb);
    });
  }
  int again(size_t nb) override {
    int st = matvec_dev<C>(c, RZK_KEY_A1, wy, nullptr, wt, nb);   // t = a1.y
    if (st == RZK_OK) st = challenge(wcg, wt, nb);                 // (its ok is not used: c and t are this library's)
    if (st == RZK_OK) st = open_response_reject_dev<C>(c, wy, wrg, wd, coin, kCoinR, lnM, wz, accept, nullptr, nb);
    return st;
  }
  int scatter(size_t nb, uint8_t rnd) override {
    return run_profiled(c, (uint64_t)nb * 2 * (n + k) * poly, "accept scatter kernel", [&](const LaunchCfg& cfg) {
      return launch_accept_scatter(cfg, wt, wz, t, z, n, k, N, accept, idx, (uint32_t)nb, rnd, rounds, done);
    });
  }
  int last() override {
    return run_profiled(c, (uint64_t)B * (n + k) * poly, "prove last kernel",
                        [&](const LaunchCfg& cfg) { return launch_prove_last(cfg, done, t, z, n, k, N, ok, B); });
  }
  void wipe(size_t retry_max, std::vector<hipError_t>& e) override {
    e.push_back(hipMemsetAsync(wy, 0, B * k * poly, c->stream));
    if (!retry_max) return;
    e.push_back(hipMemsetAsync(wt, 0, retry_max * n * poly, c->stream));
    e.push_back(hipMemsetAsync(wz, 0, retry_max * k * poly, c->stream));
  }
  void zero_outputs() override {
    (void)hipMemsetAsync(t, 0, B * n * poly, c->stream);
    (void)hipMemsetAsync(z, 0, B * k * poly, c->stream);
  }

 private:
  const C* const x;
  C *const cm, *const t, *const z, *const r;
  const uint32_t n, k, l;
  size_t o_y = 0, o_t = 0, o_z = 0, o_rg = 0, o_cg = 0;
  C *wy = nullptr, *wt = nullptr, *wz = nullptr, *wrg = nullptr, *wcg = nullptr;
};

template <class C>
int open_prove_zk_dev(rzk_ctx* c, const C* x, const uint8_t* nonce0, uint32_t stream, int gauss_kind, const uint8_t* aux32,
                      uint32_t max_rounds, C* cm, C* t, C* z, C* r, uint8_t* ok, uint8_t* rounds, uint32_t* rounds_run, size_t B) {
  if (!c) return RZK_E_ARG;
  if (rounds_run) *rounds_run = 0;
  const int rc = prove_args(c, "open prove zk", nonce0, gauss_kind, max_rounds, prove_nonce_span(max_rounds),
                            "nonce0 + 1 + 3 max_rounds leaves 128 bits", B);
  if (rc != RZK_OK) return rc;
  if (B == 0) return RZK_OK;
  if (slabs_null<kSlabsOpenProveZk>(x, cm, t, z, r, ok, rounds))
    return fail(c, RZK_E_ARG, "open prove zk: non-NULL x, c, t, z, r, ok, rounds expected");
  if (slabs_misaligned<kSlabsOpenProveZk>(x, cm, t, z, r, ok, rounds))
    return fail(c, RZK_E_ARG, "open prove zk: device slabs must be 16-byte aligned");
  if (!c->key_loaded) return fail(c, RZK_E_STATE, "commitment key not loaded");
  OpenLoop<C> loop(c, x, nonce0, stream, gauss_kind, aux32, cm, t, z, r, ok, rounds, B);
  return loop.run(max_rounds, rounds_run);
}

template <class C>
int open_prove_zk_host(rzk_ctx* c, const C* x, const uint8_t* nonce0, uint32_t stream, int gauss_kind, const uint8_t* aux32,
                       uint32_t max_rounds, C* cm, C* t, C* z, C* r, uint8_t* ok, uint8_t* rounds, uint32_t* rounds_run, size_t B) {
  if (!c) return RZK_E_ARG;
  if (rounds_run) *rounds_run = 0;
  const int rc = prove_args(c, "open prove zk", nonce0, gauss_kind, max_rounds, prove_nonce_span(max_rounds),
                            "nonce0 + 1 + 3 max_rounds leaves 128 bits", B);
  if (rc != RZK_OK) return rc;
  if (B == 0) return RZK_OK;
  if (slabs_null<kSlabsOpenProveZk>(x, cm, t, z, r, ok, rounds))
    return fail(c, RZK_E_ARG, "open prove zk: non-NULL x, c, t, z, r, ok, rounds expected");
  return host_run<kSlabsOpenProveZk>(c, {}, B, [&](const C* dx, C* dcm, C* dt, C* dz, C* dr, uint8_t* dok, uint8_t* drounds) {
    return open_prove_zk_dev<C>(c, dx, nonce0, stream, gauss_kind, aux32, max_rounds, dcm, dt, dz, dr, dok, drounds, rounds_run, B);
  }, x, cm, t, z, r, ok, rounds);
}

// ---- Linear and Sum: five slabs per direction, through the field-list kernels ----------------------------------------------
// What the two share beyond the skeleton: the slabs of a proof as fields of per-proof row counts, in one order for the
// caller's slabs and the workspace copies.
//   kept      r, r', c, c', g (rs, r', cs, c', gs): written in round 0, gathered for a retry
//   fresh     t, t', u, z, z' (ts, t', u, zs, z'): depend on y; a retry writes workspace copies, the accepted ones are scattered
class FieldLoop : public ProveLoop<int64_t> {
 public:
  static constexpr uint32_t kFields = 5;
  struct Slabs {
    int64_t* kept[kFields];    // the caller's (g / gs is an input: never written)
    int64_t* fresh[kFields];
    uint64_t kept_rows[kFields], fresh_rows[kFields];   // polynomials per proof
    const int64_t* x;                                   // and what is no field: the messages x (xs), read; ok and rounds, written
    uint8_t *ok, *rounds;
  };
  // false: an entry size or the batch times it leaves its type (field_quads)
  static bool sizes_ok(const Slabs& s, uint32_t N, size_t B) {
    uint32_t q;
    for (uint32_t f = 0; f < kFields; ++f)
      if (!field_quads(s.kept_rows[f], N, 8, B, &q) || !field_quads(s.fresh_rows[f], N, 8, B, &q)) return false;
    return true;
  }
  FieldLoop(rzk_ctx* ctx, const char* name_, const Slabs& s_, uint64_t y_rows_, uint64_t yp_rows_, uint8_t wanted_,
            const uint8_t* nonce0, uint32_t stream, int gauss_kind, const uint8_t* aux32_, double lnM_, uint8_t* ok_, uint8_t* rounds_,
            size_t B_)
      : ProveLoop<int64_t>(ctx, name_, nonce0, stream, gauss_kind, aux32_, lnM_, ok_, rounds_, B_), s(s_), y_rows(y_rows_),
        yp_rows(yp_rows_), wanted(wanted_) {}

 protected:
  void layout(Workspace& w) override {
    o_y = w.take(B * y_rows * poly), o_yp = w.take(B * yp_rows * poly);
    for (uint32_t f = 0; f < kFields; ++f) o_kept[f] = w.take(B * s.kept_rows[f] * poly), o_fresh[f] = w.take(B * s.fresh_rows[f] * poly);
  }
  void bind(char* base) override {
    wy = (int64_t*)(base + o_y), wyp = (int64_t*)(base + o_yp);
    for (uint32_t f = 0; f < kFields; ++f) wkept[f] = (int64_t*)(base + o_kept[f]), wfresh[f] = (int64_t*)(base + o_fresh[f]);
  }
  int draw_y(size_t nb) override {
    const int st = gauss(wy, nb * y_rows);
    return st != RZK_OK ? st : gauss(wyp, nb * yp_rows);
  }
  // the first kernel, after the proof's round-0 calls have written okc, okf and accept
  int first_flags() {
    return run_profiled(c, (uint64_t)B * 6, "prove first kernel", [&](const LaunchCfg& cfg) {
      return launch_prove_first_want(cfg, okc, wanted, okf, accept, live, done, rounds, B);
    });
  }
  FieldList list(int64_t* const* from, int64_t* const* to, const uint64_t* rows, uint64_t* bytes) const {
    FieldList fl{};
    fl.n = kFields;
    *bytes = 0;
    for (uint32_t f = 0; f < kFields; ++f) {
      fl.src[f] = from ? from[f] : nullptr, fl.dst[f] = to[f];
      (void)field_quads(rows[f], N, 8, B, &fl.quads[f]);   // sizes_ok held before the loop was made
      *bytes += (uint64_t)fl.quads[f] * 16;
    }
    return fl;
  }
  int gather(size_t nb) override {
    uint64_t bytes;
    const FieldList fl = list(s.kept, wkept, s.kept_rows, &bytes);
    return run_profiled(c, (uint64_t)nb * 2 * bytes, "gather fields kernel",
                        [&](const LaunchCfg& cfg) { return launch_gather_fields(cfg, fl, idx, (uint32_t)nb); });
  }
  int scatter(size_t nb, uint8_t rnd) override {
    uint64_t bytes;
    const FieldList fl = list(wfresh, s.fresh, s.fresh_rows, &bytes);
    return run_profiled(c, (uint64_t)nb * 2 * bytes, "accept scatter fields kernel", [&](const LaunchCfg& cfg) {
      return launch_accept_scatter_fields(cfg, fl, accept, idx, (uint32_t)nb, rnd, rounds, done);
    });
  }
  int last() override {
    uint64_t bytes;
    const FieldList fl = list(nullptr, s.fresh, s.fresh_rows, &bytes);
    return run_profiled(c, (uint64_t)B * bytes, "prove last fields kernel",
                        [&](const LaunchCfg& cfg) { return launch_prove_last_fields(cfg, fl, done, ok, B); });
  }
  void wipe(size_t retry_max, std::vector<hipError_t>& e) override {
    e.push_back(hipMemsetAsync(wy, 0, B * y_rows * poly, c->stream));
    e.push_back(hipMemsetAsync(wyp, 0, B * yp_rows * poly, c->stream));
    if (!retry_max) return;
    for (uint32_t f = 0; f < kFields; ++f) e.push_back(hipMemsetAsync(wfresh[f], 0, retry_max * s.fresh_rows[f] * poly, c->stream));
  }
  void zero_outputs() override {
    for (uint32_t f = 0; f < kFields; ++f) (void)hipMemsetAsync(s.fresh[f], 0, B * s.fresh_rows[f] * poly, c->stream);
  }

  const Slabs s;
  const uint64_t y_rows, yp_rows;   // polynomials of y (ys) and y' per proof
  const uint8_t wanted;             // the commit flag of a proof whose randomness passed
  int64_t *wy = nullptr, *wyp = nullptr, *wkept[kFields] = {}, *wfresh[kFields] = {};

 private:
  size_t o_y = 0, o_yp = 0, o_kept[kFields] = {}, o_fresh[kFields] = {};
};

// fields: kept = r, rp, c, cp, g; fresh = t, tp, u, z, zp
class LinearLoop final : public FieldLoop {
 public:
  LinearLoop(rzk_ctx* ctx, const Slabs& s_, const int64_t* x_, const uint8_t* nonce0, uint32_t stream, int gauss_kind, const uint8_t* aux32_,
             uint8_t* ok_, uint8_t* rounds_, size_t B_)
      : FieldLoop(ctx, "linear prove zk", s_, ctx->k, ctx->k, 3, nonce0, stream, gauss_kind, aux32_, reject_lnm(11.0 / std::sqrt((double)2)),
                  ok_, rounds_, B_),   // two response vectors (fiat_shamir.zk_lnm(2))
        x(x_) {}

 protected:
  int draw_r() override {
    const int st = uniform(c->b, s.kept[0], B * c->k);
    return st != RZK_OK ? st : uniform(c->b, s.kept[1], B * c->k);
  }
  // the commitment message of `nb` proofs from these slabs, in the field order of fiat_shamir.linear_prove
  int challenge(int64_t* const* kept, int64_t* const* fresh, size_t nb) {
    const int64_t* fields[6] = {kept[2], kept[3], kept[4], fresh[0], fresh[1], fresh[2]};   // c, cp, g, t, tp, u
    return fs_challenge_dev(c, RZK_MSG_LINEAR_COMMITMENT, 0, fields, aux32, wd, nullptr, okf, nb);
  }
  int respond(int64_t* const* kept, int64_t* const* fresh, size_t nb) {
    return rzk_linear_response_reject_batch_dev(c, wy, wyp, kept[0], kept[1], wd, coin, kCoinR, lnM, fresh[3], fresh[4], accept, nullptr, nb);
  }
  int first() override {
    int st = rzk_linear_commit_batch_dev(c, s.kept[4], x, s.kept[0], s.kept[1], wy, wyp, s.kept[2], s.kept[3], s.fresh[0], s.fresh[1],
                                         s.fresh[2], okc, B);
    if (st == RZK_OK) st = challenge(s.kept, s.fresh, B);
    if (st == RZK_OK) st = respond(s.kept, s.fresh, B);
    return st != RZK_OK ? st : first_flags();
  }
  int again(size_t nb) override {
    int st = rzk_linear_mask_batch_dev(c, wkept[4], wy, wyp, wfresh[0], wfresh[1], wfresh[2], nb);
    if (st == RZK_OK) st = challenge(wkept, wfresh, nb);   // (its ok is not used: a pending proof's hash was ok in round 0)
    if (st == RZK_OK) st = respond(wkept, wfresh, nb);
    return st;
  }

 private:
  const int64_t* const x;
};

// fields: kept = rs, rp, cs, cp, gs; fresh = ts, tp, u, zs, zp
class SumLoop final : public FieldLoop {
 public:
  SumLoop(rzk_ctx* ctx, uint32_t V_, const Slabs& s_, const int64_t* xs_, const uint8_t* nonce0, uint32_t stream, int gauss_kind,
          const uint8_t* aux32_, uint8_t* ok_, uint8_t* rounds_, size_t B_)
      : FieldLoop(ctx, "sum prove zk", s_, (uint64_t)V_ * ctx->k, ctx->k, 1, nonce0, stream, gauss_kind, aux32_,
                  reject_lnm(11.0 / std::sqrt((double)(V_ + 1))), ok_, rounds_, B_),   // V + 1 response vectors (fiat_shamir.zk_lnm(V + 1))
        V(V_), xs(xs_) {}

 protected:
  int draw_r() override {
    const int st = uniform(c->b, s.kept[0], B * V * c->k);   // every r_i of the batch under ONE nonce
    return st != RZK_OK ? st : uniform(c->b, s.kept[1], B * c->k);
  }
  int challenge(int64_t* const* kept, int64_t* const* fresh, size_t nb) {
    const int64_t* fields[6] = {kept[3], kept[2], kept[4], fresh[1], fresh[0], fresh[2]};   // cp, cs, gs, tp, ts, u
    return fs_challenge_dev(c, RZK_MSG_SUM_COMMITMENT, V, fields, aux32, wd, nullptr, okf, nb);
  }
  int respond(int64_t* const* kept, int64_t* const* fresh, size_t nb) {
    return rzk_sum_response_reject_batch_dev(c, V, wy, wyp, kept[0], kept[1], wd, coin, kCoinR, lnM, fresh[3], fresh[4], accept, nullptr, nb);
  }
  int first() override {
    int st = rzk_sum_commit_batch_dev(c, V, s.kept[4], xs, s.kept[0], s.kept[1], wy, wyp, s.kept[2], s.kept[3], s.fresh[0], s.fresh[1],
                                      s.fresh[2], okc, B);
    if (st == RZK_OK) st = challenge(s.kept, s.fresh, B);
    if (st == RZK_OK) st = respond(s.kept, s.fresh, B);
    return st != RZK_OK ? st : first_flags();
  }
  int again(size_t nb) override {
    int st = rzk_sum_mask_batch_dev(c, V, wkept[4], wy, wyp, wfresh[0], wfresh[1], wfresh[2], nb);
    if (st == RZK_OK) st = challenge(wkept, wfresh, nb);
    if (st == RZK_OK) st = respond(wkept, wfresh, nb);
    return st;
  }

 private:
  const uint32_t V;
  const int64_t* const xs;
};

const char* const kSpanLinSum = "nonce0 + 2 + 4 max_rounds leaves 128 bits";

// the checks both forms of a Linear / Sum call make before anything is staged or launched; *go = false: return rc at once
int field_loop_args(rzk_ctx* c, const char* name, const uint8_t* nonce0, int gauss_kind, uint32_t max_rounds, uint32_t* rounds_run,
                    const FieldLoop::Slabs& s, size_t B, bool* go) {
  *go = false;
  if (rounds_run) *rounds_run = 0;
  const int rc = prove_args(c, name, nonce0, gauss_kind, max_rounds, prove_nonce_span_lin_sum(max_rounds), kSpanLinSum, B);
  if (rc != RZK_OK || B == 0) return rc;
  bool null = !s.x || !s.ok || !s.rounds;
  for (uint32_t f = 0; f < FieldLoop::kFields; ++f) null = null || !s.kept[f] || !s.fresh[f];
  if (null) return named_fail(c, RZK_E_ARG, name, "non-NULL slabs, ok and rounds expected");
  if (!FieldLoop::sizes_ok(s, c->N, B)) return named_fail(c, RZK_E_ARG, name, "a proof's slab entry, or the batch of them, is too large");
  *go = true;
  return RZK_OK;
}
int field_loop_dev_args(rzk_ctx* c, const char* name, const FieldLoop::Slabs& s) {
  uintptr_t bits = (uintptr_t)s.x;
  for (uint32_t f = 0; f < FieldLoop::kFields; ++f) bits |= (uintptr_t)s.kept[f] | (uintptr_t)s.fresh[f];
  if (bits & 15u) return named_fail(c, RZK_E_ARG, name, "device slabs must be 16-byte aligned");
  if (!c->key_loaded) return fail(c, RZK_E_STATE, "commitment key not loaded");
  return RZK_OK;
}
// A Linear (S = kSlabsLinearProveZk) or Sum (kSlabsSumProveZk) call's pointers, in declaration order, as the loop's fields: the
// two lists declare g (gs), x (xs), then c, cp, t, tp, u, z, zp, r, rp (cs, ..., rs, rp), ok, rounds; the rows are the list's.
FieldLoop::Slabs field_slabs(const CallSlabs& S, const SlabDims& dm, const int64_t* g, const int64_t* x, int64_t* cm, int64_t* cpm,
                             int64_t* t, int64_t* tp, int64_t* u, int64_t* z, int64_t* zp, int64_t* r, int64_t* rp, uint8_t* ok,
                             uint8_t* rounds) {
  enum { G = 0, CM = 2, CPM, T, TP, U, Z, ZP, R, RP };   // positions in the list
  auto rows = [&](int at) { return slab_count(S.s[at].kind, dm); };
  return FieldLoop::Slabs{{r, rp, cm, cpm, const_cast<int64_t*>(g)}, {t, tp, u, z, zp}, {rows(R), rows(RP), rows(CM), rows(CPM), rows(G)},
                          {rows(T), rows(TP), rows(U), rows(Z), rows(ZP)}, x, ok, rounds};
}

int linear_prove_zk_slabs(rzk_ctx* c, const FieldLoop::Slabs& s, const uint8_t* nonce0, uint32_t stream, int gauss_kind, const uint8_t* aux32,
                          uint32_t max_rounds, uint32_t* rounds_run, size_t B) {
  const int rc = field_loop_dev_args(c, "linear prove zk", s);
  if (rc != RZK_OK) return rc;
  LinearLoop loop(c, s, s.x, nonce0, stream, gauss_kind, aux32, s.ok, s.rounds, B);
  return loop.run(max_rounds, rounds_run);
}
int sum_prove_zk_slabs(rzk_ctx* c, uint32_t V, const FieldLoop::Slabs& s, const uint8_t* nonce0, uint32_t stream, int gauss_kind,
                       const uint8_t* aux32, uint32_t max_rounds, uint32_t* rounds_run, size_t B) {
  const int rc = field_loop_dev_args(c, "sum prove zk", s);
  if (rc != RZK_OK) return rc;
  SumLoop loop(c, V, s, s.x, nonce0, stream, gauss_kind, aux32, s.ok, s.rounds, B);
  return loop.run(max_rounds, rounds_run);
}

constexpr uint32_t kSumMaxV = 1u << 20;   // rzk_sum_response_reject_batch's limit

}  // namespace

extern "C" {

int rzk_open_prove_zk_batch_dev(rzk_ctx* c, const int64_t* x, const uint8_t nonce0[16], uint32_t stream, int gauss_kind,
                                const uint8_t* aux32, uint32_t max_rounds, int64_t* cm, int64_t* t, int64_t* z, int64_t* r, uint8_t* ok,
                                uint8_t* rounds, uint32_t* rounds_run, size_t B) {
  return open_prove_zk_dev(c, x, nonce0, stream, gauss_kind, aux32, max_rounds, cm, t, z, r, ok, rounds, rounds_run, B);
}
int rzk_open_prove_zk32_batch_dev(rzk_ctx* c, const int32_t* x, const uint8_t nonce0[16], uint32_t stream, int gauss_kind,
                                  const uint8_t* aux32, uint32_t max_rounds, int32_t* cm, int32_t* t, int32_t* z, int32_t* r, uint8_t* ok,
                                  uint8_t* rounds, uint32_t* rounds_run, size_t B) {
  return open_prove_zk_dev(c, x, nonce0, stream, gauss_kind, aux32, max_rounds, cm, t, z, r, ok, rounds, rounds_run, B);
}
int rzk_open_prove_zk_batch(rzk_ctx* c, const int64_t* x, const uint8_t nonce0[16], uint32_t stream, int gauss_kind,
                            const uint8_t* aux32, uint32_t max_rounds, int64_t* cm, int64_t* t, int64_t* z, int64_t* r, uint8_t* ok,
                            uint8_t* rounds, uint32_t* rounds_run, size_t B) {
  return open_prove_zk_host(c, x, nonce0, stream, gauss_kind, aux32, max_rounds, cm, t, z, r, ok, rounds, rounds_run, B);
}
int rzk_open_prove_zk32_batch(rzk_ctx* c, const int32_t* x, const uint8_t nonce0[16], uint32_t stream, int gauss_kind,
                              const uint8_t* aux32, uint32_t max_rounds, int32_t* cm, int32_t* t, int32_t* z, int32_t* r, uint8_t* ok,
                              uint8_t* rounds, uint32_t* rounds_run, size_t B) {
  return open_prove_zk_host(c, x, nonce0, stream, gauss_kind, aux32, max_rounds, cm, t, z, r, ok, rounds, rounds_run, B);
}

int rzk_linear_prove_zk_batch_dev(rzk_ctx* c, const int64_t* g, const int64_t* x, const uint8_t nonce0[16], uint32_t stream,
                                  int gauss_kind, const uint8_t* aux32, uint32_t max_rounds, int64_t* cm, int64_t* cpm, int64_t* t,
                                  int64_t* tp, int64_t* u, int64_t* z, int64_t* zp, int64_t* r, int64_t* rp, uint8_t* ok, uint8_t* rounds,
                                  uint32_t* rounds_run, size_t B) {
  if (!c) return RZK_E_ARG;
  const FieldLoop::Slabs s = field_slabs(kSlabsLinearProveZk, dims_of(c), g, x, cm, cpm, t, tp, u, z, zp, r, rp, ok, rounds);
  bool go;
  const int rc = field_loop_args(c, "linear prove zk", nonce0, gauss_kind, max_rounds, rounds_run, s, B, &go);
  if (!go) return rc;
  return linear_prove_zk_slabs(c, s, nonce0, stream, gauss_kind, aux32, max_rounds, rounds_run, B);
}
int rzk_linear_prove_zk_batch(rzk_ctx* c, const int64_t* g, const int64_t* x, const uint8_t nonce0[16], uint32_t stream, int gauss_kind,
                              const uint8_t* aux32, uint32_t max_rounds, int64_t* cm, int64_t* cpm, int64_t* t, int64_t* tp, int64_t* u,
                              int64_t* z, int64_t* zp, int64_t* r, int64_t* rp, uint8_t* ok, uint8_t* rounds, uint32_t* rounds_run,
                              size_t B) {
  if (!c) return RZK_E_ARG;
  const FieldLoop::Slabs s = field_slabs(kSlabsLinearProveZk, dims_of(c), g, x, cm, cpm, t, tp, u, z, zp, r, rp, ok, rounds);
  bool go;
  const int rc = field_loop_args(c, "linear prove zk", nonce0, gauss_kind, max_rounds, rounds_run, s, B, &go);
  if (!go) return rc;
  return host_run<kSlabsLinearProveZk>(c, {}, B, [&](auto... d) {   // (the device pointers exist once the arena is staged: inside run)
    const FieldLoop::Slabs staged = field_slabs(kSlabsLinearProveZk, dims_of(c), d...);
    return linear_prove_zk_slabs(c, staged, nonce0, stream, gauss_kind, aux32, max_rounds, rounds_run, B);
  }, g, x, cm, cpm, t, tp, u, z, zp, r, rp, ok, rounds);
}

int rzk_sum_prove_zk_batch_dev(rzk_ctx* c, uint32_t V, const int64_t* gs, const int64_t* xs, const uint8_t nonce0[16], uint32_t stream,
                               int gauss_kind, const uint8_t* aux32, uint32_t max_rounds, int64_t* cs, int64_t* cpm, int64_t* ts,
                               int64_t* tp, int64_t* u, int64_t* zs, int64_t* zp, int64_t* rs, int64_t* rp, uint8_t* ok, uint8_t* rounds,
                               uint32_t* rounds_run, size_t B) {
  if (!c) return RZK_E_ARG;
  if (rounds_run) *rounds_run = 0;
  if (V == 0 || V > kSumMaxV) return fail(c, RZK_E_ARG, "sum prove zk: V must lie in 1 .. 2^20");
  const FieldLoop::Slabs s = field_slabs(kSlabsSumProveZk, dims_of(c, by_V(V)), gs, xs, cs, cpm, ts, tp, u, zs, zp, rs, rp, ok, rounds);
  bool go;
  const int rc = field_loop_args(c, "sum prove zk", nonce0, gauss_kind, max_rounds, rounds_run, s, B, &go);
  if (!go) return rc;
  return sum_prove_zk_slabs(c, V, s, nonce0, stream, gauss_kind, aux32, max_rounds, rounds_run, B);
}
int rzk_sum_prove_zk_batch(rzk_ctx* c, uint32_t V, const int64_t* gs, const int64_t* xs, const uint8_t nonce0[16], uint32_t stream,
                           int gauss_kind, const uint8_t* aux32, uint32_t max_rounds, int64_t* cs, int64_t* cpm, int64_t* ts, int64_t* tp,
                           int64_t* u, int64_t* zs, int64_t* zp, int64_t* rs, int64_t* rp, uint8_t* ok, uint8_t* rounds,
                           uint32_t* rounds_run, size_t B) {
  if (!c) return RZK_E_ARG;
  if (rounds_run) *rounds_run = 0;
  if (V == 0 || V > kSumMaxV) return fail(c, RZK_E_ARG, "sum prove zk: V must lie in 1 .. 2^20");
  const FieldLoop::Slabs s = field_slabs(kSlabsSumProveZk, dims_of(c, by_V(V)), gs, xs, cs, cpm, ts, tp, u, zs, zp, rs, rp, ok, rounds);
  bool go;
  const int rc = field_loop_args(c, "sum prove zk", nonce0, gauss_kind, max_rounds, rounds_run, s, B, &go);
  if (!go) return rc;
  return host_run<kSlabsSumProveZk>(c, by_V(V), B, [&](auto... d) {
    const FieldLoop::Slabs staged = field_slabs(kSlabsSumProveZk, dims_of(c, by_V(V)), d...);
    return sum_prove_zk_slabs(c, V, staged, nonce0, stream, gauss_kind, aux32, max_rounds, rounds_run, B);
  }, gs, xs, cs, cpm, ts, tp, u, zs, zp, rs, rp, ok, rounds);
}

// diagnostic: pending_compact_kernel on the caller's flags, so that its edges are tested without a prover around it
int rzk_debug_compact_dev(rzk_ctx* c, const uint8_t* live, const uint8_t* done, size_t B, uint32_t* idx, uint32_t* count) {
  if (!c || !count || (B && (!live || !done || !idx))) return RZK_E_ARG;
  if ((uint64_t)B >> 32) return fail(c, RZK_E_ARG, "compact: B must stay below 2^32");
  return compact(c, live, done, B, idx, count);
}

}  // extern "C"
