// rzk_prove_loop.cpp — the zero-knowledge Open prover with its rejection loop inside the library (include/rzk.h "prover
// loop"): x -> (c, t, z, ok, r, rounds) in one call, every tensor of the loop on the device.  The loop is
// fiat_shamir._zk_rounds / open_prove_zk[32] restated over the *_dev entry points, which are all asynchronous on the
// context's stream, with the index bookkeeping of the pending proofs in four small kernels (rzk_prove_loop_dev.hip):
//   round 0   r, y, the two coin draws, open_commit, fs_challenge, open_response_reject on the dense batch, straight into
//             the caller's c, t, z; then live = ok_commit & ok_hash, done = live & accept
//   retry     idx = the pending proofs in ascending order (the order torch.nonzero gives: the position in the sub-batch is
//             the sampler's polynomial index), their count read back — the one host synchronisation of a round —, then on
//             the dense sub-batch: y and the coin draws under the next three nonces, r and c gathered, t = a1.y, the hash,
//             the response with its test, and the accepted (t, z) scattered to the caller's slabs
//   end       t, z of every proof that never passed are zeroed, ok = done; the secret parts of the workspace are wiped
// One body for both slab widths, over the coefficient type C of the caller's slabs: it calls the typed
// forms of the entry points (rzk_ctx.h); the 32-bit ones convert inside themselves where the context has no native 32-bit
// kernels (ws32 is theirs, within the same call: the loop does not touch it).
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

int prove_args(rzk_ctx* c, const uint8_t* nonce0, int gauss_kind, uint32_t max_rounds, size_t B) {
  if (gauss_kind != 0 && gauss_kind != 1)
    return fail(c, RZK_E_ARG, "open prove zk: gauss_kind must be 0 (Box-Muller) or 1 (exact discrete Gaussian)");
  if (max_rounds < 1 || max_rounds > 255) return fail(c, RZK_E_ARG, "open prove zk: max_rounds must lie in 1 .. 255");
  if (!nonce0) return fail(c, RZK_E_ARG, "open prove zk: NULL nonce0");
  if (!c->sampler_key_set) return fail(c, RZK_E_STATE, "open prove zk: no sampler key set (rzk_sampler_set_key)");
  uint8_t last[16];
  if (!nonce_add(nonce0, prove_nonce_span(max_rounds), last))
    return fail(c, RZK_E_ARG, "open prove zk: nonce0 + 1 + 3 max_rounds leaves 128 bits");
  if ((uint64_t)B >> 32) return fail(c, RZK_E_ARG, "open prove zk: B must stay below 2^32");
  return RZK_OK;
}

template <class C>
int open_prove_zk_dev(rzk_ctx* c, const C* x, const uint8_t* nonce0, uint32_t stream, int gauss_kind, const uint8_t* aux32,
                      uint32_t max_rounds, C* cm, C* t, C* z, C* r, uint8_t* ok, uint8_t* rounds, uint32_t* rounds_run, size_t B) {
  if (!c) return RZK_E_ARG;
  if (rounds_run) *rounds_run = 0;
  int rc = prove_args(c, nonce0, gauss_kind, max_rounds, B);
  if (rc != RZK_OK) return rc;
  if (B == 0) return RZK_OK;
  if (!x || !cm || !t || !z || !r || !ok || !rounds) return fail(c, RZK_E_ARG, "open prove zk: non-NULL x, c, t, z, r, ok, rounds expected");
  if (misaligned({x, cm, t, z, r})) return fail(c, RZK_E_ARG, "open prove zk: device slabs must be 16-byte aligned");
  if (!c->key_loaded) return fail(c, RZK_E_STATE, "commitment key not loaded");
  HIPCHK(c, hipSetDevice(c->device));
  rc = pending_word(c);
  if (rc != RZK_OK) return rc;

  const uint32_t N = c->N, n = c->n, k = c->k, l = c->l;
  const size_t poly = polys<C>(c, 1);
  // Reserved once, for the full batch, before round 0.  The arenas of the calls below (ws_fs, ws_reject, ws, and ws32 on
  // the convert path) are sized by the batch of the call, which is largest in round 0: nothing grows in mid-loop.
  Workspace w;
  const size_t o_y = w.take(B * k * poly), o_t = w.take(B * n * poly), o_z = w.take(B * k * poly), o_d = w.take(B * poly);
  const size_t o_rg = w.take(B * k * poly), o_cg = w.take(B * (n + l) * poly);
  const size_t o_ca = w.take(B * poly), o_cb = w.take(B * poly), o_coin = w.take(B * sizeof(int64_t));
  const size_t o_accept = w.take(B), o_okc = w.take(B), o_okf = w.take(B), o_live = w.take(B), o_done = w.take(B);
  const size_t o_idx = w.take(B * sizeof(uint32_t)), o_count = w.take(sizeof(uint32_t));
  rc = arena_reserve(c, c->ws_prove, w.total);
  if (rc != RZK_OK) return rc;
  char* const base = (char*)c->ws_prove.p;
  auto slab = [&](size_t off) { return (C*)(base + off); };
  C *const wy = slab(o_y), *const wt = slab(o_t), *const wz = slab(o_z), *const wd = slab(o_d);
  C *const wrg = slab(o_rg), *const wcg = slab(o_cg), *const wca = slab(o_ca), *const wcb = slab(o_cb);
  int64_t* const coin = (int64_t*)(base + o_coin);
  uint8_t *const accept = (uint8_t*)(base + o_accept), *const okc = (uint8_t*)(base + o_okc), *const okf = (uint8_t*)(base + o_okf);
  uint8_t *const live = (uint8_t*)(base + o_live), *const done = (uint8_t*)(base + o_done);
  uint32_t *const idx = (uint32_t*)(base + o_idx), *const d_count = (uint32_t*)(base + o_count);

  const double lnM = reject_lnm(11.0);   // one response vector: alpha = 11 (fiat_shamir.zk_lnm(1))
  uint64_t used = 0;                      // nonces consumed
  uint8_t nonce[16];
  auto next_nonce = [&]() -> const uint8_t* {
    (void)nonce_add(nonce0, used++, nonce);   // inside the span prove_args accepted
    return nonce;
  };
  // y: `count` polynomials at rzk_sigma(ctx), Box-Muller (0) or the exact discrete Gaussian (1)
  auto gauss = [&](const uint8_t* nc, size_t count) -> int {
    if (gauss_kind == 0) return sample_gauss_keyed_dev(c, nc, stream, (double)c->sigma, wy, count);
    const uint32_t sg = c->sigma > 0xffffffffull ? 0xffffffffu : (uint32_t)c->sigma;   // (out of range: the sampler says so)
    return sample_dgauss_keyed_dev(c, nc, stream, sg, wy, count * N);
  };
  auto challenge = [&](const C* cmsg, const C* tmsg, size_t nb) -> int {
    const C* fields[2] = {cmsg, tmsg};
    return fs_challenge_dev(c, RZK_MSG_OPEN_COMMITMENT, 0, fields, aux32, wd, nullptr, okf, nb);
  };
  // y and the coins of a round on `nb` proofs: three nonces, in the order of open_prove_zk's attempt()
  auto draw = [&](size_t nb) -> int {
    int st = gauss(next_nonce(), nb * k);
    if (st == RZK_OK) st = sample_uniform_keyed_dev(c, next_nonce(), stream, (uint64_t)kCoinHalf, wca, nb);
    if (st == RZK_OK) st = sample_uniform_keyed_dev(c, next_nonce(), stream, (uint64_t)kCoinHalf, wcb, nb);
    if (st != RZK_OK) return st;
    return run_profiled(c, (uint64_t)nb * 24, "coin kernel",
                        [&](const LaunchCfg& cfg) { return launch_prove_coins(cfg, wca, wcb, N, coin, nb); });
  };

  size_t retry_max = 0;   // the largest sub-batch: how much of the workspace's t and z was written
  uint32_t ran = 0;
  auto loop = [&]() -> int {
    // ---- round 0: the dense batch, into the caller's slabs
    int st = sample_uniform_keyed_dev(c, next_nonce(), stream, c->b, r, B * k);
    if (st == RZK_OK) st = draw(B);
    if (st == RZK_OK) st = open_commit_dev<C>(c, x, r, wy, cm, t, okc, B);
    if (st == RZK_OK) st = challenge(cm, t, B);
    if (st == RZK_OK) st = open_response_reject_dev<C>(c, wy, r, wd, coin, kCoinR, lnM, z, accept, nullptr, B);
    if (st == RZK_OK)
      st = run_profiled(c, (uint64_t)B * 6, "prove first kernel",
                        [&](const LaunchCfg& cfg) { return launch_prove_first(cfg, okc, okf, accept, live, done, rounds, B); });
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
      if (nb > B) return fail(c, RZK_E_HIP, "open prove zk: pending count exceeds the batch");
      if (nb > retry_max) retry_max = nb;
      st = draw(nb);
      if (st == RZK_OK)
        st = run_profiled(c, (uint64_t)nb * (2 * k + 2 * (n + l)) * poly, "gather rows kernel", [&](const LaunchCfg& cfg) {
          return launch_gather_rows(cfg, r, wrg, k, cm, wcg, n + l, N, idx, (uint32_t)nb);
        });
      // c = commit(x; r) does not depend on y: a retry computes t = a1.y alone
      if (st == RZK_OK) st = matvec_dev<C>(c, RZK_KEY_A1, wy, nullptr, wt, nb);
      if (st == RZK_OK) st = challenge(wcg, wt, nb);   // (its ok is not used: c and t are this library's)
      if (st == RZK_OK) st = open_response_reject_dev<C>(c, wy, wrg, wd, coin, kCoinR, lnM, wz, accept, nullptr, nb);
      if (st == RZK_OK)
        st = run_profiled(c, (uint64_t)nb * 2 * (n + k) * poly, "accept scatter kernel", [&](const LaunchCfg& cfg) {
          return launch_accept_scatter(cfg, wt, wz, t, z, n, k, N, accept, idx, (uint32_t)nb, (uint8_t)rnd, rounds, done);
        });
      if (st != RZK_OK) return st;
      ++ran;
    }
    // ---- a rejected attempt never leaves: what is left of round 0 in the caller's t and z is overwritten
    return run_profiled(c, (uint64_t)B * (n + k) * poly, "prove last kernel",
                        [&](const LaunchCfg& cfg) { return launch_prove_last(cfg, done, t, z, n, k, N, ok, B); });
  };
  rc = loop();
  // Rejected responses, and the y and coins behind them, are exactly what must not be released: the y, t, z and coin parts of
  // the workspace are zeroed on the stream whichever way the loop ended (memory outside the arena is overwritten, not wiped)
  const hipError_t wiped[] = {hipMemsetAsync(wy, 0, B * k * poly, c->stream),
                              hipMemsetAsync(wca, 0, B * poly, c->stream),
                              hipMemsetAsync(wcb, 0, B * poly, c->stream),
                              hipMemsetAsync(coin, 0, B * sizeof(int64_t), c->stream),
                              retry_max ? hipMemsetAsync(wt, 0, retry_max * n * poly, c->stream) : hipSuccess,
                              retry_max ? hipMemsetAsync(wz, 0, retry_max * k * poly, c->stream) : hipSuccess};
  if (rounds_run) *rounds_run = ran;
  if (rc != RZK_OK) {   // a failed call releases no response: prove_last_kernel may not have run
    (void)hipMemsetAsync(t, 0, B * n * poly, c->stream);
    (void)hipMemsetAsync(z, 0, B * k * poly, c->stream);
    (void)hipMemsetAsync(ok, 0, B, c->stream);
    return rc;
  }
  for (const hipError_t e : wiped)
    if (e != hipSuccess) {
      c->err = std::string("open prove zk: hipMemsetAsync: ") + hipGetErrorString(e);
      return RZK_E_HIP;
    }
  return RZK_OK;
}

template <class C>
int open_prove_zk_host(rzk_ctx* c, const C* x, const uint8_t* nonce0, uint32_t stream, int gauss_kind, const uint8_t* aux32,
                       uint32_t max_rounds, C* cm, C* t, C* z, C* r, uint8_t* ok, uint8_t* rounds, uint32_t* rounds_run, size_t B) {
  if (!c) return RZK_E_ARG;
  if (rounds_run) *rounds_run = 0;
  const int rc = prove_args(c, nonce0, gauss_kind, max_rounds, B);
  if (rc != RZK_OK) return rc;
  if (B == 0) return RZK_OK;
  if (!x || !cm || !t || !z || !r || !ok || !rounds) return fail(c, RZK_E_ARG, "open prove zk: non-NULL x, c, t, z, r, ok, rounds expected");
  HostCall h(c);
  const auto dx = h.pin(x, B * c->l);
  const auto dcm = h.pout(cm, B * (c->n + c->l)), dt = h.pout(t, B * c->n), dz = h.pout(z, B * c->k), dr = h.pout(r, B * c->k);
  const auto dok = h.out(ok, B), drounds = h.out(rounds, B);
  return h.run([&] {
    return open_prove_zk_dev<C>(c, dx, nonce0, stream, gauss_kind, aux32, max_rounds, dcm, dt, dz, dr, dok, drounds, rounds_run, B);
  });
}

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

// diagnostic: pending_compact_kernel on the caller's flags, so that its edges are tested without a prover around it
int rzk_debug_compact_dev(rzk_ctx* c, const uint8_t* live, const uint8_t* done, size_t B, uint32_t* idx, uint32_t* count) {
  if (!c || !count || (B && (!live || !done || !idx))) return RZK_E_ARG;
  if ((uint64_t)B >> 32) return fail(c, RZK_E_ARG, "compact: B must stay below 2^32");
  return compact(c, live, done, B, idx, count);
}

}  // extern "C"
