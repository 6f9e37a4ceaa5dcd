// rzk_samplers.cpp — the device-side samplers of include/rzk.h: the seeded ones (Philox, rzk_rng.h) and the keyed ones
// (ChaCha20 blocks under the context's sampler key, rzk_chacha.h; the exact discrete Gaussian, §15).
#include "rzk_ctx.h"

namespace {

// One keyed draw of `npoly` polynomials into the device slab `out` (int32_t: 16-byte aligned, the slab32 rule, tested
// first): subkey = HChaCha20(key, nonce), the launch in a profiling slot (so that rzk_prof_read_kernels names the form that
// ran); the launch has copied the subkey into its kernel arguments, so the host copy is wiped whichever way the call
// ends.  launch(cfg, subkey) returns the launcher's status.
template <class C, class L>
int keyed_sample(rzk_ctx* c, const uint8_t* nonce, const C* out, size_t npoly, L launch) {
  if constexpr (sizeof(C) == 4) {
    if (misaligned({out})) return align_fail(c);
  }
  if (!c->sampler_key_set) return fail(c, RZK_E_ARG, "keyed sampler: no key set (rzk_sampler_set_key)");
  if (!nonce) return fail(c, RZK_E_ARG, "keyed sampler: NULL nonce");
  uint32_t sk[8];
  chacha_sampler_subkey(c->sampler_key, nonce, sk);
  const int rc = run_profiled(c, (uint64_t)polys<C>(c, npoly), "keyed sampler", [&](const LaunchCfg& cfg) { return launch(cfg, sk); });
  wipe(sk, sizeof(sk));
  return rc;
}

}  // namespace

extern "C" {

int rzk_sample_uniform_dev(rzk_ctx* c, uint64_t seed, uint32_t stream, uint64_t bound, int64_t* out, size_t count) {
  if (c && count == 0) return RZK_OK;
  if (!c || !out || bound == 0 || bound > (uint64_t)(c->q - 1) / 2) return RZK_E_ARG;
  return check_launch(c, launch_sample_uniform(cfg_of(c), out, count, c->N, seed, stream, (uint32_t)bound), "sampler");
}
int rzk_sample_gauss_dev(rzk_ctx* c, uint64_t seed, uint32_t stream, double sigma, int64_t* out, size_t count) {
  if (c && count == 0) return RZK_OK;
  // |x| stays far below (q-1)/2 for every sigma the parameters produce; 2^26 keeps 12 sigma inside the range
  if (!c || !out || !(sigma > 0.0) || sigma > 67108864.0) return RZK_E_ARG;
  // a profiling slot when profiling is on: rzk_prof_read_kernels names the form that ran
  return run_profiled(c, (uint64_t)count * c->N * sizeof(int64_t), "sampler", [&](const LaunchCfg& cfg) {
    return launch_sample_gauss(cfg, out, count, c->N, seed, stream, sigma);
  });
}
int rzk_sample_challenge_dev(rzk_ctx* c, uint64_t seed, uint32_t stream, int64_t* out, size_t count) {
  if (c && count == 0) return RZK_OK;
  if (!c || !out) return RZK_E_ARG;
  return check_launch(c, launch_sample_challenge(cfg_of(c), out, count, c->N, seed, stream, c->kappa), "sampler");
}

// ---- keyed samplers (v6): the same distributions from ChaCha20 blocks ------------------------------------------------
int rzk_sampler_set_key(rzk_ctx* c, const uint8_t key[32]) {
  if (!c) return RZK_E_ARG;
  wipe(c->sampler_key, sizeof(c->sampler_key));
  c->sampler_key_set = key != nullptr;
  if (key) std::memcpy(c->sampler_key, key, sizeof(c->sampler_key));
  return RZK_OK;
}

}  // extern "C"

// The four draws write int64_t or int32_t slabs (v14, slab32 prover): the same argument rules, streams and
// launches; every value an accepted argument can produce fits int32_t (tests/test_prove32_host.py), so the narrow form
// has no further range rule.
namespace rzk::api {

template <class C>
int sample_uniform_keyed_dev(rzk_ctx* c, const uint8_t* nonce, uint32_t stream, uint64_t bound, C* out, size_t count) {
  if (c && count == 0) return RZK_OK;
  if (!c || !out || bound == 0 || bound > (uint64_t)(c->q - 1) / 2) return RZK_E_ARG;
  return keyed_sample(c, nonce, out, count, [&](const LaunchCfg& cfg, const uint32_t* sk) {
    return launch_sample_uniform_chacha(cfg, out, count, c->N, sk, stream, (uint32_t)bound);
  });
}
RZK_BOTH_WIDTHS(sample_uniform_keyed_dev)

template <class C>
int sample_gauss_keyed_dev(rzk_ctx* c, const uint8_t* nonce, uint32_t stream, double sigma, C* out, size_t count) {
  if (c && count == 0) return RZK_OK;
  if (!c || !out || !(sigma > 0.0) || sigma > 67108864.0) return RZK_E_ARG;   // as rzk_sample_gauss_dev
  return keyed_sample(c, nonce, out, count, [&](const LaunchCfg& cfg, const uint32_t* sk) {
    return launch_sample_gauss_chacha(cfg, out, count, c->N, sk, stream, sigma);
  });
}
RZK_BOTH_WIDTHS(sample_gauss_keyed_dev)

// v11: the exact discrete Gaussian D_sigma (rzk_dgauss.h); count is in coefficients here
template <class C>
int sample_dgauss_keyed_dev(rzk_ctx* c, const uint8_t* nonce, uint32_t stream, uint32_t sigma, C* out, size_t count) {
  if (c && count == 0) return RZK_OK;
  if (!c || !out || sigma == 0 || sigma > kDgaussSigmaMax || count % c->N != 0) return RZK_E_ARG;
  const size_t npoly = count / c->N;
  return keyed_sample(c, nonce, out, npoly, [&](const LaunchCfg& cfg, const uint32_t* sk) {
    return launch_sample_dgauss_chacha(cfg, out, npoly, c->N, sk, stream, sigma);
  });
}
RZK_BOTH_WIDTHS(sample_dgauss_keyed_dev)

template <class C>
int sample_challenge_keyed_dev(rzk_ctx* c, const uint8_t* nonce, uint32_t stream, C* out, size_t count) {
  if (c && count == 0) return RZK_OK;
  if (!c || !out) return RZK_E_ARG;
  return keyed_sample(c, nonce, out, count, [&](const LaunchCfg& cfg, const uint32_t* sk) {
    return launch_sample_challenge_chacha(cfg, out, count, c->N, sk, stream, c->kappa);
  });
}
RZK_BOTH_WIDTHS(sample_challenge_keyed_dev)

}  // namespace rzk::api

extern "C" {

int rzk_sample_uniform_keyed_dev(rzk_ctx* c, const uint8_t nonce[16], uint32_t stream, uint64_t bound, int64_t* out, size_t count) {
  return sample_uniform_keyed_dev(c, nonce, stream, bound, out, count);
}
int rzk_sample_uniform_keyed32_dev(rzk_ctx* c, const uint8_t nonce[16], uint32_t stream, uint64_t bound, int32_t* out, size_t count) {
  return sample_uniform_keyed_dev(c, nonce, stream, bound, out, count);
}
int rzk_sample_gauss_keyed_dev(rzk_ctx* c, const uint8_t nonce[16], uint32_t stream, double sigma, int64_t* out, size_t count) {
  return sample_gauss_keyed_dev(c, nonce, stream, sigma, out, count);
}
int rzk_sample_gauss_keyed32_dev(rzk_ctx* c, const uint8_t nonce[16], uint32_t stream, double sigma, int32_t* out, size_t count) {
  return sample_gauss_keyed_dev(c, nonce, stream, sigma, out, count);
}
int rzk_sample_dgauss_keyed_dev(rzk_ctx* c, const uint8_t nonce[16], uint32_t stream, uint32_t sigma, int64_t* out, size_t count) {
  return sample_dgauss_keyed_dev(c, nonce, stream, sigma, out, count);
}
int rzk_sample_dgauss_keyed32_dev(rzk_ctx* c, const uint8_t nonce[16], uint32_t stream, uint32_t sigma, int32_t* out, size_t count) {
  return sample_dgauss_keyed_dev(c, nonce, stream, sigma, out, count);
}
int rzk_sample_challenge_keyed_dev(rzk_ctx* c, const uint8_t nonce[16], uint32_t stream, int64_t* out, size_t count) {
  return sample_challenge_keyed_dev(c, nonce, stream, out, count);
}
int rzk_sample_challenge_keyed32_dev(rzk_ctx* c, const uint8_t nonce[16], uint32_t stream, int32_t* out, size_t count) {
  return sample_challenge_keyed_dev(c, nonce, stream, out, count);
}

}  // extern "C"
