// rzk_key.cpp — the resident commitment key of a context (include/rzk.h): load, generate, expand from a seed, and the
// FS1 digest of the loaded key.
#include "rzk_ctx.h"
#include "rzk_keyplan.h"

namespace {

int fs_key_digest_dev(rzk_ctx* c, const int64_t* a_host, const int64_t* a_dev);

// a_dev: the same key on the device when the caller has it there (rzk_key_load_dev), else NULL
int key_load_impl(rzk_ctx* c, const int64_t* a_host, const int64_t* a_dev = nullptr) {
  const uint32_t N = c->N;
  // the host part (rzk_keyplan.h) first: a key it refuses leaves the context as it was — the previous key, its images,
  // its digest and every cached program stay in place
  KeyPlan kp;
  if (plan_key_tables(a_host, (size_t)(c->n + c->l) * c->k, N, c->q, c->key_class, c->key_entry, c->n_general, kp) != kPlanOk)
    return fail(c, RZK_E_ARG, "key coefficient outside the centred range");
  // from here on the previous key is gone: whichever step fails below, the context is left without a key
  c->key_loaded = false;
  const std::vector<int64_t>& general = kp.general;
  const std::vector<double>& kinf = kp.kinf;
  drop_programs(c);   // programs depend on the classification
  void* const stores[] = {c->d_key_ntt, c->d_key_l2, c->d_key_mont};
  c->d_key_ntt = nullptr;
  c->d_key_l2 = nullptr;
  c->d_key_mont = nullptr;
  hipError_t freed = hipSuccess;   // all three are released before the first error is reported
  for (void* p : stores) {
    const hipError_t e = p ? hipFree(p) : hipSuccess;
    if (freed == hipSuccess) freed = e;
  }
  HIPCHK(c, freed);
  if (c->n_general) {
    const size_t gbytes = general.size() * sizeof(int64_t);
    int rc = arena_reserve(c, c->stage, gbytes);
    if (rc != RZK_OK) return rc;
    const int64_t* staged = (const int64_t*)c->stage.p;
    if (c->small) {
      HIPCHK(c, hipMalloc((void**)&c->d_key_mont, general.size() * sizeof(uint32_t)));
      HIPCHK(c, hipMemcpyAsync(c->stage.p, general.data(), gbytes, hipMemcpyHostToDevice, c->stream));
      rc = check_launch(c, launch_key_mont(cfg_of(c), staged, c->d_key_mont, general.size(), c->dT, c->r2q), "key conversion");
    } else {
      HIPCHK(c, hipMalloc((void**)&c->d_key_ntt, (size_t)c->n_general * kKeyImages * N * sizeof(uint32_t)));
      HIPCHK(c, hipMalloc((void**)&c->d_key_l2, (size_t)c->n_general * sizeof(double)));
      HIPCHK(c, hipMemcpyAsync(c->stage.p, general.data(), gbytes, hipMemcpyHostToDevice, c->stream));
      HIPCHK(c, hipMemcpyAsync(c->d_key_l2, kinf.data(), kinf.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
      rc = check_launch(c, launch_key_transform((int)c->logn, cfg_of(c), staged, c->n_general, c->d_key_ntt, c->dT, c->d_tw),
                        "key transform");
    }
    if (rc != RZK_OK) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));   // `general` / `kinf` are host temporaries
  }
  int frc = fs_key_digest_dev(c, a_host, a_dev);
  if (frc != RZK_OK) return frc;
  c->key_loaded = true;
  return RZK_OK;
}

// FS1 key digest (rzk_keccak.h): leaf digests of the (n+l)*k key polynomials, then one root lane over the parameter
// header and those digests.  Runs once per key load, on the coefficients the load has at hand.
int fs_key_digest_dev(rzk_ctx* c, const int64_t* a_host, const int64_t* a_dev) {
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
  rc = check_launch(c, launch_fs_leaves<int64_t>(cfg, m, (c->q - 1) / 2, 0, dig, nullptr, nullptr, 1), "key leaf hash");
  if (rc != RZK_OK) return rc;
  FsRoot r{};
  fs_key_header(c->q, c->N, c->n, c->k, c->l, c->kappa, c->b, r.hdr);
  r.nhdr = kFsKeyHeaderWords;
  r.leaves = leaves;
  r.N = c->N;
  r.kappa = c->kappa;
  rc = check_launch(c, launch_fs_roots<int64_t>(cfg, r, dig, nullptr, out, 1), "key root hash");
  if (rc != RZK_OK) return rc;
  HIPCHK(c, hipMemcpyAsync(c->key_digest, out, sizeof c->key_digest, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return RZK_OK;
}

}  // namespace

extern "C" {

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

int rzk_fs_key_digest(rzk_ctx* c, uint8_t* out) {
  if (!c || !out) return RZK_E_ARG;
  if (!c->key_loaded) return fail(c, RZK_E_STATE, "commitment key not loaded");
  for (uint32_t w = 0; w < kFsDigestWords; ++w)
    for (int i = 0; i < 8; ++i) out[8 * w + i] = (uint8_t)(c->key_digest[w] >> (8 * i));   // little-endian on any host
  return RZK_OK;
}

static_assert(RZK_XOF_DOMAIN_KEY == kXofDomainKey, "the key domain of XP1");

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
    // staged without the sticky-word protocol of a host-pointer call: nothing here loads caller coefficients
    HostCall h(c);
    const auto d_seed = h.in(reinterpret_cast<const uint64_t*>(seed), 32);   // (the host bytes are only copied from)
    const auto d_slab = h.scratch<int64_t>(polys(c, n_rand));
    int rc = h.stage();
    if (rc != RZK_OK) return rc;
    int64_t* d_out = d_slab;
    size_t next = 0;
    for (uint32_t i = 0; i < n + l; ++i) {
      const uint32_t j0 = first_general(i);
      if (j0 == k) continue;
      rc = run_xof(c, kXofDomainKey, i * k + j0, k - j0, d_seed, d_out + next * N, 1);
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

}  // extern "C"
