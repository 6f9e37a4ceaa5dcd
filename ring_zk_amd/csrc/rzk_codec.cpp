// rzk_codec.cpp — the entry points around the proofs' messages (include/rzk.h), device- and host-pointer variants side by
// side: the wire codec, Fiat-Shamir challenges, the rejection step, packed records and seed expansion.  Each family
// has its kernels in a translation unit and its format in a header of its own, named at the family's section.
// The *_response_reject calls take their NULL test, alignment test, convert plan and staging from their slab lists
// (rzk_slabs.h, glue in rzk_ctx.h); the wire, packed, Fiat-Shamir and reject calls are driven by a schema or the caller's rows[].
#include "rzk_ctx.h"

// ---- v4: batched codec of the serialized protocol messages (rzk_wire_dev.hip, rzk_wire_walk.h) ------------------------
namespace {

bool wire_schema_of(const rzk_ctx* c, int kind, uint32_t V, uint32_t coef_bytes, WireSchema* s) {
  return c && wire_schema(kind, c->N, c->n, c->k, c->l, V, coef_bytes, s);
}

// slabs of the fields; only the Option of an Opening may be NULL, and only on encode
template <class C>
bool wire_slabs(const WireSchema& s, int kind, const C* const* fields, bool allow_none, WireSlabs* sl) {
  if (!fields) return false;
  for (int f = 0; f < kWireMaxFields; ++f) sl->ptr[f] = nullptr;
  for (uint32_t f = 0; f < s.nfields; ++f) {
    sl->ptr[f] = launch_addr(const_cast<C*>(fields[f]));
    if (!fields[f] && !(allow_none && kind == WIRE_OPENING && s.f[f].kind == WF_OPT)) return false;
  }
  return true;
}

template <class C = int64_t>
size_t wire_field_bytes(const rzk_ctx* c, const WireSchema& s, uint32_t f, size_t B) {
  return polys<C>(c, B * (size_t)(s.first[f + 1] - s.first[f]));
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
  HostCall h(c);
  // the staged copy of `bytes` starts on a 256-byte boundary, so alignment and offsets carry over
  const auto dbytes = h.in(bytes, total_len);
  const auto doffsets = h.in(offsets, (B + 1) * sizeof(uint64_t));
  const auto dok = h.out(ok, B);
  int64_t* dev_fields[kWireMaxFields] = {};
  for (uint32_t f = 0; f < s.nfields; ++f) h.out_to(&dev_fields[f], fields[f], wire_field_bytes(c, s, f, B));
  return h.run([&] { return rzk_wire_decode_batch_dev(c, kind, V, coef_bytes, dbytes, total_len, doffsets, dev_fields, dok, B); });
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
  HostCall h(c);
  const int64_t* dev_fields[kWireMaxFields] = {};   // (a None field stays NULL)
  for (uint32_t f = 0; f < s.nfields; ++f) h.in_to(&dev_fields[f], fields[f], wire_field_bytes(c, s, f, B));
  const auto dbytes = h.scratch<uint8_t>((size_t)dcap);
  const auto doffsets = h.scratch<uint64_t>((B + 1) * sizeof(uint64_t));
  return h.run([&] {
    const int rc = rzk_wire_encode_batch_dev(c, kind, V, coef_bytes, dev_fields, dbytes, dcap, doffsets, B);
    if (rc != RZK_OK) return rc;
    // copied out in two steps, here and not by HostCall: the offsets first, then the offsets[B] bytes they announce
    HIPCHK(c, hipMemcpyAsync(offsets, doffsets, (B + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (offsets[B] > dcap) return fail(c, RZK_E_HIP, "wire encode: message sizes exceed their maximum");
    if (offsets[B]) HIPCHK(c, hipMemcpyAsync(bytes, dbytes, offsets[B], hipMemcpyDeviceToHost, c->stream));
    return RZK_OK;
  });
}

// ---- v5: Fiat-Shamir challenges from the FS1 transcript (rzk_fs_dev.hip, rzk_keccak.h) --------------------------------
namespace {
bool fs_kind_ok(int kind) {
  return kind == RZK_MSG_OPEN_COMMITMENT || kind == RZK_MSG_LINEAR_COMMITMENT || kind == RZK_MSG_SUM_COMMITMENT;
}

}  // namespace

// The entry points below and of the packed codec exist for int64_t and int32_t slabs (v14, slab32 messages; DESIGN.md
// §19) over one body; 32-bit device slabs are 16-byte aligned.
namespace rzk::api {

template <class C>
int fs_challenge_dev(rzk_ctx* c, int kind, uint32_t V, const C* const* fields, const uint8_t* aux32, C* d, uint8_t* digest, uint8_t* ok,
                     size_t B) {
  WireSchema s;
  if (!c) return RZK_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));   // the memsets below come before the first cfg_of
  if (!fs_kind_ok(kind) || !wire_schema_of(c, kind, V, 8, &s)) return fail(c, RZK_E_ARG, "fs challenge: bad kind or V");
  if (c->kappa > c->N) return fail(c, RZK_E_ARG, "fs challenge: kappa exceeds the ring degree");
  if (!c->key_loaded) return fail(c, RZK_E_STATE, "commitment key not loaded");
  if (B == 0) return RZK_OK;
  WireSlabs sl;
  if (!d || !wire_slabs(s, kind, fields, false, &sl)) return fail(c, RZK_E_ARG, "fs challenge: NULL pointer");
  if constexpr (sizeof(C) == 4) {
    uintptr_t bits = (uintptr_t)d;
    for (uint32_t f = 0; f < s.nfields; ++f) bits |= (uintptr_t)sl.ptr[f];
    if (bits & 15u) return align_fail(c);
  }
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
  HIPCHK(c, hipMemsetAsync(d, 0, polys<C>(c, B), c->stream));   // the sampler writes the kappa non-zero coefficients only
  rc = run_profiled(c, polys<C>(c, B * (size_t)s.polys), "fs leaf kernel", [&](const LaunchCfg& cfg) {
    return launch_fs_leaves<C>(cfg, m, (c->q - 1) / 2, c->trusted ? 0 : 1, dig, ok, c->d_bad, B);
  });
  if (rc != RZK_OK) return rc;
  return run_profiled(c, (uint64_t)B * r.leaves * 32, "fs root kernel",
                      [&](const LaunchCfg& cfg) { return launch_fs_roots(cfg, r, dig, d, digest, B); });
}
RZK_BOTH_WIDTHS(fs_challenge_dev)

}  // namespace rzk::api

namespace {

template <class C>
int fs_challenge_host(rzk_ctx* c, int kind, uint32_t V, const C* const* fields, const uint8_t* aux32, C* d, uint8_t* digest, uint8_t* ok,
                      size_t B) {
  WireSchema s;
  if (!c) return RZK_E_ARG;
  if (!fs_kind_ok(kind) || !wire_schema_of(c, kind, V, 8, &s)) return fail(c, RZK_E_ARG, "fs challenge: bad kind or V");
  if (B == 0) return RZK_OK;
  WireSlabs sl;
  if (!d || !wire_slabs(s, kind, fields, false, &sl)) return fail(c, RZK_E_ARG, "fs challenge: NULL pointer");
  HostCall h(c);
  const auto dd = h.pout(d, B);
  const auto ddigest = h.out(digest, B * 32), dok = h.out(ok, B);
  const C* dev_fields[kWireMaxFields] = {};
  for (uint32_t f = 0; f < s.nfields; ++f) h.in_to(&dev_fields[f], fields[f], wire_field_bytes<C>(c, s, f, B));
  return h.run([&] { return fs_challenge_dev<C>(c, kind, V, dev_fields, aux32, dd, ddigest, dok, B); });
}

}  // namespace

int rzk_fs_challenge_batch_dev(rzk_ctx* c, int kind, uint32_t V, const int64_t* const* fields, const uint8_t* aux32,
                               int64_t* d, uint8_t* digest, uint8_t* ok, size_t B) {
  return fs_challenge_dev(c, kind, V, fields, aux32, d, digest, ok, B);
}
int rzk_fs_challenge_batch(rzk_ctx* c, int kind, uint32_t V, const int64_t* const* fields, const uint8_t* aux32,
                           int64_t* d, uint8_t* digest, uint8_t* ok, size_t B) {
  return fs_challenge_host(c, kind, V, fields, aux32, d, digest, ok, B);
}
int rzk_fs_challenge32_batch_dev(rzk_ctx* c, int kind, uint32_t V, const int32_t* const* fields, const uint8_t* aux32,
                                 int32_t* d, uint8_t* digest, uint8_t* ok, size_t B) {
  return fs_challenge_dev(c, kind, V, fields, aux32, d, digest, ok, B);
}
int rzk_fs_challenge32_batch(rzk_ctx* c, int kind, uint32_t V, const int32_t* const* fields, const uint8_t* aux32,
                             int32_t* d, uint8_t* digest, uint8_t* ok, size_t B) {
  return fs_challenge_host(c, kind, V, fields, aux32, d, digest, ok, B);
}

// ---- v7: the prover's rejection-sampling step (rzk_reject_dev.hip, rzk_reject.h) --------------------------------------
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

int rzk_reject_batch(rzk_ctx* c, uint32_t nparts, const int64_t* const* z, const int64_t* const* y, const uint32_t* rows,
                     const int64_t* coin, uint64_t R, double lnM, uint8_t* accept, int64_t* E, size_t B) {
  if (!c) return RZK_E_ARG;
  if (B == 0) return RZK_OK;
  uint64_t total = 0;
  int rc = reject_args(c, nparts, z, y, rows, coin, R, lnM, accept, &total);
  if (rc != RZK_OK) return rc;
  HostCall h(c);
  const auto dcoin = h.in(coin, B * sizeof(int64_t));
  const auto daccept = h.out(accept, B);
  const auto dE = h.out(E, B * sizeof(int64_t));
  const int64_t *dz[kRejectMaxParts] = {}, *dy[kRejectMaxParts] = {};
  for (uint32_t f = 0; f < nparts; ++f) {
    h.in_to(&dz[f], z[f], polys(c, B * rows[f]));
    h.in_to(&dy[f], y[f], polys(c, B * rows[f]));
  }
  return h.run([&] { return rzk_reject_batch_dev(c, nparts, dz, dy, rows, dcoin, R, lnM, daccept, dE, B); });
}

// ---- v13: the response and its rejection test in one call (rzk_response_stat_dev.hip) ------------------
namespace {

// One call = the response launches of `response` and the decision over the parts (z_f, y_f).  Where the rotation kernel
// runs with one wavefront per polynomial (response_stat_fused) the response rows leave the partials themselves
// (response(&stat)); everywhere else the chain runs inside the call: response(NULL), then reject_stat_kernel on (z, y).
// Either way one reject_decide_kernel over ws_reject ends the call.  may_fuse = false: the unfused side on every context
// (rzk_reject_batch_dev: z exists already, there are no response rows to leave the partials).
template <class F>
int response_reject(rzk_ctx* c, uint32_t nparts, const int64_t* const* z, const int64_t* const* y, const uint32_t* rows,
                    const int64_t* coin, uint64_t R, double lnM, uint8_t* accept, int64_t* E, size_t B, bool may_fuse, F response) {
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
  const ResponseStat stat{part, m.rows, 0, (int64_t)(c->b * c->kappa), limit};
  const bool fused = may_fuse && response_stat_fused(c);
  rc = response(fused ? &stat : nullptr);
  if (rc != RZK_OK) return rc;
  if (!fused) {
    rc = run_profiled(c, (uint64_t)B * total * c->N * 2 * sizeof(int64_t), "reject stat kernel", [&](const LaunchCfg& cfg) {
      return launch_reject_stat(cfg, m, c->q, c->b * c->kappa, limit, c->trusted, part, B);
    });
    if (rc != RZK_OK) return rc;
  }
  const double sg = (double)c->sigma;
  return run_profiled(c, (uint64_t)B * total * sizeof(RejectPartial), "reject decide kernel", [&](const LaunchCfg& cfg) {
    return launch_reject_decide(cfg, part, m.rows, coin, R, lnM, 2.0 * sg * sg, accept, E, c->d_bad, B);
  });
}

// `stat` with its partials moved to where a later launch of the call starts
ResponseStat stat_at(const ResponseStat& s, uint32_t off) {
  ResponseStat t = s;
  t.part_off = off;
  return t;
}

// the argument rules the response_reject calls share, both forms: kGo, or what the call returns
template <const CallSlabs& S, class... P>
int response_reject_args(rzk_ctx* c, size_t B, P*... p) {
  if (!c) return RZK_E_ARG;
  if (B == 0) return RZK_OK;
  return slabs_null<S>(p...) ? fail(c, RZK_E_ARG, "response reject: non-NULL y, r, d, coin, z, accept expected") : kGo;
}

}  // namespace

// the rejection step alone: response_reject without response launches
int rzk_reject_batch_dev(rzk_ctx* c, uint32_t nparts, const int64_t* const* z, const int64_t* const* y, const uint32_t* rows,
                         const int64_t* coin, uint64_t R, double lnM, uint8_t* accept, int64_t* E, size_t B) {
  if (!c) return RZK_E_ARG;
  if (B == 0) return RZK_OK;
  return response_reject(c, nparts, z, y, rows, coin, R, lnM, accept, E, B, false, [](const ResponseStat*) { return RZK_OK; });
}

// The Open form at either width (v14, slab32 prover).  The partials, the decision kernel, coin, accept and
// E do not see the width; reject_args and RejectParts only carry the addresses of z and y.  32-bit slabs run natively
// where the fused rows do, and convert everywhere else.
namespace rzk::api {

template <class C>
int open_response_reject_dev(rzk_ctx* c, const C* y, const C* r, const C* d, const int64_t* coin, uint64_t R, double lnM, C* z,
                             uint8_t* accept, int64_t* E, size_t B) {
  if (const int rc = response_reject_args<kSlabsOpenResponseReject>(c, B, y, r, d, coin, z, accept, E); rc != kGo) return rc;
  const uint32_t k = c->k;
  if constexpr (sizeof(C) == 4) {
    if (slabs_misaligned<kSlabsOpenResponseReject>(y, r, d, coin, z, accept, E)) return align_fail(c);
    if (!(program_native32(c, PG_RESPONSE, 1) && response_stat_fused(c)))
      return convert_call<kSlabsOpenResponseReject>(c, {}, B, [&](auto wy, auto wr, auto wd, auto wcoin, auto... out) {
        return open_response_reject_dev<int64_t>(c, wy, wr, wd, wcoin, R, lnM, out..., B);
      }, y, r, d, coin, z, accept, E);
  }
  const int64_t *zs[1] = {launch_addr(z)}, *ys[1] = {launch_addr(y)};
  const uint32_t rows[1] = {k};
  return response_reject(c, 1, zs, ys, rows, coin, R, lnM, accept, E, B, true, [&](const ResponseStat* st) {
    if constexpr (sizeof(C) == 4) {
      if (!st) return fail(c, RZK_E_STATE, "response reject on 32-bit slabs needs the fused rows");
    }
    return run_program<C>(c, PG_RESPONSE, 1, {{d, 1, 0}, {y, k, 0}, {r, k, 0}, {z, k, 0}}, nullptr, 1, B, 0, true, 0, 0, st);
  });
}
RZK_BOTH_WIDTHS(open_response_reject_dev)

}  // namespace rzk::api

int rzk_open_response_reject_batch_dev(rzk_ctx* c, const int64_t* y, const int64_t* r, const int64_t* d, const int64_t* coin,
                                       uint64_t R, double lnM, int64_t* z, uint8_t* accept, int64_t* E, size_t B) {
  return open_response_reject_dev(c, y, r, d, coin, R, lnM, z, accept, E, B);
}
int rzk_open_response_reject32_batch_dev(rzk_ctx* c, const int32_t* y, const int32_t* r, const int32_t* d, const int64_t* coin,
                                         uint64_t R, double lnM, int32_t* z, uint8_t* accept, int64_t* E, size_t B) {
  return open_response_reject_dev(c, y, r, d, coin, R, lnM, z, accept, E, B);
}

// The Linear form at either width: as the Open form, with two parts.
namespace {

template <class C>
int linear_response_reject_dev(rzk_ctx* c, const C* y, const C* yp, const C* r, const C* rp, const C* d, const int64_t* coin, uint64_t R,
                               double lnM, C* z, C* zp, uint8_t* accept, int64_t* E, size_t B) {
  if (const int rc = response_reject_args<kSlabsLinearResponseReject>(c, B, y, yp, r, rp, d, coin, z, zp, accept, E); rc != kGo) return rc;
  const uint32_t k = c->k;
  if constexpr (sizeof(C) == 4) {
    if (slabs_misaligned<kSlabsLinearResponseReject>(y, yp, r, rp, d, coin, z, zp, accept, E)) return align_fail(c);
    if (!(program_native32(c, PG_RESPONSE, 2) && response_stat_fused(c)))
      return convert_call<kSlabsLinearResponseReject>(c, {}, B, [&](auto wy, auto wyp, auto wr, auto wrp, auto wd, auto wcoin, auto... out) {
        return linear_response_reject_dev<int64_t>(c, wy, wyp, wr, wrp, wd, wcoin, R, lnM, out..., B);
      }, y, yp, r, rp, d, coin, z, zp, accept, E);
  }
  const int64_t *zs[2] = {launch_addr(z), launch_addr(zp)}, *ys[2] = {launch_addr(y), launch_addr(yp)};
  const uint32_t rows[2] = {k, k};
  return response_reject(c, 2, zs, ys, rows, coin, R, lnM, accept, E, B, true, [&](const ResponseStat* st) {
    if constexpr (sizeof(C) == 4) {
      if (!st) return fail(c, RZK_E_STATE, "response reject on 32-bit slabs needs the fused rows");
    }
    // the 2k rows of the program are z then zp: the order of the parts
    return run_program<C>(c, PG_RESPONSE, 2, {{d, 1, 0}, {y, k, 0}, {r, k, 0}, {z, k, 0}, {yp, k, 0}, {rp, k, 0}, {zp, k, 0}}, nullptr, 1,
                          B, 0, true, 0, 0, st);
  });
}
}  // namespace

int rzk_linear_response_reject_batch_dev(rzk_ctx* c, const int64_t* y, const int64_t* yp, const int64_t* r, const int64_t* rp,
                                         const int64_t* d, const int64_t* coin, uint64_t R, double lnM, int64_t* z, int64_t* zp,
                                         uint8_t* accept, int64_t* E, size_t B) {
  return linear_response_reject_dev(c, y, yp, r, rp, d, coin, R, lnM, z, zp, accept, E, B);
}
int rzk_linear_response_reject32_batch_dev(rzk_ctx* c, const int32_t* y, const int32_t* yp, const int32_t* r, const int32_t* rp,
                                           const int32_t* d, const int64_t* coin, uint64_t R, double lnM, int32_t* z, int32_t* zp,
                                           uint8_t* accept, int64_t* E, size_t B) {
  return linear_response_reject_dev(c, y, yp, r, rp, d, coin, R, lnM, z, zp, accept, E, B);
}

int rzk_sum_response_reject_batch_dev(rzk_ctx* c, uint32_t V, const int64_t* ys, const int64_t* yp, const int64_t* rs,
                                      const int64_t* rp, const int64_t* d, const int64_t* coin, uint64_t R, double lnM, int64_t* zs,
                                      int64_t* zp, uint8_t* accept, int64_t* E, size_t B) {
  if (const int rc = response_reject_args<kSlabsSumResponseReject>(c, B, ys, yp, rs, rp, d, coin, zs, zp, accept, E); rc != kGo) return rc;
  if (V == 0 || V > (1u << 20)) return fail(c, RZK_E_ARG, "response reject: V must lie in 1 .. 2^20");
  const uint32_t k = c->k;
  const int64_t *z2[2] = {zs, zp}, *y2[2] = {ys, yp};
  const uint32_t rows[2] = {V * k, k};
  return response_reject(c, 2, z2, y2, rows, coin, R, lnM, accept, E, B, true, [&](const ResponseStat* st) {
    // as rzk_sum_response_batch_dev: the summands as batch entries that share d, then zp; partial (b, s k + i) and (b, V k + i)
    ResponseStat s0, s1;
    if (st) s0 = stat_at(*st, 0), s1 = stat_at(*st, V * k);
    int rc = run_program(c, PG_RESPONSE, 1, {{d, 1, 1}, {ys, k, 0}, {rs, k, 0}, {zs, k, 0}}, nullptr, V, (uint64_t)B * V, 0, true, 0, 0,
                         st ? &s0 : nullptr);
    if (rc != RZK_OK) return rc;
    return run_program(c, PG_RESPONSE, 1, {{d, 1, 0}, {yp, k, 0}, {rp, k, 0}, {zp, k, 0}}, nullptr, 1, B, 0, true, 0, 0, st ? &s1 : nullptr);
  });
}

namespace {
template <class C>
int open_response_reject_host(rzk_ctx* c, const C* y, const C* r, const C* d, const int64_t* coin, uint64_t R, double lnM, C* z,
                              uint8_t* accept, int64_t* E, size_t B) {
  if (const int rc = response_reject_args<kSlabsOpenResponseReject>(c, B, y, r, d, coin, z, accept, E); rc != kGo) return rc;
  return host_run<kSlabsOpenResponseReject>(c, {}, B, [&](auto dy, auto dr, auto dd, auto dcoin, auto... out) {
    return open_response_reject_dev<C>(c, dy, dr, dd, dcoin, R, lnM, out..., B);
  }, y, r, d, coin, z, accept, E);
}
}  // namespace

int rzk_open_response_reject_batch(rzk_ctx* c, const int64_t* y, const int64_t* r, const int64_t* d, const int64_t* coin, uint64_t R,
                                   double lnM, int64_t* z, uint8_t* accept, int64_t* E, size_t B) {
  return open_response_reject_host(c, y, r, d, coin, R, lnM, z, accept, E, B);
}
int rzk_open_response_reject32_batch(rzk_ctx* c, const int32_t* y, const int32_t* r, const int32_t* d, const int64_t* coin, uint64_t R,
                                     double lnM, int32_t* z, uint8_t* accept, int64_t* E, size_t B) {
  return open_response_reject_host(c, y, r, d, coin, R, lnM, z, accept, E, B);
}

namespace {
template <class C>
int linear_response_reject_host(rzk_ctx* c, const C* y, const C* yp, const C* r, const C* rp, const C* d, const int64_t* coin, uint64_t R,
                                double lnM, C* z, C* zp, uint8_t* accept, int64_t* E, size_t B) {
  if (const int rc = response_reject_args<kSlabsLinearResponseReject>(c, B, y, yp, r, rp, d, coin, z, zp, accept, E); rc != kGo) return rc;
  return host_run<kSlabsLinearResponseReject>(c, {}, B, [&](auto dy, auto dyp, auto dr, auto drp, auto dd, auto dcoin, auto... out) {
    return linear_response_reject_dev<C>(c, dy, dyp, dr, drp, dd, dcoin, R, lnM, out..., B);
  }, y, yp, r, rp, d, coin, z, zp, accept, E);
}
}  // namespace

int rzk_linear_response_reject_batch(rzk_ctx* c, const int64_t* y, const int64_t* yp, const int64_t* r, const int64_t* rp,
                                     const int64_t* d, const int64_t* coin, uint64_t R, double lnM, int64_t* z, int64_t* zp,
                                     uint8_t* accept, int64_t* E, size_t B) {
  return linear_response_reject_host(c, y, yp, r, rp, d, coin, R, lnM, z, zp, accept, E, B);
}
int rzk_linear_response_reject32_batch(rzk_ctx* c, const int32_t* y, const int32_t* yp, const int32_t* r, const int32_t* rp,
                                       const int32_t* d, const int64_t* coin, uint64_t R, double lnM, int32_t* z, int32_t* zp,
                                       uint8_t* accept, int64_t* E, size_t B) {
  return linear_response_reject_host(c, y, yp, r, rp, d, coin, R, lnM, z, zp, accept, E, B);
}

int rzk_sum_response_reject_batch(rzk_ctx* c, uint32_t V, const int64_t* ys, const int64_t* yp, const int64_t* rs, const int64_t* rp,
                                  const int64_t* d, const int64_t* coin, uint64_t R, double lnM, int64_t* zs, int64_t* zp,
                                  uint8_t* accept, int64_t* E, size_t B) {
  if (const int rc = response_reject_args<kSlabsSumResponseReject>(c, B, ys, yp, rs, rp, d, coin, zs, zp, accept, E); rc != kGo) return rc;
  if (V == 0 || V > (1u << 20)) return fail(c, RZK_E_ARG, "response reject: V must lie in 1 .. 2^20");
  return host_run<kSlabsSumResponseReject>(
      c, by_V(V), B,
      [&](const int64_t* dys, const int64_t* dyp, const int64_t* drs, const int64_t* drp, const int64_t* dd, const int64_t* dcoin,
          int64_t* dzs, int64_t* dzp, uint8_t* daccept, int64_t* dE) {
        return rzk_sum_response_reject_batch_dev(c, V, dys, dyp, drs, drp, dd, dcoin, R, lnM, dzs, dzp, daccept, dE, B);
      },
      ys, yp, rs, rp, d, coin, zs, zp, accept, E);
}

// ---- v8: fixed-width packed records "RZKP1" (rzk_packed_dev.hip, rzk_packed.h) -----------------------------------------
static_assert(RZK_MSG_LINEAR_RESPONSE == PK_LINEAR_RESPONSE && RZK_MSG_OPEN_SHORT == PK_OPEN_SHORT &&
                  RZK_MSG_OPENING == PK_OPENING && RZK_MSG_SUM_RESPONSE == PK_SUM_RESPONSE &&
                  RZK_MSG_LINEAR_SHORT == PK_LINEAR_SHORT && RZK_MSG_SUM_SHORT == PK_SUM_SHORT,
              "packed kinds are the RZK_MSG_* values");

namespace {

bool packed_schema_of(const rzk_ctx* c, int kind, uint32_t V, PackedSchema* s) {
  return c && packed_schema(kind, c->N, c->n, c->k, c->l, V, c->q, c->verify_bound, s);
}

// argument rules shared by the entry points; on RZK_OK *s and *sl are filled
template <class C>
int packed_args(rzk_ctx* c, int kind, uint32_t V, const C* const* fields, const uint8_t* records, const uint8_t* ok, size_t B,
                PackedSchema* s, PackedSlabs* sl) {
  if (!packed_schema_of(c, kind, V, s)) return fail(c, RZK_E_ARG, "packed codec: bad kind or V");
  if (B == 0) return RZK_OK;   // a no-op, whatever the pointers
  if (!fields || !records || !ok) return fail(c, RZK_E_ARG, "packed codec: NULL pointer");
  for (int f = 0; f < kPackedMaxFields; ++f) sl->ptr[f] = nullptr;
  for (uint32_t f = 0; f < s->nfields; ++f) {
    if (!fields[f]) return fail(c, RZK_E_ARG, "packed codec: NULL slab");
    sl->ptr[f] = launch_addr(const_cast<C*>(fields[f]));   // (PackedSlabs serves both directions, so its pointers are not const)
  }
  if ((uintptr_t)records % 8) return fail(c, RZK_E_ARG, "packed codec: records must be 8-byte aligned");
  return RZK_OK;
}

template <class C>
size_t packed_field_bytes(const rzk_ctx* c, const PackedSchema& s, uint32_t f, size_t B) {
  return polys<C>(c, B * (size_t)s.f[f].rows);
}

// one launch between preset and profile bookkeeping, on slabs of C; decode: records -> slabs
template <class C>
int packed_run(rzk_ctx* c, const PackedSchema& s, const PackedSlabs& sl, uint8_t* records, uint8_t* ok, size_t B, bool decode) {
  for (uint32_t f = 0; f < s.nfields; ++f)
    if ((uintptr_t)sl.ptr[f] % 16) return fail(c, RZK_E_ARG, "packed codec: device slabs must be 16-byte aligned");
  HIPCHK(c, hipSetDevice(c->device));   // the memset below comes before the first cfg_of
  HIPCHK(c, hipMemsetAsync(ok, 1, B, c->stream));
  uint64_t slab_bytes = 0;
  for (uint32_t f = 0; f < s.nfields; ++f) slab_bytes += packed_field_bytes<C>(c, s, f, B);
  return run_profiled(c, slab_bytes + (uint64_t)B * packed_record_bytes(s), decode ? "packed decode kernel" : "packed encode kernel",
                      [&](const LaunchCfg& cfg) {
                        return decode ? launch_packed_decode<C>(cfg, s, sl, (const uint64_t*)records, ok, B)
                                      : launch_packed_encode<C>(cfg, s, sl, (uint64_t*)records, ok, B);
                      });
}

// encode reads the slabs of `fields` and writes `records`; decode the reverse
template <class C>
int packed_dev(rzk_ctx* c, int kind, uint32_t V, const C* const* fields, uint8_t* records, uint8_t* ok, size_t B, bool decode) {
  PackedSchema s;
  PackedSlabs sl;
  if (!c) return RZK_E_ARG;
  const int rc = packed_args(c, kind, V, fields, records, ok, B, &s, &sl);
  if (rc != RZK_OK || B == 0) return rc;
  return packed_run<C>(c, s, sl, records, ok, B, decode);
}

// the host forms stage the slabs on 256-byte boundaries; sl, checked on the host pointers, then names the staged copies
template <class C>
int packed_encode_host(rzk_ctx* c, int kind, uint32_t V, const C* const* fields, uint8_t* records, uint8_t* ok, size_t B) {
  PackedSchema s;
  PackedSlabs sl;
  if (!c) return RZK_E_ARG;
  int rc = packed_args(c, kind, V, fields, records, ok, B, &s, &sl);
  if (rc != RZK_OK || B == 0) return rc;
  HostCall h(c);
  const auto drecords = h.out(records, B * (size_t)packed_record_bytes(s));
  const auto dok = h.out(ok, B);
  const C* dev_fields[kPackedMaxFields] = {};
  for (uint32_t f = 0; f < s.nfields; ++f) h.in_to(&dev_fields[f], fields[f], packed_field_bytes<C>(c, s, f, B));
  return h.run([&] {
    for (uint32_t f = 0; f < s.nfields; ++f) sl.ptr[f] = launch_addr(const_cast<C*>(dev_fields[f]));
    return packed_run<C>(c, s, sl, drecords, dok, B, false);
  });
}

template <class C>
int packed_decode_host(rzk_ctx* c, int kind, uint32_t V, const uint8_t* records, C* const* fields, uint8_t* ok, size_t B) {
  PackedSchema s;
  PackedSlabs sl;
  if (!c) return RZK_E_ARG;
  const int rc = packed_args<C>(c, kind, V, fields, records, ok, B, &s, &sl);
  if (rc != RZK_OK || B == 0) return rc;
  HostCall h(c);
  const auto drecords = h.in(records, B * (size_t)packed_record_bytes(s));
  const auto dok = h.out(ok, B);
  C* dev_fields[kPackedMaxFields] = {};
  for (uint32_t f = 0; f < s.nfields; ++f) h.out_to(&dev_fields[f], fields[f], packed_field_bytes<C>(c, s, f, B));
  return h.run([&] {
    const uint8_t* rec = drecords;
    for (uint32_t f = 0; f < s.nfields; ++f) sl.ptr[f] = launch_addr(dev_fields[f]);
    return packed_run<C>(c, s, sl, const_cast<uint8_t*>(rec), dok, B, true);
  });
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
  return packed_dev(c, kind, V, fields, records, ok, B, false);
}
int rzk_packed_decode_batch_dev(rzk_ctx* c, int kind, uint32_t V, const uint8_t* records, int64_t* const* fields, uint8_t* ok,
                                size_t B) {
  return packed_dev<int64_t>(c, kind, V, fields, const_cast<uint8_t*>(records), ok, B, true);
}
int rzk_packed_encode_batch(rzk_ctx* c, int kind, uint32_t V, const int64_t* const* fields, uint8_t* records, uint8_t* ok,
                            size_t B) {
  return packed_encode_host(c, kind, V, fields, records, ok, B);
}
int rzk_packed_decode_batch(rzk_ctx* c, int kind, uint32_t V, const uint8_t* records, int64_t* const* fields, uint8_t* ok,
                            size_t B) {
  return packed_decode_host(c, kind, V, records, fields, ok, B);
}
// the same four over int32_t slabs (v14, slab32 messages): records carry no width
int rzk_packed_encode32_batch_dev(rzk_ctx* c, int kind, uint32_t V, const int32_t* const* fields, uint8_t* records, uint8_t* ok,
                                  size_t B) {
  return packed_dev(c, kind, V, fields, records, ok, B, false);
}
int rzk_packed_decode32_batch_dev(rzk_ctx* c, int kind, uint32_t V, const uint8_t* records, int32_t* const* fields, uint8_t* ok,
                                  size_t B) {
  return packed_dev<int32_t>(c, kind, V, fields, const_cast<uint8_t*>(records), ok, B, true);
}
int rzk_packed_encode32_batch(rzk_ctx* c, int kind, uint32_t V, const int32_t* const* fields, uint8_t* records, uint8_t* ok,
                              size_t B) {
  return packed_encode_host(c, kind, V, fields, records, ok, B);
}
int rzk_packed_decode32_batch(rzk_ctx* c, int kind, uint32_t V, const uint8_t* records, int32_t* const* fields, uint8_t* ok,
                              size_t B) {
  return packed_decode_host(c, kind, V, records, fields, ok, B);
}

// ---- v10: public polynomials expanded from 32-byte seeds, "XP1" (rzk_xof_dev.hip, rzk_xof.h; keys: rzk_key.cpp) ------------
int rzk::api::run_xof(rzk_ctx* c, uint32_t domain, uint32_t p0, uint32_t rows, const uint64_t* seeds, int64_t* out, size_t B) {
  const XofJob j{(uint64_t)c->q, c->N, domain, p0, rows, c->N / xof_chunk_len(c->N), xof_mask((uint64_t)c->q)};
  return run_profiled(c, (uint64_t)B * rows * c->N * sizeof(int64_t), "xof kernel",
                      [&](const LaunchCfg& cfg) { return launch_xof_uniform(cfg, j, seeds, out, B); });
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
  HostCall h(c);
  const auto dseeds = h.in(seeds, B * 32);
  const auto dout = h.pout(out, B * (size_t)rows);
  return h.run([&] { return rzk_xof_uniform_batch_dev(c, dseeds, domain, rows, dout, B); });
}
