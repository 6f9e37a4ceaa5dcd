// rzk_host.cpp — the host-pointer variants of the Mat-level operations and the three protocols (include/rzk.h): each
// names its slab list (rzk_slabs.h) and the *_dev entry point of the same name; host_call (rzk_ctx.h) derives the NULL
// test and the staging from the list.  The variants of the codecs, Fiat-Shamir, rejection and XOF entry points sit next
// to those in rzk_codec.cpp.  A call that exists for int64_t and int32_t slabs has one list: the pointers' own width stages them.
#include "rzk_ctx.h"

namespace rzk::api {

size_t HostCall::add(const void* in, void* out, size_t bytes, bool null, void* slot, void (*set)(void*, void*)) {
  if (null) return kNull;
  bufs_.push_back(Buf{in, out, bytes, total_, slot, set});
  total_ += (bytes + 255) & ~size_t(255);
  return bufs_.back().off;
}

int HostCall::stage() {
  int rc = arena_reserve(c_, c_->stage, total_);
  if (rc != RZK_OK) return rc;
  for (const Buf& b : bufs_) {
    if (b.slot) b.set(b.slot, (char*)c_->stage.p + b.off);
    if (b.in && b.bytes)
      HIPCHK(c_, hipMemcpyAsync((char*)c_->stage.p + b.off, b.in, b.bytes, hipMemcpyHostToDevice, c_->stream));
  }
  return RZK_OK;
}

int HostCall::begin() {
  HIPCHK(c_, hipSetDevice(c_->device));   // the memset comes before the first cfg_of; the thread may have another device
  HIPCHK(c_, hipMemsetAsync(c_->d_bad, 0, sizeof(uint32_t), c_->stream));
  return stage();
}

int HostCall::end(int rc) {
  if (rc != RZK_OK) {
    const std::string keep = c_->err;
    (void)take_input_error(c_);
    c_->err = keep;
    return rc;
  }
  for (const Buf& b : bufs_)
    if (b.out && b.bytes)
      HIPCHK(c_, hipMemcpyAsync(b.out, (char*)c_->stage.p + b.off, b.bytes, hipMemcpyDeviceToHost, c_->stream));
  return take_input_error(c_);
}

}  // namespace rzk::api

namespace {

int host_ntt(rzk_ctx* c, int prime, const uint32_t* in, uint32_t* out, size_t count,
             int (*dev)(rzk_ctx*, int, const uint32_t*, uint32_t*, size_t)) {
  if (c && count == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !in || !out) return RZK_E_ARG;
  HostCall h(c);
  const auto din = h.in(in, count * c->N * sizeof(uint32_t));
  const auto dout = h.out(out, count * c->N * sizeof(uint32_t));
  return h.run([&] { return dev(c, prime, din, dout, count); });
}

}  // namespace

extern "C" {

int rzk_polymul_batch(rzk_ctx* c, const int64_t* a, const int64_t* b, int64_t* out, size_t count) {
  return host_form<kSlabsPolymul>(c, count, rzk_polymul_batch_dev, a, b, out);
}
int rzk_add_batch(rzk_ctx* c, const int64_t* a, const int64_t* b, int64_t* out, size_t count) {
  return host_form<kSlabsAdd>(c, count, rzk_add_batch_dev, a, b, out);
}
int rzk_sub_batch(rzk_ctx* c, const int64_t* a, const int64_t* b, int64_t* out, size_t count) {
  return host_form<kSlabsSub>(c, count, rzk_sub_batch_dev, a, b, out);
}
int rzk_ntt_forward_batch(rzk_ctx* c, int prime, const uint32_t* in, uint32_t* out, size_t count) {
  return host_ntt(c, prime, in, out, count, rzk_ntt_forward_batch_dev);
}
int rzk_ntt_inverse_batch(rzk_ctx* c, int prime, const uint32_t* in, uint32_t* out, size_t count) {
  return host_ntt(c, prime, in, out, count, rzk_ntt_inverse_batch_dev);
}

int rzk_matvec_batch(rzk_ctx* c, int which, const int64_t* v, const int64_t* addend, int64_t* out, size_t B) {
  return host_form<kSlabsMatvec>(c, by_key(which), B, which, rzk_matvec_batch_dev, v, addend, out);
}
int rzk_matvec32_batch(rzk_ctx* c, int which, const int32_t* v, const int32_t* addend, int32_t* out, size_t B) {
  return host_form<kSlabsMatvec>(c, by_key(which), B, which, rzk_matvec32_batch_dev, v, addend, out);
}

int rzk_cmul_batch(rzk_ctx* c, const int64_t* m, uint32_t rows, const int64_t* p, int64_t* out, size_t B) {
  return host_call<kSlabsCmul>(c, by_rows(rows), B, [&](const int64_t* dm, const int64_t* dp, int64_t* dout) {
    return rzk_cmul_batch_dev(c, dm, rows, dp, dout, B);
  }, m, p, out);
}

int rzk_canonicalize_batch(rzk_ctx* c, const int64_t* in, int64_t* out, size_t count) {
  return host_form<kSlabsCanonicalize>(c, count, rzk_canonicalize_batch_dev, in, out);
}

int rzk_norm2_le_batch(rzk_ctx* c, const int64_t* v, uint32_t rows, uint64_t bound, uint8_t* ok, size_t B) {
  return host_call<kSlabsNorm2Le>(c, by_rows(rows), B, [&](const int64_t* dv, uint8_t* dok) {
    return rzk_norm2_le_batch_dev(c, dv, rows, bound, dok, B);
  }, v, ok);
}
int rzk_norm2_le32_batch(rzk_ctx* c, const int32_t* v, uint32_t rows, uint64_t bound, uint8_t* ok, size_t B) {
  return host_call<kSlabsNorm2Le>(c, by_rows(rows), B, [&](const int32_t* dv, uint8_t* dok) {
    return rzk_norm2_le32_batch_dev(c, dv, rows, bound, dok, B);
  }, v, ok);
}

int rzk_eq_batch(rzk_ctx* c, const int64_t* a, const int64_t* b, uint32_t rows, uint8_t* eq, size_t B) {
  return host_call<kSlabsEq>(c, by_rows(rows), B, [&](const int64_t* da, const int64_t* db, uint8_t* deq) {
    return rzk_eq_batch_dev(c, da, db, rows, deq, B);
  }, a, b, eq);
}

int rzk_commit_batch(rzk_ctx* c, const int64_t* x, const int64_t* r, int64_t* cm, uint8_t* ok, size_t B) {
  return host_form<kSlabsCommit>(c, B, rzk_commit_batch_dev, x, r, cm, ok);
}

int rzk_commitment_verify_batch(rzk_ctx* c, const int64_t* cm, const int64_t* x, const int64_t* r, const int64_t* f,
                                uint8_t* ok, size_t B) {
  return host_form<kSlabsCommitmentVerify>(c, B, rzk_commitment_verify_batch_dev, cm, x, r, f, ok);
}

// ---- OpenProof and its recompute step, at either width ---------------------------------------------------------------
int rzk_open_commit_batch(rzk_ctx* c, const int64_t* x, const int64_t* r, const int64_t* y, int64_t* cm, int64_t* t, uint8_t* ok,
                          size_t B) {
  return host_form<kSlabsOpenCommit>(c, B, rzk_open_commit_batch_dev, x, r, y, cm, t, ok);
}
int rzk_open_commit32_batch(rzk_ctx* c, const int32_t* x, const int32_t* r, const int32_t* y, int32_t* cm, int32_t* t, uint8_t* ok,
                            size_t B) {
  return host_form<kSlabsOpenCommit>(c, B, rzk_open_commit32_batch_dev, x, r, y, cm, t, ok);
}
int rzk_open_response_batch(rzk_ctx* c, const int64_t* y, const int64_t* r, const int64_t* d, int64_t* z, size_t B) {
  return host_form<kSlabsOpenResponse>(c, B, rzk_open_response_batch_dev, y, r, d, z);
}
int rzk_open_response32_batch(rzk_ctx* c, const int32_t* y, const int32_t* r, const int32_t* d, int32_t* z, size_t B) {
  return host_form<kSlabsOpenResponse>(c, B, rzk_open_response32_batch_dev, y, r, d, z);
}
int rzk_open_verify_batch(rzk_ctx* c, const int64_t* z, const int64_t* t, const int64_t* cm, const int64_t* d, uint8_t* accept,
                          size_t B) {
  return host_form<kSlabsOpenVerify>(c, B, rzk_open_verify_batch_dev, z, t, cm, d, accept);
}
int rzk_open_verify32_batch(rzk_ctx* c, const int32_t* z, const int32_t* t, const int32_t* cm, const int32_t* d, uint8_t* accept,
                            size_t B) {
  return host_form<kSlabsOpenVerify>(c, B, rzk_open_verify32_batch_dev, z, t, cm, d, accept);
}
int rzk_open_recover_batch(rzk_ctx* c, const int64_t* z, const int64_t* cm, const int64_t* d, int64_t* t_out, uint8_t* accept,
                           size_t B) {
  return host_form<kSlabsOpenRecover>(c, B, rzk_open_recover_batch_dev, z, cm, d, t_out, accept);
}
int rzk_open_recover32_batch(rzk_ctx* c, const int32_t* z, const int32_t* cm, const int32_t* d, int32_t* t_out, uint8_t* accept,
                             size_t B) {
  return host_form<kSlabsOpenRecover>(c, B, rzk_open_recover32_batch_dev, z, cm, d, t_out, accept);
}

// ---- LinearProof at either width --------------------------------------------------------------------------------------
int rzk_linear_commit_batch(rzk_ctx* c, const int64_t* g, const int64_t* x, const int64_t* r, const int64_t* rp,
                            const int64_t* y, const int64_t* yp, int64_t* cm, int64_t* cpm, int64_t* t, int64_t* tp,
                            int64_t* u, uint8_t* ok, size_t B) {
  return host_form<kSlabsLinearCommit>(c, B, rzk_linear_commit_batch_dev, g, x, r, rp, y, yp, cm, cpm, t, tp, u, ok);
}
int rzk_linear_commit32_batch(rzk_ctx* c, const int32_t* g, const int32_t* x, const int32_t* r, const int32_t* rp,
                              const int32_t* y, const int32_t* yp, int32_t* cm, int32_t* cpm, int32_t* t, int32_t* tp,
                              int32_t* u, uint8_t* ok, size_t B) {
  return host_form<kSlabsLinearCommit>(c, B, rzk_linear_commit32_batch_dev, g, x, r, rp, y, yp, cm, cpm, t, tp, u, ok);
}
int rzk_linear_mask_batch(rzk_ctx* c, const int64_t* g, const int64_t* y, const int64_t* yp, int64_t* t, int64_t* tp, int64_t* u,
                          size_t B) {
  return host_form<kSlabsLinearMask>(c, B, rzk_linear_mask_batch_dev, g, y, yp, t, tp, u);
}
int rzk_linear_mask32_batch(rzk_ctx* c, const int32_t* g, const int32_t* y, const int32_t* yp, int32_t* t, int32_t* tp, int32_t* u,
                            size_t B) {
  return host_form<kSlabsLinearMask>(c, B, rzk_linear_mask32_batch_dev, g, y, yp, t, tp, u);
}

int rzk_sum_mask_batch(rzk_ctx* c, uint32_t V, const int64_t* gs, const int64_t* ys, const int64_t* yp, int64_t* ts, int64_t* tp,
                       int64_t* u, size_t B) {
  return host_form<kSlabsSumMask>(c, by_V(V), B, V, rzk_sum_mask_batch_dev, gs, ys, yp, ts, tp, u);
}

int rzk_linear_response_batch(rzk_ctx* c, const int64_t* y, const int64_t* yp, const int64_t* r, const int64_t* rp,
                              const int64_t* d, int64_t* z, int64_t* zp, size_t B) {
  return host_form<kSlabsLinearResponse>(c, B, rzk_linear_response_batch_dev, y, yp, r, rp, d, z, zp);
}
int rzk_linear_response32_batch(rzk_ctx* c, const int32_t* y, const int32_t* yp, const int32_t* r, const int32_t* rp,
                                const int32_t* d, int32_t* z, int32_t* zp, size_t B) {
  return host_form<kSlabsLinearResponse>(c, B, rzk_linear_response32_batch_dev, y, yp, r, rp, d, z, zp);
}
int rzk_linear_verify_batch(rzk_ctx* c, const int64_t* z, const int64_t* zp, const int64_t* cm, const int64_t* cpm,
                            const int64_t* g, const int64_t* t, const int64_t* tp, const int64_t* u, const int64_t* d,
                            uint8_t* accept, size_t B) {
  return host_form<kSlabsLinearVerify>(c, B, rzk_linear_verify_batch_dev, z, zp, cm, cpm, g, t, tp, u, d, accept);
}
int rzk_linear_verify32_batch(rzk_ctx* c, const int32_t* z, const int32_t* zp, const int32_t* cm, const int32_t* cpm,
                              const int32_t* g, const int32_t* t, const int32_t* tp, const int32_t* u, const int32_t* d,
                              uint8_t* accept, size_t B) {
  return host_form<kSlabsLinearVerify>(c, B, rzk_linear_verify32_batch_dev, z, zp, cm, cpm, g, t, tp, u, d, accept);
}

int rzk_sum_commit_batch(rzk_ctx* c, uint32_t V, const int64_t* gs, const int64_t* xs, const int64_t* rs,
                         const int64_t* rp, const int64_t* ys, const int64_t* yp, int64_t* cs, int64_t* cpm,
                         int64_t* ts, int64_t* tp, int64_t* u, uint8_t* ok, size_t B) {
  return host_form<kSlabsSumCommit>(c, by_V(V), B, V, rzk_sum_commit_batch_dev, gs, xs, rs, rp, ys, yp, cs, cpm, ts, tp, u, ok);
}

int rzk_sum_response_batch(rzk_ctx* c, uint32_t V, const int64_t* ys, const int64_t* yp, const int64_t* rs,
                           const int64_t* rp, const int64_t* d, int64_t* zs, int64_t* zp, size_t B) {
  return host_form<kSlabsSumResponse>(c, by_V(V), B, V, rzk_sum_response_batch_dev, ys, yp, rs, rp, d, zs, zp);
}

int rzk_sum_verify_batch(rzk_ctx* c, uint32_t V, const int64_t* zs, const int64_t* zp, const int64_t* cs,
                         const int64_t* cpm, const int64_t* gs, const int64_t* ts, const int64_t* tp, const int64_t* u,
                         const int64_t* d, uint8_t* accept, size_t B) {
  return host_form<kSlabsSumVerify>(c, by_V(V), B, V, rzk_sum_verify_batch_dev, zs, zp, cs, cpm, gs, ts, tp, u, d, accept);
}

// ---- recompute steps of the short proofs ---------------------------------------------------------------------------
int rzk_linear_recover_batch(rzk_ctx* c, const int64_t* z, const int64_t* zp, const int64_t* cm, const int64_t* cpm,
                             const int64_t* g, const int64_t* d, int64_t* t_out, int64_t* tp_out, int64_t* u_out,
                             uint8_t* accept, size_t B) {
  return host_form<kSlabsLinearRecover>(c, B, rzk_linear_recover_batch_dev, z, zp, cm, cpm, g, d, t_out, tp_out, u_out, accept);
}
int rzk_linear_recover32_batch(rzk_ctx* c, const int32_t* z, const int32_t* zp, const int32_t* cm, const int32_t* cpm,
                               const int32_t* g, const int32_t* d, int32_t* t_out, int32_t* tp_out, int32_t* u_out,
                               uint8_t* accept, size_t B) {
  return host_form<kSlabsLinearRecover>(c, B, rzk_linear_recover32_batch_dev, z, zp, cm, cpm, g, d, t_out, tp_out, u_out, accept);
}

int rzk_sum_recover_batch(rzk_ctx* c, uint32_t V, const int64_t* zs, const int64_t* zp, const int64_t* cs,
                          const int64_t* cpm, const int64_t* gs, const int64_t* d, int64_t* ts_out, int64_t* tp_out,
                          int64_t* u_out, uint8_t* accept, size_t B) {
  return host_form<kSlabsSumRecover>(c, by_V(V), B, V, rzk_sum_recover_batch_dev, zs, zp, cs, cpm, gs, d, ts_out, tp_out, u_out, accept);
}

}  // extern "C"
