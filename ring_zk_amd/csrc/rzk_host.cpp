// rzk_host.cpp — the host-pointer variants of the Mat-level operations and the three protocols (include/rzk.h): each
// stages its operands through HostCall (rzk_ctx.h) and calls the *_dev entry point of the same name.  The variants of
// the codecs, Fiat-Shamir, rejection and XOF entry points sit next to those in rzk_codec.cpp.  The calls that exist for
// int64_t and int32_t slabs are one template over the coefficient type (pin / pout stage by it).
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

// out = a (op) b over `count` polynomials: polymul, add, sub
int host_binary(rzk_ctx* c, const int64_t* a, const int64_t* b, int64_t* out, size_t count,
                int (*dev)(rzk_ctx*, const int64_t*, const int64_t*, int64_t*, size_t)) {
  if (c && count == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !a || !b || !out) return RZK_E_ARG;
  HostCall h(c);
  const auto da = h.pin(a, count), db = h.pin(b, count);
  const auto dout = h.pout(out, count);
  return h.run([&] { return dev(c, da, db, dout, count); });
}

int host_ntt(rzk_ctx* c, int prime, const uint32_t* in, uint32_t* out, size_t count,
             int (*dev)(rzk_ctx*, int, const uint32_t*, uint32_t*, size_t)) {
  if (c && count == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !in || !out) return RZK_E_ARG;
  HostCall h(c);
  const auto din = h.in(in, count * c->N * sizeof(uint32_t));
  const auto dout = h.out(out, count * c->N * sizeof(uint32_t));
  return h.run([&] { return dev(c, prime, din, dout, count); });
}

template <class C>
int matvec_host(rzk_ctx* c, int which, const C* v, const C* addend, C* out, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !v || !out || which < 0 || which > 2) return RZK_E_ARG;
  const uint32_t rows = which == RZK_KEY_A1 ? c->n : (which == RZK_KEY_A2 ? c->l : c->n + c->l);
  HostCall h(c);
  const auto dv = h.pin(v, B * c->k), dadd = h.pin(addend, B * rows);
  const auto dout = h.pout(out, B * rows);
  return h.run([&] { return matvec_dev<C>(c, which, dv, dadd, dout, B); });
}

template <class C>
int open_commit_host(rzk_ctx* c, const C* x, const C* r, const C* y, C* cm, C* t, uint8_t* ok, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !x || !r || !y || !cm || !t) return RZK_E_ARG;
  HostCall h(c);
  const auto dx = h.pin(x, B * c->l), dr = h.pin(r, B * c->k), dy = h.pin(y, B * c->k);
  const auto dcm = h.pout(cm, B * (c->n + c->l)), dt = h.pout(t, B * c->n);
  const auto dok = h.out(ok, B);
  return h.run([&] { return open_commit_dev<C>(c, dx, dr, dy, dcm, dt, dok, B); });
}

template <class C>
int open_response_host(rzk_ctx* c, const C* y, const C* r, const C* d, C* z, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !y || !r || !d || !z) return RZK_E_ARG;
  HostCall h(c);
  const auto dy = h.pin(y, B * c->k), dr = h.pin(r, B * c->k), dd = h.pin(d, B);
  const auto dz = h.pout(z, B * c->k);
  return h.run([&] { return open_response_dev<C>(c, dy, dr, dd, dz, B); });
}

template <class C>
int open_verify_host(rzk_ctx* c, const C* z, const C* t, const C* cm, const C* d, uint8_t* accept, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !z || !t || !cm || !d || !accept) return RZK_E_ARG;
  HostCall h(c);
  const auto dz = h.pin(z, B * c->k), dt = h.pin(t, B * c->n), dcm = h.pin(cm, B * (c->n + c->l)), dd = h.pin(d, B);
  const auto dacc = h.out(accept, B);
  return h.run([&] { return open_a1_relation_dev<C>(c, dz, dt, dcm, dd, dacc, B, false); });
}

template <class C>
int open_recover_host(rzk_ctx* c, const C* z, const C* cm, const C* d, C* t_out, uint8_t* accept, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !z || !cm || !d || !t_out || !accept) return RZK_E_ARG;
  HostCall h(c);
  const auto dz = h.pin(z, B * c->k), dcm = h.pin(cm, B * (c->n + c->l)), dd = h.pin(d, B);
  const auto dt = h.pout(t_out, B * c->n);
  const auto dacc = h.out(accept, B);
  return h.run([&] { return open_a1_relation_dev<C>(c, dz, dt, dcm, dd, dacc, B, true); });
}

template <class C>
int norm2_le_host(rzk_ctx* c, const C* v, uint32_t rows, uint64_t bound, uint8_t* ok, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !v || !ok || rows == 0) return RZK_E_ARG;
  HostCall h(c);
  const auto dv = h.pin(v, B * rows);
  const auto dok = h.out(ok, B);
  return h.run([&] { return norm2_le_dev<C>(c, dv, rows, bound, dok, B); });
}

template <class C>
int linear_commit_host(rzk_ctx* c, const C* g, const C* x, const C* r, const C* rp, const C* y, const C* yp, C* cm, C* cpm, C* t, C* tp,
                       C* u, uint8_t* ok, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !g || !x || !r || !rp || !y || !yp || !cm || !cpm || !t || !tp || !u) return RZK_E_ARG;
  const size_t k = c->k, n = c->n, l = c->l;
  HostCall h(c);
  const auto dg = h.pin(g, B), dx = h.pin(x, B * l), dr = h.pin(r, B * k), drp = h.pin(rp, B * k), dy = h.pin(y, B * k),
             dyp = h.pin(yp, B * k);
  const auto dcm = h.pout(cm, B * (n + l)), dcpm = h.pout(cpm, B * (n + l)), dt = h.pout(t, B * n), dtp = h.pout(tp, B * n),
             du = h.pout(u, B * l);
  const auto dok = h.out(ok, B);
  return h.run([&] { return linear_commit_dev<C>(c, dg, dx, dr, drp, dy, dyp, dcm, dcpm, dt, dtp, du, dok, B); });
}

template <class C>
int linear_mask_host(rzk_ctx* c, const C* g, const C* y, const C* yp, C* t, C* tp, C* u, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !g || !y || !yp || !t || !tp || !u) return RZK_E_ARG;
  const size_t k = c->k, n = c->n, l = c->l;
  HostCall h(c);
  const auto dg = h.pin(g, B), dy = h.pin(y, B * k), dyp = h.pin(yp, B * k);
  const auto dt = h.pout(t, B * n), dtp = h.pout(tp, B * n), du = h.pout(u, B * l);
  return h.run([&] { return linear_mask_dev<C>(c, dg, dy, dyp, dt, dtp, du, B); });
}

template <class C>
int linear_response_host(rzk_ctx* c, const C* y, const C* yp, const C* r, const C* rp, const C* d, C* z, C* zp, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !y || !yp || !r || !rp || !d || !z || !zp) return RZK_E_ARG;
  const size_t kb = B * c->k;
  HostCall h(c);
  const auto dy = h.pin(y, kb), dyp = h.pin(yp, kb), dr = h.pin(r, kb), drp = h.pin(rp, kb), dd = h.pin(d, B);
  const auto dz = h.pout(z, kb), dzp = h.pout(zp, kb);
  return h.run([&] { return linear_response_dev<C>(c, dy, dyp, dr, drp, dd, dz, dzp, B); });
}

template <class C>
int linear_verify_host(rzk_ctx* c, const C* z, const C* zp, const C* cm, const C* cpm, const C* g, const C* t, const C* tp, const C* u,
                       const C* d, uint8_t* accept, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !z || !zp || !cm || !cpm || !g || !t || !tp || !u || !d || !accept) return RZK_E_ARG;
  const size_t k = c->k, n = c->n, l = c->l;
  HostCall h(c);
  const auto dz = h.pin(z, B * k), dzp = h.pin(zp, B * k), dcm = h.pin(cm, B * (n + l)), dcpm = h.pin(cpm, B * (n + l)),
             dg = h.pin(g, B), dt = h.pin(t, B * n), dtp = h.pin(tp, B * n), du = h.pin(u, B * l), dd = h.pin(d, B);
  const auto dacc = h.out(accept, B);
  return h.run([&] { return linear_verify_dev<C>(c, dz, dzp, dcm, dcpm, dg, dt, dtp, du, dd, dacc, B); });
}

template <class C>
int linear_recover_host(rzk_ctx* c, const C* z, const C* zp, const C* cm, const C* cpm, const C* g, const C* d, C* t_out, C* tp_out,
                        C* u_out, uint8_t* accept, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !z || !zp || !cm || !cpm || !g || !d || !t_out || !tp_out || !u_out || !accept) return RZK_E_ARG;
  const size_t k = c->k, n = c->n, l = c->l;
  HostCall h(c);
  const auto dz = h.pin(z, B * k), dzp = h.pin(zp, B * k), dcm = h.pin(cm, B * (n + l)), dcpm = h.pin(cpm, B * (n + l)),
             dg = h.pin(g, B), dd = h.pin(d, B);
  const auto dt = h.pout(t_out, B * n), dtp = h.pout(tp_out, B * n), du = h.pout(u_out, B * l);
  const auto dacc = h.out(accept, B);
  return h.run([&] { return linear_recover_dev<C>(c, dz, dzp, dcm, dcpm, dg, dd, dt, dtp, du, dacc, B); });
}

}  // namespace

extern "C" {

int rzk_polymul_batch(rzk_ctx* c, const int64_t* a, const int64_t* b, int64_t* out, size_t count) {
  return host_binary(c, a, b, out, count, rzk_polymul_batch_dev);
}
int rzk_add_batch(rzk_ctx* c, const int64_t* a, const int64_t* b, int64_t* out, size_t count) {
  return host_binary(c, a, b, out, count, rzk_add_batch_dev);
}
int rzk_sub_batch(rzk_ctx* c, const int64_t* a, const int64_t* b, int64_t* out, size_t count) {
  return host_binary(c, a, b, out, count, rzk_sub_batch_dev);
}
int rzk_ntt_forward_batch(rzk_ctx* c, int prime, const uint32_t* in, uint32_t* out, size_t count) {
  return host_ntt(c, prime, in, out, count, rzk_ntt_forward_batch_dev);
}
int rzk_ntt_inverse_batch(rzk_ctx* c, int prime, const uint32_t* in, uint32_t* out, size_t count) {
  return host_ntt(c, prime, in, out, count, rzk_ntt_inverse_batch_dev);
}

int rzk_matvec_batch(rzk_ctx* c, int which, const int64_t* v, const int64_t* addend, int64_t* out, size_t B) {
  return matvec_host(c, which, v, addend, out, B);
}
int rzk_matvec32_batch(rzk_ctx* c, int which, const int32_t* v, const int32_t* addend, int32_t* out, size_t B) {
  return matvec_host(c, which, v, addend, out, B);
}

int rzk_cmul_batch(rzk_ctx* c, const int64_t* m, uint32_t rows, const int64_t* p, int64_t* out, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !m || !p || !out || rows == 0) return RZK_E_ARG;
  HostCall h(c);
  const auto dm = h.pin(m, B * rows), dp = h.pin(p, B);
  const auto dout = h.pout(out, B * rows);
  return h.run([&] { return rzk_cmul_batch_dev(c, dm, rows, dp, dout, B); });
}

int rzk_canonicalize_batch(rzk_ctx* c, const int64_t* in, int64_t* out, size_t count) {
  if (c && count == 0) return RZK_OK;
  if (!c || !in || !out) return RZK_E_ARG;
  HostCall h(c);
  const auto din = h.pin(in, count);
  const auto dout = h.pout(out, count);
  return h.run([&] { return rzk_canonicalize_batch_dev(c, din, dout, count); });
}

int rzk_norm2_le_batch(rzk_ctx* c, const int64_t* v, uint32_t rows, uint64_t bound, uint8_t* ok, size_t B) {
  return norm2_le_host(c, v, rows, bound, ok, B);
}
int rzk_norm2_le32_batch(rzk_ctx* c, const int32_t* v, uint32_t rows, uint64_t bound, uint8_t* ok, size_t B) {
  return norm2_le_host(c, v, rows, bound, ok, B);
}

int rzk_eq_batch(rzk_ctx* c, const int64_t* a, const int64_t* b, uint32_t rows, uint8_t* eq, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !a || !b || !eq || rows == 0) return RZK_E_ARG;
  HostCall h(c);
  const auto da = h.pin(a, B * rows), db = h.pin(b, B * rows);
  const auto deq = h.out(eq, B);
  return h.run([&] { return rzk_eq_batch_dev(c, da, db, rows, deq, B); });
}

int rzk_commit_batch(rzk_ctx* c, const int64_t* x, const int64_t* r, int64_t* cm, uint8_t* ok, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !x || !r || !cm) return RZK_E_ARG;
  HostCall h(c);
  const auto dx = h.pin(x, B * c->l), dr = h.pin(r, B * c->k);
  const auto dcm = h.pout(cm, B * (c->n + c->l));
  const auto dok = h.out(ok, B);
  return h.run([&] { return rzk_commit_batch_dev(c, dx, dr, dcm, dok, B); });
}

int rzk_commitment_verify_batch(rzk_ctx* c, const int64_t* cm, const int64_t* x, const int64_t* r, const int64_t* f,
                                uint8_t* ok, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !cm || !x || !r || !ok) return RZK_E_ARG;
  HostCall h(c);
  const auto dcm = h.pin(cm, B * (c->n + c->l)), dx = h.pin(x, B * c->l), dr = h.pin(r, B * c->k), df = h.pin(f, B);
  const auto dok = h.out(ok, B);
  return h.run([&] { return rzk_commitment_verify_batch_dev(c, dcm, dx, dr, df, dok, B); });
}

// ---- OpenProof and its recompute step, at either width ---------------------------------------------------------------
int rzk_open_commit_batch(rzk_ctx* c, const int64_t* x, const int64_t* r, const int64_t* y, int64_t* cm, int64_t* t, uint8_t* ok,
                          size_t B) {
  return open_commit_host(c, x, r, y, cm, t, ok, B);
}
int rzk_open_commit32_batch(rzk_ctx* c, const int32_t* x, const int32_t* r, const int32_t* y, int32_t* cm, int32_t* t, uint8_t* ok,
                            size_t B) {
  return open_commit_host(c, x, r, y, cm, t, ok, B);
}
int rzk_open_response_batch(rzk_ctx* c, const int64_t* y, const int64_t* r, const int64_t* d, int64_t* z, size_t B) {
  return open_response_host(c, y, r, d, z, B);
}
int rzk_open_response32_batch(rzk_ctx* c, const int32_t* y, const int32_t* r, const int32_t* d, int32_t* z, size_t B) {
  return open_response_host(c, y, r, d, z, B);
}
int rzk_open_verify_batch(rzk_ctx* c, const int64_t* z, const int64_t* t, const int64_t* cm, const int64_t* d, uint8_t* accept,
                          size_t B) {
  return open_verify_host(c, z, t, cm, d, accept, B);
}
int rzk_open_verify32_batch(rzk_ctx* c, const int32_t* z, const int32_t* t, const int32_t* cm, const int32_t* d, uint8_t* accept,
                            size_t B) {
  return open_verify_host(c, z, t, cm, d, accept, B);
}
int rzk_open_recover_batch(rzk_ctx* c, const int64_t* z, const int64_t* cm, const int64_t* d, int64_t* t_out, uint8_t* accept,
                           size_t B) {
  return open_recover_host(c, z, cm, d, t_out, accept, B);
}
int rzk_open_recover32_batch(rzk_ctx* c, const int32_t* z, const int32_t* cm, const int32_t* d, int32_t* t_out, uint8_t* accept,
                             size_t B) {
  return open_recover_host(c, z, cm, d, t_out, accept, B);
}

// ---- LinearProof at either width --------------------------------------------------------------------------------------
int rzk_linear_commit_batch(rzk_ctx* c, const int64_t* g, const int64_t* x, const int64_t* r, const int64_t* rp,
                            const int64_t* y, const int64_t* yp, int64_t* cm, int64_t* cpm, int64_t* t, int64_t* tp,
                            int64_t* u, uint8_t* ok, size_t B) {
  return linear_commit_host(c, g, x, r, rp, y, yp, cm, cpm, t, tp, u, ok, B);
}
int rzk_linear_commit32_batch(rzk_ctx* c, const int32_t* g, const int32_t* x, const int32_t* r, const int32_t* rp,
                              const int32_t* y, const int32_t* yp, int32_t* cm, int32_t* cpm, int32_t* t, int32_t* tp,
                              int32_t* u, uint8_t* ok, size_t B) {
  return linear_commit_host(c, g, x, r, rp, y, yp, cm, cpm, t, tp, u, ok, B);
}
int rzk_linear_mask_batch(rzk_ctx* c, const int64_t* g, const int64_t* y, const int64_t* yp, int64_t* t, int64_t* tp, int64_t* u,
                          size_t B) {
  return linear_mask_host(c, g, y, yp, t, tp, u, B);
}
int rzk_linear_mask32_batch(rzk_ctx* c, const int32_t* g, const int32_t* y, const int32_t* yp, int32_t* t, int32_t* tp, int32_t* u,
                            size_t B) {
  return linear_mask_host(c, g, y, yp, t, tp, u, B);
}

int rzk_sum_mask_batch(rzk_ctx* c, uint32_t V, const int64_t* gs, const int64_t* ys, const int64_t* yp, int64_t* ts, int64_t* tp,
                       int64_t* u, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || V == 0 || !gs || !ys || !yp || !ts || !tp || !u) return RZK_E_ARG;
  const size_t k = c->k, n = c->n, l = c->l;
  HostCall h(c);
  const auto dgs = h.pin(gs, B * V), dys = h.pin(ys, B * V * k), dyp = h.pin(yp, B * k);
  const auto dts = h.pout(ts, B * V * n), dtp = h.pout(tp, B * n), du = h.pout(u, B * l);
  return h.run([&] { return rzk_sum_mask_batch_dev(c, V, dgs, dys, dyp, dts, dtp, du, B); });
}

int rzk_linear_response_batch(rzk_ctx* c, const int64_t* y, const int64_t* yp, const int64_t* r, const int64_t* rp,
                              const int64_t* d, int64_t* z, int64_t* zp, size_t B) {
  return linear_response_host(c, y, yp, r, rp, d, z, zp, B);
}
int rzk_linear_response32_batch(rzk_ctx* c, const int32_t* y, const int32_t* yp, const int32_t* r, const int32_t* rp,
                                const int32_t* d, int32_t* z, int32_t* zp, size_t B) {
  return linear_response_host(c, y, yp, r, rp, d, z, zp, B);
}
int rzk_linear_verify_batch(rzk_ctx* c, const int64_t* z, const int64_t* zp, const int64_t* cm, const int64_t* cpm,
                            const int64_t* g, const int64_t* t, const int64_t* tp, const int64_t* u, const int64_t* d,
                            uint8_t* accept, size_t B) {
  return linear_verify_host(c, z, zp, cm, cpm, g, t, tp, u, d, accept, B);
}
int rzk_linear_verify32_batch(rzk_ctx* c, const int32_t* z, const int32_t* zp, const int32_t* cm, const int32_t* cpm,
                              const int32_t* g, const int32_t* t, const int32_t* tp, const int32_t* u, const int32_t* d,
                              uint8_t* accept, size_t B) {
  return linear_verify_host(c, z, zp, cm, cpm, g, t, tp, u, d, accept, B);
}

int rzk_sum_commit_batch(rzk_ctx* c, uint32_t V, const int64_t* gs, const int64_t* xs, const int64_t* rs,
                         const int64_t* rp, const int64_t* ys, const int64_t* yp, int64_t* cs, int64_t* cpm,
                         int64_t* ts, int64_t* tp, int64_t* u, uint8_t* ok, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || V == 0 || !gs || !xs || !rs || !rp || !ys || !yp || !cs || !cpm || !ts || !tp || !u) return RZK_E_ARG;
  const size_t k = c->k, n = c->n, l = c->l;
  HostCall h(c);
  const auto dgs = h.pin(gs, B * V), dxs = h.pin(xs, B * V * l), drs = h.pin(rs, B * V * k), drp = h.pin(rp, B * k),
             dys = h.pin(ys, B * V * k), dyp = h.pin(yp, B * k);
  const auto dcs = h.pout(cs, B * V * (n + l)), dcpm = h.pout(cpm, B * (n + l)), dts = h.pout(ts, B * V * n),
             dtp = h.pout(tp, B * n), du = h.pout(u, B * l);
  const auto dok = h.out(ok, B);
  return h.run([&] { return rzk_sum_commit_batch_dev(c, V, dgs, dxs, drs, drp, dys, dyp, dcs, dcpm, dts, dtp, du, dok, B); });
}

int rzk_sum_response_batch(rzk_ctx* c, uint32_t V, const int64_t* ys, const int64_t* yp, const int64_t* rs,
                           const int64_t* rp, const int64_t* d, int64_t* zs, int64_t* zp, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || V == 0 || !ys || !yp || !rs || !rp || !d || !zs || !zp) return RZK_E_ARG;
  const size_t k = c->k;
  HostCall h(c);
  const auto dys = h.pin(ys, B * V * k), dyp = h.pin(yp, B * k), drs = h.pin(rs, B * V * k), drp = h.pin(rp, B * k),
             dd = h.pin(d, B);
  const auto dzs = h.pout(zs, B * V * k), dzp = h.pout(zp, B * k);
  return h.run([&] { return rzk_sum_response_batch_dev(c, V, dys, dyp, drs, drp, dd, dzs, dzp, B); });
}

int rzk_sum_verify_batch(rzk_ctx* c, uint32_t V, const int64_t* zs, const int64_t* zp, const int64_t* cs,
                         const int64_t* cpm, const int64_t* gs, const int64_t* ts, const int64_t* tp, const int64_t* u,
                         const int64_t* d, uint8_t* accept, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || V == 0 || !zs || !zp || !cs || !cpm || !gs || !ts || !tp || !u || !d || !accept) return RZK_E_ARG;
  const size_t k = c->k, n = c->n, l = c->l;
  HostCall h(c);
  const auto dzs = h.pin(zs, B * V * k), dzp = h.pin(zp, B * k), dcs = h.pin(cs, B * V * (n + l)),
             dcpm = h.pin(cpm, B * (n + l)), dgs = h.pin(gs, B * V), dts = h.pin(ts, B * V * n), dtp = h.pin(tp, B * n),
             du = h.pin(u, B * l), dd = h.pin(d, B);
  const auto dacc = h.out(accept, B);
  return h.run([&] { return rzk_sum_verify_batch_dev(c, V, dzs, dzp, dcs, dcpm, dgs, dts, dtp, du, dd, dacc, B); });
}

// ---- recompute steps of the short proofs ---------------------------------------------------------------------------
int rzk_linear_recover_batch(rzk_ctx* c, const int64_t* z, const int64_t* zp, const int64_t* cm, const int64_t* cpm,
                             const int64_t* g, const int64_t* d, int64_t* t_out, int64_t* tp_out, int64_t* u_out,
                             uint8_t* accept, size_t B) {
  return linear_recover_host(c, z, zp, cm, cpm, g, d, t_out, tp_out, u_out, accept, B);
}
int rzk_linear_recover32_batch(rzk_ctx* c, const int32_t* z, const int32_t* zp, const int32_t* cm, const int32_t* cpm,
                               const int32_t* g, const int32_t* d, int32_t* t_out, int32_t* tp_out, int32_t* u_out,
                               uint8_t* accept, size_t B) {
  return linear_recover_host(c, z, zp, cm, cpm, g, d, t_out, tp_out, u_out, accept, B);
}

int rzk_sum_recover_batch(rzk_ctx* c, uint32_t V, const int64_t* zs, const int64_t* zp, const int64_t* cs,
                          const int64_t* cpm, const int64_t* gs, const int64_t* d, int64_t* ts_out, int64_t* tp_out,
                          int64_t* u_out, uint8_t* accept, size_t B) {
  if (c && B == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || V == 0 || !zs || !zp || !cs || !cpm || !gs || !d || !ts_out || !tp_out || !u_out || !accept) return RZK_E_ARG;
  const size_t k = c->k, n = c->n, l = c->l;
  HostCall h(c);
  const auto dzs = h.pin(zs, B * V * k), dzp = h.pin(zp, B * k), dcs = h.pin(cs, B * V * (n + l)),
             dcpm = h.pin(cpm, B * (n + l)), dgs = h.pin(gs, B * V), dd = h.pin(d, B);
  const auto dts = h.pout(ts_out, B * V * n), dtp = h.pout(tp_out, B * n), du = h.pout(u_out, B * l);
  const auto dacc = h.out(accept, B);
  return h.run([&] { return rzk_sum_recover_batch_dev(c, V, dzs, dzp, dcs, dcpm, dgs, dd, dts, dtp, du, dacc, B); });
}

}  // extern "C"
