// rzk_slab32.cpp — the entry points over 32-bit coefficient slabs (include/rzk.h "32-bit slabs", v14; format and routing in
// rzk_slab32.h): narrow / widen, the Open cycle and the word-for-word compare rzk_eq32_batch (§19; the hash
// and the packed codec on 32-bit slabs sit beside their 64-bit siblings in rzk_codec.cpp).  A call whose programs have native 32-bit kernels on
// this context (slab32_native) launches them on the caller's slabs; every other call converts: it widens its inputs into
// the context's grow-only arena ws32, calls its 64-bit sibling there and narrows the outputs — a completeness path, not a
// performance path.  Verdicts, fault rules and the fused norm predicate are the siblings' in both.
#include "rzk_ctx.h"

namespace {

bool misaligned(std::initializer_list<const void*> slabs) {
  uintptr_t bits = 0;
  for (const void* p : slabs) bits |= reinterpret_cast<uintptr_t>(p);
  return (bits & 15u) != 0;
}
int align_fail(rzk_ctx* c) { return fail(c, RZK_E_ARG, "slab32: device slabs must be 16-byte aligned"); }

const int64_t* as64(const int32_t* p) { return reinterpret_cast<const int64_t*>(p); }   // OpSpec / Operands carry addresses; the launch's width says what they point at

int widen_polys(rzk_ctx* c, const int32_t* in, int64_t* out, size_t count) {
  const uint64_t ncoef = (uint64_t)count * c->N;
  return run_profiled(c, ncoef * 12ull, "widen kernel", [&](const LaunchCfg& cfg) { return launch_widen(cfg, in, out, ncoef); });
}
// test: the canonical test of the 64-bit kernels, reported through the sticky word (never for the library's own outputs)
int narrow_polys(rzk_ctx* c, const int64_t* in, int32_t* out, size_t count, bool test) {
  const uint64_t ncoef = (uint64_t)count * c->N;
  return run_profiled(c, ncoef * 12ull, "narrow kernel", [&](const LaunchCfg& cfg) {
    return launch_narrow(cfg, in, out, ncoef, c->hT.crt.qhalf, test && !c->trusted ? c->d_bad : nullptr);
  });
}

// The convert path of one call: its slabs as 64-bit copies in ws32.  Declare every slab (in / out, in polynomials), then
// widen_inputs() reserves the arena and widens; after the 64-bit call, narrow_outputs().
class Convert {
 public:
  explicit Convert(rzk_ctx* c) : c_(c) {}
  size_t in(const int32_t* p, size_t count) { return add(p, nullptr, count); }
  size_t out(int32_t* p, size_t count) { return add(nullptr, p, count); }
  int64_t* at(size_t i) const { return (int64_t*)((char*)c_->ws32.p + bufs_[i].off); }
  int widen_inputs() {
    int rc = arena_reserve(c_, c_->ws32, total_);
    for (size_t i = 0; rc == RZK_OK && i < bufs_.size(); ++i)
      if (bufs_[i].in) rc = widen_polys(c_, bufs_[i].in, at(i), bufs_[i].count);
    return rc;
  }
  int narrow_outputs() {
    int rc = RZK_OK;
    for (size_t i = 0; rc == RZK_OK && i < bufs_.size(); ++i)
      if (bufs_[i].out) rc = narrow_polys(c_, at(i), bufs_[i].out, bufs_[i].count, false);
    return rc;
  }
 private:
  struct Buf {
    const int32_t* in;
    int32_t* out;
    size_t count, off;
  };
  size_t add(const int32_t* in, int32_t* out, size_t count) {
    bufs_.push_back(Buf{in, out, count, total_});
    total_ += (polys(c_, count) + 255) & ~size_t(255);
    return bufs_.size() - 1;
  }
  rzk_ctx* c_;
  std::vector<Buf> bufs_;
  size_t total_ = 0;
};

// a checked program (run_checked) runs natively: its fused form when the call has flags, its plain form otherwise
bool native_checked(rzk_ctx* c, int id, uint32_t var, uint64_t bound, const uint8_t* flags) {
  if (!flags) return program_native32(c, id, var);
  return checked_fuses(c, id, var, bound) && program_native32(c, id, var | 1);
}

// open.rs:167-173 (recover: solved for t) on 32-bit slabs; the siblings' run_a1_relation at n = 1 (native) or the siblings
int a1_relation32(rzk_ctx* c, const int32_t* z, const int32_t* t, const int32_t* cm, const int32_t* d, uint8_t* accept, size_t B,
                  bool recover) {
  if (c->n != c->l) return fail(c, RZK_E_ARG, "c1_c2 split needs n == l (reference panics in Mat::add)");
  if (misaligned({z, t, cm, d})) return align_fail(c);
  const uint32_t rv = recover ? kRecoverVar : 0u;
  if (native_checked(c, PG_A1_RELATION, rv, c->verify_bound, accept)) {
    const std::vector<OpSpec> specs = {{as64(z), c->k, 0}, {as64(t), c->n, 0}, {as64(cm), c->n + c->l, 0}, {as64(d), 1, 0}};
    return run_checked(c, PG_A1_RELATION, rv, specs, accept, 1, B, B, c->verify_bound, true, false, {}, 4);
  }
  Convert cv(c);
  const size_t iz = cv.in(z, B * c->k), icm = cv.in(cm, B * (c->n + c->l)), id = cv.in(d, B);
  const size_t it = recover ? cv.out(const_cast<int32_t*>(t), B * c->n) : cv.in(t, B * c->n);
  int rc = cv.widen_inputs();
  if (rc != RZK_OK) return rc;
  rc = recover ? rzk_open_recover_batch_dev(c, cv.at(iz), cv.at(icm), cv.at(id), cv.at(it), accept, B)
               : rzk_open_verify_batch_dev(c, cv.at(iz), cv.at(it), cv.at(icm), cv.at(id), accept, B);
  return rc != RZK_OK ? rc : cv.narrow_outputs();
}

}  // namespace

extern "C" {

int rzk_narrow_batch_dev(rzk_ctx* c, const int64_t* in, int32_t* out, size_t count) {
  if (c && count == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !in || !out) return RZK_E_ARG;
  if (misaligned({in, out})) return align_fail(c);
  return narrow_polys(c, in, out, count, true);
}

int rzk_widen_batch_dev(rzk_ctx* c, const int32_t* in, int64_t* out, size_t count) {
  if (c && count == 0) return RZK_OK;
  if (!c || !in || !out) return RZK_E_ARG;
  if (misaligned({in, out})) return align_fail(c);
  return widen_polys(c, in, out, count);
}

int rzk_open_commit32_batch_dev(rzk_ctx* c, const int32_t* x, const int32_t* r, const int32_t* y, int32_t* cm, int32_t* t,
                                uint8_t* ok, size_t B) {
  if (c && B == 0) return RZK_OK;
  if (!c || !x || !r || !y || !cm || !t) return RZK_E_ARG;
  if (misaligned({x, r, y, cm, t})) return align_fail(c);
  if (native_checked(c, PG_OPEN_COMMIT, 0, c->commit_bound, ok)) {
    const std::vector<OpSpec> specs = {{as64(x), c->l, 0}, {as64(r), c->k, 0}, {as64(y), c->k, 0}, {as64(cm), c->n + c->l, 0},
                                       {as64(t), c->n, 0}};
    return run_checked(c, PG_OPEN_COMMIT, 0, specs, ok, 1, B, B, c->commit_bound, true, true, {}, 4);
  }
  Convert cv(c);
  const size_t ix = cv.in(x, B * c->l), ir = cv.in(r, B * c->k), iy = cv.in(y, B * c->k);
  const size_t icm = cv.out(cm, B * (c->n + c->l)), it = cv.out(t, B * c->n);
  int rc = cv.widen_inputs();
  if (rc != RZK_OK) return rc;
  rc = rzk_open_commit_batch_dev(c, cv.at(ix), cv.at(ir), cv.at(iy), cv.at(icm), cv.at(it), ok, B);
  return rc != RZK_OK ? rc : cv.narrow_outputs();
}

int rzk_open_response32_batch_dev(rzk_ctx* c, const int32_t* y, const int32_t* r, const int32_t* d, int32_t* z, size_t B) {
  if (c && B == 0) return RZK_OK;
  if (!c || !y || !r || !d || !z) return RZK_E_ARG;
  if (misaligned({y, r, d, z})) return align_fail(c);
  if (program_native32(c, PG_RESPONSE, 1))
    return run_program(c, PG_RESPONSE, 1, {{as64(d), 1, 0}, {as64(y), c->k, 0}, {as64(r), c->k, 0}, {as64(z), c->k, 0}}, nullptr, 1, B, 0,
                       true, 0, 0, nullptr, 4);
  Convert cv(c);
  const size_t iy = cv.in(y, B * c->k), ir = cv.in(r, B * c->k), id = cv.in(d, B), iz = cv.out(z, B * c->k);
  int rc = cv.widen_inputs();
  if (rc != RZK_OK) return rc;
  rc = rzk_open_response_batch_dev(c, cv.at(iy), cv.at(ir), cv.at(id), cv.at(iz), B);
  return rc != RZK_OK ? rc : cv.narrow_outputs();
}

int rzk_open_verify32_batch_dev(rzk_ctx* c, const int32_t* z, const int32_t* t, const int32_t* cm, const int32_t* d,
                                uint8_t* accept, size_t B) {
  if (c && B == 0) return RZK_OK;
  if (!c || !z || !t || !cm || !d || !accept) return RZK_E_ARG;
  return a1_relation32(c, z, t, cm, d, accept, B, false);
}

int rzk_open_recover32_batch_dev(rzk_ctx* c, const int32_t* z, const int32_t* cm, const int32_t* d, int32_t* t_out,
                                 uint8_t* accept, size_t B) {
  if (c && B == 0) return RZK_OK;
  if (!c || !z || !cm || !d || !t_out || !accept) return RZK_E_ARG;
  return a1_relation32(c, z, t_out, cm, d, accept, B, true);
}

// v14, slab32 prover: a1.y of a retry and the response with its rejection test.
int rzk_matvec32_batch_dev(rzk_ctx* c, int which, const int32_t* v, const int32_t* addend, int32_t* out, size_t B) {
  if (c && B == 0) return RZK_OK;
  if (!c || !v || !out || which < 0 || which > 2) return RZK_E_ARG;
  if (misaligned({v, addend, out})) return align_fail(c);
  const uint32_t rows = which == RZK_KEY_A1 ? c->n : (which == RZK_KEY_A2 ? c->l : c->n + c->l);
  const uint32_t var = (uint32_t)which * 2 + (addend ? 1 : 0);
  if (program_native32(c, PG_MATVEC, var))
    return run_program(c, PG_MATVEC, var, {{as64(v), c->k, 0}, {as64(addend), rows, 0}, {as64(out), rows, 0}}, nullptr, 1, B, 0, true, 0, 0,
                       nullptr, 4);
  Convert cv(c);
  const size_t iv = cv.in(v, B * c->k), io = cv.out(out, B * rows);
  const size_t ia = addend ? cv.in(addend, B * rows) : 0;
  int rc = cv.widen_inputs();
  if (rc != RZK_OK) return rc;
  rc = rzk_matvec_batch_dev(c, which, cv.at(iv), addend ? cv.at(ia) : nullptr, cv.at(io), B);
  return rc != RZK_OK ? rc : cv.narrow_outputs();
}

int rzk_open_response_reject32_batch_dev(rzk_ctx* c, const int32_t* y, const int32_t* r, const int32_t* d, const int64_t* coin,
                                         uint64_t R, double lnM, int32_t* z, uint8_t* accept, int64_t* E, size_t B) {
  if (!c) return RZK_E_ARG;
  if (B == 0) return RZK_OK;
  if (!y || !r || !d || !coin || !z || !accept) return fail(c, RZK_E_ARG, "response reject: non-NULL y, r, d, coin, z, accept expected");
  if (misaligned({y, r, d, z})) return align_fail(c);
  if (program_native32(c, PG_RESPONSE, 1) && response_stat_fused(c))
    return open_response_reject_native32(c, y, r, d, coin, R, lnM, z, accept, E, B);
  Convert cv(c);
  const size_t iy = cv.in(y, B * c->k), ir = cv.in(r, B * c->k), id = cv.in(d, B), iz = cv.out(z, B * c->k);
  int rc = cv.widen_inputs();
  if (rc != RZK_OK) return rc;
  rc = rzk_open_response_reject_batch_dev(c, cv.at(iy), cv.at(ir), cv.at(id), coin, R, lnM, cv.at(iz), accept, E, B);
  return rc != RZK_OK ? rc : cv.narrow_outputs();
}

// v14, slab32 messages: the compare of the short verifier.  No range test: the verdict of the consuming
// call (rzk_open_recover32_batch) has tested what it read.
int rzk_eq32_batch_dev(rzk_ctx* c, const int32_t* a, const int32_t* b, uint32_t rows, uint8_t* eq, size_t B) {
  if (c && B == 0) return RZK_OK;
  if (!c || !a || !b || !eq) return RZK_E_ARG;
  if (rows == 0) return fail(c, RZK_E_ARG, "eq32: rows must be at least 1");
  if (misaligned({a, b})) return align_fail(c);
  const uint64_t words = (uint64_t)rows * c->N;   // a multiple of 4 (N >= 4 is a power of two)
  return run_profiled(c, (uint64_t)B * words * 8ull, "eq32 kernel",
                      [&](const LaunchCfg& cfg) { return launch_eq32(cfg, a, b, words, eq, B); });
}

// ---- host-pointer forms: staged through HostCall like every other entry point ------------------------------------------
int rzk_narrow_batch(rzk_ctx* c, const int64_t* in, int32_t* out, size_t count) {
  if (c && count == 0) return RZK_OK;
  if (!c || !in || !out) return RZK_E_ARG;
  HostCall h(c);
  const auto din = h.pin(in, count);
  const auto dout = h.out(out, polys(c, count) / 2);
  return h.run([&] { return rzk_narrow_batch_dev(c, din, dout, count); });
}

int rzk_widen_batch(rzk_ctx* c, const int32_t* in, int64_t* out, size_t count) {
  if (c && count == 0) return RZK_OK;
  if (!c || !in || !out) return RZK_E_ARG;
  HostCall h(c);
  const auto din = h.in(in, polys(c, count) / 2);
  const auto dout = h.pout(out, count);
  return h.run([&] { return rzk_widen_batch_dev(c, din, dout, count); });
}

int rzk_eq32_batch(rzk_ctx* c, const int32_t* a, const int32_t* b, uint32_t rows, uint8_t* eq, size_t B) {
  if (c && B == 0) return RZK_OK;
  if (!c || !a || !b || !eq) return RZK_E_ARG;
  HostCall h(c);
  const auto da = h.in(a, polys(c, B * rows) / 2), db = h.in(b, polys(c, B * rows) / 2);
  const auto deq = h.out(eq, B);
  return h.run([&] { return rzk_eq32_batch_dev(c, da, db, rows, deq, B); });
}

int rzk_matvec32_batch(rzk_ctx* c, int which, const int32_t* v, const int32_t* addend, int32_t* out, size_t B) {
  if (c && B == 0) return RZK_OK;
  if (!c || !v || !out || which < 0 || which > 2) return RZK_E_ARG;
  const uint32_t rows = which == RZK_KEY_A1 ? c->n : (which == RZK_KEY_A2 ? c->l : c->n + c->l);
  HostCall h(c);
  const auto dv = h.in(v, polys(c, B * c->k) / 2), da = h.in(addend, polys(c, B * rows) / 2);
  const auto dout = h.out(out, polys(c, B * rows) / 2);
  return h.run([&] { return rzk_matvec32_batch_dev(c, which, dv, da, dout, B); });
}

int rzk_open_response_reject32_batch(rzk_ctx* c, const int32_t* y, const int32_t* r, const int32_t* d, const int64_t* coin, uint64_t R,
                                     double lnM, int32_t* z, uint8_t* accept, int64_t* E, size_t B) {
  if (!c) return RZK_E_ARG;
  if (B == 0) return RZK_OK;
  if (!y || !r || !d || !coin || !z || !accept) return fail(c, RZK_E_ARG, "response reject: non-NULL y, r, d, coin, z, accept expected");
  const size_t kb = B * c->k;
  HostCall h(c);
  const auto dy = h.in(y, polys(c, kb) / 2), dr = h.in(r, polys(c, kb) / 2), dd = h.in(d, polys(c, B) / 2);
  const auto dcoin = h.in(coin, B * sizeof(int64_t));
  const auto dz = h.out(z, polys(c, kb) / 2);
  const auto daccept = h.out(accept, B);
  const auto dE = h.out(E, B * sizeof(int64_t));
  return h.run([&] { return rzk_open_response_reject32_batch_dev(c, dy, dr, dd, dcoin, R, lnM, dz, daccept, dE, B); });
}

int rzk_open_commit32_batch(rzk_ctx* c, const int32_t* x, const int32_t* r, const int32_t* y, int32_t* cm, int32_t* t, uint8_t* ok,
                            size_t B) {
  if (c && B == 0) return RZK_OK;
  if (!c || !x || !r || !y || !cm || !t) return RZK_E_ARG;
  HostCall h(c);
  const auto dx = h.in(x, polys(c, B * c->l) / 2), dr = h.in(r, polys(c, B * c->k) / 2), dy = h.in(y, polys(c, B * c->k) / 2);
  const auto dcm = h.out(cm, polys(c, B * (c->n + c->l)) / 2), dt = h.out(t, polys(c, B * c->n) / 2);
  const auto dok = h.out(ok, B);
  return h.run([&] { return rzk_open_commit32_batch_dev(c, dx, dr, dy, dcm, dt, dok, B); });
}

int rzk_open_response32_batch(rzk_ctx* c, const int32_t* y, const int32_t* r, const int32_t* d, int32_t* z, size_t B) {
  if (c && B == 0) return RZK_OK;
  if (!c || !y || !r || !d || !z) return RZK_E_ARG;
  HostCall h(c);
  const auto dy = h.in(y, polys(c, B * c->k) / 2), dr = h.in(r, polys(c, B * c->k) / 2), dd = h.in(d, polys(c, B) / 2);
  const auto dz = h.out(z, polys(c, B * c->k) / 2);
  return h.run([&] { return rzk_open_response32_batch_dev(c, dy, dr, dd, dz, B); });
}

int rzk_open_verify32_batch(rzk_ctx* c, const int32_t* z, const int32_t* t, const int32_t* cm, const int32_t* d, uint8_t* accept,
                            size_t B) {
  if (c && B == 0) return RZK_OK;
  if (!c || !z || !t || !cm || !d || !accept) return RZK_E_ARG;
  HostCall h(c);
  const auto dz = h.in(z, polys(c, B * c->k) / 2), dt = h.in(t, polys(c, B * c->n) / 2);
  const auto dcm = h.in(cm, polys(c, B * (c->n + c->l)) / 2), dd = h.in(d, polys(c, B) / 2);
  const auto dacc = h.out(accept, B);
  return h.run([&] { return rzk_open_verify32_batch_dev(c, dz, dt, dcm, dd, dacc, B); });
}

int rzk_open_recover32_batch(rzk_ctx* c, const int32_t* z, const int32_t* cm, const int32_t* d, int32_t* t_out, uint8_t* accept,
                             size_t B) {
  if (c && B == 0) return RZK_OK;
  if (!c || !z || !cm || !d || !t_out || !accept) return RZK_E_ARG;
  HostCall h(c);
  const auto dz = h.in(z, polys(c, B * c->k) / 2), dcm = h.in(cm, polys(c, B * (c->n + c->l)) / 2), dd = h.in(d, polys(c, B) / 2);
  const auto dt = h.out(t_out, polys(c, B * c->n) / 2);
  const auto dacc = h.out(accept, B);
  return h.run([&] { return rzk_open_recover32_batch_dev(c, dz, dcm, dd, dt, dacc, B); });
}

}  // extern "C"
