// rzk_slab32.cpp — what only the 32-bit slab format has (include/rzk.h "32-bit slabs", v14; format and routing in
// rzk_slab32.h): narrow / widen, the word-for-word compare rzk_eq32_batch (§19) and the convert path.  The
// entry points that exist at both widths are one body each beside their 64-bit use (rzk_protocols.cpp, rzk_samplers.cpp,
// rzk_codec.cpp, rzk_prove_loop.cpp; §22).  A 32-bit call whose programs have native 32-bit kernels on this context
// (slab32_native) launches them on the caller's slabs; every other call converts (convert_call, rzk_ctx.h): it widens its
// inputs into the context's grow-only arena ws32, runs its body on int64_t there and narrows the outputs — a completeness
// path, not a performance path.  Verdicts, fault rules and the fused norm predicate are the same in both.
// narrow, widen and eq32 name their slab lists (rzk_slabs.h) like every other call.
#include "rzk_ctx.h"

namespace {

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

}  // namespace

namespace rzk::api {

int convert_begin(rzk_ctx* c, const Conv* slabs, size_t n, int64_t** wide) {
  auto room = [&](const Conv& s) { return s.in || s.out ? (polys(c, s.count) + 255) & ~size_t(255) : size_t(0); };
  size_t total = 0;
  for (size_t i = 0; i < n; ++i) total += room(slabs[i]);
  int rc = arena_reserve(c, c->ws32, total);
  char* at = (char*)c->ws32.p;
  for (size_t i = 0; rc == RZK_OK && i < n; at += room(slabs[i]), ++i) {
    wide[i] = room(slabs[i]) ? (int64_t*)at : nullptr;
    if (slabs[i].in) rc = widen_polys(c, slabs[i].in, wide[i], slabs[i].count);
  }
  return rc;
}

int convert_end(rzk_ctx* c, const Conv* slabs, size_t n, int64_t* const* wide) {
  int rc = RZK_OK;
  for (size_t i = 0; rc == RZK_OK && i < n; ++i)
    if (slabs[i].out) rc = narrow_polys(c, wide[i], slabs[i].out, slabs[i].count, false);
  return rc;
}

}  // namespace rzk::api

extern "C" {

int rzk_narrow_batch_dev(rzk_ctx* c, const int64_t* in, int32_t* out, size_t count) {
  if (const int rc = slab_args<kSlabsNarrow>(c, {}, count, in, out); rc != kGo) return rc;
  if (slabs_misaligned<kSlabsNarrow>(in, out)) return align_fail(c);
  return narrow_polys(c, in, out, count, true);
}

int rzk_widen_batch_dev(rzk_ctx* c, const int32_t* in, int64_t* out, size_t count) {
  if (const int rc = slab_args<kSlabsWiden>(c, {}, count, in, out); rc != kGo) return rc;
  if (slabs_misaligned<kSlabsWiden>(in, out)) return align_fail(c);
  return widen_polys(c, in, out, count);
}

// v14, slab32 messages: the compare of the short verifier.  No range test: the verdict of the consuming
// call (rzk_open_recover32_batch) has tested what it read.
int rzk_eq32_batch_dev(rzk_ctx* c, const int32_t* a, const int32_t* b, uint32_t rows, uint8_t* eq, size_t B) {
  if (const int rc = slab_args<kSlabsEq32>(c, {}, B, a, b, eq); rc != kGo) return rc;
  if (rows == 0) return fail(c, RZK_E_ARG, "eq32: rows must be at least 1");
  if (slabs_misaligned<kSlabsEq32>(a, b, eq)) return align_fail(c);
  const uint64_t words = (uint64_t)rows * c->N;   // a multiple of 4 (N >= 4 is a power of two)
  return run_profiled(c, (uint64_t)B * words * 8ull, "eq32 kernel",
                      [&](const LaunchCfg& cfg) { return launch_eq32(cfg, a, b, words, eq, B); });
}

// ---- host-pointer forms: staged through HostCall like every other entry point ------------------------------------------
int rzk_narrow_batch(rzk_ctx* c, const int64_t* in, int32_t* out, size_t count) {
  return host_form<kSlabsNarrow>(c, count, rzk_narrow_batch_dev, in, out);
}

int rzk_widen_batch(rzk_ctx* c, const int32_t* in, int64_t* out, size_t count) {
  return host_form<kSlabsWiden>(c, count, rzk_widen_batch_dev, in, out);
}

int rzk_eq32_batch(rzk_ctx* c, const int32_t* a, const int32_t* b, uint32_t rows, uint8_t* eq, size_t B) {
  return host_call<kSlabsEq32>(c, SizeArgs{1, rows}, B, [&](const int32_t* da, const int32_t* db, uint8_t* deq) {
    return rzk_eq32_batch_dev(c, da, db, rows, deq, B);
  }, a, b, eq);
}

}  // extern "C"
