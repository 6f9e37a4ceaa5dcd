// rzk_protocols.cpp — the device-pointer entry points of the ring / Mat primitives, the commitment scheme and the Open,
// Linear and Sum proofs (include/rzk.h): each is a short sequence of row programs and norm kernels (rzk_run.cpp).
// A call names its slab list (rzk_slabs.h): its NULL test, its alignment test and its convert plan come from the list
// (slab_args, slabs_misaligned, convert_call; rzk_ctx.h), the body keeps its own rules, its routing predicate and its launches.
#include "rzk_ctx.h"

namespace {

// accept &= check_verify_constraint(z) && (a1.z == t + c1 (.) d)      (open.rs:167-173, sum.rs:262-298)
// specs: z[k], t[n], c[n+l], d.  group / batch / nflags as in run_program; preset: initialise accept.
// n == 1: one launch, the d-product is a rotation term inside the relation row.  n >= 2 (and rotations +
// row groups available): a1.z as ONE grouped launch (each z_j transformed once for the n rows, norm predicate
// fused) into `w`, then the relation rows as pure rotations (shift_row_kernel) — 18 instead of 48 transform
// units per (4,9,4) relation.
// Verifier side: non-canonical prover data clears the proof's verdict, the call itself succeeds (sticky = false).
// recover: t is an output, t = a1.z - c1 (.) d (the kRecoverVar forms of the same programs, same launches and paths);
// accept then only carries the norm predicate and the canonical-input test.
int run_a1_relation(rzk_ctx* c, const std::vector<OpSpec>& specs, int64_t* w, uint8_t* accept, uint32_t group,
                    uint64_t batch, uint64_t nflags, bool preset, bool recover = false) {
  // (at N = 2048 the first step runs as row blocks and the second as transform products)
  const bool blocks = !c->small && c->logn >= 10 && c->logn >= c->block_min_logn;
  const bool split = w && c->n >= 2 && ((shift_ok(c) && c->use_groups && c->group_max > 1) || blocks);
  const NormSpec z_norm = {specs[0].base, group * c->k, preset ? 0 : 1, 0};
  const uint32_t rv = recover ? kRecoverVar : 0u;
  if (!split)
    return run_checked(c, PG_A1_RELATION, rv, specs, accept, group, batch, nflags, c->verify_bound, preset, false, {z_norm});
  int rc = run_checked(c, PG_A1Z, 0, {specs[0], {w, c->n, 0}}, accept, group, batch, nflags, c->verify_bound, preset, false,
                       {z_norm});
  if (rc != RZK_OK) return rc;
  return run_program(c, PG_REL_ROT, rv, {{w, c->n, 0}, specs[1], specs[2], specs[3]}, accept, group, batch, 0, false);
}

// Linear's verifier, rearranged (PG_LIN_V1B / V2B): no product with g in the first program, so it runs on the unit kernel
// (and initialises the verdicts itself where one team owns a proof); e / e' live in the workspace, in the call's width.
// recover: t, tp, u are outputs (linear.rs:224-249 solved for them).
// C = int32_t: the caller has asked linear_verify_native32 — both programs have 32-bit kernels and the call prepares no
// multiplier images (they are read from 64-bit slabs).
template <class C>
int linear_rearranged(rzk_ctx* c, const C* z, const C* zp, const C* cm, const C* cpm, const C* g, const C* t, const C* tp, const C* u,
                      const C* d, uint8_t* accept, size_t B, bool recover) {
  const uint32_t n = c->n, k = c->k, l = c->l, rv = recover ? kRecoverVar : 0u;
  int rc = arena_reserve(c, c->ws, polys<C>(c, 2 * B * l));
  if (rc != RZK_OK) return rc;
  C* e = (C*)c->ws.p;
  C* ep = e + B * l * c->N;
  const std::vector<Op<C>> v1b = {{z, k, 0}, {zp, k, 0}, {t, n, 0}, {tp, n, 0}, {cm, n + l, 0}, {cpm, n + l, 0},
                                  {d, 1, 0}, {e, l, 0}, {ep, l, 0}};
  rc = run_checked(c, PG_LIN_V1B, rv, v1b, accept, 1, B, B, c->verify_bound, true, false,
                   {{z, k, 0, 0}, {zp, k, 1, 0}});
  if (rc != RZK_OK) return rc;
  if constexpr (sizeof(C) == 8) {
    rc = prepare_dkey(c, g, B, 1, l, accept, false);   // (after the verdicts exist; l rows multiply by g)
    if (rc != RZK_OK) return rc;
  }
  DkeyScope dkey_scope{c};
  return run_program<C>(c, PG_LIN_V2B, rv | dkv(c), {{e, l, 0}, {ep, l, 0}, {g, 1, 0}, {u, l, 0}}, accept, 1, B, 0, false);
}

// Every program of a Linear call on 32-bit slabs has native kernels on this context and the call would prepare no
// multiplier images (`uses` rows per multiplier, prepare_dkey): otherwise the whole call converts — one width per call.
bool linear_native32(rzk_ctx* c, uint32_t uses, std::initializer_list<std::pair<int, uint32_t>> plain) {
  if (dkey_wanted(c, uses)) return false;
  for (const auto& p : plain)
    if (!program_native32(c, p.first, p.second)) return false;
  return true;
}
bool linear_verify_native32(rzk_ctx* c, bool recover) {
  const uint32_t rv = recover ? kRecoverVar : 0u;
  return linear_native32(c, c->l, {{PG_LIN_V2B, rv}}) && checked_native32(c, PG_LIN_V1B, rv, c->verify_bound, true);
}

// Sum's verifier (sum.rs:262-319).  recover: ts, tp, u are outputs.
int sum_relations(rzk_ctx* c, uint32_t V, const int64_t* zs, const int64_t* zp, const int64_t* cs, const int64_t* cpm,
                  const int64_t* gs, const int64_t* ts, const int64_t* tp, const int64_t* u, const int64_t* d, uint8_t* accept,
                  size_t B, bool recover) {
  const uint32_t n = c->n, k = c->k, l = c->l, rv = recover ? kRecoverVar : 0u;
  const bool by_d = sum_uses_d(c, V);
  const size_t w1polys = by_d && (size_t)B * k > (size_t)B * V * l ? (size_t)B * k : (size_t)B * V * l;   // w1[B*V][l], or D[B][k]
  int rc = arena_reserve(c, c->ws, polys(c, w1polys + B * l + B * V * n));
  if (rc != RZK_OK) return rc;
  int64_t* w1 = (int64_t*)c->ws.p;
  int64_t* w2 = w1 + w1polys * c->N;
  int64_t* w0 = w2 + B * l * c->N;   // a1.z of the relation checks (n >= 2 only)
  const std::vector<OpSpec> rel_s = {{zs, k, 0}, {ts, n, 0}, {cs, n + l, 0}, {d, 1, 1}};
  const std::vector<OpSpec> rel_p = {{zp, k, 0}, {tp, n, 0}, {cpm, n + l, 0}, {d, 1, 0}};
  // sum.rs:262-271 norm predicates ride on sum.rs:278-291 (every summand; batch entries B*V, flag per proof)
  // and sum.rs:294-298
  // (the a1.z_i key products leave the transforms of z_i's a2-columns for the D rows: operand 0 of their launch)
  rc = prepare_oimg(c, B, V, 2 * l);
  if (rc != RZK_OK) return rc;
  OimgScope oimg_scope{c};
  {
    OimgProducer images_of_zs(c, 0);
    rc = run_a1_relation(c, rel_s, w0, accept, V, B * V, B, true, recover);
  }
  if (rc != RZK_OK) return rc;
  rc = run_a1_relation(c, rel_p, w0, accept, 1, B, B, false, recover);
  if (rc != RZK_OK) return rc;
  // sum.rs:301-319.  The multipliers' images are prepared AFTER the relation rows above have initialised accept: a
  // non-canonical g_i must clear the proof's verdict, and nothing presets the flags again from here on.
  rc = prepare_dkey(c, gs, B, V, 2 * l, accept, false);
  if (rc != RZK_OK) return rc;
  DkeyScope dkey_scope{c};
  // by_d: lhs = a2.(sum_i g_i(.)z_i - zp), D in w1's place, then one relation row per row of a2; else a2.z_i into w1
  rc = by_d ? run_program(c, PG_SUM_D, V | dkv(c) | oiv(c), {{zs, V * k, 0}, {gs, V, 0}, {zp, k, 0}, {w1, k, 0}}, accept, 1, B, 0, false)
            : run_program(c, PG_MATVEC, RZK_KEY_A2 * 2, {{zs, k, 0}, {nullptr, l, 0}, {w1, l, 0}}, accept, V, B * V, 0, false);
  if (rc != RZK_OK) return rc;
  rc = run_program(c, PG_SUM_W2, V | dkv(c), {{cs, V * (n + l), 0}, {gs, V, 0}, {cpm, n + l, 0}, {w2, l, 0}}, accept, 1, B, 0, false);
  if (rc != RZK_OK) return rc;
  if (by_d) return run_program(c, PG_SUM_V4, rv, {{w1, k, 0}, {w2, l, 0}, {d, 1, 0}, {u, l, 0}}, accept, 1, B, 0, false);
  return run_program(c, PG_SUM_V3, V | rv | dkv(c), {{w1, V * l, 0}, {gs, V, 0}, {zp, k, 0}, {w2, l, 0}, {d, 1, 0}, {u, l, 0}}, accept,
                     1, B, 0, false);
}

// a checked program (run_checked) runs natively on 32-bit slabs: its fused form when the call has flags, its plain form otherwise
bool native_checked(rzk_ctx* c, int id, uint32_t var, uint64_t bound, const uint8_t* flags) {
  if (!flags) return program_native32(c, id, var);
  return checked_fuses(c, id, var, bound) && program_native32(c, id, var | 1);
}

}  // namespace

namespace rzk::api {

template <class C>
int matvec_dev(rzk_ctx* c, int which, const C* v, const C* addend, C* out, size_t B) {
  if (const int rc = slab_args<kSlabsMatvec>(c, by_key(which), B, v, addend, out); rc != kGo) return rc;
  const uint32_t rows = key_row_count(which, c->n, c->l);
  const uint32_t var = (uint32_t)which * 2 + (addend ? 1 : 0);
  if constexpr (sizeof(C) == 4) {
    if (slabs_misaligned<kSlabsMatvec>(v, addend, out)) return align_fail(c);
    if (!program_native32(c, PG_MATVEC, var))
      return convert_call<kSlabsMatvec>(c, by_key(which), B, [&](auto... w) { return matvec_dev<int64_t>(c, which, w..., B); }, v, addend, out);
  }
  return run_program<C>(c, PG_MATVEC, var, {{v, c->k, 0}, {addend, rows, 0}, {out, rows, 0}}, nullptr, 1, B);
}
RZK_BOTH_WIDTHS(matvec_dev)

template <class C>
int open_commit_dev(rzk_ctx* c, const C* x, const C* r, const C* y, C* cm, C* t, uint8_t* ok, size_t B) {
  if (const int rc = slab_args<kSlabsOpenCommit>(c, {}, B, x, r, y, cm, t, ok); rc != kGo) return rc;
  auto specs = [&] {   // of the launching branches
    return std::vector<Op<C>>{{x, c->l, 0}, {r, c->k, 0}, {y, c->k, 0}, {cm, c->n + c->l, 0}, {t, c->n, 0}};
  };
  if constexpr (sizeof(C) == 4) {
    if (slabs_misaligned<kSlabsOpenCommit>(x, r, y, cm, t, ok)) return align_fail(c);
    if (native_checked(c, PG_OPEN_COMMIT, 0, c->commit_bound, ok))   // fused, or no flags: no norm kernel (they read 64-bit slabs)
      return run_checked(c, PG_OPEN_COMMIT, 0, specs(), ok, 1, B, B, c->commit_bound, true, true, {});
    return convert_call<kSlabsOpenCommit>(c, {}, B, [&](auto... w) { return open_commit_dev<int64_t>(c, w..., B); }, x, r, y, cm, t, ok);
  } else {
    // check_commit_constraint(r) (params.rs:102-108) rides on the loads of r the commit rows do anyway
    return run_checked(c, PG_OPEN_COMMIT, 0, specs(), ok, 1, B, B, c->commit_bound, true, true, {{r, c->k, 0, 0}});
  }
}
RZK_BOTH_WIDTHS(open_commit_dev)

}  // namespace rzk::api

namespace {   // the typed forms only this file's extern "C" symbols call

template <class C>
int open_response_dev(rzk_ctx* c, const C* y, const C* r, const C* d, C* z, size_t B) {
  if (const int rc = slab_args<kSlabsOpenResponse>(c, {}, B, y, r, d, z); rc != kGo) return rc;
  if constexpr (sizeof(C) == 4) {
    if (slabs_misaligned<kSlabsOpenResponse>(y, r, d, z)) return align_fail(c);
    if (!program_native32(c, PG_RESPONSE, 1))
      return convert_call<kSlabsOpenResponse>(c, {}, B, [&](auto... w) { return open_response_dev<int64_t>(c, w..., B); }, y, r, d, z);
  }
  return run_program<C>(c, PG_RESPONSE, 1, {{d, 1, 0}, {y, c->k, 0}, {r, c->k, 0}, {z, c->k, 0}}, nullptr, 1, B);
}

// open.rs:167-173 behind rzk_open_verify and, with recover, rzk_open_recover: the recompute step of the short proof, the
// verifier's launches with the commitment message t = a1.z - c1 (.) d as output (t is written).  64-bit slabs take
// run_a1_relation with its workspace; 32-bit slabs the one-launch relation at n = 1 where it runs natively (never the
// split: program_native32 is false wherever that would apply), the convert path otherwise.
template <class C>
int open_a1_relation(rzk_ctx* c, const C* z, const C* t, const C* cm, const C* d, uint8_t* accept, size_t B, bool recover) {
  const std::vector<Op<C>> specs = {{z, c->k, 0}, {t, c->n, 0}, {cm, c->n + c->l, 0}, {d, 1, 0}};
  if constexpr (sizeof(C) == 4) {   // (the caller has asked open_relation_native32)
    return run_checked(c, PG_A1_RELATION, recover ? kRecoverVar : 0u, specs, accept, 1, B, B, c->verify_bound, true, false, {});
  } else {
    int rc = arena_reserve(c, c->ws, polys(c, B * c->n));
    if (rc != RZK_OK) return rc;
    // the norm predicate on z rides on the rows that load z
    return run_a1_relation(c, specs, (int64_t*)c->ws.p, accept, 1, B, B, true, recover);
  }
}
bool open_relation_native32(rzk_ctx* c, bool recover, const uint8_t* accept) {
  return native_checked(c, PG_A1_RELATION, recover ? kRecoverVar : 0u, c->verify_bound, accept);
}

template <class C>
int open_verify_dev(rzk_ctx* c, const C* z, const C* t, const C* cm, const C* d, uint8_t* accept, size_t B) {
  if (const int rc = slab_args<kSlabsOpenVerify>(c, {}, B, z, t, cm, d, accept); rc != kGo) return rc;
  if (const int rc = split_check(c)) return rc;
  if constexpr (sizeof(C) == 4) {
    if (slabs_misaligned<kSlabsOpenVerify>(z, t, cm, d, accept)) return align_fail(c);
    if (!open_relation_native32(c, false, accept))
      return convert_call<kSlabsOpenVerify>(c, {}, B, [&](auto... w) { return open_verify_dev<int64_t>(c, w..., B); }, z, t, cm, d, accept);
  }
  return open_a1_relation<C>(c, z, t, cm, d, accept, B, false);
}

template <class C>
int open_recover_dev(rzk_ctx* c, const C* z, const C* cm, const C* d, C* t_out, uint8_t* accept, size_t B) {
  if (const int rc = slab_args<kSlabsOpenRecover>(c, {}, B, z, cm, d, t_out, accept); rc != kGo) return rc;
  if (const int rc = split_check(c)) return rc;
  if constexpr (sizeof(C) == 4) {
    if (slabs_misaligned<kSlabsOpenRecover>(z, cm, d, t_out, accept)) return align_fail(c);
    if (!open_relation_native32(c, true, accept))
      return convert_call<kSlabsOpenRecover>(c, {}, B, [&](auto... w) { return open_recover_dev<int64_t>(c, w..., B); }, z, cm, d, t_out, accept);
  }
  return open_a1_relation<C>(c, z, t_out, cm, d, accept, B, true);
}

template <class C>
int norm2_le_dev(rzk_ctx* c, const C* v, uint32_t rows, uint64_t bound, uint8_t* ok, size_t B) {
  if (const int rc = slab_args<kSlabsNorm2Le>(c, by_rows(rows), B, v, ok); rc != kGo) return rc;
  if constexpr (sizeof(C) == 4) {
    if (slabs_misaligned<kSlabsNorm2Le>(v, ok)) return align_fail(c);
    if (!norm_native32(c))
      return convert_call<kSlabsNorm2Le>(c, by_rows(rows), B, [&](const int64_t* w, uint8_t* flags) {
        return norm2_le_dev<int64_t>(c, w, rows, bound, flags, B);
      }, v, ok);
  }
  return run_norm(c, v, rows, bound, ok, B, 0, 0);
}

// ---- LinearProof (linear.rs), at either width -------------------------------------------------------------------------
// 32-bit slabs: a call is native when every program it launches is (linear_native32) and converts as a
// whole otherwise; the native calls keep gx, a2y, e, e' as int32_t in the workspace.
template <class C>
int linear_commit_dev(rzk_ctx* c, const C* g, const C* x, const C* r, const C* rp, const C* y, const C* yp, C* cm, C* cpm, C* t, C* tp,
                      C* u, uint8_t* ok, size_t B) {
  if (const int rc = slab_args<kSlabsLinearCommit>(c, {}, B, g, x, r, rp, y, yp, cm, cpm, t, tp, u, ok); rc != kGo) return rc;
  const uint32_t n = c->n, k = c->k, l = c->l;
  if constexpr (sizeof(C) == 4) {
    if (slabs_misaligned<kSlabsLinearCommit>(g, x, r, rp, y, yp, cm, cpm, t, tp, u, ok)) return align_fail(c);
    if (!(linear_native32(c, 2 * l, {{PG_CMUL, l}, {PG_LIN_U, 0}}) && checked_native32(c, PG_LIN_COMMIT2, 0, c->commit_bound, ok != nullptr)))
      return convert_call<kSlabsLinearCommit>(c, {}, B, [&](auto... w) { return linear_commit_dev<int64_t>(c, w..., B); }, g, x, r, rp, y, yp,
                                              cm, cpm, t, tp, u, ok);
  }
  int rc = arena_reserve(c, c->ws, polys<C>(c, 2 * B * l));
  if (rc != RZK_OK) return rc;
  C* gx = (C*)c->ws.p;
  C* a2y = gx + B * l * c->N;
  if constexpr (sizeof(C) == 8) {
    // the multiplier g of every proof, transformed once for the rows that multiply by it (gx, u)
    rc = prepare_dkey(c, g, B, 1, 2 * l, nullptr, true);      // l rows of gx, l rows of u
    if (rc != RZK_OK) return rc;
  }
  DkeyScope dkey_scope{c};
  // linear.rs:91-95: gx = x_i * g
  rc = run_program<C>(c, PG_CMUL, l | dkv(c), {{x, l, 0}, {g, 1, 0}, {gx, l, 0}}, nullptr, 1, B);
  if (rc != RZK_OK) return rc;
  const std::vector<Op<C>> c2 = {{x, l, 0}, {gx, l, 0}, {r, k, 0}, {rp, k, 0}, {y, k, 0}, {yp, k, 0}, {cm, n + l, 0},
                                 {cpm, n + l, 0}, {t, n, 0}, {tp, n, 0}, {a2y, l, 0}};
  // the norm predicates on r (bit 0 of ok) and rp (bit 1) ride on the commit rows when the kernel path allows; otherwise
  // bit 0: constraint(r), bit 1: constraint(rp), and the rows clear the byte on non-canonical inputs
  rc = run_checked(c, PG_LIN_COMMIT2, 0, c2, ok, 1, B, B, c->commit_bound, true, true,
                   {{r, k, 0, 0}, {rp, k, 2, 1}});
  if (rc != RZK_OK) return rc;
  return run_program<C>(c, PG_LIN_U, dkv(c), {{a2y, l, 0}, {g, 1, 0}, {yp, k, 0}, {u, l, 0}}, ok, 1, B);
}

// The y-only half of linear_commit_dev (linear.rs:118-129): the rows of PG_LIN_COMMIT2 that read y and y' alone
// (its kMaskVar form: y is transformed once for the a1 and the a2 row) and PG_LIN_U as there.  The arithmetic is exact,
// so t, tp, u are byte for byte what the commit call writes.  No verdicts: y carries no norm rule; a non-canonical
// coefficient raises the sticky word as in rzk_matvec_batch_dev.
template <class C>
int linear_mask_dev(rzk_ctx* c, const C* g, const C* y, const C* yp, C* t, C* tp, C* u, size_t B) {
  if (const int rc = slab_args<kSlabsLinearMask>(c, {}, B, g, y, yp, t, tp, u); rc != kGo) return rc;
  const uint32_t n = c->n, k = c->k, l = c->l;
  if constexpr (sizeof(C) == 4) {
    if (slabs_misaligned<kSlabsLinearMask>(g, y, yp, t, tp, u)) return align_fail(c);
    if (!linear_native32(c, l, {{PG_LIN_COMMIT2, kMaskVar}, {PG_LIN_U, 0}}))
      return convert_call<kSlabsLinearMask>(c, {}, B, [&](auto... w) { return linear_mask_dev<int64_t>(c, w..., B); }, g, y, yp, t, tp, u);
  }
  int rc = arena_reserve(c, c->ws, polys<C>(c, B * l));
  if (rc != RZK_OK) return rc;
  C* a2y = (C*)c->ws.p;
  if constexpr (sizeof(C) == 8) {
    rc = prepare_dkey(c, g, B, 1, l, nullptr, true);   // l rows of u
    if (rc != RZK_OK) return rc;
  }
  DkeyScope dkey_scope{c};
  // (operands at the places PG_LIN_COMMIT2 gives them; the masks-only form reads none of x, gx, r, rp and writes no c, cp)
  const C* const none = nullptr;
  const std::vector<Op<C>> m2 = {{none, l, 0}, {none, l, 0}, {none, k, 0}, {none, k, 0}, {y, k, 0}, {yp, k, 0},
                                 {none, n + l, 0}, {none, n + l, 0}, {t, n, 0}, {tp, n, 0}, {a2y, l, 0}};
  rc = run_program(c, PG_LIN_COMMIT2, kMaskVar, m2, nullptr, 1, B);
  if (rc != RZK_OK) return rc;
  return run_program<C>(c, PG_LIN_U, dkv(c), {{a2y, l, 0}, {g, 1, 0}, {yp, k, 0}, {u, l, 0}}, nullptr, 1, B);
}

template <class C>
int linear_response_dev(rzk_ctx* c, const C* y, const C* yp, const C* r, const C* rp, const C* d, C* z, C* zp, size_t B) {
  if (const int rc = slab_args<kSlabsLinearResponse>(c, {}, B, y, yp, r, rp, d, z, zp); rc != kGo) return rc;
  const uint32_t k = c->k;
  if constexpr (sizeof(C) == 4) {
    if (slabs_misaligned<kSlabsLinearResponse>(y, yp, r, rp, d, z, zp)) return align_fail(c);
    if (!program_native32(c, PG_RESPONSE, 2))
      return convert_call<kSlabsLinearResponse>(c, {}, B, [&](auto... w) { return linear_response_dev<int64_t>(c, w..., B); }, y, yp, r, rp, d,
                                                z, zp);
  }
  return run_program<C>(c, PG_RESPONSE, 2, {{d, 1, 0}, {y, k, 0}, {r, k, 0}, {z, k, 0}, {yp, k, 0}, {rp, k, 0}, {zp, k, 0}},
                        nullptr, 1, B);
}

template <class C>
int linear_verify_dev(rzk_ctx* c, const C* z, const C* zp, const C* cm, const C* cpm, const C* g, const C* t, const C* tp, const C* u,
                      const C* d, uint8_t* accept, size_t B) {
  if (const int rc = slab_args<kSlabsLinearVerify>(c, {}, B, z, zp, cm, cpm, g, t, tp, u, d, accept); rc != kGo) return rc;
  if (const int rc = split_check(c)) return rc;
  const bool rearranged = c->lin_e && !c->small;
  if constexpr (sizeof(C) == 4) {
    if (slabs_misaligned<kSlabsLinearVerify>(z, zp, cm, cpm, g, t, tp, u, d, accept)) return align_fail(c);
    // (RZK_LIN_E=0: the relation rows carry rotation terms inside row_kernel, which has no 32-bit form)
    if (!(rearranged && linear_verify_native32(c, false)))
      return convert_call<kSlabsLinearVerify>(c, {}, B, [&](auto... w) { return linear_verify_dev<int64_t>(c, w..., B); }, z, zp, cm, cpm, g, t,
                                              tp, u, d, accept);
    return linear_rearranged<C>(c, z, zp, cm, cpm, g, t, tp, u, d, accept, B, false);
  } else {
    if (rearranged) return linear_rearranged<C>(c, z, zp, cm, cpm, g, t, tp, u, d, accept, B, false);
    const uint32_t n = c->n, k = c->k, l = c->l;
    int rc = arena_reserve(c, c->ws, polys(c, 2 * B * l));
    if (rc != RZK_OK) return rc;
    int64_t* w1 = (int64_t*)c->ws.p;
    int64_t* w2 = w1 + B * l * c->N;
    const std::vector<OpSpec> v1 = {{z, k, 0}, {zp, k, 0}, {t, n, 0}, {tp, n, 0}, {cm, n + l, 0}, {cpm, n + l, 0},
                                    {d, 1, 0}, {g, 1, 0}, {w1, l, 0}, {w2, l, 0}};
    // The verdicts are initialised first, then the multiplier's images are prepared (a non-canonical g clears its proof's
    // verdict: nothing may preset the flags after that), then the rows.
    rc = check_launch(c, launch_fill_u8(cfg_of(c), accept, 1, B), "flag preset");
    if (rc != RZK_OK) return rc;
    rc = prepare_dkey(c, g, B, 1, 2 * l, accept, false);
    if (rc != RZK_OK) return rc;
    DkeyScope dkey_scope{c};
    // linear.rs:218-223: norm predicates on z and zp, fused into the rows that load them when possible (both AND into the
    // verdicts the fill above has set)
    rc = run_checked(c, PG_LIN_V1, dkv(c), v1, accept, 1, B, B, c->verify_bound, false, false, {{z, k, 1, 0}, {zp, k, 1, 0}});
    if (rc != RZK_OK) return rc;
    return run_program(c, PG_LIN_V2, dkv(c), {{w1, l, 0}, {w2, l, 0}, {g, 1, 0}, {d, 1, 0}, {zp, k, 0}, {u, l, 0}}, accept, 1, B, 0,
                       false);
  }
}

// The recompute step of the short proof: the verifier's launches with the commitment message as output.
template <class C>
int linear_recover_dev(rzk_ctx* c, const C* z, const C* zp, const C* cm, const C* cpm, const C* g, const C* d, C* t_out, C* tp_out,
                       C* u_out, uint8_t* accept, size_t B) {
  if (const int rc = slab_args<kSlabsLinearRecover>(c, {}, B, z, zp, cm, cpm, g, d, t_out, tp_out, u_out, accept); rc != kGo) return rc;
  if (const int rc = split_check(c)) return rc;
  if constexpr (sizeof(C) == 4) {
    if (slabs_misaligned<kSlabsLinearRecover>(z, zp, cm, cpm, g, d, t_out, tp_out, u_out, accept)) return align_fail(c);
    if (!linear_verify_native32(c, true))
      return convert_call<kSlabsLinearRecover>(c, {}, B, [&](auto... w) { return linear_recover_dev<int64_t>(c, w..., B); }, z, zp, cm, cpm, g,
                                               d, t_out, tp_out, u_out, accept);
  }
  // on every context (small rings and RZK_LIN_E=0 included): the non-rearranged pair has no recover form
  return linear_rearranged<C>(c, z, zp, cm, cpm, g, t_out, tp_out, u_out, d, accept, B, true);
}

}  // namespace

extern "C" {

// ---- ring / Mat primitives -----------------------------------------------------------------------------------------
int rzk_polymul_batch_dev(rzk_ctx* c, const int64_t* a, const int64_t* b, int64_t* out, size_t count) {
  if (const int rc = slab_args<kSlabsPolymul>(c, {}, count, a, b, out); rc != kGo) return rc;
  return run_program(c, PG_POLYMUL, 0, {{a, 1, 0}, {b, 1, 0}, {out, 1, 0}}, nullptr, 1, count);
}

int rzk_matvec_batch_dev(rzk_ctx* c, int which, const int64_t* v, const int64_t* addend, int64_t* out, size_t B) {
  return matvec_dev(c, which, v, addend, out, B);
}
int rzk_matvec32_batch_dev(rzk_ctx* c, int which, const int32_t* v, const int32_t* addend, int32_t* out, size_t B) {
  return matvec_dev(c, which, v, addend, out, B);
}

int rzk_cmul_batch_dev(rzk_ctx* c, const int64_t* m, uint32_t rows, const int64_t* p, int64_t* out, size_t B) {
  if (const int rc = slab_args<kSlabsCmul>(c, by_rows(rows), B, m, p, out); rc != kGo) return rc;
  if (rows > (uint32_t)kMaxRows) {
    // more rows than one program holds: treat every row as its own batch entry sharing p
    return run_program(c, PG_CMUL, 1, {{m, 1, 0}, {p, 1, 1}, {out, 1, 0}}, nullptr, rows, B * rows);
  }
  return run_program(c, PG_CMUL, rows, {{m, rows, 0}, {p, 1, 0}, {out, rows, 0}}, nullptr, 1, B);
}

int rzk_canonicalize_batch_dev(rzk_ctx* c, const int64_t* in, int64_t* out, size_t count) {
  if (const int rc = slab_args<kSlabsCanonicalize>(c, {}, count, in, out); rc != kGo) return rc;
  return check_launch(c, launch_canonicalize(cfg_of(c), in, out, (uint64_t)count * c->N, c->q), "canonicalize kernel");
}

int rzk_add_batch_dev(rzk_ctx* c, const int64_t* a, const int64_t* b, int64_t* out, size_t count) {
  if (const int rc = slab_args<kSlabsAdd>(c, {}, count, a, b, out); rc != kGo) return rc;
  return check_launch(c, launch_addsub(cfg_of(c), false, a, b, out, (uint64_t)count * c->N, c->dT, c->d_bad), "add kernel");
}

int rzk_sub_batch_dev(rzk_ctx* c, const int64_t* a, const int64_t* b, int64_t* out, size_t count) {
  if (const int rc = slab_args<kSlabsSub>(c, {}, count, a, b, out); rc != kGo) return rc;
  return check_launch(c, launch_addsub(cfg_of(c), true, a, b, out, (uint64_t)count * c->N, c->dT, c->d_bad), "sub kernel");
}

int rzk_norm2_le_batch_dev(rzk_ctx* c, const int64_t* v, uint32_t rows, uint64_t bound, uint8_t* ok, size_t B) {
  return norm2_le_dev(c, v, rows, bound, ok, B);
}
int rzk_norm2_le32_batch_dev(rzk_ctx* c, const int32_t* v, uint32_t rows, uint64_t bound, uint8_t* ok, size_t B) {
  return norm2_le_dev(c, v, rows, bound, ok, B);
}

int rzk_eq_batch_dev(rzk_ctx* c, const int64_t* a, const int64_t* b, uint32_t rows, uint8_t* eq, size_t B) {
  if (const int rc = slab_args<kSlabsEq>(c, by_rows(rows), B, a, b, eq); rc != kGo) return rc;
  const uint32_t qh = c->hT.crt.qhalf;
  if (c->small) return check_launch(c, launch_eq_small(c->N, cfg_of(c), a, b, rows, eq, B, qh, c->d_bad), "eq kernel");
  return check_launch(c, launch_eq((int)c->logn, cfg_of(c), a, b, rows, eq, B, qh, c->d_bad), "eq kernel");
}

int rzk_ntt_forward_batch_dev(rzk_ctx* c, int prime, const uint32_t* in, uint32_t* out, size_t count) {
  if (c && count == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !in || !out || prime < 0 || prime >= kMaxPrimes) return RZK_E_ARG;
  if (c->small) return fail(c, RZK_E_UNSUPPORTED, "batched transforms need N >= 512");
  return check_launch(c, launch_ntt((int)c->logn, false, cfg_of(c), prime, in, out, count, c->dT, c->d_tw), "ntt forward");
}

int rzk_ntt_inverse_batch_dev(rzk_ctx* c, int prime, const uint32_t* in, uint32_t* out, size_t count) {
  if (c && count == 0) return RZK_OK;   // empty batch: nothing to do (pointers may be NULL)
  if (!c || !in || !out || prime < 0 || prime >= kMaxPrimes) return RZK_E_ARG;
  if (c->small) return fail(c, RZK_E_UNSUPPORTED, "batched transforms need N >= 512");
  return check_launch(c, launch_ntt((int)c->logn, true, cfg_of(c), prime, in, out, count, c->dT, c->d_tw), "ntt inverse");
}

uint32_t rzk_ntt_prime(int prime) { return prime >= 0 && prime < kMaxPrimes ? kPrimes[prime] : 0; }
uint32_t rzk_ntt_psi(int prime, uint32_t N) {
  if (prime < 0 || prime >= kMaxPrimes || N == 0 || (N & (N - 1)) || N > (uint32_t)kTableLen) return 0;
  return host::psi_for(prime, N);
}
uint32_t rzk_ntt_layout_index(uint32_t N, uint32_t j) {
  if (j >= N || N < 512) return 0xffffffffu;
  const uint32_t E = N / 64;
  const uint32_t lane = j / E, c = j % E;
  return (c >> 2) * 256 + lane * 4 + (c & 3);
}

// ---- commitment scheme ---------------------------------------------------------------------------------------------
int rzk_commit_batch_dev(rzk_ctx* c, const int64_t* x, const int64_t* r, int64_t* cm, uint8_t* ok, size_t B) {
  if (const int rc = slab_args<kSlabsCommit>(c, {}, B, x, r, cm, ok); rc != kGo) return rc;
  // unfused: the exact norm kernel sets ok, then the rows clear it again for proofs with non-canonical inputs
  return run_checked(c, PG_COMMIT, 0, {{x, c->l, 0}, {r, c->k, 0}, {cm, c->n + c->l, 0}}, ok, 1, B, B, c->commit_bound, true,
                     true, {{r, c->k, 0, 0}});
}

int rzk_commitment_verify_batch_dev(rzk_ctx* c, const int64_t* cm, const int64_t* x, const int64_t* r,
                                    const int64_t* f, uint8_t* ok, size_t B) {
  if (const int rc = slab_args<kSlabsCommitmentVerify>(c, {}, B, cm, x, r, f, ok); rc != kGo) return rc;
  const uint32_t var = f ? 2u : 0u;
  // commit.rs:183-185: the norm predicate on r rides on the rows that load r
  return run_checked(c, PG_COMMIT_VERIFY, var, {{x, c->l, 0}, {r, c->k, 0}, {cm, c->n + c->l, 0}, {f, 1, 0}}, ok, 1, B, B,
                     c->commit_bound, true, false, {{r, c->k, 0, 0}});
}

// ---- OpenProof and its recompute step, at either width (the templates above) ---------------------------------------
int rzk_open_commit_batch_dev(rzk_ctx* c, const int64_t* x, const int64_t* r, const int64_t* y, int64_t* cm, int64_t* t, uint8_t* ok,
                              size_t B) {
  return open_commit_dev(c, x, r, y, cm, t, ok, B);
}
int rzk_open_commit32_batch_dev(rzk_ctx* c, const int32_t* x, const int32_t* r, const int32_t* y, int32_t* cm, int32_t* t, uint8_t* ok,
                                size_t B) {
  return open_commit_dev(c, x, r, y, cm, t, ok, B);
}
int rzk_open_response_batch_dev(rzk_ctx* c, const int64_t* y, const int64_t* r, const int64_t* d, int64_t* z, size_t B) {
  return open_response_dev(c, y, r, d, z, B);
}
int rzk_open_response32_batch_dev(rzk_ctx* c, const int32_t* y, const int32_t* r, const int32_t* d, int32_t* z, size_t B) {
  return open_response_dev(c, y, r, d, z, B);
}
int rzk_open_verify_batch_dev(rzk_ctx* c, const int64_t* z, const int64_t* t, const int64_t* cm, const int64_t* d, uint8_t* accept,
                              size_t B) {
  return open_verify_dev(c, z, t, cm, d, accept, B);
}
int rzk_open_verify32_batch_dev(rzk_ctx* c, const int32_t* z, const int32_t* t, const int32_t* cm, const int32_t* d, uint8_t* accept,
                                size_t B) {
  return open_verify_dev(c, z, t, cm, d, accept, B);
}
int rzk_open_recover_batch_dev(rzk_ctx* c, const int64_t* z, const int64_t* cm, const int64_t* d, int64_t* t_out, uint8_t* accept,
                               size_t B) {
  return open_recover_dev(c, z, cm, d, t_out, accept, B);
}
int rzk_open_recover32_batch_dev(rzk_ctx* c, const int32_t* z, const int32_t* cm, const int32_t* d, int32_t* t_out, uint8_t* accept,
                                 size_t B) {
  return open_recover_dev(c, z, cm, d, t_out, accept, B);
}

// ---- LinearProof, at either width (the templates above) -------------------------------------------------------------
int rzk_linear_commit_batch_dev(rzk_ctx* c, const int64_t* g, const int64_t* x, const int64_t* r, const int64_t* rp,
                                const int64_t* y, const int64_t* yp, int64_t* cm, int64_t* cpm, int64_t* t,
                                int64_t* tp, int64_t* u, uint8_t* ok, size_t B) {
  return linear_commit_dev(c, g, x, r, rp, y, yp, cm, cpm, t, tp, u, ok, B);
}
int rzk_linear_commit32_batch_dev(rzk_ctx* c, const int32_t* g, const int32_t* x, const int32_t* r, const int32_t* rp,
                                  const int32_t* y, const int32_t* yp, int32_t* cm, int32_t* cpm, int32_t* t,
                                  int32_t* tp, int32_t* u, uint8_t* ok, size_t B) {
  return linear_commit_dev(c, g, x, r, rp, y, yp, cm, cpm, t, tp, u, ok, B);
}
int rzk_linear_mask_batch_dev(rzk_ctx* c, const int64_t* g, const int64_t* y, const int64_t* yp, int64_t* t, int64_t* tp,
                              int64_t* u, size_t B) {
  return linear_mask_dev(c, g, y, yp, t, tp, u, B);
}
int rzk_linear_mask32_batch_dev(rzk_ctx* c, const int32_t* g, const int32_t* y, const int32_t* yp, int32_t* t, int32_t* tp,
                                int32_t* u, size_t B) {
  return linear_mask_dev(c, g, y, yp, t, tp, u, B);
}
int rzk_linear_response_batch_dev(rzk_ctx* c, const int64_t* y, const int64_t* yp, const int64_t* r,
                                  const int64_t* rp, const int64_t* d, int64_t* z, int64_t* zp, size_t B) {
  return linear_response_dev(c, y, yp, r, rp, d, z, zp, B);
}
int rzk_linear_response32_batch_dev(rzk_ctx* c, const int32_t* y, const int32_t* yp, const int32_t* r,
                                    const int32_t* rp, const int32_t* d, int32_t* z, int32_t* zp, size_t B) {
  return linear_response_dev(c, y, yp, r, rp, d, z, zp, B);
}
int rzk_linear_verify_batch_dev(rzk_ctx* c, const int64_t* z, const int64_t* zp, const int64_t* cm,
                                const int64_t* cpm, const int64_t* g, const int64_t* t, const int64_t* tp,
                                const int64_t* u, const int64_t* d, uint8_t* accept, size_t B) {
  return linear_verify_dev(c, z, zp, cm, cpm, g, t, tp, u, d, accept, B);
}
int rzk_linear_verify32_batch_dev(rzk_ctx* c, const int32_t* z, const int32_t* zp, const int32_t* cm,
                                  const int32_t* cpm, const int32_t* g, const int32_t* t, const int32_t* tp,
                                  const int32_t* u, const int32_t* d, uint8_t* accept, size_t B) {
  return linear_verify_dev(c, z, zp, cm, cpm, g, t, tp, u, d, accept, B);
}

// ---- SumProof ------------------------------------------------------------------------------------------------------
int rzk_sum_commit_batch_dev(rzk_ctx* c, uint32_t V, const int64_t* gs, const int64_t* xs, const int64_t* rs,
                             const int64_t* rp, const int64_t* ys, const int64_t* yp, int64_t* cs, int64_t* cpm,
                             int64_t* ts, int64_t* tp, int64_t* u, uint8_t* ok, size_t B) {
  if (const int rc = slab_args<kSlabsSumCommit>(c, by_V(V), B, gs, xs, rs, rp, ys, yp, cs, cpm, ts, tp, u, ok); rc != kGo) return rc;
  const uint32_t n = c->n, k = c->k, l = c->l;
  const size_t wpolys = (size_t)B * V * l > (size_t)B * k ? (size_t)B * V * l : (size_t)B * k;   // w[B*V][l], or D[B][k]
  int rc = arena_reserve(c, c->ws, polys(c, B * l + wpolys));
  if (rc != RZK_OK) return rc;
  int64_t* xp = (int64_t*)c->ws.p;
  int64_t* w = xp + B * l * c->N;
  // sum.rs:107-115: xp = sum_i x_i (.) g_i
  // (XP runs before ok is preset: a non-canonical x_i / g_i is reported through the sticky word, and again by the
  //  later rows that load the same polynomials with the flags in place)
  // the V multipliers g_i of every proof, transformed once for all the rows that multiply by them (XP, D / U)
  rc = prepare_dkey(c, gs, B, V, 2 * l, nullptr, true);   // l rows of XP, l or (columns of a2) rows of U / D
  if (rc != RZK_OK) return rc;
  DkeyScope dkey_scope{c};
  rc = run_program(c, PG_SUM_XP, V | dkv(c), {{xs, V * l, 0}, {gs, V, 0}, {xp, l, 0}}, nullptr, 1, B);
  if (rc != RZK_OK) return rc;
  // the a1.y_i key products below leave the transforms of y_i's a2-columns for the D rows (operand 2 of the summand launch)
  rc = prepare_oimg(c, B, V, 2 * l);
  if (rc != RZK_OK) return rc;
  OimgScope oimg_scope{c};
  // ok[b] = constraint(rp_b) && all_i constraint(r_{b,i}): fused into the commit rows when possible.  Both launches run
  // the same program against the same flags, so they take the same side of run_checked; unfused, the norm kernels of
  // both vectors come in front of the first launch (the second then has none of its own and only ANDs into ok).
  // sum.rs:116 and 151: cp = commit(xp; rp), tp = a1.yp
  rc = run_checked(c, PG_OPEN_COMMIT, 0, {{xp, l, 0}, {rp, k, 0}, {yp, k, 0}, {cpm, n + l, 0}, {tp, n, 0}}, ok, 1, B, B,
                   c->commit_bound, true, true, {{rp, k, 0, 0}, {rs, V * k, 1, 0}});
  if (rc != RZK_OK) return rc;
  {   // sum.rs:117-120 and 145-148: c_i = commit(x_i; r_i), t_i = a1.y_i — the V summands are extra batch entries
    OimgProducer images_of_ys(c, 2);
    rc = run_checked(c, PG_OPEN_COMMIT, 0, {{xs, l, 0}, {rs, k, 0}, {ys, k, 0}, {cs, n + l, 0}, {ts, n, 0}}, ok, V, B * V, B,
                     c->commit_bound, false, true, {});
  }
  if (rc != RZK_OK) return rc;
  // sum.rs:154-160: u = sum_i (a2.y_i)(.)g_i - a2.yp
  if (sum_uses_d(c, V)) {   // = a2.(sum_i g_i(.)y_i - yp): D (k polynomials per proof, the columns a2 uses) lives where w would
    int64_t* D = w;
    rc = run_program(c, PG_SUM_D, V | dkv(c) | oiv(c), {{ys, V * k, 0}, {gs, V, 0}, {yp, k, 0}, {D, k, 0}}, ok, 1, B);
    if (rc != RZK_OK) return rc;
    return run_program(c, PG_MATVEC, RZK_KEY_A2 * 2, {{D, k, 0}, {nullptr, l, 0}, {u, l, 0}}, ok, 1, B);
  }
  rc = run_program(c, PG_MATVEC, RZK_KEY_A2 * 2, {{ys, k, 0}, {nullptr, l, 0}, {w, l, 0}}, nullptr, 1, B * V);
  if (rc != RZK_OK) return rc;
  return run_program(c, PG_SUM_U, V | dkv(c), {{w, V * l, 0}, {gs, V, 0}, {yp, k, 0}, {u, l, 0}}, ok, 1, B);
}

// The y-only half of rzk_sum_commit_batch_dev (sum.rs:145-160) as a composition of its programs: t' = a1.y' and
// t_i = a1.y_i as plain key products (the summands are batch entries), then u on the side of sum_uses_d the commit call
// takes.  No operand images: the a1 products here are PG_MATVEC launches, which do not produce them; exact arithmetic, so
// the bytes are the commit call's either way.
int rzk_sum_mask_batch_dev(rzk_ctx* c, uint32_t V, const int64_t* gs, const int64_t* ys, const int64_t* yp, int64_t* ts,
                           int64_t* tp, int64_t* u, size_t B) {
  if (const int rc = slab_args<kSlabsSumMask>(c, by_V(V), B, gs, ys, yp, ts, tp, u); rc != kGo) return rc;
  const uint32_t n = c->n, k = c->k, l = c->l;
  const size_t wpolys = (size_t)B * V * l > (size_t)B * k ? (size_t)B * V * l : (size_t)B * k;   // w[B*V][l], or D[B][k]
  int rc = arena_reserve(c, c->ws, polys(c, wpolys));
  if (rc != RZK_OK) return rc;
  int64_t* w = (int64_t*)c->ws.p;
  rc = prepare_dkey(c, gs, B, V, l, nullptr, true);   // l or (columns of a2) rows of U / D
  if (rc != RZK_OK) return rc;
  DkeyScope dkey_scope{c};
  rc = run_program(c, PG_MATVEC, RZK_KEY_A1 * 2, {{yp, k, 0}, {nullptr, n, 0}, {tp, n, 0}}, nullptr, 1, B);
  if (rc != RZK_OK) return rc;
  rc = run_program(c, PG_MATVEC, RZK_KEY_A1 * 2, {{ys, k, 0}, {nullptr, n, 0}, {ts, n, 0}}, nullptr, 1, B * V);
  if (rc != RZK_OK) return rc;
  if (sum_uses_d(c, V)) {
    int64_t* D = w;
    rc = run_program(c, PG_SUM_D, V | dkv(c), {{ys, V * k, 0}, {gs, V, 0}, {yp, k, 0}, {D, k, 0}}, nullptr, 1, B);
    if (rc != RZK_OK) return rc;
    return run_program(c, PG_MATVEC, RZK_KEY_A2 * 2, {{D, k, 0}, {nullptr, l, 0}, {u, l, 0}}, nullptr, 1, B);
  }
  rc = run_program(c, PG_MATVEC, RZK_KEY_A2 * 2, {{ys, k, 0}, {nullptr, l, 0}, {w, l, 0}}, nullptr, 1, B * V);
  if (rc != RZK_OK) return rc;
  return run_program(c, PG_SUM_U, V | dkv(c), {{w, V * l, 0}, {gs, V, 0}, {yp, k, 0}, {u, l, 0}}, nullptr, 1, B);
}

int rzk_sum_response_batch_dev(rzk_ctx* c, uint32_t V, const int64_t* ys, const int64_t* yp, const int64_t* rs,
                               const int64_t* rp, const int64_t* d, int64_t* zs, int64_t* zp, size_t B) {
  if (const int rc = slab_args<kSlabsSumResponse>(c, by_V(V), B, ys, yp, rs, rp, d, zs, zp); rc != kGo) return rc;
  const uint32_t k = c->k;
  // sum.rs:188-193: z_i = y_i + r_i (.) d — summands as batch entries, d shared by the V entries of a proof
  int rc = run_program(c, PG_RESPONSE, 1, {{d, 1, 1}, {ys, k, 0}, {rs, k, 0}, {zs, k, 0}}, nullptr, V, B * V);
  if (rc != RZK_OK) return rc;
  // sum.rs:195-197
  return run_program(c, PG_RESPONSE, 1, {{d, 1, 0}, {yp, k, 0}, {rp, k, 0}, {zp, k, 0}}, nullptr, 1, B);
}

int rzk_sum_verify_batch_dev(rzk_ctx* c, uint32_t V, const int64_t* zs, const int64_t* zp, const int64_t* cs,
                             const int64_t* cpm, const int64_t* gs, const int64_t* ts, const int64_t* tp,
                             const int64_t* u, const int64_t* d, uint8_t* accept, size_t B) {
  if (const int rc = slab_args<kSlabsSumVerify>(c, by_V(V), B, zs, zp, cs, cpm, gs, ts, tp, u, d, accept); rc != kGo) return rc;
  if (const int rc = split_check(c)) return rc;
  return sum_relations(c, V, zs, zp, cs, cpm, gs, ts, tp, u, d, accept, B, false);
}

// ---- recompute steps of the short proofs: the verifiers' launches with the commitment message as output --------------
int rzk_linear_recover_batch_dev(rzk_ctx* c, const int64_t* z, const int64_t* zp, const int64_t* cm, const int64_t* cpm,
                                 const int64_t* g, const int64_t* d, int64_t* t_out, int64_t* tp_out, int64_t* u_out,
                                 uint8_t* accept, size_t B) {
  return linear_recover_dev(c, z, zp, cm, cpm, g, d, t_out, tp_out, u_out, accept, B);
}
int rzk_linear_recover32_batch_dev(rzk_ctx* c, const int32_t* z, const int32_t* zp, const int32_t* cm, const int32_t* cpm,
                                   const int32_t* g, const int32_t* d, int32_t* t_out, int32_t* tp_out, int32_t* u_out,
                                   uint8_t* accept, size_t B) {
  return linear_recover_dev(c, z, zp, cm, cpm, g, d, t_out, tp_out, u_out, accept, B);
}

int rzk_sum_recover_batch_dev(rzk_ctx* c, uint32_t V, const int64_t* zs, const int64_t* zp, const int64_t* cs,
                              const int64_t* cpm, const int64_t* gs, const int64_t* d, int64_t* ts_out, int64_t* tp_out,
                              int64_t* u_out, uint8_t* accept, size_t B) {
  if (const int rc = slab_args<kSlabsSumRecover>(c, by_V(V), B, zs, zp, cs, cpm, gs, d, ts_out, tp_out, u_out, accept); rc != kGo) return rc;
  if (const int rc = split_check(c)) return rc;
  return sum_relations(c, V, zs, zp, cs, cpm, gs, ts_out, tp_out, u_out, d, accept, B, true);
}

}  // extern "C"
