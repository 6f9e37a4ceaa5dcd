// rzk_group.h - row_group_kernel, row_block_kernel and the shared-operand pair fwd_slots_kernel / row_slots_kernel.
// Part of the one translation unit rzk_kernels.hip (device code only; no include guards beyond #pragma once).
#pragma once
#include "rzk_unit.h"

namespace rzk {

// ---- row groups ---------------------------------------------------------------------------------------------
// One wavefront evaluates a GROUP of up to kGroupMax rows that are key products over the same operand
// list: each operand is loaded, measured and transformed once per prime and multiplied into one
// accumulator per row.  For [a1;a2].r with (n,k,l) = (4,9,4) that is 23 transforms per prime instead of 56.
// The Garner state of every row of the group lives in a per-wave global scratch line (L2 resident).
#ifndef RZK_GROUP_MIN_WAVES
#define RZK_GROUP_MIN_WAVES 1
#endif
template <int LOGN, int GM>
__global__ void __launch_bounds__(256, RZK_GROUP_MIN_WAVES)
row_group_kernel(const Program* __restrict__ prog, const Operands ops, const uint32_t* __restrict__ key_ntt,
                 const double* __restrict__ key_l2, const DevTables* __restrict__ Tp,
                 const uint32_t* __restrict__ tw_all, uint32_t* __restrict__ scratch, uint8_t* __restrict__ flags,
                 const uint32_t ntasks) {
  using G = Geo<LOGN>;
  constexpr int E = G::E;
  constexpr int N = G::N;
  static_assert(GM >= 1 && GM <= kGroupMax, "group size");
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int lane = threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint32_t* lds = smem + wave * G::LDS_WORDS;
  uint32_t* st = scratch + ((size_t)blockIdx.x * 4 + wave) * (size_t)(2 * kGroupMax) * N;   // [g][A|B][N]
  const DevTables& T = *Tp;
  const uint32_t ngroups = prog->ngroups;

  for (uint32_t task = blockIdx.x * 4 + wave; task < ntasks; task += gridDim.x * 4) {
    const uint32_t b = task / ngroups;
    const uint32_t gi = task - b * ngroups;
    const uint32_t bo = ops.group > 1 ? b / ops.group : b;
    const GroupDesc gd = prog->groups[gi];
    const uint32_t cnt = gd.count;
    const Row row0 = prog->rows[gd.row0];
    const uint32_t nt = row0.nterms;
    int np = kMaxPrimes;
    if (nt > 0) {
      float bound[GM];
#pragma unroll
      for (int g = 0; g < GM; ++g) bound[g] = 0.f;
#pragma unroll 1
      for (int pi = 0; pi < np; ++pi) {
        const PrimeConsts pc = T.pc[pi];
        const uint32_t* __restrict__ twf = tw_all + (size_t)(2 * pi) * kTableLen;
        const bool first = pi == 0;
        uint32_t acc[GM][E];
#pragma unroll
        for (int g = 0; g < GM; ++g)
#pragma unroll
          for (int c = 0; c < E; ++c) acc[g][c] = 0;
#pragma unroll 1
        for (uint32_t t = 0; t < nt; ++t) {
          const Term tm0 = prog->terms[row0.term0 + t];
          uint32_t x[E];
          float nb = 0.f;
          bool below = true;
          const bool chk = first && (tm0.kind & TERM_CHECK);
          int ln = lane;
          asm volatile("" : "+v"(ln));   // no hoisting of lane-dependent addresses (register budget)
          bool fault = false;
          load_lift<LOGN>(x, operand_ptr(ops, tm0.b_op, tm0.b_off, b, bo, N), ln, pc, first, nb, chk, ops.norm_limit, below,
                          T.crt.qhalf, ops.trusted != 0, fault);
          if (chk && !below && lane == 0) flags[bo] = 0;
          if (fault) input_fault(ops, flags, bo, lane);
          wave_fwd<LOGN>(x, ln, lds, twf, pc);
          store_operand_image<LOGN, WaveTeam>(x, ops, tm0.b_op, tm0.b_off, b, pi, ln, nb, first);
#pragma unroll
          for (int g = 0; g < GM; ++g) {
            if ((uint32_t)g < cnt) {
              const Term tg = prog->terms[prog->rows[gd.row0 + g].term0 + t];
              if (first) bound[g] = bound_fma((float)key_l2[tg.a_off], nb, bound[g]);
              const uint4* __restrict__ kp =
                  reinterpret_cast<const uint4*>(key_ntt + ((size_t)tg.a_off * kKeyImages + pi) * N);
              if (tg.sign >= 0) {   // (one wave-uniform branch per term, not a select per coefficient)
#pragma unroll
                for (int q4 = 0; q4 < E / 4; ++q4) {
                  const uint4 kv = kp[q4 * 64 + ln];
                  const uint32_t ks[4] = {kv.x, kv.y, kv.z, kv.w};
#pragma unroll
                  for (int i = 0; i < 4; ++i) acc[g][4 * q4 + i] = mac_add(acc[g][4 * q4 + i], x[4 * q4 + i], ks[i], pc);
                }
              } else {
#pragma unroll
                for (int q4 = 0; q4 < E / 4; ++q4) {
                  const uint4 kv = kp[q4 * 64 + ln];
                  const uint32_t ks[4] = {kv.x, kv.y, kv.z, kv.w};
#pragma unroll
                  for (int i = 0; i < 4; ++i) acc[g][4 * q4 + i] = mac_sub(acc[g][4 * q4 + i], x[4 * q4 + i], ks[i], pc);
                }
              }
            }
          }
        }
        if (first) {
          float mxb = bound[0];
#pragma unroll
          for (int g = 1; g < GM; ++g) mxb = bound[g] > mxb ? bound[g] : mxb;
          np = primes_for(mxb, T);
        }
        // one inverse-transform instance in a rolled loop; the row's accumulator is picked with selects so
        // that the accumulator array keeps static register indices
#pragma unroll 1
        for (uint32_t g = 0; g < cnt; ++g) {
          uint32_t w[E];
#pragma unroll
          for (int c = 0; c < E; ++c) {
            uint32_t v = acc[0][c];
#pragma unroll
            for (int gg = 1; gg < GM; ++gg) v = g == (uint32_t)gg ? acc[gg][c] : v;
            w[c] = v;
          }
          inverse_and_fold<LOGN, true>(pi, np, w, lane, lds, twf + kTableLen, pc, st + (size_t)(2 * g) * N,
                                       st + (size_t)(2 * g + 1) * N, T);
        }
      }
    }
#pragma unroll 1
    for (uint32_t g = 0; g < cnt; ++g)
      row_epilogue<LOGN>(prog, prog->rows[gd.row0 + g], ops, b, bo, lane, nt > 0, np, st + (size_t)(2 * g) * N, T, flags);
  }
}

// ---- row blocks ---------------------------------------------------------------------------------------------
// One workgroup of kBlockWaves wavefronts evaluates one block (rzk_dev.h: BlockPlan) of one proof.  Per prime:
//   phase 1  wave w transforms operands w, w+8, ... of the block and leaves them in LDS ([c][lane] order:
//            lane-consecutive words, conflict-free); the first prime also measures the operands' norms;
//   barrier; phase 2  wave w evaluates rows w, w+8, ...: multiply-accumulate from the staged transforms and the
//            resident key, inverse transform, fold into the row's Garner state (workgroup scratch in global
//            memory); barrier before the next prime overwrites the staged transforms.
// Every wave runs the same number of barriers: the prime count is the block's maximum, computed by every wave
// from the same norms in LDS (more primes than a row needs is still exact).
template <int LOGN, class TM = WaveTeam>
__global__ void __launch_bounds__(kBlockWaves << TM::LL)
row_block_kernel(const Program* __restrict__ prog, const BlockPlan* __restrict__ plan, const Operands ops,
                 const uint32_t* __restrict__ key_ntt, const double* __restrict__ key_l2,
                 const DevTables* __restrict__ Tp, const uint32_t* __restrict__ tw_all, uint32_t* __restrict__ scratch,
                 uint8_t* __restrict__ flags, const uint32_t ntasks) {
  using G = Geo<LOGN, TM::LL>;
  constexpr int E = G::E;
  constexpr int N = G::N;
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int lane = threadIdx.x & (G::LANES - 1);                                    // index inside the team
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> TM::LL);      // team of the workgroup (kBlockWaves teams)
  if constexpr (TM::LL == 7) TM::init();
  uint32_t* staged = smem;                                                     // [kBlockMaxSlots][N]
  uint32_t* lds = smem + kBlockMaxSlots * N + wave * G::LDS_WORDS;             // this wave's transposition slab
  float* norm1 = reinterpret_cast<float*>(smem + kBlockMaxSlots * N + kBlockWaves * G::LDS_WORDS);   // [slots]
  uint32_t* st = scratch + (size_t)blockIdx.x * (size_t)(2 * kBlockMaxRows) * N;   // [row][A|B][N]
  const DevTables& T = *Tp;
  const uint32_t nblocks = plan->nblocks;

  for (uint32_t task = blockIdx.x; task < ntasks; task += gridDim.x) {
    const uint32_t b = task / nblocks;
    const BlockDesc bd = plan->blk[task - b * nblocks];
    const uint32_t bo = ops.group > 1 ? b / ops.group : b;
    int np = kMaxPrimes;
#pragma unroll 1
    for (int pi = 0; pi < np; ++pi) {
      const PrimeConsts pc = T.pc[pi];
      const uint32_t* __restrict__ twf = tw_all + (size_t)(2 * pi) * kTableLen;
      const bool first = pi == 0;
      // ---- phase 1: operand transforms into LDS
#pragma unroll 1
      for (uint32_t s = wave; s < bd.nslots; s += kBlockWaves) {
        const uint32_t gs = bd.slot0 + s;
        uint32_t x[E];
        float nb = 0.f;
        bool below = true;
        const bool chk = first && plan->slot_check[gs] && ops.norm_limit;
        bool fault = false;
        int ln = lane;
        asm volatile("" : "+v"(ln));   // opaque lane ids: no lane-dependent addresses kept in registers across the steps
        load_lift<LOGN, TM>(x, operand_ptr(ops, plan->slot_op[gs], plan->slot_off[gs], b, bo, N), ln, pc, first, nb, chk,
                        ops.norm_limit, below, T.crt.qhalf, ops.trusted != 0, fault);
        if (chk && !below && (lane & 63) == 0) flags[bo] = 0;
        if (fault) input_fault(ops, flags, bo, lane);
        if (first && lane == 0) norm1[s] = nb;
        wave_fwd<LOGN, TM>(x, ln, lds, twf, pc);
        store_operand_image<LOGN, TM>(x, ops, plan->slot_op[gs], plan->slot_off[gs], b, pi, ln, nb, first);
        uint32_t* dst = staged + s * N + ln;
#pragma unroll
        for (int c = 0; c < E; ++c) dst[c * G::LANES] = x[c];
      }
      __syncthreads();
      if (first) {
        float mx = 0.f;
#pragma unroll 1
        for (uint32_t r = 0; r < bd.nrows; ++r) {
          const Row row = prog->rows[bd.row0 + r];
          float bound = 0.f;
#pragma unroll 1
          for (uint32_t t = 0; t < row.nterms; ++t)
            bound = bound_fma((float)key_l2[prog->terms[row.term0 + t].a_off], norm1[plan->term_slot[row.term0 + t]], bound);
          mx = bound > mx ? bound : mx;
        }
        np = primes_for(mx, T);
      }
      // ---- phase 2: rows from the staged transforms
#pragma unroll 1
      for (uint32_t r = wave; r < bd.nrows; r += kBlockWaves) {
        const Row row = prog->rows[bd.row0 + r];
        if (row.nterms == 0) continue;
        uint32_t acc[E];
#pragma unroll
        for (int c = 0; c < E; ++c) acc[c] = 0;
#pragma unroll 1
        for (uint32_t t = 0; t < row.nterms; ++t) {
          const Term tm = prog->terms[row.term0 + t];
          int lm = lane;
          asm volatile("" : "+v"(lm));
          const uint32_t* __restrict__ xs = staged + (size_t)plan->term_slot[row.term0 + t] * N + lm;
          const uint4* __restrict__ kp = reinterpret_cast<const uint4*>(key_ntt + ((size_t)tm.a_off * kKeyImages + pi) * N);
          if (tm.sign >= 0) {   // (one wave-uniform branch per term, not a select per coefficient)
#pragma unroll
            for (int g = 0; g < E / 4; ++g) {
              const uint4 kv = kp[G::key4(lm, g)];
              const uint32_t ks[4] = {kv.x, kv.y, kv.z, kv.w};
#pragma unroll
              for (int i = 0; i < 4; ++i) acc[4 * g + i] = mac_add(acc[4 * g + i], xs[(4 * g + i) * G::LANES], ks[i], pc);
            }
          } else {
#pragma unroll
            for (int g = 0; g < E / 4; ++g) {
              const uint4 kv = kp[G::key4(lm, g)];
              const uint32_t ks[4] = {kv.x, kv.y, kv.z, kv.w};
#pragma unroll
              for (int i = 0; i < 4; ++i) acc[4 * g + i] = mac_sub(acc[4 * g + i], xs[(4 * g + i) * G::LANES], ks[i], pc);
            }
          }
        }
        inverse_and_fold<LOGN, true, TM>(pi, np, acc, lane, lds, twf + kTableLen, pc, st + (size_t)(2 * r) * N,
                                     st + (size_t)(2 * r + 1) * N, T);
      }
      __syncthreads();   // the staged transforms are overwritten by the next prime / next task
    }
#pragma unroll 1
    for (uint32_t r = wave; r < bd.nrows; r += kBlockWaves) {
      const Row row = prog->rows[bd.row0 + r];
      row_epilogue<LOGN, TM>(prog, row, ops, b, bo, lane, row.nterms > 0, np, st + (size_t)(2 * r) * N, T, flags);
    }
  }
}

// acc +/-= stored transform (*) (key entry | second stored transform), 16-byte accesses in the NTT-domain layout
template <int LOGN, bool VEC, bool MINUS>
__device__ __forceinline__ void slot_mac(uint32_t* acc, const uint4* __restrict__ xb, const uint4* __restrict__ other, int lane,
                                         const PrimeConsts& pc) {
  constexpr int E = Geo<LOGN>::E;
#pragma unroll
  for (int g = 0; g < E / 4; ++g) {
    const uint4 xv = xb[g * 64 + lane];
    const uint4 ov = other[g * 64 + lane];
    uint32_t xs[4] = {xv.x, xv.y, xv.z, xv.w};
    const uint32_t os[4] = {ov.x, ov.y, ov.z, ov.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      uint32_t w = os[i];
      if (VEC) {   // x_a * x_b * N^-1: two Montgomery steps (the key already carries N^-1 * R)
        xs[i] = mont_lazy(xs[i], os[i], pc.p, pc.npinv);
        w = pc.ninv_r2;
      }
      acc[4 * g + i] = MINUS ? mac_sub(acc[4 * g + i], xs[i], w, pc) : mac_add(acc[4 * g + i], xs[i], w, pc);
    }
  }
}

// ---- shared-operand path ------------------------------------------------------------------------------------
// Forward pass: one wavefront per (proof, slot) transforms the slot's polynomial for the first `np_store`
// primes into ws[((b*nslots + s)*np_store + pi)*N ...] (canonical residues, NTT-domain layout) and records
// its 1-norm / max-norm in norms[(b*nslots + s)*2 ..]; slots of a checked vector also evaluate the fused
// norm predicate.
template <int LOGN>
__global__ void __launch_bounds__(256)
fwd_slots_kernel(const SlotTable* __restrict__ slots, const Operands ops, const DevTables* __restrict__ Tp,
                 const uint32_t* __restrict__ tw_all, uint32_t* __restrict__ ws, double* __restrict__ norms,
                 uint8_t* __restrict__ flags, const uint32_t ntasks, const uint32_t np_store) {
  using G = Geo<LOGN>;
  constexpr int E = G::E;
  constexpr int N = G::N;
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int lane = threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint32_t* lds = smem + wave * G::LDS_WORDS;
  const DevTables& T = *Tp;
  const uint32_t nslots = slots->nslots;
  for (uint32_t task = blockIdx.x * 4 + wave; task < ntasks; task += gridDim.x * 4) {
    const uint32_t b = task / nslots;
    const uint32_t s = task - b * nslots;
    const uint32_t bo = ops.group > 1 ? b / ops.group : b;
    const int64_t* __restrict__ src = operand_ptr(ops, slots->op[s], slots->off[s], b, bo, N);
    int32_t v[E];
    if (ops.trusted) {
#pragma unroll
      for (int e = 0; e < E; ++e) v[e] = (int32_t)src[G::j_p1(lane, e)];
    } else {
      uint32_t in_bad = 0, in_mx = 0;
#pragma unroll
      for (int e = 0; e < E; ++e) v[e] = canon_lo_mx(src[G::j_p1(lane, e)], T.crt.qhalf, in_bad, in_mx);
      if (canon_fail(in_bad, in_mx, T.crt.qhalf)) input_fault(ops, flags, bo, lane);
    }
    const float ss = wave_sum_f32(lane_sum_sq_f32<E>(v));
    if (lane == 0) {
      norms[((size_t)b * nslots + s) * 2 + 0] = (double)norm2_upper(ss) * (1.0 + 1e-6);   // upper bound of the 2-norm (read back as float)
      norms[((size_t)b * nslots + s) * 2 + 1] = 0.0;
    }
    if (slots->check[s] && ops.norm_limit) {
      if (!norm_below<E>(v, ss, ops.norm_limit) && lane == 0) flags[bo] = 0;
    }
#pragma unroll 1
    for (uint32_t pi = 0; pi < np_store; ++pi) {
      const PrimeConsts pc = T.pc[pi];
      uint32_t x[E];
#pragma unroll
      for (int e = 0; e < E; ++e) x[e] = lift(v[e], pc);
      wave_fwd<LOGN>(x, lane, lds, tw_all + (size_t)(2 * pi) * kTableLen, pc);
      uint4* __restrict__ dst = reinterpret_cast<uint4*>(ws + (((size_t)b * nslots + s) * np_store + pi) * N);
#pragma unroll
      for (int g = 0; g < E / 4; ++g) {
        uint4 o;
        o.x = csub(csub(x[4 * g + 0], pc.twop), pc.p);
        o.y = csub(csub(x[4 * g + 1], pc.twop), pc.p);
        o.z = csub(csub(x[4 * g + 2], pc.twop), pc.p);
        o.w = csub(csub(x[4 * g + 3], pc.twop), pc.p);
        dst[g * 64 + lane] = o;
      }
    }
  }
}

// Row pass of the shared-operand path.  Work is dealt so that all rows of a proof run on workgroups
// whose ids are congruent mod 8 (one XCD under the observed round-robin placement: the proof's stored
// transforms then come from that XCD's L2; placement affects speed only, never results).
template <int LOGN>
__global__ void __launch_bounds__(256, RZK_ROW_MIN_WAVES)
row_slots_kernel(const Program* __restrict__ prog, const SlotTable* __restrict__ slots, const Operands ops,
                 const uint32_t* __restrict__ key_ntt, const double* __restrict__ key_l2,
                 const DevTables* __restrict__ Tp, const uint32_t* __restrict__ tw_all,
                 const uint32_t* __restrict__ ws, const double* __restrict__ norms, uint32_t* __restrict__ scratch,
                 uint8_t* __restrict__ flags, const uint32_t batch, const uint32_t np_store) {
  using G = Geo<LOGN>;
  constexpr int E = G::E;
  constexpr int N = G::N;
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int lane = threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint32_t* lds = smem + wave * G::LDS_WORDS;
  uint32_t* st_lds = smem + 4 * G::LDS_WORDS + wave * N;
  uint32_t* st_glb = scratch + ((size_t)blockIdx.x * 4 + wave) * N;
  const DevTables& T = *Tp;
  const uint32_t nrows = prog->nrows;
  const uint32_t nslots = slots->nslots;
  const uint32_t groups = (nrows + 3) / 4;                 // row groups (4 rows, one per wave) per proof
  // item stream of this workgroup's XCD class: proofs xcd, xcd+8, ... ; each proof contributes `groups` items
  const uint32_t xcd = blockIdx.x & 7, lane_blocks = (gridDim.x + 7 - xcd) / 8;   // workgroups in this class
  const uint32_t proofs_here = batch > xcd ? (batch - xcd + 7) / 8 : 0;
  const uint32_t items = proofs_here * groups;
  for (uint32_t item = blockIdx.x >> 3; item < items; item += lane_blocks) {
    const uint32_t b = xcd + 8 * (item / groups);
    const uint32_t rowi = (item % groups) * 4 + wave;
    if (rowi >= nrows) continue;
    const uint32_t bo = ops.group > 1 ? b / ops.group : b;
    const Row row = prog->rows[rowi];
    const bool has_terms = row.nterms > 0;
    int np = 1;
    if (has_terms) {
      const double* __restrict__ nb = norms + (size_t)b * nslots * 2;
      float bound = 0.f;
#pragma unroll 1
      for (uint32_t t = 0; t < row.nterms; ++t) {
        const Term tm = prog->terms[row.term0 + t];
        const uint32_t sb = slots->term_b[row.term0 + t];
        if ((tm.kind & TERM_KIND_MASK) == TERM_VEC) {
          const uint32_t sa = slots->term_a[row.term0 + t];
          bound = bound_fma((float)nb[2 * sa], (float)nb[2 * sb], bound);   // |a (*) b|_inf <= |a|_2 |b|_2
        } else {
          bound = bound_fma((float)key_l2[tm.a_off], (float)nb[2 * sb], bound);
        }
      }
      np = primes_for(bound, T);
#pragma unroll 1
      for (int pi = 0; pi < np; ++pi) {
        const PrimeConsts pc = T.pc[pi];
        const uint32_t* __restrict__ twf = tw_all + (size_t)(2 * pi) * kTableLen;
        uint32_t acc[E];
#pragma unroll
        for (int c = 0; c < E; ++c) acc[c] = 0;
        if ((uint32_t)pi < np_store) {
          // stored transforms: multiply-accumulate only
#pragma unroll 1
          for (uint32_t t = 0; t < row.nterms; ++t) {
            const Term tm = prog->terms[row.term0 + t];
            const uint4* __restrict__ xb = reinterpret_cast<const uint4*>(
                ws + (((size_t)b * nslots + slots->term_b[row.term0 + t]) * np_store + pi) * N);
            const bool vec = (tm.kind & TERM_KIND_MASK) == TERM_VEC;
            const uint4* __restrict__ other =
                vec ? reinterpret_cast<const uint4*>(
                          ws + (((size_t)b * nslots + slots->term_a[row.term0 + t]) * np_store + pi) * N)
                    : reinterpret_cast<const uint4*>(key_ntt + ((size_t)tm.a_off * kKeyImages + pi) * N);
            // four straight-line variants behind wave-uniform branches (a select per coefficient would evaluate both
            // the add and the subtract form)
            if (vec) {
              if (tm.sign >= 0) slot_mac<LOGN, true, false>(acc, xb, other, lane, pc);
              else slot_mac<LOGN, true, true>(acc, xb, other, lane, pc);
            } else {
              if (tm.sign >= 0) slot_mac<LOGN, false, false>(acc, xb, other, lane, pc);
              else slot_mac<LOGN, false, true>(acc, xb, other, lane, pc);
            }
          }
        } else {
          // more primes needed than were stored: transform in the wave for the missing ones
          float unused = 0.f;
#pragma unroll 1
          for (uint32_t t = 0; t < row.nterms; ++t) {
            Term tm = prog->terms[row.term0 + t];
            tm.kind &= TERM_KIND_MASK;   // norm predicate already evaluated by the forward pass
            term_direct<LOGN, true>(acc, tm, ops, b, bo, lane, lds, twf, pc, pi, key_ntt, key_l2, false, unused, flags,
                                    T.crt.qhalf);
          }
        }
        inverse_and_fold<LOGN>(pi, np, acc, lane, lds, twf + kTableLen, pc, st_lds, st_glb, T);
      }
    }
    row_epilogue<LOGN>(prog, row, ops, b, bo, lane, has_terms, np, st_lds, T, flags);
  }
}

}  // namespace rzk
