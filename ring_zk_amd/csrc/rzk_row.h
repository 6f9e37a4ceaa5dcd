// rzk_row.h - row_kernel and shift_row_kernel.
// Part of the one translation unit rzk_kernels.hip (device code only; no include guards beyond #pragma once).
#pragma once
#include "rzk_unit.h"

namespace rzk {

// =============================================================================================
// row_kernel: one wavefront per output row, for programs with vector x vector products (x_i (.) g_i sums, products
// with the per-proof scalars g and f: linear.rs:94,124-129, sum.rs:107-115,154-160,301-319, commit.rs:199-209).
// Such a term needs two forward transforms whose results must both be in registers for the multiplication, so the
// unit kernel's register discipline (nothing live while an operand is transformed) does not apply; what pays here is
// the running sum staying in registers across the terms and the Garner word A staying in LDS (measured against
// unit_kernel's parked sums and global state lines: 1.36 vs 1.85 ms per launch for the Sum rows at (4,9,4), V = 8).
// Primes one after the other; the first pass measures the operands (prime count, canonical test, norm marks).
// The coefficient type of the slabs comes with the team (TeamCoef, rzk_wave.h), as in unit_kernel.
// =============================================================================================
template <int LOGN, bool HAS_SHIFT, class TM = WaveTeam, bool DD = false>
__global__ void __launch_bounds__(TM::kTeamsPerBlock << TM::LL, (LOGN <= 10 || TM::LL == 7 ? 4 : 1))   // N <= 1024 and teams of two: hold the 4 waves per SIMD the LDS allows
row_kernel(const Program* __restrict__ prog, const Operands ops, const uint32_t* __restrict__ key_ntt,
           const double* __restrict__ key_l2, const DevTables* __restrict__ Tp, const uint32_t* __restrict__ tw_all,
           uint32_t* __restrict__ scratch, uint8_t* __restrict__ flags, const uint32_t ntasks) {
  using G = Geo<LOGN, TM::LL>;
  using C = typename TeamCoef<TM>::type;   // coefficient type of the slabs
  constexpr int E = G::E;
  constexpr int N = G::N;
  constexpr bool OPQ = true;   // opaque lane ids: no hoisted address registers
  constexpr int TPB = TM::kTeamsPerBlock;
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int lane = threadIdx.x & (G::LANES - 1);
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> TM::LL);
  // per team: transposition slab, then Garner word A (one per coefficient); together they also hold the 2N-word
  // image of a rotation term, which is finished before the transforms start
  uint32_t* lds = smem + wave * (G::LDS_WORDS + N);
  uint32_t* st_lds = lds + G::LDS_WORDS;
  uint32_t* st = scratch + ((size_t)blockIdx.x * TPB + wave) * (size_t)(kScratchLines * N + 16);
  uint32_t* st_glb = st;            // Garner word B, only touched when a row needs the third prime
  uint32_t* st_sh = st + 4 * N;     // sum of the row's rotation terms mod q
  const DevTables& T = *Tp;
  const uint32_t qhalf = T.crt.qhalf;
  const bool trusted = ops.trusted != 0;
  const uint32_t nrows = prog->nrows;

  // When the task stride is a multiple of the row count a team would meet the same row of the program on every trip —
  // and with it the same SIMD (wave i of a workgroup lands on SIMD i): rows of different cost (Linear's verifier: two
  // relation rows with a rotation term, a key row, a vector x vector row) then load the SIMDs unevenly.  The row index
  // is rotated by the trip count in that case (a permutation inside each batch entry).
  const uint32_t stride = gridDim.x * TPB;
  const bool rotate_rows = nrows > 1 && stride % nrows == 0;
  uint32_t trip = 0;
  for (uint32_t task = blockIdx.x * TPB + wave; task < ntasks; task += stride, ++trip) {
    const uint32_t b = task / nrows;
    uint32_t rowi = task - b * nrows;
    if (rotate_rows) {
      rowi += trip % nrows;
      rowi = rowi >= nrows ? rowi - nrows : rowi;
    }
    const uint32_t bo = ops.group > 1 ? b / ops.group : b;
    const Row row = table_load(&prog->rows[rowi]);
    const bool has_shift = HAS_SHIFT && row.nshift > 0;
    if (has_shift) {
      bool fault = false;
#pragma unroll 1
      for (uint32_t t = 0; t < row.nshift; ++t) {
        const Term tm = table_load(&prog->terms[row.term0 + row.nterms + t]);
        const C* __restrict__ pa = operand_ptr<C>(ops, tm.a_op, tm.a_off, b, bo, N);
        int32_t a[E];
        if (trusted) {
#pragma unroll
          for (int e = 0; e < E; ++e) a[e] = (int32_t)pa[G::j_p1(lane, e)];
        } else {
          uint32_t abad = 0, amx = 0;
#pragma unroll
          for (int e = 0; e < E; ++e) a[e] = canon_lo_mx(pa[G::j_p1(lane, e)], qhalf, abad, amx);
          fault = fault || canon_fail(abad, amx, qhalf);
        }
        shift_product<LOGN, false, true, TM, kShiftH, C>(st_sh, t == 0, tm.sign < 0, a, operand_ptr<C>(ops, tm.b_op, tm.b_off, b, bo, N), lane,
                                         reinterpret_cast<int32_t*>(lds), T, fault, trusted);
      }
      if (fault) input_fault(ops, flags, bo, lane);
      TM::sync();   // the image is dead: the slab and the state words may be overwritten
    }
    const bool has_terms = row.nterms > 0;
    int np = kMaxPrimes;
    if (has_terms) {
      float bound = 0.f;
#pragma unroll 1
      for (int pi = 0; pi < np; ++pi) {
        const PrimeConsts pc = T.pc[pi];
        const uint32_t* __restrict__ twf = tw_all + (size_t)(2 * pi) * kTableLen;
        const bool first = pi == 0;
        uint32_t acc[E];
#pragma unroll
        for (int c = 0; c < E; ++c) acc[c] = 0;
#pragma unroll 1
        for (uint32_t t = 0; t < row.nterms; ++t)
          term_direct<LOGN, true, OPQ, TM, DD>(acc, table_load(&prog->terms[row.term0 + t]), ops, b, bo, lane, lds, twf, pc, pi, key_ntt,
                                           key_l2, first, bound, flags, qhalf);
        if (first) np = primes_for(bound, T);
        inverse_and_fold<LOGN, OPQ, TM>(pi, np, acc, lane, lds, twf + kTableLen, pc, st_lds, st_glb, T);
      }
    }
    row_epilogue<LOGN, TM, C>(prog, row, ops, b, bo, lane, has_terms, np, st_lds, T, flags, has_shift ? st_sh : nullptr);
  }
}

// =============================================================================================
// Shift-add row kernel: rows whose products all have a SPARSE multiplier as their `a` operand — the
// challenge d (kappa coefficients +-1, src/challenge_space.rs:12-33) in z = y + r(.)d and in the d-products
// of the verifiers.  No transform at all: the wave keeps the extended image of the other operand in LDS
// (ShiftGeo, rzk_core.h) and adds one rotation per non-zero coefficient of the multiplier; the multiplier's
// coefficients stay in registers and are walked with ballot / readlane (wave-uniform control flow).
// Exact for ANY multiplier (cost ~ its number of non-zeros): sums are kept in 32 bits when the multiplier
// is +-1-valued and |d|_1 |v|_inf < 2^30, in 64 bits (v_mad_i64_i32) below 2^62, and in two 16-bit passes
// beyond that.
// =============================================================================================
#ifndef RZK_SHIFT_BYTES_WAVES
#define RZK_SHIFT_BYTES_WAVES 4   // waves per SIMD the packed-byte instantiations of shift_row_kernel are compiled and launched for (5: 96 VGPRs, spills, measured no gain)
#endif
template <int LOGN, class TM = WaveTeam>
struct ShiftCfg {   // teams per workgroup: one team's image is 8 * N bytes of LDS, 32 KiB per workgroup at most
  static constexpr int TPB = TM::LL == 6 ? 4 : 1;
  static constexpr int WORDS = ShiftGeo<LOGN, true, TM::LL>::WORDS + (TM::LL == 6 ? 0 : kShiftListWords);   // per team
};

// BYTES: terms whose operands are short enough (shift_bytes_ok: the response rows z = y + r (.) d of every parameter set)
// rotate packed bytes instead of words (shift_product_bytes); every other term takes shift_product as before.  One
// wavefront only, and the default there (so `shift_row_kernel<10, false>` IS the packed-byte kernel, in C++ as in the names
// the launcher reports); RZK_SHIFT_BYTES=0 launches shift_row_kernel<., ., WaveTeam, false>.
// The coefficient type of the slabs comes with the team (TeamCoef, rzk_wave.h), as in unit_kernel.
template <int LOGN, bool TRUSTED, class TM = WaveTeam, bool BYTES = (TM::LL == 6)>   // TRUSTED (Operands::trusted) is a template flag here: as a run-time branch around the loads
                                                         // it changed the compiler's load scheduling (79 instead of 116 VGPRs, 86 us instead of 77)
__global__ void __launch_bounds__((ShiftCfg<LOGN, TM>::TPB << TM::LL), (BYTES ? RZK_SHIFT_BYTES_WAVES : TM::LL == 6 ? 1 : 4))   // BYTES: the register budget of the waves per SIMD the LDS request allows
shift_row_kernel(const Program* __restrict__ prog, const Operands ops, const DevTables* __restrict__ Tp,
                 uint8_t* __restrict__ flags, const uint32_t ntasks) {
  using S = ShiftGeo<LOGN, true, TM::LL>;
  using C = typename TeamCoef<TM>::type;   // coefficient type of the slabs
  constexpr int E = S::E;
  constexpr int N = S::N;
  constexpr int LANES = S::LANES;
  constexpr int TPB = ShiftCfg<LOGN, TM>::TPB;
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int lane = threadIdx.x & (LANES - 1);                                              // index inside the team
  const uint32_t team = __builtin_amdgcn_readfirstlane(threadIdx.x >> TM::LL);
  int32_t* slab = reinterpret_cast<int32_t*>(smem) + team * ShiftCfg<LOGN, TM>::WORDS;
  const DevTables& T = *Tp;
  const uint32_t q = T.crt.q;
  const uint32_t nrows = prog->nrows;

  // (Tasks of several consecutive rows that keep their common multiplier — the challenge of z = y + r (.) d — in
  // registers from row to row measured no gain at N = 512 / 1024 and a loss at N = 2048: the re-reads hit in L2.)
  for (uint32_t task = blockIdx.x * TPB + team; task < ntasks; task += gridDim.x * TPB) {
    const uint32_t b = task / nrows;
    const uint32_t rowi = task - b * nrows;
    const uint32_t bo = ops.group > 1 ? b / ops.group : b;
    const Row row = prog->rows[rowi];
    const uint32_t qhalf = T.crt.qhalf;
    constexpr bool trusted = TRUSTED;
    bool fault = false;
    {
      uint32_t res[E];
#pragma unroll
      for (int i = 0; i < E; ++i) res[i] = 0;
#pragma unroll 1
      for (uint32_t t = 0; t < row.nterms; ++t) {
        const Term tm = prog->terms[row.term0 + t];
        int32_t a[E];
        uint32_t abad = 0, amx = 0;
        load_pairs<LOGN, TM::LL, C>(a, operand_ptr<C>(ops, tm.a_op, tm.a_off, b, bo, N), lane, qhalf, abad, amx, trusted);
        if (!trusted) fault = fault || canon_fail(abad, amx, qhalf);
        const C* __restrict__ pv = operand_ptr<C>(ops, tm.b_op, tm.b_off, b, bo, N);
        bool done = false;
        if constexpr (BYTES) done = shift_product_bytes<LOGN, C>(res, tm.sign < 0, a, pv, lane, slab, T, fault, trusted);
        if (!done) shift_product<LOGN, true, false, TM, kShiftH, C>(res, false, tm.sign < 0, a, pv, lane, slab, T, fault, trusted);
      }
      // The sums move to the (now idle) image, each thread's pairs in its own 8-byte slots, so that the additions and
      // the store can run as a rolled loop with few registers and four 16-byte loads in flight per addition.
      TM::sync();
      uint2* own = reinterpret_cast<uint2*>(slab) + lane;
#pragma unroll
      for (int g = 0; g < S::G; ++g) own[g * LANES] = make_uint2(res[2 * g], res[2 * g + 1]);
    }
    constexpr int GC = S::G < 4 ? S::G : 4;   // pairs per trip
    uint32_t in_bad = 0, in_mx = 0;
    int nz = 0;
#pragma unroll 1
    for (int g0 = 0; g0 < S::G; g0 += GC) {
      uint32_t r[2 * GC];
      const uint2* own = reinterpret_cast<const uint2*>(slab) + lane + g0 * LANES;
#pragma unroll
      for (int g = 0; g < GC; ++g) {
        const uint2 v = own[g * LANES];
        r[2 * g] = v.x, r[2 * g + 1] = v.y;
      }
#pragma unroll 1
      for (uint32_t ai = 0; ai < row.nadds; ++ai) {
        const AddTerm ad = prog->adds[row.add0 + ai];
        using P2 = typename CoefPair<C>::type;
        const P2* __restrict__ p =
            reinterpret_cast<const P2*>(operand_ptr<C>(ops, ad.op & ADD_OP_MASK, ad.off, b, bo, N)) + g0 * LANES + lane;
        int32_t av[2 * GC];
        if (trusted) {
#pragma unroll
          for (int g = 0; g < GC; ++g) {
            const P2 t = ld_stream(p + g * LANES);
            pair_words(t, av[2 * g], av[2 * g + 1]);
          }
        } else {
#pragma unroll
          for (int g = 0; g < GC; ++g) canon_pair(ld_stream(p + g * LANES), qhalf, in_bad, in_mx, av[2 * g], av[2 * g + 1]);
        }
        if (ad.sign >= 0) {
#pragma unroll
          for (int i = 0; i < 2 * GC; ++i) r[i] = addq(r[i], zq_from_centered(av[i], q), q);
        } else {
#pragma unroll
          for (int i = 0; i < 2 * GC; ++i) r[i] = subq(r[i], zq_from_centered(av[i], q), q);
        }
      }
      if (row.mode == MODE_STORE) {
        if constexpr (sizeof(C) == 8) {
          int4* __restrict__ dst =
              reinterpret_cast<int4*>(const_cast<C*>(operand_ptr<C>(ops, row.out_op, row.out_off, b, bo, N))) + g0 * LANES + lane;
#pragma unroll
          for (int g = 0; g < GC; ++g) {
            const int64_t c0 = center_from_zq(r[2 * g], T.crt), c1 = center_from_zq(r[2 * g + 1], T.crt);
            st_stream(dst + g * LANES, make_int4((int32_t)c0, (int32_t)(c0 >> 32), (int32_t)c1, (int32_t)(c1 >> 32)));
          }
        } else {   // the pair layout with 8-byte accesses
          int2* __restrict__ dst =
              reinterpret_cast<int2*>(const_cast<C*>(operand_ptr<C>(ops, row.out_op, row.out_off, b, bo, N))) + g0 * LANES + lane;
#pragma unroll
          for (int g = 0; g < GC; ++g)
            st_stream(dst + g * LANES, make_int2((int32_t)center_from_zq(r[2 * g], T.crt), (int32_t)center_from_zq(r[2 * g + 1], T.crt)));
        }
      } else {
#pragma unroll
        for (int i = 0; i < 2 * GC; ++i) nz |= (r[i] != 0);
      }
    }
    if (fault || canon_fail(in_bad, in_mx, qhalf)) input_fault(ops, flags, bo, lane);
    if (row.mode != MODE_STORE) {
      if (__any(nz) && (lane & 63) == 0) flags[bo] = 0;
    }
    TM::sync();   // the next task's image overwrites the slots read above
  }
}

}  // namespace rzk
