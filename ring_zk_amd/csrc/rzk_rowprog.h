// rzk_rowprog.h - building blocks of the row-program kernels: canonical-input test, load_lift, the rotation (shift) terms, term_direct, epilogues, primes_for.
// Part of the one translation unit rzk_kernels.hip (device code only; no include guards beyond #pragma once).
#pragma once
#include "rzk_slab32.h"
#include "rzk_wave.h"

namespace rzk {

// ---- canonical-input test ---------------------------------------------------------------------------------
// A coefficient at the boundary is the centred representative a ZqI64 holds (src/params.rs:122-127): an int64 in
// [-(q-1)/2, (q-1)/2].  The arithmetic below only uses the low word, so every load also proves that the word it
// drops carries no information: with h = (q-1)/2, c is canonical  <=>  (uint64)(c + h) <= q - 1.  The 64-bit add
// is one v_lshl_add_u64; its high word is OR-ed into `bad`, its low word max-ed into `mx` (or, where the 1-norm
// pass already has max |lo|, that is compared with h instead).  A kappa*2^32 + s coefficient is therefore never
// read as s: the proof's verdict flag is cleared and / or the context's sticky input-error word is set.
__device__ __forceinline__ int32_t canon_lo(int64_t c, uint32_t qhalf, uint32_t& bad) {
  bad |= (uint32_t)(((uint64_t)c + qhalf) >> 32);
  return (int32_t)c;
}
__device__ __forceinline__ int32_t canon_lo_mx(int64_t c, uint32_t qhalf, uint32_t& bad, uint32_t& mx) {
  const uint64_t s = (uint64_t)c + qhalf;
  bad |= (uint32_t)(s >> 32);
  const uint32_t lo = (uint32_t)s;
  mx = lo > mx ? lo : mx;
  return (int32_t)c;
}
// the same for a 16-byte load of two coefficients
__device__ __forceinline__ void canon_pair(const longlong2 t, uint32_t qhalf, uint32_t& bad, uint32_t& mx, int32_t& lo0,
                                           int32_t& lo1) {
  lo0 = canon_lo_mx(t.x, qhalf, bad, mx);
  lo1 = canon_lo_mx(t.y, qhalf, bad, mx);
}
// The same tests on the coefficients of a 32-bit slab (rzk_slab32.h): no high word, so `bad` stays untouched and the one
// unsigned compare of canon_fail on the max-ed word (c + h mod 2^32 <= 2h) is the whole test.
__device__ __forceinline__ int32_t canon_lo(int32_t c, uint32_t, uint32_t&) { return c; }   // (callers also test max |c| > h)
__device__ __forceinline__ int32_t canon_lo_mx(int32_t c, uint32_t qhalf, uint32_t&, uint32_t& mx) {
  const uint32_t lo = slab32_test_word(c, qhalf);
  mx = lo > mx ? lo : mx;
  return c;
}
__device__ __forceinline__ void canon_pair(const int2 t, uint32_t qhalf, uint32_t& bad, uint32_t& mx, int32_t& lo0, int32_t& lo1) {
  lo0 = canon_lo_mx(t.x, qhalf, bad, mx);
  lo1 = canon_lo_mx(t.y, qhalf, bad, mx);
}
// Coefficient type of a launch's slabs (int64_t, the default, or int32_t): the 16- / 8-byte pair of the rotation kernels'
// accesses, and the store of a centred result (the value is below 2^31 in magnitude for every modulus: the cast is exact).
template <class C> struct CoefPair;
template <> struct CoefPair<int64_t> { using type = longlong2; };
template <> struct CoefPair<int32_t> { using type = int2; };
__device__ __forceinline__ void pair_words(const longlong2 t, int32_t& lo0, int32_t& lo1) { lo0 = (int32_t)t.x, lo1 = (int32_t)t.y; }
__device__ __forceinline__ void pair_words(const int2 t, int32_t& lo0, int32_t& lo1) { lo0 = t.x, lo1 = t.y; }
// wave-uniform verdict of the per-lane accumulators (mx holds max (lo + h) mod 2^32, canonical <=> <= 2h)
__device__ __forceinline__ bool canon_fail(uint32_t bad, uint32_t mx, uint32_t qhalf) {
  return __any((bad != 0) | (mx > 2u * qhalf)) != 0;
}
// A non-canonical coefficient was loaded for proof `bo`: clear its verdict (all bits) and raise the sticky word.
__device__ __forceinline__ void input_fault(const Operands& ops, uint8_t* flags, uint32_t bo, int lane) {
  if ((lane & 63) != 0) return;   // the first lane of the wavefront that saw the fault (teams of two report per wave)
  if (flags) {
    if (ops.pad) {
      const uintptr_t a = reinterpret_cast<uintptr_t>(flags + bo);
      __hip_atomic_fetch_and(reinterpret_cast<uint32_t*>(a & ~(uintptr_t)3), ~(0xffu << (8u * (uint32_t)(a & 3u))),
                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      flags[bo] = 0;
    }
  }
  if (ops.bad) *ops.bad = 1u;
}

// C: the coefficient type of the launch's slabs (Operands::base holds the addresses; the element width is the launch's)
template <class C = int64_t>
__device__ __forceinline__ const C* operand_ptr(const Operands& ops, uint32_t op, uint32_t off,
                                                uint32_t b, uint32_t bo, int n_coef) {
  const uint32_t idx = ops.outer[op] ? bo : b;
  return reinterpret_cast<const C*>(ops.base[op]) + ((uint64_t)idx * ops.stride[op] + off) * (uint64_t)n_coef;
}

constexpr int kEpiChunk = 16;   // coefficients per lane handled together in the epilogue (4 was slower: fewer loads in flight)
// Opaque copy of the lane id inside the loops: stops the compiler from hoisting every lane-dependent
// address out of the loops (where they sit in dozens of VGPRs) at the price of recomputing them per
// term.  At N = 1024 it costs the transform-only rows ~5 % (123 -> 87 VGPRs, but LDS already caps the kernel
// at 4 waves per SIMD), so there it is used only (template flag OPQ) by the rows that start with a shift term,
// which it keeps below 128 VGPRs (144 -> 101); at N = 2048 it takes the kernel from 254 VGPRs (1 wave per
// SIMD) to ~125 (4 waves).
constexpr int kOpaqueLaneMinLogn = 11;
#define RZK_OPAQUE(v)                                                     \
  do {                                                                    \
    if (LOGN >= kOpaqueLaneMinLogn || OPQ) asm volatile("" : "+v"(v)); \
  } while (0)

// Load one coefficient polynomial (coalesced phase-1 layout) and lift it into prime field `pc`.
// measure (the first prime pass): nrm2 = an upper bound of the polynomial's 2-norm (wave-uniform), and — check — the
// fused norm predicate sum c^2 < limit, exact (norm_below); unless `trusted`, the same pass proves that every
// coefficient is canonical (canon_lo_mx).  Later passes re-read the low words only.
// How the measure pass is laid out (MODE): the arithmetic is the same, the register footprint is not.
//   LL_FUSED   every coefficient tested, squared and lifted as it arrives, all E loads in flight (unit_kernel)
//   LL_HALVES  the same in two rolled halves: E/2 sixty-four-bit coefficients in flight
//   LL_L1INF   all E loads in flight, low words into an int array first; sum v^2 bounded by |v|_1 |v|_inf
enum : int { LL_FUSED = 0, LL_HALVES = 1, LL_L1INF = 2 };
// row_kernel keeps its running sum (and, in a vector x vector term, the first operand's transform) in registers across
// the load.  Measured on the Sum (4,9,4) / Linear configurations (A/B of prebuilt libraries, round 3): LL_L1INF for
// both operands 224-225 k / 4.35 M proofs/s, LL_HALVES for both 221 k / 4.26 M, LL_FUSED spills (128 VGPRs + 156
// bytes of scratch: 213 k / 4.10 M).  Teams of two (N = 2048) stay spill-free only with LL_HALVES.
template <class TM>
constexpr int kRowLoadMode = TM::LL == 7 ? LL_HALVES : LL_L1INF;   // row_kernel, both operands of a term
template <int LOGN, class TM = WaveTeam, int MODE = LL_FUSED, class C = int64_t>
__device__ __forceinline__ void load_lift(uint32_t* x, const C* __restrict__ src, int lane, const PrimeConsts& pc,
                                          bool measure, float& nrm2, bool check, uint64_t limit, bool& below,
                                          uint32_t qhalf, bool trusted, bool& fault) {
  using G = Geo<LOGN, TM::LL>;
  if (measure) {
    // one pass: the 64-bit coefficient is tested, squared into the float sum and lifted as soon as it arrives, so that
    // only the lifted residues stay in registers (no second copy of the polynomial)
    float part = 0.f;
    if (MODE == LL_L1INF) {
      int32_t v[G::E];
      uint32_t bad = 0;
#pragma unroll
      for (int e = 0; e < G::E; ++e) v[e] = trusted ? (int32_t)ld_stream(src + G::j_p1(lane, e)) : canon_lo(ld_stream(src + G::j_p1(lane, e)), qhalf, bad);
      uint64_t sum = 0;
      uint32_t mxa = 0;
#pragma unroll
      for (int e = 0; e < G::E; e += 2) {
        const uint32_t u0 = (uint32_t)v[e], u1 = (uint32_t)v[e + 1];
        const uint32_t a0 = v[e] < 0 ? 0u - u0 : u0;
        const uint32_t a1 = v[e + 1] < 0 ? 0u - u1 : u1;
        sum += (uint64_t)a0 + a1;
        mxa = a0 > mxa ? a0 : mxa;
        mxa = a1 > mxa ? a1 : mxa;
      }
      const float l1 = (float)TM::sum_u56(sum) * (1.0f + 0x1p-20f);
      const uint32_t wmx = TM::max_u32(mxa);
      if (!trusted) fault = fault || __any(bad != 0) || wmx > qhalf;
      // sum v^2 <= |v|_1 |v|_inf; handed on as if every thread of the team carried an equal share
      part = l1 * (float)wmx * (1.0f + 0x1p-20f) * (1.0f / (float)G::LANES);
      if (check) {   // the exact predicate needs the exact sum: float squares of the same registers
        float sq = lane_sum_sq_f32<G::E>(v);
        const float ssq = TM::sum_f32(sq);
        const double sd = (double)ssq, lim = (double)limit;
        if (sd * (1.0 + 2.0 * (double)kNormSlack) < lim) below = true;
        else if (sd * (1.0 - 2.0 * (double)kNormSlack) >= lim) below = false;
        else below = TM::sum_u56(lane_sum_sq_exact<G::E>(v)) < limit;
      }
#pragma unroll
      for (int e = 0; e < G::E; ++e) x[e] = lift(v[e], pc);
    } else if (MODE == LL_HALVES) {
      // two rolled halves: E/2 sixty-four-bit coefficients in flight instead of E.  For the kernels that keep a running
      // sum in registers across the load (row_kernel, the group and slot kernels) this is what fits 128 VGPRs without
      // spilling (row_kernel<10>: 116 VGPRs against 128 + 156 bytes of scratch); unit_kernel, with nothing else live,
      // is better off with all loads in flight at once (116 against 132 VGPRs).
      uint32_t bad = 0, mx = 0;
      constexpr int H = G::E / 2;
#pragma unroll 1
      for (int h = 0; h < 2; ++h) {
        uint32_t y[H];
#pragma unroll
        for (int e2 = 0; e2 < H; ++e2) {
          const C c = ld_stream(src + (size_t)(h * H + e2) * G::LANES + lane);
          const int32_t v = trusted ? (int32_t)c : canon_lo_mx(c, qhalf, bad, mx);
          const float f = (float)v;
          part = __builtin_fmaf(f, f, part);
          y[e2] = lift(v, pc);
        }
#pragma unroll
        for (int e2 = 0; e2 < H; ++e2) {
          x[e2] = h == 0 ? y[e2] : x[e2];
          x[H + e2] = h == 1 ? y[e2] : x[H + e2];
        }
      }
      if (!trusted) fault = fault || canon_fail(bad, mx, qhalf);
    } else if (trusted) {
#pragma unroll
      for (int e = 0; e < G::E; ++e) {
        const int32_t v = (int32_t)ld_stream(src + G::j_p1(lane, e));
        const float f = (float)v;
        part = __builtin_fmaf(f, f, part);
        x[e] = lift(v, pc);
      }
    } else {
      uint32_t bad = 0, mx = 0;
#pragma unroll
      for (int e = 0; e < G::E; ++e) {
        const int32_t v = canon_lo_mx(ld_stream(src + G::j_p1(lane, e)), qhalf, bad, mx);
        const float f = (float)v;
        part = __builtin_fmaf(f, f, part);
        x[e] = lift(v, pc);
      }
      fault = fault || canon_fail(bad, mx, qhalf);
    }
    const float ss = TM::sum_f32(part);
    nrm2 = norm2_upper(ss);
    if (check && MODE != LL_L1INF) {
      const double sd = (double)ss, lim = (double)limit;
      if (sd * (1.0 + 2.0 * (double)kNormSlack) < lim) {
        below = true;
      } else if (sd * (1.0 - 2.0 * (double)kNormSlack) >= lim) {
        below = false;
      } else {   // inside the rounding band of the limit: exact integers, from the lifted residues (v = x - 2p)
        int32_t v[G::E];
#pragma unroll
        for (int e = 0; e < G::E; ++e) v[e] = (int32_t)(x[e] - pc.twop);
        below = TM::sum_u56(lane_sum_sq_exact<G::E>(v)) < limit;
      }
    }
  } else {
#pragma unroll
    for (int e = 0; e < G::E; ++e) x[e] = lift((int32_t)ld_stream(src + G::j_p1(lane, e)), pc);
  }
}

// =============================================================================================
// Row-program kernels: the fused product / accumulate / reduce pipeline of every protocol phase.
//
// A wavefront owns polynomial-sized pieces of one proof (rzk_dev.h).  Control flow is wave-uniform and scalar (the
// wave index is read with readfirstlane).  Primes are processed one after the other; each inverse transform is folded
// at once into the running Garner state (rzk_core.h, crt_fold*), so no state occupies registers during the transforms.
// The operands' norms are measured while they are loaded for the first prime, which fixes how many primes (1..3) the
// exact result needs; the same pass proves that every coefficient is canonical.  Which kernel runs a program is
// decided once per (program, shape) by the planner (rzk_plan.h, plan_program and path_of):
//
//   unit_kernel       key-product programs (the default): one wavefront per proof walks the program's units — single
//                     rows, or pairs of rows that share their last operand; sums parked in LDS, Garner words in
//                     per-wave global scratch lines.
//   row_kernel        programs with vector x vector products: one wavefront per row, sum in registers, Garner word A
//                     in LDS.
//   shift_row_kernel  rows whose products all have the sparse challenge as multiplier: rotations, no transform.
//   row_group_kernel  (N <= 1024) / row_block_kernel (N = 2048): key blocks with n > 1, operands transformed once for
//                     several rows.
//   fwd_slots_kernel  + row_slots_kernel: when many rows of a proof use the same operands (sums over V summands at large
//                     shapes), every distinct operand ("slot") is transformed ONCE per proof into a workspace in HBM,
//                     and the rows only multiply-accumulate the stored transforms; rows that need more primes than
//                     were stored fall back to in-wave transforms for the missing primes, so results stay exact.
// =============================================================================================
#ifndef RZK_ROW_MIN_WAVES
#define RZK_ROW_MIN_WAVES 1   // minimum waves per SIMD the row kernels are compiled for (register budget)
#endif

// ---- challenge products as signed rotations (ShiftGeo, rzk_core.h): shared by shift_row_kernel and the
// shift terms of row_kernel ---------------------------------------------------------------------------------

template <int LOGN, int LL = 6, class C = int64_t>
__device__ __forceinline__ void load_pairs(int32_t* v, const C* __restrict__ src, int lane, uint32_t qhalf,
                                           uint32_t& bad, uint32_t& mx, bool trusted) {
  using S = ShiftGeo<LOGN, true, LL>;
  using P2 = typename CoefPair<C>::type;
  const P2* __restrict__ p = reinterpret_cast<const P2*>(src);
  if (trusted) {
#pragma unroll
    for (int g = 0; g < S::G; ++g) {
      const P2 t = ld_stream(p + g * S::LANES + lane);
      pair_words(t, v[2 * g], v[2 * g + 1]);
    }
  } else {
#pragma unroll
    for (int g = 0; g < S::G; ++g) canon_pair(ld_stream(p + g * S::LANES + lane), qhalf, bad, mx, v[2 * g], v[2 * g + 1]);   // coefficients g*2*LANES + 2*lane, +1
  }
}

constexpr int kShiftH = 8;   // outputs of a lane accumulated per scan over the multiplier's non-zeros (N = 2048 response rows, round 3: 160 us; 4 -> 186, 16 -> 181)
constexpr int kShiftHMem = 16;   // ... for the rotation terms inside the row kernels (sums go to the wave's scratch line)
constexpr int kShiftHMemPair = 8;   // ... of a two-wavefront team (16 measured slower: verify at N = 2048 189 vs 184 us, 40 vs 8 bytes of scratch)
// walk the non-zero coefficients of the multiplier (registers a[], lane-distributed in layout PAIR) and add
// the rotations into IN outputs of every lane; `ext` already points at the first of them
template <int LOGN, bool PAIR, int IN>
__device__ __forceinline__ void shift_scan(int64_t* acc, const int32_t* a, int lane, const int32_t* ext) {
  using S = ShiftGeo<LOGN, PAIR>;
#pragma unroll
  for (int i = 0; i < S::E; ++i) {
    uint64_t mask = __ballot(a[i] != 0);
    while (mask) {
      const int l = __builtin_ctzll(mask);
      mask &= mask - 1;
      const int32_t coef = __builtin_amdgcn_readlane(a[i], l);
      const int s = S::off(i) + (PAIR ? 2 * l : l);
      int ln = lane;
      asm volatile("" : "+v"(ln));   // keeps the 16 per-register base addresses from being hoisted into VGPRs
      shift_accum<LOGN, PAIR, int64_t, 0, IN>(acc, ln, s, coef, ext);
    }
  }
}
// (Taking two non-zeros per trip, or sixteen outputs per scan, to keep more LDS reads in flight was measured
// slower: the extra registers cost a wave per SIMD.)

// ---- teams of two wavefronts: the multiplier's non-zeros as a list in LDS (kShiftListCap entries per round) ----
// number of non-zero coefficients this WAVEFRONT holds
template <int E>
__device__ __forceinline__ uint32_t shift_count_nonzeros(const int32_t* a) {
  uint32_t cnt = 0;
#pragma unroll
  for (int i = 0; i < E; ++i) cnt += (uint32_t)__builtin_popcountll(__ballot(a[i] != 0));
  return cnt;
}
// entries [r0, r0 + cap) of the team's list; `base` = entries of the wavefronts before this one
template <int LOGN, bool PAIR, int LL>
__device__ __forceinline__ void shift_list_write(const int32_t* a, int lane, uint32_t base, uint32_t r0, int32_t* list) {
  using S = ShiftGeo<LOGN, PAIR, LL>;
  uint32_t run = base - r0;   // (mod 2^32: entries before the window wrap to huge indices and are skipped)
  int2* ent = reinterpret_cast<int2*>(list);
#pragma unroll
  for (int i = 0; i < S::E; ++i) {
    const uint64_t m = __ballot(a[i] != 0);
    const uint32_t idx = run + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    if (a[i] != 0 && idx < (uint32_t)kShiftListCap) ent[idx] = make_int2(S::j(lane, i), a[i]);
    run += (uint32_t)__builtin_popcountll(m);
  }
}
// add the rotations of the list's first `nent` entries into IN outputs of every thread
template <int LOGN, bool PAIR, int LL, int IN>
__device__ __forceinline__ void shift_scan_list(int64_t* acc, const int32_t* list, uint32_t nent, int lane, const int32_t* ext) {
  const int2* ent = reinterpret_cast<const int2*>(list);
  const int l64 = lane & 63;
#pragma unroll 1
  for (uint32_t e0 = 0; e0 < nent; e0 += 64) {
    const uint32_t m = nent - e0 < 64u ? nent - e0 : 64u;
    const int2 mine = (uint32_t)l64 < m ? ent[e0 + l64] : make_int2(0, 0);   // 64 entries per trip, one per lane
#pragma unroll 1
    for (uint32_t e = 0; e < m; ++e) {
      const int s = __builtin_amdgcn_readlane(mine.x, (int)e);
      const int32_t coef = __builtin_amdgcn_readlane(mine.y, (int)e);
      int ln = lane;
      asm volatile("" : "+v"(ln));
      shift_accum<LOGN, PAIR, int64_t, 0, IN, LL>(acc, ln, s, coef, ext);
    }
  }
}

// Build the wave's 2N-word extended image of v (ShiftGeo, rzk_core.h) straight from global memory, in two rolled
// halves so that only E/2 sixty-four-bit coefficients are in flight at a time.  measure: this is the first fill —
// it also proves that v is canonical (canon_lo) and returns max |v| over the lane's coefficients.
template <int LOGN, bool PAIR, int LL = 6, class C = int64_t>
__device__ __forceinline__ void shift_fill_from(const C* __restrict__ pv, int lane, int32_t* ext, int part,
                                                bool measure, bool canon, uint32_t qhalf, uint32_t& bad, uint32_t& mx,
                                                uint32_t& maxabs) {
  using S = ShiftGeo<LOGN, PAIR, LL>;
  constexpr int H = S::E / 2;               // registers per half; off(h*H + i) = off(i) + h * H * LANES in both layouts
  constexpr int HOFF = H * S::LANES;
#pragma unroll 1
  for (int h = 0; h < 2; ++h) {
    int32_t vh[H];
    if (PAIR) {
      using P2 = typename CoefPair<C>::type;
      const P2* __restrict__ p = reinterpret_cast<const P2*>(pv) + (size_t)h * (H / 2) * S::LANES;
#pragma unroll
      for (int g = 0; g < H / 2; ++g) {
        const P2 t = ld_stream(p + g * S::LANES + lane);   // coefficients (h*H/2 + g)*2*LANES + 2*lane, +1
        if (canon) {
          canon_pair(t, qhalf, bad, mx, vh[2 * g], vh[2 * g + 1]);
        } else {
          pair_words(t, vh[2 * g], vh[2 * g + 1]);
        }
      }
    } else {
      const C* __restrict__ p = pv + (size_t)h * H * S::LANES;
#pragma unroll
      for (int i = 0; i < H; ++i) {
        const C c = p[i * S::LANES + lane];
        vh[i] = canon ? canon_lo_mx(c, qhalf, bad, mx) : (int32_t)c;
      }
    }
    if (measure) {
#pragma unroll
      for (int i = 0; i < H; ++i) {
        const uint32_t uu = (uint32_t)vh[i];
        const uint32_t vv = vh[i] < 0 ? 0u - uu : uu;
        maxabs = vv > maxabs ? vv : maxabs;
      }
    }
    int32_t* base = ext + S::lane_base(lane) + h * HOFF;
#pragma unroll
    for (int i = 0; i < H; ++i) {
      const int32_t a = shift_part(vh[i], part);
      base[S::N + S::off(i)] = a;
      base[S::off(i)] = -a;
    }
  }
}

// res[] (in [0,q)) +/-= (a (*) v) mod q for one product term; a[] holds the multiplier's low words in layout
// PAIR, pv points at the other operand.  ext: the team's 2N-word LDS image (teams of two: followed by the
// kShiftListWords words of the non-zero list).  Team-uniform control flow.
// TO_MEM: res is a per-team line in global memory indexed by coefficient (each thread touches only its own
// coefficients) and `fresh` says that it holds nothing yet; otherwise res are the thread's E registers.
// Sums are exact 64-bit integers (v_mad_i64_i32) as long as |a|_1 |v|_inf < 2^62; beyond that v goes in as
// two 16-bit halves.  The register form accumulates HREG of a thread's outputs per scan over the multiplier (eight by
// default, the register budget of shift_row_kernel), the TO_MEM form kShiftHMem / kShiftHMemPair.
// fault: set when v holds a non-canonical coefficient (the caller tests `a`).
// HREG: outputs per scan of the register form (unit_kernel's rotation-last path runs it with nothing else live and
// takes all 16 of a lane's outputs in one scan, as the TO_MEM form does).
template <int LOGN, bool PAIR, bool TO_MEM, class TM = WaveTeam, int HREG = kShiftH, class C = int64_t>
__device__ __forceinline__ void shift_product(uint32_t* res, bool fresh, bool minus, const int32_t* a,
                                              const C* __restrict__ pv, int lane_in, int32_t* ext,
                                              const DevTables& T, bool& fault, bool trusted) {
  constexpr int LL = TM::LL;
  int lane = lane_in;
  if (LL != 6) asm volatile("" : "+v"(lane));   // per call: keeps the thread's 64-bit line / image addresses out of the kernel prologue
  using S = ShiftGeo<LOGN, PAIR, LL>;
  constexpr int E = S::E;
  constexpr int HW = TO_MEM ? (LL == 6 ? kShiftHMem : kShiftHMemPair) : HREG;   // (the in-kernel rotation terms run with nothing else live)
  constexpr int H = HW < E ? HW : E;   // outputs per scan; chunk c covers registers c*H .. c*H+H-1
  constexpr int NCH = E / H;
  constexpr bool LIST = LL != 6;
  const uint32_t q = T.crt.q, qhalf = T.crt.qhalf;
  // optimistic first fill with the whole values; it also measures v
  uint32_t vbad = 0, vmx = 0, maxv = 0;
  TM::sync();   // earlier reads of the image are done before it is overwritten
  shift_fill_from<LOGN, PAIR, LL, C>(pv, lane, ext, SHIFT_WHOLE, true, !trusted, qhalf, vbad, vmx, maxv);
  if (!trusted) fault = fault || canon_fail(vbad, vmx, qhalf);
  uint64_t suma = 0;
#pragma unroll
  for (int i = 0; i < E; ++i) {
    const uint32_t ua = (uint32_t)a[i];
    suma += a[i] < 0 ? 0u - ua : ua;
  }
  const double bound = (double)TM::sum_u56(suma) * (double)TM::max_u32(maxv);   // |exact product|_inf (E * 2^31 < 2^56 per lane)
  const int npass = __builtin_amdgcn_readfirstlane(bound < 4.0e18 ? 1 : 2);        // 4.0e18 < 2^62
  // teams of two: where this wavefront's non-zeros go in the list, and how many there are in all
  int32_t* list = ext + S::WORDS;
  uint32_t lbase = 0, ltotal = 1;   // (one wavefront: a single "round", the multiplier is walked in registers)
  if (LIST) {
    const uint32_t mine = shift_count_nonzeros<E>(a);
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane(lane >> 6);
    if ((lane & 63) == 0) list[2 * kShiftListCap + w] = (int32_t)mine;
    TM::sync();   // (also orders the image's fill before the first scan)
    const uint32_t c0 = (uint32_t)__builtin_amdgcn_readfirstlane(list[2 * kShiftListCap]);
    const uint32_t c1 = (uint32_t)__builtin_amdgcn_readfirstlane(list[2 * kShiftListCap + 1]);
    lbase = w ? c0 : 0u;
    ltotal = c0 + c1;
  }
  bool started = false;   // the TO_MEM line holds this product's partial sums
#pragma unroll 1
  for (int pass = 0; pass < npass; ++pass) {
    if (npass == 2) {   // (never for a sparse +-1 challenge) the image is rebuilt from 16-bit halves
      uint32_t u0 = 0, u1 = 0, u2 = 0;
      TM::sync();
      shift_fill_from<LOGN, PAIR, LL, C>(pv, lane, ext, pass == 0 ? SHIFT_LOW16 : SHIFT_HIGH16, false, false, qhalf, u0, u1, u2);
    }
    if (!LIST || npass == 2) TM::sync();
#pragma unroll 1
    for (uint32_t r0 = 0; r0 < (ltotal ? ltotal : 1u); r0 += LIST ? (uint32_t)kShiftListCap : 1u) {   // (a zero multiplier still initialises the sums)
      uint32_t nent = 0;
      if (LIST) {
        if (r0 || pass) TM::sync();   // the previous round's scans are over
        shift_list_write<LOGN, PAIR, LL>(a, lane, lbase, r0, list);
        TM::sync();
        nent = ltotal - r0 < (uint32_t)kShiftListCap ? ltotal - r0 : (uint32_t)kShiftListCap;   // (0 when there is no non-zero at all)
      }
#pragma unroll 1
      for (int ch = 0; ch < NCH; ++ch) {
        int64_t acc[H];
#pragma unroll
        for (int i = 0; i < H; ++i) acc[i] = 0;
        // off(c*H + i) = off(i) + LANES H c in both layouts
        if (LIST) shift_scan_list<LOGN, PAIR, LL, H>(acc, list, nent, lane, ext + ch * (S::LANES * H));
        else shift_scan<LOGN, PAIR, H>(acc, a, lane, ext + ch * (S::LANES * H));
#pragma unroll
        for (int i = 0; i < H; ++i) {
          uint32_t u = zq_from_i64(acc[i], T.crt);
          if (pass) u = montq_u(u, T.crt.r48q, T.crt);   // high halves carry the weight 2^16
          if (TO_MEM) {
            uint32_t* slot = res + S::j(lane, i) + ch * (S::LANES * H);
            const uint32_t cur = (fresh && !started) ? 0u : *slot;
            *slot = minus ? subq(cur, u, q) : addq(cur, u, q);
          } else {
#pragma unroll
            for (int c = 0; c < NCH; ++c) {   // register index c*H + i, selected without dynamic indexing
              const uint32_t cur = res[c * H + i];
              const uint32_t nw = minus ? subq(cur, u, q) : addq(cur, u, q);
              res[c * H + i] = c == ch ? nw : cur;
            }
          }
        }
      }
      started = true;
    }
  }
}

// The same product on packed bytes (ByteGeo, rzk_core.h) when the operands are short enough; one wavefront, res in
// registers.  Returns false, with nothing but `fault` touched, when they are not: the caller then runs shift_product.
// The multiplier's non-zeros are walked as in shift_scan.  The sums leave through the image to get from the scan's dword ownership back to the
// PAIR layout of res[] and of the global accesses.
template <int LOGN, class C = int64_t>
__device__ __forceinline__ bool shift_product_bytes(uint32_t* res, bool minus, const int32_t* a, const C* __restrict__ pv,
                                                    int lane, int32_t* slab, const DevTables& T, bool& fault, bool trusted) {
  using S = ShiftGeo<LOGN, true>;
  using B = ByteGeo<LOGN>;
  constexpr int E = S::E;
  const uint32_t q = T.crt.q, qhalf = T.crt.qhalf;
  uint32_t* img = reinterpret_cast<uint32_t*>(slab);
  uint32_t vbad = 0, vmx = 0, maxv = 0, suma = 0;
#pragma unroll
  for (int i = 0; i < E; ++i) {
    const uint32_t ua = (uint32_t)a[i], aa = a[i] < 0 ? 0u - ua : ua;
    suma += aa < 256u ? aa : 256u;   // saturated: 64 * 16 * 256 fits, and one entry above 255 already fails the condition
  }
  const uint32_t norm1 = wave_sum_u32(suma);
  if (norm1 > 255u) return false;   // (before v is touched: the word path loads it itself)
  wave_sync();   // earlier reads of the image are done before it is overwritten
  constexpr int GH = S::G / 2;   // pairs per half: two rolled halves, as shift_fill_from, to keep few 16-byte loads' registers live
  using P2 = typename CoefPair<C>::type;
  const P2* __restrict__ p = reinterpret_cast<const P2*>(pv) + lane;
#pragma unroll 1
  for (int h = 0; h < 2; ++h) {
    int32_t vh[2 * GH];
#pragma unroll
    for (int g = 0; g < GH; ++g) {
      const P2 t = ld_stream(p + (h * GH + g) * 64);   // coefficients (h*GH + g)*128 + 2*lane, +1
      if (trusted) pair_words(t, vh[2 * g], vh[2 * g + 1]);
      else canon_pair(t, qhalf, vbad, vmx, vh[2 * g], vh[2 * g + 1]);
    }
#pragma unroll
    for (int g = 0; g < GH; ++g) {
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const uint32_t uv = (uint32_t)vh[2 * g + c], av = vh[2 * g + c] < 0 ? 0u - uv : uv;
        maxv = av > maxv ? av : maxv;
      }
      shift_bytes_put_raw<LOGN>(vh[2 * g], vh[2 * g + 1], lane, h * GH + g, img);
    }
    // A wide operand usually shows in its first half: stop there.  The word path then loads v itself, so such a term
    // reads half of v (at worst all of it) a second time, mostly from L2; no response row of the protocols is one.
    if (h == 0 && wave_max_u32(maxv) > 127u) return false;
  }
  const uint32_t bias = wave_max_u32(maxv);
  if (!shift_bytes_ok(norm1, bias)) return false;
  if (!trusted) fault = fault || canon_fail(vbad, vmx, qhalf);
  wave_sync();
  shift_bytes_bias<LOGN>(lane, bias, img);
  wave_sync();
  uint32_t acc[B::W];
#pragma unroll
  for (int k = 0; k < B::W; ++k) acc[k] = 0;
#pragma unroll
  for (int i = 0; i < E; ++i) {
    uint64_t mask = __ballot(a[i] != 0);
    while (mask) {
      const int l = __builtin_ctzll(mask);
      mask &= mask - 1;
      const int32_t coef = __builtin_amdgcn_readlane(a[i], l);
      int ln = lane;
      asm volatile("" : "+v"(ln));   // (as shift_scan: one address register, not one per i)
      shift_bytes_accum<LOGN>(acc, ln, S::off(i) + 2 * l, coef, img);
    }
  }
  wave_sync();   // every lane's reads are over: the sums take the image's place
  shift_bytes_park<LOGN>(acc, lane, img);
  wave_sync();
  int32_t prod[E];
  shift_bytes_take<LOGN>(prod, lane, norm1 * bias, img);
#pragma unroll
  for (int i = 0; i < E; ++i) {
    const uint32_t u = zq_from_centered(prod[i], q);
    res[i] = minus ? subq(res[i], u, q) : addq(res[i], u, q);
  }
  return true;
}

// Producer side of Operands::oimg: the transform x (prime pi) of operand (op, off) of batch entry b, as it leaves wave_fwd
template <int LOGN, class TM>
__device__ __forceinline__ void store_operand_image(const uint32_t* x, const Operands& ops, uint32_t op, uint32_t off, uint32_t b,
                                                    int pi, int lane, float nrm2, bool first) {
  using G = Geo<LOGN, TM::LL>;
  if (!ops.oimg || op != ops.oimg_op || off >= 32u) return;
  const int ci = ops.oimg_col[off];
  if (ci < 0) return;
  const size_t oslot = (size_t)b * ops.oimg_n + (uint32_t)ci;
  uint4* __restrict__ dst = reinterpret_cast<uint4*>(ops.oimg + (oslot * kKeyImages + pi) * G::N);
#pragma unroll
  for (int g = 0; g < G::E / 4; ++g) dst[G::key4(lane, g)] = make_uint4(x[4 * g], x[4 * g + 1], x[4 * g + 2], x[4 * g + 3]);
  if (lane == 0) {
    if (first) ops.oimg_l2[oslot] = (double)nrm2;
    ops.oimg_np[oslot] = (uint8_t)(pi + 1);   // primes 0 .. pi are there (the passes run in this order)
  }
}

// acc +/- (term) for prime `pi`, transforming the term's operands in the wave.  The coefficient type of the operands comes
// with the team (TeamCoef, rzk_wave.h).
template <int LOGN, bool HAS_VEC, bool OPQ = false, class TM = WaveTeam, bool DD = false>
__device__ __forceinline__ void term_direct(uint32_t* acc, const Term tm, const Operands& ops, uint32_t b,
                                            uint32_t bo, int lane, uint32_t* lds, const uint32_t* __restrict__ twf,
                                            const PrimeConsts& pc, int pi, const uint32_t* __restrict__ key_ntt,
                                            const double* __restrict__ key_l2, bool first, float& bound,
                                            uint8_t* __restrict__ flags, uint32_t qhalf) {
  using G = Geo<LOGN, TM::LL>;
  using C = typename TeamCoef<TM>::type;   // coefficient type of the slabs
  constexpr int E = G::E;
  constexpr int N = G::N;
  // optional opaque copy of the lane id (RZK_OPAQUE): stops hoisting of lane-dependent addresses
  int ln = lane;
  RZK_OPAQUE(ln);
  uint32_t x[E];
  float nb = 0.f;
  bool below = true, fault = false;
  const bool chk = first && (tm.kind & (TERM_CHECK | TERM_CHECK2));
  const bool trusted = ops.trusted != 0;
  // TERM_DD: the operand's transform under this prime may already lie in the call's operand images
  bool from_image = false;
  size_t oslot = 0;
  if (DD && (tm.kind & TERM_KIND_MASK) == TERM_DD && ops.oimg) {   // (DD is a template flag: as a run-time test in every row kernel it changed the compiler's load scheduling of the ordinary rows — Linear -2 %)
    const uint32_t summand = tm.b_off / ops.oimg_k, col = tm.b_off - summand * ops.oimg_k;
    const int ci = col < 32u ? ops.oimg_col[col] : -1;
    if (ci >= 0) {
      oslot = ((size_t)bo * ops.oimg_group + summand) * ops.oimg_n + (uint32_t)ci;
      from_image = (int)ops.oimg_np[oslot] > pi;
    }
  }
  if (DD) from_image = __builtin_amdgcn_readfirstlane((int)from_image) != 0;
  if (DD && from_image) {
    const uint4* __restrict__ ip = reinterpret_cast<const uint4*>(ops.oimg + (oslot * kKeyImages + pi) * N);
#pragma unroll
    for (int g = 0; g < E / 4; ++g) {
      const uint4 iv = ip[G::key4(ln, g)];
      x[4 * g] = iv.x, x[4 * g + 1] = iv.y, x[4 * g + 2] = iv.z, x[4 * g + 3] = iv.w;
    }
    nb = (float)ops.oimg_l2[oslot];
  } else {
    load_lift<LOGN, TM, kRowLoadMode<TM>, C>(x, operand_ptr<C>(ops, tm.b_op, tm.b_off, b, bo, N), ln, pc, first, nb, chk, ops.norm_limit, below, qhalf, trusted, fault);
    if (chk && !below && (lane & 63) == 0) fail_check(flags + bo, ops.pad != 0, (tm.kind & TERM_CHECK2) != 0);
    wave_fwd<LOGN, TM>(x, ln, lds, twf, pc);
  }
  if (HAS_VEC && (tm.kind & TERM_KIND_MASK) == TERM_VEC) {
    // product of two per-proof polynomials: fold N^-1 and the Montgomery factor into one of them
    uint32_t xb[E];
#pragma unroll
    for (int c = 0; c < E; ++c) xb[c] = csub(mont_lazy(x[c], pc.ninv_r2, pc.p, pc.npinv), pc.p);
    float na = 0.f;
    bool unused_below = true;
    load_lift<LOGN, TM, kRowLoadMode<TM>, C>(x, operand_ptr<C>(ops, tm.a_op, tm.a_off, b, bo, N), ln, pc, first, na, false, 0, unused_below, qhalf, trusted, fault);
    wave_fwd<LOGN, TM>(x, ln, lds, twf, pc);
    if (first) bound = bound_fma(na, nb, bound);   // |a (*) b|_inf <= |a|_2 |b|_2
    if (tm.sign >= 0) {
#pragma unroll
      for (int c = 0; c < E; ++c) acc[c] = mac_add(acc[c], x[c], xb[c], pc);
    } else {
#pragma unroll
      for (int c = 0; c < E; ++c) acc[c] = mac_sub(acc[c], x[c], xb[c], pc);
    }
  } else {
    // resident key entry, or (TERM_DKEY) one of the batch entry's own multiplier images — same form, same use
    const bool dk = (tm.kind & TERM_KIND_MASK) == TERM_DKEY || (tm.kind & TERM_KIND_MASK) == TERM_DD;
    const size_t image = dk ? (size_t)bo * ops.dkey_n + tm.a_off : (size_t)tm.a_off;
    if (first) bound = bound_fma((float)(dk ? ops.dkey_l2[image] : key_l2[image]), nb, bound);
    const uint4* __restrict__ kp = reinterpret_cast<const uint4*>((dk ? ops.dkey_img : key_ntt) + (image * kKeyImages + pi) * N);
    if (tm.sign >= 0) {
#pragma unroll
      for (int g = 0; g < E / 4; ++g) {
        const uint4 kv = kp[G::key4(ln, g)];
        acc[4 * g + 0] = mac_add(acc[4 * g + 0], x[4 * g + 0], kv.x, pc);
        acc[4 * g + 1] = mac_add(acc[4 * g + 1], x[4 * g + 1], kv.y, pc);
        acc[4 * g + 2] = mac_add(acc[4 * g + 2], x[4 * g + 2], kv.z, pc);
        acc[4 * g + 3] = mac_add(acc[4 * g + 3], x[4 * g + 3], kv.w, pc);
      }
    } else {
#pragma unroll
      for (int g = 0; g < E / 4; ++g) {
        const uint4 kv = kp[G::key4(ln, g)];
        acc[4 * g + 0] = mac_sub(acc[4 * g + 0], x[4 * g + 0], kv.x, pc);
        acc[4 * g + 1] = mac_sub(acc[4 * g + 1], x[4 * g + 1], kv.y, pc);
        acc[4 * g + 2] = mac_sub(acc[4 * g + 2], x[4 * g + 2], kv.z, pc);
        acc[4 * g + 3] = mac_sub(acc[4 * g + 3], x[4 * g + 3], kv.w, pc);
      }
    }
  }
  if (fault) input_fault(ops, flags, bo, lane);
}

// inverse transform of the prime-`pi` accumulator and fold into the Garner state: word A in LDS, word B
// (third prime only) in the per-wave global scratch line.  acc is clobbered.
template <int LOGN, bool OPQ = false, class TM = WaveTeam>
__device__ __forceinline__ void inverse_and_fold(int pi, int np, uint32_t* acc, int lane, uint32_t* lds,
                                                 const uint32_t* __restrict__ twi, const PrimeConsts& pc,
                                                 uint32_t* st_lds, uint32_t* __restrict__ st_glb, const DevTables& T) {
  using G = Geo<LOGN, TM::LL>;
  constexpr int E = G::E;
  int li = lane;
  RZK_OPAQUE(li);
  wave_inv<LOGN, TM>(acc, li, lds, twi, pc);
  if (pi == 0) {
#pragma unroll
    for (int e = 0; e < E; ++e) st_lds[G::j_p1(li, e)] = crt_fold0(acc[e], np, T.pc, T.crt);
  } else if (pi == 1) {
    uint32_t d0[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      d0[e] = st_lds[G::j_p1(li, e)];
      acc[e] = crt_digit1(acc[e], d0[e], np, T.pc, T.crt);
    }
    if (np == 3) {
#pragma unroll
      for (int e = 0; e < E; ++e) st_glb[G::j_p1(li, e)] = crt_value01_modp2(d0[e], acc[e], T.pc, T.crt);
    }
#pragma unroll
    for (int e = 0; e < E; ++e) st_lds[G::j_p1(li, e)] = crt_value01_modq(d0[e], acc[e], T.crt);
  } else {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      uint32_t a = st_lds[G::j_p1(li, e)];
      crt_fold2(acc[e], T.pc, T.crt, a, st_glb[G::j_p1(li, e)]);
      st_lds[G::j_p1(li, e)] = a;
    }
  }
}

// Checked additions (ADD_CHECK / ADD_CHECK2: the host marks them only among the first four additions of a row): the
// fused norm predicate sum c^2 < limit of the polynomial an addition loads.  The epilogues accumulate the float sum
// of squares per marked addition while they load it; the verdict is taken here, exactly (see "norms" above: float
// total outside the rounding band of the limit, otherwise the polynomial is re-read and summed in integers).
template <int LOGN, class TM = WaveTeam, class C = int64_t>
__device__ __forceinline__ void checked_add_verdicts(const Program* __restrict__ prog, const Row row, const Operands& ops,
                                                     uint32_t b, uint32_t bo, int lane, const float* add_ss,
                                                     uint8_t* __restrict__ flags) {
  using G = Geo<LOGN, TM::LL>;
#pragma unroll 1
  for (uint32_t a = 0; a < row.nadds && a < 4; ++a) {
    const AddTerm ad = table_load(&prog->adds[row.add0 + a]);
    if (!(ad.op & (ADD_CHECK | ADD_CHECK2))) continue;
    float part = 0.f;
#pragma unroll
    for (int sl = 0; sl < 4; ++sl) part = (sl == (int)a) ? add_ss[sl] : part;
    const double sfl = (double)TM::sum_f32(part), lim = (double)ops.norm_limit;
    bool below;
    if (sfl * (1.0 + 2.0 * (double)kNormSlack) < lim) {
      below = true;
    } else if (sfl * (1.0 - 2.0 * (double)kNormSlack) >= lim) {
      below = false;
    } else {
      const C* __restrict__ src = operand_ptr<C>(ops, ad.op & ADD_OP_MASK, ad.off, b, bo, G::N);
      int32_t v[G::E];
#pragma unroll
      for (int e = 0; e < G::E; ++e) v[e] = (int32_t)src[G::j_p1(lane, e)];
      below = TM::sum_u56(lane_sum_sq_exact<G::E>(v)) < ops.norm_limit;
    }
    if (!below && (lane & 63) == 0) fail_check(flags + bo, ops.pad != 0, (ad.op & ADD_CHECK2) != 0);
  }
}

// One chunk of one plain addition: u[i] +/-= operand coefficient (j_p1(lane, e0 + i)) in 32-bit arithmetic mod q;
// canonical test unless trusted; float sum of squares into add_ss[slot] for checked additions.
template <int LOGN, int CH, class TM = WaveTeam, class C = int64_t>
__device__ __forceinline__ void add_chunk(uint32_t* u, const AddTerm ad, uint32_t a, const C* __restrict__ src, int lane,
                                          int e0, uint32_t q, uint32_t qhalf, bool trusted, uint32_t& in_bad, uint32_t& in_mx,
                                          float* add_ss) {
  using G = Geo<LOGN, TM::LL>;
  int32_t av[CH];
  if (trusted) {
#pragma unroll
    for (int i = 0; i < CH; ++i) av[i] = (int32_t)ld_stream(src + G::j_p1(lane, e0 + i));
  } else {
#pragma unroll
    for (int i = 0; i < CH; ++i) av[i] = canon_lo_mx(ld_stream(src + G::j_p1(lane, e0 + i)), qhalf, in_bad, in_mx);
  }
  if (ad.op & (ADD_CHECK | ADD_CHECK2)) {
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const float f = (float)av[i];
      sq = __builtin_fmaf(f, f, sq);
    }
    const uint32_t slot = a < 4 ? a : 3;
#pragma unroll
    for (int sl = 0; sl < 4; ++sl) add_ss[sl] += (sl == (int)slot) ? sq : 0.f;
  }
  if (ad.sign >= 0) {
#pragma unroll
    for (int i = 0; i < CH; ++i) u[i] = addq(u[i], zq_from_centered(av[i], q), q);
  } else {
#pragma unroll
    for (int i = 0; i < CH; ++i) u[i] = subq(u[i], zq_from_centered(av[i], q), q);
  }
}

// plain additions in 32-bit arithmetic mod q, then centre and store / zero test; kEpiChunk coefficients
// per lane at a time.  Checked additions also evaluate the fused norm predicate.
template <int LOGN, class TM = WaveTeam, class C = int64_t>
__device__ __forceinline__ void row_epilogue(const Program* __restrict__ prog, const Row row, const Operands& ops,
                                             uint32_t b, uint32_t bo, int lane, bool has_terms, int np,
                                             const uint32_t* st_lds, const DevTables& T, uint8_t* __restrict__ flags,
                                             const uint32_t* __restrict__ st_sh = nullptr) {
  using G = Geo<LOGN, TM::LL>;
  constexpr int E = G::E;
  constexpr int N = G::N;
  int nz = 0;
  constexpr int CH = kEpiChunk < E ? kEpiChunk : E;
  const uint32_t q = T.crt.q;
  const bool trusted = ops.trusted != 0;
  float add_ss[4] = {0.f, 0.f, 0.f, 0.f};   // per-lane partial sums of squares of checked additions (slot = add index)
  uint32_t in_bad = 0, in_mx = 0;           // canonical-input test of the additions' coefficients
#pragma unroll
  for (int e0 = 0; e0 < E; e0 += CH) {
    uint32_t u[CH];
    if (has_terms) {
#pragma unroll
      for (int i = 0; i < CH; ++i) u[i] = crt_finish_zq(st_lds[G::j_p1(lane, e0 + i)], np, T.crt);
    } else {
#pragma unroll
      for (int i = 0; i < CH; ++i) u[i] = 0;
    }
    if (st_sh) {   // sum of the row's shift terms, left by the same lanes
#pragma unroll
      for (int i = 0; i < CH; ++i) u[i] = addq(u[i], st_sh[G::j_p1(lane, e0 + i)], q);
    }
#pragma unroll 1
    for (uint32_t a = 0; a < row.nadds; ++a) {
      const AddTerm ad = table_load(&prog->adds[row.add0 + a]);
      add_chunk<LOGN, CH, TM, C>(u, ad, a, operand_ptr<C>(ops, ad.op & ADD_OP_MASK, ad.off, b, bo, N), lane, e0, q, T.crt.qhalf, trusted,
                          in_bad, in_mx, add_ss);
    }
    if (row.mode == MODE_STORE) {
      C* __restrict__ dst = const_cast<C*>(operand_ptr<C>(ops, row.out_op, row.out_off, b, bo, N));
#pragma unroll
      for (int i = 0; i < CH; ++i) st_stream(dst + G::j_p1(lane, e0 + i), (C)center_from_zq(u[i], T.crt));
    } else {
#pragma unroll
      for (int i = 0; i < CH; ++i) nz |= (u[i] != 0);
    }
  }
  if (row.mode != MODE_STORE) {
    if (__any(nz) && (lane & 63) == 0) flags[bo] = 0;
  }
  if (row.nadds && !trusted && canon_fail(in_bad, in_mx, T.crt.qhalf)) input_fault(ops, flags, bo, lane);
  if (ops.norm_limit) checked_add_verdicts<LOGN, TM, C>(prog, row, ops, b, bo, lane, add_ss, flags);
}

__device__ __forceinline__ int primes_for(float fbound, const DevTables& T) {
  // |exact result| <= bound: the smallest prime count whose range covers it
  const double bound = (double)fbound * (1.0 + 0x1p-12);   // float sums of up to kMaxTerms rounded products: stay on the safe side
  const int np = bound <= T.cap[1] ? 1 : (bound <= T.cap[2] ? 2 : 3);
  return __builtin_amdgcn_readfirstlane(np);
}

}  // namespace rzk
