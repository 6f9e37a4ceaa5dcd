// rzk_unit.h - unit_kernel and unit_io_kernel (with the parked accumulators, Garner fold and finish_row they share with the other row-program kernels).
// Part of the one translation unit rzk_kernels.hip (device code only; no include guards beyond #pragma once).
#pragma once
#include "rzk_rowprog.h"

namespace rzk {

// =============================================================================================
// unit_kernel: the default evaluation of a row program (rzk_dev.h, "wave programs").
//
// One wavefront evaluates the units of one batch entry.  Per auxiliary prime it walks the unit's items: load the
// operand (the first prime pass also proves that every coefficient is canonical and measures the norms that fix the
// number of primes), lift, forward transform, multiply into the rows' accumulators; then inverse transform, fold
// into the Garner state, and after the last prime finish the row (rotation terms, plain additions, store or zero
// test, norm marks).  Register discipline: while an operand is loaded and transformed NOTHING else is live —
//   * the accumulator of row A is parked in LDS (buffer P, N words, key layout: the lane's own 16-byte slots, so
//     no cross-lane synchronisation) and only materialises in registers with the unit's last item, in place of
//     the transform it is computed from;
//   * the accumulator of a pair's row B is born with that last item and parked in P while row A is transformed back;
//   * the Garner state (one or two words per coefficient and row) lives in a per-wave global scratch line
//     ([g][lane][4] order, 16-byte accesses; L2 / Infinity-Cache resident), not in registers or LDS;
//   * rotation terms of a single row (one wavefront, DIET_ROT_LAST) run after the transforms, accumulating straight into
//     the row's value in registers, with the 2N-word image in the (then idle) slab + P; every other unit runs them first
//     and leaves their sum in a scratch line for finish_row;
//   * a unit of exactly two key products (ITEM_DOT2) parks the first transform, not the first product, and reduces the
//     two-term sum once with the last item.
// LDS per wavefront: transposition slab (N + N/32 words) + P (N words) = 8.1 KiB at N = 1024.
// =============================================================================================
// lines (of N words) of per-wave global scratch the unit / short kernels address
constexpr int kScratchLines = 6;
#ifndef RZK_STAMPS
#define RZK_STAMPS 0
#endif
#if RZK_STAMPS   // section timers of the diagnostic build: wall cycles a wave spends per kind of step
#define RZK_T0() const uint64_t t_sec0 = __builtin_amdgcn_s_memtime()
#define RZK_T1(acc) acc += __builtin_amdgcn_s_memtime() - t_sec0
#else
#define RZK_T0() do { } while (0)
#define RZK_T1(acc) do { } while (0)
#endif

// Fair progress among the wavefronts that share a SIMD.  The VALU arbiter serves the highest priority first and,
// among equals, the OLDEST wave: left alone, the four waves of a SIMD finish one after the other (measured at
// N = 1024, one proof per wave: 84 / 105 / 128 / 143 us) and the last one runs its tail alone, with nothing to hide
// its memory latency behind.  Each wave therefore lowers its priority as it advances through its share of the launch
// (quarter by quarter: s_setprio has four levels), so that laggards are served first and all waves stay resident
// until the end.  Speed only: priorities never affect results.
__device__ __forceinline__ void set_priority_level(uint32_t level) {   // 0 = most urgent
  if (level == 0) __builtin_amdgcn_s_setprio(3);
  else if (level == 1) __builtin_amdgcn_s_setprio(2);
  else if (level == 2) __builtin_amdgcn_s_setprio(1);
  else __builtin_amdgcn_s_setprio(0);
}
__device__ __forceinline__ void set_progress_priority(uint32_t done, uint32_t total) {
  set_priority_level(__builtin_amdgcn_readfirstlane(total ? (done * 4u) / total : 0u));
}
// x (transform, phase-3 register order) times `mul` (a resident key entry or a second transform, in registers), into
// row A's accumulator.  init: nothing accumulated yet; to_regs: the unit's last item -> the sum replaces x, else -> P
template <int LOGN, bool to_regs, bool MINUS, class TM = WaveTeam>
__device__ __forceinline__ void mac_park_signed(uint32_t* x, const uint32_t* mul, uint4* P4, int lane, bool init,
                                                const PrimeConsts& pc) {
  using G = Geo<LOGN, TM::LL>;
  constexpr int E = G::E;
  if (init && !MINUS) {   // first product of a sum: the lazy product IS the sum ([0,2p)), no add and no conditional subtract
#pragma unroll
    for (int g = 0; g < E / 4; ++g) {
      uint32_t as[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) as[i] = mont_lazy(x[4 * g + i], mul[4 * g + i], pc.p, pc.npinv);
      if (to_regs) {
#pragma unroll
        for (int i = 0; i < 4; ++i) x[4 * g + i] = as[i];
      } else {
        P4[G::own4(lane, g)] = make_uint4(as[0], as[1], as[2], as[3]);
      }
    }
    return;
  }
#pragma unroll
  for (int g = 0; g < E / 4; ++g) {
    uint4 a = make_uint4(0, 0, 0, 0);
    if (!init) a = P4[G::own4(lane, g)];
    uint32_t as[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
    for (int i = 0; i < 4; ++i)
      as[i] = MINUS ? mac_sub(as[i], x[4 * g + i], mul[4 * g + i], pc) : mac_add(as[i], x[4 * g + i], mul[4 * g + i], pc);
    if (to_regs) {
#pragma unroll
      for (int i = 0; i < 4; ++i) x[4 * g + i] = as[i];
    } else {
      P4[G::own4(lane, g)] = make_uint4(as[0], as[1], as[2], as[3]);
    }
  }
}
// (the sign is tested once, outside the element loops: a per-element select of mac_add / mac_sub made the compiler
// branch per coefficient; `mul` must be a register array of the caller, never a pointer chosen at run time, or both
// candidates end up in scratch memory)
template <int LOGN, bool to_regs, class TM = WaveTeam>
__device__ __forceinline__ void mac_park(uint32_t* x, const uint32_t* mul, bool minus, uint4* P4, int lane, bool init,
                                         const PrimeConsts& pc) {
  if (minus) mac_park_signed<LOGN, to_regs, true, TM>(x, mul, P4, lane, init, pc);
  else mac_park_signed<LOGN, to_regs, false, TM>(x, mul, P4, lane, init, pc);
}

// Inverse transform of a finished accumulator and Garner step `pi` of `np` against the row's global state lines.
// Returns true when the row's value is complete: acc[e] then holds X mod q in [0,q) for coefficient e*64 + lane.
template <int LOGN, bool OPQ, class TM = WaveTeam>
__device__ __forceinline__ bool inverse_fold_global(int pi, int np, uint32_t* acc, int lane, uint32_t* lds,
                                                    const uint32_t* __restrict__ twi, const PrimeConsts& pc,
                                                    uint32_t* __restrict__ stA, uint32_t* __restrict__ stB,
                                                    const DevTables& T, const uint32_t* __restrict__ tw2i = nullptr) {
  using G = Geo<LOGN, TM::LL>;
  constexpr int E = G::E;
  int li = lane;
  RZK_OPAQUE(li);
  uint4* __restrict__ A4 = reinterpret_cast<uint4*>(stA);
  uint4* __restrict__ B4 = reinterpret_cast<uint4*>(stB);
  // the state words this step needs are requested before the transform, which hides their latency
  // (N <= 1024; at N = 2048 a lane holds 32 coefficients and the registers are not there)
  constexpr bool EARLY = E <= 16;
  uint4 sa[E / 4], sb[E / 4];
  if (EARLY && pi >= 1) {
#pragma unroll
    for (int g = 0; g < E / 4; ++g) sa[g] = A4[G::own4(li, g)];
  }
  if (EARLY && pi == 2) {
#pragma unroll
    for (int g = 0; g < E / 4; ++g) sb[g] = B4[G::own4(li, g)];
  }
  wave_inv<LOGN, TM, TeamTwLds<TM>::value, TeamTw3Lds<TM>::value>(acc, li, lds, twi, pc, tw2i);
  if (!EARLY && pi >= 1) {
#pragma unroll
    for (int g = 0; g < E / 4; ++g) sa[g] = A4[G::own4(li, g)];
  }
  if (!EARLY && pi == 2) {
#pragma unroll
    for (int g = 0; g < E / 4; ++g) sb[g] = B4[G::own4(li, g)];
  }
  if (pi == 0) {
    if (np == 1) {
#pragma unroll
      for (int e = 0; e < E; ++e) acc[e] = crt1_zq(acc[e], T.pc, T.crt);
      return true;
    }
    if (np == 2) {   // sign-test form (rzk_core.h): the first digit is the canonical residue itself
#pragma unroll
      for (int e = 0; e < E; ++e) acc[e] = crt2_digit0(acc[e], T.pc);
    } else {
#pragma unroll
      for (int e = 0; e < E; ++e) acc[e] = crt_fold0(acc[e], np, T.pc, T.crt);
    }
#pragma unroll
    for (int g = 0; g < E / 4; ++g) A4[G::own4(li, g)] = make_uint4(acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]);
    return false;
  }
  if (pi == 1 && np == 2) {
    if (T.diet & DIET_CRT2) {   // (the choice is made outside the element loops, as in mac_park)
#pragma unroll
      for (int g = 0; g < E / 4; ++g) {
        const uint4 dv = sa[g];
        const uint32_t d0[4] = {dv.x, dv.y, dv.z, dv.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[4 * g + i] = crt2_zq_short(acc[4 * g + i], d0[i], T.pc, T.crt);
      }
      return true;
    }
#pragma unroll
    for (int g = 0; g < E / 4; ++g) {
      const uint4 dv = sa[g];
      const uint32_t d0[4] = {dv.x, dv.y, dv.z, dv.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[4 * g + i] = crt2_zq(acc[4 * g + i], d0[i], T.pc, T.crt);
    }
    return true;
  }
  if (pi == 1) {
#pragma unroll
    for (int g = 0; g < E / 4; ++g) {
      const uint4 dv = sa[g];
      const uint32_t d0[4] = {dv.x, dv.y, dv.z, dv.w};
      uint32_t va[4], vb[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint32_t d1 = crt_digit1(acc[4 * g + i], d0[i], np, T.pc, T.crt);
        va[i] = crt_value01_modq(d0[i], d1, T.crt);
        vb[i] = crt_value01_modp2(d0[i], d1, T.pc, T.crt);
      }
      A4[G::own4(li, g)] = make_uint4(va[0], va[1], va[2], va[3]);
      B4[G::own4(li, g)] = make_uint4(vb[0], vb[1], vb[2], vb[3]);
    }
    return false;
  }
#pragma unroll
  for (int g = 0; g < E / 4; ++g) {
    const uint4 av = sa[g], bv = sb[g];
    uint32_t a[4] = {av.x, av.y, av.z, av.w};
    const uint32_t bb[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      crt_fold2(acc[4 * g + i], T.pc, T.crt, a[i], bb[i]);
      acc[4 * g + i] = crt_finish_zq(a[i], 3, T.crt);
    }
  }
  return true;
}

// u[e] = the row's product sum mod q (coefficient e*64 + lane; zero when the row has no products): adds the sum of
// the row's rotation terms (st_sh, left in the wave's scratch line by the same lanes), the plain additions, then
// store / zero test, norm marks of checked additions, canonical-input test of everything loaded.
template <int LOGN, int CHMAX = 16, class TM = WaveTeam, class C = int64_t>
__device__ __forceinline__ void finish_row(uint32_t* u, const Program* __restrict__ prog, const Row row,
                                           const Operands& ops, uint32_t b, uint32_t bo, int lane, const DevTables& T,
                                           uint8_t* __restrict__ flags, const uint32_t* __restrict__ st_sh) {
  using G = Geo<LOGN, TM::LL>;
  constexpr int E = G::E;
  constexpr int N = G::N;
  const uint32_t q = T.crt.q, qhalf = T.crt.qhalf;
  const bool trusted = ops.trusted != 0;
  if (st_sh) {
#pragma unroll
    for (int e = 0; e < E; ++e) u[e] = addq(u[e], st_sh[G::j_p1(lane, e)], q);
  }
  // An addition is loaded with up to 16 of a lane's coefficients in flight (a row's wall time is dominated by how
  // often it waits for HBM; 16 sixty-four-bit values are what the register budget of 4 waves per SIMD leaves room for).
  constexpr int CH = E < CHMAX ? E : CHMAX;
  float add_ss[4] = {0.f, 0.f, 0.f, 0.f};
  uint32_t in_bad = 0, in_mx = 0;
  int nz = 0;
#pragma unroll
  for (int e0 = 0; e0 < E; e0 += CH) {
#pragma unroll 1
    for (uint32_t a = 0; a < row.nadds; ++a) {
      const AddTerm ad = table_load(&prog->adds[row.add0 + a]);
      add_chunk<LOGN, CH, TM, C>(u + e0, ad, a, operand_ptr<C>(ops, ad.op & ADD_OP_MASK, ad.off, b, bo, N), lane, e0, q, qhalf, trusted,
                          in_bad, in_mx, add_ss);
    }
    if (row.mode == MODE_STORE) {
      C* __restrict__ dst = const_cast<C*>(operand_ptr<C>(ops, row.out_op, row.out_off, b, bo, N));
#pragma unroll
      for (int i = 0; i < CH; ++i) st_stream(dst + G::j_p1(lane, e0 + i), (C)center_from_zq(u[e0 + i], T.crt));
    } else {
#pragma unroll
      for (int i = 0; i < CH; ++i) nz |= (u[e0 + i] != 0);
    }
  }
  if (row.mode != MODE_STORE) {
    if (__any(nz) && (lane & 63) == 0) flags[bo] = 0;
  }
  if (row.nadds && !trusted && canon_fail(in_bad, in_mx, qhalf)) input_fault(ops, flags, bo, lane);
  if (ops.norm_limit) checked_add_verdicts<LOGN, TM, C>(prog, row, ops, b, bo, lane, add_ss, flags);
}

// Workgroups: four independent one-wavefront teams (16-wave workgroups whose SIMD mates ranked each other through an LDS
// table for exact fairness measured slower in round 2 — verify rows 90 vs 81 us — and were removed), sixteen of them
// around one image of every vector twiddle (WaveTeamTw3, RZK_TW_LDS=2: off by default, the shape costs more than the image
// gains), or ONE two-wavefront team (PairTeam, N = 2048).  Teams of two are compiled for 4 waves per SIMD (<= 128 VGPRs: 16
// coefficients per thread, the budget of the N = 1024 kernels).
// The coefficient type of the launch's slabs comes with the team (TeamCoef, rzk_wave.h): int64_t for every team of
// rzk_kernels.hip, int32_t for WaveTeam32, which rzk_slab32_dev.hip instantiates.
template <int LOGN, bool HAS_VEC, bool HAS_SHIFT, class TM = WaveTeam>
__global__ void __launch_bounds__(TM::kTeamsPerBlock << TM::LL, ((LOGN <= 10 && HAS_VEC) || TM::LL == 7 ? 4 : 1))   // vector x vector variants: hold the 4 waves per SIMD the LDS allows
unit_kernel(const Program* __restrict__ prog, const WaveProgram* __restrict__ wp, const Operands ops,
            const uint32_t* __restrict__ key_ntt, const double* __restrict__ key_l2, const DevTables* __restrict__ Tp,
            const uint32_t* __restrict__ tw_all, uint32_t* __restrict__ scratch, uint8_t* __restrict__ flags,
            const uint32_t ntasks, const uint32_t units_per_task, const uint32_t tasks_per_entry,
            const uint32_t work_per_task) {
  using G = Geo<LOGN, TM::LL>;
  using C = typename TeamCoef<TM>::type;   // coefficient type of the slabs
  constexpr int E = G::E;
  constexpr int N = G::N;
  constexpr bool OPQ = true;   // opaque lane ids: stops hoisting of lane-dependent addresses (91 vs 137 VGPRs at N = 1024)
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int lane = threadIdx.x & (G::LANES - 1);                                         // index inside the team
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> TM::LL);           // team of the workgroup
  constexpr int WPB = TM::kTeamsPerBlock;
  uint32_t* lds = smem + wave * (G::LDS_WORDS + N);             // transposition slab, then P
  uint4* P4 = reinterpret_cast<uint4*>(lds + G::LDS_WORDS);     // G::LDS_WORDS * 4 is a multiple of 16 bytes
  // Teams with the phase-2 twiddles in LDS (TeamTwLds): the images of every prime and direction lie behind the teams'
  // slabs, are copied from the global tables once per workgroup, and are read-only from the barrier on, over every
  // grid-stride trip.  Nothing else in the kernel meets at a workgroup barrier: the teams stay independent.
  // Teams with every vector twiddle in LDS (TeamTw3Lds): the same, with the phase-3 entries behind each table's phase-2 words.
  constexpr bool TWL = TeamTwLds<TM>::value, TW3 = TeamTw3Lds<TM>::value;
  using TWI = typename TeamTwImg<LOGN, TM>::type;
  const uint32_t* tw2_img = smem + WPB * (G::LDS_WORDS + N);
  if (TWL) {
    static_assert(!TWL || (TWI::kFits && WPB * (G::LDS_WORDS + N) % 4 == 0 && (WPB << TM::LL) == TWI::WORDS),
                  "one image word per thread and table, 16-byte aligned behind the slabs");
    const int src = TWI::src((int)threadIdx.x);
#pragma unroll
    for (int t = 0; t < TWI::TABLES; ++t)
      smem[WPB * (G::LDS_WORDS + N) + t * TWI::WORDS + threadIdx.x] = tw_all[(size_t)t * kTableLen + src];
    __syncthreads();
  }
  // per-wave global scratch: Garner words [row A | B][word A | B][N], then the sum of row A's rotation terms
  uint32_t* st = scratch + ((size_t)blockIdx.x * WPB + wave) * (size_t)(kScratchLines * N + 16);
  uint32_t* st_sh = st + 4 * N;
#if RZK_STAMPS   // diagnostic build only (tools/wave_timeline.py): when each wavefront ran and where
  const uint64_t stamp0 = __builtin_amdgcn_s_memrealtime();
  const uint64_t cyc0 = __builtin_amdgcn_s_memtime();
  uint64_t t_load = 0, t_fwd = 0, t_mac = 0, t_inv = 0, t_fin = 0, t_rot = 0;
#endif
  const DevTables& T = *Tp;
  const uint32_t qhalf = T.crt.qhalf;
  const bool trusted = ops.trusted != 0;
  const uint32_t nunits = wp->nunits;

  // progress of this wave through its share of the launch, in transforms (work_per_task: the host's estimate)
  const uint32_t first_task = blockIdx.x * WPB + wave;
  const uint32_t my_tasks = first_task < ntasks ? (ntasks - first_task + gridDim.x * WPB - 1) / (gridDim.x * WPB) : 0;
  const uint32_t work_total = my_tasks * work_per_task;
  uint32_t work_done = 0;
#define RZK_STEP_PRIORITY()                             \
  do {                                                  \
    set_progress_priority(work_done, work_total);       \
    ++work_done;                                        \
  } while (0)

  for (uint32_t task = first_task; task < ntasks; task += gridDim.x * WPB) {
    const uint32_t b = task / tasks_per_entry;
    const uint32_t u0 = (task - b * tasks_per_entry) * units_per_task;
    const uint32_t u1 = u0 + units_per_task < nunits ? u0 + units_per_task : nunits;
    const uint32_t bo = ops.group > 1 ? b / ops.group : b;
    if (ops.preset) {   // this team evaluates every row of the entry (host: one task per entry, one flag per entry): it owns the flag
      if (lane == 0) flags[bo] = (uint8_t)ops.preset;
      if (TM::LL != 6) TM::sync();   // the other wavefront of a pair may clear it
    }
#pragma unroll 1
    for (uint32_t ui = u0; ui < u1; ++ui) {   // (rotating the unit order per workgroup measured no gain)
      const Unit un = table_load(&wp->units[ui]);
      const Row rowA = table_load(&prog->rows[un.rowA]);
      const bool pair = un.rowB != kNoRow;
      const uint32_t un_items = un.nitems;
      const bool null_unit = un_items == 0;   // no products: additions / rotation terms only
      const bool has_shift = HAS_SHIFT && rowA.nshift > 0;
      // A single row evaluated by one wavefront takes its challenge products LAST (DIET_ROT_LAST): once its last inverse
      // transform is done the slab and P are idle (no sum of a row B is parked there), so the rotations accumulate
      // straight into the row's value in registers and the scratch line's N words are neither written nor read back.
      // (N <= 1024: rotation terms at N = 2048 exist on teams of two only — launch_units starts no one-wavefront
      // instantiation with HAS_SHIFT there — and those run their rotations first.)
      const bool rot_last = has_shift && TM::LL == 6 && E <= 16 && !pair && (T.diet & DIET_ROT_LAST) != 0;
      if (has_shift && !rot_last) {
        // challenge products first (rotations, image in slab + P); their sum mod q is built in the wave's scratch line
        // (every lane reads and writes only its own coefficients) and waits there for finish_row
        bool fault = false;
        RZK_T0();
#pragma unroll 1
        for (uint32_t t = 0; t < rowA.nshift; ++t) {
          const Term tm = table_load(&prog->terms[rowA.term0 + rowA.nterms + t]);
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
        TM::sync();   // the image is dead: slab and P may be overwritten
        RZK_T1(t_rot);
      }
      int np = null_unit ? 1 : kMaxPrimes;
      const uint32_t nit = null_unit ? 1u : un_items;
      float boundA = 0.f, boundB = 0.f;
#pragma unroll 1
      for (int pi = 0; pi < np; ++pi) {
        const PrimeConsts pc = T.pc[pi];
        const uint32_t* __restrict__ twf = tw_all + (size_t)(2 * pi) * kTableLen;
        const uint32_t* __restrict__ tw2f = tw2_img + (2 * pi) * TWI::WORDS;   // (TWL) forward image, then the inverse one
        const bool first = pi == 0;
        bool fault = false;
#pragma unroll 1
        for (uint32_t it = 0; it < nit; ++it) {
          // every array below is local to one trip: nothing is carried in registers from item to item
          const bool last = it + 1 == nit;
          RZK_STEP_PRIORITY();
          int ln = lane;
          RZK_OPAQUE(ln);
          uint32_t acc[E];    // with the last item: row A's sum
#pragma unroll
          for (int c = 0; c < E; ++c) acc[c] = 0;
          if (!null_unit) {
            const Item im = table_load(&wp->items[un.item0 + it]);
            uint32_t x[E];      // the current transform
            float nb = 0.f;
            bool below = true;
            const bool chk = first && (im.flags & (TERM_CHECK | TERM_CHECK2));
            {
              RZK_T0();
              load_lift<LOGN, TM, LL_FUSED, C>(x, operand_ptr<C>(ops, im.b_op, im.b_off, b, bo, N), ln, pc, first, nb, chk, ops.norm_limit, below, qhalf,
                              trusted, fault);
              RZK_T1(t_load);
            }
            if (chk && !below && (lane & 63) == 0) fail_check(flags + bo, ops.pad != 0, (im.flags & TERM_CHECK2) != 0);
            const bool vec = HAS_VEC && im.kind == ITEM_VEC;
            // ITEM_DOT2: row A is x1 k1 + x2 k2.  The first item parks its TRANSFORM in P (the same N words as its product) and
            // requests no key entry; the last one takes both entries and reduces the two-term sum once (dot2_lazy).
            // One wavefront, N <= 1024 (two key entries in registers next to the transform).
            const bool dot2 = !HAS_VEC && TM::LL == 6 && E <= 16 && (im.flags & ITEM_DOT2) != 0;
            // the resident key entry of row A's product is requested before the transform, which hides its latency
            // (N <= 1024; at N = 2048 the registers are not there and the entry is loaded after the transform)
            constexpr bool EARLY = E <= 16 && !HAS_VEC;   // (and not next to vector x vector items: their second transform needs the registers)
            uint32_t kreg[E];
            const uint4* __restrict__ kpA = reinterpret_cast<const uint4*>(key_ntt + ((size_t)im.keyA * kKeyImages + pi) * N);
            const bool want_key = !vec && im.keyA != kNoKey && !(dot2 && !last);
            if (EARLY && want_key) {
#pragma unroll
              for (int g = 0; g < E / 4; ++g) {
                const uint4 kv = kpA[G::key4(ln, g)];
                kreg[4 * g] = kv.x, kreg[4 * g + 1] = kv.y, kreg[4 * g + 2] = kv.z, kreg[4 * g + 3] = kv.w;
              }
            }
            {
              RZK_T0();
              wave_fwd<LOGN, TM, TWL, TW3>(x, ln, lds, twf, pc, tw2f);
              RZK_T1(t_fwd);
            }
            if (!EARLY && want_key) {
#pragma unroll
              for (int g = 0; g < E / 4; ++g) {
                const uint4 kv = kpA[G::key4(ln, g)];
                kreg[4 * g] = kv.x, kreg[4 * g + 1] = kv.y, kreg[4 * g + 2] = kv.z, kreg[4 * g + 3] = kv.w;
              }
            }
            uint32_t xb[E];   // ITEM_VEC: b's transform with N^-1 and the Montgomery factor folded in
            if (vec) {
#pragma unroll
              for (int c = 0; c < E; ++c) xb[c] = csub(mont_lazy(x[c], pc.ninv_r2, pc.p, pc.npinv), pc.p);
              float na = 0.f;
              bool unused_below = true;
              load_lift<LOGN, TM, LL_FUSED, C>(x, operand_ptr<C>(ops, im.a_op, im.a_off, b, bo, N), ln, pc, first, na, false, 0, unused_below, qhalf,
                              trusted, fault);
              wave_fwd<LOGN, TM, TWL, TW3>(x, ln, lds, twf, pc, tw2f);
              if (first) boundA = bound_fma(na, nb, boundA);
            } else if (first) {
              if (im.keyA != kNoKey) boundA = bound_fma((float)key_l2[im.keyA], nb, boundA);
              if (pair && im.keyB != kNoKey) boundB = bound_fma((float)key_l2[im.keyB], nb, boundB);
            }
            const bool feedsA = vec || im.keyA != kNoKey;
            if (!last) {
              RZK_T0();
              if (vec) {
                mac_park<LOGN, false, TM>(x, xb, im.signA < 0, P4, ln, it == 0, pc);
              } else if (dot2) {
#pragma unroll
                for (int g = 0; g < E / 4; ++g) P4[G::own4(ln, g)] = make_uint4(x[4 * g], x[4 * g + 1], x[4 * g + 2], x[4 * g + 3]);
              } else if (feedsA) {
                mac_park<LOGN, false, TM>(x, kreg, im.signA < 0, P4, ln, it == 0, pc);
              }
              RZK_T1(t_mac);
              continue;
            }
            RZK_T0();
            // ---- last item: row A's sum leaves P and materialises in registers ...
            if (fault) input_fault(ops, flags, bo, lane);
            if (first) np = primes_for(boundA > boundB ? boundA : boundB, T);
#pragma unroll
            for (int c = 0; c < E; ++c) acc[c] = x[c];
            if (vec) {
              mac_park<LOGN, true, TM>(acc, xb, im.signA < 0, P4, ln, it == 0, pc);
            } else if (dot2) {
              // the first item's entry is requested only now (before its transform nothing could hold it); a minus term
              // multiplies by p - k instead (<= p: the bound of dot2_lazy holds)
              const Item im0 = table_load(&wp->items[un.item0]);
              const uint4* __restrict__ kp1 = reinterpret_cast<const uint4*>(key_ntt + ((size_t)im0.keyA * kKeyImages + pi) * N);
              uint32_t k1[E];
#pragma unroll
              for (int g = 0; g < E / 4; ++g) {
                const uint4 kv = kp1[G::key4(ln, g)];
                k1[4 * g] = kv.x, k1[4 * g + 1] = kv.y, k1[4 * g + 2] = kv.z, k1[4 * g + 3] = kv.w;
              }
              if (im.signA < 0) {
#pragma unroll
                for (int c = 0; c < E; ++c) kreg[c] = pc.p - kreg[c];
              }
              if (im0.signA < 0) {
#pragma unroll
                for (int c = 0; c < E; ++c) k1[c] = pc.p - k1[c];
              }
#pragma unroll
              for (int g = 0; g < E / 4; ++g) {
                const uint4 v = P4[G::own4(ln, g)];   // x1, consumed before a row B's product takes the slot (below)
                const uint32_t x1[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[4 * g + i] = dot2_lazy(x1[i], k1[4 * g + i], x[4 * g + i], kreg[4 * g + i], pc);
              }
            } else if (feedsA) {
              mac_park<LOGN, true, TM>(acc, kreg, im.signA < 0, P4, ln, it == 0, pc);
            } else {   // (an item that only feeds row B)
#pragma unroll
              for (int g = 0; g < E / 4; ++g) {
                const uint4 v = P4[G::own4(ln, g)];
                acc[4 * g] = v.x, acc[4 * g + 1] = v.y, acc[4 * g + 2] = v.z, acc[4 * g + 3] = v.w;
              }
            }
            if (pair) {   // ... and row B's only product, from the same transform, takes its place in P
              const uint4* __restrict__ kb = reinterpret_cast<const uint4*>(key_ntt + ((size_t)im.keyB * kKeyImages + pi) * N);
              uint32_t kbr[E];
#pragma unroll
              for (int g = 0; g < E / 4; ++g) {
                const uint4 kv = kb[G::key4(ln, g)];
                kbr[4 * g] = kv.x, kbr[4 * g + 1] = kv.y, kbr[4 * g + 2] = kv.z, kbr[4 * g + 3] = kv.w;
              }
              mac_park<LOGN, false, TM>(x, kbr, im.signB < 0, P4, ln, true, pc);
            }
            RZK_T1(t_mac);
          }
          // ---- transform back, fold, and after the last prime finish the row(s) of the unit
#pragma unroll 1
          for (uint32_t r = 0; r < (pair ? 2u : 1u); ++r) {
            if (r == 1) {
#pragma unroll
              for (int g = 0; g < E / 4; ++g) {
                const uint4 v = P4[G::own4(ln, g)];
                acc[4 * g] = v.x, acc[4 * g + 1] = v.y, acc[4 * g + 2] = v.z, acc[4 * g + 3] = v.w;
              }
            }
            bool done = true;
            RZK_STEP_PRIORITY();
            if (!null_unit) {
              RZK_T0();
              done = inverse_fold_global<LOGN, OPQ, TM>(pi, np, acc, lane, lds, twf + kTableLen, pc, st + (size_t)(2 * r) * N,
                                                    st + (size_t)(2 * r + 1) * N, T, tw2f + TWI::WORDS);
              RZK_T1(t_inv);
            }
            if (done && rot_last) {   // (a single row: r == 0) acc[e] is the value of coefficient e*64 + lane, the register layout of the rotations
              RZK_T0();
              bool sfault = false;
#pragma unroll 1
              for (uint32_t t = 0; t < rowA.nshift; ++t) {
                const Term tm = table_load(&prog->terms[rowA.term0 + rowA.nterms + t]);
                const C* __restrict__ pa = operand_ptr<C>(ops, tm.a_op, tm.a_off, b, bo, N);
                int32_t a[E];
                if (trusted) {
#pragma unroll
                  for (int e = 0; e < E; ++e) a[e] = (int32_t)pa[G::j_p1(lane, e)];
                } else {
                  uint32_t abad = 0, amx = 0;
#pragma unroll
                  for (int e = 0; e < E; ++e) a[e] = canon_lo_mx(pa[G::j_p1(lane, e)], qhalf, abad, amx);
                  sfault = sfault || canon_fail(abad, amx, qhalf);
                }
                shift_product<LOGN, false, false, TM, kShiftHMem, C>(acc, false, tm.sign < 0, a, operand_ptr<C>(ops, tm.b_op, tm.b_off, b, bo, N), lane,
                                                  reinterpret_cast<int32_t*>(lds), T, sfault, trusted);
              }
              if (sfault) input_fault(ops, flags, bo, lane);
              TM::sync();   // the image is dead: slab and P may be overwritten
              RZK_T1(t_rot);
            }
            if (done) {
              RZK_T0();
              finish_row<LOGN, 16, TM, C>(acc, prog, table_load(&prog->rows[r ? un.rowB : un.rowA]), ops, b, bo, lane, T, flags,
                               (has_shift && !rot_last && r == 0) ? st_sh : nullptr);
              RZK_T1(t_fin);
            }
          }
        }
      }
    }
  }
#undef RZK_STEP_PRIORITY
#if RZK_STAMPS
  if (lane == 0) {
    const uint64_t stamp1 = __builtin_amdgcn_s_memrealtime();
    uint32_t hwid;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
    uint32_t xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    uint32_t* o = st + kScratchLines * N;
    o[0] = (uint32_t)stamp0, o[1] = (uint32_t)(stamp0 >> 32), o[2] = (uint32_t)stamp1, o[3] = (uint32_t)(stamp1 >> 32);
    o[4] = hwid, o[5] = xcc, o[6] = blockIdx.x, o[7] = wave;
    const uint64_t cyc1 = __builtin_amdgcn_s_memtime();
    o[8] = (uint32_t)(cyc1 - cyc0);   // shader-clock cycles of the wave's lifetime
    o[9] = (uint32_t)t_load, o[10] = (uint32_t)t_fwd, o[11] = (uint32_t)t_mac, o[12] = (uint32_t)t_inv, o[13] = (uint32_t)t_fin, o[14] = (uint32_t)t_rot;
  }
#endif
}

// =============================================================================================
// unit_io_kernel ("item outer"): the default evaluation of KEY-PRODUCT programs — every operand is read from HBM ONCE.
//
// Why: the round-3 experiment of DESIGN.md §6 (the same launches with every operand L2-resident: commit 130 -> 100 us,
// verify 76 -> 65 us) showed that unit_kernel's launches are co-bound by HBM traffic: 1.8 x the algorithmic bytes, because
// its prime-outer loop re-reads every operand for the second prime and keeps the Garner state of a row in global lines
// across a whole prime pass (evicted long before it is read back).  Here the loops are swapped:
//   for every item (operand): load it once — canonical test, norm measurement, norm mark — keep the low words in
//     registers, and for primes 0 and 1: lift, forward transform, multiply into that prime's sum of every row it feeds;
//   the sums wait in parking spots between items: row A / prime 0 in LDS (buffer P), the others (row A / prime 1, a
//     pair's row B) in the team's scratch lines in global memory, which are re-used within microseconds and stay in L2;
//   then per row: inverse transform of prime 0, first digit in REGISTERS, inverse transform of prime 1, sign-test
//     reconstruction (crt2_zq), finish_row.  No Garner state ever leaves the registers.
// Two primes are computed for every row (a row that one prime would cover is still exact with two).  Rows that need
// the third prime (full-range operands: Mat::dot on arbitrary vectors, tests) are detected once all operands have been
// measured and take one more pass over the items for prime 2 (operands re-read: the rare path), with the offset-form
// Garner steps in registers.  Everything else — units, pairs, rotation terms first, finish_row, norm marks, input
// faults, progress priorities, teams of one or two wavefronts — is unit_kernel's.
// Parking lines of a team (N words each): 0 = A/p1, 1 = B/p0, 2 = B/p1, 3 = A/p2, 4 = rotation sums, 5 = B/p2.
// =============================================================================================
template <int LOGN, class TM = WaveTeam, class C = int64_t>
__device__ __forceinline__ void load_measure(int32_t* v, const C* __restrict__ src, int lane, bool measure, float& nrm2,
                                             bool check, uint64_t limit, bool& below, uint32_t qhalf, bool trusted, bool& fault) {
  using G = Geo<LOGN, TM::LL>;
  if (!measure || trusted) {
#pragma unroll
    for (int e = 0; e < G::E; ++e) v[e] = (int32_t)src[G::j_p1(lane, e)];
  } else {
    uint32_t bad = 0, mx = 0;
#pragma unroll
    for (int e = 0; e < G::E; ++e) v[e] = canon_lo_mx(src[G::j_p1(lane, e)], qhalf, bad, mx);
    fault = fault || canon_fail(bad, mx, qhalf);
  }
  if (measure) {
    const float ss = TM::sum_f32(lane_sum_sq_f32<G::E>(v));
    nrm2 = norm2_upper(ss);
    if (check) below = norm_below<G::E, TM>(v, ss, limit);
  }
}
// a parked sum (16-byte slots of the team's own threads) -> registers
template <int LOGN, class TM, class P4T>
__device__ __forceinline__ void unpark(uint32_t* a, P4T P4, int lane) {
  using G = Geo<LOGN, TM::LL>;
#pragma unroll
  for (int g = 0; g < G::E / 4; ++g) {
    const uint4 v = P4[G::own4(lane, g)];
    a[4 * g] = v.x, a[4 * g + 1] = v.y, a[4 * g + 2] = v.z, a[4 * g + 3] = v.w;
  }
}

// Where the sums park between items (LDS budget: 10 KiB per wavefront at 4 waves per SIMD):
//   N = 512   slab 2.1 KiB + A/p0, A/p1, B/p0 (2 KiB each) = 8.1 KiB: only B/p1 and the third-prime sums use global
//             lines.  This is the default kernel of key-product programs at N = 512 (Open cycle 27.1 -> 29.6 M proofs/s).
//   N >= 1024 A/p0 in LDS, everything else in global lines: slower than unit_kernel (Open N = 1024: commit 145 vs 129 us;
//             a variant with a half-size transposition slab and both A sums in LDS: 139-146 us — the two-round
//             transpositions need ~127 VGPRs before any key entry can be requested ahead of a transform, see
//             DESIGN.md §6), so it is reachable only through RZK_UNIT_IO=1 (tests).
template <int LOGN, int LL>
struct IoCfg {
  static constexpr bool P1_FULL = LOGN == 9;                      // A / prime 1 in an LDS buffer
  static constexpr bool B0_LDS = LOGN == 9;                       // B / prime 0 in an LDS buffer
  static constexpr int N = 1 << LOGN;
  static constexpr int SLAB = Geo<LOGN, LL>::LDS_WORDS;
  static constexpr int OFF_P1 = SLAB + N;
  static constexpr int OFF_B0 = OFF_P1 + (P1_FULL ? N : 0);
  static constexpr int WORDS = OFF_B0 + (B0_LDS ? N : 0);         // LDS words per team
};
template <int LOGN, bool HAS_SHIFT, class TM = WaveTeam>
__global__ void __launch_bounds__(TM::kTeamsPerBlock << TM::LL, (TM::LL == 7 || LOGN == 10 ? 4 : 1))   // 16 coefficients per thread: 4 waves per SIMD
unit_io_kernel(const Program* __restrict__ prog, const WaveProgram* __restrict__ wp, const Operands ops,
               const uint32_t* __restrict__ key_ntt, const double* __restrict__ key_l2, const DevTables* __restrict__ Tp,
               const uint32_t* __restrict__ tw_all, uint32_t* __restrict__ scratch, uint8_t* __restrict__ flags,
               const uint32_t ntasks, const uint32_t units_per_task, const uint32_t tasks_per_entry,
               const uint32_t work_per_task) {
  using G = Geo<LOGN, TM::LL>;
  using C = typename TeamCoef<TM>::type;   // coefficient type of the slabs
  constexpr int E = G::E;
  constexpr int N = G::N;
  constexpr bool OPQ = true;
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int lane = threadIdx.x & (G::LANES - 1);
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> TM::LL);
  constexpr int TPB = TM::kTeamsPerBlock;
  // Where LDS allows (N = 512, IoCfg) the prime-1 sum of row A and the prime-0 sum of row B park in LDS buffers of their
  // own instead of global lines
  using IO = IoCfg<LOGN, TM::LL>;
  constexpr bool P1L = IO::P1_FULL, B0L = IO::B0_LDS;
  uint32_t* lds = smem + wave * IO::WORDS;                                          // transposition slab, then the parking buffers
  uint4* P4 = reinterpret_cast<uint4*>(lds + IO::SLAB);                             // A / prime 0
  uint4* P41 = reinterpret_cast<uint4*>(lds + IO::OFF_P1);                          // A / prime 1   (P1L)
  uint4* PB0 = reinterpret_cast<uint4*>(lds + IO::OFF_B0);                          // B / prime 0   (B0L)
  uint32_t* st = scratch + ((size_t)blockIdx.x * TPB + wave) * (size_t)(kScratchLines * N + 16);
  uint32_t* st_sh = st + 4 * N;
#if RZK_STAMPS
  const uint64_t stamp0 = __builtin_amdgcn_s_memrealtime();
  const uint64_t cyc0 = __builtin_amdgcn_s_memtime();
#endif
  const DevTables& T = *Tp;
  const uint32_t qhalf = T.crt.qhalf;
  const bool trusted = ops.trusted != 0;
  const uint32_t nunits = wp->nunits;
  const uint32_t first_task = blockIdx.x * TPB + wave;
  const uint32_t my_tasks = first_task < ntasks ? (ntasks - first_task + gridDim.x * TPB - 1) / (gridDim.x * TPB) : 0;
  const uint32_t work_total = my_tasks * work_per_task;
  uint32_t work_done = 0;
#define RZK_STEP_PRIORITY()                             \
  do {                                                  \
    set_progress_priority(work_done, work_total);       \
    ++work_done;                                        \
  } while (0)

  for (uint32_t task = first_task; task < ntasks; task += gridDim.x * TPB) {
    const uint32_t b = task / tasks_per_entry;
    const uint32_t u0 = (task - b * tasks_per_entry) * units_per_task;
    const uint32_t u1 = u0 + units_per_task < nunits ? u0 + units_per_task : nunits;
    const uint32_t bo = ops.group > 1 ? b / ops.group : b;
    if (ops.preset) {   // as in unit_kernel: the team that evaluates the whole entry initialises its flag
      if (lane == 0) flags[bo] = (uint8_t)ops.preset;
      if (TM::LL != 6) TM::sync();
    }
#pragma unroll 1
    for (uint32_t ui = u0; ui < u1; ++ui) {
      const Unit un = table_load(&wp->units[ui]);
      const Row rowA = table_load(&prog->rows[un.rowA]);
      const bool pair = un.rowB != kNoRow;
      const uint32_t nit = un.nitems;
      const bool has_shift = HAS_SHIFT && rowA.nshift > 0;
      if (has_shift) {
        // challenge products first (rotations, image in slab + P); their sum mod q waits in the team's line 4
        bool fault = false;
#pragma unroll 1
        for (uint32_t t = 0; t < rowA.nshift; ++t) {
          const Term tm = table_load(&prog->terms[rowA.term0 + rowA.nterms + t]);
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
        TM::sync();   // the image is dead: slab and P may be overwritten
      }
      if (nit == 0) {   // no products: additions / rotation terms only
        uint32_t u[E];
#pragma unroll
        for (int e = 0; e < E; ++e) u[e] = 0;
        RZK_STEP_PRIORITY();
        finish_row<LOGN, 16, TM, C>(u, prog, rowA, ops, b, bo, lane, T, flags, has_shift ? st_sh : nullptr);
        continue;
      }
      // ---- the items: pass 0 = primes 0 and 1 (operands measured), pass 1 = prime 2, only when the bound asks for it
      float boundA = 0.f, boundB = 0.f;
      bool fault = false, haveA = false;
      int np = 2;
#pragma unroll 1
      for (int pass = 0; pass < (np == 3 ? 2 : 1); ++pass) {
        haveA = false;
#pragma unroll 1
        for (uint32_t it = 0; it < nit; ++it) {
          const bool last = it + 1 == nit;
          int ln = lane;
          RZK_OPAQUE(ln);
          const Item im = table_load(&wp->items[un.item0 + it]);
          const C* __restrict__ src = operand_ptr<C>(ops, im.b_op, im.b_off, b, bo, N);
          const bool chk = pass == 0 && (im.flags & (TERM_CHECK | TERM_CHECK2));
          const bool feedsA = im.keyA != kNoKey;
          const bool feedsB = pair && last && im.keyB != kNoKey;
          const int pi0 = pass == 0 ? 0 : 2, pi1 = pass == 0 ? 2 : 3;
          // The operand's one trip from HBM: canonical test, norm measurement, norm mark (first pass).  With 8
          // coefficients per lane the low words simply stay in registers for the second prime (RETAIN); with 16 or
          // more they are read again — microseconds later, out of L2 — because keeping them through a transform costs
          // the registers that hold the kernel at 4 waves per SIMD.
          constexpr bool RETAIN = E <= 8;
          int32_t vkeep[RETAIN ? E : 1];
          if (RETAIN) {
            float nb = 0.f;
            bool below = true;
            load_measure<LOGN, TM, C>(vkeep, src, ln, pass == 0, nb, chk, ops.norm_limit, below, qhalf, trusted, fault);
            if (chk && !below && (lane & 63) == 0) fail_check(flags + bo, ops.pad != 0, (im.flags & TERM_CHECK2) != 0);
            if (pass == 0) {
              if (feedsA) boundA = bound_fma((float)key_l2[im.keyA], nb, boundA);
              if (pair && im.keyB != kNoKey) boundB = bound_fma((float)key_l2[im.keyB], nb, boundB);
            }
          }
#pragma unroll 1
          for (int pi = pi0; pi < pi1; ++pi) {
            RZK_STEP_PRIORITY();
            RZK_OPAQUE(ln);   // per transform: lane-dependent addresses must not be hoisted out of this loop (30 VGPRs)
            const PrimeConsts pc = T.pc[pi];
            const uint32_t* __restrict__ twf = tw_all + (size_t)(2 * pi) * kTableLen;
            uint32_t x[E];
            if (RETAIN) {
#pragma unroll
              for (int e = 0; e < E; ++e) x[e] = lift(vkeep[RETAIN ? e : 0], pc);
            } else if (pi == pi0) {
              int32_t v[E];
              float nb = 0.f;
              bool below = true;
              load_measure<LOGN, TM, C>(v, src, ln, pass == 0, nb, chk, ops.norm_limit, below, qhalf, trusted, fault);
              if (chk && !below && (lane & 63) == 0) fail_check(flags + bo, ops.pad != 0, (im.flags & TERM_CHECK2) != 0);
              if (pass == 0) {
                if (feedsA) boundA = bound_fma((float)key_l2[im.keyA], nb, boundA);
                if (pair && im.keyB != kNoKey) boundB = bound_fma((float)key_l2[im.keyB], nb, boundB);
              }
#pragma unroll
              for (int e = 0; e < E; ++e) x[e] = lift(v[e], pc);
            } else {
              const int32_t* __restrict__ lo32 = reinterpret_cast<const int32_t*>(src);
#pragma unroll
              for (int e = 0; e < E; ++e) x[e] = lift(lo32[(int)(sizeof(C) / 4) * G::j_p1(ln, e)], pc);
            }
            // (requesting row A's key entry before the transform, as unit_kernel does, does not pay here:)
            constexpr bool EARLY = false;   // (measured at N = 512: 42.3 us against 40.4 for the verify rows; at N = 1024 the entry
                                            //  would cost 30 VGPRs across the transform)
            const uint4* __restrict__ kpA = reinterpret_cast<const uint4*>(key_ntt + ((size_t)(feedsA ? im.keyA : 0) * kKeyImages + pi) * N);
            uint32_t kreg[E];
            if (EARLY && feedsA) {
              // ... but not ahead of the operand itself: the request is tied to the last lifted coefficient, or the scheduler
              // issues it first and the entry sits in registers next to the 64-bit loads of the operand (+32 VGPRs)
              int lk = ln;
              asm volatile("" : "+v"(lk) : "v"(x[E - 1]));
#pragma unroll
              for (int g = 0; g < E / 4; ++g) {
                const uint4 kv = kpA[G::key4(lk, g)];
                kreg[4 * g] = kv.x, kreg[4 * g + 1] = kv.y, kreg[4 * g + 2] = kv.z, kreg[4 * g + 3] = kv.w;
              }
            }
            wave_fwd<LOGN, TM>(x, ln, lds, twf, pc);
            if (feedsA) {
              if (!EARLY) {
#pragma unroll
                for (int g = 0; g < E / 4; ++g) {
                  const uint4 kv = kpA[G::key4(ln, g)];
                  kreg[4 * g] = kv.x, kreg[4 * g + 1] = kv.y, kreg[4 * g + 2] = kv.z, kreg[4 * g + 3] = kv.w;
                }
              }
              // (parking leaves x untouched: row B's product below is formed from the same transform)
              if (pi == 0) mac_park<LOGN, false, TM>(x, kreg, im.signA < 0, P4, ln, !haveA, pc);
              else if (P1L && pi == 1) mac_park<LOGN, false, TM>(x, kreg, im.signA < 0, P41, ln, !haveA, pc);
              else mac_park<LOGN, false, TM>(x, kreg, im.signA < 0, reinterpret_cast<uint4*>(st + (pi == 1 ? 0 : 3) * N), ln, !haveA, pc);
            }
            if (feedsB) {
              const uint4* __restrict__ kpB = reinterpret_cast<const uint4*>(key_ntt + ((size_t)im.keyB * kKeyImages + pi) * N);
              uint32_t kbr[E];
              int lb = ln;
              asm volatile("" : "+v"(lb));   // row B's entry is requested HERE, not ahead of the transform (16 VGPRs)
#pragma unroll
              for (int g = 0; g < E / 4; ++g) {
                const uint4 kv = kpB[G::key4(lb, g)];
                kbr[4 * g] = kv.x, kbr[4 * g + 1] = kv.y, kbr[4 * g + 2] = kv.z, kbr[4 * g + 3] = kv.w;
              }
              if (B0L && pi == 0) mac_park<LOGN, false, TM>(x, kbr, im.signB < 0, PB0, ln, true, pc);
              else mac_park<LOGN, false, TM>(x, kbr, im.signB < 0, reinterpret_cast<uint4*>(st + (pi == 0 ? 1 : (pi == 1 ? 2 : 5)) * N), ln, true, pc);
            }
          }
          haveA = haveA || feedsA;
        }
        if (pass == 0) {
          if (fault) input_fault(ops, flags, bo, lane);
          np = primes_for(boundA > boundB ? boundA : boundB, T);
          np = np < 2 ? 2 : np;
        }
      }
      // ---- the rows: inverse transforms back to back, reconstruction in registers
#pragma unroll 1
      for (uint32_t r = 0; r < (pair ? 2u : 1u); ++r) {
        int li = lane;
        RZK_OPAQUE(li);
        const bool have = r == 1 || haveA;
        uint32_t u[E];     // the row's value mod q
        if (!have) {
#pragma unroll
          for (int e = 0; e < E; ++e) u[e] = 0;
        } else {
          uint32_t a[E];
          if (r == 0) unpark<LOGN, TM>(a, const_cast<const uint4*>(P4), li);
          else if (B0L) unpark<LOGN, TM>(a, const_cast<const uint4*>(PB0), li);
          else unpark<LOGN, TM>(a, reinterpret_cast<const uint4*>(st + 1 * N), li);
          RZK_STEP_PRIORITY();
          RZK_OPAQUE(li);
          wave_inv<LOGN, TM>(a, li, lds, tw_all + (size_t)(2 * 0 + 1) * kTableLen, T.pc[0]);
          if (np == 2) {
#pragma unroll
            for (int e = 0; e < E; ++e) u[e] = crt2_digit0(a[e], T.pc);
            if (P1L && r == 0) unpark<LOGN, TM>(a, const_cast<const uint4*>(P41), li);
            else unpark<LOGN, TM>(a, reinterpret_cast<const uint4*>(st + (r == 0 ? 0 : 2) * N), li);
            RZK_STEP_PRIORITY();
            RZK_OPAQUE(li);
            wave_inv<LOGN, TM>(a, li, lds, tw_all + (size_t)(2 * 1 + 1) * kTableLen, T.pc[1]);
            if (T.diet & DIET_CRT2) {
#pragma unroll
              for (int e = 0; e < E; ++e) u[e] = crt2_zq_short(a[e], u[e], T.pc, T.crt);
            } else {
#pragma unroll
              for (int e = 0; e < E; ++e) u[e] = crt2_zq(a[e], u[e], T.pc, T.crt);
            }
          } else {   // three primes: the offset form, words A and B in registers
            uint32_t wb[E];
#pragma unroll
            for (int e = 0; e < E; ++e) u[e] = crt_fold0(a[e], 3, T.pc, T.crt);
            if (P1L && r == 0) unpark<LOGN, TM>(a, const_cast<const uint4*>(P41), li);
            else unpark<LOGN, TM>(a, reinterpret_cast<const uint4*>(st + (r == 0 ? 0 : 2) * N), li);
            RZK_STEP_PRIORITY();
            RZK_OPAQUE(li);
            wave_inv<LOGN, TM>(a, li, lds, tw_all + (size_t)(2 * 1 + 1) * kTableLen, T.pc[1]);
#pragma unroll
            for (int e = 0; e < E; ++e) {
              wb[e] = 0;
              crt_fold1(a[e], 3, T.pc, T.crt, u[e], wb[e]);
            }
            unpark<LOGN, TM>(a, reinterpret_cast<const uint4*>(st + (r == 0 ? 3 : 5) * N), li);
            RZK_STEP_PRIORITY();
            RZK_OPAQUE(li);
            wave_inv<LOGN, TM>(a, li, lds, tw_all + (size_t)(2 * 2 + 1) * kTableLen, T.pc[2]);
#pragma unroll
            for (int e = 0; e < E; ++e) {
              crt_fold2(a[e], T.pc, T.crt, u[e], wb[e]);
              u[e] = crt_finish_zq(u[e], 3, T.crt);
            }
          }
        }
        finish_row<LOGN, 16, TM, C>(u, prog, table_load(&prog->rows[r ? un.rowB : un.rowA]), ops, b, bo, lane, T, flags,
                                 (has_shift && r == 0) ? st_sh : nullptr);
      }
    }
  }
#undef RZK_STEP_PRIORITY
#if RZK_STAMPS
  if (lane == 0) {
    const uint64_t stamp1 = __builtin_amdgcn_s_memrealtime();
    uint32_t hwid;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
    uint32_t xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    uint32_t* o = st + kScratchLines * N;
    o[0] = (uint32_t)stamp0, o[1] = (uint32_t)(stamp0 >> 32), o[2] = (uint32_t)stamp1, o[3] = (uint32_t)(stamp1 >> 32);
    o[4] = hwid, o[5] = xcc, o[6] = blockIdx.x, o[7] = wave;
    const uint64_t cyc1 = __builtin_amdgcn_s_memtime();
    o[8] = (uint32_t)(cyc1 - cyc0);
    o[9] = o[10] = o[11] = o[12] = o[13] = o[14] = 0;
  }
#endif
}

}  // namespace rzk
