// rzk_wave.h - wave primitives: wave_sync, streaming loads / stores, DPP reductions, norms, the team types, wave_fwd / wave_inv.
// Part of the one translation unit rzk_kernels.hip (device code only; no include guards beyond #pragma once).
#pragma once
#include <hip/hip_runtime.h>
#include "rzk_core.h"
#include "rzk_dev.h"

namespace rzk {

// Order LDS traffic of the lanes of one wavefront (write phase -> read phase).  A wavefront issues
// its LDS instructions in program order, so no s_barrier is needed; the fences only stop the
// compiler from moving LDS accesses across the phase boundary.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- streaming accesses -------------------------------------------------------------------------------------------
// Coefficient slabs are read once or twice and written once per launch.  Stores use the non-temporal cache policy, so
// that results do not push the resident key, the twiddles and the teams' scratch lines out of L2; loads do not.
// Measured (Open N=1024, A/B of prebuilt libraries): stores nt +1.5 % (response 78.3 -> 76.0 us); loads
// nt -1.5 %.
template <class Tp>
__device__ __forceinline__ Tp ld_stream(const Tp* p) {
  return *p;
}
template <class Tp>
__device__ __forceinline__ void st_stream(Tp* p, Tp v) {
  __builtin_nontemporal_store(v, p);
}
__device__ __forceinline__ void st_stream(int4* p, int4 v) {
  typedef int v4i __attribute__((ext_vector_type(4)));
  v4i t;
  t.x = v.x, t.y = v.y, t.z = v.z, t.w = v.w;
  __builtin_nontemporal_store(t, reinterpret_cast<v4i*>(p));
}
__device__ __forceinline__ void st_stream(int2* p, int2 v) {
  typedef int v2i __attribute__((ext_vector_type(2)));
  v2i t;
  t.x = v.x, t.y = v.y;
  __builtin_nontemporal_store(t, reinterpret_cast<v2i*>(p));
}

// ---- wave reductions ------------------------------------------------------------------------------------
// Butterfly inside the 16-lane rows with DPP operand modifiers (xor 1, xor 2, half-row mirror, row mirror), then the
// two row broadcasts of GFX9 (row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3): six VALU instructions
// with the lane exchange folded into the arithmetic, the total in lane 63, handed out as a wave-uniform scalar by
// v_readlane.  No LDS traffic (the ds_bpermute form of __shfl_xor costs an LDS round trip per step, which a
// wave that runs alone on its SIMD cannot hide).
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t v) {   // lanes without a source read 0 (the identity of +, max)
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, false);
}
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ float dpp_f32(float v) {
  return __builtin_bit_cast(float, dpp_u32<CTRL, ROW_MASK>(__builtin_bit_cast(uint32_t, v)));
}
constexpr int kDppXor1 = 0xB1, kDppXor2 = 0x4E, kDppHalfMirror = 0x141, kDppMirror = 0x140, kDppBcast15 = 0x142,
              kDppBcast31 = 0x143;
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {   // caller guarantees the total fits 32 bits
  v += dpp_u32<kDppXor1>(v);
  v += dpp_u32<kDppXor2>(v);
  v += dpp_u32<kDppHalfMirror>(v);
  v += dpp_u32<kDppMirror>(v);
  v += dpp_u32<kDppBcast15, 0xa>(v);
  v += dpp_u32<kDppBcast31, 0xc>(v);
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ float wave_sum_f32(float v) {   // v >= 0 in every lane
  v += dpp_f32<kDppXor1>(v);
  v += dpp_f32<kDppXor2>(v);
  v += dpp_f32<kDppHalfMirror>(v);
  v += dpp_f32<kDppMirror>(v);
  v += dpp_f32<kDppBcast15, 0xa>(v);
  v += dpp_f32<kDppBcast31, 0xc>(v);
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
  uint32_t o;
  o = dpp_u32<kDppXor1>(v), v = o > v ? o : v;
  o = dpp_u32<kDppXor2>(v), v = o > v ? o : v;
  o = dpp_u32<kDppHalfMirror>(v), v = o > v ? o : v;
  o = dpp_u32<kDppMirror>(v), v = o > v ? o : v;
  o = dpp_u32<kDppBcast15, 0xa>(v), v = o > v ? o : v;
  o = dpp_u32<kDppBcast31, 0xc>(v), v = o > v ? o : v;
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
// exact 64-bit total of per-lane values below 2^56: three 24-bit digits, each summed in 32 bits (64 * 2^24 = 2^30)
__device__ __forceinline__ uint64_t wave_sum_u56(uint64_t v) {
  const uint32_t d0 = wave_sum_u32((uint32_t)v & 0xffffffu);
  const uint32_t d1 = wave_sum_u32((uint32_t)(v >> 24) & 0xffffffu);
  const uint32_t d2 = wave_sum_u32((uint32_t)(v >> 48));
  return (uint64_t)d0 + ((uint64_t)d1 << 24) + ((uint64_t)d2 << 48);
}
// any 64-bit per-lane values (the exact norm kernels): four 16-bit digits
__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
  uint64_t tot = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) tot += (uint64_t)wave_sum_u32((uint32_t)(v >> (16 * i)) & 0xffffu) << (16 * i);
  return tot;
}

// ---- norms ------------------------------------------------------------------------------------------------------
// How many auxiliary primes an exact product needs follows from |a (*) b|_inf <= |a|_2 |b|_2 (Cauchy-Schwarz), so the
// only thing measured per operand is S = sum c^2 — in FLOAT while the coefficients are loaded (v_cvt_f32_i32 +
// v_fma_f32 per coefficient, both full-rate), reduced with wave_sum_f32.  Rounding: the conversion is correct to
// 2^-24, the square to 2^-23, every accumulation step to 2^-24 of the running sum, at most 32 + 6 steps: the float
// total is within a factor (1 +- 2^-18) of S.  kNormSlack = 2^-17 covers that with room.
//   * prime count: S_up = S_float * (1 + kNormSlack) >= S; the bound only has to be safe, never tight.
//   * norm predicate (Params::check_*_constraint, sum c^2 < L with L <= 2^48): decided by the float total whenever
//     it is outside [L (1 - slack), L (1 + slack)], and by exact integer arithmetic (lane_sum_sq_exact) inside, so the
//     verdict is exact for every input: the boundary cases of the tests (flip exactly at (bound+1)^2) take that path.
constexpr float kNormSlack = 0x1p-17f;
template <int E>
__device__ __forceinline__ float lane_sum_sq_f32(const int32_t* v) {   // this lane's share of sum v^2
  float ss = 0.f;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const float f = (float)v[e];
    ss = __builtin_fmaf(f, f, ss);
  }
  return ss;
}
// this lane's share of the exact sum of min(|v|, 2^24)^2, saturated at 2^48: the team total equals sum v^2 whenever
// that is below 2^48
template <int E>
__device__ __forceinline__ uint64_t lane_sum_sq_exact(const int32_t* v) {
  uint64_t sq = 0;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const uint32_t u = (uint32_t)v[e];
    uint32_t a = v[e] < 0 ? 0u - u : u;   // magnitude in unsigned arithmetic (INT32_MIN included)
    a = a < (1u << 24) ? a : (1u << 24);
    sq += (uint64_t)a * a;
  }
  return sq < (1ull << 48) ? sq : (1ull << 48);
}
// Wave-uniform floats are kept in scalar registers: the bounds below live through whole prime passes, where every
// vector register counts (gfx9 has no scalar float ALU, so the arithmetic itself runs on the VALU; v_readfirstlane
// brings the result back).
__device__ __forceinline__ float uniform_f32(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, x)));
}

// ---- teams ------------------------------------------------------------------------------------------------------
// Who transforms one polynomial together (Geo<LOGN, LL>, rzk_core.h) and how its threads meet:
//   WaveTeam  one wavefront: the lanes run in lockstep, a "barrier" only stops the compiler from moving LDS accesses
//             across a phase boundary (wave_sync); sums are DPP reductions.
//   PairTeam  two wavefronts that ARE the workgroup (128 threads, N = 2048): s_barrier at the phase boundaries; a
//             sum is two wave reductions exchanged through two LDS words, added in the same order by both waves, so
//             that both take bit-identical decisions (prime counts, exact-path switches) and never part ways
//             before a barrier.
struct WaveTeam {
  static constexpr const char* kName = "WaveTeam";   // as a profiler prints it (launchers, rzk_kernels.hip)
  static constexpr int LL = 6;
  static constexpr int kTeamsPerBlock = 4;   // (1 with unit_kernel compiled for 5 waves per SIMD lost: commit 139 vs 129 us)
  __device__ __forceinline__ static void sync() { wave_sync(); }
  __device__ __forceinline__ static float sum_f32(float v) { return wave_sum_f32(v); }
  __device__ __forceinline__ static uint64_t sum_u56(uint64_t v) { return wave_sum_u56(v); }
  __device__ __forceinline__ static uint32_t max_u32(uint32_t v) { return wave_max_u32(v); }
};
// One wavefront per polynomial over int32_t coefficient slabs (rzk_slab32.h): WaveTeam in everything but the element
// type of the launch's operands.  The type travels with the team, not as a template parameter of its own, so that the
// kernels of the 64-bit slabs keep their template arguments (and with them their symbols and profiler names), and
// without a wrapper around a shared body (measured: inlining the body into a __global__ wrapper loses the kernel
// arguments' restrict information and cost unit_kernel<10, false, true> 14 VGPRs and a wave per SIMD).
struct WaveTeam32 : WaveTeam {
  static constexpr const char* kName = "i32";
};
template <class TM> struct TeamCoef { using type = int64_t; };
template <> struct TeamCoef<WaveTeam32> { using type = int32_t; };
// The same two teams with the phase-2 twiddles of their transforms in an LDS image behind the workgroup's slabs (Tw2Img,
// rzk_core.h; N = 1024, RZK_TW_LDS).  Like the coefficient type, the switch travels with the team: the kernels of the
// global-table path keep their template arguments and symbols, and the launchers report both under the same name.
struct WaveTeamTw : WaveTeam {};
struct WaveTeam32Tw : WaveTeam32 {};
template <> struct TeamCoef<WaveTeam32Tw> { using type = int32_t; };
template <class TM> struct TeamTwLds { static constexpr bool value = false; };
template <> struct TeamTwLds<WaveTeamTw> { static constexpr bool value = true; };
template <> struct TeamTwLds<WaveTeam32Tw> { static constexpr bool value = true; };
// ... and with ALL vector twiddles in LDS, phase 3 included (TwAllImg, rzk_core.h; RZK_TW_LDS=2).  The 24 KiB of images do not
// fit beside a four-team workgroup's slabs four times per CU; they fit once: sixteen teams per workgroup, one workgroup per
// CU, the same 4 waves per SIMD and the same 157 696 B of LDS per CU as four workgroups of WaveTeamTw.  The teams are as
// independent as ever (no rank table, no barrier after the fill).
struct WaveTeamTw3 : WaveTeam {
  static constexpr int kTeamsPerBlock = 16;
};
struct WaveTeam32Tw3 : WaveTeam32 {
  static constexpr int kTeamsPerBlock = 16;
};
template <> struct TeamCoef<WaveTeam32Tw3> { using type = int32_t; };
template <> struct TeamTwLds<WaveTeamTw3> { static constexpr bool value = true; };
template <> struct TeamTwLds<WaveTeam32Tw3> { static constexpr bool value = true; };
#ifndef RZK_TW3_IMAGE
#define RZK_TW3_IMAGE 1   // 0 (tuning build): the sixteen-team workgroups fill the full image, but phase 3 reads the global tables as
#endif                    // under RZK_TW_LDS=1: the workgroup shape alone, without the phase-3 image
#ifndef RZK_FWD3_EARLY
#define RZK_FWD3_EARLY 1  // under RZK_TW_LDS=1 the forward transform requests its phase-3 twiddles where phase 2 begins (0: tuning build, where
#endif                    // phase 3 begins, seven instructions before the block ends)
template <class TM> struct TeamTw3Lds { static constexpr bool value = false; };
template <> struct TeamTw3Lds<WaveTeamTw3> { static constexpr bool value = RZK_TW3_IMAGE != 0; };
template <> struct TeamTw3Lds<WaveTeam32Tw3> { static constexpr bool value = RZK_TW3_IMAGE != 0; };
// the image a team's workgroup keeps behind its slabs (meaningful where TeamTwLds<TM>::value)
template <int LOGN, class TM> struct TeamTwImg { using type = Tw2Img<LOGN, TM::LL>; };
template <int LOGN> struct TeamTwImg<LOGN, WaveTeamTw3> { using type = TwAllImg<LOGN, 6>; };
template <int LOGN> struct TeamTwImg<LOGN, WaveTeam32Tw3> { using type = TwAllImg<LOGN, 6>; };
struct PairTeam {
  static constexpr const char* kName = "PairTeam";   // as a profiler prints it (launchers, rzk_kernels.hip)
  static constexpr int LL = 7;
  static constexpr int kTeamsPerBlock = 1;
  __device__ __forceinline__ static void sync() { __syncthreads(); }
  __device__ __forceinline__ static float sum_f32(float v) {
    __shared__ float xf[2];
    const float w = wave_sum_f32(v);
    if ((threadIdx.x & 63) == 0) xf[(threadIdx.x >> 6) & 1] = w;
    __syncthreads();
    const float tot = xf[0] + xf[1];
    __syncthreads();   // the words are free again
    return uniform_f32(tot);
  }
  __device__ __forceinline__ static uint32_t max_u32(uint32_t v) {
    __shared__ uint32_t xm[2];
    const uint32_t w = wave_max_u32(v);
    if ((threadIdx.x & 63) == 0) xm[(threadIdx.x >> 6) & 1] = w;
    __syncthreads();
    const uint32_t tot = xm[0] > xm[1] ? xm[0] : xm[1];
    __syncthreads();
    return tot;
  }
  __device__ __forceinline__ static uint64_t sum_u56(uint64_t v) {
    __shared__ uint64_t xq[2];
    const uint64_t w = wave_sum_u56(v);
    if ((threadIdx.x & 63) == 0) xq[(threadIdx.x >> 6) & 1] = w;
    __syncthreads();
    const uint64_t tot = xq[0] + xq[1];
    __syncthreads();
    return tot;
  }
};

// BlockPairTeam: two-wavefront teams INSIDE a larger workgroup (row_block_kernel at N = 2048: eight pairs around the
// staged operand transforms).  s_barrier would stop all sixteen waves, so a pair meets through an LDS word of its own:
// the first lane of each wave adds 1 and learns from the returned value which meeting this is — an even old value
// means "I am first": wait until the word has passed old + 2; odd means the partner is already there.  The word only
// grows, so no per-wave generation state is needed; the LDS unit executes one wavefront's instructions in order, so the
// arrive is behind that wave's slab writes and the poll in front of its slab reads (release / acquire at workgroup
// scope keep the compiler honest about it).  The words are cleared once per workgroup (init).
struct BlockPairTeam {
  static constexpr const char* kName = "BlockPairTeam";   // as a profiler prints it (launchers, rzk_kernels.hip)
  static constexpr int LL = 7;
  static constexpr int kMaxPairs = 8;
  __device__ __forceinline__ static uint32_t* words() {
    __shared__ uint32_t w[kMaxPairs * 4];   // per pair: meeting counter, pad, two exchange words
    return w + ((threadIdx.x >> 7) & (kMaxPairs - 1)) * 4;
  }
  __device__ __forceinline__ static void init() {
    if ((threadIdx.x & 127) == 0) words()[0] = 0;
    __syncthreads();
  }
  __device__ __forceinline__ static void sync() {
    uint32_t* c = words();
    uint32_t old = 0;
    if ((threadIdx.x & 63) == 0) old = __hip_atomic_fetch_add(c, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    old = (uint32_t)__builtin_amdgcn_readfirstlane((int)old);
    const uint32_t target = (old | 1u) + 1u;
    while ((int32_t)(__hip_atomic_load(c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) - target) < 0) __builtin_amdgcn_s_sleep(1);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }
  __device__ __forceinline__ static float sum_f32(float v) {
    float* xf = reinterpret_cast<float*>(words() + 2);
    const float w = wave_sum_f32(v);
    if ((threadIdx.x & 63) == 0) xf[(threadIdx.x >> 6) & 1] = w;
    sync();
    const float tot = xf[0] + xf[1];
    sync();   // the words are free again
    return uniform_f32(tot);
  }
  __device__ __forceinline__ static uint32_t max_u32(uint32_t v) {
    uint32_t* xw = words() + 2;
    const uint32_t w = wave_max_u32(v);
    if ((threadIdx.x & 63) == 0) xw[(threadIdx.x >> 6) & 1] = w;
    sync();
    const uint32_t tot = xw[0] > xw[1] ? xw[0] : xw[1];
    sync();
    return tot;
  }
  __device__ __forceinline__ static uint64_t sum_u56(uint64_t v) {   // (rare path: two 28-bit halves through the two words)
    const uint64_t w = wave_sum_u56(v);
    uint32_t* xw = words() + 2;
    uint64_t tot = 0;
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {
      if ((threadIdx.x & 63) == 0) xw[(threadIdx.x >> 6) & 1] = (uint32_t)(w >> (28 * h)) & 0xfffffffu;
      sync();
      tot += ((uint64_t)xw[0] + xw[1]) << (28 * h);
      sync();
    }
    return tot;
  }
};

// tw2: the table phase 2 reads.  Left out, it is the global table tw; with IMG it is the prime's LDS image (Tw2Img).
// IMG3: that image is a TwAllImg, and phase 3 reads its twiddles from the part behind the phase-2 words.
template <int LOGN, class TM = WaveTeam, bool IMG = false, bool IMG3 = false>
__device__ __forceinline__ void wave_fwd(uint32_t* x, int lane, uint32_t* lds, const uint32_t* __restrict__ tw,
                                         const PrimeConsts& pc, const uint32_t* __restrict__ tw2 = nullptr) {
  constexpr int LL = TM::LL;
  fwd_phase1<LOGN, LL>(x, tw, pc);
  lds_put_p1<LOGN, LL>(x, lane, lds);
  TM::sync();
  lds_get_p2<LOGN, LL>(x, lane, lds);
  TM::sync();
  constexpr bool EARLY3 = RZK_FWD3_EARLY && IMG && !IMG3;   // phase 2 from LDS, phase 3 from the global table: ask for it now
  uint32_t w3[16];
  if constexpr (EARLY3) fwd_phase3_request<LOGN, LL>(w3, lane, tw);
  fwd_phase2<LOGN, LL, IMG>(x, lane, IMG ? tw2 : tw, pc);
  lds_put_p2<LOGN, LL>(x, lane, lds);
  TM::sync();
  lds_get_p3<LOGN, LL>(x, lane, lds);
  TM::sync();
  if constexpr (EARLY3) fwd_phase3_regs<LOGN, LL>(x, w3, pc);
  else fwd_phase3<LOGN, LL, IMG3>(x, lane, IMG3 ? tw2 + TwAllImg<LOGN, LL>::P3 : tw, pc);
}

template <int LOGN, class TM = WaveTeam, bool IMG = false, bool IMG3 = false>
__device__ __forceinline__ void wave_inv(uint32_t* x, int lane, uint32_t* lds, const uint32_t* __restrict__ tw,
                                         const PrimeConsts& pc, const uint32_t* __restrict__ tw2 = nullptr) {
  constexpr int LL = TM::LL;
  static_assert(!IMG3 || IMG, "the phase-3 image lies behind the phase-2 image");
  inv_phase3<LOGN, LL, IMG3>(x, lane, IMG3 ? tw2 + TwAllImg<LOGN, LL>::P3 : tw, pc);
  lds_put_p3<LOGN, LL>(x, lane, lds);
  TM::sync();
  lds_get_p2<LOGN, LL>(x, lane, lds);
  TM::sync();
  inv_phase2<LOGN, LL, IMG>(x, lane, IMG ? tw2 : tw, pc);
  lds_put_p2<LOGN, LL>(x, lane, lds);
  TM::sync();
  lds_get_p1<LOGN, LL>(x, lane, lds);
  TM::sync();
  inv_phase1<LOGN, LL>(x, tw, pc);
}

// sum v^2 < limit ?  (limit <= 2^48; ss = the team's float total of the same registers)
template <int E, class TM = WaveTeam>
__device__ __forceinline__ bool norm_below(const int32_t* v, float ss, uint64_t limit) {
  const double s = (double)ss, lim = (double)limit;
  if (s * (1.0 + 2.0 * (double)kNormSlack) < lim) return true;
  if (s * (1.0 - 2.0 * (double)kNormSlack) >= lim) return false;
  return TM::sum_u56(lane_sum_sq_exact<E>(v)) < limit;
}
// upper bound of |.|_2 from the float total
__device__ __forceinline__ float norm2_upper(float ss) {
  return uniform_f32(__builtin_sqrtf(ss * (1.0f + kNormSlack)) * (1.0f + 0x1p-20f));
}
// bound += a * b on wave-uniform non-negative floats (each step is correct to 2^-24; primes_for adds the margin)
__device__ __forceinline__ float bound_fma(float a, float b, float bound) { return uniform_f32(__builtin_fmaf(a, b, bound)); }

// Verdict of a failed norm predicate.  One-bit flags (two_bit == false): the byte is cleared with a plain store
// (idempotent, any number of rows may do it).  Two-bit flags: bit 0 or bit 1 is cleared with an agent-scope
// atomic AND on the aligned word that holds the byte, because rows of one proof on different XCDs may clear
// different bits (the host only enables this when the flag array is word aligned and a multiple of 4 long).
__device__ __forceinline__ void fail_check(uint8_t* flag, bool two_bit, bool second) {
  if (!two_bit) {
    *flag = 0;
    return;
  }
  const uintptr_t a = reinterpret_cast<uintptr_t>(flag);
  const uint32_t bit = (second ? 2u : 1u) << (8u * (uint32_t)(a & 3u));
  __hip_atomic_fetch_and(reinterpret_cast<uint32_t*>(a & ~(uintptr_t)3), ~bit, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace rzk
