// rzk_xform.h - transforms and element-wise kernels: key, dkey, ntt, addsub, norm, eq, and the small-ring (N < 512) kernels.
// Part of the one translation unit rzk_kernels.hip (device code only; no include guards beyond #pragma once).
#pragma once
#include "rzk_norm.h"
#include "rzk_rowprog.h"

namespace rzk {

// =============================================================================================
// Key transform: centred key entries -> NTT domain (x N^-1, Montgomery form) for all three primes
// =============================================================================================
template <int LOGN>
__global__ void __launch_bounds__(256)
key_transform_kernel(const int64_t* __restrict__ key, uint32_t entries, uint32_t* __restrict__ key_ntt,
                     const DevTables* __restrict__ Tp, const uint32_t* __restrict__ tw_all) {
  using G = Geo<LOGN>;
  constexpr int E = G::E;
  constexpr int N = G::N;
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const DevTables& T = *Tp;
  const int lane = threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint32_t* lds = smem + wave * G::LDS_WORDS;
  const uint32_t ntasks = entries * kKeyImages;
  for (uint32_t task = blockIdx.x * 4 + wave; task < ntasks; task += gridDim.x * 4) {
    const uint32_t entry = task / kKeyImages;
    const int pi = task % kKeyImages;
    const PrimeConsts pc = T.pc[pi];
    const int64_t* __restrict__ src = key + (uint64_t)entry * N;
    uint32_t x[E];
#pragma unroll
    for (int e = 0; e < E; ++e) x[e] = lift((int32_t)src[G::j_p1(lane, e)], pc);
    wave_fwd<LOGN>(x, lane, lds, tw_all + (size_t)(2 * pi) * kTableLen, pc);
    uint4* __restrict__ dst = reinterpret_cast<uint4*>(key_ntt + ((uint64_t)entry * kKeyImages + pi) * N);
#pragma unroll
    for (int g = 0; g < E / 4; ++g) {
      uint4 v;
      v.x = csub(mont_lazy(x[4 * g + 0], pc.ninv_r2, pc.p, pc.npinv), pc.p);
      v.y = csub(mont_lazy(x[4 * g + 1], pc.ninv_r2, pc.p, pc.npinv), pc.p);
      v.z = csub(mont_lazy(x[4 * g + 2], pc.ninv_r2, pc.p, pc.npinv), pc.p);
      v.w = csub(mont_lazy(x[4 * g + 3], pc.ninv_r2, pc.p, pc.npinv), pc.p);
      dst[g * 64 + lane] = v;
    }
  }
}

// Per-entry multiplier images (Operands::dkey_img): like key_transform_kernel, for polynomials that arrive with the batch
// (the g_i of the Linear / Sum proofs).  One wavefront per polynomial: canonical test, 2-norm, then the three images.
template <int LOGN>
__global__ void __launch_bounds__(256)
dkey_transform_kernel(const int64_t* __restrict__ g, uint64_t count, uint32_t dkey_n, uint32_t* __restrict__ img,
                      double* __restrict__ l2, const DevTables* __restrict__ Tp, const uint32_t* __restrict__ tw_all,
                      uint8_t* __restrict__ flags, uint32_t* __restrict__ bad_word, uint32_t two_bit, uint32_t trusted) {
  using G = Geo<LOGN>;
  constexpr int E = G::E;
  constexpr int N = G::N;
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const DevTables& T = *Tp;
  const int lane = threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint32_t* lds = smem + wave * G::LDS_WORDS;
  for (uint64_t poly = (uint64_t)blockIdx.x * 4 + wave; poly < count; poly += (uint64_t)gridDim.x * 4) {
    const int64_t* __restrict__ src = g + poly * N;
    int32_t v[E];
    if (trusted) {
#pragma unroll
      for (int e = 0; e < E; ++e) v[e] = (int32_t)src[G::j_p1(lane, e)];
    } else {
      uint32_t in_bad = 0, in_mx = 0;
#pragma unroll
      for (int e = 0; e < E; ++e) v[e] = canon_lo_mx(src[G::j_p1(lane, e)], T.crt.qhalf, in_bad, in_mx);
      if (canon_fail(in_bad, in_mx, T.crt.qhalf) && lane == 0) {   // as input_fault: the proof's verdict (all bits) and the sticky word
        const uint64_t entry = poly / dkey_n;
        if (flags) {
          if (two_bit) {
            const uintptr_t a = reinterpret_cast<uintptr_t>(flags + entry);
            __hip_atomic_fetch_and(reinterpret_cast<uint32_t*>(a & ~(uintptr_t)3), ~(0xffu << (8u * (uint32_t)(a & 3u))),
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          } else {
            flags[entry] = 0;
          }
        }
        if (bad_word) *bad_word = 1u;
      }
    }
    const float ss = wave_sum_f32(lane_sum_sq_f32<E>(v));
    if (lane == 0) l2[poly] = (double)norm2_upper(ss) * (1.0 + 1e-6);   // upper bound of the 2-norm (read back as float)
#pragma unroll 1
    for (int pi = 0; pi < kKeyImages; ++pi) {
      const PrimeConsts pc = T.pc[pi];
      uint32_t x[E];
#pragma unroll
      for (int e = 0; e < E; ++e) x[e] = lift(v[e], pc);
      wave_fwd<LOGN>(x, lane, lds, tw_all + (size_t)(2 * pi) * kTableLen, pc);
      uint4* __restrict__ dst = reinterpret_cast<uint4*>(img + (poly * kKeyImages + pi) * N);
#pragma unroll
      for (int q4 = 0; q4 < E / 4; ++q4) {
        uint4 o;
        o.x = csub(mont_lazy(x[4 * q4 + 0], pc.ninv_r2, pc.p, pc.npinv), pc.p);
        o.y = csub(mont_lazy(x[4 * q4 + 1], pc.ninv_r2, pc.p, pc.npinv), pc.p);
        o.z = csub(mont_lazy(x[4 * q4 + 2], pc.ninv_r2, pc.p, pc.npinv), pc.p);
        o.w = csub(mont_lazy(x[4 * q4 + 3], pc.ninv_r2, pc.p, pc.npinv), pc.p);
        dst[q4 * 64 + lane] = o;
      }
    }
  }
}

// =============================================================================================
// Stand-alone batched transforms over one auxiliary prime (the "batched NTT" of the headline metric)
// =============================================================================================
template <int LOGN>
__global__ void __launch_bounds__(256)
ntt_fwd_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint64_t count, int pi,
               const DevTables* __restrict__ Tp, const uint32_t* __restrict__ tw_all) {
  using G = Geo<LOGN>;
  constexpr int E = G::E;
  constexpr int N = G::N;
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const DevTables& T = *Tp;
  const int lane = threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint32_t* lds = smem + wave * G::LDS_WORDS;
  const PrimeConsts pc = T.pc[pi];
  const uint32_t* __restrict__ tw = tw_all + (size_t)(2 * pi) * kTableLen;
  for (uint64_t poly = (uint64_t)blockIdx.x * 4 + wave; poly < count; poly += (uint64_t)gridDim.x * 4) {
    const uint32_t* __restrict__ src = in + poly * N;
    uint32_t x[E];
#pragma unroll
    for (int e = 0; e < E; ++e) x[e] = src[G::j_p1(lane, e)];
    wave_fwd<LOGN>(x, lane, lds, tw, pc);
    uint4* __restrict__ dst = reinterpret_cast<uint4*>(out + poly * N);
#pragma unroll
    for (int g = 0; g < E / 4; ++g) {
      uint4 v;
      v.x = csub(csub(x[4 * g + 0], pc.twop), pc.p);
      v.y = csub(csub(x[4 * g + 1], pc.twop), pc.p);
      v.z = csub(csub(x[4 * g + 2], pc.twop), pc.p);
      v.w = csub(csub(x[4 * g + 3], pc.twop), pc.p);
      dst[g * 64 + lane] = v;
    }
  }
}

template <int LOGN>
__global__ void __launch_bounds__(256)
ntt_inv_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint64_t count, int pi,
               const DevTables* __restrict__ Tp, const uint32_t* __restrict__ tw_all) {
  using G = Geo<LOGN>;
  constexpr int E = G::E;
  constexpr int N = G::N;
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const DevTables& T = *Tp;
  const int lane = threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint32_t* lds = smem + wave * G::LDS_WORDS;
  const PrimeConsts pc = T.pc[pi];
  const uint32_t* __restrict__ tw = tw_all + (size_t)(2 * pi + 1) * kTableLen;
  for (uint64_t poly = (uint64_t)blockIdx.x * 4 + wave; poly < count; poly += (uint64_t)gridDim.x * 4) {
    const uint4* __restrict__ src = reinterpret_cast<const uint4*>(in + poly * N);
    uint32_t x[E];
#pragma unroll
    for (int g = 0; g < E / 4; ++g) {
      const uint4 v = src[g * 64 + lane];
      x[4 * g + 0] = v.x;
      x[4 * g + 1] = v.y;
      x[4 * g + 2] = v.z;
      x[4 * g + 3] = v.w;
    }
    wave_inv<LOGN>(x, lane, lds, tw, pc);
    uint32_t* __restrict__ dst = out + poly * N;
#pragma unroll
    for (int e = 0; e < E; ++e)
      dst[G::j_p1(lane, e)] = csub(mont_lazy(x[e], pc.ninv_r, pc.p, pc.npinv), pc.p);
  }
}

// =============================================================================================
// Element-wise kernels: Mat::add / Mat::sub, norm predicate, equality
// =============================================================================================
__global__ void __launch_bounds__(256)
addsub_kernel(const int64_t* a, const int64_t* b, int64_t* out, uint64_t n2, int sub,
              const DevTables* __restrict__ Tp, uint32_t* __restrict__ bad_word) {
  // two coefficients (16 bytes) per thread and step; out may alias a or b (in-place add/sub)
  const DevTables& T = *Tp;
  const longlong2* a2 = reinterpret_cast<const longlong2*>(a);
  const longlong2* b2 = reinterpret_cast<const longlong2*>(b);
  longlong2* o2 = reinterpret_cast<longlong2*>(out);
  const uint64_t h = T.crt.qhalf;
  bool fault = false;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2;
       i += (uint64_t)gridDim.x * blockDim.x) {
    const longlong2 x = a2[i], y = b2[i];
    fault = fault || (uint64_t)x.x + h > 2 * h || (uint64_t)x.y + h > 2 * h || (uint64_t)y.x + h > 2 * h ||
            (uint64_t)y.y + h > 2 * h;   // canonical inputs only (see canon_lo)
    longlong2 r;
    r.x = center_rounds<1>(sub ? x.x - y.x : x.x + y.x, T.crt);
    r.y = center_rounds<1>(sub ? x.y - y.y : x.y + y.y, T.crt);
    o2[i] = r;
  }
  if (fault && bad_word) *bad_word = 1u;
}

// The norm predicate of `rows` polynomials per proof, one wavefront per proof: norm_rows (rzk_norm.h), on int64_t slabs.
// (Its int32_t form is norm_kernel_i32, rzk_slab32_dev.hip.)
template <int LOGN>
__global__ void __launch_bounds__(256)
norm_kernel(const int64_t* __restrict__ v, uint32_t rows, uint64_t limit_hi, uint64_t limit_lo,
            uint8_t* __restrict__ ok, uint64_t B, int and_mode, int shift, uint32_t qhalf,
            uint32_t* __restrict__ bad_word) {
  norm_rows<LOGN, int64_t>(v, rows, limit_hi, limit_lo, ok, B, and_mode, shift, qhalf, bad_word);
}

template <int LOGN>
__global__ void __launch_bounds__(256)
eq_kernel(const int64_t* __restrict__ a, const int64_t* __restrict__ b, uint32_t rows,
          uint8_t* __restrict__ eq, uint64_t B, uint32_t qhalf, uint32_t* __restrict__ bad_word) {
  using G = Geo<LOGN>;
  constexpr int E = G::E;
  constexpr int N = G::N;
  const int lane = threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (uint64_t p = (uint64_t)blockIdx.x * 4 + wave; p < B; p += (uint64_t)gridDim.x * 4) {
    int ne = 0, bad = 0;
    for (uint32_t r = 0; r < rows; ++r) {
      const int64_t* __restrict__ pa = a + (p * rows + r) * N;
      const int64_t* __restrict__ pb = b + (p * rows + r) * N;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int64_t x = pa[G::j_p1(lane, e)], y = pb[G::j_p1(lane, e)];
        ne |= (x != y);
        // equality of canonical forms (derived PartialEq): anything else is not a ZqI64 value
        bad |= ((uint64_t)x + qhalf > 2ull * qhalf) | ((uint64_t)y + qhalf > 2ull * qhalf);
      }
    }
    const int any_ne = __any(ne), any_bad = __any(bad);
    if (lane == 0) {
      eq[p] = (uint8_t)((any_ne || any_bad) ? 0 : 1);
      if (any_bad && bad_word) *bad_word = 1u;
    }
  }
}

// =============================================================================================
// Small ring degrees (N = 4 .. 256): the reference's own unit / integration tests run at N = 4 and
// N = 16 (src/mat.rs:241, tests/test.rs:8).  One wavefront still owns one row task, but a transform
// makes no sense below one coefficient per lane, so products are the O(N^2) negacyclic convolution
// in 32-bit Montgomery arithmetic mod q, operands staged in LDS.  Same row programs, operand tables,
// epilogue and flags as the big-N kernel; this path exists for drop-in completeness, not for speed.
// =============================================================================================
__global__ void __launch_bounds__(256)
row_kernel_small(const Program* __restrict__ prog, const Operands ops, const uint32_t* __restrict__ key_mont,
                 const DevTables* __restrict__ Tp, uint8_t* __restrict__ flags, const uint32_t ntasks,
                 const uint32_t N, const uint32_t r2q) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint32_t* la = smem + wave * 2 * N;   // left operand, plain residues in [0,q)
  uint32_t* lb = la + N;                // right operand, Montgomery form
  const DevTables& T = *Tp;
  const uint32_t q = T.crt.q;
  const uint32_t nrows = prog->nrows;
  constexpr int EMAX = 4;               // N <= 256 -> at most 4 coefficients per lane

  for (uint32_t task = blockIdx.x * 4 + wave; task < ntasks; task += gridDim.x * 4) {
    const uint32_t b = task / nrows;
    const uint32_t rowi = task - b * nrows;
    const uint32_t bo = ops.group > 1 ? b / ops.group : b;
    const Row row = prog->rows[rowi];
    uint64_t pos[EMAX], neg[EMAX];
#pragma unroll
    for (int e = 0; e < EMAX; ++e) pos[e] = neg[e] = 0;
    const uint32_t qhalf = T.crt.qhalf;
    uint32_t in_bad = 0, in_mx = 0;   // canonical-input test of every coefficient this row loads

    for (uint32_t t = 0; t < row.nterms; ++t) {
      const Term tm = prog->terms[row.term0 + t];
      const int64_t* __restrict__ pb = operand_ptr(ops, tm.b_op, tm.b_off, b, bo, (int)N);
      if ((tm.kind & TERM_KIND_MASK) == TERM_KEY) {
        const uint32_t* __restrict__ km = key_mont + (size_t)tm.a_off * N;
        for (uint32_t i = lane; i < N; i += 64) {
          la[i] = zq_from_centered(canon_lo_mx(pb[i], qhalf, in_bad, in_mx), q);
          lb[i] = km[i];
        }
      } else {
        const int64_t* __restrict__ pa = operand_ptr(ops, tm.a_op, tm.a_off, b, bo, (int)N);
        for (uint32_t i = lane; i < N; i += 64) {
          la[i] = zq_from_centered(canon_lo_mx(pa[i], qhalf, in_bad, in_mx), q);
          lb[i] = montq_u(zq_from_centered(canon_lo_mx(pb[i], qhalf, in_bad, in_mx), q), r2q, T.crt);
        }
      }
      wave_sync();
#pragma unroll
      for (int e = 0; e < EMAX; ++e) {
        const uint32_t tt = lane + 64 * e;
        if (tt < N) {
          uint64_t p = 0, m = 0;
          for (uint32_t i = 0; i < N; ++i) {
            const uint32_t prod = montq_u(la[i], lb[(tt - i) & (N - 1)], T.crt);
            if (i > tt) m += prod; else p += prod;   // X^N = -1
          }
          if (tm.sign >= 0) { pos[e] += p; neg[e] += m; } else { pos[e] += m; neg[e] += p; }
        }
      }
      wave_sync();
    }

    int nz = 0;
#pragma unroll
    for (int e = 0; e < EMAX; ++e) {
      const uint32_t tt = lane + 64 * e;
      if (tt < N) {
        uint32_t u = subq((uint32_t)(pos[e] % q), (uint32_t)(neg[e] % q), q);
        for (uint32_t a = 0; a < row.nadds; ++a) {
          const AddTerm ad = prog->adds[row.add0 + a];
          const uint32_t v = zq_from_centered(
              canon_lo_mx(operand_ptr(ops, ad.op & ADD_OP_MASK, ad.off, b, bo, (int)N)[tt], qhalf, in_bad, in_mx), q);
          u = ad.sign >= 0 ? addq(u, v, q) : subq(u, v, q);
        }
        if (row.mode == MODE_STORE)
          const_cast<int64_t*>(operand_ptr(ops, row.out_op, row.out_off, b, bo, (int)N))[tt] = center_from_zq(u, T.crt);
        else
          nz |= (u != 0);
      }
    }
    if (row.mode != MODE_STORE) {
      if (__any(nz) && lane == 0) flags[bo] = 0;
    }
    if (canon_fail(in_bad, in_mx, qhalf)) input_fault(ops, flags, bo, (int)lane);
  }
}

// key entries -> Montgomery-form residues mod q (one thread per coefficient)
__global__ void __launch_bounds__(256)
key_mont_kernel(const int64_t* __restrict__ key, uint32_t* __restrict__ key_mont, uint64_t ncoef,
                const DevTables* __restrict__ Tp, uint32_t r2q) {
  const DevTables& T = *Tp;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < ncoef; i += (uint64_t)gridDim.x * blockDim.x)
    key_mont[i] = montq_u(zq_from_centered((int32_t)key[i], T.crt.q), r2q, T.crt);
}

// norm / equality for any N (used below N = 512): one wavefront per proof
__global__ void __launch_bounds__(256)
norm_kernel_small(const int64_t* __restrict__ v, uint32_t rows, uint64_t limit_hi, uint64_t limit_lo,
                  uint8_t* __restrict__ ok, uint64_t B, int and_mode, int shift, uint32_t N, uint32_t qhalf,
                  uint32_t* __restrict__ bad_word) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (uint64_t b = (uint64_t)blockIdx.x * 4 + wave; b < B; b += (uint64_t)gridDim.x * 4) {
    int good = 1;
    for (uint32_t r = 0; r < rows; ++r) {
      const int64_t* __restrict__ p = v + (b * rows + r) * N;
      uint64_t slo = 0, shi = 0;
      int huge = 0;
      for (uint32_t i = lane; i < N; i += 64) {
        const int64_t c = p[i];
        const uint64_t a = c < 0 ? 0ull - (uint64_t)c : (uint64_t)c;
        huge |= a > (uint64_t)qhalf;
        const uint64_t al = a & 0xffffffffu;
        const uint64_t ll = al * al;
        slo += ll & 0xffffffffu;
        shi += ll >> 32;
      }
      slo = wave_sum_u64(slo);
      shi = wave_sum_u64(shi);
      const uint64_t mid = shi + (slo >> 32);
      const uint64_t tot_lo = (mid << 32) | (slo & 0xffffffffu);
      const uint64_t tot_hi = mid >> 32;
      const int lt = (tot_hi < limit_hi) || (tot_hi == limit_hi && tot_lo < limit_lo);
      const int any_huge = __any(huge);
      good &= lt && !any_huge;
      if (any_huge && bad_word && lane == 0) *bad_word = 1u;
    }
    if (lane == 0) {
      if (and_mode == 0)
        ok[b] = (uint8_t)good;
      else if (and_mode == 1)
        ok[b] = (uint8_t)(ok[b] & good);
      else
        ok[b] = (uint8_t)(ok[b] | (good << shift));
    }
  }
}

__global__ void __launch_bounds__(256)
eq_kernel_small(const int64_t* __restrict__ a, const int64_t* __restrict__ b, uint32_t rows,
                uint8_t* __restrict__ eq, uint64_t B, uint32_t N, uint32_t qhalf, uint32_t* __restrict__ bad_word) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (uint64_t p = (uint64_t)blockIdx.x * 4 + wave; p < B; p += (uint64_t)gridDim.x * 4) {
    int ne = 0, bad = 0;
    const uint64_t n = (uint64_t)rows * N;
    for (uint64_t i = lane; i < n; i += 64) {
      const int64_t x = a[p * n + i], y = b[p * n + i];
      ne |= (x != y);
      bad |= ((uint64_t)x + qhalf > 2ull * qhalf) | ((uint64_t)y + qhalf > 2ull * qhalf);
    }
    const int any_ne = __any(ne), any_bad = __any(bad);
    if (lane == 0) {
      eq[p] = (uint8_t)((any_ne || any_bad) ? 0 : 1);
      if (any_bad && bad_word) *bad_word = 1u;
    }
  }
}

}  // namespace rzk
