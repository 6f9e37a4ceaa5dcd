// rzk_sample.h - device-side samplers: uniform, Gaussian, challenge.
// Part of the one translation unit rzk_kernels.hip (device code only; no include guards beyond #pragma once).
#pragma once
#include "rzk_gauss.h"
#include "rzk_rng.h"
#include "rzk_wave.h"

namespace rzk {

// =============================================================================================
// Device-side samplers: the distributions of the reference's host RNG helpers, drawn with a
// counter-based generator (rzk_rng.h).  One thread draws 4 coefficients from one Philox block (two blocks for
// the wide uniform range), so a polynomial is N/4 independent units and any number of polynomials fills the chip.
//   uniform   random_polynomial_within (src/polynomial.rs:14-25): every coefficient uniform in [-bound, bound]
//   gauss     random_polynomial_in_normal_distribution (polynomial.rs:28-44): (i64) N(0, sigma), i.e. truncated
//             toward zero as I::from_f64 does
//   challenge random_polynomial_from_challenge_set (src/challenge_space.rs:12-33): kappa coefficients +-1 at a
//             uniformly random kappa-subset of the N positions (what shuffling kappa marked slots gives)
// =============================================================================================
// One thread = one Philox block = two coefficients = one 16-byte store at a lane-consecutive address (full lines per wave
// instruction); the polynomial index is a shift (N is a power of two).  pair16: `out` is 16-byte aligned.
__device__ __forceinline__ void store_pair(int64_t* __restrict__ out, uint64_t c0, uint64_t ncoef, int64_t v0, int64_t v1, bool pair16) {
  if (pair16 && c0 + 1 < ncoef) {
    st_stream(reinterpret_cast<int4*>(out + c0), make_int4((int32_t)v0, (int32_t)(v0 >> 32), (int32_t)v1, (int32_t)(v1 >> 32)));
  } else {
    out[c0] = v0;
    if (c0 + 1 < ncoef) out[c0 + 1] = v1;
  }
}

__global__ void __launch_bounds__(256)
sample_uniform_kernel(int64_t* __restrict__ out, uint64_t ncoef, uint32_t log_ring, uint64_t seed, uint32_t stream,
                      uint32_t bound) {
  const uint32_t range = 2u * bound + 1u;   // bound <= (2^32 - 2) / 2
  const bool pair16 = (reinterpret_cast<uintptr_t>(out) & 15u) == 0;
  const uint32_t pair_mask = (1u << (log_ring - 1)) - 1u;
  for (uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x; u * 2 < ncoef; u += (uint64_t)gridDim.x * 256) {
    const uint64_t poly = u >> (log_ring - 1);
    const uint32_t blk = (uint32_t)u & pair_mask;   // block `blk` of a polynomial gives its coefficients 2 blk, 2 blk + 1
    const Philox4 a = sampler_block(seed, stream, poly, blk);
    const int64_t v0 = (int64_t)uniform_below(a.v[0], a.v[1], range) - (int64_t)bound;
    const int64_t v1 = (int64_t)uniform_below(a.v[2], a.v[3], range) - (int64_t)bound;
    store_pair(out, u * 2, ncoef, v0, v1, pair16);
  }
}

// Box-Muller, one pair per Philox block, through the word-to-pair map of rzk_gauss.h (the definition and the error bound
// of a sample are stated there).  F32 (sigma < 2^19: every sigma the parameter sets produce): the radius from a 64-bit
// uniform through exponent + v_log_f32 of the 24-bit mantissa (the tail reaches 9.4 sigma), the angle from a 32-bit
// uniform through sincospif.  The error of a sample before the truncation toward zero is far below 1 except where u0 is
// within 2^-20 or so of 1 (the logarithm cancels: up to 0.47 at sigma = 21780, probability about 1e-5) — statistical
// parity as for the generator itself.  Larger sigma (up to the 2^26 the entry point admits) keeps the double-precision
// form, whose samples need more than 24 bits.
template <bool F32>
__global__ void __launch_bounds__(256)
sample_gauss_kernel(int64_t* __restrict__ out, uint64_t ncoef, uint32_t log_ring, uint64_t seed, uint32_t stream,
                    double sigma) {
  const bool pair16 = (reinterpret_cast<uintptr_t>(out) & 15u) == 0;
  const uint32_t pair_mask = (1u << (log_ring - 1)) - 1u;
  const float sigf = (float)sigma;
  for (uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x; u * 2 < ncoef; u += (uint64_t)gridDim.x * 256) {
    const uint64_t poly = u >> (log_ring - 1);
    const uint32_t blk = (uint32_t)u & pair_mask;
    const Philox4 a = sampler_block(seed, stream, poly, blk);
    int64_t v0, v1;
    if (F32) gauss_pair_f32(a.v[0], a.v[1], a.v[2], sigf, v0, v1);
    else gauss_pair_f64(a.v[0], a.v[1], a.v[2], a.v[3], sigma, v0, v1);
    store_pair(out, u * 2, ncoef, v0, v1, pair16);
  }
}

// Diagnostic (rzk_debug_gauss_map_dev): the same map on words the caller chose, one thread per pair — how the edges of
// the map (u0 next to 1, a full turn) reach the device's intrinsics, which no seed or key produces in a test-sized draw.
template <bool F32>
__global__ void __launch_bounds__(256)
debug_gauss_map_kernel(const uint32_t* __restrict__ words, int64_t* __restrict__ out, uint64_t pairs, double sigma) {
  const float sigf = (float)sigma;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < pairs; i += (uint64_t)gridDim.x * 256) {
    const uint32_t* w = words + 4 * i;
    int64_t v0, v1;
    if (F32) gauss_pair_f32(w[0], w[1], w[2], sigf, v0, v1);
    else gauss_pair_f64(w[0], w[1], w[2], w[3], sigma, v0, v1);
    out[2 * i] = v0;
    out[2 * i + 1] = v1;
  }
}

// one wavefront per polynomial: Floyd's algorithm for a uniform kappa-subset.  Lane t draws step t's candidate (its own
// Philox block half) in parallel; only the collision rule "candidate already marked -> take j" is sequential, walked
// with readlane over an LDS byte map (same picks, same output as a one-lane loop).  All lanes then write the N
// coefficients, two per 16-byte store.
__global__ void __launch_bounds__(256)
sample_challenge_kernel(int64_t* __restrict__ out, uint64_t npoly, uint32_t n_ring, uint64_t seed, uint32_t stream,
                        uint32_t kappa) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int lane = threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int8_t* mark = reinterpret_cast<int8_t*>(smem) + (size_t)wave * n_ring;
  uint32_t* mark_w = reinterpret_cast<uint32_t*>(mark);   // n_ring is a multiple of 4
  const uint32_t kap = kappa < n_ring ? kappa : n_ring;
  const bool pair16 = (reinterpret_cast<uintptr_t>(out) & 15u) == 0;
  for (uint64_t poly = (uint64_t)blockIdx.x * 4 + wave; poly < npoly; poly += (uint64_t)gridDim.x * 4) {
    for (uint32_t i = lane; i < n_ring / 4; i += 64) mark_w[i] = 0;
    wave_sync();
    for (uint32_t t0 = 0; t0 < kap; t0 += 64) {
      const uint32_t t = t0 + lane;
      const Philox4 r = sampler_block(seed, stream, poly, t >> 1);
      const uint32_t w0 = (t & 1) ? r.v[2] : r.v[0], w1 = (t & 1) ? r.v[3] : r.v[1];
      const uint32_t j = n_ring - kap + t;                               // (lanes beyond kap: unused)
      const uint32_t pick = uniform_below(w0, w1 & ~1u, j + 1);
      const int32_t sign = (w1 & 1u) ? 1 : -1;                           // random_bool(0.5): +1 / -1
      const uint32_t m = kap - t0 < 64u ? kap - t0 : 64u;
#pragma unroll 1
      for (uint32_t e = 0; e < m; ++e) {
        const uint32_t pk = (uint32_t)__builtin_amdgcn_readlane((int)pick, (int)e);
        const uint32_t jj = (uint32_t)__builtin_amdgcn_readlane((int)j, (int)e);
        const int32_t sg = __builtin_amdgcn_readlane(sign, (int)e);
        const uint32_t pos = mark[pk] ? jj : pk;
        wave_sync();
        if (lane == 0) mark[pos] = (int8_t)sg;
        wave_sync();
      }
    }
    int64_t* dst = out + poly * n_ring;
    if (pair16) {
      for (uint32_t i = 2 * lane; i < n_ring; i += 128) {
        const int32_t a0 = mark[i], a1 = mark[i + 1];
        st_stream(reinterpret_cast<int4*>(dst + i), make_int4(a0, a0 >> 31, a1, a1 >> 31));
      }
    } else {
      for (uint32_t i = lane; i < n_ring; i += 64) dst[i] = (int64_t)mark[i];
    }
    wave_sync();
  }
}

}  // namespace rzk
