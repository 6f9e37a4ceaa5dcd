// rzk_slab32.h — the 32-bit coefficient slab format "slab32" (include/rzk.h "32-bit slabs"), shared by
// the kernels (rzk_rowprog.h: the canonical test of a 32-bit load; rzk_slab32_dev.hip: narrow / widen), the host code
// (rzk_run.cpp / rzk_slab32.cpp: which kernels a 32-bit call runs) and the CPU test (tests/test_slab32_host.py, g++).
// Plain C++.
//
// A slab32 is the dense row-major [batch][row][N] layout of every coefficient slab of the C ABI with int32_t centred
// residues in place of int64_t: the same values, narrower.  For every modulus rzk_ctx_create accepts,
// q <= 4294606851, so h = (q - 1) / 2 <= 2147303425 < 2^31 and a centred residue fits.
//   canonical    |c| <= h, as for the 64-bit slabs.  The int32 range is wider than that (2^31 > h + 1), so the test stays;
//                what it loses is the high-word half: with u = (uint32)c + h (mod 2^32), c is canonical <=> u <= 2 h.
//                (c < -h wraps to u >= 2^31 + h > 2 h; c > h gives 2 h < u < 2^31 + h < 2^32: no second wrap.)
//   narrow       int64 -> int32: the low word.  Exact for a canonical coefficient; a non-canonical one is an input fault
//                of the call (its output value is unspecified: the low word is what is stored).
//   widen        int32 -> int64: sign extension.  No test: the consuming call tests.
//   alignment    device slabs are 16-byte aligned, as elsewhere.
//   width        all operands of one launch have the same width; a call's workspace intermediates follow the call's.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RZK_S32_HD __host__ __device__ inline
#else
#define RZK_S32_HD inline
#endif

namespace rzk {

// (q - 1) / 2 of an odd modulus below 2^32
RZK_S32_HD uint32_t slab32_half(uint64_t q) { return (uint32_t)((q - 1) / 2); }

// the canonical test of a 64-bit coefficient (rzk_rowprog.h, canon_lo): (uint64)(c + h) <= 2 h
RZK_S32_HD bool slab64_canonical(int64_t c, uint32_t half) { return (uint64_t)c + half <= 2ull * half; }
// ... and of a 32-bit one: one unsigned compare on the 32-bit value.  slab32_test_word is what the kernels max over a
// polynomial's coefficients before the compare.
RZK_S32_HD uint32_t slab32_test_word(int32_t c, uint32_t half) { return (uint32_t)c + half; }
RZK_S32_HD bool slab32_canonical(int32_t c, uint32_t half) { return slab32_test_word(c, half) <= 2u * half; }
// |c| as the 32-bit norm kernel squares it (norm_rows<., int32_t>, rzk_norm.h, behind norm_kernel_i32): below 2^31 for every canonical c; INT32_MIN
// gives 2^31, and is not canonical for any modulus
RZK_S32_HD uint32_t slab32_abs(int32_t c) { return c < 0 ? 0u - (uint32_t)c : (uint32_t)c; }

// narrow: the low word; *fault is set (never cleared) when c is not canonical
RZK_S32_HD int32_t slab32_narrow(int64_t c, uint32_t half, bool* fault) {
  if (!slab64_canonical(c, half)) *fault = true;
  return (int32_t)(uint32_t)(uint64_t)c;
}
RZK_S32_HD int64_t slab32_widen(int32_t c) { return (int64_t)c; }

// ---- routing ------------------------------------------------------------------------------------------------------
// Which kernels a 32-bit launch runs.  Native 32-bit instantiations (rzk_slab32_dev.hip) exist for one-wavefront teams
// at N = 512 and N = 1024 of
//   unit_kernel / unit_io_kernel   key-product programs (no vector x vector items), with or without rotation terms
//   shift_row_kernel               the packed-byte form (RZK_SHIFT_BYTES, the default)
//   row_kernel                     programs with vector x vector items and no rotation terms (Linear: gx, u, the verifier's
//                                  last program)
// Everything else — small rings, N = 2048 (two-wavefront teams), row groups / blocks / slots (n >= 2, the split
// relation), row_kernel with rotation terms, the word-only rotation kernel, programs that multiply by prepared images —
// takes the convert path: the call widens its inputs into the context's arena, runs the 64-bit launches and narrows the
// outputs.
// The native instantiations are those of a context with its default rotation knobs at n = 1: a context with RZK_SHIFT=0
// or RZK_SHIFT_BYTES=0, or with n >= 2, converts every 32-bit call (one rule per context, not one per program).
enum Slab32Path : int { S32_UNITS = 0, S32_SHIFT = 1, S32_OTHER = 2 };   // what path_of (rzk_plan.h) names: Units, Shift, anything else
struct Slab32Facts {
  int path;          // Slab32Path of the planned program
  bool has_vec;      // vector x vector items (PlanFacts::has_vec)
  bool has_images;   // multiplier / operand images (PlanFacts::has_dkey / has_dd)
  uint32_t n;        // rows of a1 (the context's n)
  bool rot;          // challenge products run as rotations (shift_ok, rzk_run.cpp)
  bool shift_bytes;  // ... of short operands as packed bytes (RZK_SHIFT_BYTES)
  bool rows;         // path == S32_OTHER and it is row_kernel (none of blocks / groups / slots)
  bool has_shift;    // rotation terms inside the rows (PlanFacts::has_shift)
};
// plan facts (PlanFacts, rzk_plan.h) and what path_of made of them -> Slab32Facts.  Of the paths that are neither Units nor
// Shift, row_kernel is the one path_of names when the plan has no blocks, groups or slots (the order of its tests); small
// rings never get that far (slab32_native).
template <class PlanFactsT>
inline Slab32Facts slab32_facts(const PlanFactsT& f, bool path_units, bool path_shift, uint32_t n, bool rot, bool shift_bytes) {
  const bool other = !path_units && !path_shift;
  return Slab32Facts{path_units ? S32_UNITS : (path_shift ? S32_SHIFT : S32_OTHER), f.has_vec, f.has_dkey || f.has_dd, n, rot,
                     shift_bytes, other && !f.nblocks && !f.ngroups && !f.nslots, f.has_shift};
}
// small: N < 512 (schoolbook kernels); team_ll: log2 of the threads that share a polynomial (6: one wavefront)
RZK_S32_HD bool slab32_native(const Slab32Facts& f, uint32_t logn, bool small, int team_ll) {
  if (small || team_ll != 6 || (logn != 9 && logn != 10)) return false;
  if (f.n != 1 || !f.rot || !f.shift_bytes) return false;
  if (f.has_images) return false;
  if (f.path == S32_SHIFT) return true;   // (its products are per-proof polynomials by definition: has_vec says nothing)
  if (f.rows) return !f.has_shift;        // row_kernel<., false, i32, false>: vector x vector items allowed
  return f.path == S32_UNITS && !f.has_vec;
}

}  // namespace rzk
