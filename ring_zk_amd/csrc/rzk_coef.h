// rzk_coef.h — the coefficient type of a slab, as the host layer carries it.  A slab of the C ABI holds
// int64_t coefficients or, in the "slab32" format (rzk_slab32.h), int32_t ones.  The host code is written once per entry
// point over that type C: sizeof(C) is the only source of a slab's width, and an operand list has one type, so a launch
// cannot be told a width its operands do not have.  The launchers that take a slab take it typed (rzk_dev.h, DESIGN.md
// §23); what still carries addresses as int64_t* are the kernels' argument structs — Operands::base (filled by `lower`,
// rzk_ctx.h), FsMsg::ptr, PackedSlabs::ptr — and the zs / ys arrays of the reject launch.  launch_addr is the one place where
// a typed pointer becomes such an address; the launcher that reads the struct is named its type (launch_fs_leaves<C>) or,
// below run_program_lowered, a width.
// Plain C++ (tests/test_slab32_host.py compiles it with g++).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

namespace rzk {

template <class C>
inline constexpr bool is_coef = std::is_same_v<C, int64_t> || std::is_same_v<C, int32_t>;

// bytes of `count` polynomials of degree N
template <class C>
constexpr size_t poly_bytes(uint32_t N, size_t count) {
  static_assert(is_coef<C>, "a slab holds int64_t or int32_t coefficients");
  return count * (size_t)N * sizeof(C);
}

template <class C>
struct __attribute__((visibility("hidden"))) Op {   // one operand of a row-program launch (hidden: the library exports no container of it)
  static_assert(is_coef<C>, "a slab holds int64_t or int32_t coefficients");
  const C* base;
  uint32_t stride;
  uint32_t outer;   // 0: indexed by the task batch index; otherwise by the proof index b / group
};

// the address of a slab as the kernels' argument structs carry it
template <class C>
inline const int64_t* launch_addr(const C* p) {
  static_assert(is_coef<C>, "a slab holds int64_t or int32_t coefficients");
  return reinterpret_cast<const int64_t*>(p);
}
template <class C>
inline int64_t* launch_addr(C* p) {
  return const_cast<int64_t*>(launch_addr(static_cast<const C*>(p)));
}

}  // namespace rzk
