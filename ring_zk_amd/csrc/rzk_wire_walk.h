// rzk_wire_walk.h — schema of the reference's serialized protocol messages and the bounds-checked walk over one
// message, shared by the GPU codec (rzk_wire_dev.hip) and the CPU walker test (tests/test_wire_walk.py, g++).
//
// bincode with the reference's default options (src/mat.rs:424-438): little-endian, a u64 count before every Vec,
// struct fields in declaration order without tags, a 1-byte tag (0 = None, 1 = Some) before an Option value.  A
// Polynomial is its trimmed coefficient Vec (u64 len ; len x coefficient, len <= N), a Mat<I, N> is
// Vec<Vec<Polynomial>> (u64 rows ; rows x { u64 cols ; cols x polynomial }) and every Mat of a message is a
// column (cols = 1).  A message is described as up to kWireMaxFields fields, each one of
//     POLY        Polynomial                                  1 polynomial
//     OPT         Option<Polynomial>                          1 polynomial (None: no coefficients)
//     VEC(R)      Vec<Polynomial> of R                        R polynomials
//     MAT(R)      Mat R x 1                                   R polynomials
// optionally wrapped in a Vec of V (Vec<Commitment>, Vec<Mat>, Vec<Vec<Polynomial>>).  Field f owns the
// polynomials first[f] .. first[f+1]-1 of the message, in wire order, which is also the row order of its slab.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RZK_WIRE_HD __host__ __device__ inline
#else
#define RZK_WIRE_HD inline
#endif

namespace rzk {

// message kinds: the values of RZK_MSG_* (include/rzk.h)
enum WireKind : int {
  WIRE_COMMITMENT = 0,         // Commitment { c: Mat }                                       (commit.rs:134)
  WIRE_OPENING = 1,            // Opening { x: Vec<Poly>, r: Mat, f: Option<Poly> }           (commit.rs:222)
  WIRE_CHALLENGE = 2,          // {Open,Linear,Sum}ProofChallenge { d: Poly }
  WIRE_OPEN_COMMITMENT = 3,    // OpenProofCommitment { c: Commitment, t: Vec<Poly> }          (open.rs:190)
  WIRE_OPEN_RESPONSE = 4,      // OpenProofResponse { z: Mat }                                 (open.rs:222)
  WIRE_LINEAR_COMMITMENT = 5,  // LinearProofCommitment { c, cp: Commitment, g: Poly, t, tp: Vec<Poly>, u: Mat }
  WIRE_SUM_COMMITMENT = 6,     // SumProofCommitment { cp, cs: Vec<Commitment>, gs, tp: Vec<Poly>, ts: Vec<Vec<Poly>>, u: Mat }
  WIRE_SUM_RESPONSE = 7,       // SumProofResponse { zp: Mat, zs: Vec<Mat> }
  WIRE_NKINDS = 8,
};

enum WireFieldKind : uint8_t { WF_POLY = 0, WF_OPT = 1, WF_VEC = 2, WF_MAT = 3 };

constexpr int kWireMaxFields = 6;
constexpr uint32_t kWireNone = 0xffffu;   // "len" of an Option that is None (N <= 2048 < kWireNone)

struct WireField {
  uint8_t kind;    // WireFieldKind
  uint8_t outer;   // 1: wrapped in a Vec of V
  uint16_t pad;
  uint32_t rows;   // R of VEC / MAT, 1 for POLY / OPT
};

struct WireSchema {
  uint32_t nfields, N, coef_bytes, V;
  uint32_t polys;                        // polynomials per message
  uint32_t first[kWireMaxFields + 1];    // first polynomial of every field; first[nfields] = polys
  WireField f[kWireMaxFields];
};

// Fills *s for a message kind over a context (N, n, k, l) and V (Sum kinds; ignored elsewhere).  false: bad kind,
// width, or V == 0 on a Sum kind.
RZK_WIRE_HD bool wire_schema(int kind, uint32_t N, uint32_t n, uint32_t k, uint32_t l, uint32_t V, uint32_t coef_bytes,
                             WireSchema* s) {
  if (coef_bytes != 4 && coef_bytes != 8) return false;
  const bool sum = kind == WIRE_SUM_COMMITMENT || kind == WIRE_SUM_RESPONSE;
  if (sum && V == 0) return false;
  s->N = N;
  s->coef_bytes = coef_bytes;
  s->V = sum ? V : 1;
  s->nfields = 0;
  auto add = [&](uint8_t fk, uint8_t outer, uint32_t rows) {
    WireField& F = s->f[s->nfields++];
    F.kind = fk;
    F.outer = outer;
    F.pad = 0;
    F.rows = rows;
  };
  switch (kind) {
    case WIRE_COMMITMENT: add(WF_MAT, 0, n + l); break;
    case WIRE_OPENING: add(WF_VEC, 0, l); add(WF_MAT, 0, k); add(WF_OPT, 0, 1); break;
    case WIRE_CHALLENGE: add(WF_POLY, 0, 1); break;
    case WIRE_OPEN_COMMITMENT: add(WF_MAT, 0, n + l); add(WF_VEC, 0, n); break;
    case WIRE_OPEN_RESPONSE: add(WF_MAT, 0, k); break;
    case WIRE_LINEAR_COMMITMENT:
      add(WF_MAT, 0, n + l); add(WF_MAT, 0, n + l); add(WF_POLY, 0, 1);
      add(WF_VEC, 0, n); add(WF_VEC, 0, n); add(WF_MAT, 0, l);
      break;
    case WIRE_SUM_COMMITMENT:
      add(WF_MAT, 0, n + l); add(WF_MAT, 1, n + l); add(WF_VEC, 0, V);
      add(WF_VEC, 0, n); add(WF_VEC, 1, n); add(WF_MAT, 0, l);
      break;
    case WIRE_SUM_RESPONSE: add(WF_MAT, 0, k); add(WF_MAT, 1, k); break;
    default: return false;
  }
  uint32_t p = 0;
  for (uint32_t f = 0; f < s->nfields; ++f) {
    s->first[f] = p;
    p += (s->f[f].outer ? s->V : 1) * s->f[f].rows;
  }
  s->first[s->nfields] = p;
  s->polys = p;
  return true;
}

// field of polynomial j (j < polys)
RZK_WIRE_HD uint32_t wire_field_of(const WireSchema& s, uint32_t j) {
  uint32_t f = 0;
  while (f + 1 < s.nfields && j >= s.first[f + 1]) ++f;
  return f;
}

// Structural bytes of field f (counts, column prefixes, Option tag), without the polynomials' own len prefixes.
RZK_WIRE_HD uint64_t wire_field_struct(const WireSchema& s, uint32_t f) {
  const WireField& F = s.f[f];
  const uint64_t outer = F.outer ? s.V : 1;
  uint64_t b = F.outer ? 8 : 0;
  if (F.kind == WF_VEC || F.kind == WF_MAT) b += 8 * outer;
  if (F.kind == WF_MAT) b += 8 * outer * F.rows;
  if (F.kind == WF_OPT) b += 1;
  return b;
}

RZK_WIRE_HD uint64_t wire_struct_total(const WireSchema& s) {
  uint64_t b = 0;
  for (uint32_t f = 0; f < s.nfields; ++f) b += wire_field_struct(s, f);
  return b;
}

// Largest encoding of one message: every polynomial (and the Option) present at full length.
RZK_WIRE_HD uint64_t wire_max_bytes(const WireSchema& s) {
  return wire_struct_total(s) + (uint64_t)s.polys * (8 + (uint64_t)s.N * s.coef_bytes);
}

// Structural prefixes that sit immediately in front of polynomial j's len prefix (for an OPT field the tag;
// some = the tag's value), in wire order: put(value, nbytes) with nbytes 8 or 1.  Returns their total size.
template <class Put>
RZK_WIRE_HD uint32_t wire_prefixes(const WireSchema& s, uint32_t j, bool some, Put& put) {
  const uint32_t f = wire_field_of(s, j);
  const WireField& F = s.f[f];
  const uint32_t r = j - s.first[f];
  const uint32_t rr = r % F.rows;   // row inside the (inner) Vec / Mat
  uint32_t nb = 0;
  if (F.outer && r == 0) { put((uint64_t)s.V, 8); nb += 8; }
  if ((F.kind == WF_VEC || F.kind == WF_MAT) && rr == 0) { put((uint64_t)F.rows, 8); nb += 8; }
  if (F.kind == WF_MAT) { put((uint64_t)1, 8); nb += 8; }
  if (F.kind == WF_OPT) { put((uint64_t)(some ? 1 : 0), 1); nb += 1; }
  return nb;
}

// Structural bytes in front of polynomial j's len prefix, counted from the message start (its own prefixes
// included).
RZK_WIRE_HD uint64_t wire_struct_before(const WireSchema& s, uint32_t j) {
  const uint32_t f = wire_field_of(s, j);
  uint64_t b = 0;
  for (uint32_t g = 0; g < f; ++g) b += wire_field_struct(s, g);
  const WireField& F = s.f[f];
  const uint64_t r = j - s.first[f];
  const uint64_t o = r / F.rows;    // element of the outer Vec
  if (F.outer) b += 8;
  if (F.kind == WF_VEC || F.kind == WF_MAT) b += 8 * (o + 1);
  if (F.kind == WF_MAT) b += 8 * (r + 1);
  if (F.kind == WF_OPT) b += 1;
  return b;
}

// Little-endian u64 at p: two 4-byte loads where p is 4-byte aligned (every prefix except those behind an Option
// tag), bytes otherwise.
RZK_WIRE_HD uint64_t wire_load_u64(const uint8_t* p) {
  if (((uintptr_t)p & 3u) == 0) {
    const uint32_t* w = (const uint32_t*)p;
    return (uint64_t)w[0] | ((uint64_t)w[1] << 32);
  }
  uint64_t v = 0;
  for (int i = 0; i < 8; ++i) v |= (uint64_t)p[i] << (8 * i);
  return v;
}

// Reads a u64 count at *pos and requires it to equal `want`.  Caller guarantees *pos <= span.
RZK_WIRE_HD bool wire_expect(const uint8_t* msg, uint64_t span, uint64_t* pos, uint64_t want) {
  if (span - *pos < 8) return false;
  const uint64_t v = wire_load_u64(msg + *pos);
  *pos += 8;
  return v == want;
}

// Walks one message msg[0 .. span) against the schema.  For every polynomial j = 0 .. polys-1 in wire order calls
// emit(j, position of its first coefficient relative to msg, len) — len = kWireNone for an Option that is None —
// and returns the accept bit: every count equals the schema's, every len <= N, every Option tag is 0 or 1, and
// the message ends exactly at span.  The walk keeps pos <= span at all times, checks every load against the span
// before it is issued and compares every u64 from the wire with N or the expected count before it takes part in
// arithmetic, so a hostile len (2^63, 2^64 - 1) never becomes an address.  Coefficients are not read here.
template <class Emit>
RZK_WIRE_HD bool wire_walk(const uint8_t* msg, uint64_t span, const WireSchema& s, Emit& emit) {
  uint64_t pos = 0;
  uint32_t j = 0;
  for (uint32_t f = 0; f < s.nfields; ++f) {
    const WireField& F = s.f[f];
    const uint32_t outer = F.outer ? s.V : 1;
    if (F.outer && !wire_expect(msg, span, &pos, s.V)) return false;
    for (uint32_t o = 0; o < outer; ++o) {
      if ((F.kind == WF_VEC || F.kind == WF_MAT) && !wire_expect(msg, span, &pos, F.rows)) return false;
      for (uint32_t r = 0; r < F.rows; ++r) {
        if (F.kind == WF_MAT && !wire_expect(msg, span, &pos, 1)) return false;
        if (F.kind == WF_OPT) {
          if (span - pos < 1) return false;
          const uint8_t tag = msg[pos];
          pos += 1;
          if (tag > 1) return false;
          if (tag == 0) {
            emit(j++, pos, kWireNone);
            continue;
          }
        }
        if (span - pos < 8) return false;
        const uint64_t len = wire_load_u64(msg + pos);
        pos += 8;
        if (len > s.N) return false;
        const uint64_t nb = len * s.coef_bytes;   // <= 2048 * 8
        if (span - pos < nb) return false;
        emit(j++, pos, (uint32_t)len);
        pos += nb;
      }
    }
  }
  return pos == span;
}

}  // namespace rzk
