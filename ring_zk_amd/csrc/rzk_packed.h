// rzk_packed.h — the fixed-width packed proof format "RZKP1" (include/rzk.h "packed records"), shared by
// the GPU codec (rzk_packed_dev.hip), the entry points (rzk_codec.cpp: sizes and argument rules) and the CPU test
// (tests/test_packed_host.py, g++).  Plain C++.
//
// A record of kind K is one 8-byte header followed by the fields of the kind in the declaration order of the RZK_MSG_*
// table, each slab row-major, polynomial after polynomial; every record of a kind has the same size.
//   header       'R' 'Z' 'K' 'P', u8 version = 1, u8 kind, u16 V little-endian (V = 0 for the kinds without summands):
//                as one little-endian 64-bit word, packed_header(kind, V)
//   polynomial   of width W: ceil(N W / 64) little-endian 64-bit words
//   coefficient  i is the W-bit unsigned value raw = c + bias at bits [i W, (i + 1) W) of the polynomial's bit string;
//                bit j of the string is bit j % 64 of word j / 64
//   padding      bits above N W in the last word are zero (they exist only when N W % 64 != 0, which needs N < 64)
// Field classes (bias, limit = largest valid raw, W = bitlen(limit)):
//   Q   c cp cs t tp ts u g gs   bias (q - 1) / 2     limit q - 1              (W = 32 for every modulus the library takes)
//   Z   z zp zs                  bias verify_bound    limit 2 verify_bound     (|z| <= verify_bound for any accepted proof)
//   D   d                        bias 1               limit 2                  W = 2
// In every class the all-ones value 2^W - 1 is above the limit (q is odd and no power of two, 2 verify_bound is even,
// 3 > 2): encode writes it for a coefficient outside [-bias, limit - bias] and clears ok of the message, so that a
// failed record never decodes as valid.  Decode rejects a wrong header, any raw > limit and any set padding bit.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RZK_PK_HD __host__ __device__ inline
#else
#define RZK_PK_HD inline
#endif

namespace rzk {

// message kinds: the values of RZK_MSG_* (include/rzk.h); 8, 9, 11 and 12 exist in the packed format only, 10 is unassigned
enum PackedKind : int {
  PK_COMMITMENT = 0,         // c
  PK_OPENING = 1,            // a secret, not a stored proof: not supported
  PK_CHALLENGE = 2,          // d
  PK_OPEN_COMMITMENT = 3,    // c, t
  PK_OPEN_RESPONSE = 4,      // z
  PK_LINEAR_COMMITMENT = 5,  // c, cp, g, t, tp, u
  PK_SUM_COMMITMENT = 6,     // cp, cs, gs, tp, ts, u
  PK_SUM_RESPONSE = 7,       // zp, zs
  PK_LINEAR_RESPONSE = 8,    // z, zp
  PK_OPEN_SHORT = 9,         // c, d, z: the signature form of an Open proof (the verifier recomputes t)
  PK_LINEAR_SHORT = 11,      // c, cp, g, d, z, zp: the same for Linear (the verifier recomputes t, tp, u)
  PK_SUM_SHORT = 12,         // cp, cs, gs, d, zp, zs: and for Sum (tp, ts, u)
};

enum PackedClass : uint8_t { PK_Q = 0, PK_Z = 1, PK_D = 2, PK_NCLASSES = 3 };

constexpr int kPackedMaxFields = 6;
constexpr uint32_t kPackedMaxV = 65535;   // V is a u16 of the header
constexpr uint32_t kPackedVersion = 1;

struct PackedWidth {   // one field class over one context
  uint32_t W;       // bits per coefficient, 2 .. 32
  uint32_t bias;    // raw = c + bias
  uint32_t limit;   // largest valid raw; 2^W - 1 > limit
  uint32_t magic;   // ceil(2^32 / W): floor(x / W) = (x * magic) >> 32 for x < 2^27 (packed_div)
};

struct PackedField {
  uint8_t cls;      // PackedClass
  uint8_t pad[3];
  uint32_t rows;    // polynomials of the field per record (V folded in)
  uint32_t wpp;     // 64-bit words per polynomial
  uint32_t woff;    // word offset of the field's first polynomial in the record (the header is word 0)
};

struct PackedSchema {
  uint32_t nfields, N, kind, V;             // V as it stands in the header (0 for the kinds without summands)
  uint32_t polys;                           // polynomials per record
  uint32_t rec_words;                       // 64-bit words per record, header included
  uint32_t first[kPackedMaxFields + 1];     // first polynomial of every field; first[nfields] = polys
  PackedField f[kPackedMaxFields];
  PackedWidth w[PK_NCLASSES];
};

RZK_PK_HD uint32_t packed_bitlen(uint64_t v) {
  uint32_t n = 0;
  while (v) {
    ++n;
    v >>= 1;
  }
  return n;
}

// bias and limit of a class; false when the width would exceed 32 bits or all-ones would not exceed the limit
RZK_PK_HD bool packed_width(uint64_t bias, uint64_t limit, PackedWidth* w) {
  const uint32_t W = packed_bitlen(limit);
  if (W < 2 || W > 32 || bias > limit || limit >= ((1ull << W) - 1)) return false;
  w->W = W;
  w->bias = (uint32_t)bias;
  w->limit = (uint32_t)limit;
  w->magic = (uint32_t)(((1ull << 32) + W - 1) / W);
  return true;
}

// The three classes of a context.  false: q even or outside 32 bits, or verify_bound outside [1, (q-1)/2] (a response
// bound above the canonical range would make "in range" and "canonical" two different things).
RZK_PK_HD bool packed_widths(int64_t q, uint64_t verify_bound, PackedWidth w[PK_NCLASSES]) {
  if (q < 3 || q > 0xffffffffll || (q & 1) == 0) return false;
  const uint64_t half = (uint64_t)(q - 1) / 2;
  if (verify_bound < 1 || verify_bound > half) return false;
  return packed_width(half, (uint64_t)q - 1, &w[PK_Q]) && packed_width(verify_bound, 2 * verify_bound, &w[PK_Z]) &&
         packed_width(1, 2, &w[PK_D]);
}

RZK_PK_HD uint32_t packed_poly_words(uint32_t N, uint32_t W) { return (uint32_t)(((uint64_t)N * W + 63) / 64); }

RZK_PK_HD bool packed_kind_has_v(int kind) { return kind == PK_SUM_COMMITMENT || kind == PK_SUM_RESPONSE || kind == PK_SUM_SHORT; }

// Fills *s for a kind over a context (N, n, k, l, q, verify_bound) and V (Sum kinds; ignored elsewhere).  false: bad
// kind (PK_OPENING included), V == 0 or V > 65535 on a Sum kind, or a context the format does not cover (packed_widths).
RZK_PK_HD bool packed_schema(int kind, uint32_t N, uint32_t n, uint32_t k, uint32_t l, uint32_t V, int64_t q,
                             uint64_t verify_bound, PackedSchema* s) {
  const bool sum = packed_kind_has_v(kind);
  if (sum && (V == 0 || V > kPackedMaxV)) return false;
  if (!packed_widths(q, verify_bound, s->w)) return false;
  if (!sum) V = 1;
  s->N = N;
  s->kind = (uint32_t)kind;
  s->V = sum ? V : 0;
  s->nfields = 0;
  auto add = [&](uint8_t cls, uint32_t rows) {
    PackedField& F = s->f[s->nfields++];
    F.cls = cls;
    F.pad[0] = F.pad[1] = F.pad[2] = 0;
    F.rows = rows;
    F.wpp = F.woff = 0;
  };
  switch (kind) {
    case PK_COMMITMENT: add(PK_Q, n + l); break;
    case PK_CHALLENGE: add(PK_D, 1); break;
    case PK_OPEN_COMMITMENT: add(PK_Q, n + l); add(PK_Q, n); break;
    case PK_OPEN_RESPONSE: add(PK_Z, k); break;
    case PK_LINEAR_COMMITMENT:
      add(PK_Q, n + l); add(PK_Q, n + l); add(PK_Q, 1); add(PK_Q, n); add(PK_Q, n); add(PK_Q, l);
      break;
    case PK_SUM_COMMITMENT:
      add(PK_Q, n + l); add(PK_Q, V * (n + l)); add(PK_Q, V); add(PK_Q, n); add(PK_Q, V * n); add(PK_Q, l);
      break;
    case PK_SUM_RESPONSE: add(PK_Z, k); add(PK_Z, V * k); break;
    case PK_LINEAR_RESPONSE: add(PK_Z, k); add(PK_Z, k); break;
    case PK_OPEN_SHORT: add(PK_Q, n + l); add(PK_D, 1); add(PK_Z, k); break;
    case PK_LINEAR_SHORT:
      add(PK_Q, n + l); add(PK_Q, n + l); add(PK_Q, 1); add(PK_D, 1); add(PK_Z, k); add(PK_Z, k);
      break;
    case PK_SUM_SHORT:
      add(PK_Q, n + l); add(PK_Q, V * (n + l)); add(PK_Q, V); add(PK_D, 1); add(PK_Z, k); add(PK_Z, V * k);
      break;
    default: return false;
  }
  for (uint32_t f = s->nfields; f < (uint32_t)kPackedMaxFields; ++f) s->f[f] = PackedField{};
  uint32_t p = 0;
  uint64_t words = 1;
  for (uint32_t f = 0; f < s->nfields; ++f) {
    PackedField& F = s->f[f];
    F.wpp = packed_poly_words(N, s->w[F.cls].W);
    if (words > 0xffffffffull) return false;
    F.woff = (uint32_t)words;
    s->first[f] = p;
    p += F.rows;
    words += (uint64_t)F.rows * F.wpp;
  }
  for (uint32_t f = s->nfields; f <= (uint32_t)kPackedMaxFields; ++f) s->first[f] = p;
  if (words > 0xffffffffull) return false;
  s->polys = p;
  s->rec_words = (uint32_t)words;
  return true;
}

RZK_PK_HD uint64_t packed_record_bytes(const PackedSchema& s) { return 8ull * s.rec_words; }

// the header as the record's first little-endian 64-bit word
RZK_PK_HD uint64_t packed_header(uint32_t kind, uint32_t V) {
  return 0x52ull | (0x5aull << 8) | (0x4bull << 16) | (0x50ull << 24) | ((uint64_t)kPackedVersion << 32) |
         ((uint64_t)(kind & 0xffu) << 40) | ((uint64_t)(V & 0xffffu) << 48);
}

// field of polynomial j (j < polys)
RZK_PK_HD uint32_t packed_field_of(const PackedSchema& s, uint32_t j) {
  uint32_t f = 0;
  while (f + 1 < s.nfields && j >= s.first[f + 1]) ++f;
  return f;
}

// floor(x / W) for x < 2^27 through the class's magic number: the error term x (magic W - 2^32) stays below 2^32
RZK_PK_HD uint32_t packed_div(uint32_t x, const PackedWidth& w) { return (uint32_t)(((uint64_t)x * w.magic) >> 32); }

// raw value of coefficient c: c + bias when that lies in [0, limit] (true), the all-ones marker otherwise (false).
// All 64 bits of c take part: k 2^32 + s is never packed as s.
RZK_PK_HD bool packed_raw(int64_t c, const PackedWidth& w, uint32_t* raw) {
  const uint64_t u = (uint64_t)c + w.bias;   // c < -bias wraps to at least 2^63
  const bool ok = u <= w.limit;
  *raw = ok ? (uint32_t)u : (uint32_t)((1ull << w.W) - 1);
  return ok;
}

// The same rule for a coefficient of a 32-bit slab, in 32-bit arithmetic: raw = (uint32_t)c + bias, bad = raw > limit.
// Exact for every class because limit = 2 bias and bias < 2^31 (Q: bias = h = (q-1)/2 < 2^31; Z: bias = verify_bound <= h;
// D: bias = 1).  c > limit - bias = bias: c + bias <= 2^31 - 1 + bias < 2^32 does not wrap and exceeds the limit.
// c < -bias: c + bias lies in [-2^31 + bias, -1], which wraps to at least 2^31 + bias > 2 bias = limit.  So for Q every
// out-of-range c lands above 2h, and for Z and D, whose bias is small, a negative overshoot lands far above the limit.
RZK_PK_HD bool packed_raw32(int32_t c, const PackedWidth& w, uint32_t* raw) {
  const uint32_t u = (uint32_t)c + w.bias;
  const bool ok = u <= w.limit;
  *raw = ok ? u : (uint32_t)((1ull << w.W) - 1);
  return ok;
}

// "put coefficient i": ORs raw (below 2^W) into the polynomial's words, which start out zero
RZK_PK_HD void packed_put(uint64_t* words, uint32_t i, uint32_t W, uint32_t raw) {
  const uint64_t bit = (uint64_t)i * W;
  const uint32_t sh = (uint32_t)(bit & 63);
  words[bit >> 6] |= (uint64_t)raw << sh;
  if (sh + W > 64) words[(bit >> 6) + 1] |= (uint64_t)raw >> (64 - sh);
}

// "get coefficient i": the W bits at [i W, (i + 1) W)
RZK_PK_HD uint32_t packed_get(const uint64_t* words, uint32_t i, uint32_t W) {
  const uint64_t bit = (uint64_t)i * W;
  const uint32_t sh = (uint32_t)(bit & 63);
  uint64_t v = words[bit >> 6] >> sh;
  if (sh + W > 64) v |= words[(bit >> 6) + 1] << (64 - sh);
  return (uint32_t)(v & ((1ull << W) - 1));
}

// one polynomial, scalar reference forms.  encode: false when a coefficient was out of range (its marker is written).
RZK_PK_HD bool packed_encode_poly(const int64_t* c, uint32_t N, const PackedWidth& w, uint64_t* words) {
  const uint32_t nw = packed_poly_words(N, w.W);
  for (uint32_t m = 0; m < nw; ++m) words[m] = 0;
  bool ok = true;
  for (uint32_t i = 0; i < N; ++i) {
    uint32_t raw;
    ok = packed_raw(c[i], w, &raw) && ok;
    packed_put(words, i, w.W, raw);
  }
  return ok;
}

// decode: false when a raw value exceeds the limit or a padding bit is set (c is then unspecified)
RZK_PK_HD bool packed_decode_poly(const uint64_t* words, uint32_t N, const PackedWidth& w, int64_t* c) {
  bool ok = true;
  for (uint32_t i = 0; i < N; ++i) {
    const uint32_t raw = packed_get(words, i, w.W);
    ok = ok && raw <= w.limit;
    c[i] = (int64_t)raw - (int64_t)w.bias;
  }
  const uint32_t used = (uint32_t)(((uint64_t)N * w.W) & 63);
  if (used && (words[packed_poly_words(N, w.W) - 1] >> used)) ok = false;
  return ok;
}

// one record: fields[f] points at the record's own rows of field f ([rows of the field][N])
RZK_PK_HD bool packed_encode_record(const PackedSchema& s, const int64_t* const* fields, uint64_t* rec) {
  rec[0] = packed_header(s.kind, s.V);
  bool ok = true;
  for (uint32_t f = 0; f < s.nfields; ++f)
    for (uint32_t r = 0; r < s.f[f].rows; ++r)
      ok = packed_encode_poly(fields[f] + (uint64_t)r * s.N, s.N, s.w[s.f[f].cls], rec + s.f[f].woff + (uint64_t)r * s.f[f].wpp) && ok;
  return ok;
}

RZK_PK_HD bool packed_decode_record(const PackedSchema& s, const uint64_t* rec, int64_t* const* fields) {
  bool ok = rec[0] == packed_header(s.kind, s.V);
  for (uint32_t f = 0; f < s.nfields; ++f)
    for (uint32_t r = 0; r < s.f[f].rows; ++r)
      ok = packed_decode_poly(rec + s.f[f].woff + (uint64_t)r * s.f[f].wpp, s.N, s.w[s.f[f].cls], fields[f] + (uint64_t)r * s.N) && ok;
  return ok;
}

}  // namespace rzk
