// rzk_packed_kernels.inc — the text of packed_encode_kernel and packed_decode_kernel, included by rzk_packed_dev.hip once per
// coefficient width (inside namespace rzk, behind the file's helpers).  Not a template over a shared body on purpose: a
// __global__ wrapper around an inlined body moved the register lines of the 64-bit kernels and cost the 64-bit encoder
// 0.7 % (DESIGN.md §19); included as text, the 64-bit kernels are token for token what they were.  The including file defines
//   RZK_PK_KERNEL(name)   the kernel's symbol (name, name_i32)
//   RZK_PK_COEF           int64_t / int32_t: what the slabs hold (PackedSlabs carries addresses)
//   RZK_PK_PAIR           a lane's piece of two coefficients: v2l, one 16-byte access / int2, one 8-byte access.  Slabs are
//                         16-byte aligned and a piece starts at an even coefficient, so both are naturally aligned
//   RZK_PK_RAW            packed_raw / packed_raw32 (rzk_packed.h)
//   RZK_PK_UNBIAS(r, b)   the decoded coefficient r - b in the slab's type (a valid r is at most 2 b, so it fits an int32_t;
//                         the value of a rejected record is unspecified at either width)
__global__ void __launch_bounds__(64 * kWavesPerBlock) RZK_PK_KERNEL(packed_encode_kernel)(PackedSchema s, PackedSlabs sl, uint64_t* __restrict__ rec,
                                                                            uint8_t* __restrict__ ok, uint64_t npolys) {
  __shared__ uint32_t tile_all[kWavesPerBlock][kTripCoefs];
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t* tile = tile_all[wave_index()];
  const uint32_t trips = (s.N + kTripCoefs - 1) / kTripCoefs;
  const uint32_t ncoef = s.N < kTripCoefs ? s.N : kTripCoefs;   // coefficients per trip (N is a power of two)
  for (uint64_t p = (uint64_t)blockIdx.x * kWavesPerBlock + wave_index(); p < npolys;
       p += (uint64_t)gridDim.x * kWavesPerBlock) {
    const PolyTask t = poly_task(s, p);
    const PackedWidth w = s.w[s.f[t.f].cls];
    const RZK_PK_COEF* src = reinterpret_cast<const RZK_PK_COEF*>(sl.ptr[t.f]) + t.coef;
    uint64_t* dst = rec + t.word;
    if (t.j == 0 && lane == 0) rec[t.b * s.rec_words] = packed_header(s.kind, s.V);
    bool bad = false;
    const bool active = 2u * lane < ncoef;   // (N >= 4 is even: a piece never straddles the end)
    const uint32_t nw = (ncoef * w.W + 63u) / 64u;   // words of one trip, at most 2 W <= 64
    // Loads are unconditional, so that the next trip's piece stays in flight while this one is packed (a load under a
    // branch makes the compiler wait for everything outstanding): an idle lane (N < 128) re-reads the polynomial's first
    // piece and the last trip re-reads itself; both stay inside the polynomial and their values are not used (the indices
    // count coefficients, so this holds at either width).
    const uint32_t at = active ? 2u * lane : 0u;
    RZK_PK_PAIR cc = *reinterpret_cast<const RZK_PK_PAIR*>(src + at);
    for (uint32_t tr = 0; tr < trips; ++tr) {
      const uint32_t tn = tr + 1 < trips ? tr + 1 : tr;
      const RZK_PK_PAIR next = *reinterpret_cast<const RZK_PK_PAIR*>(src + tn * kTripCoefs + at);
      uint32_t r0 = 0, r1 = 0;
      if (active) {
        bad |= !RZK_PK_RAW((RZK_PK_COEF)cc.x, w, &r0);
        bad |= !RZK_PK_RAW((RZK_PK_COEF)cc.y, w, &r1);
      }
      wave_sync();   // the previous trip's reads of the tile are over
      *reinterpret_cast<uint2*>(tile + 2u * lane) = make_uint2(r0, r1);   // lanes past the end store zeros: the padding
      wave_sync();
      if (lane < nw) {
        const uint32_t bit0 = 64u * lane;
        uint64_t word = 0;
        for (uint32_t i = packed_div(bit0, w); i < kTripCoefs && i * w.W < bit0 + 64u; ++i) {
          const int32_t sh = (int32_t)(i * w.W) - (int32_t)bit0;   // -W < sh < 64
          const uint64_t v = tile[i];
          word |= sh >= 0 ? v << sh : v >> (-sh);
        }
        dst[(uint64_t)tr * 2u * w.W + lane] = word;
      }
      cc = next;
    }
    if (wave_any(bad) && lane == 0) ok[t.b] = 0;
  }
}

__global__ void __launch_bounds__(64 * kWavesPerBlock) RZK_PK_KERNEL(packed_decode_kernel)(PackedSchema s, PackedSlabs sl, const uint64_t* __restrict__ rec,
                                                                            uint8_t* __restrict__ ok, uint64_t npolys) {
  __shared__ uint64_t tile_all[kWavesPerBlock][64];
  const uint32_t lane = threadIdx.x & 63u;
  uint64_t* tile = tile_all[wave_index()];
  const uint32_t trips = (s.N + kTripCoefs - 1) / kTripCoefs;
  const uint32_t ncoef = s.N < kTripCoefs ? s.N : kTripCoefs;   // coefficients per trip (N is a power of two)
  for (uint64_t p = (uint64_t)blockIdx.x * kWavesPerBlock + wave_index(); p < npolys;
       p += (uint64_t)gridDim.x * kWavesPerBlock) {
    const PolyTask t = poly_task(s, p);
    const PackedWidth w = s.w[s.f[t.f].cls];
    const uint64_t* src = rec + t.word;
    RZK_PK_COEF* dst = reinterpret_cast<RZK_PK_COEF*>(sl.ptr[t.f]) + t.coef;
    const uint64_t mask = (1ull << w.W) - 1;
    bool bad = false;
    if (t.j == 0 && lane == 0) bad = rec[t.b * s.rec_words] != packed_header(s.kind, s.V);
    const uint32_t bits = ncoef * w.W;
    const uint32_t nw = (bits + 63u) / 64u;   // words of one trip, at most 2 W <= 64
    // unconditional loads, as in the encoder: a lane past the trip's words re-reads word 0, the last trip itself
    const uint32_t at = lane < nw ? lane : 0u;
    uint64_t word = src[at];
    for (uint32_t tr = 0; tr < trips; ++tr) {
      const uint32_t tn = tr + 1 < trips ? tr + 1 : tr;
      const uint64_t next = src[(uint64_t)tn * 2u * w.W + at];
      wave_sync();   // the previous trip's reads of the tile are over
      if (lane < nw) {
        tile[lane] = word;
        if (lane == nw - 1 && (bits & 63u)) bad |= (word >> (bits & 63u)) != 0;   // padding bits
      }
      wave_sync();
      if (2u * lane < ncoef) {
        uint32_t raw[2];
#pragma unroll
        for (uint32_t e = 0; e < 2; ++e) {
          const uint32_t bit = (2u * lane + e) * w.W;
          const uint32_t sh = bit & 63u;
          uint64_t v = tile[bit >> 6] >> sh;
          if (sh + w.W > 64u) v |= tile[(bit >> 6) + 1] << (64u - sh);   // the next word exists: the coefficient ends inside the trip
          raw[e] = (uint32_t)(v & mask);
          bad |= raw[e] > w.limit;
        }
        RZK_PK_PAIR out;
        out.x = RZK_PK_UNBIAS(raw[0], w.bias);
        out.y = RZK_PK_UNBIAS(raw[1], w.bias);
        *reinterpret_cast<RZK_PK_PAIR*>(dst + tr * kTripCoefs + 2u * lane) = out;
      }
      word = next;
    }
    if (wave_any(bad) && lane == 0) ok[t.b] = 0;
  }
}
