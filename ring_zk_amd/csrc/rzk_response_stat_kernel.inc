// rzk_response_stat_kernel.inc — the text of response_stat_kernel, included by rzk_response_stat_dev.hip once per coefficient
// width (inside namespace rzk, behind kTeams); as text and not as a template over a shared body or a further template
// argument for the reason given at the head of rzk_packed_kernels.inc: the 64-bit kernel keeps its symbol and expands to the
// instantiations of the helpers it always used (DESIGN.md §20: its resource line did not move).  The including file defines
//   RZK_RS_KERNEL(name)   the kernel's symbol (name, name_i32)
//   RZK_RS_COEF           int64_t / int32_t: what the slabs y, r, d, z hold (Operands carries addresses).  The operand loads
//                         are the coefficient-typed load_pairs / operand_ptr / shift_product_bytes of the rotation kernels
//                         (rzk_rowprog.h); the addend is one 16- / 8-byte ld_stream per pair (CoefPair) with the canonical
//                         test of its width (canon_pair); z leaves as one 16- / 8-byte non-temporal store per pair.
//   RZK_RS_TEAM           WaveTeam / WaveTeam32: the team of the word-image fallback shift_product
// The statistic, the partial layout, the flags, the DPP sums and the LDS image do not depend on the width.
template <int LOGN, bool TRUSTED, bool BYTES>
__global__ void __launch_bounds__(64 * kTeams, (BYTES ? RZK_SHIFT_BYTES_WAVES : 1))
RZK_RS_KERNEL(response_stat_kernel)(const Program* __restrict__ prog, const Operands ops, const DevTables* __restrict__ Tp, const uint32_t ntasks,
                     const ResponseStat so) {
  using S = ShiftGeo<LOGN, true, 6>;
  using C = RZK_RS_COEF;
  constexpr int E = S::E;
  constexpr int N = S::N;
  constexpr int LANES = S::LANES;
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int lane = threadIdx.x & (LANES - 1);
  const uint32_t team = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int32_t* slab = reinterpret_cast<int32_t*>(smem) + team * S::WORDS;
  const DevTables& T = *Tp;
  const uint32_t q = T.crt.q;
  const uint32_t nrows = prog->nrows;

  for (uint32_t task = blockIdx.x * kTeams + team; task < ntasks; task += gridDim.x * kTeams) {
    const uint32_t b = task / nrows;
    const uint32_t rowi = task - b * nrows;
    const uint32_t bo = ops.group > 1 ? b / ops.group : b;
    const Row row = prog->rows[rowi];
    const uint32_t qhalf = T.crt.qhalf;
    constexpr bool trusted = TRUSTED;
    bool fault = false;
    {
      uint32_t res[E];
#pragma unroll
      for (int i = 0; i < E; ++i) res[i] = 0;
#pragma unroll 1
      for (uint32_t t = 0; t < row.nterms; ++t) {
        const Term tm = prog->terms[row.term0 + t];
        int32_t a[E];
        uint32_t abad = 0, amx = 0;
        load_pairs<LOGN, 6, C>(a, operand_ptr<C>(ops, tm.a_op, tm.a_off, b, bo, N), lane, qhalf, abad, amx, trusted);
        if (!trusted) fault = fault || canon_fail(abad, amx, qhalf);
        const C* __restrict__ pv = operand_ptr<C>(ops, tm.b_op, tm.b_off, b, bo, N);
        bool done = false;
        if constexpr (BYTES) done = shift_product_bytes<LOGN, C>(res, tm.sign < 0, a, pv, lane, slab, T, fault, trusted);
        if (!done) shift_product<LOGN, true, false, RZK_RS_TEAM, kShiftH, C>(res, false, tm.sign < 0, a, pv, lane, slab, T, fault, trusted);
      }
      // the sums move to the idle image, each thread's pairs in its own 8-byte slots (as shift_row_kernel)
      wave_sync();
      uint2* own = reinterpret_cast<uint2*>(slab) + lane;
#pragma unroll
      for (int g = 0; g < S::G; ++g) own[g * LANES] = make_uint2(res[2 * g], res[2 * g + 1]);
    }
    constexpr int GC = S::G < 4 ? S::G : 4;   // pairs per trip
    uint32_t in_bad = 0, in_mx = 0;
    RejectAcc acc{0, 0, 0, 0};
#pragma unroll 1
    for (int g0 = 0; g0 < S::G; g0 += GC) {
      uint32_t r[2 * GC], vq[2 * GC];   // vq: the product sum mod q, r: with the additions
      const uint2* own = reinterpret_cast<const uint2*>(slab) + lane + g0 * LANES;
#pragma unroll
      for (int g = 0; g < GC; ++g) {
        const uint2 v = own[g * LANES];
        r[2 * g] = vq[2 * g] = v.x, r[2 * g + 1] = vq[2 * g + 1] = v.y;
      }
#pragma unroll 1
      for (uint32_t ai = 0; ai < row.nadds; ++ai) {
        const AddTerm ad = prog->adds[row.add0 + ai];
        using P2 = typename CoefPair<C>::type;
        const P2* __restrict__ p =
            reinterpret_cast<const P2*>(operand_ptr<C>(ops, ad.op & ADD_OP_MASK, ad.off, b, bo, N)) + g0 * LANES + lane;
        int32_t av[2 * GC];
        if (trusted) {
#pragma unroll
          for (int g = 0; g < GC; ++g) {
            const P2 t = ld_stream(p + g * LANES);
            pair_words(t, av[2 * g], av[2 * g + 1]);
          }
        } else {
#pragma unroll
          for (int g = 0; g < GC; ++g) canon_pair(ld_stream(p + g * LANES), qhalf, in_bad, in_mx, av[2 * g], av[2 * g + 1]);
        }
        if (ad.sign >= 0) {
#pragma unroll
          for (int i = 0; i < 2 * GC; ++i) r[i] = addq(r[i], zq_from_centered(av[i], q), q);
        } else {
#pragma unroll
          for (int i = 0; i < 2 * GC; ++i) r[i] = subq(r[i], zq_from_centered(av[i], q), q);
        }
      }
      P2Out<C>* __restrict__ dst =
          reinterpret_cast<P2Out<C>*>(const_cast<C*>(operand_ptr<C>(ops, row.out_op, row.out_off, b, bo, N))) + g0 * LANES + lane;
#pragma unroll
      for (int g = 0; g < GC; ++g) {
        const int64_t c0 = center_from_zq(r[2 * g], T.crt), c1 = center_from_zq(r[2 * g + 1], T.crt);
        store_result_pair(dst + g * LANES, c0, c1);
        // the statistic of the pair (the canonical verdict of y, r and d is wave-uniform and joins the flags below)
        reject_step_v<false>(acc, c0, center_from_zq(vq[2 * g], T.crt), false, so.vmax);
        reject_step_v<false>(acc, c1, center_from_zq(vq[2 * g + 1], T.crt), false, so.vmax);
      }
    }
    const bool noncanon = fault || canon_fail(in_bad, in_mx, qhalf);   // (both false in trusted mode)
    if (noncanon) input_fault(ops, nullptr, bo, lane);
    // a lane's clamped sum z^2 is at most 32 x 2^48 = 2^53: wave_sum_u56 is exact; S2 - 2 S1 is any 64-bit value
    const uint64_t e = wave_sum_u64(reject_e(acc));
    const uint64_t zsq = wave_sum_u56(acc.zsq);
    const uint32_t flags = (noncanon ? (uint32_t)kRejNonCanon : 0u) | (__any(acc.flags & kRejVmax) ? (uint32_t)kRejVmax : 0u);
    if (lane == 0)
      so.part[(size_t)bo * so.rows_total + so.part_off + (b - bo * ops.group) * nrows + rowi] =
          reject_partial(e, zsq, flags, so.norm_limit);
    wave_sync();   // the next task's image overwrites the slots read above
  }
}
