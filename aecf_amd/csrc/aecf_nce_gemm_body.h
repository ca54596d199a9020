// The body of the tile GEMM kernels of aecf_nce_gemm.hip -- NOT a header of its own: it is included INSIDE a __global__ function
// template <int AM, int BM, int EPI, int MAP> that has defined
//   p       NceGemmArgs      the arrangement (a kernel argument, or the multi-view kernels' adjusted copy of it)
//   vblock  unsigned int     the output tile's index in the arrangement's map
//   MULTI   constexpr bool   K runs through the segments `ms` (NceSegs) of a multi-view gradient product
// It is text and not a function because nce_gemm_kernel must compile to what it compiled to before the multi-view kernels
// existed: as a __forceinline__ function called from both, six instantiations on the register limit (EPI_RANK, EPI_TOPK,
// EPI_SUP, EPI_SETS_*, EPI_SUP_SELF) came out with other register and spill counts (profiles/multiview_resources.txt).
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = lane_id(), r16 = lane & 15, lg = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(wave_id());
    const int wm = w >> 2, wn = w & 3;

    // ---- fragment addresses
    int a_row[2], b_row[2];             // OP_ROW: per K-step of 32
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        const int ch = ((4 * ks + lg) ^ (r16 >> 1)) & 7;
        a_row[ks] = (128 * wm + r16) * 128 + (ch << 4);
        b_row[ks] = (64 * wn + r16) * 128 + (ch << 4);
    }
    // OP_COL: lane 4 q + pp of group lg reads row 32 ks + 8 lg + 4 hh + q, columns 4 pp .. 4 pp + 3 of 16-column block blk:
    //   8192 ks + 2048 lg + 512 (blk >> 1) + 256 hh + 64 q + 16 ((2 (blk & 1) + (pp >> 1)) ^ (2 (lg & 1) + hh)) + 8 (pp & 1)
    const int q = r16 >> 2, pp = r16 & 3;
    int tx[2][2];
#pragma unroll
    for (int b1 = 0; b1 < 2; ++b1)
#pragma unroll
        for (int hh = 0; hh < 2; ++hh)
            tx[b1][hh] = 2048 * lg + 64 * q + 8 * (pp & 1) + 256 * hh + 16 * ((2 * b1 + (pp >> 1)) ^ (2 * (lg & 1) + hh));
    const int a_img = 16384 * wm;                               // m blocks 8 wm + rt: image wm, block rt
    const int b_img = 16384 * (wn >> 1) + 512 * (2 * (wn & 1)); // n blocks 4 wn + ct: image wn >> 1, block 4 (wn & 1) + ct

    // MULTI: the copies are issued in K order, one step after the other, so the segment of the NEXT copy is a cursor -- its
    // segment, its K-step inside it, and the two operand origins of the segment -- that seg_next moves on: scalar adds, a
    // compare and, at a segment switch, a shift of `fields` that sits in registers; no division, no load and no barrier in a step.
    int sg_seg = 0, sg_t = 0;
    const char* sg_a = p.a;
    const char* sg_b = p.b;
    auto seg_origins = [&]() {
        const unsigned int f = (unsigned int)(ms.fields >> (8 * sg_seg)) & 255u;
        sg_a = p.a + (int64_t)(f & 31u) * ms.a_stride;
        sg_b = p.b + (f >> 5) * ms.view_bytes;
    };
    auto seg_seek = [&](int t) {
        if (MULTI) { sg_seg = t / ms.seg_steps; sg_t = t - sg_seg * ms.seg_steps; seg_origins(); }
    };
    auto seg_next = [&]() {
        if (MULTI) {
            if (++sg_t == ms.seg_steps) { sg_t = 0; ++sg_seg; seg_origins(); }
        }
    };
    // operand tile of K-step t of output tile (mi, ni) (MULTI: t is the cursor's step, K-step sg_t of its segment)
    auto src_a = [&](int t, int mi) -> OperandSrc {
        const char* pa0 = MULTI ? sg_a : p.a;
        if (MULTI) t = sg_t;
        if (AM == OP_ROW) return OperandSrc{pa0 + mi * p.a_sm + t * p.a_st, p.a_rows - BT * mi};
        if (AM == OP_COLB)      // K rows 64 t .. of tile row t / 4, columns of tiles 4 mi .. 4 mi + 3
            return OperandSrc{pa0 + ((int64_t)(t >> 2) * p.a_sm + 4 * (int64_t)mi) * 32768 + (t & 3) * 8192, 64};
        const int k0 = 64 * t < p.a_rows ? 64 * t : p.a_rows - 1;
        return OperandSrc{pa0 + (int64_t)k0 * p.lda + 512 * (int64_t)mi, 64 * t < p.a_rows ? p.a_rows - 64 * t : 1};
    };
    auto src_b = [&](int t, int ni) -> OperandSrc {
        const char* pb0 = MULTI ? sg_b : p.b;
        if (MULTI) t = sg_t;
        if (BM == OP_ROW) return OperandSrc{pb0 + (int64_t)BT * ni * p.ldb + 128 * (int64_t)t, p.b_rows - BT * ni};
        const int k0 = 64 * t < p.b_rows ? 64 * t : p.b_rows - 1;
        return OperandSrc{pb0 + (int64_t)k0 * p.ldb + 512 * (int64_t)ni, 64 * t < p.b_rows ? p.b_rows - 64 * t : 1};
    };
#define NCE_PIECE(P_, oa_, ob_, stage_, mi_, ni_)                                                                       \
    do {                                                                                                                \
        if ((P_) < 4) issue_piece<AM, (P_) & 3>(oa_, p.lda, p.a_cbytes - 512 * (mi_), smem + (stage_) * STAGE);          \
        else issue_piece<BM, (P_) & 3>(ob_, p.ldb, p.b_cbytes - 512 * (ni_), smem + (stage_) * STAGE + OPB);             \
    } while (0)
    // fragment of slot sl = 8 ks + rt (m operand) / of (ks, ct) (n operand) from the tile at lds
    auto read_a = [&](const char* la, int sl) -> u32x4 {
        const int ks = sl >> 3, rt = sl & 7;
        if (AM == OP_ROW) return *reinterpret_cast<const u32x4*>(la + a_row[ks] + 2048 * rt);
        const int o = a_img + 8192 * ks + 512 * (rt >> 1);
        return tr_frag16(la, o + tx[rt & 1][0], o + tx[rt & 1][1]);
    };
    auto read_b = [&](const char* lb, int ks, int ct) -> u32x4 {
        if (BM == OP_ROW) return *reinterpret_cast<const u32x4*>(lb + b_row[ks] + 2048 * ct);
        const int o = b_img + 8192 * ks + 512 * (ct >> 1);
        return tr_frag16(lb, o + tx[ct & 1][0], o + tx[ct & 1][1]);
    };
    auto k_range = [&](int split, int& t_beg, int& t_end) {
        t_beg = split * p.steps_per_split;
        t_end = t_beg + p.steps_per_split < p.k_steps ? t_beg + p.steps_per_split : p.k_steps;
    };
    OperandSrc pa = {nullptr, 1}, pb = {nullptr, 1};            // the copy whose pieces 3..7 are still to be issued
    // first copies of an output tile: step t_beg whole into stage 0, the first 3 pieces of step t_beg + 1 into stage 1
    auto issue_first = [&](int mi, int ni, int t_beg, int t_end) {
        if (t_beg >= t_end) return;
        seg_seek(t_beg);
        const OperandSrc oa = src_a(t_beg, mi), ob = src_b(t_beg, ni);
        NCE_PIECE(0, oa, ob, 0, mi, ni); NCE_PIECE(1, oa, ob, 0, mi, ni); NCE_PIECE(2, oa, ob, 0, mi, ni);
        NCE_PIECE(3, oa, ob, 0, mi, ni); NCE_PIECE(4, oa, ob, 0, mi, ni); NCE_PIECE(5, oa, ob, 0, mi, ni);
        NCE_PIECE(6, oa, ob, 0, mi, ni); NCE_PIECE(7, oa, ob, 0, mi, ni);
        if (t_beg + 1 < t_end) {
            seg_next();
            pa = src_a(t_beg + 1, mi); pb = src_b(t_beg + 1, ni);
            NCE_PIECE(0, pa, pb, 1, mi, ni); NCE_PIECE(1, pa, pb, 1, mi, ni); NCE_PIECE(2, pa, pb, 1, mi, ni);
        }
    };

    int mi = 0, ni = 0, split = 0, t_beg = 0, t_end = 0;
    if (!nce_tile_of<MAP>(p, vblock, mi, ni, split)) return;
    k_range(split, t_beg, t_end);
    // EPI_EXP_MASK: thread t < 256 reads the presence byte of the block's row t, thread 256 + t that of its column t (the padding:
    // no bit set).  Issued HERE, older than every operand copy, so that the copies' vmcnt counts stand and its latency passes
    // behind the K loop.
    unsigned int my_byte = 0;
    if (epi_is_mask(EPI)) {
        const int t = threadIdx.x & (BT - 1);
        const bool is_row = threadIdx.x < BT;
        const int k = BT * (is_row ? mi : ni) + t;
        if (k < (is_row ? p.m_valid : p.n_valid)) my_byte = (is_row ? p.pres_row : p.pres_col)[k];
    }
    issue_first(mi, ni, t_beg, t_end);
    {
        f32x4 acc[8][4];
#pragma unroll
        for (int rt = 0; rt < 8; ++rt)
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};

        // ---- main loop.  A K-step is 16 slots of 4 MFMAs (slot = (ks, rt): one m fragment against the 4 n fragments); the m
        // fragments run through a ring of 4 registers, read 3 slots ahead.  ONE barrier per K-step, at slot 13: by then every
        // read of this step's stage has been issued (and is waited for), and the copy of step t + 1 -- issued a full step
        // earlier -- is waited for, so behind the barrier (a) slots 13..15 read the first fragments of step t + 1 from the
        // other stage (no bubble at the step boundary) and (b) the copy of step t + 2 into THIS stage starts.  The 8
        // wave-instructions of a copy are spread over 8 slots (3 behind the barrier, 5 at the start of the next step) so that
        // their issue cost hides behind MFMAs instead of stacking up in front of them.
        u32x4 af[4], bf0[4], bf1[4];
        if (t_beg < t_end) {
            // younger than the first step's 8 pieces: the 3 pieces of the second step
            if (t_beg + 1 < t_end) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            af[0] = read_a(smem, 0); af[1] = read_a(smem, 1); af[2] = read_a(smem, 2);
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) bf0[ct] = read_b(smem + OPB, 0, ct);
        }
        int st = 0;
        // one K-step; H1 / H2: steps t + 1 / t + 2 exist (compile-time: the steady-state body has no branches)
        auto kstep = [&](int t, auto h1, auto h2) {
            constexpr bool H1 = decltype(h1)::value, H2 = decltype(h2)::value;
            const char* cur = smem + st * STAGE;
            const char* nxt = smem + (st ^ 1) * STAGE;
            OperandSrc qa = {nullptr, 1}, qb = {nullptr, 1};
#pragma unroll
            for (int sl = 0; sl < 16; ++sl) {
                if (sl == 13 && H1) {
                    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
                    __builtin_amdgcn_s_barrier();
                    if (H2) { seg_next(); qa = src_a(t + 2, mi); qb = src_b(t + 2, ni); }
                }
                if (sl < 5 && H1) {
                    switch (sl) {
                        case 0: NCE_PIECE(3, pa, pb, st ^ 1, mi, ni); break;
                        case 1: NCE_PIECE(4, pa, pb, st ^ 1, mi, ni); break;
                        case 2: NCE_PIECE(5, pa, pb, st ^ 1, mi, ni); break;
                        case 3: NCE_PIECE(6, pa, pb, st ^ 1, mi, ni); break;
                        default: NCE_PIECE(7, pa, pb, st ^ 1, mi, ni); break;
                    }
                }
                if (sl >= 13 && H2) {
                    switch (sl) {
                        case 13: NCE_PIECE(0, qa, qb, st, mi, ni); break;
                        case 14: NCE_PIECE(1, qa, qb, st, mi, ni); break;
                        default: NCE_PIECE(2, qa, qb, st, mi, ni); break;
                    }
                }
                if (sl <= 12) af[(sl + 3) & 3] = read_a(cur, sl + 3);
                else if (H1) af[(sl + 3) & 3] = read_a(nxt, sl - 13);
                if (sl >= 4 && sl <= 7) bf1[sl - 4] = read_b(cur + OPB, 1, sl - 4);
                if (sl >= 13 && H1) {
                    bf0[sl - 13] = read_b(nxt + OPB, 0, sl - 13);
                    if (sl == 15) bf0[3] = read_b(nxt + OPB, 0, 3);
                }
#pragma unroll
                for (int ct = 0; ct < 4; ++ct)
                    acc[sl & 7][ct] = Tr<BF16>::mma(sl < 8 ? bf0[ct] : bf1[ct], af[sl & 3], acc[sl & 7][ct]);
                __builtin_amdgcn_sched_barrier(0);              // the slot order IS the schedule
            }
            pa = qa; pb = qb;
            st ^= 1;
        };
        {
            using T_ = std::integral_constant<bool, true>;
            using F_ = std::integral_constant<bool, false>;
            int t = t_beg;
            for (; t + 2 < t_end; ++t) kstep(t, T_{}, T_{});
            if (t + 1 < t_end) { kstep(t, T_{}, F_{}); ++t; }
            if (t < t_end) kstep(t, F_{}, F_{});
        }

        // ---- epilogue: lane (r16, lg) holds C[m = 128 wm + 16 rt + r16][n = 64 wn + 16 ct + 4 lg + r], r = 0..3
        const int64_t gi0 = (int64_t)BT * mi + 128 * wm + r16;
        const int gj0 = BT * ni + 64 * wn + 4 * lg;
        if (EPI == EPI_OUT || EPI == EPI_OUT_TD || EPI == EPI_OUT_S || EPI == EPI_OUT_TD_S) {
            if (EPI == EPI_OUT_S || EPI == EPI_OUT_TD_S) {
                // g is stored unscaled: coef / Tc and the gradient arriving at the loss meet the float32 sums here
                float osc = p.coef * nce_dev_inv_temp(p.temp, p.min_temp);
                if (p.upstream) osc *= p.upstream[0];
#pragma unroll
                for (int rt = 0; rt < 8; ++rt)
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) acc[rt][ct] *= osc;
            }
            float* o = reinterpret_cast<float*>(p.out) + (int64_t)split * p.slab_stride;
            unsigned short* ob = reinterpret_cast<unsigned short*>(p.out);
#pragma unroll
            for (int rt = 0; rt < 8; ++rt) {
                const int64_t i = gi0 + 16 * rt;
                if (i < p.m_valid) {
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) {
                        const int j = gj0 + 16 * ct;
                        if (j < p.n_valid) {
                            if (p.out_bf16)
                                *reinterpret_cast<u32x2*>(ob + i * p.ldo + j) =
                                    u32x2{pack_bf16x2(acc[rt][ct][0], acc[rt][ct][1]), pack_bf16x2(acc[rt][ct][2], acc[rt][ct][3])};
                            else *reinterpret_cast<f32x4*>(o + i * p.ldo + j) = acc[rt][ct];
                        }
                    }
                }
            }
            if (EPI == EPI_OUT_TD || EPI == EPI_OUT_TD_S) {
                float td = 0.f;
#pragma unroll
                for (int rt = 0; rt < 8; ++rt) {
                    const int64_t i = gi0 + 16 * rt;
                    if (i < p.m_valid) {
#pragma unroll
                        for (int ct = 0; ct < 4; ++ct) {
                            const int j = gj0 + 16 * ct;
                            if (j < p.n_valid) {
                                const u32x2 x = *reinterpret_cast<const u32x2*>(p.tdot_src + i * p.ldo + j);
                                td = fmaf(acc[rt][ct][0], __uint_as_float(x[0] << 16), td);
                                td = fmaf(acc[rt][ct][1], __uint_as_float(x[0] & 0xffff0000u), td);
                                td = fmaf(acc[rt][ct][2], __uint_as_float(x[1] << 16), td);
                                td = fmaf(acc[rt][ct][3], __uint_as_float(x[1] & 0xffff0000u), td);
                            }
                        }
                    }
                }
                td = reduce_wave(td);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();                   // every wave is past its last read of the stages
                float* red = reinterpret_cast<float*>(smem);
                if (lane == 0) red[w] = td;
                __syncthreads();
                if (threadIdx.x == 0)
                    p.tdot_part[((int64_t)split * p.m_tiles + mi) * p.n_tiles + ni] =
                        ((red[0] + red[1]) + (red[2] + red[3])) + ((red[4] + red[5]) + (red[6] + red[7]));
            }
        } else if (EPI == EPI_SIG) {
            // n = l log2(e) straight from the accumulator: l = acc / Tc + bias is never formed
            const float s2 = nce_dev_inv_temp(p.temp, p.min_temp) * 1.4426950408889634f, b2 = p.bias[0] * 1.4426950408889634f;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();                       // every wave is past its last read of the stages
            float* lsp = reinterpret_cast<float*>(smem);        // [4][256] softplus sums | [4][256] g sums
            float* lsg = lsp + 4 * BT;
            // block-uniform: only tiles on the band of positives or on the ragged edge pay for the selects
            const int64_t p0 = p.row_offset + (int64_t)BT * mi;
            const bool special = BT * (mi + 1) > p.m_valid || BT * (ni + 1) > p.n_valid ||
                                 (p0 < (int64_t)BT * (ni + 1) && p0 + BT > (int64_t)BT * ni);
            unsigned short* gtile = p.e + ((int64_t)mi * p.e_tiles + 4 * ni + wn) * (BT * 64) + (128 * wm + r16) * 64 + 4 * lg;
            float rsp[8], rsg[8];
            auto rows8 = [&](auto special_c) {
                constexpr bool SP = decltype(special_c)::value;
#pragma unroll
                for (int rt = 0; rt < 8; ++rt) {
                    const int64_t i = gi0 + 16 * rt;
                    const bool iok = i < p.m_valid;
                    const int64_t jp = p.row_offset + i;
                    f32x2 sl = f32x2{0.f, 0.f}, sc = f32x2{0.f, 0.f}, sg = f32x2{0.f, 0.f};
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) {
                        const int j = gj0 + 16 * ct;
                        f32x2 g[2];
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const f32x2 n = f32x2{acc[rt][ct][2 * h], acc[rt][ct][2 * h + 1]} * f32x2{s2, s2} + f32x2{b2, b2};
                            SigTerms x = sig_terms(n);
                            if (SP) {
                                // the positive: softplus(-l) and -sigmoid(-l), formed from -n (not as differences)
                                const SigTerms y = sig_terms(-n);
#pragma unroll
                                for (int k = 0; k < 2; ++k) {
                                    const int col = j + 2 * h + k;
                                    const bool pos = col == jp, ok = iok && col < p.n_valid;
                                    x.sig[k] = ok ? (pos ? -y.sig[k] : x.sig[k]) : 0.f;
                                    x.lg2[k] = ok ? (pos ? y.lg2[k] : x.lg2[k]) : 0.f;
                                    x.corr[k] = ok ? (pos ? y.corr[k] : x.corr[k]) : 0.f;
                                }
                            }
                            sl += x.lg2; sc += x.corr; sg += x.sig;
                            g[h] = x.sig;
                        }
                        // tile (mi, 4 ni + wn) of g: row 128 wm + 16 rt + r16, columns 16 ct + 4 lg .. + 3 of its 64
                        *reinterpret_cast<u32x2*>(gtile + (16 * rt) * 64 + 16 * ct) = u32x2{pack_bf16x2(g[0][0], g[0][1]), pack_bf16x2(g[1][0], g[1][1])};
                    }
                    rsp[rt] = reduce_lg(fmaf(sl[0] + sl[1], 0.6931471805599453f, sc[0] + sc[1]));     // over the wave's 64 columns
                    rsg[rt] = reduce_lg(sg[0] + sg[1]);
                }
            };
            if (special) rows8(std::integral_constant<bool, true>{});
            else rows8(std::integral_constant<bool, false>{});
            if (lg == 0) {
#pragma unroll
                for (int rt = 0; rt < 8; ++rt) {
                    lsp[wn * BT + 128 * wm + 16 * rt + r16] = rsp[rt];
                    lsg[wn * BT + 128 * wm + 16 * rt + r16] = rsg[rt];
                }
            }
            __syncthreads();
            const int tdx = threadIdx.x & (BT - 1);
            const float* src = threadIdx.x < BT ? lsp : lsg;
            (threadIdx.x < BT ? p.sp_part : p.sg_part)[((int64_t)ni * p.m_tiles + mi) * BT + tdx] =
                (src[tdx] + src[BT + tdx]) + (src[2 * BT + tdx] + src[3 * BT + tdx]);
        } else if (EPI == EPI_RANK) {
            // row thresholds first (their latency passes while the other waves arrive); padding re-reads the last one
            const bool cols_on = p.pos_col != nullptr;                  // block-uniform
            float pr[8];
#pragma unroll
            for (int rt = 0; rt < 8; ++rt) {
                const int64_t i = gi0 + 16 * rt;
                pr[rt] = p.pos_row[i < p.m_valid ? i : p.m_valid - 1];
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();                       // every wave is past its last read of the stages
            int* lrow = reinterpret_cast<int*>(smem);           // [4][256] row counts | [2][256] column counts
            int* lcol = lrow + 4 * BT;
            // block-uniform: only tiles on the band of positives or on the ragged edge pay for the selects
            const int64_t p0 = p.row_offset + (int64_t)BT * mi;
            const bool special = BT * (mi + 1) > p.m_valid || BT * (ni + 1) > p.n_valid ||
                                 (p0 < (int64_t)BT * (ni + 1) && p0 + BT > (int64_t)BT * ni);
            // the accumulator of (rt, ct, r); SP: the positive and the padding become a NaN -- one select, and every comparison
            // with it is false.  The empty asm keeps the value opaque: comparisons that the variants below have in common would
            // otherwise be hoisted in front of the branch, hundreds of masks at once, and spill.
            auto elem = [&](auto special_c, int rt, int ct, int r) -> float {
                constexpr bool SP = decltype(special_c)::value;
                float sv = acc[rt][ct][r];
                asm volatile("" : "+v"(sv));
                if (SP) {
                    const int64_t i = gi0 + 16 * rt;
                    const int col = gj0 + 16 * ct + r;
                    sv = ((i < p.m_valid) & (col < p.n_valid) & (col != p.row_offset + i)) ? sv : __builtin_nanf("");
                }
                return sv;
            };
            // rows: greater | equal << 16 over the wave's 64 columns (<= 64 in either half), then over the 4 lane groups
            auto count_rows = [&](auto special_c) {
#pragma unroll
                for (int rt = 0; rt < 8; ++rt) {
                    int rg = 0, re = 0;
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float sv = elem(special_c, rt, ct, r);
                            rg += (int)(sv > pr[rt]);
                            re += (int)(sv == pr[rt]);
                        }
                    }
                    int v = rg | (re << 16);
                    v += __shfl_xor(v, 16, 64);
                    v += __shfl_xor(v, 32, 64);
                    if (lg == 0) lrow[wn * BT + 128 * wm + 16 * rt + r16] = v;
                }
            };
            // columns: the same over the wave's 128 rows (<= 128 in either half), then over the 16 lanes of a group
            auto count_cols = [&](auto special_c) {
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) {
                    float pc[4];
                    int cg[4], ce[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int j = gj0 + 16 * ct + r;
                        pc[r] = p.pos_col[j < p.n_valid ? j : p.n_valid - 1];
                        cg[r] = ce[r] = 0;
                    }
#pragma unroll
                    for (int rt = 0; rt < 8; ++rt) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float sv = elem(special_c, rt, ct, r);
                            cg[r] += (int)(sv > pc[r]);
                            ce[r] += (int)(sv == pc[r]);
                        }
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        int v = cg[r] | (ce[r] << 16);
                        v += __shfl_xor(v, 1, 64);
                        v += __shfl_xor(v, 2, 64);
                        v += __shfl_xor(v, 4, 64);
                        v += __shfl_xor(v, 8, 64);
                        if (r16 == 0) lcol[wm * BT + 64 * wn + 16 * ct + 4 * lg + r] = v;
                    }
                }
            };
            using T_ = std::integral_constant<bool, true>;
            using F_ = std::integral_constant<bool, false>;
            if (special) {
                count_rows(T_{});
                if (cols_on) count_cols(T_{});
            } else {
                count_rows(F_{});
                if (cols_on) count_cols(F_{});
            }
            __syncthreads();
            const int tdx = threadIdx.x;
            if (tdx < BT) {
                p.rank_row_part[((int64_t)ni * p.m_tiles + mi) * BT + tdx] = (lrow[tdx] + lrow[BT + tdx]) + (lrow[2 * BT + tdx] + lrow[3 * BT + tdx]);
            } else if (cols_on) {
                const int c = tdx - BT;
                p.rank_col_part[((int64_t)mi * p.n_tiles + ni) * BT + c] = lcol[c] + lcol[BT + c];
            }
        } else if (EPI == EPI_TOPK) {
            typedef unsigned long long u64;
            const int kk = p.topk;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();                       // every wave is past its last read of the stages
            u64* lst = reinterpret_cast<u64*>(smem);            // [4 wn][16 slots][256 rows] keys: the 128 KB of the stages
            // block-uniform: only tiles holding an excluded partner or a ragged edge pay for the selects
            const int64_t p0 = p.row_offset + (int64_t)BT * mi;
            const bool special = BT * (mi + 1) > p.m_valid || BT * (ni + 1) > p.n_valid ||
                                 (p0 < (int64_t)BT * (ni + 1) && p0 + BT > (int64_t)BT * ni);
            const unsigned int inv0 = ~(unsigned)gj0;           // inverted column of (ct, r): inv0 - (16 ct + r)
            auto rows8 = [&](auto special_c) {
                constexpr bool SP = decltype(special_c)::value;
#pragma unroll
                for (int rt = 0; rt < 8; ++rt) {
                    const int64_t i = gi0 + 16 * rt;
                    u64 K[16];
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            float sv = acc[rt][ct][r];
                            asm volatile("" : "+v"(sv));        // (opaque: keeps the two variants' common work behind the branch)
                            sv += 0.f;                          // -0 -> +0: equal scores have one image
                            const unsigned int b = __float_as_uint(sv);
                            unsigned int u = b ^ ((unsigned)((int)b >> 31) | 0x80000000u);
                            u = sv != sv ? 1u : u;
                            u64 key = ((u64)u << 32) | (u64)(inv0 - (unsigned)(16 * ct + r));
                            if (SP) {
                                const int col = gj0 + 16 * ct + r;
                                key = ((i < p.m_valid) & (col < p.n_valid) & (col != p.row_offset + i)) ? key : 0ull;
                            }
                            K[4 * ct + r] = key;
                        }
                    }
                    // the lane's 16 keys, best first: Batcher's merge exchange, 63 compare-exchanges
#define TOPK_CE(x_, y_)                                                                                                 \
    do {                                                                                                                \
        const u64 hi_ = K[x_] > K[y_] ? K[x_] : K[y_], lo_ = K[x_] > K[y_] ? K[y_] : K[x_];                             \
        K[x_] = hi_; K[y_] = lo_;                                                                                       \
    } while (0)
                    TOPK_CE(0, 1); TOPK_CE(2, 3); TOPK_CE(4, 5); TOPK_CE(6, 7); TOPK_CE(8, 9); TOPK_CE(10, 11); TOPK_CE(12, 13); TOPK_CE(14, 15);
                    TOPK_CE(0, 2); TOPK_CE(1, 3); TOPK_CE(4, 6); TOPK_CE(5, 7); TOPK_CE(8, 10); TOPK_CE(9, 11); TOPK_CE(12, 14); TOPK_CE(13, 15);
                    TOPK_CE(1, 2); TOPK_CE(5, 6); TOPK_CE(9, 10); TOPK_CE(13, 14);
                    TOPK_CE(0, 4); TOPK_CE(1, 5); TOPK_CE(2, 6); TOPK_CE(3, 7); TOPK_CE(8, 12); TOPK_CE(9, 13); TOPK_CE(10, 14); TOPK_CE(11, 15);
                    TOPK_CE(2, 4); TOPK_CE(3, 5); TOPK_CE(10, 12); TOPK_CE(11, 13);
                    TOPK_CE(1, 2); TOPK_CE(3, 4); TOPK_CE(5, 6); TOPK_CE(9, 10); TOPK_CE(11, 12); TOPK_CE(13, 14);
                    TOPK_CE(0, 8); TOPK_CE(1, 9); TOPK_CE(2, 10); TOPK_CE(3, 11); TOPK_CE(4, 12); TOPK_CE(5, 13); TOPK_CE(6, 14); TOPK_CE(7, 15);
                    TOPK_CE(4, 8); TOPK_CE(5, 9); TOPK_CE(6, 10); TOPK_CE(7, 11);
                    TOPK_CE(2, 4); TOPK_CE(3, 5); TOPK_CE(6, 8); TOPK_CE(7, 9); TOPK_CE(10, 12); TOPK_CE(11, 13);
                    TOPK_CE(1, 2); TOPK_CE(3, 4); TOPK_CE(5, 6); TOPK_CE(7, 8); TOPK_CE(9, 10); TOPK_CE(11, 12); TOPK_CE(13, 14);
#undef TOPK_CE
                    // the wave's 64 columns of the row lie in 4 lane groups: pop the largest of the 4 heads k times
                    u64* dst = lst + (wn * 16) * BT + 128 * wm + 16 * rt + r16;
                    for (int t = 0; t < kk; ++t) {
                        u64 win = K[0];
                        u64 o = __shfl_xor(win, 16, 64);
                        win = o > win ? o : win;
                        o = __shfl_xor(win, 32, 64);
                        win = o > win ? o : win;
                        if (lg == 0) dst[t * BT] = win;
                        const bool mine = K[0] == win;          // keys are distinct (only sentinels repeat)
#pragma unroll
                        for (int j = 0; j < 15; ++j) K[j] = mine ? K[j + 1] : K[j];
                        K[15] = mine ? 0ull : K[15];
                    }
                }
            };
            if (special) rows8(std::integral_constant<bool, true>{});
            else rows8(std::integral_constant<bool, false>{});
            __syncthreads();
            if (threadIdx.x < BT) {
                // one thread per row: the 4 waves' sorted lists into the tile's list
                const u64* l0 = lst + threadIdx.x;
                u64* out = p.topk_part + (((int64_t)ni * p.m_tiles + mi) * BT + threadIdx.x) * p.topk_kp;
                u64 h[4];
                int c[4];
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) { h[q4] = l0[(q4 * 16) * BT]; c[q4] = 0; }
                for (int t = 0; t < kk; ++t) {
                    const u64 h01 = h[0] > h[1] ? h[0] : h[1], h23 = h[2] > h[3] ? h[2] : h[3];
                    const u64 best = h01 > h23 ? h01 : h23;
                    out[t] = best;
#pragma unroll
                    for (int q4 = 0; q4 < 4; ++q4) {
                        const bool won = h[q4] == best;
                        c[q4] += (int)won;
                        const bool more = c[q4] < kk;
                        const u64 nx = l0[(q4 * 16 + (more ? c[q4] : 0)) * BT];
                        h[q4] = won ? (more ? nx : 0ull) : h[q4];
                    }
                }
            }
        } else {
            float scale2 = p.scale2, shift2 = p.shift2;
            // EPI_SUP: the labels of the lane's 8 rows and 16 columns are read here (their latency passes behind the exponentials)
            // and kept as 32-bit keys: equal classes have equal keys; a row that can match nothing (unlabeled or padding, which
            // re-reads the last label) gets a key no column has, and the other way round.  24 registers beside the accumulators
            // where the int64 labels would take 48 and spill.
            unsigned int kr[8], kc[16];
            if (epi_has_labels(EPI)) {
#pragma unroll
                for (int rt = 0; rt < 8; ++rt) {
                    const int i = (int)gi0 + 16 * rt;
                    const bool iok = i < p.m_valid;
                    const long long l = sup_label_at(p.lab_row, iok ? i : p.m_valid - 1);
                    kr[rt] = (iok && l >= 0) ? sup_label_key(l) : 0xffffffffu;
                }
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    const int j = gj0 + 16 * (c >> 2) + (c & 3);
                    const bool jok = j < p.n_valid;
                    const long long l = sup_label_at(p.lab_col, jok ? j : p.n_valid - 1);
                    kc[c] = (jok && l >= 0) ? sup_label_key(l) : 0xfffffffeu;
                }
            }
            // EPI_SETS_*: thread t < 256 reads the word of the block's row t, thread 256 + t that of its column t (the padding: the
            // empty set); they go to LDS behind the barrier
            unsigned long long my_set = 0ull;
            if (epi_has_sets(EPI)) {
                const int t = threadIdx.x & (BT - 1);
                const bool is_row = threadIdx.x < BT;
                const int k = BT * (is_row ? mi : ni) + t;
                const unsigned long long* src = reinterpret_cast<const unsigned long long*>(is_row ? p.lab_row : p.lab_col);
                if (k < (is_row ? p.m_valid : p.n_valid)) my_set = src[k];
            }
            // EPI_EXP_MASK: whether the thread's row or column (read in front of the K loop) holds both views of the pair; the flags
            // go to LDS behind the barrier
            const bool my_pres = epi_is_mask(EPI) && (my_byte & p.pres_need) == p.pres_need;
            if (EPI == EPI_EXP_DT || epi_has_labels(EPI) || epi_has_sets(EPI) || EPI == EPI_EXP_SELF || epi_is_mask(EPI) || epi_has_ts(EPI)) {
                scale2 = nce_dev_inv_temp(p.temp, p.min_temp) * 1.4426950408889634f;
                shift2 = scale2;
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();                       // every wave is past its last read of the stages
            if (epi_has_sets(EPI))                              // [256] row words | [256] column words, behind the 18 float planes
                reinterpret_cast<unsigned long long*>(smem + 18 * BT * 4)[threadIdx.x] = my_set;
            // EPI_EXP_MASK: [256] row flags | [256] column flags (bytes) | [8] the waves' votes, behind the 6 float planes in use
            const unsigned char* pflag = reinterpret_cast<const unsigned char*>(smem + 18 * BT * 4);
            bool all_present = true;
            if (epi_is_mask(EPI)) {
                reinterpret_cast<unsigned char*>(smem + 18 * BT * 4)[threadIdx.x] = my_pres ? 1 : 0;
                const int vote = __all(my_pres ? 1 : 0);
                int* votes = reinterpret_cast<int*>(smem + 18 * BT * 4 + 2 * BT);
                if (lane == 0) votes[w] = vote;
                __syncthreads();
                // ONE step tells the block whether its 512 rows and columns all hold the pair: then it is EPI_EXP_DT's tile
                all_present = __builtin_amdgcn_readfirstlane(((votes[0] & votes[1]) & (votes[2] & votes[3])) &
                                                             ((votes[4] & votes[5]) & (votes[6] & votes[7]))) != 0;
            }
            // E = exp2(acc scale - shift): 4 consecutive columns per lane, 8-byte stores (16 rows x 32 B per wave-instruction).
            // The sums run as packed float32 adds (both halves from their own registers); masking only on edge tiles.
            float rs[8];
            f32x2 cs2[4][2];
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) cs2[ct][0] = cs2[ct][1] = f32x2{0.f, 0.f};
            float* lrs = reinterpret_cast<float*>(smem);        // [4][256] row sums | [2][256] column sums
            float* lcs = lrs + 4 * BT;
            bool edge = BT * (mi + 1) > p.m_valid || BT * (ni + 1) > p.n_valid;            // block-uniform
            if (epi_is_self(EPI)) {
                // the band of excluded keys (column row_offset + i of row i) crosses this tile: it takes the branch of the ragged
                // edge, so only the tiles that hold such an element pay for the index test
                const int64_t p0 = p.row_offset + (int64_t)BT * mi;
                edge = edge || (p0 < (int64_t)BT * (ni + 1) && p0 + BT > (int64_t)BT * ni);
            }
            // EPI_EXP_MASK: a tile with an absent row or column (the padding included) takes that branch too, block-uniform
            if (epi_is_mask(EPI)) edge = !all_present;
            if (epi_has_ts(EPI)) {
                // EPI_EXP_DTS / EPI_EXP_MASK_S: a sweep of its own over the accumulators, IN FRONT of the E sweep, for the dT sums
                // of a per-pair temperature: t_ij = E_ij (s_ij - 1) summed per row and per column in float32 (E the float32
                // exponential the E sweep forms, by the same expression; the product is excluded by the same selects, never by
                // value).  In front, because the E sweep lets every accumulator go as it stores its row: this sweep holds the 128
                // accumulators and its 16 column sums and nothing else -- the E sweep's own peak -- and hands its sums to LDS
                // before the E sweep starts.  The scale and the lane's indices are made opaque HERE so that no exponential is
                // kept for the E sweep and no address of this sweep is formed in front of the K loop and carried through it.
                // Partials: the planes behind lcs ([4][256] rows at plane 6, [2][256] columns at plane 14).
                float* lrn = lrs + 6 * BT;
                float* lcn = lrs + 14 * BT;
                float sc2 = scale2, sh2 = shift2;
                int r16s = r16, lgs = lg;
                asm volatile("" : "+v"(sc2), "+v"(sh2), "+v"(r16s), "+v"(lgs));
                const int64_t gi0s = (int64_t)BT * mi + 128 * wm + r16s;
                const int gj0s = BT * ni + 64 * wn + 4 * lgs;
                f32x2 ts2[4][2];
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) ts2[ct][0] = ts2[ct][1] = f32x2{0.f, 0.f};
#pragma unroll
                for (int rt = 0; rt < 8; ++rt) {
                    const int64_t i = gi0s + 16 * rt;
                    f32x2 s2 = f32x2{0.f, 0.f};
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) {
                        const int j = gj0s + 16 * ct;
                        const f32x4 sv = acc[rt][ct];
                        f32x2 t01, t23;
                        t01[0] = __builtin_amdgcn_exp2f(sv[0] * sc2 - sh2) * (sv[0] - 1.0f);
                        t01[1] = __builtin_amdgcn_exp2f(sv[1] * sc2 - sh2) * (sv[1] - 1.0f);
                        t23[0] = __builtin_amdgcn_exp2f(sv[2] * sc2 - sh2) * (sv[2] - 1.0f);
                        t23[1] = __builtin_amdgcn_exp2f(sv[3] * sc2 - sh2) * (sv[3] - 1.0f);
                        if (epi_is_mask(EPI)) {
                            if (edge) {
                                const bool iok = pflag[128 * wm + 16 * rt + r16s] != 0;
                                const unsigned int cw = *reinterpret_cast<const unsigned int*>(pflag + BT + 64 * wn + 16 * ct + 4 * lgs);
                                t01[0] = (iok && (cw & 0x000000ffu)) ? t01[0] : 0.f;
                                t01[1] = (iok && (cw & 0x0000ff00u)) ? t01[1] : 0.f;
                                t23[0] = (iok && (cw & 0x00ff0000u)) ? t23[0] : 0.f;
                                t23[1] = (iok && (cw & 0xff000000u)) ? t23[1] : 0.f;
                            }
                        } else if (edge) {
                            const bool iok = i < p.m_valid;
                            t01[0] = (iok && j + 0 < p.n_valid) ? t01[0] : 0.f;
                            t01[1] = (iok && j + 1 < p.n_valid) ? t01[1] : 0.f;
                            t23[0] = (iok && j + 2 < p.n_valid) ? t23[0] : 0.f;
                            t23[1] = (iok && j + 3 < p.n_valid) ? t23[1] : 0.f;
                        }
                        s2 += t01 + t23;
                        ts2[ct][0] += t01;
                        ts2[ct][1] += t23;
                    }
                    const float v = reduce_lg(s2[0] + s2[1]);   // over the wave's 64 columns
                    if (lgs == 0) lrn[wn * BT + 128 * wm + 16 * rt + r16s] = v;
                }
#pragma unroll
                for (int ct = 0; ct < 4; ++ct)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float v = reduce_r16(ts2[ct][r >> 1][r & 1]);     // over the wave's 128 rows
                        if (r16s == 0) lcn[wm * BT + 64 * wn + 16 * ct + 4 * lgs + r] = v;
                    }
                __builtin_amdgcn_sched_barrier(0);
            }
            unsigned short* etile = p.e + ((int64_t)mi * p.e_tiles + 4 * ni + wn) * (BT * 64) + (128 * wm + r16) * 64 + 4 * lg;
#pragma unroll
            for (int rt = 0; rt < 8; ++rt) {
                const int64_t i = gi0 + 16 * rt;
                f32x2 s2 = f32x2{0.f, 0.f};
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) {
                    const int j = gj0 + 16 * ct;
                    f32x2 e01, e23;
                    e01[0] = __builtin_amdgcn_exp2f(acc[rt][ct][0] * scale2 - shift2);
                    e01[1] = __builtin_amdgcn_exp2f(acc[rt][ct][1] * scale2 - shift2);
                    e23[0] = __builtin_amdgcn_exp2f(acc[rt][ct][2] * scale2 - shift2);
                    e23[1] = __builtin_amdgcn_exp2f(acc[rt][ct][3] * scale2 - shift2);
                    if (epi_is_mask(EPI)) {
                        if (edge) {
                            // the flags carry the padding: a row or column that does not exist is absent.  Selects on the flags
                            // alone -- what an absent slot's score holds (NaN, inf) never reaches a sum
                            const bool iok = pflag[128 * wm + 16 * rt + r16] != 0;
                            const unsigned int cw = *reinterpret_cast<const unsigned int*>(pflag + BT + 64 * wn + 16 * ct + 4 * lg);
                            e01[0] = (iok && (cw & 0x000000ffu)) ? e01[0] : 0.f;
                            e01[1] = (iok && (cw & 0x0000ff00u)) ? e01[1] : 0.f;
                            e23[0] = (iok && (cw & 0x00ff0000u)) ? e23[0] : 0.f;
                            e23[1] = (iok && (cw & 0xff000000u)) ? e23[1] : 0.f;
                        }
                    } else if (edge) {
                        const bool iok = i < p.m_valid;
                        // EPI_EXP_SELF: the excluded key by its index (a row that exists has row_offset + i < n_valid < 2^31; unsigned,
                        // so that the padding rows past it wrap instead of overflowing)
                        const unsigned int js = epi_is_self(EPI) ? (unsigned)p.row_offset + (unsigned)i : 0u;
                        e01[0] = (iok && j + 0 < p.n_valid && (!epi_is_self(EPI) || (unsigned)j + 0u != js)) ? e01[0] : 0.f;
                        e01[1] = (iok && j + 1 < p.n_valid && (!epi_is_self(EPI) || (unsigned)j + 1u != js)) ? e01[1] : 0.f;
                        e23[0] = (iok && j + 2 < p.n_valid && (!epi_is_self(EPI) || (unsigned)j + 2u != js)) ? e23[0] : 0.f;
                        e23[1] = (iok && j + 3 < p.n_valid && (!epi_is_self(EPI) || (unsigned)j + 3u != js)) ? e23[1] : 0.f;
                    }
                    s2 += e01 + e23;
                    if (!epi_is_self(EPI)) {
                        cs2[ct][0] += e01;
                        cs2[ct][1] += e23;
                    }
                    // tile (mi, 4 ni + wn) of E: row 128 wm + 16 rt + r16, columns 16 ct + 4 lg .. + 3 of its 64 -- the four
                    // stores of a row group fill whole 128-byte lines of one 32 KB tile
                    *reinterpret_cast<u32x2*>(etile + (16 * rt) * 64 + 16 * ct) = u32x2{pack_bf16x2(e01[0], e01[1]), pack_bf16x2(e23[0], e23[1])};
                }
                rs[rt] = reduce_lg(s2[0] + s2[1]);              // over the wave's 64 columns
            }
            float cs[4][4];
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) { cs[ct][0] = cs2[ct][0][0]; cs[ct][1] = cs2[ct][0][1]; cs[ct][2] = cs2[ct][1][0]; cs[ct][3] = cs2[ct][1][1]; }
            if (lg == 0) {
#pragma unroll
                for (int rt = 0; rt < 8; ++rt) lrs[wn * BT + 128 * wm + 16 * rt + r16] = rs[rt];
            }
            if (!epi_is_self(EPI)) {
#pragma unroll
                for (int ct = 0; ct < 4; ++ct)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float v = reduce_r16(cs[ct][r]);  // over the wave's 128 rows
                        if (r16 == 0) lcs[wm * BT + 64 * wn + 16 * ct + 4 * lg + r] = v;
                    }
            }
            float* lrn = lcs + 2 * BT;                          // EPI_SUP: [4][256] row counts | [4][256] row sums |
            float* lrx = lrn + 4 * BT;                          //          [2][256] column counts | [2][256] column sums
            float* lcn = lrx + 4 * BT;
            float* lcx = lcn + 2 * BT;
            if (epi_has_labels(EPI)) {
                constexpr bool COLS = EPI == EPI_SUP;           // EPI_SUP_SELF: the row half alone
                // block-uniform: only tiles on the band of partners or on the ragged edge pay for the index tests
                const int64_t p0 = p.row_offset + (int64_t)BT * mi;
                const bool special = edge || (p0 < (int64_t)BT * (ni + 1) && p0 + BT > (int64_t)BT * ni);
                auto label_stats = [&](auto special_c) {
                    constexpr bool SP = decltype(special_c)::value;
                    // Matches are sparse, so the tile is first searched with the 32-bit keys: two VALU operations per element and
                    // no compare mask.  Only a row group (rt) with a key hit somewhere in the wave reads its int64 labels again
                    // (from L1 / L2) and forms the 64-bit matches and the sums -- a vote that changes no bit: a group without a
                    // match would have summed zeros.
                    // the column sums gather in LDS, in the slots of the lanes that own them (r16 == 0: one lane per column and
                    // wave), row group after row group: 32 accumulators less beside the 128 of the tile
                    float* wcn = lcn + wm * BT + 64 * wn + 4 * lg;
                    float* wcx = lcx + wm * BT + 64 * wn + 4 * lg;
                    if (COLS && r16 == 0) {
#pragma unroll
                        for (int c = 0; c < 16; ++c) wcn[16 * (c >> 2) + (c & 3)] = wcx[16 * (c >> 2) + (c & 3)] = 0.f;
                    }
#pragma unroll
                    for (int rt = 0; rt < 8; ++rt) {
                        unsigned int nearest = 0xffffffffu;
#pragma unroll
                        for (int c = 0; c < 16; ++c) {
                            const unsigned int x = kr[rt] ^ kc[c];
                            nearest = x < nearest ? x : nearest;
                        }
                        float rn = 0.f, rx = 0.f;
                        if (__any(nearest == 0u)) {
                            // (opaque: nothing this rare branch needs -- indices, addresses, the labels themselves -- may be
                            // formed in front of it or kept from the reads in front of the exponentials: it would sit in scratch)
                            int i = (int)gi0 + 16 * rt, gj = gj0;
                            const long long* lab_row = p.lab_row;
                            const long long* lab_col = p.lab_col;
                            asm volatile("" : "+v"(i), "+v"(gj), "+s"(lab_row), "+s"(lab_col));
                            const long long lr = sup_label_at(lab_row, i < p.m_valid ? i : p.m_valid - 1);
                            // SP: the partner counts by index, not here; its column relative to gj (-1: not in this lane's 64)
                            const int64_t rel = p.row_offset + i - gj;
                            const int jpr = (rel >= 0 && rel < 64) ? (int)rel : -1;
#pragma unroll
                            for (int c = 0; c < 16; ++c) {
                                const int j = gj + 16 * (c >> 2) + (c & 3);
                                // (the keys carry the padding: an equal key is a row and a column that exist)
                                bool m = (kr[rt] == kc[c]) & sup_label_match(lr, sup_label_at(lab_col, j < p.n_valid ? j : p.n_valid - 1));
                                if (SP) m = m & (jpr != 16 * (c >> 2) + (c & 3));
                                const float one = m ? 1.f : 0.f, sv = m ? acc[rt][c >> 2][c & 3] : 0.f;
                                rn += one; rx += sv;
                                if (COLS) {
                                    const float c1 = reduce_r16(one), c2 = reduce_r16(sv);  // over the group's 16 rows
                                    if (r16 == 0) {
                                        wcn[16 * (c >> 2) + (c & 3)] += c1;
                                        wcx[16 * (c >> 2) + (c & 3)] += c2;
                                    }
                                }
                            }
                            rn = reduce_lg(rn);                 // over the wave's 64 columns
                            rx = reduce_lg(rx);
                        }
                        if (lg == 0) {
                            lrn[wn * BT + 128 * wm + 16 * rt + r16] = rn;
                            lrx[wn * BT + 128 * wm + 16 * rt + r16] = rx;
                        }
                    }
                };
                if (special) label_stats(std::integral_constant<bool, true>{});
                else label_stats(std::integral_constant<bool, false>{});
            }
            if (epi_is_sets(EPI)) {
                constexpr bool JAC = EPI == EPI_SETS_JAC;
                typedef unsigned long long u64;
                __syncthreads();                                // the staged words are in place
                const u64* lsr = reinterpret_cast<const u64*>(smem + 18 * BT * 4) + 128 * wm + r16;            // + 16 rt
                const u64* lsc = reinterpret_cast<const u64*>(smem + 18 * BT * 4) + BT + 64 * wn + 4 * lg;     // + 16 ct + r
                // block-uniform: only the tiles on the band of partners pay for the index test (the padding weighs 0 by its sets)
                const int64_t p0 = p.row_offset + (int64_t)BT * mi;
                const bool special = p0 < (int64_t)BT * (ni + 1) && p0 + BT > (int64_t)BT * ni;
                // the partner of the lane's row of group rt is its element 16 ct + r where rel == 16 (ct - rt) + r
                const int64_t rel64 = p.row_offset + gi0 - gj0;
                const int rel = (rel64 > -512 && rel64 < 512) ? (int)rel64 : -4096;
                auto set_stats = [&](auto special_c) {
                    constexpr bool SP = decltype(special_c)::value;
                    float rw[8], rx[8];
#pragma unroll
                    for (int rt = 0; rt < 8; ++rt) rw[rt] = rx[rt] = 0.f;
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) {
                        u64 B[4];
                        int pb[4];
                        float cw[4], cx[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            B[r] = lsc[16 * ct + r];
                            pb[r] = JAC ? __popcll(B[r]) : 0;
                            cw[r] = cx[r] = 0.f;
                        }
#pragma unroll
                        for (int rt = 0; rt < 8; ++rt) {
                            const u64 A = lsr[16 * rt];
                            const int pa = JAC ? __popcll(A) : 0;
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                float wt = set_weight<JAC>(A, B[r], pa, pb[r]);
                                if (SP) wt = rel == 16 * (ct - rt) + r ? 0.f : wt;
                                const float sv = acc[rt][ct][r];
                                rw[rt] += wt;
                                rx[rt] = fmaf(wt, sv, rx[rt]);
                                cw[r] += wt;
                                cx[r] = fmaf(wt, sv, cx[r]);
                            }
                        }
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float c1 = reduce_r16(cw[r]), c2 = reduce_r16(cx[r]);     // over the wave's 128 rows
                            if (r16 == 0) {
                                lcn[wm * BT + 64 * wn + 16 * ct + 4 * lg + r] = c1;
                                lcx[wm * BT + 64 * wn + 16 * ct + 4 * lg + r] = c2;
                            }
                        }
                    }
#pragma unroll
                    for (int rt = 0; rt < 8; ++rt) {
                        const float r1 = reduce_lg(rw[rt]), r2 = reduce_lg(rx[rt]);         // over the wave's 64 columns
                        if (lg == 0) {
                            lrn[wn * BT + 128 * wm + 16 * rt + r16] = r1;
                            lrx[wn * BT + 128 * wm + 16 * rt + r16] = r2;
                        }
                    }
                };
                if (special) set_stats(std::integral_constant<bool, true>{});
                else set_stats(std::integral_constant<bool, false>{});
            }
            if (epi_is_sets_self(EPI)) {
                // the ROW half of the sweep above, chain for chain (ct-major over the lane's 16 elements of a row, then the lane
                // groups): 16 row accumulators and the 4 column words of the group, no column accumulators and no LDS column slots
                constexpr bool JAC = EPI == EPI_SETS_JAC_SELF;
                typedef unsigned long long u64;
                __syncthreads();                                // the staged words are in place
                const u64* lsr = reinterpret_cast<const u64*>(smem + 18 * BT * 4) + 128 * wm + r16;            // + 16 rt
                const u64* lsc = reinterpret_cast<const u64*>(smem + 18 * BT * 4) + BT + 64 * wn + 4 * lg;     // + 16 ct + r
                // block-uniform: only the tiles the band of anchors crosses pay for the index test (the padding weighs 0 by its sets)
                const int64_t p0 = p.row_offset + (int64_t)BT * mi;
                const bool special = p0 < (int64_t)BT * (ni + 1) && p0 + BT > (int64_t)BT * ni;
                // the anchor of the lane's row of group rt is its element 16 ct + r where rel == 16 (ct - rt) + r: weight 0 by INDEX,
                // never by its set or its value (a bit-identical row with the same set elsewhere in the view is a positive)
                const int64_t rel64 = p.row_offset + gi0 - gj0;
                const int rel = (rel64 > -512 && rel64 < 512) ? (int)rel64 : -4096;
                auto set_row_stats = [&](auto special_c) {
                    constexpr bool SP = decltype(special_c)::value;
                    float rw[8], rx[8];
#pragma unroll
                    for (int rt = 0; rt < 8; ++rt) rw[rt] = rx[rt] = 0.f;
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) {
                        u64 B[4];
                        int pb[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            B[r] = lsc[16 * ct + r];
                            pb[r] = JAC ? __popcll(B[r]) : 0;
                        }
#pragma unroll
                        for (int rt = 0; rt < 8; ++rt) {
                            const u64 A = lsr[16 * rt];
                            const int pa = JAC ? __popcll(A) : 0;
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                float wt = set_weight<JAC>(A, B[r], pa, pb[r]);
                                if (SP) wt = rel == 16 * (ct - rt) + r ? 0.f : wt;
                                rw[rt] += wt;
                                rx[rt] = fmaf(wt, acc[rt][ct][r], rx[rt]);
                            }
                        }
                    }
#pragma unroll
                    for (int rt = 0; rt < 8; ++rt) {
                        const float r1 = reduce_lg(rw[rt]), r2 = reduce_lg(rx[rt]);         // over the wave's 64 columns
                        if (lg == 0) {
                            lrn[wn * BT + 128 * wm + 16 * rt + r16] = r1;
                            lrx[wn * BT + 128 * wm + 16 * rt + r16] = r2;
                        }
                    }
                };
                if (special) set_row_stats(std::integral_constant<bool, true>{});
                else set_row_stats(std::integral_constant<bool, false>{});
            }
            __syncthreads();
            const int tdx = threadIdx.x;
            if (tdx < BT) {
                const int64_t o = ((int64_t)ni * p.m_tiles + mi) * BT + tdx;
                p.rowsum_part[o] = (lrs[tdx] + lrs[BT + tdx]) + (lrs[2 * BT + tdx] + lrs[3 * BT + tdx]);
                if (epi_has_ts(EPI)) p.rowsx_part[o] = (lrn[tdx] + lrn[BT + tdx]) + (lrn[2 * BT + tdx] + lrn[3 * BT + tdx]);
                if (epi_has_labels(EPI) || epi_has_sets(EPI)) {
                    p.rowcnt_part[o] = (lrn[tdx] + lrn[BT + tdx]) + (lrn[2 * BT + tdx] + lrn[3 * BT + tdx]);
                    p.rowsx_part[o] = (lrx[tdx] + lrx[BT + tdx]) + (lrx[2 * BT + tdx] + lrx[3 * BT + tdx]);
                }
            } else if (!epi_is_self(EPI)) {
                const int c = tdx - BT;
                const int64_t o = ((int64_t)mi * p.n_tiles + ni) * BT + c;
                p.colsum_part[o] = lcs[c] + lcs[BT + c];
                if (epi_has_ts(EPI)) p.colsx_part[o] = lcn[c] + lcn[BT + c];
                if (EPI == EPI_SUP || epi_is_sets(EPI)) {
                    p.colcnt_part[o] = lcn[c] + lcn[BT + c];
                    p.colsx_part[o] = lcx[c] + lcx[BT + c];
                }
            }
        }
    }
#undef NCE_PIECE
