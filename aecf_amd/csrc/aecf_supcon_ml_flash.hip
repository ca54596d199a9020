// Streaming multi-label supervised contrastive loss, bf16, gfx950 (aecf_supcon_ml_fwd_bwd): the label-aware term of
// aecf_supcon_flash.hip with a SET of classes per row instead of one class -- one uint64 per row, bit c = class c, C <= 64 -- and a
// weight in [0, 1] in place of the match.  aecf_label_sets_pack (the last kernel of this file) makes the words from multi-hot rows.
//
//   w(i, j) = 1                                   j == row_offset + i   (the partner counts by INDEX, whatever the sets say)
//           = [A_i & B_j != 0]                    weighting 0, "overlap"
//           = |A_i & B_j| / |A_i | B_j|           weighting 1, "jaccard": two __popcll and one float32 division (0 for an empty union)
//   W_i    = sum_j w(i, j)  (>= 1)     x_ij = q_i.k_j / T     lse_i = logsumexp_j x_ij
//   loss_i = lse_i - (1 / W_i) sum_j w(i, j) x_ij             G = softmax_j - w / W_i
//   dq = coef/T G k          dk = coef/T G^T q          dT = -(1/Tc) sum_i q_i . dq_i
// An empty set is an unlabeled row: its and shares no bit with anything, so it has the partner alone and is nobody's positive.
//
// The three roles are those of aecf_supcon_flash.hip on the loop of aecf_flash_stream.h, the set of a streamed row loaded inside
// weights() as its label is there:
//   STATS  online maximum m_b / sum l_b per stationary row b, and per lane the float32 sums of its w and of its w x; each live
//          split writes (m, l, wsum, psum) and sml_rows_kernel merges them in order into lse, inv_W = 1 / W and loss_rows.
//   DQ     P[a, b] = ct (exp(S/T - lse_b) - w(b, a) inv_W_b), ct = coef / T; partial Out per live split, added in order by
//          sml_dq_kernel, which leaves tq_i = q_i . dq_i for launch_nce_dtemp.
//   DK     the same weight with lse, inv_W and the set loaded per streamed row; one pass, no partials, float32 dk.
// A weight is rounded to bf16 once, as the B operand of the second product.  No float atomics, every sum in a fixed order: the
// same inputs give the same bits.  With one-hot sets w is exactly 0 or 1, every product with it is exact and every sum is the sum
// aecf_supcon_flash.hip forms: the outputs are its bits.
//
// The weighting is a template parameter (JAC) and the weight arithmetic is straight-line -- no branch on the weighting, on an empty
// intersection or on a zero weight -- so the scheduler can place it among the fragment reads and MFMAs as it places the compare of
// aecf_supcon_flash.hip; as a wave-uniform kernel argument it cost 7 % (overlap) and 19 % (jaccard) at configs[2] size
// (profiles/supcon_ml_time.txt), each branch being a scheduling barrier.
// Registers (profiles/supcon_ml_resources.txt): the overlap instances take those of aecf_supcon_flash.hip; the popcounts and the
// quotient cost the Jaccard gradient roles 2 - 4 more: d = 768 in one launch sits at the 256-VGPR limit (256 + 196 / 198 AGPRs,
// two values parked in AGPRs, no scratch) and d = 1024 in two (256 + 133 / 136).  Every instance is free of scratch and spills.
#include <math.h>

#include "aecf_flash_stream.h"

namespace aecf {

namespace {

enum { SML_STATS = 0, SML_DQ = 1, SML_DK = 2 };

struct SmlFlashArgs {
    const unsigned short* stat;     // stationary rows [ns, d]   (STATS, DQ: q; DK: k)
    const unsigned short* strm;     // streamed rows   [nm, d]   (STATS, DQ: k; DK: q)
    int64_t ns, nm;
    int64_t row_offset;             // the partner of local row i is key row_offset + i
    const uint64_t* stat_set;       // sets of the stationary rows [ns]
    const uint64_t* strm_set;       // sets of the streamed rows   [nm]
    const float* temp;              // device scalar: inv_temp = 1 / max(*temp, min_temp)
    float min_temp, coef;
    float* part_m;                  // STATS: [KS, ns] each
    float* part_l;
    float* part_w;
    float* part_ps;
    const float* lse;               // DQ, DK: [rows] of the local q rows
    const float* inv_w;
    float* part_o;                  // DQ: [KS, ns, d]
    float* out;                     // DK: dk [ns, d]
    int64_t strm_per_split;         // STATS, DQ: streamed rows per split (a multiple of 32); no launched split is empty
};

// the weight of two sets (symmetric in them), straight-line: 0 / max(|union|, 1) is the exact 0 of disjoint and of empty sets
template <bool JAC>
__device__ __forceinline__ float sml_weight(uint64_t mine, uint64_t other) {
    const uint64_t both = mine & other;
    if constexpr (!JAC) return both != 0 ? 1.0f : 0.0f;
    const int uni = __popcll(mine | other);
    return (float)__popcll(both) / (float)(uni > 0 ? uni : 1);
}

// STATS: online softmax statistics of stationary row b = r16 (replicated over lg) and this lane's share of its weights
template <bool JAC>
struct SmlStatsTerm {
    static constexpr bool FENCED = false;
    float inv_temp;
    const uint64_t* set;            // of the range's first streamed row
    uint64_t mine;
    int pos_t;
    float run_m = -INFINITY, run_l = 0.f, psum = 0.f, wsum = 0.f;
    template <int NC>
    __device__ __forceinline__ void weights(const f32x4& sacc, int a0, int lg, int r16, int len, f32x4 (&oacc)[NC], float (&pv)[4]) {
        float tmax = -INFINITY;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int a = a0 + 4 * lg + r;
            float x = -INFINITY;
            if (a < len) {
                x = sacc[r] * inv_temp;
                const float w = a == pos_t ? 1.0f : sml_weight<JAC>(mine, set[a]);
                psum = fmaf(w, x, psum);                         // (w = 0 leaves both sums as they are)
                wsum += w;
            }
            pv[r] = x;
            tmax = fmaxf(tmax, x);
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        const float new_m = fmaxf(run_m, tmax);
        if (__any(new_m > run_m)) {                               // wave-uniform
            run_l *= (run_m == -INFINITY) ? 0.f : expf(run_m - new_m);
            run_m = new_m;
        }
        float ts_ = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) ts_ += expf(pv[r] - run_m);
        ts_ += __shfl_xor(ts_, 16, 64);
        ts_ += __shfl_xor(ts_, 32, 64);
        run_l += ts_;
    }
};

// DQ: the weight of key a for the lane's query b from that query's lse and 1 / W
template <bool JAC>
struct SmlDqTerm {
    static constexpr bool FENCED = false;
    float inv_temp, ct, lse_b, inv_w_b;
    const uint64_t* set;            // key sets, of the range's first streamed row
    uint64_t mine;
    int pos_t;
    template <int NC>
    __device__ __forceinline__ void weights(const f32x4& sacc, int a0, int lg, int r16, int len, f32x4 (&oacc)[NC], float (&pv)[4]) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int a = a0 + 4 * lg + r;                        // key
            float v = 0.f;
            if (a < len) {
                v = expf(sacc[r] * inv_temp - lse_b);
                const float w = a == pos_t ? 1.0f : sml_weight<JAC>(mine, set[a]);
                v = fmaf(-w, inv_w_b, v);
                v *= ct;
            }
            pv[r] = v;
        }
    }
};

// DK: the same weight for the lane's key b and local query a: lse, 1 / W and the set are the streamed row's
template <bool JAC>
struct SmlDkTerm {
    static constexpr bool FENCED = false;
    float inv_temp, ct;
    const float* lse;               // of the range's first streamed row, as inv_w and set
    const float* inv_w;
    const uint64_t* set;
    uint64_t mine;
    int pos_t;
    template <int NC>
    __device__ __forceinline__ void weights(const f32x4& sacc, int a0, int lg, int r16, int len, f32x4 (&oacc)[NC], float (&pv)[4]) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int a = a0 + 4 * lg + r;                        // local q row
            float v = 0.f;
            if (a < len) {
                v = expf(sacc[r] * inv_temp - lse[a]);
                const float w = a == pos_t ? 1.0f : sml_weight<JAC>(mine, set[a]);
                v = fmaf(-w, inv_w[a], v);
                v *= ct;
            }
            pv[r] = v;
        }
    }
};

// CSPLIT > 1: the output columns come from CSPLIT launches of D / CSPLIT columns each (cpart = which), every one forming S
template <int KT, int ROLE, int CSPLIT, bool JAC>
__global__ __launch_bounds__(256, 1) void sml_flash_kernel(SmlFlashArgs p, int cpart) {
    constexpr int D = 32 * KT, NC = ROLE == SML_STATS ? 1 : D / 16 / CSPLIT;
    const float inv_temp = nce_dev_inv_temp(p.temp, p.min_temp);
    const int c_first = cpart * NC;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const FlashBlock f = flash_block<ROLE != SML_DK>(p.ns, p.nm, p.strm_per_split);
    const int64_t b = f.s0 + f.r16;                               // lane (lg, r16) ends with Out[b][16 c + 4 lg + r]
    const bool live = b < p.ns;
    const uint64_t mine = live ? p.stat_set[b] : (uint64_t)0;
    f32x4 oacc[NC];
    if constexpr (ROLE == SML_STATS) {
        SmlStatsTerm<JAC> term;
        term.inv_temp = inv_temp; term.set = p.strm_set + f.m_beg; term.mine = mine;
        term.pos_t = flash_rel(p.row_offset + b, f);
        flash_stream<KT, 1, false>(term, f, p.stat, p.ns, p.strm, 0, smem, oacc);
        float ps = term.psum;                                     // a lane holds a quarter of row b's weights
        float ws = term.wsum;
        ps = ps + __shfl_xor(ps, 16, 64);
        ps = ps + __shfl_xor(ps, 32, 64);
        ws = ws + __shfl_xor(ws, 16, 64);
        ws = ws + __shfl_xor(ws, 32, 64);
        if (live && f.lg == 0) {
            const int64_t o = (int64_t)f.split * p.ns + b;
            p.part_m[o] = term.run_m;
            p.part_l[o] = term.run_l;
            p.part_w[o] = ws;
            p.part_ps[o] = ps;
        }
    } else if constexpr (ROLE == SML_DQ) {
        SmlDqTerm<JAC> term;
        term.inv_temp = inv_temp; term.ct = p.coef * inv_temp; term.set = p.strm_set + f.m_beg; term.mine = mine;
        // (a lane past the last row is never stored; lse = +inf gives it weight 0 instead of exp(S/T), which overflows at low T)
        term.lse_b = live ? p.lse[b] : INFINITY; term.inv_w_b = live ? p.inv_w[b] : 0.f;
        term.pos_t = flash_rel(p.row_offset + b, f);
        flash_stream<KT, NC, true>(term, f, p.stat, p.ns, p.strm, c_first, smem, oacc);
        if (live) flash_store<NC, false>(p.part_o + ((int64_t)f.split * p.ns + b) * D, c_first, f.lg, oacc);
    } else {
        SmlDkTerm<JAC> term;
        term.inv_temp = inv_temp; term.ct = p.coef * inv_temp; term.lse = p.lse + f.m_beg; term.inv_w = p.inv_w + f.m_beg;
        term.set = p.strm_set + f.m_beg; term.mine = mine;
        term.pos_t = flash_rel(b - p.row_offset, f);
        flash_stream<KT, NC, true>(term, f, p.stat, p.ns, p.strm, c_first, smem, oacc);
        if (live) flash_store<NC, false>(p.out + b * D, c_first, f.lg, oacc);
    }
}

// the live splits of a row merged in order: m* = max m_s, l* = sum l_s e^(m_s - m*), W = sum wsum_s, psum = sum psum_s (float32);
// lse = m* + log l*, inv_W = 1 / W, loss_rows = lse - psum inv_W.  One thread per row; the empty splits' slots are not read.
__global__ __launch_bounds__(256) void sml_rows_kernel(const float* part_m, const float* part_l, const float* part_w,
                                                       const float* part_ps, int64_t rows, int ksplit, float* lse, float* inv_w,
                                                       float* loss_rows) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    float mstar = -INFINITY;
    for (int s = 0; s < ksplit; ++s) mstar = fmaxf(mstar, part_m[(int64_t)s * rows + i]);
    float lstar = 0.f, ps = 0.f, w = 0.f;
    for (int s = 0; s < ksplit; ++s) {
        const float ms = part_m[(int64_t)s * rows + i];
        lstar += (ms == -INFINITY) ? 0.f : part_l[(int64_t)s * rows + i] * expf(ms - mstar);
        w += part_w[(int64_t)s * rows + i];
        ps += part_ps[(int64_t)s * rows + i];
    }
    const float l = mstar + logf(lstar), rw = 1.0f / w;
    lse[i] = l;
    inv_w[i] = rw;
    loss_rows[i] = l - ps * rw;
}

// dq_i = sum over the live splits, in order, of their partial Out (coef / T is in the weights); tq[i] = q_i . dq_i.  One wave per row.
__global__ __launch_bounds__(256) void sml_dq_kernel(const unsigned short* q, const float* part_o, int64_t rows, int d, int ksplit,
                                                     float* dq, float* tq) {
    const int lane = lane_id();
    const int64_t i = (int64_t)blockIdx.x * 4 + wave_id();
    if (i >= rows) return;
    const unsigned short* qp = q + i * d;
    float t = 0.f;
    for (int c = lane; c < d; c += 64) {
        float o = 0.f;
        for (int s = 0; s < ksplit; ++s) o += part_o[((int64_t)s * rows + i) * d + c];
        dq[i * d + c] = o;
        t = fmaf(Tr<BF16>::to_f32(qp[c]), o, t);
    }
    t = reduce_wave(t);
    if (lane == 0) tq[i] = t;
}

// multi-hot rows [rows, classes] -> one word per row: one wave per row, lane c reads class c, the ballot of value != 0 is the word
// (classes < 64 leaves the upper lanes false).  KIND: 0 bf16, 1 float32, 2 float16, 3 uint8.
template <int KIND>
__global__ __launch_bounds__(256) void sml_pack_kernel(const void* multi_hot, int64_t rows, int classes, uint64_t* sets) {
    const int lane = lane_id();
    const int64_t i = (int64_t)blockIdx.x * 4 + wave_id();
    if (i >= rows) return;                                        // wave-uniform
    bool member = false;
    if (lane < classes) {
        const int64_t at = i * classes + lane;
        if constexpr (KIND == 1) member = reinterpret_cast<const float*>(multi_hot)[at] != 0.f;
        else if constexpr (KIND == 3) member = reinterpret_cast<const unsigned char*>(multi_hot)[at] != 0;
        else member = (reinterpret_cast<const unsigned short*>(multi_hot)[at] & 0x7fff) != 0;      // +-0 of bf16 / float16
    }
    const uint64_t word = __ballot(member);
    if (lane == 0) sets[i] = word;
}

// the column split of the gradient roles: d = 1024 alone, as in aecf_supcon_flash.hip (SML_CSPLIT_KT: the first KT that splits; a
// build with -DSML_CSPLIT_KT=24 gives the d = 768 variant profiles/supcon_ml_time.txt compares)
#ifndef SML_CSPLIT_KT
#define SML_CSPLIT_KT 32
#endif
template <int KT, int ROLE>
constexpr int sml_csplit() {
    return ROLE != SML_STATS && KT >= SML_CSPLIT_KT ? 2 : 1;
}

template <int KT, int ROLE, bool JAC>
void launch_sml_role(const SmlFlashArgs& a, int blocks, hipStream_t s) {
    constexpr int D = 32 * KT;
    constexpr int CSPLIT = sml_csplit<KT, ROLE>();
    const size_t smem = (size_t)2 * 32 * 2 * D;
    auto kern = sml_flash_kernel<KT, ROLE, CSPLIT, JAC>;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    for (int cpart = 0; cpart < CSPLIT; ++cpart) kern<<<dim3((unsigned)blocks), dim3(256), smem, s>>>(a, cpart);
}

}  // namespace

bool supcon_ml_flash_supported(int d) { return nce_flash_supported(0, d); }

// the layout of supcon_flash_workspace_bytes, the count slot holding the float32 weight sum
size_t supcon_ml_flash_workspace_bytes(int64_t rows, int64_t cols, int d) {
    const int ks = flash_split(rows, cols).rule;
    return ((size_t)ks * rows * (d + 4) + (size_t)3 * rows) * sizeof(float) + 1024;
}

void launch_supcon_ml_flash(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, float coef, const void* q,
                            const void* k, const uint64_t* q_sets, const uint64_t* k_sets, int jaccard, float* loss_rows, float* dq,
                            float* dk, void* workspace, hipStream_t s) {
    const FlashSplit sp = flash_split(rows, cols);
    float* ws = reinterpret_cast<float*>(workspace);
    float* part_o = ws;
    float* part_m = part_o + (size_t)sp.rule * rows * d;
    float* part_l = part_m + (size_t)sp.rule * rows;
    float* part_w = part_l + (size_t)sp.rule * rows;
    float* part_ps = part_w + (size_t)sp.rule * rows;
    float* lse = part_ps + (size_t)sp.rule * rows;
    float* inv_w = lse + rows;
    float* tq = inv_w + rows;
    SmlFlashArgs a;
    a.stat = (const unsigned short*)q; a.strm = (const unsigned short*)k; a.ns = rows; a.nm = cols; a.row_offset = row_offset;
    a.stat_set = q_sets; a.strm_set = k_sets; a.temp = dt.t; a.min_temp = dt.min_t; a.coef = coef;
    a.part_m = part_m; a.part_l = part_l; a.part_w = part_w; a.part_ps = part_ps;
    a.lse = lse; a.inv_w = inv_w; a.part_o = part_o; a.out = nullptr; a.strm_per_split = sp.per;
    SmlFlashArgs b = a;
    b.stat = (const unsigned short*)k; b.strm = (const unsigned short*)q; b.ns = cols; b.nm = rows;
    b.stat_set = k_sets; b.strm_set = q_sets; b.out = dk; b.strm_per_split = rows;
    const int q_blocks = (int)(((rows + 63) / 64) * sp.live), k_blocks = (int)((cols + 63) / 64);
    auto run = [&](auto kt, auto jac) {
        constexpr int KT = decltype(kt)::value;
        constexpr bool JAC = decltype(jac)::value;
        launch_sml_role<KT, SML_STATS, JAC>(a, q_blocks, s);
        sml_rows_kernel<<<dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s>>>(part_m, part_l, part_w, part_ps, rows, sp.live, lse,
                                                                                   inv_w, loss_rows);
        if (!dq) return;
        launch_sml_role<KT, SML_DQ, JAC>(a, q_blocks, s);
        sml_dq_kernel<<<dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s>>>((const unsigned short*)q, part_o, rows, d, sp.live, dq, tq);
        launch_sml_role<KT, SML_DK, JAC>(b, k_blocks, s);
    };
    dispatch_kt(d, [&](auto kt) {
        if (jaccard) run(kt, std::true_type{});
        else run(kt, std::false_type{});
    });
    if (dq && dt.d_t) launch_nce_dtemp(tq, rows, 1, dt, s);
}

void launch_label_sets_pack(int64_t rows, int classes, int kind, const void* multi_hot, uint64_t* sets, hipStream_t s) {
    const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
    switch (kind) {
        case 0: sml_pack_kernel<0><<<grid, block, 0, s>>>(multi_hot, rows, classes, sets); break;
        case 1: sml_pack_kernel<1><<<grid, block, 0, s>>>(multi_hot, rows, classes, sets); break;
        case 2: sml_pack_kernel<2><<<grid, block, 0, s>>>(multi_hot, rows, classes, sets); break;
        default: sml_pack_kernel<3><<<grid, block, 0, s>>>(multi_hot, rows, classes, sets); break;
    }
}

}  // namespace aecf
