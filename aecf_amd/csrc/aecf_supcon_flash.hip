// Streaming supervised contrastive loss (Khosla et al. 2020, the "L_out" form), bf16, gfx950 (aecf_supcon_fwd_bwd): one
// direction of the label-aware contrastive term without the [rows, cols] logits and without a [rows, cols] match mask.
//
//   match(i, j) = (j == row_offset + i) or (lq[i] >= 0 and lq[i] == lk[j])        64-bit compare; a negative label = unlabeled
//   n_i    = sum_j match(i, j)  (>= 1: the partner counts by index)     x_ij = q_i.k_j / T     lse_i = logsumexp_j x_ij
//   loss_i = lse_i - (1 / n_i) sum_j match(i, j) x_ij                   G = softmax_j - match / n_i
//   dq = coef/T G k          dk = coef/T G^T q          dT = -(1/Tc) sum_i q_i . dq_i
//
// Three roles of the streaming loop of aecf_flash_stream.h (64 stationary rows per block in registers, the other matrix streamed
// through LDS, Out^T += streamed^T P), each with a term of this file.  The label of a streamed row is loaded inside weights(), as
// NceDkTerm loads lse[a]; the compare needs no pass of its own over the embeddings.
//   STATS (stationary = local q, streamed = keys, no second product): online maximum m_b / sum l_b per stationary row b, and per
//          lane an integer count of its matches and the float32 sum of their x.  The key range is split over the blocks of a row
//          block (flash_split); each live split writes (m, l, count, psum) and sup_rows_kernel merges them in order into lse,
//          inv_n = 1 / n and loss_rows.
//   DQ    (same stationary / streamed rows, same split): P[a, b] = ct (exp(S/T - lse_b) - match(b, a) inv_n_b), ct = coef / T.  The
//          normaliser is known, so nothing rescales the accumulator; each live split writes its partial Out and sup_dq_kernel adds
//          the splits in order into the float32 dq and leaves tq_i = q_i . dq_i for launch_nce_dtemp.
//   DK    (stationary = keys, streamed = local q): the same weight with lse, inv_n and lq loaded per streamed row; one pass, no
//          partials, float32 dk.
// A weight is rounded to bf16 once, as the B operand of the second product (the loop's pack_bf16x2).  No float atomics: the same
// inputs give the same bits.  The temperature is always a device scalar.
//
// Registers (profiles/supcon_resources.txt): the DQ and DK roles carry the labels of a sub-tile's four streamed rows (8 registers)
// and a few scalars beside what the no-rescale roles of the other forms hold, and still fit where InfoNCE's DK role fits: the
// output columns come from one launch up to d = 768 (252 / 254 VGPRs + 196 AGPRs there) and from two at d = 1024 (CSPLIT, S
// formed in each), every instance free of scratch.
//
// The pooled forms (aecf_supcon_pool_fwd_bwd: NT-Xent, the supervised contrastive loss over both views).  The keys are one pool
// that holds the anchors themselves, and key self_offset + i is EXCLUDED for local row i: the three roles have a compile-time
// SELF variant (sup_pool_kernel; sup_flash_kernel is the body with SELF = false, its instances and their bits as before).
//   match(i, j) = j != self_offset + i and ((j == row_offset + i) or (lq[i] >= 0 and lq[i] == lk[j]))
//   lse_i, the softmax and G run over j != self_offset + i; dk[self_offset + i] gets nothing from row i
// The exclusion comes before the label compare -- in real use the excluded key IS the anchor: it carries the anchor's label and
// the highest score there is, 1/T.  STATS gives it x = -inf (nothing for m, l, the count or the sum of the matched x), DQ and DK
// give it weight 0 (a select, not a product: its exponential may overflow); in DK the test is "streamed row a == stationary key
// b - self_offset", the mirror of pos_t.
// An all -inf sub-tile: with an exclusion a sub-tile, or a whole split, can hold one valid key that is excluded for a row (the
// split rule cuts where it likes), so that row reaches the sum with tmax = -inf while run_m is still -inf, and exp(pv - run_m)
// would be exp(-inf + inf) = NaN.  SELF shifts by 0 instead of run_m in that state: every term is exp(-inf) = 0, and a split that
// never sees another key leaves (m = -inf, l = 0, count = 0, psum = 0), which sup_rows_kernel merges as nothing.  Some split holds
// the partner (self_offset != row_offset), so the merged maximum is finite and n >= 1.
// Registers (profiles/supcon_pool_resources.txt): one more per-lane index; the gradient roles at d = 768 / 1024 go from 252 - 255
// to 251 - 256 VGPRs, no scratch, the same CSPLIT.
#include <math.h>

#include "aecf_flash_stream.h"

namespace aecf {

namespace {

enum { SUP_STATS = 0, SUP_DQ = 1, SUP_DK = 2 };

struct SupFlashArgs {
    const unsigned short* stat;     // stationary rows [ns, d]   (STATS, DQ: q; DK: k)
    const unsigned short* strm;     // streamed rows   [nm, d]   (STATS, DQ: k; DK: q)
    int64_t ns, nm;
    int64_t row_offset;             // the partner of local row i is key row_offset + i
    const int64_t* stat_lab;        // labels of the stationary rows [ns]
    const int64_t* strm_lab;        // labels of the streamed rows   [nm]
    const float* temp;              // device scalar: inv_temp = 1 / max(*temp, min_temp)
    float min_temp, coef;
    float* part_m;                  // STATS: [KS, ns] each
    float* part_l;
    int* part_cnt;
    float* part_ps;
    const float* lse;               // DQ, DK: [rows] of the local q rows
    const float* inv_n;
    float* part_o;                  // DQ: [KS, ns, d]
    float* out;                     // DK: dk [ns, d]
    int64_t strm_per_split;         // STATS, DQ: streamed rows per split (a multiple of 32); no launched split is empty
};

// the label of a streamed row equals that of the lane's stationary row: STATS / DQ compare the query's label `mine` (unlabeled: no
// match) with the key's, DK the key's label `mine` with the query's (unlabeled: no match)
template <bool MINE_IS_QUERY>
__device__ __forceinline__ bool sup_same(int64_t mine, int64_t other) {
    return (MINE_IS_QUERY ? mine : other) >= 0 && mine == other;
}

// S / T rounded to float32 as the STATS role stores it (its x enters a maximum), never fused into the subtraction of lse: the SELF
// gradient roles form their exponent from it, so a row whose only key is its partner has x - lse = 0 and a weight of exactly 0.
// (The instances without an exclusion keep their contracted form and their bits.)
template <bool SELF>
__device__ __forceinline__ float sup_scaled(float s, float inv_temp) {
    if constexpr (SELF) {
#pragma clang fp contract(off)
        return s * inv_temp;
    } else {
        return s * inv_temp;
    }
}

// STATS: online softmax statistics of stationary row b = r16 (replicated over lg) and this lane's share of its matches
template <bool SELF>
struct SupStatsTerm {
    static constexpr bool FENCED = false;
    float inv_temp;
    const int64_t* lab;             // of the range's first streamed row
    int64_t mine;
    int pos_t, self_t;
    float run_m = -INFINITY, run_l = 0.f, psum = 0.f;
    int count = 0;
    template <int NC>
    __device__ __forceinline__ void weights(const f32x4& sacc, int a0, int lg, int r16, int len, f32x4 (&oacc)[NC], float (&pv)[4]) {
        float tmax = -INFINITY;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int a = a0 + 4 * lg + r;
            float x = -INFINITY;
            if (a < len && !(SELF && a == self_t)) {              // the excluded key: x = -inf, never a positive
                x = sacc[r] * inv_temp;
                if (a == pos_t || sup_same<true>(mine, lab[a])) {
                    psum += x;
                    count += 1;
                }
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
        // SELF: a row whose only valid keys so far were its excluded one still has run_m = -inf; every pv is -inf then, and
        // exp(-inf - 0) = 0 where exp(-inf + inf) is NaN.  (Without an exclusion the first sub-tile has a finite maximum.)
        const float shift = SELF && run_m == -INFINITY ? 0.f : run_m;
        float ts_ = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) ts_ += expf(pv[r] - shift);
        ts_ += __shfl_xor(ts_, 16, 64);
        ts_ += __shfl_xor(ts_, 32, 64);
        run_l += ts_;
    }
};

// DQ: the weight of key a for the lane's query b from that query's lse and 1 / n
template <bool SELF>
struct SupDqTerm {
    static constexpr bool FENCED = false;
    float inv_temp, ct, lse_b, inv_n_b;
    const int64_t* lab;             // key labels, of the range's first streamed row
    int64_t mine;
    int pos_t, self_t;
    template <int NC>
    __device__ __forceinline__ void weights(const f32x4& sacc, int a0, int lg, int r16, int len, f32x4 (&oacc)[NC], float (&pv)[4]) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int a = a0 + 4 * lg + r;                        // key
            float v = 0.f;
            if (a < len && !(SELF && a == self_t)) {              // the excluded key: weight 0 (its exp may overflow)
                v = expf(sup_scaled<SELF>(sacc[r], inv_temp) - lse_b);
                if (a == pos_t || sup_same<true>(mine, lab[a])) v -= inv_n_b;
                v *= ct;
            }
            pv[r] = v;
        }
    }
};

// DK: the same weight for the lane's key b and local query a: lse, 1 / n and the label are the streamed row's
template <bool SELF>
struct SupDkTerm {
    static constexpr bool FENCED = false;
    float inv_temp, ct;
    const float* lse;               // of the range's first streamed row, as inv_n and lab
    const float* inv_n;
    const int64_t* lab;
    int64_t mine;
    int pos_t, self_t;
    template <int NC>
    __device__ __forceinline__ void weights(const f32x4& sacc, int a0, int lg, int r16, int len, f32x4 (&oacc)[NC], float (&pv)[4]) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int a = a0 + 4 * lg + r;                        // local q row
            float v = 0.f;
            if (a < len && !(SELF && a == self_t)) {              // the query this key is excluded for: weight 0
                v = expf(sup_scaled<SELF>(sacc[r], inv_temp) - lse[a]);
                if (a == pos_t || sup_same<false>(mine, lab[a])) v -= inv_n[a];
                v *= ct;
            }
            pv[r] = v;
        }
    }
};

// CSPLIT > 1: the output columns come from CSPLIT launches of D / CSPLIT columns each (cpart = which), every one forming S
template <int KT, int ROLE, int CSPLIT, bool SELF>
__device__ __forceinline__ void sup_flash_body(const SupFlashArgs& p, int cpart, int64_t self_offset) {
    constexpr int D = 32 * KT, NC = ROLE == SUP_STATS ? 1 : D / 16 / CSPLIT;
    const float inv_temp = nce_dev_inv_temp(p.temp, p.min_temp);
    const int c_first = cpart * NC;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const FlashBlock f = flash_block<ROLE != SUP_DK>(p.ns, p.nm, p.strm_per_split);
    const int64_t b = f.s0 + f.r16;                               // lane (lg, r16) ends with Out[b][16 c + 4 lg + r]
    const bool live = b < p.ns;
    const int64_t mine = live ? p.stat_lab[b] : (int64_t)-1;
    f32x4 oacc[NC];
    if constexpr (ROLE == SUP_STATS) {
        SupStatsTerm<SELF> term;
        term.inv_temp = inv_temp; term.lab = p.strm_lab + f.m_beg; term.mine = mine;
        term.pos_t = flash_rel(p.row_offset + b, f);
        if constexpr (SELF) term.self_t = flash_rel(self_offset + b, f);
        flash_stream<KT, 1, false>(term, f, p.stat, p.ns, p.strm, 0, smem, oacc);
        float ps = term.psum;                                     // a lane holds a quarter of row b's matches
        int cnt = term.count;
        ps = ps + __shfl_xor(ps, 16, 64);
        ps = ps + __shfl_xor(ps, 32, 64);
        cnt = cnt + __shfl_xor(cnt, 16, 64);
        cnt = cnt + __shfl_xor(cnt, 32, 64);
        if (live && f.lg == 0) {
            const int64_t o = (int64_t)f.split * p.ns + b;
            p.part_m[o] = term.run_m;
            p.part_l[o] = term.run_l;
            p.part_cnt[o] = cnt;
            p.part_ps[o] = ps;
        }
    } else if constexpr (ROLE == SUP_DQ) {
        SupDqTerm<SELF> term;
        term.inv_temp = inv_temp; term.ct = p.coef * inv_temp; term.lab = p.strm_lab + f.m_beg; term.mine = mine;
        // (a lane past the last row is never stored; lse = +inf gives it weight 0 instead of exp(S/T), which overflows at low T)
        term.lse_b = live ? p.lse[b] : INFINITY; term.inv_n_b = live ? p.inv_n[b] : 0.f;
        term.pos_t = flash_rel(p.row_offset + b, f);
        if constexpr (SELF) term.self_t = flash_rel(self_offset + b, f);
        flash_stream<KT, NC, true>(term, f, p.stat, p.ns, p.strm, c_first, smem, oacc);
        if (live) flash_store<NC, false>(p.part_o + ((int64_t)f.split * p.ns + b) * D, c_first, f.lg, oacc);
    } else {
        SupDkTerm<SELF> term;
        term.inv_temp = inv_temp; term.ct = p.coef * inv_temp; term.lse = p.lse + f.m_beg; term.inv_n = p.inv_n + f.m_beg;
        term.lab = p.strm_lab + f.m_beg; term.mine = mine;
        term.pos_t = flash_rel(b - p.row_offset, f);
        if constexpr (SELF) term.self_t = flash_rel(b - self_offset, f);
        flash_stream<KT, NC, true>(term, f, p.stat, p.ns, p.strm, c_first, smem, oacc);
        if (live) flash_store<NC, false>(p.out + b * D, c_first, f.lg, oacc);
    }
}

template <int KT, int ROLE, int CSPLIT>
__global__ __launch_bounds__(256, 1) void sup_flash_kernel(SupFlashArgs p, int cpart) {
    sup_flash_body<KT, ROLE, CSPLIT, false>(p, cpart, 0);
}

// the pooled form (aecf_supcon_pool_fwd_bwd): key self_offset + i is excluded for local row i (an argument of its own: the
// argument block of the instances above stays what it was)
template <int KT, int ROLE, int CSPLIT>
__global__ __launch_bounds__(256, 1) void sup_pool_kernel(SupFlashArgs p, int cpart, int64_t self_offset) {
    sup_flash_body<KT, ROLE, CSPLIT, true>(p, cpart, self_offset);
}

// the live splits of a row merged in order: m* = max m_s, l* = sum l_s e^(m_s - m*), n = sum count_s, psum = sum psum_s;
// lse = m* + log l*, inv_n = 1 / n, loss_rows = lse - psum inv_n.  One thread per row; the empty splits' slots are not read.
__global__ __launch_bounds__(256) void sup_rows_kernel(const float* part_m, const float* part_l, const int* part_cnt,
                                                       const float* part_ps, int64_t rows, int ksplit, float* lse, float* inv_n,
                                                       float* loss_rows) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    float mstar = -INFINITY;
    for (int s = 0; s < ksplit; ++s) mstar = fmaxf(mstar, part_m[(int64_t)s * rows + i]);
    float lstar = 0.f, ps = 0.f;
    int cnt = 0;
    for (int s = 0; s < ksplit; ++s) {
        const float ms = part_m[(int64_t)s * rows + i];
        lstar += (ms == -INFINITY) ? 0.f : part_l[(int64_t)s * rows + i] * expf(ms - mstar);
        cnt += part_cnt[(int64_t)s * rows + i];
        ps += part_ps[(int64_t)s * rows + i];
    }
    const float l = mstar + logf(lstar), rn = 1.0f / (float)cnt;
    lse[i] = l;
    inv_n[i] = rn;
    loss_rows[i] = l - ps * rn;
}

// dq_i = sum over the live splits, in order, of their partial Out (coef / T is in the weights); tq[i] = q_i . dq_i.  One wave per row.
__global__ __launch_bounds__(256) void sup_dq_kernel(const unsigned short* q, const float* part_o, int64_t rows, int d, int ksplit,
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

template <int KT, int ROLE, bool SELF>
void launch_sup_role(const SupFlashArgs& a, int64_t self_offset, int blocks, hipStream_t s) {
    constexpr int D = 32 * KT;
    constexpr int CSPLIT = ROLE != SUP_STATS && KT >= 32 ? 2 : 1;
    const size_t smem = (size_t)2 * 32 * 2 * D;
    if constexpr (SELF) {
        auto kern = sup_pool_kernel<KT, ROLE, CSPLIT>;
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        for (int cpart = 0; cpart < CSPLIT; ++cpart) kern<<<dim3((unsigned)blocks), dim3(256), smem, s>>>(a, cpart, self_offset);
    } else {
        auto kern = sup_flash_kernel<KT, ROLE, CSPLIT>;
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        for (int cpart = 0; cpart < CSPLIT; ++cpart) kern<<<dim3((unsigned)blocks), dim3(256), smem, s>>>(a, cpart);
    }
}

}  // namespace

bool supcon_flash_supported(int d) { return nce_flash_supported(0, d); }

// [KS, rows, d] dq partials (16-byte aligned rows) | [KS, rows] m | l | count | psum | [rows] lse | inv_n | q.dq, KS = the split
// rule's count; the empty splits' slots stay unused
size_t supcon_flash_workspace_bytes(int64_t rows, int64_t cols, int d) {
    const int ks = flash_split(rows, cols).rule;
    return ((size_t)ks * rows * (d + 4) + (size_t)3 * rows) * sizeof(float) + 1024;
}

namespace {

template <bool SELF>
void launch_sup_passes(int64_t rows, int64_t cols, int64_t row_offset, int64_t self_offset, int d, const NceDevTemp& dt, float coef,
                       const void* q, const void* k, const int64_t* q_labels, const int64_t* k_labels, float* loss_rows, float* dq,
                       float* dk, void* workspace, hipStream_t s) {
    const FlashSplit sp = flash_split(rows, cols);
    float* ws = reinterpret_cast<float*>(workspace);
    float* part_o = ws;
    float* part_m = part_o + (size_t)sp.rule * rows * d;
    float* part_l = part_m + (size_t)sp.rule * rows;
    float* part_cnt = part_l + (size_t)sp.rule * rows;
    float* part_ps = part_cnt + (size_t)sp.rule * rows;
    float* lse = part_ps + (size_t)sp.rule * rows;
    float* inv_n = lse + rows;
    float* tq = inv_n + rows;
    SupFlashArgs a;
    a.stat = (const unsigned short*)q; a.strm = (const unsigned short*)k; a.ns = rows; a.nm = cols; a.row_offset = row_offset;
    a.stat_lab = q_labels; a.strm_lab = k_labels; a.temp = dt.t; a.min_temp = dt.min_t; a.coef = coef;
    a.part_m = part_m; a.part_l = part_l; a.part_cnt = reinterpret_cast<int*>(part_cnt); a.part_ps = part_ps;
    a.lse = lse; a.inv_n = inv_n; a.part_o = part_o; a.out = nullptr; a.strm_per_split = sp.per;
    SupFlashArgs b = a;
    b.stat = (const unsigned short*)k; b.strm = (const unsigned short*)q; b.ns = cols; b.nm = rows;
    b.stat_lab = k_labels; b.strm_lab = q_labels; b.out = dk; b.strm_per_split = rows;
    const int q_blocks = (int)(((rows + 63) / 64) * sp.live), k_blocks = (int)((cols + 63) / 64);
    dispatch_kt(d, [&](auto kt) {
        constexpr int KT = decltype(kt)::value;
        launch_sup_role<KT, SUP_STATS, SELF>(a, self_offset, q_blocks, s);
        sup_rows_kernel<<<dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s>>>(part_m, part_l, a.part_cnt, part_ps, rows, sp.live,
                                                                                   lse, inv_n, loss_rows);
        if (!dq) return;
        launch_sup_role<KT, SUP_DQ, SELF>(a, self_offset, q_blocks, s);
        sup_dq_kernel<<<dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s>>>((const unsigned short*)q, part_o, rows, d, sp.live, dq, tq);
        launch_sup_role<KT, SUP_DK, SELF>(b, self_offset, k_blocks, s);
    });
    if (dq && dt.d_t) launch_nce_dtemp(tq, rows, 1, dt, s);
}

}  // namespace

void launch_supcon_flash(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, float coef, const void* q,
                         const void* k, const int64_t* q_labels, const int64_t* k_labels, float* loss_rows, float* dq, float* dk,
                         void* workspace, hipStream_t s) {
    launch_sup_passes<false>(rows, cols, row_offset, 0, d, dt, coef, q, k, q_labels, k_labels, loss_rows, dq, dk, workspace, s);
}

void launch_supcon_pool_flash(int64_t rows, int64_t cols, int64_t row_offset, int64_t self_offset, int d, const NceDevTemp& dt,
                              float coef, const void* q, const void* k, const int64_t* q_labels, const int64_t* k_labels,
                              float* loss_rows, float* dq, float* dk, void* workspace, hipStream_t s) {
    launch_sup_passes<true>(rows, cols, row_offset, self_offset, d, dt, coef, q, k, q_labels, k_labels, loss_rows, dq, dk, workspace, s);
}

}  // namespace aecf
