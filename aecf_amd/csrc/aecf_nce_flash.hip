// Flash-style InfoNCE, bf16, gfx950: one direction of the contrastive term (aecf_nce_fwd_bwd) without ever materialising
// the [rows, cols] logits -- workspace O(rows d) instead of O(rows cols) (config 3: 8192 x 65536 logits = 2.1 GB float32).
//
//   loss_i = logsumexp_j(q_i.k_j / T) - q_i.k_pos(i) / T                     pos(i) = row_offset + i
//   dq_i   = coef/T (sum_j p_ij k_j - k_pos(i))         p_ij = softmax_j      = "attention output with V = K" - k_pos
//   dk_j   = coef/T (sum_i p_ij q_i - [j = pos(i)] q_i)
//
// One kernel, two roles (template MODE), both the streaming loop of aecf_flash_stream.h (64 stationary rows per block in
// registers, the other matrix streamed through LDS, Out^T += streamed^T P) with this file's terms for P:
//   DQ: P[a, b] = exp(S/T - m_b)                  online maximum m_b / sum l_b per stationary row b; a new maximum rescales Out
//   DK: P[a, b] = coef/T (exp(S/T - lse_a) - [b = pos(a)])      lse_a from the DQ pass
// DQ (stationary = local q, streamed = all keys): the key range is split over the blocks of a row block so that the grid
// fills the chip (flash_split; only the non-empty splits run); each writes its partial (m, l, Out) and a small combine kernel
// merges them, subtracts k_pos, and produces loss_rows and lse.  DK (stationary = keys, streamed = local q): one pass, no
// partials.  No float atomics: results are reproducible.  The entropy regulariser (CurriculumMasking.entropy_loss, ref
// aecf/AECFLayer.py:285-314) rides in the combine launch when asked for, so contrastive + entropy loss and their gradients
// are one call.
#include <math.h>

#include "aecf_flash_stream.h"

namespace aecf {

namespace {

enum { NCE_DQ = 0, NCE_DK = 1, NCE_DQ_DT = 2, NCE_DK_DT = 3 };     // _DT: the temperature is read from the device

struct NceFlashArgs {
    const unsigned short* stat;     // stationary rows [ns, d]   (DQ: q, DK: k)
    const unsigned short* strm;     // streamed rows   [nm, d]   (DQ: k, DK: q)
    int64_t ns, nm;
    int64_t row_offset;             // pos(i) = row_offset + i for local row i
    float inv_temp, coef;
    const float* lse;               // DK: [nm] log-sum-exp of the streamed (local q) rows
    float* part_m;                  // DQ: [KS, ns]
    float* part_l;                  // DQ: [KS, ns]
    float* part_o;                  // DQ: [KS, ns, d]
    float* out;                     // DK: dk [ns, d]
    int64_t strm_per_split;         // DQ: streamed rows per split (a multiple of 32); no launched split is empty
    const float* temp;              // _DT modes: inv_temp = 1 / max(*temp, min_temp)
    float min_temp;
};

// P of the DQ role: online softmax over the streamed keys; run_m / run_l per stationary row b = r16 (replicated over lg)
struct NceDqTerm {
    static constexpr bool FENCED = false;
    float inv_temp;
    float run_m = -INFINITY, run_l = 0.f;
    template <int NC>
    __device__ __forceinline__ void weights(const f32x4& sacc, int a0, int lg, int r16, int len, f32x4 (&oacc)[NC], float (&pv)[4]) {
        float tmax = -INFINITY;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            pv[r] = (a0 + 4 * lg + r < len) ? sacc[r] * inv_temp : -INFINITY;
            tmax = fmaxf(tmax, pv[r]);
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        const float new_m = fmaxf(run_m, tmax);
        if (__any(new_m > run_m)) {                               // wave-uniform: rescale the running sums
            const float sc = (run_m == -INFINITY) ? 0.f : expf(run_m - new_m);
            run_l *= sc;
#pragma unroll
            for (int c = 0; c < NC; ++c)
#pragma unroll
                for (int r = 0; r < 4; ++r) oacc[c][r] *= sc;
            run_m = new_m;
        }
        float ts_ = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) { pv[r] = expf(pv[r] - run_m); ts_ += pv[r]; }
        ts_ += __shfl_xor(ts_, 16, 64);
        ts_ += __shfl_xor(ts_, 32, 64);
        run_l += ts_;
    }
};

// P of the DK role: the softmax weight from the DQ pass's lse, minus one at the positive (pos_t: the streamed local q row
// whose positive is this lane's key, relative to the range; -1: none)
struct NceDkTerm {
    static constexpr bool FENCED = false;
    float inv_temp, ct;
    const float* lse;               // of the range's first streamed row
    int pos_t;
    template <int NC>
    __device__ __forceinline__ void weights(const f32x4& sacc, int a0, int lg, int r16, int len, f32x4 (&oacc)[NC], float (&pv)[4]) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int a = a0 + 4 * lg + r;                        // local q row
            float v = 0.f;
            if (a < len) {
                v = expf(sacc[r] * inv_temp - lse[a]);
                if (a == pos_t) v -= 1.0f;
                v *= ct;
            }
            pv[r] = v;
        }
    }
};

// CSPLIT > 1: the output columns are produced in CSPLIT launches of D / CSPLIT columns each (cpart = which), every one
// recomputing S -- the 16 x D float32 accumulator of a wave plus the stationary fragments exceed the register file of a
// wave beyond D = 512 (DQ, whose rescaling touches the accumulator with vector instructions) / D = 768 (DK).
template <int KT, int MODE_, int CSPLIT>
__global__ __launch_bounds__(256, 1) void nce_flash_kernel(NceFlashArgs p, int cpart) {
    constexpr int MODE = MODE_ & 1;
    if (MODE_ >= NCE_DQ_DT) p.inv_temp = nce_dev_inv_temp(p.temp, p.min_temp);
    constexpr int D = 32 * KT, NC = D / 16 / CSPLIT;
    const int c_first = cpart * NC;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const FlashBlock f = flash_block<MODE == NCE_DQ>(p.ns, p.nm, p.strm_per_split);
    const int64_t b = f.s0 + f.r16;                               // lane (lg, r16) ends with Out[b][16 c + 4 lg + r]
    f32x4 oacc[NC];
    if (MODE == NCE_DQ) {
        NceDqTerm term;
        term.inv_temp = p.inv_temp;
        flash_stream<KT, NC, true>(term, f, p.stat, p.ns, p.strm, c_first, smem, oacc);
        if (b < p.ns) {
            flash_store<NC, false>(p.part_o + ((int64_t)f.split * p.ns + b) * D, c_first, f.lg, oacc);
            if (f.lg == 0 && cpart == 0) {
                p.part_m[(int64_t)f.split * p.ns + b] = term.run_m;
                p.part_l[(int64_t)f.split * p.ns + b] = term.run_l;
            }
        }
    } else {
        NceDkTerm term;
        term.inv_temp = p.inv_temp; term.ct = p.coef * p.inv_temp; term.lse = p.lse + f.m_beg;
        term.pos_t = flash_rel(b - p.row_offset, f);
        flash_stream<KT, NC, true>(term, f, p.stat, p.ns, p.strm, c_first, smem, oacc);
        if (b < p.ns) flash_store<NC, false>(p.out + b * D, c_first, f.lg, oacc);
    }
}

// merge the key splits of a row: m* = max m_s, l* = sum l_s e^(m_s - m*), O* = sum O_s e^(m_s - m*);
// dq = coef/T (O*/l* - k_pos), lse = m* + log l*, loss = lse - q.k_pos/T.  One wave per row.
// Block 0 additionally reduces the entropy regulariser (optional): loss_e = mean((H - target)^2), d_entropy.
struct NceCombineArgs {
    const unsigned short* q;
    const unsigned short* k;
    const float* part_m;
    const float* part_l;
    const float* part_o;
    float* dq;
    float* loss_rows;
    float* lse;
    int64_t rows, row_offset;
    int d, ksplit;
    float inv_temp, coef;
    // entropy regulariser riding in this launch (n_ent == 0: off)
    const float* ent;
    float* d_ent;
    float* ent_loss;
    int64_t n_ent;
    float ent_target, ent_scale;
    // device temperature (DT): inv_temp = 1 / max(*temp, min_temp); with tdot, the wave of row i writes
    // q_i.dq_i to part_l[i] once it has read that row's partials (nothing reads part_l after this launch)
    const float* temp;
    float min_temp;
    int tdot;
};

template <bool DT>
__global__ __launch_bounds__(256) void nce_combine_kernel(NceCombineArgs p) {
    if (DT) p.inv_temp = nce_dev_inv_temp(p.temp, p.min_temp);
    const int lane = lane_id();
    const int64_t i = (int64_t)blockIdx.x * 4 + wave_id();
    if (i < p.rows) {
        float mstar = -INFINITY;
        for (int s = 0; s < p.ksplit; ++s) mstar = fmaxf(mstar, p.part_m[(int64_t)s * p.rows + i]);
        float lstar = 0.f;
        for (int s = 0; s < p.ksplit; ++s) {
            const float ms = p.part_m[(int64_t)s * p.rows + i];
            lstar += (ms == -INFINITY) ? 0.f : p.part_l[(int64_t)s * p.rows + i] * expf(ms - mstar);
        }
        const unsigned short* kp = p.k + (p.row_offset + i) * p.d;
        const unsigned short* qp = p.q + i * p.d;
        const float ct = p.coef * p.inv_temp, inv_l = 1.0f / lstar;
        float dot = 0.f, tq = 0.f;
        for (int c = lane; c < p.d; c += 64) {
            float o = 0.f;
            for (int s = 0; s < p.ksplit; ++s) {
                const float ms = p.part_m[(int64_t)s * p.rows + i];
                if (ms != -INFINITY) o += p.part_o[((int64_t)s * p.rows + i) * p.d + c] * expf(ms - mstar);
            }
            const float kv = Tr<BF16>::to_f32(kp[c]);
            const float g = ct * (o * inv_l - kv);
            p.dq[i * p.d + c] = g;
            dot = fmaf(Tr<BF16>::to_f32(qp[c]), kv, dot);
            if (DT) tq = fmaf(Tr<BF16>::to_f32(qp[c]), g, tq);
        }
        dot = reduce_wave(dot);
        if (lane == 0) {
            const float lse = mstar + logf(lstar);
            p.lse[i] = lse;
            p.loss_rows[i] = lse - dot * p.inv_temp;
        }
        if (DT && p.tdot) {
            tq = reduce_wave(tq);
            if (lane == 0) const_cast<float*>(p.part_l)[i] = tq;
        }
    }
    if (blockIdx.x == 0 && p.n_ent > 0)                           // entropy regulariser: one block, fixed order
        entropy_rider(p.ent, p.n_ent, p.ent_target, p.ent_scale, p.d_ent, p.ent_loss);
}

template <int KT, int MODE>
void launch_flash_mode(const NceFlashArgs& a, int blocks, hipStream_t s) {
    constexpr int D = 32 * KT;
    constexpr int CSPLIT = ((MODE & 1) == NCE_DQ ? (KT >= 32 ? 4 : (KT >= 24 ? 2 : 1)) : (KT >= 32 ? 2 : 1));
    const size_t smem = (size_t)2 * 32 * 2 * D;
    auto kern = nce_flash_kernel<KT, MODE, CSPLIT>;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    for (int cpart = 0; cpart < CSPLIT; ++cpart) kern<<<dim3((unsigned)blocks), dim3(256), smem, s>>>(a, cpart);
}

}  // namespace

bool nce_flash_supported(int dtype, int d) {
    return dtype == 0 && (d == 128 || d == 256 || d == 384 || d == 512 || d == 768 || d == 1024);
}

// the partials are laid out for the split rule's count (the public workspace size); the empty splits' slots stay unused
size_t nce_flash_workspace_bytes(int64_t rows, int64_t cols, int d) {
    const int ks = flash_split(rows, cols).rule;
    return ((size_t)ks * rows * (d + 2) + (size_t)rows) * sizeof(float) + 1024;
}

void launch_nce_flash(int64_t rows, int64_t cols, int64_t row_offset, int d, float inv_temp, float coef, const void* q,
                      const void* k, float* loss_rows, float* dq, float* dk, void* workspace, const float* ent, int64_t n_ent,
                      float ent_target, float ent_upstream, float* d_ent, float* ent_loss, hipStream_t s,
                      const NceDevTemp* dt) {
    const FlashSplit sp = flash_split(rows, cols);
    float* ws = reinterpret_cast<float*>(workspace);
    float* part_m = ws;
    float* part_l = part_m + (size_t)sp.rule * rows;
    float* part_o = part_l + (size_t)sp.rule * rows;
    float* lse = part_o + (size_t)sp.rule * rows * d;
    NceFlashArgs a;
    a.stat = (const unsigned short*)q; a.strm = (const unsigned short*)k; a.ns = rows; a.nm = cols; a.row_offset = row_offset;
    a.inv_temp = inv_temp; a.coef = coef; a.lse = nullptr; a.part_m = part_m; a.part_l = part_l; a.part_o = part_o;
    a.out = nullptr; a.strm_per_split = sp.per;
    NceFlashArgs b = a;
    b.stat = (const unsigned short*)k; b.strm = (const unsigned short*)q; b.ns = cols; b.nm = rows; b.lse = lse; b.out = dk;
    b.strm_per_split = rows;
    NceCombineArgs c;
    c.q = (const unsigned short*)q; c.k = (const unsigned short*)k; c.part_m = part_m; c.part_l = part_l; c.part_o = part_o;
    c.dq = dq; c.loss_rows = loss_rows; c.lse = lse; c.rows = rows; c.row_offset = row_offset; c.d = d; c.ksplit = sp.live;
    c.inv_temp = inv_temp; c.coef = coef; c.ent = ent; c.d_ent = d_ent; c.ent_loss = ent_loss; c.n_ent = ent ? n_ent : 0;
    c.ent_target = ent_target; c.ent_scale = n_ent > 0 ? 2.0f * ent_upstream / (float)n_ent : 0.f;
    // device temperature: the _DT instances; the temperature gradient from the float32 dq of the combine launch
    a.temp = b.temp = c.temp = dt ? dt->t : nullptr; a.min_temp = b.min_temp = c.min_temp = dt ? dt->min_t : 0.f;
    c.tdot = dt && dt->d_t;
    const int dq_blocks = (int)(((rows + 63) / 64) * sp.live), dk_blocks = (int)((cols + 63) / 64);
    const auto run = [&](auto dev_temp) {
        constexpr bool DT = decltype(dev_temp)::value;
        dispatch_kt(d, [&](auto kt) {
            constexpr int KT = decltype(kt)::value;
            launch_flash_mode<KT, DT ? NCE_DQ_DT : NCE_DQ>(a, dq_blocks, s);
            nce_combine_kernel<DT><<<dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s>>>(c);
            launch_flash_mode<KT, DT ? NCE_DK_DT : NCE_DK>(b, dk_blocks, s);
        });
    };
    if (dt) run(std::true_type{});
    else run(std::false_type{});
    if (dt && dt->d_t) launch_nce_dtemp(part_l, rows, 1, *dt, s);
}

}  // namespace aecf
