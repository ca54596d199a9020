// Fused classifier head, bf16, gfx950 (aecf_mlhead_forward / _backward): the multi-label classification loss of
// logits = h W^T + bias and all three gradients without the [n, C] block of logits and without its gradient -- workspace
// O((n + C) K) instead of O(n C) (65536 x 4096: 1 GiB of bf16 logits and dlogits that exist only to be consumed elementwise).
//
//   z_ic = h_i . w_c + bias_c        l_ic, g_ic = dl/dz: the element of aecf_mlloss_elem.h at (z_ic, t_ic, pos_scale_c, neg_scale_c)
//   dh_i = scale sum_c g_ic w_c      dW_c = scale sum_i g_ic h_i      dbias_c = scale sum_i g_ic
//
// Both roles are the streaming loop of aecf_flash_stream.h (64 stationary rows per block in registers, the other matrix streamed
// through LDS, Out^T[k, t] += streamed^T[k, s] g[s, t]) with this file's term: z from S and the bias in one rounded float32 add
// after the MFMA chain (no bias: no add), never rounded to bf16; the target read from the label matrix by load_targets' rules;
// g unscaled, rounded to bf16 as the B operand of the second product and nowhere else.  Unknown targets, streamed rows past the
// range (copies of the last valid one) and stationary rows past the matrix give g = 0 and an uncounted loss of 0 by select.
// The targets of a sub-tile are loaded while the sub-tile before it is worked on (raw bits, decoded where they are used).
// CLS (stationary = rows of W, i.e. classes; streamed = rows of h): the rows are split over the blocks of a class block
//     (flash_split(C, n)); every split writes, per class, its float64 loss sum (the four lanes of a class hold float32 sums
//     over the rows they own and are joined in float64), int32 valid count, float32 sum of the unrounded g and its partial
//     dW row (float32, unscaled); head_cls_combine_kernel adds the splits in order, head_totals_kernel the classes.
//     PRODUCT = false is the loss-only pass: the same term without g and without the second product.
// ROW (stationary = rows of h; streamed = rows of W): the classes are split the same way (flash_split(n, C)); one split stores
//     dh from its epilogue, more write partial rows that head_row_combine_kernel adds in order; either way the scale meets the
//     float32 sum and the result is rounded once.
// No atomics anywhere: the same bits on every run.  GENERAL = false is the instance of the plain cross-entropy (gamma_pos =
// gamma_neg = margin = 0 known at compile time): the same element code without the powers and logarithms of the other forms.
// Registers (profiles/mlhead_resources.txt): the element is heavier than the sigmoid loss's, so the output columns of a role
// come from CSPLIT launches (S recomputed) where one would spill; no instance uses scratch.
#include <math.h>

#include "aecf_flash_stream.h"
#include "aecf_mlloss_elem.h"

namespace aecf {

namespace {

enum { HEAD_CLS = 0, HEAD_ROW = 1 };

struct HeadArgs {
    const unsigned short* stat;     // stationary rows [ns, K]   (CLS: W, ROW: h)
    const unsigned short* strm;     // streamed rows   [nm, K]   (CLS: h, ROW: W)
    int64_t ns, nm;
    int64_t classes;                // the pitch of the label matrix [n, classes]
    const void* labels;
    int lkind;
    const float* bias;              // [classes] or NULL
    const float* pos_scale;
    const float* neg_scale;
    MllArgs form;
    double* part_loss;              // CLS: [KS, classes]
    int* part_cnt;                  // CLS: [KS, classes]
    float* part_g;                  // CLS: [KS, classes]
    float* part_o;                  // CLS: [KS, classes, K]; ROW: [KS, n, K] (unscaled)
    int64_t strm_per_split;         // streamed rows per split (a multiple of 32); no split is empty
    const double* totals;           // ROW with one split: the scale and the output
    const float* grad_out;
    float factor;
    int mean;
    void* dh;
    int dh_f32;
    int direct;
};

// scale of the gradients: upstream * factor, over N for the mean (0 where N == 0) -- mll_bwd_kernel's
__device__ __forceinline__ float head_scale(const double* totals, const float* grad_out, float factor, int mean) {
    const float up = (grad_out ? grad_out[0] : 1.0f) * factor;
    if (!mean) return up;
    const double N = totals[1];
    return N > 0.0 ? (float)((double)up / N) : 0.0f;
}

// The term.  CLS: lane (lg, r16) owns class s0 + r16 and meets rows m_beg + a; ROW: it owns row s0 + r16 and meets classes
// m_beg + a.  fixed = the part of the label index that the lane keeps: CLS the (clamped) class, ROW the (clamped) row times C.
template <int ROLE, bool GRAD, bool SUMS, bool GENERAL>
struct HeadTerm {
    static constexpr bool FENCED = true;
    const void* labels;
    int lkind;
    int64_t C, fixed, m_beg;
    int len, lg;
    bool stat_ok;                   // the stationary row exists
    const float *bias, *ps, *ns;
    float bias_c, a_c, b_c;         // CLS: the class's constants
    MllArgs form;
    unsigned raw[4];                // the next sub-tile's targets as loaded
    float nb[4], na[4], nn[4];      // ROW: the next sub-tile's bias and scales
    float sum_l = 0.f, sum_g = 0.f;
    int cnt = 0;

    __device__ __forceinline__ unsigned load_raw(int64_t idx) const {
        if (lkind == 1) return reinterpret_cast<const unsigned*>(labels)[idx];
        if (lkind == 0 || lkind == 2) return reinterpret_cast<const unsigned short*>(labels)[idx];
        return reinterpret_cast<const unsigned char*>(labels)[idx];
    }
    // the loads of sub-tile a0 (streamed indices clamped into the range: every address is inside the matrices)
    __device__ __forceinline__ void prefetch(int a0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            int a = a0 + 4 * lg + r;
            a = a < len ? a : len - 1;
            const int64_t m = m_beg + a;
            raw[r] = load_raw(ROLE == HEAD_CLS ? m * C + fixed : fixed + m);
            if (ROLE == HEAD_ROW) {
                nb[r] = bias ? bias[m] : 0.f;
                na[r] = ps ? ps[m] : 1.f;
                nn[r] = ns ? ns[m] : 1.f;
            }
        }
    }
    template <int NC>
    __device__ __forceinline__ void weights(const f32x4& sacc, int a0, int, int, int, f32x4 (&)[NC], float (&gv)[4]) {
        unsigned cur[4];
        float cb[4], ca[4], cn[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            cur[r] = raw[r];
            cb[r] = ROLE == HEAD_ROW ? nb[r] : bias_c;
            ca[r] = ROLE == HEAD_ROW ? na[r] : a_c;
            cn[r] = ROLE == HEAD_ROW ? nn[r] : b_c;
        }
        prefetch(a0 + 16);
        MllArgs fe = form;
        if (!GENERAL) fe.gp = fe.gn = fe.m = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float t;
            bool known;
            load_targets<1>(&cur[r], lkind, 0, &t, &known);
            const bool ok = known && stat_ok && (a0 + 4 * lg + r) < len;
            const float z = bias ? sacc[r] + cb[r] : sacc[r];
            float g = 0.f;
            if (GRAD) {
                const float ge = mll_elem<true>(z, t, ca[r], cn[r], fe);
                g = ok ? ge : 0.f;
            }
            gv[r] = g;
            if (SUMS) {
                const float le = mll_elem<false>(z, t, ca[r], cn[r], fe);
                sum_l = sum_l + (ok ? le : 0.f);
                cnt += ok ? 1 : 0;
                if (GRAD) sum_g = sum_g + g;
            }
        }
    }
};

template <int KT, int ROLE, int CSPLIT, bool PRODUCT, bool GENERAL>
__global__ __launch_bounds__(256, 1) void head_flash_kernel(HeadArgs p, int cpart) {
    constexpr int D = 32 * KT, NC = PRODUCT ? D / 16 / CSPLIT : 1;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int c_first = cpart * NC;
    const FlashBlock f = flash_block<true>(p.ns, p.nm, p.strm_per_split);
    const int64_t t = f.s0 + f.r16;                               // lane (lg, r16) ends with Out[t][16 c + 4 lg + r]
    const int64_t tc = t < p.ns ? t : p.ns - 1;
    HeadTerm<ROLE, PRODUCT, ROLE == HEAD_CLS, GENERAL> term;
    term.labels = p.labels; term.lkind = p.lkind; term.C = p.classes; term.m_beg = f.m_beg; term.len = f.len; term.lg = f.lg;
    term.fixed = ROLE == HEAD_CLS ? tc : tc * p.classes;
    term.stat_ok = t < p.ns;
    term.bias = p.bias; term.ps = p.pos_scale; term.ns = p.neg_scale;
    term.bias_c = (ROLE == HEAD_CLS && p.bias) ? p.bias[tc] : 0.f;
    term.a_c = (ROLE == HEAD_CLS && p.pos_scale) ? p.pos_scale[tc] : 1.f;
    term.b_c = (ROLE == HEAD_CLS && p.neg_scale) ? p.neg_scale[tc] : 1.f;
    term.form = p.form;
    term.prefetch(0);
    f32x4 oacc[NC];
    flash_stream<KT, NC, PRODUCT>(term, f, p.stat, p.ns, p.strm, c_first, smem, oacc);

    if (ROLE == HEAD_CLS) {                                       // a lane holds a quarter of class t's scalar sums
        double sum_l = (double)term.sum_l;
        float sum_g = term.sum_g;
        int cnt = term.cnt;
        sum_l = sum_l + __shfl_xor(sum_l, 16, 64);
        sum_l = sum_l + __shfl_xor(sum_l, 32, 64);
        sum_g = sum_g + __shfl_xor(sum_g, 16, 64);
        sum_g = sum_g + __shfl_xor(sum_g, 32, 64);
        cnt = cnt + __shfl_xor(cnt, 16, 64);
        cnt = cnt + __shfl_xor(cnt, 32, 64);
        if (t < p.ns) {
            if (PRODUCT) flash_store<NC, false>(p.part_o + ((int64_t)f.split * p.ns + t) * D, c_first, f.lg, oacc);
            if (f.lg == 0 && cpart == 0) {
                p.part_loss[(int64_t)f.split * p.ns + t] = sum_l;
                p.part_cnt[(int64_t)f.split * p.ns + t] = cnt;
                if (PRODUCT) p.part_g[(int64_t)f.split * p.ns + t] = sum_g;
            }
        }
    } else if (t < p.ns) {
        if (!p.direct) {
            flash_store<NC, false>(p.part_o + ((int64_t)f.split * p.ns + t) * D, c_first, f.lg, oacc);
        } else {
            const float sc = head_scale(p.totals, p.grad_out, p.factor, p.mean);
            const int64_t o0 = t * D + 16 * c_first + 4 * f.lg;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const f32x4 v = oacc[c] * sc;
                if (p.dh_f32)
                    *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(p.dh) + o0 + 16 * c) = v;
                else
                    *reinterpret_cast<u32x2*>(reinterpret_cast<unsigned short*>(p.dh) + o0 + 16 * c) =
                        u32x2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
            }
        }
    }
}

// the splits of a class added in order: stats[c] = loss sum (float64), stats[C + c] = valid count; with dw: dw_unscaled[c, :]
// and db_unscaled[c] (float32 sums of the float32 partials).  One wave per class.
__global__ __launch_bounds__(256) void head_cls_combine_kernel(const double* part_loss, const int* part_cnt, const float* part_g,
                                                               const float* part_o, int C, int K, int ksplit, double* stats,
                                                               float* dw, float* db) {
    const int lane = lane_id();
    const int c = (int)blockIdx.x * 4 + wave_id();
    if (c >= C) return;
    if (lane == 0) {
        double l = 0.0;
        long long k = 0;
        for (int s = 0; s < ksplit; ++s) {
            l += part_loss[(int64_t)s * C + c];
            k += part_cnt[(int64_t)s * C + c];
        }
        stats[c] = l;
        stats[C + c] = (double)k;
    }
    if (!dw) return;
    if (lane == 0) {
        float g = 0.f;
        for (int s = 0; s < ksplit; ++s) g += part_g[(int64_t)s * C + c];
        db[c] = g;
    }
    for (int k = lane; k < K; k += 64) {
        float o = 0.f;
        for (int s = 0; s < ksplit; ++s) o += part_o[((int64_t)s * C + c) * K + k];
        dw[(int64_t)c * K + k] = o;
    }
}

// totals of aecf_mlloss_forward from stats [2][C]: 256 strided partial sums in class order, then a fixed tree (one block)
__global__ __launch_bounds__(256) void head_totals_kernel(const double* stats, int C, int mean, double* totals) {
    __shared__ double red[2][256];
    double l = 0.0, k = 0.0;
    for (int c = threadIdx.x; c < C; c += 256) {
        l += stats[c];
        k += stats[C + c];
    }
    red[0][threadIdx.x] = l;
    red[1][threadIdx.x] = k;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            red[0][threadIdx.x] += red[0][threadIdx.x + w];
            red[1][threadIdx.x] += red[1][threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double aa = red[0][0], kk = red[1][0];
        totals[0] = aa;
        totals[1] = kk;
        const double r = mean ? (kk > 0.0 ? aa / kk : 0.0) : aa;
        float* tail = reinterpret_cast<float*>(totals + 2);
        tail[0] = (float)r;
        tail[1] = 0.0f;
    }
}

// dh[i, :] = scale * (the splits of row i added in order), rounded once.  One wave per row.
__global__ __launch_bounds__(256) void head_row_combine_kernel(const float* part_o, int64_t n, int K, int ksplit, const double* totals,
                                                               const float* grad_out, float factor, int mean, void* dh, int dh_f32) {
    const int lane = lane_id();
    const int64_t i = (int64_t)blockIdx.x * 4 + wave_id();
    if (i >= n) return;
    const float sc = head_scale(totals, grad_out, factor, mean);
    for (int k = lane; k < K; k += 64) {
        float o = 0.f;
        for (int s = 0; s < ksplit; ++s) o += part_o[((int64_t)s * n + i) * K + k];
        const float v = o * sc;
        if (dh_f32)
            reinterpret_cast<float*>(dh)[i * K + k] = v;
        else
            reinterpret_cast<unsigned short*>(dh)[i * K + k] = Tr<BF16>::from_f32(v);
    }
}

// dW = scale * dw_unscaled, db = scale * db_unscaled (either may be NULL)
__global__ __launch_bounds__(256) void head_scale_kernel(const float* dw_u, const float* db_u, int64_t nw, int C, const double* totals,
                                                         const float* grad_out, float factor, int mean, float* dw, float* db) {
    const float sc = head_scale(totals, grad_out, factor, mean);
    const int64_t step = (int64_t)gridDim.x * 256;
    const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (dw)
        for (int64_t i = i0; i < nw; i += step) dw[i] = dw_u[i] * sc;
    if (db)
        for (int64_t i = i0; i < C; i += step) db[i] = db_u[i] * sc;
}

// output column splits per launch: chosen from the compiler's report so that no instance uses scratch
template <int KT, int ROLE, bool PRODUCT>
constexpr int head_csplit() {
    return !PRODUCT ? 1 : (KT >= 24 ? 2 : 1);
}

template <int KT, int ROLE, bool PRODUCT>
void launch_head_role(const HeadArgs& a, int blocks, bool general, hipStream_t s) {
    constexpr int D = 32 * KT;
    constexpr int CSPLIT = head_csplit<KT, ROLE, PRODUCT>();
    const size_t smem = (size_t)2 * 32 * 2 * D;
    auto run = [&](auto kern) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        for (int cpart = 0; cpart < CSPLIT; ++cpart) kern<<<dim3((unsigned)blocks), dim3(256), smem, s>>>(a, cpart);
    };
    if (general)
        run(head_flash_kernel<KT, ROLE, CSPLIT, PRODUCT, true>);
    else
        run(head_flash_kernel<KT, ROLE, CSPLIT, PRODUCT, false>);
}

inline size_t al256(size_t v) { return (v + 255) / 256 * 256; }

struct HeadLayout {
    int ks_cls, ks_row;
    size_t o_bytes, loss_off, cnt_off, g_off, total;
};

// one slab of partial rows serves both roles: float32 [max(ks_cls C, ks_row n)][K] | float64 [ks_cls][C] loss sums |
// int32 [ks_cls][C] valid counts | float32 [ks_cls][C] g sums, every part rounded up to 256 bytes
HeadLayout head_layout(int64_t n, int C, int K) {
    HeadLayout L;
    L.ks_cls = flash_split(C, n).live;
    L.ks_row = flash_split(n, C).live;
    const size_t rows_cls = (size_t)L.ks_cls * C, rows_row = L.ks_row > 1 ? (size_t)L.ks_row * n : 0;
    L.o_bytes = al256((rows_cls > rows_row ? rows_cls : rows_row) * K * sizeof(float));
    L.loss_off = L.o_bytes;
    L.cnt_off = L.loss_off + al256(rows_cls * sizeof(double));
    L.g_off = L.cnt_off + al256(rows_cls * sizeof(int));
    L.total = L.g_off + al256(rows_cls * sizeof(float));
    return L;
}

inline bool head_general(float gp, float gn, float m) { return gp != 0.f || gn != 0.f || m != 0.f; }

}  // namespace

bool mlhead_supported(int64_t n, int classes, int k) {
    return nce_flash_supported(0, k) && classes >= 1 && classes <= 65536 && n >= 1 && n < (1ll << 31);
}

size_t mlhead_workspace_bytes(int64_t n, int classes, int k) { return head_layout(n, classes, k).total; }

void launch_mlhead_forward(int64_t n, int classes, int k, int label_dtype, const void* h, const void* w, const float* bias,
                           const void* labels, const float* pos_scale, const float* neg_scale, float gamma_pos, float gamma_neg,
                           float margin, float eps, int mean, int want_grads, double* stats, double* totals, float* dw_unscaled,
                           float* db_unscaled, void* workspace, hipStream_t s) {
    const HeadLayout L = head_layout(n, classes, k);
    const FlashSplit sp = flash_split(classes, n);
    char* ws = reinterpret_cast<char*>(workspace);
    HeadArgs x = {};
    x.stat = (const unsigned short*)w; x.strm = (const unsigned short*)h; x.ns = classes; x.nm = n; x.classes = classes;
    x.labels = labels; x.lkind = label_dtype; x.bias = bias; x.pos_scale = pos_scale; x.neg_scale = neg_scale;
    x.form = mll_args(gamma_pos, gamma_neg, margin, eps);
    x.part_o = reinterpret_cast<float*>(ws);
    x.part_loss = reinterpret_cast<double*>(ws + L.loss_off);
    x.part_cnt = reinterpret_cast<int*>(ws + L.cnt_off);
    x.part_g = reinterpret_cast<float*>(ws + L.g_off);
    x.strm_per_split = sp.per;
    const int blocks = (int)(((int64_t)classes + 63) / 64) * sp.live;
    const bool general = head_general(gamma_pos, gamma_neg, margin);
    dispatch_kt(k, [&](auto kt) {
        constexpr int KT = decltype(kt)::value;
        if (want_grads)
            launch_head_role<KT, HEAD_CLS, true>(x, blocks, general, s);
        else
            launch_head_role<KT, HEAD_CLS, false>(x, blocks, general, s);
    });
    head_cls_combine_kernel<<<dim3((unsigned)((classes + 3) / 4)), dim3(256), 0, s>>>(
        x.part_loss, x.part_cnt, x.part_g, x.part_o, classes, k, sp.live, stats, want_grads ? dw_unscaled : nullptr, db_unscaled);
    head_totals_kernel<<<dim3(1), dim3(256), 0, s>>>(stats, classes, mean, totals);
}

void launch_mlhead_backward(int64_t n, int classes, int k, int label_dtype, const void* h, const void* w, const float* bias,
                            const void* labels, const float* pos_scale, const float* neg_scale, float gamma_pos, float gamma_neg,
                            float margin, float eps, int mean, const double* totals, const float* grad_out, float factor,
                            const float* dw_unscaled, const float* db_unscaled, int dh_f32, void* dh, float* dw, float* db,
                            void* workspace, hipStream_t s) {
    if (dh) {
        const FlashSplit sp = flash_split(n, classes);
        HeadArgs y = {};
        y.stat = (const unsigned short*)h; y.strm = (const unsigned short*)w; y.ns = n; y.nm = classes; y.classes = classes;
        y.labels = labels; y.lkind = label_dtype; y.bias = bias; y.pos_scale = pos_scale; y.neg_scale = neg_scale;
        y.form = mll_args(gamma_pos, gamma_neg, margin, eps);
        y.part_o = reinterpret_cast<float*>(workspace);
        y.strm_per_split = sp.per;
        y.totals = totals; y.grad_out = grad_out; y.factor = factor; y.mean = mean; y.dh = dh; y.dh_f32 = dh_f32;
        y.direct = sp.live == 1;
        const int blocks = (int)((n + 63) / 64) * sp.live;
        const bool general = head_general(gamma_pos, gamma_neg, margin);
        dispatch_kt(k, [&](auto kt) {
            constexpr int KT = decltype(kt)::value;
            launch_head_role<KT, HEAD_ROW, true>(y, blocks, general, s);
        });
        if (!y.direct)
            head_row_combine_kernel<<<dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s>>>(y.part_o, n, k, sp.live, totals, grad_out,
                                                                                        factor, mean, dh, dh_f32);
    }
    if (dw || db) {
        const int64_t nw = (int64_t)classes * k;
        int64_t blocks = ((dw ? nw : classes) + 255) / 256;
        if (blocks > 4096) blocks = 4096;
        head_scale_kernel<<<dim3((unsigned)blocks), dim3(256), 0, s>>>(dw_unscaled, db_unscaled, nw, classes, totals, grad_out, factor,
                                                                      mean, dw, db);
    }
}

}  // namespace aecf
