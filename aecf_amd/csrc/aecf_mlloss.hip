// Multi-label classification loss, gfx950 (aecf_mlloss_forward / _backward): binary cross-entropy, focal and asymmetric loss of
// logits [n, C] against targets [n, C] as ONE elementwise formula (include/aecf_hip.h, "multi-label classification loss"):
//   l = a_c t' (1 - s)^gp (-log s)  +  b_c (1 - t') q^gn (-log(1 - q)),    s = sigmoid(x), t' = t (1 - eps) + eps / 2, q = max(s - m, 0)
//
// Arithmetic: float32 throughout, on the logit as stored.  With e = exp(-|x|), l1p = log1p(e), r = 1 / (1 + e):
//   s = x >= 0 ? r : e r        1 - s = sigmoid(-x) = x >= 0 ? e r : r            (no 1 - s subtraction)
//   -log s = max(-x, 0) + l1p   -log(1 - s) = max(x, 0) + l1p                      (softplus forms)
//   (1 - s)^gp = exp(-gp (-log(1 - s)))   s^gn = exp(-gn (-log s))   q^gn = exp(gn log q)   and exactly 1 where the exponent is 0
// With a margin m > 0 the negative side lives where q = s - m is not <= 0 (a NaN logit stays alive and gives NaN): 1 - q is
// formed as (1 - s) + m, a sum of two positive numbers.  A term whose coefficient (a_c t' or b_c (1 - t')) is 0, a dead negative
// side and an ignored element are exact zeros by select: no product with 0 stands in for a select, so no inf * 0 exists.
//
// Mapping.  A thread owns one COLUMN GROUP of V consecutive classes (V = 16 bytes of logits where C % V == 0 and the pointers
// are 16-byte aligned, else 1) and walks rows, so its V loss sums and V valid counts belong to fixed classes.  ncg = C / V:
//   ncg <= 256: rpi = 256 / ncg rows per step; thread t has group t % ncg and row t / ncg of the step -- consecutive lanes read
//               consecutive addresses across row ends.  The rpi threads of a class are joined through LDS in row order, in float64.
//   ncg  > 256: grid.y = ceil(ncg / 256) column blocks, one row per step, the thread's sums go out as they are.
// Row block bx owns rows [bx rows_pb, (bx + 1) rows_pb): partial float64 loss sums and int32 valid counts [nrb][C], every entry
// written by exactly one thread.  The finalize (one block of 1024 lanes: 64 slices x 16 classes) adds the row blocks slice by
// slice, the slices in order, the classes in order: float64, a fixed order, no atomics -- the same bits on every run.
// The backward recomputes the element and stores grad * scale, scale = upstream * factor / N read from the totals record.
#include "aecf_kernels.h"
#include "aecf_mlloss_elem.h"

#include <cmath>

namespace aecf {

namespace {

constexpr int MLL_T = 256;              // lanes of a pass block
constexpr int MLL_ELEMS = 16384;        // elements a row block should at least hold
constexpr int MLL_MAX_BLOCKS = 1024;    // row blocks at most ...
constexpr int MLL_MAX_PART = 1 << 20;   // ... and partial entries (row blocks x classes) at most
constexpr int MLL_FT = 1024;            // lanes of the finalize block: 64 slices x 16 classes

inline size_t al256(size_t v) { return (v + 255) / 256 * 256; }

struct MllGeo {
    int ncg, rpi, gy, nrb;
    int64_t rows_pb;
};

inline void mll_row_blocks(int64_t n, int C, int& nrb, int64_t& rows_pb) {
    int64_t want = (n * C + MLL_ELEMS - 1) / MLL_ELEMS;
    int64_t cap = MLL_MAX_PART / C;
    if (cap > MLL_MAX_BLOCKS) cap = MLL_MAX_BLOCKS;
    if (cap < 1) cap = 1;
    if (want < 1) want = 1;
    if (want > cap) want = cap;
    rows_pb = (n + want - 1) / want;
    nrb = (int)((n + rows_pb - 1) / rows_pb);
}

inline MllGeo mll_geo(int64_t n, int C, int V) {
    MllGeo g;
    g.ncg = C / V;
    g.gy = (g.ncg + MLL_T - 1) / MLL_T;
    g.rpi = g.gy == 1 ? MLL_T / g.ncg : 1;
    mll_row_blocks(n, C, g.nrb, g.rows_pb);
    return g;
}

template <typename T, int V>
__device__ __forceinline__ void load_logits(const typename Tr<T>::elem* logits, int64_t idx, float* x) {
    typename Tr<T>::elem v[V];
    load_bytes<sizeof(typename Tr<T>::elem) * V>(logits + idx, v);
#pragma unroll
    for (int j = 0; j < V; ++j) x[j] = Tr<T>::to_f32(v[j]);
}

struct MllWho {
    int cg, rsub;
    bool active;
};

__device__ __forceinline__ MllWho mll_who(int ncg, int rpi) {
    MllWho w;
    const int t = threadIdx.x;
    if (gridDim.y == 1) {
        w.cg = t % ncg;
        w.rsub = t / ncg;
        w.active = w.rsub < rpi;
    } else {
        w.cg = blockIdx.y * MLL_T + t;
        w.rsub = 0;
        w.active = w.cg < ncg;
    }
    return w;
}

template <typename T, int V>
__global__ __launch_bounds__(MLL_T) void mll_fwd_kernel(const typename Tr<T>::elem* __restrict__ logits, const void* __restrict__ labels,
                                                        int lkind, const float* __restrict__ pos_scale,
                                                        const float* __restrict__ neg_scale, int64_t n, int C, int ncg, int rpi,
                                                        int64_t rows_pb, MllArgs p, double* __restrict__ part_loss,
                                                        int* __restrict__ part_cnt) {
    __shared__ float sl[MLL_T * V];
    __shared__ int sc[MLL_T * V];
    const MllWho w = mll_who(ncg, rpi);
    const int c0 = w.cg * V;
    const int64_t r_lo = (int64_t)blockIdx.x * rows_pb;
    const int64_t r_hi = r_lo + rows_pb < n ? r_lo + rows_pb : n;
    float acc[V];
    int cnt[V];
#pragma unroll
    for (int j = 0; j < V; ++j) { acc[j] = 0.0f; cnt[j] = 0; }
    if (w.active) {
        float a[V], b[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            a[j] = pos_scale ? pos_scale[c0 + j] : 1.0f;
            b[j] = neg_scale ? neg_scale[c0 + j] : 1.0f;
        }
        for (int64_t r = r_lo + w.rsub; r < r_hi; r += rpi) {
            const int64_t idx = r * C + c0;
            float x[V], t[V];
            bool valid[V];
            load_logits<T, V>(logits, idx, x);
            load_targets<V>(labels, lkind, idx, t, valid);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float l = mll_elem<false>(x[j], t[j], a[j], b[j], p);
                acc[j] += valid[j] ? l : 0.0f;
                cnt[j] += valid[j] ? 1 : 0;
            }
        }
    }
    double* pl = part_loss + (int64_t)blockIdx.x * C;
    int* pc = part_cnt + (int64_t)blockIdx.x * C;
    if (gridDim.y == 1) {
#pragma unroll
        for (int j = 0; j < V; ++j) { sl[threadIdx.x * V + j] = acc[j]; sc[threadIdx.x * V + j] = cnt[j]; }
        __syncthreads();
        for (int c = threadIdx.x; c < C; c += MLL_T) {
            const int g = c / V, j = c % V;
            double s = 0.0;
            int k = 0;
            for (int rs = 0; rs < rpi; ++rs) {
                s += (double)sl[(rs * ncg + g) * V + j];
                k += sc[(rs * ncg + g) * V + j];
            }
            pl[c] = s;
            pc[c] = k;
        }
    } else if (w.active) {
#pragma unroll
        for (int j = 0; j < V; ++j) { pl[c0 + j] = (double)acc[j]; pc[c0 + j] = cnt[j]; }
    }
}

// stats [2][C] = loss sums | valid counts; totals = sum | N as float64, then the reduced loss as float32 and a zero word
__global__ __launch_bounds__(MLL_FT) void mll_finalize_kernel(const double* __restrict__ part_loss, const int* __restrict__ part_cnt,
                                                              int C, int nrb, int mean, double* __restrict__ stats,
                                                              double* __restrict__ totals) {
    __shared__ double fl[64][16];
    __shared__ long long fc[64][16];
    const int t = threadIdx.x, s = t >> 4, cl = t & 15;
    double tot_l = 0.0;
    long long tot_n = 0;
    for (int c0 = 0; c0 < C; c0 += 16) {
        const int c = c0 + cl;
        double a = 0.0;
        long long k = 0;
        if (c < C)
            for (int b = s; b < nrb; b += 64) {
                a += part_loss[(int64_t)b * C + c];
                k += part_cnt[(int64_t)b * C + c];
            }
        fl[s][cl] = a;
        fc[s][cl] = k;
        __syncthreads();
        if (t < 16 && c < C) {
            double aa = 0.0;
            long long kk = 0;
            for (int i = 0; i < 64; ++i) { aa += fl[i][t]; kk += fc[i][t]; }
            stats[c] = aa;
            stats[C + c] = (double)kk;
            tot_l += aa;
            tot_n += kk;
        }
        __syncthreads();
    }
    if (t < 16) { fl[0][t] = tot_l; fc[0][t] = tot_n; }
    __syncthreads();
    if (t == 0) {
        double aa = 0.0;
        long long kk = 0;
        for (int i = 0; i < 16; ++i) { aa += fl[0][i]; kk += fc[0][i]; }
        totals[0] = aa;
        totals[1] = (double)kk;
        const double red = mean ? (kk > 0 ? aa / (double)kk : 0.0) : aa;
        float* tail = reinterpret_cast<float*>(totals + 2);
        tail[0] = (float)red;
        tail[1] = 0.0f;
    }
}

template <typename T, int V>
__global__ __launch_bounds__(MLL_T) void mll_bwd_kernel(const typename Tr<T>::elem* __restrict__ logits, const void* __restrict__ labels,
                                                        int lkind, const float* __restrict__ pos_scale,
                                                        const float* __restrict__ neg_scale, int64_t n, int C, int ncg, int rpi,
                                                        int64_t rows_pb, MllArgs p, const double* __restrict__ totals,
                                                        const float* __restrict__ grad_out, float factor, int mean,
                                                        typename Tr<T>::elem* __restrict__ dlogits) {
    const MllWho w = mll_who(ncg, rpi);
    if (!w.active) return;
    const int c0 = w.cg * V;
    const int64_t r_lo = (int64_t)blockIdx.x * rows_pb;
    const int64_t r_hi = r_lo + rows_pb < n ? r_lo + rows_pb : n;
    const float up = (grad_out ? grad_out[0] : 1.0f) * factor;
    float scale = up;
    if (mean) {
        const double N = totals[1];
        scale = N > 0.0 ? (float)((double)up / N) : 0.0f;
    }
    float a[V], b[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        a[j] = pos_scale ? pos_scale[c0 + j] : 1.0f;
        b[j] = neg_scale ? neg_scale[c0 + j] : 1.0f;
    }
    for (int64_t r = r_lo + w.rsub; r < r_hi; r += rpi) {
        const int64_t idx = r * C + c0;
        float x[V], t[V];
        bool valid[V];
        load_logits<T, V>(logits, idx, x);
        load_targets<V>(labels, lkind, idx, t, valid);
        typename Tr<T>::elem o[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float g = mll_elem<true>(x[j], t[j], a[j], b[j], p) * scale;
            o[j] = Tr<T>::from_f32(valid[j] ? g : 0.0f);
        }
        constexpr int NB = sizeof(typename Tr<T>::elem) * V;
        __builtin_memcpy(__builtin_assume_aligned(dlogits + idx, NB >= 16 ? 16 : NB), o, NB);
    }
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <typename T>
void mll_fwd_launch(int64_t n, int C, const void* logits, const void* labels, int lkind, const float* ps, const float* ns,
                    const MllArgs& p, double* part_loss, int* part_cnt, hipStream_t s) {
    typedef typename Tr<T>::elem E;
    constexpr int VV = 16 / sizeof(E);
    const bool vec = C % VV == 0 && al16(logits) && al16(labels);
    const MllGeo g = mll_geo(n, C, vec ? VV : 1);
    const dim3 grid((unsigned)g.nrb, (unsigned)g.gy);
    if (vec)
        mll_fwd_kernel<T, VV><<<grid, dim3(MLL_T), 0, s>>>((const E*)logits, labels, lkind, ps, ns, n, C, g.ncg, g.rpi, g.rows_pb, p,
                                                           part_loss, part_cnt);
    else
        mll_fwd_kernel<T, 1><<<grid, dim3(MLL_T), 0, s>>>((const E*)logits, labels, lkind, ps, ns, n, C, g.ncg, g.rpi, g.rows_pb, p,
                                                          part_loss, part_cnt);
}

template <typename T>
void mll_bwd_launch(int64_t n, int C, const void* logits, const void* labels, int lkind, const float* ps, const float* ns,
                    const MllArgs& p, const double* totals, const float* grad_out, float factor, int mean, void* dlogits,
                    hipStream_t s) {
    typedef typename Tr<T>::elem E;
    constexpr int VV = 16 / sizeof(E);
    const bool vec = C % VV == 0 && al16(logits) && al16(labels) && al16(dlogits);
    const MllGeo g = mll_geo(n, C, vec ? VV : 1);
    const dim3 grid((unsigned)g.nrb, (unsigned)g.gy);
    if (vec)
        mll_bwd_kernel<T, VV><<<grid, dim3(MLL_T), 0, s>>>((const E*)logits, labels, lkind, ps, ns, n, C, g.ncg, g.rpi, g.rows_pb, p,
                                                           totals, grad_out, factor, mean, (E*)dlogits);
    else
        mll_bwd_kernel<T, 1><<<grid, dim3(MLL_T), 0, s>>>((const E*)logits, labels, lkind, ps, ns, n, C, g.ncg, g.rpi, g.rows_pb, p,
                                                          totals, grad_out, factor, mean, (E*)dlogits);
}

}  // namespace

bool mlloss_supported(int64_t n, int classes) { return classes <= 4096 && n <= (1ll << 30) && n * classes <= (1ll << 30); }

size_t mlloss_workspace_bytes(int64_t n, int classes) {
    int nrb;
    int64_t rows_pb;
    mll_row_blocks(n, classes, nrb, rows_pb);
    return al256((size_t)nrb * classes * 8) + al256((size_t)nrb * classes * 4);
}

void launch_mlloss_forward(int64_t n, int classes, int dtype, int label_dtype, const void* logits, const void* labels,
                           const float* pos_scale, const float* neg_scale, float gamma_pos, float gamma_neg, float margin, float eps,
                           int mean, double* stats, double* totals, void* workspace, hipStream_t s) {
    int nrb;
    int64_t rows_pb;
    mll_row_blocks(n, classes, nrb, rows_pb);
    double* part_loss = (double*)workspace;
    int* part_cnt = (int*)((char*)workspace + al256((size_t)nrb * classes * 8));
    const MllArgs p = mll_args(gamma_pos, gamma_neg, margin, eps);
    if (dtype == 1)
        mll_fwd_launch<F32>(n, classes, logits, labels, label_dtype, pos_scale, neg_scale, p, part_loss, part_cnt, s);
    else if (dtype == 2)
        mll_fwd_launch<F16>(n, classes, logits, labels, label_dtype, pos_scale, neg_scale, p, part_loss, part_cnt, s);
    else
        mll_fwd_launch<BF16>(n, classes, logits, labels, label_dtype, pos_scale, neg_scale, p, part_loss, part_cnt, s);
    mll_finalize_kernel<<<dim3(1), dim3(MLL_FT), 0, s>>>(part_loss, part_cnt, classes, nrb, mean, stats, totals);
}

void launch_mlloss_backward(int64_t n, int classes, int dtype, int label_dtype, const void* logits, const void* labels,
                            const float* pos_scale, const float* neg_scale, float gamma_pos, float gamma_neg, float margin, float eps,
                            int mean, const double* totals, const float* grad_out, float factor, void* dlogits, hipStream_t s) {
    const MllArgs p = mll_args(gamma_pos, gamma_neg, margin, eps);
    if (dtype == 1)
        mll_bwd_launch<F32>(n, classes, logits, labels, label_dtype, pos_scale, neg_scale, p, totals, grad_out, factor, mean, dlogits, s);
    else if (dtype == 2)
        mll_bwd_launch<F16>(n, classes, logits, labels, label_dtype, pos_scale, neg_scale, p, totals, grad_out, factor, mean, dlogits, s);
    else
        mll_bwd_launch<BF16>(n, classes, logits, labels, label_dtype, pos_scale, neg_scale, p, totals, grad_out, factor, mean, dlogits, s);
}

}  // namespace aecf
