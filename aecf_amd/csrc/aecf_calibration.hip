// Multi-label calibration, gfx950 (aecf_mlcal_stats / _fit_sums / _fit_update and their entry points): the reliability bins, Brier
// and NLL sums of logits [n, C] under z = x scale_c + bias_c, the Newton sums of a temperature / Platt fit, and the fit's damped
// Newton step (include/aecf_hip.h, "multi-label calibration").
//
// Arithmetic: float32 per element, on the logit as stored.  z = x * scale + bias as a rounded product and a rounded sum (this
// file is compiled without contraction, so no fma stands in for the two), or z = x where there is neither.  With e = exp(-|z|),
// l1p = log1p(e), r = 1 / (1 + e):  p = z >= 0 ? r : e r,  1 - p = z >= 0 ? e r : r,  -log p = max(-z, 0) + l1p,
// -log(1 - p) = max(z, 0) + l1p -- aecf_mlloss.hip's forms, no 1 - p subtraction.  bin = #{ j : z > e_j }.  Every exclusion (an
// unknown target, a NaN logit, a non-finite logit in the fit) is a branch around the element's adds, never a product with 0.
//
// Mapping (aecf_mlloss.hip's).  A thread owns one COLUMN GROUP of V consecutive classes and walks the rows of its row block, so
// all it adds belongs to fixed classes.  Statistics pass: the thread's bins live in LDS, one private float32 (sum of p) and one
// packed uint32 (count | positives << 16; a thread owns fewer than 2^16 rows) per (bin, class) at [bin][j][thread] -- conflict
// free -- which sizes the block: Tn = 64 .. 256 lanes with Tn V B <= 4096 slots (32 KB, so that several blocks share a CU's LDS),
// V = the 16-byte vector of the logits while V B <= 64, else half of it (8-byte loads of 16-bit logits), else 1.  The rpi = Tn / ncg threads of a class are joined in row order in float64; the scalars (Brier,
// NLL, invalid) pass through the same LDS afterwards.  Row block bx writes one float64 slab [K][C], every entry by exactly one
// thread; the finalize adds the slabs in order.  float64 above the thread, a fixed order, no atomics: the same bits on every
// run, and integer results that no arrangement can change.
#pragma clang fp contract(off)

#include <cmath>

#include "../../include/aecf_hip.h"
#include "aecf_kernels.h"

namespace aecf {

namespace {

constexpr int CAL_T = 256;              // lanes of a fit-sums block and the most of a statistics block
constexpr int CAL_ELEMS = 16384;        // elements a row block should at least hold
constexpr int CAL_MAX_BLOCKS = 1024;    // row blocks at most ...
constexpr int CAL_MAX_PART = 1 << 19;   // ... and slab columns (row blocks x classes) at most
constexpr int CAL_SLOTS = 4096;         // (bin, class, lane) slots of a statistics block: 8 bytes each
constexpr int CAL_FIT_K = 9;            // rows of the fit sums
constexpr int CAL_STATE_K = 12;         // rows of the fit state

inline size_t al256(size_t v) { return (v + 255) / 256 * 256; }
inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

struct CalEdges {
    float e[AECF_MLCAL_MAX_BINS - 1];
};

struct CalGeo {
    int ncg, rpi, gy, nrb, tn;
    int64_t rows_pb;
};

inline void cal_row_blocks(int64_t n, int C, int& nrb, int64_t& rows_pb) {
    int64_t want = (n * C + CAL_ELEMS - 1) / CAL_ELEMS;
    int64_t cap = CAL_MAX_PART / C;
    if (cap > CAL_MAX_BLOCKS) cap = CAL_MAX_BLOCKS;
    if (cap < 1) cap = 1;
    if (want < 1) want = 1;
    if (want > cap) want = cap;
    rows_pb = (n + want - 1) / want;
    nrb = (int)((n + rows_pb - 1) / rows_pb);
}

inline CalGeo cal_geo(int64_t n, int C, int V, int tn) {
    CalGeo g;
    g.tn = tn;
    g.ncg = C / V;
    g.gy = (g.ncg + tn - 1) / tn;
    g.rpi = g.gy == 1 ? tn / g.ncg : 1;
    cal_row_blocks(n, C, g.nrb, g.rows_pb);
    return g;
}

template <int NB>
__device__ __forceinline__ void load_bytes(const void* p, void* dst) {
    constexpr int A = NB >= 16 ? 16 : NB;
    __builtin_memcpy(dst, __builtin_assume_aligned(p, A), NB);
}

// V targets at element idx: positive (non-zero) and known (floating point: not NaN and not < 0; int8: not < 0)
template <int V>
__device__ __forceinline__ void load_targets(const void* labels, int kind, int64_t idx, bool* pos, bool* known) {
    if (kind == 1) {
        float v[V];
        load_bytes<4 * V>((const float*)labels + idx, v);
#pragma unroll
        for (int j = 0; j < V; ++j) { pos[j] = v[j] != 0.0f; known[j] = v[j] >= 0.0f; }
    } else if (kind == 0 || kind == 2) {
        unsigned short v[V];
        load_bytes<2 * V>((const unsigned short*)labels + idx, v);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float t = kind == 0 ? Tr<BF16>::to_f32(v[j]) : Tr<F16>::to_f32(v[j]);
            pos[j] = t != 0.0f;
            known[j] = t >= 0.0f;
        }
    } else {
        signed char v[V];
        load_bytes<V>((const signed char*)labels + idx, v);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            pos[j] = v[j] != 0;
            known[j] = kind == 3 || v[j] >= 0;
        }
    }
}

template <typename T, int V>
__device__ __forceinline__ void load_logits(const typename Tr<T>::elem* logits, int64_t idx, float* x) {
    typename Tr<T>::elem v[V];
    load_bytes<sizeof(typename Tr<T>::elem) * V>(logits + idx, v);
#pragma unroll
    for (int j = 0; j < V; ++j) x[j] = Tr<T>::to_f32(v[j]);
}

struct CalElem {
    float p, q, nlp, nlq;               // sigmoid(z), 1 - sigmoid(z), -log p, -log(1 - p)
};

__device__ __forceinline__ CalElem cal_elem(float z) {
    const float e = expf(-fabsf(z));
    const float l1p = log1pf(e);
    const float r = 1.0f / (1.0f + e);
    const float er = e * r;
    const bool up = z >= 0.0f;
    CalElem o;
    o.p = up ? r : er;
    o.q = up ? er : r;
    o.nlp = fmaxf(-z, 0.0f) + l1p;
    o.nlq = fmaxf(z, 0.0f) + l1p;
    return o;
}

// the product and the sum are rounded one after the other (no contraction in this file)
__device__ __forceinline__ float cal_z(float x, float s, float b) {
    const float m = x * s;
    return m + b;
}

struct CalWho {
    int cg, rsub, nloc, gbase;
    bool active;
};

__device__ __forceinline__ CalWho cal_who(int ncg, int rpi) {
    CalWho w;
    const int t = threadIdx.x, tn = blockDim.x;
    if (gridDim.y == 1) {
        w.cg = t % ncg;
        w.rsub = t / ncg;
        w.active = w.rsub < rpi;
        w.nloc = ncg;
        w.gbase = 0;
    } else {
        w.gbase = blockIdx.y * tn;
        w.cg = w.gbase + t;
        w.rsub = 0;
        w.active = w.cg < ncg;
        w.nloc = tn;
    }
    return w;
}

// one value per (lane, j) through buf [V][tn]: the rpi lanes of a class added in row order in float64, stored at row[c]
template <int V>
__device__ __forceinline__ void cal_join(float* buf, const float* val, const CalWho& w, int rpi, int C, double* row) {
    const int t = threadIdx.x, tn = blockDim.x;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < V; ++j) buf[j * tn + t] = val[j];
    __syncthreads();
    for (int lc = t; lc < w.nloc * V; lc += tn) {
        const int g = lc / V, j = lc % V;
        const int c = (w.gbase + g) * V + j;
        if (c >= C) continue;
        double s = 0.0;
        for (int rs = 0; rs < rpi; ++rs) s += (double)buf[j * tn + rs * w.nloc + g];
        row[c] = s;
    }
}

// slab of row block bx: [count B | positives B | sum p B | brier | nll | invalid | valid | valid positives][C]
template <typename T, int V>
__global__ __launch_bounds__(CAL_T) void cal_stats_kernel(const typename Tr<T>::elem* __restrict__ logits, const void* __restrict__ labels,
                                                          int lkind, const float* __restrict__ scale, const float* __restrict__ bias,
                                                          CalEdges edges, int B, int64_t n, int C, int ncg, int rpi, int64_t rows_pb,
                                                          double* __restrict__ part) {
    extern __shared__ float cal_smem[];
    const int t = threadIdx.x, tn = blockDim.x;
    float* conf = cal_smem;                                     // [B][V][tn]
    unsigned* cnt = (unsigned*)(cal_smem + B * V * tn);         // [B][V][tn]
    for (int s = 0; s < B * V; ++s) { conf[s * tn + t] = 0.0f; cnt[s * tn + t] = 0u; }
    const CalWho w = cal_who(ncg, rpi);
    const int c0 = w.cg * V;
    const int64_t r_lo = (int64_t)blockIdx.x * rows_pb;
    const int64_t r_hi = r_lo + rows_pb < n ? r_lo + rows_pb : n;
    const bool aff = scale != nullptr || bias != nullptr;
    float brier[V], nll[V], ninv[V], nval[V], npos[V];              // (a thread owns fewer than 2^16 rows: its counts are exact)
#pragma unroll
    for (int j = 0; j < V; ++j) { brier[j] = 0.0f; nll[j] = 0.0f; ninv[j] = 0.0f; nval[j] = 0.0f; npos[j] = 0.0f; }
    if (w.active) {
        float sc[V], bi[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            sc[j] = scale ? scale[c0 + j] : 1.0f;
            bi[j] = bias ? bias[c0 + j] : 0.0f;
        }
        for (int64_t r = r_lo + w.rsub; r < r_hi; r += rpi) {
            const int64_t idx = r * C + c0;
            float x[V];
            bool pos[V], known[V];
            load_logits<T, V>(logits, idx, x);
            load_targets<V>(labels, lkind, idx, pos, known);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const bool nan = x[j] != x[j];
                if (known[j] && nan) ninv[j] += 1.0f;
                if (known[j] && !nan) {
                    const float z = aff ? cal_z(x[j], sc[j], bi[j]) : x[j];
                    int bin = 0;                                    // (edges past the last are +inf: never exceeded)
#pragma unroll
                    for (int i = 0; i < 15; ++i) bin += z > edges.e[i] ? 1 : 0;
                    if (B > 16) {
#pragma unroll
                        for (int i = 15; i < AECF_MLCAL_MAX_BINS - 1; ++i) bin += z > edges.e[i] ? 1 : 0;
                    }
                    const CalElem el = cal_elem(z);
                    const int slot = (bin * V + j) * tn + t;
                    conf[slot] += el.p;
                    cnt[slot] += pos[j] ? 0x10001u : 1u;
                    brier[j] += pos[j] ? el.q * el.q : el.p * el.p;
                    nll[j] += pos[j] ? el.nlp : el.nlq;
                    nval[j] += 1.0f;
                    npos[j] += pos[j] ? 1.0f : 0.0f;
                }
            }
        }
    }
    __syncthreads();
    double* pb = part + (int64_t)blockIdx.x * (3 * B + 5) * C;
    const int per = w.nloc * V;
    for (int i = t; i < B * per; i += tn) {
        const int k = i / per, lc = i % per;
        const int g = lc / V, j = lc % V;
        const int c = (w.gbase + g) * V + j;
        if (c >= C) continue;
        double s = 0.0;
        unsigned a = 0u, ps = 0u;
        for (int rs = 0; rs < rpi; ++rs) {
            const int slot = (k * V + j) * tn + rs * w.nloc + g;
            s += (double)conf[slot];
            const unsigned u = cnt[slot];
            a += u & 0xffffu;
            ps += u >> 16;
        }
        pb[(int64_t)k * C + c] = (double)a;
        pb[(int64_t)(B + k) * C + c] = (double)ps;
        pb[(int64_t)(2 * B + k) * C + c] = s;
    }
    cal_join<V>(cal_smem, brier, w, rpi, C, pb + (int64_t)(3 * B) * C);
    cal_join<V>(cal_smem, nll, w, rpi, C, pb + (int64_t)(3 * B + 1) * C);
    cal_join<V>(cal_smem, ninv, w, rpi, C, pb + (int64_t)(3 * B + 2) * C);
    cal_join<V>(cal_smem, nval, w, rpi, C, pb + (int64_t)(3 * B + 3) * C);
    cal_join<V>(cal_smem, npos, w, rpi, C, pb + (int64_t)(3 * B + 4) * C);
}

// slab of row block bx: [L | g1 | g0 | h11 | h01 | h00 | used | used positives | skipped][C]
template <typename T, int V>
__global__ __launch_bounds__(CAL_T) void cal_fit_kernel(const typename Tr<T>::elem* __restrict__ logits, const void* __restrict__ labels,
                                                        int lkind, const float* __restrict__ scale, const float* __restrict__ bias,
                                                        int64_t n, int C, int ncg, int rpi, int64_t rows_pb, double* __restrict__ part) {
    __shared__ float buf[CAL_T * V];
    const CalWho w = cal_who(ncg, rpi);
    const int c0 = w.cg * V;
    const int64_t r_lo = (int64_t)blockIdx.x * rows_pb;
    const int64_t r_hi = r_lo + rows_pb < n ? r_lo + rows_pb : n;
    const bool aff = scale != nullptr || bias != nullptr;
    float acc[CAL_FIT_K][V];
#pragma unroll
    for (int k = 0; k < CAL_FIT_K; ++k)
#pragma unroll
        for (int j = 0; j < V; ++j) acc[k][j] = 0.0f;
    if (w.active) {
        float sc[V], bi[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            sc[j] = scale ? scale[c0 + j] : 1.0f;
            bi[j] = bias ? bias[c0 + j] : 0.0f;
        }
        for (int64_t r = r_lo + w.rsub; r < r_hi; r += rpi) {
            const int64_t idx = r * C + c0;
            float x[V];
            bool pos[V], known[V];
            load_logits<T, V>(logits, idx, x);
            load_targets<V>(labels, lkind, idx, pos, known);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float ax = fabsf(x[j]);
                if (known[j] && ax == INFINITY) acc[8][j] += 1.0f;
                if (known[j] && ax < INFINITY) {                    // a NaN logit is neither
                    const float z = aff ? cal_z(x[j], sc[j], bi[j]) : x[j];
                    const CalElem el = cal_elem(z);
                    const float d = pos[j] ? -el.q : el.p;          // s - y
                    const float wt = el.p * el.q;
                    const float wx = wt * x[j];
                    acc[0][j] += pos[j] ? el.nlp : el.nlq;
                    acc[1][j] += d * x[j];
                    acc[2][j] += d;
                    acc[3][j] += wx * x[j];
                    acc[4][j] += wx;
                    acc[5][j] += wt;
                    acc[6][j] += 1.0f;
                    acc[7][j] += pos[j] ? 1.0f : 0.0f;
                }
            }
        }
    }
    double* pb = part + (int64_t)blockIdx.x * CAL_FIT_K * C;
#pragma unroll
    for (int k = 0; k < CAL_FIT_K; ++k) cal_join<V>(buf, acc[k], w, rpi, C, pb + (int64_t)k * C);
}

// out[k][c] = the slabs' entries added in slab order
__global__ __launch_bounds__(256) void cal_finalize_kernel(const double* __restrict__ part, int K, int C, int nrb,
                                                           double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)K * C) return;
    const double* p = part + i;
    const int64_t pitch = (int64_t)K * C;
    double a = 0.0;
#pragma unroll 8
    for (int b = 0; b < nrb; ++b) a += p[b * pitch];
    out[i] = a;
}

// ---- the fit's optimiser: one damped Newton step of one problem (include/aecf_hip.h, "optimiser rule")
enum { ST_SCALE = 0, ST_BIAS, ST_L, ST_LAMBDA, ST_G1, ST_G0, ST_H11, ST_H01, ST_H00, ST_PHASE, ST_L0, ST_STEPS };

struct CalOut {
    float es, eb, os, ob;               // what the next sums evaluate, and the accepted parameters
};

__device__ CalOut cal_step(int mode, const double* S, double* st, int64_t pitch, float es_in, float eb_in) {
    double v[CAL_STATE_K];
    for (int k = 0; k < CAL_STATE_K; ++k) v[k] = st[k * pitch];
    const double ts = (double)es_in, tb = (double)eb_in;
    int phase = (int)v[ST_PHASE];
    bool take = false;
    if (phase == 0) {
        v[ST_LAMBDA] = 1e-3;
        v[ST_L0] = S[0];
        v[ST_L] = S[0];
        v[ST_STEPS] = 0.0;
        if (!(S[6] > 0.0 && S[7] > 0.0 && S[7] < S[6])) {           // no element, no positive or no negative: not fitted
            phase = 3;
            v[ST_SCALE] = 1.0;
            v[ST_BIAS] = 0.0;
        } else {
            phase = 1;
            take = true;
        }
    } else if (phase == 1) {
        if (S[0] <= v[ST_L] + 6.103515625e-05 * fabs(v[ST_L])) {    // accepted: not above the accepted L beyond 2^-14 of it, the
                                                                    // float32 noise of two L (a NaN is not)
            const double ds = fabs(ts - v[ST_SCALE]), db = fabs(tb - v[ST_BIAS]);
            const double tol = 9.5367431640625e-07;                 // 2^-20
            const bool small = ds <= tol * fmax(1.0, fabs(ts)) && db <= tol * fmax(1.0, fabs(tb));
            v[ST_LAMBDA] = fmax(v[ST_LAMBDA] * 0.1, 1e-9);
            v[ST_STEPS] += 1.0;
            take = true;
            if (small) phase = 2;
        } else {
            v[ST_LAMBDA] = fmin(v[ST_LAMBDA] * 10.0, 1e12);
        }
    }
    if (take) {
        v[ST_SCALE] = ts; v[ST_BIAS] = tb; v[ST_L] = fmin(S[0], v[ST_L]);
        v[ST_G1] = S[1]; v[ST_G0] = S[2]; v[ST_H11] = S[3]; v[ST_H01] = S[4]; v[ST_H00] = S[5];
    }
    CalOut o;
    o.os = (float)v[ST_SCALE];
    o.ob = (float)v[ST_BIAS];
    o.es = o.os;
    o.eb = o.ob;
    if (phase == 1) {
        const double lam = 1.0 + v[ST_LAMBDA];
        double dscale = 0.0, dbias = 0.0;
        if (mode == AECF_MLCAL_PLATT) {
            const double a = v[ST_H11] * lam, d = v[ST_H00] * lam, b = v[ST_H01];
            const double det = a * d - b * b;
            if (det > 0.0) {
                dscale = -(d * v[ST_G1] - b * v[ST_G0]) / det;
                dbias = -(a * v[ST_G0] - b * v[ST_G1]) / det;
            }
        } else {
            const double a = v[ST_H11] * lam;
            if (a > 0.0) dscale = -v[ST_G1] / a;
        }
        double ns = v[ST_SCALE] + dscale, nb = v[ST_BIAS] + dbias;
        if (!(ns == ns)) ns = v[ST_SCALE];
        if (!(nb == nb)) nb = v[ST_BIAS];
        ns = fmin(fmax(ns, 1.0 / 64.0), 64.0);
        nb = fmin(fmax(nb, -16.0), 16.0);
        o.es = (float)ns;
        o.eb = (float)nb;
    }
    v[ST_PHASE] = (double)phase;
    for (int k = 0; k < CAL_STATE_K; ++k) st[k * pitch] = v[k];
    return o;
}

// per-class problems: one lane per class
__global__ __launch_bounds__(256) void cal_update_class_kernel(int C, int mode, const double* __restrict__ sums, double* __restrict__ state,
                                                               float* __restrict__ scale_eval, float* __restrict__ bias_eval,
                                                               float* __restrict__ scale_out, float* __restrict__ bias_out) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double S[CAL_FIT_K];
    for (int k = 0; k < CAL_FIT_K; ++k) S[k] = sums[(int64_t)k * C + c];
    const CalOut o = cal_step(mode, S, state + c, C, scale_eval[c], bias_eval[c]);
    scale_eval[c] = o.es;
    bias_eval[c] = o.eb;
    scale_out[c] = o.os;
    bias_out[c] = o.ob;
}

// the shared temperature: ONE problem on the classes' sums added in class order; its state is column 0
__global__ __launch_bounds__(256) void cal_update_shared_kernel(int C, const double* __restrict__ sums, double* __restrict__ state,
                                                                float* __restrict__ scale_eval, float* __restrict__ bias_eval,
                                                                float* __restrict__ scale_out, float* __restrict__ bias_out) {
    __shared__ double tot[CAL_FIT_K];
    __shared__ float res[2];
    const int t = threadIdx.x;
    if (t < CAL_FIT_K) {
        double a = 0.0;
#pragma unroll 8
        for (int c = 0; c < C; ++c) a += sums[(int64_t)t * C + c];
        tot[t] = a;
    }
    __syncthreads();
    if (t == 0) {
        double S[CAL_FIT_K];
        for (int k = 0; k < CAL_FIT_K; ++k) S[k] = tot[k];
        const CalOut o = cal_step(AECF_MLCAL_TEMPERATURE, S, state, C, scale_eval[0], 0.0f);
        res[0] = o.es;
        res[1] = o.os;
    }
    __syncthreads();
    for (int c = t; c < C; c += 256) {
        scale_eval[c] = res[0];
        bias_eval[c] = 0.0f;
        scale_out[c] = res[1];
        bias_out[c] = 0.0f;
    }
}

inline int cal_stats_vec(int VV, int B, bool aligned, int C) {
    if (!aligned) return 1;
    int V = VV;
    while (V > 1 && (V * B > CAL_SLOTS / 64 || C % V != 0)) V /= 2;
    return V >= 4 ? V : 1;
}

inline int cal_stats_lanes(int V, int B) {
    int tn = (CAL_SLOTS / (V * B)) & ~63;
    if (tn > CAL_T) tn = CAL_T;
    return tn;
}

template <typename T, int V>
void cal_stats_go(int64_t n, int C, const void* logits, const void* labels, int lkind, const float* scale, const float* bias,
                  const CalEdges& edges, int B, double* part, hipStream_t s) {
    typedef typename Tr<T>::elem E;
    const CalGeo g = cal_geo(n, C, V, cal_stats_lanes(V, B));
    const dim3 grid((unsigned)g.nrb, (unsigned)g.gy);
    const size_t lds = (size_t)2 * B * V * g.tn * sizeof(float);
    cal_stats_kernel<T, V><<<grid, dim3(g.tn), lds, s>>>((const E*)logits, labels, lkind, scale, bias, edges, B, n, C, g.ncg, g.rpi,
                                                        g.rows_pb, part);
}

template <typename T>
void cal_stats_launch(int64_t n, int C, const void* logits, const void* labels, int lkind, const float* scale, const float* bias,
                      const CalEdges& edges, int B, double* part, hipStream_t s) {
    constexpr int VV = 16 / sizeof(typename Tr<T>::elem);
    const int V = cal_stats_vec(VV, B, al16(logits) && al16(labels), C);
    if (V == 8) {
        if constexpr (VV == 8) cal_stats_go<T, 8>(n, C, logits, labels, lkind, scale, bias, edges, B, part, s);
    } else if (V == 4) {
        cal_stats_go<T, 4>(n, C, logits, labels, lkind, scale, bias, edges, B, part, s);
    } else {
        cal_stats_go<T, 1>(n, C, logits, labels, lkind, scale, bias, edges, B, part, s);
    }
}

template <typename T>
void cal_fit_launch(int64_t n, int C, const void* logits, const void* labels, int lkind, const float* scale, const float* bias,
                    double* part, hipStream_t s) {
    typedef typename Tr<T>::elem E;
    constexpr int VV = 16 / sizeof(E);
    const bool vec = C % VV == 0 && al16(logits) && al16(labels);
    const CalGeo g = cal_geo(n, C, vec ? VV : 1, CAL_T);
    const dim3 grid((unsigned)g.nrb, (unsigned)g.gy);
    if (vec)
        cal_fit_kernel<T, VV><<<grid, dim3(CAL_T), 0, s>>>((const E*)logits, labels, lkind, scale, bias, n, C, g.ncg, g.rpi, g.rows_pb, part);
    else
        cal_fit_kernel<T, 1><<<grid, dim3(CAL_T), 0, s>>>((const E*)logits, labels, lkind, scale, bias, n, C, g.ncg, g.rpi, g.rows_pb, part);
}

inline bool cal_supported(int64_t n, int classes) { return classes <= 4096 && n <= (1ll << 30) && n * classes <= (1ll << 30); }

inline size_t cal_workspace(int64_t n, int classes, int bins) {
    int nrb;
    int64_t rows_pb;
    cal_row_blocks(n, classes, nrb, rows_pb);
    const int k = 3 * bins + 5 > CAL_FIT_K ? 3 * bins + 5 : CAL_FIT_K;
    return al256((size_t)nrb * k * classes * 8);
}

inline int cal_status() { return hipGetLastError() == hipSuccess ? AECF_OK : AECF_ERR_LAUNCH; }

// sizes first (BAD_DIMS), then the limits and the two dtype codes (UNSUPPORTED)
inline int cal_check(int64_t n, int32_t classes, int32_t dtype, int32_t label_dtype) {
    if (n <= 0 || classes <= 0) return AECF_ERR_BAD_DIMS;
    if (!cal_supported(n, classes)) return AECF_ERR_UNSUPPORTED;
    if (dtype != AECF_BF16 && dtype != AECF_F32 && dtype != AECF_F16) return AECF_ERR_UNSUPPORTED;
    if (label_dtype < AECF_BF16 || label_dtype > AECF_MLLOSS_I8) return AECF_ERR_UNSUPPORTED;
    return AECF_OK;
}

}  // namespace

}  // namespace aecf

using namespace aecf;

extern "C" {

size_t aecf_mlcal_workspace_bytes(int64_t n, int32_t classes, int32_t bins) {
    if (n <= 0 || classes <= 0 || bins < 1 || bins > AECF_MLCAL_MAX_BINS || !cal_supported(n, classes)) return 0;
    return cal_workspace(n, classes, bins);
}

int aecf_mlcal_stats(int64_t n, int32_t classes, int32_t dtype, int32_t label_dtype, const void* logits, const void* labels,
                     const float* scale, const float* bias, int32_t bins, const float* edges, double* stats, void* workspace,
                     size_t workspace_bytes, void* stream) {
    if (n <= 0 || classes <= 0 || bins < 1 || bins > AECF_MLCAL_MAX_BINS) return AECF_ERR_BAD_DIMS;
    const int st = cal_check(n, classes, dtype, label_dtype);
    if (st != AECF_OK) return st;
    if (!logits || !labels || !stats || !workspace || (bins > 1 && !edges)) return AECF_ERR_NULL_POINTER;
    CalEdges e;
    for (int i = 0; i < AECF_MLCAL_MAX_BINS - 1; ++i) e.e[i] = INFINITY;
    for (int i = 0; i < bins - 1; ++i) {
        e.e[i] = edges[i];
        if (edges[i] != edges[i] || (i > 0 && !(edges[i] >= edges[i - 1]))) return AECF_ERR_BAD_DIMS;
    }
    if (workspace_bytes < cal_workspace(n, classes, bins)) return AECF_ERR_WORKSPACE;
    int nrb;
    int64_t rows_pb;
    cal_row_blocks(n, classes, nrb, rows_pb);
    double* part = (double*)workspace;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == AECF_F32)
        cal_stats_launch<F32>(n, classes, logits, labels, label_dtype, scale, bias, e, bins, part, s);
    else if (dtype == AECF_F16)
        cal_stats_launch<F16>(n, classes, logits, labels, label_dtype, scale, bias, e, bins, part, s);
    else
        cal_stats_launch<BF16>(n, classes, logits, labels, label_dtype, scale, bias, e, bins, part, s);
    const int K = 3 * bins + 5;
    const int64_t items = (int64_t)K * classes;
    cal_finalize_kernel<<<dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s>>>(part, K, classes, nrb, stats);
    return cal_status();
}

int aecf_mlcal_fit_sums(int64_t n, int32_t classes, int32_t dtype, int32_t label_dtype, const void* logits, const void* labels,
                        const float* scale, const float* bias, double* sums, void* workspace, size_t workspace_bytes, void* stream) {
    const int st = cal_check(n, classes, dtype, label_dtype);
    if (st != AECF_OK) return st;
    if (!logits || !labels || !sums || !workspace) return AECF_ERR_NULL_POINTER;
    if (workspace_bytes < cal_workspace(n, classes, 1)) return AECF_ERR_WORKSPACE;
    int nrb;
    int64_t rows_pb;
    cal_row_blocks(n, classes, nrb, rows_pb);
    double* part = (double*)workspace;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == AECF_F32)
        cal_fit_launch<F32>(n, classes, logits, labels, label_dtype, scale, bias, part, s);
    else if (dtype == AECF_F16)
        cal_fit_launch<F16>(n, classes, logits, labels, label_dtype, scale, bias, part, s);
    else
        cal_fit_launch<BF16>(n, classes, logits, labels, label_dtype, scale, bias, part, s);
    const int64_t items = (int64_t)CAL_FIT_K * classes;
    cal_finalize_kernel<<<dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s>>>(part, CAL_FIT_K, classes, nrb, sums);
    return cal_status();
}

int aecf_mlcal_fit_update(int32_t classes, int32_t mode, const double* sums, double* state, float* scale_eval, float* bias_eval,
                          float* scale_out, float* bias_out, void* stream) {
    if (classes <= 0) return AECF_ERR_BAD_DIMS;
    if (mode != AECF_MLCAL_TEMPERATURE && mode != AECF_MLCAL_CLASS_TEMPERATURE && mode != AECF_MLCAL_PLATT) return AECF_ERR_BAD_DIMS;
    if (classes > 4096) return AECF_ERR_UNSUPPORTED;
    if (!sums || !state || !scale_eval || !bias_eval || !scale_out || !bias_out) return AECF_ERR_NULL_POINTER;
    hipStream_t s = (hipStream_t)stream;
    if (mode == AECF_MLCAL_TEMPERATURE)
        cal_update_shared_kernel<<<dim3(1), dim3(256), 0, s>>>(classes, sums, state, scale_eval, bias_eval, scale_out, bias_out);
    else
        cal_update_class_kernel<<<dim3((unsigned)((classes + 255) / 256)), dim3(256), 0, s>>>(classes, mode, sums, state, scale_eval,
                                                                                             bias_eval, scale_out, bias_out);
    return cal_status();
}

}  // extern "C"
