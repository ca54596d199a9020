// Multi-label evaluation counts, gfx950 (aecf_mlmetrics_prepare / _counts / _finalize): tie-exact average precision, AUROC and
// F1 of logits [n_all, C] against labels [n_all, C] without a sort.
//
// For class c the valid entries are the non-NaN logits; for every valid positive i, over the valid entries j of the class,
//   ge_all_i = #{ s_j >= s_i }   gt_all_i = #{ s_j > s_i }   ge_pos_i, gt_pos_i: the same over the positives only
// and AP_c = (1 / npos) sum_i ge_pos_i / ge_all_i, AUROC_c = sum_i (lt_neg_i + eq_neg_i / 2) / (npos nneg) with
//   lt_neg_i = (nvalid - ge_all_i) - (npos - ge_pos_i)      eq_neg_i = (ge_all_i - gt_all_i) - (ge_pos_i - gt_pos_i).
// The counts are integers: they are the same for any tile, block or rank arrangement.
//
// Order.  The kernels compare the ORDER IMAGE of a float32, a signed integer whose order is the order of the values: -0 is
// taken to +0 first (they tie), a negative float has its magnitude bits inverted, and a NaN -- of either sign -- becomes
// INT_MIN, which lies below the image of -inf.  An anchor is never a NaN, so a NaN key (and the padding of a tile, INT_MIN too)
// is neither >= nor > any anchor: it is counted nowhere, by a select and not by a branch.  Integer compares do not depend on
// the float mode of the wave, so +-inf, +-0 and denormals are ordinary values.
//
// prepare (three launches):
//   mlm_tile_kernel     64 rows x 64 classes through LDS: class-major float32 keys [C][Np] (Np: n_all rounded up to 64; an exact
//                       conversion, rows past n_all are NaN), and per class and 64-row chunk the ballot of the valid positives
//                       (one uint64), their number and the number of valid entries
//   mlm_scan_kernel     one block per class: the chunk numbers -> exclusive offsets (in place); npos, nvalid, ninvalid
//   mlm_compact_kernel  one wave per class and chunk: valid positive r goes to slot offset + (positives below it in its chunk)
//                       of the class's list -- row order, whatever the launch order -- as its key and its row
// counts: block (b, c) of 256 lanes.  Lane t owns row row_offset + 256 b + t for ZEROING (it writes four zeros there unless the
//   row is a valid positive of the class) and anchor p_lo + 256 b + t of the class's list, where [p_lo, p_hi) are the list slots
//   of this rank's rows (from the chunk offsets and a population count, no search); it writes the anchor's four counts at the
//   anchor's row.  Every (class, row) is written by exactly one lane.  Keys are staged 1024 at a time in LDS as order images and
//   read back as 16-byte broadcasts (every lane reads the same address); the inner loop is compare and add-with-carry on
//   integers, no label test: ge_all / gt_all run over all keys, ge_pos / gt_pos over the positive list.
// finalize: one block per class over this rank's rows; lane t takes rows t, t + 256, .. in order, then a fixed tree over the 256
//   lanes.  float64 quotients and sums; a row that is not a valid positive adds an exact 0 through a select (its divisor is 1).
#include "aecf_kernels.h"

namespace aecf {

namespace {

constexpr int MLM_A = 256;          // anchors per block (one per lane)
constexpr int MLM_K = 1024;         // keys per LDS tile
constexpr int MLM_CH = 64;          // rows per chunk of the compaction (one ballot)

inline size_t al256(size_t v) { return (v + 255) / 256 * 256; }

__device__ __forceinline__ int order_image(float v) {
    int b = __float_as_int(v);
    const bool nan = (b & 0x7fffffff) > 0x7f800000;
    b = b == (int)0x80000000 ? 0 : b;
    b ^= (b >> 31) & 0x7fffffff;
    return nan ? (int)0x80000000 : b;
}

__device__ __forceinline__ bool bits_nan(float v) { return (__float_as_int(v) & 0x7fffffff) > 0x7f800000; }

template <typename T>
__global__ __launch_bounds__(256) void mlm_tile_kernel(const typename Tr<T>::elem* __restrict__ logits,
                                                       const unsigned char* __restrict__ labels, int64_t n_all, int C, int64_t Np,
                                                       int64_t nch, float* __restrict__ keys,
                                                       unsigned long long* __restrict__ posmask, int* __restrict__ chunk_pos,
                                                       int* __restrict__ chunk_val) {
    __shared__ float tk[64][65];
    __shared__ unsigned char tl[64][68];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * 64;
    const int c0 = blockIdx.y * 64;
    for (int rr = ty; rr < 64; rr += 4) {
        const int64_t r = r0 + rr;
        const int c = c0 + tx;
        float v = __int_as_float(0x7fc00000);
        unsigned char l = 0;
        if (r < n_all && c < C) {
            v = Tr<T>::to_f32(logits[r * C + c]);
            l = labels[r * C + c] != 0;
        }
        tk[rr][tx] = v;
        tl[rr][tx] = l;
    }
    __syncthreads();
    for (int cc = ty; cc < 64; cc += 4) {
        const int c = c0 + cc;                  // the same for a whole wave
        if (c >= C) break;
        const float v = tk[tx][cc];
        const bool valid = !bits_nan(v);        // (rows past n_all hold NaN)
        const bool pos = valid && tl[tx][cc] != 0;
        const unsigned long long mpos = __ballot(pos), mval = __ballot(valid);
        keys[(int64_t)c * Np + r0 + tx] = v;    // r0 + 63 < Np
        if (tx == 0) {
            posmask[(int64_t)c * nch + blockIdx.x] = mpos;
            chunk_pos[(int64_t)c * nch + blockIdx.x] = __popcll(mpos);
            chunk_val[(int64_t)c * nch + blockIdx.x] = __popcll(mval);
        }
    }
}

// chunk_pos [C][nch]: numbers in, exclusive offsets out.  class_counts [3][C] = npos | nvalid | ninvalid
__global__ __launch_bounds__(256) void mlm_scan_kernel(int* __restrict__ chunk_pos, const int* __restrict__ chunk_val, int64_t n_all,
                                                       int C, int64_t nch, int* __restrict__ class_counts) {
    __shared__ int sp[256];
    __shared__ int sv[256];
    const int c = blockIdx.x, t = threadIdx.x;
    const int64_t per = (nch + 255) / 256;
    const int64_t lo = t * per < nch ? t * per : nch, hi = lo + per < nch ? lo + per : nch;
    int* cp = chunk_pos + (int64_t)c * nch;
    const int* cv = chunk_val + (int64_t)c * nch;
    int p = 0, v = 0;
    for (int64_t i = lo; i < hi; ++i) { p += cp[i]; v += cv[i]; }
    sp[t] = p;
    sv[t] = v;
    __syncthreads();
    if (t == 0) {
        int run = 0, val = 0;
        for (int i = 0; i < 256; ++i) {
            const int x = sp[i];
            sp[i] = run;
            run += x;
            val += sv[i];
        }
        class_counts[c] = run;
        class_counts[C + c] = val;
        class_counts[2 * C + c] = (int)(n_all - val);
    }
    __syncthreads();
    int run = sp[t];
    for (int64_t i = lo; i < hi; ++i) {
        const int x = cp[i];
        cp[i] = run;
        run += x;
    }
}

__global__ __launch_bounds__(256) void mlm_compact_kernel(const float* __restrict__ keys, const unsigned long long* __restrict__ posmask,
                                                          const int* __restrict__ chunk_off, int64_t Np, int64_t nch,
                                                          float* __restrict__ pos_key, int* __restrict__ pos_idx) {
    const int lane = lane_id();
    const int c = blockIdx.y;
    const int64_t ch = (int64_t)blockIdx.x * 4 + wave_id();
    if (ch >= nch) return;
    const unsigned long long mask = posmask[(int64_t)c * nch + ch];
    if (!((mask >> lane) & 1ull)) return;
    const int64_t r = ch * MLM_CH + lane;
    const int d = chunk_off[(int64_t)c * nch + ch] + __popcll(mask & ((1ull << lane) - 1ull));      // < npos <= n_all
    pos_key[(int64_t)c * Np + d] = keys[(int64_t)c * Np + r];
    pos_idx[(int64_t)c * Np + d] = (int)r;
}

// the list slot of the first valid positive at row x or later (x <= n_all)
__device__ __forceinline__ int list_slot(const unsigned long long* mask, const int* off, int64_t nch, int npos, int64_t x) {
    const int64_t ch = x >> 6;
    if (ch >= nch) return npos;
    return off[ch] + __popcll(mask[ch] & ((1ull << (x & 63)) - 1ull));
}

// ge += #{ image(src[j]) >= a }, gt += #{ .. > a } over j < n, src staged through the tile (all lanes of the block take part)
__device__ __forceinline__ void count_keys(const float* __restrict__ src, int n, int a, int* tile, int& ge, int& gt) {
    for (int j0 = 0; j0 < n; j0 += MLM_K) {
        __syncthreads();
        for (int u = threadIdx.x; u < MLM_K; u += 256) {
            const int j = j0 + u;
            const float v = src[j < n ? j : 0];
            tile[u] = j < n ? order_image(v) : (int)0x80000000;
        }
        __syncthreads();
#pragma unroll 4
        for (int u = 0; u < MLM_K; u += 4) {
            const int4 k = *reinterpret_cast<const int4*>(tile + u);
            ge += (k.x >= a) + (k.y >= a) + (k.z >= a) + (k.w >= a);
            gt += (k.x > a) + (k.y > a) + (k.z > a) + (k.w > a);
        }
    }
}

__global__ __launch_bounds__(256) void mlm_counts_kernel(const float* __restrict__ keys, const float* __restrict__ pos_key,
                                                         const int* __restrict__ pos_idx, const unsigned long long* __restrict__ posmask,
                                                         const int* __restrict__ chunk_off, const int* __restrict__ class_counts,
                                                         int64_t n_all, int C, int64_t Np, int64_t nch, int64_t row_offset, int64_t rows,
                                                         int* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) int tile[MLM_K];
    const int c = blockIdx.y, t = threadIdx.x;
    const unsigned long long* mask = posmask + (int64_t)c * nch;
    const int* off = chunk_off + (int64_t)c * nch;
    const int npos = class_counts[c];
    const int64_t plane = (int64_t)C * rows;
    int* o = out + (int64_t)c * rows;
    const int64_t i = (int64_t)blockIdx.x * MLM_A + t;              // this lane's row to zero, local
    if (i < rows) {
        const int64_t r = row_offset + i;
        if (!((mask[r >> 6] >> (r & 63)) & 1ull)) {
            o[i] = 0; o[plane + i] = 0; o[2 * plane + i] = 0; o[3 * plane + i] = 0;
        }
    }
    const int p_lo = list_slot(mask, off, nch, npos, row_offset), p_hi = list_slot(mask, off, nch, npos, row_offset + rows);
    const int64_t p0 = (int64_t)p_lo + (int64_t)blockIdx.x * MLM_A;
    if (p0 >= p_hi) return;                                         // the whole block: no anchors left for it
    const int64_t p = p0 + t;
    const bool active = p < p_hi;
    const int64_t ps = (int64_t)c * Np + (active ? p : p0);
    const int a = order_image(pos_key[ps]);
    const int64_t arow = pos_idx[ps] - row_offset;                  // in [0, rows) for an active lane
    int ge_all = 0, gt_all = 0, ge_pos = 0, gt_pos = 0;
    count_keys(keys + (int64_t)c * Np, (int)n_all, a, tile, ge_all, gt_all);
    count_keys(pos_key + (int64_t)c * Np, npos, a, tile, ge_pos, gt_pos);
    if (active) {
        o[arow] = ge_all; o[plane + arow] = gt_all; o[2 * plane + arow] = ge_pos; o[3 * plane + arow] = gt_pos;
    }
}

__global__ __launch_bounds__(256) void mlm_finalize_kernel(const float* __restrict__ keys, const unsigned long long* __restrict__ posmask,
                                                           const int* __restrict__ class_counts, const int* __restrict__ counts, int C,
                                                           int64_t Np, int64_t nch, int64_t row_offset, int64_t rows, float threshold,
                                                           double* __restrict__ shares) {
    __shared__ double rd[2][256];
    __shared__ int ri[3][256];
    const int c = blockIdx.x, t = threadIdx.x;
    const unsigned long long* mask = posmask + (int64_t)c * nch;
    const float* key = keys + (int64_t)c * Np;
    const int npos = class_counts[c], nvalid = class_counts[C + c];
    const int64_t plane = (int64_t)C * rows;
    const int* cn = counts + (int64_t)c * rows;
    const int thr = order_image(threshold);
    double s_ap = 0.0, s_au = 0.0;
    int tp = 0, fp = 0, fn = 0;
    for (int64_t i = t; i < rows; i += 256) {
        const int64_t r = row_offset + i;
        const bool pos = (mask[r >> 6] >> (r & 63)) & 1ull;         // a valid positive
        const float v = key[r];
        const bool valid = !bits_nan(v);
        const bool pred = valid && order_image(v) > thr;
        const int ge_all = cn[i], gt_all = cn[plane + i], ge_pos = cn[2 * plane + i], gt_pos = cn[3 * plane + i];
        const int lt_neg = (nvalid - ge_all) - (npos - ge_pos), eq_neg = (ge_all - gt_all) - (ge_pos - gt_pos);
        const double q = (double)ge_pos / (double)(pos ? ge_all : 1);
        s_ap += pos ? q : 0.0;
        s_au += pos ? (double)lt_neg + 0.5 * (double)eq_neg : 0.0;
        tp += pos && pred;
        fn += pos && !pred;
        fp += !pos && pred;
    }
    rd[0][t] = s_ap; rd[1][t] = s_au;
    ri[0][t] = tp; ri[1][t] = fp; ri[2][t] = fn;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (t < w) {
            rd[0][t] += rd[0][t + w]; rd[1][t] += rd[1][t + w];
            ri[0][t] += ri[0][t + w]; ri[1][t] += ri[1][t + w]; ri[2][t] += ri[2][t + w];
        }
        __syncthreads();
    }
    if (t == 0) {
        shares[c] = rd[0][0];
        shares[C + c] = rd[1][0];
        shares[2 * C + c] = (double)ri[0][0];
        shares[3 * C + c] = (double)ri[1][0];
        shares[4 * C + c] = (double)ri[2][0];
    }
}

struct MlmWs {
    float* keys;                        // [C][Np]
    float* pos_key;                     // [C][Np]
    int* pos_idx;                       // [C][Np]
    unsigned long long* posmask;        // [C][nch]
    int* chunk_off;                     // [C][nch]
    int* chunk_val;                     // [C][nch]
    int64_t Np, nch;
    size_t bytes;
};

MlmWs mlm_carve(const void* ws, int64_t n_all, int C) {
    MlmWs w;
    w.nch = (n_all + MLM_CH - 1) / MLM_CH;
    w.Np = w.nch * MLM_CH;
    char* p = (char*)ws;
    size_t off = 0;
    auto take = [&](size_t n) { char* r = p + off; off += al256(n); return r; };
    w.keys = (float*)take((size_t)C * w.Np * 4);
    w.pos_key = (float*)take((size_t)C * w.Np * 4);
    w.pos_idx = (int*)take((size_t)C * w.Np * 4);
    w.posmask = (unsigned long long*)take((size_t)C * w.nch * 8);
    w.chunk_off = (int*)take((size_t)C * w.nch * 4);
    w.chunk_val = (int*)take((size_t)C * w.nch * 4);
    w.bytes = off;
    return w;
}

}  // namespace

bool mlmetrics_supported(int64_t n_all, int classes) {
    return classes <= 4096 && n_all <= (1ll << 24) && n_all * classes <= (1ll << 28);
}

size_t mlmetrics_workspace_bytes(int64_t n_all, int classes) { return mlm_carve(nullptr, n_all, classes).bytes; }

MlmPrepared mlmetrics_prepared(const void* workspace, int64_t n_all, int classes) {
    const MlmWs w = mlm_carve(workspace, n_all, classes);
    return MlmPrepared{w.keys, w.posmask, w.Np, w.nch};
}

void launch_mlmetrics_prepare(int64_t n_all, int classes, int dtype, const void* logits, const uint8_t* labels, int32_t* class_counts,
                              void* workspace, hipStream_t s) {
    const MlmWs w = mlm_carve(workspace, n_all, classes);
    const dim3 grid((unsigned)w.nch, (unsigned)((classes + 63) / 64));
    if (dtype == 1)
        mlm_tile_kernel<F32><<<grid, dim3(256), 0, s>>>((const float*)logits, labels, n_all, classes, w.Np, w.nch, w.keys, w.posmask,
                                                        w.chunk_off, w.chunk_val);
    else if (dtype == 2)
        mlm_tile_kernel<F16><<<grid, dim3(256), 0, s>>>((const unsigned short*)logits, labels, n_all, classes, w.Np, w.nch, w.keys,
                                                        w.posmask, w.chunk_off, w.chunk_val);
    else
        mlm_tile_kernel<BF16><<<grid, dim3(256), 0, s>>>((const unsigned short*)logits, labels, n_all, classes, w.Np, w.nch, w.keys,
                                                         w.posmask, w.chunk_off, w.chunk_val);
    mlm_scan_kernel<<<dim3((unsigned)classes), dim3(256), 0, s>>>(w.chunk_off, w.chunk_val, n_all, classes, w.nch, class_counts);
    mlm_compact_kernel<<<dim3((unsigned)((w.nch + 3) / 4), (unsigned)classes), dim3(256), 0, s>>>(w.keys, w.posmask, w.chunk_off, w.Np,
                                                                                                  w.nch, w.pos_key, w.pos_idx);
}

void launch_mlmetrics_counts(int64_t n_all, int classes, int64_t row_offset, int64_t rows, const int32_t* class_counts, int32_t* counts,
                             const void* workspace, hipStream_t s) {
    const MlmWs w = mlm_carve(workspace, n_all, classes);
    mlm_counts_kernel<<<dim3((unsigned)((rows + MLM_A - 1) / MLM_A), (unsigned)classes), dim3(256), 0, s>>>(
        w.keys, w.pos_key, w.pos_idx, w.posmask, w.chunk_off, class_counts, n_all, classes, w.Np, w.nch, row_offset, rows, counts);
}

void launch_mlmetrics_finalize(int64_t n_all, int classes, int64_t row_offset, int64_t rows, float threshold, const int32_t* class_counts,
                               const int32_t* counts, double* shares, const void* workspace, hipStream_t s) {
    const MlmWs w = mlm_carve(workspace, n_all, classes);
    mlm_finalize_kernel<<<dim3((unsigned)classes), dim3(256), 0, s>>>(w.keys, w.posmask, class_counts, counts, classes, w.Np, w.nch,
                                                                       row_offset, rows, threshold, shares);
}

}  // namespace aecf
