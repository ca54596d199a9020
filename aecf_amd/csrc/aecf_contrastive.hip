// Contrastive (InfoNCE) term of the AECF training objective (gfx950).  NOT in the reference:
// build-defined symmetric InfoNCE on L2-normalised fused embeddings with cross-batch (all-gathered) negatives.
//
// One direction, for the local query rows q [b,d] against all keys k [B_all,d] (both unit-norm):
//     S = q k^T (MFMA GEMM, float32 out) ; logits = S / T ; loss_i = logsumexp_j(logits_ij) - logits_{i, off+i}
//     G = (softmax(logits) - onehot) * coef / T              (coef = upstream scale, e.g. 0.5 / B_all)
//     dq = G k            (gemm_nt against k^T)              dk = G^T q   (batch-reduction gemm_tn, rectangular)
// The row kernel below does the softmax / loss / G in three sweeps of a logits row; the GEMMs are the library's
// MFMA kernels.  The symmetric term is the same call with the roles of the two views swapped.
#include "aecf_kernels.h"

namespace aecf {

// z -> z / max(||z||, eps), one wave per row
template <typename T>
__global__ __launch_bounds__(256) void l2norm_fwd_kernel(int64_t n, int d, float eps, const typename Tr<T>::elem* __restrict__ z,
                                                         typename Tr<T>::elem* __restrict__ zn, float* __restrict__ inv_norm) {
    using X = Tr<T>;
    const int64_t row = (int64_t)blockIdx.x * 4 + wave_id();
    if (row >= n) return;
    const int lane = lane_id();
    float ss = 0.f;
    for (int e = lane; e < d; e += 64) { const float v = X::to_f32(z[row * d + e]); ss = fmaf(v, v, ss); }
    ss = reduce_wave(ss);
    const float inv = 1.0f / fmaxf(sqrtf(ss), eps);
    for (int e = lane; e < d; e += 64) zn[row * d + e] = X::from_f32(X::to_f32(z[row * d + e]) * inv);
    if (lane == 0) inv_norm[row] = inv;
}

// dz = (dzn - zn (dzn . zn)) * inv_norm
template <typename T>
__global__ __launch_bounds__(256) void l2norm_bwd_kernel(int64_t n, int d, const typename Tr<T>::elem* __restrict__ zn,
                                                         const float* __restrict__ inv_norm, const float* __restrict__ dzn,
                                                         typename Tr<T>::elem* __restrict__ dz) {
    using X = Tr<T>;
    const int64_t row = (int64_t)blockIdx.x * 4 + wave_id();
    if (row >= n) return;
    const int lane = lane_id();
    float dot = 0.f;
    for (int e = lane; e < d; e += 64) dot = fmaf(dzn[row * d + e], X::to_f32(zn[row * d + e]), dot);
    dot = reduce_wave(dot);
    const float inv = inv_norm[row];
    for (int e = lane; e < d; e += 64)
        dz[row * d + e] = X::from_f32((dzn[row * d + e] - X::to_f32(zn[row * d + e]) * dot) * inv);
}

// l2norm_fwd_kernel over the n = rows * views slots of x [rows][views][d] with a padding mask [n] (non-zero: the slot is absent).
// A present slot is l2norm_fwd_kernel's, operation for operation.  An absent slot is not read: its row is written as +0 and its
// inverse norm as 0, whatever it holds (NaN, inf), so that a zero weight times its key is a zero in the gradient products.  The
// wave of a row's first slot also packs the row's presence byte (bit v: view v present; pres may be NULL).
template <typename T>
__global__ __launch_bounds__(256) void l2norm_masked_fwd_kernel(int64_t n, int d, int views, float eps,
                                                                const typename Tr<T>::elem* __restrict__ z,
                                                                const unsigned char* __restrict__ mask,
                                                                typename Tr<T>::elem* __restrict__ zn, float* __restrict__ inv_norm,
                                                                unsigned char* __restrict__ pres) {
    using X = Tr<T>;
    const int64_t row = (int64_t)blockIdx.x * 4 + wave_id();
    if (row >= n) return;
    const int lane = lane_id();
    const int64_t first = row / views;
    if (pres && first * views == row) {                         // wave-uniform: lane v reads the byte of view v, one vote packs them
        const bool here = lane < views && mask[row + (lane < views ? lane : 0)] == 0;
        const unsigned long long bits = __ballot(here);
        if (lane == 0) pres[first] = (unsigned char)bits;
    }
    if (mask[row]) {
        for (int e = lane; e < d; e += 64) zn[row * d + e] = X::from_f32(0.f);
        if (lane == 0) inv_norm[row] = 0.f;
        return;
    }
    float ss = 0.f;
    for (int e = lane; e < d; e += 64) { const float v = X::to_f32(z[row * d + e]); ss = fmaf(v, v, ss); }
    ss = reduce_wave(ss);
    const float inv = 1.0f / fmaxf(sqrtf(ss), eps);
    for (int e = lane; e < d; e += 64) zn[row * d + e] = X::from_f32(X::to_f32(z[row * d + e]) * inv);
    if (lane == 0) inv_norm[row] = inv;
}

// l2norm_bwd_kernel with the same mask: the gradient of an absent slot is written as +0, whatever arrives
template <typename T>
__global__ __launch_bounds__(256) void l2norm_masked_bwd_kernel(int64_t n, int d, const typename Tr<T>::elem* __restrict__ zn,
                                                                const float* __restrict__ inv_norm, const float* __restrict__ dzn,
                                                                const unsigned char* __restrict__ mask,
                                                                typename Tr<T>::elem* __restrict__ dz) {
    using X = Tr<T>;
    const int64_t row = (int64_t)blockIdx.x * 4 + wave_id();
    if (row >= n) return;
    const int lane = lane_id();
    if (mask[row]) {
        for (int e = lane; e < d; e += 64) dz[row * d + e] = X::from_f32(0.f);
        return;
    }
    float dot = 0.f;
    for (int e = lane; e < d; e += 64) dot = fmaf(dzn[row * d + e], X::to_f32(zn[row * d + e]), dot);
    dot = reduce_wave(dot);
    const float inv = inv_norm[row];
    for (int e = lane; e < d; e += 64)
        dz[row * d + e] = X::from_f32((dzn[row * d + e] - X::to_f32(zn[row * d + e]) * dot) * inv);
}

__device__ __forceinline__ float block_reduce_max(float v, float* red) {
    v = fmaxf(v, __shfl_xor(v, 1, 64)); v = fmaxf(v, __shfl_xor(v, 2, 64)); v = fmaxf(v, __shfl_xor(v, 4, 64));
    v = fmaxf(v, __shfl_xor(v, 8, 64)); v = fmaxf(v, __shfl_xor(v, 16, 64)); v = fmaxf(v, __shfl_xor(v, 32, 64));
    __syncthreads();
    if (lane_id() == 0) red[wave_id()] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}
__device__ __forceinline__ float block_reduce_sum(float v, float* red) {
    v = reduce_wave(v);
    __syncthreads();
    if (lane_id() == 0) red[wave_id()] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// one block per local row.  DT: the temperature comes from the device, and tdot[row] = sum_j G_ij S_ij from the float32 G (the
// row's share of -T dL/dT; tdot = NULL: not wanted)
template <typename T, bool DT>
__global__ __launch_bounds__(256) void nce_rows_kernel(int64_t cols, int64_t row_offset, float inv_temp, float coef,
                                                       const float* __restrict__ S, typename Tr<T>::elem* __restrict__ G,
                                                       float* __restrict__ loss_rows, const float* temp, float min_temp,
                                                       float* __restrict__ tdot) {
    using X = Tr<T>;
    __shared__ float red[4];
    if (DT) inv_temp = nce_dev_inv_temp(temp, min_temp);
    const int64_t row = blockIdx.x;
    const float* s = S + row * cols;
    typename X::elem* g = G + row * cols;
    float mx = -INFINITY;
    for (int64_t j = threadIdx.x; j < cols; j += 256) mx = fmaxf(mx, s[j] * inv_temp);
    mx = block_reduce_max(mx, red);
    float sum = 0.f;
    for (int64_t j = threadIdx.x; j < cols; j += 256) sum += expf(s[j] * inv_temp - mx);
    sum = block_reduce_sum(sum, red);
    const float lse = mx + logf(sum);
    const int64_t pos = row_offset + row;
    const float scale = coef * inv_temp;
    float gs = 0.f;
    for (int64_t j = threadIdx.x; j < cols; j += 256) {
        const float pj = expf(s[j] * inv_temp - lse);
        const float gj = (pj - (j == pos ? 1.0f : 0.0f)) * scale;
        g[j] = X::from_f32(gj);
        if (DT) gs = fmaf(gj, s[j], gs);
    }
    if (threadIdx.x == 0) loss_rows[row] = lse - s[pos] * inv_temp;
    if (DT && tdot) {
        gs = block_reduce_sum(gs, red);
        if (threadIdx.x == 0) tdot[row] = gs;
    }
}

// d_t[0] = -(1/Tc) sum_k part[k * stride] (0 where T < min_t): 256 strided partial sums in order, then a fixed tree
__global__ __launch_bounds__(256) void nce_dtemp_kernel(const float* part, int64_t n, int64_t stride, const float* t, float min_t,
                                                        float* d_t) {
    __shared__ float red[256];
    float s = 0.f;
    for (int64_t k = threadIdx.x; k < n; k += 256) s += part[k * stride];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float tv = *t, tc = fmaxf(tv, min_t);
        d_t[0] = tv >= min_t ? -red[0] / tc : 0.f;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void transpose_rect_kernel(const typename Tr<T>::elem* __restrict__ src,
                                                             typename Tr<T>::elem* __restrict__ dst, int64_t R, int64_t C) {
    __shared__ typename Tr<T>::elem tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int64_t r0 = (int64_t)blockIdx.y * 32, c0 = (int64_t)blockIdx.x * 32;
    for (int r = ty; r < 32; r += 8) tile[r][tx] = src[(r0 + r) * C + c0 + tx];
    __syncthreads();
    for (int r = ty; r < 32; r += 8) dst[(c0 + r) * R + r0 + tx] = tile[tx][r];
}

void launch_l2norm_fwd(int dtype, int64_t n, int d, float eps, const void* z, void* zn, float* inv_norm, hipStream_t s) {
    dim3 grid((unsigned)((n + 3) / 4)), block(256);
    if (dtype == 0) l2norm_fwd_kernel<BF16><<<grid, block, 0, s>>>(n, d, eps, (const unsigned short*)z, (unsigned short*)zn, inv_norm);
    else l2norm_fwd_kernel<F32><<<grid, block, 0, s>>>(n, d, eps, (const float*)z, (float*)zn, inv_norm);
}

void launch_l2norm_masked_fwd(int dtype, int64_t n, int d, int views, float eps, const void* z, const unsigned char* mask, void* zn,
                              float* inv_norm, unsigned char* pres, hipStream_t s) {
    dim3 grid((unsigned)((n + 3) / 4)), block(256);
    if (dtype == 0)
        l2norm_masked_fwd_kernel<BF16><<<grid, block, 0, s>>>(n, d, views, eps, (const unsigned short*)z, mask, (unsigned short*)zn, inv_norm, pres);
    else l2norm_masked_fwd_kernel<F32><<<grid, block, 0, s>>>(n, d, views, eps, (const float*)z, mask, (float*)zn, inv_norm, pres);
}

void launch_l2norm_masked_bwd(int dtype, int64_t n, int d, const void* zn, const float* inv_norm, const float* dzn,
                              const unsigned char* mask, void* dz, hipStream_t s) {
    dim3 grid((unsigned)((n + 3) / 4)), block(256);
    if (dtype == 0)
        l2norm_masked_bwd_kernel<BF16><<<grid, block, 0, s>>>(n, d, (const unsigned short*)zn, inv_norm, dzn, mask, (unsigned short*)dz);
    else l2norm_masked_bwd_kernel<F32><<<grid, block, 0, s>>>(n, d, (const float*)zn, inv_norm, dzn, mask, (float*)dz);
}

void launch_l2norm_bwd(int dtype, int64_t n, int d, const void* zn, const float* inv_norm, const float* dzn, void* dz,
                       hipStream_t s) {
    dim3 grid((unsigned)((n + 3) / 4)), block(256);
    if (dtype == 0) l2norm_bwd_kernel<BF16><<<grid, block, 0, s>>>(n, d, (const unsigned short*)zn, inv_norm, dzn, (unsigned short*)dz);
    else l2norm_bwd_kernel<F32><<<grid, block, 0, s>>>(n, d, (const float*)zn, inv_norm, dzn, (float*)dz);
}

void launch_nce_rows(int dtype, int64_t rows, int64_t cols, int64_t row_offset, float inv_temp, float coef, const float* S,
                     void* G, float* loss_rows, hipStream_t s, const NceDevTemp* dt, float* tdot_scratch) {
    dim3 grid((unsigned)rows), block(256);
    if (dt) {
        float* tdot = dt->d_t ? tdot_scratch : nullptr;
        if (dtype == 0)
            nce_rows_kernel<BF16, true><<<grid, block, 0, s>>>(cols, row_offset, 0.f, coef, S, (unsigned short*)G, loss_rows, dt->t,
                                                               dt->min_t, tdot);
        else nce_rows_kernel<F32, true><<<grid, block, 0, s>>>(cols, row_offset, 0.f, coef, S, (float*)G, loss_rows, dt->t, dt->min_t, tdot);
        if (tdot) launch_nce_dtemp(tdot, rows, 1, *dt, s);
        return;
    }
    if (dtype == 0)
        nce_rows_kernel<BF16, false><<<grid, block, 0, s>>>(cols, row_offset, inv_temp, coef, S, (unsigned short*)G, loss_rows, nullptr,
                                                            0.f, nullptr);
    else nce_rows_kernel<F32, false><<<grid, block, 0, s>>>(cols, row_offset, inv_temp, coef, S, (float*)G, loss_rows, nullptr, 0.f, nullptr);
}

void launch_nce_dtemp(const float* part, int64_t n, int64_t stride, const NceDevTemp& dt, hipStream_t s) {
    nce_dtemp_kernel<<<dim3(1), dim3(256), 0, s>>>(part, n, stride, dt.t, dt.min_t, dt.d_t);
}

void launch_transpose_rect(int dtype, const void* src, void* dst, int64_t R, int64_t C, hipStream_t s) {
    dim3 grid((unsigned)(C / 32), (unsigned)(R / 32)), block(256);
    if (dtype == 0) transpose_rect_kernel<BF16><<<grid, block, 0, s>>>((const unsigned short*)src, (unsigned short*)dst, R, C);
    else transpose_rect_kernel<F32><<<grid, block, 0, s>>>((const float*)src, (float*)dst, R, C);
}

}  // namespace aecf
