// Multi-label bootstrap, gfx950 (aecf_mlboot_order / _draw / _walk): R resamples of the rows of logits [n_all, C] against labels
// [n_all, C], walked along ONE order per class, for confidence intervals of average precision, AUROC and F1.
//
// A resample of rows is a vector of integer multiplicities w_j.  The descending order of a class's scores does not depend on it,
// and weighted AP, AUROC and the confusion counts are running sums along that order, so the order is formed once (by counting,
// nothing is sorted) and walked once for all replicates, one LANE per replicate.  Everything up to the final quotients is integer
// arithmetic: a replicate's statistics do not depend on tiles, blocks, ranks or the other replicates.
//
// order: after the evaluation's prepare (aecf_metrics.hip: class-major float32 keys [C][Np] and the ballots of the valid
//   positives), block (b, c) of 256 lanes; lane t owns row r = 256 b + t as an anchor.  Keys are staged 1024 at a time in LDS as
//   order images and read back as 16-byte broadcasts; for a valid anchor gt = #{k : img_k > img_r}, eqb = #{k < r : img_k ==
//   img_r} and slot = gt + eqb, a bijection of the valid rows onto [0, nvalid): the stable descending order.  Tiles wholly before
//   the block's rows count gt and eq, the one tile that holds them counts eq under an index test, tiles after them gt only.  A NaN
//   key is INT_MIN: greater than nothing and equal to no anchor.  The entry at (class, slot) is row | head << 31 | pos << 30 |
//   pred << 29 (head: eqb == 0, the first of its tie group; pred: img_r > image(thr_c)).  Every slot is written exactly once.
// draw: replicate 0 is all ones; replicate r >= 1 makes n_all draws, draw t from philox4x32_10 with key (seed lo, seed hi) and
//   counter (t >> 1 lo, t >> 1 hi, r, 0x626f6f74): value = c[2 (t & 1) + 1] << 32 | c[2 (t & 1)], row = high 64 bits of value *
//   n_all.  The hits are counted with int32 integer atomics in a zeroed scratch [n_all][Rp] (integer adds commute: the same bits
//   on every run) and packed to uint8 W [n_all][Rp]; a count outside 0 .. 255 is clipped and counted in n_saturated.
// walk: block (g, c) is ONE wave; lane l walks replicate 64 g + l.  The order entries are uniform over the wave and read a run of
//   16 ahead; the byte gathers W[row][replicate] of run k + 1 are issued before run k is consumed.  Per tie group the lane
//   accumulates uint32 gall += w, gpos += w pos; at a head it closes the previous group:
//     S += gpos > 0 ? gpos * (GEpos / GEall) : 0   (float64; GEpos = cum_pos + gpos, GEall = cum_all + gall; the divisor of a
//                                                   lane without positive weight is 1, never 0)
//     U2 += (gall - gpos) * (2 cum_pos + gpos)     (uint64; at most 2 Wpos Wneg <= 2^63 for n_all <= 2^24, weights <= 255)
//   The branches (head, "the group holds a positive row") are class data: wave-uniform.
#include "aecf_kernels.h"

namespace aecf {

namespace {

constexpr int MLB_A = 256;          // anchors per block of the order kernel (one per lane)
constexpr int MLB_K = 1024;         // keys per LDS tile
constexpr int MLB_RUN = 16;         // order entries read ahead by the walk
constexpr unsigned int MLB_TAG = 0x626f6f74u;       // "boot": the last counter word of every draw

inline size_t al256(size_t v) { return (v + 255) / 256 * 256; }

__device__ __forceinline__ int order_image(float v) {          // aecf_metrics.hip's: -0 ties +0, NaN is INT_MIN
    int b = __float_as_int(v);
    const bool nan = (b & 0x7fffffff) > 0x7f800000;
    b = b == (int)0x80000000 ? 0 : b;
    b ^= (b >> 31) & 0x7fffffff;
    return nan ? (int)0x80000000 : b;
}

__global__ __launch_bounds__(256) void mlb_order_kernel(const float* __restrict__ keys, const unsigned long long* __restrict__ posmask,
                                                        const float* __restrict__ thr, int64_t n_all, int64_t Np, int64_t nch,
                                                        int* __restrict__ order) {
    __shared__ __attribute__((aligned(16))) int tile[MLB_K];
    const int c = blockIdx.y, t = threadIdx.x;
    const float* key = keys + (int64_t)c * Np;
    const int n = (int)n_all;
    const int own = (int)blockIdx.x * MLB_A;                    // the block's anchors are rows own .. own + 255
    const int r = own + t;
    const int a = r < n ? order_image(key[r]) : (int)0x80000000;
    int gt = 0, eqb = 0;
    for (int j0 = 0; j0 < n; j0 += MLB_K) {
        __syncthreads();
        for (int u = t; u < MLB_K; u += 256) {
            const int j = j0 + u;
            const float v = key[j < n ? j : 0];
            tile[u] = j < n ? order_image(v) : (int)0x80000000;
        }
        __syncthreads();
        if (j0 + MLB_K <= own) {                                // every key of the tile lies before every anchor of the block
#pragma unroll 4
            for (int u = 0; u < MLB_K; u += 4) {
                const int4 k = *reinterpret_cast<const int4*>(tile + u);
                gt += (k.x > a) + (k.y > a) + (k.z > a) + (k.w > a);
                eqb += (k.x == a) + (k.y == a) + (k.z == a) + (k.w == a);
            }
        } else if (j0 >= own + MLB_A) {                         // every key lies after them
#pragma unroll 4
            for (int u = 0; u < MLB_K; u += 4) {
                const int4 k = *reinterpret_cast<const int4*>(tile + u);
                gt += (k.x > a) + (k.y > a) + (k.z > a) + (k.w > a);
            }
        } else {                                                // the one tile that holds the anchors: equal keys BEFORE the row
            const int rl = r - j0;
#pragma unroll 4
            for (int u = 0; u < MLB_K; u += 4) {
                const int4 k = *reinterpret_cast<const int4*>(tile + u);
                gt += (k.x > a) + (k.y > a) + (k.z > a) + (k.w > a);
                eqb += (k.x == a && u < rl) + (k.y == a && u + 1 < rl) + (k.z == a && u + 2 < rl) + (k.w == a && u + 3 < rl);
            }
        }
    }
    if (a == (int)0x80000000) return;                           // a NaN or a row past n_all: no slot
    const bool pos = (posmask[(int64_t)c * nch + (r >> 6)] >> (r & 63)) & 1ull;
    const bool pred = a > order_image(thr[c]);
    const unsigned int e = (unsigned int)r | (eqb == 0 ? 0x80000000u : 0u) | (pos ? 0x40000000u : 0u) | (pred ? 0x20000000u : 0u);
    order[(int64_t)c * Np + gt + eqb] = (int)e;                 // gt + eqb < nvalid <= Np
}

// scratch [n_all][Rp] += the hits of replicate replicate0 + blockIdx.y; lane = one philox call = draws 2 tp and 2 tp + 1
__global__ __launch_bounds__(256) void mlb_draw_kernel(int64_t n_all, int Rp, int64_t replicate0, unsigned int k0, unsigned int k1,
                                                       int* __restrict__ scratch) {
    const int q = blockIdx.y;
    const int64_t r = replicate0 + q;
    if (r == 0) return;                                         // the point estimate: ones, set by the packing
    const int64_t tp = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (2 * tp >= n_all) return;
    unsigned int c[4] = {(unsigned int)tp, (unsigned int)((unsigned long long)tp >> 32), (unsigned int)r, MLB_TAG};
    philox4x32_10(c, k0, k1);
    const unsigned long long v0 = ((unsigned long long)c[1] << 32) | c[0], v1 = ((unsigned long long)c[3] << 32) | c[2];
    const int64_t row0 = (int64_t)__umul64hi(v0, (unsigned long long)n_all);        // < n_all
    atomicAdd(scratch + row0 * Rp + q, 1);
    if (2 * tp + 1 < n_all) {
        const int64_t row1 = (int64_t)__umul64hi(v1, (unsigned long long)n_all);
        atomicAdd(scratch + row1 * Rp + q, 1);
    }
}

// four columns per lane: int32 counts [n_all][Rp] -> uint8 W [n_all][Rp]; columns past `replicates` are 0; DRAWN: replicate 0 is 1
template <bool DRAWN>
__global__ __launch_bounds__(256) void mlb_pack_kernel(const int* __restrict__ counts, int64_t n_all, int Rp, int replicates,
                                                       int64_t replicate0, unsigned int* __restrict__ w, int* __restrict__ n_saturated) {
    const int quads = Rp >> 2;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_all * quads) return;
    const int64_t j = i / quads;
    const int q0 = (int)(i - j * quads) * 4;
    const int4 v = *reinterpret_cast<const int4*>(counts + j * Rp + q0);
    const int in[4] = {v.x, v.y, v.z, v.w};
    unsigned int packed = 0;
    int clipped = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int x = q0 + k < replicates ? in[k] : 0;
        if (DRAWN && replicate0 + q0 + k == 0) x = 1;
        const int y = x < 0 ? 0 : (x > 255 ? 255 : x);
        clipped += y != x;
        packed |= (unsigned int)y << (8 * k);
    }
    w[j * quads + (q0 >> 2)] = packed;
    if (clipped) atomicAdd(n_saturated, clipped);
}

__global__ __launch_bounds__(64) void mlb_walk_kernel(const int* __restrict__ order, const int* __restrict__ class_counts,
                                                      const unsigned char* __restrict__ w, int64_t Np, int Rp, int replicates, int C,
                                                      long long* __restrict__ stats) {
    const int c = blockIdx.y;
    const int col = (int)blockIdx.x * 64 + (int)threadIdx.x;    // < Rp: the grid has Rp / 64 blocks along x
    const int nvalid = class_counts[C + c];                     // <= n_all <= Np
    const int* ord = order + (int64_t)c * Np;
    const unsigned char* wc = w + col;
    unsigned int cum_all = 0, cum_pos = 0, gall = 0, gpos = 0, tp = 0, fp = 0, fn = 0;
    unsigned long long u2 = 0;
    double S = 0.0;
    bool ghas = false;                                          // the open group holds a positive row (wave-uniform)

    auto close_group = [&]() {
        const unsigned int ge_pos = cum_pos + gpos, ge_all = cum_all + gall;
        if (ghas) {
            const double q = (double)ge_pos / (double)(gpos > 0 ? ge_all : 1u);
            S += gpos > 0 ? (double)gpos * q : 0.0;
        }
        u2 += (unsigned long long)(gall - gpos) * (2ull * cum_pos + gpos);
        cum_pos = ge_pos;
        cum_all = ge_all;
        gall = 0;
        gpos = 0;
        ghas = false;
    };
    // entries base .. base + 15 of the class (base a multiple of 16, base + 15 < Np) and this lane's weights of their rows; an
    // entry past nvalid was never written: it reads as row 0 and is not consumed
    auto load_run = [&](int base, unsigned int* e, unsigned int* ww) {
#pragma unroll
        for (int q = 0; q < MLB_RUN; q += 4) {
            const int4 v = *reinterpret_cast<const int4*>(ord + base + q);
            e[q] = v.x; e[q + 1] = v.y; e[q + 2] = v.z; e[q + 3] = v.w;
        }
#pragma unroll
        for (int q = 0; q < MLB_RUN; ++q) {
            e[q] = base + q < nvalid ? e[q] : 0u;
            ww[q] = wc[(int64_t)(e[q] & 0xffffffu) * Rp];
        }
    };

    unsigned int e_cur[MLB_RUN], w_cur[MLB_RUN], e_nxt[MLB_RUN], w_nxt[MLB_RUN];
    if (nvalid > 0) load_run(0, e_cur, w_cur);
    for (int base = 0; base < nvalid; base += MLB_RUN) {
        const bool more = base + MLB_RUN < nvalid;
        if (more) load_run(base + MLB_RUN, e_nxt, w_nxt);
#pragma unroll
        for (int q = 0; q < MLB_RUN; ++q) {
            if (base + q < nvalid) {
                const unsigned int e = e_cur[q], wv = w_cur[q];
                if (e & 0x80000000u) close_group();             // a head: the group before it is complete
                const bool pos = e & 0x40000000u, pred = e & 0x20000000u;
                gall += wv;
                gpos += pos ? wv : 0u;
                ghas = ghas || pos;
                tp += pos && pred ? wv : 0u;
                fp += !pos && pred ? wv : 0u;
                fn += pos && !pred ? wv : 0u;
            }
        }
        if (more) {
#pragma unroll
            for (int q = 0; q < MLB_RUN; ++q) { e_cur[q] = e_nxt[q]; w_cur[q] = w_nxt[q]; }
        }
    }
    close_group();                                              // after the last slot (an empty class closes an empty group)
    if (col < replicates) {
        long long* o = stats + (int64_t)col * 7 * C + c;
        o[0] = (long long)cum_pos;
        o[C] = (long long)cum_all;
        o[2 * C] = (long long)u2;
        o[3 * C] = (long long)tp;
        o[4 * C] = (long long)fp;
        o[5 * C] = (long long)fn;
        o[6 * C] = __double_as_longlong(S);
    }
}

inline int round64(int v) { return (v + 63) / 64 * 64; }

}  // namespace

size_t mlboot_draw_workspace_bytes(int64_t n_all, int replicates) { return al256((size_t)n_all * round64(replicates) * 4); }

void launch_mlboot_order(int64_t n_all, int classes, const float* thr, int32_t* order, const void* workspace, hipStream_t s) {
    const MlmPrepared p = mlmetrics_prepared(workspace, n_all, classes);
    mlb_order_kernel<<<dim3((unsigned)((n_all + MLB_A - 1) / MLB_A), (unsigned)classes), dim3(256), 0, s>>>(p.keys, p.posmask, thr, n_all,
                                                                                                         p.Np, p.nch, order);
}

void launch_mlboot_draw(int64_t n_all, int replicates, int64_t replicate0, uint64_t seed, const int32_t* counts, uint8_t* w,
                        int32_t* n_saturated, void* workspace, hipStream_t s) {
    const int Rp = round64(replicates);
    const unsigned blocks = (unsigned)((n_all * (Rp / 4) + 255) / 256);
    if (counts) {
        mlb_pack_kernel<false><<<dim3(blocks), dim3(256), 0, s>>>(counts, n_all, Rp, replicates, replicate0, (unsigned int*)w, n_saturated);
        return;
    }
    int* scratch = (int*)workspace;
    (void)hipMemsetAsync(scratch, 0, (size_t)n_all * Rp * 4, s);
    const int64_t pairs = (n_all + 1) / 2;
    mlb_draw_kernel<<<dim3((unsigned)((pairs + 255) / 256), (unsigned)replicates), dim3(256), 0, s>>>(
        n_all, Rp, replicate0, (unsigned int)seed, (unsigned int)(seed >> 32), scratch);
    mlb_pack_kernel<true><<<dim3(blocks), dim3(256), 0, s>>>(scratch, n_all, Rp, replicates, replicate0, (unsigned int*)w, n_saturated);
}

void launch_mlboot_walk(int64_t n_all, int classes, int replicates, const int32_t* class_counts, const int32_t* order, const uint8_t* w,
                        int64_t* stats, hipStream_t s) {
    const int Rp = round64(replicates);
    const int64_t Np = (n_all + 63) / 64 * 64;
    mlb_walk_kernel<<<dim3((unsigned)(Rp / 64), (unsigned)classes), dim3(64), 0, s>>>(order, class_counts, w, Np, Rp, replicates, classes,
                                                                                    (long long*)stats);
}

}  // namespace aecf
