// Retrieval ranks of two contrastive views, bf16, gfx950 (aecf_retrieval_positive / aecf_retrieval_ranks).
//
// Local rows a [R, d] against all (gathered) rows b [C, d]; the positive of row i is column off + i.  With s_ij = a_i . b_j
// (float32 accumulation):
//   pos[i]          = s_(i, off + i)                                        retrieval_positive_kernel, one wave per row
//   row_greater[i]  = #{ j < C, j != off + i : s_ij >  pos_row[i] }         row_equal[i]: the same with ==
//   col_greater[j]  = #{ i < R, i != j - off : s_ij >  pos_col[j] }         col_equal[j]: the same with ==   (pos_col NULL: off)
// The column counts are this rank's share over its R rows, for every column: the caller sums the ranks' shares.  A comparison
// with a NaN is false on both sides, so a NaN logit or threshold counts nowhere; nothing more is done about it.
//
// The counting pass is the logits arrangement of nce_gemm_kernel with the EPI_RANK epilogue (aecf_nce_gemm.hip): 2 R C d MFMA
// flops, no exponential, nothing of the tile stored.  Counts leave a block as per-tile int32 partials (greater | equal << 16;
// a tile holds at most 256 of either): [C / 256][Rp] for the rows, [R / 256][Cp] for the columns.  rank_counts_kernel below
// unpacks and adds them in a fixed order.  Partials were taken over vector atomics onto zeroed outputs: it is what the sums of
// the two losses do, needs no memset in front of the GEMM and no atomics contended by the 256 tiles of a row; being integer
// sums, either way gives the same counts in any order.
//
// Top-k retrieval (aecf_retrieval_topk): for every row of a its k <= 16 best columns of b under the total order "higher score
// first, lower column first among equal scores, NaN (all equal) below -inf".  The same logits pass with the EPI_TOPK epilogue
// leaves, per 256 x 256 tile and row, a sorted list of the tile's best k candidates in the workspace [C / 256][Rp][KP] (KP: k
// rounded up to a power of two), each candidate one 64-bit key whose unsigned order IS that order (high word: integer image of
// the score, low word: inverted column; 0 = no candidate).  topk_merge_kernel below takes the best k of a row's lists.  Keys
// are distinct, so the result is the same set in the same order whatever the tile, block or rank arrangement.
#include "aecf_kernels.h"

namespace aecf {

namespace {

constexpr int BT = 256;

inline int64_t up256(int64_t v) { return (v + 255) / 256 * 256; }
inline size_t al256(size_t v) { return (v + 255) / 256 * 256; }

// one wave per local row: pos[i] = a_i . b_(off + i), float32
__global__ __launch_bounds__(256) void retrieval_positive_kernel(const unsigned short* a, const unsigned short* b, int64_t rows,
                                                                 int64_t row_offset, int d, float* pos) {
    const int lane = lane_id();
    const int64_t i = (int64_t)blockIdx.x * 4 + wave_id();
    if (i >= rows) return;
    const unsigned short* ap = a + i * d;
    const unsigned short* bp = b + (row_offset + i) * d;
    float dot = 0.f;
    for (int k = lane; k < d; k += 64) dot = fmaf(Tr<BF16>::to_f32(ap[k]), Tr<BF16>::to_f32(bp[k]), dot);
    dot = reduce_wave(dot);
    if (lane == 0) pos[i] = dot;
}

// greater[e] / equal[e] = sums of the unpacked per-tile partials of element e (four strided partial sums, added in order).
// Block = 64 elements x 4 parts; Rp is a multiple of 64: a block is all rows or all columns.  with_cols == 0: rows only.
__global__ __launch_bounds__(256) void rank_counts_kernel(const int* row_part, const int* col_part, int m_tiles, int n_tiles,
                                                          int64_t rows, int64_t cols, int32_t* row_greater, int32_t* row_equal,
                                                          int32_t* col_greater, int32_t* col_equal) {
    __shared__ int red[2][4][64];
    const int e = threadIdx.x & 63, part = threadIdx.x >> 6;
    const int64_t Rp = (int64_t)m_tiles * BT;
    int64_t id = (int64_t)blockIdx.x * 64 + e;
    const bool is_row = id < Rp;
    if (!is_row) id -= Rp;
    const int* src = is_row ? row_part : col_part;
    const int nt = is_row ? n_tiles : m_tiles, other = is_row ? m_tiles : n_tiles;
    int g = 0, q = 0;
    for (int t = part; t < nt; t += 4) {
        const int v = src[((int64_t)t * other + id / BT) * BT + id % BT];
        g += v & 0xffff;
        q += (int)((unsigned)v >> 16);
    }
    red[0][part][e] = g;
    red[1][part][e] = q;
    __syncthreads();
    if (part == 0) {
        g = (red[0][0][e] + red[0][1][e]) + (red[0][2][e] + red[0][3][e]);
        q = (red[1][0][e] + red[1][1][e]) + (red[1][2][e] + red[1][3][e]);
        if (is_row) {
            if (id < rows) { row_greater[id] = g; row_equal[id] = q; }
        } else if (id < cols) {
            col_greater[id] = g; col_equal[id] = q;
        }
    }
}

// values [R, k] / indices [R, k] = the k largest keys of row i's n_tiles lists, decoded.  One wave per row: a lane takes the tiles
// lane, lane + 64, .. and inserts their candidates into a sorted list of 16 registers (a tile's list is sorted, so its first
// candidate that does not enter ends the tile); then the wave pops the largest of the 64 heads k times.
__global__ __launch_bounds__(256) void topk_merge_kernel(const unsigned long long* part, int n_tiles, int64_t Rp, int kp, int k,
                                                         int64_t rows, float* values, int32_t* indices) {
    typedef unsigned long long u64;
    const int lane = lane_id();
    const int64_t row = (int64_t)blockIdx.x * 4 + wave_id();
    if (row >= rows) return;
    u64 L[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) L[j] = 0ull;
    for (int t = lane; t < n_tiles; t += 64) {
        const u64* src = part + ((int64_t)t * Rp + row) * kp;
        for (int s = 0; s < k; ++s) {
            u64 x = src[s];
            if (x <= L[15]) break;                      // (the sentinel 0 never enters)
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const u64 hi = x > L[j] ? x : L[j], lo = x > L[j] ? L[j] : x;
                L[j] = hi; x = lo;
            }
        }
    }
    for (int t = 0; t < k; ++t) {
        u64 win = L[0];
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const u64 o = __shfl_xor(win, m, 64);
            win = o > win ? o : win;
        }
        if (lane == 0) {
            // the image back to the float: sign bit set = a non-negative score, else the complement; 1 = NaN
            const unsigned int u = (unsigned int)(win >> 32);
            const unsigned int bits = u == 1u ? 0x7fc00000u : ((u & 0x80000000u) ? u ^ 0x80000000u : ~u);
            values[row * k + t] = __uint_as_float(bits);
            indices[row * k + t] = (int32_t)(~(unsigned int)win);
        }
        const bool mine = L[0] == win;
#pragma unroll
        for (int j = 0; j < 15; ++j) L[j] = mine ? L[j + 1] : L[j];
        L[15] = mine ? 0ull : L[15];
    }
}

struct RankWs {
    int* row_part;                      // [n_tiles][Rp]
    int* col_part;                      // [m_tiles][Cp]
    size_t bytes;
};

RankWs rank_carve(void* ws, int64_t rows, int64_t cols) {
    const int64_t Rp = up256(rows), Cp = up256(cols);
    RankWs w;
    char* p = (char*)ws;
    size_t off = 0;
    auto take = [&](size_t n) { char* r = p + off; off += al256(n); return r; };
    w.row_part = (int*)take((size_t)(Cp / BT) * Rp * 4);
    w.col_part = (int*)take((size_t)(Rp / BT) * Cp * 4);
    w.bytes = off;
    return w;
}

}  // namespace

bool retrieval_supported(int d) { return d % 64 == 0 && d >= 64 && d <= 4096; }

size_t retrieval_workspace_bytes(int64_t rows, int64_t cols, int d) { (void)d; return rank_carve(nullptr, rows, cols).bytes; }

void launch_retrieval_positive(int64_t rows, int64_t row_offset, int d, const void* a, const void* b, float* pos_row, hipStream_t s) {
    retrieval_positive_kernel<<<dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s>>>((const unsigned short*)a, (const unsigned short*)b,
                                                                                     rows, row_offset, d, pos_row);
}

void launch_retrieval_ranks(int64_t rows, int64_t cols, int64_t row_offset, int d, const void* a, const void* b, const float* pos_row,
                            const float* pos_col, int32_t* row_greater, int32_t* row_equal, int32_t* col_greater, int32_t* col_equal,
                            void* workspace, hipStream_t s) {
    const RankWs w = rank_carve(workspace, rows, cols);
    const int64_t Rp = up256(rows), Cp = up256(cols);
    launch_rank_gemm(rows, cols, row_offset, d, a, b, pos_row, pos_col, w.row_part, w.col_part, s);
    const int64_t elems = pos_col ? Rp + Cp : Rp;       // the column blocks come after the row blocks: leave them out
    rank_counts_kernel<<<dim3((unsigned)(elems / 64)), dim3(256), 0, s>>>(w.row_part, w.col_part, (int)(Rp / BT), (int)(Cp / BT), rows,
                                                                           cols, row_greater, row_equal, col_greater, col_equal);
}

bool retrieval_topk_supported(int d, int k) { return retrieval_supported(d) && k >= 1 && k <= 16; }

static int topk_pitch(int k) {
    int kp = 1;
    while (kp < k) kp *= 2;
    return kp;
}

size_t retrieval_topk_workspace_bytes(int64_t rows, int64_t cols, int d, int k) {
    (void)d;
    return al256((size_t)(up256(cols) / BT) * (size_t)up256(rows) * (size_t)topk_pitch(k) * 8);
}

void launch_retrieval_topk(int64_t rows, int64_t cols, int64_t row_offset, int d, int k, int exclude_partner, const void* a,
                           const void* b, float* values, int32_t* indices, void* workspace, hipStream_t s) {
    const int64_t Rp = up256(rows), Cp = up256(cols);
    const int kp = topk_pitch(k);
    unsigned long long* part = (unsigned long long*)workspace;
    launch_topk_gemm(rows, cols, row_offset, d, k, kp, exclude_partner, a, b, part, s);
    topk_merge_kernel<<<dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s>>>(part, (int)(Cp / BT), Rp, kp, k, rows, values, indices);
}

}  // namespace aecf
