// Streaming pairwise sigmoid (SigLIP) loss, bf16, gfx950 (aecf_sig_stream_fwd_bwd): loss rows and every gradient without the
// [rows, cols] block of g that the tile-GEMM form (aecf_nce_gemm.hip, EPI_SIG) keeps between its two calls -- workspace
// O(rows d) instead of O(rows cols) (8192 x 65536: 1 GB of bf16 g).
//
//   l_ij = a_i.b_j / Tc + bias        g_ij = sigmoid(l_ij) - [j = row_offset + i]        loss_i = sum_j softplus(-y_ij l_ij)
//   da_i = coef/Tc sum_j g_ij b_j     db_j = coef/Tc sum_i g_ij a_i     dbias = sum_ij g_ij     dT = -(1/Tc) sum_i a_i.da_i
//
// The kernel has the shape of nce_flash_kernel (aecf_nce_flash.hip): a block keeps 64 stationary rows (4 waves x 16) as MFMA B
// operands in registers and streams 32-row tiles of the other matrix through LDS (LDS-DMA, two buffers).  Per 16 x 16 sub-tile
//   S[s, t]     = streamed_s . stationary_t                (16x16x32 MFMAs over d)
//   g[s, t]     from S: every logit is its own term -- no running maximum, no normaliser, nothing handed between the roles
//   Out^T[c, t] += streamed^T[c, s] g[s, t]                (16x16x16 MFMAs; g, rounded to bf16 HERE and nowhere else, sits in
//                                                           the accumulator layout that is this instruction's B operand)
// DA (stationary = local rows of a, streamed = all rows of b): the column range is split over the blocks of a row block so
// that the grid fills the chip; every split writes its partial da rows and its per-row float32 sums of softplus and of g, and
// sig_flash_combine_kernel adds the splits in order, applies coef / Tc and leaves per-row sum g and a_i.da_i for the one-block
// sig_flash_scalars_kernel (dbias, dT).  DB (stationary = rows of b, streamed = local rows of a): one pass, no partials, coef /
// Tc applied to the float32 sums in the epilogue.  GRADS = false is the loss-only mode: the DA role without its second
// product, then the same combine -- the loss rows are the same float operations in the same order either way.  No float
// atomics anywhere.
//
// Registers: nothing rescales the 16 x D float32 accumulator, so the DA role needs no more column splits than the DB role
// (InfoNCE's DQ pass needs 2 / 4 at D = 768 / 1024).  Accumulator (D / 4) + stationary fragments (D / 8) per lane are 288 at
// D = 768 and 384 at D = 1024; with the KT fragment reads and the transposed reads of a sub-tile in flight beside them, the
// compiler spills at both widths in either role (D = 768: 130 - 150 registers to scratch inside the loop), so the output
// columns of D = 768 and D = 1024 come from two launches per role (CSPLIT = 2, S recomputed) and every other width from one.
// Every instance is then free of scratch.
#include <math.h>

#include "aecf_kernels.h"
#include "aecf_tile.h"

namespace aecf {

namespace {

typedef short s16x4 __attribute__((ext_vector_type(4)));

enum { SIG_DA = 0, SIG_DB = 1 };

struct SigFlashArgs {
    const unsigned short* stat;     // stationary rows [ns, d]   (DA: a, DB: b)
    const unsigned short* strm;     // streamed rows   [nm, d]   (DA: b, DB: a)
    int64_t ns, nm;
    int64_t row_offset;             // the positive of local row i of a is column row_offset + i of b
    const float* temp;              // device scalars
    const float* bias;
    float min_temp, coef;
    float* part_sp;                 // DA: [KS, ns]     sum_j softplus(-y l) of the split
    float* part_sg;                 // DA: [KS, ns]     sum_j g of the split
    float* part_o;                  // DA: [KS, ns, d]  sum_j g_ij b_j of the split (unscaled)
    float* out;                     // DB: db [ns, d]
    int64_t strm_per_split;         // DA: streamed rows per split (a multiple of 32); no split is empty
};

// sigmoid(x) and softplus(x) for x = n ln 2 in the tile form's arithmetic (sig_terms of aecf_nce_gemm.hip): u = 2^min(n, 126),
// t = 1 + u, r = 1 / t; sigmoid = u r, softplus = ln 2 (log2 t + (n - min(n, 126))) + (u - (t - 1)) r.  The last term hands back
// what the rounding of 1 + u dropped, so softplus keeps its relative accuracy down to u ~ 1e-38; the clamp keeps u finite for
// any |l| (past it sigmoid is 1 and softplus x).  Explicit fmaf only: the loss-only and the gradient instances must not be
// contracted differently.
__device__ __forceinline__ void sig_term(float n, float& sig, float& sp) {
    const float nc = fminf(n, 126.f);
    const float u = __builtin_amdgcn_exp2f(nc);
    const float t = 1.f + u;
    const float r = __builtin_amdgcn_rcpf(t);
    sig = u * r;
    const float lg2 = __builtin_amdgcn_logf(t) + (n - nc);
    const float corr = (u - (t - 1.f)) * r;
    sp = fmaf(0.6931471805599453f, lg2, corr);
}

template <int KT, int ROLE, int CSPLIT, bool GRADS>
__global__ __launch_bounds__(256, 1) void sig_flash_kernel(SigFlashArgs p, int cpart) {
    using X = Tr<BF16>;
    constexpr int D = 32 * KT, NC = GRADS ? D / 16 / CSPLIT : 1, ROWB = 2 * D;
    constexpr int TILE = 32 * ROWB;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const float inv_temp = nce_dev_inv_temp(p.temp, p.min_temp);
    const float s2 = inv_temp * 1.4426950408889634f, b2 = p.bias[0] * 1.4426950408889634f;      // l log2 e = fma(S, s2, b2)
    const int c_first = cpart * NC;

    const int lane = lane_id(), r16 = lane & 15, lg = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(wave_id());
    const int nsb = (int)((p.ns + 63) / 64);
    const int sb = (int)blockIdx.x % nsb, split = (int)blockIdx.x / nsb;
    const int64_t s0 = (int64_t)sb * 64 + 16 * w;                 // this wave's 16 stationary rows
    const int64_t m_beg = ROLE == SIG_DA ? (int64_t)split * p.strm_per_split : 0;
    const int64_t m_end = ROLE == SIG_DA ? ((m_beg + p.strm_per_split) < p.nm ? (m_beg + p.strm_per_split) : p.nm) : p.nm;

    const char* msrc = reinterpret_cast<const char*>(p.strm) + m_beg * (int64_t)ROWB;
    auto issue = [&](int m0, int buf) {               // m0: relative to m_beg
        const int left = (int)(m_end - m_beg) - m0, mv = left < 32 ? left : 32;
        ws_dma_rows_asm<KT, 32, 1, 256>(msrc + m0 * (int64_t)ROWB, (unsigned)ROWB, mv, smem + buf * TILE);
    };
    issue(0, 0);

    // stationary rows as B operands: lane (lg, r16 = t): row s0 + r16, elements 32 ks + 8 lg .. + 7
    u32x4 sreg[KT];
    {
        int64_t srow = s0 + r16;
        srow = srow < p.ns ? srow : p.ns - 1;
        const unsigned short* sp = p.stat + srow * D + 8 * lg;
#pragma unroll
        for (int ks = 0; ks < KT; ++ks) sreg[ks] = *reinterpret_cast<const u32x4*>(sp + 32 * ks);
#pragma unroll
        for (int ks = 0; ks < KT; ++ks) asm volatile("" : "+v"(sreg[ks]));      // retire the loads before the loop
    }
    f32x4 oacc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) oacc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    float sum_sp = 0.f, sum_g = 0.f;                              // DA: this lane's share of stationary row t = r16
    // the streamed index that is this lane's stationary row's positive (DA: a column of b; DB: a local row of a)
    // relative to m_beg, as every streamed index of the loop is (a 32-bit count: cols <= 2^31 - 1); -1: not in this range
    const int64_t pos64 = (ROLE == SIG_DA ? (p.row_offset + s0 + r16) : (s0 + r16 - p.row_offset)) - m_beg;
    const int len = (int)(m_end - m_beg);
    const int pos_t = (pos64 >= 0 && pos64 < (int64_t)len) ? (int)pos64 : -1;

    // fragment / transposed-read addresses inside a tile (rows s, 16-byte chunk ^ (row & 15))
    int aaddr[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) aaddr[v] = r16 * ROWB + ((((4 * v) + lg) ^ r16) << 4);
    const int q = r16 >> 2, pp = r16 & 3;

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    int cur = 0;
    for (int m0 = 0; m0 < len; m0 += 32, cur ^= 1) {
        __builtin_amdgcn_s_barrier();
        if (m0 + 32 < len) issue(m0 + 32, cur ^ 1);
        const char* tb = smem + cur * TILE;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const int a0 = m0 + 16 * sub;                         // streamed rows m_beg + a0 .. + 15 of this sub-tile
            if (a0 >= len) break;                                 // block-uniform
            const char* ts = tb + 16 * sub * ROWB;
            // ---- S[s, t]: A = streamed rows (LDS), B = stationary rows (registers)
            f32x4 sacc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KT; ++ks) {
                const u32x4 af = *reinterpret_cast<const u32x4*>(ts + aaddr[ks & 3] + (ks >> 2) * 256);
                sacc = X::mma(af, sreg[ks], sacc);
            }
            // (the term arithmetic is straight-line code: without the fences the scheduler pulls the next sub-tile's KT fragment
            //  reads and this one's NC transposed reads above it, and the two sets do not fit beside the accumulator)
            __builtin_amdgcn_sched_barrier(0);
            // lane (lg, r16): S[s = a0 + 4 lg + r][t = s0 + r16], r = 0..3.  Streamed rows past the range's end (copies of the last
            // valid one) get g = 0 and enter no sum.
            float gv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int sidx = a0 + 4 * lg + r;
                const bool pos = sidx == pos_t;
                float n = fmaf(sacc[r], s2, b2);
                n = pos ? -n : n;                                 // the positive: softplus(-l) and -sigmoid(-l), formed from -l
                float sig, sp;
                sig_term(n, sig, sp);
                const bool valid = sidx < len;
                const float g = valid ? (pos ? -sig : sig) : 0.f;
                gv[r] = g;
                if (ROLE == SIG_DA) {
                    sum_sp = sum_sp + (valid ? sp : 0.f);
                    sum_g = sum_g + g;
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            if (GRADS) {
                // ---- Out^T[c, t] += streamed^T[c, s] g[s, t]   (16x16x16: B operand = g as it sits in the accumulator)
                const u32x2 pb2 = u32x2{pack_bf16x2(gv[0], gv[1]), pack_bf16x2(gv[2], gv[3])};
                const s16x4 pb = __builtin_bit_cast(s16x4, pb2);
                // A operand: lane (lg, r16 = c): streamed rows 4 lg .. 4 lg + 3 at column 16 ct + r16 -- one transposed read;
                // lane 4 q + pp of the group supplies row 4 lg + q, columns 16 ct + 4 pp .. + 3
                const int trow = 4 * lg + q;
                const int tbase = trow * ROWB + 8 * (pp & 1);
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    const int ch = (2 * (c_first + c) + (pp >> 1)) ^ trow;    // key(row) = row & 15 = trow (16-row sub-tile)
                    const v4i16_t at = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16_t*)(ts + tbase + (ch << 4)));
                    oacc[c] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(s16x4, at), pb, oacc[c], 0, 0, 0);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }

    // ---- epilogue: lane (lg, r16 = t) holds Out[t][16 c + 4 lg + r] and a quarter of row t's scalar sums
    const int64_t t = s0 + r16;
    if (ROLE == SIG_DA) {
        sum_sp = sum_sp + __shfl_xor(sum_sp, 16, 64);
        sum_sp = sum_sp + __shfl_xor(sum_sp, 32, 64);
        sum_g = sum_g + __shfl_xor(sum_g, 16, 64);
        sum_g = sum_g + __shfl_xor(sum_g, 32, 64);
    }
    if (t < p.ns) {
        if (ROLE == SIG_DA) {
            if (GRADS) {
                float* po = p.part_o + ((int64_t)split * p.ns + t) * D + 16 * c_first + 4 * lg;
#pragma unroll
                for (int c = 0; c < NC; ++c) *reinterpret_cast<f32x4*>(po + 16 * c) = oacc[c];
            }
            if (lg == 0 && cpart == 0) {
                p.part_sp[(int64_t)split * p.ns + t] = sum_sp;
                p.part_sg[(int64_t)split * p.ns + t] = sum_g;
            }
        } else {
            const float ct = p.coef * inv_temp;
            float* po = p.out + t * D + 16 * c_first + 4 * lg;
#pragma unroll
            for (int c = 0; c < NC; ++c) *reinterpret_cast<f32x4*>(po + 16 * c) = oacc[c] * ct;
        }
    }
}

// the splits of a row added in order: loss_rows[i]; with da: da_i = coef/Tc sum_s O_s, row_g[i] = sum_j g_ij and
// row_t[i] = a_i . da_i (float32, for sig_flash_scalars_kernel).  One wave per row.
struct SigCombineArgs {
    const unsigned short* a;
    const float* part_sp;
    const float* part_sg;
    const float* part_o;
    float* loss_rows;
    float* da;                      // NULL: loss only
    float* row_g;
    float* row_t;
    int64_t rows;
    int d, ksplit;
    const float* temp;
    float min_temp, coef;
};

__global__ __launch_bounds__(256) void sig_flash_combine_kernel(SigCombineArgs p) {
    const int lane = lane_id();
    const int64_t i = (int64_t)blockIdx.x * 4 + wave_id();
    if (i >= p.rows) return;
    float sp = 0.f, sg = 0.f;
    for (int s = 0; s < p.ksplit; ++s) {
        sp += p.part_sp[(int64_t)s * p.rows + i];
        sg += p.part_sg[(int64_t)s * p.rows + i];
    }
    if (lane == 0) p.loss_rows[i] = sp;
    if (!p.da) return;
    const float ct = p.coef * nce_dev_inv_temp(p.temp, p.min_temp);
    const unsigned short* ap = p.a + i * p.d;
    float tq = 0.f;
    for (int c = lane; c < p.d; c += 64) {
        float o = 0.f;
        for (int s = 0; s < p.ksplit; ++s) o += p.part_o[((int64_t)s * p.rows + i) * p.d + c];
        const float g = ct * o;
        p.da[i * p.d + c] = g;
        tq = fmaf(Tr<BF16>::to_f32(ap[c]), g, tq);
    }
    tq = reduce_wave(tq);
    if (lane == 0) {
        p.row_g[i] = sg;
        p.row_t[i] = tq;
    }
}

// d_bias[0] = sum_i row_g[i], d_t[0] = -(1/Tc) sum_i row_t[i] (0 where *t < min_t): 256 strided partial sums in order, then
// a fixed tree (one block).  d_bias / d_t: NULL = not wanted.
__global__ __launch_bounds__(256) void sig_flash_scalars_kernel(const float* row_g, const float* row_t, int64_t n, const float* t,
                                                                float min_t, float* d_bias, float* d_t) {
    __shared__ float red[2][256];
    float g = 0.f, q = 0.f;
    for (int64_t k = threadIdx.x; k < n; k += 256) {
        g += row_g[k];
        q += row_t[k];
    }
    red[0][threadIdx.x] = g;
    red[1][threadIdx.x] = q;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            red[0][threadIdx.x] += red[0][threadIdx.x + w];
            red[1][threadIdx.x] += red[1][threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (d_bias) d_bias[0] = red[0][0];
        if (d_t) {
            const float tv = *t, tc = fmaxf(tv, min_t);
            d_t[0] = tv >= min_t ? -red[1][0] / tc : 0.f;
        }
    }
}

template <int KT, int ROLE, bool GRADS>
void launch_sig_role(const SigFlashArgs& a, int blocks, hipStream_t s) {
    constexpr int D = 32 * KT;
    constexpr int CSPLIT = GRADS && KT >= 24 ? 2 : 1;
    const size_t smem = (size_t)2 * 32 * 2 * D;
    auto kern = sig_flash_kernel<KT, ROLE, CSPLIT, GRADS>;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    for (int cpart = 0; cpart < CSPLIT; ++cpart) kern<<<dim3((unsigned)blocks), dim3(256), smem, s>>>(a, cpart);
}

// column splits of the DA role: nce_flash_ksplit's rule (enough blocks to fill 256 CUs, at least 512 columns per split, at
// most 64), then the count that the 32-row rounding of the split length leaves non-empty
struct SigSplit {
    int ks;
    int64_t per;
};
SigSplit sig_flash_split(int64_t rows, int64_t cols) {
    const int64_t rb = (rows + 63) / 64;
    int64_t ks = (256 + rb - 1) / rb;
    const int64_t max_ks = (cols + 511) / 512;
    if (ks > max_ks) ks = max_ks;
    if (ks < 1) ks = 1;
    if (ks > 64) ks = 64;
    SigSplit o;
    o.per = ((cols + ks - 1) / ks + 31) / 32 * 32;
    o.ks = (int)((cols + o.per - 1) / o.per);
    return o;
}

}  // namespace

bool sig_flash_supported(int d) { return nce_flash_supported(0, d); }

// [KS, rows, d] da partials (16-byte aligned rows) | [KS, rows] softplus sums | [KS, rows] g sums | [rows] sum g | [rows] a.da
size_t sig_flash_workspace_bytes(int64_t rows, int64_t cols, int d) {
    const int ks = sig_flash_split(rows, cols).ks;
    return ((size_t)ks * rows * (d + 2) + (size_t)2 * rows) * sizeof(float) + 1024;
}

void launch_sig_flash(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, const float* bias, float coef,
                      const void* a, const void* b, float* loss_rows, float* d_bias, float* da, float* db, void* workspace,
                      hipStream_t s) {
    const SigSplit sp = sig_flash_split(rows, cols);
    const int ks = sp.ks;
    float* ws = reinterpret_cast<float*>(workspace);
    float* part_o = ws;
    float* part_sp = part_o + (size_t)ks * rows * d;
    float* part_sg = part_sp + (size_t)ks * rows;
    float* row_g = part_sg + (size_t)ks * rows;
    float* row_t = row_g + rows;
    const bool grads = da != nullptr;
    SigFlashArgs x;
    x.stat = (const unsigned short*)a; x.strm = (const unsigned short*)b; x.ns = rows; x.nm = cols; x.row_offset = row_offset;
    x.temp = dt.t; x.bias = bias; x.min_temp = dt.min_t; x.coef = coef; x.part_sp = part_sp; x.part_sg = part_sg;
    x.part_o = part_o; x.out = nullptr; x.strm_per_split = sp.per;
    SigFlashArgs y = x;
    y.stat = (const unsigned short*)b; y.strm = (const unsigned short*)a; y.ns = cols; y.nm = rows; y.out = db;
    y.strm_per_split = rows;
    SigCombineArgs c;
    c.a = (const unsigned short*)a; c.part_sp = part_sp; c.part_sg = part_sg; c.part_o = part_o; c.loss_rows = loss_rows;
    c.da = da; c.row_g = row_g; c.row_t = row_t; c.rows = rows; c.d = d; c.ksplit = ks; c.temp = dt.t; c.min_temp = dt.min_t;
    c.coef = coef;
    const int da_blocks = (int)(((rows + 63) / 64) * ks), db_blocks = (int)((cols + 63) / 64);
    const dim3 cgrid((unsigned)((rows + 3) / 4));
#define SIG_KT(KT_)                                                                          \
    if (grads) {                                                                             \
        launch_sig_role<KT_, SIG_DA, true>(x, da_blocks, s);                                 \
        sig_flash_combine_kernel<<<cgrid, dim3(256), 0, s>>>(c);                             \
        launch_sig_role<KT_, SIG_DB, true>(y, db_blocks, s);                                 \
    } else {                                                                                 \
        launch_sig_role<KT_, SIG_DA, false>(x, da_blocks, s);                                \
        sig_flash_combine_kernel<<<cgrid, dim3(256), 0, s>>>(c);                             \
    }
    switch (d / 32) {
        case 4: SIG_KT(4) break;
        case 8: SIG_KT(8) break;
        case 12: SIG_KT(12) break;
        case 16: SIG_KT(16) break;
        case 24: SIG_KT(24) break;
        default: SIG_KT(32) break;
    }
#undef SIG_KT
    if (grads && (d_bias || dt.d_t))
        sig_flash_scalars_kernel<<<dim3(1), dim3(256), 0, s>>>(row_g, row_t, rows, dt.t, dt.min_t, d_bias, dt.d_t);
}

}  // namespace aecf
