// Streaming pairwise sigmoid (SigLIP) loss, bf16, gfx950 (aecf_sig_stream_fwd_bwd): loss rows and every gradient without the
// [rows, cols] block of g that the tile-GEMM form (aecf_nce_gemm.hip, EPI_SIG) keeps between its two calls -- workspace
// O(rows d) instead of O(rows cols) (8192 x 65536: 1 GB of bf16 g).
//
//   l_ij = a_i.b_j / Tc + bias        g_ij = sigmoid(l_ij) - [j = row_offset + i]        loss_i = sum_j softplus(-y_ij l_ij)
//   da_i = coef/Tc sum_j g_ij b_j     db_j = coef/Tc sum_i g_ij a_i     dbias = sum_ij g_ij     dT = -(1/Tc) sum_i a_i.da_i
//
// Both roles are the streaming loop of aecf_flash_stream.h (64 stationary rows per block in registers, the other matrix streamed
// through LDS, Out^T[c, t] += streamed^T[c, s] g[s, t]) with this file's term: g[s, t] from S[s, t] alone -- every logit is its
// own term, no running maximum, no normaliser, nothing handed between the roles; g is rounded to bf16 as the B operand of the
// second product and nowhere else.
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
// Every instance is then free of scratch.  (Measured before the loop stated that its range is never empty, which lowered the
// register counts of every role -- profiles/flash_stream_resources.txt; the choice has not been measured again since.)
#include <math.h>

#include "aecf_flash_stream.h"

namespace aecf {

namespace {

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

// g of either role (pos_t: the streamed index that is this lane's stationary row's positive -- DA: a column of b, DB: a local
// row of a -- relative to the range, -1: not in it); SUMS (DA): this lane's share of stationary row t = r16's softplus and g sums.
// Streamed rows past the range's end (copies of the last valid one) get g = 0 and enter no sum.  FENCED: the term arithmetic is
// straight-line code; without the fences the scheduler pulls the next sub-tile's KT fragment reads and this one's NC
// transposed reads above it, and the two sets do not fit beside the accumulator.
template <bool SUMS>
struct SigTerm {
    static constexpr bool FENCED = true;
    float s2, b2;                   // l log2 e = fma(S, s2, b2)
    int pos_t;
    float sum_sp = 0.f, sum_g = 0.f;
    template <int NC>
    __device__ __forceinline__ void weights(const f32x4& sacc, int a0, int lg, int r16, int len, f32x4 (&oacc)[NC], float (&gv)[4]) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int sidx = a0 + 4 * lg + r;
            const bool pos = sidx == pos_t;
            float n = fmaf(sacc[r], s2, b2);
            n = pos ? -n : n;                                     // the positive: softplus(-l) and -sigmoid(-l), formed from -l
            float sig, sp;
            sig_term(n, sig, sp);
            const bool valid = sidx < len;
            const float g = valid ? (pos ? -sig : sig) : 0.f;
            gv[r] = g;
            if (SUMS) {
                sum_sp = sum_sp + (valid ? sp : 0.f);
                sum_g = sum_g + g;
            }
        }
    }
};

template <int KT, int ROLE, int CSPLIT, bool GRADS>
__global__ __launch_bounds__(256, 1) void sig_flash_kernel(SigFlashArgs p, int cpart) {
    constexpr int D = 32 * KT, NC = GRADS ? D / 16 / CSPLIT : 1;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const float inv_temp = nce_dev_inv_temp(p.temp, p.min_temp);
    const int c_first = cpart * NC;
    const FlashBlock f = flash_block<ROLE == SIG_DA>(p.ns, p.nm, p.strm_per_split);
    const int64_t t = f.s0 + f.r16;                               // lane (lg, r16) ends with Out[t][16 c + 4 lg + r]
    SigTerm<ROLE == SIG_DA> term;
    term.s2 = inv_temp * 1.4426950408889634f; term.b2 = p.bias[0] * 1.4426950408889634f;
    term.pos_t = flash_rel(ROLE == SIG_DA ? (p.row_offset + t) : (t - p.row_offset), f);
    f32x4 oacc[NC];
    flash_stream<KT, NC, GRADS>(term, f, p.stat, p.ns, p.strm, c_first, smem, oacc);

    if (ROLE == SIG_DA) {                                         // a lane holds a quarter of row t's scalar sums
        float sum_sp = term.sum_sp, sum_g = term.sum_g;
        sum_sp = sum_sp + __shfl_xor(sum_sp, 16, 64);
        sum_sp = sum_sp + __shfl_xor(sum_sp, 32, 64);
        sum_g = sum_g + __shfl_xor(sum_g, 16, 64);
        sum_g = sum_g + __shfl_xor(sum_g, 32, 64);
        if (t < p.ns) {
            if (GRADS) flash_store<NC, false>(p.part_o + ((int64_t)f.split * p.ns + t) * D, c_first, f.lg, oacc);
            if (f.lg == 0 && cpart == 0) {
                p.part_sp[(int64_t)f.split * p.ns + t] = sum_sp;
                p.part_sg[(int64_t)f.split * p.ns + t] = sum_g;
            }
        }
    } else if (t < p.ns) {
        flash_store<NC, true>(p.out + t * D, c_first, f.lg, oacc, p.coef * inv_temp);
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

}  // namespace

bool sig_flash_supported(int d) { return nce_flash_supported(0, d); }

// [KS, rows, d] da partials (16-byte aligned rows) | [KS, rows] softplus sums | [KS, rows] g sums | [rows] sum g | [rows] a.da
size_t sig_flash_workspace_bytes(int64_t rows, int64_t cols, int d) {
    const int ks = flash_split(rows, cols).live;
    return ((size_t)ks * rows * (d + 2) + (size_t)2 * rows) * sizeof(float) + 1024;
}

void launch_sig_flash(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, const float* bias, float coef,
                      const void* a, const void* b, float* loss_rows, float* d_bias, float* da, float* db, void* workspace,
                      hipStream_t s) {
    const FlashSplit sp = flash_split(rows, cols);
    const int ks = sp.live;
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
    dispatch_kt(d, [&](auto kt) {
        constexpr int KT = decltype(kt)::value;
        if (grads) {
            launch_sig_role<KT, SIG_DA, true>(x, da_blocks, s);
            sig_flash_combine_kernel<<<cgrid, dim3(256), 0, s>>>(c);
            launch_sig_role<KT, SIG_DB, true>(y, db_blocks, s);
        } else {
            launch_sig_role<KT, SIG_DA, false>(x, da_blocks, s);
            sig_flash_combine_kernel<<<cgrid, dim3(256), 0, s>>>(c);
        }
    });
    if (grads && (d_bias || dt.d_t))
        sig_flash_scalars_kernel<<<dim3(1), dim3(256), 0, s>>>(row_g, row_t, rows, dt.t, dt.min_t, d_bias, dt.d_t);
}

}  // namespace aecf
