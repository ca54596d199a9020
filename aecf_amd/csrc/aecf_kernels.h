// Host-callable launchers of the device kernels (internal to libaecf_hip; the public C ABI is
// include/aecf_hip.h).  Every launcher only enqueues work on `s`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aecf_common.h"

namespace aecf {

constexpr int HPAD = 16;   // heads padded to one MFMA column tile

// ---------------- forward ----------------
// qs[j] = (W_q q + b_q)[j] * scale
void launch_prep_qs(int dtype, const void* w_in, const void* b_in, const void* query, float* qs, int E, float scale,
                    hipStream_t s);
// A[h][k] = sum_{j in head h} qs[j] W_k[j][k]   (f32 [HPAD][E] + dtype hi/lo copies for the MFMA B operand)
void launch_prep_amat(int dtype, const void* w_in, const float* qs, float* a_f32, void* a_hi, void* a_lo, int E, int H,
                      hipStream_t s);
// dst[k][j] = src[j][k]   (E x E, dtype)
void launch_transpose(int dtype, const void* src, void* dst, int E, hipStream_t s);
// up to four fragment-major copies of E x E bf16 weight matrices (optionally of the transpose) for the weight-stationary
// kernels' prologue (aecf_gemm_ws.hip): done by the same prep launch
struct FragJobs {
    int n = 0;
    const void* src[4] = {nullptr, nullptr, nullptr, nullptr};
    void* dst[4] = {nullptr, nullptr, nullptr, nullptr};
    int transposed[4] = {0, 0, 0, 0};
};
// qs, folded key matrix (f32 + hi/lo), up to two E x E transposes (t_src* may be null) and the fragment-major copies
// in one launch
void launch_prep_all(int dtype, const void* w_in, const void* b_in, const void* query, float scale, float* qs, float* a_f32,
                     void* a_hi, void* a_lo, const void* t_src0, void* t_dst0, const void* t_src1, void* t_dst1, int E,
                     int H, const FragJobs& fj, hipStream_t s);

struct GateArgs {
    const void* x;            // [B,M,E]
    const void* a_hi;         // [HPAD,E] dtype
    const void* a_lo;         // [HPAD,E] dtype (16-bit types only)
    const uint8_t* kpm;       // [B,M] or null
    const float* uniforms;    // [B,M] or null
    float* probs;             // [B,H,M]
    float* attn_w;            // [B,M]
    float* masked_w;          // [B,M] or null
    float* entropy;           // [B] or null
    float* mask_rate;         // [B] or null
    void* i_attn_w;           // the same four in the activation dtype (info copies), each may be null
    void* i_masked_w;
    void* i_entropy;
    void* i_mask_rate;
    void* i_target = nullptr; // [B] activation dtype filled with target_value (info['target_entropy']) or null
    float target_value = 0.f;
    float* ent_partial = nullptr;   // [(B + 255) / 256] sums of (nan_to_num(H) - target_value)^2 per 256 rows, or null (gate_stats only)
    PhiloxDraw ph;                  // mask_mode 1 without a uniforms tensor: the kernel draws them itself (aecf_common.h)
    int64_t B;
    int M, E, H;
    MaskCfg mask;
};
void launch_philox_uniforms(int64_t n, const PhiloxDraw& ph, float* out, hipStream_t s);   // out[i] = philox_uniform_at(ph, i)
void launch_gate_fwd(int dtype, const GateArgs& a, hipStream_t s);
void launch_gate_stats(int dtype, const GateArgs& a, hipStream_t s);   // head mean + masking from probs (scores fused elsewhere)

// C[r][n] = sum_k A(r,k) W[n][k] + bias[n]
//   pooled == 0: A(r,k) = a[r*lda + k]
//   pooled == 1: A(r,k) = sum_m probs[r][head(n)][m] * x[r][m][k]   (a = x [R,M,K], head(n) = n / hd)
struct GemmNtArgs {
    const void* a;
    const void* w;       // [N,K] dtype
    const void* bias;    // [N] dtype or null
    void* c;             // [R,N] dtype
    const float* probs;  // [R,H,M] (pooled only)
    int64_t R;
    int N, K;
    int64_t lda;
    int M, H, hd;
    int pooled;
    int out_f32;         // store C as float32 regardless of dtype (logits)
    void* v_out;         // pooled only: [R,M,N] dtype, the per-modality products W x_m + bias (or null)
    // pooled only, optional: produce the softmax weights in the same kernel (scores x . A[h] against the folded key
    // matrix) instead of reading them; probs is then an OUTPUT.  g_ahi == null: off.
    const void* w_frag = nullptr;     // optional fragment-major copy of w (see FragJobs): faster weight prologue
    const void* g_ahi = nullptr;      // [HPAD,K] dtype
    const void* g_alo = nullptr;      // [HPAD,K] dtype
    const uint8_t* g_kpm = nullptr;   // [R,M] or null
    // plain product only, optional side job of the launch's first block (weight-stationary kernel): the entropy regulariser's
    // final sum -- loss = max(sum(ent_partial[0 .. ent_nblk)) * ent_inv_n, 0) in the activation dtype (ref :309-314) -- so that
    // the forward needs no launch of its own for it (the partials come from the statistics kernel that ran before)
    const float* ent_partial = nullptr;
    int ent_nblk = 0;
    float ent_inv_n = 0.f;
    void* ent_loss = nullptr;         // [1] dtype
    // weight-stationary kernel only, optional: the bf16 LOW part of the output, c_lo = bf16(C - float(bf16(C))), same shape as c
    // (AECF_HILO_GRADS: the weight-gradient products then run on hi + lo operand pairs)
    void* c_lo = nullptr;
};
void launch_gemm_nt(int dtype, const GemmNtArgs& a, hipStream_t s);
void launch_vproj(int dtype, const GemmNtArgs& a, hipStream_t s);   // pooled == 1 path
bool gemm_ws_supported(const GemmNtArgs& a);                          // weight-stationary streaming form (bf16)
void launch_gemm_ws(const GemmNtArgs& a, hipStream_t s);

// ---------------- backward ----------------
// g_h[b] = W_v,h^T do_h[b] kernels (aecf_bwd_g.hip):
//   dx == false: da[b,h,m] = g_h[b] . x[b,m] -> ds = softmax-backward(da + dwbar/H) -> dsbuf [B,H,M]
//   dx == true : dx[b,m,k] = sum_h probs[b,h,m] g_h[b][k] + sum_h ds[b,h,m] A[h][k]
struct BwdGArgs {
    const void* x;           // [B,M,E]
    const void* dobuf;       // [B,E] dtype  (dy W_o)
    const void* wvt;         // [E(k), E(j)] dtype = W_v^T
    const float* probs;      // [B,H,M]
    const float* d_attn_w;   // [B,M] or null
    const float* d_entropy;  // [B] or null (eval mode)
    const float* attn_w;     // [B,M] (with d_entropy)
    float* dsbuf;            // [B,H,M]  (written by the da pass, read by the dx pass)
    const float* a_f32;      // [HPAD,E]
    void* dx;                // [B,M,E] dtype
    int64_t B;
    int M, E, H, hd;
    float log_M;
    const void* wvt_frag = nullptr;  // optional fragment-major copy of W_v^T (FragJobs): faster dx weight prologue
    int cu_budget = 0;               // dx_ws2: blocks to launch at most (0 = one per CU, 256); fewer leaves CUs to a collective
    // dx_ws2 side job (optional): u_out[H, E] = sum over the u_nslab slabs [H, E] the score-gradient kernel wrote before this
    // launch -- spread over the launch's blocks, done while their weights load -- so that the finalize launch finds u reduced
    const float* u_slab_in = nullptr;
    float* u_out = nullptr;
    int u_nslab = 0;
    // AECF_HILO_GRADS (dsu_ws_kernel): the low part of dobuf -- the score gradient then forms P from do_hi + do_lo, so that the
    // key-side reduction u (dW_q, dW_k, db_q, dquery hang on it) is float32-accurate as well
    const void* do_lo = nullptr;
};
void launch_bwd_g(int dtype, const BwdGArgs& a, bool dx, hipStream_t s);
// score gradient from the saved value projections: da[b,h,m] = do_h[b] . V_h[b,m]  (memory-bound, one wave per sample)
// returns false when the head size is not supported by this kernel (caller falls back to launch_bwd_g(dx = false))
bool launch_dscore_v(int dtype, const BwdGArgs& a, const void* saved_v, hipStream_t s);
bool launch_dx_ws(const BwdGArgs& a, hipStream_t s);
// score gradient + u = ds^T x straight from x (no saved V), bf16 weight-stationary engine with a head split
// (aecf_gemm_ws.hip: dsu_ws_kernel).  dsu_ws_chunks: number of [H, E] u slabs it will write (0 = shape not taken)
int dsu_ws_chunks(const BwdGArgs& a);
int launch_dsu_ws(const BwdGArgs& a, float* u_slab, hipStream_t s);        // bf16 dx on the weight-stationary engine (aecf_gemm_ws.hip)
bool dsu_ws_takes_lo(const BwdGArgs& a);     // AECF_HILO_GRADS: dsu_ws_kernel forms P from do_hi + do_lo at this shape

// out[split][j][k] = sum_{b in split} lhs[b][j] * rhs(b,k)        (f32 partial slabs, deterministic)
//   pooled == 0: rhs(b,k) = rhs[b*E + k]
//   pooled == 1: rhs(b,k) = sum_m probs[b][head(j)][m] x[b][m][k]
// colsum[split][j] = sum_b lhs[b][j]
// pooled == 1 additionally: u[split][h][k] = sum_{b,m} ds[b,h,m] x[b,m,k]
struct GemmTnArgs {
    const void* lhs;      // [B,E] dtype
    const void* rhs;      // [B,E] dtype or x [B,M,E]
    const float* probs;   // pooled
    const float* dsbuf;   // pooled
    float* out;           // [S,E,E]
    float* colsum;        // [S,E]
    float* u;             // [S,HPAD,E] pooled
    int64_t B;
    int M, E, H, hd;
    int Ej;               // lhs feature count when it differs from E (rectangular, non-pooled); 0 = E
    int splits;           // S
    int64_t rows_per_split;   // multiple of 32
    int u_splits;             // the u kernel has its own (finer) batch split: tiny output, needs more blocks
    int64_t u_rows_per_split;
    int pooled;
    int parts = 0;            // pooled: 0 = main product + u, 1 = main product only, 2 = u only (separate stage timing)
    DqpJob dq;                // bf16 transposed-read kernels only: side job of the launch (aecf_common.h); w_k == null: off
    // AECF_HILO_GRADS (aecf_gemm_tn_hilo.hip): the low parts of the operands that are derived values -- lhs_lo = do_lo (pooled
    // product; the pooled rows are split where they are formed), rhs_lo = o_lo (plain product; its lhs dy is an exact input)
    const void* lhs_lo = nullptr;
    const void* rhs_lo = nullptr;
};
void launch_gemm_tn(int dtype, const GemmTnArgs& a, hipStream_t s);
void launch_gemm_tn_tr(const GemmTnArgs& a, hipStream_t s);   // bf16, ds_read_b64_tr_b16 form (main product only)
bool gemm_tn_hilo_supported(const GemmTnArgs& a);             // hi + lo operand pairs in ONE launch (lhs_lo / rhs_lo set)
void launch_gemm_tn_hilo(const GemmTnArgs& a, hipStream_t s);
bool u_mfma_supported(const GemmTnArgs& a);                    // u = ds^T x on the matrix pipe (bf16, H <= 8, E % 128 == 0)
void launch_u_mfma(const GemmTnArgs& a, hipStream_t s);

// dst[g][i] = sum_s src[g][s*n[g] + i] for each of N segments, one launch
struct ReduceSegs {
    static constexpr int N = 5;
    const float* src[N];
    void* dst[N];
    int64_t n[N];
    int splits[N];
    int dst_gt[N];        // GradType of dst: GRAD_F32, or GRAD_BF16 / GRAD_F16 (one rounding of the float32 sum)
    float scale[N] = {1.f, 1.f, 1.f, 1.f, 1.f};   // the sum is multiplied by this before it is stored (aecf_pool_bwd_args.grad_scale)
};
void launch_reduce_segments(const ReduceSegs& r, hipStream_t s);

// dW_k[j][k] = qs[j] u[h(j)][k];  dqp[j] = scale * sum_k W_k[j][k] u[h(j)][k]
// dW_q[j][k] = dqp[j] q[k]; db_q = dqp; db_k = 0; dquery[k] = sum_j dqp[j] W_q[j][k]
struct FinalizeArgs {
    const void* w_in;
    const void* query;
    const float* qs;
    const float* u;       // [HPAD,E] reduced
    const float* dqp;     // [E] dq' (DqpJob: side job of the dW_v launch, or launch_dqp)
    void* dw_in;          // [3E,E]  float32, or bf16 / f16 (grad_gt)
    void* db_in;          // [3E]
    void* dquery;         // [E]
    int E, H, hd;
    float scale;
    int grad_gt;          // GradType of the five gradients
    float gscale = 1.f;   // every gradient this launch writes is multiplied by it (aecf_pool_bwd_args.grad_scale)
};
void launch_dqp(int dtype, const DqpJob& q, hipStream_t s);        // dq' as its own small launch (shapes without the side job)
void launch_finalize_all(int dtype, const FinalizeArgs& a, const ReduceSegs& r, hipStream_t s);   // slab reduction + the above, ONE launch

// ---------------- stand-alone pieces ----------------
void launch_mask_fwd(int64_t rows, int L, const MaskCfg& cfg, const float* w, const float* u, float* masked,
                     float* entropy, float* mask_rate, uint8_t* bits, hipStream_t s);
void launch_mask_bwd(int64_t rows, int L, int mode, float eps, float log_L, const float* w, const uint8_t* bits,
                     const float* d_masked, const float* d_entropy, float* d_w, hipStream_t s);
// partial[i] = sum over rows 256 i .. of (nan_to_num(H) - target)^2 (one block per 256 rows); loss = max(sum partial, 0) / n
void launch_entropy_partials(int dtype, int64_t n, float target, const void* entropy, float* partial, hipStream_t s);
void launch_entropy_from_partials(int dtype, int64_t n, const float* partial, void* loss, hipStream_t s);
void launch_entropy_loss(int dtype, int64_t n, float target, const void* entropy, float upstream, void* loss,
                         float* d_entropy, float* partial, hipStream_t s);
__device__ __forceinline__ float nan_to_num_ref(float e) {   // nan=0, +inf=1, -inf=0 (ref :296)
    if (e != e) return 0.f;
    if (isinf(e)) return e > 0.f ? 1.f : 0.f;
    return e;
}
// the same regulariser riding in ONE 256-thread block of another launch (the InfoNCE combine / finalize kernels): loss[0] =
// max(mean((nan_to_num(H) - target)^2), 0), d_ent[j] = scale (H_j - target) (0 where H_j is not finite; d_ent may be NULL);
// fixed order: 256 strided sums, a wave reduction, the four waves added in order
__device__ __forceinline__ void entropy_rider(const float* ent, int64_t n_ent, float target, float scale, float* d_ent, float* loss) {
    __shared__ float red[4];
    float acc = 0.f;
    for (int64_t j = threadIdx.x; j < n_ent; j += 256) {
        const float raw = ent[j];
        const float dlt = nan_to_num_ref(raw) - target;
        acc += dlt * dlt;
        if (d_ent) d_ent[j] = isfinite(raw) ? scale * dlt : 0.f;
    }
    acc = reduce_wave(acc);
    if (lane_id() == 0) red[wave_id()] = acc;
    __syncthreads();
    if (threadIdx.x == 0) loss[0] = fmaxf((red[0] + red[1] + red[2] + red[3]) / (float)n_ent, 0.f);
}
void launch_sdpa_fwd(int dtype, int64_t B, int S, int T, int E, float scale, const void* q, const void* k, const void* v,
                     void* out, float* probs, hipStream_t s);
void launch_sdpa_bwd(int dtype, int64_t B, int S, int T, int E, float scale, const void* q, const void* k, const void* v,
                     const float* probs, const void* dout, void* dq, void* dk, void* dv, hipStream_t s);

// ---------------- contrastive (aecf_contrastive.hip) ----------------
// A temperature that lives on the device (the aecf_*_dt entry points): the kernels use Tc = max(*t, min_t), deriving 1/Tc with
// the same float operations the host does for a float T (equal T, equal bits).  d_t (optional, NULL = not wanted) is WRITTEN
// with dL/dT = -(1/Tc) sum_i q_i.dq_i (0 where *t < min_t), reduced in a fixed order from float32 partials.
struct NceDevTemp {
    const float* t;
    float min_t;
    float* d_t;
};
__device__ __forceinline__ float nce_dev_inv_temp(const float* t, float min_t) { return 1.0f / fmaxf(*t, min_t); }
// d_t[0] from n partials part[k * stride] (one block; fixed order)
void launch_nce_dtemp(const float* part, int64_t n, int64_t stride, const NceDevTemp& dt, hipStream_t s);

void launch_l2norm_fwd(int dtype, int64_t n, int d, float eps, const void* z, void* zn, float* inv_norm, hipStream_t s);
void launch_l2norm_bwd(int dtype, int64_t n, int d, const void* zn, const float* inv_norm, const float* dzn, void* dz,
                       hipStream_t s);
// the same over the n = rows * views slots of [rows][views][d] with a padding mask [n] (non-zero: absent): an absent slot comes out
// as a row of +0 with inverse norm 0 (forward) and a gradient of +0 (backward) whatever it holds; pres [n / views] (may be NULL)
// receives the presence byte of every row, bit v = view v present
void launch_l2norm_masked_fwd(int dtype, int64_t n, int d, int views, float eps, const void* z, const unsigned char* mask, void* zn,
                              float* inv_norm, unsigned char* pres, hipStream_t s);
void launch_l2norm_masked_bwd(int dtype, int64_t n, int d, const void* zn, const float* inv_norm, const float* dzn,
                              const unsigned char* mask, void* dz, hipStream_t s);
// per local row i: logits = S[i,:] * inv_temp; loss_rows[i] = logsumexp - logits[row_offset + i];
// G[i,:] = (softmax - onehot) * coef * inv_temp   (dtype)
// dt != NULL: inv_temp comes from the device; with dt->d_t, the rows' sums_j G_ij S_ij go to tdot_scratch [rows] and d_t is
// formed from those (one more single-block launch)
void launch_nce_rows(int dtype, int64_t rows, int64_t cols, int64_t row_offset, float inv_temp, float coef, const float* S,
                     void* G, float* loss_rows, hipStream_t s, const NceDevTemp* dt = nullptr, float* tdot_scratch = nullptr);
// dst[c][r] = src[r][c]   (R x C, dtype; R, C multiples of 32)
void launch_modality_frontend(int dtype, int64_t rows, int dim, const void* feat, const uint8_t* drop, void* out,
                              uint8_t* present, hipStream_t s);
void launch_transpose_rect(int dtype, const void* src, void* dst, int64_t R, int64_t C, hipStream_t s);
void launch_cast_bf16_f32(const void* src, float* dst, int64_t n, hipStream_t s);     // 16-byte aligned src / dst
int launch_cast_f32_bf16_multi(int n, const float* const* src, void* const* dst, const int64_t* numel, hipStream_t s);   // n <= 8
int launch_cast_f32_f16_multi(int n, const float* const* src, void* const* dst, const int64_t* numel, hipStream_t s);    // n <= 8

// flash-style InfoNCE direction (aecf_nce_flash.hip): no [rows, cols] logits; optional entropy regulariser in the same call
bool nce_flash_supported(int dtype, int d);
size_t nce_flash_workspace_bytes(int64_t rows, int64_t cols, int d);
void launch_nce_flash(int64_t rows, int64_t cols, int64_t row_offset, int d, float inv_temp, float coef, const void* q,
                      const void* k, float* loss_rows, float* dq, float* dk, void* workspace, const float* ent, int64_t n_ent,
                      float ent_target, float ent_upstream, float* d_ent, float* ent_loss, hipStream_t s,
                      const NceDevTemp* dt = nullptr);

// InfoNCE on tile GEMMs (aecf_nce_gemm.hip): bf16 exponentials E [rows, cols] in the workspace, one or both directions.
// dt != NULL: the temperature comes from the device (inv_temp is not read); launch_nce_gemm_grads then also writes dt->d_t.
bool nce_gemm_supported(int dtype, int d, float temperature);
size_t nce_gemm_workspace_bytes(int64_t rows, int64_t cols, int d);
void launch_nce_gemm_pass1(int64_t rows, int64_t cols, int d, float inv_temp, const void* a, const void* b, void* workspace,
                           float* col_sums, hipStream_t s, const NceDevTemp* dt = nullptr);
void launch_nce_gemm_loss(int64_t rows, int64_t cols, int64_t row_offset, int d, float inv_temp, int sym, const void* a,
                          const void* b, const float* col_sums, void* workspace, float* loss_rows, const float* ent, int64_t n_ent,
                          float ent_target, float ent_upstream, float* d_ent, float* ent_loss, hipStream_t s,
                          const NceDevTemp* dt = nullptr);
void launch_nce_gemm_grads(int64_t rows, int64_t cols, int64_t row_offset, int d, float inv_temp, float coef, int sym, const void* a,
                           const void* b, void* workspace, const float* upstream, int out_bf16, void* da, void* db, hipStream_t s,
                           const NceDevTemp* dt = nullptr);

// Pairwise sigmoid (SigLIP) loss on the same tile GEMMs (aecf_nce_gemm.hip): g = sigmoid(l) - [positive] as bf16 [rows, cols] in
// the workspace (unscaled: coef / Tc and the upstream gradient are applied to the float32 sums of the gradient GEMMs).
// T and the bias are device scalars; pass 1 writes loss_rows[i] = sum_j softplus(-y_ij l_ij) and d_bias[0] = sum_ij g_ij,
// the gradient call writes dt.d_t when it is given.
bool sig_gemm_supported(int dtype, int d);
size_t sig_gemm_workspace_bytes(int64_t rows, int64_t cols, int d);
void launch_sig_gemm_pass1(int64_t rows, int64_t cols, int64_t row_offset, int d, const float* temp, float min_temp, const float* bias,
                           const void* a, const void* b, void* workspace, float* loss_rows, float* d_bias, hipStream_t s);
void launch_sig_gemm_grads(int64_t rows, int64_t cols, int d, const NceDevTemp& dt, float coef, const void* a, const void* b,
                           void* workspace, const float* upstream, int out_bf16, void* da, void* db, hipStream_t s);

// The same loss without the [rows, cols] block (aecf_sig_flash.hip): both roles stream the other matrix through LDS, workspace
// O(rows d).  Writes loss_rows; with da / db (both or neither) also the gradients at upstream 1, d_bias[0] = sum_ij g_ij and
// dt.d_t (each NULL = not wanted).
bool sig_flash_supported(int d);
size_t sig_flash_workspace_bytes(int64_t rows, int64_t cols, int d);
void launch_sig_flash(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, const float* bias, float coef,
                      const void* a, const void* b, float* loss_rows, float* d_bias, float* da, float* db, void* workspace,
                      hipStream_t s);

// Supervised contrastive loss, streaming (aecf_supcon_flash.hip): every key that carries the query's int64 label is a positive
// beside the partner at row_offset + i; workspace O(rows d).  Writes loss_rows; with dq / dk (both or neither) also the gradients
// at upstream 1 and dt.d_t (NULL = not wanted).
bool supcon_flash_supported(int d);
size_t supcon_flash_workspace_bytes(int64_t rows, int64_t cols, int d);
void launch_supcon_flash(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, float coef, const void* q,
                         const void* k, const int64_t* q_labels, const int64_t* k_labels, float* loss_rows, float* dq, float* dk,
                         void* workspace, hipStream_t s);
// The pooled form (NT-Xent, SupCon over both views): the same passes with key self_offset + i excluded for local row i -- from the
// maximum, the sum, the positives and both gradient products.  Workspace as launch_supcon_flash.
void launch_supcon_pool_flash(int64_t rows, int64_t cols, int64_t row_offset, int64_t self_offset, int d, const NceDevTemp& dt,
                              float coef, const void* q, const void* k, const int64_t* q_labels, const int64_t* k_labels,
                              float* loss_rows, float* dq, float* dk, void* workspace, hipStream_t s);

// Supervised contrastive loss on the tile GEMMs (aecf_nce_gemm.hip): both directions of the symmetric loss from ONE block of
// logits, labels shared by the two views.  The logits pass (EPI_SUP) is InfoNCE's plus the count and the float32 raw-score sum of
// the label matches per row and per column; col_stats [3][cols] (column sums of E | counts | matched sums) is what ranks exchange.
bool supcon_gemm_supported(int d, float min_temperature, int64_t cols);
size_t supcon_gemm_workspace_bytes(int64_t rows, int64_t cols, int d);
void launch_supcon_gemm_pass1(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, const void* a, const void* b,
                              const int64_t* row_labels, const int64_t* col_labels, void* workspace, float* col_stats, hipStream_t s);
void launch_supcon_gemm_loss(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, const void* a, const void* b,
                             const float* col_stats, void* workspace, float* loss_rows, hipStream_t s);
void launch_supcon_gemm_grads(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, float coef, const void* a,
                              const void* b, const int64_t* row_labels, const int64_t* col_labels, void* workspace,
                              const float* upstream, int out_bf16, void* da, void* db, hipStream_t s);

// The same with class sets (one uint64 per row) and the overlap (jaccard 0) or Jaccard (jaccard 1) weight in place of the match:
// dense weights, so a dense epilogue of its own (EPI_SETS_OV / EPI_SETS_JAC) and set_weights_kernel; workspace, supported shapes
// and loss pass are those above (col_stats: column sums of E | sums of w | sums of w * raw score).
void launch_supcon_ml_gemm_pass1(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, const void* a,
                                 const void* b, const uint64_t* row_sets, const uint64_t* col_sets, int jaccard, void* workspace,
                                 float* col_stats, hipStream_t s);
void launch_supcon_ml_gemm_grads(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, float coef,
                                 const void* a, const void* b, const uint64_t* row_sets, const uint64_t* col_sets, int jaccard,
                                 void* workspace, const float* upstream, int out_bf16, void* da, void* db, hipStream_t s);

// NT-Xent on the tile GEMMs (aecf_nce_gemm.hip): the 2 rows anchors of one rank from three logits blocks -- X = a_loc . b_all^T
// (InfoNCE's pass 1), Y = a_loc . a_all^T and Z = b_loc . b_all^T with the anchor itself (column row_offset + i) left out by index
// (EPI_EXP_SELF).  col_sums [cols] (the column sums of X, plus the row sums of Z on this rank's own range) is what ranks exchange.
bool ntxent_gemm_supported(int d, float min_temperature);
size_t ntxent_gemm_workspace_bytes(int64_t rows, int64_t cols, int d);
void launch_ntxent_gemm_pass1(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, const void* a_loc,
                              const void* b_loc, const void* a_all, const void* b_all, void* workspace, float* col_sums, hipStream_t s);
void launch_ntxent_gemm_loss(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, const void* a_loc,
                             const void* b_all, const float* col_sums, void* workspace, float* loss_rows, hipStream_t s);
void launch_ntxent_gemm_grads(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, float coef, const void* a_loc,
                              const void* b_loc, const void* a_all, const void* b_all, void* workspace, const float* upstream,
                              int out_bf16, void* d_a_loc, void* d_b_loc, void* d_a_all, void* d_b_all, hipStream_t s);

// Symmetric InfoNCE with a key queue on the tile GEMMs (aecf_nce_gemm.hip): X = a_loc . b_all^T (InfoNCE's pass 1) and two blocks
// against stored keys, U = a_loc . Qb^T and W = b_loc . Qa^T, of which the columns below the device count *q_valid are negatives
// (EPI_EXP_Q: the others left out by index).  col_sums [cols] (the column sums of X, plus the row sums of W on this rank's own
// range) is what ranks exchange.  The queues take no gradient.  launch_key_queue_push fills the ring buffers on the device:
// state = (cursor, valid), int64, never read on the host.
bool nce_queue_gemm_supported(int d, float min_temperature);
size_t nce_queue_gemm_workspace_bytes(int64_t rows, int64_t cols, int64_t q_cap, int d);
void launch_nce_queue_gemm_pass1(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, const void* a_loc,
                                 const void* b_loc, const void* b_all, const void* qa, const void* qb, int64_t q_cap,
                                 const int64_t* q_valid, void* workspace, float* col_sums, hipStream_t s);
void launch_nce_queue_gemm_loss(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, const void* a_loc,
                                const void* b_all, int64_t q_cap, const float* col_sums, void* workspace, float* loss_rows,
                                hipStream_t s);
void launch_nce_queue_gemm_grads(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, float coef,
                                 const void* a_loc, const void* b_loc, const void* b_all, const void* qa, const void* qb,
                                 int64_t q_cap, void* workspace, const float* upstream, int out_bf16, void* d_a_loc, void* d_b_loc,
                                 void* d_b_all, hipStream_t s);
void launch_key_queue_push(int64_t q_cap, int d, int64_t n, const void* src_a, const void* src_b, void* qa, void* qb, int64_t* state,
                           hipStream_t s);

// Supervised contrastive loss with a key queue on the tile GEMMs (aecf_nce_gemm.hip): the three blocks above with label positives.
// X runs EPI_SUP; U and W run EPI_SUP_Q against the ring of stored labels q_labels [q_cap] (rows only; a slot at or above *q_valid
// is no key and no positive, by index).  col_stats [3][cols] (X's column statistics, plus W's row statistics on this rank's own
// range) is what ranks exchange.  launch_key_queue_push_labeled fills the label ring with the two key rings (src_labels NULL: -1).
bool supcon_queue_gemm_supported(int d, float min_temperature, int64_t cols, int64_t q_cap);
size_t supcon_queue_gemm_workspace_bytes(int64_t rows, int64_t cols, int64_t q_cap, int d);
void launch_supcon_queue_gemm_pass1(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, const void* a_loc,
                                    const void* b_loc, const void* b_all, const void* qa, const void* qb, int64_t q_cap,
                                    const int64_t* q_valid, const int64_t* row_labels, const int64_t* col_labels,
                                    const int64_t* q_labels, void* workspace, float* col_stats, hipStream_t s);
void launch_supcon_queue_gemm_loss(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, const void* a_loc,
                                   const void* b_all, int64_t q_cap, const float* col_stats, void* workspace, float* loss_rows,
                                   hipStream_t s);
void launch_supcon_queue_gemm_grads(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, float coef,
                                    const void* a_loc, const void* b_loc, const void* b_all, const void* qa, const void* qb,
                                    int64_t q_cap, const int64_t* q_valid, const int64_t* row_labels, const int64_t* col_labels,
                                    const int64_t* q_labels, void* workspace, const float* upstream, int out_bf16, void* d_a_loc,
                                    void* d_b_loc, void* d_b_all, hipStream_t s);
void launch_key_queue_push_labeled(int64_t q_cap, int d, int64_t n, const void* src_a, const void* src_b, const int64_t* src_labels,
                                   void* qa, void* qb, int64_t* ql, int64_t* state, hipStream_t s);

// Multi-view InfoNCE on the tile GEMMs (aecf_nce_gemm.hip): the symmetric InfoNCE of every pair of views (anchor < 0) or of every
// pair with the anchor view, read in place from x_loc [rows][views][d] / x_all [cols][views][d]; one launch per stage for all
// pairs, gradient products with K through every partner block of a view.  col_sums [P][cols] is what ranks exchange.
bool nce_multi_supported(int d, float min_temperature, int64_t cols, int views, int anchor);
size_t nce_multi_workspace_bytes(int64_t rows, int64_t cols, int d, int views, int anchor);
void launch_nce_multi_pass1(int64_t rows, int64_t cols, int d, int views, int anchor, const NceDevTemp& dt, const void* x_loc,
                            const void* x_all, void* workspace, float* col_sums, hipStream_t s);
void launch_nce_multi_loss(int64_t rows, int64_t cols, int64_t row_offset, int d, int views, int anchor, const NceDevTemp& dt,
                           const void* x_loc, const void* x_all, const float* col_sums, void* workspace, float* loss_rows,
                           hipStream_t s);
void launch_nce_multi_grads(int64_t rows, int64_t cols, int64_t row_offset, int d, int views, int anchor, const NceDevTemp& dt,
                            float coef, const void* x_loc, const void* x_all, void* workspace, const float* upstream, int out_bf16,
                            void* dx_loc, void* dx_all, hipStream_t s);
// The same with missing views: pres_loc [rows] (by the local row) / pres_all [cols] (by the global column) hold one byte per row,
// bit v = view v present; pair p runs over the rows that hold both its views, with pair_coef[p] = 0.5 / n_p / P' from
// launch_nce_multi_pair_coef (one small launch over pres_all).  The workspace is nce_multi_workspace_bytes'.
void launch_nce_multi_pair_coef(int64_t cols, int views, int anchor, const unsigned char* pres_all, float* pair_coef, hipStream_t s);
void launch_nce_multi_masked_pass1(int64_t rows, int64_t cols, int d, int views, int anchor, const NceDevTemp& dt, const void* x_loc,
                                   const void* x_all, const unsigned char* pres_loc, const unsigned char* pres_all, void* workspace,
                                   float* col_sums, hipStream_t s);
void launch_nce_multi_masked_loss(int64_t rows, int64_t cols, int64_t row_offset, int d, int views, int anchor, const NceDevTemp& dt,
                                  const void* x_loc, const void* x_all, const unsigned char* pres_loc, const unsigned char* pres_all,
                                  const float* col_sums, void* workspace, float* loss_rows, hipStream_t s);
void launch_nce_multi_masked_grads(int64_t rows, int64_t cols, int64_t row_offset, int d, int views, int anchor, const NceDevTemp& dt,
                                   const float* pair_coef, const unsigned char* pres_loc, const void* x_loc, const void* x_all,
                                   void* workspace, const float* upstream, int out_bf16, void* dx_loc, void* dx_all, hipStream_t s);
// The same with a temperature and a weight PER PAIR: dt.t and dt.d_t are [P] arrays in pair order, pair_coef [P] comes from
// launch_nce_multi_pp_pair_coef (weights NULL: uniform; pres_all NULL: no view is missing), pres_loc / pres_all may be NULL (every
// row holds every view).  with_dt: pass 1 also leaves the per-pair dT sums that launch_nce_multi_pp_grads needs to write dt.d_t.
size_t nce_multi_pp_workspace_bytes(int64_t rows, int64_t cols, int d, int views, int anchor);
void launch_nce_multi_pp_pair_coef(int64_t cols, int views, int anchor, const unsigned char* pres_all, const float* weights,
                                   float* pair_coef, hipStream_t s);
void launch_nce_multi_pp_pass1(int64_t rows, int64_t cols, int d, int views, int anchor, const NceDevTemp& dt, const void* x_loc,
                               const void* x_all, const unsigned char* pres_loc, const unsigned char* pres_all, int with_dt,
                               void* workspace, float* col_sums, hipStream_t s);
void launch_nce_multi_pp_loss(int64_t rows, int64_t cols, int64_t row_offset, int d, int views, int anchor, const NceDevTemp& dt,
                              const void* x_loc, const void* x_all, const unsigned char* pres_loc, const unsigned char* pres_all,
                              const float* col_sums, void* workspace, float* loss_rows, hipStream_t s);
void launch_nce_multi_pp_grads(int64_t rows, int64_t cols, int64_t row_offset, int d, int views, int anchor, const NceDevTemp& dt,
                               const float* pair_coef, const unsigned char* pres_loc, const void* x_loc, const void* x_all,
                               void* workspace, const float* upstream, int out_bf16, void* dx_loc, void* dx_all, hipStream_t s);

// Pooled supervised contrastive loss on the tile GEMMs (aecf_nce_gemm.hip): NT-Xent's three blocks with the label statistics of the
// supervised loss -- X runs EPI_SUP, Y and Z EPI_SUP_SELF (rows only, the anchor excluded by index).  col_stats [3][cols] (X's column
// statistics, plus Z's row statistics on this rank's own range) is what ranks exchange.
bool supcon_pool_gemm_supported(int d, float min_temperature, int64_t cols);
size_t supcon_pool_gemm_workspace_bytes(int64_t rows, int64_t cols, int d);
void launch_supcon_pool_gemm_pass1(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, const void* a_loc,
                                   const void* b_loc, const void* a_all, const void* b_all, const int64_t* row_labels,
                                   const int64_t* col_labels, void* workspace, float* col_stats, hipStream_t s);
void launch_supcon_pool_gemm_loss(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, const void* a_loc,
                                  const void* b_all, const float* col_stats, void* workspace, float* loss_rows, hipStream_t s);
void launch_supcon_pool_gemm_grads(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, float coef,
                                   const void* a_loc, const void* b_loc, const void* a_all, const void* b_all, const int64_t* row_labels,
                                   const int64_t* col_labels, void* workspace, const float* upstream, int out_bf16, void* d_a_loc,
                                   void* d_b_loc, void* d_a_all, void* d_b_all, hipStream_t s);

// Pooled multi-label contrastive loss on the tile GEMMs (aecf_nce_gemm.hip): the pooled form above with class sets (one 64-bit word
// per row, bit c = class c) and the overlap (jaccard 0) or Jaccard (jaccard 1) weight in place of the match -- X runs EPI_SETS_OV /
// EPI_SETS_JAC, Y and Z EPI_SETS_OV_SELF / EPI_SETS_JAC_SELF (rows only, the anchor's own key weighs 0 by index).  Workspace,
// supported shapes and col_stats [3][cols] (column sums of E | sums of w | sums of w * raw score) are those of the pooled form.
bool supcon_ml_pool_gemm_supported(int d, float min_temperature, int64_t cols);
size_t supcon_ml_pool_gemm_workspace_bytes(int64_t rows, int64_t cols, int d);
void launch_supcon_ml_pool_gemm_pass1(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, const void* a_loc,
                                      const void* b_loc, const void* a_all, const void* b_all, const int64_t* row_sets,
                                      const int64_t* col_sets, int jaccard, void* workspace, float* col_stats, hipStream_t s);
void launch_supcon_ml_pool_gemm_loss(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, const void* a_loc,
                                     const void* b_all, const float* col_stats, void* workspace, float* loss_rows, hipStream_t s);
void launch_supcon_ml_pool_gemm_grads(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, float coef,
                                      const void* a_loc, const void* b_loc, const void* a_all, const void* b_all, const int64_t* row_sets,
                                      const int64_t* col_sets, int jaccard, void* workspace, const float* upstream, int out_bf16,
                                      void* d_a_loc, void* d_b_loc, void* d_a_all, void* d_b_all, hipStream_t s);

// Multi-label supervised contrastive loss, streaming (aecf_supcon_ml_flash.hip): a set of classes per row as one uint64 (bit c =
// class c); a key counts with weight 1 (the partner), [sets overlap] (jaccard 0) or |and| / |or| (jaccard 1).  The same passes,
// workspace layout and outputs as launch_supcon_flash.  launch_label_sets_pack: multi-hot rows [rows, classes <= 64] of kind
// 0 bf16, 1 float32, 2 float16, 3 uint8 -> the words (value != 0 = member).
bool supcon_ml_flash_supported(int d);
size_t supcon_ml_flash_workspace_bytes(int64_t rows, int64_t cols, int d);
void launch_supcon_ml_flash(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, float coef, const void* q,
                            const void* k, const uint64_t* q_sets, const uint64_t* k_sets, int jaccard, float* loss_rows, float* dq,
                            float* dk, void* workspace, hipStream_t s);
void launch_label_sets_pack(int64_t rows, int classes, int kind, const void* multi_hot, uint64_t* sets, hipStream_t s);

// Retrieval ranks of the contrastive views (aecf_retrieval.hip; the counting pass is the EPI_RANK epilogue of the logits GEMM in
// aecf_nce_gemm.hip): pos[i] = a_i . b_(row_offset + i), then per row / per column how many other logits are greater than / equal
// to the positive's.  Nothing of size rows x cols exists; the workspace is (rows + cols) x tiles int32 partials.
bool retrieval_supported(int d);
size_t retrieval_workspace_bytes(int64_t rows, int64_t cols, int d);
void launch_retrieval_positive(int64_t rows, int64_t row_offset, int d, const void* a, const void* b, float* pos_row, hipStream_t s);
void launch_retrieval_ranks(int64_t rows, int64_t cols, int64_t row_offset, int d, const void* a, const void* b, const float* pos_row,
                            const float* pos_col, int32_t* row_greater, int32_t* row_equal, int32_t* col_greater, int32_t* col_equal,
                            void* workspace, hipStream_t s);
void launch_rank_gemm(int64_t rows, int64_t cols, int64_t row_offset, int d, const void* a, const void* b, const float* pos_row,
                      const float* pos_col, int* row_part, int* col_part, hipStream_t s);

// Top-k retrieval (aecf_retrieval.hip; the selection pass is the EPI_TOPK epilogue of the same GEMM): values [rows, k] float32
// and indices [rows, k] int32 of the k <= 16 best columns of every row -- higher score first, lower column first among equal
// scores, NaN below -inf; exclude_partner drops column row_offset + i of row i.  Workspace: 8 KP bytes per row and column
// tile (KP: k rounded up to a power of two), never rows x cols.
bool retrieval_topk_supported(int d, int k);
size_t retrieval_topk_workspace_bytes(int64_t rows, int64_t cols, int d, int k);
void launch_retrieval_topk(int64_t rows, int64_t cols, int64_t row_offset, int d, int k, int exclude_partner, const void* a,
                           const void* b, float* values, int32_t* indices, void* workspace, hipStream_t s);
void launch_topk_gemm(int64_t rows, int64_t cols, int64_t row_offset, int d, int k, int kp, int exclude_partner, const void* a,
                      const void* b, unsigned long long* part, hipStream_t s);

// Multi-label evaluation counts (aecf_metrics.hip): class-major keys and the compacted valid positives of every class (prepare),
// the four compare-and-count integers of this rank's valid positives (counts), this rank's float64 shares [5][C] (finalize).
bool mlmetrics_supported(int64_t n_all, int classes);
size_t mlmetrics_workspace_bytes(int64_t n_all, int classes);
void launch_mlmetrics_prepare(int64_t n_all, int classes, int dtype, const void* logits, const uint8_t* labels, int32_t* class_counts,
                              void* workspace, hipStream_t s);
void launch_mlmetrics_counts(int64_t n_all, int classes, int64_t row_offset, int64_t rows, const int32_t* class_counts, int32_t* counts,
                             const void* workspace, hipStream_t s);
void launch_mlmetrics_finalize(int64_t n_all, int classes, int64_t row_offset, int64_t rows, float threshold, const int32_t* class_counts,
                               const int32_t* counts, double* shares, const void* workspace, hipStream_t s);
// what prepare left in the workspace, for another reader of the class-major keys (aecf_mlboot.hip)
struct MlmPrepared {
    const float* keys;                      // [C][Np], rows past n_all are NaN
    const unsigned long long* posmask;      // [C][nch] ballots of the valid positives
    int64_t Np, nch;
};
MlmPrepared mlmetrics_prepared(const void* workspace, int64_t n_all, int classes);

// Multi-label bootstrap (aecf_mlboot.hip): the stable descending order of every class by counting (after the evaluation's prepare,
// whose workspace it reads), the multiplicities W [n_all][Rp] uint8 of the replicates (Rp: replicates rounded up to 64) -- drawn,
// or packed from the caller's counts -- and the walk of the order with one lane per replicate: stats int64 [replicates][7][C] =
// Wpos | Wvalid | U2 | TP | FP | FN | the bits of the float64 S.
constexpr int MLBOOT_MAX_REPLICATES = 4096;
size_t mlboot_draw_workspace_bytes(int64_t n_all, int replicates);
void launch_mlboot_order(int64_t n_all, int classes, const float* thr, int32_t* order, const void* workspace, hipStream_t s);
void launch_mlboot_draw(int64_t n_all, int replicates, int64_t replicate0, uint64_t seed, const int32_t* counts, uint8_t* w,
                        int32_t* n_saturated, void* workspace, hipStream_t s);
void launch_mlboot_walk(int64_t n_all, int classes, int replicates, const int32_t* class_counts, const int32_t* order, const uint8_t* w,
                        int64_t* stats, hipStream_t s);

// Multi-label classification loss (aecf_mlloss.hip): BCE / focal / asymmetric loss of logits [n, C] as one elementwise formula.
// forward: one pass (per-row-block float64 loss sums and int32 valid counts per class) and a fixed-order finalize (stats [2][C],
// totals); backward: one pass that recomputes the element and scales it by upstream * factor / N read from totals.
// dtype: aecf_dtype of the logits; label_dtype: aecf_dtype, AECF_MLLOSS_U8 or AECF_MLLOSS_I8.
bool mlloss_supported(int64_t n, int classes);
size_t mlloss_workspace_bytes(int64_t n, int classes);
void launch_mlloss_forward(int64_t n, int classes, int dtype, int label_dtype, const void* logits, const void* labels,
                           const float* pos_scale, const float* neg_scale, float gamma_pos, float gamma_neg, float margin, float eps,
                           int mean, double* stats, double* totals, void* workspace, hipStream_t s);
void launch_mlloss_backward(int64_t n, int classes, int dtype, int label_dtype, const void* logits, const void* labels,
                            const float* pos_scale, const float* neg_scale, float gamma_pos, float gamma_neg, float margin, float eps,
                            int mean, const double* totals, const float* grad_out, float factor, void* dlogits, hipStream_t s);

// Fused classifier head (aecf_mlhead_flash.hip): that loss of logits = h W^T + bias, and dh, dW, dbias, on the streaming loop of
// aecf_flash_stream.h -- nothing of size n x classes exists.  forward: the CLS role (stationary classes, rows split), a combine
// of the splits (stats, and with want_grads the unscaled float32 dW / dbias) and the totals; backward: the ROW role (stationary
// rows, classes split) for dh where it is wanted, and the scaling of dW / dbias.  bf16 h [n, k] and w [classes, k].
bool mlhead_supported(int64_t n, int classes, int k);
size_t mlhead_workspace_bytes(int64_t n, int classes, int k);
void launch_mlhead_forward(int64_t n, int classes, int k, int label_dtype, const void* h, const void* w, const float* bias,
                           const void* labels, const float* pos_scale, const float* neg_scale, float gamma_pos, float gamma_neg,
                           float margin, float eps, int mean, int want_grads, double* stats, double* totals, float* dw_unscaled,
                           float* db_unscaled, void* workspace, hipStream_t s);
void launch_mlhead_backward(int64_t n, int classes, int k, int label_dtype, const void* h, const void* w, const float* bias,
                            const void* labels, const float* pos_scale, const float* neg_scale, float gamma_pos, float gamma_neg,
                            float margin, float eps, int mean, const double* totals, const float* grad_out, float factor,
                            const float* dw_unscaled, const float* db_unscaled, int dh_f32, void* dh, float* dw, float* db,
                            void* workspace, hipStream_t s);

// ---------------- presence routing (aecf_route.hip) ----------------
void launch_route_build(int64_t rows, const uint8_t* pa, const uint8_t* pb, int32_t* route, int32_t* slot, int32_t* index,
                        int32_t* counts, hipStream_t s);
void launch_rows_gather(int njobs, const void* const* src, const int64_t* src_pitch, const int32_t* const* index,
                        const int64_t* n, void* const* dst, const int64_t* dst_pitch, int64_t row_bytes, hipStream_t s);
void launch_adamw_multi(int n, float* const* p, const float* const* g, float* const* m, float* const* v, float* const* step,
                        const int64_t* numel, unsigned int* ticket, float lr, float beta1, float beta2, float eps, float weight_decay,
                        hipStream_t s);
// mixed-precision AdamW / gradient norm (aecf_optim.hip); empty tensors are skipped, dtypes are aecf_dtype values
int launch_adamw_mp(int n, void* const* p, const void* const* g, float* const* master, float* const* m, float* const* v,
                    float* const* step, const int64_t* numel, const int32_t* pdt, const int32_t* gdt, unsigned int* ticket, float lr,
                    float beta1, float beta2, float eps, float weight_decay, const float* lr_dev, const float* grad_scale,
                    const float* grad_coef, const float* found_inf, const float* found_inf2, hipStream_t s);
// the same step with the averages' tables (ema[i] NULL: no average; ema_out, or an entry, NULL: none), and the EMA alone
int launch_adamw_mp_ema(int n, void* const* p, const void* const* g, float* const* master, float* const* m, float* const* v,
                        float* const* step, const int64_t* numel, const int32_t* pdt, const int32_t* gdt, unsigned int* ticket,
                        float lr, float beta1, float beta2, float eps, float weight_decay, const float* lr_dev,
                        const float* grad_scale, const float* grad_coef, const float* found_inf, const float* found_inf2,
                        float* const* ema, void* const* ema_out, float ema_decay, const float* ema_decay_dev, hipStream_t s);
int launch_ema_update(int n, const void* const* src, const int32_t* sdt, float* const* ema, void* const* ema_out, const int32_t* odt,
                      const int64_t* numel, float decay, const float* decay_dev, const float* found_inf, const float* found_inf2,
                      hipStream_t s);
int64_t grad_norm_blocks(int n, const int64_t* numel);
void launch_grad_norm(int n, const void* const* g, const int32_t* gdt, const int64_t* numel, float max_norm, const float* grad_scale,
                      float* partial, float* out, hipStream_t s);
void launch_rows_split(int64_t rows, int64_t row_bytes, const int32_t* route, const void* src, void* const* dst, hipStream_t s);
void launch_front_pair(int dtype, int64_t rows, int dim_a, int dim_b, const void* feat_a, const void* feat_b, const float* uniforms,
                       float missing_prob, const uint8_t* drop_a, const uint8_t* drop_b, void* out_a, void* out_b,
                       uint8_t* present_a, uint8_t* present_b, int32_t* cls, hipStream_t s);
void launch_rows_select(int64_t rows, int64_t row_bytes, const int32_t* route, const int32_t* slot, const void* const* src,
                        const int64_t* src_pitch, void* dst, int64_t dst_pitch, hipStream_t s);

}  // namespace aecf
