/*
 * aecf_hip.h -- C ABI of libaecf_hip.so: the MI355X (gfx950) implementation of the AECF
 * fusion hot path (BASELINE.json north_star).
 *
 * The reference (leochlon/aecf) is pure Python and has no FFI of its own: its boundary for
 * this path is the Python API in aecf/AECFLayer.py.  Each entry point below replaces the
 * arithmetic of one reference function; the Python package aecf_amd/ binds these symbols
 * with ctypes and mirrors the reference's signatures (INTEGRATION.md shows the stub).
 *
 * Conventions
 *  - plain C symbols, plain pointers and sizes, no C++/torch types.
 *  - the CALLER owns every buffer (including the workspace); the library never allocates or
 *    frees device memory, never retains a caller pointer past the call, never synchronises
 *    the stream and never throws.
 *  - every call only enqueues kernels on `stream` (a hipStream_t passed as void*) -- plain launches: a caller that is
 *    capturing `stream` (a whole training step as one HIP graph) gets them as nodes of its own graph.
 *  - return value: AECF_OK (0) or a negative aecf_status.
 *  - dtype: AECF_BF16, AECF_F32 or AECF_F16 for x / query / weights / y.  All statistics (attention weights, entropy, mask
 *    rate, saved probabilities) are float32 (optional copies in the activation dtype: aecf_pool_fwd_args.info_*).  Parameter
 *    gradients are float32, or bf16 / f16 when aecf_pool_bwd_args.grad_dtype asks for it (16-bit parameters: the float32
 *    batch sums are rounded once, in the reduction kernel).  AECF_F16 (ABI v10) runs the LDS-tile kernels the float32 path
 *    runs, on the f16 MFMA; the bf16-only engines (weight-stationary, transposed-read reductions, AECF_HILO_GRADS,
 *    AECF_PRECISE, InfoNCE, the x-ray front-ends) are not built for it and those entry points answer AECF_ERR_UNSUPPORTED.
 *  - thread-safe and stateless: any thread may call with any stream of the current device; the library keeps nothing between
 *    calls and reads no environment: the kernels a call launches follow from its description and arguments alone.
 */
#ifndef AECF_HIP_H
#define AECF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AECF_ABI_VERSION 10

typedef enum aecf_status {
    AECF_OK = 0,
    AECF_ERR_BAD_DIMS = -1,        /* non-positive size, E % num_heads != 0, ...            */
    AECF_ERR_UNSUPPORTED = -2,     /* valid for the reference but not built here (see msg)  */
    AECF_ERR_NULL_POINTER = -3,
    AECF_ERR_WORKSPACE = -4,       /* workspace too small                                    */
    AECF_ERR_LAUNCH = -5           /* hipGetLastError() != hipSuccess after a launch         */
} aecf_status;

typedef enum aecf_dtype { AECF_BF16 = 0, AECF_F32 = 1, AECF_F16 = 2 /* ABI v10 */ } aecf_dtype;

/* Problem description shared by forward and backward.
 * Replaces: MultimodalAttentionPool.__init__/forward shape contract
 * (ref aecf/AECFLayer.py:371-407, 461-498) for the hot-path case
 *   query = fusion_query.expand(B,1,E)  (one shared query, ref :694-695),
 *   key is value = x[B,M,E] contiguous, batch_first, dropout 0, no attn_mask. */
typedef struct aecf_pool_desc {
    int64_t batch;        /* B                                   */
    int32_t modalities;   /* M = src_len, 1..8                    */
    int32_t embed_dim;    /* E, multiple of 64                    */
    int32_t num_heads;    /* H, 1..16, E % H == 0, (E/H) % 32 == 0 (bf16, f16) or % 16 == 0 (f32) */
    int32_t dtype;        /* aecf_dtype of x/query/weights/y      */
    /* curriculum masking (ref aecf/AECFLayer.py:76-99); mask_mode 0 = no CurriculumMasking
     * module attached, 1 = training-mode masking (:158-283), 2 = eval-mode (:150-156)      */
    int32_t mask_mode;
    int32_t min_active;
    float base_mask_prob;
    float entropy_target;
    float eps;            /* the module's _eps buffer, 1e-8 (:96) */
} aecf_pool_desc;

/* Forward.  Replaces nn.MultiheadAttention math (torch functional.py:5836-5852, 6576-6612,
 * called at ref :515-521) + CurriculumMasking.forward (ref :130-283) on the head-averaged
 * weights, fused.  Outputs other than y are float32. */
typedef struct aecf_pool_fwd_args {
    const void* x;               /* [B,M,E] dtype                                        */
    const void* query;           /* [E] dtype: the shared fusion query                   */
    const void* w_in;            /* [3E,E] dtype  (in_proj_weight, q|k|v)                */
    const void* b_in;            /* [3E] dtype or NULL                                   */
    const void* w_out;           /* [E,E] dtype   (out_proj.weight)                      */
    const void* b_out;           /* [E] dtype or NULL                                    */
    const uint8_t* key_padding_mask; /* [B,M] nonzero = ignore, or NULL                  */
    const float* uniforms;       /* [B,M] float32 U[0,1) (mask_mode 1) or NULL           */
    void* y;                     /* [B,E] dtype                                          */
    float* attn_w;               /* [B,M] head-averaged weights (info['attention_weights']) */
    float* masked_w;             /* [B,M] or NULL                                        */
    float* entropy;              /* [B]   or NULL                                        */
    float* mask_rate;            /* [B]   or NULL                                        */
    float* saved_probs;          /* [B,H,M] per-head softmax, saved for backward         */
    void* saved_o;               /* [B,E] dtype: pre-out-projection heads, saved for backward (or NULL) */
    void* saved_v;               /* [B,M,E] dtype: per-modality value projections W_v x + b_v, saved so that the
                                  * backward score gradient is a memory-bound dot instead of a recompute (or NULL) */
    void* workspace;
    size_t workspace_bytes;
    /* optional profiling hook: AECF_FWD_STAGES+1 hipEvent_t handles (caller-created); event[0] is recorded
     * before the first kernel and event[i] after stage i (see aecf_pool_stage_name). NULL = off. */
    void** stage_events;
    /* optional copies of the four info tensors in the ACTIVATION dtype, written by the same kernel (the reference
     * returns info in the input dtype, ref :520-543, so a bf16 caller needs no cast kernels); NULL = not wanted */
    void* info_attn_w;           /* [B,M] dtype */
    void* info_masked_w;         /* [B,M] dtype */
    void* info_entropy;          /* [B]   dtype */
    void* info_mask_rate;        /* [B]   dtype */
    /* optional: aecf_pool_prep_bytes(desc) bytes that receive everything the BACKWARD derives from the parameters alone
     * (scaled query projection, folded key matrix, W_v^T / W_o^T and their MFMA-fragment copies), produced by the
     * forward's own preparation launch.  Hand the same buffer to aecf_pool_backward (parameters unchanged in
     * between -- what autograd guarantees) and its preparation stage disappears.  NULL = off. */
    void* saved_prep;
    /* optional (mask_mode 1): info['target_entropy'] of the reference (ref :273, full_like(entropy, log(M) * target)):
     * [B] dtype filled with target_entropy_value by the kernel that writes the other info tensors; NULL = not wanted */
    void* info_target_entropy;
    float target_entropy_value;  /* the caller's log(M) * entropy_target, rounded to float32 */
    /* AECF_PRECISE (desc.dtype == AECF_BF16 only): the float32-STORE form of the bf16 path ("bf16
     * tolerance"): x / query / weights are bf16 as usual and every product of exact bf16 operands runs on the bf16 MFMA
     * kernels, but no intermediate is rounded to bf16 -- the pooled heads o are kept in float32 and the products that
     * consume an intermediate accumulate from it in float32.  y, saved_o (and in the backward dx and all parameter
     * gradients) are then float32 buffers; workspace = aecf_pool_precise_workspace_bytes.  A verification mode (it moves
     * twice the bytes): what "outputs match within 1e-3 relative, bf16" is asserted on. */
    int32_t flags;
    /* optional (mask_mode 1; ABI v7): partial sums of CurriculumMasking.entropy_loss over the rows of this call (ref
     * aecf/AECFLayer.py:285-314), float32 [(B + 255) / 256]: entry i = sum over rows 256 i .. of (nan_to_num(H) - target)^2 with
     * H = the entropy as the info tensor holds it and target = target_entropy_value.  Written by the kernel that writes the
     * entropies, so that a later entropy_loss of exactly this tensor is ONE small launch (aecf_entropy_loss_from_partials)
     * instead of a pass over the rows.  NULL = not wanted. */
    float* ent_loss_partial;
    /* ABI v8.  AECF_DRAW_UNIFORMS (mask_mode 1, uniforms == NULL): the statistics kernel draws the Bernoulli uniforms of ref
     * aecf/AECFLayer.py:204 itself -- for weight element i exactly the value `torch.rand(B*M, device=...)` would hold at i when
     * the device generator stands at (philox_seed, philox_offset): Philox4x32-10, subsequence = the element's thread of
     * torch's launch of philox_threads threads (its grid: min(ceil(n / 256), CUs * 8) blocks of 256), 2^-32 + v 2^-32 with 1.0
     * mapped to 0.0.  The caller advances its generator by what that torch call would have consumed (4 per 4*threads elements).
     * One launch and a [B,M] float32 tensor less per step; a caller who needs a recorded draw (parity tests, data-parallel
     * shards of one global draw) keeps passing `uniforms`. */
    uint64_t philox_seed;
    uint64_t philox_offset;
    uint32_t philox_threads;
    /* ABI v8, optional (mask_mode 1, with ent_loss_partial): [1] dtype, CurriculumMasking.entropy_loss over the rows of this
     * call -- max(mean((nan_to_num(H) - target)^2), 0), ref :285-314 -- written by the out-projection launch's first block from
     * the partial sums (no launch of its own; shapes the weight-stationary kernel does not take: one small launch).  NULL = off. */
    void* ent_loss;
    /* ABI v8, AECF_HILO_GRADS: [B,E] dtype, the LOW part of saved_o -- bf16(o - float(bf16(o))) -- written beside it by the
     * value projection; hand both to the backward (see aecf_pool_bwd_args.saved_o_lo).  Required with the flag. */
    void* saved_o_lo;
    /* ABI v9, AECF_DRAW_UNIFORMS: this call's rows are rows [r0, r0 + B) of a LARGER batch whose mask uniforms are ONE draw
     * `torch.rand(B_global * M)` -- a data-parallel rank's shard.  philox_element0 = r0 * M is the element of that draw the
     * call's first weight element is, and philox_threads is the thread count of the GLOBAL launch; weight element i of the call
     * takes the value the global tensor holds at philox_element0 + i.  Every rank passes the same (seed, offset) and advances its
     * generator by what the global call consumes: N-rank masks are the one-rank masks bit for bit with no uniforms tensor and no
     * launch.  0 = the call is the whole draw. */
    int64_t philox_element0;
} aecf_pool_fwd_args;

#define AECF_PRECISE 1
#define AECF_DRAW_UNIFORMS 2
/* AECF_HILO_GRADS (bf16; aecf_pool_hilo_bwd_workspace_bytes(desc) > 0 says the shape is built): the WEIGHT-GRADIENT products
 * of the backward take the operands that are derived values as bf16 hi + lo pairs -- dW_o = dy^T (o_hi + o_lo), dW_v = do_hi^T
 * P_hi + do_hi^T P_lo + do_lo^T P_hi with do = dy W_o and the pooled rows P split where they are formed, the key-side reduction
 * from do_hi + do_lo -- so that float32-STORED parameter gradients are float32-accurate (the bf16 roundings of the derived
 * operands are what puts the default path's dW at 1.3 - 2.3e-3 of fp32 math at the headline shape: above north_star's 1e-3).
 * Everything else (y, dx, the kernels) is the default path.  Set it on BOTH calls.  ONE launch per product (round 5,
 * aecf_gemm_tn_hilo.hip: hi and lo tiles of a step side by side in LDS, one accumulator set, one slab set); the backward
 * workspace is the larger aecf_pool_hilo_bwd_workspace_bytes (do_lo).  The Python layer sets it by itself whenever the parameter
 * gradients are float32-stored (float32 master weights under bf16 activations); with bf16 parameters the gradient's own
 * rounding (2^-9) hides what the flag buys.  Built for every bf16 shape whose value projection runs on the weight-stationary
 * kernel: E in {256, 512, 768, 1024}, M <= 4, head_dim % 32 == 0 (not E = 1024 with M = 3); M = 5..8, other E, float16 and
 * float32 return AECF_ERR_UNSUPPORTED.  The key-side term comes from do_hi + do_lo on the head-split score-gradient kernel where
 * it has room for the low tiles (E = 256 / 512, M <= 3; E = 256, M = 4), else on the recompute pass (W_v^T do per head from the
 * exact bf16 W_v, float32 accumulation) -- never from saved_v, whose elements are rounded to bf16: with the flag the backward
 * does not read saved_v, and the forward may be given NULL there. */
#define AECF_HILO_GRADS 4
/* AECF_PREP_READY (forward only, with saved_prep; ABI v9): saved_prep already holds the preparation an earlier forward made from
 * these very parameters and this query (same embed_dim / num_heads / dtype; the batch may differ): the preparation launch is
 * skipped.  For loops in which the parameters provably stand still -- inference, gradient accumulation over micro-batches.  The
 * caller is responsible for "unchanged" (the Python layer keys its cache on the identity, storage and version counter of the
 * parameters and the query, in eval mode / without gradient recording only, and never sets the flag while the stream is being
 * captured: a captured forward always prepares for itself). */
#define AECF_PREP_READY 8

/* Backward (autograd transpose of the above). */
typedef struct aecf_pool_bwd_args {
    const void* x;
    const void* query;
    const void* w_in;
    const void* b_in;
    const void* w_out;
    const void* dy;              /* [B,E] dtype                                          */
    const float* d_attn_w;       /* [B,M] grad on info['attention_weights'] or NULL      */
    const float* d_entropy;      /* [B] grad on info['entropy'] (eval mode only) or NULL */
    const float* attn_w;         /* [B,M] forward output (needed with d_entropy)         */
    const float* saved_probs;    /* [B,H,M]                                              */
    const void* saved_o;         /* [B,E]                                                */
    const void* saved_v;         /* [B,M,E] or NULL (NULL: the score gradient recomputes W_v^T do per head;
                                  * not read with AECF_HILO_GRADS) */
    void* dx;                    /* [B,M,E] dtype                                        */
    void* dquery;                /* [E]     grad_dtype                                   */
    void* dw_in;                 /* [3E,E]  grad_dtype                                   */
    void* db_in;                 /* [3E]    grad_dtype                                   */
    void* dw_out;                /* [E,E]   grad_dtype                                   */
    void* db_out;                /* [E]     grad_dtype                                   */
    void* workspace;
    size_t workspace_bytes;
    void** stage_events;         /* AECF_BWD_STAGES+1 hipEvent_t handles or NULL (profiling hook) */
    /* element type of the five parameter gradients: AECF_F32, or AECF_BF16 / AECF_F16 when desc.dtype is that type (the
     * float32 batch sums are rounded once, in the reduction kernel -- what autograd's cast to a 16-bit parameter does) */
    int32_t grad_dtype;
    int32_t flags;               /* AECF_PRECISE: dy bf16; saved_o, dx and the gradients float32 (see aecf_pool_fwd_args.flags) */
    const void* saved_prep;      /* buffer filled by aecf_pool_forward (see aecf_pool_fwd_args.saved_prep) or NULL */
    /* optional hipEvent_t (caller-created): recorded on `stream` as soon as ALL FIVE parameter gradients (dquery, dw_in,
     * db_in, dw_out, db_out) are final.  With it set the backward computes the input gradient dx LAST (otherwise it comes
     * before dW_v), so a data-parallel caller can run the gradients' all-reduce on another stream behind the dx kernel
     * (aecf_amd/dp.py: GradOverlap).  stage_events are not recorded in this order of stages.
     * NULL = off. */
    void* param_grads_event;
    const void* saved_o_lo;      /* AECF_HILO_GRADS: the forward's low part of saved_o, else NULL (ABI v8) */
    /* ABI v9: the five parameter gradients are multiplied by grad_scale as their float32 batch sums are stored (before the one
     * rounding of a bf16 gradient) -- a data-parallel caller passes 1 / world, so that the gradient average is ONE sum
     * all-reduce with no divide launch around it.  dx is not scaled.  0 = 1 (off). */
    float grad_scale;
} aecf_pool_bwd_args;

#define AECF_FWD_STAGES 4   /* prep, gate, vproj, outproj */
#define AECF_BWD_STAGES 8   /* prep, dout, dw_out, dscore, u, dx, dw_v, finalize */

int aecf_abi_version(void);
/* name of forward (backward == 0) or backward stage i, or NULL when out of range */
const char* aecf_pool_stage_name(int backward, int stage);
const char* aecf_status_string(int status);

/* validates the description; returns AECF_OK or the reason it cannot run */
int aecf_pool_check(const aecf_pool_desc* d);
/* scratch bytes needed by forward / backward for this description */
size_t aecf_pool_fwd_workspace_bytes(const aecf_pool_desc* d);
size_t aecf_pool_bwd_workspace_bytes(const aecf_pool_desc* d);
/* 1 when the backward of this description is faster with the forward's per-modality value projections
 * (aecf_pool_fwd_args.saved_v), 0 when it derives the score gradient from x itself and saved_v should stay NULL
 * (bf16, E in {256, 512}, M <= 4: the forward then writes B*M*E fewer elements; always 1 for f32 and f16) */
int aecf_pool_wants_saved_v(const aecf_pool_desc* d);
/* workspace bytes of a call with AECF_PRECISE set (backward == 0: forward) */
size_t aecf_pool_precise_workspace_bytes(const aecf_pool_desc* d, int backward);
/* backward workspace bytes of a call with AECF_HILO_GRADS set; 0 = the flag is not built for this description */
size_t aecf_pool_hilo_bwd_workspace_bytes(const aecf_pool_desc* d);
/* bytes of the optional parameter-preparation buffer shared by forward and backward (saved_prep) */
size_t aecf_pool_prep_bytes(const aecf_pool_desc* d);

/* The generator call of AECF_DRAW_UNIFORMS on its own (tests, callers that want the tensor): out[i], i < n, = the float32
 * uniform described at aecf_pool_fwd_args.philox_seed for element element0 + i of the draw (element0: see philox_element0).  aecf_philox_host evaluates one element on the host (known-answer
 * tests; `raw` != NULL additionally receives the four 32-bit outputs of the Philox4x32-10 block the element comes from). */
int aecf_philox_uniforms(int64_t n, uint64_t seed, uint64_t offset, uint32_t threads, int64_t element0, float* out, void* stream);
float aecf_philox_host(uint64_t seed, uint64_t offset, uint32_t threads, int64_t element, uint32_t* raw);

int aecf_pool_forward(const aecf_pool_desc* d, const aecf_pool_fwd_args* a, void* stream);
int aecf_pool_backward(const aecf_pool_desc* d, const aecf_pool_bwd_args* a, void* stream);

/* Stand-alone CurriculumMasking.forward on rows of length L (ref aecf/AECFLayer.py:130-283).
 * weights [rows,L] float32, any L.  mode 1 = train (uniforms required), 2 = eval.
 * Any output pointer may be NULL -- except mask_bits in train mode when L > 64 (rows that long keep their bits there). */
int aecf_curriculum_mask_forward(int64_t rows, int32_t L, int32_t mode, int32_t min_active,
                                 float base_mask_prob, float entropy_target, float eps,
                                 const float* weights, const float* uniforms,
                                 float* masked, float* entropy, float* mask_rate,
                                 uint8_t* mask_bits, void* stream);

/* Gradient of the stand-alone module's masked output and (eval mode) entropy w.r.t. weights.
 * d_masked [rows,L] or NULL, d_entropy [rows] or NULL, mask_bits from the forward (train). */
int aecf_curriculum_mask_backward(int64_t rows, int32_t L, int32_t mode, float eps,
                                  const float* weights, const uint8_t* mask_bits,
                                  const float* d_masked, const float* d_entropy,
                                  float* d_weights, void* stream);

/* CurriculumMasking.entropy_loss forward + backward (ref aecf/AECFLayer.py:285-314):
 * loss[0] = mean((nan_to_num(H) - log(last_seq_len)*entropy_target)^2); d_entropy = dloss/dH * upstream.
 * partial: scratch of aecf_entropy_loss_workspace_bytes(n). */
size_t aecf_entropy_loss_workspace_bytes(int64_t n);
/* loss[0] (dtype) = max(sum of the (n + 255) / 256 partial sums aecf_pool_forward left in ent_loss_partial, 0) / n */
int aecf_entropy_loss_from_partials(int64_t n, int32_t dtype, const float* partial, void* loss, void* stream);
/* entropy [n] and loss [1] have element type dtype -- AECF_BF16, AECF_F32 or AECF_F16 (the reference computes the loss in
 * the dtype of info['entropy']); the arithmetic and d_entropy [n] are float32. */
int aecf_entropy_loss_fwd_bwd(int64_t n, int32_t dtype, int32_t last_seq_len, float entropy_target,
                              const void* entropy, float upstream, void* loss,
                              float* d_entropy, void* workspace, void* stream);

/* Projection-free single-head attention softmax(Q K^T * scale) V (ref aecf/AECFLayer.py:556-581).
 * q [B,S,E], k,v [B,T,E] dtype (AECF_BF16, AECF_F32 or AECF_F16); out [B,S,E] dtype; probs [B,S,T] float32 saved for backward. */
int aecf_sdpa_forward(int64_t B, int32_t S, int32_t T, int32_t E, int32_t dtype, float scale,
                      const void* q, const void* k, const void* v, void* out, float* probs,
                      void* stream);
int aecf_sdpa_backward(int64_t B, int32_t S, int32_t T, int32_t E, int32_t dtype, float scale,
                       const void* q, const void* k, const void* v, const float* probs,
                       const void* dout, void* dq, void* dk, void* dv, void* stream);

/* ---- general multi-head attention ----
 * Everything nn.MultiheadAttention does for MultimodalAttentionPool.forward OUTSIDE the shared-query hot path
 * (ref aecf/AECFLayer.py:409-418, 480-521; torch functional.py:5836-5852, 6504-6519, 6554-6612): per-sample
 * queries, tgt_len > 1, key != value, attn_mask, key_padding_mask, attention dropout.  Batch-major tensors.
 *   Q = query W_q^T + b_q, K = key W_k^T + b_k, V = value W_v^T + b_v            (NT GEMMs)
 *   per (b,h): p = softmax(Q_h K_h^T / sqrt(hd) + attn_mask, key_padding_mask -> -inf); p' = dropout(p)
 *   o_h = p' V_h ;  y = o W_o^T + b_o ;  attn_w = mean_h p'   (the weights are returned AFTER dropout, as torch does)
 * Dropout takes explicit uniforms: keep = (u >= dropout_p), p' = p * keep / (1 - dropout_p)  (torch draws its own
 * Philox stream inside F.dropout, so the pattern is distribution-, not bit-, compatible).  tgt_len, src_len <= 4096 (the
 * score rows of a chunk of query positions live in LDS; longer targets are walked in chunks). */
typedef struct aecf_mha_desc {
    int64_t batch;
    int32_t tgt_len;      /* T */
    int32_t src_len;      /* S */
    int32_t embed_dim;    /* E <= 1024, multiple of 32 (f32) / 64 (bf16, f16) */
    int32_t num_heads;    /* H, any divisor of E */
    int32_t dtype;        /* aecf_dtype of activations and weights */
    float dropout_p;      /* 0 = no dropout (then dropout_uniforms may be NULL) */
} aecf_mha_desc;

typedef struct aecf_mha_fwd_args {
    const void* query;           /* [B,T,E] dtype */
    const void* key;             /* [B,S,E] dtype */
    const void* value;           /* [B,S,E] dtype */
    const void* w_in;            /* [3E,E] */
    const void* b_in;            /* [3E] or NULL */
    const void* w_out;           /* [E,E] */
    const void* b_out;           /* [E] or NULL */
    const float* attn_mask;      /* additive float32 mask (-inf = blocked) [T,S] or [B*H,T,S], or NULL */
    int64_t attn_mask_stride;    /* 0 for a shared [T,S] mask, T*S for one per (b*H + h) */
    const uint8_t* key_padding_mask; /* [B,S] nonzero = ignore, or NULL */
    const float* dropout_uniforms;   /* [B*H,T,S] float32 U[0,1), or NULL when dropout_p == 0 */
    void* y;                     /* [B,T,E] dtype */
    float* attn_w;               /* [B,T,S] head-averaged weights (after dropout) */
    void* saved_q;               /* [B*T,E] dtype projections, kept for the backward */
    void* saved_k;               /* [B*S,E] */
    void* saved_v;               /* [B*S,E] */
    void* saved_o;               /* [B*T,E] pre-out-projection heads */
    float* saved_probs;          /* [B,H,T,S] softmax (before dropout) */
} aecf_mha_fwd_args;

typedef struct aecf_mha_bwd_args {
    const void* query;
    const void* key;
    const void* value;
    const void* w_in;
    const void* w_out;
    const float* dropout_uniforms;
    const void* dy;              /* [B,T,E] dtype */
    const float* d_attn_w;       /* [B,T,S] or NULL */
    const void* saved_q;
    const void* saved_k;
    const void* saved_v;
    const void* saved_o;
    const float* saved_probs;
    void* dquery;                /* [B,T,E] dtype */
    void* dkey;                  /* [B,S,E] dtype */
    void* dvalue;                /* [B,S,E] dtype */
    float* dw_in;                /* [3E,E] float32 */
    float* db_in;                /* [3E]   */
    float* dw_out;               /* [E,E]  */
    float* db_out;               /* [E]    */
    void* workspace;
    size_t workspace_bytes;
} aecf_mha_bwd_args;

int aecf_mha_check(const aecf_mha_desc* d);
size_t aecf_mha_bwd_workspace_bytes(const aecf_mha_desc* d);
int aecf_mha_forward(const aecf_mha_desc* d, const aecf_mha_fwd_args* a, void* stream);
int aecf_mha_backward(const aecf_mha_desc* d, const aecf_mha_bwd_args* a, void* stream);

/* ---- missing-modality front-end (ref xrays/train_xrays_example.py:156-177, 202-203) ----
 * One pass over one modality's feature rows feat [rows,dim]: rows with drop[r] != 0 are zeroed (the reference's
 * clone + masked write, :173-176) and present[r] = (||row||_2 > 1e-6) of the row AS WRITTEN (the reference's
 * torch.norm(...) > 1e-6 presence test, :202-203).  drop may be NULL (evaluation: presence only); out may equal
 * feat (in place) and may be NULL when drop is NULL (nothing to write).  Norm accumulated in float32.  dtype: AECF_BF16 or
 * AECF_F32 (AECF_F16: AECF_ERR_UNSUPPORTED, checked before the pointers; the same for aecf_front_pair). */
int aecf_modality_frontend(int64_t rows, int32_t dim, int32_t dtype, const void* feat, const uint8_t* drop,
                           void* out, uint8_t* present, void* stream);

/* ---- presence routing around the pool (ref xrays/train_xrays_example.py:205-234) ----
 * The reference routes rows with boolean masks + torch.where + torch.stack + index_put.  Here: one routing table built on
 * the device, then row moves driven by it.
 *   aecf_route_build: class of every row from the two presence vectors -- 0 both present (:205), 1 only a (:206),
 *     2 only b (:207), 3 neither -- its slot inside its class (ascending row order, what torch.where yields), the inverse
 *     lists index[c*rows + slot] = row for c = 0..2, and counts[4] (the only values the host reads back).
 *   aecf_rows_gather: up to 3 jobs dst_j[i] = src_j[index_j[i]], i < n_j, in ONE launch (rows of row_bytes bytes; pitches in
 *     bytes).  E.g. the [n_both, 2, E] pool input of :213-216 = two jobs writing the halves of one destination row.
 *   aecf_rows_select: dst[r] = src_{route[r]}[slot[r]] (class 3 or a NULL source: zeros); EVERY row of dst is written once,
 *     so no memset / index_put is needed (the fused [B, 2E] rows of :209-234; the backward of a gather). */
int aecf_route_build(int64_t rows, const uint8_t* present_a, const uint8_t* present_b, int32_t* route,
                     int32_t* slot, int32_t* index, int32_t* counts, void* stream);
int aecf_rows_gather(int32_t njobs, const void* const* src, const int64_t* src_pitch,
                     const int32_t* const* index, const int64_t* n, void* const* dst,
                     const int64_t* dst_pitch, int64_t row_bytes, void* stream);
int aecf_rows_select(int64_t rows, int64_t row_bytes, const int32_t* route, const int32_t* slot,
                     const void* const* src, const int64_t* src_pitch, void* dst, int64_t dst_pitch,
                     void* stream);

/* ---- static routing (every branch keeps all rows, so a whole step has fixed shapes and can be one HIP graph) ----
 *   aecf_front_pair: both modality front-ends, the missing-modality decisions (ref :156-172) and the row classes in one
 *     launch.  Decisions come from uniforms [3, rows] (a dropped if u0 < missing_prob, b if u1 < missing_prob; a row that
 *     would lose both keeps a when u2 > 0.5, else b), or from drop_a / drop_b (either may be NULL), or none (all three
 *     NULL).  present_x = not dropped and ||row|| > 1e-6 (float32; false for NaN rows, as torch.norm(...) > 1e-6 is, :202-203);
 *     out_x = the row if present_x else zeros (out_x != feat_x); cls as aecf_route_build's route.
 *   aecf_rows_select with slot == NULL reads src_c[r] (identity slots): fused[r] = the row of the branch that owns r.
 *   aecf_rows_split: its backward, dst_c[r] = src[r] if route[r] == c else zeros, c = 0..2 (NULL dst_c skipped), one launch. */
int aecf_front_pair(int64_t rows, int32_t dim_a, int32_t dim_b, int32_t dtype, const void* feat_a, const void* feat_b,
                    const float* uniforms, float missing_prob, const uint8_t* drop_a, const uint8_t* drop_b,
                    void* out_a, void* out_b, uint8_t* present_a, uint8_t* present_b, int32_t* cls, void* stream);
int aecf_rows_split(int64_t rows, int64_t row_bytes, const int32_t* route, const void* src, void* const* dst,
                    void* stream);

/* float32 -> bf16 (round to nearest even) of up to 8 tensors in one launch: the activation-dtype copies of float32 MASTER
 * parameters a mixed-precision step hands to aecf_pool_forward (w_in, b_in, w_out, b_out, query; ABI v9).  What
 * `p.to(torch.bfloat16)` does per tensor (ref: the reference trains in one dtype; torch's autocast makes these copies), as one
 * launch of 2048-element blocks.  src[i] / dst[i]: device pointers, numel[i] elements each; host arrays of length n <= 8. */
int aecf_cast_f32_to_bf16(int32_t n, const float* const* src, void* const* dst, const int64_t* numel, void* stream);
/* The same for float32 -> IEEE half (ABI v10): round to nearest even, overflow to +-inf, NaN stays NaN -- `p.to(torch.float16)`
 * bit for bit.  The kernels' own float16 stores use the same conversion. */
int aecf_cast_f32_to_f16(int32_t n, const float* const* src, void* const* dst, const int64_t* numel, void* stream);

/* ---- the example trainer's optimiser step (ref xrays/train_xrays_example.py:322-323, 376: torch.optim.AdamW) ----
 * AdamW (decoupled weight decay, no amsgrad) over n float32 tensors in one launch per 24 tensors: arrays of n device
 * pointers (param, grad, exp_avg, exp_avg_sq: numel[i] floats each; step[i]: ONE float, the number of steps taken so far,
 * advanced on the device so that a captured step replays with a fresh count) and ticket = AECF_ADAMW_TICKET_WORDS * ((n + 23) / 24)
 * zero-initialised uint32 the launches use to find their last block (they leave them zero).  Arithmetic in float32; the bias corrections
 * 1 - beta^t are formed as -expm1(t ln beta) in float32 (relative error ~1e-7; torch uses double on the host or, capturable,
 * a float32 pow on the device).  beta = 0 is not supported (ln). */
#define AECF_ADAMW_TICKET_WORDS 65
int aecf_adamw_step(int32_t n, void* const* param, const void* const* grad, void* const* exp_avg,
                    void* const* exp_avg_sq, void* const* step, const int64_t* numel, void* ticket, float lr,
                    float beta1, float beta2, float eps, float weight_decay, void* stream);

/* ---- the optimiser step of a mixed-precision trainer (new entry points under ABI v10, no bump) ----
 * aecf_adamw_mp_step: the update and the ticket contract of aecf_adamw_step (it replaces the same torch.optim.AdamW of ref
 * xrays/train_xrays_example.py:322-323, for a model held in bf16 / f16) over tensors whose param[i] is param_dtype[i] and whose
 * grad[i] is grad_dtype[i] (aecf_dtype values, independent of each other).  exp_avg / exp_avg_sq / step are float32 always.
 * master (the array, or any entry) may be NULL; master[i] != NULL with a 16-bit param[i] is its float32 master weight [numel[i]]:
 * it is read and updated in float32 and param[i] is only WRITTEN, with the round-to-nearest-even conversion of
 * aecf_cast_f32_to_bf16 / _f16 (param == master.to(dtype) bit for bit).  Without a master the parameter is widened, updated in
 * float32 and rounded once on the store.  (A master beside a float32 parameter is ignored.)  Tensors with numel[i] == 0 are
 * skipped, their pointers are not read.
 * Launch-wide DEVICE float32 scalars, each may be NULL:
 *   lr_dev      replaces `lr` (what a tensor lr is to torch's fused AdamW): a captured step follows the value at replay time;
 *   grad_scale  the loss scale of torch.amp.GradScaler: gradients are multiplied by 1 / *grad_scale (replaces unscale_);
 *   grad_coef   the clip coefficient aecf_grad_norm wrote (out + 1): gradients are multiplied by it (replaces the in-place
 *               scaling of torch.nn.utils.clip_grad_norm_; the gradients themselves are not rewritten);
 *   found_inf, found_inf2   when either holds a non-zero value the launches write NOTHING: no parameter, master, moment or
 *               step counter changes (the skipped step of torch.amp.GradScaler / torch's fused AdamW).  Two, so that the
 *               scaler's flag and aecf_grad_norm's (out + 2) are OR-ed on the device without a launch in between.
 * Checks, before anything touches the device: n < 0 or a negative numel -> AECF_ERR_BAD_DIMS; a dtype outside the three ->
 * AECF_ERR_UNSUPPORTED; n == 0 or every tensor empty -> AECF_OK without a launch; a required pointer NULL ->
 * AECF_ERR_NULL_POINTER. */
int aecf_adamw_mp_step(int32_t n, void* const* param, const void* const* grad, void* const* master, void* const* exp_avg,
                       void* const* exp_avg_sq, void* const* step, const int64_t* numel, const int32_t* param_dtype,
                       const int32_t* grad_dtype, void* ticket, float lr, float beta1, float beta2, float eps,
                       float weight_decay, const float* lr_dev, const float* grad_scale, const float* grad_coef,
                       const float* found_inf, const float* found_inf2, void* stream);
/* aecf_adamw_mp_ema_step: aecf_adamw_mp_step (its arguments, update, ticket contract, launch grouping and checks; the moments and
 * weights it writes are bit-equal) that also keeps an exponential moving average of the weights in the SAME launch -- the
 * momentum key encoder of MoCo, the averaged weights people evaluate and ship (NOT in the reference, whose trainer has no
 * averaged model; it replaces a torch._foreach_lerp_ over every parameter plus a cast pass after the step).  New entry points
 * under ABI v10, no bump.
 *   ema            array of n device pointers, required; ema[i]: float32 [numel[i]], or NULL: tensor i has no average;
 *   ema_out        the array or any entry may be NULL; ema_out[i]: [numel[i]] of param_dtype[i], written as the
 *                  round-to-nearest-even of the new average by the conversions of aecf_cast_f32_to_bf16 / _f16
 *                  (ema_out == ema.to(dtype) bit for bit).  Beside a float32 parameter it is ignored: let `ema` BE the output;
 *   ema_decay      beta; ema_decay_dev (may be NULL): ONE device float that replaces it, read at replay time as lr_dev is.
 * After the update of an element, with w' the weight as STORED (the new float32 master, the float32 parameter itself, or --
 * 16-bit parameter without a master -- the float32 value of the rounded parameter) and om = fl(1 - beta):
 *   e' = fma(om, fl(w' - e), e)           (one rounding of the difference, one of the fused sum)
 * beta is clamped to [0, 1] on the device; a NaN beta leaves every average and ema_out as it was and the step itself goes on.
 * A non-zero found_inf / found_inf2 writes nothing, the averages included. */
int aecf_adamw_mp_ema_step(int32_t n, void* const* param, const void* const* grad, void* const* master, void* const* exp_avg,
                           void* const* exp_avg_sq, void* const* step, const int64_t* numel, const int32_t* param_dtype,
                           const int32_t* grad_dtype, void* ticket, float lr, float beta1, float beta2, float eps,
                           float weight_decay, const float* lr_dev, const float* grad_scale, const float* grad_coef,
                           const float* found_inf, const float* found_inf2, void* const* ema, void* const* ema_out,
                           float ema_decay, const float* ema_decay_dev, void* stream);
/* aecf_ema_update: the same average without an optimiser step, for tensors that had no gradient in a step and for callers on
 * another optimiser: one launch per 24 tensors, no tickets.  w' = float32(src[i]) (src_dtype[i]), the arithmetic above, so the
 * result is bit-equal to the fused step's on the same stored weights.  ema[i]: float32 [numel[i]], required; ema_out (the array
 * or any entry may be NULL): [numel[i]] of out_dtype[i] (read only where ema_out is given; an AECF_F32 output is ignored, as
 * above).  decay / decay_dev / found_inf / found_inf2 as above.  Tensors with numel[i] == 0 are skipped.
 * Checks, before anything touches the device: n < 0 or a negative numel -> AECF_ERR_BAD_DIMS; a dtype outside the three ->
 * AECF_ERR_UNSUPPORTED; n == 0 or every tensor empty -> AECF_OK without a launch; a required pointer NULL ->
 * AECF_ERR_NULL_POINTER. */
int aecf_ema_update(int32_t n, const void* const* src, const int32_t* src_dtype, void* const* ema, void* const* ema_out,
                    const int32_t* out_dtype, const int64_t* numel, float decay, const float* decay_dev,
                    const float* found_inf, const float* found_inf2, void* stream);
/* Global L2 norm of n gradients of mixed dtype (replaces the norm of torch.nn.utils.clip_grad_norm_ and the inf check of
 * torch.amp.GradScaler) in two launches, fixed summation order, no float atomics: blocks store partial sums of squares into
 * `workspace` (aecf_grad_norm_workspace_bytes(n, numel); 0 for n <= 0, NULL or a negative numel), one block adds them in index
 * order and writes three DEVICE floats:
 *   out[0] = sqrt(sum g^2) / scale                  (scale = *grad_scale, 1 when grad_scale is NULL)
 *   out[1] = min(1, max_norm / (out[0] + 1e-6))     (clip_grad_norm_'s coefficient; 1 when max_norm <= 0: norm only)
 *   out[2] = 1 if the sum is not finite, else 0.
 * Checks as above, then workspace_bytes too small -> AECF_ERR_WORKSPACE. */
size_t aecf_grad_norm_workspace_bytes(int32_t n, const int64_t* numel);
int aecf_grad_norm(int32_t n, const void* const* grad, const int32_t* grad_dtype, const int64_t* numel, float max_norm,
                   const float* grad_scale, void* workspace, size_t workspace_bytes, float* out, void* stream);

/* ---- contrastive term (BASELINE.json north_star; NOT in the reference: SURVEY.md 8a row A9, build-defined) ----
 * Row-wise L2 normalisation zn = z / max(||z||, eps) and its backward dz = (dzn - zn (dzn.zn)) * inv_norm. */
int aecf_l2norm_forward(int64_t n, int32_t d, int32_t dtype, float eps, const void* z, void* zn,
                        float* inv_norm, void* stream);
int aecf_l2norm_backward(int64_t n, int32_t d, int32_t dtype, const void* zn, const float* inv_norm,
                         const float* dzn, void* dz, void* stream);
/* The same over the n = rows * views slots of x [rows][views][d] with a padding mask [n] (uint8, non-zero = the slot is ABSENT, the
 * fusion pool's key_padding_mask row by row).  A present slot has the bits of aecf_l2norm_forward / _backward.  An absent slot is
 * never read: forward writes its row of zn as +0 and its inv_norm as 0, backward writes its row of dz as +0 -- whatever z or dzn
 * hold there (NaN, inf).  presence [n / views] (may be NULL) receives one byte per row, bit v set = view v present: the bytes the
 * aecf_nce_multi_masked_* calls read.  1 <= views <= 8, n % views == 0 (AECF_ERR_BAD_DIMS), then dtype, then NULL pointers. */
int aecf_l2norm_masked_forward(int64_t n, int32_t d, int32_t views, int32_t dtype, float eps, const void* z, const uint8_t* mask,
                               void* zn, float* inv_norm, uint8_t* presence, void* stream);
int aecf_l2norm_masked_backward(int64_t n, int32_t d, int32_t dtype, const void* zn, const float* inv_norm, const float* dzn,
                                const uint8_t* mask, void* dz, void* stream);
/* One InfoNCE direction, forward + backward in one call: local unit-norm queries q [rows,d] against all
 * (all-gathered) unit-norm keys k [cols,d]; the positive of local row i is key row_offset + i.
 *   loss_rows[i] = logsumexp_j(q_i.k_j / T) - q_i.k_pos / T                       float32 [rows]
 *   dq = coef/T * (softmax - onehot) k          float32 [rows,d]
 *   dk = coef/T * (softmax - onehot)^T q        float32 [cols,d]   (sum over ranks is the caller's reduce-scatter)
 * Two implementations, chosen by the workspace the caller hands over (the caller owns the memory):
 *   * tile-GEMM form (bf16, d % 64 == 0, temperature >= 0.025; workspace aecf_nce_workspace_bytes = rows x cols bf16 + O(rows
 *     + cols) floats): E = exp((q.k - 1)/T) is written once as bf16, its row sums come out of the same GEMM epilogue, the
 *     softmax weights are formed in place and dq / dk are two more tile GEMMs (transposed LDS reads: no transposed copies).
 *     6 rows cols d flops.  Rows of q and k MUST have L2 norm <= 1 (+ bf16 rounding): 1/T is used as the shift of every exponent.
 *   * streaming ("flash") form (bf16, d in {128, 256, 384, 512, 768, 1024}; workspace aecf_nce_stream_workspace_bytes =
 *     O(rows d)): the [rows, cols] logits are never materialised -- key tiles stream through LDS under an online max / sum per
 *     row, a second streaming pass forms dk from the saved log-sum-exp.  8 rows cols d flops; any norms, any temperature.
 *   A workspace of at least aecf_nce_workspace_bytes selects the first, a smaller one of at least
 *   aecf_nce_stream_workspace_bytes the second.  Otherwise (float32, other d): materialising float32 form, d % 64 == 0 and
 *   cols % 64 == 0. */
size_t aecf_nce_workspace_bytes(int64_t rows, int64_t cols, int32_t d, int32_t dtype);
size_t aecf_nce_stream_workspace_bytes(int64_t rows, int64_t cols, int32_t d, int32_t dtype);   /* 0: no streaming form */
int aecf_nce_fwd_bwd(int64_t rows, int64_t cols, int64_t row_offset, int32_t d, int32_t dtype,
                     float temperature, float coef, const void* q, const void* k, float* loss_rows,
                     float* dq, float* dk, void* workspace, size_t workspace_bytes, void* stream);

/* The loss side of the objective as ONE call (BASELINE.json north_star "contrastive + entropy_loss terms and their backward
 * are a second fused kernel"; README.md:205-208 of the reference for the entropy term): one InfoNCE direction exactly as
 * aecf_nce_fwd_bwd (bf16, streaming form) and, riding in its row-combine launch, CurriculumMasking.entropy_loss forward +
 * backward (ref aecf/AECFLayer.py:285-314) on entropy [n_entropy] float32:
 *   entropy_loss[0] = mean((nan_to_num(H) - log(last_seq_len) * entropy_target)^2), d_entropy = d loss / dH * entropy_upstream.
 * n_entropy == 0: contrastive term only.  Workspace: aecf_nce_workspace_bytes(rows, cols, d, AECF_BF16) (tile-GEMM form) or
 * aecf_nce_stream_workspace_bytes (streaming form), as for aecf_nce_fwd_bwd. */
int aecf_loss_fwd_bwd(int64_t rows, int64_t cols, int64_t row_offset, int32_t d, float temperature, float coef,
                      const void* q, const void* k, float* loss_rows, float* dq, float* dk, int64_t n_entropy,
                      int32_t last_seq_len, float entropy_target, const float* entropy, float entropy_upstream,
                      float* entropy_loss, float* d_entropy, void* workspace, size_t workspace_bytes, void* stream);


/* BOTH directions of the symmetric InfoNCE from ONE block of logits (build-defined, as above): local rows a [rows,d] (global
 * indices row_offset .. row_offset + rows) against all gathered keys b [cols,d], unit-norm bf16 rows, d % 64 == 0, T >= 0.025:
 *   L = coef * sum_i [ lse_j(a_i.b_j/T) - a_i.b_pos/T ]  +  coef * sum_i [ lse_i'(a_i'.b_pos/T) - a_i.b_pos/T ],  pos = row_offset + i
 * The second term's softmax runs down the COLUMNS of the global logits; a rank holds only its row block, so the column sums of
 * E = exp((a.b - 1)/T) are the one quantity ranks exchange:
 *   pass1: E (bf16, workspace), its row sums (workspace), and THIS rank's column sums col_sums [cols] (float32)
 *   caller: all-reduce (sum) of col_sums over the ranks (nothing to do on one rank)
 *   loss:  loss_rows[i] = both terms of local row i (float32 [rows]) from the summed column sums; optionally
 *          CurriculumMasking.entropy_loss forward + backward riding in the same launch (arguments as aecf_loss_fwd_bwd;
 *          n_entropy == 0: off).  Also prepares the normalisers the gradients need (kept in the workspace).
 *   grads: da = dL/da [rows,d]; db = this rank's share of dL/db [cols,d] (the sum over ranks is the caller's reduce-scatter), both
 *          multiplied by upstream[0] when `upstream` (a DEVICE float32 scalar: the gradient arriving at this term; no host read)
 *          is given, in float32 or -- one rounding of the float32 sums -- bf16 (grad_dtype).  May run long after `loss` (an
 *          autograd backward): the workspace must be left alone in between; it overwrites E with the softmax weights, so it
 *          runs once per pass1.
 * 6 rows cols d MFMA flops for both directions (2 for the logits, 2 + 2 for the gradient products through transposed LDS
 * reads) against 16 rows cols d for two calls of the streaming form.  Workspace: rows x cols bf16 + O(rows + cols) floats. */
size_t aecf_nce_sym_workspace_bytes(int64_t rows, int64_t cols, int32_t d);
int aecf_nce_sym_pass1(int64_t rows, int64_t cols, int32_t d, float temperature, const void* a, const void* b,
                       void* workspace, size_t workspace_bytes, float* col_sums, void* stream);
int aecf_nce_sym_loss(int64_t rows, int64_t cols, int64_t row_offset, int32_t d, float temperature, const void* a,
                      const void* b, const float* col_sums, void* workspace, size_t workspace_bytes, float* loss_rows,
                      int64_t n_entropy, int32_t last_seq_len, float entropy_target, const float* entropy,
                      float entropy_upstream, float* entropy_loss, float* d_entropy, void* stream);
int aecf_nce_sym_grads(int64_t rows, int64_t cols, int64_t row_offset, int32_t d, float temperature, float coef,
                       const void* a, const void* b, void* workspace, size_t workspace_bytes, const float* upstream,
                       int32_t grad_dtype, void* da, void* db, void* stream);

/* ---- device temperature: the five calls above with T read from device memory (a learnable temperature) ----
 * `temperature` is a DEVICE float32 scalar; the kernels use Tc = max(*temperature, min_temperature) (min_temperature > 0, a host
 * float) and derive 1/Tc on the device with the float operations the host uses for a float T: a device T equal to a float T
 * gives bit-identical outputs.  Nothing is read on the host, so the calls can be captured in a graph and replay the value the
 * scalar holds at replay time.  The form is chosen from dtype, d, the workspace and min_temperature, never from T: the tile
 * forms need min_temperature >= 0.025 (the constant shift 1/T of their exponentials; the sym calls answer
 * AECF_ERR_UNSUPPORTED below it, aecf_nce_fwd_bwd_dt / aecf_loss_fwd_bwd_dt take the streaming or materialising form).
 * d_temperature (DEVICE float32 scalar, may be NULL = not wanted) is WRITTEN, not accumulated, with
 *   dL/dT = -(1/Tc) sum_i q_i . dq_i      (0 where *temperature < min_temperature: the gradient of clamp(T, min))
 * for this call's term: one direction at upstream 1 (aecf_nce_fwd_bwd_dt, aecf_loss_fwd_bwd_dt: scale it as dq / dk), both
 * directions of THIS rank's rows times upstream[0] (aecf_nce_sym_grads_dt: the shares of the ranks sum to the global value).
 * It is reduced in a fixed order from the float32 gradient before any rounding (one extra single-block launch); no float
 * atomics.  Checks before any launch: sizes, then dtype (float16: AECF_ERR_UNSUPPORTED) and the tile form's min_temperature,
 * then NULL pointers (temperature included). */
int aecf_nce_fwd_bwd_dt(int64_t rows, int64_t cols, int64_t row_offset, int32_t d, int32_t dtype,
                        const float* temperature, float min_temperature, float coef, const void* q, const void* k,
                        float* loss_rows, float* dq, float* dk, float* d_temperature, void* workspace,
                        size_t workspace_bytes, void* stream);
int aecf_loss_fwd_bwd_dt(int64_t rows, int64_t cols, int64_t row_offset, int32_t d, const float* temperature,
                         float min_temperature, float coef, const void* q, const void* k, float* loss_rows, float* dq,
                         float* dk, float* d_temperature, int64_t n_entropy, int32_t last_seq_len, float entropy_target,
                         const float* entropy, float entropy_upstream, float* entropy_loss, float* d_entropy,
                         void* workspace, size_t workspace_bytes, void* stream);
int aecf_nce_sym_pass1_dt(int64_t rows, int64_t cols, int32_t d, const float* temperature, float min_temperature,
                          const void* a, const void* b, void* workspace, size_t workspace_bytes, float* col_sums,
                          void* stream);
int aecf_nce_sym_loss_dt(int64_t rows, int64_t cols, int64_t row_offset, int32_t d, const float* temperature,
                         float min_temperature, const void* a, const void* b, const float* col_sums, void* workspace,
                         size_t workspace_bytes, float* loss_rows, int64_t n_entropy, int32_t last_seq_len,
                         float entropy_target, const float* entropy, float entropy_upstream, float* entropy_loss,
                         float* d_entropy, void* stream);
int aecf_nce_sym_grads_dt(int64_t rows, int64_t cols, int64_t row_offset, int32_t d, const float* temperature,
                          float min_temperature, float coef, const void* a, const void* b, void* workspace,
                          size_t workspace_bytes, const float* upstream, int32_t grad_dtype, void* da, void* db,
                          float* d_temperature, void* stream);

/* ---- sigmoid contrastive loss (SigLIP; build-defined like the InfoNCE term: the reference has no contrastive term) ----
 * Local rows a [rows,d] (global indices row_offset .. row_offset + rows) against all gathered rows b [cols,d] of the other view,
 * unit-norm bf16 rows, d % 64 == 0, any row and column counts (rows <= cols).  The temperature and the bias are DEVICE float32
 * scalars (learnable; nothing is read on the host, so the calls capture into a graph):
 *   Tc    = max(*temperature, min_temperature)            (any min_temperature > 0: no exponent shift, no 0.025 floor)
 *   l_ij  = (a_i . b_j) / Tc + *bias
 *   L     = coef * sum_ij softplus(-y_ij l_ij)            y_ij = +1 if j == row_offset + i else -1,  coef = 1 / cols
 *   g_ij  = sigmoid(l_ij) - [j == row_offset + i]         (the positive's entry is formed as -sigmoid(-l))
 *   da    = coef/Tc * upstream * g b        db = coef/Tc * upstream * g^T a        dbias = coef * sum_ij g_ij
 *   dT    = -(1/Tc) sum_i a_i . da_i   (0 where *temperature < min_temperature)
 * Every logit is its own binary term: no row or column normaliser, nothing to exchange between the two calls.
 *   pass1: the logits GEMM with g written ONCE as bf16 into the workspace by its epilogue (softplus as max(x, 0) +
 *          log1p(exp(-|x|)) in exact-residual form; padded rows and columns are stored as 0 and enter no sum);
 *          loss_rows[i] = sum_j softplus(-y_ij l_ij)  (float32 [rows]) and d_bias[0] = sum_ij g_ij  -- both WITHOUT coef:
 *          pass1 does not take it; the caller multiplies (d_bias is this rank's share at upstream 1, from the float32 g before
 *          its rounding).
 *   grads: da [rows,d] and this rank's share of db [cols,d] (the sum over ranks is the caller's reduce-scatter), float32 or --
 *          one rounding of the float32 sums -- bf16 (grad_dtype).  g is stored unscaled; coef / Tc and upstream[0] (`upstream`:
 *          a DEVICE float32 scalar, NULL = 1) are applied to the float32 sums in the output stage of the two products.
 *          d_temperature (may be NULL = not wanted) is this rank's share of dL/dT times upstream[0].  The workspace is only
 *          read: grads may run any number of times after one pass1, with T unchanged in between.
 * d_bias and d_temperature are WRITTEN, not accumulated; all sums are reduced in a fixed order from float32 partials (no float
 * atomics: the same inputs give the same bits).  Caller-owned buffers, a stream argument, no allocation, no synchronisation.
 * Checks before any launch: sizes, then dtype / shape support (d % 64 != 0, a grad_dtype other than bf16 / float32:
 * AECF_ERR_UNSUPPORTED), then NULL pointers, then the workspace size.  6 rows cols d MFMA flops.
 * Workspace: rows x cols bf16 + O((rows + cols) (cols / 256 + d)) floats; aecf_sig_workspace_bytes answers 0 where the
 * shape is not served. */
size_t aecf_sig_workspace_bytes(int64_t rows, int64_t cols, int32_t d);
int aecf_sig_pass1(int64_t rows, int64_t cols, int64_t row_offset, int32_t d, const float* temperature, float min_temperature,
                   const float* bias, const void* a, const void* b, void* workspace, size_t workspace_bytes,
                   float* loss_rows, float* d_bias, void* stream);
int aecf_sig_grads(int64_t rows, int64_t cols, int64_t row_offset, int32_t d, const float* temperature, float min_temperature,
                   float coef, const void* a, const void* b, void* workspace, size_t workspace_bytes, const float* upstream,
                   int32_t grad_dtype, void* da, void* db, float* d_temperature, void* stream);

/* The same loss in ONE call that never holds the rows x cols block: the streaming form, for batches whose g does not fit.  Same
 * inputs and formulas (bf16 unit-norm rows, device T and bias, Tc = max(*temperature, min_temperature), y_ij = +1 only on
 * j == row_offset + i), d in {128, 256, 384, 512, 768, 1024}:
 *   l_ij = (a_i . b_j) / Tc + *bias        g_ij = sigmoid(l_ij) - [j == row_offset + i]
 *   loss_rows[i] = sum_j softplus(-y_ij l_ij)          float32 [rows], WITHOUT coef
 *   d_bias[0]    = sum_ij g_ij                         WITHOUT coef, from the float32 g
 *   da = coef/Tc g b   float32 [rows,d]        db = coef/Tc g^T a   float32 [cols,d] (this rank's share)       at upstream 1
 *   d_temperature[0] = -(1/Tc) sum_i a_i . da_i        (0 where *temperature < min_temperature)
 * Two roles of one kernel, each a single independent pass (no maximum, no normaliser, nothing handed from one to the other): da
 * with the rows of a held in registers and b streamed through LDS, its column range split over blocks and the splits' float32
 * partials added in a fixed order by a combine launch that also leaves d_bias and d_temperature; db with the rows of b held and
 * a streamed, no partials.  g is rounded to bf16 only as the operand of the gradient products; every scalar sum takes the
 * float32 value.  No float atomics: the same inputs give the same bits.  d_bias and d_temperature are WRITTEN, not accumulated,
 * and may be NULL (= not wanted).
 * Loss-only mode: da == db == NULL runs the first role without its gradient product and writes loss_rows alone (d_bias and
 * d_temperature are ignored and may be NULL); loss_rows has the same bits as with gradients.
 * 8 rows cols d MFMA flops (each role forms the logits: 2 + 2, and 2 + 2 for the products) against the tile form's 6; at
 * d = 768 and d = 1024 the output columns of each role come from two launches that both form the logits (12 rows cols d).
 * Workspace, in order: [splits, rows, d] float32 da partials | [splits, rows] softplus sums | [splits, rows] g sums |
 * [rows] sum_j g_ij | [rows] a_i . da_i; splits <= 64 does not grow with cols beyond that.  aecf_sig_stream_workspace_bytes
 * answers 0 where the width is not served.  Caller-owned buffers, a stream argument, no allocation, no synchronisation, nothing
 * read on the host.  Checks before any launch: sizes (AECF_ERR_BAD_DIMS), then the width (AECF_ERR_UNSUPPORTED), then NULL among
 * temperature, bias, a, b, loss_rows, workspace or exactly one of da / db NULL (AECF_ERR_NULL_POINTER), then the workspace
 * size (AECF_ERR_WORKSPACE). */
size_t aecf_sig_stream_workspace_bytes(int64_t rows, int64_t cols, int32_t d);      /* 0: width not served */
int aecf_sig_stream_fwd_bwd(int64_t rows, int64_t cols, int64_t row_offset, int32_t d, const float* temperature,
                            float min_temperature, const float* bias, float coef, const void* a, const void* b,
                            float* loss_rows, float* d_bias, float* d_temperature, float* da, float* db,
                            void* workspace, size_t workspace_bytes, void* stream);

/* ---- supervised contrastive loss (Khosla et al. 2020, the "L_out" form; build-defined like the InfoNCE term) ----
 * One direction: local unit-norm bf16 rows q [rows,d] (global indices row_offset .. row_offset + rows) against all gathered
 * unit-norm bf16 rows k [cols,d] of the other view, d in {128, 256, 384, 512, 768, 1024}, with int64 DEVICE labels q_labels [rows]
 * and k_labels [cols].  Every key that carries the query's label is a positive beside the partner:
 *   match(i, j) = (j == row_offset + i) or (q_labels[i] >= 0 and q_labels[i] == k_labels[j])
 *                 a negative label = unlabeled: the partner only, and two unlabeled rows never match; all 64 bits are compared;
 *                 the partner counts by INDEX, whatever the two labels say
 *   n_i    = sum_j match(i, j)   (>= 1)        Tc = max(*temperature, min_temperature)   (a DEVICE float32 scalar, as above)
 *   x_ij   = (q_i . k_j) / Tc                  lse_i = logsumexp_j x_ij
 *   loss_rows[i] = lse_i - (1 / n_i) sum_j match(i, j) x_ij                  float32 [rows], WITHOUT coef
 *   G      = softmax_j(x) - match / n_i
 *   dq = coef/Tc G k   float32 [rows,d]        dk = coef/Tc G^T q   float32 [cols,d] (this rank's share)        at upstream 1
 *   d_temperature[0] = -(1/Tc) sum_i q_i . dq_i    (0 where *temperature < min_temperature; WRITTEN, may be NULL = not wanted)
 * With every label negative, or all labels distinct, this is the InfoNCE direction of aecf_nce_fwd_bwd_dt.
 * Three passes of the streaming loop, nothing of size rows x cols anywhere (neither logits nor a match mask): statistics
 * (running maximum and sum, the count and the float32 sum of the matched x per row; the key range split over blocks, the live
 * splits merged in a fixed order into lse, 1 / n and loss_rows), then dq (the same split; weights coef/Tc (exp(x - lse) - match /
 * n), partial sums per live split added in a fixed order) and dk (one pass, no partials).  The normaliser is known before either
 * gradient pass, so no accumulator is ever rescaled.  A weight is rounded to bf16 once, as the operand of the gradient products.
 * No float atomics: the same inputs give the same bits.
 * Loss-only mode: dq == dk == NULL runs the statistics and the merge alone; d_temperature must then be NULL too; loss_rows has the
 * same bits as with gradients.
 * Workspace, in order, with splits the rule's count (<= 64, does not grow with cols beyond that): [splits, rows, d] float32 dq
 * partials | [splits, rows] m | l | count (int32) | matched-x sums | [rows] lse | 1 / n | q_i . dq_i, + 1024 bytes:
 * (splits * rows * (d + 4) + 3 * rows) * 4 + 1024.  aecf_supcon_workspace_bytes answers 0 where the width is not served.
 * Caller-owned buffers, a stream argument, no allocation, no synchronisation, nothing read on the host (the call captures into a
 * graph), nothing read from the workspace before it is written.  Checks before any launch: sizes (rows, cols, d > 0,
 * cols < 2^31, min_temperature > 0, 0 <= row_offset, row_offset + rows <= cols: AECF_ERR_BAD_DIMS), then the width (AECF_ERR_UNSUPPORTED),
 * then NULL among temperature, q, k, q_labels, k_labels, loss_rows, workspace, exactly one of dq / dk NULL, or d_temperature
 * given without dq / dk (AECF_ERR_NULL_POINTER), then the workspace size (AECF_ERR_WORKSPACE). */
size_t aecf_supcon_workspace_bytes(int64_t rows, int64_t cols, int32_t d);      /* 0: not served */
int aecf_supcon_fwd_bwd(int64_t rows, int64_t cols, int64_t row_offset, int32_t d, const float* temperature,
                        float min_temperature, float coef, const void* q, const void* k, const int64_t* q_labels,
                        const int64_t* k_labels, float* loss_rows, float* dq, float* dk, float* d_temperature,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ---- the pooled forms: NT-Xent (SimCLR) and the supervised contrastive loss over BOTH views ----
 * aecf_supcon_fwd_bwd with ONE key excluded per row.  The caller puts both views into one key buffer k [cols,d] (the Python layer:
 * the gathered rows of view b, then those of view a) with their labels k_labels [cols]; local row i (a row of either view) has its
 * partner at row_offset + i and ITSELF at self_offset + i, and the latter takes no part in anything:
 *   match(i, j) = j != self_offset + i and ((j == row_offset + i) or (q_labels[i] >= 0 and q_labels[i] == k_labels[j]))
 *                 the exclusion comes first: the excluded key usually carries the row's own label and the highest score, 1/Tc
 *   n_i    = sum_j match(i, j)   (>= 1: the partner)                  x_ij = (q_i . k_j) / Tc
 *   lse_i  = logsumexp over j != self_offset + i of x_ij
 *   loss_rows[i] = lse_i - (1 / n_i) sum_j match(i, j) x_ij            float32 [rows], WITHOUT coef
 *   G_ij   = softmax over j != self_offset + i of x_ij - match / n_i,  G_ij = 0 at j = self_offset + i
 *   dq = coef/Tc G k        dk = coef/Tc G^T q  (dk[self_offset + i] gets nothing from row i, and the other rows' shares)
 *   d_temperature[0] = -(1/Tc) sum_i q_i . dq_i    (0 where *temperature < min_temperature; WRITTEN, may be NULL = not wanted)
 * With every label negative this is one half of NT-Xent: 2 B anchors, each against the other 2 B - 1 rows of both views.
 * The same three passes, SELF instances of the same kernels: the excluded key's x is -inf in the statistics pass (a sub-tile or a
 * whole split whose only valid key is excluded for a row leaves that row at m = -inf, l = 0, count = 0, sum = 0, which the merge
 * skips) and its weight is 0 in both gradient passes.  Loss-only mode, the workspace (layout and size: aecf_supcon_workspace_bytes
 * answers for both calls), no atomics, no host read, capturable: all as aecf_supcon_fwd_bwd.  Checks, in its order: sizes (those
 * of aecf_supcon_fwd_bwd, and 0 <= self_offset, self_offset + rows <= cols, self_offset != row_offset: AECF_ERR_BAD_DIMS), the
 * width (AECF_ERR_UNSUPPORTED), the pointers (AECF_ERR_NULL_POINTER), the workspace size (AECF_ERR_WORKSPACE). */
int aecf_supcon_pool_fwd_bwd(int64_t rows, int64_t cols, int64_t row_offset, int64_t self_offset, int32_t d,
                             const float* temperature, float min_temperature, float coef, const void* q, const void* k,
                             const int64_t* q_labels, const int64_t* k_labels, float* loss_rows, float* dq, float* dk,
                             float* d_temperature, void* workspace, size_t workspace_bytes, void* stream);

/* ---- supervised contrastive loss, tile-GEMM form: BOTH directions of the symmetric loss from ONE block of logits ----
 * The symmetric loss gives both views the same labels, so the match relation is symmetric and one match matrix serves both
 * directions.  This rank owns its local rows a [rows,d] of one view (global indices row_offset .. row_offset + rows) against all
 * gathered rows b [cols,d] of the other view, unit-norm bf16 rows, with int64 DEVICE labels row_labels [rows], col_labels [cols]:
 *   m_ij  = (j == row_offset + i) or (row_labels[i] >= 0 and row_labels[i] == col_labels[j])
 *           all 64 bits compared; a negative label = unlabeled, never a match; the partner counts by INDEX, whatever the labels say
 *   x_ij  = a_i . b_j / Tc,  Tc = max(*temperature, min_temperature),  E_ij = exp(x_ij - 1/Tc)   (the shift of the InfoNCE tile form)
 *   l_i   = sum_j E_ij      n_i  = sum_j m_ij      s_i  = sum_j m_ij x_ij        row statistics, this rank's rows
 *   c_j   = sum_i E_ij      nc_j = sum_i m_ij      sc_j = sum_i m_ij x_ij        column statistics, summed over the ranks
 *   loss_rows[i] = [log l_i + 1/Tc - s_i / n_i] + [log c_p + 1/Tc - sc_p / nc_p],   p = row_offset + i        WITHOUT coef
 *   W_ij  = coef/Tc * upstream * ( E_ij (1/l_i + 1/c_j) - m_ij (1/n_i + 1/nc_j) )
 *   da = W b [rows,d]      db = W^T a [cols,d] (this rank's share)      dT = -(1/Tc) sum_i a_i . da_i  (0 where *temperature < min_temperature)
 * The column direction is DEFINED on the transposed match matrix of the same call, and every column counts its partner once:
 * nc = 1 + the matches by label.  With labels shared by the views this is the sum of two aecf_supcon_fwd_bwd directions (a against
 * b and b against a); with every label negative, or all labels distinct, every output has the bits of aecf_nce_sym_pass1_dt /
 * _loss_dt / _grads_dt on the same inputs.
 *   pass1: the logits GEMM.  Its epilogue writes E once as bf16 (workspace), leaves the row and column sums of E exactly as the
 *          InfoNCE form does, and the count and float32 sum of the raw scores a_i . b_j of the matches BY LABEL (the partner
 *          excluded: it is added from its own float32 dot later) per row and per column of every tile; fixed-order partials, no
 *          atomics.  col_stats [3][cols] float32 gets this rank's column statistics: c | count | raw-score sum.  Counts travel
 *          as float32 (exact: cols <= 2^24), so ONE all-reduce carries all three.
 *   caller: all-reduce (sum) of col_stats over the ranks (nothing to do on one rank)
 *   loss:  loss_rows [rows] from the summed col_stats, with n = 1 + count and s = (dot + sum) / Tc in both directions; prepares
 *          1/l, 1/n (rows) and 1/c, 1/nc (columns) in the workspace.
 *   grads: the weights in place over E (m formed again from the labels), then da and this rank's share of db as in
 *          aecf_nce_sym_grads_dt: float32 or -- one rounding of the float32 sums -- bf16 (grad_dtype), multiplied by upstream[0]
 *          (a DEVICE float32 scalar, NULL = 1); d_temperature (may be NULL) is WRITTEN with this rank's share of dL/dT times
 *          upstream[0].  It consumes the stored block: it runs once per pass1.
 * Served: bf16 rows, d % 64 == 0, 64 <= d <= 4096, min_temperature >= 0.025 (1/Tc is the constant shift of every exponential),
 * cols <= 2^24.  6 rows cols d MFMA flops for both directions against 16 for two streaming calls.
 * Workspace, in order, each piece rounded up to 256 bytes, Rp / Cp = rows / cols rounded up to 256, + 256 bytes:
 *   E [Rp][Cp] bf16 | row partials [3][Cp/256][Rp] | column partials [3][Rp/256][Cp] | row statistics [3][Rp] | 1/l [Rp] |
 *   1/n [Rp] | 1/c [Cp] | 1/nc [Cp] | the partner's exponential [Rp] | da slabs [splits][rows][d]   (float32 but E; splits: the K
 *   split of da = W b, as in the InfoNCE form).  The query answers 0 where the shape is not served (d, cols > 2^24).
 * Caller-owned buffers, a stream argument, no allocation, no synchronisation, nothing read on the host (the calls capture into a
 * graph), nothing read from the workspace before it is written; no float atomics: the same inputs give the same bits.  Checks
 * before any launch, as for the streaming call: sizes (rows, cols, d > 0, cols < 2^31, min_temperature > 0, 0 <= row_offset,
 * row_offset + rows <= cols: AECF_ERR_BAD_DIMS), then d, min_temperature < 0.025, cols > 2^24 or a grad_dtype other than bf16 /
 * float32 (AECF_ERR_UNSUPPORTED), then NULL pointers (AECF_ERR_NULL_POINTER; upstream and d_temperature may be NULL), then the
 * workspace size (AECF_ERR_WORKSPACE). */
size_t aecf_supcon_sym_workspace_bytes(int64_t rows, int64_t cols, int32_t d);      /* 0: not served */
int aecf_supcon_sym_pass1(int64_t rows, int64_t cols, int64_t row_offset, int32_t d, const float* temperature,
                          float min_temperature, const void* a, const void* b, const int64_t* row_labels,
                          const int64_t* col_labels, void* workspace, size_t workspace_bytes,
                          float* col_stats /* [3][cols] */, void* stream);
int aecf_supcon_sym_loss(int64_t rows, int64_t cols, int64_t row_offset, int32_t d, const float* temperature,
                         float min_temperature, const void* a, const void* b, const float* col_stats /* summed over ranks */,
                         void* workspace, size_t workspace_bytes, float* loss_rows, void* stream);
int aecf_supcon_sym_grads(int64_t rows, int64_t cols, int64_t row_offset, int32_t d, const float* temperature,
                          float min_temperature, float coef, const void* a, const void* b, const int64_t* row_labels,
                          const int64_t* col_labels, void* workspace, size_t workspace_bytes, const float* upstream,
                          int32_t grad_dtype, void* da, void* db, float* d_temperature, void* stream);

/* ---- NT-Xent, tile-GEMM form (build-defined; the pooled loss of aecf_supcon_pool_fwd_bwd with every label negative) ----
 * NT-Xent (SimCLR) over ONE pool of the 2 cols rows of both views: every row is an anchor, its positive is its partner in the other
 * view, its negatives are the other 2 cols - 2 rows of BOTH views, itself left out.  A rank holds its local rows a_loc, b_loc
 * [rows,d] (global rows row_offset .. row_offset + rows) and the gathered a_all, b_all [cols,d], unit-norm bf16 rows; a_all / b_all
 * may alias a_loc / b_loc on one rank.  Tc = max(*temperature, min_temperature), E(s) = exp((s - 1) / Tc).  Three logits blocks:
 *   X = a_loc . b_all^T   partner at column row_offset + i              row sums lX_i, this rank's column sums cX_j
 *   Y = a_loc . a_all^T   the anchor itself at column row_offset + i, EXCLUDED BY INDEX (E = 0 stored and summed)   row sums lY_i
 *   Z = b_loc . b_all^T   the same                                                                                   row sums lZ_i
 * The b x a block is X^T and is never formed.  Denominators: anchors of view a, Da_i = lX_i + lY_i (local); anchors of view b,
 * Db_j = sum over ranks of cX_j, plus lZ of the rank that owns row j.  With s_i = a_i . b_(row_offset + i):
 *   loss_rows[i] = [log Da_i + 1/Tc - s_i/Tc] + [log Db_(row_offset + i) + 1/Tc - s_i/Tc]         both anchors of pair i, WITHOUT coef
 *   W_X = ct (E_X (1/Da_i + 1/Db_j) - 2 [j == row_offset + i])    W_Y = ct E_Y / Da_i    W_Z = ct E_Z / Db_(row_offset + i)
 *         ct = coef / Tc * upstream; W_Y and W_Z are 0 at the excluded key
 *   d_a_loc = W_X b_all + W_Y a_all [rows,d]     d_b_loc = W_Z b_all [rows,d]
 *   d_a_all = W_Y^T a_loc [cols,d]               d_b_all = W_X^T a_loc + W_Z^T b_loc [cols,d]        (this rank's shares)
 *   dT = -(1/Tc) [ sum_i a_i . d_a_loc_i + sum_i b_i . d_b_loc_i ]   (0 where *temperature < min_temperature)
 * The shares of the ranks sum to the global gradients.
 *   pass1: the three logits GEMMs.  X is aecf_nce_sym_pass1_dt to the bit; Y and Z run an epilogue of their own that leaves the
 *          excluded key out by its index, never by its value, and writes row sums only.  Then Da = lX + lY (workspace) and
 *          col_sums [cols] float32 = this rank's cX, plus lZ on its own range [row_offset, row_offset + rows): one float32
 *          addition each, fixed order, no atomics.
 *   caller: all-reduce (sum) of col_sums over the ranks (nothing to do on one rank): it then holds Db.
 *   loss:  loss_rows [rows] from Da and the summed col_sums; prepares 1/Da and 1/Db in the workspace.
 *   grads: the three weights passes in place over the blocks, then the six products.  Where two products land on one output
 *          (d_a_loc, d_b_all) they are summed in float32 and rounded ONCE to grad_dtype (float32 or bf16); everything is multiplied
 *          by upstream[0] (a DEVICE float32 scalar, NULL = 1); d_temperature (may be NULL) is WRITTEN with this rank's share of
 *          dL/dT times upstream[0], reduced in a fixed order from float32 partials.  It consumes the stored blocks: it runs once
 *          per pass1.
 * Only the device-temperature form exists.  Served: bf16 rows, d % 64 == 0, 64 <= d <= 4096, min_temperature >= 0.025 (1/Tc is
 * the constant shift of every exponential), rows <= cols.  18 rows cols d MFMA flops (three logits blocks and six gradient
 * products of 2 rows cols d each) against 64 for the two pooled streaming directions.
 * Workspace, in order, each piece rounded up to 256 bytes, Rp / Cp = rows / cols rounded up to 256, + 256 bytes:
 *   E_X | E_Y | E_Z, each [Rp][Cp] bf16 | row partials [Cp/256][Rp] | column partials [Rp/256][Cp] | Da [Rp] | lY [Rp] | lZ [Rp] |
 *   1/Da [Rp] | 1/Db [Cp] | 1/Db at the partner [Rp] | the partner's exponential [Rp] | zeros [Cp] |
 *   dT partials [3][32][16][Rp/256] | da slabs [2 splits][rows][d] | d_b_all stage [2][cols][d]
 *   (float32 but E; splits: the K split of da = W b, as in the InfoNCE form).  The query answers 0 where the shape is not served.
 * Caller-owned buffers, a stream argument, no allocation, no synchronisation, nothing read on the host, nothing read from the
 * workspace before it is written; no float atomics: the same inputs give the same bits.  Checks before any launch, in the order
 * of the supervised tile form: sizes (rows, cols, d > 0, cols < 2^31, min_temperature > 0, 0 <= row_offset, row_offset + rows <=
 * cols: AECF_ERR_BAD_DIMS), then d, min_temperature < 0.025 or a grad_dtype other than bf16 / float32 (AECF_ERR_UNSUPPORTED),
 * then NULL pointers (AECF_ERR_NULL_POINTER; upstream and d_temperature may be NULL), then the workspace size
 * (AECF_ERR_WORKSPACE). */
size_t aecf_ntxent_sym_workspace_bytes(int64_t rows, int64_t cols, int32_t d);      /* 0: not served */
int aecf_ntxent_sym_pass1(int64_t rows, int64_t cols, int64_t row_offset, int32_t d, const float* temperature,
                          float min_temperature, const void* a_loc, const void* b_loc, const void* a_all, const void* b_all,
                          void* workspace, size_t workspace_bytes, float* col_sums /* [cols] */, void* stream);
int aecf_ntxent_sym_loss(int64_t rows, int64_t cols, int64_t row_offset, int32_t d, const float* temperature,
                         float min_temperature, const void* a_loc, const void* b_all, const float* col_sums /* summed over ranks */,
                         void* workspace, size_t workspace_bytes, float* loss_rows, void* stream);
int aecf_ntxent_sym_grads(int64_t rows, int64_t cols, int64_t row_offset, int32_t d, const float* temperature,
                          float min_temperature, float coef, const void* a_loc, const void* b_loc, const void* a_all,
                          const void* b_all, void* workspace, size_t workspace_bytes, const float* upstream, int32_t grad_dtype,
                          void* d_a_loc, void* d_b_loc, void* d_a_all, void* d_b_all, float* d_temperature, void* stream);

/* ---- InfoNCE with a key queue, tile-GEMM form (build-defined; MoCo's queue / cross-batch memory for the symmetric loss) ----
 * The symmetric InfoNCE of aecf_nce_sym_*_dt with stored keys of past steps as further negatives.  A rank holds its local rows
 * a_loc, b_loc [rows,d] (global rows row_offset .. row_offset + rows), the gathered b_all [cols,d] (it may alias b_loc on one rank)
 * and two ring buffers Qa, Qb [q_cap,d] of past keys of view a / view b, all unit-norm bf16 rows.  V = *q_valid is a DEVICE int64
 * with 0 <= V <= q_cap (clamped into that range): slots 0 .. V - 1 of either queue are keys, negatives of the OTHER view's anchors.
 * Tc = max(*temperature, min_temperature), E(s) = exp((s - 1) / Tc).  Three logits blocks:
 *   X = a_loc . b_all^T   partner at column row_offset + i                      row sums lX_i, this rank's column sums cX_j
 *   U = a_loc . Qb^T      columns j >= V EXCLUDED BY INDEX (E = 0 stored and summed)   row sums lU_i
 *   W = b_loc . Qa^T      the same                                                     row sums lW_i
 * Denominators: anchors of view a, Da_i = lX_i + lU_i (local); anchors of view b, Db_j = sum over ranks of cX_j, plus lW of the rank
 * that owns row j.  With s_i = a_i . b_(row_offset + i):
 *   loss_rows[i] = [log Da_i + 1/Tc - s_i/Tc] + [log Db_(row_offset + i) + 1/Tc - s_i/Tc]         both anchors of pair i, WITHOUT coef
 *   W_X = ct (E_X (1/Da_i + 1/Db_j) - 2 [j == row_offset + i])    W_U = ct E_U / Da_i    W_W = ct E_W / Db_(row_offset + i)
 *         ct = coef / Tc * upstream; a queue block has no partner: its column row_offset + i is a negative like any other
 *   d_a_loc = W_X b_all + W_U Qb [rows,d]     d_b_loc = W_W Qa [rows,d]     d_b_all = W_X^T a_loc [cols,d]   (this rank's share)
 *   dT = -(1/Tc) [ sum_i a_i . d_a_loc_i + sum_i b_i . d_b_loc_i ]   (X's column side rides in W_X; 0 where *temperature < min_temperature)
 * The queues take no gradient and no product is formed for them.  The shares of the ranks sum to the global gradients.
 *   pass1: the three logits GEMMs.  X is aecf_nce_sym_pass1_dt to the bit.  U and W run an epilogue of their own: V is read from
 *          the device once per block; a tile wholly below V runs the unmasked tile's code, a tile wholly at or above V stores
 *          zeros without running its K loop, the tile V crosses tests every column's index.  Exclusion is never by value: what a
 *          slot at or above V holds cannot reach a sum, a bit-identical twin of a partner below V counts.  Then Da = lX + lU
 *          (workspace) and col_sums [cols] float32 = this rank's cX, plus lW on its own range [row_offset, row_offset + rows): one
 *          float32 addition each, fixed order, no atomics.
 *   caller: all-reduce (sum) of col_sums over the ranks (nothing to do on one rank): it then holds Db.
 *   loss:  loss_rows [rows] from Da and the summed col_sums; prepares 1/Da and 1/Db in the workspace.
 *   grads: the three weights passes in place over the blocks, then the four products.  d_a_loc is ONE float32 sum over the slabs of
 *          W_X b_all with those of W_U Qb behind them, rounded once to grad_dtype (float32 or bf16); everything is multiplied by
 *          upstream[0] (a DEVICE float32 scalar, NULL = 1); d_temperature (may be NULL) is WRITTEN with this rank's share of dL/dT
 *          times upstream[0], reduced in a fixed order from the float32 partials of the three da-type products.  It consumes the
 *          stored blocks: it runs once per pass1.  It reads Qa and Qb again (q_valid is not read: the stored blocks carry it), so
 *          the queues must not change between pass1 and grads.  The products run over ALL q_cap slots with an exact-zero weight
 *          on the slots at or above V: those slots MUST HOLD FINITE ROWS (zeros after allocation, past keys after a wrap), or
 *          0 * inf = NaN reaches the gradients.  The cost therefore follows q_cap, not V, in the products; only the logits pass
 *          skips the tiles above V.
 * Only the device-temperature form exists.  Served: bf16 rows, d % 64 == 0, 64 <= d <= 4096, min_temperature >= 0.025 (1/Tc is
 * the constant shift of every exponential), rows <= cols < 2^31, 1 <= q_cap < 2^31.  With q_cap = cols, 14 rows cols d MFMA flops
 * (three logits blocks and four gradient products of 2 rows cols d each) against NT-Xent's 18.
 * Workspace, in order, each piece rounded up to 256 bytes, Rp / Cp / Qp = rows / cols / q_cap rounded up to 256, Zp = max(Cp, Qp),
 * + 256 bytes:
 *   E_X [Rp][Cp] bf16 | E_U [Rp][Qp] bf16 | E_W [Rp][Qp] bf16 | row partials [Zp/256][Rp] | column partials [Rp/256][Cp] | Da [Rp] |
 *   lU [Rp] | lW [Rp] | 1/Da [Rp] | 1/Db [Cp] | 1/Db at the partner [Rp] | the partner's exponential [Rp] | zeros [Zp] |
 *   dT partials [3][32][16][Rp/256] | da slabs [splits(Cp) + splits(Qp)][rows][d]
 *   (float32 but E; splits: the K split of da = W b, as in the InfoNCE form).  The query answers 0 where the shape is not served.
 * Caller-owned buffers, a stream argument, no allocation, no synchronisation, nothing read on the host, nothing read from the
 * workspace before it is written; no float atomics: the same inputs give the same bits.  Checks before any launch, in the order
 * of the NT-Xent tile form: sizes (rows, cols, d, q_cap > 0, cols and q_cap < 2^31, min_temperature > 0, 0 <= row_offset,
 * row_offset + rows <= cols: AECF_ERR_BAD_DIMS), then d, min_temperature < 0.025 or a grad_dtype other than bf16 / float32
 * (AECF_ERR_UNSUPPORTED), then NULL pointers (AECF_ERR_NULL_POINTER; upstream and d_temperature may be NULL), then the workspace
 * size (AECF_ERR_WORKSPACE).
 *
 * aecf_key_queue_push fills the two ring buffers on the device.  state is a DEVICE int64[2] = (cursor, valid); row i of the n source
 * rows src_a / src_b [n,d] goes to slot (cursor + i) mod q_cap of Qa / Qb (n > q_cap: only the last q_cap rows are written, to the
 * slots they would have ended in); then cursor = (cursor + n) mod q_cap and valid = min(valid + n, q_cap), written by a one-thread
 * launch behind the copy on the same stream, so every row copy reads the cursor the push found.  &state[1] is the q_valid of the
 * calls above.  No host read, no atomics, capturable; the same inputs give the same bits.  d % 8 == 0 (16-byte copies), any
 * 16-byte aligned row type of 2 d bytes; n = 0 launches nothing.  Checks: q_cap, d > 0, q_cap < 2^31, n >= 0 (AECF_ERR_BAD_DIMS),
 * d % 8 (AECF_ERR_UNSUPPORTED), NULL pointers (AECF_ERR_NULL_POINTER; the sources may be NULL where n == 0). */
size_t aecf_nce_queue_workspace_bytes(int64_t rows, int64_t cols, int64_t q_cap, int32_t d);      /* 0: not served */
int aecf_nce_queue_pass1(int64_t rows, int64_t cols, int64_t row_offset, int32_t d, const float* temperature,
                         float min_temperature, const void* a_loc, const void* b_loc, const void* Qa, const void* Qb, int64_t q_cap,
                         const int64_t* q_valid, const void* b_all, void* workspace, size_t workspace_bytes,
                         float* col_sums /* [cols] */, void* stream);
int aecf_nce_queue_loss(int64_t rows, int64_t cols, int64_t row_offset, int32_t d, const float* temperature,
                        float min_temperature, const void* a_loc, const void* b_all, int64_t q_cap,
                        const float* col_sums /* summed over ranks */, void* workspace, size_t workspace_bytes, float* loss_rows,
                        void* stream);
int aecf_nce_queue_grads(int64_t rows, int64_t cols, int64_t row_offset, int32_t d, const float* temperature,
                         float min_temperature, float coef, const void* a_loc, const void* b_loc, const void* Qa, const void* Qb,
                         int64_t q_cap, const int64_t* q_valid, const void* b_all, void* workspace, size_t workspace_bytes,
                         const float* upstream, int32_t grad_dtype, void* d_a_loc, void* d_b_loc, void* d_b_all,
                         float* d_temperature, void* stream);
int aecf_key_queue_push(int64_t q_cap, int32_t d, int64_t n, const void* src_a, const void* src_b, void* Qa, void* Qb,
                        int64_t* state /* device (cursor, valid) */, void* stream);

/* ---- supervised contrastive loss with a key queue, tile-GEMM form (build-defined; cross-batch memory with LABELLED past keys) ----
 * aecf_supcon_sym_* with the stored keys of aecf_nce_queue_*: a stored key of the anchor's class is a POSITIVE, every stored key a
 * term of the denominator.  A rank holds its local rows a_loc, b_loc [rows,d] with labels row_labels [rows] (shared by the two
 * views), the gathered b_all [cols,d] with col_labels [cols], the two key rings Qa, Qb [q_cap,d] and ONE ring of stored labels
 * q_labels [q_cap] (slot s of both key rings belongs to the same past row), int64 DEVICE labels, a negative label = unlabeled,
 * never a match, all 64 bits compared; V = *q_valid as above.  For anchor a_i with partner p = row_offset + i:
 *   P(i)   = {p, by INDEX} + {j != p: col_labels[j] == row_labels[i] >= 0} + {slots s < V of Qb: q_labels[s] == row_labels[i] >= 0}
 *   Da_i   = sum_j E(a_i . b_j) + sum_{s<V} E(a_i . Qb_s)                                  same-class keys stay in the denominator
 *   loss   = log Da_i + 1/Tc - (1/|P(i)|) sum_{k in P(i)} a_i . k / Tc
 * Anchor b_g is the mirror image on the transpose of the same a x b block plus the slots of Qa; loss_rows[i] is the sum of both
 * anchors of pair i, WITHOUT coef.  A slot at or above V is no key and no positive BY ITS INDEX, whatever row or label it holds; a
 * stored key is nobody's partner: a bit-identical twin of the partner below V is a key like any other, a positive only by its label.
 * Three logits blocks: X = a_loc . b_all^T runs aecf_supcon_sym_pass1's epilogue to the bit (row and column statistics: sum of E |
 * count | float32 sum of the matched raw scores); U = a_loc . Qb^T and W = b_loc . Qa^T run ONE epilogue that joins the key-queue
 * form's (the count read once per block; a tile at or above it stores zeros for E and all three row partials and skips its K loop;
 * only the crossed tile selects per column in the E loop; the count enters the search through the column keys) with the row
 * half of the label search (32-bit key vote, the 64-bit compare only in a
 * row group with a hit, no column accumulators).
 *   pass1: the three GEMMs; row statistics = X's + U's (workspace); col_stats [3][cols] float32 = this rank's column statistics of
 *          X, plus W's row statistics on its own range [row_offset, row_offset + rows): one float32 addition each, no atomics.
 *   caller: all-reduce (sum) of col_stats over the ranks (nothing to do on one rank).
 *   loss:  loss_rows [rows] by aecf_supcon_sym_loss's kernel on the combined statistics (n = 1 + count); takes no labels.
 *   grads: W_X = ct (E (1/Da_i + 1/Db_j) - m_ij (1/na_i + 1/nb_j)) as aecf_supcon_sym_grads; W_U = ct (E / Da_i - m_is / na_i) and
 *          W_W = ct (E / Db_p - m_is / nb_p) with m_is = [s < V] [q_labels[s] == row_labels[i] >= 0], V read from the device; a slot
 *          at or above V gets an exact zero.  Then the four products, the slab sum and the dT reduction of aecf_nce_queue_grads:
 *          d_a_loc = W_X b_all + W_U Qb, d_b_loc = W_W Qa, d_b_all = W_X^T a_loc; float32 or bf16 (one rounding), times upstream[0];
 *          d_temperature as there.  It consumes the stored blocks (once per pass1) and reads Qa, Qb, q_labels and *q_valid again:
 *          none of them may change between pass1 and grads.  The key slots at or above V MUST HOLD FINITE ROWS (the products read
 *          them with a zero weight); the label slots at or above V may hold anything.
 * With an empty queue (V = 0) every output has the bits of aecf_supcon_sym_*; with every label negative, those of aecf_nce_queue_*.
 * Served: bf16 unit rows, d % 64 == 0, 64 <= d <= 4096, min_temperature >= 0.025, rows <= cols, cols + q_cap <= 2^24: an anchor's
 * count 1 + (cols - 1) + q_cap adds two blocks' counts and has to stay an exact float32 integer.  The query answers 0 elsewhere.
 * Workspace, in order, each piece rounded up to 256 bytes, Rp / Cp / Qp rounded up to 256, Zp = max(Cp, Qp), + 256 bytes:
 *   E_X [Rp][Cp] bf16 | E_U [Rp][Qp] bf16 | E_W [Rp][Qp] bf16 | row partials [3][Zp/256][Rp] | column partials [3][Rp/256][Cp] |
 *   row statistics [3][Rp] | U's [3][Rp] | W's [3][Rp] | 1/Da [Rp] | 1/na [Rp] | 1/Db [Cp] | 1/nb [Cp] | 1/Db and 1/nb at the
 *   partner [Rp] each | the partner's exponential [Rp] | zeros [Zp] | dT partials [3][32][16][Rp/256] |
 *   da slabs [splits(Cp) + splits(Qp)][rows][d]      (float32 but E)
 * Caller-owned buffers, a stream argument, no allocation, no synchronisation, nothing read on the host (capturable), nothing read
 * from the workspace before it is written; no float atomics: the same inputs give the same bits.  Checks before any launch: the
 * sizes of aecf_nce_queue_* (AECF_ERR_BAD_DIMS), then d, min_temperature < 0.025, cols + q_cap > 2^24 or a grad_dtype other than
 * bf16 / float32 (AECF_ERR_UNSUPPORTED), then NULL pointers (AECF_ERR_NULL_POINTER; upstream and d_temperature may be NULL), then
 * the workspace size (AECF_ERR_WORKSPACE).
 *
 * aecf_key_queue_push_labeled is aecf_key_queue_push with the label ring Ql [q_cap] int64: the label of source row i goes to the
 * slot its keys go to, read from the cursor the push found (the label copy runs in front of the launch that bumps the state).
 * src_labels == NULL writes -1 into the slots the push fills, so that no label of an overwritten key stays attached to a new one.
 * Checks as aecf_key_queue_push, Ql among the pointers. */
size_t aecf_supcon_queue_workspace_bytes(int64_t rows, int64_t cols, int64_t q_cap, int32_t d);      /* 0: not served */
int aecf_supcon_queue_pass1(int64_t rows, int64_t cols, int64_t row_offset, int32_t d, const float* temperature,
                            float min_temperature, const void* a_loc, const void* b_loc, const void* Qa, const void* Qb,
                            int64_t q_cap, const int64_t* q_valid, const void* b_all, const int64_t* row_labels,
                            const int64_t* col_labels, const int64_t* q_labels, void* workspace, size_t workspace_bytes,
                            float* col_stats /* [3][cols] */, void* stream);
int aecf_supcon_queue_loss(int64_t rows, int64_t cols, int64_t row_offset, int32_t d, const float* temperature,
                           float min_temperature, const void* a_loc, const void* b_all, int64_t q_cap,
                           const float* col_stats /* summed over ranks */, void* workspace, size_t workspace_bytes,
                           float* loss_rows, void* stream);
int aecf_supcon_queue_grads(int64_t rows, int64_t cols, int64_t row_offset, int32_t d, const float* temperature,
                            float min_temperature, float coef, const void* a_loc, const void* b_loc, const void* Qa, const void* Qb,
                            int64_t q_cap, const int64_t* q_valid, const void* b_all, const int64_t* row_labels,
                            const int64_t* col_labels, const int64_t* q_labels, void* workspace, size_t workspace_bytes,
                            const float* upstream, int32_t grad_dtype, void* d_a_loc, void* d_b_loc, void* d_b_all,
                            float* d_temperature, void* stream);
int aecf_key_queue_push_labeled(int64_t q_cap, int32_t d, int64_t n, const void* src_a, const void* src_b,
                                const int64_t* src_labels, void* Qa, void* Qb, int64_t* Ql,
                                int64_t* state /* device (cursor, valid) */, void* stream);

/* ---- pooled supervised contrastive loss, tile-GEMM form (build-defined; aecf_supcon_pool_fwd_bwd's loss over both anchor halves) ----
 * The supervised contrastive loss of Khosla et al. over ONE pool of the 2 cols rows of both views: every row is an anchor, its
 * keys are the other 2 cols - 1 rows, its positives among them its partner in the other view (by INDEX) and every row of either
 * view with its label.  Buffers as in the NT-Xent tile form (a_loc, b_loc [rows,d], a_all, b_all [cols,d], unit-norm bf16 rows;
 * a_all / b_all may alias a_loc / b_loc on one rank), labels as in the supervised tile form: int64 DEVICE arrays row_labels [rows],
 * col_labels [cols], SHARED by the views, a negative label = unlabeled.  m_ij = [row_labels[i] == col_labels[j] >= 0], all 64 bits
 * compared.  Tc = max(*temperature, min_temperature), E(s) = exp((s - 1) / Tc).  Three logits blocks, per row i of the rank:
 *   X = a_loc . b_all^T   the partner (column row_offset + i) excluded from m, counted by index     lX, nX, sX   and columns cX, ncX, scX
 *   Y = a_loc . a_all^T   the anchor itself (column row_offset + i) excluded by INDEX: no key, no positive      lY, nY, sY
 *   Z = b_loc . b_all^T   the same                                                                              lZ, nZ, sZ
 * (l: sum of E, n: matches by label, s: float32 sum of their raw scores.)  Anchor a_i: Da = lX + lY, ka = nX + nY, sa = sX + sY,
 * local.  Anchor b_g, g = row_offset + i: Db_g = sum over ranks of cX_g + lZ_g, kb_g = sum ncX_g + nZ_g, sb_g = sum scX_g + sZ_g
 * (Z of the rank that owns row g).  With dot_i = a_i . b_g, na = 1 + ka, nb = 1 + kb:
 *   loss_rows[i] = [log Da_i + 1/Tc - (dot_i + sa_i) / na_i / Tc] + [log Db_g + 1/Tc - (dot_i + sb_g) / nb_g / Tc]      WITHOUT coef
 *   W_X = ct (E_X (1/Da_i + 1/Db_j) - m_ij (1/na_i + 1/nb_j)), the partner a positive by index with its float32 exponential
 *   W_Y = ct (E_Y / Da_i - m_ij / na_i)       W_Z = ct (E_Z / Db_g - m_ij / nb_g)       both exactly 0 at the excluded key
 *         ct = coef / Tc * upstream
 *   d_a_loc = W_X b_all + W_Y a_all [rows,d]     d_b_loc = W_Z b_all [rows,d]
 *   d_a_all = W_Y^T a_loc [cols,d]               d_b_all = W_X^T a_loc + W_Z^T b_loc [cols,d]        (this rank's shares)
 *   dT = -(1/Tc) [ sum_i a_i . d_a_loc_i + sum_i b_i . d_b_loc_i ]   (0 where *temperature < min_temperature)
 * The shares of the ranks sum to the global gradients.  With every label negative, or all labels distinct, every output has the
 * bits of aecf_ntxent_sym_pass1 / _loss / _grads on the same inputs (col_stats[0] those of col_sums).
 *   pass1: the three logits GEMMs.  X is aecf_supcon_sym_pass1 to the bit; Y and Z run an epilogue of their own (the E loop of the
 *          NT-Xent blocks, the row half of X's label search with the anchor excluded by index, no column statistics).  Then the
 *          combined row statistics (workspace) and col_stats [3][cols] float32 = this rank's column statistics of X (c | count |
 *          raw-score sum), plus Z's row statistics on its own range [row_offset, row_offset + rows): one float32 addition per
 *          quantity and side, fixed order, no atomics.
 *   caller: all-reduce (sum) of col_stats over the ranks (nothing to do on one rank): it then holds Db | kb | sb.
 *   loss:  loss_rows [rows]; prepares 1/Da, 1/na (rows) and 1/Db, 1/nb (columns) in the workspace.
 *   grads: the three weights passes in place over the blocks (m formed again from the labels), then the six products as in
 *          aecf_ntxent_sym_grads: two products on one output are summed in float32 and rounded ONCE to grad_dtype; everything is
 *          multiplied by upstream[0] (a DEVICE float32 scalar, NULL = 1); d_temperature (may be NULL) is WRITTEN with this rank's
 *          share of dL/dT times upstream[0].  It consumes the stored blocks: it runs once per pass1.
 * Served: bf16 rows, d % 64 == 0, 64 <= d <= 4096, min_temperature >= 0.025, rows <= cols, cols <= 2^23: counts travel as float32
 * and an anchor's count adds two blocks' (each at most cols - 1), so na = 1 + ka <= 2 cols - 1 is exact in float32 up to
 * cols = 2^23, half the bound of the cross-view form.  18 rows cols d MFMA flops.
 * Workspace, in order, each piece rounded up to 256 bytes, Rp / Cp = rows / cols rounded up to 256, + 256 bytes:
 *   E_X | E_Y | E_Z, each [Rp][Cp] bf16 | row partials [3][Cp/256][Rp] | column partials [3][Rp/256][Cp] |
 *   row statistics [3][Rp] (X's, then combined) | Y's [3][Rp] | Z's [3][Rp] | 1/Da [Rp] | 1/na [Rp] | 1/Db [Cp] | 1/nb [Cp] |
 *   1/Db at the partner [Rp] | 1/nb at the partner [Rp] | the partner's exponential [Rp] | zeros [Cp] |
 *   dT partials [3][32][16][Rp/256] | da slabs [2 splits][rows][d] | d_b_all stage [2][cols][d]
 *   (float32 but E; splits: the K split of da = W b, as in the InfoNCE form).  The query answers 0 where the shape is not served
 *   (d, rows > cols, cols > 2^23).
 * Caller-owned buffers, a stream argument, no allocation, no synchronisation, nothing read on the host, nothing read from the
 * workspace before it is written; no float atomics: the same inputs give the same bits.  Checks before any launch, in the order
 * of the supervised tile form: sizes (rows, cols, d > 0, cols < 2^31, min_temperature > 0, 0 <= row_offset, row_offset + rows <=
 * cols: AECF_ERR_BAD_DIMS), then d, min_temperature < 0.025, cols > 2^23 or a grad_dtype other than bf16 / float32
 * (AECF_ERR_UNSUPPORTED), then NULL pointers (AECF_ERR_NULL_POINTER; upstream and d_temperature may be NULL), then the workspace
 * size (AECF_ERR_WORKSPACE). */
size_t aecf_supcon_pool_sym_workspace_bytes(int64_t rows, int64_t cols, int32_t d);      /* 0: not served */
int aecf_supcon_pool_sym_pass1(int64_t rows, int64_t cols, int64_t row_offset, int32_t d, const float* temperature,
                               float min_temperature, const void* a_loc, const void* b_loc, const void* a_all, const void* b_all,
                               const int64_t* row_labels, const int64_t* col_labels, void* workspace, size_t workspace_bytes,
                               float* col_stats /* [3][cols] */, void* stream);
int aecf_supcon_pool_sym_loss(int64_t rows, int64_t cols, int64_t row_offset, int32_t d, const float* temperature,
                              float min_temperature, const void* a_loc, const void* b_all,
                              const float* col_stats /* summed over ranks */, void* workspace, size_t workspace_bytes,
                              float* loss_rows, void* stream);
int aecf_supcon_pool_sym_grads(int64_t rows, int64_t cols, int64_t row_offset, int32_t d, const float* temperature,
                               float min_temperature, float coef, const void* a_loc, const void* b_loc, const void* a_all,
                               const void* b_all, const int64_t* row_labels, const int64_t* col_labels, void* workspace,
                               size_t workspace_bytes, const float* upstream, int32_t grad_dtype, void* d_a_loc, void* d_b_loc,
                               void* d_a_all, void* d_b_all, float* d_temperature, void* stream);

/* ---- multi-label supervised contrastive loss (build-defined like the supervised term above, whose contract this one repeats) ----
 * One direction as above, with a SET of classes per row instead of one class: q_sets [rows] and k_sets [cols] are DEVICE arrays of
 * one uint64 per row, bit c = class c, C <= 64 classes (aecf_label_sets_pack makes them from multi-hot rows).  A key counts with a
 * weight in [0, 1]:
 *   A_i = q_sets[i], B_j = k_sets[j]
 *   w(i, j) = 1                                    if j == row_offset + i   (the partner counts by INDEX, whatever the sets say)
 *           = [ A_i & B_j != 0 ]                   weighting AECF_SETS_OVERLAP (0)
 *           = popcount(A_i & B_j) / popcount(A_i | B_j)   weighting AECF_SETS_JACCARD (1): all 64 bits, a float32 division;
 *                                                  0 when the union is empty
 *   an empty set = an unlabeled row: the partner only, and it is nobody's positive by label
 *   W_i    = sum_j w(i, j)   (>= 1)        Tc = max(*temperature, min_temperature)   (a DEVICE float32 scalar, as above)
 *   x_ij   = (q_i . k_j) / Tc              lse_i = logsumexp_j x_ij
 *   loss_rows[i] = lse_i - (1 / W_i) sum_j w(i, j) x_ij                      float32 [rows], WITHOUT coef
 *   G      = softmax_j(x) - w / W_i
 *   dq = coef/Tc G k   float32 [rows,d]        dk = coef/Tc G^T q   float32 [cols,d] (this rank's share)        at upstream 1
 *   d_temperature[0] = -(1/Tc) sum_i q_i . dq_i    (0 where *temperature < min_temperature; WRITTEN, may be NULL = not wanted)
 * With one-hot sets (class c < 64 <-> bit c, unlabeled <-> 0) both weightings give the bits of aecf_supcon_fwd_bwd; with all sets
 * empty or pairwise disjoint they are the InfoNCE direction.
 * The three passes of aecf_supcon_fwd_bwd with the weight in place of the match: the statistics pass keeps float32 sums of w and
 * of w x per row (merged over the live splits in a fixed order into lse, 1 / W and loss_rows); the gradient passes use the weights
 * coef/Tc (exp(x - lse) - w / W), rounded to bf16 once.  No float atomics: the same inputs give the same bits.
 * Loss-only mode: dq == dk == NULL runs the statistics and the merge alone; d_temperature must then be NULL too; loss_rows has the
 * same bits as with gradients.
 * Workspace: the layout and size of aecf_supcon_workspace_bytes, the count slot holding the float32 weight sum:
 * (splits * rows * (d + 4) + 3 * rows) * 4 + 1024.  aecf_supcon_ml_workspace_bytes answers 0 where the width is not served.
 * Caller-owned buffers, a stream argument, no allocation, no synchronisation, nothing read on the host (the call captures into a
 * graph), nothing read from the workspace before it is written.  Checks before any launch: sizes (rows, cols, d > 0,
 * cols < 2^31, min_temperature > 0, 0 <= row_offset, row_offset + rows <= cols: AECF_ERR_BAD_DIMS), then the width and the weighting
 * (AECF_ERR_UNSUPPORTED), then NULL among temperature, q, k, q_sets, k_sets, loss_rows, workspace, exactly one of dq / dk NULL, or
 * d_temperature given without dq / dk (AECF_ERR_NULL_POINTER), then the workspace size (AECF_ERR_WORKSPACE).
 *
 * aecf_label_sets_pack: multi_hot is a contiguous DEVICE array [rows, classes], 1 <= classes <= 64, of kind AECF_BF16, AECF_F32,
 * AECF_F16 or AECF_SETS_U8 (one byte per class: torch bool / uint8); sets[i] gets bit c where multi_hot[i, c] != 0 (-0.0 is no
 * member), the bits from `classes` up stay 0.  One wave per row, one 64-lane ballot.  Checks: rows <= 0 or classes outside 1..64
 * (AECF_ERR_BAD_DIMS), then the kind (AECF_ERR_UNSUPPORTED), then NULL (AECF_ERR_NULL_POINTER). */
#define AECF_SETS_OVERLAP 0
#define AECF_SETS_JACCARD 1
#define AECF_SETS_U8 3
size_t aecf_supcon_ml_workspace_bytes(int64_t rows, int64_t cols, int32_t d);      /* 0: not served */
int aecf_supcon_ml_fwd_bwd(int64_t rows, int64_t cols, int64_t row_offset, int32_t d, const float* temperature,
                           float min_temperature, float coef, const void* q, const void* k, const uint64_t* q_sets,
                           const uint64_t* k_sets, int32_t weighting, float* loss_rows, float* dq, float* dk,
                           float* d_temperature, void* workspace, size_t workspace_bytes, void* stream);
int aecf_label_sets_pack(int64_t rows, int32_t classes, int32_t kind, const void* multi_hot, uint64_t* sets, void* stream);

/* ---- multi-label contrastive loss, tile-GEMM form: BOTH directions of the symmetric loss from ONE block of logits ----
 * aecf_supcon_sym_* with a SET of classes per row in place of its label: row_sets [rows] and col_sets [cols] are DEVICE arrays of
 * one uint64 per row, bit c = class c (aecf_label_sets_pack makes them).  This rank's local rows a [rows,d] of one view (global
 * indices row_offset .. row_offset + rows) run against all gathered rows b [cols,d] of the other view, unit-norm bf16 rows:
 *   w_ij  = 1                                            if j == row_offset + i   (the partner, by INDEX, whatever the sets say)
 *         = [A_i & B_j != 0]                             weighting AECF_SETS_OVERLAP
 *         = popcount(A_i & B_j) / popcount(A_i | B_j)    weighting AECF_SETS_JACCARD: all 64 bits, ONE correctly rounded float32
 *                                                        division, 0 for an empty union; an empty set is nobody's positive by label
 *   x_ij  = a_i . b_j / Tc,  Tc = max(*temperature, min_temperature),  E_ij = exp(x_ij - 1/Tc)   (the shift of the InfoNCE tile form)
 *   l_i = sum_j E_ij    Wr_i = sum_j w_ij   Xr_i = sum_j w_ij x_ij      rows of this rank
 *   c_j = sum_i E_ij    Wc_j = sum_i w_ij   Xc_j = sum_i w_ij x_ij      columns, summed over the ranks
 *   loss_rows[i] = [log l_i + 1/Tc - Xr_i / Wr_i] + [log c_p + 1/Tc - Xc_p / Wc_p],   p = row_offset + i        WITHOUT coef
 *   W_ij  = coef/Tc * upstream * ( E_ij (1/l_i + 1/c_j) - w_ij (1/Wr_i + 1/Wc_j) )
 *   da = W b [rows,d]      db = W^T a [cols,d] (this rank's share)      dT = -(1/Tc) sum_i a_i . da_i  (0 where *temperature < min_temperature)
 * Both weightings are symmetric in (A, B), so one weight matrix serves both directions; the column direction is DEFINED on the
 * transpose of the same call's matrix.  With sets shared by the views this is the sum of two aecf_supcon_ml_fwd_bwd directions;
 * with all sets empty or pairwise disjoint every output has the bits of aecf_nce_sym_pass1_dt / _loss_dt / _grads_dt; with one-hot
 * sets both weightings give the same bits, the column sums of E and of w those of aecf_supcon_sym_pass1 on the matching labels.
 *   pass1: the logits GEMM with a dense set epilogue, one instance per weighting.  It writes E once as bf16 (workspace) and leaves
 *          the row and column sums of E exactly as the InfoNCE form does; then every tile runs a sweep over its accumulators that
 *          adds, per row and per column, the float32 sum of w and the float32 sum of w * raw score a_i . b_j (each product fused
 *          into its addition), the partner and the padding excluded: the partner joins later from its own float32 dot with weight
 *          1.  Fixed-order partials, no atomics.  col_stats [3][cols] float32 gets this rank's column statistics:
 *          c | sum of the label weights | sum of w * raw score.
 *   caller: all-reduce (sum) of col_stats over the ranks (nothing to do on one rank)
 *   loss:  loss_rows [rows] from the summed col_stats, with W = 1 + weight sum and X = (dot + sum) / Tc in both directions;
 *          prepares 1/l, 1/Wr (rows) and 1/c, 1/Wc (columns) in the workspace.
 *   grads: the weights in place over E (w formed again from the words), then da and this rank's share of db as in
 *          aecf_supcon_sym_grads: float32 or bf16 (grad_dtype), multiplied by upstream[0] (a DEVICE float32 scalar, NULL = 1);
 *          d_temperature (may be NULL) is WRITTEN with this rank's share of dL/dT times upstream[0].  It consumes the stored
 *          block: it runs once per pass1.
 * Served: the shapes of aecf_supcon_sym_*: bf16 rows, d % 64 == 0, 64 <= d <= 4096, min_temperature >= 0.025, cols <= 2^24.
 * Workspace: the layout and size of aecf_supcon_sym_workspace_bytes, the weight sums in the count slots:
 *   E [Rp][Cp] bf16 | row partials [3][Cp/256][Rp] | column partials [3][Rp/256][Cp] | row statistics [3][Rp] | 1/l [Rp] |
 *   1/Wr [Rp] | 1/c [Cp] | 1/Wc [Cp] | the partner's exponential [Rp] | da slabs [splits][rows][d], each piece rounded up to 256
 *   bytes, + 256 bytes.  The query answers 0 where the shape is not served.
 * Caller-owned buffers, a stream argument, no allocation, no synchronisation, nothing read on the host (the calls capture into a
 * graph), nothing read from the workspace before it is written; no float atomics, fixed-order partial sums: the same inputs give
 * the same bits.  Checks before any launch, in the order of aecf_supcon_sym_*: sizes (AECF_ERR_BAD_DIMS), then d,
 * min_temperature < 0.025, cols > 2^24, an unknown weighting, or a grad_dtype other than bf16 / float32 (AECF_ERR_UNSUPPORTED),
 * then NULL pointers (AECF_ERR_NULL_POINTER; upstream and d_temperature may be NULL), then the workspace size
 * (AECF_ERR_WORKSPACE). */
size_t aecf_supcon_ml_sym_workspace_bytes(int64_t rows, int64_t cols, int32_t d);      /* 0: not served */
int aecf_supcon_ml_sym_pass1(int64_t rows, int64_t cols, int64_t row_offset, int32_t d, const float* temperature,
                             float min_temperature, const void* a, const void* b, const uint64_t* row_sets,
                             const uint64_t* col_sets, int32_t weighting, void* workspace, size_t workspace_bytes,
                             float* col_stats /* [3][cols] */, void* stream);
int aecf_supcon_ml_sym_loss(int64_t rows, int64_t cols, int64_t row_offset, int32_t d, const float* temperature,
                            float min_temperature, const void* a, const void* b, const float* col_stats /* summed over ranks */,
                            void* workspace, size_t workspace_bytes, float* loss_rows, void* stream);
int aecf_supcon_ml_sym_grads(int64_t rows, int64_t cols, int64_t row_offset, int32_t d, const float* temperature,
                             float min_temperature, float coef, const void* a, const void* b, const uint64_t* row_sets,
                             const uint64_t* col_sets, int32_t weighting, void* workspace, size_t workspace_bytes,
                             const float* upstream, int32_t grad_dtype, void* da, void* db, float* d_temperature, void* stream);

/* ---- pooled multi-label contrastive loss, tile-GEMM form: aecf_supcon_pool_sym_* with a SET of classes per row ----
 * The supervised contrastive loss of Khosla et al. over ONE pool of the 2 cols rows of both views, with class sets where
 * aecf_supcon_pool_sym_* has one label: every row is an anchor, its keys are the other 2 cols - 1 rows (itself left out by INDEX),
 * and a key of either view counts with the weight of aecf_supcon_ml_sym_*.  Buffers as in the pooled form (a_loc, b_loc [rows,d],
 * a_all, b_all [cols,d], unit-norm bf16 rows; a_all / b_all may alias a_loc / b_loc on one rank).  row_sets [rows] and col_sets
 * [cols] are DEVICE arrays of one 64-bit word per row, SHARED by the views, bit c = class c (aecf_label_sets_pack makes them; all
 * 64 bits count, the sign bit is class 63); the empty set marks an unlabeled row: its only positive is its partner and it is
 * nobody's positive by label.
 *   w(A, B) = [A & B != 0]                          weighting AECF_SETS_OVERLAP
 *           = popcount(A & B) / popcount(A | B)     weighting AECF_SETS_JACCARD: ONE correctly rounded float32 division, 0 for an
 *                                                   empty union
 * Tc = max(*temperature, min_temperature), E(s) = exp((s - 1) / Tc).  Three logits blocks, per row i of the rank, g = row_offset + i:
 *   X = a_loc . b_all^T   the partner (column g) excluded from the sweep, weight 1 by index          lX, wX, sX   and columns cX, wcX, scX
 *   Y = a_loc . a_all^T   the anchor itself (column g) excluded by INDEX: no key, weight 0, whatever its set and value   lY, wY, sY
 *   Z = b_loc . b_all^T   the same                                                                                       lZ, wZ, sZ
 * (l: sum of E, w: float32 sum of the weights, s: float32 sum of weight * raw score, each product fused into its addition.)
 * Anchor a_i: Da = lX + lY, ka = wX + wY, sa = sX + sY, local.  Anchor b_g: Db_g = sum over ranks of cX_g + lZ_g, kb_g = sum wcX_g
 * + wZ_g, sb_g = sum scX_g + sZ_g (Z of the rank that owns row g).  With dot_i = a_i . b_g, na = 1 + ka, nb = 1 + kb:
 *   loss_rows[i] = [log Da_i + 1/Tc - (dot_i + sa_i) / na_i / Tc] + [log Db_g + 1/Tc - (dot_i + sb_g) / nb_g / Tc]      WITHOUT coef
 *   W_X = ct (E_X (1/Da_i + 1/Db_j) - w_ij (1/na_i + 1/nb_j)), the partner with w = 1 by index and its float32 exponential
 *   W_Y = ct (E_Y / Da_i - w_ij / na_i)       W_Z = ct (E_Z / Db_g - w_ij / nb_g)       both exactly 0 at the excluded key
 *         ct = coef / Tc * upstream
 *   d_a_loc = W_X b_all + W_Y a_all [rows,d]     d_b_loc = W_Z b_all [rows,d]
 *   d_a_all = W_Y^T a_loc [cols,d]               d_b_all = W_X^T a_loc + W_Z^T b_loc [cols,d]        (this rank's shares)
 *   dT = -(1/Tc) [ sum_i a_i . d_a_loc_i + sum_i b_i . d_b_loc_i ]   (0 where *temperature < min_temperature)
 * The shares of the ranks sum to the global gradients.  With all sets empty or pairwise disjoint every output has the bits of
 * aecf_ntxent_sym_pass1 / _loss / _grads on the same inputs (col_stats[0] those of col_sums); outside the rank's own range
 * col_stats has the bits of aecf_supcon_ml_sym_pass1.
 *   pass1: the three logits GEMMs.  X is aecf_supcon_ml_sym_pass1 to the bit; Y and Z run a row-only form of its dense epilogue
 *          (the E loop of the NT-Xent blocks, then the row half of the set sweep in the same summation order, the anchor's own
 *          element with weight 0 by index, no column statistics).  Then the combined row statistics (workspace) and col_stats
 *          [3][cols] float32 = this rank's column statistics of X (c | sum of w | sum of w * raw score), plus Z's row statistics
 *          on its own range [row_offset, row_offset + rows): one float32 addition per quantity and side, fixed order, no atomics.
 *   caller: all-reduce (sum) of col_stats over the ranks (nothing to do on one rank): it then holds Db | kb | sb.
 *   loss:  loss_rows [rows]; prepares 1/Da, 1/na (rows) and 1/Db, 1/nb (columns) in the workspace.
 *   grads: the three weights passes in place over the blocks (w formed again from the words), then the six products as in
 *          aecf_supcon_pool_sym_grads: two products on one output are summed in float32 and rounded ONCE to grad_dtype;
 *          everything is multiplied by upstream[0] (a DEVICE float32 scalar, NULL = 1); d_temperature (may be NULL) is WRITTEN
 *          with this rank's share of dL/dT times upstream[0].  It consumes the stored blocks: it runs once per pass1.
 * Served: the shapes of aecf_supcon_pool_sym_*: bf16 rows, d % 64 == 0, 64 <= d <= 4096, min_temperature >= 0.025, rows <= cols,
 * cols <= 2^23: an anchor's overlap weight sum adds two blocks' (each at most cols - 1) and stays an exact float32 integer up to
 * there; Jaccard keeps the same bound.  18 rows cols d MFMA flops.
 * Workspace: the layout and size of aecf_supcon_pool_sym_workspace_bytes, the weight sums in the count slots.  The query answers 0
 * where the shape is not served (d, rows > cols, cols > 2^23).
 * Caller-owned buffers, a stream argument, no allocation, no synchronisation, nothing read on the host (the calls capture into a
 * graph), nothing read from the workspace before it is written; no float atomics: the same inputs give the same bits.  Checks
 * before any launch, in the order of the two families this one joins: sizes (rows, cols, d > 0, cols < 2^31, min_temperature > 0,
 * 0 <= row_offset, row_offset + rows <= cols: AECF_ERR_BAD_DIMS), then d, min_temperature < 0.025, cols > 2^23, an unknown
 * weighting or a grad_dtype other than bf16 / float32 (AECF_ERR_UNSUPPORTED), then NULL pointers (AECF_ERR_NULL_POINTER; upstream
 * and d_temperature may be NULL), then the workspace size (AECF_ERR_WORKSPACE). */
size_t aecf_supcon_ml_pool_sym_workspace_bytes(int64_t rows, int64_t cols, int32_t d);      /* 0: not served */
int aecf_supcon_ml_pool_sym_pass1(int64_t rows, int64_t cols, int64_t row_offset, int32_t d, const float* temperature,
                                  float min_temperature, const void* a_loc, const void* b_loc, const void* a_all, const void* b_all,
                                  const int64_t* row_sets, const int64_t* col_sets, int32_t weighting, void* workspace,
                                  size_t workspace_bytes, float* col_stats /* [3][cols] */, void* stream);
int aecf_supcon_ml_pool_sym_loss(int64_t rows, int64_t cols, int64_t row_offset, int32_t d, const float* temperature,
                                 float min_temperature, const void* a_loc, const void* b_all,
                                 const float* col_stats /* summed over ranks */, void* workspace, size_t workspace_bytes,
                                 float* loss_rows, void* stream);
int aecf_supcon_ml_pool_sym_grads(int64_t rows, int64_t cols, int64_t row_offset, int32_t d, const float* temperature,
                                  float min_temperature, float coef, const void* a_loc, const void* b_loc, const void* a_all,
                                  const void* b_all, const int64_t* row_sets, const int64_t* col_sets, int32_t weighting,
                                  void* workspace, size_t workspace_bytes, const float* upstream, int32_t grad_dtype, void* d_a_loc,
                                  void* d_b_loc, void* d_a_all, void* d_b_all, float* d_temperature, void* stream);

/* ---- multi-view InfoNCE, tile-GEMM form (build-defined; the symmetric InfoNCE of aecf_nce_sym_*_dt over several pairs of views) ----
 * x holds `views` views side by side: x_loc [rows][views][d] are a rank's local rows (global rows row_offset .. row_offset + rows),
 * x_all [cols][views][d] the gathered ones, unit-norm bf16 rows read IN PLACE with a row pitch of views * d * 2 bytes; x_all may
 * alias x_loc on one rank.  The pairs, in this order (p = 0 .. P - 1):
 *   anchor = -1      every (m, n) with m < n, lexicographic: (0,1) (0,2) .. (1,2) ..            P = views (views - 1) / 2
 *   anchor = k >= 0  (min(k, n), max(k, n)) for every n != k, n rising                         P = views - 1
 * In pair (m, n) view m supplies the local rows (the a role) and view n the keys (the b role); the positive of local row i is
 * key row_offset + i.  Every pair is the symmetric InfoNCE of aecf_nce_sym_*_dt on x_loc[:, m] and x_all[:, n], all pairs at ONE
 * Tc = max(*temperature, min_temperature) and with the SAME coef (the caller folds 1 / P into it):
 *   pass1: ONE logits launch over the P blocks (the block index selects pair and tile), one sums launch: E_p in the workspace,
 *          col_sums [P][cols] float32 = this rank's column sums of every pair.
 *   caller: all-reduce (sum) of col_sums over the ranks (nothing to do on one rank).
 *   loss:  loss_rows [P][rows], WITHOUT coef; prepares the normalisers of every pair, one launch.
 *   grads: the weights of all pairs in place (one launch), then
 *            dx_loc[:, m] = sum over the pairs (m, n) of W_(m,n) x_all[:, n]          [rows][views][d]   the a-role products of view m
 *            dx_all[:, n] = sum over the pairs (m, n) of W_(m,n)^T x_loc[:, m]        [cols][views][d]   the b-role products of view n
 *          (dx_all: this rank's share; the shares of the ranks sum to the global gradient).  Each is ONE GEMM launch for all views
 *          whose K loop runs through every partner block of the view: an element is one float32 sum over all partners, rounded
 *          ONCE to grad_dtype (float32 or bf16) -- no per-pair stage, no add pass.  A view with no pair in a role is written as
 *          zeros: every element of both outputs is written on every call.  Everything is multiplied by upstream[0] (a DEVICE
 *          float32 scalar, NULL = 1); d_temperature (may be NULL) is WRITTEN with dL/dT = -(1/Tc) sum_m sum_i x_loc[i, m] .
 *          dx_loc[i, m] from the float32 accumulators, views in rising order, fixed order (0 where *temperature <
 *          min_temperature).  It consumes the stored blocks: it runs once per pass1.
 * For every pair, col_sums[p] and loss_rows[p] have the bits of aecf_nce_sym_pass1_dt / aecf_nce_sym_loss_dt on contiguous copies
 * of the two views; with views = 2 every output (dx_loc[:, 0] = da, dx_all[:, 1] = db, dT included) has the bits of
 * aecf_nce_sym_*_dt at the same coef.
 * Served: bf16 rows, d % 64 == 0, 64 <= d <= 4096, min_temperature >= 0.025, 2 <= views <= 8, -1 <= anchor < views, rows <= cols,
 * cols < 2^31.  Workspace, in order, each piece rounded up to 256 bytes, Rp / Cp = rows / cols rounded up to 256, + 256 bytes:
 *   E [P][Rp][Cp] bf16 (each block in the tiles of the InfoNCE form) | row partials [P][Cp/256][Rp] | column partials
 *   [P][Rp/256][Cp] | row sums [P][Rp] | 1/l [P][Rp] | 1/c [P][Cp] | the positive's exponential [P][Rp] |
 *   da slabs [splits][rows][views][d]        (float32 but E; splits: the K split of da = W b, as in the InfoNCE form)
 * The query answers 0 where the shape is not served.  Caller-owned buffers, a stream argument, no allocation, no synchronisation,
 * nothing read on the host, no float atomics: the same inputs give the same bits.  Checks before any launch: sizes (rows, cols,
 * d > 0, cols < 2^31, rows <= cols, min_temperature > 0, 0 <= row_offset, row_offset + rows <= cols, 2 <= views <= 8, -1 <= anchor
 * < views: AECF_ERR_BAD_DIMS), then d, min_temperature < 0.025 or a grad_dtype other than bf16 / float32 (AECF_ERR_UNSUPPORTED),
 * then NULL pointers (AECF_ERR_NULL_POINTER; upstream and d_temperature may be NULL), then the workspace size
 * (AECF_ERR_WORKSPACE). */
size_t aecf_nce_multi_workspace_bytes(int64_t rows, int64_t cols, int32_t d, int32_t views, int32_t anchor);      /* 0: not served */
int aecf_nce_multi_pass1(int64_t rows, int64_t cols, int32_t d, int32_t views, int32_t anchor, const float* temperature,
                         float min_temperature, const void* x_loc, const void* x_all, void* workspace, size_t workspace_bytes,
                         float* col_sums /* [P][cols] */, void* stream);
int aecf_nce_multi_loss(int64_t rows, int64_t cols, int64_t row_offset, int32_t d, int32_t views, int32_t anchor,
                        const float* temperature, float min_temperature, const void* x_loc, const void* x_all,
                        const float* col_sums /* summed over ranks */, void* workspace, size_t workspace_bytes,
                        float* loss_rows /* [P][rows] */, void* stream);
int aecf_nce_multi_grads(int64_t rows, int64_t cols, int64_t row_offset, int32_t d, int32_t views, int32_t anchor,
                         const float* temperature, float min_temperature, float coef, const void* x_loc, const void* x_all,
                         void* workspace, size_t workspace_bytes, const float* upstream, int32_t grad_dtype,
                         void* dx_loc /* [rows][views][d] */, void* dx_all /* [cols][views][d], this rank's share */,
                         float* d_temperature, void* stream);

/* ---- multi-view InfoNCE with missing views (build-defined; aecf_nce_multi_* where a row may lack views) ----
 * pres_loc [rows] (indexed by the LOCAL row) and pres_all [cols] (indexed by the GLOBAL row / column) hold one byte per row, bit v
 * set = view v of that row is present (aecf_l2norm_masked_forward packs them; pres_all[row_offset + i] == pres_loc[i]).  For pair
 * p = (m, n) of the pair list above, V_p = the global rows that hold both views, n_p = |V_p| over all ranks.  Pair p is the symmetric
 * InfoNCE of aecf_nce_multi_* restricted to V_p on both sides -- only rows of V_p are anchors, only rows of V_p are keys, down
 * the columns too -- and the total is the mean over the P' pairs with n_p > 0:
 *   L = sum_p pair_coef[p] sum_i loss_rows[p][i],   pair_coef[p] = 0.5 / n_p / P'  (0 where n_p = 0; L = 0 where P' = 0).
 * Exclusion is by the bytes and by index, with selects, never by value: x_loc / x_all must hold FINITE rows at absent slots (the
 * masked normalisation writes zeros there), and then no output depends on what the caller's unnormalised input held.
 *   pair_coef: ONE small launch over pres_all: integer counts of every n_p, pair_coef [P] float32 = 0.5 / n_p / P' formed in
 *          float64 and rounded once (with every view present: the float32 the unmasked form is handed as coef).
 *   pass1: aecf_nce_multi_pass1 with E = 0 -- in the stored block, its row sums and its column sums -- wherever the row or the
 *          column is outside V_p.  A 256 x 256 tile whose rows and columns are all in V_p runs the unmasked tile's code.
 *   loss:  a local row outside V_p: loss_rows[p][i] = 0, normaliser 0 (no log of an empty sum, no 1 / 0); a column outside V_p:
 *          normaliser 0.  loss_rows are WITHOUT pair_coef.
 *   grads: the weights with pair_coef[p] per pair and the partner term for the rows of V_p alone; then the gradient products, the
 *          dT sum and the slab sum of aecf_nce_multi_grads UNCHANGED: an excluded weight is a zero.  The gradient at an absent
 *          (row, view) is an exact zero; an empty pair contributes zeros.
 * With every view present col_sums, loss_rows, dx_loc, dx_all and d_temperature have the bits of aecf_nce_multi_* at
 * coef = 0.5 / cols / P.  Served shapes, workspace (the query returns aecf_nce_multi_workspace_bytes' value and layout), checks and
 * their order: as aecf_nce_multi_*; pres_loc, pres_all and pair_coef may not be NULL (AECF_ERR_NULL_POINTER).  pair_coef checks
 * cols, views and anchor (AECF_ERR_BAD_DIMS), then NULL pointers.  Nothing is read on the host; no float atomics. */
size_t aecf_nce_multi_masked_workspace_bytes(int64_t rows, int64_t cols, int32_t d, int32_t views, int32_t anchor);   /* 0: not served */
int aecf_nce_multi_masked_pair_coef(int64_t cols, int32_t views, int32_t anchor, const uint8_t* pres_all,
                                    float* pair_coef /* [P] */, void* stream);
int aecf_nce_multi_masked_pass1(int64_t rows, int64_t cols, int32_t d, int32_t views, int32_t anchor, const float* temperature,
                                float min_temperature, const void* x_loc, const void* x_all, const uint8_t* pres_loc,
                                const uint8_t* pres_all, void* workspace, size_t workspace_bytes, float* col_sums /* [P][cols] */,
                                void* stream);
int aecf_nce_multi_masked_loss(int64_t rows, int64_t cols, int64_t row_offset, int32_t d, int32_t views, int32_t anchor,
                               const float* temperature, float min_temperature, const void* x_loc, const void* x_all,
                               const uint8_t* pres_loc, const uint8_t* pres_all, const float* col_sums /* summed over ranks */,
                               void* workspace, size_t workspace_bytes, float* loss_rows /* [P][rows] */, void* stream);
int aecf_nce_multi_masked_grads(int64_t rows, int64_t cols, int64_t row_offset, int32_t d, int32_t views, int32_t anchor,
                                const float* temperature, float min_temperature, const float* pair_coef, const void* x_loc,
                                const void* x_all, const uint8_t* pres_loc, void* workspace, size_t workspace_bytes,
                                const float* upstream, int32_t grad_dtype, void* dx_loc, void* dx_all, float* d_temperature,
                                void* stream);

/* ---- multi-view InfoNCE, per pair (build-defined; aecf_nce_multi_* / aecf_nce_multi_masked_* with a temperature and a weight for
 * every pair) ----
 * One family serves both forms: pres_loc / pres_all as in aecf_nce_multi_masked_*, or BOTH NULL = every row holds every view
 * (n_p = cols).  temperatures [P] float32 on the device, in the order of the pair list above; pair p runs at
 * Tc_p = max(temperatures[p], min_temperature), read on the device.  With weights w_p >= 0 (pair_weights [P] float32 on the device,
 * NULL = all 1) and W = the sum of w_p over the pairs with n_p > 0,
 *   L = sum_p pair_coef[p] sum_i loss_rows[p][i],   pair_coef[p] = 0.5 / n_p * w_p / W   (0 where n_p = 0, w_p = 0 or W = 0).
 *   pair_coef: ONE small launch: the integer counts of aecf_nce_multi_masked_pair_coef, then 0.5 / n_p / (W / w_p) in float64,
 *          rounded once -- equal weights give aecf_nce_multi_masked_pair_coef's bits, and without missing views the float32 that
 *          aecf_nce_multi_grads is handed as coef = 0.5 / cols / P.  Zeros come from selects: no 0 / 0 is formed.
 *   pass1: the logits launch of aecf_nce_multi_pass1 / _masked_pass1 with scale and shift of every block from its pair's Tc_p.
 *          with_dt != 0 (needed where grads is to write d_temperatures): the instance that, after E is stored, sweeps the float32
 *          accumulators once more and leaves, per pair, this rank's row sums RS_i = sum_j E_ij (s_ij - 1) and column sums
 *          CS_j = sum_i E_ij (s_ij - 1) in the workspace (E the float32 exponential, never the stored bf16; excluded rows and
 *          columns by the same selects on the presence bytes).
 *   loss:  the finalize launch at Tc_p; also keeps s_ii - 1 of every row of V_p for the dT sums.  loss_rows WITHOUT pair_coef.
 *   grads: the weights W_p = pair_coef[p] upstream / Tc_p (...) per pair, then the gradient products and the slab sum of
 *          aecf_nce_multi_grads unchanged (da in its plain form: dT does not come from it).  d_temperatures [P] (may be NULL) is
 *          WRITTEN, this rank's share, by one launch of P blocks in a fixed order:
 *            dL/dT_p = -(pair_coef[p] upstream / Tc_p^2) [ sum_i RS_i / l_i + sum_j CS_j / c_j - 2 sum_i (s_ii - 1) ]
 *          with l the row sums and c the ALL-REDUCED column sums of E (so the shares of the ranks sum to the global gradient with
 *          no further exchange); 0 where temperatures[p] < min_temperature, and an exact 0 where pair_coef[p] = 0.
 * Where every temperatures[p] holds the bits of one T, col_sums and loss_rows have the bits of aecf_nce_multi_* /
 * aecf_nce_multi_masked_* at T, and with equal weights dx_loc and dx_all too; the sum of d_temperatures agrees with their
 * d_temperature to rounding (it is formed by another route).  Served shapes, checks and their order: as aecf_nce_multi_*;
 * pres_loc and pres_all must be both NULL or both given (pass1, loss: AECF_ERR_NULL_POINTER), pair_coef may not be NULL; pres_all and
 * pair_weights of pair_coef may be NULL.  Workspace: aecf_nce_multi_workspace_bytes' layout without its trailing 256 bytes, then
 *   row partials of E (s - 1) [P][Cp/256][Rp] | column partials [P][Rp/256][Cp] | RS [P][Rp] | CS [P][cols] | s_ii - 1 [P][Rp]
 * (float32, each rounded up to 256 bytes) + 256 bytes.  Nothing is read on the host; no float atomics. */
size_t aecf_nce_multi_pp_workspace_bytes(int64_t rows, int64_t cols, int32_t d, int32_t views, int32_t anchor);       /* 0: not served */
int aecf_nce_multi_pp_pair_coef(int64_t cols, int32_t views, int32_t anchor, const uint8_t* pres_all /* may be NULL */,
                                const float* pair_weights /* [P], may be NULL */, float* pair_coef /* [P] */, void* stream);
int aecf_nce_multi_pp_pass1(int64_t rows, int64_t cols, int32_t d, int32_t views, int32_t anchor, const float* temperatures /* [P] */,
                            float min_temperature, const void* x_loc, const void* x_all, const uint8_t* pres_loc,
                            const uint8_t* pres_all, int32_t with_dt, void* workspace, size_t workspace_bytes,
                            float* col_sums /* [P][cols] */, void* stream);
int aecf_nce_multi_pp_loss(int64_t rows, int64_t cols, int64_t row_offset, int32_t d, int32_t views, int32_t anchor,
                           const float* temperatures, float min_temperature, const void* x_loc, const void* x_all,
                           const uint8_t* pres_loc, const uint8_t* pres_all, const float* col_sums /* summed over ranks */,
                           void* workspace, size_t workspace_bytes, float* loss_rows /* [P][rows] */, void* stream);
int aecf_nce_multi_pp_grads(int64_t rows, int64_t cols, int64_t row_offset, int32_t d, int32_t views, int32_t anchor,
                            const float* temperatures, float min_temperature, const float* pair_coef, const void* x_loc,
                            const void* x_all, const uint8_t* pres_loc, void* workspace, size_t workspace_bytes,
                            const float* upstream, int32_t grad_dtype, void* dx_loc, void* dx_all,
                            float* d_temperatures /* [P], may be NULL */, void* stream);

/* ---- retrieval ranks of the contrastive views (build-defined like the contrastive terms they evaluate: the reference has no
 * contrastive term and no retrieval evaluation, so there are no reference lines to cite) ----
 * Local rows a [rows,d] (global indices row_offset .. row_offset + rows) against all gathered rows b [cols,d] of the other view,
 * bf16, d % 64 == 0, 64 <= d <= 4096, any row and column counts with row_offset + rows <= cols.  The rows are taken as given
 * (unit norm or not).  With s_ij = a_i . b_j accumulated in float32, the positive of row i is column row_offset + i:
 *   positive:  pos_row[i]     = s_(i, row_offset + i)                                                  float32 [rows]
 *   ranks:     row_greater[i] = #{ j < cols, j != row_offset + i : s_ij >  pos_row[i] }                int32 [rows]
 *              row_equal[i]   = #{ j < cols, j != row_offset + i : s_ij == pos_row[i] }
 *              col_greater[j] = #{ i < rows, i != j - row_offset : s_ij >  pos_col[j] }                int32 [cols]
 *              col_equal[j]   = #{ i < rows, i != j - row_offset : s_ij == pos_col[j] }
 * pos_col [cols] holds every column's threshold (the positives of all ranks, gathered by the caller); col_* are THIS rank's
 * share over its rows, for every column: the caller sums the ranks' shares.  pos_col == NULL switches the column direction
 * off (col_greater / col_equal are then not touched and may be NULL).  The rank of a positive is greater + f * equal with the
 * caller's tie rule f.  A comparison with a NaN is false on both sides: a NaN logit or threshold is counted nowhere.
 * One logits pass (2 rows cols d MFMA flops) whose epilogue compares and counts; nothing of size rows x cols is stored.
 * Workspace: (rows + cols) * tiles int32 partials, O((rows + cols) cols / 256) in all; aecf_retrieval_workspace_bytes answers 0
 * where the shape is not served.  Outputs are WRITTEN, not accumulated; integer sums: the same inputs give the same counts.
 * Caller-owned buffers, a stream argument, no allocation, no synchronisation, nothing read on the host.  Checks before any
 * launch: sizes and row_offset + rows <= cols (AECF_ERR_BAD_DIMS), then the width (AECF_ERR_UNSUPPORTED), then NULL pointers
 * (AECF_ERR_NULL_POINTER), then the workspace size (AECF_ERR_WORKSPACE). */
size_t aecf_retrieval_workspace_bytes(int64_t rows, int64_t cols, int32_t d);      /* 0: shape not served */
int aecf_retrieval_positive(int64_t rows, int64_t cols, int64_t row_offset, int32_t d, const void* a, const void* b,
                            float* pos_row, void* stream);
int aecf_retrieval_ranks(int64_t rows, int64_t cols, int64_t row_offset, int32_t d, const void* a, const void* b,
                         const float* pos_row, const float* pos_col /* [cols] or NULL */, int32_t* row_greater,
                         int32_t* row_equal, int32_t* col_greater, int32_t* col_equal, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ---- top-k retrieval: the best k keys of every query (build-defined like the retrieval ranks above: the reference has no
 * contrastive term and no retrieval evaluation, so there are no reference lines to cite) ----
 * Rows a [rows,d] against rows b [cols,d], bf16, d % 64 == 0, 64 <= d <= 4096, 1 <= k <= 16, cols < 2^31, any row and column
 * counts; the rows are taken as given (unit norm or not) and need not pair with each other.  With s_ij = a_i . b_j accumulated
 * in float32, row i of the outputs holds the k first columns of row i of s in this total order:
 *   1. the higher score first;  2. among equal scores (-0 == +0) the lower column index first;
 *   3. every NaN score is equal to every other NaN score and comes after -inf.
 *   values  [rows,k] float32   the scores, in that order         indices [rows,k] int32   their columns, 0 <= index < cols
 * The order is total, so the result does not depend on tile, block or rank arrangement.  exclude_partner != 0 removes the one
 * element (i, row_offset + i) from row i (the row's own partner among the gathered keys) and needs
 * 0 <= row_offset, row_offset + rows <= cols; with exclude_partner == 0 row_offset is ignored.  k may not exceed the columns
 * that remain (cols, or cols - 1 with exclude_partner), so no padding ever surfaces.  For the other direction swap a and b.
 * One logits pass (2 rows cols d MFMA flops) whose epilogue selects, per 256 x 256 tile and row, the tile's best k candidates
 * -- nothing of size rows x cols is stored -- and one small kernel that merges a row's lists.
 * Workspace: 8 KP Rp ceil(cols / 256) bytes (KP: k rounded up to a power of two, Rp: rows rounded up to 256), at most 4096 more
 * for alignment; aecf_retrieval_topk_workspace_bytes answers 0 where the shape or k is not served.  Outputs are WRITTEN; the
 * same inputs give the same bits.  Caller-owned buffers, a stream argument, no allocation, no synchronisation, nothing read on
 * the host.  Checks before any launch and before any pointer is read: sizes -- rows, cols, k <= 0, k beyond the columns left,
 * with exclude_partner row_offset < 0 or row_offset + rows > cols -- (AECF_ERR_BAD_DIMS), then d or k > 16
 * (AECF_ERR_UNSUPPORTED), then NULL pointers (AECF_ERR_NULL_POINTER), then the workspace size (AECF_ERR_WORKSPACE). */
size_t aecf_retrieval_topk_workspace_bytes(int64_t rows, int64_t cols, int32_t d, int32_t k);      /* 0: not served */
int aecf_retrieval_topk(int64_t rows, int64_t cols, int64_t row_offset, int32_t d, int32_t k, int32_t exclude_partner,
                        const void* a, const void* b, float* values, int32_t* indices, void* workspace,
                        size_t workspace_bytes, void* stream);

/* ---- multi-label evaluation: tie-exact average precision, AUROC and F1 counts (what the reference's example computes on the
 * host with sklearn, xrays/train_xrays_example.py:260-295 calculate_metrics, plus AUROC; the compare-and-count form is
 * build-defined) ----
 * logits [n_all,classes] row-major, AECF_F32 / AECF_BF16 / AECF_F16; labels [n_all,classes] uint8, positive iff non-zero.  For a
 * class c the VALID entries are the non-NaN logits.  For every valid positive i, over the valid entries j of its class:
 *   ge_all_i = #{ s_j >= s_i }   gt_all_i = #{ s_j > s_i }   ge_pos_i, gt_pos_i: the same over the valid positives only
 * from which, with npos / nneg / nvalid the class's numbers of valid positives, valid negatives and valid entries,
 *   AP_c    = (1 / npos) sum_i ge_pos_i / ge_all_i            (every sample at one score shares that threshold's precision)
 *   AUROC_c = sum_i (lt_neg_i + eq_neg_i / 2) / (npos nneg),  lt_neg_i = (nvalid - ge_all_i) - (npos - ge_pos_i),
 *                                                             eq_neg_i = (ge_all_i - gt_all_i) - (ge_pos_i - gt_pos_i)
 * Nothing is sorted; the counts are integers, the same for any tile, block or rank arrangement.
 *   prepare:   reads all n_all rows; fills the workspace and class_counts int32 [3][classes] = npos | nvalid | ninvalid.
 *              Every rank runs it on the gathered rows.
 *   counts:    for this rank's rows row_offset .. row_offset + rows, counts int32 [4][classes][rows] =
 *              ge_all | gt_all | ge_pos | gt_pos at (class, row - row_offset); 0 where the entry is not a valid positive.
 *              WRITTEN, not accumulated.  rows == 0 is valid and launches nothing (counts may then be NULL).
 *   finalize:  shares float64 [5][classes] over this rank's rows = sum ge_pos / ge_all | sum (lt_neg + eq_neg / 2) | TP | FP | FN,
 *              the last three with "predicted positive" = logit > logit_threshold among the valid entries.  Quotients and
 *              sums in float64 in a fixed order (lane t of 256 takes rows t, t + 256, ..; then a fixed tree); the second and
 *              the last three are sums of integers and half-integers, exact.  The caller adds the ranks' shares and divides.
 * NaN rule: a NaN logit is an invalid entry of its class: never a key, never an anchor, in none of npos, nneg, TP, FP, FN, and
 * counted in ninvalid.  It is excluded by selects (a NaN's order image lies below -inf's; a non-positive's divisor is 1), never
 * by a division by zero.  +-inf, +-0 and denormals are ordinary values and -0 ties +0: values are compared through an integer
 * image of their order, which does not depend on the float mode.
 * Workspace, in this order, every part rounded up to 256 bytes, with Np = n_all rounded up to 64 and nch = Np / 64:
 *   keys float32 [classes][Np] (class-major, an exact conversion) | positive keys float32 [classes][Np] and their rows int32
 *   [classes][Np] (the valid positives of a class in row order, npos of them) | uint64 [classes][nch] ballots of the valid
 *   positives | int32 [classes][nch] list offsets of the chunks | int32 [classes][nch] valid entries of the chunks
 * i.e. 3 * 4 classes Np + 16 classes nch bytes before the rounding.  counts and finalize read the workspace prepare filled.
 * Served: 1 <= classes <= 4096, 1 <= n_all <= 2^24, n_all * classes <= 2^28; outside them aecf_mlmetrics_workspace_bytes
 * answers 0 and the calls AECF_ERR_UNSUPPORTED.  Cost: npos (n_all + npos) compare-and-count pairs per class, a few vector
 * operations each.  Caller-owned buffers, a stream argument, no allocation, no synchronisation, nothing read on the host, no
 * atomics.  Checks before any launch: sizes -- n_all, classes <= 0, rows < 0, row_offset < 0, row_offset + rows > n_all, a NaN
 * threshold -- (AECF_ERR_BAD_DIMS), then the limits and the dtype (AECF_ERR_UNSUPPORTED), then NULL pointers
 * (AECF_ERR_NULL_POINTER), then the workspace size (AECF_ERR_WORKSPACE). */
size_t aecf_mlmetrics_workspace_bytes(int64_t n_all, int32_t classes);      /* 0: shape not served */
int aecf_mlmetrics_prepare(int64_t n_all, int32_t classes, int32_t dtype, const void* logits, const uint8_t* labels,
                           int32_t* class_counts, void* workspace, size_t workspace_bytes, void* stream);
int aecf_mlmetrics_counts(int64_t n_all, int32_t classes, int64_t row_offset, int64_t rows, const int32_t* class_counts,
                          int32_t* counts, const void* workspace, size_t workspace_bytes, void* stream);
int aecf_mlmetrics_finalize(int64_t n_all, int32_t classes, int64_t row_offset, int64_t rows, float logit_threshold,
                            const int32_t* class_counts, const int32_t* counts, double* shares, const void* workspace,
                            size_t workspace_bytes, void* stream);

/* ---- multi-label bootstrap: R resamples of the ROWS walked along one order per class, for confidence intervals of average
 * precision, AUROC and F1 (the reference's example compares point estimates only, xrays/train_xrays_example.py:260-295; the
 * resampling, the order by counting and the walk are build-defined) ----
 * A resample of rows is a vector of integer multiplicities w_j (a row carries all its classes, so macro scores see the joint
 * resample).  The descending order of a class's scores does not depend on it, and weighted AP, AUROC and the confusion counts
 * are running sums along that order.  Inputs as "multi-label evaluation": logits [n_all,classes], labels uint8, a NaN logit is
 * an invalid entry of its class and gets no slot.
 *   order:  runs the evaluation's prepare (workspace and class_counts int32 [3][classes] = npos | nvalid | ninvalid as there), then
 *           writes order int32 [classes][Np] (Np: n_all rounded up to 64): for a valid row r of class c, with img the integer
 *           order image of the evaluation, slot = #{k : img_k > img_r} + #{k < r : img_k == img_r} -- the STABLE DESCENDING
 *           order, a bijection of the valid rows onto [0, nvalid) -- and order[c][slot] = r | head << 31 | pos << 30 | pred << 29:
 *           head = no equal key before r (the first of its tie group), pos = the label, pred = logit > thresholds[c]
 *           (thresholds: float32 [classes] on the device, logit thresholds; a NaN threshold predicts every valid entry
 *           positive).  Slots nvalid .. Np - 1 are not written.  Every slot is written exactly once; no atomics.
 *   draw:   weights uint8 [n_all][Rp] (Rp: replicates rounded up to 64; row-major by data row, replicates contiguous) for the
 *           replicates replicate0 .. replicate0 + replicates - 1; columns past `replicates` are 0.  counts == NULL: global
 *           replicate 0 is all ones (the point estimate); replicate r >= 1 is the multinomial bootstrap, n_all draws: draw t
 *           takes philox4x32_10 (Salmon et al. 2011; 10 rounds, multipliers 0xD2511F53 / 0xCD9E8D57, key increments
 *           0x9E3779B9 / 0xBB67AE85) with key (seed lo, seed hi) and counter (t >> 1 lo, t >> 1 hi, r, 0x626f6f74); its 64-bit
 *           value is c[2 (t & 1) + 1] << 32 | c[2 (t & 1)], its row the high 64 bits of value * n_all; weights[j][r - replicate0]
 *           is the number of draws that hit j.  A replicate depends on (seed, r, n_all) only.  The hits are counted with int32
 *           integer atomics in the workspace (zeroed by the call); integer adds commute, so the bits are the same on every run.
 *           counts != NULL: int32 [n_all][Rp] multiplicities of the caller (nothing is drawn, no replicate is forced to ones, the
 *           workspace is not used and may be NULL).  Either way a count outside 0 .. 255 is clipped to that range and the number
 *           of clipped entries is ADDED to *n_saturated (int32 on the device; the caller zeroes it).
 *   walk:   stats int64 [replicates][7][classes] = Wpos | Wvalid | U2 | TP | FP | FN | S, the last as the bits of a float64.
 *           Along the order of class c, with w the replicate's weights, per tie group g (gall = sum w, gpos = sum w pos over
 *           the group; cum_pos, cum_all: the same sums over the groups before it):
 *             S  += gpos > 0 ? (double)gpos * ((double)(cum_pos + gpos) / (double)(cum_all + gall)) : 0     in slot order
 *             U2 += (gall - gpos) * (2 cum_pos + gpos)                                          (uint64, <= 2 Wpos Wneg <= 2^63)
 *           and TP / FP / FN the weighted counts of pos and pred.  From them AP = S / Wpos (sklearn's step-wise average
 *           precision with sample_weight), AUROC = U2 / (2 Wpos (Wvalid - Wpos)) (half credit for ties), F1 = 2 TP / (2 TP + FP
 *           + FN).  Everything but S is an integer; S is one float64 quotient, product and sum per group that holds a positive
 *           weight, in slot order, by one lane: the statistics of a replicate depend on nothing but the inputs and its weights.
 *           One wave per (64 replicates, class); the wave takes n_all steps.
 * Workspace: order's is the evaluation's (aecf_mlboot_workspace_bytes = aecf_mlmetrics_workspace_bytes); draw's is int32
 * [n_all][Rp], rounded up to 256 bytes (aecf_mlboot_draw_workspace_bytes).  Served: the evaluation's limits, 1 <= replicates <=
 * 4096 per call, replicate0 + replicates <= 2^31; outside them the size queries answer 0 and the calls AECF_ERR_UNSUPPORTED.
 * Buffers are 16-byte aligned, caller-owned; a stream argument, no allocation, no synchronisation, nothing read on the host.
 * Checks before any launch and before any pointer is read: sizes -- n_all, classes, replicates <= 0, replicate0 < 0 or beyond
 * 2^31 - replicates -- (AECF_ERR_BAD_DIMS), then the limits and the dtype (AECF_ERR_UNSUPPORTED), then NULL pointers
 * (AECF_ERR_NULL_POINTER), then the workspace size (AECF_ERR_WORKSPACE). */
size_t aecf_mlboot_workspace_bytes(int64_t n_all, int32_t classes);                 /* 0: shape not served */
size_t aecf_mlboot_draw_workspace_bytes(int64_t n_all, int32_t replicates);         /* 0: not served */
int aecf_mlboot_order(int64_t n_all, int32_t classes, int32_t dtype, const void* logits, const uint8_t* labels,
                      const float* thresholds, int32_t* class_counts, int32_t* order, void* workspace, size_t workspace_bytes,
                      void* stream);
int aecf_mlboot_draw(int64_t n_all, int32_t replicates, int64_t replicate0, uint64_t seed, const int32_t* counts, uint8_t* weights,
                     int32_t* n_saturated, void* workspace, size_t workspace_bytes, void* stream);
int aecf_mlboot_walk(int64_t n_all, int32_t classes, int32_t replicates, const int32_t* class_counts, const int32_t* order,
                     const uint8_t* weights, int64_t* stats, void* stream);

/* ---- multi-label classification loss: binary cross-entropy, focal and asymmetric loss as one elementwise formula (replaces the
 * reference example's torch criterion, xrays/train_xrays_example.py:327 nn.BCEWithLogitsLoss(), applied at :366 and :374; the
 * weights, the focusing exponents, the margin, the smoothing and the unknown labels are build-defined) ----
 * logits [n,classes] row-major, AECF_F32 / AECF_BF16 / AECF_F16, read as stored; labels [n,classes] of label_dtype: an aecf_dtype
 * value, AECF_MLLOSS_U8 (torch bool / uint8) or AECF_MLLOSS_I8.  With s = sigmoid(x), t' = t (1 - eps) + eps / 2,
 * q = max(s - margin, 0), a = pos_scale[c] and b = neg_scale[c] (float32 [classes], NULL: 1):
 *   l     = - a t' (1 - s)^gamma_pos log s  -  b (1 - t') q^gamma_neg log(1 - q)
 *   dl/dx = - a t' (1 - s)^gamma_pos [ (1 - s) - gamma_pos s log s ]
 *           - b (1 - t') s (1 - s) [ gamma_neg q^(gamma_neg - 1) log(1 - q) - q^gamma_neg / (1 - q) ]
 * with p^0 = 1 for every p.  Where s - margin <= 0 in float32 the second term and its gradient are exact zeros.  Float32
 * arithmetic: e = exp(-|x|), l1p = log1p(e), r = 1 / (1 + e); s and 1 - s are r and e r (by the sign of x), -log s and
 * -log(1 - s) are max(-+x, 0) + l1p, powers are exp(gamma log(.)) with the exponent-0 case exactly 1, and with a margin 1 - q is
 * (1 - s) + margin.  A term whose coefficient a t' or b (1 - t') is 0 is an exact 0 whatever the logit holds.
 * UNKNOWN targets: floating point: NaN or < 0; AECF_MLLOSS_I8: < 0 (other non-zero -> 1); AECF_MLLOSS_U8: none (non-zero -> 1).
 * An unknown element adds nothing, is not counted, and its gradient is an exact zero by select: its logit reaches no output.
 * On a valid element a +-inf logit gives the limit of the formula, a NaN logit a NaN loss and a NaN gradient there only.
 *   forward:  two launches.  stats float64 [2][classes] = loss sums | valid counts per class; totals, 24 bytes: float64 sum of
 *             the loss, float64 N (valid elements), float32 reduced loss (AECF_MLLOSS_MEAN: sum / N, 0 where N == 0;
 *             AECF_MLLOSS_SUM: sum), one zero float32.  Per-thread float32 sums over the rows a thread owns, float64 above them in
 *             a fixed order, no atomics: the same bits on every run.
 *   backward: one launch, recomputes the element from (logits, labels) and stores dlogits [n,classes] of dtype =
 *             dl/dx * scale, rounded once; scale = grad_out[0] (float32 on the device, NULL: 1) * factor, divided by totals' N for
 *             AECF_MLLOSS_MEAN (0 where N == 0).  Reads only N of totals, so a caller that sums stats over ranks hands over the
 *             global N.
 * Workspace (forward), with nrb0 = min(max(ceil(n classes / 16384), 1), min(1024, max(1, 2^20 / classes))),
 * rows_pb = ceil(n / nrb0) and nrb = ceil(n / rows_pb): float64 [nrb][classes] | int32 [nrb][classes], each rounded up to 256
 * bytes.  16-byte loads and stores where classes is a multiple of the 16-byte vector of the logits and the pointers are 16-byte
 * aligned, else element accesses.  Served: 1 <= classes <= 4096, n classes <= 2^30; outside them aecf_mlloss_workspace_bytes
 * answers 0 and the calls AECF_ERR_UNSUPPORTED.  Caller-owned buffers, a stream argument, no allocation, no synchronisation,
 * nothing read on the host.  Checks before any pointer is read: n, classes <= 0, a gamma that is negative or not finite, margin or
 * label_smoothing outside [0, 1), a reduction outside the two, a factor that is not finite (AECF_ERR_BAD_DIMS), then the limits
 * and the two dtype codes (AECF_ERR_UNSUPPORTED), then NULL pointers (AECF_ERR_NULL_POINTER), then the workspace size
 * (AECF_ERR_WORKSPACE). */
#define AECF_MLLOSS_U8 3
#define AECF_MLLOSS_I8 4
#define AECF_MLLOSS_MEAN 0
#define AECF_MLLOSS_SUM 1
size_t aecf_mlloss_workspace_bytes(int64_t n, int32_t classes);             /* 0: shape not served */
int aecf_mlloss_forward(int64_t n, int32_t classes, int32_t dtype, int32_t label_dtype, const void* logits, const void* labels,
                        const float* pos_scale, const float* neg_scale, float gamma_pos, float gamma_neg, float margin,
                        float label_smoothing, int32_t reduction, double* stats, double* totals, void* workspace,
                        size_t workspace_bytes, void* stream);
int aecf_mlloss_backward(int64_t n, int32_t classes, int32_t dtype, int32_t label_dtype, const void* logits, const void* labels,
                         const float* pos_scale, const float* neg_scale, float gamma_pos, float gamma_neg, float margin,
                         float label_smoothing, int32_t reduction, const double* totals, const float* grad_out, float factor,
                         void* dlogits, void* stream);

/* ---- fused classifier head: the multi-label classification loss above of logits = h W^T + bias and its three gradients,
 * without the logits (replaces classifier[3] of the reference example's model, xrays/train_xrays_example.py nn.Linear, together
 * with the criterion; the streaming form is build-defined) ----
 * h [n,k] and w [classes,k] (nn.Linear's layout) row-major AECF_BF16; bias float32 [classes] or NULL; labels [n,classes] of
 * label_dtype with the label kinds and the UNKNOWN rule of aecf_mlloss_*; pos_scale / neg_scale float32 [classes] or NULL; the
 * form parameters of aecf_mlloss_forward.  With z_ic = h_i . w_c + bias_c, l and g = dl/dz the element of aecf_mlloss_* at z:
 *   loss = sum_ic l_ic (/ N)      dh_i = scale sum_c g_ic w_c      dW_c = scale sum_i g_ic h_i      dbias_c = scale sum_i g_ic
 * Nothing of size n x classes is allocated, written or read besides the labels.  Both passes are one streaming loop: 64
 * stationary rows per block in registers, the other matrix through LDS in tiles of 32 rows, S = streamed . stationary on bf16
 * MFMAs with float32 accumulation, the element, then Out^T += streamed^T g on MFMAs again.
 * Rounding points: z = S + bias_c is ONE rounded float32 add after the MFMA chain (bias NULL: no add) and is never rounded to
 * bf16; the element is aecf_mlloss's float32 arithmetic; g enters both gradient products rounded ONCE to bf16 (unscaled), the
 * products accumulate in float32; dbias sums the UNROUNDED float32 g; the scale meets the float32 sums and each output is
 * rounded once.  An unknown target, whatever its logit, adds nothing, is not counted and has g = 0 by select.  Non-finite
 * features are the caller's problem as in any GEMM: a NaN row of h reaches dW even when all its targets are unknown, because
 * the product forms 0 x NaN.
 *   forward:  the CLS role (stationary = 64 classes, streamed = rows of h, the rows split over
 *             KSc = splits(classes, n) blocks per class block), a combine of the splits in split order and a one-block sum
 *             over the classes.  stats float64 [2][classes] = loss sums | valid counts and totals (24 bytes) as
 *             aecf_mlloss_forward leaves them.  A lane adds the losses of the rows it meets in float32; the four lanes of a
 *             class, the splits and the classes are added in float64 in a fixed order; no atomics: the same bits on every
 *             run.  want_grads = 1: also dw_unscaled float32 [classes][k] = sum_i g_ic h_i and db_unscaled float32 [classes] =
 *             sum_i g_ic (before any scale).  want_grads = 0: the loss-only pass, without the second product: the same float
 *             operations in the same order for the loss; dw_unscaled / db_unscaled are not touched and may be NULL.
 *   backward: scale = grad_out[0] (float32 on the device, NULL: 1) * factor, divided by totals' N for AECF_MLLOSS_MEAN (0 where
 *             N == 0); reads only N of totals, so a caller that sums stats over ranks hands over the global N.  dh [n][k] of
 *             dh_dtype (AECF_BF16 or AECF_F32) by the ROW role (stationary = 64 rows of h, streamed = rows of w, the classes
 *             split over KSr = splits(n, classes) blocks per row block; one split stores from its epilogue, more are combined
 *             in split order); dw float32 [classes][k] = scale dw_unscaled and db float32 [classes] = scale db_unscaled by one
 *             small launch.  Any of dh, dw, db may be NULL; with dh NULL no ROW launch happens and h, w, labels and the
 *             workspace are not read.
 * splits(s, m): ks = min(ceil(256 / ceil(s / 64)), ceil(m / 512), 64), at least 1; per = ceil(m / ks) rounded up to 32; the
 * count is ceil(m / per).  Widths 768 and 1024 take their output columns from two launches per role (the scores recomputed).
 * Workspace, every part rounded up to 256 bytes: float32 [max(KSc classes, KSr n where KSr > 1)][k] partial rows | float64
 * [KSc][classes] loss sums | int32 [KSc][classes] valid counts | float32 [KSc][classes] g sums.  One size serves both calls; the
 * forward's contents are not needed by the backward.
 * Served: AECF_BF16 h and w, k in {128, 256, 384, 512, 768, 1024}, 1 <= classes <= 65536, 1 <= n < 2^31; every index into the
 * label matrix is formed in 64-bit arithmetic.  Outside them aecf_mlhead_workspace_bytes answers 0 and the calls
 * AECF_ERR_UNSUPPORTED.  Caller-owned buffers, a stream argument, no allocation, no synchronisation, nothing read on the host.
 * Checks before any pointer is read: n, classes, k <= 0, want_grads outside {0, 1}, a gamma that is negative or not finite,
 * margin or label_smoothing outside [0, 1), a reduction outside the two, a factor that is not finite (AECF_ERR_BAD_DIMS), then
 * the limits and the dtype codes (AECF_ERR_UNSUPPORTED), then NULL pointers (AECF_ERR_NULL_POINTER), then the workspace size
 * (AECF_ERR_WORKSPACE; the backward needs it only with dh). */
size_t aecf_mlhead_workspace_bytes(int64_t n, int32_t classes, int32_t k);  /* 0: shape not served */
int aecf_mlhead_forward(int64_t n, int32_t classes, int32_t k, int32_t dtype, int32_t label_dtype, const void* h, const void* w,
                        const float* bias, const void* labels, const float* pos_scale, const float* neg_scale, float gamma_pos,
                        float gamma_neg, float margin, float label_smoothing, int32_t reduction, int32_t want_grads, double* stats,
                        double* totals, float* dw_unscaled, float* db_unscaled, void* workspace, size_t workspace_bytes,
                        void* stream);
int aecf_mlhead_backward(int64_t n, int32_t classes, int32_t k, int32_t dtype, int32_t label_dtype, const void* h, const void* w,
                         const float* bias, const void* labels, const float* pos_scale, const float* neg_scale, float gamma_pos,
                         float gamma_neg, float margin, float label_smoothing, int32_t reduction, const double* totals,
                         const float* grad_out, float factor, const float* dw_unscaled, const float* db_unscaled, int32_t dh_dtype,
                         void* dh, float* dw, float* db, void* workspace, size_t workspace_bytes, void* stream);

/* ---- multi-label calibration: reliability bins (ECE / MCE), Brier score and NLL of logits [n,classes] under a per-class scale
 * and bias, and the fit of that scaling by minimising the NLL (temperature scaling after Guo et al. 2017; Platt scaling per
 * class).  The reference names calibration as the property its fusion layer keeps and measures none of it; the statistics, the
 * bins in logit space and the optimiser are build-defined ----
 * logits [n,classes] row-major, AECF_F32 / AECF_BF16 / AECF_F16, read as stored; labels [n,classes] of label_dtype with the label
 * kinds and the UNKNOWN rule of aecf_mlloss_* (floating point: NaN or < 0; AECF_MLLOSS_I8: < 0; AECF_MLLOSS_U8: none).  A known
 * target is positive iff non-zero.  An element is VALID iff its target is known and its logit is not NaN.  A NaN logit on a known
 * target is counted in n_invalid[c] and reaches nothing else; an unknown target's logit reaches no output.  Exclusions are
 * selects, never products with 0.
 * Calibrated logit: z = x scale[c] + bias[c] in float32 (float32 [classes] on the device, either may be NULL: scale 1, bias 0),
 * the product and the sum rounded one after the other, never an fma; with both NULL z = x and nothing is multiplied.  +-inf
 * gives the limits (p = 1 / 0, NLL 0 or inf).  (A z that is NaN though x is not -- inf 0, inf - inf -- makes its class's sums NaN.)
 * Bin: edges is a HOST array of bins - 1 ascending float32 values e_1 .. e_{bins-1} (1 <= bins <= AECF_MLCAL_MAX_BINS; it is
 * copied into the launch arguments and may be NULL for bins == 1); the bin of an element is #{ j : z > e_j }, so an element on
 * an edge belongs to the lower bin.  Equal-width probability bins are e_j = float32(log(j / (bins - j))).
 * Per element, float32, aecf_mlloss's forms: e = exp(-|z|), l1p = log1p(e), r = 1 / (1 + e); p = sigmoid(z) and 1 - p are r and
 * e r by the sign of z, -log p and -log(1 - p) are max(-+z, 0) + l1p.  Brier term: (1 - p)^2 for a positive, p^2 for a negative;
 * NLL term: -log p or -log(1 - p).
 *   stats:    two launches.  stats float64 [3 bins + 5][classes], rows in this order: bin_count [bins] | bin_pos [bins] | bin_conf
 *             [bins] (the sum of p over a bin's elements) | brier_sum | nll_sum | n_invalid | n_valid | n_pos.  Counts are exact
 *             float64 integers, so one all-reduce of the block joins the ranks.
 *   fit_sums: two launches.  Over the valid elements with a FINITE logit (a +-inf logit stays +-inf under every positive scale
 *             and is left out), with s = sigmoid(z), y the target, w = s (1 - s) and x the stored logit as float32, sums float64
 *             [9][classes] = L = sum nll | g1 = sum (s - y) x | g0 = sum (s - y) | h11 = sum w x^2 | h01 = sum w x | h00 = sum w |
 *             n_used | n_used positives | n_skipped (the +-inf logits on known targets).  s - y is -(1 - p) or p, no subtraction.
 *   Sums: per-thread float32 over the rows a thread owns, float64 above that in a fixed order (the threads of a class in row
 *   order, the row blocks in order), no atomics: the same bits on every run; the integer rows are the same for any block, tile
 *   or rank arrangement.
 *   fit_update: one launch holding the optimiser, one lane per independent problem.  mode AECF_MLCAL_TEMPERATURE: ONE problem,
 *             the classes' sums added in class order in float64, one scale written to all classes, bias 0 (T = 1 / scale);
 *             AECF_MLCAL_CLASS_TEMPERATURE: a scale per class, bias 0; AECF_MLCAL_PLATT: a scale and a bias per class.
 *             sums are those of the parameters in scale_eval / bias_eval (float32 [classes], what fit_sums was given); the call
 *             overwrites them with the parameters to evaluate next and writes the last ACCEPTED parameters to scale_out /
 *             bias_out.  state is float64 [12][classes], ZEROED by the caller before the first call (the shared temperature
 *             uses column 0), rows: accepted scale | accepted bias | accepted L | lambda | accepted g1 | g0 | h11 | h01 | h00 |
 *             phase (0 fresh, 1 running, 2 converged, 3 not fitted) | the first L | accepted steps.
 * Optimiser rule: a Newton step damped in Levenberg-Marquardt fashion on the convex NLL.  First call: the evaluated parameters
 * (the caller hands over scale 1, bias 0) are accepted; a problem without a used element, without a positive or without a
 * negative among them is not fitted (phase 3: scale 1, bias 0 for good).  Later calls: a trial whose L does not exceed the
 * accepted L by more than 2^-14 of it -- two L of float32 elements cannot be told apart more finely, and without the slack the
 * last Newton steps, which lower L by less than that, would be refused -- is accepted and lambda divided by 10 (floor 1e-9);
 * the accepted L kept in the state is the smallest L of an accepted trial.  If the step was at most 2^-20 max(1, |theta|) in
 * every parameter the problem is converged and stops moving.  Any other trial (a NaN L too) is rejected: the accepted
 * parameters and their sums stay, lambda is multiplied by 10 (at most 1e12).  The next trial is accepted - (H + lambda diag H)^-1 g, lambda starting at 1e-3, with H =
 * [h11 h01; h01 h00] and g = (g1, g0) for AECF_MLCAL_PLATT and H = h11, g = g1 for the temperatures (no step where the damped
 * matrix is not positive), clamped to scale in [1/64, 64] and bias in [-16, 16] and ROUNDED to float32: the fit evaluates z with
 * the float32 values aecf_mlcal_stats later applies, and an unevaluated trial is never an output.
 * Workspace (stats and fit_sums), with nrb0 = min(max(ceil(n classes / 16384), 1), min(1024, max(1, 2^19 / classes))),
 * rows_pb = ceil(n / nrb0), nrb = ceil(n / rows_pb): float64 [nrb][max(3 bins + 5, 9)][classes], rounded up to 256 bytes; a
 * workspace sized for bins serves fit_sums too.  16-byte loads where classes is a multiple of the logits' 16-byte vector and the
 * pointers are 16-byte aligned (stats: 8-byte loads of 16-bit logits where bins > 8, element accesses where bins > 16 -- the
 * bins of a thread's classes live in LDS), else element accesses.  Served: 1 <= classes <=
 * 4096, n classes <= 2^30; outside them aecf_mlcal_workspace_bytes answers 0 and the calls AECF_ERR_UNSUPPORTED.  Caller-owned
 * buffers, a stream argument, no allocation, no synchronisation, nothing read from the device on the host.  Checks before any
 * launch: n, classes <= 0, bins outside 1 .. 32, a mode outside the three (AECF_ERR_BAD_DIMS), then the limits and the two dtype
 * codes (AECF_ERR_UNSUPPORTED), then NULL pointers (AECF_ERR_NULL_POINTER; the edges are then read: a NaN or a descent among
 * them is AECF_ERR_BAD_DIMS), then the workspace size (AECF_ERR_WORKSPACE). */
#define AECF_MLCAL_MAX_BINS 32
#define AECF_MLCAL_TEMPERATURE 0
#define AECF_MLCAL_CLASS_TEMPERATURE 1
#define AECF_MLCAL_PLATT 2
size_t aecf_mlcal_workspace_bytes(int64_t n, int32_t classes, int32_t bins);            /* 0: shape or bins not served */
int aecf_mlcal_stats(int64_t n, int32_t classes, int32_t dtype, int32_t label_dtype, const void* logits, const void* labels,
                     const float* scale, const float* bias, int32_t bins, const float* edges, double* stats, void* workspace,
                     size_t workspace_bytes, void* stream);
int aecf_mlcal_fit_sums(int64_t n, int32_t classes, int32_t dtype, int32_t label_dtype, const void* logits, const void* labels,
                        const float* scale, const float* bias, double* sums, void* workspace, size_t workspace_bytes,
                        void* stream);
int aecf_mlcal_fit_update(int32_t classes, int32_t mode, const double* sums, double* state, float* scale_eval, float* bias_eval,
                          float* scale_out, float* bias_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AECF_HIP_H */
