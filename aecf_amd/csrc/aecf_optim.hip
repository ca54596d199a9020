// AdamW over a LIST of float32 tensors in one launch (the optimiser step of the example trainer, ref
// xrays/train_xrays_example.py:322-323, 376: torch.optim.AdamW(lr=1e-4, weight_decay=0.01)).
// torch's fused multi-tensor kernel hands a block a chunk of 65536 elements, so the ~1 M parameters of the example model run on
// ~30 blocks (40 us, tools/debug/adamw_time.py); here a block takes 1024 elements (16-byte accesses),
// the tensor table travels in the kernel arguments, and the per-tensor step counters live on the device (a captured step
// replays with a fresh count): every block reads the counters at its start, the LAST block to finish increments them.
//   p *= 1 - lr wd;  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;
//   p -= (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps),   t = step + 1        (torch/optim/adamw.py, amsgrad off)
#include <math.h>

#include "../../include/aecf_hip.h"
#include "aecf_kernels.h"

namespace aecf {

namespace {

constexpr int OPT_MAX_TENSORS = 24;
constexpr int OPT_BLOCK_ELEMS = 1024;
constexpr unsigned int OPT_SUBTICKETS = 64;          // + 1 top ticket: AECF_ADAMW_TICKET_WORDS uint32 per launch group

struct AdamArgs {
    float* p[OPT_MAX_TENSORS];
    const float* g[OPT_MAX_TENSORS];
    float* m[OPT_MAX_TENSORS];
    float* v[OPT_MAX_TENSORS];
    float* step[OPT_MAX_TENSORS];
    int64_t numel[OPT_MAX_TENSORS];
    unsigned int first_block[OPT_MAX_TENSORS + 1];
    unsigned int* ticket;
    int n;
    float lr, beta1, beta2, eps, weight_decay;
    float log_beta1, log_beta2;                       // natural logs, rounded from double on the host
};

__global__ __launch_bounds__(256) void adamw_multi_kernel(AdamArgs a) {
    int t = 0;
    while (t + 1 < a.n && blockIdx.x >= a.first_block[t + 1]) ++t;          // (<= 24 entries: linear)
    // 1 - beta^t = -expm1(t ln beta) in float32 (no cancellation for small t; torch's capturable path raises beta to a float32
    // step tensor as well); block-uniform, every lane forms it
    const float step = a.step[t][0] + 1.0f;
    const float step_size = a.lr / -expm1f(step * a.log_beta1), bc2_sqrt = sqrtf(-expm1f(step * a.log_beta2));
    const float decay = 1.0f - a.lr * a.weight_decay;
    const int64_t base = (int64_t)(blockIdx.x - a.first_block[t]) * OPT_BLOCK_ELEMS + 4 * threadIdx.x;
    const int64_t n = a.numel[t];
    float* p = a.p[t];
    const float* g = a.g[t];
    float* m = a.m[t];
    float* v = a.v[t];
    auto update = [&](float& pp, float gg, float& mm, float& vv) {
        pp *= decay;
        mm = a.beta1 * mm + (1.0f - a.beta1) * gg;
        vv = a.beta2 * vv + (1.0f - a.beta2) * gg * gg;
        const float denom = sqrtf(vv) / bc2_sqrt + a.eps;
        pp -= step_size * (mm / denom);
    };
    const bool vec = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                       reinterpret_cast<uintptr_t>(v)) & 15) == 0;
    if (vec && base + 4 <= n) {
        f32x4 pv = *reinterpret_cast<f32x4*>(p + base), mv = *reinterpret_cast<f32x4*>(m + base);
        f32x4 vv = *reinterpret_cast<f32x4*>(v + base);
        const f32x4 gv = *reinterpret_cast<const f32x4*>(g + base);
        float pa[4] = {pv[0], pv[1], pv[2], pv[3]}, ma[4] = {mv[0], mv[1], mv[2], mv[3]}, va[4] = {vv[0], vv[1], vv[2], vv[3]};
#pragma unroll
        for (int i = 0; i < 4; ++i) update(pa[i], gv[i], ma[i], va[i]);
        *reinterpret_cast<f32x4*>(p + base) = f32x4{pa[0], pa[1], pa[2], pa[3]};
        *reinterpret_cast<f32x4*>(m + base) = f32x4{ma[0], ma[1], ma[2], ma[3]};
        *reinterpret_cast<f32x4*>(v + base) = f32x4{va[0], va[1], va[2], va[3]};
    } else {
        for (int64_t i = base; i < base + 4 && i < n; ++i) update(p[i], g[i], m[i], v[i]);
    }
    // the last block to finish advances every tensor's counter (all other blocks have read theirs) and re-arms the tickets.
    // Two levels -- 64 sub-tickets by blockIdx % 64, whoever completes one takes a top ticket -- so that the thousands of blocks
    // of a large model do not queue on one address
    __shared__ int is_last;
    __syncthreads();
    if (threadIdx.x == 0) {
        // no fence: every lane's read of its step counter has been consumed by now (the barrier above), and that is all the last
        // block's write has to wait for.  A __threadfence() here made every block write back its XCD's L2 (the XCDs' L2s are
        // not coherent with each other): 0.74 TB/s at any size, 630 us for 16 M parameters
        int last = 0;
        const unsigned int sub = blockIdx.x % OPT_SUBTICKETS;
        const unsigned int expect = (gridDim.x - sub + OPT_SUBTICKETS - 1) / OPT_SUBTICKETS;
        if (atomicAdd(a.ticket + 1 + sub, 1u) == expect - 1) {
            a.ticket[1 + sub] = 0u;
            const unsigned int nsub = gridDim.x < OPT_SUBTICKETS ? gridDim.x : OPT_SUBTICKETS;
            if (atomicAdd(a.ticket, 1u) == nsub - 1) {
                a.ticket[0] = 0u;
                last = 1;
            }
        }
        is_last = last;
    }
    __syncthreads();
    // (one lane per tensor)
    if (is_last && (int)threadIdx.x < a.n) a.step[threadIdx.x][0] += 1.0f;
}

}  // namespace

// tensors in groups of OPT_MAX_TENSORS; ticket: 65 zero-initialised unsigned per group
void launch_adamw_multi(int n, float* const* p, const float* const* g, float* const* m, float* const* v, float* const* step,
                        const int64_t* numel, unsigned int* ticket, float lr, float beta1, float beta2, float eps, float weight_decay,
                        hipStream_t s) {
    for (int g0 = 0, grp = 0; g0 < n; g0 += OPT_MAX_TENSORS, ++grp) {
        AdamArgs a;
        a.n = (n - g0) < OPT_MAX_TENSORS ? (n - g0) : OPT_MAX_TENSORS;
        unsigned int blocks = 0;
        for (int i = 0; i < a.n; ++i) {
            a.p[i] = p[g0 + i]; a.g[i] = g[g0 + i]; a.m[i] = m[g0 + i]; a.v[i] = v[g0 + i]; a.step[i] = step[g0 + i];
            a.numel[i] = numel[g0 + i];
            a.first_block[i] = blocks;
            blocks += (unsigned int)((numel[g0 + i] + OPT_BLOCK_ELEMS - 1) / OPT_BLOCK_ELEMS);
        }
        a.first_block[a.n] = blocks;
        a.ticket = ticket + (size_t)grp * (OPT_SUBTICKETS + 1);
        a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.weight_decay = weight_decay;
        a.log_beta1 = (float)log((double)beta1);
        a.log_beta2 = (float)log((double)beta2);
        if (blocks) adamw_multi_kernel<<<dim3(blocks), dim3(256), 0, s>>>(a);
    }
}

// ---- mixed precision: the same update over parameters and gradients of float32 / bf16 / f16, optional float32 masters ----
// (replaces torch.optim.AdamW of ref xrays/train_xrays_example.py:322-323 for a bf16 / f16 model, torch.amp.GradScaler's
// unscale + skip and the scaling pass of torch.nn.utils.clip_grad_norm_, all on the one elementwise pass)
// A lane takes 4 elements where parameter and gradient are both float32 (the layout of adamw_multi_kernel) and 8 where either
// is 16-bit: one 16-byte access per 16-bit tensor, two per float32 tensor.  With a master the float32 weight is read from and
// written to it and the 16-bit parameter is only WRITTEN, as the round-to-nearest-even of the new master (pack2 /
// Tr::from_f32, the conversions of aecf_cast_f32_to_bf16 / _f16: param == master.to(dtype) bit for bit); without one the
// parameter is widened, updated in float32 and rounded once on the store.  Moments are float32 always.
// Launch-wide device scalars, each optional: lr_dev (replaces the float lr; a captured step follows it), grad_scale (the AMP
// loss scale: g * (1 / scale), the reciprocal formed once per block by a correctly rounded division), grad_coef (the clip
// coefficient grad_sumsq_finalize_kernel wrote) and two found_inf flags (GradScaler's and the norm's; either non-zero: every
// block returns before it reads or writes anything else, the tickets stay armed and no counter advances).
namespace {

struct AdamMpArgs {
    void* p[OPT_MAX_TENSORS];
    const void* g[OPT_MAX_TENSORS];
    float* master[OPT_MAX_TENSORS];                   // NULL: none
    float* m[OPT_MAX_TENSORS];
    float* v[OPT_MAX_TENSORS];
    float* step[OPT_MAX_TENSORS];
    int64_t numel[OPT_MAX_TENSORS];
    unsigned int first_block[OPT_MAX_TENSORS + 1];
    unsigned char pdt[OPT_MAX_TENSORS], gdt[OPT_MAX_TENSORS];          // aecf_dtype
    unsigned int* ticket;
    const float *lr_dev, *grad_scale, *grad_coef, *found_inf, *found_inf2;
    int n;
    float lr, beta1, beta2, eps, weight_decay;
    float log_beta1, log_beta2;
};

template <typename T> __device__ __forceinline__ float opt_load1(const void* q, int64_t i) {
    if constexpr (std::is_same<T, F32>::value) return reinterpret_cast<const float*>(q)[i];
    else if constexpr (std::is_same<T, F16>::value) return f16_bits_to_f32(reinterpret_cast<const unsigned short*>(q)[i]);
    else return bf16_bits_to_f32(reinterpret_cast<const unsigned short*>(q)[i]);
}
template <typename T> __device__ __forceinline__ void opt_store1(void* q, int64_t i, float f) {
    if constexpr (std::is_same<T, F32>::value) reinterpret_cast<float*>(q)[i] = f;
    else reinterpret_cast<unsigned short*>(q)[i] = Tr<T>::from_f32(f);
}
// N consecutive elements from a 16-byte aligned address: N / 4 accesses of float32, one access of 8 16-bit elements
template <typename T, int N> __device__ __forceinline__ void opt_loadv(const void* q, int64_t i, float (&o)[N]) {
    if constexpr (std::is_same<T, F32>::value) {
#pragma unroll
        for (int k = 0; k < N; k += 4) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(q) + i + k);
            o[k] = x[0]; o[k + 1] = x[1]; o[k + 2] = x[2]; o[k + 3] = x[3];
        }
    } else {
        static_assert(N == 8, "a 16-bit tensor moves 8 elements per lane");
        const u32x4 w = *reinterpret_cast<const u32x4*>(reinterpret_cast<const unsigned short*>(q) + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if constexpr (std::is_same<T, F16>::value) {
                o[2 * k] = f16_bits_to_f32(w[k] & 0xffffu); o[2 * k + 1] = f16_bits_to_f32(w[k] >> 16);
            } else {
                o[2 * k] = bf16_bits_to_f32(w[k] & 0xffffu); o[2 * k + 1] = bf16_bits_to_f32(w[k] >> 16);
            }
        }
    }
}
template <typename T, int N> __device__ __forceinline__ void opt_storev(void* q, int64_t i, const float (&o)[N]) {
    if constexpr (std::is_same<T, F32>::value) {
#pragma unroll
        for (int k = 0; k < N; k += 4)
            *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(q) + i + k) = f32x4{o[k], o[k + 1], o[k + 2], o[k + 3]};
    } else {
        static_assert(N == 8, "a 16-bit tensor moves 8 elements per lane");
        *reinterpret_cast<u32x4*>(reinterpret_cast<unsigned short*>(q) + i) =
            u32x4{pack2<T>(o[0], o[1]), pack2<T>(o[2], o[3]), pack2<T>(o[4], o[5]), pack2<T>(o[6], o[7])};
    }
}

template <typename T> constexpr bool opt_is_f32 = std::is_same<T, F32>::value;
// elements per lane and per block of a (parameter, gradient) dtype pair; the host sizes the grid with the same numbers
template <typename PT, typename GT> constexpr int opt_lane_elems = (opt_is_f32<PT> && opt_is_f32<GT>) ? 4 : 8;
static int opt_block_elems(int pdt, int gdt) { return (pdt == AECF_F32 && gdt == AECF_F32) ? OPT_BLOCK_ELEMS : 2 * OPT_BLOCK_ELEMS; }

// the weight as STORED, in float32: the new master / float32 parameter itself, or the rounded 16-bit parameter widened again
template <typename PT> __device__ __forceinline__ float opt_stored(float f, bool has_master) {
    if constexpr (opt_is_f32<PT>) return f;
    else return has_master ? f : Tr<PT>::to_f32(Tr<PT>::from_f32(f));
}
// e' = e + om (w' - e), one rounding of the difference and one of the fused sum (the form tests/ema_cases.py tells from the others)
__device__ __forceinline__ float ema_next(float om, float w, float e) { return __fmaf_rn(om, __fsub_rn(w, e), e); }

// EMA (compile-time): after the update also e <- ema_next(om, w', e) on the float32 average `e` (NULL: this tensor has none)
// and, for a 16-bit parameter, eo <- round(e') (NULL: none).  EMA = false is adamw_mp_kernel's body, unchanged.
template <typename PT, typename GT, bool EMA>
__device__ __forceinline__ void adamw_mp_body(const AdamMpArgs& a, int t, float lr, float gmul, float* e, void* eo, float om) {
    constexpr int L = opt_lane_elems<PT, GT>;
    // (the expressions of adamw_multi_kernel, in its order)
    const float step = a.step[t][0] + 1.0f;
    const float step_size = lr / -expm1f(step * a.log_beta1), bc2_sqrt = sqrtf(-expm1f(step * a.log_beta2));
    const float decay = 1.0f - lr * a.weight_decay;
    const int64_t base = ((int64_t)(blockIdx.x - a.first_block[t]) * 256 + threadIdx.x) * L;
    const int64_t n = a.numel[t];
    void* p = a.p[t];
    const void* g = a.g[t];
    float* m = a.m[t];
    float* v = a.v[t];
    float* w = opt_is_f32<PT> ? nullptr : a.master[t];           // float32 weight of a 16-bit parameter, if kept
    auto update = [&](float& pp, float gg, float& mm, float& vv) {
        gg *= gmul;
        pp *= decay;
        mm = a.beta1 * mm + (1.0f - a.beta1) * gg;
        vv = a.beta2 * vv + (1.0f - a.beta2) * gg * gg;
        const float denom = sqrtf(vv) / bc2_sqrt + a.eps;
        pp -= step_size * (mm / denom);
    };
    if constexpr (opt_is_f32<PT>) eo = nullptr;                   // (the caller lets `ema` BE the output tensor)
    uintptr_t bits = reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                     reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(w);
    if constexpr (EMA) bits |= reinterpret_cast<uintptr_t>(e) | reinterpret_cast<uintptr_t>(eo);
    const bool vec = (bits & 15) == 0;
    if (vec && base + L <= n) {
        float pa[L], ga[L], ma[L], va[L];
        if (w) opt_loadv<F32, L>(w, base, pa);
        else opt_loadv<PT, L>(p, base, pa);
        opt_loadv<GT, L>(g, base, ga);
        opt_loadv<F32, L>(m, base, ma);
        opt_loadv<F32, L>(v, base, va);
#pragma unroll
        for (int i = 0; i < L; ++i) update(pa[i], ga[i], ma[i], va[i]);
        if (w) opt_storev<F32, L>(w, base, pa);
        opt_storev<PT, L>(p, base, pa);
        opt_storev<F32, L>(m, base, ma);
        opt_storev<F32, L>(v, base, va);
        if constexpr (EMA) {
            if (e) {
                float ea[L];
                opt_loadv<F32, L>(e, base, ea);
#pragma unroll
                for (int i = 0; i < L; ++i) ea[i] = ema_next(om, opt_stored<PT>(pa[i], w != nullptr), ea[i]);
                opt_storev<F32, L>(e, base, ea);
                if constexpr (!opt_is_f32<PT>) {
                    if (eo) opt_storev<PT, L>(eo, base, ea);
                }
            }
        }
    } else {
        for (int64_t i = base; i < base + L && i < n; ++i) {
            float pp = w ? w[i] : opt_load1<PT>(p, i), mm = m[i], vv = v[i];
            update(pp, opt_load1<GT>(g, i), mm, vv);
            if (w) w[i] = pp;
            opt_store1<PT>(p, i, pp);
            m[i] = mm;
            v[i] = vv;
            if constexpr (EMA) {
                if (e) {
                    const float en = ema_next(om, opt_stored<PT>(pp, w != nullptr), e[i]);
                    e[i] = en;
                    if constexpr (!opt_is_f32<PT>) {
                        if (eo) opt_store1<PT>(eo, i, en);
                    }
                }
            }
        }
    }
}

// the averages' part of a launch (adamw_mp_ema_kernel only): tables beside AdamMpArgs, one decay for the launch
struct EmaTail {
    float* ema[OPT_MAX_TENSORS];                      // float32 [numel]; NULL: the tensor has no average
    void* ema_out[OPT_MAX_TENSORS];                   // the parameter's dtype; NULL: none (ignored beside a float32 parameter)
    const float* decay_dev;                           // replaces `decay` when set, read at replay time
    float decay;
};
// AdamMpArgs is 1576 bytes of kernel arguments (7 x 192 of tables, 100 + 48 of first_block / dtypes, 4 of padding, 6 x 8 of
// pointers, 32 of scalars); EmaTail adds 2 x 192 + 8 + 4 (+ 4 of padding) = 400: 1976 of the 4096 a launch may carry
struct AdamMpEmaArgs {
    AdamMpArgs a;
    EmaTail x;
};
static_assert(sizeof(AdamMpArgs) == 1576 && sizeof(AdamMpEmaArgs) == 1976, "the byte counts of the comment above");

// 1 - beta of an EMA launch, block-uniform: beta clamped to [0, 1] by selects (a NaN passes both and comes out NaN: the
// caller then skips the averages, and only them)
__device__ __forceinline__ float ema_one_minus(const float* decay_dev, float decay) {
    float b = decay_dev ? decay_dev[0] : decay;
    b = b < 0.0f ? 0.0f : b;
    b = b > 1.0f ? 1.0f : b;
    return __fsub_rn(1.0f, b);
}

__global__ __launch_bounds__(256) void adamw_mp_kernel(AdamMpArgs a) {
    // block-uniform, read by every block and written by none of this launch
    if ((a.found_inf && a.found_inf[0] != 0.0f) || (a.found_inf2 && a.found_inf2[0] != 0.0f)) return;
    int t = 0;
    while (t + 1 < a.n && blockIdx.x >= a.first_block[t + 1]) ++t;
    const float lr = a.lr_dev ? a.lr_dev[0] : a.lr;
    float gmul = a.grad_scale ? __fdiv_rn(1.0f, a.grad_scale[0]) : 1.0f;
    if (a.grad_coef) gmul *= a.grad_coef[0];
    switch (a.pdt[t] * 3 + a.gdt[t]) {                // aecf_dtype: AECF_BF16 = 0, AECF_F32 = 1, AECF_F16 = 2
        case 0: adamw_mp_body<BF16, BF16, false>(a, t, lr, gmul, nullptr, nullptr, 0.0f); break;
        case 1: adamw_mp_body<BF16, F32, false>(a, t, lr, gmul, nullptr, nullptr, 0.0f); break;
        case 2: adamw_mp_body<BF16, F16, false>(a, t, lr, gmul, nullptr, nullptr, 0.0f); break;
        case 3: adamw_mp_body<F32, BF16, false>(a, t, lr, gmul, nullptr, nullptr, 0.0f); break;
        case 4: adamw_mp_body<F32, F32, false>(a, t, lr, gmul, nullptr, nullptr, 0.0f); break;
        case 5: adamw_mp_body<F32, F16, false>(a, t, lr, gmul, nullptr, nullptr, 0.0f); break;
        case 6: adamw_mp_body<F16, BF16, false>(a, t, lr, gmul, nullptr, nullptr, 0.0f); break;
        case 7: adamw_mp_body<F16, F32, false>(a, t, lr, gmul, nullptr, nullptr, 0.0f); break;
        default: adamw_mp_body<F16, F16, false>(a, t, lr, gmul, nullptr, nullptr, 0.0f); break;
    }
    // the two-level ticket of adamw_multi_kernel, and no fence for the reason given there
    __shared__ int is_last;
    __syncthreads();
    if (threadIdx.x == 0) {
        int last = 0;
        const unsigned int sub = blockIdx.x % OPT_SUBTICKETS;
        const unsigned int expect = (gridDim.x - sub + OPT_SUBTICKETS - 1) / OPT_SUBTICKETS;
        if (atomicAdd(a.ticket + 1 + sub, 1u) == expect - 1) {
            a.ticket[1 + sub] = 0u;
            const unsigned int nsub = gridDim.x < OPT_SUBTICKETS ? gridDim.x : OPT_SUBTICKETS;
            if (atomicAdd(a.ticket, 1u) == nsub - 1) {
                a.ticket[0] = 0u;
                last = 1;
            }
        }
        is_last = last;
    }
    __syncthreads();
    if (is_last && (int)threadIdx.x < a.n) a.step[threadIdx.x][0] += 1.0f;
}

// ---- AdamW + exponential moving average of the weights in the same pass (aecf_adamw_mp_ema_step) ----
// adamw_mp_kernel with its body's EMA flag set: the lane that holds the new float32 weight also reads and writes its average,
// two more 16-byte accesses per float32 vector (one more store for a 16-bit ema_out).  A set found_inf / found_inf2 returns
// before anything is written, the averages included.
__global__ __launch_bounds__(256) void adamw_mp_ema_kernel(AdamMpEmaArgs k) {
    const AdamMpArgs& a = k.a;
    // block-uniform, read by every block and written by none of this launch
    if ((a.found_inf && a.found_inf[0] != 0.0f) || (a.found_inf2 && a.found_inf2[0] != 0.0f)) return;
    int t = 0;
    while (t + 1 < a.n && blockIdx.x >= a.first_block[t + 1]) ++t;
    const float lr = a.lr_dev ? a.lr_dev[0] : a.lr;
    float gmul = a.grad_scale ? __fdiv_rn(1.0f, a.grad_scale[0]) : 1.0f;
    if (a.grad_coef) gmul *= a.grad_coef[0];
    float* e = nullptr;
    void* eo = nullptr;
    const float om = ema_one_minus(k.x.decay_dev, k.x.decay);
    if (om == om) {
        e = k.x.ema[t];
        eo = k.x.ema_out[t];
    }
    switch (a.pdt[t] * 3 + a.gdt[t]) {                // aecf_dtype: AECF_BF16 = 0, AECF_F32 = 1, AECF_F16 = 2
        case 0: adamw_mp_body<BF16, BF16, true>(a, t, lr, gmul, e, eo, om); break;
        case 1: adamw_mp_body<BF16, F32, true>(a, t, lr, gmul, e, eo, om); break;
        case 2: adamw_mp_body<BF16, F16, true>(a, t, lr, gmul, e, eo, om); break;
        case 3: adamw_mp_body<F32, BF16, true>(a, t, lr, gmul, e, eo, om); break;
        case 4: adamw_mp_body<F32, F32, true>(a, t, lr, gmul, e, eo, om); break;
        case 5: adamw_mp_body<F32, F16, true>(a, t, lr, gmul, e, eo, om); break;
        case 6: adamw_mp_body<F16, BF16, true>(a, t, lr, gmul, e, eo, om); break;
        case 7: adamw_mp_body<F16, F32, true>(a, t, lr, gmul, e, eo, om); break;
        default: adamw_mp_body<F16, F16, true>(a, t, lr, gmul, e, eo, om); break;
    }
    // (the ticket of adamw_mp_kernel)
    __shared__ int is_last;
    __syncthreads();
    if (threadIdx.x == 0) {
        int last = 0;
        const unsigned int sub = blockIdx.x % OPT_SUBTICKETS;
        const unsigned int expect = (gridDim.x - sub + OPT_SUBTICKETS - 1) / OPT_SUBTICKETS;
        if (atomicAdd(a.ticket + 1 + sub, 1u) == expect - 1) {
            a.ticket[1 + sub] = 0u;
            const unsigned int nsub = gridDim.x < OPT_SUBTICKETS ? gridDim.x : OPT_SUBTICKETS;
            if (atomicAdd(a.ticket, 1u) == nsub - 1) {
                a.ticket[0] = 0u;
                last = 1;
            }
        }
        is_last = last;
    }
    __syncthreads();
    if (is_last && (int)threadIdx.x < a.n) a.step[threadIdx.x][0] += 1.0f;
}

// ---- the same EMA without an optimiser step (aecf_ema_update): tensors that had no gradient, callers on another optimiser ----
// w' = float32(src); a lane takes 4 elements where source and output are float32 and 8 where either is 16-bit.  No tickets:
// nothing is counted.
struct EmaArgs {
    const void* src[OPT_MAX_TENSORS];
    float* ema[OPT_MAX_TENSORS];
    void* ema_out[OPT_MAX_TENSORS];                   // NULL: none
    int64_t numel[OPT_MAX_TENSORS];
    unsigned int first_block[OPT_MAX_TENSORS + 1];
    unsigned char sdt[OPT_MAX_TENSORS], odt[OPT_MAX_TENSORS];          // aecf_dtype; odt is AECF_F32 where there is no ema_out
    const float *decay_dev, *found_inf, *found_inf2;
    int n;
    float decay;
};

template <typename ST, typename OT>
__device__ __forceinline__ void ema_body(const EmaArgs& a, int t, float om) {
    constexpr int L = opt_lane_elems<ST, OT>;
    const int64_t base = ((int64_t)(blockIdx.x - a.first_block[t]) * 256 + threadIdx.x) * L;
    const int64_t n = a.numel[t];
    const void* src = a.src[t];
    float* e = a.ema[t];
    void* eo = opt_is_f32<OT> ? nullptr : a.ema_out[t];
    const bool vec = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(e) | reinterpret_cast<uintptr_t>(eo)) & 15) == 0;
    if (vec && base + L <= n) {
        float wa[L], ea[L];
        opt_loadv<ST, L>(src, base, wa);
        opt_loadv<F32, L>(e, base, ea);
#pragma unroll
        for (int i = 0; i < L; ++i) ea[i] = ema_next(om, wa[i], ea[i]);
        opt_storev<F32, L>(e, base, ea);
        if constexpr (!opt_is_f32<OT>) {
            if (eo) opt_storev<OT, L>(eo, base, ea);
        }
    } else {
        for (int64_t i = base; i < base + L && i < n; ++i) {
            const float en = ema_next(om, opt_load1<ST>(src, i), e[i]);
            e[i] = en;
            if constexpr (!opt_is_f32<OT>) {
                if (eo) opt_store1<OT>(eo, i, en);
            }
        }
    }
}

__global__ __launch_bounds__(256) void ema_update_kernel(EmaArgs a) {
    if ((a.found_inf && a.found_inf[0] != 0.0f) || (a.found_inf2 && a.found_inf2[0] != 0.0f)) return;
    const float om = ema_one_minus(a.decay_dev, a.decay);
    if (!(om == om)) return;
    int t = 0;
    while (t + 1 < a.n && blockIdx.x >= a.first_block[t + 1]) ++t;
    switch (a.sdt[t] * 3 + a.odt[t]) {
        case 0: ema_body<BF16, BF16>(a, t, om); break;
        case 1: ema_body<BF16, F32>(a, t, om); break;
        case 2: ema_body<BF16, F16>(a, t, om); break;
        case 3: ema_body<F32, BF16>(a, t, om); break;
        case 4: ema_body<F32, F32>(a, t, om); break;
        case 5: ema_body<F32, F16>(a, t, om); break;
        case 6: ema_body<F16, BF16>(a, t, om); break;
        case 7: ema_body<F16, F32>(a, t, om); break;
        default: ema_body<F16, F16>(a, t, om); break;
    }
}

// ---- global L2 norm of gradients of mixed dtype (torch.nn.utils.clip_grad_norm_'s norm; torch.amp.GradScaler's inf check) ----
// Launch 1: a block sums the squares of NORM_BLOCK_ELEMS consecutive elements of one tensor (16-byte accesses, a lane's
// elements in order, then a fixed butterfly over the wave and the four waves in order) and stores ONE float32 partial at its
// own index.  Launch 2: one block adds the partials (lane i takes i, i + 256, ... in order, the same fixed tree) and writes
// the norm, the clip coefficient and the non-finite flag.  No float atomics, no fence: the kernel boundary is the hand-off.
constexpr int NORM_BLOCK_ELEMS = 4096;

struct NormArgs {
    const void* g[OPT_MAX_TENSORS];
    int64_t numel[OPT_MAX_TENSORS];
    unsigned int first_block[OPT_MAX_TENSORS + 1];
    unsigned char gdt[OPT_MAX_TENSORS];
    float* partial;                                   // [first_block[n]]
    int n;
};

// sum over the 256 lanes of a block in a fixed order; valid in lane 0
__device__ __forceinline__ float block_sum_256(float x) {
    __shared__ float wave_sum[4];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = x;
    __syncthreads();
    return ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
}

template <typename T>
__device__ __forceinline__ float sumsq_body(const void* g, int64_t n, int64_t block0) {
    constexpr int L = opt_is_f32<T> ? 4 : 8;
    const bool aligned = (reinterpret_cast<uintptr_t>(g) & 15) == 0;
    float acc = 0.0f;
#pragma unroll
    for (int it = 0; it < NORM_BLOCK_ELEMS / (256 * L); ++it) {
        const int64_t i = block0 + ((int64_t)it * 256 + threadIdx.x) * L;
        if (aligned && i + L <= n) {
            float x[L];
            opt_loadv<T, L>(g, i, x);
#pragma unroll
            for (int k = 0; k < L; ++k) acc += x[k] * x[k];
        } else {
            for (int64_t k = i; k < i + L && k < n; ++k) {
                const float x = opt_load1<T>(g, k);
                acc += x * x;
            }
        }
    }
    return acc;
}

__global__ __launch_bounds__(256) void grad_sumsq_kernel(NormArgs a) {
    int t = 0;
    while (t + 1 < a.n && blockIdx.x >= a.first_block[t + 1]) ++t;
    const int64_t block0 = (int64_t)(blockIdx.x - a.first_block[t]) * NORM_BLOCK_ELEMS;
    float acc;
    if (a.gdt[t] == AECF_F32) acc = sumsq_body<F32>(a.g[t], a.numel[t], block0);
    else if (a.gdt[t] == AECF_F16) acc = sumsq_body<F16>(a.g[t], a.numel[t], block0);
    else acc = sumsq_body<BF16>(a.g[t], a.numel[t], block0);
    acc = block_sum_256(acc);
    if (threadIdx.x == 0) a.partial[blockIdx.x] = acc;
}

__global__ __launch_bounds__(256) void grad_sumsq_finalize_kernel(const float* __restrict__ partial, int64_t count, float max_norm,
                                                                  const float* __restrict__ grad_scale, float* __restrict__ out) {
    float acc = 0.0f;
    for (int64_t i = threadIdx.x; i < count; i += 256) acc += partial[i];
    acc = block_sum_256(acc);
    if (threadIdx.x == 0) {
        const float total = grad_scale ? sqrtf(acc) / grad_scale[0] : sqrtf(acc);
        out[0] = total;
        out[1] = max_norm > 0.0f ? fminf(1.0f, max_norm / (total + 1e-6f)) : 1.0f;
        out[2] = isfinite(acc) ? 0.0f : 1.0f;
    }
}

}  // namespace

// tensors with numel > 0 in groups of OPT_MAX_TENSORS; ticket as for launch_adamw_multi.  Returns the number of launches.
// with_ema: adamw_mp_ema_kernel with the averages' tables beside the same arguments (ema required then, ema_out may be NULL)
static int launch_adamw_mp_any(bool with_ema, int n, void* const* p, const void* const* g, float* const* master, float* const* m,
                               float* const* v, float* const* step, const int64_t* numel, const int32_t* pdt, const int32_t* gdt,
                               unsigned int* ticket, float lr, float beta1, float beta2, float eps, float weight_decay,
                               const float* lr_dev, const float* grad_scale, const float* grad_coef, const float* found_inf,
                               const float* found_inf2, float* const* ema, void* const* ema_out, float ema_decay,
                               const float* ema_decay_dev, hipStream_t s) {
    int launches = 0;
    AdamMpEmaArgs k;
    AdamMpArgs& a = k.a;
    a.n = 0;
    unsigned int blocks = 0;
    auto flush = [&]() {
        if (a.n == 0) return;
        a.first_block[a.n] = blocks;
        a.ticket = ticket + (size_t)launches * (OPT_SUBTICKETS + 1);
        a.lr_dev = lr_dev; a.grad_scale = grad_scale; a.grad_coef = grad_coef; a.found_inf = found_inf; a.found_inf2 = found_inf2;
        a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.weight_decay = weight_decay;
        a.log_beta1 = (float)log((double)beta1);
        a.log_beta2 = (float)log((double)beta2);
        if (with_ema) {
            k.x.decay = ema_decay; k.x.decay_dev = ema_decay_dev;
            adamw_mp_ema_kernel<<<dim3(blocks), dim3(256), 0, s>>>(k);
        } else {
            adamw_mp_kernel<<<dim3(blocks), dim3(256), 0, s>>>(a);
        }
        ++launches;
        a.n = 0;
        blocks = 0;
    };
    for (int i = 0; i < n; ++i) {
        if (numel[i] == 0) continue;
        const int j = a.n++;
        a.p[j] = p[i]; a.g[j] = g[i]; a.master[j] = master ? master[i] : nullptr; a.m[j] = m[i]; a.v[j] = v[i]; a.step[j] = step[i];
        a.numel[j] = numel[i];
        a.pdt[j] = (unsigned char)pdt[i]; a.gdt[j] = (unsigned char)gdt[i];
        a.first_block[j] = blocks;
        if (with_ema) {
            k.x.ema[j] = ema[i];
            k.x.ema_out[j] = ema_out ? ema_out[i] : nullptr;
        }
        const int be = opt_block_elems(pdt[i], gdt[i]);
        blocks += (unsigned int)((numel[i] + be - 1) / be);
        if (a.n == OPT_MAX_TENSORS) flush();
    }
    flush();
    return launches;
}

int launch_adamw_mp(int n, void* const* p, const void* const* g, float* const* master, float* const* m, float* const* v,
                    float* const* step, const int64_t* numel, const int32_t* pdt, const int32_t* gdt, unsigned int* ticket, float lr,
                    float beta1, float beta2, float eps, float weight_decay, const float* lr_dev, const float* grad_scale,
                    const float* grad_coef, const float* found_inf, const float* found_inf2, hipStream_t s) {
    return launch_adamw_mp_any(false, n, p, g, master, m, v, step, numel, pdt, gdt, ticket, lr, beta1, beta2, eps, weight_decay,
                               lr_dev, grad_scale, grad_coef, found_inf, found_inf2, nullptr, nullptr, 0.0f, nullptr, s);
}

int launch_adamw_mp_ema(int n, void* const* p, const void* const* g, float* const* master, float* const* m, float* const* v,
                        float* const* step, const int64_t* numel, const int32_t* pdt, const int32_t* gdt, unsigned int* ticket,
                        float lr, float beta1, float beta2, float eps, float weight_decay, const float* lr_dev,
                        const float* grad_scale, const float* grad_coef, const float* found_inf, const float* found_inf2,
                        float* const* ema, void* const* ema_out, float ema_decay, const float* ema_decay_dev, hipStream_t s) {
    return launch_adamw_mp_any(true, n, p, g, master, m, v, step, numel, pdt, gdt, ticket, lr, beta1, beta2, eps, weight_decay,
                               lr_dev, grad_scale, grad_coef, found_inf, found_inf2, ema, ema_out, ema_decay, ema_decay_dev, s);
}

// tensors with numel > 0 in groups of OPT_MAX_TENSORS, one launch each.  Returns the number of launches
int launch_ema_update(int n, const void* const* src, const int32_t* sdt, float* const* ema, void* const* ema_out, const int32_t* odt,
                      const int64_t* numel, float decay, const float* decay_dev, const float* found_inf, const float* found_inf2,
                      hipStream_t s) {
    int launches = 0;
    EmaArgs a;
    a.n = 0;
    unsigned int blocks = 0;
    auto flush = [&]() {
        if (a.n == 0) return;
        a.first_block[a.n] = blocks;
        a.decay = decay; a.decay_dev = decay_dev; a.found_inf = found_inf; a.found_inf2 = found_inf2;
        ema_update_kernel<<<dim3(blocks), dim3(256), 0, s>>>(a);
        ++launches;
        a.n = 0;
        blocks = 0;
    };
    for (int i = 0; i < n; ++i) {
        if (numel[i] == 0) continue;
        const int j = a.n++;
        void* out = ema_out ? ema_out[i] : nullptr;
        const int od = (out && odt) ? odt[i] : AECF_F32;
        a.src[j] = src[i]; a.ema[j] = ema[i]; a.ema_out[j] = od == AECF_F32 ? nullptr : out;
        a.numel[j] = numel[i];
        a.sdt[j] = (unsigned char)sdt[i]; a.odt[j] = (unsigned char)od;
        a.first_block[j] = blocks;
        const int be = opt_block_elems(sdt[i], od);
        blocks += (unsigned int)((numel[i] + be - 1) / be);
        if (a.n == OPT_MAX_TENSORS) flush();
    }
    flush();
    return launches;
}

int64_t grad_norm_blocks(int n, const int64_t* numel) {
    int64_t blocks = 0;
    for (int i = 0; i < n; ++i) blocks += (numel[i] + NORM_BLOCK_ELEMS - 1) / NORM_BLOCK_ELEMS;
    return blocks;
}

// partial: grad_norm_blocks(n, numel) floats (> 0: the caller returns early otherwise); out: 3 floats
void launch_grad_norm(int n, const void* const* g, const int32_t* gdt, const int64_t* numel, float max_norm, const float* grad_scale,
                      float* partial, float* out, hipStream_t s) {
    NormArgs a;
    a.n = 0;
    unsigned int blocks = 0;
    int64_t done = 0;
    auto flush = [&]() {
        if (a.n == 0) return;
        a.first_block[a.n] = blocks;
        a.partial = partial + done;
        grad_sumsq_kernel<<<dim3(blocks), dim3(256), 0, s>>>(a);
        done += blocks;
        a.n = 0;
        blocks = 0;
    };
    for (int i = 0; i < n; ++i) {
        if (numel[i] == 0) continue;
        const int k = a.n++;
        a.g[k] = g[i]; a.numel[k] = numel[i]; a.gdt[k] = (unsigned char)gdt[i];
        a.first_block[k] = blocks;
        blocks += (unsigned int)((numel[i] + NORM_BLOCK_ELEMS - 1) / NORM_BLOCK_ELEMS);
        if (a.n == OPT_MAX_TENSORS) flush();
    }
    flush();
    grad_sumsq_finalize_kernel<<<dim3(1), dim3(256), 0, s>>>(partial, done, max_norm, grad_scale, out);
}

}  // namespace aecf
