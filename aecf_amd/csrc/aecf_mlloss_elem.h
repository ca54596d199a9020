// The element of the multi-label classification loss (include/aecf_hip.h, "multi-label classification loss"), shared by the
// elementwise kernels over stored logits (aecf_mlloss.hip) and by the streaming classifier head that forms its logits in
// registers (aecf_mlhead_flash.hip): the form parameters, the target rules and the loss / derivative of one valid element.
#pragma once
#include "aecf_kernels.h"

namespace aecf {

struct MllArgs {
    float gp, gn, m, ome, he;           // gamma+, gamma-, margin, 1 - eps, eps / 2
};

inline MllArgs mll_args(float gp, float gn, float m, float eps) {
    MllArgs p;
    p.gp = gp; p.gn = gn; p.m = m; p.ome = 1.0f - eps; p.he = 0.5f * eps;
    return p;
}

template <int NB>
__device__ __forceinline__ void load_bytes(const void* p, void* dst) {
    constexpr int A = NB >= 16 ? 16 : NB;
    __builtin_memcpy(dst, __builtin_assume_aligned(p, A), NB);
}

// V targets at element idx: value (int kinds: non-zero -> 1) and validity (floating point: not NaN and not < 0; int8: not < 0)
template <int V>
__device__ __forceinline__ void load_targets(const void* labels, int kind, int64_t idx, float* t, bool* valid) {
    if (kind == 1) {
        float v[V];
        load_bytes<4 * V>((const float*)labels + idx, v);
#pragma unroll
        for (int j = 0; j < V; ++j) { t[j] = v[j]; valid[j] = v[j] >= 0.0f; }
    } else if (kind == 0 || kind == 2) {
        unsigned short v[V];
        load_bytes<2 * V>((const unsigned short*)labels + idx, v);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            t[j] = kind == 0 ? Tr<BF16>::to_f32(v[j]) : Tr<F16>::to_f32(v[j]);
            valid[j] = t[j] >= 0.0f;
        }
    } else {
        signed char v[V];
        load_bytes<V>((const signed char*)labels + idx, v);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            t[j] = v[j] != 0 ? 1.0f : 0.0f;
            valid[j] = kind == 3 || v[j] >= 0;
        }
    }
}

// the loss (GRAD false) or dl/dx (GRAD true) of one valid element
template <bool GRAD>
__device__ __forceinline__ float mll_elem(float x, float t, float a, float b, const MllArgs& p) {
    const float tp = t * p.ome + p.he;
    const float cp = a * tp, cn = b * (1.0f - tp);
    const float e = expf(-fabsf(x));
    const float l1p = log1pf(e);
    const float r = 1.0f / (1.0f + e);
    const float er = e * r;
    const bool up = x >= 0.0f;
    const float sg = up ? r : er;                   // sigmoid(x)
    const float s1 = up ? er : r;                   // 1 - sigmoid(x)
    const float nls = fmaxf(-x, 0.0f) + l1p;        // -log sigmoid(x)
    const float nl1 = fmaxf(x, 0.0f) + l1p;         // -log(1 - sigmoid(x))
    float out = 0.0f;
    if (cp > 0.0f) {
        const float wp = p.gp == 0.0f ? 1.0f : expf(-p.gp * nl1);
        if (!GRAD) {
            out = (cp * wp) * nls;
        } else {
            const float sl = sg > 0.0f ? sg * nls : 0.0f;           // s (-log s) -> 0 at x = -inf
            out = -(cp * wp) * (s1 + p.gp * sl);
        }
    }
    if (cn > 0.0f) {
        float neg = 0.0f;
        if (p.m == 0.0f) {
            const float wn = p.gn == 0.0f ? 1.0f : expf(-p.gn * nls);
            if (!GRAD) {
                neg = (cn * wn) * nl1;
            } else {
                const float sl = s1 > 0.0f ? s1 * nl1 : 0.0f;       // (1 - s) (-log(1 - s)) -> 0 at x = +inf
                neg = (cn * wn) * (sg + p.gn * sl);
            }
        } else {
            const float q = sg - p.m;
            if (!(q <= 0.0f)) {                                     // alive; a NaN stays alive
                const float om = s1 + p.m;                          // 1 - q
                const float nl = -logf(om);
                const float nlq = nl < 0.0f ? 0.0f : nl;             // (1 - q rounded above 1) by select: a NaN stays a NaN
                const float wn = p.gn == 0.0f ? 1.0f : expf(p.gn * logf(q));
                if (!GRAD) {
                    neg = (cn * wn) * nlq;
                } else {
                    float inner = wn / om;
                    if (p.gn != 0.0f) inner += p.gn * (wn / q) * nlq;
                    neg = cn * (sg * s1) * inner;
                }
            }
        }
        out += neg;
    }
    return out;
}

}  // namespace aecf
