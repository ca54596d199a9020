// The streaming loop of the contrastive kernels that never materialise the [rows, cols] scores (nce_flash_kernel of
// aecf_nce_flash.hip, sig_flash_kernel of aecf_sig_flash.hip), bf16, gfx950, with the host-side split rule and width dispatch
// that go with it.
//
// A block keeps 64 "stationary" rows (4 waves x 16) as MFMA B operands in registers and streams tiles of 32 rows of the other
// matrix through LDS (LDS-DMA, two buffers).  Per 16 x 16 sub-tile:
//   S[a, b]      = streamed_a . stationary_b        (16x16x32 MFMAs over d; accumulator row = a, column = b)
//   P[a, b]      = term.weights(S)                  what turns a score into a weight: the ONLY part a loss form owns
//   Out^T[c, b] += streamed^T[c, a] P[a, b]         16x16x16 MFMAs: the accumulator layout of S (4 consecutive a per lane) IS the
//                                                   B-operand layout of that instruction, and streamed^T is a transposed LDS
//                                                   read (ds_read_b64_tr_b16) of the tile already there
//
// A term is a small struct held by the kernel.  It carries the per-row scalars of its form (InfoNCE DQ: running maximum and
// sum; sigmoid DA: softplus and g sums; the DK / DB roles: none) and provides
//   static constexpr bool FENCED;      sched_barrier(0) around weights(): keeps the scheduler from pulling the next sub-tile's
//                                      fragment reads and this one's transposed reads above straight-line term arithmetic
//   void weights(sacc, a0, lg, r16, len, oacc, pv);
//                                      lane (lg, r16) holds S[a = a0 + 4 lg + r][b = r16], r = 0..3, a relative to the range's
//                                      start; rows a >= len are copies of the last valid one and must get weight 0.  Fills
//                                      pv[4]; may touch oacc (InfoNCE's DQ role rescales it).
#pragma once
#include <type_traits>

#include "aecf_kernels.h"
#include "aecf_tile.h"

namespace aecf {

// ---- host ----------------------------------------------------------------------------------------------------------------

// column splits of the role whose stationary rows are the local ones: enough blocks to fill 256 CUs, at least 512 columns
// per split, at most 64 (rule); per = the split length rounded up to the 32-row tile; live = the splits that rounding leaves
// non-empty (live <= rule; the empty ones are the last).  Workspaces may be sized by either count; only live splits run.
struct FlashSplit {
    int rule, live;
    int64_t per;
};
inline FlashSplit flash_split(int64_t rows, int64_t cols) {
    const int64_t rb = (rows + 63) / 64;
    int64_t ks = (256 + rb - 1) / rb;
    const int64_t max_ks = (cols + 511) / 512;
    if (ks > max_ks) ks = max_ks;
    if (ks < 1) ks = 1;
    if (ks > 64) ks = 64;
    FlashSplit o;
    o.rule = (int)ks;
    o.per = ((cols + ks - 1) / ks + 31) / 32 * 32;
    o.live = (int)((cols + o.per - 1) / o.per);
    return o;
}

// f(std::integral_constant<int, KT>) for the supported widths d = 32 KT (nce_flash_supported)
template <class F>
void dispatch_kt(int d, F&& f) {
    switch (d / 32) {
        case 4: f(std::integral_constant<int, 4>{}); break;
        case 8: f(std::integral_constant<int, 8>{}); break;
        case 12: f(std::integral_constant<int, 12>{}); break;
        case 16: f(std::integral_constant<int, 16>{}); break;
        case 24: f(std::integral_constant<int, 24>{}); break;
        default: f(std::integral_constant<int, 32>{}); break;
    }
}

// ---- device --------------------------------------------------------------------------------------------------------------

typedef short s16x4 __attribute__((ext_vector_type(4)));

// what a block works on: blockIdx.x = split * row blocks + row block; this wave's 16 stationary rows start at s0; the block
// streams rows m_beg .. m_beg + len - 1 (len > 0).  Every streamed index inside the loop is relative to m_beg: a 32-bit count
// (2^31 rows of the narrowest width, d = 128, are 512 GiB).
struct FlashBlock {
    int r16, lg, split, len;
    int64_t s0, m_beg;
};
template <bool SPLIT>
__device__ __forceinline__ FlashBlock flash_block(int64_t ns, int64_t nm, int64_t per_split) {
    FlashBlock f;
    const int lane = lane_id();
    f.r16 = lane & 15;
    f.lg = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(wave_id());
    const int nsb = (int)((ns + 63) / 64);
    const int sb = (int)blockIdx.x % nsb;
    f.split = (int)blockIdx.x / nsb;
    f.s0 = (int64_t)sb * 64 + 16 * w;
    f.m_beg = SPLIT ? (int64_t)f.split * per_split : 0;
    const int64_t m_end = SPLIT ? ((f.m_beg + per_split) < nm ? (f.m_beg + per_split) : nm) : nm;
    f.len = (int)(m_end - f.m_beg);
    return f;
}

// a streamed index relative to the block's range, -1 when it is not in it
__device__ __forceinline__ int flash_rel(int64_t idx, const FlashBlock& f) {
    const int64_t rel = idx - f.m_beg;
    return (rel >= 0 && rel < (int64_t)f.len) ? (int)rel : -1;
}

// oacc[c] (+)= the loop above over the block's range, for the NC output column blocks c_first .. c_first + NC - 1 (16 columns
// each); PRODUCT = false: scores and term only (NC = 1, oacc stays 0).  lds: 2 tiles of 32 rows x 64 KT bytes.
template <int KT, int NC, bool PRODUCT, class Term>
__device__ __forceinline__ void flash_stream(Term& term, const FlashBlock& f, const unsigned short* stat, int64_t ns,
                                             const unsigned short* strm, int c_first, char* lds, f32x4 (&oacc)[NC]) {
    using X = Tr<BF16>;
    constexpr int D = 32 * KT, ROWB = 2 * D, TILE = 32 * ROWB;
    const int r16 = f.r16, lg = f.lg, len = f.len;
    __builtin_assume(len > 0);      // only non-empty ranges are launched; knowing it, the compiler needs far fewer registers

    const char* msrc = reinterpret_cast<const char*>(strm) + f.m_beg * (int64_t)ROWB;
    auto issue = [&](int m0, int buf) {
        const int left = len - m0, mv = left < 32 ? left : 32;
        ws_dma_rows_asm<KT, 32, 1, 256>(msrc + m0 * (int64_t)ROWB, (unsigned)ROWB, mv, lds + buf * TILE);
    };
    issue(0, 0);

    // stationary rows as B operands: lane (lg, r16 = b): row s0 + r16, elements 32 ks + 8 lg .. + 7
    u32x4 sreg[KT];
    {
        int64_t srow = f.s0 + r16;
        srow = srow < ns ? srow : ns - 1;
        const unsigned short* sp = stat + srow * D + 8 * lg;
#pragma unroll
        for (int ks = 0; ks < KT; ++ks) sreg[ks] = *reinterpret_cast<const u32x4*>(sp + 32 * ks);
#pragma unroll
        for (int ks = 0; ks < KT; ++ks) asm volatile("" : "+v"(sreg[ks]));      // retire the loads before the loop
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) oacc[c] = f32x4{0.f, 0.f, 0.f, 0.f};

    // fragment / transposed-read addresses inside a tile (rows a, 16-byte chunk ^ (row & 15))
    int aaddr[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) aaddr[v] = r16 * ROWB + ((((4 * v) + lg) ^ r16) << 4);
    const int q = r16 >> 2, pp = r16 & 3;

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    int cur = 0;
    for (int m0 = 0; m0 < len; m0 += 32, cur ^= 1) {
        __builtin_amdgcn_s_barrier();
        if (m0 + 32 < len) issue(m0 + 32, cur ^ 1);
        const char* tb = lds + cur * TILE;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const int a0 = m0 + 16 * sub;                         // streamed rows m_beg + a0 .. + 15 of this sub-tile
            if (a0 >= len) break;                                 // block-uniform
            const char* ts = tb + 16 * sub * ROWB;
            // ---- S[a, b]: A = streamed rows (LDS), B = stationary rows (registers)
            f32x4 sacc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KT; ++ks) {
                const u32x4 af = *reinterpret_cast<const u32x4*>(ts + aaddr[ks & 3] + (ks >> 2) * 256);
                sacc = X::mma(af, sreg[ks], sacc);
            }
            if (Term::FENCED) __builtin_amdgcn_sched_barrier(0);
            float pv[4];
            term.weights(sacc, a0, lg, r16, len, oacc, pv);
            if (Term::FENCED) __builtin_amdgcn_sched_barrier(0);
            if (PRODUCT) {
                // ---- Out^T[c, b] += streamed^T[c, a] P[a, b]   (16x16x16: B operand = P as it sits in the accumulator,
                // rounded to bf16 HERE and nowhere else)
                const u32x2 pb2 = u32x2{pack_bf16x2(pv[0], pv[1]), pack_bf16x2(pv[2], pv[3])};
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
            if (Term::FENCED) __builtin_amdgcn_sched_barrier(0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
}

// lane (lg, r16 = b) holds Out[b][16 (c_first + c) + 4 lg + r]: row[...] = oacc (SCALE: times ct); row = &out[b][0]
template <int NC, bool SCALE>
__device__ __forceinline__ void flash_store(float* row, int c_first, int lg, const f32x4 (&oacc)[NC], float ct = 1.f) {
    float* po = row + 16 * c_first + 4 * lg;
#pragma unroll
    for (int c = 0; c < NC; ++c) *reinterpret_cast<f32x4*>(po + 16 * c) = SCALE ? oacc[c] * ct : oacc[c];
}

}  // namespace aecf
