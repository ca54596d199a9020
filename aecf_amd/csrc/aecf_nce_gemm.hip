// Contrastive term (InfoNCE) on three tile GEMMs, bf16, gfx950 -- the fast path of aecf_nce_fwd_bwd / aecf_nce_sym_*.
//
// Local rows a [R, d] against all (gathered) keys b [C, d], unit-norm rows, positives at column off + i:
//   pass 1   E[i, j] = exp((a_i.b_j - 1) / T)   bf16 [Rp, Cp] in the workspace, stored as [Rp/256][Cp/64] tiles of [256][64]
//            (32 KB each, contiguous: the copy of an operand tile of either product reads whole DRAM pages instead of 128-
//            or 512-byte pieces of rows 128 KB apart) (the shift 1/T bounds every logit of unit-norm
//            rows, so no running maximum is needed and COLUMN sums are meaningful across row blocks and across ranks);
//            row sums l_i and column sums c_j of E come out of the same epilogue (float32, fixed-order partials).
//   pass 2   W[i, j] = coef/T (E_ij (1/l_i + sym/c_j) - (1 + sym) [j = off + i])          in place over E
//            da = W b   (reduction over the keys, split over blocks, float32 slabs reduced in fixed order)
//            db = W^T a (reduction over the local rows)
// sym = 0 is one InfoNCE direction (row softmax); sym = 1 adds the other direction of the symmetric loss from the SAME
// logits block: its softmax runs down the columns, whose sums are the only thing ranks have to exchange (one all-reduce of
// C floats between the passes).  2 R C d flops for the logits + 4 R C d for the two gradient products, against 8 R C d per
// direction of the streaming form (aecf_nce_flash.hip), which stays as the O(R d)-workspace alternative.
//
// One kernel, three operand arrangements.  Block = 512 threads = 8 waves as 2 (m) x 4 (n), block tile 256 x 256, K-step 64,
// wave tile 128 x 64 = 8 x 4 accumulators of v_mfma_f32_16x16x32_bf16; both operand tiles arrive by LDS-DMA
// (global_load_lds_dwordx4, two stages of 2 x 32 KB), one raw s_barrier per K-step, the copy of step t + 1 flies behind the
// MFMAs of step t.  An operand whose K index is the fast axis of its source (OP_ROW: a, b in pass 1, W in da) is a
// [256 rows][128 B] tile read with ds_read_b128; one whose K index is the slow axis (OP_COL: b in da, W and a in db) is a
// [64 k][512 B] tile read TRANSPOSED with ds_read_b64_tr_b16 -- no transposed copy of W or of the embeddings exists.
// The product is formed transposed (the n operand is the MFMA A operand), so a lane ends with 4 consecutive output columns
// of one row: 8-byte bf16 / 16-byte float32 stores.
//
// The pairwise sigmoid (SigLIP) loss rides on the same kernel (aecf_sig_pass1 / aecf_sig_grads): l = a.b / Tc + bias,
// L = coef sum_ij softplus(-y_ij l_ij).  Its logits pass is the EPI_SIG epilogue: g = sigmoid(l) - [j = off + i] goes ONCE, as
// bf16, into the tiled workspace layout above (padding stored as 0), with two per-row float32 partials per n tile (sum softplus,
// sum g before the rounding) reduced in a fixed order by sig_rows_kernel / sig_dbias_kernel -- no column sums, no exchange
// between the passes, no weights pass.  g is stored UNSCALED: coef / Tc and the upstream scalar multiply the float32
// accumulators in the output stage of the two gradient products (EPI_OUT_S / EPI_OUT_TD_S), so nothing small is rounded to bf16
// (sigmoid = e^-30 is 9e-14 there) and one logits pass serves any upstream.  The epilogue holds v_exp, v_rcp and v_log per
// element (EPI_EXP: one v_exp); a block owns its CU (128 KB of stages), so there is no other block's MFMA work to hide them
// behind and no next tile in this block: what was done instead is to keep everything around them short -- the logit is never
// formed (n = l log2 e comes out of one packed fma on the accumulator), softplus needs no max, no select and no second
// exponential (sig_terms), the sums are packed adds, and the positive / ragged-edge selects run only in the tiles that hold
// such elements (a block-uniform branch).
//
// Retrieval ranks (aecf_retrieval_ranks, host side in aecf_retrieval.hip) are a fourth epilogue of the logits arrangement,
// EPI_RANK: nothing of the tile is stored.  Every float32 accumulator s_ij is compared with the threshold of its row
// (pos_row[i]) and of its column (pos_col[j], NULL = that direction off) and counted: greater and equal, per row over the
// tile's 256 columns and per column over its 256 rows, the positive (j = off + i) and the padding excluded -- selects that run
// only in the tiles that hold such elements, as in EPI_SIG.  A comparison with a NaN is false on both sides: such an
// element is counted nowhere.  How the counts leave the block: per-tile integer partials, greater in the low and equal in
// the high 16 bits of one int32 (a tile holds at most 256 of either), [n_tiles][Rp] for the rows and [m_tiles][Cp] for the
// columns, summed by rank_counts_kernel.  Taken over vector atomics onto zeroed outputs because it is the arrangement the
// row / column sums of the two losses already have (no memset node in front of the launch, no contended atomics on the
// 256 tiles of a row, plain coalesced stores); integer sums are exact in any order, so either would be deterministic.
//
// Top-k retrieval (aecf_retrieval_topk, host side and merge in aecf_retrieval.hip) is a fifth epilogue of the same arrangement,
// EPI_TOPK: nothing of the tile is stored either; every row of the tile leaves its best k candidates.  A candidate is ONE
// 64-bit key -- high word the order-preserving integer image of the float32 score (NaN -> 1: below -inf's 0x007fffff, above
// the sentinel 0; -0 counted as +0), low word the inverted global column -- so "higher score first, lower column first among
// equal scores" is a single unsigned compare and the result cannot depend on tile, block or rank order.  A lane sorts the 16
// keys it holds of a row (63 compare-exchanges, all in registers); the 4 lane groups holding the row's 64 columns of this
// wave then pop the largest head k times (two xor shuffles per pop) into LDS, where the stages were; one thread per row
// merges the 4 waves' lists into the tile's list [k] of the workspace [n_tiles][Rp][KP].  The accumulators are consumed rt by
// rt: 32 key registers at a time next to them, no scratch.  The excluded partner and the padding become the sentinel -- a
// select that only the tiles holding such elements run, as above.
//
// The symmetric supervised contrastive loss (aecf_supcon_sym_pass1 / _loss / _grads) is a sixth epilogue, EPI_SUP, plus label-aware
// variants of the three small kernels.  Both views share the labels, so one match matrix m_ij = [j = off + i] or [lr_i = lc_j >= 0]
// serves both directions, and the positives of the labels are a sparse correction to InfoNCE's weights:
//   W_ij = ct (E_ij (1/l_i + 1/c_j) - m_ij (1/n_i + 1/nc_j)),   n_i = sum_j m_ij,  nc_j = sum_i m_ij.
// EPI_SUP is EPI_EXP_DT to the bit (E, its row and column sums) and adds, per row and per column of the tile, the count and the
// float32 sum of the raw accumulators of the matches BY LABEL -- the partner is excluded (tiles on its band and on the ragged edge
// take the block-uniform `special` branch) and joins later from its own float32 dot, as in InfoNCE.  A lane reads the labels of
// its 8 rows and 16 columns once, in front of the exponentials, and keeps them as 32-bit keys (24 registers; the int64 labels
// themselves would take 48 beside the 128 accumulators and spill): the tile is searched with two VALU operations per element
// and no compare mask, and only a row group with a key hit somewhere in the wave reads its labels again, compares all 64 bits and
// sums -- at about 6 matches in 65536 columns most groups skip it, and a skipped group stores the zeros it would have summed.
// The column sums of the matches gather in LDS, in the slots of the lanes that own them, not in 32 more registers.
// The partials leave as the sums of E do ([n_tiles][Rp] / [m_tiles][Cp], fixed order, no atomics); sup_sums_kernel reduces three
// quantities where nce_sums_kernel reduces one, counts as float32 so that ONE all-reduce of [3][cols] carries what ranks
// exchange; sup_finalize_kernel puts the mean of the positives' scores where InfoNCE has the partner's, and sup_weights_kernel
// forms m again from the labels (8 bytes per column, L2-resident) and subtracts 1/n_i + 1/nc_j -- exactly 2.0f where no label is
// shared, so that every output then has InfoNCE's bits.  The gradient products are launch_grad_products, unchanged.
//
// The multi-label form (aecf_supcon_ml_sym_pass1 / _loss / _grads) gives every row a SET of classes, one uint64 (bit c = class c),
// and a weight w_ij in [0, 1] where the single-label form has a match: [A_i & B_j != 0] (overlap) or |A_i & B_j| / |A_i | B_j|
// (Jaccard), 1 for the partner by index.  The weights are dense -- thousands of positives per row -- so the sparse vote of EPI_SUP
// has no place: EPI_SETS_OV / EPI_SETS_JAC (the weighting is a template parameter) run a dense sweep over every tile.
//   * The E loop is EPI_EXP_DT's, untouched: E and its row and column sums keep their bits.
//   * The block's 256 row words and 256 column words (4 KiB; the padding as the empty set, which weighs 0 against everything) are
//     read in front of the exponentials and staged in the LDS the operand stages have vacated; the sweep reads them from there,
//     so no set lives in a register across the E loop.
//   * The sweep runs AFTER the E loop, when its 24 sum registers are dead, column group (ct) by column group: a lane holds the 4
//     column words of the group (and, Jaccard, their popcounts), 8 column accumulators and 16 row accumulators, and reads the row
//     word of each of its 8 row groups from LDS.  Jaccard takes ONE 64-bit popcount per element (the intersection; the union is
//     pa + pb - inter from the per-word popcounts) and one correctly rounded float32 division.
//   * Summation order, the same for the sum of w and for the sum of w * accumulator (each product fused into its addition, one
//     rounding): a ROW's statistic is a chain over the lane's 16 elements of the row, ct-major (16 additions), then the 4 lane
//     groups (xor 16, xor 32: 2), the block's 4 column waves ((w0 + w1) + (w2 + w3): 2), then sup_sums_kernel over the n tiles
//     (ceil(n_tiles / 4) + 2).  A COLUMN's is a chain over the lane's 8 row groups (8), the 16 lanes of the group (4), the 2 row
//     waves (1), then sup_sums_kernel over the m tiles (ceil(m_tiles / 4) + 2).  The partner is excluded by index on the tiles
//     of its band (the block-uniform `special` branch) and joins later from its own float32 dot with weight 1.
// sup_sums_kernel and sup_finalize_kernel serve unchanged (the weight sums stand where the counts stood); set_weights_kernel forms
// w again from the words next to sup_weights_kernel.
//
// NT-Xent (aecf_ntxent_sym_pass1 / _loss / _grads) is the pool of both views -- every row of either view an anchor against the other
// 2 C - 1 rows -- on THREE logits blocks of one rank: X = a_loc . b_all^T is the InfoNCE pass above, unchanged (EPI_EXP_DT); Y = a_loc .
// a_all^T and Z = b_loc . b_all^T hold the anchor itself at column row_offset + i, and EPI_EXP_SELF leaves it out: E = 0 in the stored
// tile and in the row sum, by index (exp((a.a - 1) / T) is about 1 beside sums that may total 1e-10: it cannot be subtracted later,
// and a bit-identical row elsewhere in the view is a legitimate key).  It is EPI_EXP_DT's E loop; the tiles the band of excluded
// keys crosses take the block-uniform branch of the ragged edge, and the column sums, which nobody needs, are not formed.  The
// b x a block is X^T.  Da = lX + lY is local; Db = the ranks' column sums of X plus lZ of the row's owner: ntx_combine_kernel adds a
// rank's lZ into its own range of its column sums before the ONE all-reduce.  nce_finalize_kernel and nce_weights_dt_kernel serve
// unchanged (l := Da, c := Db; Y and Z with v = 0, Z with u_i = 1 / Db_(off + i) from ntx_prep_kernel), and the six gradient products
// are the da / db launchers: two da products leave their slabs behind one another for one slab sum (d a_loc), two db products a
// float32 stage (d b_all) -- one rounding per output.  18 R C d flops against 64 for two pooled streaming directions.
//
// The pooled supervised contrastive loss (aecf_supcon_pool_sym_pass1 / _loss / _grads; Khosla et al.: every row of either view an
// anchor, its positives the partner and every row of the pool with its label) is NT-Xent's three blocks with the label statistics of
// the supervised loss on each: X runs EPI_SUP unchanged, Y and Z a seventh epilogue, EPI_SUP_SELF -- EPI_EXP_SELF's E loop and the ROW
// half of EPI_SUP's label search (the anchor excluded by index where X excludes the partner), without the 32 column accumulators of
// E and the LDS column slots of the matches.  sup_pool_combine_kernel adds X's and Y's row statistics (anchor a_i) and puts Z's into
// the rank's own range of col_stats [3][cols] before the one all-reduce (anchor b_g); sup_finalize_kernel and sup_weights_kernel serve
// unchanged, Y and Z take the SELF variant of the weights (v = rnc = 0, nothing at the excluded key).  Products as NT-Xent's.
//
// The pooled multi-label form (aecf_supcon_ml_pool_sym_pass1 / _loss / _grads) is that pooled loss with the dense set weights of the
// multi-label form: X runs EPI_SETS_OV / EPI_SETS_JAC unchanged, Y and Z two further epilogues, EPI_SETS_OV_SELF / EPI_SETS_JAC_SELF --
// EPI_EXP_SELF's E loop, the words staged in LDS as EPI_SETS_* stage them, then the ROW half of the dense sweep in the same chain
// order (ct-major over the lane's 16 elements of a row, the lane groups, the four column waves, sup_sums_kernel), the anchor's own
// element weighing 0 BY INDEX on the tiles the band crosses (a bit-identical row with the same set elsewhere in the view is a
// positive).  No column accumulators, LDS column slots or column partials: neither instance needs scratch.  Workspace, combine, prep,
// finalize and the products are the pooled form's; set_weights_kernel's SELF variant (W = ct (E u_i - w rn_i), v = rnc = 0, w := 0 at
// the anchor's own key) serves Y and Z.  Two blocks' overlap weight sums add in float32: cols <= 2^23.
#include <math.h>
#include <type_traits>

#include "aecf_kernels.h"
#include "aecf_tile.h"

namespace aecf {

namespace {

enum { OP_ROW = 0, OP_COL = 1, OP_COLB = 2 };      // OP_COLB: OP_COL from the tiled E (m operand of db)
// _DT / _TD forms (device temperature): EPI_EXP_DT derives scale2 / shift2 from max(*temp, min_temp); EPI_OUT_TD also writes the
// block's sum of acc * (the bf16 m-operand rows of tdot_src at the output's position) -- q_i.dq_i summed over the tile, from the
// float32 accumulator -- to tdot_part[(split m_tiles + mi) n_tiles + ni]
// EPI_SIG (sigmoid loss, logits pass): g = sigmoid(l) - [positive] as bf16 into the tiled workspace + two per-row partials per
// n tile; EPI_OUT_S / EPI_OUT_TD_S: EPI_OUT / EPI_OUT_TD with the float32 accumulator multiplied by coef / Tc * upstream first
// EPI_RANK (retrieval ranks, logits pass): nothing stored; per-tile counts of acc > / == the row's and the column's threshold
// EPI_TOPK (top-k retrieval, logits pass): nothing stored; per-tile sorted lists of the k best (score, column) keys of every row
// EPI_SUP (supervised contrastive loss, logits pass): EPI_EXP_DT plus, per row and per column of the tile, the count and the float32
// sum of the raw accumulators of the elements that match by label (the partner and the padding excluded)
enum { EPI_EXP = 0, EPI_OUT = 1, EPI_EXP_DT = 2, EPI_OUT_TD = 3, EPI_SIG = 4, EPI_OUT_S = 5, EPI_OUT_TD_S = 6, EPI_RANK = 7, EPI_TOPK = 8,
       EPI_SUP = 9, EPI_SETS_OV = 10, EPI_SETS_JAC = 11, EPI_EXP_SELF = 12, EPI_SUP_SELF = 13,
       EPI_SETS_OV_SELF = 14, EPI_SETS_JAC_SELF = 15 };
// EPI_SETS_OV / EPI_SETS_JAC (multi-label contrastive loss, logits pass): EPI_EXP_DT plus, per row and per column of the tile, the
// float32 sums of w and of w * raw accumulator, w the overlap / Jaccard weight of the two class sets (partner and padding excluded)
constexpr bool epi_is_sets(int epi) { return epi == EPI_SETS_OV || epi == EPI_SETS_JAC; }
// EPI_EXP_SELF (NT-Xent, the a x a and b x b blocks of the logits pass): EPI_EXP_DT with ONE key per row left out BY INDEX -- the
// element of row i at column row_offset + i (the anchor itself in the gathered rows of its own view) is E = 0 in the stored tile
// and in the row sum, whatever its value; only the row sums leave the block (no column partials)
// EPI_SUP_SELF (pooled supervised contrastive loss, the a x a and b x b blocks): EPI_EXP_SELF's E loop, then the ROW half of EPI_SUP's
// label search -- count and float32 raw-score sum of the matches by label per row, the anchor itself (column row_offset + i) left
// out by index where EPI_SUP leaves the partner out; no column sums, counts or partials of any kind
// EPI_SETS_OV_SELF / EPI_SETS_JAC_SELF (pooled multi-label contrastive loss, the a x a and b x b blocks): EPI_EXP_SELF's E loop, then
// the ROW half of the dense sweep of EPI_SETS_* -- the float32 sums of w and of w * raw accumulator per row, the anchor itself
// (column row_offset + i) with weight 0 by index where EPI_SETS_* leave the partner out; no column sums or partials of any kind
constexpr bool epi_is_sets_self(int epi) { return epi == EPI_SETS_OV_SELF || epi == EPI_SETS_JAC_SELF; }
constexpr bool epi_has_sets(int epi) { return epi_is_sets(epi) || epi_is_sets_self(epi); }    // the class words are staged in LDS
constexpr bool epi_is_self(int epi) { return epi == EPI_EXP_SELF || epi == EPI_SUP_SELF || epi_is_sets_self(epi); }
constexpr bool epi_has_labels(int epi) { return epi == EPI_SUP || epi == EPI_SUP_SELF; }
enum { MAP_2D = 0, MAP_UNITS = 1, MAP_SPLITX = 2 };

constexpr int BT = 256;                 // block tile (m and n)
constexpr int OPB = 32768;              // bytes of one operand tile (256 x 64 bf16)
constexpr int STAGE = 2 * OPB;

struct NceGemmArgs {
    const char* a;                      // m operand
    const char* b;                      // n operand
    unsigned int lda, ldb;              // source row pitch, bytes
    int64_t a_sm, a_st;                 // OP_ROW m operand: origin of tile (mi, t) = a + mi a_sm + t a_st;  OP_COLB: a_sm = tiles per tile row
    int a_rows, b_rows;                 // source rows that exist (the rest re-read the last one)
    int a_cbytes, b_cbytes;             // OP_COL: bytes of a source row that exist (multiple of 16; the rest re-read chunk 0)
    int m_tiles, n_tiles, k_steps;      // output tiles, K / 64
    int splits, steps_per_split;        // MAP_UNITS: K range of a block
    int m_valid, n_valid;               // output rows / columns that exist
    // EPI_EXP
    unsigned short* e;                  // [m_tiles][e_tiles][256][64]
    int64_t e_tiles;                    // tiles of 64 columns per tile row = Cp / 64
    float scale2, shift2;               // E = exp2(acc * scale2 - shift2)
    float* rowsum_part;                 // [n_tiles][m_tiles 256]
    float* colsum_part;                 // [m_tiles][n_tiles 256]
    // EPI_OUT
    void* out;                          // [splits][m_valid][ldo] float32, or (out_bf16, no splits) bf16
    int64_t ldo, slab_stride;
    int out_bf16;
    // EPI_EXP_DT
    const float* temp;
    float min_temp;
    // EPI_OUT_TD
    const unsigned short* tdot_src;     // [m_valid][ldo] bf16
    float* tdot_part;                   // [splits][m_tiles][n_tiles]
    // EPI_SIG (also reads temp / min_temp and writes g through e / e_tiles)
    const float* bias;                  // device scalar
    int64_t row_offset;                 // the positive of output row i is column row_offset + i
    float* sp_part;                     // [n_tiles][m_tiles 256]  sum_j softplus(-y l)
    float* sg_part;                     // [n_tiles][m_tiles 256]  sum_j (sigmoid(l) - [positive]), float32 before the bf16 rounding
    // EPI_OUT_S / EPI_OUT_TD_S (also read temp / min_temp)
    float coef;
    const float* upstream;              // device scalar, may be NULL (= 1)
    // EPI_RANK (also reads row_offset)
    const float* pos_row;               // [m_valid]  threshold of output row i
    const float* pos_col;               // [n_valid]  threshold of output column j; NULL: no column counts
    int* rank_row_part;                 // [n_tiles][m_tiles 256]  greater | equal << 16
    int* rank_col_part;                 // [m_tiles][n_tiles 256]
    // EPI_TOPK (also reads row_offset: the excluded partner of output row i is column row_offset + i)
    unsigned long long* topk_part;      // [n_tiles][m_tiles 256][topk_kp]  keys, best first; slots >= topk are not written
    int topk, topk_kp;                  // k <= 16 and the list pitch (k rounded up to a power of two)
    // EPI_SUP (also reads temp / min_temp / row_offset and writes E and its sums as EPI_EXP_DT)
    const long long* lab_row;           // [m_valid]  int64 class of output row i (negative: unlabeled)
    const long long* lab_col;           // [n_valid]  int64 class of output column j
    float* rowcnt_part;                 // [n_tiles][m_tiles 256]  matches by label per row of the tile, as float32
    float* rowsx_part;                  // [n_tiles][m_tiles 256]  float32 sum of their accumulators
    float* colcnt_part;                 // [m_tiles][n_tiles 256]  the same per column
    float* colsx_part;                  // [m_tiles][n_tiles 256]
    // EPI_SETS_OV / EPI_SETS_JAC: lab_row / lab_col hold the uint64 class sets of the rows / columns (bit c = class c), the four
    // partials above the sums of w and of w * accumulator
};

// The match by label of the supervised contrastive loss: the same non-negative class, all 64 bits compared.  The ONE place that
// decides it (the logits epilogue and the weights pass both call it): a set-valued form would put its overlap or Jaccard weight
// here.  The partner (column row_offset + i) is a positive by index and is handled by the callers.
// label k of a [n <= 2^24] int64 array through a 32-bit byte offset: one address register per load beside a uniform base
__device__ __forceinline__ long long sup_label_at(const long long* labels, int k) {
    return *reinterpret_cast<const long long*>(reinterpret_cast<const char*>(labels) + ((unsigned int)k << 3));
}
__device__ __forceinline__ bool sup_label_match(long long row_label, long long col_label) {
    return row_label >= 0 && row_label == col_label;
}
// a 31-bit key of a class for the epilogue's search: equal classes have equal keys (the converse is decided by sup_label_match)
__device__ __forceinline__ unsigned int sup_label_key(long long label) {
    return ((unsigned int)label ^ ((unsigned int)((unsigned long long)label >> 32) * 0x9e3779b1u)) & 0x7fffffffu;
}

// The weight of two class sets (multi-label form): JAC false: 1 where they share a class; true: |A & B| / |A | B| over all 64 bits,
// ONE correctly rounded float32 division, 0 for an empty union.  pa / pb: the popcounts of the two words (read by JAC only).  The
// ONE place that decides it: the logits epilogue and the weights pass both call it.
template <bool JAC>
__device__ __forceinline__ float set_weight(unsigned long long a, unsigned long long b, int pa, int pb) {
    const unsigned long long both = a & b;
    if (!JAC) return both != 0ull ? 1.f : 0.f;
    const int inter = __popcll(both), uni = pa + pb - inter;
    return __fdiv_rn((float)inter, (float)(uni > 0 ? uni : 1));
}

// sigmoid(x) and the pieces of softplus(x) for x = n ln 2, two elements: u = 2^min(n, 126), t = 1 + u, r = 1 / t;
//   sigmoid = u r,   softplus = ln 2 * lg2 + corr with lg2 = log2 t + (n - min(n, 126)) and corr = (u - (t - 1)) r:
// corr hands back what the rounding of 1 + u dropped (t - 1 and u - (t - 1) are exact), so softplus keeps its relative
// accuracy down to u ~ 1e-38 without a branch; the clamp keeps u finite for any 1 / T (past it sigmoid is 1 and softplus x).
struct SigTerms {
    f32x2 sig, lg2, corr;
};
__device__ __forceinline__ SigTerms sig_terms(f32x2 n) {
    const f32x2 nc = f32x2{fminf(n[0], 126.f), fminf(n[1], 126.f)};
    const f32x2 u = f32x2{__builtin_amdgcn_exp2f(nc[0]), __builtin_amdgcn_exp2f(nc[1])};
    const f32x2 t = u + f32x2{1.f, 1.f};
    const f32x2 r = f32x2{__builtin_amdgcn_rcpf(t[0]), __builtin_amdgcn_rcpf(t[1])};
    SigTerms o;
    o.sig = u * r;
    o.lg2 = f32x2{__builtin_amdgcn_logf(t[0]), __builtin_amdgcn_logf(t[1])} + (n - nc);
    o.corr = (u - (t - f32x2{1.f, 1.f})) * r;
    return o;
}

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
__device__ __forceinline__ void dma16(const char* src, unsigned int voff, char* lds_dst) {
    const unsigned int dst = (unsigned)(size_t)(lds_void_t*)lds_dst;
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(src), "s"(dst) : "memory", "m0");
}
#pragma clang diagnostic pop

// [256 rows][128 B] tile (OP_ROW), 16-byte chunk p of row r at chunk p ^ ((r >> 1) & 7): 16 consecutive rows x one logical chunk
// cover the 16 slots of a 256-byte bank row (conflict-free ds_read_b128).  The DMA destination is lane-linear, so the
// permutation goes on the source address.  A tile is 4 pieces (one wave-instruction per wave each); piece i of thread tid
// copies chunk c = tid + 512 i: row (tid >> 3) + 64 i, physical chunk tid & 7.  Rows >= rows_valid re-read the last one.
//
// [64 k][512 B] tile (OP_COL) = two [64][256 B] images of 8-row x 32-column subtiles (cdna_hip_programming.md T10, image (a)):
//   off(r, ch) = 2048 (r >> 3) + 512 (ch >> 2) + 64 (r & 7) + 16 ((ch & 3) ^ ((r >> 2) & 3))
// chunk c = tid + 512 i of image im lands at byte 16 c = row 8 (c >> 7) + ((c >> 2) & 7), chunk 4 ((c >> 5) & 3) + ((c & 3) ^ ((row >> 2) & 3));
// piece = 2 im + i.  cbytes = bytes of the source row that exist from the tile's first column on (chunks past it re-read chunk 0).
struct OperandSrc {
    const char* src;                    // origin of the tile (wave-uniform)
    int rows_valid;
};

template <int MODE, int PIECE>
__device__ __forceinline__ void issue_piece(const OperandSrc& o, unsigned int ld, int cbytes, char* lds) {
    const int tid = threadIdx.x;
    const int wbase = __builtin_amdgcn_readfirstlane(tid & ~63);
    if (MODE == OP_ROW) {
        const int row = (tid >> 3) + 64 * PIECE;
        const int rowc = row < o.rows_valid ? row : o.rows_valid - 1;
        const unsigned int voff = (unsigned)rowc * ld + (unsigned)(((tid & 7) ^ ((tid >> 4) & 7)) << 4);
        dma16(o.src, voff, lds + (wbase + 512 * PIECE) * 16);
    } else {
        constexpr int im = PIECE >> 1, i = PIECE & 1;
        const int row = 8 * (tid >> 7) + 32 * i + ((tid >> 2) & 7);
        const int rowc = row < o.rows_valid ? row : o.rows_valid - 1;
        int cb = 256 * im + 16 * (4 * ((tid >> 5) & 3) + ((tid & 3) ^ ((row >> 2) & 3)));
        if (MODE == OP_COLB) {
            // columns 64 jb .. 64 jb + 63 of a tile row live in tile jb: [256 rows][128 B], 32 KB apart
            dma16(o.src, (unsigned)row * 128u + (unsigned)(cb >> 7) * 32768u + (unsigned)(cb & 127),
                  lds + 16384 * im + (wbase + 512 * i) * 16);
        } else {
            cb = cb < cbytes ? cb : 0;
            dma16(o.src, (unsigned)rowc * ld + (unsigned)cb, lds + 16384 * im + (wbase + 512 * i) * 16);
        }
    }
}

// block id (virtual: a block of the logits pass walks several) -> (m tile, n tile, K split); false = padding id
template <int MAP>
__device__ __forceinline__ bool nce_tile_of(const NceGemmArgs& p, unsigned int vb, int& mi, int& ni, int& split) {
    const unsigned int x = vb & 7u, s = vb >> 3;                // blocks b and b + 8 share an XCD (its L2)
    split = 0;
    if (MAP == MAP_2D) {
        // 32 consecutive blocks of an XCD form a 4 (m) x 8 (n) patch of tiles: 12 operand panels serve 32 tiles
        const unsigned int nsm = (p.m_tiles + 3) / 4, nsn = (p.n_tiles + 7) / 8;
        const unsigned int T = (s >> 5) * 8u + x, wi = s & 31u;
        if (T >= nsm * nsn) return false;
        mi = (int)((T / nsn) * 4 + (wi & 3));
        ni = (int)((T % nsn) * 8 + (wi >> 2));
        return mi < p.m_tiles && ni < p.n_tiles;
    } else if (MAP == MAP_SPLITX) {
        // 8 K splits, one per XCD: every block of an XCD walks the same K range, so the n operand's K slices are shared by
        // all of them through its L2; the n tiles of an m tile are neighbours (the m operand is fetched once)
        ni = (int)(s % p.n_tiles);
        mi = (int)(s / p.n_tiles);
        split = (int)x;
        return mi < p.m_tiles;
    } else {
        // the n tiles of one (m tile, K split) are neighbours on one XCD: the big operand is fetched from HBM once
        const unsigned int unit = (s / p.n_tiles) * 8u + x;
        if (unit >= (unsigned)(p.m_tiles * p.splits)) return false;
        ni = (int)(s % p.n_tiles);
        mi = (int)(unit % p.m_tiles);
        split = (int)(unit / p.m_tiles);
        return true;
    }
}

template <int AM, int BM, int EPI, int MAP>
__global__ __launch_bounds__(512, 2) void nce_gemm_kernel(NceGemmArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = lane_id(), r16 = lane & 15, lg = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(wave_id());
    const int wm = w >> 2, wn = w & 3;

    // ---- fragment addresses
    int a_row[2], b_row[2];             // OP_ROW: per K-step of 32
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        const int ch = ((4 * ks + lg) ^ (r16 >> 1)) & 7;
        a_row[ks] = (128 * wm + r16) * 128 + (ch << 4);
        b_row[ks] = (64 * wn + r16) * 128 + (ch << 4);
    }
    // OP_COL: lane 4 q + pp of group lg reads row 32 ks + 8 lg + 4 hh + q, columns 4 pp .. 4 pp + 3 of 16-column block blk:
    //   8192 ks + 2048 lg + 512 (blk >> 1) + 256 hh + 64 q + 16 ((2 (blk & 1) + (pp >> 1)) ^ (2 (lg & 1) + hh)) + 8 (pp & 1)
    const int q = r16 >> 2, pp = r16 & 3;
    int tx[2][2];
#pragma unroll
    for (int b1 = 0; b1 < 2; ++b1)
#pragma unroll
        for (int hh = 0; hh < 2; ++hh)
            tx[b1][hh] = 2048 * lg + 64 * q + 8 * (pp & 1) + 256 * hh + 16 * ((2 * b1 + (pp >> 1)) ^ (2 * (lg & 1) + hh));
    const int a_img = 16384 * wm;                               // m blocks 8 wm + rt: image wm, block rt
    const int b_img = 16384 * (wn >> 1) + 512 * (2 * (wn & 1)); // n blocks 4 wn + ct: image wn >> 1, block 4 (wn & 1) + ct

    // operand tile of K-step t of output tile (mi, ni)
    auto src_a = [&](int t, int mi) -> OperandSrc {
        if (AM == OP_ROW) return OperandSrc{p.a + mi * p.a_sm + t * p.a_st, p.a_rows - BT * mi};
        if (AM == OP_COLB)      // K rows 64 t .. of tile row t / 4, columns of tiles 4 mi .. 4 mi + 3
            return OperandSrc{p.a + ((int64_t)(t >> 2) * p.a_sm + 4 * (int64_t)mi) * 32768 + (t & 3) * 8192, 64};
        const int k0 = 64 * t < p.a_rows ? 64 * t : p.a_rows - 1;
        return OperandSrc{p.a + (int64_t)k0 * p.lda + 512 * (int64_t)mi, 64 * t < p.a_rows ? p.a_rows - 64 * t : 1};
    };
    auto src_b = [&](int t, int ni) -> OperandSrc {
        if (BM == OP_ROW) return OperandSrc{p.b + (int64_t)BT * ni * p.ldb + 128 * (int64_t)t, p.b_rows - BT * ni};
        const int k0 = 64 * t < p.b_rows ? 64 * t : p.b_rows - 1;
        return OperandSrc{p.b + (int64_t)k0 * p.ldb + 512 * (int64_t)ni, 64 * t < p.b_rows ? p.b_rows - 64 * t : 1};
    };
#define NCE_PIECE(P_, oa_, ob_, stage_, mi_, ni_)                                                                       \
    do {                                                                                                                \
        if ((P_) < 4) issue_piece<AM, (P_) & 3>(oa_, p.lda, p.a_cbytes - 512 * (mi_), smem + (stage_) * STAGE);          \
        else issue_piece<BM, (P_) & 3>(ob_, p.ldb, p.b_cbytes - 512 * (ni_), smem + (stage_) * STAGE + OPB);             \
    } while (0)
    // fragment of slot sl = 8 ks + rt (m operand) / of (ks, ct) (n operand) from the tile at lds
    auto read_a = [&](const char* la, int sl) -> u32x4 {
        const int ks = sl >> 3, rt = sl & 7;
        if (AM == OP_ROW) return *reinterpret_cast<const u32x4*>(la + a_row[ks] + 2048 * rt);
        const int o = a_img + 8192 * ks + 512 * (rt >> 1);
        return tr_frag16(la, o + tx[rt & 1][0], o + tx[rt & 1][1]);
    };
    auto read_b = [&](const char* lb, int ks, int ct) -> u32x4 {
        if (BM == OP_ROW) return *reinterpret_cast<const u32x4*>(lb + b_row[ks] + 2048 * ct);
        const int o = b_img + 8192 * ks + 512 * (ct >> 1);
        return tr_frag16(lb, o + tx[ct & 1][0], o + tx[ct & 1][1]);
    };
    auto k_range = [&](int split, int& t_beg, int& t_end) {
        t_beg = split * p.steps_per_split;
        t_end = t_beg + p.steps_per_split < p.k_steps ? t_beg + p.steps_per_split : p.k_steps;
    };
    OperandSrc pa = {nullptr, 1}, pb = {nullptr, 1};            // the copy whose pieces 3..7 are still to be issued
    // first copies of an output tile: step t_beg whole into stage 0, the first 3 pieces of step t_beg + 1 into stage 1
    auto issue_first = [&](int mi, int ni, int t_beg, int t_end) {
        if (t_beg >= t_end) return;
        const OperandSrc oa = src_a(t_beg, mi), ob = src_b(t_beg, ni);
        NCE_PIECE(0, oa, ob, 0, mi, ni); NCE_PIECE(1, oa, ob, 0, mi, ni); NCE_PIECE(2, oa, ob, 0, mi, ni);
        NCE_PIECE(3, oa, ob, 0, mi, ni); NCE_PIECE(4, oa, ob, 0, mi, ni); NCE_PIECE(5, oa, ob, 0, mi, ni);
        NCE_PIECE(6, oa, ob, 0, mi, ni); NCE_PIECE(7, oa, ob, 0, mi, ni);
        if (t_beg + 1 < t_end) {
            pa = src_a(t_beg + 1, mi); pb = src_b(t_beg + 1, ni);
            NCE_PIECE(0, pa, pb, 1, mi, ni); NCE_PIECE(1, pa, pb, 1, mi, ni); NCE_PIECE(2, pa, pb, 1, mi, ni);
        }
    };

    int mi = 0, ni = 0, split = 0, t_beg = 0, t_end = 0;
    if (!nce_tile_of<MAP>(p, blockIdx.x, mi, ni, split)) return;
    k_range(split, t_beg, t_end);
    issue_first(mi, ni, t_beg, t_end);
    {
        f32x4 acc[8][4];
#pragma unroll
        for (int rt = 0; rt < 8; ++rt)
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};

        // ---- main loop.  A K-step is 16 slots of 4 MFMAs (slot = (ks, rt): one m fragment against the 4 n fragments); the m
        // fragments run through a ring of 4 registers, read 3 slots ahead.  ONE barrier per K-step, at slot 13: by then every
        // read of this step's stage has been issued (and is waited for), and the copy of step t + 1 -- issued a full step
        // earlier -- is waited for, so behind the barrier (a) slots 13..15 read the first fragments of step t + 1 from the
        // other stage (no bubble at the step boundary) and (b) the copy of step t + 2 into THIS stage starts.  The 8
        // wave-instructions of a copy are spread over 8 slots (3 behind the barrier, 5 at the start of the next step) so that
        // their issue cost hides behind MFMAs instead of stacking up in front of them.
        u32x4 af[4], bf0[4], bf1[4];
        if (t_beg < t_end) {
            // younger than the first step's 8 pieces: the 3 pieces of the second step
            if (t_beg + 1 < t_end) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            af[0] = read_a(smem, 0); af[1] = read_a(smem, 1); af[2] = read_a(smem, 2);
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) bf0[ct] = read_b(smem + OPB, 0, ct);
        }
        int st = 0;
        // one K-step; H1 / H2: steps t + 1 / t + 2 exist (compile-time: the steady-state body has no branches)
        auto kstep = [&](int t, auto h1, auto h2) {
            constexpr bool H1 = decltype(h1)::value, H2 = decltype(h2)::value;
            const char* cur = smem + st * STAGE;
            const char* nxt = smem + (st ^ 1) * STAGE;
            OperandSrc qa = {nullptr, 1}, qb = {nullptr, 1};
#pragma unroll
            for (int sl = 0; sl < 16; ++sl) {
                if (sl == 13 && H1) {
                    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
                    __builtin_amdgcn_s_barrier();
                    if (H2) { qa = src_a(t + 2, mi); qb = src_b(t + 2, ni); }
                }
                if (sl < 5 && H1) {
                    switch (sl) {
                        case 0: NCE_PIECE(3, pa, pb, st ^ 1, mi, ni); break;
                        case 1: NCE_PIECE(4, pa, pb, st ^ 1, mi, ni); break;
                        case 2: NCE_PIECE(5, pa, pb, st ^ 1, mi, ni); break;
                        case 3: NCE_PIECE(6, pa, pb, st ^ 1, mi, ni); break;
                        default: NCE_PIECE(7, pa, pb, st ^ 1, mi, ni); break;
                    }
                }
                if (sl >= 13 && H2) {
                    switch (sl) {
                        case 13: NCE_PIECE(0, qa, qb, st, mi, ni); break;
                        case 14: NCE_PIECE(1, qa, qb, st, mi, ni); break;
                        default: NCE_PIECE(2, qa, qb, st, mi, ni); break;
                    }
                }
                if (sl <= 12) af[(sl + 3) & 3] = read_a(cur, sl + 3);
                else if (H1) af[(sl + 3) & 3] = read_a(nxt, sl - 13);
                if (sl >= 4 && sl <= 7) bf1[sl - 4] = read_b(cur + OPB, 1, sl - 4);
                if (sl >= 13 && H1) {
                    bf0[sl - 13] = read_b(nxt + OPB, 0, sl - 13);
                    if (sl == 15) bf0[3] = read_b(nxt + OPB, 0, 3);
                }
#pragma unroll
                for (int ct = 0; ct < 4; ++ct)
                    acc[sl & 7][ct] = Tr<BF16>::mma(sl < 8 ? bf0[ct] : bf1[ct], af[sl & 3], acc[sl & 7][ct]);
                __builtin_amdgcn_sched_barrier(0);              // the slot order IS the schedule
            }
            pa = qa; pb = qb;
            st ^= 1;
        };
        {
            using T_ = std::integral_constant<bool, true>;
            using F_ = std::integral_constant<bool, false>;
            int t = t_beg;
            for (; t + 2 < t_end; ++t) kstep(t, T_{}, T_{});
            if (t + 1 < t_end) { kstep(t, T_{}, F_{}); ++t; }
            if (t < t_end) kstep(t, F_{}, F_{});
        }

        // ---- epilogue: lane (r16, lg) holds C[m = 128 wm + 16 rt + r16][n = 64 wn + 16 ct + 4 lg + r], r = 0..3
        const int64_t gi0 = (int64_t)BT * mi + 128 * wm + r16;
        const int gj0 = BT * ni + 64 * wn + 4 * lg;
        if (EPI == EPI_OUT || EPI == EPI_OUT_TD || EPI == EPI_OUT_S || EPI == EPI_OUT_TD_S) {
            if (EPI == EPI_OUT_S || EPI == EPI_OUT_TD_S) {
                // g is stored unscaled: coef / Tc and the gradient arriving at the loss meet the float32 sums here
                float osc = p.coef * nce_dev_inv_temp(p.temp, p.min_temp);
                if (p.upstream) osc *= p.upstream[0];
#pragma unroll
                for (int rt = 0; rt < 8; ++rt)
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) acc[rt][ct] *= osc;
            }
            float* o = reinterpret_cast<float*>(p.out) + (int64_t)split * p.slab_stride;
            unsigned short* ob = reinterpret_cast<unsigned short*>(p.out);
#pragma unroll
            for (int rt = 0; rt < 8; ++rt) {
                const int64_t i = gi0 + 16 * rt;
                if (i < p.m_valid) {
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) {
                        const int j = gj0 + 16 * ct;
                        if (j < p.n_valid) {
                            if (p.out_bf16)
                                *reinterpret_cast<u32x2*>(ob + i * p.ldo + j) =
                                    u32x2{pack_bf16x2(acc[rt][ct][0], acc[rt][ct][1]), pack_bf16x2(acc[rt][ct][2], acc[rt][ct][3])};
                            else *reinterpret_cast<f32x4*>(o + i * p.ldo + j) = acc[rt][ct];
                        }
                    }
                }
            }
            if (EPI == EPI_OUT_TD || EPI == EPI_OUT_TD_S) {
                float td = 0.f;
#pragma unroll
                for (int rt = 0; rt < 8; ++rt) {
                    const int64_t i = gi0 + 16 * rt;
                    if (i < p.m_valid) {
#pragma unroll
                        for (int ct = 0; ct < 4; ++ct) {
                            const int j = gj0 + 16 * ct;
                            if (j < p.n_valid) {
                                const u32x2 x = *reinterpret_cast<const u32x2*>(p.tdot_src + i * p.ldo + j);
                                td = fmaf(acc[rt][ct][0], __uint_as_float(x[0] << 16), td);
                                td = fmaf(acc[rt][ct][1], __uint_as_float(x[0] & 0xffff0000u), td);
                                td = fmaf(acc[rt][ct][2], __uint_as_float(x[1] << 16), td);
                                td = fmaf(acc[rt][ct][3], __uint_as_float(x[1] & 0xffff0000u), td);
                            }
                        }
                    }
                }
                td = reduce_wave(td);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();                   // every wave is past its last read of the stages
                float* red = reinterpret_cast<float*>(smem);
                if (lane == 0) red[w] = td;
                __syncthreads();
                if (threadIdx.x == 0)
                    p.tdot_part[((int64_t)split * p.m_tiles + mi) * p.n_tiles + ni] =
                        ((red[0] + red[1]) + (red[2] + red[3])) + ((red[4] + red[5]) + (red[6] + red[7]));
            }
        } else if (EPI == EPI_SIG) {
            // n = l log2(e) straight from the accumulator: l = acc / Tc + bias is never formed
            const float s2 = nce_dev_inv_temp(p.temp, p.min_temp) * 1.4426950408889634f, b2 = p.bias[0] * 1.4426950408889634f;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();                       // every wave is past its last read of the stages
            float* lsp = reinterpret_cast<float*>(smem);        // [4][256] softplus sums | [4][256] g sums
            float* lsg = lsp + 4 * BT;
            // block-uniform: only tiles on the band of positives or on the ragged edge pay for the selects
            const int64_t p0 = p.row_offset + (int64_t)BT * mi;
            const bool special = BT * (mi + 1) > p.m_valid || BT * (ni + 1) > p.n_valid ||
                                 (p0 < (int64_t)BT * (ni + 1) && p0 + BT > (int64_t)BT * ni);
            unsigned short* gtile = p.e + ((int64_t)mi * p.e_tiles + 4 * ni + wn) * (BT * 64) + (128 * wm + r16) * 64 + 4 * lg;
            float rsp[8], rsg[8];
            auto rows8 = [&](auto special_c) {
                constexpr bool SP = decltype(special_c)::value;
#pragma unroll
                for (int rt = 0; rt < 8; ++rt) {
                    const int64_t i = gi0 + 16 * rt;
                    const bool iok = i < p.m_valid;
                    const int64_t jp = p.row_offset + i;
                    f32x2 sl = f32x2{0.f, 0.f}, sc = f32x2{0.f, 0.f}, sg = f32x2{0.f, 0.f};
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) {
                        const int j = gj0 + 16 * ct;
                        f32x2 g[2];
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const f32x2 n = f32x2{acc[rt][ct][2 * h], acc[rt][ct][2 * h + 1]} * f32x2{s2, s2} + f32x2{b2, b2};
                            SigTerms x = sig_terms(n);
                            if (SP) {
                                // the positive: softplus(-l) and -sigmoid(-l), formed from -n (not as differences)
                                const SigTerms y = sig_terms(-n);
#pragma unroll
                                for (int k = 0; k < 2; ++k) {
                                    const int col = j + 2 * h + k;
                                    const bool pos = col == jp, ok = iok && col < p.n_valid;
                                    x.sig[k] = ok ? (pos ? -y.sig[k] : x.sig[k]) : 0.f;
                                    x.lg2[k] = ok ? (pos ? y.lg2[k] : x.lg2[k]) : 0.f;
                                    x.corr[k] = ok ? (pos ? y.corr[k] : x.corr[k]) : 0.f;
                                }
                            }
                            sl += x.lg2; sc += x.corr; sg += x.sig;
                            g[h] = x.sig;
                        }
                        // tile (mi, 4 ni + wn) of g: row 128 wm + 16 rt + r16, columns 16 ct + 4 lg .. + 3 of its 64
                        *reinterpret_cast<u32x2*>(gtile + (16 * rt) * 64 + 16 * ct) = u32x2{pack_bf16x2(g[0][0], g[0][1]), pack_bf16x2(g[1][0], g[1][1])};
                    }
                    rsp[rt] = reduce_lg(fmaf(sl[0] + sl[1], 0.6931471805599453f, sc[0] + sc[1]));     // over the wave's 64 columns
                    rsg[rt] = reduce_lg(sg[0] + sg[1]);
                }
            };
            if (special) rows8(std::integral_constant<bool, true>{});
            else rows8(std::integral_constant<bool, false>{});
            if (lg == 0) {
#pragma unroll
                for (int rt = 0; rt < 8; ++rt) {
                    lsp[wn * BT + 128 * wm + 16 * rt + r16] = rsp[rt];
                    lsg[wn * BT + 128 * wm + 16 * rt + r16] = rsg[rt];
                }
            }
            __syncthreads();
            const int tdx = threadIdx.x & (BT - 1);
            const float* src = threadIdx.x < BT ? lsp : lsg;
            (threadIdx.x < BT ? p.sp_part : p.sg_part)[((int64_t)ni * p.m_tiles + mi) * BT + tdx] =
                (src[tdx] + src[BT + tdx]) + (src[2 * BT + tdx] + src[3 * BT + tdx]);
        } else if (EPI == EPI_RANK) {
            // row thresholds first (their latency passes while the other waves arrive); padding re-reads the last one
            const bool cols_on = p.pos_col != nullptr;                  // block-uniform
            float pr[8];
#pragma unroll
            for (int rt = 0; rt < 8; ++rt) {
                const int64_t i = gi0 + 16 * rt;
                pr[rt] = p.pos_row[i < p.m_valid ? i : p.m_valid - 1];
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();                       // every wave is past its last read of the stages
            int* lrow = reinterpret_cast<int*>(smem);           // [4][256] row counts | [2][256] column counts
            int* lcol = lrow + 4 * BT;
            // block-uniform: only tiles on the band of positives or on the ragged edge pay for the selects
            const int64_t p0 = p.row_offset + (int64_t)BT * mi;
            const bool special = BT * (mi + 1) > p.m_valid || BT * (ni + 1) > p.n_valid ||
                                 (p0 < (int64_t)BT * (ni + 1) && p0 + BT > (int64_t)BT * ni);
            // the accumulator of (rt, ct, r); SP: the positive and the padding become a NaN -- one select, and every comparison
            // with it is false.  The empty asm keeps the value opaque: comparisons that the variants below have in common would
            // otherwise be hoisted in front of the branch, hundreds of masks at once, and spill.
            auto elem = [&](auto special_c, int rt, int ct, int r) -> float {
                constexpr bool SP = decltype(special_c)::value;
                float sv = acc[rt][ct][r];
                asm volatile("" : "+v"(sv));
                if (SP) {
                    const int64_t i = gi0 + 16 * rt;
                    const int col = gj0 + 16 * ct + r;
                    sv = ((i < p.m_valid) & (col < p.n_valid) & (col != p.row_offset + i)) ? sv : __builtin_nanf("");
                }
                return sv;
            };
            // rows: greater | equal << 16 over the wave's 64 columns (<= 64 in either half), then over the 4 lane groups
            auto count_rows = [&](auto special_c) {
#pragma unroll
                for (int rt = 0; rt < 8; ++rt) {
                    int rg = 0, re = 0;
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float sv = elem(special_c, rt, ct, r);
                            rg += (int)(sv > pr[rt]);
                            re += (int)(sv == pr[rt]);
                        }
                    }
                    int v = rg | (re << 16);
                    v += __shfl_xor(v, 16, 64);
                    v += __shfl_xor(v, 32, 64);
                    if (lg == 0) lrow[wn * BT + 128 * wm + 16 * rt + r16] = v;
                }
            };
            // columns: the same over the wave's 128 rows (<= 128 in either half), then over the 16 lanes of a group
            auto count_cols = [&](auto special_c) {
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) {
                    float pc[4];
                    int cg[4], ce[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int j = gj0 + 16 * ct + r;
                        pc[r] = p.pos_col[j < p.n_valid ? j : p.n_valid - 1];
                        cg[r] = ce[r] = 0;
                    }
#pragma unroll
                    for (int rt = 0; rt < 8; ++rt) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float sv = elem(special_c, rt, ct, r);
                            cg[r] += (int)(sv > pc[r]);
                            ce[r] += (int)(sv == pc[r]);
                        }
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        int v = cg[r] | (ce[r] << 16);
                        v += __shfl_xor(v, 1, 64);
                        v += __shfl_xor(v, 2, 64);
                        v += __shfl_xor(v, 4, 64);
                        v += __shfl_xor(v, 8, 64);
                        if (r16 == 0) lcol[wm * BT + 64 * wn + 16 * ct + 4 * lg + r] = v;
                    }
                }
            };
            using T_ = std::integral_constant<bool, true>;
            using F_ = std::integral_constant<bool, false>;
            if (special) {
                count_rows(T_{});
                if (cols_on) count_cols(T_{});
            } else {
                count_rows(F_{});
                if (cols_on) count_cols(F_{});
            }
            __syncthreads();
            const int tdx = threadIdx.x;
            if (tdx < BT) {
                p.rank_row_part[((int64_t)ni * p.m_tiles + mi) * BT + tdx] = (lrow[tdx] + lrow[BT + tdx]) + (lrow[2 * BT + tdx] + lrow[3 * BT + tdx]);
            } else if (cols_on) {
                const int c = tdx - BT;
                p.rank_col_part[((int64_t)mi * p.n_tiles + ni) * BT + c] = lcol[c] + lcol[BT + c];
            }
        } else if (EPI == EPI_TOPK) {
            typedef unsigned long long u64;
            const int kk = p.topk;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();                       // every wave is past its last read of the stages
            u64* lst = reinterpret_cast<u64*>(smem);            // [4 wn][16 slots][256 rows] keys: the 128 KB of the stages
            // block-uniform: only tiles holding an excluded partner or a ragged edge pay for the selects
            const int64_t p0 = p.row_offset + (int64_t)BT * mi;
            const bool special = BT * (mi + 1) > p.m_valid || BT * (ni + 1) > p.n_valid ||
                                 (p0 < (int64_t)BT * (ni + 1) && p0 + BT > (int64_t)BT * ni);
            const unsigned int inv0 = ~(unsigned)gj0;           // inverted column of (ct, r): inv0 - (16 ct + r)
            auto rows8 = [&](auto special_c) {
                constexpr bool SP = decltype(special_c)::value;
#pragma unroll
                for (int rt = 0; rt < 8; ++rt) {
                    const int64_t i = gi0 + 16 * rt;
                    u64 K[16];
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            float sv = acc[rt][ct][r];
                            asm volatile("" : "+v"(sv));        // (opaque: keeps the two variants' common work behind the branch)
                            sv += 0.f;                          // -0 -> +0: equal scores have one image
                            const unsigned int b = __float_as_uint(sv);
                            unsigned int u = b ^ ((unsigned)((int)b >> 31) | 0x80000000u);
                            u = sv != sv ? 1u : u;
                            u64 key = ((u64)u << 32) | (u64)(inv0 - (unsigned)(16 * ct + r));
                            if (SP) {
                                const int col = gj0 + 16 * ct + r;
                                key = ((i < p.m_valid) & (col < p.n_valid) & (col != p.row_offset + i)) ? key : 0ull;
                            }
                            K[4 * ct + r] = key;
                        }
                    }
                    // the lane's 16 keys, best first: Batcher's merge exchange, 63 compare-exchanges
#define TOPK_CE(x_, y_)                                                                                                 \
    do {                                                                                                                \
        const u64 hi_ = K[x_] > K[y_] ? K[x_] : K[y_], lo_ = K[x_] > K[y_] ? K[y_] : K[x_];                             \
        K[x_] = hi_; K[y_] = lo_;                                                                                       \
    } while (0)
                    TOPK_CE(0, 1); TOPK_CE(2, 3); TOPK_CE(4, 5); TOPK_CE(6, 7); TOPK_CE(8, 9); TOPK_CE(10, 11); TOPK_CE(12, 13); TOPK_CE(14, 15);
                    TOPK_CE(0, 2); TOPK_CE(1, 3); TOPK_CE(4, 6); TOPK_CE(5, 7); TOPK_CE(8, 10); TOPK_CE(9, 11); TOPK_CE(12, 14); TOPK_CE(13, 15);
                    TOPK_CE(1, 2); TOPK_CE(5, 6); TOPK_CE(9, 10); TOPK_CE(13, 14);
                    TOPK_CE(0, 4); TOPK_CE(1, 5); TOPK_CE(2, 6); TOPK_CE(3, 7); TOPK_CE(8, 12); TOPK_CE(9, 13); TOPK_CE(10, 14); TOPK_CE(11, 15);
                    TOPK_CE(2, 4); TOPK_CE(3, 5); TOPK_CE(10, 12); TOPK_CE(11, 13);
                    TOPK_CE(1, 2); TOPK_CE(3, 4); TOPK_CE(5, 6); TOPK_CE(9, 10); TOPK_CE(11, 12); TOPK_CE(13, 14);
                    TOPK_CE(0, 8); TOPK_CE(1, 9); TOPK_CE(2, 10); TOPK_CE(3, 11); TOPK_CE(4, 12); TOPK_CE(5, 13); TOPK_CE(6, 14); TOPK_CE(7, 15);
                    TOPK_CE(4, 8); TOPK_CE(5, 9); TOPK_CE(6, 10); TOPK_CE(7, 11);
                    TOPK_CE(2, 4); TOPK_CE(3, 5); TOPK_CE(6, 8); TOPK_CE(7, 9); TOPK_CE(10, 12); TOPK_CE(11, 13);
                    TOPK_CE(1, 2); TOPK_CE(3, 4); TOPK_CE(5, 6); TOPK_CE(7, 8); TOPK_CE(9, 10); TOPK_CE(11, 12); TOPK_CE(13, 14);
#undef TOPK_CE
                    // the wave's 64 columns of the row lie in 4 lane groups: pop the largest of the 4 heads k times
                    u64* dst = lst + (wn * 16) * BT + 128 * wm + 16 * rt + r16;
                    for (int t = 0; t < kk; ++t) {
                        u64 win = K[0];
                        u64 o = __shfl_xor(win, 16, 64);
                        win = o > win ? o : win;
                        o = __shfl_xor(win, 32, 64);
                        win = o > win ? o : win;
                        if (lg == 0) dst[t * BT] = win;
                        const bool mine = K[0] == win;          // keys are distinct (only sentinels repeat)
#pragma unroll
                        for (int j = 0; j < 15; ++j) K[j] = mine ? K[j + 1] : K[j];
                        K[15] = mine ? 0ull : K[15];
                    }
                }
            };
            if (special) rows8(std::integral_constant<bool, true>{});
            else rows8(std::integral_constant<bool, false>{});
            __syncthreads();
            if (threadIdx.x < BT) {
                // one thread per row: the 4 waves' sorted lists into the tile's list
                const u64* l0 = lst + threadIdx.x;
                u64* out = p.topk_part + (((int64_t)ni * p.m_tiles + mi) * BT + threadIdx.x) * p.topk_kp;
                u64 h[4];
                int c[4];
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) { h[q4] = l0[(q4 * 16) * BT]; c[q4] = 0; }
                for (int t = 0; t < kk; ++t) {
                    const u64 h01 = h[0] > h[1] ? h[0] : h[1], h23 = h[2] > h[3] ? h[2] : h[3];
                    const u64 best = h01 > h23 ? h01 : h23;
                    out[t] = best;
#pragma unroll
                    for (int q4 = 0; q4 < 4; ++q4) {
                        const bool won = h[q4] == best;
                        c[q4] += (int)won;
                        const bool more = c[q4] < kk;
                        const u64 nx = l0[(q4 * 16 + (more ? c[q4] : 0)) * BT];
                        h[q4] = won ? (more ? nx : 0ull) : h[q4];
                    }
                }
            }
        } else {
            float scale2 = p.scale2, shift2 = p.shift2;
            // EPI_SUP: the labels of the lane's 8 rows and 16 columns are read here (their latency passes behind the exponentials)
            // and kept as 32-bit keys: equal classes have equal keys; a row that can match nothing (unlabeled or padding, which
            // re-reads the last label) gets a key no column has, and the other way round.  24 registers beside the accumulators
            // where the int64 labels would take 48 and spill.
            unsigned int kr[8], kc[16];
            if (epi_has_labels(EPI)) {
#pragma unroll
                for (int rt = 0; rt < 8; ++rt) {
                    const int i = (int)gi0 + 16 * rt;
                    const bool iok = i < p.m_valid;
                    const long long l = sup_label_at(p.lab_row, iok ? i : p.m_valid - 1);
                    kr[rt] = (iok && l >= 0) ? sup_label_key(l) : 0xffffffffu;
                }
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    const int j = gj0 + 16 * (c >> 2) + (c & 3);
                    const bool jok = j < p.n_valid;
                    const long long l = sup_label_at(p.lab_col, jok ? j : p.n_valid - 1);
                    kc[c] = (jok && l >= 0) ? sup_label_key(l) : 0xfffffffeu;
                }
            }
            // EPI_SETS_*: thread t < 256 reads the word of the block's row t, thread 256 + t that of its column t (the padding: the
            // empty set); they go to LDS behind the barrier
            unsigned long long my_set = 0ull;
            if (epi_has_sets(EPI)) {
                const int t = threadIdx.x & (BT - 1);
                const bool is_row = threadIdx.x < BT;
                const int k = BT * (is_row ? mi : ni) + t;
                const unsigned long long* src = reinterpret_cast<const unsigned long long*>(is_row ? p.lab_row : p.lab_col);
                if (k < (is_row ? p.m_valid : p.n_valid)) my_set = src[k];
            }
            if (EPI == EPI_EXP_DT || epi_has_labels(EPI) || epi_has_sets(EPI) || EPI == EPI_EXP_SELF) {
                scale2 = nce_dev_inv_temp(p.temp, p.min_temp) * 1.4426950408889634f;
                shift2 = scale2;
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();                       // every wave is past its last read of the stages
            if (epi_has_sets(EPI))                              // [256] row words | [256] column words, behind the 18 float planes
                reinterpret_cast<unsigned long long*>(smem + 18 * BT * 4)[threadIdx.x] = my_set;
            // E = exp2(acc scale - shift): 4 consecutive columns per lane, 8-byte stores (16 rows x 32 B per wave-instruction).
            // The sums run as packed float32 adds (both halves from their own registers); masking only on edge tiles.
            float rs[8];
            f32x2 cs2[4][2];
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) cs2[ct][0] = cs2[ct][1] = f32x2{0.f, 0.f};
            float* lrs = reinterpret_cast<float*>(smem);        // [4][256] row sums | [2][256] column sums
            float* lcs = lrs + 4 * BT;
            bool edge = BT * (mi + 1) > p.m_valid || BT * (ni + 1) > p.n_valid;            // block-uniform
            if (epi_is_self(EPI)) {
                // the band of excluded keys (column row_offset + i of row i) crosses this tile: it takes the branch of the ragged
                // edge, so only the tiles that hold such an element pay for the index test
                const int64_t p0 = p.row_offset + (int64_t)BT * mi;
                edge = edge || (p0 < (int64_t)BT * (ni + 1) && p0 + BT > (int64_t)BT * ni);
            }
            unsigned short* etile = p.e + ((int64_t)mi * p.e_tiles + 4 * ni + wn) * (BT * 64) + (128 * wm + r16) * 64 + 4 * lg;
#pragma unroll
            for (int rt = 0; rt < 8; ++rt) {
                const int64_t i = gi0 + 16 * rt;
                f32x2 s2 = f32x2{0.f, 0.f};
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) {
                    const int j = gj0 + 16 * ct;
                    f32x2 e01, e23;
                    e01[0] = __builtin_amdgcn_exp2f(acc[rt][ct][0] * scale2 - shift2);
                    e01[1] = __builtin_amdgcn_exp2f(acc[rt][ct][1] * scale2 - shift2);
                    e23[0] = __builtin_amdgcn_exp2f(acc[rt][ct][2] * scale2 - shift2);
                    e23[1] = __builtin_amdgcn_exp2f(acc[rt][ct][3] * scale2 - shift2);
                    if (edge) {
                        const bool iok = i < p.m_valid;
                        // EPI_EXP_SELF: the excluded key by its index (a row that exists has row_offset + i < n_valid < 2^31; unsigned,
                        // so that the padding rows past it wrap instead of overflowing)
                        const unsigned int js = epi_is_self(EPI) ? (unsigned)p.row_offset + (unsigned)i : 0u;
                        e01[0] = (iok && j + 0 < p.n_valid && (!epi_is_self(EPI) || (unsigned)j + 0u != js)) ? e01[0] : 0.f;
                        e01[1] = (iok && j + 1 < p.n_valid && (!epi_is_self(EPI) || (unsigned)j + 1u != js)) ? e01[1] : 0.f;
                        e23[0] = (iok && j + 2 < p.n_valid && (!epi_is_self(EPI) || (unsigned)j + 2u != js)) ? e23[0] : 0.f;
                        e23[1] = (iok && j + 3 < p.n_valid && (!epi_is_self(EPI) || (unsigned)j + 3u != js)) ? e23[1] : 0.f;
                    }
                    s2 += e01 + e23;
                    if (!epi_is_self(EPI)) {
                        cs2[ct][0] += e01;
                        cs2[ct][1] += e23;
                    }
                    // tile (mi, 4 ni + wn) of E: row 128 wm + 16 rt + r16, columns 16 ct + 4 lg .. + 3 of its 64 -- the four
                    // stores of a row group fill whole 128-byte lines of one 32 KB tile
                    *reinterpret_cast<u32x2*>(etile + (16 * rt) * 64 + 16 * ct) = u32x2{pack_bf16x2(e01[0], e01[1]), pack_bf16x2(e23[0], e23[1])};
                }
                rs[rt] = reduce_lg(s2[0] + s2[1]);              // over the wave's 64 columns
            }
            float cs[4][4];
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) { cs[ct][0] = cs2[ct][0][0]; cs[ct][1] = cs2[ct][0][1]; cs[ct][2] = cs2[ct][1][0]; cs[ct][3] = cs2[ct][1][1]; }
            if (lg == 0) {
#pragma unroll
                for (int rt = 0; rt < 8; ++rt) lrs[wn * BT + 128 * wm + 16 * rt + r16] = rs[rt];
            }
            if (!epi_is_self(EPI)) {
#pragma unroll
                for (int ct = 0; ct < 4; ++ct)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float v = reduce_r16(cs[ct][r]);  // over the wave's 128 rows
                        if (r16 == 0) lcs[wm * BT + 64 * wn + 16 * ct + 4 * lg + r] = v;
                    }
            }
            float* lrn = lcs + 2 * BT;                          // EPI_SUP: [4][256] row counts | [4][256] row sums |
            float* lrx = lrn + 4 * BT;                          //          [2][256] column counts | [2][256] column sums
            float* lcn = lrx + 4 * BT;
            float* lcx = lcn + 2 * BT;
            if (epi_has_labels(EPI)) {
                constexpr bool COLS = EPI == EPI_SUP;           // EPI_SUP_SELF: the row half alone
                // block-uniform: only tiles on the band of partners or on the ragged edge pay for the index tests
                const int64_t p0 = p.row_offset + (int64_t)BT * mi;
                const bool special = edge || (p0 < (int64_t)BT * (ni + 1) && p0 + BT > (int64_t)BT * ni);
                auto label_stats = [&](auto special_c) {
                    constexpr bool SP = decltype(special_c)::value;
                    // Matches are sparse, so the tile is first searched with the 32-bit keys: two VALU operations per element and
                    // no compare mask.  Only a row group (rt) with a key hit somewhere in the wave reads its int64 labels again
                    // (from L1 / L2) and forms the 64-bit matches and the sums -- a vote that changes no bit: a group without a
                    // match would have summed zeros.
                    // the column sums gather in LDS, in the slots of the lanes that own them (r16 == 0: one lane per column and
                    // wave), row group after row group: 32 accumulators less beside the 128 of the tile
                    float* wcn = lcn + wm * BT + 64 * wn + 4 * lg;
                    float* wcx = lcx + wm * BT + 64 * wn + 4 * lg;
                    if (COLS && r16 == 0) {
#pragma unroll
                        for (int c = 0; c < 16; ++c) wcn[16 * (c >> 2) + (c & 3)] = wcx[16 * (c >> 2) + (c & 3)] = 0.f;
                    }
#pragma unroll
                    for (int rt = 0; rt < 8; ++rt) {
                        unsigned int nearest = 0xffffffffu;
#pragma unroll
                        for (int c = 0; c < 16; ++c) {
                            const unsigned int x = kr[rt] ^ kc[c];
                            nearest = x < nearest ? x : nearest;
                        }
                        float rn = 0.f, rx = 0.f;
                        if (__any(nearest == 0u)) {
                            // (opaque: nothing this rare branch needs -- indices, addresses, the labels themselves -- may be
                            // formed in front of it or kept from the reads in front of the exponentials: it would sit in scratch)
                            int i = (int)gi0 + 16 * rt, gj = gj0;
                            const long long* lab_row = p.lab_row;
                            const long long* lab_col = p.lab_col;
                            asm volatile("" : "+v"(i), "+v"(gj), "+s"(lab_row), "+s"(lab_col));
                            const long long lr = sup_label_at(lab_row, i < p.m_valid ? i : p.m_valid - 1);
                            // SP: the partner counts by index, not here; its column relative to gj (-1: not in this lane's 64)
                            const int64_t rel = p.row_offset + i - gj;
                            const int jpr = (rel >= 0 && rel < 64) ? (int)rel : -1;
#pragma unroll
                            for (int c = 0; c < 16; ++c) {
                                const int j = gj + 16 * (c >> 2) + (c & 3);
                                // (the keys carry the padding: an equal key is a row and a column that exist)
                                bool m = (kr[rt] == kc[c]) & sup_label_match(lr, sup_label_at(lab_col, j < p.n_valid ? j : p.n_valid - 1));
                                if (SP) m = m & (jpr != 16 * (c >> 2) + (c & 3));
                                const float one = m ? 1.f : 0.f, sv = m ? acc[rt][c >> 2][c & 3] : 0.f;
                                rn += one; rx += sv;
                                if (COLS) {
                                    const float c1 = reduce_r16(one), c2 = reduce_r16(sv);  // over the group's 16 rows
                                    if (r16 == 0) {
                                        wcn[16 * (c >> 2) + (c & 3)] += c1;
                                        wcx[16 * (c >> 2) + (c & 3)] += c2;
                                    }
                                }
                            }
                            rn = reduce_lg(rn);                 // over the wave's 64 columns
                            rx = reduce_lg(rx);
                        }
                        if (lg == 0) {
                            lrn[wn * BT + 128 * wm + 16 * rt + r16] = rn;
                            lrx[wn * BT + 128 * wm + 16 * rt + r16] = rx;
                        }
                    }
                };
                if (special) label_stats(std::integral_constant<bool, true>{});
                else label_stats(std::integral_constant<bool, false>{});
            }
            if (epi_is_sets(EPI)) {
                constexpr bool JAC = EPI == EPI_SETS_JAC;
                typedef unsigned long long u64;
                __syncthreads();                                // the staged words are in place
                const u64* lsr = reinterpret_cast<const u64*>(smem + 18 * BT * 4) + 128 * wm + r16;            // + 16 rt
                const u64* lsc = reinterpret_cast<const u64*>(smem + 18 * BT * 4) + BT + 64 * wn + 4 * lg;     // + 16 ct + r
                // block-uniform: only the tiles on the band of partners pay for the index test (the padding weighs 0 by its sets)
                const int64_t p0 = p.row_offset + (int64_t)BT * mi;
                const bool special = p0 < (int64_t)BT * (ni + 1) && p0 + BT > (int64_t)BT * ni;
                // the partner of the lane's row of group rt is its element 16 ct + r where rel == 16 (ct - rt) + r
                const int64_t rel64 = p.row_offset + gi0 - gj0;
                const int rel = (rel64 > -512 && rel64 < 512) ? (int)rel64 : -4096;
                auto set_stats = [&](auto special_c) {
                    constexpr bool SP = decltype(special_c)::value;
                    float rw[8], rx[8];
#pragma unroll
                    for (int rt = 0; rt < 8; ++rt) rw[rt] = rx[rt] = 0.f;
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) {
                        u64 B[4];
                        int pb[4];
                        float cw[4], cx[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            B[r] = lsc[16 * ct + r];
                            pb[r] = JAC ? __popcll(B[r]) : 0;
                            cw[r] = cx[r] = 0.f;
                        }
#pragma unroll
                        for (int rt = 0; rt < 8; ++rt) {
                            const u64 A = lsr[16 * rt];
                            const int pa = JAC ? __popcll(A) : 0;
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                float wt = set_weight<JAC>(A, B[r], pa, pb[r]);
                                if (SP) wt = rel == 16 * (ct - rt) + r ? 0.f : wt;
                                const float sv = acc[rt][ct][r];
                                rw[rt] += wt;
                                rx[rt] = fmaf(wt, sv, rx[rt]);
                                cw[r] += wt;
                                cx[r] = fmaf(wt, sv, cx[r]);
                            }
                        }
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float c1 = reduce_r16(cw[r]), c2 = reduce_r16(cx[r]);     // over the wave's 128 rows
                            if (r16 == 0) {
                                lcn[wm * BT + 64 * wn + 16 * ct + 4 * lg + r] = c1;
                                lcx[wm * BT + 64 * wn + 16 * ct + 4 * lg + r] = c2;
                            }
                        }
                    }
#pragma unroll
                    for (int rt = 0; rt < 8; ++rt) {
                        const float r1 = reduce_lg(rw[rt]), r2 = reduce_lg(rx[rt]);         // over the wave's 64 columns
                        if (lg == 0) {
                            lrn[wn * BT + 128 * wm + 16 * rt + r16] = r1;
                            lrx[wn * BT + 128 * wm + 16 * rt + r16] = r2;
                        }
                    }
                };
                if (special) set_stats(std::integral_constant<bool, true>{});
                else set_stats(std::integral_constant<bool, false>{});
            }
            if (epi_is_sets_self(EPI)) {
                // the ROW half of the sweep above, chain for chain (ct-major over the lane's 16 elements of a row, then the lane
                // groups): 16 row accumulators and the 4 column words of the group, no column accumulators and no LDS column slots
                constexpr bool JAC = EPI == EPI_SETS_JAC_SELF;
                typedef unsigned long long u64;
                __syncthreads();                                // the staged words are in place
                const u64* lsr = reinterpret_cast<const u64*>(smem + 18 * BT * 4) + 128 * wm + r16;            // + 16 rt
                const u64* lsc = reinterpret_cast<const u64*>(smem + 18 * BT * 4) + BT + 64 * wn + 4 * lg;     // + 16 ct + r
                // block-uniform: only the tiles the band of anchors crosses pay for the index test (the padding weighs 0 by its sets)
                const int64_t p0 = p.row_offset + (int64_t)BT * mi;
                const bool special = p0 < (int64_t)BT * (ni + 1) && p0 + BT > (int64_t)BT * ni;
                // the anchor of the lane's row of group rt is its element 16 ct + r where rel == 16 (ct - rt) + r: weight 0 by INDEX,
                // never by its set or its value (a bit-identical row with the same set elsewhere in the view is a positive)
                const int64_t rel64 = p.row_offset + gi0 - gj0;
                const int rel = (rel64 > -512 && rel64 < 512) ? (int)rel64 : -4096;
                auto set_row_stats = [&](auto special_c) {
                    constexpr bool SP = decltype(special_c)::value;
                    float rw[8], rx[8];
#pragma unroll
                    for (int rt = 0; rt < 8; ++rt) rw[rt] = rx[rt] = 0.f;
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) {
                        u64 B[4];
                        int pb[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            B[r] = lsc[16 * ct + r];
                            pb[r] = JAC ? __popcll(B[r]) : 0;
                        }
#pragma unroll
                        for (int rt = 0; rt < 8; ++rt) {
                            const u64 A = lsr[16 * rt];
                            const int pa = JAC ? __popcll(A) : 0;
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                float wt = set_weight<JAC>(A, B[r], pa, pb[r]);
                                if (SP) wt = rel == 16 * (ct - rt) + r ? 0.f : wt;
                                rw[rt] += wt;
                                rx[rt] = fmaf(wt, acc[rt][ct][r], rx[rt]);
                            }
                        }
                    }
#pragma unroll
                    for (int rt = 0; rt < 8; ++rt) {
                        const float r1 = reduce_lg(rw[rt]), r2 = reduce_lg(rx[rt]);         // over the wave's 64 columns
                        if (lg == 0) {
                            lrn[wn * BT + 128 * wm + 16 * rt + r16] = r1;
                            lrx[wn * BT + 128 * wm + 16 * rt + r16] = r2;
                        }
                    }
                };
                if (special) set_row_stats(std::integral_constant<bool, true>{});
                else set_row_stats(std::integral_constant<bool, false>{});
            }
            __syncthreads();
            const int tdx = threadIdx.x;
            if (tdx < BT) {
                const int64_t o = ((int64_t)ni * p.m_tiles + mi) * BT + tdx;
                p.rowsum_part[o] = (lrs[tdx] + lrs[BT + tdx]) + (lrs[2 * BT + tdx] + lrs[3 * BT + tdx]);
                if (epi_has_labels(EPI) || epi_has_sets(EPI)) {
                    p.rowcnt_part[o] = (lrn[tdx] + lrn[BT + tdx]) + (lrn[2 * BT + tdx] + lrn[3 * BT + tdx]);
                    p.rowsx_part[o] = (lrx[tdx] + lrx[BT + tdx]) + (lrx[2 * BT + tdx] + lrx[3 * BT + tdx]);
                }
            } else if (!epi_is_self(EPI)) {
                const int c = tdx - BT;
                const int64_t o = ((int64_t)mi * p.n_tiles + ni) * BT + c;
                p.colsum_part[o] = lcs[c] + lcs[BT + c];
                if (EPI == EPI_SUP || epi_is_sets(EPI)) {
                    p.colcnt_part[o] = lcn[c] + lcn[BT + c];
                    p.colsx_part[o] = lcx[c] + lcx[BT + c];
                }
            }
        }
    }
#undef NCE_PIECE
}

// ---- small kernels around the GEMMs ------------------------------------------------------------------------------------

// l[i] = sum over the column tiles' partials, c[j] = sum over the row tiles' (fixed order: four strided partial sums per
// element, added in order).  Block = 64 elements x 4 parts.
__global__ __launch_bounds__(256) void nce_sums_kernel(const float* rowsum_part, const float* colsum_part, int m_tiles, int n_tiles,
                                                       int64_t rows, int64_t cols, float* l, float* c) {
    __shared__ float red[4][64];
    const int e = threadIdx.x & 63, part = threadIdx.x >> 6;
    const int64_t Rp = (int64_t)m_tiles * BT;
    int64_t id = (int64_t)blockIdx.x * 64 + e;                  // Rp is a multiple of 64: a block is all rows or all columns
    const bool is_row = id < Rp;
    if (!is_row) id -= Rp;
    const float* src = is_row ? rowsum_part : colsum_part;
    const int nt = is_row ? n_tiles : m_tiles, other = is_row ? m_tiles : n_tiles;
    float s = 0.f;
    for (int t = part; t < nt; t += 4) s += src[((int64_t)t * other + id / BT) * BT + id % BT];
    red[part][e] = s;
    __syncthreads();
    if (part == 0) {
        const float v = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
        if (is_row) { if (id < rows) l[id] = v; }
        else if (id < cols && c) c[id] = v;
    }
}

struct NceFinArgs {
    const unsigned short* a;            // [rows, d]
    const unsigned short* b;            // [cols, d]
    const float* l;                     // [rows]   row sums of E
    const float* c;                     // [cols]   column sums of E, all ranks (sym)
    float* u;                           // [Rp]     1 / l (0 in the padding)
    float* v;                           // [Cp]     1 / c (0 in the padding / sym == 0)
    float* loss_rows;                   // [rows]
    float* ediag;                       // [rows]   exp((a_i.b_pos - 1)/T) in float32: the positive's exponential before rounding
    int64_t rows, cols, row_offset, Rp, Cp;
    int d, sym;
    float inv_temp;
    const float* ent;                   // entropy regulariser riding in this launch (n_ent == 0: off)
    float* d_ent;
    float* ent_loss;
    int64_t n_ent;
    float ent_target, ent_scale;
    const float* temp;                  // DT: inv_temp = 1 / max(*temp, min_temp)
    float min_temp;
};

// The two terms of a loss row, log(sum) + 1/T - s/T with s the positive's score (InfoNCE) or the mean of the positives' scores
// (supervised loss), with their roundings pinned: the row term takes s/T in one fused multiply-add, the column term subtracts the
// rounded product.  Written out so that both losses round alike whatever the compiler would contract: with no label shared the
// supervised loss has InfoNCE's bits.
__device__ __forceinline__ float nce_row_term(float sum, float inv_temp, float s) {
#pragma clang fp contract(off)
    return fmaf(-inv_temp, s, logf(sum) + inv_temp);
}
__device__ __forceinline__ float nce_col_term(float sum, float inv_temp, float s) {
#pragma clang fp contract(off)
    const float scaled = inv_temp * s;
    return (logf(sum) + inv_temp) - scaled;
}

// one wave per local row: u_i, the positive logit a_i.b_pos, loss_i = log l_i + 1/T - s_ii/T (+ log c_pos + 1/T - s_ii/T);
// the waves past the rows fill v; block 0 also carries CurriculumMasking.entropy_loss (ref aecf/AECFLayer.py:285-314)
template <bool DT>
__global__ __launch_bounds__(256) void nce_finalize_kernel(NceFinArgs p) {
    if (DT) p.inv_temp = nce_dev_inv_temp(p.temp, p.min_temp);
    const int lane = lane_id();
    const int64_t i = (int64_t)blockIdx.x * 4 + wave_id();
    if (i < p.rows) {
        const unsigned short* ap = p.a + i * p.d;
        const unsigned short* bp = p.b + (p.row_offset + i) * p.d;
        float dot = 0.f;
        for (int k = lane; k < p.d; k += 64) dot = fmaf(Tr<BF16>::to_f32(ap[k]), Tr<BF16>::to_f32(bp[k]), dot);
        dot = reduce_wave(dot);
        if (lane == 0) {
            const float li = p.l[i];
            p.u[i] = 1.0f / li;
            p.ediag[i] = __builtin_amdgcn_exp2f((dot - 1.0f) * p.inv_temp * 1.4426950408889634f);
            float loss = nce_row_term(li, p.inv_temp, dot);
            if (p.sym) loss += nce_col_term(p.c[p.row_offset + i], p.inv_temp, dot);
            p.loss_rows[i] = loss;
        }
    } else if (i < p.Rp) {
        if (lane == 0) p.u[i] = 0.f;
    }
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < p.Cp; j += (int64_t)gridDim.x * 256)
        p.v[j] = (p.sym && j < p.cols) ? 1.0f / p.c[j] : 0.f;
    if (blockIdx.x == 0 && p.n_ent > 0) entropy_rider(p.ent, p.n_ent, p.ent_target, p.ent_scale, p.d_ent, p.ent_loss);
}

// W = ct (E (u_i + v_j) - npos [j = off + i]) in place over the tiled E, 8 elements per thread.  The positive's weight is a
// small difference of O(1) terms (softmax weight minus one): it is formed from the float32 exponential, not from the bf16 one.
__device__ __forceinline__ void nce_weights_body(unsigned short* e, int64_t e_tiles, int64_t m_tiles, const float* u, const float* v,
                                                 const float* ediag, int64_t rows, int64_t row_offset, float ct, float npos,
                                                 const float* upstream) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;         // 16-byte chunk: 2048 per tile, 8 per tile row
    if (id >= m_tiles * e_tiles * 2048) return;
    const int64_t tile = id >> 11;
    const int within = (int)(id & 2047);
    const int64_t i = (tile / e_tiles) * BT + (within >> 3), j0 = (tile % e_tiles) * 64 + 8 * (within & 7);
    u32x4* ptr = reinterpret_cast<u32x4*>(e) + id;
    const u32x4 raw = *ptr;
    const float ui = u[i];
    const f32x4 v0 = *reinterpret_cast<const f32x4*>(v + j0), v1 = *reinterpret_cast<const f32x4*>(v + j0 + 4);
    float x[8];
    Tr<BF16>::unpack(raw, x);
    const float vv[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
    const int64_t jp = (i < rows) ? row_offset + i - j0 : -1;
    if (upstream) ct *= upstream[0];                           // d loss / d (this call's term): a device scalar, no host read
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        float wv = x[k] * (ui + vv[k]);
        if (jp == k) wv = ediag[i] * (ui + vv[k]) - npos;
        x[k] = ct * wv;
    }
    *ptr = Tr<BF16>::pack(x);
}

__global__ __launch_bounds__(256) void nce_weights_kernel(unsigned short* e, int64_t e_tiles, int64_t m_tiles, const float* u,
                                                          const float* v, const float* ediag, int64_t rows, int64_t row_offset,
                                                          float ct, float npos, const float* upstream) {
    nce_weights_body(e, e_tiles, m_tiles, u, v, ediag, rows, row_offset, ct, npos, upstream);
}

// ct = coef / max(*temp, min_temp), formed as the host forms coef * (1 / T)
__global__ __launch_bounds__(256) void nce_weights_dt_kernel(unsigned short* e, int64_t e_tiles, int64_t m_tiles, const float* u,
                                                             const float* v, const float* ediag, int64_t rows, int64_t row_offset,
                                                             float coef, float npos, const float* upstream, const float* temp,
                                                             float min_temp) {
    nce_weights_body(e, e_tiles, m_tiles, u, v, ediag, rows, row_offset, coef * nce_dev_inv_temp(temp, min_temp), npos, upstream);
}

// ---- supervised contrastive loss: the label-aware variants of the three kernels above ----------------------------------

// nce_sums_kernel over three quantities (blockIdx.y: 0 the sums of E, 1 the counts, 2 the sums of the matched accumulators):
// row_part [3][n_tiles][Rp] -> row_stats [3][Rp], col_part [3][m_tiles][Cp] -> col_stats [3][cols]; the same four strided
// partial sums per element, added in order
__global__ __launch_bounds__(256) void sup_sums_kernel(const float* row_part, const float* col_part, int m_tiles, int n_tiles,
                                                       int64_t rows, int64_t cols, float* row_stats, float* col_stats) {
    __shared__ float red[4][64];
    const int e = threadIdx.x & 63, part = threadIdx.x >> 6;
    const int64_t Rp = (int64_t)m_tiles * BT, Cp = (int64_t)n_tiles * BT;
    const int64_t q = blockIdx.y;
    int64_t id = (int64_t)blockIdx.x * 64 + e;                  // Rp is a multiple of 64: a block is all rows or all columns
    const bool is_row = id < Rp;
    if (!is_row) id -= Rp;
    const float* src = is_row ? row_part + q * n_tiles * Rp : col_part + q * m_tiles * Cp;
    const int nt = is_row ? n_tiles : m_tiles, other = is_row ? m_tiles : n_tiles;
    float s = 0.f;
    for (int t = part; t < nt; t += 4) s += src[((int64_t)t * other + id / BT) * BT + id % BT];
    red[part][e] = s;
    __syncthreads();
    if (part == 0) {
        const float v = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
        if (is_row) { if (id < rows) row_stats[q * Rp + id] = v; }
        else if (id < cols) col_stats[q * cols + id] = v;
    }
}

struct SupFinArgs {
    const unsigned short* a;            // [rows, d]
    const unsigned short* b;            // [cols, d]
    const float* row_stats;             // [3][Rp]    l | count | matched sum of this rank's rows
    const float* col_stats;             // [3][cols]  c | count | matched sum, all ranks
    float* u;                           // [Rp]  1 / l     (0 in the padding)
    float* rn;                          // [Rp]  1 / n
    float* v;                           // [Cp]  1 / c
    float* rnc;                         // [Cp]  1 / nc
    float* loss_rows;                   // [rows]
    float* ediag;                       // [rows]
    int64_t rows, cols, row_offset, Rp, Cp;
    int d;
    const float* temp;
    float min_temp;
};

// nce_finalize_kernel with the positives of the labels: one wave per local row.  The partner keeps its own float32 dot; n = 1 +
// count, the mean of the positives' raw scores is (dot + matched sum) / n in both directions, and 1 / Tc meets it once, in the
// expression InfoNCE has for its one positive (count == 0: its bits).
__global__ __launch_bounds__(256) void sup_finalize_kernel(SupFinArgs p) {
    const float inv_temp = nce_dev_inv_temp(p.temp, p.min_temp);
    const int lane = lane_id();
    const int64_t i = (int64_t)blockIdx.x * 4 + wave_id();
    if (i < p.rows) {
        const unsigned short* ap = p.a + i * p.d;
        const unsigned short* bp = p.b + (p.row_offset + i) * p.d;
        float dot = 0.f;
        for (int k = lane; k < p.d; k += 64) dot = fmaf(Tr<BF16>::to_f32(ap[k]), Tr<BF16>::to_f32(bp[k]), dot);
        dot = reduce_wave(dot);
        if (lane == 0) {
            const int64_t pc = p.row_offset + i;
            const float li = p.row_stats[i];
            p.u[i] = 1.0f / li;
            p.ediag[i] = __builtin_amdgcn_exp2f((dot - 1.0f) * inv_temp * 1.4426950408889634f);
            const float rni = 1.0f / (1.0f + p.row_stats[p.Rp + i]);
            p.rn[i] = rni;
            const float mean_r = (dot + p.row_stats[2 * p.Rp + i]) * rni;
            const float mean_c = (dot + p.col_stats[2 * p.cols + pc]) * (1.0f / (1.0f + p.col_stats[p.cols + pc]));
            p.loss_rows[i] = nce_row_term(li, inv_temp, mean_r) + nce_col_term(p.col_stats[pc], inv_temp, mean_c);
        }
    } else if (i < p.Rp) {
        if (lane == 0) { p.u[i] = 0.f; p.rn[i] = 0.f; }
    }
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < p.Cp; j += (int64_t)gridDim.x * 256) {
        p.v[j] = j < p.cols ? 1.0f / p.col_stats[j] : 0.f;
        p.rnc[j] = j < p.cols ? 1.0f / (1.0f + p.col_stats[p.cols + j]) : 0.f;
    }
}

// nce_weights_dt_kernel with the positives of the labels: W = ct (E (u_i + v_j) - m_ij (rn_i + rnc_j)) in place over the tiled E.
// m is formed again from the labels (1 row label and 8 column labels per thread; the column labels stay in L2).  The partner's
// weight is ediag_i (u_i + v_p) - (rn_i + rnc_p): with no label shared the subtrahend is exactly 2 and every element has the
// bits of nce_weights_dt_kernel.
// SELF (blocks Y and Z of the pooled loss): the element at column row_offset + i is the anchor itself -- no positive, its weight
// exactly ct * 0 (ediag is not read); the callers pass a vector of zeros for v and rnc, so that a chunk without a match has the
// bits of nce_weights_dt_kernel at v = 0 and a match is E u_i - rn_i.
template <bool SELF>
__global__ __launch_bounds__(256) void sup_weights_kernel(unsigned short* e, int64_t e_tiles, int64_t m_tiles, const float* u,
                                                          const float* v, const float* rn, const float* rnc, const float* ediag,
                                                          const long long* lab_row, const long long* lab_col, int64_t rows,
                                                          int64_t cols, int64_t row_offset, float coef, const float* upstream,
                                                          const float* temp, float min_temp) {
    float ct = coef * nce_dev_inv_temp(temp, min_temp);
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;         // 16-byte chunk: 2048 per tile, 8 per tile row
    if (id >= m_tiles * e_tiles * 2048) return;
    const int64_t tile = id >> 11;
    const int within = (int)(id & 2047);
    const int64_t i = (tile / e_tiles) * BT + (within >> 3), j0 = (tile % e_tiles) * 64 + 8 * (within & 7);
    u32x4* ptr = reinterpret_cast<u32x4*>(e) + id;
    const u32x4 raw = *ptr;
    const float ui = u[i];
    const f32x4 v0 = *reinterpret_cast<const f32x4*>(v + j0), v1 = *reinterpret_cast<const f32x4*>(v + j0 + 4);
    const bool iok = i < rows;
    const long long lr = lab_row[iok ? i : rows - 1];
    const int64_t jp = iok ? row_offset + i - j0 : -1;
    unsigned int mm = 0;                                        // bit k: element k is a positive (by label or the partner)
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int64_t j = j0 + k;
        const long long lck = lab_col[j < cols ? j : cols - 1];
        if (SELF) { if (iok && j < cols && sup_label_match(lr, lck) && jp != k) mm |= 1u << k; }
        else if (iok && j < cols && (sup_label_match(lr, lck) || jp == k)) mm |= 1u << k;
    }
    float x[8];
    Tr<BF16>::unpack(raw, x);
    const float vv[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
    float rni = 0.f, rc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (mm) {
        rni = rn[i];
        const f32x4 r0 = *reinterpret_cast<const f32x4*>(rnc + j0), r1 = *reinterpret_cast<const f32x4*>(rnc + j0 + 4);
        rc[0] = r0[0]; rc[1] = r0[1]; rc[2] = r0[2]; rc[3] = r0[3]; rc[4] = r1[0]; rc[5] = r1[1]; rc[6] = r1[2]; rc[7] = r1[3];
    }
    if (upstream) ct *= upstream[0];                           // d loss / d (this call's term): a device scalar, no host read
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        float wv = x[k] * (ui + vv[k]);
        if (jp == k) wv = SELF ? 0.f : ediag[i] * (ui + vv[k]) - (rni + rc[k]);
        else if ((mm >> k) & 1u) wv = x[k] * (ui + vv[k]) - (rni + rc[k]);
        x[k] = ct * wv;
    }
    *ptr = Tr<BF16>::pack(x);
}

// sup_weights_kernel with class sets: W = ct (E (u_i + v_j) - w_ij (rn_i + rnc_j)) in place over the tiled E, w formed again from
// the words (1 row word and 8 column words per 16-byte chunk; the column words stay in L2), the product w (rn + rnc) fused into
// the subtraction (one rounding).  The partner's weight is ediag_i (u_i + v_p) - (rn_i + rnc_p), w = 1 by index: with no set
// weight anywhere in its row and column the subtrahend is exactly 2; an element with w = 0 takes InfoNCE's expression.
// SELF (blocks Y and Z of the pooled multi-label loss): the element at column row_offset + i is the anchor itself -- w := 0 by index
// and E is stored as 0 there, so its weight is exactly ct * 0 (ediag is not read); the callers pass a vector of zeros for v and
// rnc, so that W = ct (E u_i - w_ij rn_i) and a chunk without a weight has the bits of nce_weights_dt_kernel at v = 0.
template <bool JAC, bool SELF>
__global__ __launch_bounds__(256) void set_weights_kernel(unsigned short* e, int64_t e_tiles, int64_t m_tiles, const float* u,
                                                          const float* v, const float* rn, const float* rnc, const float* ediag,
                                                          const unsigned long long* set_row, const unsigned long long* set_col,
                                                          int64_t rows, int64_t cols, int64_t row_offset, float coef,
                                                          const float* upstream, const float* temp, float min_temp) {
#pragma clang fp contract(off)
    float ct = coef * nce_dev_inv_temp(temp, min_temp);
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;         // 16-byte chunk: 2048 per tile, 8 per tile row
    if (id >= m_tiles * e_tiles * 2048) return;
    const int64_t tile = id >> 11;
    const int within = (int)(id & 2047);
    const int64_t i = (tile / e_tiles) * BT + (within >> 3), j0 = (tile % e_tiles) * 64 + 8 * (within & 7);
    u32x4* ptr = reinterpret_cast<u32x4*>(e) + id;
    const u32x4 raw = *ptr;
    const float ui = u[i];
    const f32x4 v0 = *reinterpret_cast<const f32x4*>(v + j0), v1 = *reinterpret_cast<const f32x4*>(v + j0 + 4);
    const bool iok = i < rows;
    const unsigned long long A = iok ? set_row[i] : 0ull;       // the padding: the empty set, weight 0
    const int pa = JAC ? __popcll(A) : 0;
    const int64_t jp = iok ? row_offset + i - j0 : -1;
    float wt[8];
    bool any = false;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int64_t j = j0 + k;
        const unsigned long long B = j < cols ? set_col[j] : 0ull;
        wt[k] = jp == k ? (SELF ? 0.f : 1.f) : set_weight<JAC>(A, B, pa, JAC ? __popcll(B) : 0);
        any = any || wt[k] != 0.f;
    }
    float x[8];
    Tr<BF16>::unpack(raw, x);
    const float vv[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
    float rni = 0.f, rc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (any) {
        rni = rn[i];
        const f32x4 r0 = *reinterpret_cast<const f32x4*>(rnc + j0), r1 = *reinterpret_cast<const f32x4*>(rnc + j0 + 4);
        rc[0] = r0[0]; rc[1] = r0[1]; rc[2] = r0[2]; rc[3] = r0[3]; rc[4] = r1[0]; rc[5] = r1[1]; rc[6] = r1[2]; rc[7] = r1[3];
    }
    if (upstream) ct *= upstream[0];                           // d loss / d (this call's term): a device scalar, no host read
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        float wv = x[k] * (ui + vv[k]);
        if (jp == k) wv = SELF ? 0.f : fmaf(ediag[i], ui + vv[k], -(rni + rc[k]));
        else if (wt[k] != 0.f) wv = fmaf(-wt[k], rni + rc[k], wv);
        x[k] = ct * wv;
    }
    *ptr = Tr<BF16>::pack(x);
}

// out[i] = sum_s slab[s][i], float4 (rounded once to bf16 when the caller wants the gradient in that dtype)
__global__ __launch_bounds__(256) void nce_slab_sum_kernel(const float* slabs, int splits, int64_t n4, int64_t stride, void* out,
                                                           int out_bf16) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= n4) return;
    f32x4 s = *reinterpret_cast<const f32x4*>(slabs + 4 * id);
    for (int k = 1; k < splits; ++k) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(slabs + (int64_t)k * stride + 4 * id);
        s[0] += t[0]; s[1] += t[1]; s[2] += t[2]; s[3] += t[3];
    }
    if (out_bf16) *reinterpret_cast<u32x2*>(reinterpret_cast<unsigned short*>(out) + 4 * id) = u32x2{pack_bf16x2(s[0], s[1]), pack_bf16x2(s[2], s[3])};
    else *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(out) + 4 * id) = s;
}

// ---- sigmoid loss: the reductions behind EPI_SIG -----------------------------------------------------------------------

// loss_rows[i] = sum over the n tiles of the softplus partials, gsum[i] = the same of the g partials (fixed order: four
// strided partial sums per row, added in order).  Block = 64 rows x 4 parts; both arrays are [n_tiles][Rp].
__global__ __launch_bounds__(256) void sig_rows_kernel(const float* sp_part, const float* sg_part, int n_tiles, int64_t Rp, int64_t rows,
                                                       float* loss_rows, float* gsum) {
    __shared__ float red[2][4][64];
    const int e = threadIdx.x & 63, part = threadIdx.x >> 6;
    const int64_t id = (int64_t)blockIdx.x * 64 + e;            // < Rp (a multiple of 64)
    float s = 0.f, g = 0.f;
    for (int t = part; t < n_tiles; t += 4) {
        s += sp_part[(int64_t)t * Rp + id];
        g += sg_part[(int64_t)t * Rp + id];
    }
    red[0][part][e] = s;
    red[1][part][e] = g;
    __syncthreads();
    if (part == 0) {
        if (id < rows) loss_rows[id] = (red[0][0][e] + red[0][1][e]) + (red[0][2][e] + red[0][3][e]);
        gsum[id] = (red[1][0][e] + red[1][1][e]) + (red[1][2][e] + red[1][3][e]);         // 0 in the padding
    }
}

// d_bias[0] = sum_i gsum[i]: 256 strided partial sums in order, then a fixed tree (one block)
__global__ __launch_bounds__(256) void sig_dbias_kernel(const float* gsum, int64_t n, float* d_bias) {
    __shared__ float red[256];
    float s = 0.f;
    for (int64_t k = threadIdx.x; k < n; k += 256) s += gsum[k];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) d_bias[0] = red[0];
}

template <int AM, int BM, int EPI, int MAP>
void launch_gemm(const NceGemmArgs& a, unsigned int blocks, hipStream_t s) {
    auto kern = nce_gemm_kernel<AM, BM, EPI, MAP>;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * STAGE);
    kern<<<dim3(blocks), dim3(512), 2 * STAGE, s>>>(a);
}

inline int64_t up256(int64_t v) { return (v + 255) / 256 * 256; }
inline size_t al256(size_t v) { return (v + 255) / 256 * 256; }

// workspace carve
struct NceWs {
    unsigned short* e;                  // [Rp][Cp] bf16
    float* rowsum_part;                 // [n_tiles][Rp]
    float* colsum_part;                 // [m_tiles][Cp]
    float* l;                           // [Rp]
    float* u;                           // [Rp]
    float* v;                           // [Cp]
    float* ediag;                       // [Rp]
    float* c_local;                     // [Cp]  column sums when the caller passes none
    float* slabs;                       // [splits][rows][d]
    size_t bytes;
};

int da_splits(int64_t Rp, int64_t Cp, int d) {
    const int64_t items = (Rp / BT) * ((d + BT - 1) / BT);
    int64_t s = (768 + items - 1) / items;              // about three blocks per CU ...
    const int64_t cap = Cp / 64 / 8;                    // ... of at least 8 K-steps each
    s = s > cap ? cap : s;
    if (s >= 5 && s <= 12 && cap >= 8) s = 8;          // one split per XCD (MAP_SPLITX)
    return (int)(s < 1 ? 1 : (s > 32 ? 32 : s));
}

NceWs carve(void* ws, int64_t rows, int64_t cols, int d) {
    const int64_t Rp = up256(rows), Cp = up256(cols);
    const int64_t mt = Rp / BT, nt = Cp / BT;
    NceWs w;
    char* p = (char*)ws;
    size_t off = 0;
    auto take = [&](size_t n) { char* r = p + off; off += al256(n); return r; };
    w.e = (unsigned short*)take((size_t)Rp * Cp * 2);
    w.rowsum_part = (float*)take((size_t)nt * Rp * 4);
    w.colsum_part = (float*)take((size_t)mt * Cp * 4);
    w.l = (float*)take((size_t)Rp * 4);
    w.u = (float*)take((size_t)Rp * 4);
    w.v = (float*)take((size_t)Cp * 4);
    w.ediag = (float*)take((size_t)Rp * 4);
    w.c_local = (float*)take((size_t)Cp * 4);
    w.slabs = (float*)take((size_t)da_splits(Rp, Cp, d) * rows * d * 4);
    w.bytes = off;
    return w;
}

// workspace carve of the sigmoid loss
struct SigWs {
    unsigned short* g;                  // [Rp][Cp] bf16, tiled as E
    float* sp_part;                     // [n_tiles][Rp]
    float* sg_part;                     // [n_tiles][Rp]
    float* gsum;                        // [Rp]
    float* tdot_part;                   // [splits <= 32][m_tiles][n_tiles_d <= 16]
    float* slabs;                       // [splits][rows][d]
    size_t bytes;
};

SigWs sig_carve(void* ws, int64_t rows, int64_t cols, int d) {
    const int64_t Rp = up256(rows), Cp = up256(cols);
    const int64_t mt = Rp / BT, nt = Cp / BT;
    SigWs w;
    char* p = (char*)ws;
    size_t off = 0;
    auto take = [&](size_t n) { char* r = p + off; off += al256(n); return r; };
    w.g = (unsigned short*)take((size_t)Rp * Cp * 2);
    w.sp_part = (float*)take((size_t)nt * Rp * 4);
    w.sg_part = (float*)take((size_t)nt * Rp * 4);
    w.gsum = (float*)take((size_t)Rp * 4);
    w.tdot_part = (float*)take((size_t)32 * 16 * mt * 4);
    w.slabs = (float*)take((size_t)da_splits(Rp, Cp, d) * rows * d * 4);
    w.bytes = off;
    return w;
}

// the logits arrangement: a [rows, d] . b [cols, d]^T as OP_ROW x OP_ROW operands over MAP_2D, and its block count; the
// caller adds its epilogue's fields
struct LogitsLaunch {
    NceGemmArgs g;
    unsigned int blocks;
};
LogitsLaunch logits_args(int64_t rows, int64_t cols, int d, const void* a, const void* b) {
    const int64_t Rp = up256(rows), Cp = up256(cols);
    LogitsLaunch o = {};
    NceGemmArgs& g = o.g;
    g.a = (const char*)a; g.b = (const char*)b; g.lda = g.ldb = 2u * (unsigned)d;
    g.a_sm = (int64_t)BT * g.lda; g.a_st = 128;
    g.a_rows = (int)rows; g.b_rows = (int)cols;
    g.m_tiles = (int)(Rp / BT); g.n_tiles = (int)(Cp / BT); g.k_steps = d / 64;
    g.splits = 1; g.steps_per_split = g.k_steps;
    g.m_valid = (int)rows; g.n_valid = (int)cols;
    const unsigned int nsm = (g.m_tiles + 3) / 4, nsn = (g.n_tiles + 7) / 8;
    o.blocks = ((nsm * nsn + 7) / 8) * 8 * 32;
    return o;
}

// da = W b (m = local rows, n = d, K = keys, split over K into slabs that are then summed) and db = W^T a (m = keys, n = d,
// K = local rows) over the tiled bf16 weights wt [Rp][Cp]; outputs float32 or -- one rounding of the float32 sums -- bf16.
// g0: the epilogue's scalar fields (coef / upstream / temp), everything else zero.  dt with d_t: dL/dT = -(1/T) sum_i a_i.da_i
// from per-block partials of the float32 da products (EPI_TD) in tdot_part [splits m_tiles n_tiles].
//
// The da product alone: its float32 slabs go to `slabs` [splits][rows][d]; with `direct` and no K split the GEMM stores its own
// output there (float32 or bf16) instead.  want_td: the EPI_TD instance, a's rows as tdot_src, partials into tdot_part.  Returns
// the number of slabs written (0: stored directly); the caller sums them and reduces the partials.
template <int EPI_PLAIN, int EPI_TD>
int launch_da_product(int64_t rows, int64_t cols, int d, const NceGemmArgs& g0, const unsigned short* wt, float* slabs, float* tdot_part,
                      bool want_td, const void* a, const void* b, int out_bf16, void* direct, hipStream_t s) {
    const int64_t Rp = up256(rows), Cp = up256(cols);
    const int n_tiles_d = (d + BT - 1) / BT;
    NceGemmArgs g = g0;
    g.a = (const char*)wt; g.lda = 128; g.a_rows = (int)Rp;           // tile (mi, t) of W: [256][128 B], contiguous
    g.a_sm = (Cp / 64) * (int64_t)32768; g.a_st = 32768;
    g.b = (const char*)b; g.ldb = 2u * (unsigned)d; g.b_rows = (int)cols; g.b_cbytes = 2 * d;
    g.m_tiles = (int)(Rp / BT); g.n_tiles = n_tiles_d; g.k_steps = (int)(Cp / 64);
    g.splits = da_splits(Rp, Cp, d);
    g.steps_per_split = (g.k_steps + g.splits - 1) / g.splits;
    g.m_valid = (int)rows; g.n_valid = d;
    const bool to_slabs = g.splits > 1 || !direct;
    g.out = to_slabs ? (void*)slabs : direct; g.ldo = d; g.slab_stride = rows * (int64_t)d;
    g.out_bf16 = to_slabs ? 0 : out_bf16;
    const unsigned int units = (unsigned)(g.m_tiles * g.splits);
    const unsigned int bx = 8u * g.m_tiles * g.n_tiles, bu = ((units + 7) / 8) * 8 * g.n_tiles;
    if (want_td) {
        g.tdot_src = (const unsigned short*)a; g.tdot_part = tdot_part;
        if (g.splits == 8) launch_gemm<OP_ROW, OP_COL, EPI_TD, MAP_SPLITX>(g, bx, s);
        else launch_gemm<OP_ROW, OP_COL, EPI_TD, MAP_UNITS>(g, bu, s);
    } else {
        if (g.splits == 8) launch_gemm<OP_ROW, OP_COL, EPI_PLAIN, MAP_SPLITX>(g, bx, s);
        else launch_gemm<OP_ROW, OP_COL, EPI_PLAIN, MAP_UNITS>(g, bu, s);
    }
    return to_slabs ? g.splits : 0;
}

// the partials one da product leaves in tdot_part
inline int64_t da_tdot_count(int64_t rows, int64_t cols, int d) {
    const int64_t Rp = up256(rows), Cp = up256(cols);
    return (int64_t)da_splits(Rp, Cp, d) * (Rp / BT) * ((d + BT - 1) / BT);
}

inline void launch_slab_sum(const float* slabs, int n_slabs, int64_t n, void* out, int out_bf16, hipStream_t s) {
    const int64_t n4 = n / 4;
    nce_slab_sum_kernel<<<dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s>>>(slabs, n_slabs, n4, n, out, out_bf16);
}

// The db product alone: db [cols][d] stored by the GEMM itself (no K split), float32 or bf16.
template <int EPI_PLAIN>
void launch_db_product(int64_t rows, int64_t cols, int d, const NceGemmArgs& g0, const unsigned short* wt, const void* a, int out_bf16,
                       void* db, hipStream_t s) {
    const int64_t Rp = up256(rows), Cp = up256(cols);
    NceGemmArgs g = g0;
    g.a = (const char*)wt; g.lda = 128; g.a_rows = (int)Rp; g.a_cbytes = 0; g.a_sm = Cp / 64;
    g.b = (const char*)a; g.ldb = 2u * (unsigned)d; g.b_rows = (int)rows; g.b_cbytes = 2 * d;
    g.m_tiles = (int)(Cp / BT); g.n_tiles = (d + BT - 1) / BT; g.k_steps = (int)(Rp / 64);
    g.splits = 1; g.steps_per_split = g.k_steps;
    g.m_valid = (int)cols; g.n_valid = d;
    g.out = db; g.ldo = d; g.slab_stride = 0; g.out_bf16 = out_bf16;
    const unsigned int units = (unsigned)g.m_tiles;
    launch_gemm<OP_COLB, OP_COL, EPI_PLAIN, MAP_UNITS>(g, ((units + 7) / 8) * 8 * g.n_tiles, s);
}

template <int EPI_PLAIN, int EPI_TD>
void launch_grad_products(int64_t rows, int64_t cols, int d, const NceGemmArgs& g0, const unsigned short* wt, float* slabs,
                          float* tdot_part, const NceDevTemp* dt, const void* a, const void* b, int out_bf16, void* da, void* db,
                          hipStream_t s) {
    const bool want_td = dt && dt->d_t;
    const int n_slabs = launch_da_product<EPI_PLAIN, EPI_TD>(rows, cols, d, g0, wt, slabs, tdot_part, want_td, a, b, out_bf16, da, s);
    if (n_slabs) launch_slab_sum(slabs, n_slabs, rows * (int64_t)d, da, out_bf16, s);
    if (want_td) launch_nce_dtemp(tdot_part, da_tdot_count(rows, cols, d), 1, *dt, s);
    launch_db_product<EPI_PLAIN>(rows, cols, d, g0, wt, a, out_bf16, db, s);
}

}  // namespace

bool nce_gemm_supported(int dtype, int d, float temperature) {
    // 1/T is the shift of every exponent: e^(-2/T) has to stay a normal float32 / bf16
    return dtype == 0 && d % 64 == 0 && d >= 64 && d <= 4096 && temperature >= 0.025f;
}

size_t nce_gemm_workspace_bytes(int64_t rows, int64_t cols, int d) { return carve(nullptr, rows, cols, d).bytes + 256; }

// pass 1: E, row sums (workspace) and this rank's column sums (col_sums, may be NULL when sym == 0)
void launch_nce_gemm_pass1(int64_t rows, int64_t cols, int d, float inv_temp, const void* a, const void* b, void* workspace,
                           float* col_sums, hipStream_t s, const NceDevTemp* dt) {
    const NceWs w = carve(workspace, rows, cols, d);
    const int64_t Rp = up256(rows), Cp = up256(cols);
    LogitsLaunch L = logits_args(rows, cols, d, a, b);
    NceGemmArgs& g = L.g;
    g.e = w.e; g.e_tiles = Cp / 64;
    g.scale2 = inv_temp * 1.4426950408889634f; g.shift2 = g.scale2;
    g.rowsum_part = w.rowsum_part; g.colsum_part = w.colsum_part;
    if (dt) {
        g.temp = dt->t; g.min_temp = dt->min_t;
        launch_gemm<OP_ROW, OP_ROW, EPI_EXP_DT, MAP_2D>(g, L.blocks, s);
    } else {
        launch_gemm<OP_ROW, OP_ROW, EPI_EXP, MAP_2D>(g, L.blocks, s);
    }
    nce_sums_kernel<<<dim3((unsigned)((Rp + Cp) / 64)), dim3(256), 0, s>>>(w.rowsum_part, w.colsum_part, g.m_tiles, g.n_tiles,
                                                                                   rows, cols, w.l, col_sums ? col_sums : w.c_local);
}

// normalisers + loss rows (col_sums: all ranks' sums when sym; NULL = pass 1's own) [+ the entropy regulariser riding along]
void launch_nce_gemm_loss(int64_t rows, int64_t cols, int64_t row_offset, int d, float inv_temp, int sym, const void* a,
                          const void* b, const float* col_sums, void* workspace, float* loss_rows, const float* ent, int64_t n_ent,
                          float ent_target, float ent_upstream, float* d_ent, float* ent_loss, hipStream_t s, const NceDevTemp* dt) {
    const NceWs w = carve(workspace, rows, cols, d);
    const int64_t Rp = up256(rows), Cp = up256(cols);
    NceFinArgs f = {};
    f.a = (const unsigned short*)a; f.b = (const unsigned short*)b; f.l = w.l; f.c = col_sums ? col_sums : w.c_local;
    f.u = w.u; f.v = w.v; f.ediag = w.ediag; f.loss_rows = loss_rows; f.rows = rows; f.cols = cols; f.row_offset = row_offset; f.Rp = Rp; f.Cp = Cp;
    f.d = d; f.sym = sym; f.inv_temp = inv_temp;
    f.ent = ent; f.d_ent = d_ent; f.ent_loss = ent_loss; f.n_ent = ent ? n_ent : 0; f.ent_target = ent_target;
    f.ent_scale = n_ent > 0 ? 2.0f * ent_upstream / (float)n_ent : 0.f;
    if (dt) {
        f.temp = dt->t; f.min_temp = dt->min_t;
        nce_finalize_kernel<true><<<dim3((unsigned)((Rp + 3) / 4)), dim3(256), 0, s>>>(f);
    } else {
        nce_finalize_kernel<false><<<dim3((unsigned)((Rp + 3) / 4)), dim3(256), 0, s>>>(f);
    }
}

// gradients: weights in place over E (scaled by the device scalar `upstream` when given), da = W b, db = W^T a; outputs float32
// or -- one rounding of the float32 sums -- bf16.  launch_nce_gemm_loss must have run on this workspace.
void launch_nce_gemm_grads(int64_t rows, int64_t cols, int64_t row_offset, int d, float inv_temp, float coef, int sym, const void* a,
                           const void* b, void* workspace, const float* upstream, int out_bf16, void* da, void* db, hipStream_t s,
                           const NceDevTemp* dt) {
    const NceWs w = carve(workspace, rows, cols, d);
    const int64_t Rp = up256(rows), Cp = up256(cols);
    const int64_t chunks = Rp * (Cp / 8);
    if (dt)
        nce_weights_dt_kernel<<<dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, s>>>(
            w.e, Cp / 64, Rp / BT, w.u, w.v, w.ediag, rows, row_offset, coef, sym ? 2.0f : 1.0f, upstream, dt->t, dt->min_t);
    else
        nce_weights_kernel<<<dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, s>>>(w.e, Cp / 64, Rp / BT, w.u, w.v, w.ediag, rows, row_offset,
                                                                                        coef * inv_temp, sym ? 2.0f : 1.0f, upstream);
    // the tdot partials go into the row-sum partials pass 1 left behind (dead since its sums launch; splits <= max(1, Cp / 512)
    // and n_tiles <= 16, so the splits m_tiles n_tiles partials fit in its Cp m_tiles floats); this rank's rows, both directions
    // when sym.  The weights carry every scalar: the epilogues scale nothing.
    launch_grad_products<EPI_OUT, EPI_OUT_TD>(rows, cols, d, NceGemmArgs{}, w.e, w.slabs, w.rowsum_part, dt, a, b, out_bf16, da, db, s);
}

// ---- supervised contrastive loss on the same GEMMs, both directions from one block (include/aecf_hip.h) ---------------------

namespace {

// workspace carve of the supervised loss
struct SupWs {
    unsigned short* e;                  // [Rp][Cp] bf16, tiled as E
    float* row_part;                    // [3][n_tiles][Rp]  sums of E | counts | matched sums
    float* col_part;                    // [3][m_tiles][Cp]
    float* row_stats;                   // [3][Rp]  l | count | matched sum
    float* u;                           // [Rp]
    float* rn;                          // [Rp]
    float* v;                           // [Cp]
    float* rnc;                         // [Cp]
    float* ediag;                       // [Rp]
    float* slabs;                       // [splits][rows][d]
    size_t bytes;
};

SupWs sup_carve(void* ws, int64_t rows, int64_t cols, int d) {
    const int64_t Rp = up256(rows), Cp = up256(cols);
    const int64_t mt = Rp / BT, nt = Cp / BT;
    SupWs w;
    char* p = (char*)ws;
    size_t off = 0;
    auto take = [&](size_t n) { char* r = p + off; off += al256(n); return r; };
    w.e = (unsigned short*)take((size_t)Rp * Cp * 2);
    w.row_part = (float*)take((size_t)3 * nt * Rp * 4);
    w.col_part = (float*)take((size_t)3 * mt * Cp * 4);
    w.row_stats = (float*)take((size_t)3 * Rp * 4);
    w.u = (float*)take((size_t)Rp * 4);
    w.rn = (float*)take((size_t)Rp * 4);
    w.v = (float*)take((size_t)Cp * 4);
    w.rnc = (float*)take((size_t)Cp * 4);
    w.ediag = (float*)take((size_t)Rp * 4);
    w.slabs = (float*)take((size_t)da_splits(Rp, Cp, d) * rows * d * 4);
    w.bytes = off;
    return w;
}

}  // namespace

// counts travel as float32 (exact below 2^24) so that one all-reduce carries the three column statistics
bool supcon_gemm_supported(int d, float min_temperature, int64_t cols) {
    return nce_gemm_supported(0, d, min_temperature) && cols <= ((int64_t)1 << 24);
}

size_t supcon_gemm_workspace_bytes(int64_t rows, int64_t cols, int d) { return sup_carve(nullptr, rows, cols, d).bytes + 256; }

// pass 1: E, the row statistics (workspace) and this rank's column statistics col_stats [3][cols]
void launch_supcon_gemm_pass1(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, const void* a, const void* b,
                              const int64_t* row_labels, const int64_t* col_labels, void* workspace, float* col_stats, hipStream_t s) {
    const SupWs w = sup_carve(workspace, rows, cols, d);
    const int64_t Rp = up256(rows), Cp = up256(cols);
    LogitsLaunch L = logits_args(rows, cols, d, a, b);
    NceGemmArgs& g = L.g;
    g.e = w.e; g.e_tiles = Cp / 64;
    g.temp = dt.t; g.min_temp = dt.min_t; g.row_offset = row_offset;
    g.lab_row = (const long long*)row_labels; g.lab_col = (const long long*)col_labels;
    const int64_t rplane = (int64_t)g.n_tiles * Rp, cplane = (int64_t)g.m_tiles * Cp;
    g.rowsum_part = w.row_part; g.rowcnt_part = w.row_part + rplane; g.rowsx_part = w.row_part + 2 * rplane;
    g.colsum_part = w.col_part; g.colcnt_part = w.col_part + cplane; g.colsx_part = w.col_part + 2 * cplane;
    launch_gemm<OP_ROW, OP_ROW, EPI_SUP, MAP_2D>(g, L.blocks, s);
    sup_sums_kernel<<<dim3((unsigned)((Rp + Cp) / 64), 3), dim3(256), 0, s>>>(w.row_part, w.col_part, g.m_tiles, g.n_tiles, rows, cols,
                                                                              w.row_stats, col_stats);
}

// normalisers + loss rows from the column statistics of all ranks
void launch_supcon_gemm_loss(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, const void* a, const void* b,
                             const float* col_stats, void* workspace, float* loss_rows, hipStream_t s) {
    const SupWs w = sup_carve(workspace, rows, cols, d);
    SupFinArgs f = {};
    f.a = (const unsigned short*)a; f.b = (const unsigned short*)b; f.row_stats = w.row_stats; f.col_stats = col_stats;
    f.u = w.u; f.rn = w.rn; f.v = w.v; f.rnc = w.rnc; f.loss_rows = loss_rows; f.ediag = w.ediag;
    f.rows = rows; f.cols = cols; f.row_offset = row_offset; f.Rp = up256(rows); f.Cp = up256(cols); f.d = d;
    f.temp = dt.t; f.min_temp = dt.min_t;
    sup_finalize_kernel<<<dim3((unsigned)((f.Rp + 3) / 4)), dim3(256), 0, s>>>(f);
}

// gradients: weights in place over E, da = W b, db = W^T a, dt.d_t; launch_supcon_gemm_loss must have run on this workspace
void launch_supcon_gemm_grads(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, float coef, const void* a,
                              const void* b, const int64_t* row_labels, const int64_t* col_labels, void* workspace,
                              const float* upstream, int out_bf16, void* da, void* db, hipStream_t s) {
    const SupWs w = sup_carve(workspace, rows, cols, d);
    const int64_t Rp = up256(rows), Cp = up256(cols);
    const int64_t chunks = Rp * (Cp / 8);
    sup_weights_kernel<false><<<dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, s>>>(
        w.e, Cp / 64, Rp / BT, w.u, w.v, w.rn, w.rnc, w.ediag, (const long long*)row_labels, (const long long*)col_labels, rows, cols,
        row_offset, coef, upstream, dt.t, dt.min_t);
    // the tdot partials go into the first plane of the row partials (dead since the sums launch), as in launch_nce_gemm_grads
    launch_grad_products<EPI_OUT, EPI_OUT_TD>(rows, cols, d, NceGemmArgs{}, w.e, w.slabs, w.row_part, &dt, a, b, out_bf16, da, db, s);
}

// ---- multi-label contrastive loss on the same GEMMs: class sets and a weighting in place of the labels (include/aecf_hip.h).
// The workspace is SupWs (the weight sums where the counts stand); the loss pass is launch_supcon_gemm_loss.

void launch_supcon_ml_gemm_pass1(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, const void* a,
                                 const void* b, const uint64_t* row_sets, const uint64_t* col_sets, int jaccard, void* workspace,
                                 float* col_stats, hipStream_t s) {
    const SupWs w = sup_carve(workspace, rows, cols, d);
    const int64_t Rp = up256(rows), Cp = up256(cols);
    LogitsLaunch L = logits_args(rows, cols, d, a, b);
    NceGemmArgs& g = L.g;
    g.e = w.e; g.e_tiles = Cp / 64;
    g.temp = dt.t; g.min_temp = dt.min_t; g.row_offset = row_offset;
    g.lab_row = (const long long*)row_sets; g.lab_col = (const long long*)col_sets;
    const int64_t rplane = (int64_t)g.n_tiles * Rp, cplane = (int64_t)g.m_tiles * Cp;
    g.rowsum_part = w.row_part; g.rowcnt_part = w.row_part + rplane; g.rowsx_part = w.row_part + 2 * rplane;
    g.colsum_part = w.col_part; g.colcnt_part = w.col_part + cplane; g.colsx_part = w.col_part + 2 * cplane;
    if (jaccard) launch_gemm<OP_ROW, OP_ROW, EPI_SETS_JAC, MAP_2D>(g, L.blocks, s);
    else launch_gemm<OP_ROW, OP_ROW, EPI_SETS_OV, MAP_2D>(g, L.blocks, s);
    sup_sums_kernel<<<dim3((unsigned)((Rp + Cp) / 64), 3), dim3(256), 0, s>>>(w.row_part, w.col_part, g.m_tiles, g.n_tiles, rows, cols,
                                                                              w.row_stats, col_stats);
}

void launch_supcon_ml_gemm_grads(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, float coef,
                                 const void* a, const void* b, const uint64_t* row_sets, const uint64_t* col_sets, int jaccard,
                                 void* workspace, const float* upstream, int out_bf16, void* da, void* db, hipStream_t s) {
    const SupWs w = sup_carve(workspace, rows, cols, d);
    const int64_t Rp = up256(rows), Cp = up256(cols);
    const int64_t chunks = Rp * (Cp / 8);
    const dim3 grid((unsigned)((chunks + 255) / 256));
    const unsigned long long* sr = (const unsigned long long*)row_sets;
    const unsigned long long* sc = (const unsigned long long*)col_sets;
    if (jaccard)
        set_weights_kernel<true, false><<<grid, dim3(256), 0, s>>>(w.e, Cp / 64, Rp / BT, w.u, w.v, w.rn, w.rnc, w.ediag, sr, sc, rows,
                                                                   cols, row_offset, coef, upstream, dt.t, dt.min_t);
    else
        set_weights_kernel<false, false><<<grid, dim3(256), 0, s>>>(w.e, Cp / 64, Rp / BT, w.u, w.v, w.rn, w.rnc, w.ediag, sr, sc, rows,
                                                                    cols, row_offset, coef, upstream, dt.t, dt.min_t);
    // the tdot partials go into the first plane of the row partials (dead since the sums launch), as in launch_nce_gemm_grads
    launch_grad_products<EPI_OUT, EPI_OUT_TD>(rows, cols, d, NceGemmArgs{}, w.e, w.slabs, w.row_part, &dt, a, b, out_bf16, da, db, s);
}

// ---- NT-Xent on the same GEMMs: three logits blocks of one rank, one exchange (include/aecf_hip.h) -------------------------------
//   X = a_loc . b_all^T (EPI_EXP_DT, InfoNCE's pass 1 to the bit: row sums lX, this rank's column sums cX)
//   Y = a_loc . a_all^T, Z = b_loc . b_all^T (EPI_EXP_SELF: the anchor itself, column row_offset + i, left out by index; row sums)
// Da = lX + lY is local; Db = sum over ranks of cX, plus lZ on the owner's range: each rank adds its lZ into its own range of
// col_sums before the ONE all-reduce.  The b x a block is X^T and is never formed.  Loss and weights are InfoNCE's kernels with
// l := Da, c := Db; Y and Z take the weights body with v = 0 (Z with u_i = 1 / Db_(off + i)) and nothing at the excluded key.

namespace {

// Da_i = lX_i + lY_i in place over l; col_sums[off + i] += lZ_i: one thread per local row, one float32 addition each, no atomics
__global__ __launch_bounds__(256) void ntx_combine_kernel(float* l, const float* ly, const float* lz, float* col_sums, int64_t rows,
                                                          int64_t row_offset) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    l[i] = l[i] + ly[i];
    col_sums[row_offset + i] = col_sums[row_offset + i] + lz[i];
}

// what the weights of Y and Z read: uz_i = 1 / Db_(off + i) (the v of its column; 0 in the padding) and a vector of zeros [Cp]
// that stands for v and for the float32 exponential at the excluded key
__global__ __launch_bounds__(256) void ntx_prep_kernel(const float* v, float* uz, float* zero, int64_t rows, int64_t row_offset,
                                                       int64_t Rp, int64_t Cp) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < Cp) zero[k] = 0.f;
    if (k < Rp) uz[k] = k < rows ? v[row_offset + k] : 0.f;
}

struct NtxWs {
    unsigned short* e[3];               // X | Y | Z, each [Rp][Cp] bf16, tiled as E
    float* rowsum_part;                 // [n_tiles][Rp]   one block after the other
    float* colsum_part;                 // [m_tiles][Cp]   block X
    float* l;                           // [Rp]  lX, then Da
    float* ly;                          // [Rp]
    float* lz;                          // [Rp]
    float* u;                           // [Rp]  1 / Da
    float* v;                           // [Cp]  1 / Db
    float* uz;                          // [Rp]  1 / Db_(off + i)
    float* ediag;                       // [Rp]
    float* zero;                        // [Cp]
    float* tdot_part;                   // [3][splits <= 32][m_tiles][n_tiles_d <= 16]
    float* slabs;                       // [2 splits][rows][d]: the slabs of W_X b_all, behind them those of W_Y a_all
    float* stage;                       // [2][cols][d]: W_X^T a_loc | W_Z^T b_loc in float32
    size_t bytes;
};

NtxWs ntx_carve(void* ws, int64_t rows, int64_t cols, int d) {
    const int64_t Rp = up256(rows), Cp = up256(cols);
    const int64_t mt = Rp / BT, nt = Cp / BT;
    NtxWs w;
    char* p = (char*)ws;
    size_t off = 0;
    auto take = [&](size_t n) { char* r = p + off; off += al256(n); return r; };
    for (int k = 0; k < 3; ++k) w.e[k] = (unsigned short*)take((size_t)Rp * Cp * 2);
    w.rowsum_part = (float*)take((size_t)nt * Rp * 4);
    w.colsum_part = (float*)take((size_t)mt * Cp * 4);
    w.l = (float*)take((size_t)Rp * 4);
    w.ly = (float*)take((size_t)Rp * 4);
    w.lz = (float*)take((size_t)Rp * 4);
    w.u = (float*)take((size_t)Rp * 4);
    w.v = (float*)take((size_t)Cp * 4);
    w.uz = (float*)take((size_t)Rp * 4);
    w.ediag = (float*)take((size_t)Rp * 4);
    w.zero = (float*)take((size_t)Cp * 4);
    w.tdot_part = (float*)take((size_t)3 * 32 * 16 * mt * 4);
    w.slabs = (float*)take((size_t)2 * da_splits(Rp, Cp, d) * rows * d * 4);
    w.stage = (float*)take((size_t)2 * cols * d * 4);
    w.bytes = off;
    return w;
}

}  // namespace

bool ntxent_gemm_supported(int d, float min_temperature) { return nce_gemm_supported(0, d, min_temperature); }

size_t ntxent_gemm_workspace_bytes(int64_t rows, int64_t cols, int d) { return ntx_carve(nullptr, rows, cols, d).bytes + 256; }

// pass 1: the three blocks, Da (workspace) and col_sums [cols] = this rank's cX, plus lZ on [row_offset, row_offset + rows)
void launch_ntxent_gemm_pass1(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, const void* a_loc,
                              const void* b_loc, const void* a_all, const void* b_all, void* workspace, float* col_sums, hipStream_t s) {
    const NtxWs w = ntx_carve(workspace, rows, cols, d);
    const int64_t Rp = up256(rows), Cp = up256(cols);
    {
        LogitsLaunch L = logits_args(rows, cols, d, a_loc, b_all);
        NceGemmArgs& g = L.g;
        g.e = w.e[0]; g.e_tiles = Cp / 64;
        g.rowsum_part = w.rowsum_part; g.colsum_part = w.colsum_part;
        g.temp = dt.t; g.min_temp = dt.min_t;
        launch_gemm<OP_ROW, OP_ROW, EPI_EXP_DT, MAP_2D>(g, L.blocks, s);
        nce_sums_kernel<<<dim3((unsigned)((Rp + Cp) / 64)), dim3(256), 0, s>>>(w.rowsum_part, w.colsum_part, g.m_tiles, g.n_tiles, rows, cols,
                                                                               w.l, col_sums);
    }
    for (int k = 1; k < 3; ++k) {
        LogitsLaunch L = logits_args(rows, cols, d, k == 1 ? a_loc : b_loc, k == 1 ? a_all : b_all);
        NceGemmArgs& g = L.g;
        g.e = w.e[k]; g.e_tiles = Cp / 64;
        g.rowsum_part = w.rowsum_part;
        g.temp = dt.t; g.min_temp = dt.min_t; g.row_offset = row_offset;
        launch_gemm<OP_ROW, OP_ROW, EPI_EXP_SELF, MAP_2D>(g, L.blocks, s);
        // the row blocks of the sums launch alone: this block leaves no column partials
        nce_sums_kernel<<<dim3((unsigned)(Rp / 64)), dim3(256), 0, s>>>(w.rowsum_part, nullptr, g.m_tiles, g.n_tiles, rows, cols,
                                                                        k == 1 ? w.ly : w.lz, nullptr);
    }
    ntx_combine_kernel<<<dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s>>>(w.l, w.ly, w.lz, col_sums, rows, row_offset);
}

// normalisers + loss rows of this rank's 2 rows anchors from the col_sums of all ranks: InfoNCE's finalize with l := Da, c := Db
void launch_ntxent_gemm_loss(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, const void* a_loc,
                             const void* b_all, const float* col_sums, void* workspace, float* loss_rows, hipStream_t s) {
    const NtxWs w = ntx_carve(workspace, rows, cols, d);
    NceFinArgs f = {};
    f.a = (const unsigned short*)a_loc; f.b = (const unsigned short*)b_all; f.l = w.l; f.c = col_sums;
    f.u = w.u; f.v = w.v; f.ediag = w.ediag; f.loss_rows = loss_rows; f.rows = rows; f.cols = cols; f.row_offset = row_offset;
    f.Rp = up256(rows); f.Cp = up256(cols); f.d = d; f.sym = 1;
    f.temp = dt.t; f.min_temp = dt.min_t;
    nce_finalize_kernel<true><<<dim3((unsigned)((f.Rp + 3) / 4)), dim3(256), 0, s>>>(f);
}

// gradients: the three weights passes in place, then
//   d_a_loc = W_X b_all + W_Y a_all (one slab sum over both products' slabs)      d_b_loc = W_Z b_all
//   d_a_all = W_Y^T a_loc                                                         d_b_all = W_X^T a_loc + W_Z^T b_loc (float32 stage)
// every output rounded once from its float32 sum; dt.d_t from the partials of the three da products, one fixed-order reduction
void launch_ntxent_gemm_grads(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, float coef, const void* a_loc,
                              const void* b_loc, const void* a_all, const void* b_all, void* workspace, const float* upstream,
                              int out_bf16, void* d_a_loc, void* d_b_loc, void* d_a_all, void* d_b_all, hipStream_t s) {
    const NtxWs w = ntx_carve(workspace, rows, cols, d);
    const int64_t Rp = up256(rows), Cp = up256(cols);
    const int64_t chunks = Rp * (Cp / 8);
    const dim3 wgrid((unsigned)((chunks + 255) / 256));
    ntx_prep_kernel<<<dim3((unsigned)(Cp / 256)), dim3(256), 0, s>>>(w.v, w.uz, w.zero, rows, row_offset, Rp, Cp);
    nce_weights_dt_kernel<<<wgrid, dim3(256), 0, s>>>(w.e[0], Cp / 64, Rp / BT, w.u, w.v, w.ediag, rows, row_offset, coef, 2.0f, upstream,
                                                      dt.t, dt.min_t);
    nce_weights_dt_kernel<<<wgrid, dim3(256), 0, s>>>(w.e[1], Cp / 64, Rp / BT, w.u, w.zero, w.zero, rows, row_offset, coef, 0.0f, upstream,
                                                      dt.t, dt.min_t);
    nce_weights_dt_kernel<<<wgrid, dim3(256), 0, s>>>(w.e[2], Cp / 64, Rp / BT, w.uz, w.zero, w.zero, rows, row_offset, coef, 0.0f, upstream,
                                                      dt.t, dt.min_t);
    const bool want_td = dt.d_t != nullptr;
    const int64_t n_td = da_tdot_count(rows, cols, d), n_loc = rows * (int64_t)d, n_all = cols * (int64_t)d;
    const NceGemmArgs g0 = {};
    // both products always leave float32 slabs, those of W_Y a_all behind those of W_X b_all: one sum, one rounding
    const int sx = launch_da_product<EPI_OUT, EPI_OUT_TD>(rows, cols, d, g0, w.e[0], w.slabs, w.tdot_part, want_td, a_loc, b_all, 0,
                                                          nullptr, s);
    const int sy = launch_da_product<EPI_OUT, EPI_OUT_TD>(rows, cols, d, g0, w.e[1], w.slabs + sx * n_loc, w.tdot_part + n_td, want_td,
                                                          a_loc, a_all, 0, nullptr, s);
    launch_slab_sum(w.slabs, sx + sy, n_loc, d_a_loc, out_bf16, s);
    const int sz = launch_da_product<EPI_OUT, EPI_OUT_TD>(rows, cols, d, g0, w.e[2], w.slabs, w.tdot_part + 2 * n_td, want_td, b_loc,
                                                          b_all, out_bf16, d_b_loc, s);
    if (sz) launch_slab_sum(w.slabs, sz, n_loc, d_b_loc, out_bf16, s);
    if (want_td) launch_nce_dtemp(w.tdot_part, 3 * n_td, 1, dt, s);
    launch_db_product<EPI_OUT>(rows, cols, d, g0, w.e[1], a_loc, out_bf16, d_a_all, s);
    launch_db_product<EPI_OUT>(rows, cols, d, g0, w.e[0], a_loc, 0, w.stage, s);
    launch_db_product<EPI_OUT>(rows, cols, d, g0, w.e[2], b_loc, 0, w.stage + n_all, s);
    launch_slab_sum(w.stage, 2, n_all, d_b_all, out_bf16, s);
}

// ---- pooled supervised contrastive loss (Khosla et al.: one pool of both views) on the same GEMMs: NT-Xent's three logits blocks
// with the label statistics of the supervised loss on each (include/aecf_hip.h) ------------------------------------------------------
//   X = a_loc . b_all^T (EPI_SUP, the cross-view pass 1 to the bit: row statistics and this rank's column statistics; the partner is
//       excluded from the matches and joins by index from its own float32 dot)
//   Y = a_loc . a_all^T, Z = b_loc . b_all^T (EPI_SUP_SELF: the anchor itself, column row_offset + i, is no key and no positive; row
//       statistics alone)
// Anchor a_i: (Da, ka, sa) = X's row statistics + Y's; anchor b_g: (Db, kb, sb) = the ranks' column statistics of X plus Z's row
// statistics of the row's owner -- sup_pool_combine_kernel adds a rank's Z statistics into its own range of col_stats before the ONE
// all-reduce of [3][cols].  sup_finalize_kernel serves unchanged on the combined statistics; W_X is sup_weights_kernel's, W_Y and W_Z
// its SELF variant (v = rnc = 0; Z with u and rn gathered at off + i); the six gradient products are those of NT-Xent.

namespace {

// ntx_combine_kernel over the three quantities q (sums of E | counts | matched sums): row_stats[q][i] = X[q][i] + Y[q][i] in place
// over X's, col_stats[q][off + i] += Z[q][i]; one thread per local row, one float32 addition per quantity and side, no atomics
__global__ __launch_bounds__(256) void sup_pool_combine_kernel(float* row_stats, const float* y_stats, const float* z_stats,
                                                               float* col_stats, int64_t rows, int64_t cols, int64_t row_offset,
                                                               int64_t Rp) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        row_stats[q * Rp + i] = row_stats[q * Rp + i] + y_stats[q * Rp + i];
        col_stats[q * cols + row_offset + i] = col_stats[q * cols + row_offset + i] + z_stats[q * Rp + i];
    }
}

// what the weights of Y and Z read: uz_i = 1 / Db_(off + i) and rnz_i = 1 / nb_(off + i) (the v and rnc of the row's own column; 0 in
// the padding) and a vector of zeros [Cp] that stands for v and rnc
__global__ __launch_bounds__(256) void sup_pool_prep_kernel(const float* v, const float* rnc, float* uz, float* rnz, float* zero,
                                                            int64_t rows, int64_t row_offset, int64_t Rp, int64_t Cp) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < Cp) zero[k] = 0.f;
    if (k < Rp) {
        uz[k] = k < rows ? v[row_offset + k] : 0.f;
        rnz[k] = k < rows ? rnc[row_offset + k] : 0.f;
    }
}

struct SupPoolWs {
    unsigned short* e[3];               // X | Y | Z, each [Rp][Cp] bf16, tiled as E
    float* row_part;                    // [3][n_tiles][Rp]  sums of E | counts | matched sums, one block after the other
    float* col_part;                    // [3][m_tiles][Cp]  block X
    float* row_stats;                   // [3][Rp]  X's, then the combined Da | ka | sa
    float* y_stats;                     // [3][Rp]
    float* z_stats;                     // [3][Rp]
    float* u;                           // [Rp]  1 / Da
    float* rn;                          // [Rp]  1 / na
    float* v;                           // [Cp]  1 / Db
    float* rnc;                         // [Cp]  1 / nb
    float* uz;                          // [Rp]  1 / Db_(off + i)
    float* rnz;                         // [Rp]  1 / nb_(off + i)
    float* ediag;                       // [Rp]
    float* zero;                        // [Cp]
    float* tdot_part;                   // [3][splits <= 32][m_tiles][n_tiles_d <= 16]
    float* slabs;                       // [2 splits][rows][d]: the slabs of W_X b_all, behind them those of W_Y a_all
    float* stage;                       // [2][cols][d]: W_X^T a_loc | W_Z^T b_loc in float32
    size_t bytes;
};

SupPoolWs sup_pool_carve(void* ws, int64_t rows, int64_t cols, int d) {
    const int64_t Rp = up256(rows), Cp = up256(cols);
    const int64_t mt = Rp / BT, nt = Cp / BT;
    SupPoolWs w;
    char* p = (char*)ws;
    size_t off = 0;
    auto take = [&](size_t n) { char* r = p + off; off += al256(n); return r; };
    for (int k = 0; k < 3; ++k) w.e[k] = (unsigned short*)take((size_t)Rp * Cp * 2);
    w.row_part = (float*)take((size_t)3 * nt * Rp * 4);
    w.col_part = (float*)take((size_t)3 * mt * Cp * 4);
    w.row_stats = (float*)take((size_t)3 * Rp * 4);
    w.y_stats = (float*)take((size_t)3 * Rp * 4);
    w.z_stats = (float*)take((size_t)3 * Rp * 4);
    w.u = (float*)take((size_t)Rp * 4);
    w.rn = (float*)take((size_t)Rp * 4);
    w.v = (float*)take((size_t)Cp * 4);
    w.rnc = (float*)take((size_t)Cp * 4);
    w.uz = (float*)take((size_t)Rp * 4);
    w.rnz = (float*)take((size_t)Rp * 4);
    w.ediag = (float*)take((size_t)Rp * 4);
    w.zero = (float*)take((size_t)Cp * 4);
    w.tdot_part = (float*)take((size_t)3 * 32 * 16 * mt * 4);
    w.slabs = (float*)take((size_t)2 * da_splits(Rp, Cp, d) * rows * d * 4);
    w.stage = (float*)take((size_t)2 * cols * d * 4);
    w.bytes = off;
    return w;
}

}  // namespace

// An anchor's count adds the matches of two blocks, each at most cols - 1 (the partner / the anchor excluded): 1 + ka <= 2 cols - 1
// has to stay exact in float32, so cols <= 2^23 -- half the bound of the cross-view form.
bool supcon_pool_gemm_supported(int d, float min_temperature, int64_t cols) {
    return nce_gemm_supported(0, d, min_temperature) && cols <= ((int64_t)1 << 23);
}

size_t supcon_pool_gemm_workspace_bytes(int64_t rows, int64_t cols, int d) { return sup_pool_carve(nullptr, rows, cols, d).bytes + 256; }

// pass 1: the three blocks, the combined row statistics (workspace) and col_stats [3][cols] = this rank's column statistics of X, plus
// the row statistics of Z on [row_offset, row_offset + rows)
void launch_supcon_pool_gemm_pass1(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, const void* a_loc,
                                   const void* b_loc, const void* a_all, const void* b_all, const int64_t* row_labels,
                                   const int64_t* col_labels, void* workspace, float* col_stats, hipStream_t s) {
    const SupPoolWs w = sup_pool_carve(workspace, rows, cols, d);
    const int64_t Rp = up256(rows), Cp = up256(cols);
    for (int k = 0; k < 3; ++k) {
        LogitsLaunch L = logits_args(rows, cols, d, k == 2 ? b_loc : a_loc, k == 1 ? a_all : b_all);
        NceGemmArgs& g = L.g;
        g.e = w.e[k]; g.e_tiles = Cp / 64;
        g.temp = dt.t; g.min_temp = dt.min_t; g.row_offset = row_offset;
        g.lab_row = (const long long*)row_labels; g.lab_col = (const long long*)col_labels;
        const int64_t rplane = (int64_t)g.n_tiles * Rp, cplane = (int64_t)g.m_tiles * Cp;
        g.rowsum_part = w.row_part; g.rowcnt_part = w.row_part + rplane; g.rowsx_part = w.row_part + 2 * rplane;
        if (k == 0) {
            g.colsum_part = w.col_part; g.colcnt_part = w.col_part + cplane; g.colsx_part = w.col_part + 2 * cplane;
            launch_gemm<OP_ROW, OP_ROW, EPI_SUP, MAP_2D>(g, L.blocks, s);
            sup_sums_kernel<<<dim3((unsigned)((Rp + Cp) / 64), 3), dim3(256), 0, s>>>(w.row_part, w.col_part, g.m_tiles, g.n_tiles, rows,
                                                                                      cols, w.row_stats, col_stats);
        } else {
            launch_gemm<OP_ROW, OP_ROW, EPI_SUP_SELF, MAP_2D>(g, L.blocks, s);
            // the row blocks of the sums launch alone: this block leaves no column partials
            sup_sums_kernel<<<dim3((unsigned)(Rp / 64), 3), dim3(256), 0, s>>>(w.row_part, nullptr, g.m_tiles, g.n_tiles, rows, cols,
                                                                               k == 1 ? w.y_stats : w.z_stats, nullptr);
        }
    }
    sup_pool_combine_kernel<<<dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s>>>(w.row_stats, w.y_stats, w.z_stats, col_stats, rows,
                                                                                       cols, row_offset, Rp);
}

// normalisers + loss rows of this rank's 2 rows anchors from the col_stats of all ranks: sup_finalize_kernel on the combined statistics
void launch_supcon_pool_gemm_loss(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, const void* a_loc,
                                  const void* b_all, const float* col_stats, void* workspace, float* loss_rows, hipStream_t s) {
    const SupPoolWs w = sup_pool_carve(workspace, rows, cols, d);
    SupFinArgs f = {};
    f.a = (const unsigned short*)a_loc; f.b = (const unsigned short*)b_all; f.row_stats = w.row_stats; f.col_stats = col_stats;
    f.u = w.u; f.rn = w.rn; f.v = w.v; f.rnc = w.rnc; f.loss_rows = loss_rows; f.ediag = w.ediag;
    f.rows = rows; f.cols = cols; f.row_offset = row_offset; f.Rp = up256(rows); f.Cp = up256(cols); f.d = d;
    f.temp = dt.t; f.min_temp = dt.min_t;
    sup_finalize_kernel<<<dim3((unsigned)((f.Rp + 3) / 4)), dim3(256), 0, s>>>(f);
}

namespace {

// the six products, two slab sums and the dT reduction over the three weighted blocks
//   d_a_loc = W_X b_all + W_Y a_all (one slab sum over both products' slabs)      d_b_loc = W_Z b_all
//   d_a_all = W_Y^T a_loc                                                         d_b_all = W_X^T a_loc + W_Z^T b_loc (float32 stage)
void sup_pool_products(const SupPoolWs& w, int64_t rows, int64_t cols, int d, const NceDevTemp& dt, const void* a_loc, const void* b_loc,
                       const void* a_all, const void* b_all, int out_bf16, void* d_a_loc, void* d_b_loc, void* d_a_all, void* d_b_all,
                       hipStream_t s) {
    const bool want_td = dt.d_t != nullptr;
    const int64_t n_td = da_tdot_count(rows, cols, d), n_loc = rows * (int64_t)d, n_all = cols * (int64_t)d;
    const NceGemmArgs g0 = {};
    // both products always leave float32 slabs, those of W_Y a_all behind those of W_X b_all: one sum, one rounding
    const int sx = launch_da_product<EPI_OUT, EPI_OUT_TD>(rows, cols, d, g0, w.e[0], w.slabs, w.tdot_part, want_td, a_loc, b_all, 0,
                                                          nullptr, s);
    const int sy = launch_da_product<EPI_OUT, EPI_OUT_TD>(rows, cols, d, g0, w.e[1], w.slabs + sx * n_loc, w.tdot_part + n_td, want_td,
                                                          a_loc, a_all, 0, nullptr, s);
    launch_slab_sum(w.slabs, sx + sy, n_loc, d_a_loc, out_bf16, s);
    const int sz = launch_da_product<EPI_OUT, EPI_OUT_TD>(rows, cols, d, g0, w.e[2], w.slabs, w.tdot_part + 2 * n_td, want_td, b_loc,
                                                          b_all, out_bf16, d_b_loc, s);
    if (sz) launch_slab_sum(w.slabs, sz, n_loc, d_b_loc, out_bf16, s);
    if (want_td) launch_nce_dtemp(w.tdot_part, 3 * n_td, 1, dt, s);
    launch_db_product<EPI_OUT>(rows, cols, d, g0, w.e[1], a_loc, out_bf16, d_a_all, s);
    launch_db_product<EPI_OUT>(rows, cols, d, g0, w.e[0], a_loc, 0, w.stage, s);
    launch_db_product<EPI_OUT>(rows, cols, d, g0, w.e[2], b_loc, 0, w.stage + n_all, s);
    launch_slab_sum(w.stage, 2, n_all, d_b_all, out_bf16, s);
}

}  // namespace

// gradients: the three weights passes in place, then the six products in the arrangement of launch_ntxent_gemm_grads
//   d_a_loc = W_X b_all + W_Y a_all (one slab sum over both products' slabs)      d_b_loc = W_Z b_all
//   d_a_all = W_Y^T a_loc                                                         d_b_all = W_X^T a_loc + W_Z^T b_loc (float32 stage)
// every output rounded once from its float32 sum; dt.d_t from the partials of the three da products, one fixed-order reduction
void launch_supcon_pool_gemm_grads(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, float coef,
                                   const void* a_loc, const void* b_loc, const void* a_all, const void* b_all, const int64_t* row_labels,
                                   const int64_t* col_labels, void* workspace, const float* upstream, int out_bf16, void* d_a_loc,
                                   void* d_b_loc, void* d_a_all, void* d_b_all, hipStream_t s) {
    const SupPoolWs w = sup_pool_carve(workspace, rows, cols, d);
    const int64_t Rp = up256(rows), Cp = up256(cols);
    const int64_t chunks = Rp * (Cp / 8);
    const dim3 wgrid((unsigned)((chunks + 255) / 256));
    const long long* lr = (const long long*)row_labels;
    const long long* lc = (const long long*)col_labels;
    sup_pool_prep_kernel<<<dim3((unsigned)(Cp / 256)), dim3(256), 0, s>>>(w.v, w.rnc, w.uz, w.rnz, w.zero, rows, row_offset, Rp, Cp);
    sup_weights_kernel<false><<<wgrid, dim3(256), 0, s>>>(w.e[0], Cp / 64, Rp / BT, w.u, w.v, w.rn, w.rnc, w.ediag, lr, lc, rows, cols,
                                                          row_offset, coef, upstream, dt.t, dt.min_t);
    sup_weights_kernel<true><<<wgrid, dim3(256), 0, s>>>(w.e[1], Cp / 64, Rp / BT, w.u, w.zero, w.rn, w.zero, nullptr, lr, lc, rows, cols,
                                                         row_offset, coef, upstream, dt.t, dt.min_t);
    sup_weights_kernel<true><<<wgrid, dim3(256), 0, s>>>(w.e[2], Cp / 64, Rp / BT, w.uz, w.zero, w.rnz, w.zero, nullptr, lr, lc, rows, cols,
                                                         row_offset, coef, upstream, dt.t, dt.min_t);
    sup_pool_products(w, rows, cols, d, dt, a_loc, b_loc, a_all, b_all, out_bf16, d_a_loc, d_b_loc, d_a_all, d_b_all, s);
}

// ---- pooled multi-label contrastive loss: the pooled form above with class sets and a weighting in place of the labels
// (include/aecf_hip.h).  X runs EPI_SETS_OV / EPI_SETS_JAC unchanged, Y and Z their row-only SELF forms (the anchor's own key weighs
// 0 by index); workspace (SupPoolWs, the weight sums where the counts stand), combine, prep, the loss pass and the six products are
// those of the pooled single-label form, the weights passes set_weights_kernel's (Y and Z its SELF variant, v = rnc = 0).

// An anchor's weight sum adds two blocks' (each at most cols - 1): the overlap sums are integers and stay exact in float32 up to
// cols = 2^23; Jaccard keeps the same bound.
bool supcon_ml_pool_gemm_supported(int d, float min_temperature, int64_t cols) {
    return supcon_pool_gemm_supported(d, min_temperature, cols);
}

size_t supcon_ml_pool_gemm_workspace_bytes(int64_t rows, int64_t cols, int d) { return supcon_pool_gemm_workspace_bytes(rows, cols, d); }

void launch_supcon_ml_pool_gemm_pass1(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, const void* a_loc,
                                      const void* b_loc, const void* a_all, const void* b_all, const int64_t* row_sets,
                                      const int64_t* col_sets, int jaccard, void* workspace, float* col_stats, hipStream_t s) {
    const SupPoolWs w = sup_pool_carve(workspace, rows, cols, d);
    const int64_t Rp = up256(rows), Cp = up256(cols);
    for (int k = 0; k < 3; ++k) {
        LogitsLaunch L = logits_args(rows, cols, d, k == 2 ? b_loc : a_loc, k == 1 ? a_all : b_all);
        NceGemmArgs& g = L.g;
        g.e = w.e[k]; g.e_tiles = Cp / 64;
        g.temp = dt.t; g.min_temp = dt.min_t; g.row_offset = row_offset;
        g.lab_row = (const long long*)row_sets; g.lab_col = (const long long*)col_sets;
        const int64_t rplane = (int64_t)g.n_tiles * Rp, cplane = (int64_t)g.m_tiles * Cp;
        g.rowsum_part = w.row_part; g.rowcnt_part = w.row_part + rplane; g.rowsx_part = w.row_part + 2 * rplane;
        if (k == 0) {
            g.colsum_part = w.col_part; g.colcnt_part = w.col_part + cplane; g.colsx_part = w.col_part + 2 * cplane;
            if (jaccard) launch_gemm<OP_ROW, OP_ROW, EPI_SETS_JAC, MAP_2D>(g, L.blocks, s);
            else launch_gemm<OP_ROW, OP_ROW, EPI_SETS_OV, MAP_2D>(g, L.blocks, s);
            sup_sums_kernel<<<dim3((unsigned)((Rp + Cp) / 64), 3), dim3(256), 0, s>>>(w.row_part, w.col_part, g.m_tiles, g.n_tiles, rows,
                                                                                      cols, w.row_stats, col_stats);
        } else {
            if (jaccard) launch_gemm<OP_ROW, OP_ROW, EPI_SETS_JAC_SELF, MAP_2D>(g, L.blocks, s);
            else launch_gemm<OP_ROW, OP_ROW, EPI_SETS_OV_SELF, MAP_2D>(g, L.blocks, s);
            // the row blocks of the sums launch alone: this block leaves no column partials
            sup_sums_kernel<<<dim3((unsigned)(Rp / 64), 3), dim3(256), 0, s>>>(w.row_part, nullptr, g.m_tiles, g.n_tiles, rows, cols,
                                                                               k == 1 ? w.y_stats : w.z_stats, nullptr);
        }
    }
    sup_pool_combine_kernel<<<dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s>>>(w.row_stats, w.y_stats, w.z_stats, col_stats, rows,
                                                                                       cols, row_offset, Rp);
}

// sup_finalize_kernel on the combined statistics, the weight sums where the counts stood
void launch_supcon_ml_pool_gemm_loss(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, const void* a_loc,
                                     const void* b_all, const float* col_stats, void* workspace, float* loss_rows, hipStream_t s) {
    launch_supcon_pool_gemm_loss(rows, cols, row_offset, d, dt, a_loc, b_all, col_stats, workspace, loss_rows, s);
}

namespace {

template <bool JAC>
void set_pool_weights(const SupPoolWs& w, int64_t rows, int64_t cols, int64_t row_offset, float coef, const int64_t* row_sets,
                      const int64_t* col_sets, const float* upstream, const NceDevTemp& dt, hipStream_t s) {
    const int64_t Rp = up256(rows), Cp = up256(cols);
    const int64_t chunks = Rp * (Cp / 8);
    const dim3 wgrid((unsigned)((chunks + 255) / 256));
    const unsigned long long* sr = (const unsigned long long*)row_sets;
    const unsigned long long* sc = (const unsigned long long*)col_sets;
    set_weights_kernel<JAC, false><<<wgrid, dim3(256), 0, s>>>(w.e[0], Cp / 64, Rp / BT, w.u, w.v, w.rn, w.rnc, w.ediag, sr, sc, rows, cols,
                                                               row_offset, coef, upstream, dt.t, dt.min_t);
    set_weights_kernel<JAC, true><<<wgrid, dim3(256), 0, s>>>(w.e[1], Cp / 64, Rp / BT, w.u, w.zero, w.rn, w.zero, nullptr, sr, sc, rows, cols,
                                                              row_offset, coef, upstream, dt.t, dt.min_t);
    set_weights_kernel<JAC, true><<<wgrid, dim3(256), 0, s>>>(w.e[2], Cp / 64, Rp / BT, w.uz, w.zero, w.rnz, w.zero, nullptr, sr, sc, rows,
                                                              cols, row_offset, coef, upstream, dt.t, dt.min_t);
}

}  // namespace

// gradients: sup_pool_prep_kernel, the three set weights passes in place, then the products of launch_supcon_pool_gemm_grads
void launch_supcon_ml_pool_gemm_grads(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, float coef,
                                      const void* a_loc, const void* b_loc, const void* a_all, const void* b_all, const int64_t* row_sets,
                                      const int64_t* col_sets, int jaccard, void* workspace, const float* upstream, int out_bf16,
                                      void* d_a_loc, void* d_b_loc, void* d_a_all, void* d_b_all, hipStream_t s) {
    const SupPoolWs w = sup_pool_carve(workspace, rows, cols, d);
    const int64_t Rp = up256(rows), Cp = up256(cols);
    sup_pool_prep_kernel<<<dim3((unsigned)(Cp / 256)), dim3(256), 0, s>>>(w.v, w.rnc, w.uz, w.rnz, w.zero, rows, row_offset, Rp, Cp);
    if (jaccard) set_pool_weights<true>(w, rows, cols, row_offset, coef, row_sets, col_sets, upstream, dt, s);
    else set_pool_weights<false>(w, rows, cols, row_offset, coef, row_sets, col_sets, upstream, dt, s);
    sup_pool_products(w, rows, cols, d, dt, a_loc, b_loc, a_all, b_all, out_bf16, d_a_loc, d_b_loc, d_a_all, d_b_all, s);
}

// ---- sigmoid (SigLIP) loss on the same GEMMs ---------------------------------------------------------------------------

bool sig_gemm_supported(int dtype, int d) { return dtype == 0 && d % 64 == 0 && d >= 64 && d <= 4096; }

size_t sig_gemm_workspace_bytes(int64_t rows, int64_t cols, int d) { return sig_carve(nullptr, rows, cols, d).bytes + 256; }

// logits pass: g (workspace), loss_rows[i] = sum_j softplus(-y_ij l_ij), d_bias[0] = sum_ij g_ij
void launch_sig_gemm_pass1(int64_t rows, int64_t cols, int64_t row_offset, int d, const float* temp, float min_temp, const float* bias,
                           const void* a, const void* b, void* workspace, float* loss_rows, float* d_bias, hipStream_t s) {
    const SigWs w = sig_carve(workspace, rows, cols, d);
    const int64_t Rp = up256(rows), Cp = up256(cols);
    LogitsLaunch L = logits_args(rows, cols, d, a, b);
    NceGemmArgs& g = L.g;
    g.e = w.g; g.e_tiles = Cp / 64;
    g.temp = temp; g.min_temp = min_temp; g.bias = bias; g.row_offset = row_offset;
    g.sp_part = w.sp_part; g.sg_part = w.sg_part;
    launch_gemm<OP_ROW, OP_ROW, EPI_SIG, MAP_2D>(g, L.blocks, s);
    sig_rows_kernel<<<dim3((unsigned)(Rp / 64)), dim3(256), 0, s>>>(w.sp_part, w.sg_part, g.n_tiles, Rp, rows, loss_rows, w.gsum);
    sig_dbias_kernel<<<dim3(1), dim3(256), 0, s>>>(w.gsum, rows, d_bias);
}

// da = (coef / Tc upstream) g b, db = (coef / Tc upstream) g^T a over the g launch_sig_gemm_pass1 left (read, not modified);
// dt.d_t (when wanted) from the float32 da as in launch_nce_gemm_grads
void launch_sig_gemm_grads(int64_t rows, int64_t cols, int d, const NceDevTemp& dt, float coef, const void* a, const void* b,
                           void* workspace, const float* upstream, int out_bf16, void* da, void* db, hipStream_t s) {
    const SigWs w = sig_carve(workspace, rows, cols, d);
    NceGemmArgs g0 = {};
    g0.temp = dt.t; g0.min_temp = dt.min_t; g0.coef = coef; g0.upstream = upstream;
    launch_grad_products<EPI_OUT_S, EPI_OUT_TD_S>(rows, cols, d, g0, w.g, w.slabs, w.tdot_part, &dt, a, b, out_bf16, da, db, s);
}

// ---- retrieval ranks: the counting pass (thresholds, reduction and checks in aecf_retrieval.hip) -------------------------

// per-tile packed counts of a [rows, d] . b [cols, d]^T against pos_row / pos_col (NULL: rows only) into row_part [n_tiles][Rp] and
// col_part [m_tiles][Cp] (Rp, Cp: rows, cols rounded up to 256)
void launch_rank_gemm(int64_t rows, int64_t cols, int64_t row_offset, int d, const void* a, const void* b, const float* pos_row,
                      const float* pos_col, int* row_part, int* col_part, hipStream_t s) {
    LogitsLaunch L = logits_args(rows, cols, d, a, b);
    NceGemmArgs& g = L.g;
    g.row_offset = row_offset;
    g.pos_row = pos_row; g.pos_col = pos_col; g.rank_row_part = row_part; g.rank_col_part = col_part;
    launch_gemm<OP_ROW, OP_ROW, EPI_RANK, MAP_2D>(g, L.blocks, s);
}

// ---- top-k retrieval: the selection pass (merge of the tiles' lists and checks in aecf_retrieval.hip) ---------------------

// per-tile sorted lists of the k <= 16 best keys of every row of a [rows, d] . b [cols, d]^T into part [n_tiles][Rp][kp];
// exclude_partner: element (i, row_offset + i) is not a candidate
void launch_topk_gemm(int64_t rows, int64_t cols, int64_t row_offset, int d, int k, int kp, int exclude_partner, const void* a,
                      const void* b, unsigned long long* part, hipStream_t s) {
    LogitsLaunch L = logits_args(rows, cols, d, a, b);
    NceGemmArgs& g = L.g;
    g.row_offset = exclude_partner ? row_offset : -((int64_t)1 << 40);      // no row has a partner on any tile
    g.topk_part = part; g.topk = k; g.topk_kp = kp;
    launch_gemm<OP_ROW, OP_ROW, EPI_TOPK, MAP_2D>(g, L.blocks, s);
}

}  // namespace aecf
