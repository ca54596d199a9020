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
//
// Multi-view InfoNCE (aecf_nce_multi_pass1 / _loss / _grads) is the symmetric InfoNCE above over P pairs of the views that lie side
// by side in x [rows][views][d] -- every pair m < n, or every pair with one anchor view -- with ONE launch per stage.  Operands are
// read in place: lda = ldb = views d 2 bytes, a view's origin d 2 bytes behind the previous one.  The logits pass is
// nce_multi_logits_kernel: block b is tile b % blocks_per_pair of pair b / blocks_per_pair (blocks_per_pair is a multiple of 8, so a
// tile keeps its XCD and its MAP_2D patch), a pair table in the kernel arguments gives the two origins, and E, the partials, the
// sums and the normalisers of pair p lie p strides behind pair 0's in the workspace; the epilogue is EPI_EXP_DT, so every pair has
// the bits of a two-view call on contiguous copies.  Sums, finalize and weights kernels take the pair from blockIdx.y.  The
// gradient products are nce_multi_product_kernel: block b works for slot b / blocks_per_view, a view that has the role, and its K
// loop runs through the tiles of EVERY partner block of that view -- da: [W_(m,n1) | W_(m,n2) | ..] [x_all[:, n1]; x_all[:, n2]; ..],
// db: sum over m of W_(m,n)^T x_loc[:, m] -- so an output element is one float32 sum over all partners (K split into slabs and the
// fixed-order slab sum as before for da, stored by the GEMM for db) and is rounded once; there is no per-pair stage.  A segment is
// named by 8 bits (pair, partner view) of one 64-bit word per slot; inside the K loop a scalar cursor (segment, K-step in it, the
// two operand origins) moves one step per copy: adds and a compare, a shift at a segment switch -- no barrier, no load and no
// division in a step (aecf_nce_gemm_body.h).  dT comes from the EPI_OUT_TD partials of all da slots in one nce_dtemp_kernel, and
// nce_multi_finish_kernel sums the slabs into dx_loc and writes the zeros of the views that have no role.  With views = 2 the
// three calls give the bits of aecf_nce_sym_*_dt.
//
// Multi-view InfoNCE with missing views (aecf_nce_multi_masked_pair_coef / _pass1 / _loss / _grads) is that form where a row may lack
// views: one presence byte per row (bit v: view v present; pres_loc by the local row, pres_all by the global column), and pair
// (m, n) runs over V_p, the rows that hold both bits, on both sides.  The logits pass is a further epilogue on
// nce_multi_logits_kernel, EPI_EXP_MASK: each of the block's 512 threads loads one of its 256 row bytes or 256 column bytes (the
// way EPI_SETS_* load class words), the flags go to LDS and one vote tells the block whether all 512 hold the pair -- then it
// runs EPI_EXP_DT's tile, bit for bit; otherwise it takes the block-uniform branch of the ragged edge with the flags in place of
// the `iok` / `j < n_valid` selects, so E = 0 in the stored tile, the row sum and the column sum wherever the row or the column
// is outside V_p -- by a select on the byte, never by value.  nce_multi_sums_kernel serves unchanged (a zero adds nothing).
// nce_multi_pair_coef_kernel counts every n_p from pres_all with integers and writes pair_coef[p] = 0.5 / n_p / P' (float64,
// rounded once; 0 for an empty pair; P' = the pairs that have a row): nothing is read on the host.  The masked finalize kernel
// gives a row outside V_p u = 0, ediag = 0 and a loss row of 0 and a column outside V_p v = 0 -- no log of an empty sum, no 1 / 0;
// the masked weights kernel takes coef from pair_coef[blockIdx.y] and applies the partner term to the rows of V_p alone.  The
// gradient products (nce_multi_product_kernel), nce_dtemp_kernel and nce_multi_finish_kernel are reused as they are: an excluded
// weight is a zero, and the caller's normalised rows hold zeros in the absent slots (aecf_l2norm_masked_forward), so 0 * key = 0.
// No K loop is skipped: a masked pair costs a full pair (a compacting form is not built).
//
// Multi-view InfoNCE with a temperature and a weight per pair (aecf_nce_multi_pp_pair_coef / _pass1 / _loss / _grads) is either form
// above (presence bytes given or NULL) with temp [P] and pair_coef [P] in place of one T and one coef.  The logits pass is
// nce_multi_pp_logits_kernel -- nce_multi_logits_kernel with p.temp advanced by the pair, so scale2 / shift2 are the pair's; equal
// bits of T give the bits of the one-temperature pass.  nce_multi_pp_pair_coef_kernel normalises the weights over the pairs that
// have a row (0.5 / n_p / (W / w_p), float64, rounded once: equal weights give 0.5 / n_p / P' to the bit; zeros by select, no
// 0 / 0); finalize and weights kernels of their own read temp[pair] and pair_coef[pair].  W_p carries coef_p / T_p, so the gradient
// products and the slab sum are reused as they are, da in its plain EPI_OUT form: dT cannot come from it, because its K loop has
// summed over every partner block of a view.  dT per pair instead: where the temperatures want a gradient the logits pass runs
// EPI_EXP_DTS / EPI_EXP_MASK_S, which sweep the float32 accumulators once more IN FRONT of the E sweep and leave partials of
// RS_i = sum_j E_ij (s_ij - 1) and CS_j = sum_i E_ij (s_ij - 1) laid out like the partials of E (E the float32 exponential, excluded
// elements by the same selects); nce_multi_sums_kernel reduces them in a second launch, the finalize kernel keeps s_ii - 1, and
// nce_multi_pp_dtemp_kernel (one block per pair, fixed order) forms
//   dL/dT_p = -(coef_p upstream / T_p^2) [ sum_i RS_i / l_i + sum_j CS_j / c_j - 2 sum_i (s_ii - 1) ]
// with c the all-reduced column sums: a rank's local column partials times the global 1 / c, so the ranks' shares add up to the
// gradient with no further exchange.  Nothing is recovered from the stored bf16 E.
//
// Symmetric InfoNCE with a key queue (aecf_nce_queue_pass1 / _loss / _grads, aecf_key_queue_push) is NT-Xent's arrangement with the
// two extra blocks taken against STORED keys of past steps: X = a_loc . b_all^T unchanged (EPI_EXP_DT), U = a_loc . Qb^T and W = b_loc .
// Qa^T over two ring buffers [q_cap, d] of which slots 0 .. V - 1 hold keys, V a DEVICE int64.  EPI_EXP_Q is EPI_EXP_SELF's E loop
// and row partials with `column < V` where that has the excluded band: V is read once per block in front of the first operand copy;
// a tile wholly at or above it stores zeros and ends on a block-uniform branch without a K-step, a tile wholly below it runs the
// unmasked loop, the tile V crosses selects per column -- by index, never by value: what a stale slot holds reaches no sum, a
// bit-identical twin of a partner below V counts.  Da = lX + lU, Db = the ranks' cX plus lW on the owner's range
// (ntx_combine_kernel), finalize and weights unchanged (a queue block has no partner element: its weights pass runs with rows =
// 0).  The queues take no gradient, so four products: d a_loc one float32 sum over the slabs of W_X b_all with those of W_U Qb
// behind them, d b_loc = W_W Qa, d b_all = W_X^T a_loc.  The products run over all q_cap slots with an exact-zero weight above V
// (the cost follows q_cap, not V; the slots must hold finite rows).  The ring buffer keeps (cursor, valid) on the device: a copy
// kernel that reads the old cursor, a one-thread launch behind it that bumps both -- no host read, no atomics, capturable.
//
// The supervised contrastive loss with a key queue (aecf_supcon_queue_pass1 / _loss / _grads, aecf_key_queue_push_labeled) joins the
// two: the three blocks above with the label statistics of the pooled supervised form.  X runs EPI_SUP unchanged; U and W run
// EPI_SUP_Q -- EPI_EXP_Q's count, dead tile, unmasked tile and crossed tile, plus the ROW half of the label search against ONE ring
// of stored labels Ql [q_cap] (slot s of Qa, Qb and Ql is the same past row).  A slot at or above V is no key and no positive by
// its index: it gets the 32-bit key no row has, and its label is never read.  A stored key is nobody's partner and nobody's self.
// sup_sums_kernel (row blocks alone), sup_pool_combine_kernel and sup_finalize_kernel serve unchanged on (Da, ka, sa) = X's + U's
// and (Db, kb, sb) = the ranks' column statistics of X plus W's on the owner's range: one all-reduce of [3][cols].  W_X is
// sup_weights_kernel<false>, W_U and W_W its QUEUE variant (m = [j < V] & label match, V from the device; v = rnc = 0; W with u, rn
// gathered at off + i).  The four products, the slab sum and the dT reduction are those of the key-queue InfoNCE.  The label ring is
// written by a copy kernel of its own between the key copy and the bump, from the cursor the push found.
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
       EPI_SETS_OV_SELF = 14, EPI_SETS_JAC_SELF = 15, EPI_EXP_MASK = 16, EPI_EXP_DTS = 17, EPI_EXP_MASK_S = 18, EPI_EXP_Q = 19,
       EPI_SUP_Q = 20 };
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
// EPI_EXP_MASK (multi-view InfoNCE with missing views, logits pass): EPI_EXP_DT with E = 0 -- in the stored tile, the row sum and
// the column sum -- wherever the row or the column lacks a view of the block's pair: pres_row / pres_col hold one byte per row /
// column (bit v = view v present), pres_need the two bits of the pair.  Excluded by a select on the byte, never by value.  A block
// whose 256 rows and 256 columns all hold both views runs EPI_EXP_DT's path; the others take the branch of the ragged edge.
// EPI_EXP_DTS / EPI_EXP_MASK_S (multi-view InfoNCE with a temperature per pair that wants its gradient, logits pass): EPI_EXP_DT /
// EPI_EXP_MASK to the bit, then a second sweep over the accumulators that leaves the float32 sums of E_ij (s_ij - 1) per row and
// per column of the tile in rowsx_part / colsx_part (laid out like rowsum_part / colsum_part): the dT sums of that pair.
constexpr bool epi_is_mask(int epi) { return epi == EPI_EXP_MASK || epi == EPI_EXP_MASK_S; }
constexpr bool epi_has_ts(int epi) { return epi == EPI_EXP_DTS || epi == EPI_EXP_MASK_S; }
// EPI_EXP_Q (InfoNCE with a key queue, the blocks of local rows against stored keys): EPI_EXP_SELF's E loop and row partials over
// the n_valid slots of a ring buffer of which only columns 0 .. *q_valid - 1 hold keys (q_valid: a DEVICE int64, handed over in
// q_count and read once per block).  A column at or above it is E = 0 in the stored tile and in the row sum BY INDEX; a tile wholly
// below it runs the unmasked loop, a tile wholly at or above it stores zeros without running its K loop, and only the tile the
// count crosses pays for the per-column test.  No column sums or partials of any kind.
// EPI_SUP_Q (supervised contrastive loss with a key queue, the same two blocks): EPI_EXP_Q's arrangement to the letter -- the count
// in q_count, the dead tile, the unmasked tile, the crossed tile -- plus the ROW half of EPI_SUP's label search as EPI_SUP_SELF has
// it, against the ring of stored labels in lab_col: rowcnt_part / rowsx_part get the count and the float32 raw-score sum of the
// slots below the count whose label is the row's.  No partner and no self: a stored key is nobody's.
constexpr bool epi_is_queue(int epi) { return epi == EPI_EXP_Q || epi == EPI_SUP_Q; }
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
    // EPI_EXP_MASK (also reads temp / min_temp and writes E and its sums as EPI_EXP_DT)
    const unsigned char* pres_row;      // [m_valid]  presence byte of output row i (bit v: view v present)
    const unsigned char* pres_col;      // [n_valid]  presence byte of output column j
    unsigned int pres_need;             // the bits a row and a column must both hold: the two views of the pair
    // EPI_EXP_Q / EPI_SUP_Q (also read temp / min_temp; EPI_SUP_Q also lab_row / lab_col and writes rowcnt_part / rowsx_part)
    const long long* q_count;           // DEVICE int64: columns 0 .. *q_count - 1 hold keys (read once per block)
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

// nce_gemm_kernel and the multi-view kernels below share their body as text (aecf_nce_gemm_body.h says why).
//
// The segments of a multi-view gradient product (MULTI): K runs through the partner blocks of one view, seg_steps K-steps each.
// Field s of `fields` (8 bits) names segment s: bits 0..4 the pair whose weights block is the m operand (a_stride bytes apart
// in the workspace), bits 5..7 the view whose rows are the n operand (view_bytes apart inside a row of x).
struct NceSegs {
    unsigned long long fields;
    int seg_steps;
    int64_t a_stride;
    unsigned int view_bytes;
};

template <int AM, int BM, int EPI, int MAP>
__global__ __launch_bounds__(512, 2) void nce_gemm_kernel(NceGemmArgs p) {
    constexpr bool MULTI = false;
    const unsigned int vblock = blockIdx.x;
    const NceSegs ms = {};
#include "aecf_nce_gemm_body.h"
}

// ---- multi-view InfoNCE: all pair blocks in one launch (include/aecf_hip.h, "multi-view InfoNCE") ----------------------------
//
// The logits pass of P pairs: block b works on pair b / blocks_per_pair, tile b % blocks_per_pair of that pair's own MAP_2D
// map (blocks_per_pair is a multiple of 8, so a tile keeps the XCD it has in a launch of its own).  The pair table supplies the
// two operand origins inside the rows of x; E and the partials of pair p lie p strides behind those of pair 0.  Everything
// else is the kernel above.
constexpr int MV_MAX_VIEWS = 8, MV_MAX_PAIRS = 28;

struct NceMultiLogits {
    unsigned char m[MV_MAX_PAIRS], n[MV_MAX_PAIRS];     // pair p = (view m[p]: the local rows, view n[p]: the gathered keys)
    unsigned int blocks_per_pair, view_bytes;
    int64_t e_stride, rowsum_stride, colsum_stride;     // elements
};

template <int EPI>
__global__ __launch_bounds__(512, 2) void nce_multi_logits_kernel(NceGemmArgs p, NceMultiLogits mv) {
    const unsigned int pair = blockIdx.x / mv.blocks_per_pair;
    p.a += mv.m[pair] * mv.view_bytes;
    p.b += mv.n[pair] * mv.view_bytes;
    p.e += pair * mv.e_stride;
    p.rowsum_part += pair * mv.rowsum_stride;
    p.colsum_part += pair * mv.colsum_stride;
    if (EPI == EPI_EXP_MASK) p.pres_need = (1u << mv.m[pair]) | (1u << mv.n[pair]);
    constexpr int AM = OP_ROW, BM = OP_ROW, MAP = MAP_2D;
    constexpr bool MULTI = false;
    const unsigned int vblock = blockIdx.x - pair * mv.blocks_per_pair;
    const NceSegs ms = {};
#include "aecf_nce_gemm_body.h"
}

// The logits pass with a temperature PER PAIR (aecf_nce_multi_pp_*): nce_multi_logits_kernel with p.temp advanced to the pair's
// own element, so the epilogue derives scale2 / shift2 from that pair's T -- equal bits of T give the bits of the kernel above.
// EPI_EXP_DT / EPI_EXP_MASK: nothing else.  EPI_EXP_DTS / EPI_EXP_MASK_S: the partials of the dT sums too, pair p's behind pair 0's
// by the strides of the partials of E.  A kernel of its own: the one above keeps its code.
template <int EPI>
__global__ __launch_bounds__(512, 2) void nce_multi_pp_logits_kernel(NceGemmArgs p, NceMultiLogits mv) {
    const unsigned int pair = blockIdx.x / mv.blocks_per_pair;
    p.a += mv.m[pair] * mv.view_bytes;
    p.b += mv.n[pair] * mv.view_bytes;
    p.e += pair * mv.e_stride;
    p.rowsum_part += pair * mv.rowsum_stride;
    p.colsum_part += pair * mv.colsum_stride;
    p.temp += pair;
    if (epi_has_ts(EPI)) {
        p.rowsx_part += pair * mv.rowsum_stride;
        p.colsx_part += pair * mv.colsum_stride;
    }
    if (epi_is_mask(EPI)) p.pres_need = (1u << mv.m[pair]) | (1u << mv.n[pair]);
    constexpr int AM = OP_ROW, BM = OP_ROW, MAP = MAP_2D;
    constexpr bool MULTI = false;
    const unsigned int vblock = blockIdx.x - pair * mv.blocks_per_pair;
    const NceSegs ms = {};
#include "aecf_nce_gemm_body.h"
}

// A gradient product of every view that has the role, one launch: block b works on slot b / blocks_per_view (a view with at
// least one pair in the role) and walks the K ranges of ALL its partner blocks, so an output element is one float32 sum.
struct NceMultiProduct {
    unsigned long long fields[MV_MAX_VIEWS];            // NceSegs::fields of the slot
    int n_segs[MV_MAX_VIEWS];
    int out_view[MV_MAX_VIEWS];                         // the view whose gradient the slot forms
    unsigned int blocks_per_view, view_bytes;
    int seg_steps, out_elem_bytes;
    int64_t a_stride, tdot_stride;
};

template <int AM, int BM, int EPI, int MAP>
__global__ __launch_bounds__(512, 2) void nce_multi_product_kernel(NceGemmArgs p, NceMultiProduct mv) {
    const unsigned int slot = blockIdx.x / mv.blocks_per_view;
    const int view = mv.out_view[slot];
    p.k_steps = mv.n_segs[slot] * mv.seg_steps;
    p.steps_per_split = (p.k_steps + p.splits - 1) / p.splits;
    p.out = reinterpret_cast<char*>(p.out) + (int64_t)view * p.n_valid * mv.out_elem_bytes;
    if (EPI == EPI_OUT_TD) {
        p.tdot_src += (int64_t)view * p.n_valid;
        p.tdot_part += slot * mv.tdot_stride;
    }
    const NceSegs ms = {mv.fields[slot], mv.seg_steps, mv.a_stride, mv.view_bytes};
    constexpr bool MULTI = true;
    const unsigned int vblock = blockIdx.x - slot * mv.blocks_per_view;
#include "aecf_nce_gemm_body.h"
}

// ---- small kernels around the GEMMs ------------------------------------------------------------------------------------

// l[i] = sum over the column tiles' partials, c[j] = sum over the row tiles' (fixed order: four strided partial sums per
// element, added in order).  Block = 64 elements x 4 parts.
__device__ __forceinline__ void nce_sums_body(const float* rowsum_part, const float* colsum_part, int m_tiles, int n_tiles,
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

__global__ __launch_bounds__(256) void nce_sums_kernel(const float* rowsum_part, const float* colsum_part, int m_tiles, int n_tiles,
                                                       int64_t rows, int64_t cols, float* l, float* c) {
    nce_sums_body(rowsum_part, colsum_part, m_tiles, n_tiles, rows, cols, l, c);
}

// multi-view: the sums of pair blockIdx.y, in the order nce_sums_kernel has; l [P][Rp], c [P][cols]
__global__ __launch_bounds__(256) void nce_multi_sums_kernel(const float* rowsum_part, const float* colsum_part, int m_tiles,
                                                             int n_tiles, int64_t rows, int64_t cols, float* l, float* c) {
    const int64_t pair = blockIdx.y, Rp = (int64_t)m_tiles * BT, Cp = (int64_t)n_tiles * BT;
    nce_sums_body(rowsum_part + pair * n_tiles * Rp, colsum_part + pair * m_tiles * Cp, m_tiles, n_tiles, rows, cols, l + pair * Rp,
                  c + pair * cols);
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

// multi-view: nce_finalize_kernel<true> (sym, no rider) for pair blockIdx.y = (view m, view n) of the table, operation for
// operation; the rows of a view lie `views` d apart inside x.  l, u, ediag [P][Rp], c [P][cols], v [P][Cp], loss_rows [P][rows]
struct NceMultiFin {
    unsigned char m[MV_MAX_PAIRS], n[MV_MAX_PAIRS];
    int views;
};
__global__ __launch_bounds__(256) void nce_multi_finalize_kernel(NceFinArgs p, NceMultiFin mv) {
    const int64_t pair = blockIdx.y, ld = (int64_t)mv.views * p.d;
    const float inv_temp = nce_dev_inv_temp(p.temp, p.min_temp);
    const float* c = p.c + pair * p.cols;
    const int lane = lane_id();
    const int64_t i = (int64_t)blockIdx.x * 4 + wave_id();
    if (i < p.rows) {
        const unsigned short* ap = p.a + i * ld + mv.m[pair] * p.d;
        const unsigned short* bp = p.b + (p.row_offset + i) * ld + mv.n[pair] * p.d;
        float dot = 0.f;
        for (int k = lane; k < p.d; k += 64) dot = fmaf(Tr<BF16>::to_f32(ap[k]), Tr<BF16>::to_f32(bp[k]), dot);
        dot = reduce_wave(dot);
        if (lane == 0) {
            const float li = p.l[pair * p.Rp + i];
            p.u[pair * p.Rp + i] = 1.0f / li;
            p.ediag[pair * p.Rp + i] = __builtin_amdgcn_exp2f((dot - 1.0f) * inv_temp * 1.4426950408889634f);
            float loss = nce_row_term(li, inv_temp, dot);
            loss += nce_col_term(c[p.row_offset + i], inv_temp, dot);
            p.loss_rows[pair * p.rows + i] = loss;
        }
    } else if (i < p.Rp) {
        if (lane == 0) p.u[pair * p.Rp + i] = 0.f;
    }
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < p.Cp; j += (int64_t)gridDim.x * 256)
        p.v[pair * p.Cp + j] = j < p.cols ? 1.0f / c[j] : 0.f;
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

// multi-view: the weights of pair blockIdx.y over its own E block; u, ediag [P][Rp], v [P][Cp]
__global__ __launch_bounds__(256) void nce_multi_weights_kernel(unsigned short* e, int64_t e_tiles, int64_t m_tiles, const float* u,
                                                                const float* v, const float* ediag, int64_t rows, int64_t row_offset,
                                                                float coef, const float* upstream, const float* temp, float min_temp) {
    const int64_t pair = blockIdx.y, Rp = m_tiles * BT, Cp = e_tiles * 64;
    nce_weights_body(e + pair * Rp * Cp, e_tiles, m_tiles, u + pair * Rp, v + pair * Cp, ediag + pair * Rp, rows, row_offset,
                     coef * nce_dev_inv_temp(temp, min_temp), 2.0f, upstream);
}

// ---- multi-view InfoNCE with missing views: the small kernels around the EPI_EXP_MASK logits pass.  A presence byte per row
// (bit v: view v present); pair p = (m, n) counts the rows that hold both bits -- V_p, n_p of them over all ranks.

// pair_coef[p] = 0.5 / n_p / P' in float32 (formed in float64 and rounded once, as the host forms the unmasked coef), 0 where
// n_p = 0; P' = the pairs with n_p > 0.  One block: an integer histogram of the 256 byte values of pres_all (integer atomics in
// LDS: the counts do not depend on the order), then thread p sums the bins that hold both bits of pair p.
__global__ __launch_bounds__(256) void nce_multi_pair_coef_kernel(const unsigned char* pres_all, int64_t cols, NceMultiFin mv, int pairs,
                                                                  float* pair_coef) {
    __shared__ int hist[256];
    __shared__ int n_p[MV_MAX_PAIRS];
    hist[threadIdx.x] = 0;
    __syncthreads();
    for (int64_t j = threadIdx.x; j < cols; j += 256) atomicAdd(&hist[pres_all[j]], 1);
    __syncthreads();
    if ((int)threadIdx.x < pairs) {
        const unsigned int need = (1u << mv.m[threadIdx.x]) | (1u << mv.n[threadIdx.x]);
        int n = 0;
        for (unsigned int b = 0; b < 256; ++b) n += (b & need) == need ? hist[b] : 0;
        n_p[threadIdx.x] = n;
    }
    __syncthreads();
    if ((int)threadIdx.x < pairs) {
        int live = 0;
        for (int q = 0; q < pairs; ++q) live += n_p[q] > 0 ? 1 : 0;
        const int n = n_p[threadIdx.x];
        pair_coef[threadIdx.x] = n > 0 ? (float)(0.5 / (double)n / (double)live) : 0.f;
    }
}

// nce_multi_finalize_kernel with the presence bytes: a local row outside V_p gets u = 0, ediag = 0 and a loss row of 0 (no log of
// an empty sum, no 1 / 0, and its slots of x are not read); a column outside V_p gets v = 0.  A row of V_p is the unmasked kernel's,
// operation for operation.  pres_loc [rows] by the local row, pres_all [cols] by the global column.
__global__ __launch_bounds__(256) void nce_multi_masked_finalize_kernel(NceFinArgs p, NceMultiFin mv, const unsigned char* pres_loc,
                                                                        const unsigned char* pres_all) {
    const int64_t pair = blockIdx.y, ld = (int64_t)mv.views * p.d;
    const unsigned int need = (1u << mv.m[pair]) | (1u << mv.n[pair]);
    const float inv_temp = nce_dev_inv_temp(p.temp, p.min_temp);
    const float* c = p.c + pair * p.cols;
    const int lane = lane_id();
    const int64_t i = (int64_t)blockIdx.x * 4 + wave_id();
    if (i < p.rows && (pres_loc[i] & need) == need) {
        const unsigned short* ap = p.a + i * ld + mv.m[pair] * p.d;
        const unsigned short* bp = p.b + (p.row_offset + i) * ld + mv.n[pair] * p.d;
        float dot = 0.f;
        for (int k = lane; k < p.d; k += 64) dot = fmaf(Tr<BF16>::to_f32(ap[k]), Tr<BF16>::to_f32(bp[k]), dot);
        dot = reduce_wave(dot);
        if (lane == 0) {
            const float li = p.l[pair * p.Rp + i];
            p.u[pair * p.Rp + i] = 1.0f / li;
            p.ediag[pair * p.Rp + i] = __builtin_amdgcn_exp2f((dot - 1.0f) * inv_temp * 1.4426950408889634f);
            float loss = nce_row_term(li, inv_temp, dot);
            loss += nce_col_term(c[p.row_offset + i], inv_temp, dot);
            p.loss_rows[pair * p.rows + i] = loss;
        }
    } else if (i < p.Rp) {
        if (lane == 0) {
            p.u[pair * p.Rp + i] = 0.f;
            p.ediag[pair * p.Rp + i] = 0.f;
            if (i < p.rows) p.loss_rows[pair * p.rows + i] = 0.f;
        }
    }
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < p.Cp; j += (int64_t)gridDim.x * 256)
        p.v[pair * p.Cp + j] = (j < p.cols && (pres_all[j] & need) == need) ? 1.0f / c[j] : 0.f;
}

// nce_multi_weights_kernel with the presence bytes: coef of pair blockIdx.y from pair_coef (0 for an empty pair: its block comes
// out as zeros), and the partner term -2 [j = off + i] for the rows of V_p alone -- elsewhere E = 0 and u = 0 give W = 0.  The
// arithmetic of a row of V_p is nce_weights_body's.
__global__ __launch_bounds__(256) void nce_multi_masked_weights_kernel(unsigned short* e, int64_t e_tiles, int64_t m_tiles, const float* u,
                                                                       const float* v, const float* ediag, int64_t rows,
                                                                       int64_t row_offset, const float* pair_coef, const NceMultiFin mv,
                                                                       const unsigned char* pres_loc, const float* upstream,
                                                                       const float* temp, float min_temp) {
    const int64_t pair = blockIdx.y, Rp = m_tiles * BT, Cp = e_tiles * 64;
    const unsigned int need = (1u << mv.m[pair]) | (1u << mv.n[pair]);
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;         // 16-byte chunk: 2048 per tile, 8 per tile row
    if (id >= m_tiles * e_tiles * 2048) return;
    e += pair * Rp * Cp; u += pair * Rp; v += pair * Cp; ediag += pair * Rp;
    float ct = pair_coef[pair] * nce_dev_inv_temp(temp, min_temp);
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
    const bool in_pair = i < rows && (pres_loc[i < rows ? i : 0] & need) == need;
    const int64_t jp = in_pair ? row_offset + i - j0 : -1;
    if (upstream) ct *= upstream[0];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        float wv = x[k] * (ui + vv[k]);
        if (jp == k) wv = ediag[i] * (ui + vv[k]) - 2.0f;
        x[k] = ct * wv;
    }
    *ptr = Tr<BF16>::pack(x);
}

// ---- multi-view InfoNCE with a temperature and a weight per pair (aecf_nce_multi_pp_*): the small kernels.  They have bodies of
// their own; the kernels of the one-temperature forms above keep their code.

// pair_coef[p] = 0.5 / n_p * w_p / W in float32, W = the sum of the weights of the pairs with n_p > 0 (pair order, float64); formed
// as 0.5 / n_p / (W / w_p) in float64 and rounded once, so equal weights give the 0.5 / n_p / P' of nce_multi_pair_coef_kernel to
// the bit.  0 where n_p = 0, where w_p = 0 and where W = 0 (no 0 / 0).  pres_all NULL: every row holds every view, n_p = cols.
// weights NULL: every w_p = 1.  One block; the counts are nce_multi_pair_coef_kernel's integer histogram.
__global__ __launch_bounds__(256) void nce_multi_pp_pair_coef_kernel(const unsigned char* pres_all, int64_t cols, NceMultiFin mv, int pairs,
                                                                     const float* weights, float* pair_coef) {
    __shared__ int hist[256];
    __shared__ int n_p[MV_MAX_PAIRS];
    hist[threadIdx.x] = 0;
    __syncthreads();
    if (pres_all)
        for (int64_t j = threadIdx.x; j < cols; j += 256) atomicAdd(&hist[pres_all[j]], 1);
    __syncthreads();
    if ((int)threadIdx.x < pairs) {
        const unsigned int need = (1u << mv.m[threadIdx.x]) | (1u << mv.n[threadIdx.x]);
        int n = (int)cols;
        if (pres_all) {
            n = 0;
            for (unsigned int b = 0; b < 256; ++b) n += (b & need) == need ? hist[b] : 0;
        }
        n_p[threadIdx.x] = n;
    }
    __syncthreads();
    if ((int)threadIdx.x < pairs) {
        double total = 0.0;
        for (int q = 0; q < pairs; ++q) total += n_p[q] > 0 ? (weights ? (double)weights[q] : 1.0) : 0.0;
        const int n = n_p[threadIdx.x];
        const double wp = weights ? (double)weights[threadIdx.x] : 1.0;
        pair_coef[threadIdx.x] = (n > 0 && wp > 0.0 && total > 0.0) ? (float)(0.5 / (double)n / (total / wp)) : 0.f;
    }
}

// nce_multi_finalize_kernel / nce_multi_masked_finalize_kernel (pres_loc NULL / not) at the pair's own temperature temp[pair],
// operation for operation; sdiag [P][Rp] (may be NULL) takes s_ii - 1 of every row of the pair in float32, 0 outside V_p: the
// positives' term of the dT sums.
__global__ __launch_bounds__(256) void nce_multi_pp_finalize_kernel(NceFinArgs p, NceMultiFin mv, const unsigned char* pres_loc,
                                                                    const unsigned char* pres_all, float* sdiag) {
    const int64_t pair = blockIdx.y, ld = (int64_t)mv.views * p.d;
    const unsigned int need = (1u << mv.m[pair]) | (1u << mv.n[pair]);
    const float inv_temp = nce_dev_inv_temp(p.temp + pair, p.min_temp);
    const float* c = p.c + pair * p.cols;
    const int lane = lane_id();
    const int64_t i = (int64_t)blockIdx.x * 4 + wave_id();
    if (i < p.rows && (!pres_loc || (pres_loc[i] & need) == need)) {
        const unsigned short* ap = p.a + i * ld + mv.m[pair] * p.d;
        const unsigned short* bp = p.b + (p.row_offset + i) * ld + mv.n[pair] * p.d;
        float dot = 0.f;
        for (int k = lane; k < p.d; k += 64) dot = fmaf(Tr<BF16>::to_f32(ap[k]), Tr<BF16>::to_f32(bp[k]), dot);
        dot = reduce_wave(dot);
        if (lane == 0) {
            const float li = p.l[pair * p.Rp + i];
            p.u[pair * p.Rp + i] = 1.0f / li;
            p.ediag[pair * p.Rp + i] = __builtin_amdgcn_exp2f((dot - 1.0f) * inv_temp * 1.4426950408889634f);
            float loss = nce_row_term(li, inv_temp, dot);
            loss += nce_col_term(c[p.row_offset + i], inv_temp, dot);
            p.loss_rows[pair * p.rows + i] = loss;
            if (sdiag) sdiag[pair * p.Rp + i] = dot - 1.0f;
        }
    } else if (i < p.Rp) {
        if (lane == 0) {
            p.u[pair * p.Rp + i] = 0.f;
            p.ediag[pair * p.Rp + i] = 0.f;
            if (i < p.rows) p.loss_rows[pair * p.rows + i] = 0.f;
            if (sdiag) sdiag[pair * p.Rp + i] = 0.f;
        }
    }
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < p.Cp; j += (int64_t)gridDim.x * 256)
        p.v[pair * p.Cp + j] = (j < p.cols && (!pres_all || (pres_all[j] & need) == need)) ? 1.0f / c[j] : 0.f;
}

// nce_multi_masked_weights_kernel at the pair's own temperature: ct = pair_coef[pair] / max(temp[pair], min_temp), the partner term
// for the rows of V_p alone (pres_loc NULL: every row).  The arithmetic of an element is nce_weights_body's.
__global__ __launch_bounds__(256) void nce_multi_pp_weights_kernel(unsigned short* e, int64_t e_tiles, int64_t m_tiles, const float* u,
                                                                   const float* v, const float* ediag, int64_t rows, int64_t row_offset,
                                                                   const float* pair_coef, const NceMultiFin mv,
                                                                   const unsigned char* pres_loc, const float* upstream,
                                                                   const float* temp, float min_temp) {
    const int64_t pair = blockIdx.y, Rp = m_tiles * BT, Cp = e_tiles * 64;
    const unsigned int need = (1u << mv.m[pair]) | (1u << mv.n[pair]);
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;         // 16-byte chunk: 2048 per tile, 8 per tile row
    if (id >= m_tiles * e_tiles * 2048) return;
    e += pair * Rp * Cp; u += pair * Rp; v += pair * Cp; ediag += pair * Rp;
    float ct = pair_coef[pair] * nce_dev_inv_temp(temp + pair, min_temp);
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
    const bool in_pair = i < rows && (!pres_loc || (pres_loc[i] & need) == need);
    const int64_t jp = in_pair ? row_offset + i - j0 : -1;
    if (upstream) ct *= upstream[0];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        float wv = x[k] * (ui + vv[k]);
        if (jp == k) wv = ediag[i] * (ui + vv[k]) - 2.0f;
        x[k] = ct * wv;
    }
    *ptr = Tr<BF16>::pack(x);
}

// d_temp[p] for pair blockIdx.x, this rank's share:
//   dL/dT_p = -(coef_p upstream / Tc_p^2) [ sum_i u_i RS_i + sum_j v_j CS_j - 2 sum_i (s_ii - 1) ],   0 where temp[p] < min_temp
// RS [P][Rp] / CS [P][cols]: this rank's row / column sums of E (s - 1) (the reduced partials of EPI_EXP_DTS); u, sdiag [P][Rp],
// v [P][Cp] -- v from the all-reduced column sums.  Rows and columns outside the pair (padding, absent views) hold u = 0 / v = 0 and
// zero sums.  Every term float32, never the stored bf16 E.  Fixed order: 256 strided sums per term, then a fixed tree; a pair with
// coef_p = 0 is written as an exact 0 by a select.
__global__ __launch_bounds__(256) void nce_multi_pp_dtemp_kernel(const float* rs, const float* cs, const float* u, const float* v,
                                                                 const float* sdiag, int64_t rows, int64_t cols, int64_t Rp, int64_t Cp,
                                                                 const float* pair_coef, const float* upstream, const float* temp,
                                                                 float min_temp, float* d_temp) {
    __shared__ float red[3][256];
    const int64_t pair = blockIdx.x;
    rs += pair * Rp; u += pair * Rp; sdiag += pair * Rp; cs += pair * cols; v += pair * Cp;
    float sr = 0.f, sc = 0.f, sd = 0.f;
    for (int64_t i = threadIdx.x; i < rows; i += 256) {
        sr = fmaf(u[i], rs[i], sr);
        sd += sdiag[i];
    }
    for (int64_t j = threadIdx.x; j < cols; j += 256) sc = fmaf(v[j], cs[j], sc);
    red[0][threadIdx.x] = sr; red[1][threadIdx.x] = sc; red[2][threadIdx.x] = sd;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            red[0][threadIdx.x] += red[0][threadIdx.x + w];
            red[1][threadIdx.x] += red[1][threadIdx.x + w];
            red[2][threadIdx.x] += red[2][threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float tv = temp[pair], tc = fmaxf(tv, min_temp), coef = pair_coef[pair];
        float g = coef / (tc * tc);
        if (upstream) g *= upstream[0];
        const float sum = (red[0][0] + red[1][0]) - 2.0f * red[2][0];
        d_temp[pair] = (tv >= min_temp && coef != 0.f) ? -g * sum : 0.f;
    }
}

// multi-view: dx_loc = the fixed-order sum of the da slabs [splits][rows][views d] where the view has the a role and 0 where it has
// none (bit v of da_mask), rounded once; and the zeros of the views of dx_all [cols][views d] that have no b role (db_mask) --
// the db product stores the others itself.  One thread per 4 elements of dx_loc, then of dx_all.
__global__ __launch_bounds__(256) void nce_multi_finish_kernel(const float* slabs, int splits, int64_t rows, int64_t cols, int views, int d,
                                                               unsigned int da_mask, unsigned int db_mask, void* dx_loc, void* dx_all,
                                                               int out_bf16) {
    const int64_t pitch4 = (int64_t)views * d / 4, n_loc = rows * pitch4;
    int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= n_loc + cols * pitch4) return;
    const bool loc = id < n_loc;
    if (!loc) id -= n_loc;
    const int view = (int)((id % pitch4) * 4 / d);
    f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
    if (loc) {
        if ((da_mask >> view) & 1u) {
            s = *reinterpret_cast<const f32x4*>(slabs + 4 * id);
            for (int k = 1; k < splits; ++k) {
                const f32x4 t = *reinterpret_cast<const f32x4*>(slabs + (int64_t)k * 4 * n_loc + 4 * id);
                s[0] += t[0]; s[1] += t[1]; s[2] += t[2]; s[3] += t[3];
            }
        }
    } else if ((db_mask >> view) & 1u) {
        return;
    }
    void* out = loc ? dx_loc : dx_all;
    if (out_bf16) *reinterpret_cast<u32x2*>(reinterpret_cast<unsigned short*>(out) + 4 * id) = u32x2{pack_bf16x2(s[0], s[1]), pack_bf16x2(s[2], s[3])};
    else *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(out) + 4 * id) = s;
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
// QUEUE (blocks U and W of the supervised loss with a key queue; cols = the capacity, lab_col = the ring of stored labels): NO
// partner element and no self -- a stored key is nobody's -- and m = [j < *q_count] & the label match, the count read from the
// device (clamped into 0 .. cols; the label of a slot at or above it may be anything).  v and rnc are the vector of zeros as for
// SELF; ediag is not read.  A slot at or above the count holds E = 0 and m = 0: its weight is an exact zero.
template <bool SELF, bool QUEUE = false>
__global__ __launch_bounds__(256) void sup_weights_kernel(unsigned short* e, int64_t e_tiles, int64_t m_tiles, const float* u,
                                                          const float* v, const float* rn, const float* rnc, const float* ediag,
                                                          const long long* lab_row, const long long* lab_col, int64_t rows,
                                                          int64_t cols, int64_t row_offset, float coef, const float* upstream,
                                                          const float* temp, float min_temp, const long long* q_count) {
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
    const int64_t jp = (iok && !QUEUE) ? row_offset + i - j0 : -1;
    int64_t qv = cols;
    if (QUEUE) { const long long c = *q_count; qv = c < 0 ? 0 : (c > cols ? cols : c); }
    unsigned int mm = 0;                                        // bit k: element k is a positive (by label or the partner)
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int64_t j = j0 + k;
        const long long lck = lab_col[j < cols ? j : cols - 1];
        if (QUEUE) { if (iok && j < qv && sup_label_match(lr, lck)) mm |= 1u << k; }
        else if (SELF) { if (iok && j < cols && sup_label_match(lr, lck) && jp != k) mm |= 1u << k; }
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

// ---- multi-view InfoNCE: every pair of views (or every pair with one anchor view) of x [rows][views][d] (include/aecf_hip.h) ----

namespace {

// the pairs in the order of the definition: anchor < 0 every m < n, lexicographic; else (min(k, n), max(k, n)) for n != k, rising
struct MvPairs {
    int count;
    unsigned char m[MV_MAX_PAIRS], n[MV_MAX_PAIRS];
};

MvPairs mv_pairs(int views, int anchor) {
    MvPairs t = {};
    for (int m = 0; m < views; ++m)
        for (int n = anchor < 0 ? m + 1 : 0; n < views; ++n) {
            if (anchor >= 0 && (m != anchor || n == anchor)) continue;
            t.m[t.count] = (unsigned char)(m < n ? m : n);
            t.n[t.count] = (unsigned char)(m < n ? n : m);
            ++t.count;
        }
    return t;
}

// workspace carve of the multi-view form: the two-view arrays once per pair, pair after pair, and one set of slabs
struct MvWs {
    unsigned short* e;                  // [P][Rp][Cp] bf16, each block tiled as E
    float* rowsum_part;                 // [P][n_tiles][Rp]
    float* colsum_part;                 // [P][m_tiles][Cp]
    float* l;                           // [P][Rp]
    float* u;                           // [P][Rp]
    float* v;                           // [P][Cp]
    float* ediag;                       // [P][Rp]
    float* slabs;                       // [splits][rows][views][d]
    size_t bytes;
};

MvWs mv_carve(void* ws, int64_t rows, int64_t cols, int d, int views, int pairs) {
    const int64_t Rp = up256(rows), Cp = up256(cols);
    const int64_t mt = Rp / BT, nt = Cp / BT;
    const size_t P = (size_t)pairs;
    MvWs w;
    char* p = (char*)ws;
    size_t off = 0;
    auto take = [&](size_t n) { char* r = p + off; off += al256(n); return r; };
    w.e = (unsigned short*)take(P * Rp * Cp * 2);
    w.rowsum_part = (float*)take(P * nt * Rp * 4);
    w.colsum_part = (float*)take(P * mt * Cp * 4);
    w.l = (float*)take(P * Rp * 4);
    w.u = (float*)take(P * Rp * 4);
    w.v = (float*)take(P * Cp * 4);
    w.ediag = (float*)take(P * Rp * 4);
    w.slabs = (float*)take((size_t)da_splits(Rp, Cp, d) * rows * views * d * 4);
    w.bytes = off;
    return w;
}

// the per-pair form (aecf_nce_multi_pp_*): the carve above, then the arrays of the dT sums
struct MvPpWs {
    MvWs w;
    float* rowsx_part;                  // [P][n_tiles][Rp]  partials of the row sums of E (s - 1)
    float* colsx_part;                  // [P][m_tiles][Cp]  partials of the column sums
    float* rs;                          // [P][Rp]
    float* cs;                          // [P][cols]         this rank's
    float* sdiag;                       // [P][Rp]           s_ii - 1
    size_t bytes;
};

MvPpWs mv_pp_carve(void* ws, int64_t rows, int64_t cols, int d, int views, int pairs) {
    const int64_t Rp = up256(rows), Cp = up256(cols);
    const int64_t mt = Rp / BT, nt = Cp / BT;
    const size_t P = (size_t)pairs;
    MvPpWs o;
    o.w = mv_carve(ws, rows, cols, d, views, pairs);
    char* p = (char*)ws;
    size_t off = o.w.bytes;
    auto take = [&](size_t n) { char* r = p + off; off += al256(n); return r; };
    o.rowsx_part = (float*)take(P * nt * Rp * 4);
    o.colsx_part = (float*)take(P * mt * Cp * 4);
    o.rs = (float*)take(P * Rp * 4);
    o.cs = (float*)take(P * cols * 4);
    o.sdiag = (float*)take(P * Rp * 4);
    o.bytes = off;
    return o;
}

// the slots of one role: a view with at least one pair in it, and its partner blocks in pair order.  role_b false: the views
// that supply local rows (da: the partner is the pair's n view); true: the views that supply keys (db: the partner is its m view)
void mv_slots(const MvPairs& t, int views, bool role_b, NceMultiProduct& mv, int& slots, unsigned int& mask) {
    slots = 0;
    mask = 0;
    for (int v = 0; v < views; ++v) {
        unsigned long long f = 0;
        int k = 0;
        for (int p = 0; p < t.count; ++p)
            if ((role_b ? t.n[p] : t.m[p]) == v) f |= (unsigned long long)(p | ((role_b ? t.m[p] : t.n[p]) << 5)) << (8 * k++);
        if (!k) continue;
        mv.fields[slots] = f; mv.n_segs[slots] = k; mv.out_view[slots] = v;
        ++slots;
        mask |= 1u << v;
    }
}

template <int AM, int BM, int EPI, int MAP>
void launch_multi_product(const NceGemmArgs& a, const NceMultiProduct& mv, unsigned int blocks, hipStream_t s) {
    auto kern = nce_multi_product_kernel<AM, BM, EPI, MAP>;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * STAGE);
    kern<<<dim3(blocks), dim3(512), 2 * STAGE, s>>>(a, mv);
}

}  // namespace

bool nce_multi_supported(int d, float min_temperature, int64_t cols, int views, int anchor) {
    return nce_gemm_supported(0, d, min_temperature) && cols <= 0x7fffffff && views >= 2 && views <= MV_MAX_VIEWS && anchor >= -1 &&
           anchor < views;
}

size_t nce_multi_workspace_bytes(int64_t rows, int64_t cols, int d, int views, int anchor) {
    return mv_carve(nullptr, rows, cols, d, views, mv_pairs(views, anchor).count).bytes + 256;
}

size_t nce_multi_pp_workspace_bytes(int64_t rows, int64_t cols, int d, int views, int anchor) {
    return mv_pp_carve(nullptr, rows, cols, d, views, mv_pairs(views, anchor).count).bytes + 256;
}

namespace {
// pass 1 of all pairs: one logits launch, one sums launch; col_sums [P][cols] are this rank's.  pres_loc / pres_all non-NULL: the
// form with missing views (EPI_EXP_MASK); the sums kernel serves both -- an excluded element is an exact zero in every partial.
// per_pair: 0 one temperature (dt.t [1]); 1 a temperature per pair (dt.t [P], the workspace of nce_multi_pp_workspace_bytes); 2 that
// and the dT sums of every pair: the EPI_EXP_DTS / EPI_EXP_MASK_S instance and a second sums launch over its partials
void mv_pass1(int64_t rows, int64_t cols, int d, int views, int anchor, const NceDevTemp& dt, const void* x_loc, const void* x_all,
              const unsigned char* pres_loc, const unsigned char* pres_all, int per_pair, void* workspace, float* col_sums,
              hipStream_t s) {
    const MvPairs t = mv_pairs(views, anchor);
    const MvWs w = mv_carve(workspace, rows, cols, d, views, t.count);
    const int64_t Rp = up256(rows), Cp = up256(cols);
    LogitsLaunch L = logits_args(rows, cols, d, x_loc, x_all);
    NceGemmArgs& g = L.g;
    g.lda = g.ldb = 2u * (unsigned)d * (unsigned)views;             // the views lie side by side in a row of x
    g.a_sm = (int64_t)BT * g.lda;
    g.e = w.e; g.e_tiles = Cp / 64;
    g.rowsum_part = w.rowsum_part; g.colsum_part = w.colsum_part;
    g.temp = dt.t; g.min_temp = dt.min_t;
    NceMultiLogits mv = {};
    for (int p = 0; p < t.count; ++p) { mv.m[p] = t.m[p]; mv.n[p] = t.n[p]; }
    mv.blocks_per_pair = L.blocks; mv.view_bytes = 2u * (unsigned)d;
    mv.e_stride = Rp * Cp; mv.rowsum_stride = (int64_t)g.n_tiles * Rp; mv.colsum_stride = (int64_t)g.m_tiles * Cp;
    g.pres_row = pres_loc; g.pres_col = pres_all;
    auto kern = pres_loc ? nce_multi_logits_kernel<EPI_EXP_MASK> : nce_multi_logits_kernel<EPI_EXP_DT>;
    MvPpWs pw = {};
    if (per_pair) {
        pw = mv_pp_carve(workspace, rows, cols, d, views, t.count);
        g.rowsx_part = pw.rowsx_part; g.colsx_part = pw.colsx_part;
        if (per_pair == 2) kern = pres_loc ? nce_multi_pp_logits_kernel<EPI_EXP_MASK_S> : nce_multi_pp_logits_kernel<EPI_EXP_DTS>;
        else kern = pres_loc ? nce_multi_pp_logits_kernel<EPI_EXP_MASK> : nce_multi_pp_logits_kernel<EPI_EXP_DT>;
    }
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * STAGE);
    kern<<<dim3(L.blocks * (unsigned)t.count), dim3(512), 2 * STAGE, s>>>(g, mv);
    const dim3 sgrid((unsigned)((Rp + Cp) / 64), (unsigned)t.count);
    nce_multi_sums_kernel<<<sgrid, dim3(256), 0, s>>>(w.rowsum_part, w.colsum_part, g.m_tiles, g.n_tiles, rows, cols, w.l, col_sums);
    if (per_pair == 2)
        nce_multi_sums_kernel<<<sgrid, dim3(256), 0, s>>>(pw.rowsx_part, pw.colsx_part, g.m_tiles, g.n_tiles, rows, cols, pw.rs, pw.cs);
}
}  // namespace

void launch_nce_multi_pass1(int64_t rows, int64_t cols, int d, int views, int anchor, const NceDevTemp& dt, const void* x_loc,
                            const void* x_all, void* workspace, float* col_sums, hipStream_t s) {
    mv_pass1(rows, cols, d, views, anchor, dt, x_loc, x_all, nullptr, nullptr, 0, workspace, col_sums, s);
}

void launch_nce_multi_masked_pass1(int64_t rows, int64_t cols, int d, int views, int anchor, const NceDevTemp& dt, const void* x_loc,
                                   const void* x_all, const unsigned char* pres_loc, const unsigned char* pres_all, void* workspace,
                                   float* col_sums, hipStream_t s) {
    mv_pass1(rows, cols, d, views, anchor, dt, x_loc, x_all, pres_loc, pres_all, 0, workspace, col_sums, s);
}

void launch_nce_multi_pp_pass1(int64_t rows, int64_t cols, int d, int views, int anchor, const NceDevTemp& dt, const void* x_loc,
                               const void* x_all, const unsigned char* pres_loc, const unsigned char* pres_all, int with_dt,
                               void* workspace, float* col_sums, hipStream_t s) {
    mv_pass1(rows, cols, d, views, anchor, dt, x_loc, x_all, pres_loc, pres_all, with_dt ? 2 : 1, workspace, col_sums, s);
}

// pair_coef [P] of the per-pair form: the weights normalised over the pairs that have a row, on the device.  pres_all NULL: no
// view is missing; weights NULL: uniform
void launch_nce_multi_pp_pair_coef(int64_t cols, int views, int anchor, const unsigned char* pres_all, const float* weights,
                                   float* pair_coef, hipStream_t s) {
    const MvPairs t = mv_pairs(views, anchor);
    NceMultiFin mv = {};
    for (int p = 0; p < t.count; ++p) { mv.m[p] = t.m[p]; mv.n[p] = t.n[p]; }
    mv.views = views;
    nce_multi_pp_pair_coef_kernel<<<dim3(1), dim3(256), 0, s>>>(pres_all, cols, mv, t.count, weights, pair_coef);
}

// pair_coef [P] of the form with missing views from the gathered presence bytes: one small launch, nothing read on the host
void launch_nce_multi_pair_coef(int64_t cols, int views, int anchor, const unsigned char* pres_all, float* pair_coef, hipStream_t s) {
    const MvPairs t = mv_pairs(views, anchor);
    NceMultiFin mv = {};
    for (int p = 0; p < t.count; ++p) { mv.m[p] = t.m[p]; mv.n[p] = t.n[p]; }
    mv.views = views;
    nce_multi_pair_coef_kernel<<<dim3(1), dim3(256), 0, s>>>(pres_all, cols, mv, t.count, pair_coef);
}

namespace {
// normalisers and loss rows [P][rows] of all pairs in one launch; col_sums [P][cols]: all ranks' sums
void mv_loss(int64_t rows, int64_t cols, int64_t row_offset, int d, int views, int anchor, const NceDevTemp& dt, const void* x_loc,
             const void* x_all, const unsigned char* pres_loc, const unsigned char* pres_all, bool per_pair, const float* col_sums,
             void* workspace, float* loss_rows, hipStream_t s) {
    const MvPairs t = mv_pairs(views, anchor);
    const MvWs w = mv_carve(workspace, rows, cols, d, views, t.count);
    const int64_t Rp = up256(rows), Cp = up256(cols);
    NceFinArgs f = {};
    f.a = (const unsigned short*)x_loc; f.b = (const unsigned short*)x_all; f.l = w.l; f.c = col_sums;
    f.u = w.u; f.v = w.v; f.ediag = w.ediag; f.loss_rows = loss_rows; f.rows = rows; f.cols = cols; f.row_offset = row_offset; f.Rp = Rp; f.Cp = Cp;
    f.d = d; f.sym = 1; f.temp = dt.t; f.min_temp = dt.min_t;
    NceMultiFin mv = {};
    for (int p = 0; p < t.count; ++p) { mv.m[p] = t.m[p]; mv.n[p] = t.n[p]; }
    mv.views = views;
    const dim3 grid((unsigned)((Rp + 3) / 4), (unsigned)t.count);
    if (per_pair)       // dt.t [P]; s_ii - 1 of every row goes to the per-pair workspace for the dT sums
        nce_multi_pp_finalize_kernel<<<grid, dim3(256), 0, s>>>(f, mv, pres_loc, pres_all,
                                                                mv_pp_carve(workspace, rows, cols, d, views, t.count).sdiag);
    else if (pres_loc) nce_multi_masked_finalize_kernel<<<grid, dim3(256), 0, s>>>(f, mv, pres_loc, pres_all);
    else nce_multi_finalize_kernel<<<grid, dim3(256), 0, s>>>(f, mv);
}
}  // namespace

void launch_nce_multi_loss(int64_t rows, int64_t cols, int64_t row_offset, int d, int views, int anchor, const NceDevTemp& dt,
                           const void* x_loc, const void* x_all, const float* col_sums, void* workspace, float* loss_rows,
                           hipStream_t s) {
    mv_loss(rows, cols, row_offset, d, views, anchor, dt, x_loc, x_all, nullptr, nullptr, false, col_sums, workspace, loss_rows, s);
}

void launch_nce_multi_masked_loss(int64_t rows, int64_t cols, int64_t row_offset, int d, int views, int anchor, const NceDevTemp& dt,
                                  const void* x_loc, const void* x_all, const unsigned char* pres_loc, const unsigned char* pres_all,
                                  const float* col_sums, void* workspace, float* loss_rows, hipStream_t s) {
    mv_loss(rows, cols, row_offset, d, views, anchor, dt, x_loc, x_all, pres_loc, pres_all, false, col_sums, workspace, loss_rows, s);
}

void launch_nce_multi_pp_loss(int64_t rows, int64_t cols, int64_t row_offset, int d, int views, int anchor, const NceDevTemp& dt,
                              const void* x_loc, const void* x_all, const unsigned char* pres_loc, const unsigned char* pres_all,
                              const float* col_sums, void* workspace, float* loss_rows, hipStream_t s) {
    mv_loss(rows, cols, row_offset, d, views, anchor, dt, x_loc, x_all, pres_loc, pres_all, true, col_sums, workspace, loss_rows, s);
}

// gradients: the weights of all pairs in place (one launch), then ONE da launch (every view with the a role; K through all its
// partner blocks, float32 slabs) and ONE db launch (every view with the b role, stored by the GEMM), then the slab sum, which
// also writes the zeros of the views without a role.  launch_nce_multi_loss must have run on this workspace.  pair_coef / pres_loc
// non-NULL: the form with missing views -- its weights kernel, then the SAME products, dT sum and slab sum: an excluded element of
// W is a zero, and the normalised rows of an absent slot are zeros, so every product is right as it stands.
namespace {
void mv_grads(int64_t rows, int64_t cols, int64_t row_offset, int d, int views, int anchor, const NceDevTemp& dt, float coef,
              const float* pair_coef, const unsigned char* pres_loc, bool per_pair, const void* x_loc, const void* x_all,
              void* workspace, const float* upstream, int out_bf16, void* dx_loc, void* dx_all, hipStream_t s) {
    const MvPairs t = mv_pairs(views, anchor);
    const MvWs w = mv_carve(workspace, rows, cols, d, views, t.count);
    const int64_t Rp = up256(rows), Cp = up256(cols);
    const int64_t chunks = Rp * (Cp / 8);
    const dim3 wgrid((unsigned)((chunks + 255) / 256), (unsigned)t.count);
    if (per_pair) {     // dt.t, dt.d_t and pair_coef [P]; pres_loc may be NULL.  dT does not come from the da product: its K loop
                        // has summed over every partner of a view, so the per-pair sums of pass 1 form it (below)
        NceMultiFin pm = {};
        for (int p = 0; p < t.count; ++p) { pm.m[p] = t.m[p]; pm.n[p] = t.n[p]; }
        pm.views = views;
        nce_multi_pp_weights_kernel<<<wgrid, dim3(256), 0, s>>>(w.e, Cp / 64, Rp / BT, w.u, w.v, w.ediag, rows, row_offset, pair_coef, pm,
                                                                pres_loc, upstream, dt.t, dt.min_t);
        if (dt.d_t) {
            const MvPpWs pw = mv_pp_carve(workspace, rows, cols, d, views, t.count);
            nce_multi_pp_dtemp_kernel<<<dim3((unsigned)t.count), dim3(256), 0, s>>>(pw.rs, pw.cs, w.u, w.v, pw.sdiag, rows, cols, Rp, Cp,
                                                                                    pair_coef, upstream, dt.t, dt.min_t, dt.d_t);
        }
    } else if (pair_coef) {
        NceMultiFin pm = {};
        for (int p = 0; p < t.count; ++p) { pm.m[p] = t.m[p]; pm.n[p] = t.n[p]; }
        pm.views = views;
        nce_multi_masked_weights_kernel<<<wgrid, dim3(256), 0, s>>>(w.e, Cp / 64, Rp / BT, w.u, w.v, w.ediag, rows, row_offset, pair_coef,
                                                                    pm, pres_loc, upstream, dt.t, dt.min_t);
    } else {
        nce_multi_weights_kernel<<<wgrid, dim3(256), 0, s>>>(w.e, Cp / 64, Rp / BT, w.u, w.v, w.ediag, rows, row_offset, coef, upstream,
                                                             dt.t, dt.min_t);
    }
    const int n_tiles_d = (d + BT - 1) / BT;
    const unsigned int pitch = 2u * (unsigned)d * (unsigned)views;
    unsigned int da_mask = 0, db_mask = 0;
    int splits = 0;
    {   // da: launch_da_product's arrangement per view; the partials of the dT sum go where the two-view form puts them
        NceGemmArgs g = {};
        g.a = (const char*)w.e; g.lda = 128; g.a_rows = (int)Rp;
        g.a_sm = (Cp / 64) * (int64_t)32768; g.a_st = 32768;
        g.b = (const char*)x_all; g.ldb = pitch; g.b_rows = (int)cols; g.b_cbytes = 2 * d;
        g.m_tiles = (int)(Rp / BT); g.n_tiles = n_tiles_d;
        g.splits = splits = da_splits(Rp, Cp, d);
        g.m_valid = (int)rows; g.n_valid = d;
        g.out = w.slabs; g.ldo = (int64_t)views * d; g.slab_stride = rows * g.ldo; g.out_bf16 = 0;
        g.tdot_src = (const unsigned short*)x_loc; g.tdot_part = w.rowsum_part;
        NceMultiProduct mv = {};
        int slots = 0;
        mv_slots(t, views, false, mv, slots, da_mask);
        mv.view_bytes = 2u * (unsigned)d; mv.seg_steps = (int)(Cp / 64); mv.out_elem_bytes = 4;
        mv.a_stride = Rp * Cp * 2; mv.tdot_stride = (int64_t)g.splits * g.m_tiles * g.n_tiles;
        const unsigned int units = (unsigned)(g.m_tiles * g.splits);
        mv.blocks_per_view = g.splits == 8 ? 8u * g.m_tiles * g.n_tiles : ((units + 7) / 8) * 8 * g.n_tiles;
        const unsigned int blocks = mv.blocks_per_view * (unsigned)slots;
        if (dt.d_t && !per_pair) {
            if (g.splits == 8) launch_multi_product<OP_ROW, OP_COL, EPI_OUT_TD, MAP_SPLITX>(g, mv, blocks, s);
            else launch_multi_product<OP_ROW, OP_COL, EPI_OUT_TD, MAP_UNITS>(g, mv, blocks, s);
            launch_nce_dtemp(w.rowsum_part, slots * mv.tdot_stride, 1, dt, s);          // views in slot order, then a fixed tree
        } else {
            if (g.splits == 8) launch_multi_product<OP_ROW, OP_COL, EPI_OUT, MAP_SPLITX>(g, mv, blocks, s);
            else launch_multi_product<OP_ROW, OP_COL, EPI_OUT, MAP_UNITS>(g, mv, blocks, s);
        }
    }
    {   // db: launch_db_product's arrangement per view, stored straight into its columns of dx_all
        NceGemmArgs g = {};
        g.a = (const char*)w.e; g.lda = 128; g.a_rows = (int)Rp; g.a_cbytes = 0; g.a_sm = Cp / 64;
        g.b = (const char*)x_loc; g.ldb = pitch; g.b_rows = (int)rows; g.b_cbytes = 2 * d;
        g.m_tiles = (int)(Cp / BT); g.n_tiles = n_tiles_d;
        g.splits = 1;
        g.m_valid = (int)cols; g.n_valid = d;
        g.out = dx_all; g.ldo = (int64_t)views * d; g.slab_stride = 0; g.out_bf16 = out_bf16;
        NceMultiProduct mv = {};
        int slots = 0;
        mv_slots(t, views, true, mv, slots, db_mask);
        mv.view_bytes = 2u * (unsigned)d; mv.seg_steps = (int)(Rp / 64); mv.out_elem_bytes = out_bf16 ? 2 : 4;
        mv.a_stride = Rp * Cp * 2;
        mv.blocks_per_view = (((unsigned)g.m_tiles + 7) / 8) * 8 * g.n_tiles;
        launch_multi_product<OP_COLB, OP_COL, EPI_OUT, MAP_UNITS>(g, mv, mv.blocks_per_view * (unsigned)slots, s);
    }
    const int64_t n4 = (rows + cols) * ((int64_t)views * d / 4);
    nce_multi_finish_kernel<<<dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s>>>(w.slabs, splits, rows, cols, views, d, da_mask, db_mask,
                                                                                     dx_loc, dx_all, out_bf16);
}
}  // namespace

void launch_nce_multi_grads(int64_t rows, int64_t cols, int64_t row_offset, int d, int views, int anchor, const NceDevTemp& dt,
                            float coef, const void* x_loc, const void* x_all, void* workspace, const float* upstream, int out_bf16,
                            void* dx_loc, void* dx_all, hipStream_t s) {
    mv_grads(rows, cols, row_offset, d, views, anchor, dt, coef, nullptr, nullptr, false, x_loc, x_all, workspace, upstream, out_bf16, dx_loc,
             dx_all, s);
}

void launch_nce_multi_masked_grads(int64_t rows, int64_t cols, int64_t row_offset, int d, int views, int anchor, const NceDevTemp& dt,
                                   const float* pair_coef, const unsigned char* pres_loc, const void* x_loc, const void* x_all,
                                   void* workspace, const float* upstream, int out_bf16, void* dx_loc, void* dx_all, hipStream_t s) {
    mv_grads(rows, cols, row_offset, d, views, anchor, dt, 0.f, pair_coef, pres_loc, false, x_loc, x_all, workspace, upstream, out_bf16,
             dx_loc, dx_all, s);
}

void launch_nce_multi_pp_grads(int64_t rows, int64_t cols, int64_t row_offset, int d, int views, int anchor, const NceDevTemp& dt,
                               const float* pair_coef, const unsigned char* pres_loc, const void* x_loc, const void* x_all,
                               void* workspace, const float* upstream, int out_bf16, void* dx_loc, void* dx_all, hipStream_t s) {
    mv_grads(rows, cols, row_offset, d, views, anchor, dt, 0.f, pair_coef, pres_loc, true, x_loc, x_all, workspace, upstream, out_bf16,
             dx_loc, dx_all, s);
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
        row_offset, coef, upstream, dt.t, dt.min_t, nullptr);
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

// ---- symmetric InfoNCE with a key queue on the same GEMMs: NT-Xent's arrangement with the two extra blocks taken against stored
// keys (include/aecf_hip.h) -------------------------------------------------------------------------------------------------------
//   X = a_loc . b_all^T (EPI_EXP_DT, InfoNCE's pass 1 to the bit: row sums lX, this rank's column sums cX)
//   U = a_loc . Qb^T, W = b_loc . Qa^T (EPI_EXP_Q: the columns at or above *q_valid left out by index; row sums)
// Da = lX + lU is local; Db = sum over ranks of cX, plus lW on the owner's range: ntx_combine_kernel, before the ONE all-reduce.
// Loss and weights are InfoNCE's kernels with l := Da, c := Db; U and W take the weights body with v = 0 and NO partner (rows = 0:
// column row_offset + i of a queue is a negative like any other), W with u_i = 1 / Db_(off + i).  The queues take no gradient: four
// products, the two on d_a_loc summed from their slabs in one pass.

namespace {

struct QueWs {
    unsigned short* e[3];               // X [Rp][Cp] | U [Rp][Qp] | W [Rp][Qp] bf16, tiled as E
    float* rowsum_part;                 // [max(Cp, Qp) / 256][Rp]   one block after the other
    float* colsum_part;                 // [m_tiles][Cp]   block X
    float* l;                           // [Rp]  lX, then Da
    float* lu;                          // [Rp]
    float* lw;                          // [Rp]
    float* u;                           // [Rp]  1 / Da
    float* v;                           // [Cp]  1 / Db
    float* uz;                          // [Rp]  1 / Db_(off + i)
    float* ediag;                       // [Rp]
    float* zero;                        // [max(Cp, Qp)]
    float* tdot_part;                   // [3][splits <= 32][m_tiles][n_tiles_d <= 16]
    float* slabs;                       // [splits X + splits Q][rows][d]: the slabs of W_X b_all, behind them those of W_U Qb
    size_t bytes;
};

QueWs que_carve(void* ws, int64_t rows, int64_t cols, int64_t q_cap, int d) {
    const int64_t Rp = up256(rows), Cp = up256(cols), Qp = up256(q_cap), Zp = Cp > Qp ? Cp : Qp;
    const int64_t mt = Rp / BT;
    QueWs w;
    char* p = (char*)ws;
    size_t off = 0;
    auto take = [&](size_t n) { char* r = p + off; off += al256(n); return r; };
    w.e[0] = (unsigned short*)take((size_t)Rp * Cp * 2);
    for (int k = 1; k < 3; ++k) w.e[k] = (unsigned short*)take((size_t)Rp * Qp * 2);
    w.rowsum_part = (float*)take((size_t)(Zp / BT) * Rp * 4);
    w.colsum_part = (float*)take((size_t)mt * Cp * 4);
    w.l = (float*)take((size_t)Rp * 4);
    w.lu = (float*)take((size_t)Rp * 4);
    w.lw = (float*)take((size_t)Rp * 4);
    w.u = (float*)take((size_t)Rp * 4);
    w.v = (float*)take((size_t)Cp * 4);
    w.uz = (float*)take((size_t)Rp * 4);
    w.ediag = (float*)take((size_t)Rp * 4);
    w.zero = (float*)take((size_t)Zp * 4);
    w.tdot_part = (float*)take((size_t)3 * 32 * 16 * mt * 4);
    w.slabs = (float*)take((size_t)(da_splits(Rp, Cp, d) + da_splits(Rp, Qp, d)) * rows * d * 4);
    w.bytes = off;
    return w;
}

// Ring buffer of past keys.  Row i of the m = min(n, q_cap) LAST source rows goes to slot (cursor + n - m + i) mod q_cap of its
// queue, 16 bytes per thread; every thread reads the cursor the push found (the bump is a launch of its own behind this one).
__global__ __launch_bounds__(256) void key_queue_copy_kernel(int64_t q_cap, int chunks, int64_t n, int64_t m, const u32x4* src_a,
                                                             const u32x4* src_b, u32x4* qa, u32x4* qb, const long long* state) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= m * chunks) return;
    const int64_t i = n - m + id / chunks;
    const int c = (int)(id % chunks);
    const long long cur = state[0];
    const int64_t slot = (int64_t)(((cur < 0 ? 0 : cur) % q_cap + i % q_cap) % q_cap);
    qa[slot * chunks + c] = src_a[i * chunks + c];
    qb[slot * chunks + c] = src_b[i * chunks + c];
}

// cursor = (cursor + n) mod q_cap, valid = min(valid + n, q_cap): one thread, plain vector stores
__global__ __launch_bounds__(64) void key_queue_bump_kernel(int64_t q_cap, int64_t n, long long* state) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const long long cur = state[0], val = state[1];
    const long long v0 = val < 0 ? 0 : (val > q_cap ? q_cap : val);
    state[0] = ((cur < 0 ? 0 : cur) % q_cap + n % q_cap) % q_cap;
    state[1] = n >= q_cap - v0 ? q_cap : v0 + n;
}

}  // namespace

bool nce_queue_gemm_supported(int d, float min_temperature) { return nce_gemm_supported(0, d, min_temperature); }

size_t nce_queue_gemm_workspace_bytes(int64_t rows, int64_t cols, int64_t q_cap, int d) {
    return que_carve(nullptr, rows, cols, q_cap, d).bytes + 256;
}

void launch_key_queue_push(int64_t q_cap, int d, int64_t n, const void* src_a, const void* src_b, void* qa, void* qb, int64_t* state,
                           hipStream_t s) {
    if (n <= 0) return;
    const int64_t m = n < q_cap ? n : q_cap;
    const int chunks = d / 8;
    key_queue_copy_kernel<<<dim3((unsigned)((m * chunks + 255) / 256)), dim3(256), 0, s>>>(
        q_cap, chunks, n, m, (const u32x4*)src_a, (const u32x4*)src_b, (u32x4*)qa, (u32x4*)qb, (const long long*)state);
    key_queue_bump_kernel<<<dim3(1), dim3(64), 0, s>>>(q_cap, n, (long long*)state);
}

// pass 1: the three blocks, Da (workspace) and col_sums [cols] = this rank's cX, plus lW on [row_offset, row_offset + rows)
void launch_nce_queue_gemm_pass1(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, const void* a_loc,
                                 const void* b_loc, const void* b_all, const void* qa, const void* qb, int64_t q_cap,
                                 const int64_t* q_valid, void* workspace, float* col_sums, hipStream_t s) {
    const QueWs w = que_carve(workspace, rows, cols, q_cap, d);
    const int64_t Rp = up256(rows), Cp = up256(cols), Qp = up256(q_cap);
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
        LogitsLaunch L = logits_args(rows, q_cap, d, k == 1 ? a_loc : b_loc, k == 1 ? qb : qa);
        NceGemmArgs& g = L.g;
        g.e = w.e[k]; g.e_tiles = Qp / 64;
        g.rowsum_part = w.rowsum_part;
        g.temp = dt.t; g.min_temp = dt.min_t;
        g.q_count = reinterpret_cast<const long long*>(q_valid);            // EPI_EXP_Q: the device count of valid slots
        launch_gemm<OP_ROW, OP_ROW, EPI_EXP_Q, MAP_2D>(g, L.blocks, s);
        // the row blocks of the sums launch alone: this block leaves no column partials
        nce_sums_kernel<<<dim3((unsigned)(Rp / 64)), dim3(256), 0, s>>>(w.rowsum_part, nullptr, g.m_tiles, g.n_tiles, rows, q_cap,
                                                                        k == 1 ? w.lu : w.lw, nullptr);
    }
    ntx_combine_kernel<<<dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s>>>(w.l, w.lu, w.lw, col_sums, rows, row_offset);
}

// normalisers + loss rows of this rank's pairs from the col_sums of all ranks: InfoNCE's finalize with l := Da, c := Db
void launch_nce_queue_gemm_loss(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, const void* a_loc,
                                const void* b_all, int64_t q_cap, const float* col_sums, void* workspace, float* loss_rows,
                                hipStream_t s) {
    const QueWs w = que_carve(workspace, rows, cols, q_cap, d);
    NceFinArgs f = {};
    f.a = (const unsigned short*)a_loc; f.b = (const unsigned short*)b_all; f.l = w.l; f.c = col_sums;
    f.u = w.u; f.v = w.v; f.ediag = w.ediag; f.loss_rows = loss_rows; f.rows = rows; f.cols = cols; f.row_offset = row_offset;
    f.Rp = up256(rows); f.Cp = up256(cols); f.d = d; f.sym = 1;
    f.temp = dt.t; f.min_temp = dt.min_t;
    nce_finalize_kernel<true><<<dim3((unsigned)((f.Rp + 3) / 4)), dim3(256), 0, s>>>(f);
}

// gradients: the three weights passes in place, then
//   d_a_loc = W_X b_all + W_U Qb (one slab sum over both products' slabs)      d_b_loc = W_W Qa      d_b_all = W_X^T a_loc
// every output rounded once from its float32 sum; dt.d_t from the partials of the three da products, one fixed-order reduction.
// Every slot of the queues is read (the weight of a slot at or above *q_valid is an exact zero): they must hold finite rows.
void launch_nce_queue_gemm_grads(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, float coef,
                                 const void* a_loc, const void* b_loc, const void* b_all, const void* qa, const void* qb,
                                 int64_t q_cap, void* workspace, const float* upstream, int out_bf16, void* d_a_loc, void* d_b_loc,
                                 void* d_b_all, hipStream_t s) {
    const QueWs w = que_carve(workspace, rows, cols, q_cap, d);
    const int64_t Rp = up256(rows), Cp = up256(cols), Qp = up256(q_cap), Zp = Cp > Qp ? Cp : Qp;
    const dim3 xgrid((unsigned)((Rp * (Cp / 8) + 255) / 256)), qgrid((unsigned)((Rp * (Qp / 8) + 255) / 256));
    ntx_prep_kernel<<<dim3((unsigned)(Zp / 256)), dim3(256), 0, s>>>(w.v, w.uz, w.zero, rows, row_offset, Rp, Zp);
    nce_weights_dt_kernel<<<xgrid, dim3(256), 0, s>>>(w.e[0], Cp / 64, Rp / BT, w.u, w.v, w.ediag, rows, row_offset, coef, 2.0f, upstream,
                                                      dt.t, dt.min_t);
    // rows = 0: no element of a queue block is a partner
    nce_weights_dt_kernel<<<qgrid, dim3(256), 0, s>>>(w.e[1], Qp / 64, Rp / BT, w.u, w.zero, w.zero, 0, row_offset, coef, 0.0f, upstream,
                                                      dt.t, dt.min_t);
    nce_weights_dt_kernel<<<qgrid, dim3(256), 0, s>>>(w.e[2], Qp / 64, Rp / BT, w.uz, w.zero, w.zero, 0, row_offset, coef, 0.0f, upstream,
                                                      dt.t, dt.min_t);
    const bool want_td = dt.d_t != nullptr;
    const int64_t n_tdx = da_tdot_count(rows, cols, d), n_tdq = da_tdot_count(rows, q_cap, d), n_loc = rows * (int64_t)d;
    const NceGemmArgs g0 = {};
    // both products always leave float32 slabs, those of W_U Qb behind those of W_X b_all: one sum, one rounding
    const int sx = launch_da_product<EPI_OUT, EPI_OUT_TD>(rows, cols, d, g0, w.e[0], w.slabs, w.tdot_part, want_td, a_loc, b_all, 0,
                                                          nullptr, s);
    const int su = launch_da_product<EPI_OUT, EPI_OUT_TD>(rows, q_cap, d, g0, w.e[1], w.slabs + sx * n_loc, w.tdot_part + n_tdx, want_td,
                                                          a_loc, qb, 0, nullptr, s);
    launch_slab_sum(w.slabs, sx + su, n_loc, d_a_loc, out_bf16, s);
    const int sw = launch_da_product<EPI_OUT, EPI_OUT_TD>(rows, q_cap, d, g0, w.e[2], w.slabs, w.tdot_part + n_tdx + n_tdq, want_td, b_loc,
                                                          qa, out_bf16, d_b_loc, s);
    if (sw) launch_slab_sum(w.slabs, sw, n_loc, d_b_loc, out_bf16, s);
    if (want_td) launch_nce_dtemp(w.tdot_part, n_tdx + 2 * n_tdq, 1, dt, s);
    launch_db_product<EPI_OUT>(rows, cols, d, g0, w.e[0], a_loc, out_bf16, d_b_all, s);
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
                                                          row_offset, coef, upstream, dt.t, dt.min_t, nullptr);
    sup_weights_kernel<true><<<wgrid, dim3(256), 0, s>>>(w.e[1], Cp / 64, Rp / BT, w.u, w.zero, w.rn, w.zero, nullptr, lr, lc, rows, cols,
                                                         row_offset, coef, upstream, dt.t, dt.min_t, nullptr);
    sup_weights_kernel<true><<<wgrid, dim3(256), 0, s>>>(w.e[2], Cp / 64, Rp / BT, w.uz, w.zero, w.rnz, w.zero, nullptr, lr, lc, rows, cols,
                                                         row_offset, coef, upstream, dt.t, dt.min_t, nullptr);
    sup_pool_products(w, rows, cols, d, dt, a_loc, b_loc, a_all, b_all, out_bf16, d_a_loc, d_b_loc, d_a_all, d_b_all, s);
}

// ---- supervised contrastive loss with a key queue: the key-queue InfoNCE's three blocks with the label statistics of the supervised
// loss on each (include/aecf_hip.h) ---------------------------------------------------------------------------------------------------
//   X = a_loc . b_all^T (EPI_SUP, the cross-view pass 1 to the bit: row statistics and this rank's column statistics)
//   U = a_loc . Qb^T, W = b_loc . Qa^T (EPI_SUP_Q: the slots at or above *q_valid left out by index, of the sums and of the matches;
//       the ring of stored labels Ql as column labels; row statistics alone)
// Anchor a_i: (Da, ka, sa) = X's row statistics + U's; anchor b_g: (Db, kb, sb) = the ranks' column statistics of X plus W's row
// statistics of the row's owner -- sup_pool_combine_kernel, before the ONE all-reduce of [3][cols].  sup_finalize_kernel serves
// unchanged; W_X is sup_weights_kernel's, W_U and W_W its QUEUE variant (v = rnc = 0; W with u and rn gathered at off + i); the four
// products are those of launch_nce_queue_gemm_grads.  The queues and their labels take no gradient.

namespace {

struct SupQueWs {
    unsigned short* e[3];               // X [Rp][Cp] | U [Rp][Qp] | W [Rp][Qp] bf16, tiled as E
    float* row_part;                    // [3][max(Cp, Qp) / 256][Rp]  sums of E | counts | matched sums, one block after the other
    float* col_part;                    // [3][m_tiles][Cp]  block X
    float* row_stats;                   // [3][Rp]  X's, then the combined Da | ka | sa
    float* u_stats;                     // [3][Rp]
    float* w_stats;                     // [3][Rp]
    float* u;                           // [Rp]  1 / Da
    float* rn;                          // [Rp]  1 / na
    float* v;                           // [Cp]  1 / Db
    float* rnc;                         // [Cp]  1 / nb
    float* uz;                          // [Rp]  1 / Db_(off + i)
    float* rnz;                         // [Rp]  1 / nb_(off + i)
    float* ediag;                       // [Rp]
    float* zero;                        // [max(Cp, Qp)]
    float* tdot_part;                   // [3][splits <= 32][m_tiles][n_tiles_d <= 16]
    float* slabs;                       // [splits X + splits Q][rows][d]: the slabs of W_X b_all, behind them those of W_U Qb
    size_t bytes;
};

SupQueWs sup_que_carve(void* ws, int64_t rows, int64_t cols, int64_t q_cap, int d) {
    const int64_t Rp = up256(rows), Cp = up256(cols), Qp = up256(q_cap), Zp = Cp > Qp ? Cp : Qp;
    const int64_t mt = Rp / BT;
    SupQueWs w;
    char* p = (char*)ws;
    size_t off = 0;
    auto take = [&](size_t n) { char* r = p + off; off += al256(n); return r; };
    w.e[0] = (unsigned short*)take((size_t)Rp * Cp * 2);
    for (int k = 1; k < 3; ++k) w.e[k] = (unsigned short*)take((size_t)Rp * Qp * 2);
    w.row_part = (float*)take((size_t)3 * (Zp / BT) * Rp * 4);
    w.col_part = (float*)take((size_t)3 * mt * Cp * 4);
    w.row_stats = (float*)take((size_t)3 * Rp * 4);
    w.u_stats = (float*)take((size_t)3 * Rp * 4);
    w.w_stats = (float*)take((size_t)3 * Rp * 4);
    w.u = (float*)take((size_t)Rp * 4);
    w.rn = (float*)take((size_t)Rp * 4);
    w.v = (float*)take((size_t)Cp * 4);
    w.rnc = (float*)take((size_t)Cp * 4);
    w.uz = (float*)take((size_t)Rp * 4);
    w.rnz = (float*)take((size_t)Rp * 4);
    w.ediag = (float*)take((size_t)Rp * 4);
    w.zero = (float*)take((size_t)Zp * 4);
    w.tdot_part = (float*)take((size_t)3 * 32 * 16 * mt * 4);
    w.slabs = (float*)take((size_t)(da_splits(Rp, Cp, d) + da_splits(Rp, Qp, d)) * rows * d * 4);
    w.bytes = off;
    return w;
}

// The ring of stored labels beside the two key rings: the label of row i of the m = min(n, q_cap) LAST source rows goes to the slot
// key_queue_copy_kernel gives its keys, from the cursor the push found (the bump runs behind both copies).  src == NULL: -1, so
// that no label of an overwritten key stays attached to a new one.
__global__ __launch_bounds__(256) void key_queue_label_copy_kernel(int64_t q_cap, int64_t n, int64_t m, const long long* src,
                                                                   long long* ql, const long long* state) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= m) return;
    const int64_t i = n - m + id;
    const long long cur = state[0];
    const int64_t slot = (int64_t)(((cur < 0 ? 0 : cur) % q_cap + i % q_cap) % q_cap);
    ql[slot] = src ? src[i] : -1ll;
}

}  // namespace

// An anchor's count adds the matches of two blocks, at most cols - 1 of the batch (the partner excluded) and q_cap of the queue:
// 1 + (cols - 1) + q_cap has to stay an exact float32 integer, so cols + q_cap <= 2^24.
bool supcon_queue_gemm_supported(int d, float min_temperature, int64_t cols, int64_t q_cap) {
    return nce_gemm_supported(0, d, min_temperature) && cols + q_cap <= ((int64_t)1 << 24);
}

size_t supcon_queue_gemm_workspace_bytes(int64_t rows, int64_t cols, int64_t q_cap, int d) {
    return sup_que_carve(nullptr, rows, cols, q_cap, d).bytes + 256;
}

void launch_key_queue_push_labeled(int64_t q_cap, int d, int64_t n, const void* src_a, const void* src_b, const int64_t* src_labels,
                                   void* qa, void* qb, int64_t* ql, int64_t* state, hipStream_t s) {
    if (n <= 0) return;
    const int64_t m = n < q_cap ? n : q_cap;
    const int chunks = d / 8;
    key_queue_copy_kernel<<<dim3((unsigned)((m * chunks + 255) / 256)), dim3(256), 0, s>>>(
        q_cap, chunks, n, m, (const u32x4*)src_a, (const u32x4*)src_b, (u32x4*)qa, (u32x4*)qb, (const long long*)state);
    key_queue_label_copy_kernel<<<dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s>>>(q_cap, n, m, (const long long*)src_labels,
                                                                                       (long long*)ql, (const long long*)state);
    key_queue_bump_kernel<<<dim3(1), dim3(64), 0, s>>>(q_cap, n, (long long*)state);
}

// pass 1: the three blocks, the combined row statistics (workspace) and col_stats [3][cols] = this rank's column statistics of X, plus
// the row statistics of W on [row_offset, row_offset + rows)
void launch_supcon_queue_gemm_pass1(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, const void* a_loc,
                                    const void* b_loc, const void* b_all, const void* qa, const void* qb, int64_t q_cap,
                                    const int64_t* q_valid, const int64_t* row_labels, const int64_t* col_labels,
                                    const int64_t* q_labels, void* workspace, float* col_stats, hipStream_t s) {
    const SupQueWs w = sup_que_carve(workspace, rows, cols, q_cap, d);
    const int64_t Rp = up256(rows), Cp = up256(cols), Qp = up256(q_cap);
    {
        LogitsLaunch L = logits_args(rows, cols, d, a_loc, b_all);
        NceGemmArgs& g = L.g;
        g.e = w.e[0]; g.e_tiles = Cp / 64;
        g.temp = dt.t; g.min_temp = dt.min_t; g.row_offset = row_offset;
        g.lab_row = (const long long*)row_labels; g.lab_col = (const long long*)col_labels;
        const int64_t rplane = (int64_t)g.n_tiles * Rp, cplane = (int64_t)g.m_tiles * Cp;
        g.rowsum_part = w.row_part; g.rowcnt_part = w.row_part + rplane; g.rowsx_part = w.row_part + 2 * rplane;
        g.colsum_part = w.col_part; g.colcnt_part = w.col_part + cplane; g.colsx_part = w.col_part + 2 * cplane;
        launch_gemm<OP_ROW, OP_ROW, EPI_SUP, MAP_2D>(g, L.blocks, s);
        sup_sums_kernel<<<dim3((unsigned)((Rp + Cp) / 64), 3), dim3(256), 0, s>>>(w.row_part, w.col_part, g.m_tiles, g.n_tiles, rows, cols,
                                                                                  w.row_stats, col_stats);
    }
    for (int k = 1; k < 3; ++k) {
        LogitsLaunch L = logits_args(rows, q_cap, d, k == 1 ? a_loc : b_loc, k == 1 ? qb : qa);
        NceGemmArgs& g = L.g;
        g.e = w.e[k]; g.e_tiles = Qp / 64;
        g.temp = dt.t; g.min_temp = dt.min_t;
        g.lab_row = (const long long*)row_labels; g.lab_col = (const long long*)q_labels;
        g.q_count = reinterpret_cast<const long long*>(q_valid);
        const int64_t rplane = (int64_t)g.n_tiles * Rp;
        g.rowsum_part = w.row_part; g.rowcnt_part = w.row_part + rplane; g.rowsx_part = w.row_part + 2 * rplane;
        launch_gemm<OP_ROW, OP_ROW, EPI_SUP_Q, MAP_2D>(g, L.blocks, s);
        // the row blocks of the sums launch alone: this block leaves no column partials
        sup_sums_kernel<<<dim3((unsigned)(Rp / 64), 3), dim3(256), 0, s>>>(w.row_part, nullptr, g.m_tiles, g.n_tiles, rows, q_cap,
                                                                           k == 1 ? w.u_stats : w.w_stats, nullptr);
    }
    sup_pool_combine_kernel<<<dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s>>>(w.row_stats, w.u_stats, w.w_stats, col_stats, rows,
                                                                                       cols, row_offset, Rp);
}

// normalisers + loss rows of this rank's pairs from the col_stats of all ranks: sup_finalize_kernel on the combined statistics
void launch_supcon_queue_gemm_loss(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, const void* a_loc,
                                   const void* b_all, int64_t q_cap, const float* col_stats, void* workspace, float* loss_rows,
                                   hipStream_t s) {
    const SupQueWs w = sup_que_carve(workspace, rows, cols, q_cap, d);
    SupFinArgs f = {};
    f.a = (const unsigned short*)a_loc; f.b = (const unsigned short*)b_all; f.row_stats = w.row_stats; f.col_stats = col_stats;
    f.u = w.u; f.rn = w.rn; f.v = w.v; f.rnc = w.rnc; f.loss_rows = loss_rows; f.ediag = w.ediag;
    f.rows = rows; f.cols = cols; f.row_offset = row_offset; f.Rp = up256(rows); f.Cp = up256(cols); f.d = d;
    f.temp = dt.t; f.min_temp = dt.min_t;
    sup_finalize_kernel<<<dim3((unsigned)((f.Rp + 3) / 4)), dim3(256), 0, s>>>(f);
}

// gradients: the three weights passes in place, then the four products of launch_nce_queue_gemm_grads
//   d_a_loc = W_X b_all + W_U Qb (one slab sum over both products' slabs)      d_b_loc = W_W Qa      d_b_all = W_X^T a_loc
// every output rounded once from its float32 sum; dt.d_t from the partials of the three da products, one fixed-order reduction.
// Every slot of the key rings is read (the weight of a slot at or above *q_valid is an exact zero): they must hold finite rows.
void launch_supcon_queue_gemm_grads(int64_t rows, int64_t cols, int64_t row_offset, int d, const NceDevTemp& dt, float coef,
                                    const void* a_loc, const void* b_loc, const void* b_all, const void* qa, const void* qb,
                                    int64_t q_cap, const int64_t* q_valid, const int64_t* row_labels, const int64_t* col_labels,
                                    const int64_t* q_labels, void* workspace, const float* upstream, int out_bf16, void* d_a_loc,
                                    void* d_b_loc, void* d_b_all, hipStream_t s) {
    const SupQueWs w = sup_que_carve(workspace, rows, cols, q_cap, d);
    const int64_t Rp = up256(rows), Cp = up256(cols), Qp = up256(q_cap), Zp = Cp > Qp ? Cp : Qp;
    const dim3 xgrid((unsigned)((Rp * (Cp / 8) + 255) / 256)), qgrid((unsigned)((Rp * (Qp / 8) + 255) / 256));
    const long long* lr = (const long long*)row_labels;
    const long long* lc = (const long long*)col_labels;
    const long long* lq = (const long long*)q_labels;
    const long long* qv = (const long long*)q_valid;
    sup_pool_prep_kernel<<<dim3((unsigned)(Zp / 256)), dim3(256), 0, s>>>(w.v, w.rnc, w.uz, w.rnz, w.zero, rows, row_offset, Rp, Zp);
    sup_weights_kernel<false><<<xgrid, dim3(256), 0, s>>>(w.e[0], Cp / 64, Rp / BT, w.u, w.v, w.rn, w.rnc, w.ediag, lr, lc, rows, cols,
                                                          row_offset, coef, upstream, dt.t, dt.min_t, nullptr);
    sup_weights_kernel<false, true><<<qgrid, dim3(256), 0, s>>>(w.e[1], Qp / 64, Rp / BT, w.u, w.zero, w.rn, w.zero, nullptr, lr, lq, rows,
                                                                q_cap, row_offset, coef, upstream, dt.t, dt.min_t, qv);
    sup_weights_kernel<false, true><<<qgrid, dim3(256), 0, s>>>(w.e[2], Qp / 64, Rp / BT, w.uz, w.zero, w.rnz, w.zero, nullptr, lr, lq, rows,
                                                                q_cap, row_offset, coef, upstream, dt.t, dt.min_t, qv);
    const bool want_td = dt.d_t != nullptr;
    const int64_t n_tdx = da_tdot_count(rows, cols, d), n_tdq = da_tdot_count(rows, q_cap, d), n_loc = rows * (int64_t)d;
    const NceGemmArgs g0 = {};
    // both products always leave float32 slabs, those of W_U Qb behind those of W_X b_all: one sum, one rounding
    const int sx = launch_da_product<EPI_OUT, EPI_OUT_TD>(rows, cols, d, g0, w.e[0], w.slabs, w.tdot_part, want_td, a_loc, b_all, 0,
                                                          nullptr, s);
    const int su = launch_da_product<EPI_OUT, EPI_OUT_TD>(rows, q_cap, d, g0, w.e[1], w.slabs + sx * n_loc, w.tdot_part + n_tdx, want_td,
                                                          a_loc, qb, 0, nullptr, s);
    launch_slab_sum(w.slabs, sx + su, n_loc, d_a_loc, out_bf16, s);
    const int sw = launch_da_product<EPI_OUT, EPI_OUT_TD>(rows, q_cap, d, g0, w.e[2], w.slabs, w.tdot_part + n_tdx + n_tdq, want_td, b_loc,
                                                          qa, out_bf16, d_b_loc, s);
    if (sw) launch_slab_sum(w.slabs, sw, n_loc, d_b_loc, out_bf16, s);
    if (want_td) launch_nce_dtemp(w.tdot_part, n_tdx + 2 * n_tdq, 1, dt, s);
    launch_db_product<EPI_OUT>(rows, cols, d, g0, w.e[0], a_loc, out_bf16, d_b_all, s);
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
