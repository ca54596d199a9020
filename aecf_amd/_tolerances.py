"""Per-tensor bounds of the bf16-STORED path against float32 math.  Kept inside the package so
that the runtime smoke check (``__graft_entry__.smoke``) and the tests assert the SAME numbers without the package depending
on the tests tree.  Not used by any product path."""

# ---- the bf16 contract, per tensor: measured on MI355X over the g2 / hot fixtures, the shape sweep and
# the random cases (round 3, gpurun_out/parity_errors.jsonl: maxima in the comments) + ~10-20 % margin.  A bf16-STORED tensor
# carries one output rounding (up to 2^-9 of ITS OWN magnitude, 3.9e-3 of the largest element in the worst case); the
# parameter gradients are float32 batch sums of products whose operands (do = dy W_o, the pooled rows) were rounded to bf16
# once each.  Nothing here is a blanket tolerance: a tensor that drifts by 20 % fails.
#   bf16-stored gradients (bf16 parameters):           y 3.25e-3  wbar 3.34e-3  dx 4.09e-3 (smoke's scaled modalities)  dquery 4.04e-3  dw_in 4.36e-3
#                                                      db_in 4.31e-3  dw_out 3.92e-3  db_out 3.02e-3
BF16_BOUNDS = dict(y=4.0e-3, wbar=4.0e-3, dx=4.5e-3, dquery=5.0e-3, dw_in=5.2e-3, db_in=5.2e-3, dw_out=4.7e-3, db_out=3.7e-3)
#   float32-stored gradients of the bf16 kernels (float32 master parameters; y / wbar / dx still bf16-stored):
#                                                      y 3.79e-3  wbar 3.76e-3  dx 4.10e-3  dq 4.41e-3  dw_in 3.97e-3
#                                                      db_in 3.63e-3  dw_out 2.46e-3  db_out 8e-8 (a float32 column sum of dy)
BF16_F32GRAD_BOUNDS = dict(y=4.2e-3, wbar=4.2e-3, dx=4.5e-3, dq=5.0e-3, dquery=5.0e-3, dw_in=4.4e-3, db_in=4.0e-3, dw_out=3.0e-3,
                           db_out=1e-5)
#   ... where the hi + lo weight-gradient products are built (bf16, d = 256 / 512 / 768 / 1024, M <= 4, as the weight-stationary
#   value projection takes them: on by themselves for float32-stored gradients, layer.PoolOptions.hilo_grads) the three gradients
#   that are sums of products of DERIVED operands meet north_star's 1e-3 with an order of magnitude to spare: measured 3-5e-6 at
#   the headline shape.  dq / dquery here is the
#   gradient handed back through a bf16 query tensor (one output rounding) and keeps its bound.
BF16_F32GRAD_HILO_BOUNDS = dict(BF16_F32GRAD_BOUNDS, dw_in=1e-4, db_in=1e-4, dw_out=1e-4)

# ---- the same numbers BLOCK-WISE (tests/pool_score_cases.py, tests/test_pool_score_gpu.py).  The tables above
# are asserted on whole tensors under the loss y . dy + wbar . dwbar, where the value term of dx and the v block of dw_in / db_in
# set the maximum: at d >= 512 the d_attn_w / H term is 0.1 % .. 0.3 % of it and may be missing altogether within dx 4.5e-3 and
# dw_in 5.2e-3.  The score-path tests run dy, dwbar and the eval-mode entropy gradient apart and score dx (whole, per modality,
# ragged tail rows), dquery, dw_out, db_out and the q / k / v blocks of dw_in / db_in each against its own largest element.  Their
# bf16 / float16 bound is computed per block and case, max(2 x torch's module in that dtype on the same upstream, 2^-8 / 2^-11) (it
# comes out near 1e-2, never above 4e-2); what IS read from here, on blocks instead of tensors: BF16_BOUNDS['dx'] on the whole of dx wherever
# dy flows (the tighter of the two there), and the BF16_F32GRAD_HILO_BOUNDS entries on every float32-stored block.  Measured on
# MI355X, largest value over the 16 cases (routes dsu_ws, dsu_ws with low tiles, dscore_v, bwd_g recompute):
#   whole dx under dy / dy + dwbar, of 4.5e-3:           dsu_ws 3.79e-3 (B = 1)  low tiles 3.55e-3  dscore_v 3.73e-3  bwd_g 3.55e-3
#   score blocks under dwbar alone, error / (2 x torch):  dsu_ws 0.40  low tiles 0.42 (dx.tail)  dscore_v 0.46  bwd_g 0.44
#   ... under a key_padding_mask:                         0.33 / 0.38 / 0.43 / 0.36;   entropy gradient alone: 0.32 / 0.33 / 0.40 / 0.26
#   float32-stored blocks of the hi + lo routes, of their own maximum (bound 1e-4): dw_in.q 6.7e-6  dw_in.k 6.7e-6  dw_in.v 6.9e-6
#                                                         db_in.q 6.7e-6  db_in.v 3.3e-6  dw_out 3.4e-6; dquery 1e-5 (bound 5e-3)
#   float32 kernels (dscore_v), every block: <= 5.9e-7 of its own maximum (bound 1e-5 / 2e-5); float16: <= 0.50 of 2 x torch
# No block exceeded its bound, so nothing here was widened; db_in.k is exactly 0 under every upstream.

# ---- MHA_GENERAL_BF16: the general attention route (aecf_mha_forward / _backward) in bf16 against the float64 oracle, measured on
# MI355X (tests/test_mha_edges_gpu.py, test_general_path_reach; records mha_edges_* of tests/helpers.record_errors).  This route
# has no fixed table: its bound is computed per case and per tensor inside the tests, max(2 x the error of
# torch.nn.MultiheadAttention run in bfloat16 on the CPU on the same values, 2^-8) (tests/mha_edges_cases.py: bf16_bounds), so
# the numbers below are a record, the reference's beside the kernel's, not something a test reads.  Per-tensor maxima:
#                                                        y        wbar     dquery   dkey     dvalue   dw_in    db_in    dw_out   db_out
#   options x chunks, eval (36 cases)          kernel    7.19e-3  6.99e-3  1.14e-2  9.36e-3  8.07e-3  6.10e-3  4.90e-3  5.04e-3  3.20e-3
#                                              torch     1.44e-2  1.67e-2  1.31e-2  1.70e-2  1.79e-2  1.32e-2  4.90e-3  8.64e-3  3.20e-3
#   options x chunks, dropout (12 cases)       kernel    8.20e-3  1.46e-2  8.16e-3  8.28e-3  1.12e-2  6.62e-3  4.16e-3  4.95e-3  3.00e-3
#     (torch's module cannot repeat the draw: bound = the largest eval-mode bound of the geometry; wbar 1.46e-2 of 2.91e-2)
#   lengths and head sizes (10 reach rows)     kernel    4.82e-3  4.58e-3  5.82e-3  6.11e-3  7.37e-3  5.69e-3  4.10e-3  6.07e-3  3.34e-3
#                                              torch     6.05e-3  8.67e-3  7.71e-3  1.17e-2  8.19e-3  8.54e-3  4.71e-3  6.07e-3  3.34e-3
#   64 chunks, carries that add up             kernel    3.88e-3  2.15e-3  4.17e-3  4.94e-3  2.82e-3  6.17e-3  3.48e-3  5.58e-3  3.82e-3
#                                              torch     5.44e-3  2.15e-3  8.83e-3  8.82e-3  4.75e-3  1.04e-2  4.50e-3  5.66e-3  3.82e-3
# The kernel is at or below torch's own bf16 error on every tensor (softmax, dropout and the dk / dv sums stay in float32 between
# the bf16 stores); the largest error over bound of any case and tensor is 0.77, none needs more than 2 x the reference.  Same
# runs: float32 at most 3.7e-6 (bound 1e-5), float16 at most 1.44e-3 (bound 1e-3 + 2^-11 = 1.49e-3).
