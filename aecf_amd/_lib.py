"""ctypes binding of libaecf_hip.so (the C ABI declared in include/aecf_hip.h).

The library is the product: there is no Python / PyTorch fallback for its arithmetic.  If
it is missing or an entry point is absent, loading fails loudly.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_float, c_int, c_int32, c_int64, c_size_t, c_uint32, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# AECF_LIB_PATH: another build of the same library (A/B timing of kernel variants on one box); default = the in-tree build
LIB_PATH = os.environ.get("AECF_LIB_PATH") or os.path.join(_HERE, "lib", "libaecf_hip.so")

AECF_ABI_VERSION = 10
AECF_BF16 = 0
AECF_F32 = 1
AECF_F16 = 2
AECF_SETS_U8 = 3            # aecf_label_sets_pack: one byte per class (torch bool / uint8)
AECF_MLLOSS_U8 = 3          # aecf_mlloss_*: label codes beside the aecf_dtype values (bool / uint8, int8 with negative = unknown)
AECF_MLLOSS_I8 = 4
AECF_MLLOSS_MEAN = 0        # aecf_mlloss_*: reduction
AECF_MLLOSS_SUM = 1
AECF_MLCAL_MAX_BINS = 32    # aecf_mlcal_*: bins at most, and the fit's modes
AECF_MLCAL_TEMPERATURE = 0
AECF_MLCAL_CLASS_TEMPERATURE = 1
AECF_MLCAL_PLATT = 2
AECF_SETS_OVERLAP = 0
AECF_SETS_JACCARD = 1
AECF_PRECISE = 1
AECF_DRAW_UNIFORMS = 2
AECF_HILO_GRADS = 4
AECF_PREP_READY = 8
AECF_FWD_STAGES = 4
AECF_BWD_STAGES = 8



class PoolDesc(Structure):
    _fields_ = [
        ("batch", c_int64),
        ("modalities", c_int32),
        ("embed_dim", c_int32),
        ("num_heads", c_int32),
        ("dtype", c_int32),
        ("mask_mode", c_int32),
        ("min_active", c_int32),
        ("base_mask_prob", c_float),
        ("entropy_target", c_float),
        ("eps", c_float),
    ]


class PoolFwdArgs(Structure):
    _fields_ = [
        ("x", c_void_p), ("query", c_void_p), ("w_in", c_void_p), ("b_in", c_void_p),
        ("w_out", c_void_p), ("b_out", c_void_p), ("key_padding_mask", c_void_p),
        ("uniforms", c_void_p), ("y", c_void_p), ("attn_w", c_void_p), ("masked_w", c_void_p),
        ("entropy", c_void_p), ("mask_rate", c_void_p), ("saved_probs", c_void_p),
        ("saved_o", c_void_p), ("saved_v", c_void_p), ("workspace", c_void_p), ("workspace_bytes", c_size_t),
        ("stage_events", c_void_p),
        ("info_attn_w", c_void_p), ("info_masked_w", c_void_p), ("info_entropy", c_void_p),
        ("info_mask_rate", c_void_p), ("saved_prep", c_void_p),
        ("info_target_entropy", c_void_p), ("target_entropy_value", c_float), ("flags", c_int32),
        ("ent_loss_partial", c_void_p),
        ("philox_seed", c_uint64), ("philox_offset", c_uint64), ("philox_threads", c_uint32), ("ent_loss", c_void_p),
        ("saved_o_lo", c_void_p), ("philox_element0", c_int64),
    ]


class PoolBwdArgs(Structure):
    _fields_ = [
        ("x", c_void_p), ("query", c_void_p), ("w_in", c_void_p), ("b_in", c_void_p),
        ("w_out", c_void_p), ("dy", c_void_p), ("d_attn_w", c_void_p), ("d_entropy", c_void_p),
        ("attn_w", c_void_p), ("saved_probs", c_void_p), ("saved_o", c_void_p), ("saved_v", c_void_p),
        ("dx", c_void_p),
        ("dquery", c_void_p), ("dw_in", c_void_p), ("db_in", c_void_p), ("dw_out", c_void_p),
        ("db_out", c_void_p), ("workspace", c_void_p), ("workspace_bytes", c_size_t),
        ("stage_events", c_void_p),
        ("grad_dtype", c_int32), ("flags", c_int32), ("saved_prep", c_void_p), ("param_grads_event", c_void_p),
        ("saved_o_lo", c_void_p), ("grad_scale", c_float),
    ]


class MhaDesc(Structure):
    _fields_ = [("batch", c_int64), ("tgt_len", c_int32), ("src_len", c_int32), ("embed_dim", c_int32),
                ("num_heads", c_int32), ("dtype", c_int32), ("dropout_p", c_float)]


class MhaFwdArgs(Structure):
    _fields_ = [("query", c_void_p), ("key", c_void_p), ("value", c_void_p), ("w_in", c_void_p), ("b_in", c_void_p),
                ("w_out", c_void_p), ("b_out", c_void_p), ("attn_mask", c_void_p), ("attn_mask_stride", c_int64),
                ("key_padding_mask", c_void_p), ("dropout_uniforms", c_void_p), ("y", c_void_p), ("attn_w", c_void_p),
                ("saved_q", c_void_p), ("saved_k", c_void_p), ("saved_v", c_void_p), ("saved_o", c_void_p),
                ("saved_probs", c_void_p)]


class MhaBwdArgs(Structure):
    _fields_ = [("query", c_void_p), ("key", c_void_p), ("value", c_void_p), ("w_in", c_void_p), ("w_out", c_void_p),
                ("dropout_uniforms", c_void_p), ("dy", c_void_p), ("d_attn_w", c_void_p), ("saved_q", c_void_p),
                ("saved_k", c_void_p), ("saved_v", c_void_p), ("saved_o", c_void_p), ("saved_probs", c_void_p),
                ("dquery", c_void_p), ("dkey", c_void_p), ("dvalue", c_void_p), ("dw_in", c_void_p), ("db_in", c_void_p),
                ("dw_out", c_void_p), ("db_out", c_void_p), ("workspace", c_void_p), ("workspace_bytes", c_size_t)]


# every symbol include/aecf_hip.h declares: (name, restype, argtypes)
_SYMBOLS = [
    ("aecf_abi_version", c_int, []),
    ("aecf_status_string", c_char_p, [c_int]),
    ("aecf_pool_stage_name", c_char_p, [c_int, c_int]),
    ("aecf_pool_check", c_int, [POINTER(PoolDesc)]),
    ("aecf_pool_fwd_workspace_bytes", c_size_t, [POINTER(PoolDesc)]),
    ("aecf_pool_bwd_workspace_bytes", c_size_t, [POINTER(PoolDesc)]),
    ("aecf_pool_prep_bytes", c_size_t, [POINTER(PoolDesc)]),
    ("aecf_pool_hilo_bwd_workspace_bytes", c_size_t, [POINTER(PoolDesc)]),
    ("aecf_pool_wants_saved_v", c_int, [POINTER(PoolDesc)]),
    ("aecf_pool_precise_workspace_bytes", c_size_t, [POINTER(PoolDesc), c_int]),
    ("aecf_philox_uniforms", c_int, [c_int64, c_uint64, c_uint64, c_uint32, c_int64, c_void_p, c_void_p]),
    ("aecf_philox_host", c_float, [c_uint64, c_uint64, c_uint32, c_int64, c_void_p]),
    ("aecf_pool_forward", c_int, [POINTER(PoolDesc), POINTER(PoolFwdArgs), c_void_p]),
    ("aecf_pool_backward", c_int, [POINTER(PoolDesc), POINTER(PoolBwdArgs), c_void_p]),
    ("aecf_curriculum_mask_forward", c_int,
     [c_int64, c_int32, c_int32, c_int32, c_float, c_float, c_float, c_void_p, c_void_p, c_void_p,
      c_void_p, c_void_p, c_void_p, c_void_p]),
    ("aecf_curriculum_mask_backward", c_int,
     [c_int64, c_int32, c_int32, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("aecf_entropy_loss_workspace_bytes", c_size_t, [c_int64]),
    ("aecf_entropy_loss_from_partials", c_int, [c_int64, c_int32, c_void_p, c_void_p, c_void_p]),
    ("aecf_entropy_loss_fwd_bwd", c_int,
     [c_int64, c_int32, c_int32, c_float, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("aecf_sdpa_forward", c_int,
     [c_int64, c_int32, c_int32, c_int32, c_int32, c_float, c_void_p, c_void_p, c_void_p, c_void_p,
      c_void_p, c_void_p]),
    ("aecf_sdpa_backward", c_int,
     [c_int64, c_int32, c_int32, c_int32, c_int32, c_float, c_void_p, c_void_p, c_void_p, c_void_p,
      c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("aecf_mha_check", c_int, [POINTER(MhaDesc)]),
    ("aecf_mha_bwd_workspace_bytes", c_size_t, [POINTER(MhaDesc)]),
    ("aecf_mha_forward", c_int, [POINTER(MhaDesc), POINTER(MhaFwdArgs), c_void_p]),
    ("aecf_mha_backward", c_int, [POINTER(MhaDesc), POINTER(MhaBwdArgs), c_void_p]),
    ("aecf_modality_frontend", c_int, [c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("aecf_loss_fwd_bwd", c_int,
     [c_int64, c_int64, c_int64, c_int32, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
      c_int32, c_float, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    ("aecf_route_build", c_int, [c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("aecf_rows_gather", c_int, [c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    ("aecf_rows_select", c_int, [c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    ("aecf_front_pair", c_int, [c_int64, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("aecf_cast_f32_to_bf16", c_int, [c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("aecf_cast_f32_to_f16", c_int, [c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("aecf_adamw_step", c_int, [c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float,
                                c_float, c_float, c_float, c_void_p]),
    # mixed precision: + master[], param_dtype[], grad_dtype[] and the device scalars lr_dev, grad_scale, grad_coef, found_inf x 2
    ("aecf_adamw_mp_step", c_int, [c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_float, c_float, c_float, c_float, c_float, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_void_p]),
    # + ema[], ema_out[], ema_decay, ema_decay_dev: the step with the weights' moving average in the same launch
    ("aecf_adamw_mp_ema_step", c_int, [c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_float, c_float, c_float, c_float, c_float, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p]),
    ("aecf_ema_update", c_int, [c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p,
                                c_void_p, c_void_p]),
    ("aecf_grad_norm_workspace_bytes", c_size_t, [c_int32, c_void_p]),
    ("aecf_grad_norm", c_int, [c_int32, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    ("aecf_rows_split", c_int, [c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("aecf_l2norm_forward", c_int, [c_int64, c_int32, c_int32, c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("aecf_l2norm_backward", c_int, [c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("aecf_nce_workspace_bytes", c_size_t, [c_int64, c_int64, c_int32, c_int32]),
    ("aecf_nce_stream_workspace_bytes", c_size_t, [c_int64, c_int64, c_int32, c_int32]),
    ("aecf_nce_sym_workspace_bytes", c_size_t, [c_int64, c_int64, c_int32]),
    ("aecf_nce_sym_pass1", c_int,
     [c_int64, c_int64, c_int32, c_float, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    ("aecf_nce_sym_loss", c_int,
     [c_int64, c_int64, c_int64, c_int32, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_int64,
      c_int32, c_float, c_void_p, c_float, c_void_p, c_void_p, c_void_p]),
    ("aecf_nce_sym_grads", c_int,
     [c_int64, c_int64, c_int64, c_int32, c_float, c_float, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_int32,
      c_void_p, c_void_p, c_void_p]),
    ("aecf_nce_fwd_bwd", c_int,
     [c_int64, c_int64, c_int64, c_int32, c_int32, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p,
      c_void_p, c_void_p, c_size_t, c_void_p]),
    # device temperature: (const float* temperature, float min_temperature) in place of the float, + float* d_temperature
    ("aecf_nce_fwd_bwd_dt", c_int,
     [c_int64, c_int64, c_int64, c_int32, c_int32, c_void_p, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p,
      c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    ("aecf_loss_fwd_bwd_dt", c_int,
     [c_int64, c_int64, c_int64, c_int32, c_void_p, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
      c_void_p, c_int64, c_int32, c_float, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    ("aecf_nce_sym_pass1_dt", c_int,
     [c_int64, c_int64, c_int32, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    ("aecf_nce_sym_loss_dt", c_int,
     [c_int64, c_int64, c_int64, c_int32, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p,
      c_int64, c_int32, c_float, c_void_p, c_float, c_void_p, c_void_p, c_void_p]),
    ("aecf_nce_sym_grads_dt", c_int,
     [c_int64, c_int64, c_int64, c_int32, c_void_p, c_float, c_float, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p,
      c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    # sigmoid contrastive loss: device temperature and bias
    ("aecf_sig_workspace_bytes", c_size_t, [c_int64, c_int64, c_int32]),
    ("aecf_sig_pass1", c_int,
     [c_int64, c_int64, c_int64, c_int32, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p,
      c_void_p, c_void_p]),
    ("aecf_sig_grads", c_int,
     [c_int64, c_int64, c_int64, c_int32, c_void_p, c_float, c_float, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p,
      c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("aecf_sig_stream_workspace_bytes", c_size_t, [c_int64, c_int64, c_int32]),
    ("aecf_sig_stream_fwd_bwd", c_int,
     [c_int64, c_int64, c_int64, c_int32, c_void_p, c_float, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p,
      c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    # supervised contrastive loss, streaming: device temperature, int64 labels of the local rows and of the gathered keys
    ("aecf_supcon_workspace_bytes", c_size_t, [c_int64, c_int64, c_int32]),
    ("aecf_supcon_fwd_bwd", c_int,
     [c_int64, c_int64, c_int64, c_int32, c_void_p, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
      c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    # the pooled form (NT-Xent, SupCon over both views): the same call with the key at self_offset + i excluded for row i
    ("aecf_supcon_pool_fwd_bwd", c_int,
     [c_int64, c_int64, c_int64, c_int64, c_int32, c_void_p, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
      c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    # supervised contrastive loss, symmetric, on the tile GEMMs: pass 1 (column statistics out), loss, gradients
    ("aecf_supcon_sym_workspace_bytes", c_size_t, [c_int64, c_int64, c_int32]),
    ("aecf_supcon_sym_pass1", c_int,
     [c_int64, c_int64, c_int64, c_int32, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p,
      c_void_p]),
    ("aecf_supcon_sym_loss", c_int,
     [c_int64, c_int64, c_int64, c_int32, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    ("aecf_supcon_sym_grads", c_int,
     [c_int64, c_int64, c_int64, c_int32, c_void_p, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
      c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    # NT-Xent on the tile GEMMs: three logits blocks of one rank (a x b, a x a, b x b), one all-reduce of [cols] between the passes
    ("aecf_ntxent_sym_workspace_bytes", c_size_t, [c_int64, c_int64, c_int32]),
    ("aecf_ntxent_sym_pass1", c_int,
     [c_int64, c_int64, c_int64, c_int32, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p,
      c_void_p]),
    ("aecf_ntxent_sym_loss", c_int,
     [c_int64, c_int64, c_int64, c_int32, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    ("aecf_ntxent_sym_grads", c_int,
     [c_int64, c_int64, c_int64, c_int32, c_void_p, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
      c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    # symmetric InfoNCE with a key queue on the tile GEMMs: a x b plus two blocks against stored keys (Qa, Qb, capacity, device
    # count of valid slots), and the ring-buffer push (state = device int64 (cursor, valid))
    ("aecf_nce_queue_workspace_bytes", c_size_t, [c_int64, c_int64, c_int64, c_int32]),
    ("aecf_nce_queue_pass1", c_int,
     [c_int64, c_int64, c_int64, c_int32, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p,
      c_void_p, c_size_t, c_void_p, c_void_p]),
    ("aecf_nce_queue_loss", c_int,
     [c_int64, c_int64, c_int64, c_int32, c_void_p, c_float, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_size_t, c_void_p,
      c_void_p]),
    ("aecf_nce_queue_grads", c_int,
     [c_int64, c_int64, c_int64, c_int32, c_void_p, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p,
      c_void_p, c_void_p, c_size_t, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("aecf_key_queue_push", c_int, [c_int64, c_int32, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    # supervised contrastive loss with a key queue: the calls above plus row_labels, col_labels and the ring of stored labels
    # (int64, device) behind b_all; col_stats [3][cols]; the push that also writes the label ring (src_labels NULL: -1)
    ("aecf_supcon_queue_workspace_bytes", c_size_t, [c_int64, c_int64, c_int64, c_int32]),
    ("aecf_supcon_queue_pass1", c_int,
     [c_int64, c_int64, c_int64, c_int32, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p,
      c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    ("aecf_supcon_queue_loss", c_int,
     [c_int64, c_int64, c_int64, c_int32, c_void_p, c_float, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_size_t, c_void_p,
      c_void_p]),
    ("aecf_supcon_queue_grads", c_int,
     [c_int64, c_int64, c_int64, c_int32, c_void_p, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p,
      c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("aecf_key_queue_push_labeled", c_int,
     [c_int64, c_int32, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    # multi-view InfoNCE on the tile GEMMs: every pair of views of x [rows][views][d] in place, one all-reduce of [P][cols]
    ("aecf_nce_multi_workspace_bytes", c_size_t, [c_int64, c_int64, c_int32, c_int32, c_int32]),
    ("aecf_nce_multi_pass1", c_int,
     [c_int64, c_int64, c_int32, c_int32, c_int32, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    ("aecf_nce_multi_loss", c_int,
     [c_int64, c_int64, c_int64, c_int32, c_int32, c_int32, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
      c_void_p, c_void_p]),
    ("aecf_nce_multi_grads", c_int,
     [c_int64, c_int64, c_int64, c_int32, c_int32, c_int32, c_void_p, c_float, c_float, c_void_p, c_void_p, c_void_p, c_size_t,
      c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    # multi-view InfoNCE with missing views: presence bytes per row, per-pair coefficients formed on the device
    ("aecf_nce_multi_masked_workspace_bytes", c_size_t, [c_int64, c_int64, c_int32, c_int32, c_int32]),
    ("aecf_nce_multi_masked_pair_coef", c_int, [c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    ("aecf_nce_multi_masked_pass1", c_int,
     [c_int64, c_int64, c_int32, c_int32, c_int32, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
      c_void_p, c_void_p]),
    ("aecf_nce_multi_masked_loss", c_int,
     [c_int64, c_int64, c_int64, c_int32, c_int32, c_int32, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
      c_void_p, c_size_t, c_void_p, c_void_p]),
    ("aecf_nce_multi_masked_grads", c_int,
     [c_int64, c_int64, c_int64, c_int32, c_int32, c_int32, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
      c_size_t, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    # multi-view InfoNCE with a temperature and a weight per pair (pres pointers NULL: no view is missing)
    ("aecf_nce_multi_pp_workspace_bytes", c_size_t, [c_int64, c_int64, c_int32, c_int32, c_int32]),
    ("aecf_nce_multi_pp_pair_coef", c_int, [c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("aecf_nce_multi_pp_pass1", c_int,
     [c_int64, c_int64, c_int32, c_int32, c_int32, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p,
      c_size_t, c_void_p, c_void_p]),
    ("aecf_nce_multi_pp_loss", c_int,
     [c_int64, c_int64, c_int64, c_int32, c_int32, c_int32, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
      c_void_p, c_size_t, c_void_p, c_void_p]),
    ("aecf_nce_multi_pp_grads", c_int,
     [c_int64, c_int64, c_int64, c_int32, c_int32, c_int32, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
      c_size_t, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("aecf_l2norm_masked_forward", c_int,
     [c_int64, c_int32, c_int32, c_int32, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("aecf_l2norm_masked_backward", c_int, [c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    # pooled supervised contrastive loss on the tile GEMMs: NT-Xent's three blocks with labels, one all-reduce of [3][cols]
    ("aecf_supcon_pool_sym_workspace_bytes", c_size_t, [c_int64, c_int64, c_int32]),
    ("aecf_supcon_pool_sym_pass1", c_int,
     [c_int64, c_int64, c_int64, c_int32, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
      c_size_t, c_void_p, c_void_p]),
    ("aecf_supcon_pool_sym_loss", c_int,
     [c_int64, c_int64, c_int64, c_int32, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    ("aecf_supcon_pool_sym_grads", c_int,
     [c_int64, c_int64, c_int64, c_int32, c_void_p, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
      c_void_p, c_size_t, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    # pooled multi-label contrastive loss on the tile GEMMs: the pooled form with class sets and a weighting in place of the labels
    ("aecf_supcon_ml_pool_sym_workspace_bytes", c_size_t, [c_int64, c_int64, c_int32]),
    ("aecf_supcon_ml_pool_sym_pass1", c_int,
     [c_int64, c_int64, c_int64, c_int32, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32,
      c_void_p, c_size_t, c_void_p, c_void_p]),
    ("aecf_supcon_ml_pool_sym_loss", c_int,
     [c_int64, c_int64, c_int64, c_int32, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    ("aecf_supcon_ml_pool_sym_grads", c_int,
     [c_int64, c_int64, c_int64, c_int32, c_void_p, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
      c_int32, c_void_p, c_size_t, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    # multi-label contrastive loss, symmetric, on the tile GEMMs: class sets and a weighting in place of the labels
    ("aecf_supcon_ml_sym_workspace_bytes", c_size_t, [c_int64, c_int64, c_int32]),
    ("aecf_supcon_ml_sym_pass1", c_int,
     [c_int64, c_int64, c_int64, c_int32, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_size_t,
      c_void_p, c_void_p]),
    ("aecf_supcon_ml_sym_loss", c_int,
     [c_int64, c_int64, c_int64, c_int32, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    ("aecf_supcon_ml_sym_grads", c_int,
     [c_int64, c_int64, c_int64, c_int32, c_void_p, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p,
      c_size_t, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    # multi-label supervised contrastive loss: uint64 class sets in place of the labels, a weighting; the packing of multi-hot rows
    ("aecf_supcon_ml_workspace_bytes", c_size_t, [c_int64, c_int64, c_int32]),
    ("aecf_supcon_ml_fwd_bwd", c_int,
     [c_int64, c_int64, c_int64, c_int32, c_void_p, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p,
      c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    ("aecf_label_sets_pack", c_int, [c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    # retrieval ranks: positives, then greater / equal counts per row and per column
    ("aecf_retrieval_workspace_bytes", c_size_t, [c_int64, c_int64, c_int32]),
    ("aecf_retrieval_positive", c_int, [c_int64, c_int64, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("aecf_retrieval_ranks", c_int,
     [c_int64, c_int64, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
      c_void_p, c_size_t, c_void_p]),
    # top-k retrieval: values / indices of the k best columns of every row
    ("aecf_retrieval_topk_workspace_bytes", c_size_t, [c_int64, c_int64, c_int32, c_int32]),
    ("aecf_retrieval_topk", c_int,
     [c_int64, c_int64, c_int64, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    # multi-label evaluation: class-major keys + compacted positives, the four compare-and-count integers, float64 shares [5][C]
    ("aecf_mlmetrics_workspace_bytes", c_size_t, [c_int64, c_int32]),
    ("aecf_mlmetrics_prepare", c_int, [c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    ("aecf_mlmetrics_counts", c_int, [c_int64, c_int32, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    ("aecf_mlmetrics_finalize", c_int,
     [c_int64, c_int32, c_int64, c_int64, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    # multi-label bootstrap: the stable descending order by counting, the multiplicities uint8 [n_all][Rp], the walk with one lane
    # per replicate -> int64 [replicates][7][C]
    ("aecf_mlboot_workspace_bytes", c_size_t, [c_int64, c_int32]),
    ("aecf_mlboot_draw_workspace_bytes", c_size_t, [c_int64, c_int32]),
    ("aecf_mlboot_order", c_int,
     [c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    ("aecf_mlboot_draw", c_int, [c_int64, c_int32, c_int64, c_uint64, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    ("aecf_mlboot_walk", c_int, [c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    # multi-label classification loss (BCE / focal / asymmetric): per-class stats + totals, then the gradient in one pass
    ("aecf_mlloss_workspace_bytes", c_size_t, [c_int64, c_int32]),
    ("aecf_mlloss_forward", c_int,
     [c_int64, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, c_float, c_float, c_int32,
      c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    ("aecf_mlloss_backward", c_int,
     [c_int64, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, c_float, c_float, c_int32,
      c_void_p, c_void_p, c_float, c_void_p, c_void_p]),
    # fused classifier head: that loss of h W^T + bias and dh / dW / dbias on the streaming loop, nothing of size n x classes
    ("aecf_mlhead_workspace_bytes", c_size_t, [c_int64, c_int32, c_int32]),
    ("aecf_mlhead_forward", c_int,
     [c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float,
      c_float, c_float, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    ("aecf_mlhead_backward", c_int,
     [c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float,
      c_float, c_float, c_int32, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
      c_size_t, c_void_p]),
    # multi-label calibration: reliability bins + Brier + NLL per class, the Newton sums of a scaling fit and its damped step
    ("aecf_mlcal_workspace_bytes", c_size_t, [c_int64, c_int32, c_int32]),
    ("aecf_mlcal_stats", c_int,
     [c_int64, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_size_t,
      c_void_p]),
    ("aecf_mlcal_fit_sums", c_int,
     [c_int64, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    ("aecf_mlcal_fit_update", c_int, [c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
]
SYMBOL_NAMES = [s[0] for s in _SYMBOLS]

_lib = None


def load() -> ctypes.CDLL:
    """Load libaecf_hip.so once.  Raises RuntimeError (never falls back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"aecf_amd: HIP library not found at {LIB_PATH}. Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` or `make -C aecf_amd/csrc`. "
            "There is no CPU / PyTorch fallback for the fusion path.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, restype, argtypes in _SYMBOLS:
        try:
            fn = getattr(lib, name)
        except AttributeError as e:  # pragma: no cover - build error
            raise RuntimeError(f"aecf_amd: {LIB_PATH} does not export {name}") from e
        fn.restype = restype
        fn.argtypes = argtypes
    ver = lib.aecf_abi_version()
    if ver != AECF_ABI_VERSION:
        raise RuntimeError(f"aecf_amd: ABI version mismatch: library {ver}, binding {AECF_ABI_VERSION}")
    _lib = lib
    return lib


def status_string(status: int) -> str:
    return load().aecf_status_string(status).decode()


def check(status: int, what: str) -> None:
    if status != 0:
        raise RuntimeError(f"aecf_amd: {what} failed: {status_string(status)} (status {status})")
