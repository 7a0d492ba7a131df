"""ctypes binding of include/umlh.h + the in-tree hipcc build of libumlh.so."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
_PKG = os.path.dirname(_HERE)
_ROOT = os.path.dirname(_PKG)
_CSRC = os.path.join(_PKG, "csrc")
_INCLUDE = os.path.join(_ROOT, "include")
_SO = os.path.join(_HERE, "libumlh.so")

OPT_IDS = {"sgd": 0, "adam": 1, "adamw": 2}          # engine/optimizer/optim.py:6 AVAI_OPTIMS
PREC_IDS = {"fp32": 0, "bf16": 1}
(S_LOSS_IMG, S_LOSS_TXT, S_ACC_IMG, S_ACC_TXT, S_GSCALE_IMG, S_GSCALE_TXT, S_CORRECT, S_LOSS_SUM,
 S_GRAD_DOT, S_GRAD_N2_IMG, S_GRAD_N2_TXT, S_GRAD_AGREE) = range(12)
N_CORE_SCALARS = 8
N_SCALARS = 12

SOURCES = ["umlh_p2p.hip", "umlh_kernels_f32.hip", "umlh_kernels_bf16.hip", "umlh_kernels_micro.hip", "umlh_kernels_seq.hip", "umlh_kernels_enc.hip", "umlh_kernels_align.hip", "umlh_kernels_align_ext.hip", "umlh_kernels_probe.hip", "umlh_kernels_softmax_probe.hip", "umlh_kernels_knn.hip", "umlh_kernels_spectral.hip", "umlh_kernels_capture.hip", "umlh_kernels_stepstats.hip", "umlh_kernels_rollout.hip", "umlh_kernels_classstats.hip", "umlh_kernels_evalreport.hip", "umlh_kernels_outlier.hip", "umlh_kernels_seqload.hip", "umlh_kernels_tabular.hip", "umlh_kernels_gauss.hip", "umlh_api.cpp", "umlh_ops.cpp", "umlh_encoder.cpp"]


class UmlhError(RuntimeError):
    pass


class Config(C.Structure):
    _fields_ = [("d_img", C.c_int32), ("d_shared", C.c_int32), ("num_classes", C.c_int32),
                ("has_proj", C.c_int32), ("learnable_temp", C.c_int32), ("optimizer", C.c_int32),
                ("precision", C.c_int32), ("max_rows_img", C.c_int32), ("max_rows_txt", C.c_int32),
                ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("momentum", C.c_double),
                ("weight_decay", C.c_double)]


class Buffers(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("w_head", "m_head", "v_head", "w_proj", "m_proj", "v_proj",
                                          "scales", "m_scales", "v_scales", "workspace")] + \
               [("workspace_bytes", C.c_uint64)]


class Batch(C.Structure):
    _fields_ = [("feats", C.c_void_p), ("labels", C.c_void_p), ("index", C.c_void_p),
                ("rows", C.c_int32), ("global_rows", C.c_int32), ("feats_bf16", C.c_void_p)]


class Stream(C.Structure):
    _fields_ = [("feats", C.c_void_p), ("feats_bf16", C.c_void_p), ("labels", C.c_void_p), ("index", C.c_void_p),
                ("offsets", C.POINTER(C.c_int32))]


SPAN_FEISTEL, SPAN_TABLE, SPAN_IOTA = range(3)      # UMLH_SPAN_*


class IndexSpanDesc(C.Structure):                  # umlh_index_span_t
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("n", C.c_int64), ("seed", C.c_uint64), ("order", C.c_void_p),
                ("start", C.c_int64), ("count", C.c_int64)]


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p)   # umlh_allreduce_fn
COMM_ID_BYTES = 128


class GroupItem(C.Structure):
    _fields_ = [("handle", C.c_void_p), ("img", C.POINTER(Stream)), ("txt", C.POINTER(Stream)),
                ("lr", C.POINTER(C.c_double)), ("first_step", C.c_int64), ("alpha", C.c_float), ("img_alpha", C.c_float),
                ("scalars_out", C.c_void_p)]


class EncLayer(C.Structure):
    _fields_ = [("T", C.c_int32), ("B", C.c_int32), ("Z", C.c_int32), ("H", C.c_int32), ("d_ff", C.c_int32),
                ("p", C.c_float), ("eps", C.c_float), ("seed", C.c_uint64), ("seed_device", C.c_void_p)]


class Hyper(C.Structure):
    _fields_ = [("lr", C.c_double), ("step", C.c_int64), ("alpha", C.c_float), ("img_alpha", C.c_float),
                ("flags", C.c_int32), ("reserved", C.c_int32)]


class AeCfg(C.Structure):                          # umlh_ae_cfg_t
    _fields_ = [("dim_obs", C.c_int32), ("dim_common", C.c_int32), ("dim_latent", C.c_int32)]


class AeGroupItem(C.Structure):                    # umlh_ae_group_item_t: one run of umlh_ae_train_steps_grouped
    _fields_ = [("cfg", AeCfg), ("P", C.POINTER(C.c_void_p)), ("M", C.POINTER(C.c_void_p)), ("V", C.POINTER(C.c_void_p)),
                ("x", C.c_void_p), ("ldx", C.c_int64), ("idx_x", C.c_void_p), ("batch_x", C.c_int32),
                ("y", C.c_void_p), ("ldy", C.c_int64), ("idx_y", C.c_void_p), ("batch_y", C.c_int32),
                ("backward_y", C.c_int32), ("alpha_x", C.c_float), ("alpha_y", C.c_float),
                ("optimizer", C.c_int32), ("lr", C.c_double), ("first_step", C.c_int64), ("beta1", C.c_double), ("beta2", C.c_double),
                ("eps", C.c_double), ("momentum", C.c_double), ("weight_decay", C.c_double), ("losses", C.c_void_p)]


class AeEvalItem(C.Structure):                     # umlh_ae_eval_item_t: one run of umlh_ae_forward_grouped
    _fields_ = [("cfg", AeCfg), ("P", C.POINTER(C.c_void_p)),
                ("x", C.c_void_p), ("ldx", C.c_int64), ("idx_x", C.c_void_p), ("n_x", C.c_int32),
                ("y", C.c_void_p), ("ldy", C.c_int64), ("idx_y", C.c_void_p), ("n_y", C.c_int32),
                ("losses", C.c_void_p), ("rec_x", C.c_void_p), ("rec_y", C.c_void_p), ("emb_x", C.c_void_p), ("emb_y", C.c_void_p)]


AE_MAX_GROUP = 64                                  # UMLH_AE_MAX_GROUP


class AlignPair(C.Structure):                      # umlh_align_pair_t: one member of umlh_align_pairs
    _fields_ = [("a", C.c_void_p), ("lda", C.c_int32), ("d_a", C.c_int32), ("b", C.c_void_p), ("ldb", C.c_int32), ("d_b", C.c_int32),
                ("n", C.c_int64), ("cka", C.c_int32), ("topk", C.c_int32), ("out5", C.c_void_p), ("knn_a", C.c_void_p),
                ("knn_b", C.c_void_p), ("scores_a", C.c_void_p), ("scores_b", C.c_void_p)]


ALIGN_MAX_PAIRS = 64                               # UMLH_ALIGN_MAX_PAIRS


class RolloutCfg(C.Structure):
    _fields_ = [("Z", C.c_int32), ("d_ff", C.c_int32), ("D", C.c_int32), ("n_layers", C.c_int32), ("steps", C.c_int32),
                ("eps", C.c_float)]


def _prototypes() -> dict:
    """name -> (restype, argtypes) of every declaration of include/umlh.h, in the header's order and sections.
    tests/test_abi_cpu.py parses the header and holds this table to it, both ways."""
    rc, vp, i32, i64, u64, f32, f64 = C.c_int, C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_float, C.c_double
    P, pv = C.POINTER, C.POINTER(C.c_void_p)
    cfg, batch, hyper, stream, enc = P(Config), P(Batch), P(Hyper), P(Stream), P(EncLayer)
    return {
        "umlh_last_error": (C.c_char_p, ()),
        "umlh_version": (rc, ()),
        # handle
        "umlh_workspace_bytes": (u64, (cfg,)),
        "umlh_create": (rc, (cfg, pv)),
        "umlh_destroy": (rc, (vp,)),
        "umlh_bind": (rc, (vp, P(Buffers))),
        "umlh_enable_diagnostics": (rc, (vp, i32)),
        "umlh_set_diagnostic_columns": (rc, (vp, i32)),
        "umlh_freeze_proj_row": (rc, (vp, i32)),
        # forward pieces and the fused step
        "umlh_zero_shot_init": (rc, (vp, vp, vp, i64, vp)),
        "umlh_logits": (rc, (vp, batch, C.c_int, vp, vp)),
        "umlh_project": (rc, (vp, batch, vp, vp)),
        "umlh_train_step": (rc, (vp, batch, batch, hyper, vp, vp)),
        # multi-step, grouped and micro-step launches
        "umlh_train_steps": (rc, (vp, stream, stream, i32, P(f64), i64, f32, f32, vp, vp)),
        "umlh_train_steps_grouped": (rc, (P(GroupItem), i32, i32, vp)),
        "umlh_micro_status": (rc, (vp, P(i32))),
        "umlh_micro_launches": (rc, (vp, P(i64))),
        "umlh_step_status": (rc, (vp, P(i32))),
        # peer-to-peer all-reduce
        "umlh_p2p_region_bytes": (u64, (i64, i32)),
        "umlh_p2p_alloc": (rc, (u64, pv)),
        "umlh_p2p_free": (rc, (vp,)),
        "umlh_p2p_export": (rc, (vp, vp)),
        "umlh_p2p_open": (rc, (vp, pv)),
        "umlh_p2p_close": (rc, (vp,)),
        "umlh_p2p_attach": (rc, (vp, pv, i32, i32)),
        "umlh_step_launches": (rc, (vp, P(i64))),
        # data-parallel transport and split step
        "umlh_comm_unique_id": (rc, (vp,)),
        "umlh_comm_init_rank": (rc, (vp, vp, i32, i32)),
        "umlh_set_comm": (rc, (vp, vp, i32)),
        "umlh_set_allreduce": (rc, (vp, ALLREDUCE_FN, vp, i32)),
        "umlh_grad_step": (rc, (vp, batch, batch, hyper, vp)),
        "umlh_grad_buffer": (rc, (vp, pv, P(u64))),
        "umlh_debug_buffer": (rc, (vp, pv, P(u64))),
        "umlh_apply_update": (rc, (vp, hyper, vp, vp)),
        # evaluation, profiling, bf16 shadow
        "umlh_eval_batch": (rc, (vp, batch, vp, vp)),
        "umlh_eval_rows": (rc, (vp, batch, vp, vp)),
        "umlh_profile_enable": (rc, (vp, C.c_int)),
        "umlh_profile_read": (rc, (vp, P(f32))),
        "umlh_to_bf16": (rc, (vp, vp, i64, vp)),
        # MultiBench critics: next-step MSE decoder, InfoNCE
        "umlh_seq_mse_forward": (rc, (vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp)),
        "umlh_seq_mse_backward": (rc, (vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp)),
        "umlh_seq_mse_backward_scratch_floats": (u64, (i32, i32, i32, i32)),
        "umlh_infonce_forward": (rc, (vp, vp, i32, i32, f32, vp, vp, vp, vp, vp, vp, vp)),
        "umlh_infonce_backward": (rc, (vp, vp, vp, vp, vp, i32, i32, f32, vp, vp, vp)),
        # MultiBench shared encoder: ops
        "umlh_gemm_f32": (rc, (vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, f32, i32, vp, vp)),
        "umlh_bias_act": (rc, (vp, vp, i64, i32, i32, vp)),
        "umlh_relu_backward": (rc, (vp, vp, i64, vp)),
        "umlh_dropout": (rc, (vp, i64, f32, u64, vp)),
        "umlh_add_inplace": (rc, (vp, vp, i64, vp)),
        "umlh_colsum": (rc, (vp, i32, i32, vp, vp)),
        "umlh_add_layernorm_forward": (rc, (vp, vp, vp, vp, i32, i32, f32, vp, vp, vp, vp, vp)),
        "umlh_layernorm_backward": (rc, (vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp)),
        "umlh_add_positions": (rc, (vp, vp, i32, i32, i32, vp)),
        "umlh_positions_backward": (rc, (vp, i32, i32, i32, vp, vp)),
        "umlh_gather_rows": (rc, (vp, vp, i32, i32, vp, i32, vp)),
        "umlh_attention_forward": (rc, (vp, vp, i32, i32, i32, i32, f32, u64, vp, vp, vp)),
        "umlh_attention_backward": (rc, (vp, vp, vp, vp, i32, i32, i32, i32, f32, u64, vp, vp)),
        # MultiBench shared encoder: layer, stack, plan
        "umlh_encoder_layer_saved_floats": (u64, (enc,)),
        "umlh_encoder_layer_scratch_floats": (u64, (enc,)),
        "umlh_encoder_layer_forward": (rc, (enc, pv, vp, vp, vp, vp, vp, vp)),
        "umlh_encoder_layer_backward": (rc, (enc, pv, vp, vp, vp, vp, vp, pv, vp, vp)),
        "umlh_encoder_stack_forward": (rc, (enc, i32, pv, vp, vp, vp, vp, vp, vp)),
        "umlh_encoder_stack_backward": (rc, (enc, i32, pv, vp, vp, vp, vp, vp, vp, pv, vp, vp, vp)),
        "umlh_encoder_plan_floats": (u64, (enc, i32)),
        "umlh_encoder_plan_create": (rc, (enc, i32, pv, i32, vp, pv)),
        "umlh_encoder_plan_offsets": (rc, (vp, P(u64))),
        "umlh_encoder_plan_forward": (rc, (vp, u64, vp)),
        "umlh_encoder_plan_backward": (rc, (vp, vp)),
        "umlh_encoder_plan_destroy": (None, (vp,)),
        # permutation, standalone optimizer
        "umlh_random_permutation": (rc, (i64, u64, vp, vp)),
        "umlh_index_block": (rc, (P(IndexSpanDesc), i32, vp, P(IndexSpanDesc), i32, vp, vp)),
        "umlh_optimizer_step": (rc, (i32, vp, vp, vp, vp, i64, f64, i64, f64, f64, f64, f64, f64, vp)),
        "umlh_optimizer_step_multi": (rc, (i32, i32, pv, pv, pv, pv, P(i64), f64, i64, f64, f64, f64, f64, f64, vp)),
        # alignment metrics
        "umlh_align_scratch_bytes": (u64, (i64, i32, i32, i32, i32)),
        "umlh_align_knn": (rc, (vp, i64, i32, i32, i32, i32, vp, vp, vp, u64, vp)),
        "umlh_align_mutual_knn": (rc, (vp, vp, i64, i32, vp, vp, u64, vp)),
        "umlh_align_cka": (rc, (vp, i32, i32, vp, i32, i32, i64, i32, vp, vp, u64, vp)),
        "umlh_align_ext_scratch_bytes": (u64, (i32, i64, i32, i32, i32, i32)),
        "umlh_align_cka_unbiased": (rc, (vp, i32, i32, vp, i32, i32, i64, i32, vp, vp, u64, vp)),
        "umlh_align_cka_rbf": (rc, (vp, i32, i32, vp, i32, i32, i64, f64, i32, i32, vp, vp, u64, vp)),
        "umlh_align_cknna": (rc, (vp, vp, vp, vp, i64, i32, vp, vp, u64, vp)),
        "umlh_align_list_stats": (rc, (vp, vp, i64, i32, vp, vp, vp, u64, vp)),
        "umlh_align_pairs_scratch": (u64, (P(AlignPair), i32, i32)),
        "umlh_align_pairs": (rc, (P(AlignPair), i32, i32, vp, u64, vp)),
        # linear probes
        "umlh_masked_mean": (rc, (vp, i32, i32, i32, i64, i64, vp, vp, i32, vp)),
        "umlh_probe_scratch_bytes": (u64, (i64, i32, i32)),
        "umlh_probe_column_stats": (rc, (vp, i64, i32, i32, vp, vp, u64, vp)),
        "umlh_probe_fit": (rc, (vp, i64, i32, i32, vp, vp, i32, f64, i32, f64, vp, vp, vp, vp, u64, vp)),
        "umlh_probe_score": (rc, (vp, i64, i32, i32, vp, vp, vp, vp, vp, vp)),
        # multinomial logistic probe
        "umlh_softmax_probe_scratch_bytes": (u64, (i64, i32, i32, i32, i32)),
        "umlh_softmax_probe_eval": (rc, (vp, i64, i32, i32, vp, vp, i32, f64, vp, i32, vp, vp, i32, vp, vp, u64, vp)),
        "umlh_softmax_probe_fit": (rc, (vp, i64, i32, i32, vp, vp, i32, f64, i32, i32, f64, i32, vp, i32, vp, vp, vp, u64, vp)),
        "umlh_softmax_probe_fold": (rc, (vp, i32, i32, i32, vp, vp, i32, vp, vp)),
        # k-nearest-neighbour probe
        "umlh_knn_scratch_bytes": (u64, (i64, i64, i32, i32, i32)),
        "umlh_knn_search": (rc, (vp, i64, i32, vp, i64, i32, i32, i32, i32, vp, vp, vp, u64, vp)),
        "umlh_knn_vote": (rc, (vp, i64, i32, vp, i64, vp, vp, vp, vp, vp)),
        # singular values and effective rank
        "umlh_spectral_scratch_bytes": (u64, (i32, i64, i32)),
        "umlh_svdvals": (rc, (vp, i32, i64, i32, i64, i64, vp, vp, u64, vp)),
        "umlh_effective_rank": (rc, (vp, i32, i64, i32, i64, i64, f64, vp, vp, vp, u64, vp)),
        "umlh_effective_rank_seq": (rc, (vp, i32, i32, i32, i64, i64, vp, i32, f64, vp, vp, vp, u64, vp)),
        # principal subspaces and SVCCA
        "umlh_subspace_scratch_bytes": (u64, (i64, i32, i32, i32)),
        "umlh_principal_subspace": (rc, (vp, i64, i32, i64, i32, i32, vp, vp, vp, u64, vp)),
        "umlh_svcca": (rc, (vp, vp, i64, i32, i32, i64, i64, i32, vp, vp, vp, vp, u64, vp)),
        # embedding capture: ragged row compaction, mean paired cosine
        "umlh_seq_compact": (rc, (vp, i32, i32, i32, i64, i64, vp, i32, vp, i64, i64, vp, vp)),
        "umlh_paired_cosine_scratch_bytes": (u64, (i64, i32)),
        "umlh_paired_cosine": (rc, (vp, i64, vp, i64, i64, i32, f64, vp, vp, vp, u64, vp)),
        # per-step logged statistics: trivial next-frame error, masked reconstruction error
        "umlh_seq_step_stats_scratch_bytes": (u64, (i32, i32, i32)),
        "umlh_seq_step_stats": (rc, (vp, i64, i64, vp, i64, i64, i32, i32, i32, vp, vp, vp, u64, vp)),
        # rollout and spectral-bias spectra
        "umlh_rollout": (rc, (P(RolloutCfg), pv, vp, vp, vp, vp, vp, vp, vp, i64, i64, vp, i64, i64, vp)),
        "umlh_seq_spectrum_scratch_bytes": (u64, (i32, i32, i32)),
        "umlh_seq_spectrum": (rc, (vp, i64, i64, i32, i32, i32, vp, vp, u64, vp)),
        # class index and class statistics of the feature capture
        "umlh_class_index_scratch_bytes": (u64, (i64, i32)),
        "umlh_class_index": (rc, (vp, i64, i32, vp, vp, vp, u64, vp)),
        "umlh_class_stats_scratch_bytes": (u64, (i64, i32, i32)),
        "umlh_class_stats": (rc, (vp, i64, i64, i32, vp, vp, i32, vp, i64, vp, vp, vp, u64, vp)),
        # class-wise validation report: top-k classes per row, per-class counters
        "umlh_eval_topk_scratch_bytes": (u64, (i64, i64, i32, i32, i32)),
        "umlh_eval_topk": (rc, (vp, i64, i32, vp, i64, i32, i32, vp, vp, i32, i32, vp, vp, vp, u64, vp)),
        "umlh_eval_classwise": (rc, (vp, i64, i32, vp, i64, vp, vp, vp, vp, vp, vp)),
        # outlier clamp and feature preparation: row quantile and global k-th of |x|, clamp (+ normalise), k-NN accuracy
        "umlh_outlier_scratch_bytes": (u64, (i32, i64, i64)),
        "umlh_row_abs_quantile": (rc, (vp, i64, i64, i64, f64, vp, vp, vp, vp, vp, vp, u64, vp)),
        "umlh_abs_kth": (rc, (vp, i64, i64, i64, i64, vp, vp, u64, vp)),
        "umlh_clamp_rows": (rc, (vp, i64, i64, i64, vp, i32, vp, i64, vp)),
        "umlh_knn_accuracy": (rc, (vp, i64, i64, i64, vp, vp, u64, vp)),
        # robustness test sets: time-series noise on a table of the device loader
        "umlh_seq_perturb": (rc, (vp, i64, i32, i32, i32, vp, vp, f32, u64, vp, vp, vp)),
        # MIMIC loader: standardisation of a cleaned float / double table, tabular noise, row gather
        "umlh_tab_standardize_scratch": (u64, (i64, i32)),
        "umlh_tab_standardize": (rc, (vp, i32, i64, i32, i64, vp, i64, vp, vp, u64, vp)),
        "umlh_tab_perturb": (rc, (vp, i64, i32, i64, vp, vp, f32, f32, u64, vp, i64, vp)),
        "umlh_rows_gather": (rc, (pv, P(i32), i32, i64, vp, i32, pv, vp)),
        # the Gaussian toy's autoencoder: forward, fused training steps
        "umlh_ae_scratch": (u64, (P(AeCfg), i32, i32, i32)),
        "umlh_ae_forward": (rc, (P(AeCfg), pv, vp, i64, vp, i32, vp, i64, vp, i32, vp, vp, vp, vp, vp, vp, u64, vp)),
        "umlh_ae_train_steps": (rc, (P(AeCfg), pv, pv, pv, vp, i64, vp, i32, vp, i64, vp, i32, i32, i32, f32, f32, i32, f64, i64,
                                     f64, f64, f64, f64, f64, vp, vp, u64, vp)),
        "umlh_ae_group_scratch": (u64, (P(AeGroupItem), i32, i32)),
        "umlh_ae_eval_group_scratch": (u64, (P(AeEvalItem), i32)),
        "umlh_ae_train_steps_grouped": (rc, (P(AeGroupItem), i32, i32, vp, u64, vp)),
        "umlh_ae_forward_grouped": (rc, (P(AeEvalItem), i32, vp, u64, vp)),
        # device loader of the affect datasets: first nonzero row, column and per-sequence standardisation, batch gather-pad
        "umlh_seq_first_nonzero": (rc, (vp, i64, i32, i32, vp, vp)),
        "umlh_seq_column_standardize_scratch": (u64, (i64, i32)),
        "umlh_seq_column_standardize": (rc, (vp, i64, i32, i64, vp, i64, vp, vp, u64, vp)),
        "umlh_seq_standardize": (rc, (vp, i64, i32, i32, vp, vp)),
        "umlh_seq_gather_pad": (rc, (pv, P(i32), i32, i64, i32, vp, vp, i32, i32, pv, vp, vp)),
    }


PROTOTYPES = _prototypes()
EXPORTS = list(PROTOTYPES)


def lib_path() -> str:
    return _SO


def build_library(force: bool = False, verbose: bool = False) -> str:
    """Cross-compile the HIP sources for gfx950 into umlh/libumlh.so (in-tree, so the
    binary travels with the repo snapshot to the GPU box)."""
    srcs = [os.path.join(_CSRC, s) for s in SOURCES]
    deps = srcs + [os.path.join(_CSRC, h) for h in os.listdir(_CSRC) if h.endswith(".h")] + [os.path.join(_INCLUDE, "umlh.h")]
    if not force and os.path.exists(_SO) and all(os.path.getmtime(_SO) >= os.path.getmtime(d) for d in deps):
        return _SO
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
           "-I", _INCLUDE, "-I", _CSRC, *srcs, "-o", _SO + ".tmp"]
    if os.environ.get("UMLH_BUILD_ABLATIONS") == "1":     # kernel-analysis build: timing-only work-skipping switches
        cmd.insert(1, "-DUMLH_ABLATIONS")
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise UmlhError(f"hipcc failed ({res.returncode}):\n{res.stderr[-4000:]}")
    os.replace(_SO + ".tmp", _SO)
    return _SO


_LIB = None


def load_library():
    """dlopen libumlh.so and declare every prototype of include/umlh.h.  Raises
    UmlhError if the extension has not been built: there is no fallback path."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(_SO):
        raise UmlhError(f"{_SO} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                        "(hipcc --offload-arch=gfx950). The HIP extension is mandatory; there is no CPU fallback.")
    lib = C.CDLL(_SO)
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, list(argtypes)
    _LIB = lib
    return lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load_library().umlh_last_error()
        raise UmlhError(f"{what} failed with code {rc}: {msg.decode() if msg else ''}")
