"""ctypes binding of libradvlm_hip.so (the C ABI declared in include/radvlm_hip.h).

The product path has no fallback: if the shared library is missing or a kernel returns an error code, this
module raises.  Tensors are plain torch CUDA(HIP) tensors used only as device memory; every call is
asynchronous on the current torch stream.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libradvlm_hip.so")

_c_void_p = ctypes.c_void_p
_i64 = ctypes.c_int64
_i32 = ctypes.c_int
_f32 = ctypes.c_float
_f64 = ctypes.c_double

ACT_NONE, ACT_QUICK_GELU, ACT_GELU, ACT_GELU_TANH = 0, 1, 2, 3

_SIGS = {
    "rv_gemm_nt_bf16": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _c_void_p, _i64, _i32, _i32, _i32,
                        _i32, _i32, _i32, _c_void_p, _c_void_p],
    "rv_gemm_bf16": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _c_void_p, _i64, _i32, _i32, _i32, _i32, _i32,
                     _f32, _i32, _i32, _i32, _c_void_p, _c_void_p],
    "rv_gemm_bf16_ex": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _c_void_p, _i64, _i32, _i32, _i32, _i32, _i32,
                        _f32, _i32, _i32, _i32, _c_void_p, _i64, _c_void_p, _i64, _i32, _c_void_p, _i64, _c_void_p, _c_void_p],
    "rv_gemm_plan": [_i32, _i32, _i32, _i32, _i32, _i64, _i64, _i32, _i64, _i64, _i64, _i32, ctypes.POINTER(ctypes.c_int32)],
    "rv_gemm_rope_bf16": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i32, _i32, _i32, _c_void_p, _c_void_p, _i32, _i32, _i32,
                          _c_void_p, _i64, _c_void_p, _c_void_p],
    "rv_gemm_swiglu_fwd_bf16": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _i32, _i32, _i32, _c_void_p, _i64, _c_void_p,
                                _c_void_p],
    "rv_gemm_swiglu_bwd_bf16": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _i32, _i32, _i32, _c_void_p,
                                _i64, _c_void_p, _c_void_p],
    "rv_dropout_bf16": [_c_void_p, _c_void_p, _i64, _f32, ctypes.c_uint64, _c_void_p],
    "rv_dropout_add_bf16": [_c_void_p, _c_void_p, _i64, _f32, ctypes.c_uint64, _c_void_p],
    "rv_gemm_dropout_add_bf16": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _i32, _i32, _i32, _i32, _f32, _f32, ctypes.c_uint64, _i32, _c_void_p,
                                 _c_void_p],
    "rv_lora_a_grad_bf16": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _i32, _i32, _i32, _f32, ctypes.c_uint64, _i32, _c_void_p, _i64, _c_void_p],
    "rv_lora_down_bf16": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _i32, _i32, _i32, _f32, _f32, ctypes.c_uint64, _c_void_p, _c_void_p],
    "rv_transpose_bf16": [_c_void_p, _i64, _i64, _i64, _c_void_p, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _c_void_p],
    "rv_rmsnorm_fwd": [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _i32, _i32, _f32, _c_void_p],
    "rv_rmsnorm_bwd": [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _i32, _c_void_p, _i32, _i32, _i32, _c_void_p],
    "rv_layernorm_fwd": [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _i32, _i32, _f32, _c_void_p],
    "rv_layernorm_bwd": [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _i32, _c_void_p, _i32, _i32, _i32, _c_void_p],
    "rv_quick_gelu_fwd": [_c_void_p, _c_void_p, _i64, _c_void_p],
    "rv_quick_gelu_bwd": [_c_void_p, _c_void_p, _c_void_p, _i64, _c_void_p],
    "rv_colsum_f32": [_c_void_p, _i32, _i32, _c_void_p, _i32, _c_void_p],
    "rv_colsum_partial_bf16": [_c_void_p, _i64, _i32, _i32, _c_void_p, _i32, _c_void_p],
    "rv_rope_inplace": [_c_void_p, _i64, _c_void_p, _i32, _i32, _i32, _i32, _i32, _i32, _c_void_p],
    "rv_attn_fwd": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _c_void_p, _i64, _c_void_p, _c_void_p, _i32, _i32, _i32, _i32,
                    _i32, _i32, _f32, _c_void_p, _c_void_p],
    "rv_attn_bwd": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _c_void_p,
                    _c_void_p, _c_void_p, _c_void_p, _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i32, _i32,
                    _i32, _i32, _i32, _i32, _f32, _c_void_p, _c_void_p],
    "rv_attn_fwd_gqa": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _i32, _i32, _i32,
                        _i32, _i32, _i32, _i32, _f32, _c_void_p, _c_void_p],
    "rv_attn_bwd_gqa": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _c_void_p,
                        _c_void_p, _c_void_p, _c_void_p, _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _c_void_p, _i32,
                        _i32, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _c_void_p, _i64, _c_void_p, _c_void_p],
    "rv_attn_fwd_nat": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _i32, _i32, _i32,
                        _i32, _i32, _i32, _i32, _f32, _c_void_p, _c_void_p],
    "rv_attn_bwd_nat": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _i64,
                        _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _c_void_p, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _c_void_p, _i64,
                        _c_void_p, _c_void_p, _c_void_p, _c_void_p],
    "rv_attn_bwd_gqa_rope": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _c_void_p,
                             _c_void_p, _c_void_p, _c_void_p, _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _c_void_p, _i32,
                             _i32, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _c_void_p],
    "rv_transpose_bf16_varlen": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _i32,
                                 _c_void_p],
    "rv_rope_inplace_pos": [_c_void_p, _i64, _c_void_p, _c_void_p, _i32, _i32, _i32, _i32, _i32, _c_void_p],
    "rv_gelu_tanh_fwd": [_c_void_p, _c_void_p, _i64, _c_void_p],
    "rv_gelu_tanh_bwd": [_c_void_p, _c_void_p, _c_void_p, _i64, _c_void_p],
    "rv_weighted_segment_sum_rows": [_c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _i32, _c_void_p, _i64, _i32,
                                     _c_void_p],
    "rv_max4_rows_fwd": [_c_void_p, _i64, _c_void_p, _c_void_p, _i32, _c_void_p, _i64, _c_void_p, _i32, _c_void_p],
    "rv_max4_rows_bwd": [_c_void_p, _i64, _c_void_p, _c_void_p, _i32, _c_void_p, _c_void_p, _i64, _i32, _c_void_p],
    "rv_add_pos_rows": [_c_void_p, _c_void_p, _i32, _i32, _i32, _c_void_p],
    "rv_swiglu_fwd": [_c_void_p, _i64, _c_void_p, _i64, _i32, _i32, _c_void_p],
    "rv_swiglu_bwd": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _i32, _i32, _c_void_p],
    "rv_gelu_fwd": [_c_void_p, _c_void_p, _i64, _c_void_p],
    "rv_gelu_bwd": [_c_void_p, _c_void_p, _c_void_p, _i64, _c_void_p],
    "rv_cross_entropy": [_c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _i64, _i32, _i32, _f32, _c_void_p],
    "rv_sum_f32": [_c_void_p, _i64, _f32, _c_void_p, _c_void_p],
    "rv_policy_loss_bf16": [_c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _f32, _f32, _f32, _c_void_p,
                            _c_void_p, _i64, _i32, _i32, _c_void_p],
    "rv_seq_logp_sums_f64": [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _i32, _i32, _c_void_p],
    "rv_dpo_pairs_f64": [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _i32, _i32, _f64, _f64, _f64, _f64, _c_void_p, _c_void_p, _c_void_p, _i32,
                         _c_void_p],
    "rv_gspo_seqs_f64": [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _f64, _f64, _f64, _c_void_p,
                         _c_void_p, _c_void_p, _c_void_p, _i32, _i32, _c_void_p],
    "rv_gather_rows": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i32, _i32, _c_void_p],
    "rv_segment_sum_rows": [_c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _i32, _c_void_p, _i64, _i32, _c_void_p],
    "rv_normalize_tiles_u8": [_c_void_p, _c_void_p, _i32, _i32, _i32, _i32, _i32, ctypes.c_double, ctypes.POINTER(_f32), ctypes.POINTER(_f32), _c_void_p],
    "rv_im2col_patches": [_c_void_p, _c_void_p, _i32, _i32, _i32, _i32, _i32, _c_void_p],
    "rv_clip_embed": [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _i32, _i32, _i32, _c_void_p],
    "rv_adamw": [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _i64, _f32, _f32, _f32, _f32, _f32, _f32, _f32,
                 _c_void_p, _c_void_p],
    "rv_sumsq_partial_bf16": [_c_void_p, _i64, _c_void_p, _i32, _c_void_p],
    "rv_clip_coef": [_c_void_p, _i32, _f32, _c_void_p, _c_void_p],
    "rv_cast_f32_to_bf16": [_c_void_p, _c_void_p, _i64, _c_void_p],
    "rv_cast_bf16_to_f32": [_c_void_p, _c_void_p, _i64, _c_void_p],
    "rv_add_bf16": [_c_void_p, _c_void_p, _c_void_p, _i64, _c_void_p],
    "rv_gemv_bf16": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _c_void_p, _i64, _i32, _i32, _i32, _i32, _c_void_p, _i64,
                     _c_void_p],
    "rv_quantize_rows_w8_bf16": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i32, _i32, _c_void_p],
    "rv_gemv_w8_bf16": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _c_void_p, _i64, _c_void_p, _c_void_p, _i64, _i32, _i32, _i32, _i32,
                        _c_void_p, _i64, _c_void_p],
    "rv_quantize_rows_mxfp4_bf16": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _i32, _i32, _c_void_p],
    "rv_gemv_w4_bf16": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _c_void_p, _i64, _i32, _i32, _i32, _i32,
                        _c_void_p, _i64, _c_void_p],
    "rv_attn_decode_bf16": [_c_void_p, _i64, _c_void_p, _i64, _i64, _i32, _c_void_p, _i32, _c_void_p, _i64, _c_void_p, _i64, _i32, _i32, _i32,
                            _i32, _i32, _f32, _c_void_p],
    "rv_attn_decode_probs_f32": [_c_void_p, _i64, _c_void_p, _i64, _i64, _c_void_p, _i32, _i32, _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64,
                                 _i32, _i32, _i32, _i32, _f32, _c_void_p],
    "rv_kv_votes_f32": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _c_void_p, _i32, _c_void_p, _i64, _c_void_p, _i64, _i32, _i32, _i32, _i32,
                        _i32, _f32, _c_void_p],
    "rv_kv_select_i32": [_c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _i64, _i32, _i32, _i32, _i32, _i32, _c_void_p],
    "rv_kv_gather_bf16": [_c_void_p, _i64, _i32, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _i64, _i32, _i32, _i32, _i32, _i32,
                          _i32, _c_void_p],
    "rv_attn_extend_bf16": [_c_void_p, _i64, _c_void_p, _i64, _i64, _i32, _c_void_p, _c_void_p, _i32, _c_void_p, _i64, _c_void_p, _i64, _i32,
                            _i32, _i32, _i32, _i32, _i32, _i32, _f32, _c_void_p],
    "rv_kv_append_bf16": [_c_void_p, _i64, _c_void_p, _i64, _i64, _c_void_p, _i32, _i32, _i32, _c_void_p],
    "rv_argmax_rows_f32": [_c_void_p, _i64, _i32, _i32, _c_void_p, _c_void_p],
    "rv_logits_process_argmax_f32": [_c_void_p, _i64, _i32, _i32, _c_void_p, _i64, _i32, _f32, _i32, _c_void_p, _i32, _c_void_p, _c_void_p, _i32,
                                     _c_void_p, _c_void_p],
    "rv_logits_process_argmax_rows_f32": [_c_void_p, _i64, _i32, _i32, _c_void_p, _i64, _i32, _i32, _c_void_p, _c_void_p, _c_void_p, _f32,
                                          _i32, _c_void_p, _i32, _c_void_p, _i32, _c_void_p, _i32, _c_void_p, _c_void_p, _i32, _c_void_p,
                                          _c_void_p, _c_void_p],
    "rv_sample_rows_f32": [_c_void_p, _i64, _i32, _i32, _c_void_p, _c_void_p, _f32, _i32, _f32, _f32, _i32, _c_void_p, _c_void_p, _c_void_p, _i64,
                           _c_void_p],
    "rv_attn_decode_beam_bf16": [_c_void_p, _i64, _c_void_p, _i64, _i64, _i32, _c_void_p, _i32, _c_void_p, _c_void_p, _c_void_p, _i64, _i32, _i32,
                                 _c_void_p, _i64, _c_void_p, _i64, _i32, _i32, _i32, _i32, _i32, _f32, _c_void_p],
    "rv_attn_decode_verify_bf16": [_c_void_p, _i64, _c_void_p, _i64, _i64, _i32, _c_void_p, _i32, _c_void_p, _i64, _c_void_p, _i64, _i32, _i32,
                                   _i32, _i32, _i32, _i32, _f32, _c_void_p],
    "rv_kv_quantize_rows_bf16": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _i32, _i32, _i32,
                                 _c_void_p],
    "rv_kv_append_q8_bf16": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i32, _i32, _i32, _i32, _c_void_p],
    "rv_attn_decode_kv8_bf16": [_c_void_p, _i64, _c_void_p, _i64, _i64, _i32, _c_void_p, _i64, _i64, _i32, _c_void_p, _i32, _c_void_p, _i64,
                                _c_void_p, _i64, _i32, _i32, _i32, _i32, _i32, _f32, _c_void_p],
    "rv_attn_decode_shared_bf16": [_c_void_p, _i64, _c_void_p, _i64, _i64, _i32, _c_void_p, _c_void_p, _c_void_p, _i32, _c_void_p, _i64,
                                   _c_void_p, _i64, _i32, _i32, _i32, _i32, _i32, _f32, _c_void_p],
    "rv_log_softmax_rows_f32": [_c_void_p, _i64, _i32, _i32, _c_void_p],
    "rv_beam_topk_f32": [_c_void_p, _i64, _i32, _i32, _i32, _c_void_p, _i32, _c_void_p, _c_void_p, _c_void_p, _i64, _c_void_p],
    "rv_cfg_guide_rows_f32": [_c_void_p, _i64, _c_void_p, _i64, _i32, _i32, _f32, _c_void_p, _i64, _c_void_p],
    "rv_dola_contrast_rows_f32": [_c_void_p, _i64, _c_void_p, _i64, _i64, _i32, _i32, _i32, _f32, _c_void_p, _c_void_p, _c_void_p, _i64,
                                  _c_void_p],
    "rv_constrain_rows_f32": [_c_void_p, _i64, _i32, _i32, _c_void_p, _i32, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _i32, _i32,
                              _c_void_p],
    "rv_attn_extend_prefix_bf16": [_c_void_p, _i64, _c_void_p, _i64, _i64, _i32, _i32, _c_void_p, _i64, _i64, _i32, _i32, _c_void_p, _c_void_p,
                                   _c_void_p, _c_void_p, _i64, _c_void_p, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _c_void_p],
    "rv_token_logprob_rows_f32": [_c_void_p, _i64, _i32, _i32, _c_void_p, _c_void_p, _i32, _c_void_p, _c_void_p, _c_void_p],
    "rv_lora_merge_bf16": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _i32, _i32, _i32, _f32, _c_void_p],
    "rv_lora_down_rows_bf16": [_c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _i64, _i32, _c_void_p, _i64, _i32, _i32, _i32, _f32, _c_void_p,
                               _i64, _c_void_p],
    "rv_gemv_lora_bf16": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _i32, _i32, _c_void_p, _i32, _i32, _i32, _c_void_p, _i32, _i32, _i32,
                          _c_void_p, _i32, _i32, _i32, _i64, _c_void_p, _i64, _c_void_p, _c_void_p, _i64, _i32, _i32, _i32, _c_void_p, _i64,
                          _c_void_p],
}

EXPORTED_SYMBOLS = ["rv_version", "rv_gemm_select_kernel", "rv_gemm_set_cu_budget", "rv_attn_fwd_nat_pairs", "rv_gemv_split",
                    "rv_w8_row_bytes", "rv_w4_row_bytes", "rv_w4_scale_row_bytes", "rv_sample_uniform24", "rv_sample_ws_bytes", "rv_beam_topk_ws_bytes", "rv_cfg_guide_ws_bytes",
                    "rv_dola_ws_bytes", "rv_lora_down_split", "rv_attn_decode_probs_ws_bytes", "rv_kv_votes_ws_bytes",
                    "rv_kv_select_ws_bytes"] + sorted(_SIGS)

_lib = None


class RadvlmHipError(RuntimeError):
    pass


def load():
    """Load the shared library (no GPU needed to load); raises if it has not been built."""
    global _lib
    if _lib is None:
        path = os.environ.get("RADVLM_HIP_LIB", _LIB_PATH)     # override: A/B of two builds (tools/), never a fallback
        if not os.path.exists(path):
            raise RadvlmHipError(f"{path} not found: build it with radvlm_amd/csrc/build.sh "
                                 "(or __graft_entry__.build()); there is no CPU fallback")
        lib = ctypes.CDLL(path)
        lib.rv_version.restype = ctypes.c_char_p
        lib.rv_w8_row_bytes.argtypes = [_i32]
        lib.rv_w8_row_bytes.restype = _i64
        for fn in (lib.rv_w4_row_bytes, lib.rv_w4_scale_row_bytes):
            fn.argtypes = [_i32]
            fn.restype = _i64
        lib.rv_sample_uniform24.argtypes = [ctypes.c_uint64, ctypes.c_int32]
        lib.rv_sample_uniform24.restype = ctypes.c_uint32
        lib.rv_sample_ws_bytes.argtypes = [ctypes.c_int]
        lib.rv_sample_ws_bytes.restype = ctypes.c_int64
        lib.rv_beam_topk_ws_bytes.argtypes = [_i32, _i32, _i32, _i32]
        lib.rv_beam_topk_ws_bytes.restype = _i64
        lib.rv_cfg_guide_ws_bytes.argtypes = [_i32]
        lib.rv_cfg_guide_ws_bytes.restype = _i64
        lib.rv_dola_ws_bytes.argtypes = [_i32, _i32]
        lib.rv_dola_ws_bytes.restype = _i64
        lib.rv_attn_decode_probs_ws_bytes.argtypes = [_i32, _i32, _i32]
        lib.rv_attn_decode_probs_ws_bytes.restype = _i64
        lib.rv_kv_votes_ws_bytes.argtypes = [_i32, _i32, _i32, _i32, _i32]
        lib.rv_kv_votes_ws_bytes.restype = _i64
        lib.rv_kv_select_ws_bytes.argtypes = [_i32, _i32, _i64]
        lib.rv_kv_select_ws_bytes.restype = _i64
        for name, sig in _SIGS.items():
            fn = getattr(lib, name)
            fn.argtypes = sig
            fn.restype = _i32
        _lib = lib
    return _lib


def _ptr(t):
    if t is None:
        return None
    if isinstance(t, int):
        return t
    assert t.is_cuda, "radvlm_amd kernels take device tensors only"
    return t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def call(name, *args):
    lib = load()
    rc = getattr(lib, name)(*[(_ptr(a) if (a is None or isinstance(a, torch.Tensor)) else a) for a in args], _stream())
    if rc != 0:
        raise RadvlmHipError(f"{name} failed with code {rc}")


_zeros = {}


def zeros16(device=None):
    device = torch.device(device or torch.cuda.current_device())
    key = (device.type, device.index)
    if key not in _zeros:
        _zeros[key] = torch.zeros(64, dtype=torch.uint8, device=device)
    return _zeros[key]
