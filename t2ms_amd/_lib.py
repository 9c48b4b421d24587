"""ctypes binding of libt2s_hip.so (C ABI: include/t2s.h).

The HIP library IS the product: there is no CPU or PyTorch fallback.  If the
shared object is missing, or a tensor is not on a GPU, the call fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("T2S_LIB", os.path.join(_HERE, "libt2s_hip.so"))   # T2S_LIB: A/B another build (tools/)

N_BLOCKS = 4
LAT_C, LAT_W, LAT = 64, 30, 1920
D_MODEL, N_TOK = 128, 480
TRAIN_F32, TRAIN_BF16 = 0, 1   # t2s.h: T2S_TRAIN_F32 / T2S_TRAIN_BF16
MATH_F32, MATH_BF16X3, MATH_BF16 = 0, 1, 2    # t2s.h: T2S_MATH_F32 / T2S_MATH_BF16X3 / T2S_MATH_BF16
MATH_CODES = {"f32": MATH_F32, "bf16x3": MATH_BF16X3, "bf16": MATH_BF16}
DIT_N_TENSORS = 10 + 10 * N_BLOCKS   # t2s.h: T2S_DIT_N_TENSORS (pointers of t2s_dit_weights, declaration order)
MSE_SCRATCH_FLOATS = 1024       # t2s.h: T2S_MSE_SCRATCH_FLOATS
EVAL_MAX_LAG, EVAL_MDD_BINS = 64, 50   # t2s.h: T2S_EVAL_MAX_LAG / T2S_EVAL_MDD_BINS
EVAL_CORR_MAX_SERIES, EVAL_MOTION_MAX_LEN = 64, 4096   # t2s.h: T2S_EVAL_CORR_MAX_SERIES / T2S_EVAL_MOTION_MAX_LEN
EVAL_RUNS_MAX_CHANNELS = 16     # t2s_eval_runs.h: T2S_EVAL_RUNS_MAX_CHANNELS

c_float_p = C.c_void_p  # device pointers travel as opaque addresses


class DitBlockWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in
                ("qkv_w", "qkv_b", "proj_w", "proj_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b", "ada_w", "ada_b")]


class DitWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in
                ("conv_w", "conv_b", "patch_w", "patch_b", "pos_embed", "ln_w", "ln_b", "out_w", "out_b",
                 "time_freqs")] + [("blk", DitBlockWeights * N_BLOCKS)]


class DitBlockGrads(C.Structure):
    _fields_ = DitBlockWeights._fields_


class DitGrads(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in
                ("conv_w", "conv_b", "patch_w", "patch_b", "ln_w", "ln_b", "out_w", "out_b")] + \
               [("blk", DitBlockGrads * N_BLOCKS)]


class VaeStackWeights(C.Structure):
    _fields_ = [("conv3_w", C.c_void_p * 4), ("conv1_w", C.c_void_p * 4)]


class VaeWeights(C.Structure):
    _fields_ = [("hidden", C.c_int), ("res_hidden", C.c_int), ("n_res_layers", C.c_int), ("emb", C.c_int),
                ("dec_conv1_w", C.c_void_p), ("dec_conv1_b", C.c_void_p), ("dec_stack", VaeStackWeights),
                ("dec_ct1_w", C.c_void_p), ("dec_ct1_b", C.c_void_p), ("dec_ct2_w", C.c_void_p),
                ("dec_ct2_b", C.c_void_p),
                ("enc_conv1_w", C.c_void_p), ("enc_conv1_b", C.c_void_p), ("enc_conv2_w", C.c_void_p),
                ("enc_conv2_b", C.c_void_p), ("enc_conv3_w", C.c_void_p), ("enc_conv3_b", C.c_void_p),
                ("enc_stack", VaeStackWeights), ("enc_prevq_w", C.c_void_p), ("enc_prevq_b", C.c_void_p)]


class VaeEncGrads(C.Structure):
    _fields_ = [("conv1_w", C.c_void_p), ("conv1_b", C.c_void_p), ("conv2_w", C.c_void_p), ("conv2_b", C.c_void_p),
                ("conv3_w", C.c_void_p), ("conv3_b", C.c_void_p), ("stack_conv3_w", C.c_void_p * 4), ("stack_conv1_w", C.c_void_p * 4),
                ("prevq_w", C.c_void_p), ("prevq_b", C.c_void_p)]


class VaeDecGrads(C.Structure):          # t2s_vae_dec_grads
    _fields_ = [("conv1_w", C.c_void_p), ("conv1_b", C.c_void_p), ("stack_conv3_w", C.c_void_p * 4), ("stack_conv1_w", C.c_void_p * 4),
                ("ct1_w", C.c_void_p), ("ct1_b", C.c_void_p), ("ct2_w", C.c_void_p), ("ct2_b", C.c_void_p)]


TS2VEC_MAX_BLOCKS = 16
TS2VEC_ENCODE_MAX_T = 4096      # t2s.h: T2S_TS2VEC_ENCODE_MAX_T


class Ts2vecWeights(C.Structure):
    _fields_ = [("input_dims", C.c_int), ("hidden", C.c_int), ("output_dims", C.c_int), ("depth", C.c_int),
                ("fc_w", C.c_void_p), ("fc_b", C.c_void_p),
                ("conv1_w", C.c_void_p * TS2VEC_MAX_BLOCKS), ("conv1_b", C.c_void_p * TS2VEC_MAX_BLOCKS),
                ("conv2_w", C.c_void_p * TS2VEC_MAX_BLOCKS), ("conv2_b", C.c_void_p * TS2VEC_MAX_BLOCKS),
                ("proj_w", C.c_void_p), ("proj_b", C.c_void_p)]


TS2VEC_TRAIN_MAX_T, TS2VEC_TRAIN_MAX_B = 128, 16   # t2s.h: T2S_TS2VEC_TRAIN_MAX_T / _MAX_B


class Ts2vecGrads(C.Structure):          # t2s_ts2vec_grads: the pointer fields of Ts2vecWeights, writable
    _fields_ = [f for f in Ts2vecWeights._fields_ if f[1] is not C.c_int]


class Ts2vecView(C.Structure):
    _fields_ = [("start", C.c_void_p), ("mask", C.c_void_p), ("keep", C.c_void_p), ("length", C.c_int), ("pad_", C.c_int)]


class Ts2vecStep(C.Structure):
    _fields_ = [("x", C.c_void_p), ("B", C.c_int), ("T", C.c_int), ("crop_l", C.c_int), ("temporal_unit", C.c_int),
                ("alpha", C.c_float), ("keep_scale", C.c_float), ("x_nan_count", C.c_int), ("pad_", C.c_int),
                ("view", Ts2vecView * 2)]


class AdamwTensor(C.Structure):          # t2s_adamw_tensor
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
                ("n", C.c_uint64)]


MLP_LAYERS, MLP_PACKED_FLOATS = 8, 397888   # t2s.h: T2S_MLP_LAYERS, T2S_MLP_PACKED_FLOATS
MLP_LAYER_FIELDS = (("value_w", "cross_attn.value.weight"), ("value_b", "cross_attn.value.bias"),
                    ("proj_w", "cross_attn.proj.weight"), ("proj_b", "cross_attn.proj.bias"),
                    ("norm2_w", "norm2.weight"), ("norm2_b", "norm2.bias"),
                    ("mlp0_w", "mlp.0.weight"), ("mlp0_b", "mlp.0.bias"), ("mlp2_w", "mlp.2.weight"), ("mlp2_b", "mlp.2.bias"),
                    ("pos0_w", "mlp2.0.weight"), ("pos0_b", "mlp2.0.bias"), ("pos2_w", "mlp2.2.weight"), ("pos2_b", "mlp2.2.bias"))


class MlpLayerWeights(C.Structure):
    _fields_ = [(f, C.c_void_p) for f, _ in MLP_LAYER_FIELDS]


class MlpWeights(C.Structure):
    _fields_ = [("layer", MlpLayerWeights * MLP_LAYERS)]


MLP_GRAD_PART_FLOATS = 391744           # t2s.h: T2S_MLP_GRAD_PART_FLOATS


class MlpGrads(C.Structure):            # t2s_mlp_grads: the same fields, writable
    _fields_ = [("layer", MlpLayerWeights * MLP_LAYERS)]


TSAE_D_MODEL, TSAE_MAX_LAYERS, TSAE_MAX_T = 64, 6, 2000   # t2s.h: T2S_TSAE_D_MODEL / _MAX_LAYERS / _MAX_T
TSAE_MAX_FEATURES, TSAE_MAX_D_FF = 16, 512                 # t2s.h: T2S_TSAE_MAX_FEATURES / _MAX_D_FF
TSAE_TRAIN_MAX_T = 192                                     # t2s.h: T2S_TSAE_TRAIN_MAX_T


class TsaeAttnWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("in_proj_w", "in_proj_b", "out_proj_w", "out_proj_b")]


class TsaeEncLayer(C.Structure):
    _fields_ = [("self_attn", TsaeAttnWeights)] + \
               [(n, C.c_void_p) for n in ("linear1_w", "linear1_b", "linear2_w", "linear2_b",
                                          "norm1_w", "norm1_b", "norm2_w", "norm2_b")]


class TsaeDecLayer(C.Structure):
    _fields_ = [("self_attn", TsaeAttnWeights), ("multihead_attn", TsaeAttnWeights)] + \
               [(n, C.c_void_p) for n in ("linear1_w", "linear1_b", "linear2_w", "linear2_b",
                                          "norm1_w", "norm1_b", "norm2_w", "norm2_b", "norm3_w", "norm3_b")]


class TsaeWeights(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("n_features", "d_model", "d_ff", "heads", "n_enc", "n_dec")] + \
               [(n, C.c_void_p) for n in ("value_embedding_w", "value_embedding_b", "embedding_ln_w", "embedding_ln_b")] + \
               [("enc", TsaeEncLayer * TSAE_MAX_LAYERS), ("dec", TsaeDecLayer * TSAE_MAX_LAYERS)] + \
               [(n, C.c_void_p) for n in ("input_projection_w", "input_projection_b",
                                          "output_projection_w", "output_projection_b")]


class SampleConfig(C.Structure):
    _fields_ = [("mode", C.c_int), ("steps", C.c_int), ("cfg_scale", C.c_float), ("batch", C.c_int),
                ("length", C.c_int), ("use_graph", C.c_int), ("seed", C.c_uint64), ("row0", C.c_uint32),
                ("ddpm_coef", C.c_void_p), ("t_values", C.c_void_p)]


MODE_DDPM, MODE_RF, MODE_LMS = 0, 1, 2   # t2s.h: T2S_MODE_DDPM / T2S_MODE_RF / T2S_MODE_LMS

# every symbol include/t2s.h declares: (name, restype, argtypes)
_VP, _I, _F, _U64, _U32 = C.c_void_p, C.c_int, C.c_float, C.c_uint64, C.c_uint32
SYMBOLS = {
    "t2s_last_error": (C.c_char_p, []),
    "t2s_version": (C.c_char_p, []),
    "t2s_dit_create": (_I, [C.POINTER(DitWeights), _I, C.POINTER(_VP)]),
    "t2s_dit_create_w": (_I, [C.POINTER(DitWeights), _I, _I, C.POINTER(_VP)]),
    "t2s_dit_latent_w": (_I, [_VP]),
    "t2s_dit_update_weights": (_I, [_VP, C.POINTER(DitWeights), _VP]),
    "t2s_dit_destroy": (None, [_VP]),
    "t2s_dit_max_seqs": (_I, [_VP]),
    "t2s_time_embedding": (_I, [_VP, _VP, _VP, _I, _VP]),
    "t2s_time_embedding_freqs": (_I, [_VP, _VP, _VP, _I, _VP]),
    "t2s_dit_weights_check": (_I, [C.POINTER(DitWeights), C.POINTER(C.c_uint64), _I]),
    "t2s_dit_weights_check_w": (_I, [C.POINTER(DitWeights), _I, C.POINTER(C.c_uint64), _I]),
    "t2s_dit_forward": (_I, [_VP, _VP, _VP, _I, _VP, _VP, _I, _VP]),
    "t2s_dit_forward_cfg": (_I, [_VP, _VP, _VP, _VP, _VP, _VP, _I, _VP]),
    "t2s_dit_forward_cfg_rows": (_I, [_VP, _VP, _VP, _I, _VP, _VP, _VP, _I, _VP]),
    "t2s_dit_read_stream": (_I, [_VP, _VP, _I, _VP]),
    "t2s_dit_timing_begin": (_I, [_VP]),
    "t2s_dit_timing_end": (_I, [_VP, C.POINTER(C.c_double)]),
    "t2s_dit_timing_end_ex": (_I, [_VP, C.POINTER(C.c_double), _I]),
    "t2s_dit_set_train_dtype": (_I, [_VP, _I]),
    "t2s_dit_set_math": (_I, [_VP, _I]),
    "t2s_eval_mse_wape": (_I, [_VP, _VP, _VP, _VP, _I, _I, _VP]),
    "t2s_eval_mrr": (_I, [_VP, _VP, _VP, _VP, _VP, _I, _I, _I, _F, _VP]),
    "t2s_eval_ed": (_I, [_VP, _VP, _VP, _VP, _I, _I, _I, _VP]),
    "t2s_eval_crps": (_I, [_VP, _VP, _VP, _VP, _I, _I, _I, _I, _VP]),
    "t2s_eval_dtw": (_I, [_VP, _VP, _VP, _VP, _I, _I, _I, _VP]),
    "t2s_eval_features_workspace_bytes": (_U64, [_I, _I, _I]),
    "t2s_eval_moments": (_I, [_VP, _VP, _VP, _VP, _I, _I, _I, _VP, _U64, _VP]),
    "t2s_eval_mdd": (_I, [_VP, _VP, _VP, _VP, _I, _I, _I, _VP, _U64, _VP]),
    "t2s_eval_corr_workspace_bytes": (_U64, [_I, _I, _I]),
    "t2s_eval_corr": (_I, [_VP, _VP, _VP, _VP, _I, _I, _I, _VP, _U64, _VP]),
    "t2s_eval_shift": (_I, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I, _I, _I, _I, _VP]),
    "t2s_eval_dtw_ragged": (_I, [_VP, _VP, _VP, _VP, _VP, _VP, _I, _I, _I, _I, _VP]),
    "t2s_ts2vec_encode": (_I, [C.POINTER(Ts2vecWeights), _VP, _VP, _VP, _I, _I, _VP]),
    "t2s_ts2vec_encode_workspace_bytes": (_U64, [C.POINTER(Ts2vecWeights), _I, _I]),
    "t2s_ts2vec_encode_long": (_I, [C.POINTER(Ts2vecWeights), _VP, _VP, _VP, _I, _I, _VP, _U64, _VP]),
    "t2s_ts2vec_train_workspace_bytes": (_U64, [C.POINTER(Ts2vecWeights), _I, _I]),
    "t2s_ts2vec_train_step": (_I, [C.POINTER(Ts2vecWeights), C.POINTER(Ts2vecGrads), C.POINTER(Ts2vecStep), _VP, _VP, _U64, _VP]),
    "t2s_swa_update_multi": (_I, [_VP, _I, _U64, C.c_int64, _VP]),
    "t2s_mlp_pack": (_I, [C.POINTER(MlpWeights), _VP, _VP]),
    "t2s_mlp_forward": (_I, [_VP, _VP, _VP, _VP, _VP, _VP, _I, _VP]),
    "t2s_mlp_backward": (_I, [C.POINTER(MlpWeights), _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.POINTER(MlpGrads), _VP, _U64, _I, _VP]),
    "t2s_attn_fwd_x3": (_I, [_VP, _VP, _VP, _VP, _I, _VP]),
    "t2s_attn_fwd_bf16p": (_I, [_VP, _VP, _VP, _VP, _I, _VP]),
    "t2s_attn_fwd_bf16": (_I, [_VP, _VP, _VP, _VP, _VP, _I, _VP]),
    "t2s_attn_train": (_I, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _I, _I, _VP]),
    "t2s_wgrad": (_I, [_VP, _VP, _VP, _VP, _I, _I, _I, _I, _I, _VP]),
    "t2s_dit_train_forward": (_I, [_VP, C.POINTER(DitWeights), _VP, _VP, _I, _VP, _VP, _I, _VP]),
    "t2s_dit_train_backward": (_I, [_VP, _VP, C.POINTER(DitGrads), _I, _VP]),
    "t2s_dit_train_input_grad": (_I, [_VP, _VP, _I, _VP]),
    "t2s_adamw_step": (_I, [_VP, _VP, _VP, _VP, _U64, _F, _F, _F, _F, _F, _I, _VP]),
    "t2s_adamw_step_multi": (_I, [_VP, _I, _U64, _F, _F, _F, _F, _F, _I, _VP]),
    "t2s_mse_backward": (_I, [_VP, _VP, _VP, _VP, _VP, _U64, _VP]),
    "t2s_attn_fwd": (_I, [_VP, _VP, _VP, _VP, _I, _VP]),
    "t2s_attn_fwd_packed": (_I, [_VP, _VP, _VP, _VP, _I, _VP]),
    "t2s_attn_fwd_packed_n": (_I, [_VP, _VP, _VP, _VP, _I, _I, _VP]),
    "t2s_ddpm_step": (_I, [_VP, _VP, _VP, _VP, _VP, _I, _F, _U64, _U32, _U32, _I, _VP]),
    "t2s_lms_step": (_I, [_VP, _VP, _VP, _VP, _VP, _VP, _I, _F, _U64, _U32, _U32, _I, _VP]),
    "t2s_lms_step_n": (_I, [_VP, _VP, _VP, _VP, _VP, _VP, _I, _F, _U64, _U32, _U32, _I, _I, _VP]),
    "t2s_ddpm_p_sample": (_I, [_VP, _VP, _VP, _VP, _VP, _VP, _I, _I, _VP]),
    "t2s_ddpm_p_sample_n": (_I, [_VP, _VP, _VP, _VP, _VP, _VP, _I, _I, _I, _VP]),
    "t2s_ddpm_q_sample_n": (_I, [_VP, _VP, _VP, _VP, _VP, _VP, _I, _I, _I, _VP]),
    "t2s_vae_decode_w": (_I, [_VP, _VP, _VP, _VP, _I, _I, _I, _VP]),
    "t2s_mse": (_I, [_VP, _VP, _VP, _U64, _VP]),
    "t2s_mse_ws": (_I, [_VP, _VP, _VP, _U64, _VP, _VP]),
    "t2s_rf_step": (_I, [_VP, _VP, _VP, _F, _F, _I, _VP]),
    "t2s_ddpm_q_sample": (_I, [_VP, _VP, _VP, _VP, _VP, _VP, _I, _I, _VP]),
    "t2s_rf_create_flow": (_I, [_VP, _VP, _VP, _VP, _I, _VP]),
    "t2s_philox_normal": (_I, [_VP, _U64, _U32, _U32, _I, _I, _VP]),
    "t2s_philox_uniform": (_I, [_VP, _U64, _U32, _U32, _I, _I, _VP]),
    "t2s_vae_create": (_I, [C.POINTER(VaeWeights), C.POINTER(_VP)]),
    "t2s_vae_destroy": (None, [_VP]),
    "t2s_vae_update_weights": (_I, [_VP, C.POINTER(VaeWeights), _VP]),
    "t2s_vae_encode_backward": (_I, [_VP, _VP, _VP, _VP, C.POINTER(VaeEncGrads), _I, _I, _VP]),
    "t2s_vae_decode_backward": (_I, [_VP, _VP, _VP, _VP, C.POINTER(VaeDecGrads), _VP, _I, _I, _I, _VP]),
    "t2s_vae_encode_backward_mc": (_I, [_VP, _VP, _VP, _VP, C.POINTER(VaeEncGrads), _I, _I, _I, _VP]),
    "t2s_vae_decode_backward_mc": (_I, [_VP, _VP, _VP, _VP, C.POINTER(VaeDecGrads), _VP, _I, _I, _I, _VP]),
    "t2s_vae_decode": (_I, [_VP, _VP, _VP, _VP, _I, _I, _VP]),
    "t2s_vae_encode": (_I, [_VP, _VP, _VP, _VP, _I, _I, _VP]),
    "t2s_vae_create_mc": (_I, [C.POINTER(VaeWeights), _I, C.POINTER(_VP)]),
    "t2s_vae_channels": (_I, [_VP]),
    "t2s_vae_encode_mc": (_I, [_VP, _VP, _VP, _VP, _I, _I, _I, _VP]),
    "t2s_vae_decode_mc": (_I, [_VP, _VP, _VP, _VP, _I, _I, _I, _VP]),
    "t2s_vae_decode_mc_ragged": (_I, [_VP, _VP, _VP, _VP, _VP, _I, _I, _I, _VP]),
    "t2s_vae_encode_mc_ragged": (_I, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _I, _I, _I, _VP]),
    "t2s_sampler_create": (_I, [_VP, _VP, C.POINTER(SampleConfig), C.POINTER(_VP)]),
    "t2s_sampler_create_lms": (_I, [_VP, _VP, C.POINTER(SampleConfig), _VP, C.POINTER(_VP)]),
    "t2s_sampler_destroy": (None, [_VP]),
    "t2s_sampler_run": (_I, [_VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "t2s_sampler_set_lanes": (_I, [_VP, _I]),
    "t2s_sampler_set_loop_graph": (_I, [_VP, _I]),
    "t2s_sampler_set_guided_steps": (_I, [_VP, _I, _I]),
    "t2s_sampler_guided_steps": (_I, [_VP, C.POINTER(_I), C.POINTER(_I)]),
    "t2s_sampler_set_row0": (_I, [_VP, _U32]),
    "t2s_sampler_set_rows": (_I, [_VP, _VP, _VP, _VP, _I]),
    "t2s_sampler_set_lengths": (_I, [_VP, _VP, _I]),
    "t2s_philox_normal_rows": (_I, [_VP, _VP, _VP, _U32, _I, _I, _VP]),
    "t2s_sampler_graph_lanes": (_I, [_VP]),
    "t2s_sampler_lane_pool": (_I, []),
    "t2s_tsae_create": (_I, [C.POINTER(TsaeWeights), C.POINTER(_VP)]),
    "t2s_tsae_destroy": (None, [_VP]),
    "t2s_tsae_positional": (_I, [_VP, _VP, _I, _I, _VP]),
    "t2s_tsae_workspace_bytes": (_U64, [_VP, _I, _I]),
    "t2s_tsae_encode": (_I, [_VP, _VP, _VP, _I, _I, _VP, _U64, _VP]),
    "t2s_tsae_decode": (_I, [_VP, _VP, _VP, _VP, _I, _I, _VP, _U64, _VP]),
    "t2s_tsae_generate": (_I, [_VP, _VP, _VP, _I, _I, _VP, _U64, _VP]),
    "t2s_tsae_update_weights": (_I, [_VP, C.POINTER(TsaeWeights), _VP]),
    "t2s_tsae_train_workspace_bytes": (_U64, [_VP, _I, _I]),
    "t2s_tsae_train_forward": (_I, [_VP, _VP, _VP, _I, _I, _F, _U64, _VP, _U64, _VP]),
    "t2s_tsae_train_backward": (_I, [_VP, _VP, _VP, C.POINTER(TsaeWeights), _I, _I, _F, _U64, _VP, _U64, _VP]),
}

_lib: Optional[C.CDLL] = None


class T2SError(RuntimeError):
    pass


# include/t2s_wide_train.h: the entries of wide-latent training (an extension header with a table of its own, resolved by
# lib() with SYMBOLS; tests/test_wide_train_host.py compares the two as tests/test_cabi_symbols.py does for t2s.h)
SYMBOLS_WIDE_TRAIN = {
    "t2s_dit_set_trainable": (_I, [_VP, _I]),
    "t2s_attn_train_n": (_I, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _I, _I, _I, _VP]),
}

# include/t2s_wide_math.h: bf16x3 / bf16 inference at the wide latent widths (tests/test_wide_math_host.py)
SYMBOLS_WIDE_MATH = {
    "t2s_dit_set_wide_math": (_I, [_VP, _I]),
    "t2s_attn_fwd_x3_n": (_I, [_VP, _VP, _VP, _VP, _I, _I, _VP]),
    "t2s_attn_fwd_bf16p_n": (_I, [_VP, _VP, _VP, _VP, _I, _I, _VP]),
}

# include/t2s_wide_train_bf16.h: the bf16 mixed-precision training step at the wide latent widths (tests/test_wide_train_bf16_host.py)
SYMBOLS_WIDE_TRAIN_BF16 = {
    "t2s_dit_set_wide_train_bf16": (_I, [_VP, _I]),
    "t2s_attn_train_bf16_n": (_I, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _I, _I, _VP]),
}

# include/t2s_train_rows.h: one launch form of the training step's row kernels alone -- for tests / benchmarking of those
# kernels (tests/test_train_rows.py, tests/test_train_rows_host.py); no class of this package calls it
TRAIN_ROWS_OPS = {"QKV0": 0, "QKV1": 1, "FC1": 2, "FC2": 3, "LIN128": 4, "GELUBWD": 5, "LNBWD256": 6, "LNBWD384": 7, "FINAL_FUSED": 8,
                  "F_QKV": 16, "F_FC1": 17, "F_FC2": 18, "F_LIN128": 19, "F_LIN256": 20, "F_LIN384": 21, "F_GELUBWD": 22,
                  "F_GATE_RES": 23, "F_GATE_BWD": 24, "F_LN_MOD_BWD": 25, "F_GELU": 26, "F_FINAL": 27}   # T2S_ROWS_*


class TrainRowsArgs(C.Structure):        # t2s_train_rows_args
    _fields_ = [(n, C.c_void_p) for n in
                ("a", "w", "bias", "mod", "res", "aux", "ln_x", "dout", "ln_w", "ln_b", "out", "save_a", "x_out", "q", "k", "v",
                 "dx", "dmod", "g_ln_w", "g_ln_b", "g_out_w", "g_out_b")] + \
               [(n, C.c_int) for n in ("shift_off", "scale_off", "gate_off")]


SYMBOLS_TRAIN_ROWS = {
    "t2s_train_rows": (_I, [_I, _I, _I, _I, _I, C.POINTER(TrainRowsArgs), _VP]),
}

# include/t2s_eval_runs.h: myevaluation.py's scores over the packed ragged clips of a motion test split, all runs, one call
# (metrics.motion_runs; tests/test_myeval_host.py)
SYMBOLS_EVAL_RUNS = {
    "t2s_eval_runs": (_I, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I, _I, _I, _I, _VP]),
}


def lib() -> C.CDLL:
    """Load libt2s_hip.so (once).  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise T2SError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                f"or `make -C t2ms_amd/csrc` (hipcc --offload-arch=gfx950).  There is no CPU fallback.")
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in (list(SYMBOLS.items()) + list(SYMBOLS_WIDE_TRAIN.items()) + list(SYMBOLS_WIDE_MATH.items()) +
                                  list(SYMBOLS_WIDE_TRAIN_BF16.items()) + list(SYMBOLS_TRAIN_ROWS.items()) +
                                  list(SYMBOLS_EVAL_RUNS.items())):
            fn = getattr(handle, name)  # AttributeError if the .so does not export it
            fn.restype, fn.argtypes = res, args
        _lib = handle
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().t2s_last_error().decode("utf-8", "replace")
        raise T2SError(f"{what or 't2s call'} failed (rc={rc}): {msg}")


def dev_ptr(t: Optional[torch.Tensor], name: str = "tensor", dtype=torch.float32) -> Optional[int]:
    """Raw device address of a contiguous CUDA(HIP) tensor; None passes NULL."""
    if t is None:
        return None
    if not t.is_cuda:
        raise T2SError(f"{name} must live on a GPU (got device {t.device}); the HIP path has no CPU fallback")
    if t.dtype != dtype:
        raise T2SError(f"{name} must be {dtype} (got {t.dtype})")
    if not t.is_contiguous():
        raise T2SError(f"{name} must be contiguous")
    return t.data_ptr()


def as_f32(t: torch.Tensor) -> torch.Tensor:
    """fp32 contiguous view/copy on the tensor's own (GPU) device."""
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def ragged_layout(lengths, max_length, what: str, batch=None):
    """The host tables of a ragged launch (t2s_vae_*_mc_ragged, t2s_sampler_set_lengths), validated here before anything
    reaches the library: (int32 lengths (n), uint64 offsets (n + 1) = prefix sums of the lengths, uint64 offsets4 (n + 1) =
    prefix sums of L_b // 4).  Every length is an integer, 0 (an empty row) or in [8, max_length] (max_length None: 2**20);
    `batch`: the row count the caller's object holds.  T2SError otherwise."""
    import operator

    import numpy as np
    try:
        vals = [operator.index(v) for v in lengths]
        if any(isinstance(v, bool) for v in lengths):
            raise TypeError
    except TypeError:
        raise T2SError(f"{what}: lengths must be a sequence of integers") from None
    if not vals:
        raise T2SError(f"{what}: lengths is empty")
    if batch is not None and len(vals) != int(batch):
        raise T2SError(f"{what}: {len(vals)} lengths for {int(batch)} rows")
    top = (1 << 20) if max_length is None else int(max_length)
    for r, v in enumerate(vals):
        if v != 0 and not 8 <= v <= top:
            raise T2SError(f"{what}: lengths[{r}] = {v} (0, or 8 .. {top})")
    lens = np.asarray(vals, dtype=np.int32)
    off = np.zeros(len(vals) + 1, dtype=np.uint64)
    off4 = np.zeros(len(vals) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens.astype(np.uint64))
    off4[1:] = np.cumsum((lens // 4).astype(np.uint64))
    return lens, off, off4


def ragged_device_tables(lens, off, off4, device):
    """ragged_layout's tables on the device: ONE pinned staging tensor, one asynchronous copy on the current stream ->
    (tensor to keep alive, lengths pointer, offsets pointer, offsets4 pointer)."""
    import numpy as np
    n = len(lens)
    pad = np.zeros(n + (n & 1), dtype=np.int32)
    pad[:n] = lens
    host = np.concatenate([off, off4, pad.view(np.uint64)])
    t = torch.from_numpy(host.view(np.int64)).pin_memory().to(device, non_blocking=True)
    base = t.data_ptr()
    return t, base + 16 * (n + 1), base, base + 8 * (n + 1)


_DEVICE_LOCKS = {}


def device_lock(device) -> "threading.RLock":
    """Per device, re-entrant: held by everything in this package that allocates, frees, copies synchronously or synchronises
    the DEVICE -- building / growing / destroying a handle, a Sampler's create / stage / run / destroy -- so that none of it
    runs while another thread's sampler run has a stream capture open.  HIP answers a device-wide synchronous call from ANY
    thread (hipDeviceSynchronize = torch.cuda.synchronize(), a synchronous hipMemcpy) with an error while a capture is open
    on the device, thread-local capture mode notwithstanding, and that error invalidates the capture (reproduced in round 5 by
    a diagnosis build without this serialisation, last carried by commit f0cbfbc).  The caller's OWN
    device-wide calls in other threads are not covered: see include/t2s.h "Threads"."""
    import threading
    return _DEVICE_LOCKS.setdefault(str(torch.device(device)), threading.RLock())


def destroy_locked(fn_name: str, device_key: str, ptr) -> None:
    """Finalizer body of the handle owners: t2s_*_destroy frees device memory -- under the device's lock (device_lock)."""
    with device_lock(device_key):
        getattr(lib(), fn_name)(ptr)


def stream_ptr(device=None) -> int:
    return torch.cuda.current_stream(device).cuda_stream
