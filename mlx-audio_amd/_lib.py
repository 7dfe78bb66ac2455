"""ctypes binding of libkokoro_hip.so (include/kokoro_hip.h).  Fails loudly when the library
is missing: there is no CPU or PyTorch fallback for the hot path."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libkokoro_hip.so")

KK_F32, KK_BF16, KK_I32, KK_F16 = 0, 1, 2, 3
CSM_WEIGHTS = {0: "f32", 1: "bf16", 2: "q8", 3: "q4"}  # kk_csm_weight_format
CSM_WEIGHTS_MIXED, CSM_WEIGHTS_DEQUANTIZED = 0x100, 0x200
NOISE_ZERO, NOISE_INJECTED, NOISE_PHILOX = 0, 1, 2
ACT_NONE, ACT_LRELU, ACT_GELU, ACT_SNAKE = 0, 1, 2, 3
KK_PCM_F32, KK_PCM_S16LE, KK_PCM_MULAW, KK_PCM_ALAW = 0, 1, 2, 3


class KKConfig(C.Structure):
    _fields_ = [
        ("n_token", C.c_int32), ("hidden_dim", C.c_int32), ("style_dim", C.c_int32), ("n_layer", C.c_int32),
        ("max_dur", C.c_int32), ("text_encoder_kernel_size", C.c_int32),
        ("plbert_hidden", C.c_int32), ("plbert_heads", C.c_int32), ("plbert_intermediate", C.c_int32),
        ("plbert_max_pos", C.c_int32), ("plbert_layers", C.c_int32), ("plbert_embedding", C.c_int32),
        ("decoder_hidden", C.c_int32), ("upsample_initial_channel", C.c_int32), ("n_upsamples", C.c_int32),
        ("upsample_rates", C.c_int32 * 4), ("upsample_kernel_sizes", C.c_int32 * 4),
        ("n_resblock_kernels", C.c_int32), ("resblock_kernel_sizes", C.c_int32 * 4),
        ("resblock_dilations", (C.c_int32 * 3) * 4),
        ("gen_istft_n_fft", C.c_int32), ("gen_istft_hop_size", C.c_int32), ("compute_dtype", C.c_int32),
    ]


class KKMimiConfig(C.Structure):
    _fields_ = [
        ("dim", C.c_int32), ("nq", C.c_int32), ("bins", C.c_int32), ("qdim", C.c_int32), ("num_heads", C.c_int32),
        ("num_layers", C.c_int32), ("dim_feedforward", C.c_int32), ("nfilters", C.c_int32),
        ("n_ratios", C.c_int32), ("ratios", C.c_int32 * 8),
        ("ksize", C.c_int32), ("residual_ksize", C.c_int32), ("last_ksize", C.c_int32), ("upsample_stride", C.c_int32),
        ("compress", C.c_int32), ("rope_base", C.c_float), ("compute_dtype", C.c_int32),
    ]


class KKSnacConfig(C.Structure):  # kk_snac_config
    _fields_ = [
        ("sampling_rate", C.c_int32), ("encoder_dim", C.c_int32), ("n_encoder_rates", C.c_int32), ("encoder_rates", C.c_int32 * 8),
        ("latent_dim", C.c_int32), ("decoder_dim", C.c_int32), ("n_decoder_rates", C.c_int32), ("decoder_rates", C.c_int32 * 8),
        ("attn_window_size", C.c_int32), ("codebook_size", C.c_int32), ("codebook_dim", C.c_int32), ("n_vq", C.c_int32),
        ("vq_strides", C.c_int32 * 8), ("noise", C.c_int32), ("depthwise", C.c_int32), ("compute_dtype", C.c_int32),
    ]


class KKWhisperConfig(C.Structure):
    _fields_ = [("n_mels", C.c_int32), ("n_audio_ctx", C.c_int32), ("n_audio_state", C.c_int32), ("n_audio_head", C.c_int32),
                ("n_audio_layer", C.c_int32)]


class KKWhisperTextConfig(C.Structure):
    _fields_ = [("n_vocab", C.c_int32), ("n_text_ctx", C.c_int32), ("n_text_state", C.c_int32), ("n_text_head", C.c_int32),
                ("n_text_layer", C.c_int32), ("n_audio_ctx", C.c_int32), ("n_audio_state", C.c_int32)]


class KKWhisperPickParams(C.Structure):  # kk_whisper_pick_params
    _fields_ = [("n_vocab", C.c_int32), ("eot", C.c_int32), ("blank", C.c_int32), ("no_timestamps", C.c_int32), ("timestamp_begin", C.c_int32),
                ("max_initial_timestamp_index", C.c_int32), ("without_timestamps", C.c_int32), ("suppress_blank", C.c_int32)]


class KKWhisperPickState(C.Structure):  # kk_whisper_pick_state
    _fields_ = [("last", C.c_int32), ("penultimate", C.c_int32), ("last_timestamp", C.c_int32), ("ended", C.c_int32), ("count", C.c_int32),
                ("sum_logprob", C.c_float), ("last_logprob", C.c_float), ("reserved", C.c_int32)]


class KKWhisperRowsItem(C.Structure):  # kk_whisper_rows_item
    _fields_ = [("row", C.c_int32), ("pos", C.c_int32), ("count", C.c_int32), ("from_", C.c_int32), ("keep", C.c_int32), ("slot", C.c_int32)]


class KKWhisperBeamBufs(C.Structure):  # kk_whisper_beam_bufs: device pointers of a beam search on caller-owned buffers
    _fields_ = [("n_audio", C.c_int32), ("beam_size", C.c_int32), ("max_candidates", C.c_int32), ("n_ctx", C.c_int32), ("cap", C.c_int32), ("reserved", C.c_int32),
                ("cand_token", C.c_void_p), ("cand_logprob", C.c_void_p), ("owner", C.c_void_p * 2), ("parent", C.c_void_p), ("fin_score", C.c_void_p),
                ("fin_length", C.c_void_p), ("fin_tokens", C.c_void_p), ("fin_count", C.c_void_p), ("complete", C.c_void_p), ("not_complete", C.c_void_p)]


WHISPER_MAX_ROWS = 32  # KK_WHISPER_MAX_ROWS
WHISPER_MAX_GROUP = 8  # KK_WHISPER_MAX_GROUP
WHISPER_GROUP_PLAIN, WHISPER_GROUP_BEAM = 0, 1  # KK_WHISPER_GROUP_*


class KKLlamaArgs(C.Structure):
    _fields_ = [("num_layers", C.c_int32), ("num_heads", C.c_int32), ("num_kv_heads", C.c_int32), ("head_dim", C.c_int32),
                ("hidden", C.c_int32), ("intermediate", C.c_int32), ("rope_theta", C.c_float), ("rope_factor", C.c_float), ("rms_eps", C.c_float)]


class KKCsmConfig(C.Structure):
    _fields_ = [("text_vocab_size", C.c_int32), ("audio_vocab_size", C.c_int32), ("audio_num_codebooks", C.c_int32), ("max_seq_len", C.c_int32),
                ("backbone", KKLlamaArgs), ("decoder", KKLlamaArgs)]


class KKCsmSampler(C.Structure):  # kk_csm_sampler
    _fields_ = [("temperature", C.c_float), ("top_k", C.c_int32), ("top_p", C.c_float), ("min_p", C.c_float), ("min_tokens_to_keep", C.c_int32),
                ("seed", C.c_uint64), ("use_device_rng", C.c_int32)]


# every symbol include/kokoro_hip.h declares: name -> (restype, argtypes)
_vp, _i, _f, _sz, _u64 = C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.c_uint64
SIGNATURES = {
    "kk_create": (_i, [C.POINTER(KKConfig), C.POINTER(_vp)]),
    "kk_destroy": (None, [_vp]),
    "kk_load_tensor": (_i, [_vp, C.c_char_p, _i, C.POINTER(C.c_int64), _i, _vp]),
    "kk_finalize": (_i, [_vp, _vp]),
    "kk_workspace_bytes": (_sz, [_vp, _i, _i, _i]),
    "kk_context_create": (_i, [_vp, C.POINTER(_vp)]),
    "kk_context_destroy": (None, [_vp]),
    "kk_context_model": (_vp, [_vp]),
    "kk_context_workspace_bytes": (_sz, [_vp, _i, _i, _i]),
    "kk_forward_text": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "kk_forward_audio": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _u64, _vp, _sz, _vp, _vp]),
    "kk_forward": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _u64, _vp, _sz, _vp, _vp, _vp]),
    "kk_last_error": (C.c_char_p, []),
    "kk_abi_version": (_i, []),
    "kk_abi_minor": (_i, []),
    "kk_op_conv1d": (_i, [_vp, _i, _vp, _i, _i, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _f, _i, _f, _vp, _i, _f, _i, _vp, _i, _i, _vp, _i, _i]),
    "kk_op_conv1d_bf16": (_i, [_vp, _i, _vp, _i, _i, _vp, _vp, _i, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _f, _i, _f, _vp, _i, _f, _i, _vp, _i, _i, _vp, _i]),
    "kk_op_conv1d_bf16_fused": (_i, [_vp, _i, _vp, _i, _i, _vp, _vp, _i, _i, _vp, _i, _i, _i, _i, _i, _vp, _vp, _i, _i, _f, _vp, _vp, _i, _f,
                                     _vp, _i, _vp, C.POINTER(C.c_int)]),
    "kk_op_adain": (_i, [_vp, _i, _vp, _i, _i, _vp, _i, _vp, _i, _i, _f, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _vp, _sz, _i, _i]),
    "kk_op_norm_finalize": (_i, [_vp, _i, _i, _vp, _i, _vp, _i, _vp, C.c_longlong, _vp, _i, _vp, _vp, _vp, _vp, _i, _i]),
    "kk_op_mimi_conv": (_i, [_vp, _i, _vp, C.c_longlong, _i, _i, _i, _vp, _i, _vp, _i, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, C.c_longlong, _i, _i,
                             _vp, C.c_longlong, _i, _i, _i, _vp, _sz, C.POINTER(C.c_int)]),
    "kk_op_mimi_rvq_sum": (_i, [_vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _i]),
    "kk_op_mimi_upsample": (_i, [_vp, _i, _vp, C.c_longlong, _vp, _i, _i, _i, _i, _vp, _i]),
    "kk_op_mimi_rope": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _i]),
    "kk_op_mimi_conv_cout1": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _i, _i, _vp, _i, _vp, _i, _vp, C.POINTER(C.c_int)]),
    "kk_op_mimi_edge_pad": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _vp]),
    "kk_op_mimi_rvq_argmin": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "kk_op_mimi_carry": (_i, [_vp, _i, _i, _i, C.POINTER(_vp), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                              C.POINTER(C.c_longlong), _vp, _vp, _vp, _i, _i, _i, C.c_ulonglong]),
    "kk_op_layernorm": (_i, [_vp, _i, _vp, _i, _vp, _i, _i, _vp, _i, _vp, _vp, _vp, _i, _f, _i, _f, _vp, _i, _i]),
    "kk_op_lstm": (_i, [_vp, _i, _vp, _vp, _i, _i, _vp, _vp, _i, _i]),
    "kk_op_lstm_bf16": (_i, [_vp, _i, _vp, _vp, _i, _vp, _vp, _i, _i]),
    "kk_op_linear_rows": (_i, [_vp, _i, _vp, C.c_longlong, _i, _i, _vp, _vp, _i, _i, _vp, _i, _vp, _vp, C.c_longlong, _i]),
    "kk_op_attention": (_i, [_vp, _i, _vp, _i, _i, _vp, _i, _vp, _i, _i]),
    "kk_op_source_stft": (_i, [_vp, _i, _vp, _i, _vp, _vp, _f, _i, _vp, _u64, _vp, _vp, _vp, _i, _i]),
    "kk_op_source_stft_ragged": (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _f, _i, _vp, _u64, _vp, _vp, _vp, _i, _i]),
    "kk_op_kokoro_style_fc": (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _i]),
    "kk_op_kokoro_fill_style": (_i, [_vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _vp, _i]),
    "kk_op_kokoro_embedding": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _vp, _i]),
    "kk_op_kokoro_duration": (_i, [_vp, _i, _vp, _i, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, _vp, _i]),
    "kk_op_kokoro_alignment": (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _i]),
    "kk_op_kokoro_gather_rows": (_i, [_vp, _i, _vp, _i, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i]),
    "kk_op_kokoro_copy_slice": (_i, [_vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _vp, _i]),
    "kk_op_kokoro_lens": (_i, [_vp, _i, _vp, _vp, _i, _i, _i]),
    "kk_op_kokoro_convert": (_i, [_vp, _i, _vp, _i, _i, _vp, _i, _i, _i, _i]),
    "kk_op_albert_embed": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _i, _i, _i, _vp, _i]),
    "kk_op_istft_head": (_i, [_vp, _i, _vp, _i, _i, _vp, _vp, _i, _i]),
    "kk_op_pack_head_w": (_i, [_vp, _vp, _vp]),
    "kk_op_conv_post_istft": (_i, [_vp, _i, _vp, _i, _i, _vp, _vp, _vp, _f, _vp, _vp, _i]),
    "kk_debug_info": (_i, [_vp, C.c_char_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "kk_debug_fetch": (_i, [_vp, _vp, C.c_char_p, _vp]),
    "kk_debug_override": (_i, [_vp, C.c_char_p, _vp]),
    "kk_debug_clear": (None, [_vp]),
    # flags: see include/kokoro_hip.h; bit 11 (2048) = conv variant 4 slab by slab also where its whole-K or ring form is routed
    "kk_debug_force_generic": (None, [_vp, _i]),
    "kk_op_pack_w_frag": (_i, [_vp, _vp, _vp, _i, _i, _i]),
    "kk_csm_create": (_i, [C.POINTER(KKCsmConfig), C.POINTER(_vp)]),
    "kk_csm_destroy": (None, [_vp]),
    "kk_csm_load_tensor": (_i, [_vp, C.c_char_p, C.POINTER(C.c_int64), _i, _vp]),
    "kk_csm_set_weight_dtype": (_i, [_vp, _i]),
    "kk_csm_load_quantized": (_i, [_vp, C.c_char_p, C.POINTER(C.c_int64), _vp, _vp, _vp, _i, _i]),
    "kk_csm_weight_format": (_i, [_vp]),
    "kk_csm_weight_fallback_reason": (C.c_char_p, [_vp]),
    "kk_csm_weight_bytes": (_i, [_vp, C.POINTER(_sz), C.POINTER(_sz)]),
    "kk_csm_finalize": (_i, [_vp, _vp]),
    "kk_csm_share": (_i, [_vp, C.POINTER(_vp)]),
    "kk_csm_setup_caches": (_i, [_vp, _i]),
    "kk_csm_reset_caches": (_i, [_vp]),
    "kk_csm_position": (_i, [_vp]),
    "kk_csm_set_padding": (_i, [_vp, _i, _vp]),
    "kk_csm_workspace_bytes": (_sz, [_vp, _i, _i]),
    "kk_csm_generate_frame": (_i, [_vp, _vp, _i, _i, _vp, _vp, _f, _i, _vp, _vp, _sz, _vp]),
    "kk_csm_generate_frame_ex": (_i, [_vp, _vp, _i, _i, _vp, _vp, C.POINTER(KKCsmSampler), _vp, _vp, _vp, _sz, _vp]),
    "kk_csm_set_row_sampler": (_i, [_vp, _vp, _i, C.POINTER(KKCsmSampler)]),
    "kk_csm_generate_frame_rows": (_i, [_vp, _vp, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _sz, _vp]),
    "kk_csm_admit": (_i, [_vp, _vp, _i, _i, _vp, _vp, C.POINTER(KKCsmSampler), _vp, C.c_int32, _vp, _sz, _vp]),
    "kk_csm_prefix_create": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _sz, C.POINTER(_vp)]),
    "kk_csm_prefix_length": (_i, [_vp]),
    "kk_csm_prefix_bytes": (_sz, [_vp]),
    "kk_csm_prefix_read": (_i, [_vp, _vp, _vp, _sz]),
    "kk_csm_prefix_destroy": (None, [_vp]),
    "kk_csm_prefix_capture": (_i, [_vp, _vp, _i, _i, C.POINTER(_vp)]),
    "kk_csm_admit_transfer": (_i, [_vp, _vp, _i, _vp, _vp, _i]),
    "kk_csm_admit_prefixed": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp, C.POINTER(KKCsmSampler), _vp, C.c_int32, _vp, _sz, _vp]),
    "kk_csm_park_row": (_i, [_vp, _i]),
    "kk_csm_reset_caches_parked": (_i, [_vp]),
    "kk_csm_shift_caches": (_i, [_vp, _vp, _i, _vp, _sz]),
    "kk_csm_row_state": (_i, [_vp, _vp, C.POINTER(C.c_int32)]),
    "kk_csm_set_graph_mode": (_i, [_vp, _i]),
    "kk_csm_debug_logits": (_i, [_vp, _vp, _i, _vp]),
    "kk_csm_debug_timestamps": (_i, [_vp, _i]),
    "kk_op_csm_sample": (_i, [_vp, _i, _i, _vp, _f, _i, _vp, _vp]),
    "kk_op_csm_sample_ex": (_i, [_vp, _i, _i, _vp, C.POINTER(KKCsmSampler), _vp, _vp, _vp, _vp]),
    "kk_op_csm_sample_rows": (_i, [_vp, _i, _i, _vp, C.POINTER(KKCsmSampler), _vp, _vp, _vp, _vp]),
    "kk_op_csm_uniforms": (_i, [_vp, _i, _i, _u64, _vp, _vp, _vp]),
    "kk_csm_frag_choice": (_i, [_i, _i, _i, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "kk_csm_frag_pack": (_i, [_vp, _i, _i, _i, _vp]),
    "kk_csm_qfrag_bytes": (_i, [_i, _i, _i, _i, _i, C.POINTER(_sz), C.POINTER(_sz)]),
    "kk_csm_qfrag_pack": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "kk_op_csm_gemv_q": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _i, _i, _vp, C.c_longlong, _vp, _f, _vp, _i, _i, _i, _i, _vp, _vp, _vp, C.c_longlong, _vp,
                              C.c_longlong, _vp]),
    "kk_op_csm_gemm_prompt_q": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _i, _i, _vp, C.c_longlong, _vp, C.c_longlong, _vp, C.c_longlong]),
    "kk_op_csm_gemv": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, C.c_longlong, _vp, _f, _vp, _i, _i, _i, _i, _vp, _vp, _vp, C.c_longlong, _vp, C.c_longlong, _vp]),
    "kk_op_csm_gemm_prompt": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, C.c_longlong, _vp, C.c_longlong, _vp, C.c_longlong]),
    "kk_op_csm_linear_skinny": (_i, [_vp, _i, _i, _i, _vp, _i, _vp, _vp, _vp, _vp, _sz]),
    "kk_op_csm_attn_single": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "kk_op_csm_attn_prompt": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "kk_op_attn_cache_block": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, _vp]),
    "kk_mimi_create": (_i, [C.POINTER(KKMimiConfig), C.POINTER(_vp)]),
    "kk_mimi_destroy": (None, [_vp]),
    "kk_mimi_load_tensor": (_i, [_vp, C.c_char_p, C.POINTER(C.c_int64), _i, _vp]),
    "kk_mimi_finalize": (_i, [_vp, _vp]),
    "kk_mimi_samples_per_frame": (C.c_int64, [_vp]),
    "kk_mimi_workspace_bytes": (_sz, [_vp, _i, _i]),
    "kk_mimi_decode": (_i, [_vp, _vp, _i, _i, _vp, _vp, _sz, _vp]),
    "kk_mimi_stream_create": (_i, [_vp, _i, _i, C.POINTER(_vp)]),
    "kk_mimi_stream_create_chunked": (_i, [_vp, _i, _i, _i, _i, C.POINTER(_vp)]),
    "kk_mimi_stream_chunk_frames": (_i, [_vp]),
    "kk_mimi_stream_set_chunk": (_i, [_vp, _i]),
    "kk_mimi_stream_max_chunk_frames": (_i, [_vp]),
    "kk_mimi_encode_step": (_i, [_vp, _vp, _i, _vp, _vp, _sz, _vp]),
    "kk_mimi_stream_destroy": (None, [_vp]),
    "kk_mimi_stream_reset": (_i, [_vp]),
    "kk_mimi_stream_frames": (_i, [_vp]),
    "kk_mimi_stream_set_context": (_i, [_vp, _i]),
    "kk_mimi_stream_workspace_bytes": (_sz, [_vp, _i]),
    "kk_mimi_decode_step": (_i, [_vp, _vp, _i, _vp, _vp, _sz, _vp]),
    "kk_mimi_stream_create_rows": (_i, [_vp, _i, _i, _i, C.POINTER(_vp)]),
    "kk_mimi_stream_reset_row": (_i, [_vp, _vp, _i]),
    "kk_mimi_stream_row_frames": (_i, [_vp, _i]),
    "kk_mimi_decode_step_rows": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _sz, _vp]),
    "kk_mimi_stream_row_snapshot": (_i, [_vp, _vp, _i, C.POINTER(C.c_int32), _vp, _sz, C.POINTER(_sz)]),
    "kk_mimi_stream_create_rows_encoder": (_i, [_vp, _i, _i, _i, C.POINTER(_vp)]),
    "kk_mimi_encode_step_rows": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _sz, _vp]),
    "kk_mimi_encode_frames": (_i, [_vp, _i]),
    "kk_mimi_encode_workspace_bytes": (_sz, [_vp, _i, _i]),
    "kk_mimi_encode": (_i, [_vp, _vp, _i, _i, _vp, _vp, _sz, _vp]),
    "kk_resampler_create": (_i, [_i, _i, C.POINTER(_vp)]),
    "kk_resampler_destroy": (None, [_vp]),
    "kk_resampler_set_row": (_i, [_vp, _vp, _i, _i, _i, _vp, _i]),
    "kk_resampler_step": (_i, [_vp, _vp, _vp, C.c_longlong, _vp, _vp, _vp, C.c_longlong, _vp]),
    "kk_resampler_block_outputs": (_i, []),
    "kk_op_resample": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _vp]),
    "kk_resampler_set_row_fmt": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _i, _i]),
    "kk_resampler_step_fmt": (_i, [_vp, _vp, _vp, C.c_longlong, _vp, _vp, _vp, C.c_longlong, _vp]),
    "kk_pcm_convert_rows": (_i, [_vp, _i, _vp, C.c_longlong, _vp, _vp, C.c_longlong, _vp, _vp]),
    "kk_op_pcm_convert": (_i, [_vp, _vp, _i, _vp, _i, _i]),
    "kk_vad_create": (_i, [_i, C.POINTER(_vp)]),
    "kk_vad_destroy": (None, [_vp]),
    "kk_vad_set_row": (_i, [_vp, _vp, _i, _i, _f, _i]),
    "kk_vad_step": (_i, [_vp, _vp, _vp, C.c_longlong, _vp, _vp, _vp, C.c_longlong]),
    "kk_op_vad": (_i, [_vp, _vp, _i, _i, _f, _i, _vp, _vp]),
    "kk_vad_ring_create": (_i, [_i, C.POINTER(_vp)]),
    "kk_vad_ring_destroy": (None, [_vp]),
    "kk_vad_ring_set_row": (_i, [_vp, _vp, _i, _i, _f, _i, C.c_longlong, C.c_longlong]),
    "kk_vad_ring_step": (_i, [_vp, _vp, _vp, C.c_longlong, _vp, _vp, _vp, _vp, _vp, C.c_longlong]),
    "kk_ring_write_rows": (_i, [_vp, _i, _vp, C.c_longlong, _vp, C.c_longlong, C.c_longlong, _vp, _vp]),
    "kk_ring_read_rows": (_i, [_vp, _i, _vp, C.c_longlong, C.c_longlong, _vp, C.c_longlong, _vp, _vp, _vp]),
    "kk_op_log_mel": (_i, [_vp, _i, _vp, C.c_longlong, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i]),
    "kk_op_attention_long": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _vp, _i]),
    "kk_whisper_create": (_i, [C.POINTER(KKWhisperConfig), C.POINTER(_vp)]),
    "kk_whisper_destroy": (None, [_vp]),
    "kk_whisper_load_tensor": (_i, [_vp, C.c_char_p, C.POINTER(C.c_int64), _i, _vp]),
    "kk_whisper_finalize": (_i, [_vp, _vp]),
    "kk_whisper_encode_workspace_bytes": (_sz, [_vp, _i]),
    "kk_whisper_encode": (_i, [_vp, _vp, _i, _vp, _vp, _sz, _vp]),
    "kk_op_whisper_attn_rows_scratch_bytes": (_sz, [_i, _i, _i]),
    "kk_op_whisper_attn_rows": (_i, [_vp, _i, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _sz]),
    "kk_op_whisper_linear_rows": (_i, [_vp, _i, _i, _i, _vp, C.c_longlong, _vp, _vp, _i, _vp, C.c_longlong, _vp, C.c_longlong, _vp, C.c_longlong, _vp, _i]),
    "kk_op_whisper_embed": (_i, [_vp, _i, _i, _vp, _vp, _vp, _i, _vp, _i, _vp]),
    "kk_op_whisper_pick": (_i, [_vp, _i, _vp, C.c_longlong, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "kk_op_whisper_pick_reset": (_i, [_vp, _i, _vp, _vp]),
    "kk_op_whisper_pick_sampled": (_i, [_vp, _i, _vp, C.c_longlong, _vp, _vp, _f, _u64, _vp, _vp, _vp, _i, _vp, _vp]),
    "kk_whisper_text_create": (_i, [C.POINTER(KKWhisperTextConfig), C.POINTER(_vp)]),
    "kk_whisper_text_destroy": (None, [_vp]),
    "kk_whisper_text_load_tensor": (_i, [_vp, C.c_char_p, C.POINTER(C.c_int64), _i, _vp]),
    "kk_whisper_text_finalize": (_i, [_vp, _vp]),
    "kk_whisper_text_load_quantized": (_i, [_vp, C.c_char_p, C.POINTER(C.c_int64), _vp, _vp, _vp, _i, _i]),
    "kk_whisper_text_weight_info": (_i, [_vp, C.POINTER(_sz), C.POINTER(_sz), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "kk_whisper_text_weight_fallback": (C.c_char_p, [_vp, _i]),
    "kk_op_whisper_linear_rows_q": (_i, [_vp, _i, _i, _i, _vp, C.c_longlong, _vp, _vp, _i, _i, _vp, _i, _vp, C.c_longlong, _vp, C.c_longlong, _vp, C.c_longlong,
                                        _vp, _i]),
    "kk_op_whisper_embed_q": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _i, _vp]),
    "kk_whisper_text_state_bytes": (_sz, [_vp, _i]),
    "kk_whisper_text_workspace_bytes": (_sz, [_vp, _i, _i]),
    "kk_whisper_text_set_audio": (_i, [_vp, _vp, _i, _vp, _vp, _sz, _vp, _sz]),
    "kk_whisper_text_forward": (_i, [_vp, _vp, _i, _i, _vp, _vp, _i, _vp, _sz]),
    "kk_whisper_text_position": (_i, [_vp]),
    "kk_whisper_text_rewind": (_i, [_vp, _i]),
    "kk_whisper_text_pick_setup": (_i, [_vp, _vp, C.POINTER(KKWhisperPickParams), _vp]),
    "kk_whisper_text_pick": (_i, [_vp, _vp]),
    "kk_whisper_text_not_ended": (_i, [_vp, _vp, C.POINTER(C.c_int32)]),
    "kk_whisper_text_read": (_i, [_vp, _vp, _vp, _i, _vp]),
    "kk_whisper_text_state_bytes_groups": (_sz, [_vp, _i, _i]),
    "kk_whisper_text_set_audio_groups": (_i, [_vp, _vp, _i, _i, _vp, _vp, _sz, _vp, _sz]),
    "kk_whisper_text_sample_setup": (_i, [_vp, _vp, _f, _u64, _vp]),
    "kk_op_whisper_attn_rows_owned": (_i, [_vp, _i, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _sz]),
    "kk_op_whisper_beam_topk": (_i, [_vp, _i, _i, _vp, C.c_longlong, _vp, _vp, _vp, _vp, _vp]),
    "kk_op_whisper_beam_reset": (_i, [_vp, C.POINTER(KKWhisperBeamBufs)]),
    "kk_op_whisper_beam_select": (_i, [_vp, C.POINTER(KKWhisperBeamBufs), _i, _i, _vp, _vp, _vp, _vp]),
    "kk_whisper_text_beam_state_bytes": (_sz, [_vp, _i, _i, _i]),
    "kk_whisper_text_beam_setup": (_i, [_vp, _vp, _i, _i, _vp, _sz]),
    "kk_whisper_text_beam_not_complete": (_i, [_vp, _vp, C.POINTER(C.c_int32)]),
    "kk_whisper_text_beam_read": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "kk_whisper_text_rows_state_bytes": (_sz, [_vp, _i]),
    "kk_whisper_text_rows_workspace_bytes": (_sz, [_vp, _i, _i]),
    "kk_whisper_text_rows_open": (_i, [_vp, _vp, _i, _vp, _sz]),
    "kk_whisper_text_rows_admit": (_i, [_vp, _vp, _i, _vp, _vp, _i, C.POINTER(KKWhisperPickParams), _vp, _vp, _sz]),
    "kk_whisper_text_rows_forward": (_i, [_vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _sz]),
    "kk_whisper_text_rows_pick": (_i, [_vp, _vp, _vp, _i]),
    "kk_whisper_text_rows_flags": (_i, [_vp, _vp, _vp]),
    "kk_whisper_text_rows_read": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp]),
    "kk_whisper_text_rows_set_token": (_i, [_vp, _vp, _i, _i, _vp]),
    "kk_whisper_text_rows_set_draw": (_i, [_vp, _vp, _i, C.c_float, C.c_uint64, C.c_uint32]),
    "kk_whisper_text_rows_groups_state_bytes": (_sz, [_vp, _i]),
    "kk_whisper_text_rows_groups_bind": (_i, [_vp, _vp, _vp, _sz]),
    "kk_whisper_text_rows_admit_group": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _i, C.POINTER(KKWhisperPickParams), _vp, _i, _vp, _sz]),
    "kk_whisper_text_rows_group_read": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "kk_whisper_text_rows_group_release": (_i, [_vp, _i]),
    "kk_whisper_text_rows_group_offers": (_i, [_vp, _vp, _i, _vp, _vp]),
    "kk_op_mel_windows": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _vp]),
    "kk_op_log_mel_spans": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "kk_op_whisper_qk_rows_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "kk_op_whisper_qk_rows": (_i, [_vp, _i, _i, _i, _vp, _vp, _i, _i, _vp, _i, _i, _vp, C.c_longlong]),
    "kk_op_whisper_align_matrix_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "kk_op_whisper_align_matrix": (_i, [_vp, _i, _i, _vp, C.c_longlong, C.c_longlong, _i, _vp, _i, _vp, _i, _f, _i, _i, _vp, _i, _vp, _sz]),
    "kk_op_whisper_median_filter": (_i, [_vp, C.c_longlong, _i, _vp, C.c_longlong, _i, _vp, C.c_longlong]),
    "kk_op_whisper_dtw_workspace_bytes": (_sz, [_i, _i, _i]),
    "kk_op_whisper_dtw": (_i, [_vp, _i, _vp, C.c_longlong, _i, _vp, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz]),
    "kk_whisper_text_qk_bytes": (_sz, [_vp, _i, _i, _i, _i]),
    "kk_whisper_text_forward_qk": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _sz, _vp, _sz]),
    "kk_snac_create": (_i, [C.POINTER(KKSnacConfig), C.POINTER(_vp)]),
    "kk_snac_destroy": (None, [_vp]),
    "kk_snac_load_tensor": (_i, [_vp, C.c_char_p, C.POINTER(C.c_int64), _i, _vp]),
    "kk_snac_finalize": (_i, [_vp, _vp]),
    "kk_snac_hop_length": (C.c_int64, [_vp]),
    "kk_snac_decode_samples": (C.c_int64, [_vp, _i]),
    "kk_snac_decode_workspace_bytes": (_sz, [_vp, _i, _i]),
    "kk_snac_decode": (_i, [_vp, _vp, _i, _i, C.POINTER(_vp), C.POINTER(_vp), _vp, _sz, _vp]),
    "kk_snac_encode_frames": (_i, [_vp, _i]),
    "kk_snac_encode_workspace_bytes": (_sz, [_vp, _i, _i]),
    "kk_snac_encode": (_i, [_vp, _vp, _i, _i, _vp, _vp, _sz, C.POINTER(_vp)]),
    "kk_snac_debug_info": (_i, [_vp, C.c_char_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "kk_snac_debug_fetch": (_i, [_vp, _vp, C.c_char_p, _vp]),
    "kk_op_snac_dw_conv": (_i, [_vp, _i, _vp, C.c_longlong, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, C.c_longlong, _i]),
    "kk_op_snac_residual_unit": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _i, _vp, _vp, _vp, _i, C.POINTER(C.c_int)]),
    "kk_op_snac_from_codes": (_i, [_vp, _i, _i, _i, _i, C.POINTER(_vp), C.POINTER(C.c_int32), C.POINTER(_vp), _i, _vp, _vp, _i, _i]),
    "kk_op_snac_vq_search": (_i, [_vp, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _i]),
    "kk_op_snac_conv_cout1": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _i, _i, _vp, _i, _vp, _vp, _i, _vp]),
    "kk_mimi_debug_info": (_i, [_vp, C.c_char_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "kk_mimi_debug_fetch": (_i, [_vp, _vp, C.c_char_p, _vp]),
    "kk_debug_set_op_wfrag": (None, [_vp]),
    "kk_debug_set_op_variant": (None, [_i]),  # 4 (default), 5, or 40 = variant 4 slab by slab where its whole-K form would run; 41 / 51 = generic epilogue
    "kk_debug_last_conv_epi": (_i, []),
    "kk_debug_set_op_accumulate": (None, [_i]),
    "kk_debug_set_op_post_slope": (None, [_f]),
    "kk_set_graph_mode": (_i, [_vp, _i]),
    "kk_set_quantization": (_i, [_vp, _i, _i]),
    "kk_quantized_layers": (_i, [_vp]),
    "kk_mxfp8_bytes": (_i, [_i, _i, C.POINTER(_sz), C.POINTER(_sz)]),
    "kk_mxfp8_pack_weight": (_i, [_vp, _i, _i, _i, _vp, _vp]),
    "kk_op_linear_mxfp8": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _i]),
    "kk_profile_begin": (_i, [_vp, _i]),
    "kk_profile_end": (_i, [_vp, _i, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
}

_lib = None


class KokoroHipError(RuntimeError):
    pass


def load():
    """Load the shared library (once).  Raises KokoroHipError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("KK_HIP_LIB", LIB_PATH)  # instrumented side builds only (build.py --trace)
    if not os.path.exists(path):
        raise KokoroHipError(
            f"{path} not found: build it with `python mlx-audio_amd/build.py` (hipcc, gfx950). "
            "The Kokoro hot path has no CPU or PyTorch fallback."
        )
    # torch brings its own copy of the HIP runtime (torch/lib/libamdhip64.so).  If this library were loaded first it would bind to the system
    # copy under /opt/rocm, torch would then load its own, and the process would hold TWO HIP runtimes: the first hipMalloc of kk_finalize
    # fails (seen with `python __graft_entry__.py smoke`, where build() loads the library before anything imports torch).  Importing torch
    # first makes its runtime the one this library's libamdhip64 dependency resolves to.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    if lib.kk_abi_version() != 2 or lib.kk_abi_minor() < 29:
        raise KokoroHipError("libkokoro_hip.so ABI version mismatch")
    _lib = lib
    return lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().kk_last_error()
        raise KokoroHipError(f"{what}: {msg.decode() if msg else 'unknown error'}")
