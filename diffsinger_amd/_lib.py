"""ctypes binding of libdsdenoise.so (include/dsdenoise.h).

There is exactly one compute path: the HIP library.  If it is missing or does not load, importing
this module raises - there is no eager / CPU fallback to fall through to.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libdsdenoise.so")

DSD_MAX_TERMS = 8
DSD_MAX_OUT = 3
DSD_SRC_MODEL = -1
DSD_SRC_NOISE_BASE = -1000
DSD_SAMPLE_GRAPH = 1
DSD_SAMPLE_TRANSPOSE = 2
DSD_SAMPLE_GRAPH_LAZY = 4
BACKBONE_IDS = {"wavenet": 0, "lynxnet": 1}
AUX_CONVNEXT = 2
DSD_NOISE_NORMAL, DSD_NOISE_UNIFORM = 0, 1
DSD_DOMAIN_X_T, DSD_DOMAIN_STEP, DSD_DOMAIN_VOC_SOURCE, DSD_DOMAIN_VOC_PRE, DSD_DOMAIN_VOC_PHASE = 1, 2, 3, 4, 5
DSD_TRACK_F64, DSD_TRACK_F32, DSD_TRACK_PCM = 0, 1, 2
DSD_SCORE_WORKSPACE_BYTES = 65536
DSD_CURVE_MAX, DSD_CURVE_CHUNK = 32, 256
DSD_CURVE_PLAIN, DSD_CURVE_CLIP, DSD_CURVE_GENDER, DSD_CURVE_PITCH = 0, 1, 2, 3
DSD_DIFFUSE_DDPM, DSD_DIFFUSE_REFLOW = 0, 1
LOSS_IDS = {"l1": 0, "l2": 1}                               # DSD_LOSS_*
DUR_LOSS_IDS = {"mse": 0, "huber": 1}                       # DSD_DUR_*
ACT_IDS = {"PReLU": 0, "SiLU": 1, "ReLU": 2}
SCHEDULE_IDS = {"linear": 0, "cosine": 1}                  # DSD_SCHEDULE_*
DSD_DDPM_TABLES = 12
# DSD_SAMPLER_*: the DDPM family under the names of hparams['diff_accelerator'], rectified flow under `rf_` + algorithm
SAMPLER_IDS = {"ddpm": 0, "ddim": 1, "pndm": 2, "dpm-solver": 3, "unipc": 4, "rf_euler": 5, "rf_rk2": 6, "rf_rk4": 7,
               "rf_rk5": 8, "rf_euler_onnx": 9}

EXPORTS = [
    "dsd_api_version", "dsd_create", "dsd_create_any_width", "dsd_destroy", "dsd_last_error", "dsd_load_weight",
    "dsd_finalize_weights", "dsd_prepare_cond", "dsd_denoise", "dsd_sample", "dsd_get_stats",
    "dsd_kernel_timing", "dsd_kernel_timing_read", "dsd_kernel_timing_classes", "dsd_kernel_ledger", "dsd_kernel_ledger_reset", "dsd_set_precision", "dsd_aux_decode", "dsd_encoder_create", "dsd_encode", "dsd_vocoder_create", "dsd_vocode", "dsd_vocode_ragged",
    "dsd_token_encoder_create", "dsd_token_encode", "dsd_predict_dur", "dsd_cond_assemble", "dsd_set_lengths",
    "dsd_mel_create", "dsd_mel_filterbank", "dsd_mel_num_frames", "dsd_mel_analyze",
    "dsd_rmvpe_create", "dsd_rmvpe_num_frames", "dsd_rmvpe_filterbank", "dsd_rmvpe_mel_to_hidden", "dsd_rmvpe_decode",
    "dsd_rmvpe_decode_at", "dsd_rmvpe_decode_viterbi", "dsd_rmvpe_infer",
    "dsd_hnsep_create", "dsd_hnsep_num_frames", "dsd_hnsep_mask", "dsd_hnsep_separate", "dsd_base_harmonic",
    "dsd_variance_curves",
    "dsd_length_regulate", "dsd_frame_curve", "dsd_seconds_to_frames", "dsd_curve_resample",
    "dsd_noise_fill",
    "dsd_ddpm_tables_fill", "dsd_program_build", "dsd_program_free", "dsd_onnx_ddpm_plan",
    "dsd_track_plan", "dsd_track_place", "dsd_track_peak", "dsd_track_export",
    "dsd_diffuse", "dsd_masked_loss", "dsd_curve_stats", "dsd_dur_score",
    "dsd_model_open", "dsd_model_close", "dsd_model_count", "dsd_model_find", "dsd_model_section", "dsd_model_config",
    "dsd_model_tensor", "dsd_model_meta_at", "dsd_model_meta", "dsd_model_create",
    "dsd_variance_open", "dsd_variance_close", "dsd_variance_info", "dsd_variance_backbone", "dsd_variance_encode",
    "dsd_variance_dur", "dsd_variance_pitch_cond", "dsd_variance_cond", "dsd_variance_pitch_post", "dsd_variance_post",
    "dsd_acoustic_open", "dsd_acoustic_close", "dsd_acoustic_info", "dsd_acoustic_handle", "dsd_acoustic_condition",
    "dsd_acoustic_plan", "dsd_acoustic_start", "dsd_acoustic_sample",
    "dsd_acoustic_set_lengths", "dsd_acoustic_spk_mix", "dsd_variance_spk_mix", "dsd_vocode_seeded",
    "dsd_word_dur", "dsd_group_midi", "dsd_rhythm_align", "dsd_variance_set_lengths",
]
DSD_API_VERSION = 10
DSD_EINVAL, DSD_ESTATE, DSD_EHIP, DSD_ENOMEM, DSD_ENOTFOUND, DSD_EIO = -1, -2, -3, -4, -5, -6
DSD_MODEL_FORMAT_VERSION, DSD_MODEL_MAX_SECTIONS, DSD_MODEL_MAX_TENSORS, DSD_MODEL_MAX_META = 1, 64, 65536, 65536
DSD_MODEL_MAX_NAME, DSD_MODEL_ALIGN = 255, 64
POS_ROPE, POS_REL, POS_NONE, POS_SIN = 0, 1, 2, 3       # DSD_POS_*
FFN_ACTS = {"gelu": 0, "relu": 1, "swish": 2, "swiglu": 3}    # DSD_FFN_* (TransformerFFNLayer, common_layers.py:126-136)
DSD_VARIANCE_TABLES, DSD_VAR_PITCH, DSD_VAR_VARIANCES, DSD_VAR_MAX_CURVES = 10, 0, 1, 4
DSD_ACOUSTIC_TABLES, DSD_AC_FS2, DSD_AC_AUX, DSD_AC_DENOISER, DSD_AC_PITCH_BINS = 11, 0, 1, 2, 300
DSD_AC_START_NOISE, DSD_AC_START_MIX, DSD_AC_START_SOURCE = 0, 1, 2
EMBED_FLAGS = {"energy": 1, "breathiness": 2, "voicing": 4, "tension": 8, "key_shift": 16, "speed": 32}


class DsdConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "struct_size", "backbone", "in_dims", "n_feats", "num_layers", "num_channels", "hidden_size",
        "dilation_cycle_length", "expansion_factor", "kernel_size", "activation", "strong_cond", "device")]


class DsdEncoderConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("vocab_size", C.c_int32), ("hidden_size", C.c_int32),
                ("enc_layers", C.c_int32), ("num_heads", C.c_int32), ("ffn_kernel_size", C.c_int32),
                ("num_spk", C.c_int32), ("num_lang", C.c_int32), ("embed_flags", C.c_uint32), ("pos_mode", C.c_int32),
                ("device", C.c_int32), ("ffn_act", C.c_int32)]


class DsdVocoderConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("num_mels", C.c_int32), ("sampling_rate", C.c_int32),
                ("upsample_initial_channel", C.c_int32), ("n_ups", C.c_int32), ("upsample_rates", C.c_int32 * 8),
                ("upsample_kernel_sizes", C.c_int32 * 8), ("resblock", C.c_int32), ("n_kernels", C.c_int32),
                ("resblock_kernel_sizes", C.c_int32 * 8), ("n_dilations", C.c_int32 * 8),
                ("resblock_dilation_sizes", (C.c_int32 * 4) * 8), ("harmonic_num", C.c_int32), ("mini_nsf", C.c_int32),
                ("noise_sigma", C.c_float), ("device", C.c_int32)]


class DsdMelConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("sampling_rate", C.c_int32), ("n_fft", C.c_int32), ("win_size", C.c_int32),
                ("hop_size", C.c_int32), ("num_mels", C.c_int32), ("fmin", C.c_double), ("fmax", C.c_double),
                ("clip_val", C.c_double), ("device", C.c_int32)]


class DsdRmvpeConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("n_blocks", C.c_int32), ("n_gru", C.c_int32), ("en_de_layers", C.c_int32),
                ("inter_layers", C.c_int32), ("en_out_channels", C.c_int32), ("device", C.c_int32)]


class DsdHnsepConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("n_fft", C.c_int32), ("hop_length", C.c_int32), ("nout", C.c_int32),
                ("nout_lstm", C.c_int32), ("is_mono", C.c_int32), ("device", C.c_int32)]


class DsdTokenEncoderConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("hidden_size", C.c_int32), ("enc_layers", C.c_int32), ("num_heads", C.c_int32),
                ("ffn_kernel_size", C.c_int32), ("out_dims", C.c_int32), ("dur_layers", C.c_int32), ("dur_chans", C.c_int32),
                ("dur_kernel_size", C.c_int32), ("dur_offset", C.c_float), ("pos_mode", C.c_int32), ("device", C.c_int32),
                ("ffn_act", C.c_int32)]


class _AssembleGather(C.Structure):
    _fields_ = [("table", C.c_void_p), ("batch_stride", C.c_int64), ("rows", C.c_int64), ("idx", C.c_void_p),
                ("idx_offset", C.c_int64), ("scale", C.c_float), ("row_scale", C.c_void_p)]


class _AssembleTerm(C.Structure):
    _fields_ = [("s", C.c_void_p), ("v", C.c_void_p)]


class DsdAssembleArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("device", C.c_int32), ("B", C.c_int32), ("T", C.c_int32), ("H", C.c_int32),
                ("n_gather", C.c_int32), ("n_terms", C.c_int32), ("gather", _AssembleGather * 4), ("term", _AssembleTerm * 16)]


class DsdEncodeExtras(C.Structure):
    _fields_ = [("languages", C.c_void_p), ("spk_embed_id", C.c_void_p), ("spk_mix_embed", C.c_void_p),
                ("spk_mix_bstride", C.c_int64), ("spk_mix_tstride", C.c_int64), ("key_shift", C.c_void_p),
                ("speed", C.c_void_p), ("energy", C.c_void_p), ("breathiness", C.c_void_p), ("voicing", C.c_void_p),
                ("tension", C.c_void_p)]


class DsdNoiseSpec(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("kind", C.c_int32), ("domain", C.c_uint32), ("first_stream", C.c_int32),
                ("n", C.c_int32), ("B", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32),
                ("seeds", C.POINTER(C.c_uint64)), ("scale", C.c_float), ("src", C.c_void_p), ("src_scale", C.c_float)]


class DsdDiffuseSpec(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("kind", C.c_int32), ("B", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32),
                ("domain", C.c_uint32), ("x0", C.c_void_p), ("eps", C.c_void_p), ("a", C.c_void_p), ("c", C.c_void_p),
                ("seeds", C.POINTER(C.c_uint64))]


class DsdLossSpec(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("kind", C.c_int32), ("B", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32),
                ("pred", C.c_void_p), ("target", C.c_void_p), ("non_padding", C.c_void_p), ("t", C.c_void_p)]


class DsdCurveResult(C.Structure):
    _fields_ = [("close", C.c_int64), ("total", C.c_int64), ("sum_target", C.c_double), ("sum_target_sq", C.c_double),
                ("sum_residual_sq", C.c_double)]


class DsdDurSpec(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("kind", C.c_int32), ("B", C.c_int32), ("L", C.c_int32), ("n_words", C.c_int32),
                ("offset", C.c_float), ("rhythm_tolerance", C.c_float), ("pdur_tolerance", C.c_float),
                ("dur_pred", C.c_void_p), ("dur_gt", C.c_void_p), ("ph2word", C.c_void_p), ("mask", C.c_void_p)]


class DsdDurResult(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("pdur_sum", "wdur_sum", "sdur_sum", "pdur_mean", "wdur_mean", "sdur_mean")] + \
               [(n, C.c_int64) for n in ("rhythm_correct", "rhythm_total", "pdur_accurate", "pdur_total")]


class DsdCurve(C.Structure):
    _fields_ = [("points", C.c_void_p), ("out", C.c_void_p), ("uv_out", C.c_void_p), ("src_step", C.c_double),
                ("dst_step", C.c_double), ("n_points", C.c_int32), ("length", C.c_int32), ("pad_to", C.c_int32),
                ("op", C.c_int32), ("lo", C.c_float), ("hi", C.c_float)]


class DsdModelSectionInfo(C.Structure):
    _fields_ = [("name", C.c_char_p), ("kind", C.c_int32), ("config_size", C.c_int32), ("n_tensors", C.c_int32),
                ("total_floats", C.c_int64)]


class DsdModelTensorInfo(C.Structure):
    _fields_ = [("name", C.c_char_p), ("ndim", C.c_int32), ("shape", C.c_int64 * 4), ("count", C.c_int64),
                ("data", C.POINTER(C.c_float))]


class DsdVarianceConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("hidden_size", C.c_int32), ("vocab_size", C.c_int32), ("num_lang", C.c_int32),
                ("num_spk", C.c_int32), ("predict_dur", C.c_int32), ("predict_pitch", C.c_int32),
                ("use_melody_encoder", C.c_int32), ("use_glide_embed", C.c_int32), ("use_lang_id", C.c_int32),
                ("use_spk_id", C.c_int32), ("variances", C.c_uint32), ("melody_hidden_size", C.c_int32),
                ("glide_rows", C.c_int32), ("glide_embed_scale", C.c_float), ("smooth_width", C.c_int32),
                ("pitch_repeat_bins", C.c_int32), ("pitd_norm_min", C.c_float), ("pitd_norm_max", C.c_float),
                ("pitd_clip_min", C.c_float), ("pitd_clip_max", C.c_float), ("var_repeat_bins", C.c_int32),
                ("var_norm_min", C.c_float * 4), ("var_norm_max", C.c_float * 4), ("var_clamp_min", C.c_float * 4),
                ("var_clamp_max", C.c_float * 4), ("var_no_clamp", C.c_int32 * 4), ("diffusion_type", C.c_int32),
                ("timesteps", C.c_int32), ("k_step", C.c_int32), ("time_scale_factor", C.c_float)]


class DsdVarianceEncodeArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("B", C.c_int32), ("L", C.c_int32), ("W", C.c_int32), ("tokens", C.c_void_p),
                ("word_div", C.c_void_p), ("word_dur", C.c_void_p), ("ph_dur", C.c_void_p), ("languages", C.c_void_p),
                ("encoder_out", C.c_void_p), ("x_masks", C.c_void_p), ("ph2word", C.c_void_p)]


class DsdVarianceDurArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("B", C.c_int32), ("L", C.c_int32), ("encoder_out", C.c_void_p),
                ("x_masks", C.c_void_p), ("ph_midi", C.c_void_p), ("spk_embed", C.c_void_p), ("spk_rows", C.c_int32),
                ("ph_dur_pred", C.c_void_p)]


class DsdVariancePitchCondArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("B", C.c_int32), ("L", C.c_int32), ("N", C.c_int32), ("T", C.c_int32),
                ("encoder_out", C.c_void_p), ("ph_dur", C.c_void_p), ("note_midi", C.c_void_p), ("note_rest", C.c_void_p),
                ("note_dur", C.c_void_p), ("note_glide", C.c_void_p), ("pitch", C.c_void_p), ("expr", C.c_void_p),
                ("retake", C.c_void_p), ("spk_embed", C.c_void_p), ("spk_rows", C.c_int32),
                ("lengths", C.POINTER(C.c_int32)), ("pitch_cond", C.c_void_p), ("base_pitch", C.c_void_p)]


class DsdVarianceCondArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("B", C.c_int32), ("L", C.c_int32), ("T", C.c_int32), ("encoder_out", C.c_void_p),
                ("ph_dur", C.c_void_p), ("pitch", C.c_void_p), ("curves", C.c_void_p * 4), ("retake", C.c_void_p),
                ("spk_embed", C.c_void_p), ("spk_rows", C.c_int32), ("variance_cond", C.c_void_p)]


class DsdAcousticConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("hidden_size", C.c_int32), ("vocab_size", C.c_int32), ("out_dims", C.c_int32),
                ("num_lang", C.c_int32), ("num_spk", C.c_int32), ("use_lang_id", C.c_int32), ("use_spk_id", C.c_int32),
                ("embed_flags", C.c_uint32), ("f0_discrete", C.c_int32), ("use_shallow_diffusion", C.c_int32),
                ("shift_min", C.c_float), ("shift_max", C.c_float), ("speed_min", C.c_float), ("speed_max", C.c_float),
                ("mel_base_e", C.c_int32), ("diffusion_type", C.c_int32), ("timesteps", C.c_int32), ("k_step", C.c_int32),
                ("schedule_type", C.c_int32), ("max_beta", C.c_double), ("t_start", C.c_float), ("time_scale_factor", C.c_float)]


class DsdAcousticConditionArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("B", C.c_int32), ("L", C.c_int32), ("T", C.c_int32), ("tokens", C.c_void_p),
                ("durations", C.c_void_p), ("f0", C.c_void_p), ("curves", C.c_void_p * 4), ("gender", C.c_void_p),
                ("velocity", C.c_void_p), ("spk_embed", C.c_void_p), ("spk_rows", C.c_int32), ("languages", C.c_void_p),
                ("condition", C.c_void_p), ("aux_mel", C.c_void_p), ("f0_coarse", C.c_void_p)]


class DsdAcousticPlan(C.Structure):
    _fields_ = [("mode", C.c_int32), ("start", C.c_int32), ("t_max", C.c_int32), ("speedup", C.c_int32), ("t_start", C.c_float),
                ("n_step_noise", C.c_int32), ("src_scale", C.c_float), ("noise_scale", C.c_float), ("steps", C.c_int32)]


class DsdWordDurArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("B", C.c_int32), ("N", C.c_int32), ("W", C.c_int32), ("dur", C.c_void_p),
                ("index", C.c_void_p), ("slur", C.c_void_p), ("totals", C.POINTER(C.c_int64)), ("word_dur", C.c_void_p),
                ("index_out", C.c_void_p)]


class DsdGroupMidiArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("B", C.c_int32), ("Nn", C.c_int32), ("G", C.c_int32), ("L", C.c_int32), ("T", C.c_int32),
                ("note_midi", C.c_void_p), ("note_dur", C.c_void_p), ("group_dur", C.c_void_p), ("ph2word", C.c_void_p),
                ("midi", C.c_void_p)]


class DsdRhythmAlignArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("B", C.c_int32), ("L", C.c_int32), ("W", C.c_int32), ("ph_dur_pred", C.c_void_p),
                ("ph2word", C.c_void_p), ("word_dur", C.c_void_p), ("ph_dur", C.c_void_p)]


class DsdSpkMixArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("B", C.c_int32), ("rows", C.c_int32), ("N", C.c_int32),
                ("ids", C.POINTER(C.c_int32)), ("values", C.c_void_p), ("normalize", C.c_int32), ("out", C.c_void_p)]


class DsdVocodeSeededArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("B", C.c_int32), ("T", C.c_int32), ("vocoder", C.c_void_p), ("mel", C.c_void_p),
                ("stride_b", C.c_int64), ("stride_m", C.c_int64), ("stride_t", C.c_int64), ("lengths", C.POINTER(C.c_int32)),
                ("f0", C.c_void_p), ("seeds", C.POINTER(C.c_uint64)), ("wav_out", C.c_void_p)]


# the config struct of each handle kind (the DSD_* enum), and the create call dsd_model_create makes for it
KIND_CONFIGS = {0: DsdConfig, 1: DsdConfig, 2: DsdConfig, 3: DsdEncoderConfig, 4: DsdVocoderConfig, 5: DsdTokenEncoderConfig,
                6: DsdMelConfig, 7: DsdRmvpeConfig, 8: DsdHnsepConfig, 10: DsdVarianceConfig,       # 9 is not assigned
                11: DsdAcousticConfig}
KIND_NAMES = {0: "wavenet", 1: "lynxnet", 2: "aux_convnext", 3: "fs2_acoustic", 4: "nsf_hifigan", 5: "fs2_tokens", 6: "mel",
              7: "rmvpe", 8: "hnsep_vr", 10: "variance_tables", 11: "acoustic_tables"}


class DsdTerm(C.Structure):
    _fields_ = [("src", C.c_int32), ("coef", C.c_float)]


class DsdLincomb(C.Structure):
    _fields_ = [("dst", C.c_int32), ("n_terms", C.c_int32), ("terms", DsdTerm * DSD_MAX_TERMS)]


class DsdEval(C.Structure):
    _fields_ = [("x_buf", C.c_int32), ("t", C.c_float), ("n_out", C.c_int32), ("out", DsdLincomb * DSD_MAX_OUT)]


class DsdProgram(C.Structure):
    _fields_ = [("n_bufs", C.c_int32), ("result_buf", C.c_int32), ("n_evals", C.c_int32),
                ("n_noise", C.c_int32), ("evals", C.POINTER(DsdEval))]


class DsdSamplerSpec(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("sampler", C.c_int32), ("timesteps", C.c_int32), ("t_max", C.c_int32),
                ("speedup", C.c_int32), ("t_lo", C.c_int32), ("noise_index0", C.c_int32), ("steps", C.c_int32),
                ("tables", C.POINTER(C.c_float)), ("t_start", C.c_double), ("time_scale_factor", C.c_double)]


class DsdStats(C.Structure):
    _fields_ = [("weight_bytes", C.c_int64), ("workspace_bytes", C.c_int64),
                ("flops_per_frame_nfe", C.c_int64), ("bytes_per_frame_nfe", C.c_int64),
                ("kernels_per_nfe", C.c_int32), ("graphs_cached", C.c_int32),
                ("layer_launches", C.c_int32), ("fused_tiles", C.c_int32), ("split_tiles", C.c_int32),
                ("precision", C.c_int32)]


class DsdKernelTime(C.Structure):
    _fields_ = [("name", C.c_char * 96), ("mean_ms", C.c_double), ("launches_timed", C.c_int64),
                ("launches", C.c_int64), ("evaluations", C.c_int64), ("flops_per_launch", C.c_double),
                ("bytes_per_launch", C.c_double)]


class DsdKernelLaunches(C.Structure):
    _fields_ = [("symbol", C.c_char_p), ("group", C.c_int32), ("reserved", C.c_int32), ("launches", C.c_int64)]


class NativeLibraryError(RuntimeError):
    pass


def _load():
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryError(
            f"{LIB_PATH} is missing: build it with `python -m diffsinger_amd.build_native` "
            "(hipcc --offload-arch=gfx950). diffsinger_amd has no CPU or eager fallback.")
    # torch ships its own libamdhip64.so.7; importing torch first makes the dynamic loader bind this
    # library to the SAME HIP runtime instance that owns torch's device memory and streams.
    import torch  # noqa: F401
    try:
        lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    except OSError as e:  # pragma: no cover
        raise NativeLibraryError(f"could not load {LIB_PATH}: {e}") from e
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    lib.dsd_api_version.restype = C.c_int
    lib.dsd_create.argtypes = [C.POINTER(DsdConfig), C.POINTER(vp)]
    lib.dsd_create_any_width.argtypes = [C.POINTER(DsdConfig), C.POINTER(vp)]
    lib.dsd_destroy.argtypes = [vp]
    lib.dsd_destroy.restype = None
    lib.dsd_last_error.argtypes = [vp]
    lib.dsd_last_error.restype = C.c_char_p
    lib.dsd_load_weight.argtypes = [vp, C.c_char_p, vp, C.POINTER(i64), i32, i32]
    lib.dsd_finalize_weights.argtypes = [vp]
    lib.dsd_prepare_cond.argtypes = [vp, vp, i32, i32, i64, i64, i64, vp]
    lib.dsd_denoise.argtypes = [vp, vp, vp, i32, vp, vp]
    lib.dsd_sample.argtypes = [vp, C.POINTER(DsdProgram), vp, vp, vp, vp, vp, C.c_uint32, vp]
    lib.dsd_aux_decode.argtypes = [vp, vp, i32, i32, i64, i64, i64, vp, vp, vp, vp]
    lib.dsd_vocoder_create.argtypes = [C.POINTER(DsdVocoderConfig), C.POINTER(vp)]
    lib.dsd_vocode.argtypes = [vp, vp, i32, i32, i64, i64, i64, vp, vp, vp, vp, vp, vp]
    lib.dsd_vocode_ragged.argtypes = [vp, vp, i32, i32, i64, i64, i64, C.POINTER(C.c_int32), vp, vp, vp, vp, vp, vp]
    lib.dsd_encoder_create.argtypes = [C.POINTER(DsdEncoderConfig), C.POINTER(vp)]
    lib.dsd_token_encoder_create.argtypes = [C.POINTER(DsdTokenEncoderConfig), C.POINTER(vp)]
    lib.dsd_token_encode.argtypes = [vp, vp, vp, i32, i32, vp, vp]
    lib.dsd_predict_dur.argtypes = [vp, vp, vp, i32, i32, vp, vp]
    lib.dsd_cond_assemble.argtypes = [C.POINTER(DsdAssembleArgs), vp, vp]
    lib.dsd_set_lengths.argtypes = [vp, C.POINTER(C.c_int32), i32, vp]
    lib.dsd_encode.argtypes = [vp, vp, vp, vp, i32, i32, i32, C.POINTER(DsdEncodeExtras), vp, vp]
    lib.dsd_mel_create.argtypes = [C.POINTER(DsdMelConfig), C.POINTER(vp)]
    lib.dsd_mel_filterbank.argtypes = [C.POINTER(DsdMelConfig), C.POINTER(C.c_float)]
    lib.dsd_mel_num_frames.argtypes = [C.POINTER(DsdMelConfig), i64, C.c_double, C.c_double]
    lib.dsd_mel_num_frames.restype = i64
    lib.dsd_mel_analyze.argtypes = [vp, vp, i32, i64, i64, C.POINTER(i64), C.c_double, C.c_double, vp, i64, i64, i64, vp]
    lib.dsd_rmvpe_create.argtypes = [C.POINTER(DsdRmvpeConfig), C.POINTER(vp)]
    lib.dsd_rmvpe_num_frames.argtypes = [i64, i32]
    lib.dsd_rmvpe_num_frames.restype = i64
    lib.dsd_rmvpe_filterbank.argtypes = [C.POINTER(C.c_float)]
    lib.dsd_rmvpe_mel_to_hidden.argtypes = [vp, vp, i32, i32, i64, i64, i64, C.POINTER(i64), vp, i64, i64, vp]
    lib.dsd_rmvpe_decode.argtypes = [vp, vp, i32, i32, i64, i64, C.c_float, vp, i64, vp]
    lib.dsd_rmvpe_decode_at.argtypes = [vp, vp, vp, i32, i32, i64, i64, i64, C.c_float, vp, i64, vp]
    lib.dsd_rmvpe_decode_viterbi.argtypes = [vp, vp, i32, i32, i64, i64, C.POINTER(i64), C.c_float, vp, i64, vp, i64, vp]
    lib.dsd_rmvpe_infer.argtypes = [vp, vp, i32, i64, i64, C.POINTER(i64), i32, C.c_float, vp, i64, vp, i64, i64, vp]
    lib.dsd_hnsep_create.argtypes = [C.POINTER(DsdHnsepConfig), C.POINTER(vp)]
    lib.dsd_hnsep_num_frames.argtypes = [i64, i32]
    lib.dsd_hnsep_num_frames.restype = i64
    lib.dsd_hnsep_mask.argtypes = [vp, vp, i32, i32, i64, i64, i64, i64, C.POINTER(i64), vp, i64, i64, i64, i64, vp]
    lib.dsd_hnsep_separate.argtypes = [vp, vp, i32, i64, i64, i64, C.POINTER(i64), vp, i64, i64, vp]
    lib.dsd_base_harmonic.argtypes = [vp, vp, i32, i64, i64, C.POINTER(i64), vp, i64, C.POINTER(i64), i32, i32, i32, vp, i64, vp]
    lib.dsd_variance_curves.argtypes = [vp, vp, vp, vp, i32, i64, C.POINTER(i64), i32, i32, C.POINTER(i64), i32, i32, vp, vp, vp,
                                        vp, i64, vp]
    lib.dsd_length_regulate.argtypes = [i32, vp, i32, i32, i32, vp, vp]
    lib.dsd_frame_curve.argtypes = [i32, vp, vp, vp, vp, i32, i32, i32, C.POINTER(i32), C.POINTER(C.c_float), i32, vp, vp, vp, vp]
    lib.dsd_seconds_to_frames.argtypes = [C.POINTER(C.c_float), i32, C.c_double, C.POINTER(i64), C.POINTER(i64)]
    lib.dsd_curve_resample.argtypes = [i32, C.POINTER(DsdCurve), i32, vp]
    lib.dsd_noise_fill.argtypes = [i32, C.POINTER(DsdNoiseSpec), vp, vp]
    lib.dsd_ddpm_tables_fill.argtypes = [i32, i32, C.c_double, C.POINTER(C.c_float)]
    lib.dsd_program_build.argtypes = [C.POINTER(DsdSamplerSpec), C.POINTER(C.POINTER(DsdProgram))]
    lib.dsd_program_free.argtypes = [C.POINTER(DsdProgram)]
    lib.dsd_program_free.restype = None
    lib.dsd_onnx_ddpm_plan.argtypes = [i32, i32, C.POINTER(i64), i32, i32, C.c_double, C.POINTER(i32), C.POINTER(i32)]
    lib.dsd_track_plan.argtypes = [i32, C.POINTER(C.c_double), C.POINTER(i64), i32, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]
    lib.dsd_track_place.argtypes = [i32, vp, i64, i64, i64, vp, i64, vp]
    lib.dsd_track_peak.argtypes = [i32, vp, i64, vp, vp]
    lib.dsd_track_export.argtypes = [i32, vp, i64, i32, vp, vp, vp]
    lib.dsd_diffuse.argtypes = [i32, C.POINTER(DsdDiffuseSpec), vp, vp, vp]
    lib.dsd_masked_loss.argtypes = [i32, C.POINTER(DsdLossSpec), vp, vp, vp]
    lib.dsd_curve_stats.argtypes = [i32, vp, vp, vp, i64, C.c_float, vp, vp, vp]
    lib.dsd_dur_score.argtypes = [i32, C.POINTER(DsdDurSpec), vp, vp, vp, vp, vp]
    lib.dsd_model_open.argtypes = [C.c_char_p, C.POINTER(vp)]
    lib.dsd_model_close.argtypes = [vp]
    lib.dsd_model_close.restype = None
    lib.dsd_model_count.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    lib.dsd_model_find.argtypes = [vp, C.c_char_p]
    lib.dsd_model_section.argtypes = [vp, i32, C.POINTER(DsdModelSectionInfo)]
    lib.dsd_model_config.argtypes = [vp, i32, vp, i32]
    lib.dsd_model_tensor.argtypes = [vp, i32, i32, C.POINTER(DsdModelTensorInfo)]
    lib.dsd_model_meta_at.argtypes = [vp, i32, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p)]
    lib.dsd_model_meta.argtypes = [vp, C.c_char_p]
    lib.dsd_model_meta.restype = C.c_char_p
    lib.dsd_model_create.argtypes = [vp, i32, i32, C.POINTER(vp)]
    lib.dsd_variance_open.argtypes = [vp, C.c_char_p, i32, C.POINTER(vp)]
    lib.dsd_variance_close.argtypes = [vp]
    lib.dsd_variance_close.restype = None
    lib.dsd_variance_info.argtypes = [vp, C.POINTER(DsdVarianceConfig)]
    lib.dsd_variance_backbone.argtypes = [vp, i32, C.POINTER(vp)]
    lib.dsd_variance_encode.argtypes = [vp, C.POINTER(DsdVarianceEncodeArgs), vp]
    lib.dsd_variance_dur.argtypes = [vp, C.POINTER(DsdVarianceDurArgs), vp]
    lib.dsd_variance_pitch_cond.argtypes = [vp, C.POINTER(DsdVariancePitchCondArgs), vp]
    lib.dsd_variance_cond.argtypes = [vp, C.POINTER(DsdVarianceCondArgs), vp]
    lib.dsd_variance_pitch_post.argtypes = [vp, vp, vp, i32, i32, vp, vp]
    lib.dsd_variance_post.argtypes = [vp, vp, i32, i32, C.POINTER(vp), vp]
    lib.dsd_acoustic_open.argtypes = [vp, C.c_char_p, i32, C.POINTER(vp)]
    lib.dsd_acoustic_close.argtypes = [vp]
    lib.dsd_acoustic_close.restype = None
    lib.dsd_acoustic_info.argtypes = [vp, C.POINTER(DsdAcousticConfig)]
    lib.dsd_acoustic_handle.argtypes = [vp, i32, C.POINTER(vp)]
    lib.dsd_acoustic_condition.argtypes = [vp, C.POINTER(DsdAcousticConditionArgs), vp]
    lib.dsd_acoustic_plan.argtypes = [C.POINTER(DsdAcousticConfig), C.c_float, i32, C.POINTER(DsdAcousticPlan)]
    lib.dsd_acoustic_start.argtypes = [vp, C.POINTER(DsdAcousticPlan), vp, vp, i32, i32, vp, vp]
    lib.dsd_acoustic_sample.argtypes = [vp, C.POINTER(DsdAcousticPlan), vp, vp, vp, i32, i32, C.c_uint32, vp, vp]
    lib.dsd_acoustic_set_lengths.argtypes = [vp, C.POINTER(C.c_int32), i32, vp]
    lib.dsd_acoustic_spk_mix.argtypes = [vp, C.POINTER(DsdSpkMixArgs), vp]
    lib.dsd_variance_spk_mix.argtypes = [vp, C.POINTER(DsdSpkMixArgs), vp]
    lib.dsd_vocode_seeded.argtypes = [C.POINTER(DsdVocodeSeededArgs), vp]
    lib.dsd_word_dur.argtypes = [i32, C.POINTER(DsdWordDurArgs), vp]
    lib.dsd_group_midi.argtypes = [i32, C.POINTER(DsdGroupMidiArgs), vp]
    lib.dsd_rhythm_align.argtypes = [i32, C.POINTER(DsdRhythmAlignArgs), vp]
    lib.dsd_variance_set_lengths.argtypes = [vp, C.POINTER(C.c_int32), i32, vp]
    lib.dsd_get_stats.argtypes = [vp, C.POINTER(DsdStats)]
    lib.dsd_kernel_timing.argtypes = [vp, i32]
    lib.dsd_set_precision.argtypes = [vp, i32]
    lib.dsd_kernel_timing_read.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(i64)]
    lib.dsd_kernel_timing_classes.argtypes = [vp, C.POINTER(DsdKernelTime), i32, C.POINTER(i32), C.POINTER(C.c_double)]
    lib.dsd_kernel_ledger.argtypes = [C.POINTER(DsdKernelLaunches), i32, C.POINTER(i32)]
    lib.dsd_kernel_ledger_reset.argtypes = []
    for name in EXPORTS:
        getattr(lib, name)
    if lib.dsd_api_version() != 10:
        raise NativeLibraryError("libdsdenoise.so API version mismatch")
    return lib


_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        _LIB = _load()
    return _LIB


def check(handle, rc, what):
    if rc == 0:
        return
    msg = lib().dsd_last_error(handle).decode("utf-8", "replace")
    raise NativeLibraryError(f"{what} failed ({rc}): {msg}")


def kernel_ledger():
    """The launch ledger (dsd_kernel_ledger): [(mangled host-stub symbol or None, kernel group, launches)], one per kernel
    instantiation the library can launch, in registry order."""
    n = C.c_int32(0)
    check(None, lib().dsd_kernel_ledger(None, 0, C.byref(n)), "dsd_kernel_ledger")
    rows = (DsdKernelLaunches * max(1, n.value))()
    check(None, lib().dsd_kernel_ledger(rows, n.value, C.byref(n)), "dsd_kernel_ledger")
    return [(r.symbol.decode() if r.symbol else None, int(r.group), int(r.launches)) for r in rows[:n.value]]


def kernel_ledger_reset():
    check(None, lib().dsd_kernel_ledger_reset(), "dsd_kernel_ledger_reset")


def load_state_dict(handle, sd):
    """Every tensor of `sd` (torch tensors or arrays, copied through host float32) into the handle, then finalize."""
    import numpy as np
    for name, v in sd.items():
        a = np.ascontiguousarray(v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v), dtype=np.float32)
        shape = (C.c_int64 * max(1, a.ndim))(*(a.shape or (1,)))
        check(handle, lib().dsd_load_weight(handle, name.encode(), a.ctypes.data_as(C.POINTER(C.c_float)), shape, a.ndim, 0),
              f"dsd_load_weight({name})")
    check(handle, lib().dsd_finalize_weights(handle), "dsd_finalize_weights")


def program_to_c(prog):
    """schedule.Program -> (DsdProgram, keepalive)."""
    n = len(prog.evals)
    arr = (DsdEval * max(n, 1))()
    for i, ev in enumerate(prog.evals):
        ce = arr[i]
        ce.x_buf = ev.x_buf
        ce.t = float(ev.t)
        if not (1 <= len(ev.outs) <= DSD_MAX_OUT):
            raise ValueError(f"eval {i}: {len(ev.outs)} outputs")
        ce.n_out = len(ev.outs)
        for o, (dst, terms) in enumerate(ev.outs):
            if not (1 <= len(terms) <= DSD_MAX_TERMS):
                raise ValueError(f"eval {i} out {o}: {len(terms)} terms")
            ce.out[o].dst = dst
            ce.out[o].n_terms = len(terms)
            for k, (src, coef) in enumerate(terms):
                ce.out[o].terms[k].src = src
                ce.out[o].terms[k].coef = float(coef)
    p = DsdProgram()
    p.n_bufs = prog.n_bufs
    p.result_buf = prog.result_buf
    p.n_evals = n
    p.n_noise = prog.n_noise
    p.evals = C.cast(arr, C.POINTER(DsdEval))
    return p, arr
