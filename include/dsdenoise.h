/*
 * libdsdenoise - MI355X-native (gfx950) diffusion denoiser for DiffSinger.
 *
 * C-ABI drop-in boundary for the ONE hot path of hrukalive/DiffSinger inference: the backbone
 * forward (WaveNet / LYNXNet) and the sampling loops that call it once per NFE.  Every entry
 * point replaces (is bound in place of) a reference Python interface, cited per function as
 * `path:line` into the reference tree.  Plain pointers and sizes only: no torch types cross
 * this boundary.  All device pointers are fp32, on the HIP device the handle was created for;
 * `stream` is a `hipStream_t` passed as `void*` (NULL = the null stream).
 *
 * Return value: 0 on success, a negative DSD_E* code on failure; nothing is thrown across the
 * ABI.  `dsd_last_error` returns a human-readable message for the last failure on a handle.
 * One `dsd_handle` type stands behind nine kinds of model (the DSD_* enum below); a call on a
 * kind it does not take returns DSD_ESTATE with "<call>: this handle is <what> (use <calls>)",
 * a NULL handle DSD_EINVAL.  INTEGRATION.md has the table of calls and kinds.
 *
 * Threading: like the reference modules (module-level `noise_list`/`bar`,
 * modules/core/ddpm.py:78,276,324) a handle is NOT re-entrant: calls on one handle are
 * serialised by the caller.  One handle per (model, device, process).
 */
#ifndef DSDENOISE_H_
#define DSDENOISE_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSD_API_VERSION 10

/* error codes */
#define DSD_OK 0
#define DSD_EINVAL (-1)   /* bad argument / shape / enum                        */
#define DSD_ESTATE (-2)   /* call order violated (weights missing, no cond ...) */
#define DSD_EHIP (-3)     /* a HIP runtime call failed                          */
#define DSD_ENOMEM (-4)   /* device allocation failed                           */
#define DSD_ENOTFOUND (-5) /* unknown weight name                                */
#define DSD_EIO (-6)      /* a path that cannot be opened or read (dsd_model_open) */

typedef struct dsd_handle dsd_handle;

/* modules/backbones/__init__.py:6-9  BACKBONES = {'wavenet': WaveNet, 'lynxnet': LYNXNet} */
enum { DSD_BACKBONE_WAVENET = 0, DSD_BACKBONE_LYNXNET = 1,
       /* modules/aux_decoder/__init__.py:7-9  AUX_DECODERS = {'convnext': ConvNeXtDecoder}: not a denoiser - the
          shallow-diffusion aux decoder that produces the loop's start point (see dsd_aux_decode) */
       DSD_AUX_CONVNEXT = 2,
       /* modules/fastspeech/acoustic_encoder.py:14  FastSpeech2Acoustic: the producer of `cond` (see dsd_encode);
          created with dsd_encoder_create, not dsd_create */
       DSD_ENC_FS2_ACOUSTIC = 3,
       /* modules/nsf_hifigan/models.py:207  Generator (NSF-HiFiGAN vocoder: mel + f0 -> waveform; see dsd_vocode);
          created with dsd_vocoder_create */
       DSD_VOC_NSF_HIFIGAN = 4,
       /* modules/fastspeech/tts_modules.py:353  FastSpeech2Encoder on caller-assembled embeddings (+ DurationPredictor /
          out_proj): the encoders of the variance model; created with dsd_token_encoder_create */
       DSD_ENC_FS2_TOKENS = 5,
       /* modules/nsf_hifigan/nvSTFT.py:26  STFT (waveform -> log-mel analysis, no weights; see dsd_mel_analyze);
          created with dsd_mel_create */
       DSD_MEL_ANALYSIS = 6,
       /* modules/pe/rmvpe/inference.py:14  RMVPE pitch extractor (E2E0 + MelSpectrogram + to_local_average_f0);
          created with dsd_rmvpe_create */
       DSD_PE_RMVPE = 7,
       /* modules/hnsep/vr/nets.py:72  CascadedNet (VR harmonic-noise separator, is_complex=True) and the variance curves
          built on it; created with dsd_hnsep_create */
       DSD_HNSEP_VR = 8 };
/* A model file has one more section kind, DSD_VARIANCE_TABLES = 10 (the variance model's embedding tables: not a handle,
   see dsd_variance_open).  9 is not assigned, and a model file reader refuses it as unknown.  DSD_ACOUSTIC_TABLES = 11 is
   the acoustic model's counterpart (see dsd_acoustic_open). */
/* modules/backbones/lynxnet.py:38-42  activation_classes */
enum { DSD_ACT_PRELU = 0, DSD_ACT_SILU = 1, DSD_ACT_RELU = 2 };

/*
 * Constructor arguments of the backbone, i.e. what
 *   build_backbone(out_dims, num_feats, backbone_type, backbone_args)   modules/backbones/__init__.py:12-18
 * forwards to WaveNet.__init__ (modules/backbones/wavenet.py:52) or
 * LYNXNet.__init__ (modules/backbones/lynxnet.py:91-92), plus hparams['hidden_size']
 * (wavenet.py:65, lynxnet.py:113).
 */
typedef struct dsd_config {
    int32_t struct_size;            /* sizeof(dsd_config), for forward compatibility        */
    int32_t backbone;               /* DSD_BACKBONE_*                                       */
    int32_t in_dims;                /* M: mel bins / repeat bins (`in_dims`)                */
    int32_t n_feats;                /* F: `n_feats`                                         */
    int32_t num_layers;             /* L                                                    */
    int32_t num_channels;           /* C                                                    */
    int32_t hidden_size;            /* H: encoder hidden size of `cond`                     */
    int32_t dilation_cycle_length;  /* WaveNet only                                         */
    int32_t expansion_factor;       /* LYNXNet only                                         */
    int32_t kernel_size;            /* LYNXNet: depthwise conv (odd); aux decoder: in/out conv */
    int32_t activation;             /* LYNXNet only: DSD_ACT_*                              */
    int32_t strong_cond;            /* LYNXNet only: 0/1                                    */
    int32_t device;                 /* HIP device ordinal                                   */
} dsd_config;

/* Replaces: BACKBONES[backbone_type](out_dims, num_feats, **kwargs)  (backbones/__init__.py:16-18). */
int dsd_create(const dsd_config* cfg, dsd_handle** out);
/*
 * dsd_create for every width the reference builds.  dsd_create itself returns DSD_EINVAL for a LYNXNet or a ConvNeXt aux
 * decoder whose num_channels is not a multiple of 32, and for a LYNXNet whose num_channels * expansion_factor is not; the
 * reference has neither rule.  Same struct, same handle, same calls afterwards; `num_channels` is the model's true width and
 * dsd_load_weight takes the reference's state_dict names and shapes at that width.
 *   LYNXNet (modules/backbones/lynxnet.py:90-126): every even num_channels >= 4 and every expansion_factor >= 1.  Odd widths
 *     and widths below 4 are DSD_EINVAL because the reference cannot build them either: SinusoidalPosEmb
 *     (modules/commons/common_layers.py:268-281) emits 2 * (C // 2) values into a Linear(C, 4C) and divides by C / 2 - 1 - the
 *     rule dsd_create applies to a WaveNet.  kernel_size stays odd and <= 63 (with an even one the reference's own residual
 *     add fails: padding = kernel_size // 2 gives T + 1 frames).
 *   ConvNeXt aux decoder (modules/aux_decoder/convnext.py:58-85): every num_channels >= 1.
 *   WaveNet, and every width dsd_create accepts: exactly what dsd_create does.
 * Cost: the network RUNS at the next multiple of 32, Cp = (num_channels + 31) / 32 * 32 (LYNXNet's inner width at
 * Cp * expansion_factor), with the extra channels exactly zero throughout and every LayerNorm taken over the true
 * num_channels.  Weight memory, workspace (dsd_get_stats) and time are those of a model of width Cp: a LYNXNet of 500 channels
 * costs what one of 512 does and takes the same kernels.
 */
int dsd_create_any_width(const dsd_config* cfg, dsd_handle** out);
void dsd_destroy(dsd_handle* h);
/* Message for the last failed call on `h` (h == NULL: last failed dsd_create / dsd_create_any_width).  Never NULL. */
const char* dsd_last_error(const dsd_handle* h);
int dsd_api_version(void);

/*
 * Replaces: nn.Module.load_state_dict for the backbone (utils/__init__.py:166-222 load_ckpt ->
 * strict load).  `name` is the reference state_dict key relative to the backbone, e.g.
 * "residual_layers.3.dilated_conv.weight" (wavenet.py:22-31,56-72; lynxnet.py:52-62,71-74,104-124);
 * `shape`/`ndim` must equal the reference parameter's shape.  `data` is read during the call
 * (host pointer if on_device == 0, device pointer otherwise).  One extra, non-parameter entry is
 * accepted: "diffusion_embedding.freqs" [C/2], the SinusoidalPosEmb frequency table
 * (common_layers.py:275-276); if it is not supplied it is computed in fp32 on the host.
 */
int dsd_load_weight(dsd_handle* h, const char* name, const float* data, const int64_t* shape,
                    int32_t ndim, int32_t on_device);
/* Strictness check (every parameter present) + re-layout into MFMA fragment order on the device. */
int dsd_finalize_weights(dsd_handle* h);

/*
 * Hoists ResidualBlock.conditioner_projection / LYNXNetResidualLayer.conditioner_projection
 * (wavenet.py:30,35; lynxnet.py:72,77-82) out of the denoise loop: they depend on `cond` only.
 * The reference's own ONNX exporter does the same hoist (utils/onnx_helper.py:267-349).
 * cond element (b, h, t) is read at cond[b*stride_b + h*stride_h + t*stride_t], so both the
 * backbone's [B,H,T] view (wavenet.py:75-81) and GaussianDiffusion.forward's [B,T,H] `condition`
 * (ddpm.py:353-357) can be passed without a transpose.  Also (re)sizes the workspace for (B, T).
 */
int dsd_prepare_cond(dsd_handle* h, const float* cond, int32_t B, int32_t T, int64_t stride_b,
                     int64_t stride_h, int64_t stride_t, void* stream);

/*
 * Replaces: WaveNet.forward / LYNXNet.forward(spec, diffusion_step, cond)
 * (wavenet.py:75-107, lynxnet.py:128-163) for the cond given to the last dsd_prepare_cond.
 * x, out: [B, F, M, T] contiguous device fp32 (out must not alias x: the reference does not
 * mutate its input either).  t: device fp32, t_len == B or 1 (a [1] step is broadcast,
 * reflow.py:135); integer steps are passed as their float value (common_layers.py:277).
 */
int dsd_denoise(dsd_handle* h, const float* x, const float* t, int32_t t_len, float* out, void* stream);

/*
 * Shallow-diffusion aux decoder (the step right before the loop: it produces the `src_spec` the loop starts
 * from).  A handle created with backbone == DSD_AUX_CONVNEXT takes
 *   in_dims = mel bins M (`out_dims`), n_feats = 1, hidden_size = H (`in_dims` of the decoder),
 *   num_channels / num_layers / kernel_size = ConvNeXtDecoder's keyword arguments
 * and the state_dict of ConvNeXtDecoder (modules/aux_decoder/convnext.py:58-76: inconv.*, conv.N.{gamma,
 * dwconv.*, norm.*, pwconv1.*, pwconv2.*}, outconv.*) through dsd_load_weight / dsd_finalize_weights.
 * Replaces: AuxDecoderAdaptor.forward(condition, infer)  (modules/aux_decoder/__init__.py:58-71) =
 * ConvNeXtDecoder.forward (convnext.py:78-85) + denorm_spec (:53-56).
 *   cond  element (b, h, t) at cond[b*stride_b + h*stride_h + t*stride_t]  ([B,T,H] `condition` or [B,H,T])
 *   out   [B, T, M] contiguous;  out = y * out_scale[m] + out_shift[m]   (NULL, NULL = raw decoder output)
 */
int dsd_aux_decode(dsd_handle* h, const float* cond, int32_t B, int32_t T, int64_t stride_b, int64_t stride_h,
                   int64_t stride_t, float* out, const float* out_scale, const float* out_shift, void* stream);

/*
 * FastSpeech2 acoustic encoder: phoneme tokens + durations + f0 -> `condition` [B, T, H], the tensor every entry
 * point above consumes.  Constructor arguments = what FastSpeech2Acoustic.__init__ reads from hparams
 * (modules/fastspeech/acoustic_encoder.py:15-63) in the reference fork's rotary-embedding configuration
 * (`use_pos_embed: true, use_rope: true`, configs/acoustic.yaml:66; `ffn_act: gelu`, configs/base.yaml:32).
 * Weights: the FastSpeech2Acoustic state_dict (`txt_embed.weight`, `dur_embed.*`, `encoder.layers.N.op.{layer_norm1,
 * self_attn.{in_proj,out_proj}.weight, self_attn.rotary_embed.freqs, layer_norm2, ffn.ffn_1, ffn.ffn_2}.*`,
 * `encoder.layer_norm.*`, `pitch_embed.*`, optional `lang_embed / spk_embed / variance_embeds.X / key_shift_embed /
 * speed_embed`) through dsd_load_weight / dsd_finalize_weights.
 */
#define DSD_EMBED_ENERGY 1u
#define DSD_EMBED_BREATHINESS 2u
#define DSD_EMBED_VOICING 4u
#define DSD_EMBED_TENSION 8u
#define DSD_EMBED_KEY_SHIFT 16u
#define DSD_EMBED_SPEED 32u

/* Positional information of a FastSpeech2Encoder (tts_modules.py:362-364,378-384,390-395) */
enum { DSD_POS_ROPE = 0,   /* use_pos_embed && use_rope: rotary embedding inside the attention (MultiheadSelfAttentionWithRoPE) */
       DSD_POS_REL = 1,    /* use_pos_embed && !use_rope && rel_pos: x * sqrt(H) + RelPositionalEncoding table
                              (espnet_positional_embedding.py:26-47,98-113), torch.nn.MultiheadAttention(bias=False);
                              weights `...self_attn.in_proj_weight` instead of `in_proj.weight` + `rotary_embed.freqs`, plus
                              `encoder.embed_positions.div_term` [H/2] = exp(arange(0, H, 2) * -(ln 10000 / H)) */
       DSD_POS_NONE = 2,   /* !use_pos_embed: no positions; attention and weight names as DSD_POS_REL */
       DSD_POS_SIN = 3 };  /* use_pos_embed && !use_rope && !rel_pos: x + SinusoidalPositionalEmbedding(positions)
                              (common_layers.py:44-99; positions count the non-padding tokens from 1, utils/__init__.py:118-128);
                              attention and weight names as DSD_POS_REL, plus `encoder.embed_positions.freqs` [H/2] =
                              exp(arange(H/2) * -(ln 10000 / (H/2 - 1))); the checkpoint's `encoder.embed_positions._float_tensor`
                              buffer is accepted and ignored */

/* TransformerFFNLayer's activation between ffn_1 and ffn_2 (common_layers.py:126-136): GELU (exact erf), ReLU, SiLU
   ('swish'), or SwiGLU - ffn_1 then has 2 * 4H output channels, `out * silu(gate)` with out = the first half
   (common_layers.py:107-117) */
enum { DSD_FFN_GELU = 0, DSD_FFN_RELU = 1, DSD_FFN_SWISH = 2, DSD_FFN_SWIGLU = 3 };

typedef struct dsd_encoder_config {
    int32_t struct_size;      /* sizeof(dsd_encoder_config)                                          */
    int32_t vocab_size;       /* FastSpeech2Acoustic(vocab_size)                                     */
    int32_t hidden_size;      /* hparams['hidden_size']                                              */
    int32_t enc_layers;       /* hparams['enc_layers']                                               */
    int32_t num_heads;        /* hparams['num_heads']                                                */
    int32_t ffn_kernel_size;  /* hparams['enc_ffn_kernel_size'] (odd)                                */
    int32_t num_spk;          /* hparams['num_spk'] if use_spk_id else 0                             */
    int32_t num_lang;         /* hparams['num_lang'] if use_lang_id else 0 (table has num_lang + 1 rows) */
    uint32_t embed_flags;     /* DSD_EMBED_*: use_energy_embed ... use_speed_embed                   */
    int32_t pos_mode;         /* DSD_POS_*                                                           */
    int32_t device;
    int32_t ffn_act;          /* DSD_FFN_*: hparams['ffn_act'] (TransformerFFNLayer, common_layers.py:120-151) */
} dsd_encoder_config;

/* Optional inputs of FastSpeech2Acoustic.forward (acoustic_encoder.py:82-88); NULL = not given.  All device pointers. */
typedef struct dsd_encode_extras {
    const int64_t* languages;      /* [B, T_txt]   (use_lang_id)                                     */
    const int64_t* spk_embed_id;   /* [B]          (use_spk_id, when spk_mix_embed is NULL)          */
    const float* spk_mix_embed;    /* element (b,t,h) at [b*bstride + t*tstride + h] (use_spk_id)    */
    int64_t spk_mix_bstride, spk_mix_tstride;
    const float* key_shift;        /* [B, T] each                                                    */
    const float* speed;
    const float* energy;
    const float* breathiness;
    const float* voicing;
    const float* tension;
} dsd_encode_extras;

int dsd_encoder_create(const dsd_encoder_config* cfg, dsd_handle** out);
/*
 * Replaces: FastSpeech2Acoustic.forward(txt_tokens, mel2ph, f0, key_shift, speed, spk_embed_id, languages, **kwargs)
 * (acoustic_encoder.py:82-118).  txt_tokens [B, T_txt] int64 (0 = padding), mel2ph [B, T] int64 (1-based token
 * index per frame, 0 = padding frame), f0 [B, T] Hz; cond_out [B, T, H] contiguous.
 */
int dsd_encode(dsd_handle* h, const int64_t* txt_tokens, const int64_t* mel2ph, const float* f0, int32_t B,
               int32_t T_txt, int32_t T, const dsd_encode_extras* extras, float* cond_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Variance model (modules/toplevel.py:125-309, BASELINE config 5): the pieces between the tokens and the pitch /
 * multi-variance denoisers, which are ordinary dsd_create handles.
 *
 * A "token encoder" is the FastSpeech2Encoder (tts_modules.py:353-428, rotary configuration) on embeddings the caller
 * assembled (dsd_cond_assemble below), with the two heads the variance model hangs on it:
 *   - FastSpeech2Variance (variance_encoder.py:14-99): encoder + DurationPredictor (tts_modules.py:53-134)
 *   - MelodyEncoder (variance_encoder.py:102-148): encoder + out_proj Linear(hidden, out_dims)
 * Weights: `encoder.layers.N.op.*`, `encoder.layer_norm.*` as for dsd_encoder_create; `out_proj.{weight,bias}` when
 * out_dims > 0; `dur_predictor.conv.N.1.{weight,bias}` (Conv1d), `dur_predictor.conv.N.3.{weight,bias}` (LayerNorm over
 * channels, eps 1e-12) and `dur_predictor.linear.{weight,bias}` when dur_layers > 0.
 */
typedef struct dsd_token_encoder_config {
    int32_t struct_size;      /* sizeof(dsd_token_encoder_config)                                     */
    int32_t hidden_size;      /* hparams['hidden_size'] (melody encoder: melody_encoder_args.hidden_size) */
    int32_t enc_layers;
    int32_t num_heads;
    int32_t ffn_kernel_size;  /* odd                                                                  */
    int32_t out_dims;         /* MelodyEncoder.out_proj output size; 0 = no projection                */
    int32_t dur_layers;       /* dur_prediction_args.num_layers; 0 = no duration predictor            */
    int32_t dur_chans;        /* dur_prediction_args.hidden_size                                      */
    int32_t dur_kernel_size;  /* dur_prediction_args.kernel_size (odd)                                */
    float dur_offset;         /* dur_prediction_args.log_offset                                       */
    int32_t pos_mode;         /* DSD_POS_*                                                            */
    int32_t device;
    int32_t ffn_act;          /* DSD_FFN_*                                                            */
} dsd_token_encoder_config;

int dsd_token_encoder_create(const dsd_token_encoder_config* cfg, dsd_handle** out);
/*
 * Replaces: FastSpeech2Encoder.forward(main_embed, extra_embed, padding_mask) (tts_modules.py:400-428) [+ out_proj,
 * variance_encoder.py:147].  embed [B, L, H] = embed_scale * main_embed + extra_embed (tts_modules.py:387-389; no additive
 * positions in the rotary configuration; DSD_POS_REL adds them inside), padding_mask [B, L] bytes (non-zero = padding), enc_out [B, L, H or out_dims].
 */
int dsd_token_encode(dsd_handle* h, const float* embed, const uint8_t* padding_mask, int32_t B, int32_t L,
                     float* enc_out, void* stream);
/*
 * Replaces: DurationPredictor.forward(xs, x_masks, infer=True) (tts_modules.py:112-134): dur_cond [B, L, H] ->
 * dur_out [B, L] = clamp(exp(linear(...)) - offset, min 0), zero at padding.
 */
int dsd_predict_dur(dsd_handle* h, const float* dur_cond, const uint8_t* padding_mask, int32_t B, int32_t L,
                    float* dur_out, void* stream);

/*
 * Gather-and-add assembly of a [B, T, H] tensor: every embedding sum of the variance model
 * (variance_encoder.py:70-96,137-146; toplevel.py:233-236,246-276,289-298) is an instance of
 *   out[b,t,:] = sum_g scale_g * rowscale_g[b,t] * table_g[b*batch_stride_g + idx_g[b,t], :]
 *              + sum_k s_k[b,t] * v_k[:]
 * - an nn.Embedding lookup is a gather with batch_stride 0; `torch.gather(F.pad(x, [0,0,1,0]), 1, mel2ph)` is a gather
 *   from x with idx - 1 (`idx_offset` = -1; a negative row reads as zeros);
 * - Linear(1, H)(x) is the two terms (s = x, v = weight[:, 0]) and (s = 1, v = bias); s = NULL means 1.
 * Terms are added in the order given (gathers first).  No handle: nothing here has weights of its own.
 */
#define DSD_ASSEMBLE_MAX_GATHER 4
#define DSD_ASSEMBLE_MAX_TERMS 16
typedef struct dsd_assemble_args {
    int32_t struct_size;      /* sizeof(dsd_assemble_args) */
    int32_t device;
    int32_t B, T, H;
    int32_t n_gather, n_terms;
    struct {
        const float* table;       /* [rows, H] (batch_stride 0) or [B, rows, H]                     */
        int64_t batch_stride;     /* in elements                                                    */
        int64_t rows;             /* rows per batch item; an index outside [0, rows) reads as zeros */
        const int64_t* idx;       /* [B, T]                                                         */
        int64_t idx_offset;       /* added to every index                                           */
        float scale;
        const float* row_scale;   /* [B, T] or NULL                                                 */
    } gather[DSD_ASSEMBLE_MAX_GATHER];
    struct {
        const float* s;           /* [B, T] or NULL (= 1)                                           */
        const float* v;           /* [H]                                                            */
    } term[DSD_ASSEMBLE_MAX_TERMS];
} dsd_assemble_args;

int dsd_cond_assemble(const dsd_assemble_args* args, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Duration-to-frame stages of the deployment twins (deployment/modules/): what an editor's staged calls do between the
 * token-level encoders and a frame-level condition.  Both entries are handle-free like dsd_cond_assemble: `device` is
 * the HIP device index, nothing has weights, and neither keeps device memory.
 * ------------------------------------------------------------------------------------------ */
/*
 * Replaces: LengthRegulator.forward(dur) (deployment/modules/fastspeech2.py:31-40).
 *   dur      [B, L] int64 on the device, 1 <= L <= 2048 (the encoders' token limit)
 *   mel2x    [B, T] int64 on the device: frame p of item b holds i + 1 for the token i with
 *            cumsum(dur)[i - 1] <= p < cumsum(dur)[i], and 0 at or past the item's total (the reference's masked sum adds
 *            nothing there).  A zero duration owns no frame and is skipped, as in the reference.
 * T is the caller's: the reference sizes its output by the largest total of the batch, which is a device read-back; pass
 * that total to get its shape, or the frame count of the curves the result will be used with.  Durations past T are cut.
 * B < 1, L outside [1, 2048] or T < 1 is DSD_EINVAL.  The durations themselves are not read back: non-negative values are
 * the caller's contract (a negative one counts as 0 here, where the reference would shift every later token).
 */
int dsd_length_regulate(int32_t device, const int64_t* dur, int32_t B, int32_t L, int32_t T, int64_t* mel2x, void* stream);
/*
 * Replaces: the curve part of DiffSingerVarianceONNX.forward_pitch_preprocess (deployment/modules/toplevel.py:251-258)
 * with the smoothing operator of build_smooth_op (:179-194):
 *   frame_midi[t] = pad(note_midi, [1, 0])[mel2note[t]]            forward_mel2x_gather with x_dim=None (:214-222)
 *   base[t]       = sum_k weights[k] * frame_midi[clamp(t - (K - 1) / 2 + k, 0, len - 1)]
 *                   Conv1d(1, 1, K, bias=False, padding='same', padding_mode='replicate'): (K - 1) / 2 frames of padding
 *                   in front and the rest behind, so an even K looks one frame further ahead than back
 *   blend[t]      = base[t] * retake[t] + pitch[t] * !retake[t]     the base pitch without a melody encoder (:257)
 *   delta[t]      = (pitch[t] - base[t]) * !retake[t]               the delta pitch with one (:254); its base pitch is base
 * All three outputs are always written; the caller picks the form its model uses.
 *   note_midi [B, N] fp32, mel2note [B, T] int64 (an index outside [1, N] reads 0), pitch [B, T] fp32, retake [B, T] bytes
 *   (non-zero = retake); base_out, blend_out, delta_out [B, T] fp32; all on the device
 *   lengths   HOST array of B frame counts in [0, T], or NULL (every item has T frames): item b replicates at its own
 *             last frame, nothing at or past lengths[b] is read, and its outputs there are 0
 *   weights   HOST array of the K taps, 1 <= K <= 255.  The reference's are sin(pi * linspace(0, 1, K)) in fp32 divided
 *             by their fp32 sum, K = round(midi_smooth_width * audio_sample_rate / hop_size); they travel in the launch's
 *             arguments, so any K costs the same and nothing is cached.  (K = 1 makes that 0 / 0: the reference's
 *             operator is NaN there, and so is this one when given the same tap.)
 */
int dsd_frame_curve(int32_t device, const float* note_midi, const int64_t* mel2note, const float* pitch,
                    const uint8_t* retake, int32_t B, int32_t N, int32_t T, const int32_t* lengths, const float* weights,
                    int32_t K, float* base_out, float* blend_out, float* delta_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * The segment front end: what stands between a `.ds` segment's text fields and the calls above.  Handle-free.
 * ------------------------------------------------------------------------------------------ */
/*
 * Replaces: ph_acc = round(cumsum(ph_dur) / timestep + 0.5); durations = diff(ph_acc, prepend 0)
 * (inference/ds_acoustic.py:102-104, inference/ds_variance.py:151,179), as torch evaluates it ON THE CPU, on any host:
 *   acc      a double running sum of the fp32 inputs (torch's CPU cumsum accumulates fp32 in double)
 *   c_i      = (float)acc
 *   b_i      = rintf(c_i / (float)timestep + 0.5f)      an fp32 divide, half to even
 *   frames_i = b_i - b_{i-1}, b_{-1} = 0;  *total_out = b_{n-1}
 * Host arithmetic only: no device is touched, so the caller knows the frame count T of a segment without a read-back.
 *   seconds     HOST array of n durations, each finite and >= 0
 *   frames_out  HOST array of n frame counts (a zero duration may give 0)
 * DSD_EINVAL for a NULL pointer, n < 1, a timestep that is not finite or not positive, an input that is not finite or is
 * negative, or a boundary that does not fit int32 frames.
 */
int dsd_seconds_to_frames(const float* seconds, int32_t n, double timestep, int64_t* frames_out, int64_t* total_out);
/*
 * Replaces: resample_align_curve (utils/infer_utils.py:41-53) and what the inference front ends do to its result, for up
 * to DSD_CURVE_MAX curves in one launch (two when a DSD_CURVE_PITCH curve is among them).  The descriptors are a HOST
 * array that travels in the launch arguments: no device memory is allocated, nothing is synchronised, and the call can
 * be captured into a hipGraph.
 *
 * Resampling, bit for bit numpy's (np.interp over original_timestep * arange(n) at arange(0, (n - 1) * original_timestep,
 * target_timestep)), all in IEEE double without contraction:
 *   count = ceil(((n_points - 1) * src_step) / dst_step)
 *   frame k < min(count, length):  x = k * dst_step;  j = the largest index with src_step * j <= x
 *       j >= n_points - 1     -> p[n_points - 1]
 *       src_step * j == x     -> p[j]
 *       otherwise             -> ((p[j + 1] - p[j]) / (src_step * (j + 1) - src_step * j)) * (x - src_step * j) + p[j]
 *     rounded to fp32;  frames count .. length hold the last computed value;  out[length .. pad_to) = 0
 * then, on the fp32 value v:
 *   DSD_CURVE_PLAIN    nothing
 *   DSD_CURVE_CLIP     min(max(v, lo), hi)                                      velocity (ds_acoustic.py:169-176)
 *   DSD_CURVE_GENDER   v * (v >= 0 ? hi : |lo|) in double, rounded to fp32, then clipped to [lo, hi]: the key shift of a
 *                      gender curve (ds_acoustic.py:154-159), lo <= 0 <= hi the model's key-shift range
 *   DSD_CURVE_PITCH    an f0 curve in Hz to MIDI pitch with the unvoiced frames filled (ds_variance.py:244-249 through
 *                      interp_f0, utils/pitch_utils.py:13-20, and librosa's hz_to_midi): uv = (v == 0); an unvoiced frame
 *                      takes the linear interpolation of log2 f0 between the nearest voiced frames on either side, the
 *                      nearest voiced value at the ends, -inf when no frame is voiced; out = 12 * (log2 f - log2 440) + 69.
 *                      Evaluated in double, rounded to fp32 where the host path stores fp32 (log2 f0 and the filled f0) and
 *                      at the output: within a few fp32 roundings of the host path, not bit-equal to it.  uv_out (bytes,
 *                      1 = unvoiced) is written when given; out[length .. pad_to) = 0 and uv_out there = 0.
 * The points are finite by the caller's contract; they are not read back.  DSD_EINVAL before the device is touched, the
 * message naming the curve and the field: a NULL curves, n_curves outside [1, DSD_CURVE_MAX], a NULL points or out,
 * n_points < 2 (the reference itself fails on one point), length < 1, pad_to < length, a step that is not finite or not
 * positive, an unknown op, CLIP bounds with lo > hi or a NaN, a GENDER range without lo <= 0 <= hi, a uv_out on a curve
 * that is not DSD_CURVE_PITCH.
 */
#define DSD_CURVE_MAX 32
#define DSD_CURVE_CHUNK 256     /* frames a workgroup takes at a time (a PITCH curve's fill carries across them) */
enum { DSD_CURVE_PLAIN = 0, DSD_CURVE_CLIP = 1, DSD_CURVE_GENDER = 2, DSD_CURVE_PITCH = 3 };
typedef struct dsd_curve {
    const float* points;        /* device, n_points fp32, finite */
    float* out;                 /* device, pad_to floats */
    uint8_t* uv_out;            /* DSD_CURVE_PITCH: device, pad_to bytes, or NULL */
    double src_step, dst_step;  /* seconds, > 0 */
    int32_t n_points;           /* >= 2 */
    int32_t length;             /* align_length, >= 1 */
    int32_t pad_to;             /* >= length: the row of a zero-padded batch */
    int32_t op;                 /* DSD_CURVE_* */
    float lo, hi;               /* CLIP: bounds; GENDER: the key-shift range */
} dsd_curve;
int dsd_curve_resample(int32_t device, const dsd_curve* curves, int32_t n_curves, void* stream);

/* ------------------------------------------------------------------------------------------
 * Seeded draws on the device: the x_T and step noise of the samplers, the vocoder's phases and noise.  Handle-free:
 * `device` is the HIP device index.  Element (row, col) of a draw is a pure function of (seed, domain, stream, row, col):
 * it does not depend on B, on padding, on the launch shape or on what the process drew before, so a ragged batch draws
 * for item b exactly what a lone call with seeds[b] draws, and a C caller draws what the Python side draws.
 *
 * The generator:
 *   block     Philox4x32-10 (Salmon et al., Random123): multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 /
 *             0xBB67AE85.  Known answers (counter; key -> output):
 *               0 0 0 0; 0 0                                          -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8
 *               ffffffff x 4; ffffffff x 2                            -> 408f276d 41c83b0e a20bc7c6 6d5451fd
 *               243f6a88 85a308d3 13198a2e 03707344; a4093822 299f31d0 -> d16cfe09 94fdcceb 5001e420 24126ea1
 *   address   key = (seed & 0xffffffff, seed >> 32) of the item's 64-bit seed; counter = (col >> 2, row, stream, domain);
 *             the four output words w[0..3] serve the columns 4 * (col >> 2) + 0..3
 *   uniform   u(w) = ((w >> 9) + 0.5) * 2^-23: exact in fp32, strictly inside (0, 1).  DSD_NOISE_UNIFORM: column c is
 *             u(w[c & 3]).
 *   normal    Box-Muller on word pairs in fp32 with the precise logf / sqrtf / sincosf: r = sqrt(-2 log u(w0)),
 *             theta = 2 pi u(w1), z0 = r cos(theta), z1 = r sin(theta); (w2, w3) gives z2, z3.  |z| <= 5.7681.
 *   domain    a caller-chosen 32-bit tag that keeps the tensors drawn under one seed apart (the Python side uses 1 = x_T,
 *             2 = sampler step noise, 3 = vocoder source noise, 4 = vocoder pre-noise, 5 = vocoder initial phases,
 *             6 = pitch x_T, 7 = variance x_T, 8 = the scoring step's t, 9 = the scoring step's noise,
 *             10 / 11 = the same two for the variance predictor)
 *   stream    numbers the tensors of a sequence: the k-th step noise of a sampler run
 *
 *   out = src_scale * src + scale * eps   (src == NULL: out = scale * eps), each product and the sum rounded to fp32 on
 *   its own.  With src this is the start mix of shallow diffusion / reflow in the same launch; out may be src.
 *
 * The seeds travel in the launch arguments: the call does not synchronise, allocates nothing and can be captured into a
 * hipGraph (the seeds are then part of the captured launch).  A 16-byte store per four columns when cols % 4 == 0 and
 * out (and src) are 16-byte aligned, scalar stores otherwise.  DSD_EINVAL before any device work for a NULL spec, out or
 * seeds, a wrong struct_size, an unknown kind, n, B, rows or cols below 1, or more than 2^31 - 1 elements.
 * ------------------------------------------------------------------------------------------ */
#define DSD_DOMAIN_X_T 1         /* the domains above that a renderer draws under, by name                 */
#define DSD_DOMAIN_STEP 2
#define DSD_DOMAIN_VOC_SOURCE 3
#define DSD_DOMAIN_VOC_PRE 4
#define DSD_DOMAIN_VOC_PHASE 5
#define DSD_NOISE_NORMAL 0
#define DSD_NOISE_UNIFORM 1
typedef struct dsd_noise_spec {
    int32_t struct_size;
    int32_t kind;            /* DSD_NOISE_NORMAL or DSD_NOISE_UNIFORM                          */
    uint32_t domain;
    int32_t first_stream;    /* out[k] is stream first_stream + k                              */
    int32_t n, B, rows, cols;/* out is dense [n][B][rows][cols]                                */
    const uint64_t* seeds;   /* HOST, B values: one seed per item                              */
    float scale;
    const float* src;        /* device, [n][B][rows][cols] dense, or NULL                      */
    float src_scale;
} dsd_noise_spec;
int dsd_noise_fill(int32_t device, const dsd_noise_spec* spec, float* out, void* stream);

/*
 * NSF-HiFiGAN generator (the step after the loop: mel -> waveform).  The constructor arguments are the fields of the
 * checkpoint's config.json that Generator.__init__ reads (modules/nsf_hifigan/models.py:207-260), `mini_nsf: false`.
 * Weights: the Generator state_dict in its inference form, i.e. after remove_weight_norm() (models.py:292-302):
 * `m_source.l_linear.*`, `noise_convs.N.*`, `conv_pre.*`, `ups.N.*` ([C_in, C_out, K] as ConvTranspose1d stores it),
 * `resblocks.N.convs1.M.* / convs2.M.*` (ResBlock1) or `resblocks.N.convs.M.*` (ResBlock2), `conv_post.*`;
 * with mini_nsf: `source_conv.*` instead of `m_source.*` / `noise_convs.*`.
 * Accepted (DSD_EINVAL otherwise, with the layer named; what is accepted runs for every (B, T) - DESIGN.md 4d, "Vocoder
 * configurations"): 1..8 upsampling stages of any rate u >= 1 with a kernel in [u, 8u], kernel - u even; 1..8 residual
 * kernels, odd and <= 15, with 1..4 dilations each and dilation * (kernel / 2) <= 48; harmonic_num 0..15;
 * upsample_initial_channel divisible by 2^n_ups; every convolution's resident input rows within 160 KiB of LDS per 32-frame
 * tile (num_mels <= 848, upsample_initial_channel >> i <= 848 at stage i, a residual stage of at most 272 channels at a reach
 * of 48 frames, 352 at k 11 / dilation 5); without mini_nsf and with two or more stages an even last rate (the reference's
 * noise_convs give one frame too few for an odd one, models.py:239-245) and prod(upsample_rates[i+1:]) <= 2409.
 */
#define DSD_VOC_MAX_UPS 8
#define DSD_VOC_MAX_KERNELS 8
#define DSD_VOC_MAX_DILS 4
typedef struct dsd_vocoder_config {
    int32_t struct_size;
    int32_t num_mels;
    int32_t sampling_rate;
    int32_t upsample_initial_channel;
    int32_t n_ups;
    int32_t upsample_rates[DSD_VOC_MAX_UPS];
    int32_t upsample_kernel_sizes[DSD_VOC_MAX_UPS];
    int32_t resblock;                                  /* 1 = ResBlock1, 2 = ResBlock2 */
    int32_t n_kernels;
    int32_t resblock_kernel_sizes[DSD_VOC_MAX_KERNELS];
    int32_t n_dilations[DSD_VOC_MAX_KERNELS];
    int32_t resblock_dilation_sizes[DSD_VOC_MAX_KERNELS][DSD_VOC_MAX_DILS];
    int32_t harmonic_num;                              /* SourceModuleHnNSF(harmonic_num=8), models.py:221-224 */
    int32_t mini_nsf;                                  /* h.mini_nsf (models.py:212-225): 1 = fastsinegen source, added
                                                          once through `source_conv` after the second upsampling */
    float noise_sigma;                                 /* h.noise_sigma (models.py:213,272-273): > 0 adds
                                                          noise_sigma * pre_noise after conv_pre; 0 = off */
    int32_t device;
} dsd_vocoder_config;

int dsd_vocoder_create(const dsd_vocoder_config* cfg, dsd_handle** out);
/*
 * Replaces: Generator.forward(x, f0)  (models.py:262-290) with the two random draws of SineGen made explicit:
 *   mel      element (b, m, t) at mel[b*stride_b + m*stride_m + t*stride_t]: natural-log mel, [B, num_mels, T] view
 *            (the wrapper's 2.30259 * log10-mel, vocoders/nsf_hifigan.py:59-64, is the caller's)
 *   f0       [B, T] Hz, 0 = unvoiced
 *   rand_ini [harmonic_num + 1] uniform [0,1) initial phases (torch.rand, models.py:145; element 0 is ignored)
 *   noise    [B, T * prod(upsample_rates), harmonic_num + 1] standard normals (torch.randn_like, models.py:165)
 *            (both may be NULL for a mini_nsf generator: its source is deterministic)
 *   pre_noise [B, upsample_initial_channel, T] standard normals (torch.randn_like(x), models.py:273); required when the
 *            configuration's noise_sigma > 0, ignored (may be NULL) otherwise
 *   wav_out  [B, T * prod(upsample_rates)]
 */
int dsd_vocode(dsd_handle* h, const float* mel, int32_t B, int32_t T, int64_t stride_b, int64_t stride_m,
               int64_t stride_t, const float* f0, const float* rand_ini, const float* noise, const float* pre_noise,
               float* wav_out, void* stream);
/*
 * Ragged vocoder batch: dsd_vocode over B segments zero-padded to T frames, where item b holds lengths[b] valid frames and
 * comes out as if it had been vocoded alone at T = lengths[b] with its own draws (the frames past an item's end - at every
 * rate, lengths[b] * prod(upsample_rates[:i]) after i upsamplings - are the zero padding of every convolution and of the
 * source, and the tiles that hold only such frames are not computed).  lengths: HOST array of B values, 1 <= lengths[b] <= T.
 *   rand_ini  [B][harmonic_num + 1]: one row per item (a lone call draws its own)
 *   noise     [B, T * prod(upsample_rates), harmonic_num + 1]: item b's first lengths[b] * prod(upsample_rates) rows are used
 *   pre_noise [B, upsample_initial_channel, T]: item b's [:, :lengths[b]] is used
 * The null / mini_nsf / noise_sigma rules are dsd_vocode's; samples of wav_out at or past lengths[b] * prod(upsample_rates)
 * are unspecified.  dsd_set_lengths does not apply to vocoder handles: this call takes the lengths explicitly.
 */
int dsd_vocode_ragged(dsd_handle* h, const float* mel, int32_t B, int32_t T, int64_t stride_b, int64_t stride_m,
                      int64_t stride_t, const int32_t* lengths, const float* f0, const float* rand_ini, const float* noise,
                      const float* pre_noise, float* wav_out, void* stream);
/*
 * The vocoder with its draws made where they are used.  Replaces: the three dsd_noise_fill calls of Generator._seeded_draws
 * (diffsinger_amd/vocoder.py) plus dsd_vocode / dsd_vocode_ragged, i.e. torch.rand / torch.randn_like of models.py:145, 165
 * and 273 under per-item seeds.  The result is bit for bit the waveform dsd_vocode_ragged (lengths != NULL) or dsd_vocode
 * (lengths == NULL) gives at the same (B, T, lengths) when its inputs come from dsd_noise_fill at stream 0, scale 1:
 *   rand_ini   DSD_NOISE_UNIFORM, DSD_DOMAIN_VOC_PHASE, rows 1, cols harmonic_num + 1: a ragged call draws one row per item
 *              from seeds[b], a dense call one shared row from seeds[0] (as the reference draws one per call)
 *   noise      DSD_NOISE_NORMAL, DSD_DOMAIN_VOC_SOURCE, rows T * prod(upsample_rates), cols harmonic_num + 1, seeds[b]
 *   pre_noise  DSD_NOISE_NORMAL, DSD_DOMAIN_VOC_PRE, rows upsample_initial_channel, cols T, seeds[b]; only with noise_sigma > 0
 * but neither noise nor pre_noise is ever written: the source kernel draws its sample row's Philox blocks and the pre-noise
 * kernel four frames per block, and the only draw kept is rand_ini, [B, harmonic_num + 1] in the handle's workspace.  An
 * element of a draw does not depend on T or B, so item b of a ragged call comes out as it does alone with seeds[b].
 * The seeds travel in the launch arguments, 64 items per launch: the call reads nothing back and can be captured after a
 * first call at the same sizes.  The handle sits inside the struct; the entry check and the errors are dsd_vocode's and
 * land on that handle (a handle of another kind: DSD_ESTATE).  DSD_EINVAL: NULL args, a wrong struct_size (both without a
 * device), NULL vocoder, mel, f0 or wav_out, B < 1, T < 1, a length outside [1, T], both strides non-unit, and NULL seeds
 * unless the generator draws nothing (mini_nsf with noise_sigma == 0).
 */
typedef struct dsd_vocode_seeded_args {
    int32_t struct_size;
    int32_t B, T;
    dsd_handle* vocoder;
    const float* mel;          /* as dsd_vocode's, with its strides                                             */
    int64_t stride_b, stride_m, stride_t;
    const int32_t* lengths;    /* HOST [B] in [1, T], or NULL for a dense batch                                 */
    const float* f0;           /* [B, T]                                                                        */
    const uint64_t* seeds;     /* HOST [B]; may be NULL only for a generator that draws nothing                 */
    float* wav_out;            /* [B, T * prod(upsample_rates)]                                                 */
} dsd_vocode_seeded_args;
int dsd_vocode_seeded(const dsd_vocode_seeded_args* args, void* stream);

/*
 * Ragged batches.  The reference runs one utterance per call (inference/ds_acoustic.py:214-271), because padding a batch
 * changes results near the end of the shorter items: frames beyond an item's end are not zero after the first layer and
 * leak into valid frames through every convolution along time.  With per-item lengths the library treats frames
 * t >= lengths[b] of item b as the convolutions' zero padding - in the dilated convolutions of the WaveNet, the depthwise
 * convolution of LYNXNet and the ConvNeXt aux decoder - so item b of a padded batch comes out as if it had been run alone
 * at T = lengths[b] (outputs at its padded frames are unspecified), and several segments of a project can share one
 * launch.  lengths: HOST array of B values (copied, stream-ordered); applies to the following dsd_prepare_cond / dsd_denoise
 * / dsd_sample / dsd_aux_decode calls at batch size B until changed; NULL restores dense batches.  WaveNet, LYNXNet and
 * aux-decoder handles take the call; every other kind answers DSD_ESTATE (a vocoder takes dsd_vocode_ragged, the analysis
 * calls take their lengths as an argument).
 */
int dsd_set_lengths(dsd_handle* h, const int32_t* lengths, int32_t B, void* stream);

/* ------------------------------------------------------------------------------------------
 * Mel analysis: waveform -> natural-log mel, the analysis front end the reference pairs with its vocoder (resynthesis
 * inference/val_nsf_hifigan.py:65, the binarizer's mel preprocessing/acoustic_binarizer.py:103 through get_mel_torch
 * utils/binarizer_utils.py:13-26, key-shift / speed augmentation augmentation/spec_stretch.py:31).  The output is what
 * dsd_vocode takes.  A mel handle has no weights: every other entry point returns DSD_ESTATE on it, and the mel entry
 * points return DSD_ESTATE on any other handle.
 * ------------------------------------------------------------------------------------------ */
/* STFT.__init__(sr, n_mels, n_fft, win_size, hop_length, fmin, fmax, clip_val)  (nvSTFT.py:27-48) */
typedef struct dsd_mel_config {
    int32_t struct_size;      /* sizeof(dsd_mel_config)                                      */
    int32_t sampling_rate;    /* sr                                                          */
    int32_t n_fft;
    int32_t win_size;         /* <= n_fft                                                    */
    int32_t hop_size;         /* hop_length                                                  */
    int32_t num_mels;         /* n_mels                                                      */
    double fmin, fmax;        /* Hz, 0 <= fmin < fmax                                        */
    double clip_val;          /* dynamic_range_compression_torch's clamp (nvSTFT.py:19-20)   */
    int32_t device;
} dsd_mel_config;

int dsd_mel_create(const dsd_mel_config* cfg, dsd_handle** out);
/*
 * Replaces: librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax) as nvSTFT.py:47-48 calls it: Slaney mel scale, Slaney area
 * normalisation, float32 weights (the library's one definition of the filterbank).  Host only, no device needed.
 * out: [num_mels][n_fft / 2 + 1] host floats.
 */
int dsd_mel_filterbank(const dsd_mel_config* cfg, float* out);
/*
 * Frame count of STFT.get_mel(y, keyshift, speed, center=False) on n_samples samples (nvSTFT.py:52-75):
 *   N' = round(n_fft 2^(keyshift/12)), W' = round(win_size 2^(keyshift/12)), H' = round(hop_size speed) (ties to even),
 *   reflect pads (W'-H')//2 and (W'-H'+1)//2 (floor division: negative pads crop),  T = 1 + (L + pads - N') // H'.
 * Returns T >= 1, or DSD_EINVAL where torch raises (a reflect pad >= n_samples, a padded signal shorter than N') or the
 * configuration / keyshift / speed is invalid.  Host only.
 */
int64_t dsd_mel_num_frames(const dsd_mel_config* cfg, int64_t n_samples, double keyshift, double speed);
/*
 * Replaces: STFT.get_mel(y, keyshift, speed, center=False)  (nvSTFT.py:50-87): reflect pad, torch.stft with the periodic
 * Hann window centred in the N'-sample frame, |X|, with keyshift != 0 the bins zero-padded / truncated to n_fft/2 + 1 and
 * scaled by win_size / W', the mel projection, log(clamp(., clip_val)).
 *   wav      item b's sample s at wav[b * wav_stride_b + s], s < n_samples (device fp32)
 *   lengths  HOST array of B sample counts (1 <= lengths[b] <= n_samples) or NULL (every item n_samples long).  Item b is
 *            computed exactly as a lone call on its own lengths[b] samples: reflected at its own end, nothing past it read.
 *   mel_out  element (b, m, t) at mel_out[b * stride_b + m * stride_m + t * stride_t], t < T_b = dsd_mel_num_frames(cfg,
 *            lengths[b], keyshift, speed) ([B, num_mels, T] or [B, T, num_mels] views); frames at or past T_b are not written.
 * One (keyshift, speed) per call.  The DFT basis of each (N', W') is built on the device at its first use and cached.
 */
int dsd_mel_analyze(dsd_handle* h, const float* wav, int32_t B, int64_t n_samples, int64_t wav_stride_b,
                    const int64_t* lengths, double keyshift, double speed, float* mel_out, int64_t stride_b,
                    int64_t stride_m, int64_t stride_t, void* stream);

/* ------------------------------------------------------------------------------------------
 * RMVPE pitch extraction: waveform -> f0 at 16 kHz / hop 160 (100 frames per second), the extractor the reference's
 * binarizers and augmentation select with `pe: rmvpe` (modules/pe/rmvpe/inference.py).  fp32 throughout.  Weights load
 * through dsd_load_weight / dsd_finalize_weights under the reference's state_dict names; `unet.tf.*` (TimbreFilter, never
 * called in forward) and `*.num_batches_tracked` are accepted and ignored, any other unknown name is DSD_ENOTFOUND.  An
 * RMVPE handle returns DSD_ESTATE on every entry point but these and the weight loading; the dsd_rmvpe_* calls return
 * DSD_ESTATE on any other handle.
 * ------------------------------------------------------------------------------------------ */
/* E2E0(n_blocks, n_gru, (2, 2), en_de_layers, inter_layers, 1, en_out_channels)  (modules/pe/rmvpe/model.py:8-31);
   the reference's RMVPE builds E2E0(4, 1, (2, 2)) with en_de_layers 5, inter_layers 4, en_out_channels 16 */
typedef struct dsd_rmvpe_config {
    int32_t struct_size;        /* sizeof(dsd_rmvpe_config)                                        */
    int32_t n_blocks;           /* ConvBlockRes per encoder / intermediate / decoder block, >= 1   */
    int32_t n_gru;              /* 1: BiGRU(384, 256) + Linear(512, 360); 0: Linear(384, 360)      */
    int32_t en_de_layers;       /* 1 .. 5                                                          */
    int32_t inter_layers;       /* >= 1                                                            */
    int32_t en_out_channels;    /* a multiple of 8, 8 .. 64                                        */
    int32_t device;
} dsd_rmvpe_config;

int dsd_rmvpe_create(const dsd_rmvpe_config* cfg, dsd_handle** out);
/*
 * Frame count of RMVPE.infer_from_audio on n_samples samples at sample_rate: L16 = n_samples, or ceil(16000 n_samples /
 * sample_rate) after the resampler; T = 1 + L16 // 160.  DSD_EINVAL where torch.stft's reflect pad raises (L16 <= 512) or
 * sample_rate < 1.  Host only.
 */
int64_t dsd_rmvpe_num_frames(int64_t n_samples, int32_t sample_rate);
/*
 * The mel filterbank MelSpectrogram stores (spec.py:22-29): librosa.filters.mel(sr=16000, n_fft=1024, n_mels=128, fmin=30,
 * fmax=8000, htk=True) - HTK mel scale, Slaney area normalisation, float32.  out: [128][513] host floats.  Host only.
 */
int dsd_rmvpe_filterbank(float* out);
/*
 * Replaces: RMVPE.mel2hidden(mel)  (inference.py:24-29): zero pad to Tp = 32 ceil(T / 32) frames, E2E0.forward over the
 * padded frames (the reverse GRU starts at frame Tp - 1), crop to T.
 *   mel         element (b, m, t) of the natural-log mel [B, 128, T] at mel[b * stride_b + m * stride_m + t * stride_t]
 *               (device fp32)
 *   lengths     HOST array of B frame counts (1 <= lengths[b] <= T) or NULL; item b is computed exactly as a lone call on
 *               its own lengths[b] frames
 *   hidden_out  element (b, t, c) of [B, T, 360] at hidden_out[b * h_stride_b + t * h_stride_t + c]; frames at or past
 *               T_b are not written
 */
int dsd_rmvpe_mel_to_hidden(dsd_handle* h, const float* mel, int32_t B, int32_t T, int64_t stride_b, int64_t stride_m,
                         int64_t stride_t, const int64_t* lengths, float* hidden_out, int64_t h_stride_b,
                         int64_t h_stride_t, void* stream);
/*
 * Replaces: RMVPE.decode(hidden, thred, use_viterbi=False) = to_local_average_f0  (utils.py:8-23) on a device [B, T, 360]
 * hidden (classes contiguous): f0_out[b * f0_stride_b + t] (device fp32), 0 where max < thred.
 */
int dsd_rmvpe_decode(dsd_handle* h, const float* hidden, int32_t B, int32_t T, int64_t h_stride_b, int64_t h_stride_t,
                     float thred, float* f0_out, int64_t f0_stride_b, void* stream);
/*
 * Replaces: to_local_average_f0(hidden, center=centers, thred)  (utils.py:8-23 with the argument of :11-14): the window
 * [clip(c - 4, 0), clip(c + 5, 360)) sits around centers[b * c_stride_b + t] (device int32, clamped to [0, 359]) instead of
 * the argmax; the threshold still reads the frame's maximum, so a window of zeros on a voiced frame gives 10 Hz.
 * 1 <= T <= 131072 frames, as dsd_rmvpe_decode_viterbi: above it DSD_EINVAL before any launch.
 */
int dsd_rmvpe_decode_at(dsd_handle* h, const float* hidden, const int32_t* centers, int32_t B, int32_t T, int64_t h_stride_b,
                        int64_t h_stride_t, int64_t c_stride_b, float thred, float* f0_out, int64_t f0_stride_b, void* stream);
/*
 * Replaces: RMVPE.decode(hidden, thred, use_viterbi=True) = to_viterbi_f0  (utils.py:26-43) and the
 * librosa.sequence.viterbi (0.9.2; the reference pins librosa < 0.10) it calls, restated: 360 states, the row-normalised
 * triangular transition matrix of utils.py:29-31, a uniform initial distribution, eps = the float32 tiny.  log_prob is
 * formed in double from the fp32 hidden (the reference: in float32); value, the transition terms and every comparison are
 * double, first index on ties.  Then to_local_average_f0 around the path.
 *   lengths     HOST array of B frame counts (1 <= lengths[b] <= T) or NULL; item b is decoded exactly as a lone call on
 *               its own lengths[b] frames, and frames at or past T_b are not written (f0_out and path_out)
 *   path_out    NULL, or the path: state of frame t at path_out[b * path_stride_b + t] (device int32, 0 .. 359)
 * A frame whose 360 values sum to zero makes the reference's probabilities NaN; here the call returns and every state it
 * writes is in [0, 359], nothing more.  The log_prob and back-pointer workspaces take 3600 bytes per frame: 1 <= T <= 131072
 * frames and B * T <= 1048576 frames per call, above which DSD_EINVAL (naming the cap) before any launch.
 */
int dsd_rmvpe_decode_viterbi(dsd_handle* h, const float* hidden, int32_t B, int32_t T, int64_t h_stride_b, int64_t h_stride_t,
                             const int64_t* lengths, float thred, float* f0_out, int64_t f0_stride_b, int32_t* path_out,
                             int64_t path_stride_b, void* stream);
/*
 * Replaces: RMVPE.infer_from_audio(audio, sample_rate, thred, use_viterbi=False)  (inference.py:38-51): resample to 16 kHz
 * unless sample_rate == 16000 (torchaudio Resample(sr, 16000, lowpass_filter_width=128): Hann-windowed sinc, rolloff
 * 0.99), MelSpectrogram(center=True), mel2hidden, decode.
 *   wav         item b's sample s at wav[b * wav_stride_b + s], s < n_samples (device fp32)
 *   lengths     HOST array of B sample counts (1 <= lengths[b] <= n_samples) or NULL; item b is computed exactly as a lone
 *               call on its own samples (its own resampled length, frames and padding)
 *   f0_out      f0 of frame t < T_b = dsd_rmvpe_num_frames(lengths[b], sample_rate) at f0_out[b * f0_stride_b + t]
 *   hidden_out  NULL, or the sigmoid output as in dsd_rmvpe_mel_to_hidden
 */
int dsd_rmvpe_infer(dsd_handle* h, const float* wav, int32_t B, int64_t n_samples, int64_t wav_stride_b,
                    const int64_t* lengths, int32_t sample_rate, float thred, float* f0_out, int64_t f0_stride_b,
                    float* hidden_out, int64_t h_stride_b, int64_t h_stride_t, void* stream);

/* ------------------------------------------------------------------------------------------
 * Sampling programs.  Every sampler of the reference (ddpm.py:149-204,221-351 p_sample /
 * p_sample_ddim / p_sample_plms; dpm_solver_pytorch.py:1171-1213; uni_pc.py:590-672;
 * reflow.py:66-138 euler/rk2/rk4/rk5) is a sequence of backbone evaluations whose results enter
 * the solver state only through linear combinations with scalar coefficients that are known
 * before the loop starts.  A program states exactly that: per evaluation, the state buffer fed
 * to the backbone, the model time, and up to DSD_MAX_OUT linear combinations
 *      dst = sum_k coef_k * src_k,     src_k in { model output, state buffers, injected noise }
 * which the library fuses into the epilogue of the backbone's last GEMM.  The coefficients are
 * computed on the host, once per (sampler, schedule, steps) - by dsd_program_build below for a
 * caller of this header, by diffsinger_amd/schedule.py (the same arithmetic, and the yardstick the
 * library's builder is tested against) for the Python side; the device does NFE + axpy.
 * ------------------------------------------------------------------------------------------ */
#define DSD_MAX_TERMS 8
#define DSD_MAX_OUT 3
#define DSD_SRC_MODEL (-1)            /* the backbone output of this evaluation            */
#define DSD_SRC_NOISE_BASE (-1000)    /* src = DSD_SRC_NOISE_BASE - k : k-th injected noise */

typedef struct dsd_term {
    int32_t src;   /* state buffer id >= 0, DSD_SRC_MODEL, or DSD_SRC_NOISE_BASE - k */
    float coef;
} dsd_term;

/* One output of an evaluation.  All outputs of an evaluation read the buffers as they were BEFORE it, so a destination may be
 * a source of the same or of another output (a swap is two outputs).  The outputs of one evaluation must have DISTINCT
 * destinations: they are stored in no promised order, so dsd_sample refuses a duplicate dst with DSD_EINVAL.  A source may be
 * listed more than once in one combination (the model output included); the terms are summed. */
typedef struct dsd_lincomb {
    int32_t dst;      /* state buffer id; distinct among the outputs of one evaluation */
    int32_t n_terms;  /* 1..DSD_MAX_TERMS */
    dsd_term terms[DSD_MAX_TERMS];
} dsd_lincomb;

typedef struct dsd_eval {
    int32_t x_buf;    /* state buffer holding the backbone input x_t */
    float t;          /* model time fed to SinusoidalPosEmb (same for the whole batch) */
    int32_t n_out;    /* 1..DSD_MAX_OUT */
    dsd_lincomb out[DSD_MAX_OUT];
} dsd_eval;

/* Buffer 0 holds x_init on entry.  Every OTHER buffer is undefined on entry - it holds whatever the handle's previous call
 * left there (the buffers are cleared only when they are allocated) - so a program reads a buffer other than 0, as x_buf or as
 * a source, only after an earlier evaluation has written it.  dsd_sample checks the ranges below (DSD_EINVAL, before anything
 * is launched), not this order. */
typedef struct dsd_program {
    int32_t n_bufs;          /* number of state buffers, 1..64 (each [B, F*M, T]); buffer 0 = x_T on entry, the rest undefined */
    int32_t result_buf;      /* buffer holding the sample after the last evaluation */
    int32_t n_evals;
    int32_t n_noise;         /* number of injected [B,F,M,T] noise tensors referenced by terms */
    const dsd_eval* evals;
} dsd_program;

#define DSD_SAMPLE_GRAPH 1u      /* replay the whole loop from a cached hipGraph (captured at first use) */
#define DSD_SAMPLE_GRAPH_LAZY 4u /* with DSD_SAMPLE_GRAPH: run a (program, batch shape) eagerly the first time and capture
                                    its graph when it comes back - capture costs about one loop, and the segments of a
                                    project all differ in length (8 segments of 480-1000 frames: 250 ms capturing each,
                                    136 ms lazily) */
#define DSD_SAMPLE_TRANSPOSE 2u  /* out is [B,T,M] (F == 1) or [B,F,T,M] and
                                    out = sample * out_scale[f*M+m] + out_shift[f*M+m]
                                    (x.transpose(2,3).squeeze(1) + denorm_spec, ddpm.py:350,382-383) */

/*
 * Replaces: the loop of GaussianDiffusion.inference (ddpm.py:244-349) / RectifiedFlow.inference
 * (reflow.py:132-136) after x has been initialised, for the cond of the last dsd_prepare_cond.
 *   x_init    [B,F,M,T] device: initial state (x_T, or the shallow-diffusion start)
 *   noise     n_noise x [B,F,M,T] device, or NULL when n_noise == 0 (ancestral DDPM, ddpm.py:153)
 *   out       [B,F,M,T], or the transposed/denormalised form with DSD_SAMPLE_TRANSPOSE
 *   out_scale/out_shift: device [F*M] (only with DSD_SAMPLE_TRANSPOSE; NULL = identity)
 */
int dsd_sample(dsd_handle* h, const dsd_program* prog, const float* x_init, const float* noise,
               float* out, const float* out_scale, const float* out_shift, uint32_t flags, void* stream);

/* ------------------------------------------------------------------------------------------
 * Building the programs.  Host only and handle-free: no device is touched, and a failure leaves its message in
 * dsd_last_error(NULL).  One build per (sampler, schedule, steps); the result can be run any number of times.
 * ------------------------------------------------------------------------------------------ */
#define DSD_SCHEDULE_LINEAR 0   /* linear_beta_schedule(timesteps, max_beta)  (ddpm.py:64-68): linspace(1e-4, max_beta) */
#define DSD_SCHEDULE_COSINE 1   /* cosine_beta_schedule(timesteps, s=0.008)   (ddpm.py:71-82); max_beta is not read     */
#define DSD_DDPM_TABLES 12
/*
 * Replaces: the register_buffer block of GaussianDiffusion.__init__ (ddpm.py:93-115).  out: HOST, [12][timesteps] fp32 -
 * betas, alphas_cumprod, alphas_cumprod_prev, sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod,
 * log_one_minus_alphas_cumprod, sqrt_recip_alphas_cumprod, sqrt_recipm1_alphas_cumprod, posterior_variance,
 * posterior_log_variance_clipped, posterior_mean_coef1, posterior_mean_coef2, in this order.  Double arithmetic in the
 * reference's (numpy's) operation order, each value rounded to fp32 once.  DSD_EINVAL for a NULL out, an unknown
 * schedule_type or timesteps < 1.
 */
int dsd_ddpm_tables_fill(int32_t schedule_type, int32_t timesteps, double max_beta, float* out);

enum { DSD_SAMPLER_DDPM = 0,            /* p_sample, ancestral (ddpm.py:123-156,347-349): t_max - t_lo steps, one injected
                                           noise tensor per step                                                         */
       DSD_SAMPLER_DDIM = 1,            /* p_sample_ddim (ddpm.py:158-167,334-343)                                       */
       DSD_SAMPLER_PLMS = 2,            /* p_sample_plms, 'pndm' (ddpm.py:169-204,323-333)                               */
       DSD_SAMPLER_DPM_SOLVER_PP = 3,   /* DPM-Solver++ 2M, time_uniform, multistep (dpm_solver_pytorch.py:1171-1213)    */
       DSD_SAMPLER_UNIPC = 4,           /* UniPC bh2, order 2, time_uniform, multistep (uni_pc.py:590-672)               */
       DSD_SAMPLER_RF_EULER = 5,        /* RectifiedFlow.inference (reflow.py:66-138)                                    */
       DSD_SAMPLER_RF_RK2 = 6,
       DSD_SAMPLER_RF_RK4 = 7,
       DSD_SAMPLER_RF_RK5 = 8,
       DSD_SAMPLER_RF_EULER_ONNX = 9 }; /* RectifiedFlowONNX's euler loop (deployment/modules/rectified_flow.py:58-62):
                                           t_start is rounded to fp32 first and dt, the step times are fp32 arithmetic   */

typedef struct dsd_sampler_spec {
    int32_t struct_size;       /* sizeof(dsd_sampler_spec)                                                              */
    int32_t sampler;           /* DSD_SAMPLER_*                                                                          */
    /* the DDPM family (DSD_SAMPLER_DDPM .. DSD_SAMPLER_UNIPC); not read for rectified flow */
    int32_t timesteps;         /* length of each table                                                                  */
    int32_t t_max;             /* the loop starts at step t_max - 1 (K_step_infer, or timesteps); 0 = the empty program  */
    int32_t speedup;           /* >= 1: DDIM / PLMS step by it, DPM-Solver++ / UniPC run t_max / speedup steps over
                                  betas[:t_max]; the ancestral sampler does not read it                                  */
    int32_t t_lo;              /* ancestral only: this program covers steps t_max - 1 .. t_lo (a chunk of the loop)      */
    int32_t noise_index0;      /* ancestral only: the step at t_max - 1 takes noise tensor noise_index0, the next one
                                  noise_index0 + 1, ...; n_noise = noise_index0 + t_max - t_lo                           */
    /* rectified flow (DSD_SAMPLER_RF_*); not read for the DDPM family */
    int32_t steps;             /* sampling_steps                                                                        */
    const float* tables;       /* HOST, [12][timesteps]: from dsd_ddpm_tables_fill, or a checkpoint's own buffers in that
                                  order (the reference reads the buffers as they stand, ddpm.py:117-167)                 */
    double t_start;            /* T_start_infer (0 without a shallow source)                                            */
    double time_scale_factor;  /* hparams['time_scale_factor']                                                          */
} dsd_sampler_spec;

/*
 * Replaces: the sampler dispatch of GaussianDiffusion.inference (ddpm.py:244-349) and RectifiedFlow.inference
 * (reflow.py:117-136) up to the point where the loop runs - everything they compute that does not depend on x.
 * *out is ONE allocation that owns its `evals`; release it with dsd_program_free (NULL is fine).  The scalar arithmetic is
 * the reference's own: fp32 where it works on fp32 tensors (the discrete VP schedule of DPM-Solver++ / UniPC with
 * interpolate_fn's neighbour choice, torch.linspace's two-sided rule, the lambda = -5.1 clip of DPM-Solver++), double for
 * the products of such scalars that multiply one tensor, rounded to fp32 once.  expf / logf / expm1f are the C library's.
 * DSD_EINVAL, with *out untouched and nothing allocated: a NULL argument, a wrong struct_size, an unknown sampler; for the
 * DDPM family NULL tables, timesteps < 1, t_max outside [0, timesteps], speedup < 1, t_lo outside [0, t_max], a negative noise_index0,
 * t_max / speedup < 2 for DPM-Solver++ / UniPC (the reference asserts steps >= order); steps < 0 for rectified flow; a
 * program that would exceed DSD_MAX_TERMS or DSD_MAX_OUT (none of today's samplers does).
 */
int dsd_program_build(const dsd_sampler_spec* spec, dsd_program** out);
void dsd_program_free(dsd_program* prog);

/*
 * Replaces: how GaussianDiffusionONNX.forward derives its loop from the runtime inputs `steps` and `depth`
 * (deployment/modules/diffusion.py:105-131).  depth < 0 (no shallow source): *speedup = timesteps / steps snapped DOWN to
 * one of `factors` (HOST, ascending: the factors of timesteps), *t_max = k_step.  Otherwise depth * timesteps is rounded in
 * fp32, half to even, and capped at k_step; *speedup = that / steps (at least 1, NOT snapped) and *t_max = the depth
 * rounded down to a multiple of it.  DSD_EINVAL for NULL outputs, timesteps or steps < 1, k_step < 0, a NaN depth, or
 * (depth < 0) no factor <= the wanted speed-up.
 */
int dsd_onnx_ddpm_plan(int32_t timesteps, int32_t k_step, const int64_t* factors, int32_t n_factors, int32_t steps,
                       double depth, int32_t* t_max, int32_t* speedup);

/*
 * Arithmetic of the residual layers' two GEMMs (API v10).  DSD_PRECISION_F32 (default): fp32 operands on
 * v_mfma_f32_16x16x4_f32 - the reference's arithmetic, what every BASELINE number is measured in.  DSD_PRECISION_BF16X3
 * (opt-in; SURVEY.md section 7 "hard parts"): every operand split x = hi + lo into two bf16 values, a product evaluated as
 * hi.hi + hi.lo + lo.hi on v_mfma_f32_16x16x32_bf16 with fp32 accumulation; activations, FiLM, gate, residual and skip
 * arithmetic stay fp32.  Measured against the fp32 oracle: 9.9e-6 on one evaluation, 1.9e-6 on the 50-NFE DPM-Solver++
 * sample (tools/bf16x3_tolerance.py; asserted on the GPU in tests/test_gpu_bf16x3.py at the fp32 tolerances).  Exists for the
 * fused WaveNet layer kernel at C = 256 (batched grids) and for LYNXNet's two pointwise GEMMs at C = 1024 / 512 with
 * expansion 2, and - on a vocoder handle (dsd_vocoder_create) - for the residual-block convolutions of every stage with 64 to 256
 * channels, a multiple of 32 (voc_x3.hip: 7e-6 .. 2.4e-5 off the fp32 oracle on the waveform, tools/bf16x3_vocoder_tolerance.py;
 * asserted at the fp32 tolerance in tests/test_gpu_vocoder_x3.py); conv_pre, the transposed convolutions, the 32- / 16-channel
 * stages, conv_post and the source stay fp32, as do other shapes and kernels whatever the mode.  WaveNet, LYNXNet and vocoder
 * handles take the call; every other kind of handle answers DSD_ESTATE, an unknown mode DSD_EINVAL.  Also set for every DENOISER
 * handle of the process by the environment variable DSD_PRECISION=1 at dsd_create (a vocoder handle takes the explicit call
 * only).  May be called at any time; after dsd_finalize_weights it re-packs the weights - the fp32 packing is the same in either
 * mode, so switching back reproduces the fp32 results bit for bit.  dsd_get_stats().precision reports the mode from the path that
 * ran: for a vocoder, BF16X3 after a dsd_vocode / dsd_vocode_ragged call that launched a split-bf16 kernel.
 */
#define DSD_PRECISION_F32 0
#define DSD_PRECISION_BF16X3 1
int dsd_set_precision(dsd_handle* h, int32_t mode);

/* Introspection used by tests, bench.py and the roofline report.  dsd_get_stats and the dsd_kernel_timing* calls below take
   every kind of handle but the analysis ones (mel, RMVPE, separator: DSD_ESTATE). */
typedef struct dsd_stats {
    int64_t weight_bytes;        /* packed weights on the device                        */
    int64_t workspace_bytes;     /* current arena size                                  */
    int64_t flops_per_frame_nfe; /* algorithmic FLOPs per mel frame per NFE (hoisted)   */
    int64_t bytes_per_frame_nfe; /* algorithmic HBM bytes per mel frame per NFE         */
    int32_t kernels_per_nfe;     /* launch sites of a backbone evaluation: the layers' launches and 3 around them (1: the
                                    edge kernel).  A WaveNet in fp32 without the edge kernel launches one kernel fewer than
                                    this: its skip-projection site is folded into the layers' out-proj weights */
    int32_t graphs_cached;
    /* The launch plan of the handle's last call, under the path switches of that call.  WaveNet, how a residual layer runs
       on the current batch shape (API v10): launches per layer (1 = the fused layer kernel over every tile, 2 = the row-split
       pair or the two GEMMs, 3 = a mixed plan: the whole rounds of tiles on the fused kernel, the remainder on the row-split
       pair) and how many tiles each form covers - tiles of their segment's own width (16 or 32 frames) */
    int32_t layer_launches;
    int32_t fused_tiles;
    int32_t split_tiles;
    int32_t precision;           /* DSD_PRECISION_BF16X3: the plan (vocoder: the last call) has a split-bf16 launch, else F32 */
} dsd_stats;
int dsd_get_stats(const dsd_handle* h, dsd_stats* out);

/*
 * Timing hook for bench.py: while enabled, every launch of the dominant kernel (WaveNet: dilated-conv +
 * FiLM + gate GEMM; LYNXNet: the LayerNorm -> C->4C -> SwiGLU GEMM) carries a hipEvent start/stop pair
 * attached to the dispatch itself (hipExtLaunchKernelGGL) on the stream the kernel is launched on; graph
 * replay is bypassed while enabled.  dsd_kernel_timing_read returns the mean kernel duration in milliseconds
 * over the launches recorded since the last reset and their count, plus - for reference - the mean time of
 * an EMPTY hipEventRecord pair on that stream (what a plain event bracket would have added).
 */
int dsd_kernel_timing(dsd_handle* h, int32_t enable);
int dsd_kernel_timing_read(dsd_handle* h, double* mean_ms, double* empty_pair_ms, int64_t* launches);

/*
 * The same pass per kernel CLASS (API v10): the layer kernels of an evaluation are several instantiations (tile halo by
 * dilation, the segments of a mixed plan, the two networks of the variance model each on its own handle), and the roofline
 * report weights them by time.  Classes are returned largest share first; reading does not reset (dsd_kernel_timing does).
 *   name              kernel + template arguments as rocprofv3 prints them, e.g. "wn_layer_kernel<4, 48, 0>"
 *   mean_ms           mean begin -> end time of the launches that carried events (every 7th of the class)
 *   launches          all launches of the class over the pass, evaluations the backbone evaluations of the pass
 *   flops_per_launch  algorithmic FLOPs of one launch over its VALID frames, bytes_per_launch likewise (8(d))
 */
typedef struct dsd_kernel_time {
    char name[96];
    double mean_ms;
    int64_t launches_timed;
    int64_t launches;
    int64_t evaluations;
    double flops_per_launch;
    double bytes_per_launch;
} dsd_kernel_time;
int dsd_kernel_timing_classes(dsd_handle* h, dsd_kernel_time* out, int32_t max_classes, int32_t* n_classes,
                              double* empty_pair_ms);

/*
 * The launch ledger: which kernel instantiations ran.  The library keeps one entry per kernel instantiation it can launch
 * (the GEMM forms, the WaveNet and LYNXNet layer kernels, the vocoder's), and every launch adds one to its entry's count -
 * on the host, when the launch is issued, whether it executes at once or is recorded into a stream capture (the replays of
 * a captured graph add nothing).  The counts are per process, over all handles and devices.  Takes no handle.
 *   dsd_kernel_ledger        fills out[0 .. min(max_entries, *n_entries)) and sets *n_entries to the number of entries the
 *                            library has (constant from load on: call with max_entries = 0 to size the array)
 *   dsd_kernel_ledger_reset  zeroes every count
 *   symbol    the mangled name of the kernel's host-side launch stub, e.g. _ZN3dsd27__device_stub__gemm_kernelILi0E...;
 *             c++filt gives the kernel and its template arguments.  Owned by the library; NULL if it did not resolve
 *   group     1: GEMM forms, 2: WaveNet layer kernels, 4: LYNXNet layer kernels, 8: vocoder kernels
 */
typedef struct dsd_kernel_launches {
    const char* symbol;
    int32_t group;
    int32_t reserved;
    int64_t launches;
} dsd_kernel_launches;
int dsd_kernel_ledger(dsd_kernel_launches* out, int32_t max_entries, int32_t* n_entries);
int dsd_kernel_ledger_reset(void);

/*
 * VR harmonic-noise separation and the variance curves (utils/decomposed_waveform.py: DecomposedWaveformVocalRemover,
 * utils/binarizer_utils.py: get_energy_librosa, get_breathiness, get_voicing, get_tension_base_harmonic).  fp32 throughout.
 * Weights load through dsd_load_weight under CascadedNet's state_dict names (aux_out.weight and num_batches_tracked are
 * accepted and unused), then dsd_finalize_weights.  A separator handle returns DSD_ESTATE on every entry point but these
 * and the weight loading.
 */
/* CascadedNet(n_fft, hop_length, nout, nout_lstm, is_complex=True, is_mono)  (modules/hnsep/vr/nets.py:72-117) */
typedef struct dsd_hnsep_config {
    int32_t struct_size;        /* sizeof(dsd_hnsep_config)                                                          */
    int32_t n_fft;              /* a multiple of 64, 128 .. 4096                                                     */
    int32_t hop_length;         /* 1 .. n_fft / 2                                                                    */
    int32_t nout;               /* a multiple of 4, 4 .. 64                                                          */
    int32_t nout_lstm;          /* a multiple of 8, 8 .. 128                                                         */
    int32_t is_mono;            /* 1: nin = 2 (one complex channel); 0: nin = 4 (stereo; a mono clip is repeated to two
                                   channels and the outputs averaged, as DecomposedWaveformVocalRemover._infer)      */
    int32_t device;
} dsd_hnsep_config;

int dsd_hnsep_create(const dsd_hnsep_config* cfg, dsd_handle** out);
/*
 * Frame count of predict_from_audio's padded spectrogram for a clip of n_samples: 32 (n // 32 + 1), n = n_samples //
 * hop_length + 1 (always a multiple of 32).  DSD_EINVAL for n_samples < 1 or hop_length < 1.  Host only.
 */
int64_t dsd_hnsep_num_frames(int64_t n_samples, int32_t hop_length);
/*
 * Replaces: CascadedNet.forward(spec) in eval mode: complex spectrogram [B, C, n_fft / 2 + 1, T] -> bounded complex mask of the
 * same shape (bins past n_fft / 2 replicate the last one).  C = 1 (mono model) or 2.
 *   spec        re of element (b, c, f, t) at spec[b * s_stride_b + c * s_stride_c + f * s_stride_f + t * s_stride_t], im at
 *               the next float (torch.view_as_real) (device fp32)
 *   lengths     HOST array of B frame counts (multiples of 16, 16 <= lengths[b] <= T) or NULL (T, a multiple of 16); item
 *               b is computed exactly as a lone call on its own frames
 *   mask_out    same layout with the m_stride_* strides; frames at or past lengths[b] are not written
 */
int dsd_hnsep_mask(dsd_handle* h, const float* spec, int32_t B, int32_t T, int64_t s_stride_b, int64_t s_stride_c,
                   int64_t s_stride_f, int64_t s_stride_t, const int64_t* lengths, float* mask_out, int64_t m_stride_b,
                   int64_t m_stride_c, int64_t m_stride_f, int64_t m_stride_t, void* stream);
/*
 * Replaces: CascadedNet.predict_from_audio (nets.py:148-166): zero pad to dsd_hnsep_num_frames frames, STFT (periodic Hann,
 * center=True, pad_mode 'constant') of each channel, spec * forward(spec), iSTFT, crop to the clip.
 *   wav           channel c of item b: sample s at wav[b * wav_stride_b + c * wav_stride_c + s], s < n_samples (device
 *                 fp32); a stereo model with wav_stride_c == 0 sees one clip on both channels (DecomposedWaveformVocalRemover.
 *                 _infer's repeat; one STFT serves both); a mono model ignores wav_stride_c
 *   lengths       HOST array of B sample counts (1 <= lengths[b] <= n_samples) or NULL; item b is computed exactly as a lone
 *                 call on its own samples
 *   harmonic_out  the harmonic part: sample s < lengths[b] of channel c of item b at harmonic_out[b * out_stride_b +
 *                 c * out_stride_c + s]; a stereo model with out_stride_c == 0 writes the mean of its two channels
 *                 (_infer's torch.mean over channels) at harmonic_out[b * out_stride_b + s]
 */
int dsd_hnsep_separate(dsd_handle* h, const float* wav, int32_t B, int64_t n_samples, int64_t wav_stride_b,
                       int64_t wav_stride_c, const int64_t* lengths, float* harmonic_out, int64_t out_stride_b,
                       int64_t out_stride_c, void* stream);
/*
 * Replaces: DecomposedWaveformPyWorld._kth_harmonic(0)  (decomposed_waveform.py:132-193) after its host part: STFT of the
 * harmonic part (Nuttall window of win_size, n_fft = win_size, hop_size, center=True, pad_mode 'reflect'), the per-frame bin
 * mask center = f0 win_size / sample_rate, [max(center - 3.5, 0), min(center + 3.5, win_size / 2 + 1)), center >= 1 (frames
 * at or past f0_lengths[b]: 0), iSTFT with length = the clip's samples.  Needs lengths[b] > win_size / 2 (torch's reflect pad)
 * and hop_size <= win_size / 2 (a larger hop lets the window-square envelope reach 0, where torch.istft raises).
 *   harmonic      item b's sample s at harmonic[b * stride_b + s], s < lengths[b] (device fp32)
 *   f0            the interpolated, edge-padded f0 (fp32, Hz) of frame t < f0_lengths[b] at f0[b * f0_stride_b + t]
 *   out           the base harmonic at out[b * out_stride_b + s], s < lengths[b]
 * Any separator handle serves (no weights are used).
 */
int dsd_base_harmonic(dsd_handle* h, const float* harmonic, int32_t B, int64_t n_samples, int64_t stride_b,
                      const int64_t* lengths, const float* f0, int64_t f0_stride_b, const int64_t* f0_lengths,
                      int32_t sample_rate, int32_t hop_size, int32_t win_size, float* out, int64_t out_stride_b,
                      void* stream);
/* tension domains of get_tension_base_harmonic */
enum { DSD_TENSION_RATIO = 0, DSD_TENSION_DB = 1, DSD_TENSION_LOGIT = 2 };
/*
 * Replaces: get_energy_librosa (binarizer_utils.py:82-102) on the waveform (energy), the aperiodic part = waveform - harmonic
 * (get_breathiness), the harmonic part (get_voicing), and get_tension_base_harmonic from the harmonic part and the base
 * harmonic.  The RMS is librosa 0.9.2's feature.rms(frame_length=win_size, hop_length=hop_size, center=True,
 * pad_mode="constant"); it is padded with zeros or cropped to frames[b]; dB is amplitude_to_db(amin=1e-5, top_db=80) against
 * the item's own maximum.
 *   wav, harmonic, base   item b's sample s < lengths[b] at ptr[b * stride_b + s] (device fp32); each may be NULL when no
 *                         requested curve needs it (energy: wav; breathiness: wav, harmonic; voicing: harmonic; tension:
 *                         harmonic, base)
 *   frames                HOST array of B curve lengths (`length` of the reference)
 *   energy_db             1: energy, breathiness and voicing in dB ('db'); 0: the padded RMS itself ('amplitude')
 *   energy, breathiness, voicing, tension   frame t < frames[b] of item b at ptr[b * out_stride_b + t], or NULL (not computed)
 */
int dsd_variance_curves(dsd_handle* h, const float* wav, const float* harmonic, const float* base, int32_t B,
                        int64_t stride_b, const int64_t* lengths, int32_t hop_size, int32_t win_size, const int64_t* frames,
                        int32_t tension_domain, int32_t energy_db, float* energy, float* breathiness, float* voicing,
                        float* tension, int64_t out_stride_b, void* stream);

/* ------------------------------------------------------------------------------------------
 * A project's track on the device: place each vocoded segment at its offset, cross-fade where it overlaps what is there,
 * export the samples.  Handle-free like dsd_noise_fill: `device` is the HIP device index; no call allocates or
 * synchronises, and every device call can be captured into a hipGraph (one chain of launches).
 *
 * Replaces: the fold of inference/ds_acoustic.py:231-259 over the segments (result = [], cursor = 0; per segment
 * gap = round(offset * sr) - cursor; gap >= 0: append gap zeros and the waveform; else cross_fade(result, wav, cursor + gap))
 * with cross_fade of utils/infer_utils.py:89-96, and save_wav of utils/infer_utils.py:99-104.  Everything float64.
 *
 * The track always ends where the last placed segment ends, so the fold equals placing segment k in place into a float64
 * track of the final length.  With s = round(offset_k * sr), n = len(wav_k), p = the end of segment k - 1 (0 for the
 * first) and F = p - s:
 *   gap      F <= 0:  track[p:s] = 0, track[s:s+n] = wav
 *   overlap  F > 0:   for j in [0, F): r_j = j * (1.0 / (F - 1)), r_{F-1} = 1.0 exactly, r_0 = 0 when F == 1 (np.linspace);
 *                     track[s+j] = (1 - r_j) * track[s+j] + r_j * wav[j], each operation rounded on its own in float64;
 *                     then track[p:s+n] = wav[F:]
 * The results are bit for bit numpy's.
 * ------------------------------------------------------------------------------------------ */

/*
 * Replaces: round(param['offset'] * sr) and the cursor bookkeeping of ds_acoustic.py:253-259.  Host only: never touches a
 * device.  starts_out[k] = nearbyint(offsets_seconds[k] * sample_rate) in double - half to even, as Python's round;
 * prev_ends_out[k] = the p above; *total_out = the end of the last segment = the length of the track.
 * DSD_EINVAL (message under dsd_last_error(NULL)), with nothing promised about the outputs, for: a NULL argument, n_seg < 1 or
 * sample_rate < 1; a length below 1 (stricter than the reference, which would append an empty array: the vocoder never
 * returns one); a start below 0, or an overlap longer than the new segment (F > n) - the two layouts where the reference
 * raises ValueError; a track of more than 2^31 - 1 samples.
 */
int dsd_track_plan(int32_t n_seg, const double* offsets_seconds, const int64_t* lengths, int32_t sample_rate,
                   int64_t* starts_out, int64_t* prev_ends_out, int64_t* total_out);

/*
 * Replaces: one turn of the loop of ds_acoustic.py:252-259 with cross_fade (infer_utils.py:89-96).  One launch: the gap's
 * zeros, the blend and the copy of segment `src` (device fp32, n samples) into `track` (device float64, `total` samples,
 * 8-byte aligned), as above.  Calls are placed in segment order on one stream; after the last one every sample of
 * [0, total) has been written, so the track needs no memset.
 * The call checks the geometry of its own arguments - 0 <= start, n >= 1, start + n <= total <= 2^31 - 1,
 * 0 <= prev_end <= total, prev_end - start <= n - and returns DSD_EINVAL before device selection and before any launch
 * where they fail (also for a NULL or misaligned pointer): a caller without a plan cannot write outside the track.
 */
int dsd_track_place(int32_t device, double* track, int64_t total, int64_t start, int64_t prev_end, const float* src,
                    int64_t n, void* stream);

/*
 * Replaces: np.abs(wav).max() of save_wav(norm=True) (infer_utils.py:100-101).  *peak_out (device, 8-byte aligned) =
 * max |track[i]| over [0, total): exact, a maximum does not depend on the order.  A NaN sample gives a NaN, as in numpy.
 * The call zeroes peak_out itself (a memset node in front of the one launch).
 */
int dsd_track_peak(int32_t device, const double* track, int64_t total, double* peak_out, void* stream);

/*
 * Replaces: save_wav's arithmetic (infer_utils.py:100-104), and the track's way out in the other two formats.
 *   DSD_TRACK_F64   out is double[total]: a copy
 *   DSD_TRACK_F32   out is float[total]: each sample rounded once to fp32
 *   DSD_TRACK_PCM   out is int16_t[total]: v * 32767 in double, truncated toward zero (numpy's astype(np.int16))
 * peak (device double, from dsd_track_peak), or NULL: with a peak the value is (v / *peak) * 32767, in that order
 * (norm=True); DSD_TRACK_PCM only, DSD_EINVAL with the other kinds.
 * Two deviations, both where numpy's own result is undefined: a product outside int16 saturates to -32768 / 32767 (numpy
 * wraps, platform-dependent; NaN gives 0), and a zero peak gives zeros (numpy divides 0 / 0).
 * DSD_EINVAL before any launch for a NULL track or out, an unknown kind, total outside [1, 2^31 - 1] or a misaligned pointer.
 */
#define DSD_TRACK_F64 0
#define DSD_TRACK_F32 1
#define DSD_TRACK_PCM 2
int dsd_track_export(int32_t device, const double* track, int64_t total, int32_t kind, const double* peak, void* out,
                     void* stream);

/* ------------------------------------------------------------------------------------------
 * Validation scoring: what the reference's `_validation_step` computes around ONE denoiser evaluation
 * (training/acoustic_task.py:119-197, training/variance_task.py:162-305) - the noising step of p_losses, the masked
 * losses, the curve metrics and the duration loss with its metrics.  No backward pass; training stays out of scope.
 * Handle-free like dsd_noise_fill: `device` is the HIP device index.  No call synchronises or allocates, and every call
 * can be captured into a hipGraph.  DSD_EINVAL before any device work for a NULL pointer that is not marked optional, a
 * wrong struct_size, an unknown kind, a size below 1, more than 2^31 - 1 elements, or a misaligned pointer.
 *
 * The rounding rule of every reduction below:
 *   - a term is formed as the reference forms it wherever only IEEE fp32 add / sub / mul / div is involved, each
 *     operation rounded on its own (no contraction into FMAs);
 *   - whatever goes through the math library (log, exp) is evaluated in double from the fp32 input;
 *   - the terms are summed in DOUBLE in an order fixed by the problem size alone: workgroup g of G = min(1024,
 *     ceil(n / 2048)) takes the spans g, g + G, ... of 2048 consecutive elements, thread i of 256 takes the elements
 *     i, i + 256, ... of a span in turn, the 256 thread sums are added pairwise (i with i + 128, then + 64, ... + 1), the
 *     G workgroup sums go to `workspace`, and one last workgroup adds them the same way (thread i: partials i, i + 256,
 *     ...).  No floating-point atomics: a result is bit-identical from run to run.
 * workspace: device, DSD_SCORE_WORKSPACE_BYTES, 8-byte aligned, the caller's; two calls on different streams need two.
 * ------------------------------------------------------------------------------------------ */
#define DSD_SCORE_WORKSPACE_BYTES 65536

/* The noising step of p_losses on a dense [B][rows][cols] tensor (rows = F * M, cols = T).
 *   DSD_DIFFUSE_DDPM    ddpm.py:206-219   x_t = fl(fl(a[b] * x0) + fl(c[b] * eps)),  target = eps
 *                       (a = sqrt_alphas_cumprod[t], c = sqrt_one_minus_alphas_cumprod[t], gathered by the caller)
 *   DSD_DIFFUSE_REFLOW  reflow.py:36-41   target = fl(x0 - eps),  x_t = fl(eps + fl(a[b] * target))  with a = t; the
 *                       reference's own association, not (1 - t) * eps + t * x0.  c is not read.
 * eps == NULL: eps is drawn inside the launch from `seeds` under `domain`, stream 0, DSD_NOISE_NORMAL - element for
 * element what dsd_noise_fill draws at the same (seed, domain, row, col) - and `target` is required.  With a given eps
 * and DSD_DIFFUSE_DDPM target may be NULL.  16-byte loads and stores when cols % 4 == 0 and every pointer is 16-byte
 * aligned, the scalar path otherwise.  An output equal to an input (or to the other output) is DSD_EINVAL. */
#define DSD_DIFFUSE_DDPM 0
#define DSD_DIFFUSE_REFLOW 1
typedef struct dsd_diffuse_spec {
    int32_t struct_size;
    int32_t kind;            /* DSD_DIFFUSE_*                                                   */
    int32_t B, rows, cols;
    uint32_t domain;         /* of the in-launch draw (the Python side uses 9 = scoring noise; 8 = scoring t) */
    const float* x0;         /* device [B][rows][cols]: the normalised ground truth             */
    const float* eps;        /* device, the same shape, or NULL: drawn from seeds               */
    const float* a;          /* device [B]                                                      */
    const float* c;          /* device [B]; DSD_DIFFUSE_DDPM only                               */
    const uint64_t* seeds;   /* HOST, B values; read when eps == NULL                           */
} dsd_diffuse_spec;
int dsd_diffuse(int32_t device, const dsd_diffuse_spec* spec, float* x_t, float* target, void* stream);

/* DiffusionLoss / RectifiedFlowLoss / nn.L1Loss as a reduction (diff_loss.py:16-34, reflow_loss.py:18-50,
 * aux_decoder/__init__.py:10-12) over pred, target [B][rows][cols].
 *   term   = |d| (DSD_LOSS_L1) or fl(d * d) (DSD_LOSS_L2) with d = fl(fl(pred * m) - fl(target * m)) in fp32,
 *            m = non_padding[b][col] (NULL: d = fl(pred - target))
 *   weight   t != NULL: the term times, in double, the log-norm weight of item b (reflow_loss.py:26-34)
 *            0.398942 / t' / (1 - t') * exp(-0.5 * log(t' / (1 - t'))^2) + 1e-7,  t' = clip((double)t[b], 1e-7, 1 - 1e-7),
 *            evaluated in double once per item
 *   out[0] = the sum, out[1] = sum / (B * rows * cols): the reference's .mean() over all elements, padded ones included */
#define DSD_LOSS_L1 0
#define DSD_LOSS_L2 1
typedef struct dsd_loss_spec {
    int32_t struct_size;
    int32_t kind;                /* DSD_LOSS_*                        */
    int32_t B, rows, cols;
    const float* pred;           /* device [B][rows][cols]            */
    const float* target;         /* device [B][rows][cols]            */
    const float* non_padding;    /* device [B][cols], or NULL         */
    const float* t;              /* device [B], or NULL               */
} dsd_loss_spec;
int dsd_masked_loss(int32_t device, const dsd_loss_spec* spec, void* workspace, double* out, void* stream);

/* RawCurveAccuracy and RawCurveR2Score in one pass (metrics/curve.py) over n elements, valid where mask != 0 (NULL: all):
 *   close = count of |fl(pred - target)| <= tolerance (fp32 compare), total = count of valid elements,
 *   sum_target = sum target, sum_target_sq = sum fl(target * target), sum_residual_sq = sum fl(r * r), r = fl(target - pred) */
typedef struct dsd_curve_result {
    int64_t close, total;
    double sum_target, sum_target_sq, sum_residual_sq;
} dsd_curve_result;
int dsd_curve_stats(int32_t device, const float* pred, const float* target, const uint8_t* mask, int64_t n, float tolerance,
                    void* workspace, dsd_curve_result* out, void* stream);

/* DurationLoss, RhythmCorrectness and PhonemeDurationAccuracy (dur_loss.py:30-56, metrics/duration.py,
 * tts_modules.py:250-275) on dur_pred, dur_gt [B][L] fp32, ph2word [B][L] int64 (0 = padding; values outside
 * [0, n_words) belong to no word), n_words = ph2word.max() + 1 >= 2, optional mask [B][L] uint8.
 *   word sums   p = dur_pred clamped at 0 (NaN kept); wdur_pred[b][w - 1], wdur_gt[b][w - 1], w = 1 .. n_words - 1, are
 *               the sums of p / dur_gt over the phonemes of word w, added in phoneme order in fp32 - bit for bit torch's
 *               CPU scatter_add, and the same on every run.  The item sums (sdur) are added the same way over all L.
 *   losses      per element e(x, y) = g(log((double)fl(x + offset)) - log((double)fl(y + offset))), g(d) = d * d
 *               (DSD_DUR_MSE) or the Huber function with delta 1 (DSD_DUR_HUBER); pdur over B * L on the UNCLAMPED
 *               prediction, wdur over B * (n_words - 1) word sums, sdur over B item sums; sums and means as doubles.
 *               The lambda-weighted total is the caller's.
 *   rhythm      a word is valid when mask is NULL or any of its phonemes has mask != 0;
 *               correct = valid and |fl(wdur_pred - wdur_gt)| <= fl(wdur_gt * rhythm_tolerance)
 *   phonemes    pd = p * (ph2word > 0); align = rint(fl(pd * fl(wdur_gt[w] / max(wdur_pred[w], 1e-5)))) (0 at w = 0);
 *               accurate = |fl(align - dur_gt)| <= fl(dur_gt * pdur_tolerance) and mask; total = B * L or the mask's count */
#define DSD_DUR_MSE 0
#define DSD_DUR_HUBER 1
typedef struct dsd_dur_spec {
    int32_t struct_size;
    int32_t kind;                /* DSD_DUR_*                         */
    int32_t B, L, n_words;
    float offset;                /* DurationLoss.offset (log_offset)  */
    float rhythm_tolerance, pdur_tolerance;
    const float* dur_pred;       /* device [B][L], raw                */
    const float* dur_gt;         /* device [B][L]                     */
    const int64_t* ph2word;      /* device [B][L]                     */
    const uint8_t* mask;         /* device [B][L], or NULL            */
} dsd_dur_spec;
typedef struct dsd_dur_result {
    double pdur_sum, wdur_sum, sdur_sum;
    double pdur_mean, wdur_mean, sdur_mean;
    int64_t rhythm_correct, rhythm_total, pdur_accurate, pdur_total;
} dsd_dur_result;
int dsd_dur_score(int32_t device, const dsd_dur_spec* spec, float* wdur_pred, float* wdur_gt, void* workspace,
                  dsd_dur_result* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Model files: every model a render needs in ONE file, opened without Python.  A file holds up to DSD_MODEL_MAX_SECTIONS
 * named sections - each one handle: its kind (the DSD_* enum), the bytes of that kind's config struct and its tensors
 * under the names, shapes and fp32 data dsd_load_weight takes - and a table of UTF-8 key / value strings for what a
 * caller needs besides weights (timesteps, K_step, spec_min / spec_max, hop size, sample rate, the phoneme list; the
 * value syntax is the caller's, the library stores and returns it).  The byte layout (format version 1, little-endian)
 * is DESIGN.md section 4n; diffsinger_amd/modelfile.py writes it.
 *
 * Replaces: torch.load of a checkpoint + load_state_dict (utils/__init__.py:166-222 load_ckpt), the config.json beside a
 * vocoder checkpoint (modules/nsf_hifigan/env.py, vocoders/nsf_hifigan.py:22-30) and the hparams a model's constructor
 * reads - for a process that has none of them.
 *
 * dsd_model_open reads the whole file into host memory and validates ALL of it before it returns - magic, version, the
 * recorded size against the file's, the CRC-32, every count, offset, length, name, shape and config size - so no accessor
 * ever looks at an unchecked byte, and every pointer an accessor hands out (names, keys, values, tensor data: 64-byte
 * aligned) points into that one buffer and stays valid until dsd_model_close.  The reader is host code only: no device is
 * touched before dsd_model_create.  A failure of any call below leaves its message under dsd_last_error(NULL).
 *   DSD_EIO     the path cannot be opened, is not a regular file, or cannot be read to its end
 *   DSD_ENOMEM  no host memory for the file
 *   DSD_EINVAL  a NULL argument, an index out of range, or a file that is refused (the message names the section, the
 *               tensor and the field): bad magic; unknown format version; recorded size != file size; CRC mismatch; a count
 *               over its limit; an offset, length or table past the end of the file; tensor data not 64-byte aligned; a
 *               shape whose product is not the stored count, or overflows 64 bits; a negative dim; ndim > 4; a name or key
 *               that is empty, longer than 255 bytes, holds a NUL or is not followed by one; two sections, two tensors of
 *               a section or two keys with one name; an unknown kind; a config size that is not sizeof that kind's struct;
 *               a stored struct_size that is not the config size (for kinds 0..2: a `backbone` that is not the kind); a
 *               tensor on a DSD_MEL_ANALYSIS section
 * ------------------------------------------------------------------------------------------ */
#define DSD_MODEL_FORMAT_VERSION 1
#define DSD_MODEL_MAX_SECTIONS 64
#define DSD_MODEL_MAX_TENSORS 65536     /* per section */
#define DSD_MODEL_MAX_META 65536
#define DSD_MODEL_MAX_NAME 255          /* bytes of a section name, tensor name or metadata key */
#define DSD_MODEL_ALIGN 64              /* of tensor data, in the file and in memory */

typedef struct dsd_model_file dsd_model_file;

typedef struct dsd_model_section_info {
    const char* name;
    int32_t kind;            /* DSD_BACKBONE_WAVENET .. DSD_HNSEP_VR, or DSD_VARIANCE_TABLES             */
    int32_t config_size;     /* sizeof the kind's config struct: what dsd_model_config copies            */
    int32_t n_tensors;
    int64_t total_floats;    /* the sum of the tensors' counts                                           */
} dsd_model_section_info;

typedef struct dsd_model_tensor_info {
    const char* name;        /* the reference state_dict key, as dsd_load_weight takes it                */
    int32_t ndim;            /* 0 .. 4                                                                   */
    int64_t shape[4];        /* shape[ndim ..] = 0                                                       */
    int64_t count;           /* the product of shape[0 .. ndim) (1 for ndim == 0)                        */
    const float* data;       /* host, count floats, DSD_MODEL_ALIGN-aligned                              */
} dsd_model_tensor_info;

int dsd_model_open(const char* path, dsd_model_file** out);      /* *out = NULL on failure */
void dsd_model_close(dsd_model_file* f);                         /* NULL is fine */
int dsd_model_count(const dsd_model_file* f, int32_t* n_sections, int32_t* n_meta);    /* either output may be NULL */
/* index of the section called section_name, DSD_ENOTFOUND when there is none, DSD_EINVAL for a NULL argument */
int dsd_model_find(const dsd_model_file* f, const char* section_name);
int dsd_model_section(const dsd_model_file* f, int32_t i, dsd_model_section_info* out);
/* Copies section i's config struct as stored; cfg_size must be its config_size.  The stored `device` field means nothing:
   dsd_model_create overwrites it, and so does every other reader of the copy. */
int dsd_model_config(const dsd_model_file* f, int32_t i, void* cfg_out, int32_t cfg_size);
int dsd_model_tensor(const dsd_model_file* f, int32_t i, int32_t j, dsd_model_tensor_info* out);
int dsd_model_meta_at(const dsd_model_file* f, int32_t k, const char** key, const char** value);
/* the value stored under key, NULL if there is none (or an argument is NULL) */
const char* dsd_model_meta(const dsd_model_file* f, const char* key);

/*
 * One section -> one finalized handle on `device`: the create call of the section's kind (dsd_create_any_width for
 * DSD_BACKBONE_WAVENET / _LYNXNET / DSD_AUX_CONVNEXT, dsd_encoder_create, dsd_vocoder_create, dsd_token_encoder_create,
 * dsd_mel_create, dsd_rmvpe_create, dsd_hnsep_create) on the stored config with `device` put into it, dsd_load_weight
 * (on_device = 0) of every tensor in file order, dsd_finalize_weights; a DSD_MEL_ANALYSIS section stops after the create.
 * The handle is what those calls would have given: release it with dsd_destroy; it does not refer to the file afterwards.
 * On failure the half-built handle is destroyed, *out = NULL, the code is the failing call's (DSD_ESTATE for a section that
 * lacks a tensor its model needs, DSD_ENOTFOUND for one it does not know) and the message under dsd_last_error(NULL) names
 * the section, the tensor where one was being loaded, and that call's own message.
 */
int dsd_model_create(const dsd_model_file* f, int32_t section, int32_t device, dsd_handle** out);

/* ------------------------------------------------------------------------------------------
 * The variance model's staged twin on one model file: DiffSingerVarianceONNX (deployment/modules/toplevel.py:132-302) and
 * FastSpeech2VarianceONNX (deployment/modules/fastspeech2.py:133-184) stage by stage, for a process without Python.  One
 * object owns the embedding tables the stages read and the model's inner handles (the token encoders and the two
 * denoisers); every stage but the sampler is one call here.  The sampler stage stays dsd_prepare_cond + dsd_program_build +
 * dsd_sample on the handles dsd_variance_backbone lends out.
 *
 * A section of kind DSD_VARIANCE_TABLES holds a dsd_variance_config and, in fp32 under the wrapper's state_dict names,
 *   fs2.txt_embed.weight [vocab_size, H]                        always
 *   cross_lingual_mask [vocab_size]                             always; 1 where the token is in cross_lingual_token_idx, else
 *                                                               0; all zeros switches the language embedding off
 *   fs2.lang_embed.weight [num_lang + 1, H]                     use_lang_id
 *   fs2.onset_embed.weight [2, H], fs2.word_dur_embed.{weight [H, 1], bias [H]}, fs2.midi_embed.weight [128, H]   predict_dur
 *   fs2.ph_dur_embed.{weight [H, 1], bias [H]}                  not predict_dur
 *   spk_embed.weight [num_spk, H]                               use_spk_id (no stage reads it: the caller mixes from it)
 *   melody_encoder.note_midi_embed.{weight [Hm, 1], bias [Hm]}, melody_encoder.note_dur_embed.{weight, bias}       use_melody_encoder
 *   melody_encoder.note_glide_embed.weight [glide_rows, Hm]     use_glide_embed
 *   pitch_retake_embed.weight [2, H]                            predict_pitch
 *   smooth_taps [smooth_width]                                  predict_pitch, optional: the K taps of build_smooth_op as the
 *                                                               exporter's torch computed them (the reference bakes its own
 *                                                               into the exported graph in the same way)
 *                                                               for K >= 2 every tap finite and their sum within 1e-4 of 1
 *   delta_pitch_embed.{weight [H, 1], bias [H]}                 predict_pitch with a melody encoder
 *   base_pitch_embed.{weight [H, 1], bias [H]}                  predict_pitch without one
 *   pitch_embed.{weight [H, 1], bias [H]}, variance_embeds.<name>.{weight [H, 1], bias [H]}                        variances != 0
 * Kind 9 is not assigned: a reader refuses it as unknown.  The format version stays 1; a reader from before this kind
 * refuses such a section by its kind.  dsd_model_create answers DSD_EINVAL for the kind (use dsd_variance_open).
 * ------------------------------------------------------------------------------------------ */
#define DSD_VARIANCE_TABLES 10
#define DSD_VAR_PITCH 0          /* dsd_variance_backbone: the pitch predictor's denoiser                  */
#define DSD_VAR_VARIANCES 1      /* ... and the multi-variance predictor's                                  */
#define DSD_VAR_MAX_CURVES 4     /* energy, breathiness, voicing, tension (param_adaptor.py:10)              */

typedef struct dsd_variance_config {
    int32_t struct_size;         /* sizeof(dsd_variance_config)                                              */
    int32_t hidden_size;         /* hparams['hidden_size']                                                   */
    int32_t vocab_size;
    int32_t num_lang;            /* lang_embed has num_lang + 1 rows                                         */
    int32_t num_spk;
    int32_t predict_dur;         /* 0/1: the word form of the encoder and the duration predictor             */
    int32_t predict_pitch;       /* 0/1                                                                      */
    int32_t use_melody_encoder;  /* 0/1; needs predict_pitch                                                 */
    int32_t use_glide_embed;     /* 0/1; needs use_melody_encoder                                            */
    int32_t use_lang_id;         /* 0/1                                                                      */
    int32_t use_spk_id;          /* 0/1                                                                      */
    uint32_t variances;          /* DSD_EMBED_ENERGY .. DSD_EMBED_TENSION: the predicted variances; their order in every
                                    argument below is the order of the bits (VARIANCE_CHECKLIST)             */
    int32_t melody_hidden_size;  /* melody_encoder_args.hidden_size (0 without a melody encoder)            */
    int32_t glide_rows;          /* len(glide_types) + 1 (0 without a glide table)                           */
    float glide_embed_scale;
    int32_t smooth_width;        /* K = round(midi_smooth_width * audio_sample_rate / hop_size), 1 .. 255    */
    int32_t pitch_repeat_bins;   /* pitch_prediction_args.repeat_bins                                        */
    float pitd_norm_min, pitd_norm_max, pitd_clip_min, pitd_clip_max;
    int32_t var_repeat_bins;     /* total_repeat_bins / the number of predicted variances                    */
    /* indexed by the variance's place in the checklist (0 energy .. 3 tension), read where its bit is set   */
    float var_norm_min[DSD_VAR_MAX_CURVES], var_norm_max[DSD_VAR_MAX_CURVES];
    float var_clamp_min[DSD_VAR_MAX_CURVES], var_clamp_max[DSD_VAR_MAX_CURVES];
    int32_t var_no_clamp[DSD_VAR_MAX_CURVES];    /* 1: the curve is not clamped                              */
    int32_t diffusion_type;      /* DSD_DIFFUSE_DDPM / DSD_DIFFUSE_REFLOW                                    */
    int32_t timesteps, k_step;
    float time_scale_factor;
} dsd_variance_config;

typedef struct dsd_variance dsd_variance;        /* opaque; not a dsd_handle */

/*
 * Replaces: DiffSingerVarianceONNX.__init__ + load_state_dict + build_smooth_op (toplevel.py:133-194).
 * Finds `<prefix>.tables` (kind DSD_VARIANCE_TABLES), `<prefix>.fs2` and - with a melody encoder - `<prefix>.melody` (kind
 * DSD_ENC_FS2_TOKENS), `<prefix>.pitch` (predict_pitch) and `<prefix>.variances` (variances != 0; kinds 0 or 1).  Host checks
 * come first, so a file that is refused touches no device: the tables against their config (a missing tensor, one the
 * flags exclude and a wrong shape are DSD_EINVAL naming the tensor), every flag 0/1, smooth_width in [1, 255], and each
 * inner config against the tables' (a mismatch names both fields).  Then the inner handles are made by dsd_model_create,
 * the tables are uploaded once, and the K smoothing taps are taken from `smooth_taps` where the section has it.  Where it has
 * not, they are computed on the host: sin(pi * linspace(0, 1, K)) with the fp32 argument, each sine rounded from double,
 * divided by their sum (added in double, rounded once) - within 2^-20 of torch's own, whose CPU sine is accurate to one ulp
 * and whose sum order follows the host's vector width, so that no C code gives torch's bits for every K.  K = 1 is 0 / 0 = NaN,
 * as in the reference.  On any failure everything built so far is released and *out = NULL.
 */
int dsd_variance_open(const dsd_model_file* f, const char* prefix, int32_t device, dsd_variance** out);
void dsd_variance_close(dsd_variance* v);            /* NULL is fine */
/* the tables' config as stored (hparams the stages and the caller's dsd_sampler_spec / out_scale / out_shift need) */
int dsd_variance_info(const dsd_variance* v, dsd_variance_config* out);
/* which: DSD_VAR_PITCH / DSD_VAR_VARIANCES.  *out is borrowed: it lives until dsd_variance_close, never dsd_destroy it.
   DSD_EINVAL for a predictor the model does not have. */
int dsd_variance_backbone(const dsd_variance* v, int32_t which, dsd_handle** out);

/*
 * The stage calls.  Every pointer but `lengths` is device memory; int64 where the twin takes LongTensors, bytes for its
 * bool tensors (non-zero = true).  Each call checks all of its arguments on the host before the first launch, reads nothing
 * back, and allocates only when a size grows past what the object's workspace holds: a second call at the same sizes
 * allocates nothing and may be captured in a HIP graph.  DSD_EINVAL: a NULL object, args or required pointer; a wrong
 * struct_size; B < 1; L, W or N outside [1, 2048]; T < 1; a stage the model does not have; a word-form input on a
 * phoneme-form model or the reverse; `languages` missing on a model whose mask has a set entry; `spk_embed` on a model
 * without use_spk_id; spk_rows that is neither 1 nor the stage's length; a lengths entry outside [0, T].  An index outside
 * its table reads as zeros (dsd_cond_assemble); that is the caller's contract, not checked.  Each stage keeps ONE workspace
 * per object, on the object's device (every call makes that device current in the calling thread): two calls of the same
 * stage on one object must not run concurrently, neither from two threads nor on two streams; use one object per stream.
 */
/* Replaces: forward_linguistic_encoder_word / _phoneme (fastspeech2.py:145-176). */
typedef struct dsd_variance_encode_args {
    int32_t struct_size;
    int32_t B, L, W;              /* W words: the word form (predict_dur); 0: the phoneme form                 */
    const int64_t* tokens;        /* [B, L]                                                                    */
    const int64_t* word_div;      /* [B, W] phonemes per word   (word form)                                    */
    const int64_t* word_dur;      /* [B, W] frames per word     (word form)                                    */
    const int64_t* ph_dur;        /* [B, L] frames per phoneme  (phoneme form)                                 */
    const int64_t* languages;     /* [B, L] or NULL                                                            */
    float* encoder_out;           /* [B, L, H]                                                                 */
    uint8_t* x_masks;             /* [B, L]: tokens == 0                                                       */
    int64_t* ph2word;             /* [B, L] or NULL: the word form's length-regulated word index, if wanted
                                     (DSD_EINVAL on a phoneme-form model, which has none)                    */
} dsd_variance_encode_args;
int dsd_variance_encode(dsd_variance* v, const dsd_variance_encode_args* args, void* stream);

/* Replaces: forward_dur_predictor (fastspeech2.py:178-184). */
typedef struct dsd_variance_dur_args {
    int32_t struct_size;
    int32_t B, L;
    const float* encoder_out;     /* [B, L, H]                                                                 */
    const uint8_t* x_masks;       /* [B, L]                                                                    */
    const int64_t* ph_midi;       /* [B, L]                                                                    */
    const float* spk_embed;       /* [B, spk_rows, H] or NULL                                                  */
    int32_t spk_rows;             /* 1 or L                                                                    */
    float* ph_dur_pred;           /* [B, L]                                                                    */
} dsd_variance_dur_args;
int dsd_variance_dur(dsd_variance* v, const dsd_variance_dur_args* args, void* stream);

/* Replaces: forward_pitch_preprocess (toplevel.py:224-261) with MelodyEncoder.forward (variance_encoder.py:130-148). */
typedef struct dsd_variance_pitch_cond_args {
    int32_t struct_size;
    int32_t B, L, N, T;
    const float* encoder_out;     /* [B, L, H]                                                                 */
    const int64_t* ph_dur;        /* [B, L]                                                                    */
    const float* note_midi;       /* [B, N]; < 0: a padding note                                               */
    const uint8_t* note_rest;     /* [B, N]; read with a melody encoder                                        */
    const int64_t* note_dur;      /* [B, N]                                                                    */
    const int64_t* note_glide;    /* [B, N] or NULL (= zeros)                                                  */
    const float* pitch;           /* [B, T]                                                                    */
    const float* expr;            /* [B, T] or NULL (= 1)                                                      */
    const uint8_t* retake;        /* [B, T]                                                                    */
    const float* spk_embed;       /* [B, spk_rows, H] or NULL                                                  */
    int32_t spk_rows;             /* 1 or T                                                                    */
    const int32_t* lengths;       /* HOST, [B] frame counts in [0, T], or NULL: see dsd_frame_curve            */
    float* pitch_cond;            /* [B, T, H]                                                                 */
    float* base_pitch;            /* [B, T]                                                                    */
} dsd_variance_pitch_cond_args;
int dsd_variance_pitch_cond(dsd_variance* v, const dsd_variance_pitch_cond_args* args, void* stream);

/* Replaces: forward_variance_preprocess (toplevel.py:273-290). */
typedef struct dsd_variance_cond_args {
    int32_t struct_size;
    int32_t B, L, T;
    const float* encoder_out;     /* [B, L, H]                                                                 */
    const int64_t* ph_dur;        /* [B, L]                                                                    */
    const float* pitch;           /* [B, T]                                                                    */
    const float* curves[DSD_VAR_MAX_CURVES];     /* [B, T] each: the first V entries, V predicted variances in order */
    const uint8_t* retake;        /* [B, T, V]                                                                 */
    const float* spk_embed;       /* [B, spk_rows, H] or NULL                                                  */
    int32_t spk_rows;             /* 1 or T                                                                    */
    float* variance_cond;         /* [B, T, H]                                                                 */
} dsd_variance_cond_args;
int dsd_variance_cond(dsd_variance* v, const dsd_variance_cond_args* args, void* stream);

/*
 * Replaces: forward_pitch_postprocess (toplevel.py:269-271) with PitchDiffusionONNX.denorm_spec's mean over the bins
 * (deployment/modules/diffusion.py:185-190) and clamp_spec.  sample [B, T, M] as dsd_sample(..., DSD_SAMPLE_TRANSPOSE) writes
 * it with the caller's out_scale / out_shift (M = pitch_repeat_bins): pitch_pred[b, t] = clamp(mean_m sample[b, t, m],
 * pitd_clip_min, pitd_clip_max) + base_pitch[b, t].  The bins are added lane-wise (lane l takes m = l, l + 64, ...) and then
 * across the wave by halving strides 32, 16, .. 1; the sum is divided by M.
 */
int dsd_variance_pitch_post(dsd_variance* v, const float* sample, const float* base_pitch, int32_t B, int32_t T,
                            float* pitch_pred, void* stream);
/*
 * Replaces: forward_variance_postprocess (toplevel.py:296-302) with MultiVarianceDiffusionONNX.denorm_spec's mean
 * (diffusion.py:217-222).  sample [B, V, T, M] ([B, T, M] for V = 1), M = var_repeat_bins: curves_out[i][b, t] =
 * clamp(mean_m sample[b, i, t, m]) for the first V entries, each [B, T]; a variance with var_no_clamp is not clamped.
 */
int dsd_variance_post(dsd_variance* v, const float* sample, int32_t B, int32_t T, float* const* curves_out, void* stream);

/*
 * Speaker mixes on the device.  Replaces: `torch.sum(spk_embed(ids) * values, dim=2)` of the inference front ends
 * (inference/ds_acoustic.py:191-197, inference/ds_variance.py:315-326), for a caller who cannot read `spk_embed.weight` out
 * of the file.  out[b, r, h] = sum over n = 0 .. N-1, in that order, of w[b, r, n] * table[ids[b, n], h]; each product and
 * each sum is rounded to fp32 on its own (no fused multiply-add).  w = values, or with normalize: values / s, a correctly
 * rounded division by s = values[b, r, 0] + values[b, r, 1] + ... in index order.  Nothing is read back: negative
 * proportions and a zero sum are the caller's to exclude, and IEEE arithmetic gives what it gives (a zero sum: inf or NaN).
 * A padding speaker is an id with value 0.  `out` is what the stage calls take as spk_embed with spk_rows = rows.
 * One launch: lanes run along H (16 bytes per lane where H % 4 == 0 and table and out are 16-byte aligned), and all lanes of
 * a (b, r) row read its weights at one address per step.  The ids travel to the device in the object's own small buffer,
 * stream-ordered (use one object per stream).
 * DSD_EINVAL, with nothing launched: a NULL object, args or pointer, a wrong struct_size, a model without use_spk_id or
 * with a frozen_spk_embed (the acoustic twin), B, rows or N below 1, an id outside [0, num_spk).
 * The variance entry reads the tables section's spk_embed.weight; rows is 1, L (dsd_variance_dur) or T.
 */
typedef struct dsd_spk_mix_args {
    int32_t struct_size;
    int32_t B, rows, N;        /* rows: 1 or the stage's length; N >= 1                                         */
    const int32_t* ids;        /* HOST [B, N], each in [0, num_spk)                                             */
    const float* values;       /* device [B, rows, N]                                                           */
    int32_t normalize;         /* 0/1: 1 divides each value by its row's sum                                    */
    float* out;                /* device [B, rows, H]                                                           */
} dsd_spk_mix_args;
int dsd_variance_spk_mix(dsd_variance* v, const dsd_spk_mix_args* args, void* stream);

/* ------------------------------------------------------------------------------------------
 * The acoustic model's staged twin on one model file: DiffSingerAcousticONNX (deployment/modules/toplevel.py:20-103) with
 * FastSpeech2AcousticONNX.forward (deployment/modules/fastspeech2.py:43-130) as its first stage and GaussianDiffusionONNX /
 * RectifiedFlowONNX (deployment/modules/diffusion.py:105-161, rectified_flow.py:37-68) as its second, for a process without
 * Python: phonemes, durations and f0 in, mel out.  One object owns the inner handles (the acoustic encoder, the aux decoder
 * of shallow diffusion, the denoiser), the constants the stages read and the sampler programs it has built.
 *
 * A section of kind DSD_ACOUSTIC_TABLES holds a dsd_acoustic_config and, in fp32,
 *   cross_lingual_mask [vocab_size]        always; 1 where the token is in cross_lingual_token_idx, else 0; all zeros
 *                                          switches the language embedding off (every token then takes lang_embed's row 0)
 *   spec_min [out_dims], spec_max [out_dims]   always (the writer broadcasts a scalar); spec_max[m] > spec_min[m]
 *   fs2.pitch_embed.weight [300, H]        f0_discrete: the Embedding over f0_to_coarse (fastspeech2.py:54-57)
 *   frozen_spk_embed [H]                   optional, needs use_spk_id: takes the place of the caller's spk_embed
 *   frozen_key_shift [1]                   optional, needs DSD_EMBED_KEY_SHIFT: takes the place of the gender curve
 * The format version stays 1 and DSD_API_VERSION stays 10: the kind is an addition, as DSD_VARIANCE_TABLES was.
 * dsd_model_create answers DSD_EINVAL for the kind (use dsd_acoustic_open).
 * ------------------------------------------------------------------------------------------ */
#define DSD_ACOUSTIC_TABLES 11
#define DSD_AC_FS2 0             /* dsd_acoustic_handle: the acoustic encoder (dsd_encode)                 */
#define DSD_AC_AUX 1             /* ... the aux decoder of shallow diffusion (dsd_aux_decode)              */
#define DSD_AC_DENOISER 2        /* ... the denoiser (dsd_prepare_cond / dsd_sample)                       */
#define DSD_AC_PITCH_BINS 300    /* rows of the discrete f0 embedding                                      */

typedef struct dsd_acoustic_config {
    int32_t struct_size;         /* sizeof(dsd_acoustic_config)                                              */
    int32_t hidden_size;         /* hparams['hidden_size']                                                   */
    int32_t vocab_size;
    int32_t out_dims;            /* M mel bins                                                               */
    int32_t num_lang;            /* lang_embed has num_lang + 1 rows (0 without use_lang_id)                 */
    int32_t num_spk;             /* 0 without use_spk_id                                                     */
    int32_t use_lang_id;         /* 0/1: the encoder has a lang_embed                                        */
    int32_t use_spk_id;          /* 0/1                                                                      */
    uint32_t embed_flags;        /* DSD_EMBED_*: the variance, key-shift and speed embeddings of the encoder */
    int32_t f0_discrete;         /* 0/1: f0_embed_type == 'discrete'                                         */
    int32_t use_shallow_diffusion;   /* 0/1: the model has an aux decoder                                    */
    float shift_min, shift_max;  /* augmentation_args.random_pitch_shifting.range (read with the key-shift bit)  */
    float speed_min, speed_max;  /* augmentation_args.random_time_stretching.range (read with the speed bit)     */
    int32_t mel_base_e;          /* 0/1; 0: the sampler stage multiplies its mel by 2.30259 (log10 -> ln)    */
    int32_t diffusion_type;      /* DSD_DIFFUSE_DDPM / DSD_DIFFUSE_REFLOW                                    */
    int32_t timesteps, k_step;   /* DDPM; k_step == timesteps without shallow diffusion                      */
    int32_t schedule_type;       /* DSD_SCHEDULE_LINEAR / _COSINE (DDPM)                                     */
    double max_beta;             /* the linear schedule's max_beta as the wrapper built its tables (DDPM)    */
    float t_start;               /* hparams['T_start'] (reflow; 0 without shallow diffusion)                 */
    float time_scale_factor;     /* hparams['time_scale_factor'] (reflow)                                    */
} dsd_acoustic_config;

typedef struct dsd_acoustic dsd_acoustic;        /* opaque; not a dsd_handle */

/*
 * Replaces: DiffSingerAcousticONNX.__init__ + load_state_dict (toplevel.py:20-53).
 * Finds `<prefix>.tables` (kind DSD_ACOUSTIC_TABLES), `<prefix>.fs2` (DSD_ENC_FS2_ACOUSTIC), `<prefix>.aux` (DSD_AUX_CONVNEXT,
 * with use_shallow_diffusion) and `<prefix>.denoiser` (kind 0 or 1).  Host checks come first, so a file that is refused
 * touches no device: the tables against their config (a missing tensor, one the config excludes and a wrong shape are
 * DSD_EINVAL naming the tensor), every flag 0/1, every mask value 0/1, spec_max[m] > spec_min[m], shift_min <= 0 <= shift_max,
 * 0 < speed_min <= speed_max, and each inner config against the tables' (encoder hidden_size, vocab_size, embed_flags,
 * num_spk, num_lang; denoiser in_dims == out_dims, n_feats == 1, hidden_size; aux decoder in_dims, n_feats, hidden_size; a
 * mismatch names both fields).  Then the inner handles are made by dsd_model_create and the constants - k = (spec_max -
 * spec_min) / 2 and mid = (spec_max + spec_min) / 2, formed in fp32 - are uploaded once.  On any failure everything built
 * so far is released and *out = NULL.
 */
int dsd_acoustic_open(const dsd_model_file* f, const char* prefix, int32_t device, dsd_acoustic** out);
void dsd_acoustic_close(dsd_acoustic* a);            /* NULL is fine */
/* the tables' config as stored */
int dsd_acoustic_info(const dsd_acoustic* a, dsd_acoustic_config* out);
/* which: DSD_AC_FS2 / DSD_AC_AUX / DSD_AC_DENOISER.  *out is borrowed: it lives until dsd_acoustic_close, never dsd_destroy
   it.  DSD_EINVAL for DSD_AC_AUX on a model without shallow diffusion. */
int dsd_acoustic_handle(const dsd_acoustic* a, int32_t which, dsd_handle** out);

/*
 * The stage calls follow dsd_variance_*'s conventions: every pointer is device memory unless marked HOST; each call checks
 * all of its arguments on the host before the first launch, reads nothing back, keeps ONE workspace per stage per object on
 * the object's device (made current by every call) that only grows - a second call at the same sizes allocates nothing and
 * may be captured in a HIP graph.  Use one object per stream.
 *
 * Replaces: forward_fs2_aux (toplevel.py:61-81) with FastSpeech2AcousticONNX.forward (fastspeech2.py:59-130), in this
 * order: durations * (tokens > 0); mel2ph = dsd_length_regulate; f0 * (mel2ph > 0); languages * mask[tokens] (zeros when the
 * model has a lang_embed and the mask is all zeros); the key shift - frozen_key_shift broadcast where the file has it, else
 * with g = clip(gender, -1, 1) and m = g < 0: g * ((1 - m) * shift_max + m * |shift_min|), each product and sum rounded to
 * fp32 on its own; the speed clip(velocity, speed_min, speed_max), 1 for a NULL velocity; frozen_spk_embed in place of
 * spk_embed where the file has it; dsd_encode on the encoder handle; with f0_discrete, condition +
 * pitch_embed.weight[f0_to_coarse(f0)] by dsd_cond_assemble (the encoder's own pitch term is stored as zeros and sees f0 = 0);
 * dsd_aux_decode last, with the denorm x * k + mid.
 * DSD_EINVAL: what dsd_variance_* refuses of this kind (NULL object, args or required pointer, struct_size, B < 1, L outside
 * [1, 2048], T < 1, spk_embed on a model without use_spk_id or missing on one with it and no frozen_spk_embed, spk_rows
 * neither 1 nor T); gender NULL where it is read; a curve NULL for a set DSD_EMBED_ENERGY .. _TENSION bit or given for a
 * cleared one; gender / velocity given on a model without the embedding; aux_mel on a model without an aux decoder, or
 * NULL on one with it; languages NULL while the mask has a set entry (and the model a lang_embed).
 */
typedef struct dsd_acoustic_condition_args {
    int32_t struct_size;
    int32_t B, L, T;
    const int64_t* tokens;        /* [B, L]; 0 = padding                                                       */
    const int64_t* durations;     /* [B, L] frames per phoneme; every item's total is at most T                */
    const float* f0;              /* [B, T] Hz                                                                 */
    const float* curves[4];       /* [B, T] each, by the order of the DSD_EMBED_ENERGY .. _TENSION bits; NULL where clear */
    const float* gender;          /* [B, T] or NULL                                                            */
    const float* velocity;        /* [B, T] or NULL (= 1)                                                      */
    const float* spk_embed;       /* [B, spk_rows, H] or NULL                                                  */
    int32_t spk_rows;             /* 1 or T                                                                    */
    const int64_t* languages;     /* [B, L] or NULL                                                            */
    float* condition;             /* [B, T, H]                                                                 */
    float* aux_mel;               /* [B, T, M]: exactly when the model has shallow diffusion                   */
    int64_t* f0_coarse;           /* [B, T] or NULL: f0_to_coarse(f0 * (mel2ph > 0)), if wanted; f0_discrete only */
} dsd_acoustic_condition_args;
int dsd_acoustic_condition(dsd_acoustic* a, const dsd_acoustic_condition_args* args, void* stream);

/*
 * Replaces: how GaussianDiffusionONNX.forward (diffusion.py:105-131) and RectifiedFlowONNX.forward (rectified_flow.py:
 * 37-57) turn the runtime inputs `depth` and `steps` into a start state and a loop.  Host only, and on a config, not an
 * object: it runs without a GPU.  depth < 0: no shallow source (forward_diffusion / forward_reflow).
 *   DDPM    (t_max, speedup) = dsd_onnx_ddpm_plan on the factors of `timesteps`.  start: NOISE without a source or when
 *           t_max >= timesteps; MIX for 0 < t_max < timesteps with src_scale = sqrt_alphas_cumprod[t_max - 1] and noise_scale
 *           = sqrt_one_minus_alphas_cumprod[t_max - 1] of dsd_ddpm_tables_fill(schedule_type, timesteps, max_beta); SOURCE at
 *           t_max == 0.  n_step_noise = t_max when speedup == 1 (the ancestral sampler), else 0 (DDIM).
 *   reflow  t_start = max(fp32(1 - depth), fp32(T_start)) with a source, 0 without.  NOISE for t_start <= 0, SOURCE for
 *           t_start >= 1, else MIX with src_scale = t_start and noise_scale = fp32(1.0 - (double)t_start).  t_max, speedup
 *           and n_step_noise are 0.
 * NOISE has src_scale 0 and noise_scale 1, SOURCE 1 and 0.  DSD_EINVAL: a NULL argument, a wrong cfg->struct_size, an
 * unknown diffusion_type, a NaN depth, steps < 1 on DDPM, and whatever dsd_onnx_ddpm_plan / dsd_ddpm_tables_fill refuse.
 */
#define DSD_AC_START_NOISE 0
#define DSD_AC_START_MIX 1
#define DSD_AC_START_SOURCE 2
typedef struct dsd_acoustic_plan_t {
    int32_t mode;                 /* DSD_DIFFUSE_DDPM / DSD_DIFFUSE_REFLOW                                      */
    int32_t start;                /* DSD_AC_START_*                                                            */
    int32_t t_max, speedup;       /* DDPM                                                                      */
    float t_start;                /* reflow                                                                    */
    int32_t n_step_noise;         /* [B, 1, M, T] tensors dsd_acoustic_sample reads from step_noise            */
    float src_scale, noise_scale;
    int32_t steps;                /* as given: reflow's euler steps                                            */
} dsd_acoustic_plan_t;
int dsd_acoustic_plan(const dsd_acoustic_config* cfg, float depth, int32_t steps, dsd_acoustic_plan_t* out);

/*
 * Replaces: the start state of GaussianDiffusionONNX.forward (diffusion.py:117-129: norm_spec, q_sample) and
 * RectifiedFlowONNX.forward (rectified_flow.py:45-56).  SOURCE or MIX: x[b, 0, m, t] = src_scale * ((source[b, t, m] - mid[m])
 * / k[m]) + noise_scale * noise[b, 0, m, t] - a correctly rounded division, both products and the sum rounded on their own;
 * SOURCE, and MIX with noise == NULL, write the normalised, transposed source alone (after the latter the caller mixes
 * seeded noise in place: dsd_noise_fill with src = x, src_scale, scale = noise_scale).  NOISE copies noise to x.  x must not
 * overlap source or noise.  DSD_EINVAL: a NULL object, plan or x, B < 1, T < 1, B * M * T > 2^31 - 1, an unknown plan->start,
 * source NULL for SOURCE / MIX, noise NULL for NOISE.
 */
int dsd_acoustic_start(dsd_acoustic* a, const dsd_acoustic_plan_t* plan, const float* source, const float* noise, int32_t B,
                       int32_t T, float* x, void* stream);

/*
 * Replaces: the loop and denorm_spec of GaussianDiffusionONNX.forward (diffusion.py:131-161) / RectifiedFlowONNX.forward
 * (rectified_flow.py:58-68), and ensure_mel_base (toplevel.py:55-59).  dsd_prepare_cond on the denoiser with the [B, T, H]
 * strides; the plan's program from dsd_program_build - DDIM at (t_max, speedup), the ancestral sampler in chunks of 50 steps
 * with step_noise consumed in order, DSD_SAMPLER_RF_EULER_ONNX for reflow, the empty program at t_max == 0, t_start >= 1 or
 * (reflow) steps < 1 - cached on the object per plan (at most 32, then the cache is cleared); dsd_sample with
 * DSD_SAMPLE_TRANSPOSE | flags, out_scale = k, out_shift = mid; with mel_base_e == 0 one more launch multiplies mel in place
 * by fp32(2.30259).  flags: DSD_SAMPLE_GRAPH / DSD_SAMPLE_GRAPH_LAZY (not inside a capture of the caller's own).
 * DSD_EINVAL: a NULL object, plan, condition, x or mel, B < 1, T < 1, a plan whose mode is not the model's or whose fields
 * are out of range, step_noise NULL with n_step_noise > 0, a flag other than the two.
 */
int dsd_acoustic_sample(dsd_acoustic* a, const dsd_acoustic_plan_t* plan, const float* condition, const float* x,
                        const float* step_noise, int32_t B, int32_t T, uint32_t flags, float* mel, void* stream);

/*
 * Ragged lengths through the acoustic object.  Replaces: the one-utterance-per-call loop of inference/ds_acoustic.py:214-271
 * for a C caller, as dsd_set_lengths does for a handle.  lengths: HOST array of B values, copied; NULL restores dense
 * batches.  It applies to the following dsd_acoustic_condition / _start / _sample calls at batch size B until changed: item
 * b of a padded batch comes out as the same item run alone through the same calls at T = lengths[b] - condition, aux mel and
 * mel over t < lengths[b]; outputs at t >= lengths[b] are unspecified.  The encoder gives this by itself (its frames do not
 * mix along time); the aux decoder and the denoiser get it from dsd_set_lengths on the inner handles, which this call sets
 * both or, on a refusal, neither.  The object touches the inner handles' lengths only inside this call: a caller who set
 * lengths on a borrowed handle and never calls this keeps that behaviour.  Works with DSD_SAMPLE_GRAPH / _GRAPH_LAZY (the
 * graph key holds the lengths), with the chunked ancestral sampler, and with dsd_noise_fill in place on x (element (m, t) of
 * x_T does not depend on T).  DSD_EINVAL: a NULL object, B < 1, a negative length; then, from the stage calls: a length above
 * that call's T (DSD_EINVAL) and a call at another B (DSD_ESTATE).
 */
int dsd_acoustic_set_lengths(dsd_acoustic* a, const int32_t* lengths, int32_t B, void* stream);
/* dsd_spk_mix_args (above dsd_variance_spk_mix) on the table the encoder handle holds; rows is 1 or T */
int dsd_acoustic_spk_mix(dsd_acoustic* a, const dsd_spk_mix_args* args, void* stream);

/* ------------------------------------------------------------------------------------------
 * The variance front end's score algebra: what stands between a score and the inputs of dsd_variance_encode / _dur
 * (word_dur, ph_midi), and between dsd_variance_dur's prediction and the integer durations every later stage takes.
 * Three handle-free entries in the style of dsd_length_regulate: `device` is the HIP device index; every array is on the
 * device but the ones marked HOST; every argument is checked on the host before the first launch; nothing is read back, no
 * device memory is kept, and each call can be captured in a HIP graph.  B lies in [1, 65535]; every token, word or note
 * count in [1, 2048].  DSD_EINVAL, with nothing launched: NULL args or a NULL required pointer, a wrong struct_size, a size
 * outside those ranges, and what each entry names below.  DSD_API_VERSION stays 10: the entries are additions.
 * ------------------------------------------------------------------------------------------ */
/*
 * Replaces: word_dur from ph_num / ph_dur or from note_slur / note_dur, and its alignment to the notes' frames
 * (inference/ds_variance.py:185-206).
 *   index[i]        = the given index (the front end's ph2word: 1-based, 0 for a padding phone), or with `slur` the
 *                     inclusive count of the non-slur notes up to and including note i: cumsum(~is_slur).  A leading slur
 *                     has index 0 and is dropped, as by the reference's [:, 1:].  A padding note carries slur = 1, dur = 0.
 *   word_dur[w - 1] = the sum of dur[i] over index[i] == w; an index outside [1, W] adds nothing.  int64 arithmetic:
 *                     exact in any order (the reference's scatter_add).
 * With `totals` the words are aligned to the item's frame count as :202-205 does through mel2word: with
 * c[w] = min(word_dur[0] + .. + word_dur[w], totals[b]) the durations become c[w] - c[w - 1] (what a cut mel2word counts),
 * and where the sum is smaller than totals[b] the last word with a non-zero duration takes the rest (the padding with
 * mel2word's last value).  An item whose words are all zero stays all zero.  Exactly one of index and slur is given; a
 * total outside [0, 2^31 - 1] is DSD_EINVAL.  Negative durations are the caller's to exclude.
 */
typedef struct dsd_word_dur_args {
    int32_t struct_size;
    int32_t B, N, W;              /* N phones (index) or notes (slur); W words                                 */
    const int64_t* dur;           /* [B, N] frames per phone or note                                           */
    const int64_t* index;         /* [B, N], or NULL                                                           */
    const uint8_t* slur;          /* [B, N] bytes (non-zero = slur), or NULL                                   */
    const int64_t* totals;        /* HOST [B] frame counts, or NULL: no alignment                              */
    int64_t* word_dur;            /* [B, W]                                                                    */
    int64_t* index_out;           /* [B, N] or NULL: the index itself, if wanted                               */
} dsd_word_dur_args;
int dsd_word_dur(int32_t device, const dsd_word_dur_args* args, void* stream);
/*
 * Replaces: the `midi` input of the variance model, the rounded per-phone or per-word mean of the frame MIDI curve
 * (inference/ds_variance.py:219-241).  Frames belong to notes (note_dur) and to groups (group_dur: ph_dur, or the aligned
 * word_dur) exactly as dsd_length_regulate assigns them at this T: a zero duration owns no frame, and a frame at or past a
 * row's total belongs to nothing - the frame MIDI there is 0, the F.pad(note_midi, [1, 0]) row.  For group g with
 * n = group_dur[g] and its frames' MIDI values m_0, m_1, .. in frame order,
 *   sum = ((0.0f + m_0 / (float)n) + m_1 / (float)n) + ..      every division and addition rounded to fp32 on its own
 *   r[g] = (int64)rintf(sum)                                   half to even, as torch.round; 0 for a group with no frame
 * which is torch's CPU scatter_add of frame_midi / mel2dur, bit for bit.  Without ph2word, midi [B, G] = r.  With it the
 * groups are words and midi [B, L] is gathered: midi[b, i] = r[ph2word[b, i] - 1], 0 for an index outside [1, G].
 * One lane walks a group's frames (the sum is one dependent chain by definition): the cost is T additions at most.
 * note_midi holds the rests already filled (:138-145).  L is 0 without ph2word; T < 1 is DSD_EINVAL.
 */
typedef struct dsd_group_midi_args {
    int32_t struct_size;
    int32_t B, Nn, G, L, T;       /* Nn notes, G groups, L phones (0 without ph2word), T frames                */
    const float* note_midi;       /* [B, Nn]                                                                   */
    const int64_t* note_dur;      /* [B, Nn]                                                                   */
    const int64_t* group_dur;     /* [B, G]                                                                    */
    const int64_t* ph2word;       /* [B, L] or NULL                                                            */
    int64_t* midi;                /* [B, L] with ph2word, else [B, G]                                          */
} dsd_group_midi_args;
int dsd_group_midi(int32_t device, const dsd_group_midi_args* args, void* stream);
/*
 * Replaces: RhythmRegulator.forward with its default eps = 1e-5 (modules/fastspeech/tts_modules.py:250-275), called on the
 * duration predictor's output at inference/ds_variance.py:339.
 *   d[i]     = ph_dur_pred[i] * (ph2word[i] > 0)
 *   s[w]     = the fp32 sum of d[i] over ph2word[i] == w, in index order from 0.0f (torch's CPU scatter_add)
 *   alpha[w] = (float)word_dur[w - 1] / max(s[w], 1e-5f),  alpha[0] = 0
 *   ph_dur[i] = (int64)rintf(d[i] * alpha[ph2word[i]])      half to even
 * defined for ph2word in any order, not only the non-decreasing one dsd_length_regulate makes.  An index outside [0, W]
 * adds nothing and gets duration 0.
 */
typedef struct dsd_rhythm_align_args {
    int32_t struct_size;
    int32_t B, L, W;
    const float* ph_dur_pred;     /* [B, L]                                                                    */
    const int64_t* ph2word;       /* [B, L]                                                                    */
    const int64_t* word_dur;      /* [B, W]                                                                    */
    int64_t* ph_dur;              /* [B, L]                                                                    */
} dsd_rhythm_align_args;
int dsd_rhythm_align(int32_t device, const dsd_rhythm_align_args* args, void* stream);

/*
 * Ragged lengths through the variance object: the twin of dsd_acoustic_set_lengths.  Replaces: the one-segment-per-call loop
 * of inference/ds_variance.py:344-360 for a C caller.  lengths: HOST array of B frame counts, copied; NULL restores dense
 * batches bit for bit.  Everything dsd_set_lengths would refuse is checked first (B outside [1, 65535], a negative length:
 * DSD_EINVAL); then dsd_set_lengths runs on each denoiser the model has, so both are set, or neither.  The object keeps its
 * own copy and checks the (B, T) of the following dsd_variance_pitch_cond / _cond / _pitch_post / _post calls against it:
 * another B is DSD_ESTATE, a length above T is DSD_EINVAL.  dsd_variance_pitch_cond with args->lengths == NULL then takes
 * the object's copy for dsd_frame_curve; a non-NULL args->lengths that differs from the copy is DSD_EINVAL.  The token-level
 * stages need nothing (their padding is tokens == 0).  Item b of a padded batch comes out as the same item run alone at
 * T = lengths[b]; outputs at or past lengths[b] are whatever the padded computation gives: read lengths[b] frames.
 * Without this call no stage changes.
 */
int dsd_variance_set_lengths(dsd_variance* v, const int32_t* lengths, int32_t B, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DSDENOISE_H_ */
