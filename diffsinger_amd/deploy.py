"""The staged, editor-facing entry points of the deployment twins (`deployment/modules/toplevel.py`,
`deployment/modules/fastspeech2.py`) on libdsdenoise.

An editor does not call `DiffSingerVariance.forward`: it calls one stage at a time - linguistic encoder, duration
predictor, pitch pre-process / sampler / post-process, variance pre-process / sampler / post-process, and on the acoustic
side `forward_fs2_aux` followed by one sampler stage - with durations (`word_div`, `word_dur`, `ph_dur`, `note_dur`)
instead of a precomputed `mel2ph`, and with the `retake` masks and `expr` of partial re-rendering.
`DiffSingerVarianceDeploy` and `DiffSingerAcousticDeploy` expose those stages with the reference's signatures and return
shapes.  They subclass `DiffSingerVariance` / `DiffSingerAcoustic`, add no parameters, and load the same checkpoints.

What is new underneath is the duration-to-frame work, on two handle-free entries: `dsd_length_regulate` (durations ->
mel2x by prefix sum and binary search) and `dsd_frame_curve` (frame MIDI gather, the replicate-padded sinusoidal smoothing,
and the retake blend in one launch).  Encoders, `dsd_predict_dur`, `dsd_cond_assemble` and the samplers (`forward_onnx`)
are the ones the parent classes run.  Extra keywords beyond the reference's: `noise=` / `step_noise=` on the sampler
stages (the x_T, for reproducible runs), `lengths=` on `forward_pitch_preprocess` (a ragged batch).  Inference only; no
CPU path.  The twins' `view_as_*` methods only trim modules for export and have no counterpart here.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .encoder import PAD_INDEX, FastSpeech2Acoustic
from .hparams import hparams
from .toplevel import DiffSingerAcoustic
from .variance import DiffSingerVariance, _arange_idx, _check_infer, assemble, lin1

# f0_to_coarse (deployment/modules/fastspeech2.py:14-28)
F0_BIN = 256
F0_MEL_MIN = 1127 * np.log(1 + 50.0 / 700)
F0_MEL_MAX = 1127 * np.log(1 + 1100.0 / 700)


def _device_index(t, what):
    if t.device.type != "cuda":
        raise RuntimeError(f"diffsinger_amd.deploy.{what} runs only on an MI355X (HIP) device; there is no CPU path")
    return t.device.index if t.device.index is not None else torch.cuda.current_device()


def _fail(what, rc):
    raise _lib.NativeLibraryError(f"{what} failed ({rc}): {_lib.lib().dsd_last_error(None).decode()}")


def length_regulate(dur, t_len=None):
    """`LengthRegulator.forward(dur)` (fastspeech2.py:31-40) on `dsd_length_regulate`: dur [B, L] int64 -> mel2x [B, T].
    `t_len` None takes the reference's T, the batch's largest total, which costs a read-back; a caller that knows its
    frame count passes it."""
    dev = _device_index(dur, "length_regulate")
    dur = dur.detach().to(torch.int64).contiguous()
    bsz, n_tok = dur.shape
    if t_len is None:
        t_len = int(dur.sum(dim=1).max())
    out = torch.empty((bsz, t_len), device=dur.device, dtype=torch.int64)
    if bsz == 0 or t_len == 0:
        return out
    stream = torch.cuda.current_stream(dur.device).cuda_stream
    rc = _lib.lib().dsd_length_regulate(dev, C.c_void_p(dur.data_ptr()), bsz, n_tok, t_len, C.c_void_p(out.data_ptr()),
                                        C.c_void_p(stream))
    if rc != 0:
        _fail("dsd_length_regulate", rc)
    return out


def smooth_kernel(kernel_size):
    """The taps of `build_smooth_op` (toplevel.py:189-192), with its own numpy / torch fp32 ops."""
    k = torch.sin(torch.from_numpy(np.linspace(0, 1, kernel_size).astype(np.float32) * np.pi))
    k /= k.sum()
    return k


def frame_curve(note_midi, mel2note, pitch, retake, weights, lengths=None):
    """`dsd_frame_curve`: -> (base, blend, delta), each [B, T] (include/dsdenoise.h).  weights: the K taps, a host tensor."""
    dev = _device_index(mel2note, "frame_curve")
    device = mel2note.device
    bsz, t_len = mel2note.shape
    note_midi = note_midi.detach().to(device=device, dtype=torch.float32).contiguous()
    mel2note = mel2note.detach().to(torch.int64).contiguous()
    pitch = pitch.detach().to(device=device, dtype=torch.float32).expand(bsz, t_len).contiguous()
    retake = retake.detach().to(device=device, dtype=torch.bool).expand(bsz, t_len).contiguous()
    if note_midi.dim() != 2 or note_midi.shape[0] != bsz:
        raise ValueError(f"note_midi [B={bsz}, N] expected, got {tuple(note_midi.shape)}")
    out = torch.empty((3, bsz, t_len), device=device, dtype=torch.float32)
    if bsz == 0 or t_len == 0:
        return out[0], out[1], out[2]
    w = np.ascontiguousarray(weights.detach().cpu().numpy() if torch.is_tensor(weights) else weights, dtype=np.float32)
    lens = None
    if lengths is not None:
        vals = [int(v) for v in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
        if len(vals) != bsz:
            raise ValueError(f"{len(vals)} lengths for a batch of {bsz}")
        lens = (C.c_int32 * bsz)(*vals)
    stream = torch.cuda.current_stream(device).cuda_stream
    rc = _lib.lib().dsd_frame_curve(dev, C.c_void_p(note_midi.data_ptr()), C.c_void_p(mel2note.data_ptr()),
                                    C.c_void_p(pitch.data_ptr()), C.c_void_p(retake.data_ptr()), bsz, note_midi.shape[1],
                                    t_len, lens, w.ctypes.data_as(C.POINTER(C.c_float)), int(w.shape[0]),
                                    C.c_void_p(out[0].data_ptr()), C.c_void_p(out[1].data_ptr()),
                                    C.c_void_p(out[2].data_ptr()), C.c_void_p(stream))
    if rc != 0:
        _fail("dsd_frame_curve", rc)
    return out[0], out[1], out[2]


def _spk_gather(spk_embed, bsz, t_len, dev):
    """[B or 1, T or 1, H] as an assemble gather over the frames (or tokens)."""
    idx = _arange_idx(bsz, t_len, dev) if spk_embed.shape[1] == t_len and t_len > 1 else \
        torch.zeros((bsz, t_len), dtype=torch.int64, device=dev)
    return spk_embed.expand(bsz, -1, -1), idx, 0, 1.0


def _cross_lingual(module, cross_lingual_token_idx):
    idx = torch.LongTensor(list(cross_lingual_token_idx) if cross_lingual_token_idx is not None else [])
    module.register_buffer('cross_lingual_token_idx', idx, persistent=False)
    return len(idx) > 0                                    # an empty list switches the language embedding off (:51-52, 141-142)


def _masked_languages(module, tokens, languages):
    """languages * any(tokens == cross_lingual_token_idx) (fastspeech2.py:80-84, 153-158)."""
    return languages * torch.isin(tokens, module.cross_lingual_token_idx.to(tokens.device))


def f0_to_coarse(f0):
    """deployment/modules/fastspeech2.py:21-28."""
    f0_mel = 1127 * (1 + f0 / 700).log()
    a = (F0_BIN - 2) / (F0_MEL_MAX - F0_MEL_MIN)
    b = F0_MEL_MIN * a - 1.
    f0_mel = torch.where(f0_mel > 0, f0_mel * a - b, f0_mel)
    torch.clip_(f0_mel, min=1., max=float(F0_BIN - 1))
    return torch.round(f0_mel).long()


# ==================================================================================================== variance
class DiffSingerVarianceDeploy(DiffSingerVariance):
    """`DiffSingerVarianceONNX` (deployment/modules/toplevel.py:132-302) stage by stage."""

    def __init__(self, vocab_size, cross_lingual_token_idx=None):
        super().__init__(vocab_size=vocab_size)
        if not _cross_lingual(self, cross_lingual_token_idx):
            self.fs2.use_lang_id = False
        self.hidden_size = hparams['hidden_size']
        self.smooth = None                                  # (kernel size, taps) once build_smooth_op has run

    # ---- helpers of the twin ----------------------------------------------------------------------------
    def build_smooth_op(self, device=None):
        """toplevel.py:179-194: the taps are computed once per kernel size, on the host; `device` is accepted for parity."""
        k = round(hparams['midi_smooth_width'] * hparams['audio_sample_rate'] / hparams['hop_size'])
        if not 1 <= k <= 255:
            raise ValueError(f"midi smoothing kernel of {k} frames is outside [1, 255]")
        self.smooth = (k, smooth_kernel(k))

    def embed_frozen_spk(self, encoder_out):
        if hparams['use_spk_id'] and hasattr(self, 'frozen_spk_embed'):
            encoder_out += self.frozen_spk_embed.to(encoder_out.device)
        return encoder_out

    def _encode_tokens(self, tokens, gathers, terms, languages):
        fs2 = self.fs2
        bsz, n_ph = tokens.shape
        h = self.hidden_size
        gathers = [(fs2.txt_embed.weight, tokens, 0, math.sqrt(h))] + gathers
        if fs2.use_lang_id:
            gathers.append((fs2.lang_embed.weight, _masked_languages(self, tokens, languages), 0, 1.0))
        embed = assemble(bsz, n_ph, h, gathers, terms, tokens.device)
        x_masks = tokens == PAD_INDEX
        return self.embed_frozen_spk(fs2._encode(embed, x_masks, h)), x_masks

    # ---- stages ------------------------------------------------------------------------------------------
    def forward_linguistic_encoder_word(self, tokens, word_div, word_dur, languages=None):
        """-> encoder_out [B, T_ph, H], x_masks [B, T_ph] (fastspeech2.py:145-161)."""
        _check_infer(self)
        _device_index(tokens, "forward_linguistic_encoder_word")
        ph2word = length_regulate(word_div, tokens.shape[1])
        onset = ph2word > nn.functional.pad(ph2word, [1, -1])
        ph_word_dur = torch.gather(nn.functional.pad(word_dur, [1, 0]), 1, ph2word)
        return self._encode_tokens(tokens, [(self.fs2.onset_embed.weight, onset.long(), 0, 1.0)],
                                   lin1(self.fs2.word_dur_embed, ph_word_dur.float()), languages)

    def forward_linguistic_encoder_phoneme(self, tokens, ph_dur, languages=None):
        """-> encoder_out, x_masks (fastspeech2.py:163-176)."""
        _check_infer(self)
        _device_index(tokens, "forward_linguistic_encoder_phoneme")
        return self._encode_tokens(tokens, [], lin1(self.fs2.ph_dur_embed, ph_dur.float()), languages)

    def forward_dur_predictor(self, encoder_out, x_masks, ph_midi, spk_embed=None):
        """-> ph_dur_pred [B, T_ph] fp32 (fastspeech2.py:178-184)."""
        _check_infer(self)
        dev = encoder_out.device
        _device_index(encoder_out, "forward_dur_predictor")
        fs2 = self.fs2
        bsz, n_ph, h = encoder_out.shape
        gathers = [(encoder_out, _arange_idx(bsz, n_ph, dev), 0, 1.0), (fs2.midi_embed.weight, ph_midi, 0, 1.0)]
        if hparams['use_spk_id'] and spk_embed is not None:
            gathers.append(_spk_gather(spk_embed, bsz, n_ph, dev))
        dur_cond = assemble(bsz, n_ph, h, gathers, [], dev)
        handle = fs2.native_handle(dev)
        mask = x_masks.to(device=dev, dtype=torch.uint8).contiguous()
        dur = torch.empty((bsz, n_ph), device=dev, dtype=torch.float32)
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(handle, _lib.lib().dsd_predict_dur(handle, C.c_void_p(dur_cond.data_ptr()), C.c_void_p(mask.data_ptr()), bsz,
                                                      n_ph, C.c_void_p(dur.data_ptr()), C.c_void_p(stream)), "dsd_predict_dur")
        return dur

    def forward_mel2x_gather(self, x_src, x_dur, x_dim=None, t_len=None):
        """toplevel.py:214-222: x_src [B, L, x_dim] (or [B, L] with x_dim None) spread over the frames of x_dur."""
        mel2x = length_regulate(x_dur, t_len)
        if x_dim is None:
            return torch.gather(nn.functional.pad(x_src, [1, 0]), 1, mel2x)
        bsz, t_len = mel2x.shape
        return assemble(bsz, t_len, x_dim, [(x_src, mel2x, -1, 1.0)], [], x_src.device)

    def forward_pitch_preprocess(self, encoder_out, ph_dur, note_midi=None, note_rest=None, note_dur=None, note_glide=None,
                                 pitch=None, expr=None, retake=None, spk_embed=None, *, lengths=None):
        """-> pitch_cond [B, T, H], base_pitch [B, T] (toplevel.py:224-261).  T is `retake`'s; `lengths` [B] makes the
        smoothing of a zero-padded batch replicate at every item's own last frame."""
        _check_infer(self)
        dev = encoder_out.device
        _device_index(encoder_out, "forward_pitch_preprocess")
        bsz, t_len = retake.shape
        h = self.hidden_size
        gathers = [(encoder_out, length_regulate(ph_dur, t_len), -1, 1.0)]
        mel2note = length_regulate(note_dur, t_len)
        if self.use_melody_encoder:
            if self.melody_encoder.use_glide_embed and note_glide is None:
                note_glide = torch.zeros_like(note_dur)
            gathers.append((self.melody_encoder(note_midi, note_rest, note_dur, glide=note_glide), mel2note, -1, 1.0))
        # retake embedding: e * embed[1] + (1 - e) * embed[0]; with e in {0, 1} that is the lookup itself (:239-249)
        e = retake.float() if expr is None else (expr * retake).float().expand(bsz, t_len)
        emb = self.pitch_retake_embed.weight
        terms = [(e, emb[1]), (1.0 - e, emb[0])]
        if self.smooth is None:
            self.build_smooth_op(dev)
        base, blend, delta = frame_curve(note_midi, mel2note, pitch, retake, self.smooth[1], lengths)
        if self.use_melody_encoder:
            base_pitch = base
            terms += lin1(self.delta_pitch_embed, delta)
        else:
            base_pitch = blend
            terms += lin1(self.base_pitch_embed, blend)
        if hparams['use_spk_id'] and spk_embed is not None:
            gathers.append(_spk_gather(spk_embed, bsz, t_len, dev))
        return assemble(bsz, t_len, h, gathers, terms, dev), base_pitch

    def forward_pitch_reflow(self, pitch_cond, steps: int = 10, *, noise=None, step_noise=None):
        """-> x_pred [B, T], the mean over the bins, unclamped (toplevel.py:263-267); DDIM when diffusion_type is 'ddpm'."""
        return _sample(self.pitch_predictor, pitch_cond, steps, noise, step_noise)

    def forward_pitch_postprocess(self, x_pred, base_pitch):
        return self.pitch_predictor._post_denorm(x_pred) + base_pitch          # clamp_spec (toplevel.py:269-271)

    def forward_variance_preprocess(self, encoder_out, ph_dur, pitch, variances: dict = None, retake=None, spk_embed=None):
        """-> variance_cond [B, T, H] (toplevel.py:273-290); retake [B, T, V] bool, V in variance_prediction_list order."""
        _check_infer(self)
        dev = encoder_out.device
        _device_index(encoder_out, "forward_variance_preprocess")
        bsz, t_len = pitch.shape
        gathers = [(encoder_out, length_regulate(ph_dur, t_len), -1, 1.0)]
        terms = lin1(self.pitch_embed, pitch)
        keeps = (~retake).float().unbind(dim=2)             # non_retake_masks (:279-282)
        for name, keep in zip(self.variance_prediction_list, keeps):
            layer = self.variance_embeds[name]
            terms += [(variances[name] * keep, layer.weight.reshape(-1)), (keep, layer.bias)]
        if hparams['use_spk_id'] and spk_embed is not None:
            gathers.append(_spk_gather(spk_embed, bsz, t_len, dev))
        return assemble(bsz, t_len, self.hidden_size, gathers, terms, dev)

    def forward_variance_reflow(self, variance_cond, steps: int = 10, *, noise=None, step_noise=None):
        """-> xs_pred [B, T] (one variance) or [B, V, T] (toplevel.py:292-294)."""
        return _sample(self.variance_predictor, variance_cond, steps, noise, step_noise)

    def forward_variance_postprocess(self, xs_pred):
        xs = [xs_pred] if self.variance_predictor.num_feats == 1 else xs_pred.unbind(dim=1)
        return tuple(self.variance_predictor.clamp_spec(xs))


def _sample(predictor, cond, steps, noise, step_noise, **source):
    """The twin's sampler call, `predictor(cond, steps=steps[, x_start / x_end, depth])`, on `forward_onnx`."""
    if hasattr(predictor, "denoise_fn"):
        return predictor.forward_onnx(cond, steps=steps, noise=noise, step_noise=step_noise, **source)
    if step_noise is not None:
        raise ValueError("step_noise belongs to ancestral DDPM sampling; rectified flow draws x_T only")
    return predictor.forward_onnx(cond, steps=steps, noise=noise, **source)


# ==================================================================================================== acoustic
class _FastSpeech2AcousticDiscrete(FastSpeech2Acoustic):
    """`f0_embed_type: discrete` (fastspeech2.py:54-57, 92-94): `pitch_embed` is an Embedding(300, H) over f0_to_coarse.
    The native encoder's own Linear(1, H) pitch term is loaded as zeros; the lookup is added by `dsd_cond_assemble`."""

    def __init__(self, vocab_size):
        super().__init__(vocab_size=vocab_size)
        self.pitch_embed = nn.Embedding(300, self._hidden, PAD_INDEX)

    def _native_state(self):
        sd = dict(self.state_dict())
        sd["pitch_embed.weight"] = torch.zeros(self._hidden, 1)
        sd["pitch_embed.bias"] = torch.zeros(self._hidden)
        return sd


class DiffSingerAcousticDeploy(DiffSingerAcoustic):
    """`DiffSingerAcousticONNX` (deployment/modules/toplevel.py:20-103) with `FastSpeech2AcousticONNX.forward`
    (deployment/modules/fastspeech2.py:43-130) as its first stage."""

    def __init__(self, vocab_size, out_dims, cross_lingual_token_idx=None):
        super().__init__(vocab_size, out_dims)
        self.f0_embed_type = hparams.get('f0_embed_type', 'continuous')
        if self.f0_embed_type == 'discrete':
            del self.fs2
            self.fs2 = _FastSpeech2AcousticDiscrete(vocab_size=vocab_size)
        self.use_lang_id = _cross_lingual(self, cross_lingual_token_idx) and self.fs2.use_lang_id
        if hparams.get('use_key_shift_embed', False):
            self.shift_min, self.shift_max = hparams['augmentation_args']['random_pitch_shifting']['range']
        if hparams.get('use_speed_embed', False):
            self.speed_min, self.speed_max = hparams['augmentation_args']['random_time_stretching']['range']
        self.mel_base = hparams.get('mel_base', '10')

    def ensure_mel_base(self, mel):
        if self.mel_base != 'e':
            mel = mel * 2.30259                             # log10 mel to log mel (toplevel.py:55-59)
        return mel

    def _frozen(self, name):
        for owner in (self.fs2, self):
            if hasattr(owner, name):
                return getattr(owner, name)
        return None

    def forward_fs2_aux(self, tokens, durations, f0, variances: dict, gender=None, velocity=None, spk_embed=None,
                        languages=None):
        """-> condition [B, T, H] (, aux_mel_pred [B, T, M] with shallow diffusion) (toplevel.py:61-81).  T is f0's: the
        durations of every item total at most T, frames past an item's total are padding (mel2ph 0)."""
        _check_infer(self)
        dev = f0.device
        _device_index(f0, "forward_fs2_aux")
        fs2 = self.fs2
        bsz, t_len = f0.shape
        durations = durations * (tokens > 0)
        mel2ph = length_regulate(durations, t_len)
        f0 = f0 * (mel2ph > 0)
        kw = dict(variances or {})
        if self.use_lang_id:
            kw["languages"] = _masked_languages(self, tokens, languages)
        elif fs2.use_lang_id:           # a multilingual model without cross-lingual tokens: every token takes index 0,
            kw["languages"] = torch.zeros_like(tokens)      # lang_embed's padding row (zeros in a trained checkpoint)
        if fs2.use_key_shift_embed:
            frozen = self._frozen('frozen_key_shift')
            if frozen is not None:
                kw["key_shift"] = frozen.to(dev).reshape(-1, 1)
            else:
                gender = torch.clip(gender, min=-1., max=1.)
                gender_mask = (gender < 0.).float()
                kw["key_shift"] = gender * ((1. - gender_mask) * self.shift_max + gender_mask * abs(self.shift_min))
        if fs2.use_speed_embed:
            kw["speed"] = torch.ones((1, 1), device=dev) if velocity is None else \
                torch.clip(velocity, min=self.speed_min, max=self.speed_max)
        if fs2.use_spk_id:
            frozen = self._frozen('frozen_spk_embed')
            mix = frozen if frozen is not None else spk_embed
            if mix is None:
                raise ValueError("use_spk_id model: `spk_embed` [B, T or 1, H] (or a frozen_spk_embed) is required")
            kw["spk_mix_embed"] = mix.to(dev)
        discrete = self.f0_embed_type == 'discrete'
        condition = fs2(tokens, mel2ph, torch.zeros_like(f0) if discrete else f0, **kw)
        if discrete:
            condition = assemble(bsz, t_len, condition.shape[-1],
                                 [(condition, _arange_idx(bsz, t_len, dev), 0, 1.0),
                                  (fs2.pitch_embed.weight, f0_to_coarse(f0), 0, 1.0)], [], dev)
        if self.use_shallow_diffusion:
            return condition, self.aux_decoder(condition, infer=True)
        return condition

    def forward_shallow_diffusion(self, condition, x_start, depth, steps: int, *, noise=None, step_noise=None):
        return self.ensure_mel_base(_sample(self.diffusion, condition, steps, noise, step_noise, x_start=x_start, depth=depth))

    def forward_diffusion(self, condition, steps: int, *, noise=None, step_noise=None):
        return self.ensure_mel_base(_sample(self.diffusion, condition, steps, noise, step_noise))

    def forward_shallow_reflow(self, condition, x_end, depth, steps: int, *, noise=None):
        return self.ensure_mel_base(_sample(self.diffusion, condition, steps, noise, None, x_end=x_end, depth=depth))

    def forward_reflow(self, condition, steps: int, *, noise=None):
        return self.ensure_mel_base(_sample(self.diffusion, condition, steps, noise, None))
