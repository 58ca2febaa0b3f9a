"""The variance model's staged twin as a C program drives it (include/dsdenoise.h, dsd_variance_open .. dsd_variance_post),
from Python.

`Variance(file, prefix, device)` opens the object from a model file (`modelfile.variance_sections` packs one) and exposes
the stage calls on torch tensors, one method per C call with the argument names of `deploy.DiffSingerVarianceDeploy`, which
stays the path of the Python shims and the yardstick these calls are tested against.  `sample` is the sampler stage a C
caller writes itself - dsd_prepare_cond + dsd_program_build + dsd_sample on the borrowed handle - and returns what the
post stages take: the denormalised sample before the mean over the bins.  No CPU path.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, cprogram

NAMES = ("energy", "breathiness", "voicing", "tension")        # the order of the DSD_EMBED_* bits


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _as(t, dtype, device):
    return None if t is None else t.detach().to(device=device, dtype=dtype).contiguous()


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class Variance:
    def __init__(self, file, prefix, device=0):
        self._v = None
        dev = torch.device(device if not isinstance(device, int) else f"cuda:{device}")
        if dev.type != "cuda":
            raise RuntimeError(f"diffsinger_amd.cvariance runs only on an MI355X (HIP) device; got {dev.type}. There is no CPU path.")
        self.device = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        vp = C.c_void_p()
        _lib.check(None, _lib.lib().dsd_variance_open(file._f, str(prefix).encode(), self.device.index, C.byref(vp)), "dsd_variance_open")
        self._v = vp
        self.cfg = _lib.DsdVarianceConfig()
        _lib.check(None, _lib.lib().dsd_variance_info(self._v, C.byref(self.cfg)), "dsd_variance_info")
        self.names = [n for i, n in enumerate(NAMES) if self.cfg.variances >> i & 1]
        self._programs = {}

    def close(self):
        if self._v is not None:
            for entry in self._programs.values():
                _lib.lib().dsd_program_free(entry[0])
            self._programs = {}
            _lib.lib().dsd_variance_close(self._v)
            self._v = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:      # interpreter shutdown
            pass

    def backbone(self, which):
        """the borrowed denoiser handle: _lib.DSD_VAR_PITCH or _lib.DSD_VAR_VARIANCES"""
        hp = C.c_void_p()
        _lib.check(None, _lib.lib().dsd_variance_backbone(self._v, int(which), C.byref(hp)), "dsd_variance_backbone")
        return hp

    def spk_mix(self, ids, values, normalize=False, out=None):
        """dsd_variance_spk_mix: ids [B, N] ints (host), values [B, rows, N] -> [B, rows, H], what `dur` (rows 1 or L) and
        `pitch_cond` / `cond` (rows 1 or T) take as spk_embed"""
        from .cacoustic import _spk_mix
        return _spk_mix(_lib.lib().dsd_variance_spk_mix, "dsd_variance_spk_mix", self._v, self.device, self.cfg.hidden_size, ids,
                        values, normalize, out)

    def set_lengths(self, lengths):
        """dsd_variance_set_lengths: B frame counts for the following pitch_cond / cond / post calls and both denoisers, or
        None for dense batches"""
        if lengths is None:
            arr, n = None, 0
        else:
            lens = [int(v) for v in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
            arr, n = (C.c_int32 * len(lens))(*lens), len(lens)
        _lib.check(None, _lib.lib().dsd_variance_set_lengths(self._v, arr, n, _stream(self.device)), "dsd_variance_set_lengths")

    # ---- stages ------------------------------------------------------------------------------------------
    def encode(self, tokens, word_div=None, word_dur=None, ph_dur=None, languages=None, want_ph2word=False):
        """-> encoder_out [B, L, H], x_masks [B, L] bool (, ph2word [B, L])"""
        d, i64 = self.device, torch.int64
        tokens = _as(tokens, i64, d)
        bsz, n_ph = tokens.shape
        keep = [tokens] + [_as(t, i64, d) for t in (word_div, word_dur, ph_dur, languages)]
        enc = torch.empty((bsz, n_ph, self.cfg.hidden_size), device=d, dtype=torch.float32)
        masks = torch.empty((bsz, n_ph), device=d, dtype=torch.uint8)
        ph2word = torch.empty((bsz, n_ph), device=d, dtype=i64) if want_ph2word else None
        a = _lib.DsdVarianceEncodeArgs(C.sizeof(_lib.DsdVarianceEncodeArgs), bsz, n_ph, 0 if word_div is None else word_div.shape[1],
                                       *[_ptr(t) for t in keep], _ptr(enc), _ptr(masks), _ptr(ph2word))
        _lib.check(None, _lib.lib().dsd_variance_encode(self._v, C.byref(a), _stream(d)), "dsd_variance_encode")
        return (enc, masks.bool(), ph2word) if want_ph2word else (enc, masks.bool())

    def dur(self, encoder_out, x_masks, ph_midi, spk_embed=None):
        """-> ph_dur_pred [B, L] fp32"""
        d = self.device
        enc, masks = _as(encoder_out, torch.float32, d), _as(x_masks, torch.uint8, d)
        midi, spk = _as(ph_midi, torch.int64, d), _as(spk_embed, torch.float32, d)
        bsz, n_ph, _ = enc.shape
        out = torch.empty((bsz, n_ph), device=d, dtype=torch.float32)
        a = _lib.DsdVarianceDurArgs(C.sizeof(_lib.DsdVarianceDurArgs), bsz, n_ph, _ptr(enc), _ptr(masks), _ptr(midi), _ptr(spk),
                                    0 if spk is None else spk.shape[1], _ptr(out))
        _lib.check(None, _lib.lib().dsd_variance_dur(self._v, C.byref(a), _stream(d)), "dsd_variance_dur")
        return out

    def pitch_cond(self, encoder_out, ph_dur, note_midi, note_rest, note_dur, note_glide=None, pitch=None, expr=None, retake=None,
                   spk_embed=None, lengths=None, out=None):
        """-> pitch_cond [B, T, H], base_pitch [B, T]; T is `retake`'s.  `out`: (pitch_cond, base_pitch) to write into."""
        d, f32, i64 = self.device, torch.float32, torch.int64
        retake = _as(retake, torch.uint8, d)
        bsz, t_len = retake.shape
        enc, ph_dur, note_midi = _as(encoder_out, f32, d), _as(ph_dur, i64, d), _as(note_midi, f32, d)
        note_rest, note_dur, note_glide = _as(note_rest, torch.uint8, d), _as(note_dur, i64, d), _as(note_glide, i64, d)
        pitch = pitch.detach().to(device=d, dtype=f32).expand(bsz, t_len).contiguous()
        expr = None if expr is None else expr.detach().to(device=d, dtype=f32).expand(bsz, t_len).contiguous()
        spk = _as(spk_embed, f32, d)
        lens = None
        if lengths is not None:
            lens = (C.c_int32 * bsz)(*[int(x) for x in (lengths.tolist() if torch.is_tensor(lengths) else lengths)])
        cond, base = out if out is not None else (torch.empty((bsz, t_len, self.cfg.hidden_size), device=d, dtype=f32),
                                                  torch.empty((bsz, t_len), device=d, dtype=f32))
        a = _lib.DsdVariancePitchCondArgs(C.sizeof(_lib.DsdVariancePitchCondArgs), bsz, enc.shape[1], note_midi.shape[1], t_len, _ptr(enc),
                                          _ptr(ph_dur), _ptr(note_midi), _ptr(note_rest), _ptr(note_dur), _ptr(note_glide), _ptr(pitch),
                                          _ptr(expr), _ptr(retake), _ptr(spk), 0 if spk is None else spk.shape[1], lens, _ptr(cond),
                                          _ptr(base))
        self._keep = (enc, ph_dur, note_midi, note_rest, note_dur, note_glide, pitch, expr, retake, spk)       # a captured graph reads them
        _lib.check(None, _lib.lib().dsd_variance_pitch_cond(self._v, C.byref(a), _stream(d)), "dsd_variance_pitch_cond")
        return cond, base

    def cond(self, encoder_out, ph_dur, pitch, variances, retake, spk_embed=None):
        """-> variance_cond [B, T, H]; variances: {name: [B, T]}, retake [B, T, V] bool"""
        d, f32 = self.device, torch.float32
        pitch = _as(pitch, f32, d)
        bsz, t_len = pitch.shape
        enc, ph_dur, spk = _as(encoder_out, f32, d), _as(ph_dur, torch.int64, d), _as(spk_embed, f32, d)
        retake = _as(retake, torch.uint8, d)
        curves = [_as(variances[n], f32, d) for n in self.names]
        out = torch.empty((bsz, t_len, self.cfg.hidden_size), device=d, dtype=f32)
        a = _lib.DsdVarianceCondArgs(C.sizeof(_lib.DsdVarianceCondArgs), bsz, enc.shape[1], t_len, _ptr(enc), _ptr(ph_dur), _ptr(pitch),
                                     (C.c_void_p * 4)(*[c.data_ptr() for c in curves]), _ptr(retake), _ptr(spk),
                                     0 if spk is None else spk.shape[1], _ptr(out))
        _lib.check(None, _lib.lib().dsd_variance_cond(self._v, C.byref(a), _stream(d)), "dsd_variance_cond")
        return out

    def pitch_post(self, sample, base_pitch, out=None):
        """sample [B, T, M] -> pitch_pred [B, T]"""
        d = self.device
        sample, base = _as(sample, torch.float32, d), _as(base_pitch, torch.float32, d)
        bsz, t_len = base.shape
        out = torch.empty((bsz, t_len), device=d, dtype=torch.float32) if out is None else out
        _lib.check(None, _lib.lib().dsd_variance_pitch_post(self._v, _ptr(sample), _ptr(base), bsz, t_len, _ptr(out), _stream(d)),
                   "dsd_variance_pitch_post")
        return out

    def post(self, sample):
        """sample [B, V, T, M] ([B, T, M] for one variance) -> {name: [B, T]}"""
        d = self.device
        sample = _as(sample, torch.float32, d)
        bsz, t_len = sample.shape[0], sample.shape[-2]
        outs = [torch.empty((bsz, t_len), device=d, dtype=torch.float32) for _ in self.names]
        ptrs = (C.c_void_p * 4)(*[o.data_ptr() for o in outs])
        _lib.check(None, _lib.lib().dsd_variance_post(self._v, _ptr(sample), bsz, t_len, ptrs, _stream(d)), "dsd_variance_post")
        return dict(zip(self.names, outs))

    # ---- the sampler stage, as a C caller writes it ---------------------------------------------------
    def affine(self, which):
        """(out_scale, out_shift) [F * M] of dsd_sample's DSD_SAMPLE_TRANSPOSE, from the config: k = (max - min) / 2 and
        b = (max + min) / 2 in fp32, the twins' x * k + b"""
        c = self.cfg
        if which == _lib.DSD_VAR_PITCH:
            lo, hi, m = np.float32([c.pitd_norm_min]), np.float32([c.pitd_norm_max]), c.pitch_repeat_bins
        else:
            slots = [NAMES.index(n) for n in self.names]
            lo, hi, m = np.float32([c.var_norm_min[s] for s in slots]), np.float32([c.var_norm_max[s] for s in slots]), c.var_repeat_bins
        k, b = (hi - lo) / np.float32(2), (hi + lo) / np.float32(2)
        return (torch.from_numpy(np.repeat(k, m)).to(self.device), torch.from_numpy(np.repeat(b, m)).to(self.device))

    def sample(self, which, cond, steps, noise, out=None):
        """Rectified flow, the twin's euler loop (DSD_SAMPLER_RF_EULER_ONNX) from x_T = noise [B, F, M, T] on `cond` [B, T, H]
        -> the denormalised sample [B, T, M] / [B, F, T, M]."""
        if self.cfg.diffusion_type != _lib.DSD_DIFFUSE_REFLOW:
            raise NotImplementedError("Variance.sample builds the rectified-flow program; a DDPM model's is the caller's")
        h = self.backbone(which)
        d = self.device
        cond, noise = _as(cond, torch.float32, d), _as(noise, torch.float32, d)
        bsz, t_len, hid = cond.shape
        _, f, m, _ = noise.shape
        key = (which, int(steps))
        if key not in self._programs:
            s, _ = cprogram.spec("rf_euler_onnx", steps=steps, t_start=0.0, time_scale_factor=self.cfg.time_scale_factor)
            p = C.POINTER(_lib.DsdProgram)()
            _lib.check(None, _lib.lib().dsd_program_build(C.byref(s), C.byref(p)), "dsd_program_build")
            self._programs[key] = (p,) + self.affine(which)
        prog, scale, shift = self._programs[key]
        out = torch.empty((bsz, t_len, m) if f == 1 else (bsz, f, t_len, m), device=d, dtype=torch.float32) if out is None else out
        st = _stream(d)
        _lib.check(h, _lib.lib().dsd_prepare_cond(h, _ptr(cond), bsz, t_len, t_len * hid, 1, hid, st), "dsd_prepare_cond")
        _lib.check(h, _lib.lib().dsd_sample(h, prog, _ptr(noise), None, _ptr(out), _ptr(scale), _ptr(shift), _lib.DSD_SAMPLE_TRANSPOSE, st),
                   "dsd_sample")
        return out
