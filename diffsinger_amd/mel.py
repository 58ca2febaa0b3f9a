"""Mel analysis on libdsdenoise: waveform -> natural-log mel (drop-in for `modules/nsf_hifigan/nvSTFT.py:STFT` and
`utils/binarizer_utils.py:get_mel_torch`).

`STFT(sr, n_mels, n_fft, win_size, hop_length, fmin, fmax, clip_val)` takes nvSTFT.STFT's constructor arguments and
defaults; `get_mel(y, keyshift, speed)` is STFT.get_mel with center=False (the only form the reference calls) on a
[B, L] waveform on the GPU, and returns [B, n_mels, T] - what `vocoder.Generator.forward` takes.  `get_mel_ragged`
analyses segments of different lengths in one call, each exactly as a lone call would.  The filterbank is the library's
restatement of librosa.filters.mel (Slaney scale and normalisation, float32; `mel_filterbank`).  No CPU path.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib


def _config(sr, n_fft, win_size, hop_length, n_mels, fmin, fmax, clip_val=1e-5, device=0):
    fmax = float(sr) / 2 if fmax is None else float(fmax)
    return _lib.DsdMelConfig(C.sizeof(_lib.DsdMelConfig), int(sr), int(n_fft), int(win_size), int(hop_length), int(n_mels),
                             float(fmin), fmax, float(clip_val), int(device))


def mel_filterbank(sr, n_fft, n_mels, fmin, fmax):
    """librosa.filters.mel(sr=sr, n_fft=n_fft, n_mels=n_mels, fmin=fmin, fmax=fmax): [n_mels, n_fft // 2 + 1] float32."""
    cfg = _config(sr, n_fft, n_fft, 1, n_mels, fmin, fmax)
    out = np.zeros((int(n_mels), int(n_fft) // 2 + 1), dtype=np.float32)
    rc = _lib.lib().dsd_mel_filterbank(C.byref(cfg), out.ctypes.data_as(C.POINTER(C.c_float)))
    if rc != 0:
        raise ValueError(f"dsd_mel_filterbank failed ({rc}): {_lib.lib().dsd_last_error(None).decode()}")
    return out


class STFT:
    def __init__(self, sr=22050, n_mels=80, n_fft=1024, win_size=1024, hop_length=256, fmin=20, fmax=11025, clip_val=1e-5,
                 device=None):
        self.target_sr = sr
        self.n_mels = n_mels
        self.n_fft = n_fft
        self.win_size = win_size
        self.hop_length = hop_length
        self.fmin = fmin
        self.fmax = fmax
        self.clip_val = clip_val
        self.device = torch.device("cuda" if device is None else device)
        self._handles = {}

    def _cfg(self, device_index=0):
        return _config(self.target_sr, self.n_fft, self.win_size, self.hop_length, self.n_mels, self.fmin, self.fmax,
                       self.clip_val, device_index)

    def num_frames(self, n_samples, keyshift=0, speed=1):
        cfg = self._cfg()
        t = _lib.lib().dsd_mel_num_frames(C.byref(cfg), int(n_samples), float(keyshift), float(speed))
        if t < 1:
            raise ValueError(f"{n_samples} samples are too short for keyshift={keyshift}, speed={speed}: "
                             f"{_lib.lib().dsd_last_error(None).decode()}")
        return int(t)

    def _handle(self, device):
        if device.type != "cuda":
            raise RuntimeError(f"diffsinger_amd.mel.STFT runs only on an MI355X (HIP) device; got a {device.type} tensor. "
                               "There is no CPU path - use the reference module for CPU.")
        idx = device.index if device.index is not None else torch.cuda.current_device()
        if idx not in self._handles:
            cfg = self._cfg(idx)
            hp = C.c_void_p()
            rc = _lib.lib().dsd_mel_create(C.byref(cfg), C.byref(hp))
            if rc != 0:
                raise _lib.NativeLibraryError(f"dsd_mel_create failed ({rc}): {_lib.lib().dsd_last_error(None).decode()}")
            self._handles[idx] = hp
        return self._handles[idx]

    def __del__(self):
        try:
            for hp in self._handles.values():
                _lib.lib().dsd_destroy(hp)
        except Exception:      # interpreter shutdown
            pass
        self._handles = {}

    def _analyze(self, y, lengths, keyshift, speed, out):
        handle = self._handle(y.device)
        stream = torch.cuda.current_stream(y.device).cuda_stream
        b, n = y.shape
        lens = None if lengths is None else (C.c_int64 * b)(*[int(v) for v in lengths])
        sb, sm, st_ = out.stride()
        _lib.check(handle, _lib.lib().dsd_mel_analyze(handle, C.c_void_p(y.data_ptr()), b, n, y.stride(0), lens,
                                                       float(keyshift), float(speed), C.c_void_p(out.data_ptr()),
                                                       sb, sm, st_, C.c_void_p(stream)), "dsd_mel_analyze")

    @staticmethod
    def _prepare(y):
        if not torch.is_tensor(y) or y.dim() != 2:
            raise ValueError("y must be a [B, L] tensor")
        if y.device.type != "cuda":
            raise RuntimeError(f"diffsinger_amd.mel.STFT runs only on an MI355X (HIP) device; got a {y.device.type} tensor. "
                               "There is no CPU path - use the reference module for CPU.")
        return y.to(torch.float32).contiguous()

    def get_mel(self, y, keyshift=0, speed=1, center=False, out=None):
        """nvSTFT.py:50-87: y [B, L] -> [B, n_mels, T].  `out` may be any [B, n_mels, T] view (e.g. a transposed
        [B, T, n_mels] tensor)."""
        if center:
            raise NotImplementedError("center=True: no reference caller uses it (nvSTFT.STFT.get_mel is called with center=False)")
        y = self._prepare(y)
        t = self.num_frames(y.shape[1], keyshift, speed)
        if out is None:
            out = torch.empty(y.shape[0], self.n_mels, t, device=y.device, dtype=torch.float32)
        elif tuple(out.shape) != (y.shape[0], self.n_mels, t) or out.dtype != torch.float32 or out.device != y.device:
            raise ValueError(f"out must be a float32 [{y.shape[0]}, {self.n_mels}, {t}] tensor on {y.device}")
        with torch.no_grad():
            self._analyze(y, None, keyshift, speed, out)
        return out

    def get_mel_ragged(self, waveforms, keyshift=0, speed=1):
        """One library call over segments of different lengths: a list of 1-D waveforms -> a list of [n_mels, T_b],
        each equal to get_mel on that waveform alone."""
        if not waveforms:
            return []
        if any(w.dim() != 1 for w in waveforms):
            raise ValueError("get_mel_ragged takes a list of 1-D waveforms")
        lengths = [int(w.shape[0]) for w in waveforms]
        frames = [self.num_frames(n, keyshift, speed) for n in lengths]
        dev = waveforms[0].device
        y = torch.zeros(len(waveforms), max(lengths), device=dev, dtype=torch.float32)
        for i, w in enumerate(waveforms):
            y[i, : lengths[i]] = w
        y = self._prepare(y)
        out = torch.empty(len(waveforms), self.n_mels, max(frames), device=dev, dtype=torch.float32)
        with torch.no_grad():
            self._analyze(y, lengths, keyshift, speed, out)
        return [out[i, :, : frames[i]] for i in range(len(waveforms))]


def get_mel_torch(waveform, samplerate, *, num_mel_bins=128, hop_size=512, win_size=2048, fft_size=2048, fmin=40,
                  fmax=16000, keyshift=0, speed=1, device=None):
    """utils/binarizer_utils.py:13-26: numpy waveform -> numpy [T, num_mel_bins] log-mel."""
    dev = torch.device("cuda" if device is None else device)
    stft = STFT(samplerate, num_mel_bins, fft_size, win_size, hop_size, fmin, fmax, device=dev)
    wav = torch.from_numpy(np.ascontiguousarray(waveform, dtype=np.float32)).to(dev)
    mel = stft.get_mel(wav.unsqueeze(0), keyshift=keyshift, speed=speed).squeeze(0).T
    return mel.cpu().numpy()
