"""RMVPE pitch extraction on libdsdenoise (drop-in for `modules/pe/rmvpe/`: `RMVPE`, `E2E0`).

`RMVPE(model_path_or_state_dict)` runs waveform -> f0 on the GPU: the resampler to 16 kHz, the HTK log-mel, E2E0 and
to_local_average_f0 are HIP kernels (rmvpe_kernels.hip, mel_kernels.hip); get_pitch's post-processing is numpy on the
host, as in the reference.  `decode_viterbi` / `use_viterbi=True` is to_viterbi_f0: librosa.sequence.viterbi restated as
a HIP kernel in double.  `infer_from_audio_ragged` extracts the f0 of clips of different lengths in one call, each
exactly as a lone call would.  `E2E0` is the reference's torch module (same module and state_dict names): the weight
container of synthetic checkpoints and the torch restatement tools/time_pitch.py times against.  No CPU path.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch
from torch import nn

from . import _lib
from .harness import resample_align_curve
from .variance_harness import interp_f0

SAMPLE_RATE, N_CLASS, N_MELS = 16000, 360, 128


# ---------------------------------------------------------------------------------------------------------------- E2E0
class ConvBlockRes(nn.Module):
    def __init__(self, in_channels, out_channels, momentum=0.01):
        super().__init__()
        self.conv = nn.Sequential(
            nn.Conv2d(in_channels, out_channels, (3, 3), (1, 1), (1, 1), bias=False),
            nn.BatchNorm2d(out_channels, momentum=momentum), nn.ReLU(),
            nn.Conv2d(out_channels, out_channels, (3, 3), (1, 1), (1, 1), bias=False),
            nn.BatchNorm2d(out_channels, momentum=momentum), nn.ReLU())
        self.is_shortcut = in_channels != out_channels
        if self.is_shortcut:
            self.shortcut = nn.Conv2d(in_channels, out_channels, (1, 1))

    def forward(self, x):
        return self.conv(x) + (self.shortcut(x) if self.is_shortcut else x)


class ResEncoderBlock(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size, n_blocks=1, momentum=0.01):
        super().__init__()
        self.conv = nn.ModuleList([ConvBlockRes(in_channels if i == 0 else out_channels, out_channels, momentum)
                                   for i in range(n_blocks)])
        self.kernel_size = kernel_size
        if kernel_size is not None:
            self.pool = nn.AvgPool2d(kernel_size=kernel_size)

    def forward(self, x):
        for c in self.conv:
            x = c(x)
        return (x, self.pool(x)) if self.kernel_size is not None else x


class ResDecoderBlock(nn.Module):
    def __init__(self, in_channels, out_channels, stride, n_blocks=1, momentum=0.01):
        super().__init__()
        out_padding = (0, 1) if stride == (1, 2) else (1, 1)
        self.conv1 = nn.Sequential(
            nn.ConvTranspose2d(in_channels, out_channels, (3, 3), stride, (1, 1), out_padding, bias=False),
            nn.BatchNorm2d(out_channels, momentum=momentum), nn.ReLU())
        self.conv2 = nn.ModuleList([ConvBlockRes(out_channels * 2 if i == 0 else out_channels, out_channels, momentum)
                                    for i in range(n_blocks)])

    def forward(self, x, concat_tensor):
        x = torch.cat((self.conv1(x), concat_tensor), dim=1)
        for c in self.conv2:
            x = c(x)
        return x


class Encoder(nn.Module):
    def __init__(self, in_channels, in_size, n_encoders, kernel_size, n_blocks, out_channels=16, momentum=0.01):
        super().__init__()
        self.bn = nn.BatchNorm2d(in_channels, momentum=momentum)
        self.layers = nn.ModuleList()
        self.latent_channels = []
        for _ in range(n_encoders):
            self.layers.append(ResEncoderBlock(in_channels, out_channels, kernel_size, n_blocks, momentum=momentum))
            self.latent_channels.append([out_channels, in_size])
            in_channels, out_channels, in_size = out_channels, out_channels * 2, in_size // 2
        self.out_size, self.out_channel = in_size, out_channels

    def forward(self, x):
        skips = []
        x = self.bn(x)
        for layer in self.layers:
            s, x = layer(x)
            skips.append(s)
        return x, skips


class Intermediate(nn.Module):
    def __init__(self, in_channels, out_channels, n_inters, n_blocks, momentum=0.01):
        super().__init__()
        self.layers = nn.ModuleList([ResEncoderBlock(in_channels if i == 0 else out_channels, out_channels, None, n_blocks,
                                                     momentum) for i in range(n_inters)])

    def forward(self, x):
        for layer in self.layers:
            x = layer(x)
        return x


class TimbreFilter(nn.Module):
    def __init__(self, latent_rep_channels):
        super().__init__()
        self.layers = nn.ModuleList([ConvBlockRes(c[0], c[0]) for c in latent_rep_channels])


class Decoder(nn.Module):
    def __init__(self, in_channels, n_decoders, stride, n_blocks, momentum=0.01):
        super().__init__()
        self.layers = nn.ModuleList()
        for _ in range(n_decoders):
            self.layers.append(ResDecoderBlock(in_channels, in_channels // 2, stride, n_blocks, momentum))
            in_channels //= 2

    def forward(self, x, skips):
        for i, layer in enumerate(self.layers):
            x = layer(x, skips[-1 - i])
        return x


class DeepUnet0(nn.Module):
    def __init__(self, kernel_size, n_blocks, en_de_layers=5, inter_layers=4, in_channels=1, en_out_channels=16):
        super().__init__()
        self.encoder = Encoder(in_channels, N_MELS, en_de_layers, kernel_size, n_blocks, en_out_channels)
        self.intermediate = Intermediate(self.encoder.out_channel // 2, self.encoder.out_channel, inter_layers, n_blocks)
        self.tf = TimbreFilter(self.encoder.latent_channels)
        self.decoder = Decoder(self.encoder.out_channel, en_de_layers, kernel_size, n_blocks)

    def forward(self, x):
        x, skips = self.encoder(x)
        return self.decoder(self.intermediate(x), skips)


class BiGRU(nn.Module):
    def __init__(self, input_features, hidden_features, num_layers):
        super().__init__()
        self.gru = nn.GRU(input_features, hidden_features, num_layers=num_layers, batch_first=True, bidirectional=True)

    def forward(self, x):
        return self.gru(x)[0]


class E2E0(nn.Module):
    """modules/pe/rmvpe/model.py:8-31 (torch; the GPU path is RMVPE below)."""

    def __init__(self, n_blocks, n_gru, kernel_size, en_de_layers=5, inter_layers=4, in_channels=1, en_out_channels=16):
        super().__init__()
        self.config = dict(n_blocks=n_blocks, n_gru=n_gru, en_de_layers=en_de_layers, inter_layers=inter_layers,
                           en_out_channels=en_out_channels)
        self.unet = DeepUnet0(kernel_size, n_blocks, en_de_layers, inter_layers, in_channels, en_out_channels)
        self.cnn = nn.Conv2d(en_out_channels, 3, (3, 3), padding=(1, 1))
        if n_gru:
            self.fc = nn.Sequential(BiGRU(3 * N_MELS, 256, n_gru), nn.Linear(512, N_CLASS), nn.Dropout(0.25), nn.Sigmoid())
        else:
            self.fc = nn.Sequential(nn.Linear(3 * N_MELS, N_CLASS), nn.Dropout(0.25), nn.Sigmoid())

    def forward(self, mel):
        mel = mel.transpose(-1, -2).unsqueeze(1)
        return self.fc(self.cnn(self.unet(mel)).transpose(1, 2).flatten(-2))


# ---------------------------------------------------------------------------------------------------------------- GPU path
def rmvpe_filterbank():
    """librosa.filters.mel(sr=16000, n_fft=1024, n_mels=128, fmin=30, fmax=8000, htk=True): [128, 513] float32."""
    out = np.zeros((N_MELS, 513), dtype=np.float32)
    rc = _lib.lib().dsd_rmvpe_filterbank(out.ctypes.data_as(C.POINTER(C.c_float)))
    if rc != 0:
        raise ValueError(f"dsd_rmvpe_filterbank failed ({rc})")
    return out


def num_frames(n_samples, sample_rate=SAMPLE_RATE):
    """Frames RMVPE.infer_from_audio gives for n_samples samples at sample_rate (1 + L16 // 160)."""
    t = _lib.lib().dsd_rmvpe_num_frames(int(n_samples), int(sample_rate))
    if t < 1:
        raise ValueError(f"{n_samples} samples at {sample_rate} Hz are too short: {_lib.lib().dsd_last_error(None).decode()}")
    return int(t)


def _config_of(sd):
    E = len({k.split(".")[3] for k in sd if k.startswith("unet.encoder.layers.")})
    nb = len({k.split(".")[5] for k in sd if k.startswith("unet.encoder.layers.0.conv.")})
    inter = len({k.split(".")[3] for k in sd if k.startswith("unet.intermediate.layers.")})
    return dict(n_blocks=nb, n_gru=int("fc.0.gru.weight_ih_l0" in sd), en_de_layers=E, inter_layers=inter,
                en_out_channels=int(sd["cnn.weight"].shape[1]))


class RMVPE:
    """modules/pe/rmvpe/inference.py:RMVPE on the MI355X.  `model_path_or_state_dict`: a checkpoint path (its ['model'],
    read with weights_only) or a state_dict; the architecture is read off the names (the reference always builds
    E2E0(4, 1, (2, 2)))."""

    def __init__(self, model_path_or_state_dict, hop_length=160, device=None):
        if hop_length != 160:
            raise NotImplementedError("hop_length != 160: the reference's RMVPE is trained at hop 160 and no caller changes it")
        sd = model_path_or_state_dict
        if not isinstance(sd, dict):
            sd = torch.load(sd, map_location="cpu", weights_only=True)["model"]
        self.device = torch.device("cuda" if device is None else device)
        if self.device.type != "cuda":
            raise RuntimeError("diffsinger_amd.pitch.RMVPE runs only on an MI355X (HIP) device; there is no CPU path")
        self.config = _config_of(sd)
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", idx)
        cfg = self._native_config(idx)
        hp = C.c_void_p()
        rc = _lib.lib().dsd_rmvpe_create(C.byref(cfg), C.byref(hp))
        if rc != 0:
            raise _lib.NativeLibraryError(f"dsd_rmvpe_create failed ({rc}): {_lib.lib().dsd_last_error(None).decode()}")
        self._h = hp
        self._sd = sd
        _lib.load_state_dict(hp, sd)

    # -- model files (diffsinger_amd/modelfile.py: section_of / attach) --------------------------------------------------
    def _native_config(self, device_index):
        return _lib.DsdRmvpeConfig(C.sizeof(_lib.DsdRmvpeConfig), self.config["n_blocks"], self.config["n_gru"],
                                   self.config["en_de_layers"], self.config["inter_layers"], self.config["en_out_channels"],
                                   device_index)

    def _native_tensors(self):
        """name -> tensor of what the handle loaded"""
        return dict(self._sd)

    def _install_native(self, handle, sd, device):
        """run on `handle` (finalized, of this configuration, on `device`) from now on; `sd` is what it holds"""
        _lib.lib().dsd_destroy(self._h)
        self._h, self._sd, self.device = handle, sd, device

    def __del__(self):
        try:
            _lib.lib().dsd_destroy(self._h)
        except Exception:      # interpreter shutdown, or a failed constructor
            pass

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    @torch.no_grad()
    def mel2hidden(self, mel, lengths=None):
        """inference.py:24-29: mel [B, 128, T] (any strides) -> hidden [B, T, 360] on the GPU."""
        mel = torch.as_tensor(mel, dtype=torch.float32, device=self.device)
        b, m, t = mel.shape
        if m != N_MELS:
            raise ValueError(f"mel must be [B, {N_MELS}, T]")
        out = torch.zeros(b, t, N_CLASS, device=self.device)
        lens = None if lengths is None else (C.c_int64 * b)(*[int(v) for v in lengths])
        _lib.check(self._h, _lib.lib().dsd_rmvpe_mel_to_hidden(self._h, C.c_void_p(mel.data_ptr()), b, t, *mel.stride(), lens,
                                                            C.c_void_p(out.data_ptr()), t * N_CLASS, N_CLASS, self._stream()),
                   "dsd_rmvpe_mel_to_hidden")
        return out

    def _hidden(self, hidden):
        h = torch.as_tensor(hidden, dtype=torch.float32, device=self.device)
        if h.dim() == 2:
            h = h[None]
        return h.contiguous()

    @torch.no_grad()
    def decode(self, hidden, thred=0.03, use_viterbi=False, center=None):
        """to_local_average_f0 on hidden [B, T, 360] (or [T, 360]) -> f0 numpy [B, T] ([T] for B = 1, as the reference's
        .squeeze(0)).  `center` [B, T] (or [T]) integers: the window sits around them instead of the argmax
        (to_local_average_f0(hidden, center=...)).  The Viterbi decode is `decode_viterbi`."""
        if use_viterbi:
            raise NotImplementedError("decode(use_viterbi=True) is spelled decode_viterbi(hidden, thred) here "
                                      "(librosa.sequence.viterbi restated on the GPU)")
        h = self._hidden(hidden)
        b, t, _ = h.shape
        f0 = torch.empty(b, t, device=self.device)
        if center is None:
            _lib.check(self._h, _lib.lib().dsd_rmvpe_decode(self._h, C.c_void_p(h.data_ptr()), b, t, t * N_CLASS, N_CLASS,
                                                            float(thred), C.c_void_p(f0.data_ptr()), t, self._stream()),
                       "dsd_rmvpe_decode")
        else:
            c = torch.as_tensor(center, device=self.device).to(torch.int32).reshape(b, t).contiguous()
            _lib.check(self._h, _lib.lib().dsd_rmvpe_decode_at(self._h, C.c_void_p(h.data_ptr()), C.c_void_p(c.data_ptr()), b, t,
                                                               t * N_CLASS, N_CLASS, t, float(thred),
                                                               C.c_void_p(f0.data_ptr()), t, self._stream()),
                       "dsd_rmvpe_decode_at")
        f0 = f0.cpu().numpy()
        return f0[0] if b == 1 else f0

    def _viterbi(self, h, lengths, thred, f0, path=None):
        """dsd_rmvpe_decode_viterbi on device tensors: hidden h [B, T, 360] (contiguous) -> f0 [B, T] (and the int32 path
        [B, T]); frames at or past lengths[b] are left as they are."""
        b, t, _ = h.shape
        lens = None if lengths is None else (C.c_int64 * b)(*[int(v) for v in lengths])
        _lib.check(self._h, _lib.lib().dsd_rmvpe_decode_viterbi(
            self._h, C.c_void_p(h.data_ptr()), b, t, t * N_CLASS, N_CLASS, lens, float(thred), C.c_void_p(f0.data_ptr()),
            f0.stride(0), C.c_void_p(None if path is None else path.data_ptr()), 0 if path is None else path.stride(0),
            self._stream()), "dsd_rmvpe_decode_viterbi")

    @torch.no_grad()
    def decode_viterbi(self, hidden, thred=0.03, lengths=None, return_path=False):
        """to_viterbi_f0 (utils.py:26-43) on hidden [B, T, 360] (or [T, 360]): the librosa.sequence.viterbi path over the 360
        classes, then to_local_average_f0 around it -> f0 numpy [B, T] ([T] for B = 1).  With `lengths` (B frame counts)
        item b is decoded as a lone call on its first lengths[b] frames and a list of B arrays comes back.  With
        return_path: (f0, path), the path as int64 like librosa's."""
        h = self._hidden(hidden)
        b, t, _ = h.shape
        f0 = torch.zeros(b, t, device=self.device)
        path = torch.zeros(b, t, dtype=torch.int32, device=self.device) if return_path else None
        self._viterbi(h, lengths, thred, f0, path)
        f0 = f0.cpu().numpy()
        if return_path:
            path = path.cpu().numpy().astype(np.int64)
        if lengths is not None:
            f0 = [f0[i, : int(n)] for i, n in enumerate(lengths)]
            path = [path[i, : int(n)] for i, n in enumerate(lengths)] if return_path else None
        elif b == 1:
            f0, path = f0[0], (path[0] if return_path else None)
        return (f0, path) if return_path else f0

    @torch.no_grad()
    def _infer(self, wav, lengths, sample_rate, thred, want_hidden=False, use_viterbi=False):
        b, n = wav.shape
        want_hidden = want_hidden or use_viterbi     # the Viterbi decode reads the hidden where dsd_rmvpe_infer left it
        frames = [num_frames(v, sample_rate) for v in lengths]
        t = max(frames)
        f0 = torch.zeros(b, t, device=self.device)
        hid = torch.zeros(b, t, N_CLASS, device=self.device) if want_hidden else None
        lens = (C.c_int64 * b)(*[int(v) for v in lengths])
        _lib.check(self._h, _lib.lib().dsd_rmvpe_infer(
            self._h, C.c_void_p(wav.data_ptr()), b, n, wav.stride(0), lens, int(sample_rate), float(thred),
            C.c_void_p(f0.data_ptr()), t, C.c_void_p(hid.data_ptr() if want_hidden else None), t * N_CLASS, N_CLASS,
            self._stream()), "dsd_rmvpe_infer")
        if use_viterbi:
            self._viterbi(hid, frames, thred, f0)
        return f0, hid, frames

    def infer_from_audio(self, audio, sample_rate=16000, thred=0.03, use_viterbi=False):
        """inference.py:38-51: a 1-D numpy waveform -> f0 numpy [T] float32."""
        wav = torch.from_numpy(np.ascontiguousarray(audio, dtype=np.float32)).to(self.device)[None]
        f0, _, _ = self._infer(wav, [wav.shape[1]], sample_rate, thred, use_viterbi=use_viterbi)
        return f0[0].cpu().numpy()

    def infer_from_audio_ragged(self, waveforms, sample_rate=16000, thred=0.03, want_hidden=False, *, use_viterbi=False):
        """One call over clips of different lengths: a list of 1-D waveforms (numpy or tensors) -> a list of f0 numpy
        arrays, each equal to infer_from_audio on that clip alone (with want_hidden: a list of (f0, hidden) pairs)."""
        if not len(waveforms):
            return []
        ws = [torch.as_tensor(np.asarray(w, dtype=np.float32) if not torch.is_tensor(w) else w, dtype=torch.float32) for w in waveforms]
        lengths = [int(w.shape[0]) for w in ws]
        wav = torch.zeros(len(ws), max(lengths), device=self.device)
        for i, w in enumerate(ws):
            wav[i, : lengths[i]] = w.to(self.device)
        f0, hid, frames = self._infer(wav, lengths, sample_rate, thred, want_hidden, use_viterbi)
        f0 = f0.cpu().numpy()
        if not want_hidden:
            return [f0[i, : frames[i]] for i in range(len(ws))]
        hid = hid.cpu().numpy()
        return [(f0[i, : frames[i]], hid[i, : frames[i]]) for i in range(len(ws))]

    def get_pitch(self, waveform, samplerate, length, *, hop_size, f0_min=65, f0_max=1100, speed=1, interp_uv=False,
                  use_viterbi=False):
        """inference.py:53-70 -> (f0 [length] float32, uv [length] bool).  `use_viterbi` is an extension of the reference's
        signature (its get_pitch always decodes by the local average): the binarizers' way to the Viterbi decode."""
        f0 = self.infer_from_audio(waveform, sample_rate=samplerate, use_viterbi=use_viterbi)
        f0, uv = interp_f0(f0)
        hop_size = int(np.round(hop_size * speed))
        time_step = hop_size / samplerate
        f0_res = resample_align_curve(f0, 0.01, time_step, length)
        uv_res = resample_align_curve(uv.astype(np.float32), 0.01, time_step, length) > 0.5
        if not interp_uv:
            f0_res[uv_res] = 0
        return f0_res, uv_res


def initialize_pe(hparams=None):
    """basics/base_pe / utils/binarizer_utils: hparams['pe'] (default 'parselmouth') and hparams['pe_ckpt'] -> an
    extractor.  Only 'rmvpe' runs here."""
    if hparams is None:
        from .hparams import hparams
    pe = hparams.get("pe", "parselmouth")
    if pe == "rmvpe":
        return RMVPE(hparams["pe_ckpt"])
    if pe in ("parselmouth", "harvest"):
        raise NotImplementedError(f"pe '{pe}' is a CPU library extractor; use the reference's for it (only 'rmvpe' runs on the GPU)")
    raise ValueError(f"unknown pitch extractor: {pe}")
