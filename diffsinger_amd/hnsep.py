"""VR harmonic-noise separation and the variance curves on libdsdenoise (drop-in for `modules/hnsep/vr/`,
`utils/decomposed_waveform.py` with `algorithm='vr'` and the curve functions of `utils/binarizer_utils.py`).

`HnSep(model_path_or_state_dict, config)` runs `CascadedNet.predict_from_audio` on the GPU: the complex STFT, the five
U-Nets (implicit-GEMM convs on the fp32 MFMA, BiLSTMs), the bounded mask, the masked iSTFT are HIP kernels
(hnsep_kernels.hip).  `DecomposedWaveform(..., algorithm='vr')` gives `harmonic()`, `harmonic(0)` and `aperiodic()`;
`get_energy_librosa`, `get_breathiness`, `get_voicing` and `get_tension_base_harmonic` keep the reference's signatures
and have batched forms over lists of clips.  `CascadedNet` is the reference's torch module (same module and state_dict
names): the weight container of synthetic checkpoints and the torch restatement tools/time_hnsep.py times against.
There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import pathlib

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import _lib
from .variance_harness import interp_f0

TENSION_DOMAINS = {"ratio": 0, "db": 1, "logit": 2}


# -------------------------------------------------------------------------------------------------------- CascadedNet
def _cba(nin, nout, k=3, stride=1, pad=1, dilation=1, leaky=False):
    """Conv2DBNActiv: conv without bias, BatchNorm2d, ReLU or LeakyReLU(0.01); state_dict `conv.0.*`, `conv.1.*`."""
    m = nn.Module()
    m.conv = nn.Sequential(nn.Conv2d(nin, nout, k, stride, pad, dilation=dilation, bias=False), nn.BatchNorm2d(nout),
                           nn.LeakyReLU(0.01) if leaky else nn.ReLU())
    m.forward = m.conv.forward
    return m


class _Encoder(nn.Module):
    def __init__(self, nin, nout):
        super().__init__()
        self.conv1 = _cba(nin, nout, 3, 2, 1, leaky=True)
        self.conv2 = _cba(nout, nout, 3, 1, 1, leaky=True)

    def forward(self, x):
        return self.conv2(self.conv1(x))


class _Decoder(nn.Module):
    def __init__(self, nin, nout):
        super().__init__()
        self.conv1 = _cba(nin, nout)

    def forward(self, x, skip):
        x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
        if skip.shape[3] != x.shape[3]:          # crop_center on the frame axis (never on predict_from_audio's path)
            s = (skip.shape[3] - x.shape[3]) // 2
            skip = skip[:, :, :, s:s + x.shape[3]]
        return self.conv1(torch.cat([x, skip], 1))


class _Mean(nn.Module):
    def forward(self, x):
        return x.mean(-2, keepdim=True)


class _ASPP(nn.Module):
    def __init__(self, c, dilations):
        super().__init__()
        self.conv1 = nn.Sequential(_Mean(), _cba(c, c, 1, 1, 0))
        self.conv2 = _cba(c, c, 1, 1, 0)
        self.conv3 = _cba(c, c, 3, 1, dilations[0], dilations[0])
        self.conv4 = _cba(c, c, 3, 1, dilations[1], dilations[1])
        self.conv5 = _cba(c, c, 3, 1, dilations[2], dilations[2])
        self.bottleneck = _cba(5 * c, c, 1, 1, 0)

    def forward(self, x):
        f1 = self.conv1(x).expand(-1, -1, x.shape[2], -1)
        return self.bottleneck(torch.cat([f1, self.conv2(x), self.conv3(x), self.conv4(x), self.conv5(x)], 1))


class _LSTMModule(nn.Module):
    def __init__(self, nin_conv, nin_lstm, nout_lstm):
        super().__init__()
        self.conv = _cba(nin_conv, 1, 1, 1, 0)
        self.lstm = nn.LSTM(input_size=nin_lstm, hidden_size=nout_lstm // 2, bidirectional=True)
        self.dense = nn.Sequential(nn.Linear(nout_lstm, nin_lstm), nn.BatchNorm1d(nin_lstm), nn.ReLU())

    def forward(self, x):
        n, _, bins, frames = x.shape
        h = self.conv(x)[:, 0].permute(2, 0, 1)                     # [frames, N, bins]
        h, _ = self.lstm(h)
        h = self.dense(h.reshape(-1, h.shape[-1]))
        return h.reshape(frames, n, 1, bins).permute(1, 2, 3, 0)


class BaseNet(nn.Module):
    def __init__(self, nin, nout, nin_lstm, nout_lstm, dilations=((4, 2), (8, 4), (12, 6))):
        super().__init__()
        self.enc1 = _cba(nin, nout)
        self.enc2 = _Encoder(nout, 2 * nout)
        self.enc3 = _Encoder(2 * nout, 4 * nout)
        self.enc4 = _Encoder(4 * nout, 6 * nout)
        self.enc5 = _Encoder(6 * nout, 8 * nout)
        self.aspp = _ASPP(8 * nout, dilations)
        self.dec4 = _Decoder(14 * nout, 6 * nout)
        self.dec3 = _Decoder(10 * nout, 4 * nout)
        self.dec2 = _Decoder(6 * nout, 2 * nout)
        self.lstm_dec2 = _LSTMModule(2 * nout, nin_lstm, nout_lstm)
        self.dec1 = _Decoder(3 * nout + 1, nout)

    def forward(self, x):
        e1 = self.enc1(x)
        e2 = self.enc2(e1)
        e3 = self.enc3(e2)
        e4 = self.enc4(e3)
        h = self.aspp(self.enc5(e4))
        h = self.dec2(self.dec3(self.dec4(h, e4), e3), e2)
        return self.dec1(torch.cat([h, self.lstm_dec2(h)], 1), e1)


class CascadedNet(nn.Module):
    """modules/hnsep/vr/nets.py:CascadedNet with is_complex=True (the only form load_sep_model builds), eval mode."""

    def __init__(self, n_fft, hop_length, nout=32, nout_lstm=128, is_complex=True, is_mono=False):
        super().__init__()
        if not is_complex:
            raise NotImplementedError("is_complex=False: load_sep_model always builds the complex model")
        self.n_fft, self.hop_length, self.is_mono = n_fft, hop_length, bool(is_mono)
        self.max_bin, self.output_bin = n_fft // 2, n_fft // 2 + 1
        nl = self.max_bin // 2
        nin = 2 if is_mono else 4
        self.stg1_low_band_net = nn.Sequential(BaseNet(nin, nout // 2, nl // 2, nout_lstm), _cba(nout // 2, nout // 4, 1, 1, 0))
        self.stg1_high_band_net = BaseNet(nin, nout // 4, nl // 2, nout_lstm // 2)
        self.stg2_low_band_net = nn.Sequential(BaseNet(nout // 4 + nin, nout, nl // 2, nout_lstm), _cba(nout, nout // 2, 1, 1, 0))
        self.stg2_high_band_net = BaseNet(nout // 4 + nin, nout // 2, nl // 2, nout_lstm // 2)
        self.stg3_full_band_net = BaseNet(3 * nout // 4 + nin, nout, nl, nout_lstm)
        self.out = nn.Conv2d(nout, nin, 1, bias=False)
        self.aux_out = nn.Conv2d(3 * nout // 4, nin, 1, bias=False)

    def forward(self, spec):
        x = torch.cat([spec.real, spec.imag], 1)[:, :, :self.max_bin]
        bw = x.shape[2] // 2
        lo, hi = x[:, :, :bw], x[:, :, bw:]
        l1, h1 = self.stg1_low_band_net(lo), self.stg1_high_band_net(hi)
        l2 = self.stg2_low_band_net(torch.cat([lo, l1], 1))
        h2 = self.stg2_high_band_net(torch.cat([hi, h1], 1))
        f3 = self.stg3_full_band_net(torch.cat([x, torch.cat([l1, h1], 2), torch.cat([l2, h2], 2)], 1))
        m = self.out(f3)
        c = m.shape[1] // 2
        m = torch.complex(m[:, :c], m[:, c:])
        mag = m.abs()
        m = torch.tanh(mag) * m / (mag + 1e-8)
        pad = (0, 0, 0, self.output_bin - m.shape[2])
        return torch.complex(F.pad(m.real, pad, mode="replicate"), F.pad(m.imag, pad, mode="replicate"))

    def predict_from_audio(self, x):
        """nets.py:148-166 in torch (the timing tool's comparison and the float64 oracle of the long clips)."""
        b, c, t = x.shape
        x = x.reshape(b * c, t)
        pad_l, pad_r, _ = padding(t, self.hop_length)
        win = torch.hann_window(self.n_fft, dtype=x.dtype, device=x.device)
        spec = torch.stft(F.pad(x, (pad_l, pad_r)), self.n_fft, self.hop_length, window=win, return_complex=True,
                          pad_mode="constant")
        spec = spec.reshape(b, c, spec.shape[-2], spec.shape[-1])
        pred = (spec * self.forward(spec)).reshape(b * c, spec.shape[-2], spec.shape[-1])
        y = torch.istft(pred, self.n_fft, self.hop_length, window=win)
        return y[:, pad_l:pad_l + t].reshape(b, c, t)


def padding(n_samples, hop_length):
    """predict_from_audio's zero padding -> (left, right, padded frame count)."""
    n_frames = n_samples // hop_length + 1
    t_pad = (32 * (n_frames // 32 + 1) - 1) * hop_length - n_samples
    left = t_pad // 2 // hop_length * hop_length
    return left, t_pad - left, 32 * (n_frames // 32 + 1)


def num_frames(n_samples, hop_length):
    return int(_lib.lib().dsd_hnsep_num_frames(int(n_samples), int(hop_length)))


def read_config(model_path):
    """The config.yaml next to a checkpoint (load_sep_model) -> CascadedNet's constructor arguments."""
    import yaml
    with open(pathlib.Path(model_path).with_name("config.yaml"), "r") as f:
        a = yaml.safe_load(f)
    return dict(n_fft=a["n_fft"], hop_length=a["hop_length"], nout=a["n_out"], nout_lstm=a["n_out_lstm"],
                is_mono=bool(a["is_mono"]))


def load_sep_model(model_path, device="cpu"):
    """modules/hnsep/vr/__init__.py:load_sep_model: the torch mirror with the checkpoint's weights (weights_only load)."""
    model = CascadedNet(**read_config(model_path), is_complex=True)
    model.load_state_dict(torch.load(model_path, map_location="cpu", weights_only=True))
    return model.to(device).eval()


# ------------------------------------------------------------------------------------------------------------ the GPU
class HnSep:
    """The separator on the MI355X.  `model`: a checkpoint path (config.yaml beside it), a CascadedNet, or a state_dict
    with `config` = CascadedNet's arguments (n_fft, hop_length, nout, nout_lstm, is_mono)."""

    def __init__(self, model, config=None, device=None):
        if isinstance(model, CascadedNet):
            config = dict(n_fft=model.n_fft, hop_length=model.hop_length, nout=model.out.in_channels,
                          nout_lstm=2 * model.stg3_full_band_net.lstm_dec2.lstm.hidden_size, is_mono=model.is_mono)
            sd = model.state_dict()
        elif isinstance(model, dict):
            if config is None:
                raise ValueError("a state_dict needs config=dict(n_fft, hop_length, nout, nout_lstm, is_mono)")
            sd = model
        else:
            config = read_config(model)
            sd = torch.load(model, map_location="cpu", weights_only=True)
        self.config = dict(config)
        self.device = torch.device("cuda" if device is None else device)
        if self.device.type != "cuda":
            raise RuntimeError("diffsinger_amd.hnsep.HnSep runs only on an MI355X (HIP) device; there is no CPU path")
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", idx)
        cfg = self._native_config(idx)
        hp = C.c_void_p()
        rc = _lib.lib().dsd_hnsep_create(C.byref(cfg), C.byref(hp))
        if rc != 0:
            raise _lib.NativeLibraryError(f"dsd_hnsep_create failed ({rc}): {_lib.lib().dsd_last_error(None).decode()}")
        self._h = hp
        self._sd = sd
        _lib.load_state_dict(hp, sd)
        self.is_mono = bool(self.config["is_mono"])

    # -- model files (diffsinger_amd/modelfile.py: section_of / attach) --------------------------------------------------
    def _native_config(self, device_index):
        c = self.config
        return _lib.DsdHnsepConfig(C.sizeof(_lib.DsdHnsepConfig), int(c["n_fft"]), int(c["hop_length"]), int(c["nout"]),
                                   int(c["nout_lstm"]), int(bool(c["is_mono"])), device_index)

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
    def mask(self, spec, lengths=None):
        """CascadedNet.forward: complex spec [B, C, n_fft / 2 + 1, T] (T and lengths multiples of 16) -> complex mask."""
        s = torch.view_as_real(torch.as_tensor(spec, device=self.device).to(torch.complex64).contiguous())
        b, c, f, t, _ = s.shape
        out = torch.zeros_like(s)
        lens = None if lengths is None else (C.c_int64 * b)(*[int(v) for v in lengths])
        _lib.check(self._h, _lib.lib().dsd_hnsep_mask(
            self._h, C.c_void_p(s.data_ptr()), b, t, *s.stride()[:4], lens, C.c_void_p(out.data_ptr()), *out.stride()[:4],
            self._stream()), "dsd_hnsep_mask")
        return torch.view_as_complex(out)

    @torch.no_grad()
    def separate_ragged(self, waveforms):
        """The harmonic parts of 1-D clips of any lengths, in one call, each exactly as its lone call -> list of
        float32 device tensors."""
        clips = [torch.as_tensor(np.asarray(w, dtype=np.float32) if not torch.is_tensor(w) else w, dtype=torch.float32,
                                 device=self.device).reshape(-1) for w in waveforms]
        lens = [int(v.shape[0]) for v in clips]
        n = max(lens)
        wav = torch.zeros(len(clips), n, device=self.device)
        for i, v in enumerate(clips):
            wav[i, :lens[i]] = v
        out = torch.zeros(len(clips), n, device=self.device)
        _lib.check(self._h, _lib.lib().dsd_hnsep_separate(
            self._h, C.c_void_p(wav.data_ptr()), len(clips), n, n, 0, (C.c_int64 * len(clips))(*lens),
            C.c_void_p(out.data_ptr()), n, 0, self._stream()), "dsd_hnsep_separate")
        return [out[i, :lens[i]] for i in range(len(clips))]

    @torch.no_grad()
    def predict_from_audio(self, x):
        """nets.py:148-166: x [B, C, T] with C the model's channel count (1 mono, 2 stereo; each channel its own STFT, the
        network sees them jointly) -> the harmonic parts [B, C, T] as a device tensor.  (DecomposedWaveform's mono clip on
        a stereo model, repeated and averaged, is separate_ragged.)"""
        x = torch.as_tensor(x, dtype=torch.float32, device=self.device)
        c = 1 if self.is_mono else 2
        if x.dim() != 3 or x.shape[1] != c:
            raise ValueError(f"predict_from_audio takes [B, {c}, T] for this {'mono' if c == 1 else 'stereo'} model, "
                             f"got {list(x.shape)}")
        x = x.contiguous()
        b, _, n = x.shape
        out = torch.zeros(b, c, n, device=self.device)
        _lib.check(self._h, _lib.lib().dsd_hnsep_separate(
            self._h, C.c_void_p(x.data_ptr()), b, n, c * n, n, None, C.c_void_p(out.data_ptr()), c * n, n, self._stream()),
            "dsd_hnsep_separate")
        return out

    @torch.no_grad()
    def base_harmonic_ragged(self, harmonics, f0s, samplerate, hop_size, win_size):
        """_kth_harmonic(0) of each (harmonic part, f0) pair: f0 is interpolated over unvoiced frames and edge-padded to
        n_samples // hop + 1 frames on the host, as in the reference."""
        hs = [torch.as_tensor(h, dtype=torch.float32, device=self.device).reshape(-1) for h in harmonics]
        lens = [int(h.shape[0]) for h in hs]
        f0p = []
        for h_len, f0 in zip(lens, f0s):
            f0 = np.asarray(f0, dtype=np.float64).copy()
            pad = h_len // hop_size - len(f0) + 1
            if pad > 0:
                f0 = np.pad(f0, (0, pad), mode="constant", constant_values=(f0[0], f0[-1]))
            f0p.append(interp_f0(f0)[0].astype(np.float32))
        n, nf, b = max(lens), max(len(f) for f in f0p), len(hs)
        wav = torch.zeros(b, n, device=self.device)
        f0d = torch.zeros(b, nf, device=self.device)
        for i in range(b):
            wav[i, :lens[i]] = hs[i]
            f0d[i, :len(f0p[i])] = torch.from_numpy(f0p[i]).to(self.device)
        out = torch.zeros(b, n, device=self.device)
        _lib.check(self._h, _lib.lib().dsd_base_harmonic(
            self._h, C.c_void_p(wav.data_ptr()), b, n, n, (C.c_int64 * b)(*lens), C.c_void_p(f0d.data_ptr()), nf,
            (C.c_int64 * b)(*[len(f) for f in f0p]), int(samplerate), int(hop_size), int(win_size), C.c_void_p(out.data_ptr()),
            n, self._stream()), "dsd_base_harmonic")
        return [out[i, :lens[i]] for i in range(b)]

    @torch.no_grad()
    def curves_ragged(self, waveforms, harmonics, base_harmonics, lengths, hop_size, win_size, domain="logit",
                      which=("energy", "breathiness", "voicing", "tension"), energy_domain="db"):
        """The four variance curves of each clip (any of the signal lists may be None when no requested curve needs it)
        -> dict name -> list of float32 numpy arrays of lengths[i] frames.  energy_domain 'amplitude' leaves the first
        three curves as RMS (get_energy_librosa's domain)."""
        if domain not in TENSION_DOMAINS:
            raise ValueError(f"Invalid domain: {domain}")
        if energy_domain not in ("db", "amplitude"):
            raise ValueError(f"Invalid domain: {energy_domain}")
        sigs = [waveforms, harmonics, base_harmonics]
        ref = next(s for s in sigs if s is not None)
        b = len(ref)
        lens = [int(np.asarray(v.shape)[-1]) if torch.is_tensor(v) else len(v) for v in ref]
        n = max(lens)
        dev = []
        for s in sigs:
            if s is None:
                dev.append(None)
                continue
            t = torch.zeros(b, n, device=self.device)
            for i, v in enumerate(s):
                t[i, :lens[i]] = torch.as_tensor(v, dtype=torch.float32, device=self.device).reshape(-1)
            dev.append(t)
        T = max(1, max(int(v) for v in lengths))
        outs = {k: torch.zeros(b, T, device=self.device) if k in which else None
                for k in ("energy", "breathiness", "voicing", "tension")}
        ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else None)   # noqa: E731
        _lib.check(self._h, _lib.lib().dsd_variance_curves(
            self._h, ptr(dev[0]), ptr(dev[1]), ptr(dev[2]), b, n, (C.c_int64 * b)(*lens), int(hop_size), int(win_size),
            (C.c_int64 * b)(*[int(v) for v in lengths]), TENSION_DOMAINS[domain], int(energy_domain == "db"), ptr(outs["energy"]), ptr(outs["breathiness"]),
            ptr(outs["voicing"]), ptr(outs["tension"]), T, self._stream()), "dsd_variance_curves")
        return {k: [v[i, :int(lengths[i])].cpu().numpy() for i in range(b)] for k, v in outs.items() if v is not None}


# ------------------------------------------------------------------------------------- decomposition and the curves
class DecomposedWaveform:
    """utils/decomposed_waveform.py:DecomposedWaveform for algorithm='vr' (`model`: an HnSep).  harmonic(), harmonic(0)
    and aperiodic() run on the GPU and are cached as in the reference; numpy float32 out."""

    def __init__(self, waveform, samplerate, f0, *, hop_size=None, fft_size=None, win_size=None, algorithm="vr",
                 model=None, base_harmonic_radius=3.5):
        if algorithm == "world":
            raise NotImplementedError("algorithm='world' (pyworld CheapTrick / D4C / synthesis) stays on the reference")
        if algorithm != "vr":
            raise ValueError(f" [x] Unknown harmonic-noise separator: {algorithm}")
        if model is None:
            raise ValueError("algorithm='vr' needs model=HnSep(...)")
        if base_harmonic_radius != 3.5:
            raise NotImplementedError("base_harmonic_radius != 3.5")
        self._waveform = np.asarray(waveform, dtype=np.float32)
        self._samplerate, self._f0 = samplerate, f0
        self._hop_size = hop_size
        self._fft_size = fft_size if fft_size is not None else win_size
        self._win_size = win_size
        self.model = model
        self._harmonic_part = self._aperiodic_part = None
        self._harmonics = {}

    samplerate = property(lambda self: self._samplerate)
    hop_size = property(lambda self: self._hop_size)
    fft_size = property(lambda self: self._fft_size)
    win_size = property(lambda self: self._win_size)

    def _infer(self):
        h = self.model.separate_ragged([self._waveform])[0].cpu().numpy()
        self._harmonic_part = h
        self._aperiodic_part = self._waveform - h

    def harmonic(self, k=None):
        if k is not None:
            if k != 0:
                raise NotImplementedError("harmonic(k) for k > 0: no binarizer calls it")
            if 0 not in self._harmonics:
                self._harmonics[0] = self.model.base_harmonic_ragged(
                    [self.harmonic()], [self._f0], self._samplerate, self._hop_size, self._win_size)[0].cpu().numpy()
            return self._harmonics[0]
        if self._harmonic_part is None:
            self._infer()
        return self._harmonic_part

    def aperiodic(self):
        if self._aperiodic_part is None:
            self._infer()
        return self._aperiodic_part


def get_energy_librosa(waveform, length, *, hop_size, win_size, domain="db", model=None):
    """binarizer_utils.py:82-102 on the GPU (`model`: any HnSep handle; no weights are used)."""
    if domain not in ("db", "amplitude"):
        raise ValueError(f"Invalid domain: {domain}")
    if model is None:
        raise ValueError("get_energy_librosa needs model=HnSep(...) (the curves run on the GPU)")
    return model.curves_ragged([waveform], None, None, [length], hop_size, win_size, which=("energy",),
                               energy_domain=domain)["energy"][0]


def _decomposed(waveform, samplerate, f0, hop_size, fft_size, win_size, model):
    if isinstance(waveform, DecomposedWaveform):
        return waveform
    return DecomposedWaveform(waveform, samplerate, f0, hop_size=hop_size, fft_size=fft_size, win_size=win_size,
                              algorithm="vr", model=model)


def get_breathiness(waveform, samplerate, f0, length, *, hop_size=None, fft_size=None, win_size=None, model=None):
    w = _decomposed(waveform, samplerate, f0, hop_size, fft_size, win_size, model)
    return w.model.curves_ragged([w._waveform], [w.harmonic()], None, [length], w.hop_size, w.win_size,
                                 which=("breathiness",))["breathiness"][0]


def get_voicing(waveform, samplerate, f0, length, *, hop_size=None, fft_size=None, win_size=None, model=None):
    w = _decomposed(waveform, samplerate, f0, hop_size, fft_size, win_size, model)
    return w.model.curves_ragged(None, [w.harmonic()], None, [length], w.hop_size, w.win_size,
                                 which=("voicing",))["voicing"][0]


def get_tension_base_harmonic(waveform, samplerate, f0, length, *, hop_size=None, fft_size=None, win_size=None,
                              domain="logit", model=None):
    w = _decomposed(waveform, samplerate, f0, hop_size, fft_size, win_size, model)
    return w.model.curves_ragged(None, [w.harmonic()], [w.harmonic(0)], [length], w.hop_size, w.win_size, domain=domain,
                                 which=("tension",))["tension"][0]


def variance_curves_batch(model, waveforms, f0s, lengths, *, samplerate, hop_size, win_size, domain="logit"):
    """Batched form: the harmonic parts, base harmonics and all four curves of a list of clips in three GPU calls ->
    dict name -> list of numpy arrays."""
    harm = model.separate_ragged(waveforms)
    base = model.base_harmonic_ragged(harm, f0s, samplerate, hop_size, win_size)
    return model.curves_ragged(waveforms, harm, base, lengths, hop_size, win_size, domain=domain)
