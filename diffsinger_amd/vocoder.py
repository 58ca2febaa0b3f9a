"""NSF-HiFiGAN vocoder on libdsdenoise (drop-in for `modules/nsf_hifigan/models.py:Generator` and the
`modules/vocoders/nsf_hifigan.py:NsfHifiGAN` wrapper's `spec2wav_torch`).

`Generator(h)` takes the checkpoint's config (dict / AttrDict, the fields models.py:207-260 reads) and holds its
parameters under the reference's names in their inference form (after `remove_weight_norm()`); a checkpoint that
still carries `weight_g` / `weight_v` pairs is folded on load (`w = g * v / ||v||`, the norm over all dims but 0,
torch.nn.utils.weight_norm's default).  `forward(x, f0)` = models.py:262-290 with SineGen's two random draws
(`torch.rand` initial phases, `torch.randn_like` noise) made on the caller's device, passed in for
reproducibility, or - `forward(x, f0, seed=...)` - drawn by the library's counter-based generator (noise.py);
`mini_nsf: true` generators (fastsinegen source, `source_conv`) have no random draws.
`forward(x, f0, lengths=[...])` vocodes a zero-padded batch of segments in one ragged call (dsd_vocode_ragged): item b
comes out as the segment alone at T = lengths[b] would, draws included.
`forward_seeded(x, f0, seeds, lengths=None)` binds dsd_vocode_seeded, the entry a C caller uses: the same waveform as
`forward(..., seed=seeds)` bit for bit, with the draws made inside the kernels that use them; `forward` itself stays on the
fill-then-vocode path.
Inference only; no CPU path.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from . import noise as seeded
from .backbones import _NativeBackbone


def _get(h, key, default=None):
    v = h.get(key, default) if hasattr(h, "get") else getattr(h, key, default)
    return default if v is None else v


class _ResBlock(nn.Module):
    def __init__(self, kind, ch, k, dils):
        super().__init__()
        mk = lambda d: nn.Conv1d(ch, ch, k, 1, dilation=d, padding=(k * d - d) // 2)   # noqa: E731
        if kind == 1:
            self.convs1 = nn.ModuleList([mk(d) for d in dils])
            self.convs2 = nn.ModuleList([mk(1) for _ in dils])
        else:
            self.convs = nn.ModuleList([mk(d) for d in dils])


class _Source(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.l_linear = nn.Linear(dim, 1)


class Generator(_NativeBackbone):
    def __init__(self, h):
        super().__init__()
        self.mini_nsf = bool(_get(h, "mini_nsf", False))
        self.h = h
        self.num_mels = int(_get(h, "num_mels"))
        self.sampling_rate = int(_get(h, "sampling_rate"))
        self.upsample_rates = [int(v) for v in _get(h, "upsample_rates")]
        self.upsample_kernel_sizes = [int(v) for v in _get(h, "upsample_kernel_sizes")]
        self.upsample_initial_channel = int(_get(h, "upsample_initial_channel"))
        self.resblock = 1 if str(_get(h, "resblock", "1")) == "1" else 2
        self.resblock_kernel_sizes = [int(v) for v in _get(h, "resblock_kernel_sizes")]
        self.resblock_dilation_sizes = [[int(d) for d in ds] for ds in _get(h, "resblock_dilation_sizes")]
        self.noise_sigma = _get(h, "noise_sigma", None)          # models.py:213: > 0 adds sigma * randn after conv_pre
        self.harmonic_num = int(_get(h, "harmonic_num", 8))      # optional key; the reference hard-codes 8 (models.py:223)
        self.upp = int(np.prod(self.upsample_rates))
        self._hidden = self.num_mels
        if not self.mini_nsf:
            self.m_source = _Source(self.harmonic_num + 1)
            self.noise_convs = nn.ModuleList()
        self.conv_pre = nn.Conv1d(self.num_mels, self.upsample_initial_channel, 7, 1, padding=3)
        self.ups = nn.ModuleList()
        self.resblocks = nn.ModuleList()
        ch = self.upsample_initial_channel
        for i, (u, k) in enumerate(zip(self.upsample_rates, self.upsample_kernel_sizes)):
            ch //= 2
            self.ups.append(nn.ConvTranspose1d(2 * ch, ch, k, u, padding=(k - u) // 2))
            for rk, rd in zip(self.resblock_kernel_sizes, self.resblock_dilation_sizes):
                self.resblocks.append(_ResBlock(self.resblock, ch, rk, rd))
            if self.mini_nsf:
                if i == 1:
                    self.source_conv = nn.Conv1d(1, ch, 1)
            elif i + 1 < len(self.upsample_rates):
                sf = int(np.prod(self.upsample_rates[i + 1:]))
                self.noise_convs.append(nn.Conv1d(1, ch, kernel_size=sf * 2, stride=sf, padding=sf // 2))
            else:
                self.noise_convs.append(nn.Conv1d(1, ch, kernel_size=1))
        self.conv_post = nn.Conv1d(ch, 1, 7, 1, padding=3)
        self._register_load_state_dict_pre_hook(self._fold_weight_norm)

    @staticmethod
    def _fold_weight_norm(state_dict, prefix, *args):
        """Checkpoints saved before remove_weight_norm(): `X.weight_g`, `X.weight_v`  ->  `X.weight`."""
        for key in [k for k in state_dict if k.startswith(prefix) and k.endswith(".weight_g")]:
            base = key[:-len("weight_g")]
            g, v = state_dict.pop(key), state_dict.pop(base + "weight_v")
            norm = v.flatten(1).norm(dim=1).reshape(-1, *([1] * (v.dim() - 1)))
            state_dict[base + "weight"] = v * (g / norm)

    def remove_weight_norm(self):           # the parameters are already stored without weight norm
        pass

    def _config(self, device_index):
        cfg = _lib.DsdVocoderConfig()
        cfg.struct_size = C.sizeof(_lib.DsdVocoderConfig)
        cfg.num_mels, cfg.sampling_rate = self.num_mels, self.sampling_rate
        cfg.upsample_initial_channel = self.upsample_initial_channel
        cfg.n_ups = len(self.upsample_rates)
        for i, (u, k) in enumerate(zip(self.upsample_rates, self.upsample_kernel_sizes)):
            cfg.upsample_rates[i], cfg.upsample_kernel_sizes[i] = u, k
        cfg.resblock = self.resblock
        cfg.n_kernels = len(self.resblock_kernel_sizes)
        for j, (rk, rd) in enumerate(zip(self.resblock_kernel_sizes, self.resblock_dilation_sizes)):
            cfg.resblock_kernel_sizes[j] = rk
            cfg.n_dilations[j] = len(rd)
            for d, dv in enumerate(rd):
                cfg.resblock_dilation_sizes[j][d] = dv
        cfg.harmonic_num = self.harmonic_num
        cfg.mini_nsf = int(self.mini_nsf)
        cfg.noise_sigma = float(self.noise_sigma) if self.noise_sigma is not None and self.noise_sigma > 0 else 0.0
        cfg.device = device_index
        return cfg

    def prepare_cond(self, cond, layout="BHT"):
        raise RuntimeError("the vocoder has no conditioner; call forward(mel, f0)")

    def _seeded_draws(self, seed, b, t, dev, per_item):
        """The draws of `forward(seed=)`: -> (rand_ini [dim] - per_item: [b, dim] -, noise [b, t * upp, dim], pre_noise
        [b, C0, t]), those a lone `forward` would not draw None.  Item i's values depend on its seed alone, not on b or t."""
        seeds = seeded.as_seeds(seed, b)
        dim = self.harmonic_num + 1
        rand_ini = noise = pre = None
        if not self.mini_nsf:
            ini_seeds = seeds if per_item else seeds[:1]
            rand_ini = seeded.fill((1, len(ini_seeds), 1, dim), ini_seeds, seeded.VOC_PHASE, kind="uniform", device=dev)
            rand_ini = rand_ini.view(b, dim) if per_item else rand_ini.view(dim)
            noise = seeded.fill((1, b, t * self.upp, dim), seeds, seeded.VOC_SOURCE, device=dev)[0]
        if self.noise_sigma is not None and self.noise_sigma > 0:
            pre = seeded.fill((1, b, self.upsample_initial_channel, t), seeds, seeded.VOC_PRE, device=dev)[0]
        return rand_ini, noise, pre

    def forward(self, x, f0, *, lengths=None, rand_ini=None, noise=None, pre_noise=None, seed=None):
        """x: [B, num_mels, T] natural-log mel, f0: [B, T] -> [B, 1, T * prod(upsample_rates)].

        `lengths` (B ints in [1, T]): a ragged batch - item b holds `lengths[b]` valid frames and comes out as it would
        alone at that length; the output past `lengths[b] * prod(upsample_rates)` is zero.  The draws are then per item:
        `rand_ini` [B, harmonic_num + 1], `noise` [B, T * upp, harmonic_num + 1] (item b's first lengths[b] * upp rows),
        `pre_noise` [B, C0, T] (item b's first lengths[b] frames); those not passed are drawn item by item in the order
        and shapes B lone calls would draw them, so the generator state afterwards is the one those calls leave.

        `seed`: every draw is made on the device from it instead (noise.py; domains VOC_PHASE, VOC_SOURCE, VOC_PRE), torch's
        generator is not touched, and no draw may be passed as well.  A dense call takes one int (its one `rand_ini` comes
        from it, as the reference draws one; B ints give each item's noise its own seed and the phases the first), a ragged
        call one int per item: item b then comes out as it does alone with `seed=seeds[b]`."""
        if seed is not None and not (rand_ini is None and noise is None and pre_noise is None):
            raise ValueError("seed= draws on the device: pass either seed or rand_ini / noise / pre_noise, not both")
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise RuntimeError("diffsinger_amd.vocoder.Generator is inference-only: call it under torch.no_grad()")
        if x.dim() != 3 or x.shape[1] != self.num_mels or tuple(f0.shape) != (x.shape[0], x.shape[2]):
            raise ValueError(f"x [B, {self.num_mels}, T] and f0 [B, T] expected; got {tuple(x.shape)}, {tuple(f0.shape)}")
        if lengths is not None:
            return self._forward_ragged(x, f0, lengths, rand_ini, noise, pre_noise, seed)
        dev = x.device
        handle = self.native_handle(dev)
        b, _, t = x.shape
        out = torch.empty((b, 1, t * self.upp), device=dev, dtype=torch.float32)
        if b == 0 or t == 0:
            return out
        x = x.detach().to(torch.float32)
        sb, sm, st_ = x.stride()
        if st_ != 1 and sm != 1:
            x = x.contiguous()
            sb, sm, st_ = x.stride()
        f0 = f0.detach().to(device=dev, dtype=torch.float32).contiguous()
        dim = self.harmonic_num + 1
        want_pre = self.noise_sigma is not None and self.noise_sigma > 0      # models.py:272-273
        if seed is not None:
            rand_ini, noise, pre_noise = self._seeded_draws(seed, b, t, dev, per_item=False)
        # the reference's order of random draws (same generator state in, same state out): SineGen's initial phases
        # (models.py:145), its additive noise (:165), and only then - after conv_pre - the noise_sigma normals (:272-273)
        if not self.mini_nsf:
            if rand_ini is None:
                rand_ini = torch.rand(dim, device=dev)
            if noise is None:
                noise = torch.randn((b, t * self.upp, dim), device=dev)
        pre_ptr = None
        if want_pre:
            c0 = self.upsample_initial_channel
            if pre_noise is None:
                pre_noise = torch.randn((b, c0, t), device=dev)
            pre_noise = pre_noise.detach().to(device=dev, dtype=torch.float32).contiguous()
            if tuple(pre_noise.shape) != (b, c0, t):
                raise ValueError(f"pre_noise [{b}, {c0}, {t}] expected")
            pre_ptr = C.c_void_p(pre_noise.data_ptr())
        if self.mini_nsf:           # deterministic source (models.py:251-260): nothing else to draw
            stream = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(handle, _lib.lib().dsd_vocode(handle, C.c_void_p(x.data_ptr()), b, t, sb, sm, st_,
                                                     C.c_void_p(f0.data_ptr()), None, None, pre_ptr,
                                                     C.c_void_p(out.data_ptr()), C.c_void_p(stream)), "dsd_vocode")
            return out
        rand_ini = rand_ini.detach().to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
        noise = noise.detach().to(device=dev, dtype=torch.float32).contiguous()
        if rand_ini.numel() != dim or tuple(noise.shape) != (b, t * self.upp, dim):
            raise ValueError(f"rand_ini [{dim}] and noise [{b}, {t * self.upp}, {dim}] expected")
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(handle, _lib.lib().dsd_vocode(handle, C.c_void_p(x.data_ptr()), b, t, sb, sm, st_,
                                                 C.c_void_p(f0.data_ptr()), C.c_void_p(rand_ini.data_ptr()),
                                                 C.c_void_p(noise.data_ptr()), pre_ptr, C.c_void_p(out.data_ptr()),
                                                 C.c_void_p(stream)), "dsd_vocode")
        return out


    def forward_seeded(self, x, f0, seeds, lengths=None):
        """dsd_vocode_seeded: `forward(x, f0, lengths=lengths, seed=seeds)` bit for bit, with the draws made inside the kernels
        that use them - no noise [B, T * upp, dim] or pre_noise [B, C0, T] tensor exists.  seeds: one int or B ints (None only
        for a generator that draws nothing); a dense call takes its one row of initial phases from the first."""
        if x.dim() != 3 or x.shape[1] != self.num_mels or tuple(f0.shape) != (x.shape[0], x.shape[2]):
            raise ValueError(f"x [B, {self.num_mels}, T] and f0 [B, T] expected; got {tuple(x.shape)}, {tuple(f0.shape)}")
        dev = x.device
        handle = self.native_handle(dev)
        b, _, t = x.shape
        x = x.detach().to(torch.float32)
        sb, sm, st_ = x.stride()
        if st_ != 1 and sm != 1:
            x = x.contiguous()
            sb, sm, st_ = x.stride()
        f0 = f0.detach().to(device=dev, dtype=torch.float32).contiguous()
        out = torch.empty((b, 1, t * self.upp), device=dev, dtype=torch.float32)
        seeds_c = None if seeds is None else (C.c_uint64 * max(1, b))(*seeded.as_seeds(seeds, b))
        lens_c = None
        if lengths is not None:
            lens = [int(v) for v in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
            if len(lens) != b:
                raise ValueError(f"lengths: {b} values expected; got {len(lens)}")
            lens_c = (C.c_int32 * max(1, b))(*lens)
        a = _lib.DsdVocodeSeededArgs(C.sizeof(_lib.DsdVocodeSeededArgs), b, t, handle, C.c_void_p(x.data_ptr()), sb, sm, st_, lens_c,
                                     C.c_void_p(f0.data_ptr()), seeds_c, C.c_void_p(out.data_ptr()))
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(handle, _lib.lib().dsd_vocode_seeded(C.byref(a), C.c_void_p(stream)), "dsd_vocode_seeded")
        if lengths is not None:
            for i, n in enumerate(lens):        # as forward(lengths=): the library leaves the samples past an item's end unspecified
                if n < t:
                    out[i, :, n * self.upp:] = 0
        return out

    def draw(self, t_len, device):
        """The random draws of a lone `forward` over `t_len` frames, made as it makes them (same calls, same order):
        -> (rand_ini [dim] or None, noise [1, t_len * upp, dim] or None, pre_noise [1, C0, t_len] or None)."""
        dim = self.harmonic_num + 1
        rand_ini = None if self.mini_nsf else torch.rand(dim, device=device)
        noise = None if self.mini_nsf else torch.randn((1, t_len * self.upp, dim), device=device)
        pre = None
        if self.noise_sigma is not None and self.noise_sigma > 0:
            pre = torch.randn((1, self.upsample_initial_channel, t_len), device=device)
        return rand_ini, noise, pre

    def _forward_ragged(self, x, f0, lengths, rand_ini, noise, pre_noise, seed=None):
        lens = [int(v) for v in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
        b, _, t = x.shape
        if len(lens) != b or any(v < 1 or v > t for v in lens):
            raise ValueError(f"lengths: {b} values in [1, {t}] expected; got {lens}")
        dev = x.device
        handle = self.native_handle(dev)
        x = x.detach().to(torch.float32)
        sb, sm, st_ = x.stride()
        if st_ != 1 and sm != 1:
            x = x.contiguous()
            sb, sm, st_ = x.stride()
        f0 = f0.detach().to(device=dev, dtype=torch.float32).contiguous()
        dim, upp, c0 = self.harmonic_num + 1, self.upp, self.upsample_initial_channel
        want_pre = self.noise_sigma is not None and self.noise_sigma > 0
        if seed is not None:        # whole-batch draws: item i's first lengths[i] frames are what it draws alone
            rand_ini, noise, pre_noise = self._seeded_draws(seed, b, t, dev, per_item=True)
        draw_ini = not self.mini_nsf and rand_ini is None
        draw_noise = not self.mini_nsf and noise is None
        draw_pre = want_pre and pre_noise is None
        if draw_ini:
            rand_ini = torch.empty((b, dim), device=dev)
        if draw_noise:
            noise = torch.zeros((b, t * upp, dim), device=dev)
        if draw_pre:
            pre_noise = torch.zeros((b, c0, t), device=dev)
        for i, n in enumerate(lens):        # per item, in item order: what a lone call at T = lengths[i] draws (see forward)
            if draw_ini:
                rand_ini[i] = torch.rand(dim, device=dev)
            if draw_noise:
                noise[i, :n * upp] = torch.randn((1, n * upp, dim), device=dev)[0]
            if draw_pre:
                pre_noise[i, :, :n] = torch.randn((1, c0, n), device=dev)[0]
        pre_ptr = None
        if want_pre:
            pre_noise = pre_noise.detach().to(device=dev, dtype=torch.float32).contiguous()
            if tuple(pre_noise.shape) != (b, c0, t):
                raise ValueError(f"pre_noise [{b}, {c0}, {t}] expected")
            pre_ptr = C.c_void_p(pre_noise.data_ptr())
        ini_ptr = noise_ptr = None
        if not self.mini_nsf:
            rand_ini = rand_ini.detach().to(device=dev, dtype=torch.float32).contiguous()
            noise = noise.detach().to(device=dev, dtype=torch.float32).contiguous()
            if tuple(rand_ini.shape) != (b, dim) or tuple(noise.shape) != (b, t * upp, dim):
                raise ValueError(f"rand_ini [{b}, {dim}] and noise [{b}, {t * upp}, {dim}] expected")
            ini_ptr, noise_ptr = C.c_void_p(rand_ini.data_ptr()), C.c_void_p(noise.data_ptr())
        out = torch.empty((b, 1, t * upp), device=dev, dtype=torch.float32)
        lens_c = (C.c_int32 * b)(*lens)
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(handle, _lib.lib().dsd_vocode_ragged(handle, C.c_void_p(x.data_ptr()), b, t, sb, sm, st_, lens_c,
                                                        C.c_void_p(f0.data_ptr()), ini_ptr, noise_ptr, pre_ptr,
                                                        C.c_void_p(out.data_ptr()), C.c_void_p(stream)), "dsd_vocode_ragged")
        for i, n in enumerate(lens):        # the library leaves the samples past an item's end unspecified
            if n < t:
                out[i, :, n * upp:] = 0
        return out


class NsfHifiGAN:
    """The `spec2wav_torch` half of modules/vocoders/nsf_hifigan.py:16-70 around a `Generator` (the checkpoint /
    config loading of `load_model`, models.py:18-33, is the caller's: pass the built generator and its config)."""

    def __init__(self, generator: Generator, mel_base="10"):
        self.model, self.h, self.mel_base = generator, generator.h, mel_base

    def spec2wav_torch(self, mel, **kwargs):        # mel: [B, T, bins]
        with torch.no_grad():
            c = mel.transpose(2, 1)
            if self.mel_base != 'e':
                assert self.mel_base in [10, '10'], "mel_base must be 'e', '10' or 10."
                c = 2.30259 * c                      # log10 to log mel (nsf_hifigan.py:62-64)
            f0 = kwargs.get('f0')
            if f0 is None:
                raise ValueError("the NSF generator needs f0 (models.py:262)")
            extra = {k: kwargs[k] for k in ("lengths", "rand_ini", "noise", "pre_noise", "seed") if kwargs.get(k) is not None}
            return self.model(c, f0, **extra).view(-1)
