"""The acoustic model's staged twin as a C program drives it (include/dsdenoise.h, dsd_acoustic_open .. dsd_acoustic_sample),
from Python.

`Acoustic(file, prefix, device)` opens the object from a model file (`modelfile.acoustic_sections` packs one) and exposes
the stage calls on torch tensors, one method per C call with the argument names of `deploy.DiffSingerAcousticDeploy`, which
stays the path of the Python shims and the yardstick these calls are tested against.  `plan(cfg, depth, steps)` is the
host-only dsd_acoustic_plan and needs no GPU.  No CPU path for the stages.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib

NAMES = ("energy", "breathiness", "voicing", "tension")        # the order of the DSD_EMBED_* bits


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _as(t, dtype, device):
    return None if t is None else t.detach().to(device=device, dtype=dtype).contiguous()


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _spk_mix(entry, name, obj, device, hidden, ids, values, normalize, out):
    """dsd_acoustic_spk_mix / dsd_variance_spk_mix on `obj`; the shapes go to the library as given, which refuses what it refuses"""
    ids = [[int(i) for i in row] for row in (ids.tolist() if torch.is_tensor(ids) else ids)]
    values = _as(values, torch.float32, device)
    bsz, rows, n = values.shape
    if len(ids) != bsz or any(len(row) != n for row in ids):
        raise ValueError(f"ids: [{bsz}, {n}] ints expected")
    if out is None:
        out = torch.empty((bsz, rows, hidden), device=device, dtype=torch.float32)
    flat = (C.c_int32 * max(1, bsz * n))(*[i for row in ids for i in row])
    a = _lib.DsdSpkMixArgs(C.sizeof(_lib.DsdSpkMixArgs), bsz, rows, n, flat, _ptr(values), int(bool(normalize)), _ptr(out))
    _lib.check(None, entry(obj, C.byref(a), _stream(device)), name)
    return out


def plan(cfg, depth, steps):
    """dsd_acoustic_plan on a `_lib.DsdAcousticConfig`: depth None = no shallow source -> `_lib.DsdAcousticPlan`"""
    out = _lib.DsdAcousticPlan()
    _lib.check(None, _lib.lib().dsd_acoustic_plan(C.byref(cfg), -1.0 if depth is None else float(depth), int(steps), C.byref(out)),
               "dsd_acoustic_plan")
    return out


class Acoustic:
    def __init__(self, file, prefix, device=0):
        self._a = None
        dev = torch.device(device if not isinstance(device, int) else f"cuda:{device}")
        if dev.type != "cuda":
            raise RuntimeError(f"diffsinger_amd.cacoustic runs only on an MI355X (HIP) device; got {dev.type}. There is no CPU path.")
        self.device = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        ap = C.c_void_p()
        _lib.check(None, _lib.lib().dsd_acoustic_open(file._f, str(prefix).encode(), self.device.index, C.byref(ap)), "dsd_acoustic_open")
        self._a = ap
        self.cfg = _lib.DsdAcousticConfig()
        _lib.check(None, _lib.lib().dsd_acoustic_info(self._a, C.byref(self.cfg)), "dsd_acoustic_info")
        self.names = [n for i, n in enumerate(NAMES) if self.cfg.embed_flags >> i & 1]
        self._keep = ()

    def close(self):
        if self._a is not None:
            _lib.lib().dsd_acoustic_close(self._a)
            self._a = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:      # interpreter shutdown
            pass

    def handle(self, which):
        """a borrowed inner handle: _lib.DSD_AC_FS2, DSD_AC_AUX or DSD_AC_DENOISER"""
        hp = C.c_void_p()
        _lib.check(None, _lib.lib().dsd_acoustic_handle(self._a, int(which), C.byref(hp)), "dsd_acoustic_handle")
        return hp

    def set_lengths(self, lengths):
        """dsd_acoustic_set_lengths: B frame counts for the following condition / start / sample calls, or None for dense batches"""
        if lengths is None:
            arr, n = None, 0
        else:
            lens = [int(v) for v in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
            arr, n = (C.c_int32 * max(1, len(lens)))(*lens), len(lens)
        _lib.check(None, _lib.lib().dsd_acoustic_set_lengths(self._a, arr, n, _stream(self.device)), "dsd_acoustic_set_lengths")

    def spk_mix(self, ids, values, normalize=False, out=None):
        """dsd_acoustic_spk_mix: ids [B, N] ints (host), values [B, rows, N] -> [B, rows, H], what `condition` takes as spk_embed"""
        return _spk_mix(_lib.lib().dsd_acoustic_spk_mix, "dsd_acoustic_spk_mix", self._a, self.device, self.cfg.hidden_size, ids,
                        values, normalize, out)

    # ---- stages ------------------------------------------------------------------------------------------
    def condition(self, tokens, durations, f0, variances=None, gender=None, velocity=None, spk_embed=None, languages=None,
                  out=None, want_coarse=False):
        """forward_fs2_aux -> condition [B, T, H] (, aux_mel [B, T, M] with shallow diffusion) (, f0_coarse [B, T] int64 with
        `want_coarse`).  `out`: (condition, aux_mel or None) to write into."""
        d, f32, i64 = self.device, torch.float32, torch.int64
        tokens, durations, f0 = _as(tokens, i64, d), _as(durations, i64, d), _as(f0, f32, d)
        bsz, n_ph = tokens.shape
        t_len = f0.shape[1]
        curves = [None if (variances or {}).get(n) is None else _as(variances[n], f32, d) for n in NAMES]
        gender, velocity = _as(gender, f32, d), _as(velocity, f32, d)
        spk, languages = _as(spk_embed, f32, d), _as(languages, i64, d)
        if out is not None:
            cond, aux = out
        else:
            cond = torch.empty((bsz, t_len, self.cfg.hidden_size), device=d, dtype=f32)
            aux = torch.empty((bsz, t_len, self.cfg.out_dims), device=d, dtype=f32) if self.cfg.use_shallow_diffusion else None
        coarse = torch.empty((bsz, t_len), device=d, dtype=i64) if want_coarse else None
        a = _lib.DsdAcousticConditionArgs(C.sizeof(_lib.DsdAcousticConditionArgs), bsz, n_ph, t_len, _ptr(tokens), _ptr(durations), _ptr(f0),
                                          (C.c_void_p * 4)(*[None if c is None else c.data_ptr() for c in curves]), _ptr(gender),
                                          _ptr(velocity), _ptr(spk), 0 if spk is None else spk.shape[1], _ptr(languages), _ptr(cond),
                                          _ptr(aux), _ptr(coarse))
        self._keep = (tokens, durations, f0, curves, gender, velocity, spk, languages)       # a captured graph reads them
        _lib.check(None, _lib.lib().dsd_acoustic_condition(self._a, C.byref(a), _stream(d)), "dsd_acoustic_condition")
        res = (cond,) + ((aux,) if self.cfg.use_shallow_diffusion else ()) + ((coarse,) if want_coarse else ())
        return res[0] if len(res) == 1 else res

    def plan(self, depth, steps):
        return plan(self.cfg, depth, steps)

    def start(self, p, source=None, noise=None, shape=None, out=None):
        """dsd_acoustic_start: source [B, T, M] and / or noise [B, 1, M, T] -> x [B, 1, M, T]"""
        d = self.device
        source, noise = _as(source, torch.float32, d), _as(noise, torch.float32, d)
        if shape is not None:
            bsz, t_len = shape
        elif source is not None:
            bsz, t_len = source.shape[0], source.shape[1]
        else:
            bsz, t_len = noise.shape[0], noise.shape[-1]
        x = torch.empty((bsz, 1, self.cfg.out_dims, t_len), device=d, dtype=torch.float32) if out is None else out
        _lib.check(None, _lib.lib().dsd_acoustic_start(self._a, C.byref(p), _ptr(source), _ptr(noise), bsz, t_len, _ptr(x), _stream(d)),
                   "dsd_acoustic_start")
        return x

    def sample(self, p, condition, x, step_noise=None, flags=0, out=None):
        """dsd_acoustic_sample: condition [B, T, H], x [B, 1, M, T] (, step_noise [n, B, 1, M, T]) -> mel [B, T, M]"""
        d = self.device
        condition, x, step_noise = _as(condition, torch.float32, d), _as(x, torch.float32, d), _as(step_noise, torch.float32, d)
        bsz, t_len, _ = condition.shape
        if step_noise is not None and step_noise.shape[0] < p.n_step_noise:
            raise ValueError(f"the plan reads {p.n_step_noise} step-noise tensors, {step_noise.shape[0]} given")
        mel = torch.empty((bsz, t_len, self.cfg.out_dims), device=d, dtype=torch.float32) if out is None else out
        _lib.check(None, _lib.lib().dsd_acoustic_sample(self._a, C.byref(p), _ptr(condition), _ptr(x), _ptr(step_noise), bsz, t_len,
                                                        int(flags), _ptr(mel), _stream(d)), "dsd_acoustic_sample")
        return mel
