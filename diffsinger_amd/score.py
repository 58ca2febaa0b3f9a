"""Validation scoring on the device: thin bindings of dsd_diffuse, dsd_masked_loss, dsd_curve_stats and dsd_dur_score
(include/dsdenoise.h, "Validation scoring").  losses.py, metrics.py and the wrappers' `forward_score` are built on these.

Every reduction returns float64 / int64 values in a small device tensor: nothing here synchronises.  A result is
bit-identical from run to run (sums in double, in an order fixed by the element count; no floating-point atomics).
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from . import noise as seeded

KINDS = {"ddpm": _lib.DSD_DIFFUSE_DDPM, "reflow": _lib.DSD_DIFFUSE_REFLOW}

_WORKSPACES = {}


def _where(t):
    if t.device.type != "cuda":
        raise RuntimeError(f"diffsinger_amd scoring runs only on an MI355X (HIP) device; got a {t.device.type} tensor. "
                           "There is no CPU path - use the reference module for CPU.")
    index = t.device.index if t.device.index is not None else torch.cuda.current_device()
    stream = torch.cuda.current_stream(t.device).cuda_stream
    return index, stream


def _workspace(index, stream):
    """The partial sums' DSD_SCORE_WORKSPACE_BYTES: one per (device, stream), so concurrent streams never share one."""
    key = (index, stream)
    if key not in _WORKSPACES:
        _WORKSPACES[key] = torch.empty(_lib.DSD_SCORE_WORKSPACE_BYTES // 8, dtype=torch.float64, device=torch.device("cuda", index))
    return _WORKSPACES[key]


def _f32(t, device=None):
    return t.detach().to(device=device if device is not None else t.device, dtype=torch.float32).contiguous()


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def diffuse(kind, x0, a, c=None, eps=None, seeds=None, domain=seeded.SCORE_NOISE, want_target=True):
    """The noising step of p_losses on x0 [B, ...rows..., T] -> (x_t, target), both shaped like x0.  `a`, `c`: [B] fp32
    coefficients (DDPM: sqrt_alphas_cumprod[t], sqrt_one_minus_alphas_cumprod[t]; reflow: a = t).  `eps` given: used as
    the noise; else it is drawn in the launch from `seeds` under `domain` - what noise.fill draws.  DDPM's target IS eps:
    with a given eps and want_target=False none is written and None returned."""
    x0 = _f32(x0)
    b, cols = x0.shape[0], x0.shape[-1]
    rows = x0.numel() // max(b * cols, 1)
    index, stream = _where(x0)
    spec = _lib.DsdDiffuseSpec()
    spec.struct_size, spec.kind = C.sizeof(spec), KINDS[kind]
    spec.B, spec.rows, spec.cols, spec.domain = b, rows, cols, int(domain)
    a = _f32(a, x0.device).reshape(-1)
    if a.numel() != b:
        raise ValueError(f"a: {b} coefficients expected; got {a.numel()}")
    spec.x0, spec.a = x0.data_ptr(), a.data_ptr()
    if kind == "ddpm":
        c = _f32(c, x0.device).reshape(-1)
        if c.numel() != b:
            raise ValueError(f"c: {b} coefficients expected; got {c.numel()}")
        spec.c = c.data_ptr()
    keep = None
    if eps is not None:
        eps = _f32(eps, x0.device)
        if eps.shape != x0.shape:
            raise ValueError(f"eps {tuple(eps.shape)} does not match x0 {tuple(x0.shape)}")
        spec.eps = eps.data_ptr()
    else:
        keep = (C.c_uint64 * b)(*seeded.as_seeds(seeds, b))
        spec.seeds = C.cast(keep, C.POINTER(C.c_uint64))
    x_t = torch.empty_like(x0)
    target = torch.empty_like(x0) if (want_target or eps is None or kind != "ddpm") else None
    _lib.check(None, _lib.lib().dsd_diffuse(index, C.byref(spec), _ptr(x_t), _ptr(target), C.c_void_p(stream)), "dsd_diffuse")
    return x_t, target


def masked_loss(kind, pred, target, non_padding=None, t=None):
    """-> float64 [2] on the device: (sum, mean over ALL elements) of |d| ("l1") or d * d ("l2") with
    d = pred * m - target * m.  pred, target: [B, ..., T]; non_padding: [B, T] (any shape of B * T elements) or None;
    t: [B] or None - the log-norm weight of RectifiedFlowLoss per item."""
    pred, target = _f32(pred), _f32(target, pred.device)
    if pred.shape != target.shape:
        raise ValueError(f"pred {tuple(pred.shape)} and target {tuple(target.shape)} differ")
    b, cols = pred.shape[0], pred.shape[-1]
    rows = pred.numel() // max(b * cols, 1)
    index, stream = _where(pred)
    spec = _lib.DsdLossSpec()
    spec.struct_size, spec.kind = C.sizeof(spec), _lib.LOSS_IDS[kind]
    spec.B, spec.rows, spec.cols = b, rows, cols
    spec.pred, spec.target = pred.data_ptr(), target.data_ptr()
    if non_padding is not None:
        non_padding = _f32(non_padding, pred.device)
        if non_padding.numel() != b * cols:
            raise ValueError(f"non_padding: {b} x {cols} values expected; got {tuple(non_padding.shape)}")
        spec.non_padding = non_padding.data_ptr()
    if t is not None:
        t = _f32(t, pred.device).reshape(-1)
        if t.numel() != b:
            raise ValueError(f"t: {b} values expected; got {t.numel()}")
        spec.t = t.data_ptr()
    out = torch.empty(2, dtype=torch.float64, device=pred.device)
    _lib.check(None, _lib.lib().dsd_masked_loss(index, C.byref(spec), _ptr(_workspace(index, stream)), _ptr(out),
                                                C.c_void_p(stream)), "dsd_masked_loss")
    return out


def curve_stats(pred, target, mask=None, tolerance=0.0):
    """-> (counts int64 [2] = (close, total), sums float64 [3] = (sum target, sum target^2, sum (target - pred)^2)), views
    of one device buffer; elements where mask is False are left out."""
    pred, target = _f32(pred), _f32(target, pred.device)
    index, stream = _where(pred)
    if mask is not None:
        mask = mask.detach().to(device=pred.device, dtype=torch.uint8).contiguous()
    raw = torch.empty(5, dtype=torch.int64, device=pred.device)
    _lib.check(None, _lib.lib().dsd_curve_stats(index, _ptr(pred), _ptr(target), _ptr(mask), pred.numel(), float(tolerance),
                                                _ptr(_workspace(index, stream)), _ptr(raw), C.c_void_p(stream)),
               "dsd_curve_stats")
    return raw[:2], raw[2:].view(torch.float64)


def dur_score(dur_pred, dur_gt, ph2word, mask=None, n_words=None, offset=1.0, loss_type="mse", rhythm_tolerance=0.05,
              pdur_tolerance=0.2):
    """-> dict of device tensors: `sums` / `means` float64 [3] (pdur, wdur, sdur), `counts` int64 [4] (rhythm correct, rhythm
    total, phoneme accurate, phoneme total), `wdur_pred` / `wdur_gt` fp32 [B, n_words - 1].  n_words: ph2word.max() + 1 where
    the caller has it (read back from the device otherwise)."""
    dur_pred = _f32(dur_pred)
    dur_gt = _f32(dur_gt, dur_pred.device)
    ph2word = ph2word.detach().to(device=dur_pred.device, dtype=torch.int64).contiguous()
    if not (dur_pred.dim() == 2 and dur_pred.shape == dur_gt.shape == ph2word.shape):
        raise ValueError(f"dur_pred, dur_gt and ph2word must be [B, L]; got {tuple(dur_pred.shape)}, {tuple(dur_gt.shape)}, "
                         f"{tuple(ph2word.shape)}")
    index, stream = _where(dur_pred)
    if n_words is None:
        n_words = int(ph2word.max()) + 1
    b, length = dur_pred.shape
    spec = _lib.DsdDurSpec()
    spec.struct_size, spec.kind = C.sizeof(spec), _lib.DUR_LOSS_IDS[loss_type]
    spec.B, spec.L, spec.n_words = b, length, int(n_words)
    spec.offset, spec.rhythm_tolerance, spec.pdur_tolerance = float(offset), float(rhythm_tolerance), float(pdur_tolerance)
    spec.dur_pred, spec.dur_gt, spec.ph2word = dur_pred.data_ptr(), dur_gt.data_ptr(), ph2word.data_ptr()
    if mask is not None:
        mask = mask.detach().to(device=dur_pred.device, dtype=torch.uint8).contiguous()
        if mask.shape != dur_pred.shape:
            raise ValueError(f"mask {tuple(mask.shape)} does not match dur_pred {tuple(dur_pred.shape)}")
        spec.mask = mask.data_ptr()
    words = torch.empty((2, b, max(int(n_words) - 1, 0)), dtype=torch.float32, device=dur_pred.device)
    raw = torch.empty(10, dtype=torch.int64, device=dur_pred.device)
    _lib.check(None, _lib.lib().dsd_dur_score(index, C.byref(spec), _ptr(words[0]), _ptr(words[1]),
                                              _ptr(_workspace(index, stream)), _ptr(raw), C.c_void_p(stream)), "dsd_dur_score")
    f64 = raw[:6].view(torch.float64)
    return {"sums": f64[:3], "means": f64[3:], "counts": raw[6:], "wdur_pred": words[0], "wdur_gt": words[1]}
