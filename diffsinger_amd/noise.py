"""Seeded random draws on the device (dsd_noise_fill): what `torch.randn` / `torch.rand` are to the default paths.

Element (row, col) of stream s is a pure function of (seed, domain, s, row, col) - Philox4x32-10, specified in
include/dsdenoise.h - so a draw depends neither on the batch it is made in nor on the process's generator state:
item b of a ragged batch draws what a lone call with `seeds[b]` draws, and a C caller draws what this module draws.

`domain` keeps the tensors drawn under one seed apart; the shims use the constants below.  `stream` numbers the
tensors of a sequence (the k-th step noise of an ancestral run).
"""
from __future__ import annotations

import ctypes as C
import operator

import torch

from . import _lib

# domains: one per tensor a seeded run draws
X_T = 1             # the sampler's start state (GaussianDiffusion / RectifiedFlow)
STEP = 2            # ancestral DDPM's per-step noise, stream = step index
VOC_SOURCE = 3      # the vocoder's additive source noise [T * upp, harmonic_num + 1]
VOC_PRE = 4         # its noise_sigma normals after conv_pre [C0, T]
VOC_PHASE = 5       # SineGen's initial phases (uniform) [1, harmonic_num + 1]
PITCH_X_T = 6       # the variance pair: the pitch predictor's start state ...
VARIANCE_X_T = 7    # ... and the variance predictor's
SCORE_T = 8         # forward_score: the items' diffusion time (uniform) [1, 1] ...
SCORE_NOISE = 9     # ... and the noise of its noising step
SCORE_VAR_T = 10    # the variance model scores two predictors under one seed: the pitch predictor draws under the two
SCORE_VAR_NOISE = 11    # above, the variance predictor under these

KINDS = {"normal": _lib.DSD_NOISE_NORMAL, "uniform": _lib.DSD_NOISE_UNIFORM}


def as_seeds(seed, b):
    """`seed=` as the shims take it - an int (every item the same seed) or a sequence of `b` ints - as a list of b ints."""
    if torch.is_tensor(seed):
        seed = seed.tolist()
    try:
        seeds = [operator.index(seed)] * b
    except TypeError:
        seeds = [operator.index(s) for s in seed]
    if len(seeds) != b:
        raise ValueError(f"seed: one int or {b} ints expected; got {len(seeds)}")
    if any(s < 0 or s >> 64 for s in seeds):
        raise ValueError("seed: values in [0, 2^64) expected")
    return seeds


def fill(shape, seeds, domain, first_stream=0, kind="normal", src=None, scale=1.0, src_scale=1.0, out=None, device=None):
    """-> [n, B, rows, cols] fp32 on the device, drawn on the current stream: out[k] is stream `first_stream + k`, item b
    under `seeds[b]` (an int: every item).  `shape` is (n, B, rows, cols), or a dsd_noise_spec-shaped `_lib.DsdNoiseSpec`
    whose shape fields are taken.  With `src` (the same shape): src_scale * src + scale * eps in the one launch.
    `out` (dense fp32, the same element count) is written in place and returned."""
    if isinstance(shape, _lib.DsdNoiseSpec):
        shape = (shape.n, shape.B, shape.rows, shape.cols)
    n, b, rows, cols = (int(v) for v in shape)
    if kind not in KINDS:
        raise ValueError(f"kind: one of {sorted(KINDS)} expected; got {kind!r}")
    seeds = as_seeds(seeds, b)
    if out is None:
        if device is None:
            device = src.device if src is not None else torch.device("cuda", torch.cuda.current_device())
        out = torch.empty((n, b, rows, cols), device=device, dtype=torch.float32)
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != n * b * rows * cols:
        raise ValueError(f"out: dense fp32 of {n * b * rows * cols} elements expected")
    dev = out.device
    if dev.type != "cuda":
        raise ValueError("noise.fill draws on the GPU; there is no CPU path")
    spec = _lib.DsdNoiseSpec()
    spec.struct_size = C.sizeof(_lib.DsdNoiseSpec)
    spec.kind, spec.domain, spec.first_stream = KINDS[kind], int(domain), int(first_stream)
    spec.n, spec.B, spec.rows, spec.cols = n, b, rows, cols
    arr = (C.c_uint64 * b)(*seeds)
    spec.seeds = C.cast(arr, C.POINTER(C.c_uint64))
    spec.scale, spec.src_scale = float(scale), float(src_scale)
    if src is not None:
        src = src.detach().to(device=dev, dtype=torch.float32).contiguous()
        if src.numel() != out.numel():
            raise ValueError(f"src: {out.numel()} elements expected; got {src.numel()}")
        spec.src = src.data_ptr()
    index = dev.index if dev.index is not None else torch.cuda.current_device()
    stream = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(None, _lib.lib().dsd_noise_fill(index, C.byref(spec), C.c_void_p(out.data_ptr()), C.c_void_p(stream)),
               "dsd_noise_fill")
    return out
