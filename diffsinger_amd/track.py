"""A project's track on the device (dsd_track_plan / _place / _peak / _export): what `np.concatenate`, `cross_fade` and
`save_wav` are to the default path of `run_inference`.

The reference folds the segments into a growing float64 array; the track always ends where the last placed segment
ends, so the fold equals placing each segment in place into a float64 track of the final length (include/dsdenoise.h
has the rule, DESIGN.md section 4k the argument).  `plan` computes where every segment goes on the host; a `Track` owns
the device buffer, and `place` writes one segment - gap zeros, cross-fade, copy - in one launch on the current stream,
bit for bit what numpy computes.  Nothing here synchronises but `Track.numpy()`.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

SPAN = 512          # samples of the track one workgroup covers (csrc/dsd_internal.h: kTrackSpan)
KINDS = {"f64": (_lib.DSD_TRACK_F64, torch.float64), "f32": (_lib.DSD_TRACK_F32, torch.float32),
         "pcm": (_lib.DSD_TRACK_PCM, torch.int16)}


class Plan(NamedTuple):
    starts: Tuple[int, ...]         # round(offset * sample_rate) of each segment
    prev_ends: Tuple[int, ...]      # where the segment before it ended (0 for the first)
    total: int                      # the end of the last segment = the length of the track


def _refused(rc, what):
    """DSD_EINVAL -> ValueError with the library's message (the layouts numpy itself raises on); anything else as usual."""
    if rc == -1:
        raise ValueError(_lib.lib().dsd_last_error(None).decode("utf-8", "replace"))
    _lib.check(None, rc, what)


def plan(offsets: Sequence[float], lengths: Sequence[int], sample_rate: int) -> Plan:
    """Where each segment of a project goes: `offsets` in seconds, `lengths` in samples.  ValueError for a layout the
    reference raises on (a start before the track, an overlap longer than the new segment) and for an empty segment."""
    n = len(offsets)
    if len(lengths) != n:
        raise ValueError(f"plan: {n} offsets but {len(lengths)} lengths")
    offs = (C.c_double * max(n, 1))(*[float(o) for o in offsets])
    lens = (C.c_int64 * max(n, 1))(*[int(v) for v in lengths])
    starts, ends, total = (C.c_int64 * max(n, 1))(), (C.c_int64 * max(n, 1))(), C.c_int64()
    _refused(_lib.lib().dsd_track_plan(n, offs, lens, int(sample_rate), starts, ends, C.byref(total)), "dsd_track_plan")
    return Plan(tuple(starts[:n]), tuple(ends[:n]), int(total.value))


class Track:
    """The float64 track of `total` samples on `device`, and the 8 bytes of its peak.  `layout`: the `Plan` that
    `place(k, wav)` reads segment k's position from; without one, `place_at(start, prev_end, wav)`.  Segments are placed
    in order on one stream; after the last one every sample has been written (the buffer is never cleared)."""

    def __init__(self, total: int, device="cuda", layout: Optional[Plan] = None):
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("a Track lives on the GPU; there is no CPU path")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if layout is not None and layout.total != int(total):
            raise ValueError(f"Track: total {total} but the plan's is {layout.total}")
        self.total, self.device, self.layout = int(total), device, layout
        self.buf = torch.empty(self.total, dtype=torch.float64, device=device)
        self.peak = torch.zeros(1, dtype=torch.float64, device=device)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def place_at(self, start: int, prev_end: int, wav: torch.Tensor):
        if wav.device != self.device:
            raise ValueError(f"place: the segment is on {wav.device}, the track on {self.device}")
        wav = wav.detach().reshape(-1).to(torch.float32).contiguous()
        _refused(_lib.lib().dsd_track_place(self.device.index, C.c_void_p(self.buf.data_ptr()), self.total, int(start), int(prev_end),
                                            C.c_void_p(wav.data_ptr()), wav.numel(), self._stream()), "dsd_track_place")

    def place(self, k: int, wav: torch.Tensor):
        """Segment k of the plan: `wav` is its waveform (fp32 on the track's device), of the planned length."""
        if self.layout is None:
            raise ValueError("place(k, wav) needs the Track's plan; use place_at(start, prev_end, wav)")
        end = self.layout.prev_ends[k + 1] if k + 1 < len(self.layout.starts) else self.layout.total
        if wav.numel() != end - self.layout.starts[k]:
            raise ValueError(f"place: segment {k} was planned with {end - self.layout.starts[k]} samples, got {wav.numel()}")
        self.place_at(self.layout.starts[k], self.layout.prev_ends[k], wav)

    def compute_peak(self) -> torch.Tensor:
        """-> the device tensor [1] holding max |track| (np.abs(track).max(), exact)."""
        _lib.check(None, _lib.lib().dsd_track_peak(self.device.index, C.c_void_p(self.buf.data_ptr()), self.total,
                                                   C.c_void_p(self.peak.data_ptr()), self._stream()), "dsd_track_peak")
        return self.peak

    def export(self, kind: str = "f64", norm: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """-> the track as a device tensor: 'f64' (a copy), 'f32' (rounded once) or 'pcm' (int16 by `save_wav`'s rule,
        `norm=True`: divided by the peak first).  Out-of-range samples saturate and a zero peak gives zeros."""
        if kind not in KINDS:
            raise ValueError(f"kind: one of {sorted(KINDS)} expected; got {kind!r}")
        code, dtype = KINDS[kind]
        if norm and kind != "pcm":
            raise ValueError("norm=True applies to kind='pcm' only")
        if out is None:
            out = torch.empty(self.total, dtype=dtype, device=self.device)
        elif out.dtype != dtype or out.device != self.device or not out.is_contiguous() or out.numel() != self.total:
            raise ValueError(f"out: dense {dtype} of {self.total} elements on {self.device} expected")
        peak = C.c_void_p(self.compute_peak().data_ptr()) if norm else None
        _lib.check(None, _lib.lib().dsd_track_export(self.device.index, C.c_void_p(self.buf.data_ptr()), self.total, code, peak,
                                                     C.c_void_p(out.data_ptr()), self._stream()), "dsd_track_export")
        return out

    def numpy(self) -> np.ndarray:
        """The float64 track on the host: the one device-to-host copy (it synchronises)."""
        return self.buf.cpu().numpy()
