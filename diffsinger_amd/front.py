"""The segment front end on the library: a `.ds` segment's durations in seconds and its control curves -> frame counts,
mel2ph and frame-level tensors, on `dsd_seconds_to_frames` and `dsd_curve_resample` (include/dsdenoise.h), with
`dsd_length_regulate` for the durations.

What it replaces is the host path of `harness.AcousticHarness.preprocess_input` and of the curve / duration parts of
`variance_harness.VarianceHarness.preprocess_input` (= the reference's `inference/ds_acoustic.py:102-177`,
`inference/ds_variance.py:151,179,244-278`, `utils/infer_utils.py:41-53`): one `np.interp` and one upload per curve, a
`cumsum / round / diff` on whatever device the harness sits on, and a read-back for the frame count.  Here the frame
counts are the reference's CPU result on any device and known on the host, everything a segment (or a ragged group) needs
travels to the device in ONE copy from a pinned buffer, and one launch (two with a PITCH curve) resamples every curve
straight into the rows of zero-padded [B, T_max] tensors.

`seconds_to_frames` is host arithmetic and needs no device; everything else runs only on an MI355X (HIP) device.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

PLAIN, CLIP, GENDER, PITCH = _lib.DSD_CURVE_PLAIN, _lib.DSD_CURVE_CLIP, _lib.DSD_CURVE_GENDER, _lib.DSD_CURVE_PITCH
MAX_CURVES = _lib.DSD_CURVE_MAX         # per library call; `resample` splits longer lists
CHUNK = _lib.DSD_CURVE_CHUNK            # frames a workgroup takes at a time


def _refused(rc, what):
    if rc == -1:                        # DSD_EINVAL: the caller's arguments
        raise ValueError(_lib.lib().dsd_last_error(None).decode("utf-8", "replace"))
    _lib.check(None, rc, what)


def seconds_to_frames(seconds, timestep: float) -> Tuple[np.ndarray, int]:
    """Durations in seconds -> (frames per item as np.int64, their total), by rounding the cumulative boundaries:
    `diff(round(cumsum(seconds) / timestep + 0.5), prepend 0)` as torch evaluates it on the CPU (dsd_seconds_to_frames)."""
    sec = np.ascontiguousarray(np.asarray(seconds, dtype=np.float32).reshape(-1))
    frames = np.empty(sec.shape[0], dtype=np.int64)
    total = C.c_int64(0)
    _refused(_lib.lib().dsd_seconds_to_frames(sec.ctypes.data_as(C.POINTER(C.c_float)), sec.shape[0], float(timestep),
                                              frames.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(total)), "dsd_seconds_to_frames")
    return frames, int(total.value)


def parse_curve(text) -> np.ndarray:
    """A `.ds` curve field ('440.0 441.2 ...', or a sequence of numbers) -> fp32 points."""
    return np.array(text.split(), np.float32) if isinstance(text, str) else np.asarray(text, dtype=np.float32).reshape(-1)


@dataclass
class Curve:
    """One curve of a `resample` call.  `out` / `uv`: where to write - contiguous 1-D device tensors of `pad_to` (default
    `length`) elements, e.g. a row of a zero-padded batch - or None / True to have them allocated."""
    points: np.ndarray
    src_step: float
    dst_step: float
    length: int
    op: int = PLAIN
    lo: float = 0.0
    hi: float = 0.0
    pad_to: Optional[int] = None
    out: Optional[torch.Tensor] = None
    uv: object = None                   # PITCH only: True (allocate) or a uint8 / bool tensor


def _device(device) -> torch.device:
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("diffsinger_amd.front runs only on an MI355X (HIP) device; there is no CPU path")
    return device if device.index is not None else torch.device("cuda", torch.cuda.current_device())


class _Staging:
    """The pinned host buffer of the uploads, per device: grown when needed, reused once the copy that read it is done."""
    _by_device: Dict[int, "_Staging"] = {}

    def __init__(self):
        self.buf, self.done = None, None

    @classmethod
    def of(cls, device) -> "_Staging":
        return cls._by_device.setdefault(device.index, cls())

    def take(self, nbytes: int) -> np.ndarray:
        if self.done is not None:
            self.done.synchronize()
        if self.buf is None or self.buf.numel() < nbytes:
            self.buf = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8).pin_memory()
        return self.buf.numpy()[:nbytes]

    def upload(self, nbytes: int, device) -> torch.Tensor:
        dev = torch.empty(nbytes, dtype=torch.uint8, device=device)
        dev.copy_(self.buf[:nbytes], non_blocking=True)
        if self.done is None:
            self.done = torch.cuda.Event()
        self.done.record(torch.cuda.current_stream(device))
        return dev


def _check_row(t, n, dtypes, device, what):
    if not (isinstance(t, torch.Tensor) and t.device == device and t.dtype in dtypes and t.dim() == 1 and t.numel() == n
            and t.is_contiguous()):
        raise ValueError(f"front.resample: {what} must be a contiguous 1-D {dtypes[0]} tensor of {n} elements on {device}")


def _launch(curves: Sequence[Curve], points_dev: torch.Tensor, offsets: Sequence[int], device):
    """`curves` (with out / uv tensors in place) over the uploaded points, MAX_CURVES per library call."""
    lib, stream = _lib.lib(), C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    base = points_dev.data_ptr()
    for k0 in range(0, len(curves), MAX_CURVES):
        part = curves[k0:k0 + MAX_CURVES]
        arr = (_lib.DsdCurve * len(part))()
        for d, c, off in zip(arr, part, offsets[k0:k0 + MAX_CURVES]):
            d.points, d.out = base + 4 * off, c.out.data_ptr()
            d.uv_out = c.uv.data_ptr() if isinstance(c.uv, torch.Tensor) else None
            d.src_step, d.dst_step = float(c.src_step), float(c.dst_step)
            d.n_points, d.length, d.pad_to, d.op = len(c.points), int(c.length), int(c.pad_to), int(c.op)
            d.lo, d.hi = float(c.lo), float(c.hi)
        _refused(lib.dsd_curve_resample(device.index, arr, len(part), stream), "dsd_curve_resample")


def _prepare(curves: Sequence[Curve], device) -> List[Curve]:
    ready = []
    for i, c in enumerate(curves):
        pts = np.ascontiguousarray(np.asarray(c.points, dtype=np.float32).reshape(-1))
        pad_to = int(c.length if c.pad_to is None else c.pad_to)
        if c.op == GENDER and not (float(np.float32(c.lo)) == float(c.lo) and float(np.float32(c.hi)) == float(c.hi)):
            raise ValueError(f"front.resample: curve {i}: a GENDER range travels in fp32; ({c.lo}, {c.hi}) is not exact there")
        out, uv = c.out, c.uv
        if out is None:
            out = torch.empty(max(pad_to, 0), dtype=torch.float32, device=device)
        else:
            _check_row(out, pad_to, (torch.float32,), device, f"curve {i}: out")
        if uv is True:
            uv = torch.empty(max(pad_to, 0), dtype=torch.uint8, device=device)
        elif isinstance(uv, torch.Tensor):
            _check_row(uv, pad_to, (torch.uint8, torch.bool), device, f"curve {i}: uv")
        else:
            uv = None
        ready.append(Curve(pts, c.src_step, c.dst_step, c.length, c.op, c.lo, c.hi, pad_to, out, uv))
    return ready


def resample(curves: Sequence[Curve], device) -> list:
    """Every curve resampled to its `dst_step`, cut / held to `length`, finished by its `op` and zero up to `pad_to`
    (dsd_curve_resample): ONE upload of all points, one launch per MAX_CURVES curves (two with a PITCH curve among them).
    -> per curve its fp32 tensor [pad_to], or (pitch, uv as bool) for a PITCH curve asked for `uv`."""
    device = _device(device)
    ready = _prepare(curves, device)
    if not ready:
        return []
    offsets = np.concatenate(([0], np.cumsum([len(c.points) for c in ready]))).tolist()
    stage = _Staging.of(device)
    host = stage.take(4 * offsets[-1]).view(np.float32)
    for c, off in zip(ready, offsets):
        host[off:off + len(c.points)] = c.points
    points_dev = stage.upload(4 * offsets[-1], device)
    _launch(ready, points_dev, offsets, device)
    return [c.out if c.uv is None else (c.out, c.uv.view(torch.bool) if c.uv.dtype == torch.uint8 else c.uv) for c in ready]


def resample_uploaded(curves: Sequence[Curve], points: torch.Tensor, offsets: Sequence[int]) -> list:
    """The launches of `resample` alone, over points that are already on the device (fp32; curve i's start at
    points[offsets[i]]).  With `out` (and `uv`) given for every curve nothing is allocated, copied or synchronised, so the
    call can be captured into a graph and replayed over new points."""
    device = _device(points.device)
    if points.dtype != torch.float32 or not points.is_contiguous():
        raise ValueError("front.resample_uploaded: points must be a contiguous fp32 tensor")
    ready = _prepare(curves, device)
    for i, (c, off) in enumerate(zip(ready, offsets)):
        if off < 0 or off + len(c.points) > points.numel():
            raise ValueError(f"front.resample_uploaded: curve {i} reads past the uploaded points")
    _launch(ready, points, list(offsets), device)
    return [c.out if c.uv is None else (c.out, c.uv.view(torch.bool) if c.uv.dtype == torch.uint8 else c.uv) for c in ready]


@dataclass
class CurveSpec:
    """A curve of a segment for `segment_inputs`: its points (or `.ds` text), their timestep and the finishing op."""
    points: object
    src_step: float
    op: int = PLAIN
    lo: float = 0.0
    hi: float = 0.0
    uv: bool = False


def segment_inputs(frames: Sequence[Dict[str, np.ndarray]], lengths: Sequence[int], curves: Sequence[Dict[str, CurveSpec]],
                   timestep: float, device) -> dict:
    """The frame-level inputs of one segment (B = 1) or of a ragged group.
      frames     per segment: {name: frames per token} - what `seconds_to_frames` gave for its `ph_dur` (and `note_dur`),
                 after whatever the caller does to them on the host (padding tokens zeroed, phones aligned to the notes)
      lengths    per segment: its frame count T_i (durations past it are cut, frames past a total own no token: 0)
      curves     per segment: {name: CurveSpec}; a name some segment lacks leaves that segment's row zero
    Everything is packed into one pinned host buffer and travels in ONE copy; then one dsd_length_regulate per duration
    name and one dsd_curve_resample per MAX_CURVES curves write the rows of zero-padded tensors.  Nothing is read back.
    -> dict(dur={name: [B, L_max] int64}, mel2x={name: [B, T_max] int64}, curves={name: [B, T_max] fp32},
            uv={name: [B, T_max] bool}), T_max = max(lengths)."""
    device = _device(device)
    n_seg = len(frames)
    assert n_seg >= 1 and len(curves) == n_seg and len(lengths) == n_seg
    lengths = [int(t) for t in lengths]
    t_max = max(lengths)
    if t_max < 1:
        raise ValueError("front.segment_inputs: the durations give no frame")
    dur_names = list(dict.fromkeys(name for seg in frames for name in seg))
    l_max = {name: max(len(seg[name]) for seg in frames if name in seg) for name in dur_names}
    dur_off, nbytes = {}, 0
    for name in dur_names:
        dur_off[name] = nbytes
        nbytes += 8 * n_seg * l_max[name]
    dur_bytes = nbytes
    parsed = [{name: parse_curve(s.points) for name, s in seg.items()} for seg in curves]
    n_points = sum(len(p) for seg in parsed for p in seg.values())
    stage = _Staging.of(device)
    host = stage.take(dur_bytes + 4 * n_points)
    for name in dur_names:
        block = host[dur_off[name]:dur_off[name] + 8 * n_seg * l_max[name]].view(np.int64).reshape(n_seg, l_max[name])
        block[:] = 0
        for i, seg in enumerate(frames):
            if name in seg:
                block[i, :len(seg[name])] = seg[name]
    pts_host = host[dur_bytes:].view(np.float32)
    names = list(dict.fromkeys(name for seg in curves for name in seg))
    rows = {name: torch.zeros(n_seg, t_max, dtype=torch.float32, device=device) for name in names}
    uvs = {name: torch.zeros(n_seg, t_max, dtype=torch.uint8, device=device)
           for name in names if any(seg[name].uv for seg in curves if name in seg)}
    todo, offsets, off = [], [], 0
    for i, (seg, pts) in enumerate(zip(curves, parsed)):
        if lengths[i] < 1:
            continue                    # nothing to resample onto: the row stays zero
        for name, spec in seg.items():
            p = pts[name]
            pts_host[off:off + len(p)] = p
            todo.append(Curve(p, spec.src_step, timestep, lengths[i], spec.op, spec.lo, spec.hi, t_max, rows[name][i],
                              uvs[name][i] if name in uvs else None))
            offsets.append(off)
            off += len(p)
    blob = stage.upload(dur_bytes + 4 * n_points, device)
    stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    durs, mel2x = {}, {}
    for name in dur_names:
        durs[name] = blob[dur_off[name]:dur_off[name] + 8 * n_seg * l_max[name]].view(torch.int64).view(n_seg, l_max[name])
        mel2x[name] = torch.empty(n_seg, t_max, dtype=torch.int64, device=device)
        _refused(_lib.lib().dsd_length_regulate(device.index, C.c_void_p(durs[name].data_ptr()), n_seg, l_max[name], t_max,
                                                C.c_void_p(mel2x[name].data_ptr()), stream), "dsd_length_regulate")
    if todo:
        _launch(_prepare(todo, device), blob[dur_bytes:].view(torch.float32), offsets, device)
    return dict(dur=durs, mel2x=mel2x, curves=rows, uv={name: u.view(torch.bool) for name, u in uvs.items()})
