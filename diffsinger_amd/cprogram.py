"""The library's own program builder (dsd_ddpm_tables_fill / dsd_program_build / dsd_onnx_ddpm_plan) from Python.

What a C caller gets from include/dsdenoise.h, read back into the types of schedule.py so that the two can be compared:
`schedule.py` stays the scheduler of the Python shims (diffusion.py) and the yardstick the C builder is tested against.
Host only: nothing here needs a device.
"""
from __future__ import annotations

import ctypes as C
from contextlib import contextmanager
from typing import Tuple

import numpy as np

from . import _lib, schedule

RF_ALGORITHMS = ("euler", "rk2", "rk4", "rk5")


def tables(schedule_type: str = "linear", timesteps: int = 1000, max_beta: float = 0.01) -> schedule.DDPMTables:
    """dsd_ddpm_tables_fill as a schedule.DDPMTables."""
    if schedule_type not in _lib.SCHEDULE_IDS:
        raise ValueError(f"unknown schedule_type {schedule_type!r}")
    out = np.empty((_lib.DSD_DDPM_TABLES, max(int(timesteps), 0)), dtype=np.float32)
    rc = _lib.lib().dsd_ddpm_tables_fill(_lib.SCHEDULE_IDS[schedule_type], int(timesteps), float(max_beta),
                                         out.ctypes.data_as(C.POINTER(C.c_float)))
    _lib.check(None, rc, "dsd_ddpm_tables_fill")
    return schedule.DDPMTables.from_arrays(dict(zip(schedule.DDPMTables.NAMES, out)))


def tables_array(tb: schedule.DDPMTables) -> np.ndarray:
    """[12][timesteps] fp32, the `tables` of a dsd_sampler_spec."""
    return np.ascontiguousarray(np.stack([np.asarray(getattr(tb, n), dtype=np.float32) for n in schedule.DDPMTables.NAMES]))


def spec(sampler: str, tb: schedule.DDPMTables | None = None, t_max: int = 0, speedup: int = 1, t_lo: int = 0,
         noise_index0: int = 0, steps: int = 0, t_start: float = 0.0, time_scale_factor: float = 1000.0):
    """(DsdSamplerSpec, keepalive).  `sampler`: 'ddpm', 'ddim', 'pndm', 'dpm-solver', 'unipc' (with `tb`, t_max, speedup,
    t_lo, noise_index0) or 'rf_euler', 'rf_rk2', 'rf_rk4', 'rf_rk5', 'rf_euler_onnx' (with steps, t_start,
    time_scale_factor)."""
    if sampler not in _lib.SAMPLER_IDS:
        raise ValueError(f"unknown sampler {sampler!r}")
    s = _lib.DsdSamplerSpec()
    s.struct_size, s.sampler = C.sizeof(_lib.DsdSamplerSpec), _lib.SAMPLER_IDS[sampler]
    arr = None
    if tb is not None:
        arr = tables_array(tb)
        s.timesteps = arr.shape[1]
        s.tables = arr.ctypes.data_as(C.POINTER(C.c_float))
    s.t_max, s.speedup, s.t_lo, s.noise_index0, s.steps = int(t_max), int(speedup), int(t_lo), int(noise_index0), int(steps)
    s.t_start, s.time_scale_factor = float(t_start), float(time_scale_factor)
    return s, arr


@contextmanager
def built(sampler_spec):
    """The dsd_program as the library built it (a POINTER(DsdProgram), what dsd_sample takes); freed on exit."""
    p = C.POINTER(_lib.DsdProgram)()
    _lib.check(None, _lib.lib().dsd_program_build(C.byref(sampler_spec), C.byref(p)), "dsd_program_build")
    try:
        yield p
    finally:
        _lib.lib().dsd_program_free(p)


def from_c(prog) -> schedule.Program:
    """A DsdProgram read back as a schedule.Program (coefficients and times as the fp32 values the struct holds)."""
    evals = []
    for i in range(prog.n_evals):
        ce = prog.evals[i]
        ev = schedule.Eval(int(ce.x_buf), float(ce.t))
        for o in range(ce.n_out):
            lc = ce.out[o]
            ev.outs.append((int(lc.dst), [(int(lc.terms[k].src), float(lc.terms[k].coef)) for k in range(lc.n_terms)]))
        evals.append(ev)
    return schedule.Program(int(prog.n_bufs), int(prog.result_buf), evals, n_noise=int(prog.n_noise))


def build(sampler_spec) -> schedule.Program:
    """dsd_program_build, read back; `sampler_spec` is a DsdSamplerSpec or the (spec, keepalive) pair of spec()."""
    if isinstance(sampler_spec, tuple):
        sampler_spec = sampler_spec[0]
    with built(sampler_spec) as p:
        return from_c(p.contents)


def onnx_ddpm_plan(timesteps: int, k_step: int, factors, steps: int, depth=None) -> Tuple[int, int]:
    """dsd_onnx_ddpm_plan: (t_max, speedup), as schedule.onnx_ddpm_plan."""
    f = np.ascontiguousarray(np.asarray(factors, dtype=np.int64).reshape(-1))
    t_max, speedup = C.c_int32(), C.c_int32()
    rc = _lib.lib().dsd_onnx_ddpm_plan(int(timesteps), int(k_step), f.ctypes.data_as(C.POINTER(C.c_int64)), f.size, int(steps),
                                       -1.0 if depth is None else float(depth), C.byref(t_max), C.byref(speedup))
    _lib.check(None, rc, "dsd_onnx_ddpm_plan")
    return t_max.value, speedup.value
