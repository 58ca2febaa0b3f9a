"""The segment front end without a GPU: dsd_seconds_to_frames against torch's CPU expression, the rule's restatement and
the reference's own results (G27); every DSD_EINVAL of dsd_seconds_to_frames and dsd_curve_resample (decided before the
device is touched); and tests/front_ref.py itself against G27."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import front_ref
from diffsinger_amd import _lib, front

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g27_front.npz")


@pytest.fixture(scope="module")
def g27():
    return np.load(GOLDEN)


def torch_cpu_frames(sec, step):
    """inference/ds_acoustic.py:102-104 as the harness restates it, on the CPU."""
    seconds = torch.from_numpy(np.asarray(sec, dtype=np.float32))
    bounds = torch.round(torch.cumsum(seconds, dim=0) / step + 0.5).long()
    return torch.diff(bounds, dim=0, prepend=torch.zeros(1, dtype=torch.long)).numpy()


def test_seconds_to_frames_is_torch_cpu_and_g27(g27):
    cases = front_ref.duration_cases()
    assert {"one", "one_zero", "zero_inside"} <= {c[0] for c in cases}
    for name, sec, step in cases:
        frames, total = front.seconds_to_frames(sec, step)
        assert frames.dtype == np.int64 and frames.shape == sec.shape
        np.testing.assert_array_equal(frames, torch_cpu_frames(sec, step), err_msg=name)
        np.testing.assert_array_equal(frames, g27[f"dur_{name}"], err_msg=name)
        np.testing.assert_array_equal(frames, front_ref.seconds_to_frames(sec, step)[0], err_msg=name)
        assert total == int(frames.sum()) and (frames >= 0).all()


def test_accumulation_rule_bites():
    """At least 20 of the cases give other frames under a sequential fp32 running sum: the library's answer is the CPU's."""
    biting = 0
    for name, sec, step in front_ref.duration_cases():
        frames, _ = front.seconds_to_frames(sec, step)
        if not np.array_equal(frames, front_ref.seconds_to_frames_fp32_sum(sec, step)[0]):
            biting += 1
            np.testing.assert_array_equal(frames, torch_cpu_frames(sec, step), err_msg=name)
    assert biting >= 20


def test_seconds_to_frames_random_against_torch():
    rng = np.random.Generator(np.random.PCG64(2710))
    for _ in range(300):
        sec = rng.uniform(0.0, 0.7, int(rng.integers(1, 120))).round(6).astype(np.float32)
        step = front_ref.STEPS[int(rng.integers(0, len(front_ref.STEPS)))]
        np.testing.assert_array_equal(front.seconds_to_frames(sec, step)[0], torch_cpu_frames(sec, step))


def _s2f(sec, n, step, frames=True, total=True):
    lib = _lib.lib()
    buf = (C.c_float * max(len(sec), 1))(*sec)
    out = (C.c_int64 * max(len(sec), 1))()
    tot = C.c_int64(-7)
    rc = lib.dsd_seconds_to_frames(buf if sec is not None else None, n, step, out if frames else None,
                                   C.byref(tot) if total else None)
    return rc, lib.dsd_last_error(None).decode()


def test_seconds_to_frames_einval():
    ok = [0.1, 0.2]
    assert _s2f(ok, 2, 0.01)[0] == 0
    lib = _lib.lib()
    out, tot = (C.c_int64 * 2)(), C.c_int64()
    assert lib.dsd_seconds_to_frames(None, 2, 0.01, out, C.byref(tot)) == -1
    assert "null" in lib.dsd_last_error(None).decode()
    assert _s2f(ok, 2, 0.01, frames=False)[0] == -1
    assert _s2f(ok, 2, 0.01, total=False)[0] == -1
    for n in (0, -3):
        rc, msg = _s2f(ok, n, 0.01)
        assert rc == -1 and "n must be positive" in msg
    for step in (0.0, -0.01, math.nan, math.inf, -math.inf, 1e-60, 1e60):       # the last two are 0 and inf in fp32
        rc, msg = _s2f(ok, 2, step)
        assert rc == -1 and "timestep" in msg, step
    for bad in (math.nan, math.inf, -math.inf, -0.001):
        rc, msg = _s2f([0.1, bad], 2, 0.01)
        assert rc == -1 and "seconds[1]" in msg, bad
    rc, msg = _s2f([1.0, 3.0e7], 2, 0.01)                                       # 3e9 frames
    assert rc == -1 and "int32" in msg
    rc, msg = _s2f([3.0e38, 3.0e38], 2, 1.0)                                    # the fp32 prefix is inf
    assert rc == -1 and "int32" in msg
    assert _s2f([0.0, -0.0], 2, 0.01)[0] == 0                                   # a negative zero is a zero
    with pytest.raises(ValueError, match="n must be positive"):
        front.seconds_to_frames([], 0.01)


def _descriptor(**kw):
    host = (C.c_float * 16)()
    d = dict(points=C.addressof(host), out=C.addressof(host), uv_out=None, src_step=0.005, dst_step=front_ref.HOP,
             n_points=8, length=4, pad_to=4, op=_lib.DSD_CURVE_PLAIN, lo=0.0, hi=0.0)
    d.update(kw)
    c = _lib.DsdCurve()
    for k, v in d.items():
        setattr(c, k, v)
    return c, host


def _resample_rc(curves, n=None):
    lib = _lib.lib()
    arr = (_lib.DsdCurve * max(len(curves), 1))(*curves)
    rc = lib.dsd_curve_resample(0, arr, len(curves) if n is None else n, None)
    return rc, lib.dsd_last_error(None).decode()


def test_curve_resample_einval():
    """Every refusal is DSD_EINVAL, decided before the device is looked at (so it is the same with and without a GPU), and
    names the curve and the field.  The pointers are host addresses: nothing is dereferenced."""
    lib = _lib.lib()
    assert lib.dsd_curve_resample(0, None, 1, None) == -1 and "null" in lib.dsd_last_error(None).decode()
    good, keep = _descriptor()
    for n in (0, -1, 33):
        rc, msg = _resample_rc([good], n)
        assert rc == -1 and "n_curves" in msg
    nan, inf = math.nan, math.inf
    bad = [(dict(points=None), "points"), (dict(out=None), "out"), (dict(n_points=1), "n_points"), (dict(n_points=0), "n_points"),
           (dict(n_points=-5), "n_points"), (dict(length=0), "length"), (dict(length=-1), "length"), (dict(pad_to=3), "pad_to"),
           (dict(src_step=0.0), "src_step"), (dict(src_step=-0.01), "src_step"), (dict(src_step=nan), "src_step"),
           (dict(src_step=inf), "src_step"), (dict(dst_step=0.0), "dst_step"), (dict(dst_step=-1.0), "dst_step"),
           (dict(dst_step=nan), "dst_step"), (dict(dst_step=inf), "dst_step"), (dict(op=4), "unknown op"), (dict(op=-1), "unknown op"),
           (dict(op=_lib.DSD_CURVE_CLIP, lo=1.0, hi=0.5), "CLIP"), (dict(op=_lib.DSD_CURVE_CLIP, lo=nan, hi=0.5), "CLIP"),
           (dict(op=_lib.DSD_CURVE_CLIP, lo=0.0, hi=nan), "CLIP"), (dict(op=_lib.DSD_CURVE_GENDER, lo=1.0, hi=5.0), "GENDER"),
           (dict(op=_lib.DSD_CURVE_GENDER, lo=-5.0, hi=-1.0), "GENDER"), (dict(op=_lib.DSD_CURVE_GENDER, lo=-inf, hi=5.0), "GENDER"),
           (dict(op=_lib.DSD_CURVE_GENDER, lo=nan, hi=5.0), "GENDER"), (dict(uv_out=C.addressof(keep)), "uv_out"),
           (dict(op=_lib.DSD_CURVE_CLIP, lo=0.0, hi=1.0, uv_out=C.addressof(keep)), "uv_out"),
           (dict(src_step=1e-300, dst_step=1e300), "no frame")]
    for kw, word in bad:
        c, hold = _descriptor(**kw)
        rc, msg = _resample_rc([good, c])
        assert rc == -1, kw
        assert "curve 1" in msg and word in msg, (kw, msg)
    # a descriptor that passes every check gets as far as the device selection: not EINVAL but "no HIP device".  Only where
    # there is no device - with one the call would launch, and these pointers are host addresses.
    if not torch.cuda.is_available():
        rc, msg = _resample_rc([good])
        assert rc not in (0, -1) and "no HIP device" in msg


def test_python_side_refuses_before_the_library():
    with pytest.raises(RuntimeError, match="no CPU path"):
        front.resample([front.Curve(np.zeros(4, np.float32), 0.01, 0.01, 3)], "cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        front.segment_inputs([{"ph": np.array([3])}], [3], [{}], 0.01, "cpu")


def test_front_ref_against_g27(g27):
    """The restated resampling rule, numpy's own interp and the harness's host function all give the reference's curves."""
    from diffsinger_amd.harness import resample_align_curve
    for name, pts, src, dst, length in front_ref.curve_cases():
        want = g27[f"rs_{name}"]
        assert want.dtype == np.float32 and want.shape == (length,)
        np.testing.assert_array_equal(front_ref.resample_rule(pts, src, dst, length), want, err_msg=name)
        np.testing.assert_array_equal(front_ref.resample_numpy(pts, src, dst, length), want, err_msg=name)
        np.testing.assert_array_equal(resample_align_curve(pts, src, dst, length), want, err_msg=name)


def test_front_ref_ops_against_g27(g27):
    """The host forms of CLIP and GENDER in front_ref give the reference's `speed` and `key_shift`, and the frame counts
    give its mel2ph, on the acoustic segments."""
    hp = front_ref.ACOUSTIC_HP["augmentation_args"]
    shifts = []
    for i, seg in enumerate(front_ref.acoustic_segments()):
        sec = np.array(seg["ph_dur"].split(), np.float32)
        assert front_ref.boundaries_clear_of_integers(sec, front_ref.HOP)
        frames, total = front.seconds_to_frames(sec, front_ref.HOP)
        mel2ph = g27[f"seg{i}_mel2ph"]
        assert mel2ph.shape == (1, total)
        np.testing.assert_array_equal(np.repeat(np.arange(1, len(frames) + 1), frames), mel2ph[0])
        curve = lambda key: front_ref.resample_numpy(np.array(seg[key].split(), np.float32),           # noqa: E731
                                                     float(seg["f0_timestep" if key == "f0_seq" else key + "_timestep"]),
                                                     front_ref.HOP, total)
        np.testing.assert_array_equal(curve("f0_seq"), g27[f"seg{i}_f0"][0])
        np.testing.assert_array_equal(curve("energy"), g27[f"seg{i}_energy"][0])
        if isinstance(seg["gender"], str):
            lo, hi = hp["random_pitch_shifting"]["range"]
            got = front_ref.gender_host(curve("gender"), lo, hi)
            np.testing.assert_array_equal(got, g27[f"seg{i}_key_shift"][0])
            shifts.append(got)
        if "velocity" in seg:
            lo, hi = hp["random_time_stretching"]["range"]
            np.testing.assert_array_equal(front_ref.clip_host(curve("velocity"), lo, hi), g27[f"seg{i}_speed"][0])
    shifts = np.concatenate(shifts)
    assert shifts.min() == -5.0 and shifts.max() == 5.0             # the gender curves reach past both bounds


def test_pitch_oracle_and_host_path_agree():
    """The float64 oracle and the host path differ by fp32 roundings only, uv is the same, -inf where nothing is voiced."""
    from diffsinger_amd.variance_harness import hz_to_midi, interp_f0
    rng = np.random.Generator(np.random.PCG64(2711))
    f0 = rng.uniform(80, 800, 300).astype(np.float32)
    f0[:7] = 0
    f0[100:140] = 0
    f0[-3:] = 0
    host, uv = front_ref.pitch_host(f0)
    np.testing.assert_array_equal(host, hz_to_midi(interp_f0(f0.copy())[0]).astype(np.float32))
    oracle, uv64 = front_ref.pitch_oracle(f0)
    np.testing.assert_array_equal(uv, uv64)
    assert np.abs(host.astype(np.float64) - oracle).max() < 2e-4
    assert np.isneginf(front_ref.pitch_oracle(np.zeros(5, np.float32))[0]).all()
    assert np.isneginf(front_ref.pitch_host(np.zeros(5, np.float32))[0]).all()
