"""Numpy restatements of the segment front end's two rules (include/dsdenoise.h: dsd_seconds_to_frames,
dsd_curve_resample), a float64 oracle of the PITCH op, and the seeded cases that tests/golden/make_golden_front.py (G27),
tests/test_front_host.py and tests/test_gpu_front.py share.  Nothing here calls the library."""
import numpy as np

STEPS = (0.005, 0.01, 0.02, 512 / 44100, 256 / 44100, 128 / 24000, 0.0116099773)
HOP = 512 / 44100


# ------------------------------------------------------------------------------------------------ durations -> frames
def seconds_to_frames(seconds, timestep):
    """The rule: a double running sum of the fp32 inputs, every prefix rounded to fp32, an fp32 divide, + 0.5f, half to even."""
    sec = np.asarray(seconds, dtype=np.float32)
    c = np.cumsum(sec.astype(np.float64)).astype(np.float32)
    b = np.rint(c / np.float32(timestep) + np.float32(0.5)).astype(np.int64)
    return np.diff(b, prepend=0), int(b[-1])


def seconds_to_frames_fp32_sum(seconds, timestep):
    """The same with a sequential fp32 running sum: what an accumulation rule that is NOT the CPU's gives."""
    c = np.cumsum(np.asarray(seconds, dtype=np.float32))
    assert c.dtype == np.float32
    b = np.rint(c / np.float32(timestep) + np.float32(0.5)).astype(np.int64)
    return np.diff(b, prepend=0), int(b[-1])


def duration_cases():
    """[(name, fp32 seconds, timestep)]: the edges, a dozen plain draws, and 24 cases found by a seeded search for inputs
    on which the sequential-fp32 sum gives other frames (durations rounded to 6 decimals, 1-199 tokens)."""
    cases = [("one", np.array([0.37], np.float32), HOP),
             ("one_zero", np.array([0.0], np.float32), HOP),
             ("zero_inside", np.array([0.12, 0.0, 0.3, 0.0, 0.0, 0.05], np.float32), HOP),
             ("half_frames", (np.array([3.5, 2.0, 1.5, 4.0, 0.5]) * 0.01).astype(np.float32), 0.01)]
    rng = np.random.Generator(np.random.PCG64(2700))
    for k in range(12):
        n = int(rng.integers(1, 200))
        cases.append((f"plain{k}", rng.uniform(0.02, 0.6, n).round(6).astype(np.float32), STEPS[k % len(STEPS)]))
    found = 0
    while found < 24:
        n = int(rng.integers(1, 200))
        sec = rng.uniform(0.02, 0.6, n).round(6).astype(np.float32)
        step = STEPS[int(rng.integers(0, len(STEPS)))]
        if not np.array_equal(seconds_to_frames(sec, step)[0], seconds_to_frames_fp32_sum(sec, step)[0]):
            cases.append((f"bite{found}", sec, step))
            found += 1
    return cases


# ------------------------------------------------------------------------------------------------------- resampling
def resample_numpy(points, src_step, dst_step, length):
    """utils/infer_utils.py:41-53 with numpy's own interp and arange: what the device result must equal bit for bit."""
    points = np.asarray(points, dtype=np.float32)
    src_t = src_step * np.arange(len(points))
    dst_t = np.arange(0, (len(points) - 1) * src_step, dst_step)
    curve = np.interp(dst_t, src_t, points).astype(points.dtype)
    if len(curve) >= length:
        return curve[:length]
    return np.concatenate((curve, np.full(length - len(curve), fill_value=curve[-1])), axis=0)


def resample_count(n_points, src_step, dst_step):
    return int(np.ceil(((n_points - 1) * src_step) / dst_step))


def resample_rule(points, src_step, dst_step, length):
    """The rule of the header spelled out frame by frame, in Python floats (IEEE double, nothing contracted)."""
    p = [float(v) for v in np.asarray(points, dtype=np.float32)]
    n = len(p)
    src_step, dst_step = float(src_step), float(dst_step)
    count = resample_count(n, src_step, dst_step)
    out = np.empty(length, dtype=np.float32)
    for k in range(min(count, length)):
        x = k * dst_step
        j = min(int(x / src_step), n - 1)
        while j > 0 and src_step * j > x:
            j -= 1
        while j < n - 1 and src_step * (j + 1) <= x:
            j += 1
        if j >= n - 1:
            v = p[n - 1]
        elif src_step * j == x:
            v = p[j]
        else:
            v = ((p[j + 1] - p[j]) / (src_step * (j + 1) - src_step * j)) * (x - src_step * j) + p[j]
        out[k] = np.float32(v)
    out[min(count, length):] = out[min(count, length) - 1]
    return out


def curve_cases():
    """[(name, fp32 points, src_step, dst_step, length)]: the edges, then seeded draws over STEPS, 2-399 points and
    lengths within +-5 of the resampled count."""
    rng = np.random.Generator(np.random.PCG64(2701))
    pts = lambda n: rng.uniform(-3, 3, n).astype(np.float32)        # noqa: E731
    cases = [("two_points", pts(2), 0.05, HOP, 7), ("three_points", pts(3), 0.02, 0.005, 9),
             ("same_step", pts(40), 0.01, 0.01, 39), ("same_step_hop", pts(33), HOP, HOP, 40),
             ("up", pts(25), 0.02, 0.005, 96), ("down", pts(200), 0.005, 0.02, 50),
             ("incommensurate", pts(300), 0.005, HOP, resample_count(300, 0.005, HOP)),
             ("length_one", pts(17), 0.01, HOP, 1)]
    for k in range(16):
        n = int(rng.integers(2, 400))
        src, dst = STEPS[int(rng.integers(0, len(STEPS)))], STEPS[int(rng.integers(0, len(STEPS)))]
        length = max(1, resample_count(n, src, dst) + int(rng.integers(-5, 6)))
        cases.append((f"draw{k}", pts(n), src, dst, length))
    return cases


# ------------------------------------------------------------------------------------------------------ finishing ops
def clip_host(v, lo, hi):
    """torch.clip of an fp32 tensor: the bounds in fp32."""
    return np.minimum(np.maximum(v, np.float32(lo)), np.float32(hi)).astype(np.float32)


def gender_host(v, lo, hi):
    """ds_acoustic.py:154-159 as the harness restates it: the product in float64, then fp32, then the clip."""
    up = v >= 0
    shift = v * (up * hi + (1 - up) * abs(lo))
    assert shift.dtype == np.float64
    return clip_host(shift.astype(np.float32), lo, hi)


def pitch_host(f0):
    """The host path of `load_pitch` (variance_harness.py: interp_f0, hz_to_midi): fp32 log2, the interpolant stored in
    fp32, fp32 exp2, fp32 log2 -> (MIDI as fp32, uv)."""
    f0 = np.asarray(f0, dtype=np.float32)
    uv = f0 == 0
    logf = np.log2(f0 + uv)
    logf[uv] = -np.inf
    if uv.any() and not uv.all():
        logf[uv] = np.interp(np.where(uv)[0], np.where(~uv)[0], logf[~uv])
    filled = 2 ** logf
    assert logf.dtype == np.float32 and filled.dtype == np.float32
    with np.errstate(divide="ignore"):
        return (12 * (np.log2(filled) - np.log2(440.0)) + 69).astype(np.float32), uv


def pitch_oracle(f0):
    """The same curve in float64 throughout: log2 of the fp32 f0, the interpolation, the MIDI map -> (float64, uv)."""
    f0 = np.asarray(f0, dtype=np.float32).astype(np.float64)
    uv = f0 == 0
    logf = np.full(f0.shape, -np.inf)
    logf[~uv] = np.log2(f0[~uv])
    if uv.any() and not uv.all():
        logf[uv] = np.interp(np.where(uv)[0], np.where(~uv)[0], logf[~uv])
    return 12 * (logf - np.log2(440.0)) + 69, uv


# ------------------------------------------------------------------------------------------ acoustic segments (G27)
ACOUSTIC_HP = dict(hop_size=512, audio_sample_rate=44100, use_spk_id=False, use_lang_id=False, use_energy_embed=True,
                   use_breathiness_embed=True, use_key_shift_embed=True, use_speed_embed=True,
                   augmentation_args=dict(random_pitch_shifting=dict(range=[-5.0, 5.0]),
                                          random_time_stretching=dict(range=[0.5, 2.0])))
ACOUSTIC_PHONES = ["a", "b", "c", "d", "e"]


def acoustic_segments():
    """A dozen seeded `.ds` segments: every curve the acoustic front end resamples, at timesteps from STEPS, the gender and
    velocity curves reaching past both bounds.  The cumulative duration boundaries sit at half frames (k + 0.5), as far
    from a rounding step as they can be, so that no accumulation order can move one."""
    rng = np.random.Generator(np.random.PCG64(2702))
    names = ACOUSTIC_PHONES + ["SP", "AP"]
    segs = []
    for i in range(12):
        n_ph = int(rng.integers(1, 14))
        bounds = np.cumsum(rng.integers(2, 30, n_ph)) + 0.5
        dur = np.diff(bounds * HOP, prepend=0.0)
        total = float(bounds[-1] * HOP)
        seg = {"offset": 0.0, "ph_seq": " ".join(names[int(k)] for k in rng.integers(0, len(names), n_ph)),
               "ph_dur": " ".join(repr(float(v)) for v in dur)}
        for key, lo, hi in (("f0_seq", 80.0, 800.0), ("energy", -60.0, -10.0), ("breathiness", -70.0, -20.0),
                            ("gender", -1.4, 1.4), ("velocity", 0.2, 2.6)):
            step = STEPS[int(rng.integers(0, len(STEPS)))]
            n = max(2, int(total / step) + int(rng.integers(-3, 4)))
            seg[key] = " ".join(str(v) for v in rng.uniform(lo, hi, n).round(3))
            seg["f0_timestep" if key == "f0_seq" else key + "_timestep"] = repr(step)
        if i % 4 == 3:
            seg["gender"] = 0.3
            del seg["velocity"]
        segs.append(seg)
    return segs


def boundaries_clear_of_integers(seconds, timestep, margin=0.05):
    """Every cumulative boundary cumsum(seconds) / timestep, in float64, is at least `margin` frames from an integer: that
    is where round(boundary + 0.5) steps, so no accumulation order or device can move a frame count."""
    b = np.cumsum(np.asarray(seconds, dtype=np.float32).astype(np.float64)) / float(timestep)
    return bool(np.all(np.abs(b - np.rint(b)) >= margin))


def retimed(segment, keys=("ph_dur", "note_dur"), timestep=HOP):
    """A copy of a fixture segment whose duration fields are moved so that every cumulative boundary sits at a half frame
    (the boundary's own frame + 0.5): the fixtures' durations are random to 4 decimals and some of their boundaries come
    within 0.05 frames of a rounding step, where the default path's on-device cumsum may round the other way."""
    out = dict(segment)
    for key in keys:
        if key in segment:
            b = np.cumsum(np.array(segment[key].split(), np.float64)) / timestep
            snapped = (np.floor(b) + 0.5) * timestep
            out[key] = " ".join(repr(float(v)) for v in np.diff(snapped, prepend=0.0))
    return out
