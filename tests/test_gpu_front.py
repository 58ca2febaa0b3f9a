"""-m gpu: the segment front end on the device (dsd_curve_resample, diffsinger_amd/front.py, the harnesses' device_front
option, examples/c_abi_front.c) against numpy's own result (tests/front_ref.py: np.interp / np.arange exactly as the
reference calls them) and the reference's own (G27).

Every comparison is exact (assert_array_equal / torch.equal) but one.  The resampling performs numpy's IEEE double operations
in numpy's order, each rounded on its own, and rounds to fp32 once, so any difference is a bug - a single contracted fma is
one.  The exception is the PITCH op, which is evaluated in double where the host path works in fp32: its uv flags are
compared exactly, its values against a float64 oracle, where the device may deviate at most twice as far as the host numpy
path does on the same inputs (each side rounds the same chain - log2, stored interpolant, exp2, log2 - to fp32 and may land
on either neighbour at each step).

The shapes are sized by C = front.CHUNK, the frames a workgroup takes at a time.
"""
import copy
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import front_ref  # noqa: E402
from diffsinger_amd import front  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
C = front.CHUNK
HOP = front_ref.HOP


def host(t):
    return t.cpu().numpy()


def on_points(f0_like, **kw):
    """A curve whose frames sit on its points (src_step == dst_step, one point more than frames): frame k = point k."""
    pts = np.concatenate((np.asarray(f0_like, dtype=np.float32), np.zeros(1, np.float32)))
    return front.Curve(pts, HOP, HOP, len(pts) - 1, **kw)


class CountingLib:
    """The library with its dsd_curve_resample calls counted."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if name != "dsd_curve_resample":
            return fn

        def counted(device, arr, n, stream):
            self.calls.append(n)
            return fn(device, arr, n, stream)
        return counted


@pytest.fixture
def counting(monkeypatch):
    lib = CountingLib(front._lib.lib())
    monkeypatch.setattr(front._lib, "lib", lambda: lib)
    return lib


# ---- resampling --------------------------------------------------------------------------------------------------------
def test_cases_equal_numpy_and_the_reference(counting):
    """front_ref.curve_cases(): 2 and 3 points, equal steps (every frame on a source point), up- and down-sampling,
    incommensurate steps (0.005 -> 512/44100), lengths below, at and above the resampled count, length 1 - in ONE call."""
    g27 = np.load(os.path.join(GOLDEN, "g27_front.npz"))
    cases = front_ref.curve_cases()
    assert {2, 3} <= {len(c[1]) for c in cases} and any(c[4] == 1 for c in cases)
    assert any(c[2] == c[3] for c in cases) and any(c[2] < c[3] for c in cases) and any(c[2] > c[3] for c in cases)
    rel = {np.sign(c[4] - front_ref.resample_count(len(c[1]), c[2], c[3])) for c in cases}
    assert rel == {-1, 0, 1}
    got = front.resample([front.Curve(p, src, dst, n) for _, p, src, dst, n in cases], "cuda")
    assert counting.calls == [len(cases)] and len(cases) <= front.MAX_CURVES
    for (name, p, src, dst, n), out in zip(cases, got):
        assert out.dtype == torch.float32 and tuple(out.shape) == (n,)
        np.testing.assert_array_equal(host(out), front_ref.resample_numpy(p, src, dst, n), err_msg=name)
        np.testing.assert_array_equal(host(out), g27[f"rs_{name}"], err_msg=name)


def test_lengths_around_the_count_and_the_padding():
    """One curve at length = count - 1, count, count + 1 and 1, each into a row longer than it: the rest of the row is 0
    whatever was there, and nothing past the row is touched."""
    rng = np.random.Generator(np.random.PCG64(2720))
    p = rng.uniform(-2, 2, 300).astype(np.float32)
    count = front_ref.resample_count(300, 0.005, HOP)
    lengths, pad = [count - 1, count, count + 1, 1], count + 40
    block = torch.full((len(lengths) + 1, pad), float("nan"), device="cuda")
    front.resample([front.Curve(p, 0.005, HOP, n, pad_to=pad, out=block[i]) for i, n in enumerate(lengths)], "cuda")
    got = host(block)
    for i, n in enumerate(lengths):
        np.testing.assert_array_equal(got[i, :n], front_ref.resample_numpy(p, 0.005, HOP, n))
        assert not got[i, n:].any()
    assert np.isnan(got[-1]).all()


def test_one_frame_past_two_chunks():
    rng = np.random.Generator(np.random.PCG64(2721))
    n = 2 * C + 1
    p = rng.uniform(-2, 2, int(n * HOP / 0.005) + 9).astype(np.float32)
    out, = front.resample([front.Curve(p, 0.005, HOP, n)], "cuda")
    np.testing.assert_array_equal(host(out), front_ref.resample_numpy(p, 0.005, HOP, n))


def _mixed(n_curves, seed):
    """`n_curves` curves of every op and of lengths from 1 to past two chunks, with their host results."""
    rng = np.random.Generator(np.random.PCG64(seed))
    curves, want = [], []
    for i in range(n_curves):
        src, dst = front_ref.STEPS[int(rng.integers(0, 7))], front_ref.STEPS[int(rng.integers(0, 7))]
        n_pts = int(rng.integers(2, 700))
        length = 1 if i == 5 else max(1, front_ref.resample_count(n_pts, src, dst) + int(rng.integers(-5, 6)))
        op = i % 4
        p = rng.uniform(-1.5, 1.5, n_pts).astype(np.float32)
        if op == front.PITCH:
            p = np.where(rng.random(n_pts) < 0.3, 0.0, 200.0 + 100.0 * np.abs(p)).astype(np.float32)
        lo, hi = ((-5.0, 5.0) if op == front.GENDER else (-0.75, 0.5) if op == front.CLIP else (0.0, 0.0))
        curves.append(front.Curve(p, src, dst, length, op, lo, hi, pad_to=length + int(rng.integers(0, 9)),
                                  uv=True if op == front.PITCH else None))
        v = front_ref.resample_numpy(p, src, dst, length)
        want.append(v if op == front.PLAIN else front_ref.clip_host(v, lo, hi) if op == front.CLIP
                    else front_ref.gender_host(v, lo, hi) if op == front.GENDER else v)
    return curves, want


def _check_mixed(curves, want, got, errs):
    for c, w, g in zip(curves, want, got):
        if c.op == front.PITCH:
            out, uv = host(g[0]), host(g[1])
            oracle, uv64 = front_ref.pitch_oracle(w)
            np.testing.assert_array_equal(uv[:c.length], uv64)
            assert not uv[c.length:].any() and not out[c.length:].any()
            if uv64.all():
                assert np.isneginf(out[:c.length]).all()
            else:
                errs.append((np.abs(out[:c.length] - oracle).max(), np.abs(front_ref.pitch_host(w)[0] - oracle).max(), c.length))
        else:
            out = host(g)
            np.testing.assert_array_equal(out[:c.length], w)
            assert not out[c.length:].any()


def test_32_mixed_curves_in_one_call_and_33_split(counting):
    errs = []
    curves, want = _mixed(32, 2722)
    assert max(c.length for c in curves) > 2 * C
    _check_mixed(curves, want, front.resample(curves, "cuda"), errs)
    assert counting.calls == [32]
    curves, want = _mixed(33, 2723)
    _check_mixed(curves, want, front.resample(curves, "cuda"), errs)
    assert counting.calls == [32, 32, 1]
    assert max(e[0] for e in errs) <= 2 * max(e[1] for e in errs)


# ---- finishing ops -----------------------------------------------------------------------------------------------------
def test_clip_on_and_beyond_both_bounds():
    lo, hi = 0.5, 2.0
    v = np.array([0.5, 2.0, 0.49999997, 2.0000002, 0.50000006, 1.9999999, -3.0, 7.0, 1.0, 0.0, -0.0], np.float32)
    out, = front.resample([on_points(v, op=front.CLIP, lo=lo, hi=hi)], "cuda")
    np.testing.assert_array_equal(host(out), front_ref.clip_host(v, lo, hi))
    assert host(out).min() == lo and host(out).max() == hi
    # a bound that fp32 does not hold: the clip is torch's, against the bound rounded to fp32
    t = torch.clip(torch.from_numpy(v).cuda(), min=0.3, max=1.7)
    out, = front.resample([on_points(v, op=front.CLIP, lo=0.3, hi=1.7)], "cuda")
    assert torch.equal(out, t)


def test_gender_negative_zero_and_positive():
    lo, hi = -5.0, 12.0
    v = np.array([-1.0, -0.5, -0.1234567, -0.0, 0.0, 0.1234567, 0.5, 1.0, -1.3, 1.2, 1e-30, -1e-30], np.float32)
    out, = front.resample([on_points(v, op=front.GENDER, lo=lo, hi=hi)], "cuda")
    want = front_ref.gender_host(v, lo, hi)
    np.testing.assert_array_equal(host(out), want)
    np.testing.assert_array_equal(np.signbit(host(out)), np.signbit(want))
    assert want.min() == lo and want.max() == hi and (want == 0).any()
    with pytest.raises(ValueError, match="fp32"):
        front.resample([on_points(v, op=front.GENDER, lo=-0.1, hi=5.0)], "cuda")


# ---- PITCH -------------------------------------------------------------------------------------------------------------
def pitch_curves():
    """{name: f0 per frame}: unvoiced at the head, at the tail and inside; a gap across a chunk boundary (and one across
    two); one voiced frame; all voiced; all unvoiced; a voiced frame at the first and at the last place of a chunk."""
    rng = np.random.Generator(np.random.PCG64(2724))
    f0 = lambda n: rng.uniform(70.0, 900.0, n).astype(np.float32)          # noqa: E731
    out = {}
    v = f0(200)
    v[:11] = 0; v[60:75] = 0; v[120] = 0; v[-9:] = 0
    out["head_inside_tail"] = v
    v = f0(2 * C + 1)
    v[C - 20:C + 13] = 0; v[2 * C - 1:] = 0
    out["gap_over_a_boundary"] = v
    v = f0(3 * C + 5)
    v[C - 3:2 * C + 7] = 0; v[:C - 40] = 0
    out["gap_over_a_whole_chunk"] = v
    v = np.zeros(2 * C + 30, np.float32)
    v[C + 17] = 311.5
    out["one_voiced"] = v
    out["all_voiced"] = f0(C + 9)
    out["all_unvoiced"] = np.zeros(C + 3, np.float32)
    v = np.zeros(3 * C, np.float32)
    v[C - 1] = 100.0; v[C] = 0; v[2 * C] = 800.0
    out["chunk_edges"] = v
    v = f0(7)
    v[3] = 0
    out["short"] = v
    return out


def test_pitch_fill_uv_and_accuracy():
    cases = pitch_curves()
    got = front.resample([on_points(v, op=front.PITCH, uv=True) for v in cases.values()], "cuda")
    dev_err, host_err, frames = 0.0, 0.0, 0
    for (name, v), (out, uv) in zip(cases.items(), got):
        out, uv = host(out), host(uv)
        oracle, uv64 = front_ref.pitch_oracle(v)
        assert uv.dtype == np.bool_
        np.testing.assert_array_equal(uv, uv64, err_msg=name)
        if uv64.all():
            assert np.isneginf(out).all(), name
            continue
        assert np.isfinite(out).all(), name
        voiced = np.flatnonzero(~uv64)
        assert (out[:voiced[0]] == out[voiced[0]]).all() and (out[voiced[-1]:] == out[voiced[-1]]).all(), name   # the ends hold
        dev_err = max(dev_err, np.abs(out - oracle).max())
        host_err = max(host_err, np.abs(front_ref.pitch_host(v)[0] - oracle).max())
        frames += len(v)
    print(f"PITCH: {frames} frames, device max |error| {dev_err:.3e}, host numpy path {host_err:.3e} (MIDI)")
    assert frames >= 600
    assert dev_err <= 2 * host_err


def test_pitch_without_uv_and_through_a_resampling():
    """uv_out NULL; and a PITCH curve that is really resampled (0.005 -> hop): uv from the resampled f0, exactly."""
    rng = np.random.Generator(np.random.PCG64(2725))
    p = rng.uniform(100, 600, 500).astype(np.float32)
    p[40:90] = 0; p[300:420] = 0
    n = front_ref.resample_count(500, 0.005, HOP) + 3
    a, (b, uv) = front.resample([front.Curve(p, 0.005, HOP, n, front.PITCH), front.Curve(p, 0.005, HOP, n, front.PITCH, uv=True)],
                                "cuda")
    assert torch.equal(a, b)
    f0 = front_ref.resample_numpy(p, 0.005, HOP, n)
    oracle, uv64 = front_ref.pitch_oracle(f0)
    np.testing.assert_array_equal(host(uv), uv64)
    assert np.abs(host(a) - oracle).max() <= 2 * np.abs(front_ref.pitch_host(f0)[0] - oracle).max()


# ---- capture -----------------------------------------------------------------------------------------------------------
def test_capture_and_replay():
    """The launches over uploaded points, captured once and replayed over new points, give what an eager call gives."""
    rng = np.random.Generator(np.random.PCG64(2726))
    sizes, n = [400, 700, 90], 2 * C + 1
    offsets = [0, 400, 1100]
    points = torch.zeros(sum(sizes), device="cuda")
    outs = torch.zeros(3, n + 5, device="cuda")
    uv = torch.zeros(n + 5, dtype=torch.uint8, device="cuda")

    def curves(rows, uv_row):
        dummy = [np.zeros(s, np.float32) for s in sizes]
        return [front.Curve(dummy[0], 0.005, HOP, n, front.PLAIN, pad_to=n + 5, out=rows[0]),
                front.Curve(dummy[1], 0.005, HOP, n, front.PITCH, pad_to=n + 5, out=rows[1], uv=uv_row),
                front.Curve(dummy[2], 0.05, HOP, n, front.CLIP, -0.5, 0.5, pad_to=n + 5, out=rows[2])]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        front.resample_uploaded(curves(outs, uv), points, offsets)
    for seed in (1, 2):
        p = rng.uniform(-1, 1, sum(sizes)).astype(np.float32)
        p[400:1100] = np.where(rng.random(700) < 0.4, 0.0, 300.0 + 100.0 * p[400:1100])
        points.copy_(torch.from_numpy(p).cuda())
        outs.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        eager, eager_uv = torch.full_like(outs, float("nan")), torch.zeros_like(uv)
        front.resample_uploaded(curves(eager, eager_uv), points, offsets)
        assert torch.equal(outs, eager) and torch.equal(uv, eager_uv)
        np.testing.assert_array_equal(host(outs[0, :n]), front_ref.resample_numpy(p[:400], 0.005, HOP, n))
        np.testing.assert_array_equal(host(outs[2, :n]), front_ref.clip_host(front_ref.resample_numpy(p[1100:], 0.05, HOP, n), -0.5, 0.5))


# ---- the harnesses -----------------------------------------------------------------------------------------------------
def _same_batches(a, b, skip=()):
    assert set(a) == set(b)
    for k in a:
        if k in skip:
            continue
        if a[k] is None:
            assert b[k] is None, k
            continue
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k


def _clear(segments, keys):
    for s in segments:
        for k in keys:
            if k in s:
                assert front_ref.boundaries_clear_of_integers(np.array(s[k].split(), np.float32), HOP), k


@pytest.fixture(scope="module")
def project():
    """The acoustic harness of test_gpu_vocoder_ragged with a small model, and the G11 project re-timed: the fixture's own
    durations are random to 4 decimals and put boundaries within 0.05 frames of a rounding step (all three segments), where
    the default path's on-device cumsum may round the other way; front_ref.retimed moves every boundary to a half frame."""
    from diffsinger_amd import harness
    from diffsinger_amd.hparams import hparams
    from test_gpu_vocoder_ragged import _project_harness
    saved = dict(hparams)
    h = _project_harness()
    segs = [front_ref.retimed(s) for s in harness.load_ds(os.path.join(GOLDEN, "g11_segments.ds"))]
    _clear(segs, ("ph_dur",))
    yield h, segs, dict(hparams)
    hparams.clear()
    hparams.update(saved)


def test_acoustic_preprocess_and_collate(project):
    from diffsinger_amd.hparams import hparams
    h, segs, hp = project
    hparams.clear()
    hparams.update(hp)
    default = [h.preprocess_input(s, idx=i) for i, s in enumerate(segs)]
    assert any(b["key_shift"].size(1) > 1 for b in default) and any(b["speed"].size(1) > 1 for b in default)
    assert any(b["spk_mix_value"].size(1) > 1 for b in default)
    for s, d in zip(segs, default):
        _same_batches(d, h.preprocess_input(copy.deepcopy(s), device_front=True))
    group, rows = h.preprocess_group(copy.deepcopy(segs))
    for d, g in zip(default, group):
        _same_batches(d, g)
    want, lens = h.collate(default)
    got, lens_front = h.collate(group, rows)
    assert lens == lens_front and got["mel2ph"] is rows["mel2ph"] and got["f0"] is rows["f0"] and got["energy"] is rows["energy"]
    _same_batches(want, got)


def test_acoustic_segments_equal_the_reference():
    """front_ref.acoustic_segments() (boundaries at half frames): device_front gives the reference's own CPU tensors (G27)."""
    from diffsinger_amd import harness
    from diffsinger_amd.hparams import hparams
    g27 = np.load(os.path.join(GOLDEN, "g27_front.npz"))
    saved = dict(hparams)
    try:
        hparams.clear()
        hparams.update(front_ref.ACOUSTIC_HP)
        h = harness.AcousticHarness(None, None, harness.SimplePhonemeTable(front_ref.ACOUSTIC_PHONES), device="cuda")
        segs = front_ref.acoustic_segments()
        _clear(segs, ("ph_dur",))
        group, _ = h.preprocess_group(copy.deepcopy(segs))
        for i, (s, g) in enumerate(zip(segs, group)):
            one = h.preprocess_input(s, idx=i, device_front=True)
            _same_batches(h.preprocess_input(s, idx=i), one)
            _same_batches(one, g)
            for k, v in one.items():
                np.testing.assert_array_equal(host(v), g27[f"seg{i}_{k}"], err_msg=f"seg{i}_{k}")
    finally:
        hparams.clear()
        hparams.update(saved)


def test_acoustic_run_inference(project):
    from diffsinger_amd.hparams import hparams
    h, segs, hp = project
    hparams.clear()
    hparams.update(hp)
    for bs in (1, 4):
        want = h.run_inference(copy.deepcopy(segs), seed=7, device_noise=True, batch_size=bs)
        got = h.run_inference(copy.deepcopy(segs), seed=7, device_noise=True, batch_size=bs, device_front=True)
        assert want.dtype == got.dtype and want.shape == got.shape and want.any()
        np.testing.assert_array_equal(got, want)


def test_variance_preprocess():
    """G13's variance project re-timed to half-frame boundaries (segments 1 and 2 of the fixture are within 0.05 frames of
    a rounding step): every key of preprocess_input equal, whatever is loaded; `pitch` (load_pitch) within the PITCH bound."""
    import variance_cases as vc
    from diffsinger_amd import harness, variance_harness as vh
    from diffsinger_amd.hparams import hparams
    saved = dict(hparams)
    try:
        hparams.clear()
        hparams.update(vc.HARNESS_HP)
        h = vh.VarianceHarness(vc.FakeVarianceModel(), harness.SimplePhonemeTable(vc.HARNESS_PHONES), spk_map=vc.HARNESS_SPK,
                               device="cuda")
        segs = [front_ref.retimed(s) for s in harness.load_ds(os.path.join(GOLDEN, "g13_variance_segments.ds"))]
        _clear(segs, ("ph_dur", "note_dur"))
        seen_pitch = False
        for i, s in enumerate(segs):
            for load_dur in ((False, True) if "ph_dur" in s else (False,)):
                for load_pitch in ((False, True) if "f0_seq" in s else (False,)):
                    want = h.preprocess_input(copy.deepcopy(s), idx=i, load_dur=load_dur, load_pitch=load_pitch)
                    got = h.preprocess_input(copy.deepcopy(s), idx=i, load_dur=load_dur, load_pitch=load_pitch, device_front=True)
                    _same_batches(want, got, skip=("pitch",))
                    if load_pitch:
                        seen_pitch = True
                        f0 = h._curve(s, "f0_seq", "f0_timestep", want["pitch"].size(1))
                        oracle, uv = front_ref.pitch_oracle(f0)
                        assert uv.any() and got["pitch"].shape == want["pitch"].shape
                        assert np.abs(host(got["pitch"])[0] - oracle).max() <= 2 * np.abs(host(want["pitch"])[0] - oracle).max()
        assert seen_pitch
        # phones that do not add up to the notes: the last phone takes the rest / the phones are cut
        for scale in (0.8, 1.3):
            s = dict(segs[1])
            s["ph_dur"] = " ".join(repr(float(v) * scale) for v in s["ph_dur"].split())
            s = front_ref.retimed(s, keys=("ph_dur",))
            _clear([s], ("ph_dur",))
            _same_batches(h.preprocess_input(copy.deepcopy(s), load_dur=True), h.preprocess_input(copy.deepcopy(s), load_dur=True, device_front=True))
    finally:
        hparams.clear()
        hparams.update(saved)


# ---- a plain-C caller --------------------------------------------------------------------------------------------------
def test_c_example(tmp_path):
    exe = tmp_path / "c_abi_front"
    libdir = os.path.join(ROOT, "diffsinger_amd")
    cmd = ["gcc", "-std=c99", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "examples", "c_abi_front.c"), "-L" + libdir, "-ldsdenoise", "-L/opt/rocm/lib", "-lamdhip64", "-lm",
           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)]
    subprocess.run(cmd, check=True)
    res = subprocess.run([str(exe), str(tmp_path / "front.bin")], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    # the example's segment, restated
    sec = np.array([0.12, 0.305, 0.0, 0.61, 0.2175, 0.48, 0.57], np.float32)
    seconds = torch.from_numpy(sec)
    bounds = torch.round(torch.cumsum(seconds, dim=0) / HOP + 0.5).long()
    frames = torch.diff(bounds, dim=0, prepend=torch.zeros(1, dtype=torch.long)).numpy()
    lines = res.stdout.split("\n")
    assert lines[0] == "frames " + " ".join(str(int(f)) for f in frames) and lines[1] == f"total {int(frames.sum())}"
    i = np.arange(461)
    f0 = np.where((i < 9) | ((i >= 200) & (i < 262)) | (i >= 440), 0.0, 220.0 + 0.25 * ((i * 37) % 401)).astype(np.float32)
    energy = (-60.0 + 0.125 * ((np.arange(231) * 53) % 397)).astype(np.float32)
    velocity = (0.25 + 0.125 * ((np.arange(24) * 7) % 20)).astype(np.float32)
    raw = (tmp_path / "front.bin").read_bytes()
    T, = struct.unpack("<q", raw[:8])
    assert T == int(frames.sum()) and len(raw) == 8 + 8 * T + 12 * T + T
    mel2ph = np.frombuffer(raw, np.int64, T, 8)
    curves = np.frombuffer(raw, np.float32, 3 * T, 8 + 8 * T).reshape(3, T)
    uv = np.frombuffer(raw, np.uint8, T, 8 + 20 * T)
    np.testing.assert_array_equal(mel2ph, np.repeat(np.arange(1, 8), frames))
    np.testing.assert_array_equal(curves[1], front_ref.resample_numpy(energy, 0.01, HOP, T))
    speed = front_ref.clip_host(front_ref.resample_numpy(velocity, 0.1, HOP, T), 0.5, 2.0)
    np.testing.assert_array_equal(curves[2], speed)
    assert speed.min() == 0.5 and speed.max() == 2.0
    f0_frames = front_ref.resample_numpy(f0, 0.005, HOP, T)
    oracle, uv64 = front_ref.pitch_oracle(f0_frames)
    np.testing.assert_array_equal(uv.astype(bool), uv64)
    assert uv64[0] and uv64[-1] and uv64.sum() > 20 and not uv64.all()
    assert np.abs(curves[0] - oracle).max() <= 2 * np.abs(front_ref.pitch_host(f0_frames)[0] - oracle).max()
