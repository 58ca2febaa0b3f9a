"""-m gpu: a project's track on the device (dsd_track_place / _peak / _export, diffsinger_amd/track.py,
run_inference(device_mix=True), examples/c_abi_track.c) against tests/track_ref.py - the reference's fold restated with
harness.cross_fade, and save_wav's arithmetic.

Every comparison is exact (assert_array_equal in float64, int16 or bytes).  Both sides perform the same IEEE-754 operations
in the same order - a product, a product and a sum per faded sample, each rounded to float64; one product (or a quotient
and a product) and a truncation per exported sample; a maximum, which has no order - so any difference is a bug, and a
single contracted fma in the blend is one.  The shapes are sized by W = track.SPAN, the samples one workgroup covers.
"""
import copy
import math
import os
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import track_ref  # noqa: E402
from diffsinger_amd import track  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = track.SPAN


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def place_all(starts, wavs, buf=None):
    """The segments placed in order into a track that is NaN everywhere first -> the Track."""
    lengths = [len(w) for w in wavs]
    ends, total = track_ref.layout_plan(starts, lengths)
    t = track.Track(total, "cuda")
    if buf is not None:
        t.buf = buf
    t.buf.fill_(float("nan"))
    for s, p, w in zip(starts, ends, wavs):
        t.place_at(s, p, cuda(w))
    return t


def waves(lengths, seed):
    return [track_ref.waveform(seed + k, n) for k, n in enumerate(lengths)]


# (starts, lengths).  Two segments [a, a + n0) and a second one at gap g or overlap F behind / inside it
def _two(a, n0, n1, gap=None, fade=None):
    return ([a, a + n0 + gap] if fade is None else [a, a + n0 - fade]), [n0, n1]


CASES = {
    # one segment of every length class, at 0 and behind leading silence of odd and even length
    **{f"n{n}_at{a}": ([a], [n]) for n in (1, W - 1, W, W + 1, 3 * W + 5) for a in (0, 3, W + 2)},
    # gaps 0, 1, W + 1 behind a segment of odd and of even end
    **{f"gap{g}_end{n0}": _two(0, n0, W + 1, gap=g) for g in (0, 1, W + 1) for n0 in (W - 1, W)},
    # fades 1, 2, 3, W + 1 at odd and even starts; F = n for n = 1, W - 1, W + 1
    **{f"fade{f}_start{a}": _two(a, 2 * W + 7, 3 * W + 5, fade=f) for f in (1, 2, 3, W + 1) for a in (0, 1)},
    **{f"fade_whole{n}_start{a}": _two(a, 2 * W + 6, n, fade=n) for n in (1, 2, W - 1, W + 1) for a in (0, 1)},
    "fade3_into_n3": _two(5, W, 3, fade=3),
    # a third segment inside the fade of the first two; a segment that starts before its predecessor's start; both at once
    "third_inside_fade": ([0, 2 * W, 2 * W + 100], [3 * W, 2 * W + 1, 3 * W + 5]),
    "before_predecessor": ([7, 2 * W + 1, 2 * W - 100], [2 * W + 50, 60, W + 200]),
    "chain": ([1, W, W - 1, 3 * W + 3, 6 * W + 3], [W + 30, 2 * W, 3 * W + 5, W + 1, 1]),
}


@pytest.mark.parametrize("name", list(CASES))
def test_place_equals_the_fold(name):
    starts, lengths = CASES[name]
    wavs = waves(lengths, 2500)
    want = track_ref.fold_starts(starts, wavs)
    got = place_all(starts, wavs).numpy()
    assert got.dtype == np.float64 and not np.isnan(got).any()              # no sample left unwritten
    np.testing.assert_array_equal(got, want)


def test_place_every_golden_layout():
    g24 = np.load(track_ref.GOLDEN)
    for name, sr, offsets, lengths, seeds in track_ref.LAYOUTS:
        wavs = track_ref.layout_waves(lengths, seeds)
        layout = track.plan(offsets, lengths, sr)
        t = track.Track(layout.total, "cuda", layout)
        t.buf.fill_(float("nan"))
        for k, w in enumerate(wavs):
            t.place(k, cuda(w))
        np.testing.assert_array_equal(t.numpy(), g24[f"{name}_track"], err_msg=name)
        np.testing.assert_array_equal(t.export("pcm").cpu().numpy(), g24[f"{name}_pcm"], err_msg=name)
        np.testing.assert_array_equal(t.export("pcm", norm=True).cpu().numpy(), g24[f"{name}_pcm_norm"], err_msg=name)
        assert float(t.compute_peak().cpu()[0]) == np.abs(g24[f"{name}_track"]).max()


def test_track_at_an_odd_double():
    """A track whose first sample is 8 but not 16 bytes aligned: the pairs then start at the odd indices."""
    starts, lengths = CASES["chain"]
    wavs = waves(lengths, 2600)
    want = track_ref.fold_starts(starts, wavs)
    big = torch.empty(want.shape[0] + 1, dtype=torch.float64, device="cuda")
    assert big.data_ptr() % 16 == 0
    t = place_all(starts, wavs, buf=big[1:])
    np.testing.assert_array_equal(t.numpy(), want)
    assert float(t.compute_peak().cpu()[0]) == np.abs(want).max()
    np.testing.assert_array_equal(t.export("f64").cpu().numpy(), want)
    np.testing.assert_array_equal(t.export("f32").cpu().numpy(), want.astype(np.float32))
    np.testing.assert_array_equal(t.export("pcm", norm=True).cpu().numpy(), track_ref.pcm(want, norm=True))
    odd_out = torch.zeros(want.shape[0] + 1, dtype=torch.int16, device="cuda")[1:]       # ... and an out at an odd element
    np.testing.assert_array_equal(t.export("pcm", out=odd_out).cpu().numpy(), track_ref.pcm(want))


def test_place_refuses_on_the_device_too():
    t = track.Track(100, "cuda")
    with pytest.raises(ValueError, match="dsd_track_place: .* ends past the track's 100 samples"):
        t.place_at(90, 0, torch.zeros(11, device="cuda"))
    with pytest.raises(ValueError, match="the overlap of 6 samples is longer than the segment's 5"):
        t.place_at(10, 16, torch.zeros(5, device="cuda"))


def _values(n, seed):
    """A float64 track with more bits than fp32 holds, |v| < 1."""
    a = track_ref.waveform(seed, n).astype(np.float64)
    return a * 0.73 + track_ref.waveform(seed + 1, n).astype(np.float64) * 2.0 ** -27


@pytest.mark.parametrize("n", [1, 2, W - 1, W, W + 1, 3 * W + 5])
def test_export_and_peak(n):
    v = _values(n, 2700 + n)
    t = track.Track(n, "cuda")
    t.buf.copy_(cuda(v))
    np.testing.assert_array_equal(t.export("f64").cpu().numpy(), v)
    f32 = t.export("f32").cpu().numpy()
    assert f32.dtype == np.float32 and not np.array_equal(f32.astype(np.float64), v)
    np.testing.assert_array_equal(f32, v.astype(np.float32))
    assert float(t.compute_peak().cpu()[0]) == np.abs(v).max()
    pcm, pcm_norm = t.export("pcm").cpu().numpy(), t.export("pcm", norm=True).cpu().numpy()
    assert pcm.dtype == np.int16
    np.testing.assert_array_equal(pcm, track_ref.pcm(v))
    np.testing.assert_array_equal(pcm_norm, track_ref.pcm(v, norm=True))
    assert np.abs(pcm_norm.astype(np.int32)).max() == 32767
    np.testing.assert_array_equal(t.numpy(), v)                             # exports leave the track alone


def test_pcm_saturates_and_a_zero_peak_gives_zeros():
    v = np.array([1.5, -1.5, 1.0, -1.0, 32767.4 / 32767, -32768.9 / 32767, 0.99999, -0.99999, 0.0, -0.0, 1e300, -1e300,
                  float("inf"), float("-inf"), 2.0 ** -1074, 0.5 / 32767, -0.5 / 32767, 1.0 / 32767])
    t = track.Track(v.shape[0], "cuda")
    t.buf.copy_(cuda(v))
    got = t.export("pcm").cpu().numpy()
    assert got[:4].tolist() == [32767, -32768, 32767, -32767]
    np.testing.assert_array_equal(got, track_ref.pcm(v))
    t.buf.zero_()
    assert float(t.compute_peak().cpu()[0]) == 0.0
    assert not t.export("pcm", norm=True).cpu().numpy().any()
    assert not t.export("pcm").cpu().numpy().any()


def test_peak_is_exact_and_sees_a_negative_maximum_in_the_last_workgroup():
    n = 2 * W + 37
    v = _values(n, 2800)
    v[n - 3] = -1.75 - 2.0 ** -40
    t = track.Track(n, "cuda")
    t.buf.copy_(cuda(v))
    t.peak.fill_(123.0)                                                     # the call zeroes it itself
    assert float(t.compute_peak().cpu()[0]) == 1.75 + 2.0 ** -40 == np.abs(v).max()
    np.testing.assert_array_equal(t.export("pcm", norm=True).cpu().numpy(), track_ref.pcm(v, norm=True))
    v[5] = float("nan")
    t.buf.copy_(cuda(v))
    assert math.isnan(float(t.compute_peak().cpu()[0]))                     # as np.abs(v).max()


def test_capture_and_replay():
    """Place x 3 + peak + export in one captured chain on one stream, replayed twice with new segment contents."""
    starts, lengths = [3, W + 1, 4 * W], [W + 40, 2 * W + 1, W - 1]
    ends, total = track_ref.layout_plan(starts, lengths)
    t = track.Track(total, "cuda")
    segs = [torch.zeros(n, device="cuda") for n in lengths]
    pcm = torch.zeros(total, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for s, p, seg in zip(starts, ends, segs):
            t.place_at(s, p, seg)
        t.export("pcm", norm=True, out=pcm)
    for seed in (2900, 2950):
        wavs = waves(lengths, seed)
        for seg, w in zip(segs, wavs):
            seg.copy_(cuda(w))
        t.buf.fill_(float("nan"))
        pcm.zero_()
        graph.replay()
        torch.cuda.synchronize()
        want = track_ref.fold_starts(starts, wavs)
        np.testing.assert_array_equal(t.numpy(), want)
        assert float(t.peak.cpu()[0]) == np.abs(want).max()
        np.testing.assert_array_equal(pcm.cpu().numpy(), track_ref.pcm(want, norm=True))


# ---- a project through the harness ------------------------------------------------------------------------------------
def test_harness_device_mix(tmp_path):
    from diffsinger_amd import harness
    from diffsinger_amd.hparams import hparams
    from test_gpu_vocoder import GOLDEN
    from test_gpu_vocoder_ragged import _project_harness
    saved = dict(hparams)
    try:
        h = _project_harness()
        segs = [dict(s) for s in copy.deepcopy(harness.load_ds(os.path.join(GOLDEN, "g11_segments.ds")))]
        segs[1]["offset"], segs[2]["offset"] = 0.7, 2.0             # the first pair overlaps, the second has a gap
        sr, hop = hparams["audio_sample_rate"], hparams["hop_size"]
        lengths = [int(h.preprocess_input(s, idx=i)["mel2ph"].size(1)) * hop for i, s in enumerate(segs)]
        layout = track.plan([s["offset"] for s in segs], lengths, sr)
        assert layout.prev_ends[1] > layout.starts[1] and layout.prev_ends[2] < layout.starts[2]
        copies = []
        real = track.Track.numpy
        track.Track.numpy = lambda self: copies.append(1) or real(self)
        try:
            for bs in (1, 4):
                host = h.run_inference(segs, seed=7, device_noise=True, batch_size=bs)
                mixed = h.run_inference(segs, seed=7, device_noise=True, batch_size=bs, device_mix=True)
                assert mixed.dtype == np.float64 and mixed.shape == (layout.total,)
                np.testing.assert_array_equal(mixed, host)
            assert len(copies) == 2                                 # one device-to-host copy per run
        finally:
            track.Track.numpy = real
        a = h.run_inference(segs, seed=7, device_noise=True, out_path=tmp_path / "host.wav")
        b = h.run_inference(segs, seed=7, device_noise=True, device_mix=True, out_path=tmp_path / "device.wav")
        np.testing.assert_array_equal(a, b)
        assert (tmp_path / "host.wav").read_bytes() == (tmp_path / "device.wav").read_bytes()
        mels = h.run_inference(segs, seed=7, device_noise=True, device_mix=True, save_mel=True)      # the flag is ignored
        assert isinstance(mels, list) and len(mels) == 3 and "mel" in mels[0]
        segs[2]["offset"] = 0.5                                     # the overlap is now longer than the third segment
        with pytest.raises(ValueError, match="dsd_track_plan: segment 2 overlaps the track by"):
            h.run_inference(segs, seed=7, device_noise=True, device_mix=True)
        with pytest.raises(ValueError):                             # the default path: numpy's own error
            h.run_inference(segs, seed=7, device_noise=True)
    finally:
        hparams.clear()
        hparams.update(saved)


# ---- a plain-C caller --------------------------------------------------------------------------------------------------
def test_c_example_equals_the_oracle(tmp_path):
    exe = tmp_path / "c_abi_track"
    libdir = os.path.join(ROOT, "diffsinger_amd")
    cmd = ["gcc", "-std=c99", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "examples", "c_abi_track.c"), "-L" + libdir, "-ldsdenoise", "-L/opt/rocm/lib", "-lamdhip64", "-lm",
           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)]
    subprocess.run(cmd, check=True)
    res = subprocess.run([str(exe), str(tmp_path / "track.s16")], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    # the example's segments: amp * sin(2 pi f i / sr) in double through the C library's sin (math.sin here), rounded to fp32
    sr, two_pi = 44100, 2.0 * 3.14159265358979323846
    spec = [(0.010, 3000, 220.0, 0.5), (0.070, 2500, 330.0, 0.8), (0.150, 1777, 440.0, 0.3)]
    wavs = [np.array([amp * math.sin(two_pi * f * i / sr) for i in range(n)], dtype=np.float64).astype(np.float32)
            for _, n, f, amp in spec]
    want = track_ref.fold([s[0] for s in spec], wavs, sr)
    want_pcm = track_ref.pcm(want, norm=True)
    lines = dict(line.split(None, 1) for line in res.stdout.splitlines())
    assert int(lines["total"]) == want.shape[0] == 8392
    assert float(lines["peak"]) == np.abs(want).max()
    assert int(lines["checksum"]) == int(np.abs(want_pcm.astype(np.int64)).sum())
    got = np.fromfile(tmp_path / "track.s16", dtype=np.int16)
    np.testing.assert_array_equal(got, want_pcm)
