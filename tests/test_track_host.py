"""Host side of the track entries: dsd_track_plan against Python's own round and against G24 (the reference's fold on the
layouts of tests/track_ref.py), every refusal of dsd_track_plan and of the argument checks of dsd_track_place / _peak /
_export (they come before the device is selected, so none of this needs a GPU), and the oracle itself against G24."""
import ctypes as C

import numpy as np
import pytest

import track_ref
from diffsinger_amd import _lib, track

EINVAL = -1


@pytest.fixture(scope="module")
def g24():
    return np.load(track_ref.GOLDEN)


def raw_plan(offsets, lengths, sample_rate, n=None):
    n = len(offsets) if n is None else n
    offs = (C.c_double * max(len(offsets), 1))(*offsets)
    lens = (C.c_int64 * max(len(lengths), 1))(*lengths)
    starts, ends, total = (C.c_int64 * max(n, 1))(), (C.c_int64 * max(n, 1))(), C.c_int64()
    rc = _lib.lib().dsd_track_plan(n, offs, lens, sample_rate, starts, ends, C.byref(total))
    return rc, list(starts[:max(n, 0)]), list(ends[:max(n, 0)]), total.value


def last_error():
    return _lib.lib().dsd_last_error(None).decode()


@pytest.mark.parametrize("sample_rate", [44100, 16000])
def test_plan_rounds_as_python(sample_rate):
    """10 000 seeded offsets, each a one-segment plan's start: nearbyint(offset * sr) is Python's round(offset * sr)."""
    rng = np.random.default_rng(2400 + sample_rate)
    offsets = rng.uniform(0.0, 600.0, 10000)
    offsets[:2000] = np.round(offsets[:2000], 3)                    # what a .ds file holds: a few decimals
    offsets[2000:3000] = (rng.integers(0, 10 ** 6, 1000) + 0.5) / sample_rate       # at or next to a half
    lib = _lib.lib()
    start, end, total = C.c_int64(), C.c_int64(), C.c_int64()
    one = (C.c_int64 * 1)(7)
    for off in offsets.tolist():
        rc = lib.dsd_track_plan(1, (C.c_double * 1)(off), one, sample_rate, C.byref(start), C.byref(end), C.byref(total))
        want = round(off * sample_rate)
        assert (rc, start.value, end.value, total.value) == (0, want, 0, want + 7), off


def test_plan_exact_halves_go_to_even():
    assert track.plan([0.5], [1], 44101).starts == (22050,)          # 22050.5
    assert track.plan([1.5], [1], 3).starts == (4,)                  # 4.5
    assert track.plan([0.5], [1], 3).starts == (2,)                  # 1.5
    assert track.plan([0.5], [1], 1).starts == (0,)                  # 0.5
    assert track.plan([2.5], [1], 1).starts == (2,)
    assert track.plan([3.5], [1], 1).starts == (4,)


def test_plan_of_every_golden_layout(g24):
    assert list(g24["names"]) == [c[0] for c in track_ref.LAYOUTS]
    for name in g24["names"]:
        sr, offsets, lengths = int(g24[f"{name}_sr"]), g24[f"{name}_offsets"].tolist(), g24[f"{name}_lengths"].tolist()
        starts = track_ref.starts_of(offsets, sr)
        ends, total = track_ref.layout_plan(starts, lengths)
        assert total == g24[f"{name}_track"].shape[0], name
        got = track.plan(offsets, lengths, sr)
        assert got == track.Plan(tuple(starts), tuple(ends), total), name


def test_plan_refuses_what_the_reference_raises_on(g24):
    assert list(g24["bad_names"]) == [c[0] for c in track_ref.MALFORMED]
    words = {"negative_first": "segment 0 starts at sample -3, before the track",
             "fade_too_long": "segment 1 overlaps the track by 50 samples but is only 20 long",
             "negative_later": "segment 2 starts at sample -2, before the track"}
    for name, sr, offsets, lengths, seeds in track_ref.MALFORMED:
        assert str(g24[f"{name}_raised"]) == "ValueError", name     # the reference raised
        with pytest.raises(ValueError):                             # ... and so does the restated fold
            track_ref.fold(offsets, track_ref.layout_waves(lengths, seeds), sr)
        rc, *_ = raw_plan(offsets, lengths, sr)
        assert rc == EINVAL and words[name] in last_error(), (name, last_error())
        with pytest.raises(ValueError, match="dsd_track_plan: segment"):
            track.plan(offsets, lengths, sr)


def test_plan_refusals():
    lib = _lib.lib()
    d1, i1, o = (C.c_double * 1)(0.0), (C.c_int64 * 1)(5), (C.c_int64 * 1)()
    good = [1, d1, i1, 44100, o, o, o]
    assert lib.dsd_track_plan(*good) == 0
    for k in (1, 2, 4, 5, 6):                                       # each pointer NULL in turn
        args = list(good)
        args[k] = None
        assert lib.dsd_track_plan(*args) == EINVAL and "dsd_track_plan: null argument" in last_error()
    for n_seg in (0, -1):
        assert raw_plan([0.0], [5], 44100, n=n_seg)[0] == EINVAL and "n_seg must be positive" in last_error()
    for sr in (0, -44100):
        assert raw_plan([0.0], [5], sr)[0] == EINVAL and "sample_rate must be positive" in last_error()
    for bad in (0, -4):                                             # stricter than the reference: no empty segment
        assert raw_plan([0.0, 0.1], [5, bad], 100)[0] == EINVAL and f"segment 1 has length {bad}" in last_error()
    assert raw_plan([float("nan")], [5], 100)[0] == EINVAL and "before the track" in last_error()
    assert raw_plan([-0.006], [5], 100)[0] == EINVAL and "starts at sample -1" in last_error()
    assert raw_plan([-0.004], [5], 100)[0] == 0                     # round(-0.4) is 0: numpy takes it too
    # a track of more than 2^31 - 1 samples: by its last end, by a start, by a length
    top = 2 ** 31 - 1
    assert raw_plan([0.0, float(top - 4)], [5, 4], 1) == (0, [0, top - 4], [0, 5], top)
    for offsets, lengths in (([0.0, float(top - 4)], [5, 5]), ([float(top + 1)], [1]), ([float("inf")], [1]), ([0.0], [top + 1]),
                             ([1e300], [1]), ([0.0], [2 ** 62])):
        assert raw_plan(offsets, lengths, 1)[0] == EINVAL and "past 2^31 - 1 samples" in last_error(), (offsets, lengths)
    # F == n is the longest fade there is; F == n + 1 is refused
    assert raw_plan([0.0, 5.0], [10, 5], 1) == (0, [0, 5], [0, 10], 10)
    assert raw_plan([0.0, 4.0], [10, 5], 1)[0] == EINVAL and "overlaps the track by 6 samples but is only 5 long" in last_error()
    with pytest.raises(ValueError, match="2 offsets but 1 lengths"):
        track.plan([0.0, 1.0], [5], 100)
    with pytest.raises(ValueError, match="n_seg must be positive"):
        track.plan([], [], 100)


def test_place_checks_its_own_geometry():
    """DSD_EINVAL before device selection and before any launch: the pointers are host memory nobody dereferences."""
    lib = _lib.lib()
    host = (C.c_double * 8)()
    t = C.cast(host, C.c_void_p)
    s = C.c_void_p(t.value + 32)
    dev, st = 0, None

    def place(track_p=t, total=100, start=10, prev_end=5, src=s, n=20):
        return lib.dsd_track_place(dev, track_p, total, start, prev_end, src, n, st)

    cases = [(dict(track_p=None), "null argument"), (dict(src=None), "null argument"),
             (dict(total=0), "total 0 outside [1, 2^31 - 1]"), (dict(total=2 ** 31), "outside [1, 2^31 - 1]"),
             (dict(n=0), "n must be positive (0)"), (dict(n=-3), "n must be positive (-3)"),
             (dict(start=-1), "start -1 is before the track"),
             (dict(start=81), "[81, 81 + 20) ends past the track's 100 samples"),
             (dict(start=101, n=1), "ends past the track's 100 samples"),
             (dict(start=2 ** 62, n=2 ** 62), "ends past the track"), (dict(n=2 ** 63 - 1), "ends past the track"),
             (dict(prev_end=-1), "prev_end -1 outside [0, 100]"), (dict(prev_end=101), "prev_end 101 outside [0, 100]"),
             (dict(prev_end=31), "the overlap of 21 samples is longer than the segment's 20"),
             (dict(track_p=C.c_void_p(t.value + 4)), "track must be 8-byte and src 4-byte aligned"),
             (dict(src=C.c_void_p(s.value + 2)), "track must be 8-byte and src 4-byte aligned")]
    for kwargs, words in cases:
        assert place(**kwargs) == EINVAL, kwargs
        assert "dsd_track_place: " in last_error() and words in last_error(), (kwargs, last_error())


def test_peak_and_export_check_their_arguments():
    lib = _lib.lib()
    host = (C.c_double * 8)()
    t = C.cast(host, C.c_void_p)
    o = C.c_void_p(t.value + 32)
    odd = C.c_void_p(t.value + 1)
    for args, words in (((0, None, 10, o, None), "null argument"), ((0, t, 10, None, None), "null argument"),
                        ((0, t, 0, o, None), "total 0 outside"), ((0, t, 2 ** 31, o, None), "total 2147483648 outside [1, 2^31 - 1]"),
                        ((0, odd, 10, o, None), "track is not 8-byte aligned"),
                        ((0, t, 10, C.c_void_p(o.value + 4), None), "peak_out is not 8-byte aligned")):
        assert lib.dsd_track_peak(*args) == EINVAL and "dsd_track_peak: " + words in last_error(), (args, last_error())
    f64, f32, pcm = _lib.DSD_TRACK_F64, _lib.DSD_TRACK_F32, _lib.DSD_TRACK_PCM
    for args, words in (((0, None, 10, pcm, None, o, None), "null argument"), ((0, t, 10, pcm, None, None, None), "null argument"),
                        ((0, t, 10, 3, None, o, None), "unknown kind 3"), ((0, t, 10, -1, None, o, None), "unknown kind -1"),
                        ((0, t, 10, f64, t, o, None), "a peak normalises DSD_TRACK_PCM only"),
                        ((0, t, 10, f32, t, o, None), "a peak normalises DSD_TRACK_PCM only"),
                        ((0, t, 0, pcm, None, o, None), "total 0 outside"), ((0, odd, 10, pcm, None, o, None), "track is not 8-byte"),
                        ((0, t, 10, f64, None, C.c_void_p(o.value + 4), None), "out or peak is not aligned to its element size"),
                        ((0, t, 10, f32, None, C.c_void_p(o.value + 2), None), "out or peak is not aligned to its element size"),
                        ((0, t, 10, pcm, None, odd, None), "out or peak is not aligned to its element size"),
                        ((0, t, 10, pcm, C.c_void_p(t.value + 4), o, None), "out or peak is not aligned to its element size")):
        assert lib.dsd_track_export(*args) == EINVAL and "dsd_track_export: " + words in last_error(), (args, last_error())


def test_oracle_equals_the_reference(g24):
    """track_ref (the fold restated with harness.cross_fade, save_wav restated in numpy) against what the reference's own
    cross_fade and save_wav gave: array_equal, float64 track and both int16 files."""
    for name, sr, offsets, lengths, seeds in track_ref.LAYOUTS:
        assert g24[f"{name}_offsets"].tolist() == list(offsets) and g24[f"{name}_seeds"].tolist() == list(seeds)
        wavs = track_ref.layout_waves(lengths, seeds)
        assert all(w.dtype == np.float32 and np.abs(w).max() < 1 for w in wavs)
        got = track_ref.fold(offsets, wavs, sr)
        want = g24[f"{name}_track"]
        assert got.dtype == np.float64 and want.dtype == np.float64 and np.array_equal(got, want), name
        assert np.array_equal(track_ref.fold_starts(track_ref.starts_of(offsets, sr), wavs), want), name
        assert np.array_equal(track_ref.pcm(got), g24[f"{name}_pcm"]), name
        assert np.array_equal(track_ref.pcm(got, norm=True), g24[f"{name}_pcm_norm"]), name


def test_span_is_the_kernels():
    """track.SPAN (what the GPU tests size their cases by) is kTrackSpan of csrc/dsd_internal.h."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(_lib.HERE), "diffsinger_amd", "csrc", "dsd_internal.h")).read()
    assert int(re.search(r"constexpr int kTrackSpan = (\d+);", src).group(1)) == track.SPAN
