"""Oracle of the track entries (dsd_track_plan / _place / _peak / _export): the reference's fold over the segments
(inference/ds_acoustic.py:231-259) restated with `harness.cross_fade` - which G11 pins bit for bit to the reference's
`cross_fade` - and `save_wav`'s arithmetic (utils/infer_utils.py:99-104) restated in numpy.  Everything float64, on the host.

tests/golden/g24_track.npz holds what the reference's own functions gave on LAYOUTS and MALFORMED
(tests/golden/make_golden_track.py); the waveforms are recomputed from their seeds by `waveform`, whose arithmetic is exact
(integers and one power-of-two scale), so every platform gets the same bits.
"""
import os

import numpy as np

from diffsinger_amd.harness import cross_fade

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g24_track.npz")


def waveform(seed, n):
    """n fp32 samples in [-1, 1): a 64-bit integer hash of (seed, index), its top 24 bits scaled by 2^-23."""
    with np.errstate(over="ignore"):
        h = (np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
             + np.uint64(seed) * np.uint64(0xBF58476D1CE4E5B9))
        h ^= h >> np.uint64(31)
        h *= np.uint64(0x94D049BB133111EB)
        h ^= h >> np.uint64(29)
    return ((h >> np.uint64(40)).astype(np.float64) * 2.0 ** -23 - 1.0).astype(np.float32)


def starts_of(offsets, sample_rate):
    return [round(o * sample_rate) for o in offsets]


def fold(offsets, wavs, sample_rate):
    """The loop of ds_acoustic.py:231-259 (as harness.run_inference has it): -> the float64 track.  Raises numpy's
    ValueError on the layouts the reference raises on."""
    track, cursor = np.zeros(0), 0
    for off, wav in zip(offsets, wavs):
        gap = round(off * sample_rate) - cursor
        if gap >= 0:
            track = np.concatenate((track, np.zeros(gap), wav))
        else:
            track = cross_fade(track, wav, cursor + gap)
        cursor += gap + wav.shape[0]
    return track


def fold_starts(starts, wavs):
    """`fold` on sample positions (sample rate 1: round(int) is the int)."""
    return fold(starts, wavs, 1)


def layout_plan(starts, lengths):
    """(prev_ends, total) of a well-formed layout."""
    ends, end = [], 0
    for s, n in zip(starts, lengths):
        ends.append(end)
        end = s + n
    return ends, end


def pcm(track, norm=False):
    """save_wav's int16: (track / max|track| if norm else track) * 32767, truncated toward zero - and the library's two
    documented deviations where numpy's own result is undefined: outside int16 the value saturates, a zero peak gives zeros."""
    track = np.asarray(track, dtype=np.float64)
    if norm:
        peak = np.abs(track).max()
        if peak == 0:
            return np.zeros(track.shape, np.int16)
        scaled = (track / peak) * 32767
    else:
        scaled = track * 32767
    return np.clip(np.trunc(scaled), -32768, 32767).astype(np.int16)


def _at(sample_rate, starts):
    return [s / sample_rate for s in starts]


# (name, sample_rate, offsets in seconds, lengths, seeds).  round(offset * sample_rate) is the start the comment names.
LAYOUTS = [
    # an overlap of 47, then a gap of 229
    ("overlap_gap", 44100, _at(44100, [0, 353, 882]), [400, 300, 350], [2401, 2402, 2403]),
    # leading silence (odd start), gap 0, gap 1
    ("silence_first", 44100, _at(44100, [127, 427, 528]), [300, 100, 77], [2404, 2405, 2406]),
    # the third segment starts inside the fade [300, 400) of the first two
    ("inside_fade", 44100, _at(44100, [0, 300, 350]), [400, 200, 300], [2407, 2408, 2409]),
    # the third segment starts before its predecessor's start
    ("before_predecessor", 44100, _at(44100, [0, 250, 200]), [300, 60, 200], [2410, 2411, 2412]),
    # F = 1, then F = 2
    ("fade_one_two", 44100, _at(44100, [0, 199, 247]), [200, 50, 30], [2413, 2414, 2415]),
    # F = n: the new segment is all fade; then gap 0
    ("fade_whole", 44100, _at(44100, [3, 253, 303]), [300, 50, 41], [2416, 2417, 2418]),
    # offsets that land on exact halves at 16 kHz (2.5 -> 2, 3.5 -> 4 after a gap) and a single-sample segment
    ("halves", 16000, [2.5 / 16000, 0.0125 + 3.5 / 16000, 0.02], [150, 100, 1], [2419, 2420, 2421]),
    # one segment alone
    ("single", 16000, [0.001], [333], [2422]),
]
# layouts on which the reference raises: a first start below 0; an overlap longer than the new segment; a later start below 0
MALFORMED = [
    ("negative_first", 44100, [-3 / 44100], [10], [2431]),
    ("fade_too_long", 44100, _at(44100, [0, 50]), [100, 20], [2432, 2433]),
    ("negative_later", 44100, [0.0, 40 / 44100, -2 / 44100], [50, 30, 200], [2434, 2435, 2436]),
]


def layout_waves(lengths, seeds):
    return [waveform(s, n) for s, n in zip(seeds, lengths)]
