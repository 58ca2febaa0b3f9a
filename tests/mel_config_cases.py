"""The cases of the mel configuration suite: dsd_mel_create / dsd_mel_analyze at the edges of what they accept (odd sizes,
hops longer than the window, windows of 1 .. 3 taps, the largest n_fft and N', 1024 mels, empty filters, fmax above
Nyquist, a band the key shift moves out of the spectrum, another clip).  Shared by the host tests (test_mel_host.py),
the GPU tests (test_gpu_mel_configs.py) and the generator of G26 (golden/make_golden_mel_configs.py), so that all three
build the same seeded waveforms (mel_ref.waveform).  Nothing but seeds and settings is stored here; G26 holds the
reference's own fp32 STFT.get_mel of every row.

Bars.  The floor of a case is |G26 - mel_ref in float64|, computed from the committed fixture; the bar of a case is
2 max(family floor, case floor) with the family floors and the factor 2 of test_gpu_mel.py.  Both terms come from the
reference side."""
import os
from collections import OrderedDict

import numpy as np

import mel_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
G26 = os.path.join(GOLDEN, "g26_mel_configs.npz")
FLOOR_LOG, FLOOR_LIN = 7.6e-5, 2.8e-7       # test_gpu_mel.py: the reference's fp32 against float64 over G17


def _cfg(sr, n_fft, win_size, hop, n_mels, fmin, fmax, clip=1e-5):
    return dict(sr=sr, n_fft=n_fft, win_size=win_size, hop=hop, n_mels=n_mels, fmin=float(fmin), fmax=float(fmax), clip=clip)


def _case(cfg, seed, n, ks, sp, reaches):
    return dict(cfg=cfg, seed=seed, n=n, ks=ks, sp=sp, reaches=reaches)


TINY = _cfg(16000, 64, 64, 16, 8, 0, 8000)
SPEECH = _cfg(16000, 512, 400, 160, 40, 0, 8000)
ODDWIN = _cfg(44100, 1024, 1001, 333, 64, 55, 12000)
HOP_GT_WIN = _cfg(16000, 256, 128, 300, 20, 100, 7000)
HOP_GT_WIN_ODD = _cfg(16000, 256, 129, 300, 20, 100, 7000)
HOP1 = _cfg(16000, 64, 48, 1, 8, 0, 8000)
BIG = _cfg(44100, 16384, 16384, 4096, 32, 20, 2000)
HIGH_FMIN = _cfg(44100, 2048, 2048, 512, 16, 6000, 6400)

# tag: config, waveform seed, samples, key shift, speed, what path of csrc/mel_kernels.hip / mel_run only this row reaches
CASES = OrderedDict(
    tiny=_case(TINY, 2601, 1200, 0, 1, "33 bins in one 64-row tile, two tap chunks, T = 75: one cut frame tile after a full one"),
    speech=_case(SPEECH, 2602, 16000, 0, 1, "W < N with an even off = 56"),
    oddwin_up=_case(ODDWIN, 2603, 30000, 2.3, 1, "N' = 1169, W' = 1143: both odd, off = 13"),
    oddwin_dn=_case(ODDWIN, 2604, 30000, -4.1, 0.9, "N' = 808, W' = 790, H' = 300: the bins past N'/2 are zero-padded"),
    oddfft=_case(_cfg(22050, 1001, 600, 200, 30, 0, 11025), 2605, 15000, 0, 1,
                 "odd n_fft (the top bin is 500 of 1001) and an odd N - W: off = 200 floors"),
    hop_gt_win=_case(HOP_GT_WIN, 2606, 20000, 0, 1, "hop > win: pads -86 / -86, the frame index is shifted into the item"),
    hop_gt_win_odd=_case(HOP_GT_WIN_ODD, 2607, 20000, 0, 1, "pads -86 / -85: the floor division of a negative odd W - H"),
    hop1=_case(HOP1, 2608, 200, 0, 1, "hop 1: pads 23 / 24 (unequal), T = 184"),
    big=_case(BIG, 2609, 80000, 0, 1, "the largest n_fft: 512 tap chunks, pad 6144"),
    big_up=_case(BIG, 2610, 120000, 12, 1, "N' = W' = 32768, the accepted maximum"),
    mels1024=_case(_cfg(44100, 2048, 2048, 512, 1024, 0, 22050), 2611, 12000, 0, 1,
                   "the maximum M: 253 empty filters between live ones"),
    over_nyquist=_case(_cfg(16000, 512, 512, 128, 80, 20, 11025), 2612, 8000, 0, 1,
                       "fmax above Nyquist: 6 empty filters at the top, a cut triangle at bin K - 1"),
    high_fmin=_case(HIGH_FMIN, 2613, 12000, -3, 1, "k_lo = 279 and a narrow band; N' = 1722"),
    high_fmin_gone=_case(HIGH_FMIN, 2614, 12000, -24, 1, "N'/2 = 256 < k_lo: nb == 0, no DFT launch, every value is log(clip)"),
    all_empty=_case(_cfg(16000, 2, 2, 1, 4, 100, 200), 2615, 64, 0, 1, "no filter touches a bin"),
    win3=_case(_cfg(16000, 8, 3, 2, 3, 0, 8000), 2616, 300, 0, 1, "3 taps in one partial chunk (Kpad 32), pads 0 / 1"),
    win2=_case(_cfg(16000, 8, 2, 1, 3, 0, 8000), 2617, 300, 0, 1, "Hann(2) = [0, 1]"),
    win1=_case(_cfg(16000, 4, 1, 1, 2, 0, 8000), 2618, 100, 0, 1, "Hann(1) = [1] (torch.hann_window), not 0.5 - 0.5 cos(0)"),
    clip_hi=_case(dict(SPEECH, clip=1e-2), 2602, 16000, 0, 1, "a clamp that bites on live filters"),
)
TAGS = list(CASES)
DEAD = ("high_fmin_gone", "all_empty")      # peak 0: every value is log(float32(clip))


def configs():
    """the distinct configurations of CASES, by the first tag that uses each"""
    seen, out = [], OrderedDict()
    for tag, c in CASES.items():
        if c["cfg"] not in seen:
            seen.append(c["cfg"])
            out[tag] = c["cfg"]
    return out


def clip_wave(tag):
    c = CASES[tag]
    return mel_ref.waveform(c["seed"], c["n"], c["cfg"]["sr"])


def oracle_linear(tag, y=None):
    """mel_ref in float64 before the clamp and log: [n_mels, T]"""
    c = CASES[tag]
    return mel_ref.get_mel(clip_wave(tag) if y is None else y, c["cfg"], c["ks"], c["sp"], linear=True)


_g26 = None


def g26(tag):
    """the reference's own fp32 STFT.get_mel of the row: [n_mels, T] float32"""
    global _g26
    if _g26 is None:
        z = np.load(G26)
        tags = [str(t) for t in z["tags"]]
        assert tags == TAGS, "g26_mel_configs.npz is not of these cases: rerun golden/make_golden_mel_configs.py"
        for i, t in enumerate(tags):
            c = CASES[t]
            want = np.array([c["seed"], c["n"], c["ks"], c["sp"], c["cfg"]["clip"]], dtype=np.float64)
            assert np.array_equal(z[f"c{i}_meta"], want), t
        _g26 = {t: z[f"c{i}_mel"] for i, t in enumerate(tags)}
    return _g26[tag]


def errors_of(got, lin, clip):
    """test_gpu_mel.errors on given arrays: (log-mel max error, linear error / the item's peak) of a log-mel `got` against the
    float64 linear mel `lin`; the linear figure is None where the peak is 0."""
    got = np.asarray(got, dtype=np.float64)
    floor = np.maximum(lin, clip)
    peak = lin.max()
    e_lin = float(np.abs(np.exp(got) - floor).max() / peak) if peak > 0 else None
    return float(np.abs(got - np.log(floor)).max()), e_lin


_floors = {}


def floors(tag):
    """(log, linear) of G26 against mel_ref in float64: the reference's own fp32 error on this row"""
    if tag not in _floors:
        _floors[tag] = errors_of(g26(tag), oracle_linear(tag), CASES[tag]["cfg"]["clip"])
    return _floors[tag]


def bars(tag):
    f_log, f_lin = floors(tag)
    return 2 * max(FLOOR_LOG, f_log), 2 * max(FLOOR_LIN, f_lin or 0.0)


def live_filters(tag):
    """rows of the filterbank with a non-zero weight on a bin this row's N' computes"""
    c = CASES[tag]
    cfg = c["cfg"]
    fb = mel_ref.filterbank(cfg["sr"], cfg["n_fft"], cfg["n_mels"], cfg["fmin"], cfg["fmax"])
    n = mel_ref.geometry(cfg["n_fft"], cfg["win_size"], cfg["hop"], c["ks"], c["sp"])[0]
    return (fb[:, : n // 2 + 1] != 0).any(axis=1)
