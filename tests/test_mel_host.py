"""CPU checks of the mel analysis boundary (no device): the library's filterbank against librosa's definition (restated in
tests/mel_ref.py and, independently, transformers' Slaney bank), the Slaney scale's known answers, the frame count and
its rounding rules against the formula and G17's shapes, and the rejections - at the production configurations and at
every configuration of mel_config_cases.py; G26's shapes; and the float64 oracle alone against G26 (the floors that the
GPU suite's bars are made of)."""
import ctypes as C
import os
import sys
import warnings

import numpy as np
import pytest

import mel_config_cases as mc
import mel_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CONFIGS = [mel_ref.PROD, mel_ref.SMALL] + list(mc.configs().values())
IDS = ["prod", "small"] + list(mc.configs())


def cfg_of(c, **over):
    from diffsinger_amd import _lib
    d = dict(sr=c["sr"], n_fft=c["n_fft"], win_size=c["win_size"], hop=c["hop"], n_mels=c["n_mels"], fmin=c["fmin"],
             fmax=c["fmax"], clip=c.get("clip", 1e-5), device=0)
    d.update(over)
    return _lib.DsdMelConfig(C.sizeof(_lib.DsdMelConfig), d["sr"], d["n_fft"], d["win_size"], d["hop"], d["n_mels"],
                             d["fmin"], d["fmax"], d["clip"], d["device"])


def frames(cfg, n, ks=0.0, sp=1.0):
    from diffsinger_amd import _lib
    return _lib.lib().dsd_mel_num_frames(C.byref(cfg), n, ks, sp)


@pytest.mark.parametrize("c", CONFIGS, ids=IDS)
def test_filterbank_matches_librosa_definition(c):
    from diffsinger_amd.mel import mel_filterbank
    fb = mel_filterbank(c["sr"], c["n_fft"], c["n_mels"], c["fmin"], c["fmax"])
    assert fb.shape == (c["n_mels"], c["n_fft"] // 2 + 1) and fb.dtype == np.float32
    want = mel_ref.filterbank(c["sr"], c["n_fft"], c["n_mels"], c["fmin"], c["fmax"])
    assert np.array_equal(fb, want)          # the same float64 steps, the same float32 roundings
    # every filter is one contiguous run of non-zero bins (what the projection kernel relies on)
    for row in fb:
        nz = np.nonzero(row)[0]
        assert len(nz) == 0 or nz[-1] - nz[0] + 1 == len(nz)


@pytest.mark.parametrize("c", CONFIGS, ids=IDS)
def test_filterbank_matches_transformers_slaney(c):
    audio_utils = pytest.importorskip("transformers.audio_utils")
    from diffsinger_amd.mel import mel_filterbank
    fb = mel_filterbank(c["sr"], c["n_fft"], c["n_mels"], c["fmin"], c["fmax"])
    if c["n_fft"] % 2:
        # mel_filter_bank centres the bins at linspace(0, sr // 2, bins): librosa's k sr / n_fft only at an even n_fft.  Its
        # scale, triangles and norm on librosa's centres (what G26's generator hands the reference at an odd n_fft)
        if GOLDEN not in sys.path:
            sys.path.insert(0, GOLDEN)
        from make_golden_mel_configs import _mel_odd
        want = _mel_odd(c["sr"], c["n_fft"], c["n_mels"], c["fmin"], c["fmax"])
    else:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                  # "at least one mel filter has all zero values"
            want = audio_utils.mel_filter_bank(num_frequency_bins=c["n_fft"] // 2 + 1, num_mel_filters=c["n_mels"],
                                               min_frequency=c["fmin"], max_frequency=c["fmax"], sampling_rate=c["sr"],
                                               norm="slaney", mel_scale="slaney").T
    assert np.abs(fb - want).max() <= 1e-6 * np.abs(want).max()


def test_slaney_scale_known_answers():
    # 1000 Hz = 15 mel; linear at 200/3 Hz per mel below: a filterbank whose 3 points are 0, 15, 30 mel has its peak at
    # the bin nearest 1000 Hz and its lower edge at 0 Hz
    assert mel_ref._hz_to_mel(1000.0) == pytest.approx(15.0, abs=1e-12)
    assert mel_ref._hz_to_mel(200.0 / 3) == pytest.approx(1.0, abs=1e-12)
    assert mel_ref._mel_to_hz(7.5) == pytest.approx(500.0, abs=1e-9)
    from diffsinger_amd.mel import mel_filterbank
    sr, n_fft = 16000, 1600                                    # 10 Hz bins
    fb = mel_filterbank(sr, n_fft, 1, 0.0, 1000.0)             # mel points 0, 7.5, 15 -> 0, 500, 1000 Hz
    assert np.argmax(fb[0]) == 50 and fb[0, 0] == 0.0 and fb[0, 100] == 0.0
    assert fb[0, 50] == pytest.approx(2.0 / 1000.0, rel=1e-6)           # Slaney area norm 2 / (f2 - f0) at the apex
    assert fb[0, 25] == pytest.approx(1.0 / 1000.0, rel=1e-6)           # linear ramp (Hz and mel are linear here)


@pytest.mark.parametrize("c", CONFIGS, ids=IDS)
@pytest.mark.parametrize("ks,sp", [(0, 1), (3, 1), (-5.5, 1), (12, 1), (0, 1.25), (2, 0.8), (0.1, 1), (-3.7, 1.1), (0, 4.5),
                                   (7.3, 0.3)])
def test_num_frames_formula(c, ks, sp):
    cfg = cfg_of(c)
    n_, w_, h_, pl, pr = mel_ref.geometry(c["n_fft"], c["win_size"], c["hop"], ks, sp)
    valid = 1 <= w_ <= n_ <= 32768 and h_ >= 1               # what mel_geometry accepts; outside it every length is refused
    # around the reflect limit (pad < L), around the first length that fills one frame (with negative pads too: L + padL +
    # padR >= N'), and one hop further
    edge = [max(pl, pr) + d for d in (-1, 0, 1, 2)] + [n_ - pl - pr + d for d in (-1, 0, 1, h_ - 1, h_, h_ + 1)]
    for n in [1, 100, 700, 769, 800, 1024, 2047, 2048, 4100, 44100, 13_230_000] + [v for v in edge if v >= 1]:
        want = mel_ref.num_frames(n, c["n_fft"], c["win_size"], c["hop"], ks, sp) if valid else None
        got = frames(cfg, n, ks, sp)
        assert got == (want if want is not None else -1), (n, got, want)


def test_num_frames_rounding_ties_to_even():
    cfg = cfg_of(mel_ref.PROD)
    # 512 * speed = 512.5 -> 512 (ties to even), 513.5 -> 514; int(np.round()) agrees
    assert int(np.round(512 * (512.5 / 512))) == 512
    n = 44100
    assert frames(cfg, n, 0.0, 512.5 / 512) == frames(cfg, n, 0.0, 1.0)
    assert frames(cfg, n, 0.0, 513.5 / 512) == 1 + (n + (2048 - 514) // 2 + (2048 - 514 + 1) // 2 - 2048) // 514
    # a keyshift whose float32 value would round N' differently: the ABI carries doubles
    ks = 12 * np.log2(2048.5 / 2048)                         # N' = round(2048.5...) in double
    assert frames(cfg, n, ks, 1.0) == mel_ref.num_frames(n, 2048, 2048, 512, ks, 1.0)


def test_num_frames_matches_g17_shapes():
    z = np.load(os.path.join(GOLDEN, "g17_mel.npz"))
    for i in range(int(z["n_cases"])):
        seed, n, ks, sp, small = z[f"c{i}_meta"]
        c = mel_ref.SMALL if small else mel_ref.PROD
        assert z[f"c{i}_mel"].shape == (c["n_mels"], frames(cfg_of(c), int(n), float(ks), float(sp)))


def test_num_frames_matches_g26_shapes():
    for tag, k in mc.CASES.items():
        c = k["cfg"]
        assert mc.g26(tag).shape == (c["n_mels"], frames(cfg_of(c), k["n"], float(k["ks"]), float(k["sp"]))), tag
        assert mc.g26(tag).dtype == np.float32


@pytest.mark.parametrize("tag", mc.TAGS)
def test_oracle_against_g26(tag):
    """mel_ref alone against the reference's own fp32 output: the floor of every row is finite and small, so a broken
    oracle (or a fixture of other cases) cannot pass the GPU suite silently.  Hann(1) = [1]: at win1 the old window 0 gave
    log(clip) everywhere, 2.9 off in log-mel."""
    k = mc.CASES[tag]
    c = k["cfg"]
    want = mc.g26(tag)
    got = mel_ref.get_mel(mc.clip_wave(tag), c, k["ks"], k["sp"], clip=c["clip"])
    assert got.shape == want.shape and np.isfinite(got).all() and np.isfinite(want).all()
    f_log, f_lin = mc.floors(tag)
    assert np.isfinite(f_log) and f_log < 1e-3, f_log
    assert float(np.abs(got - want).max()) == pytest.approx(f_log, abs=1e-12)
    if tag in mc.DEAD:
        assert f_lin is None and np.all(got == np.log(c["clip"]))
        assert np.abs(want - np.log(np.float32(c["clip"]))).max() <= 1e-6
    else:
        assert np.isfinite(f_lin) and f_lin < 1e-6, f_lin
        assert (got > np.log(c["clip"])).any()                # a live row is not all clamp
    if tag == "win1":
        # log-mel inside the family floor (5.2e-7).  Linear: 3.8e-7 of a peak of 1.8e-4, which is the float32 rounding of a
        # stored log-mel near -8.6 (half an ulp there is 4.8e-7 relative) and not the transform: inside the family's bar
        assert f_log <= mc.FLOOR_LOG and f_lin <= 2 * mc.FLOOR_LIN, (f_log, f_lin)
    if tag == "clip_hi":
        assert (got == np.log(c["clip"])).mean() > 0.05      # the clamp bites
    # the geometry the row's sentence promises
    assert mel_ref.num_frames(k["n"], c["n_fft"], c["win_size"], c["hop"], k["ks"], k["sp"]) == want.shape[1]


def test_case_geometries():
    """the sizes the table of cases names"""
    g = lambda tag: mel_ref.geometry(*(mc.CASES[tag]["cfg"][k] for k in ("n_fft", "win_size", "hop")), mc.CASES[tag]["ks"],
                                     mc.CASES[tag]["sp"])
    assert g("oddwin_up")[:2] == (1169, 1143) and g("oddwin_dn")[:3] == (808, 790, 300)
    assert g("hop_gt_win")[3:] == (-86, -86) and g("hop_gt_win_odd")[3:] == (-86, -85) and g("hop1")[3:] == (23, 24)
    assert g("big_up")[:2] == (32768, 32768) and g("big")[3] == 6144 and g("high_fmin")[0] == 1722
    assert g("high_fmin_gone")[0] // 2 == 256 and g("win3")[3:] == (0, 1)
    assert int((~mc.live_filters("mels1024")).sum()) == 253 and int((~mc.live_filters("over_nyquist")).sum()) == 6
    assert not mc.live_filters("all_empty").any() and not mc.live_filters("high_fmin_gone").any()


def test_too_short_and_bad_configs_rejected():
    from diffsinger_amd import _lib
    lib = _lib.lib()
    cfg = cfg_of(mel_ref.PROD)
    assert frames(cfg, 768) == -1          # reflect pad 768 >= L: torch raises
    assert frames(cfg, 769) == 1
    assert b"too short" in lib.dsd_last_error(None)
    assert frames(cfg, 44100, 0.0, 0.0) == -1 and frames(cfg, 44100, float("nan"), 1.0) == -1
    assert frames(cfg, 44100, 200.0, 1.0) == -1            # N' beyond the supported 32768
    h = C.c_void_p()
    out = np.zeros((128, 1025), np.float32)
    for over in (dict(win_size=4096), dict(n_fft=1), dict(hop=0), dict(n_mels=0), dict(fmin=16000.0), dict(fmin=-1.0),
                 dict(clip=0.0), dict(sr=0)):
        bad = cfg_of(mel_ref.PROD, **over)
        assert lib.dsd_mel_create(C.byref(bad), C.byref(h)) == -1, over
        assert lib.dsd_mel_filterbank(C.byref(bad), out.ctypes.data_as(C.POINTER(C.c_float))) == -1, over
        assert frames(bad, 44100) == -1, over
    bad = cfg_of(mel_ref.PROD)
    bad.struct_size = 8
    assert lib.dsd_mel_create(C.byref(bad), C.byref(h)) == -1
    assert b"struct_size" in lib.dsd_last_error(None)


def test_struct_size_and_handle_kinds():
    from diffsinger_amd import _lib
    assert C.sizeof(_lib.DsdMelConfig) == 56
    assert _lib.DsdMelConfig.fmin.offset == 24 and _lib.DsdMelConfig.device.offset == 48
    cfg = _lib.DsdConfig(C.sizeof(_lib.DsdConfig), 6, 128, 1, 20, 256, 256, 4, 0, 0, 0, 0, 0)     # DSD_MEL_ANALYSIS
    h = C.c_void_p()
    assert _lib.lib().dsd_create(C.byref(cfg), C.byref(h)) == -1
    assert b"unknown backbone" in _lib.lib().dsd_last_error(None)
    # the mel entry points on a NULL handle
    assert _lib.lib().dsd_mel_analyze(None, None, 1, 1, 1, None, 0.0, 1.0, None, 1, 1, 1, None) == -1


def test_cpu_tensor_and_center_rejected():
    import torch
    from diffsinger_amd.mel import STFT
    s = STFT(44100, 128, 2048, 2048, 512, 40, 16000)
    with pytest.raises(NotImplementedError):
        s.get_mel(torch.zeros(1, 4096), center=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        s.get_mel(torch.zeros(1, 4096))
    with pytest.raises(ValueError):
        s.num_frames(100)
    assert s.num_frames(44100) == 1 + (44100 + 768 + 768 - 2048) // 512
