"""-m gpu: VR harmonic-noise separation and the variance curves (dsd_hnsep_*, dsd_base_harmonic, dsd_variance_curves,
diffsinger_amd.hnsep) against the reference's fp32 separator (G19) and the float64 restatement in tests/hnsep_ref.py.

Tolerances are stated from measurement.  Each G19 case records the reference's own fp32 CPU error against the float64
oracle (FLOOR: harmonic part and mask separately; tests/golden/make_golden_hnsep.py prints them: harmonic 1.1e-7 ..
8.1e-7, mask 1.0e-6 .. 1.1e-5).  The HIP result must stay within 2 FLOOR of the float64 oracle and within FLOOR + 2 FLOOR
of G19.  The curves have no reference fp32 run (librosa is not installed); their bound is stated against the float64
restatement: 1e-4 dB on energy / breathiness / voicing, 1e-5 on tension's ratio, the logit domain checked through the
ratio (its slope near the clip ends is 1e4).  Ragged items must be bit-identical to their lone calls."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hnsep_ref  # noqa: E402
import mel_ref  # noqa: E402
from diffsinger_amd import _lib, hnsep, synth  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SR = 44100
CURVE_DB_BAR = 1e-4
TENSION_BAR = 1e-5


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"


@pytest.fixture(scope="module")
def g19():
    return np.load(os.path.join(GOLDEN, "g19_hnsep.npz"))


def _gen():
    sys.path.insert(0, GOLDEN)
    import make_golden_hnsep
    return make_golden_hnsep


_SEP = {}


def sep_of(cfg_name, seed):
    key = (cfg_name, seed)
    if key not in _SEP:
        cfg = _gen().CONFIGS[cfg_name]
        sd = synth.hnsep_state_dict(cfg, seed)
        _SEP[key] = (hnsep.HnSep(sd, cfg), sd, cfg)
    return _SEP[key]


def case(g19, i):
    wseed, yseed, n, ci = (int(v) for v in g19[f"c{i}_meta"])
    name = list(_gen().CONFIGS)[ci]
    return name, wseed, mel_ref.waveform(yseed, n, SR).astype(np.float32)


N_SMALL_CASES = 6


@pytest.mark.parametrize("i", range(N_SMALL_CASES))
def test_g19_case(g19, i):
    """harmonic part (and the mask where stored) against G19 and the float64 oracle."""
    name, wseed, x = case(g19, i)
    sp, sd, cfg = sep_of(name, wseed)
    fl_h, fl_m, mid = (float(v) for v in g19[f"c{i}_floor"])
    got = sp.separate_ragged([x])[0].cpu().numpy()
    want, mk64 = hnsep_ref.separate(hnsep_ref.model64(sd, cfg), x, cfg)
    assert np.abs(got - want).max() <= 2 * fl_h, (np.abs(got - want).max(), fl_h)
    assert np.abs(got - g19[f"c{i}_harmonic"]).max() <= 3 * fl_h
    c = 1 if cfg["is_mono"] else 2
    spec, _ = hnsep_ref.spec_of(x, cfg)
    spec = np.stack([spec] * c)[None].astype(np.complex64)
    gm = sp.mask(torch.from_numpy(spec)).cpu().numpy()[0]
    assert gm.shape == mk64.shape
    assert np.abs(gm - mk64).max() <= 2 * fl_m, (np.abs(gm - mk64).max(), fl_m)
    if f"c{i}_mask" in g19:
        assert np.abs(gm - g19[f"c{i}_mask"]).max() <= 3 * fl_m
    assert mid > 0.1            # the fixture's masks are not saturated


def test_production_clip(g19):
    """the production layout (n_fft 2048, hop 512, nout 32, nout_lstm 128) on G19's 1.5-s clip."""
    i = 6
    name, wseed, x = case(g19, i)
    sp, sd, cfg = sep_of(name, wseed)
    fl_h = float(g19[f"c{i}_floor"][0])
    got = sp.separate_ragged([x])[0].cpu().numpy()
    assert np.abs(got - g19[f"c{i}_harmonic"]).max() <= 3 * fl_h
    want, _ = hnsep_ref.separate(hnsep_ref.model64(sd, cfg), x, cfg)
    assert np.abs(got - want).max() <= 2 * fl_h


def test_production_10s():
    """a 10-s clip of the production layout against the float64 torch mirror; its floor is the reference's own fp32
    error on the same clip (the mirror in fp32 on the CPU: measured 1.1e-6)."""
    cfg = dict(synth.HNSEP_PROD)
    sp, sd, _ = sep_of("prod", 1902)
    x = mel_ref.waveform(1990, 10 * SR, SR).astype(np.float32)
    got = sp.separate_ragged([x])[0].cpu().numpy()
    m32 = hnsep_ref.model64(sd, cfg).float()
    with torch.no_grad():
        h32 = m32.predict_from_audio(torch.from_numpy(x)[None, None])[0, 0].numpy()
        h64 = hnsep_ref.model64(sd, cfg).predict_from_audio(torch.from_numpy(x.astype(np.float64))[None, None])[0, 0].numpy()
    floor = float(np.abs(h32 - h64).max())
    assert np.abs(got - h64).max() <= 2 * floor, (np.abs(got - h64).max(), floor)


def test_stereo_averages_channels(g19):
    """a stereo model sees the clip on both channels; the output is the mean of its two channel outputs."""
    i = 4
    name, wseed, x = case(g19, i)
    sp, sd, cfg = sep_of(name, wseed)
    spec, pl = hnsep_ref.spec_of(x, cfg)
    m = sp.mask(torch.from_numpy(np.stack([spec] * 2)[None].astype(np.complex64))).cpu().numpy()[0]
    ys = [hnsep_ref.istft(spec * m[c], cfg["n_fft"], cfg["hop_length"], hnsep_ref.hann(cfg["n_fft"]))[pl:pl + len(x)]
          for c in range(2)]
    assert np.abs(ys[0] - ys[1]).max() > 1e-3          # the two channels' masks differ
    got = sp.separate_ragged([x])[0].cpu().numpy()
    assert np.abs(got - 0.5 * (ys[0] + ys[1])).max() <= 3 * float(g19[f"c{i}_floor"][0]) + 1e-6


def test_base_harmonic(g19):
    """_kth_harmonic(0) of G19's harmonic part against the reference's fp32 result and the float64 oracle."""
    gen = _gen()
    h = g19[f"c{gen.BASE_CASE}_harmonic"]
    f0 = g19["base_f0"]
    sp, _, _ = sep_of("small", 1900)
    got = sp.base_harmonic_ragged([h], [f0], SR, gen.BASE_HOP, gen.BASE_WIN)[0].cpu().numpy()
    want = hnsep_ref.base_harmonic(h, f0, SR, gen.BASE_HOP, gen.BASE_WIN)
    fl = float(g19["base_floor"][0])
    assert np.abs(got - want).max() <= 2 * fl, (np.abs(got - want).max(), fl)
    assert np.abs(got - g19["base_harmonic"]).max() <= 3 * fl
    # frames at the center >= 1 edge (86.0 Hz: masked out, 86.3 Hz: kept) shape the result
    assert np.abs(got).max() > 0.01


def test_base_harmonic_win96_ragged():
    """win_size 96, hop 24: the window is no multiple of the 64-row tile, so the inverse DFT's second row tile is partly
    past the frame (rows 96..127 are not written), and 2 (win / 2 + 1) = 98 leaves the forward one partly empty too.  Two
    clips of 0.2 s and 0.35 s (368 and 644 frames: 6 and 11 frame tiles, the last ones partial) in one ragged call are
    bit-identical to their lone calls and within twice the float32 restatement's own error of the float64 oracle."""
    sp, _, _ = sep_of("small", 1900)
    hop, win = 24, 96
    lens = [int(0.2 * SR), int(0.35 * SR)]
    hs = [mel_ref.waveform(1985 + i, n, SR).astype(np.float32) for i, n in enumerate(lens)]
    # center = f0 win / sr from 2.8 to 4.1 bins (the band's edges cross bins), an unvoiced gap, f0 shorter than the frames
    f0s = [1600.0 + 300.0 * np.sin(np.arange(n // hop + 1 - 5) / 9.0 + i) for i, n in enumerate(lens)]
    for f0 in f0s:
        f0[40:60] = 0.0
    rag = sp.base_harmonic_ragged(hs, f0s, SR, hop, win)
    for h, f0, r in zip(hs, f0s, rag):
        assert torch.equal(r, sp.base_harmonic_ragged([h], [f0], SR, hop, win)[0])
        want = hnsep_ref.base_harmonic(h, f0, SR, hop, win)
        floor = float(np.abs(hnsep_ref.base_harmonic(h, f0, SR, hop, win, dtype=np.float32) - want).max())
        err = float(np.abs(r.cpu().numpy() - want).max())
        print(f"base harmonic win 96, {len(h)} samples: error {err:.3g}, float32 restatement {floor:.3g}, peak {np.abs(want).max():.3g}")
        assert np.abs(want).max() > 0.01 and floor > 0
        assert err <= 2 * floor, (err, floor)


def test_curves():
    """energy, breathiness, voicing (dB) and tension in every domain against the float64 restatement, with `length`
    both past the RMS frames (zero pad, then the top-db clamp) and short of them (crop)."""
    sp, _, _ = sep_of("small", 1900)
    hop, win = 512, 2048
    x = mel_ref.waveform(1960, 30000, SR).astype(np.float32)
    h = sp.separate_ragged([x])[0].cpu().numpy()
    f0 = np.full(30000 // hop + 1, 220.0)
    f0[10:20] = 0.0
    b = sp.base_harmonic_ragged([h], [f0], SR, hop, win)[0].cpu().numpy()
    for length in (30000 // hop + 9, 40):
        cv = {k: v[0] for k, v in sp.curves_ragged([x], [h], [b], [length], hop, win, domain="ratio").items()}
        ref = dict(energy=hnsep_ref.energy(x, length, hop, win), breathiness=hnsep_ref.energy(x - h, length, hop, win),
                   voicing=hnsep_ref.energy(h, length, hop, win))
        for k, v in ref.items():
            assert cv[k].shape == (length,)
            assert np.abs(cv[k] - v).max() <= CURVE_DB_BAR, (k, np.abs(cv[k] - v).max())
        assert np.abs(cv["tension"] - hnsep_ref.tension(h, b, length, hop, win, "ratio")).max() <= TENSION_BAR
        if length > 30000 // hop + 1:
            assert cv["energy"][-1] == pytest.approx(cv["energy"].max() - 80.0, abs=1e-3)   # padded frames at the clamp
        lg = sp.curves_ragged(None, [h], [b], [length], hop, win, domain="logit", which=("tension",))["tension"][0]
        r = np.clip(hnsep_ref.tension(h, b, length, hop, win, "ratio"), 1e-4, 1 - 1e-4)
        assert np.abs(1 / (1 + np.exp(-lg.astype(np.float64))) - r).max() <= TENSION_BAR
        db = sp.curves_ragged(None, [h], [b], [length], hop, win, domain="db", which=("tension",))["tension"][0]
        assert np.abs(db - hnsep_ref.tension(h, b, length, hop, win, "db")).max() <= 1e-2
    amp = hnsep.get_energy_librosa(x, 50, hop_size=hop, win_size=win, domain="amplitude", model=sp)
    assert np.abs(amp - hnsep_ref.energy(x, 50, hop, win, "amplitude")).max() <= 1e-6


def test_ragged_bit_identical():
    """clips of mixed lengths in one call: each item bit-identical to its lone call (separation, base harmonic, curves)."""
    sp, _, _ = sep_of("small", 1900)
    lens = [16000, 300, 5127, 9000]          # 300 samples: one 32-frame block; all past win_size / 2 = 256
    xs = [mel_ref.waveform(1970 + i, n, SR).astype(np.float32) for i, n in enumerate(lens)]
    rag = sp.separate_ragged(xs)
    for x, r in zip(xs, rag):
        assert torch.equal(r, sp.separate_ragged([x])[0])
    hop, win = 128, 512
    f0s = [np.full(n // hop + 1, 150.0 + 10 * i) for i, n in enumerate(lens)]
    bag = sp.base_harmonic_ragged(rag, f0s, SR, hop, win)
    for h, f0, r in zip(rag, f0s, bag):
        assert torch.equal(r, sp.base_harmonic_ragged([h], [f0], SR, hop, win)[0])
    frames = [n // hop + 1 for n in lens]
    cr = sp.curves_ragged(xs, rag, bag, frames, hop, win)
    for i in range(len(xs)):
        lone = sp.curves_ragged([xs[i]], [rag[i]], [bag[i]], [frames[i]], hop, win)
        for k in lone:
            assert np.array_equal(cr[k][i], lone[k][0]), k


def test_decomposed_waveform_caches_and_world():
    sp, _, _ = sep_of("small", 1900)
    x = mel_ref.waveform(1980, 6000, SR).astype(np.float32)
    f0 = np.full(6000 // 128 + 1, 200.0)
    d = hnsep.DecomposedWaveform(x, SR, f0, hop_size=128, fft_size=512, win_size=512, algorithm="vr", model=sp)
    h = d.harmonic()
    assert d.harmonic() is h and d.harmonic(0) is d.harmonic(0)
    assert np.array_equal(d.aperiodic(), x - h)
    with pytest.raises(NotImplementedError, match="WORLD|world"):
        hnsep.DecomposedWaveform(x, SR, f0, hop_size=128, win_size=512, algorithm="world", model=sp)


def test_error_paths():
    lib = _lib.lib()
    hp = C.c_void_p()
    bad = _lib.DsdHnsepConfig(C.sizeof(_lib.DsdHnsepConfig), 500, 128, 8, 16, 1, 0)        # n_fft not a multiple of 64
    assert lib.dsd_hnsep_create(C.byref(bad), C.byref(hp)) != 0
    bad = _lib.DsdHnsepConfig(C.sizeof(_lib.DsdHnsepConfig) - 4, 512, 128, 8, 16, 1, 0)    # struct_size
    assert lib.dsd_hnsep_create(C.byref(bad), C.byref(hp)) != 0
    ok = _lib.DsdHnsepConfig(C.sizeof(_lib.DsdHnsepConfig), 512, 128, 8, 16, 1, 0)
    assert lib.dsd_hnsep_create(C.byref(ok), C.byref(hp)) == 0
    try:
        x = torch.zeros(1, 1000, device="cuda")
        # weights not finalized
        assert lib.dsd_hnsep_separate(hp, C.c_void_p(x.data_ptr()), 1, 1000, 1000, 0, None, C.c_void_p(x.data_ptr()), 1000, 0,
                                      None) != 0
        assert b"finalized" in lib.dsd_last_error(hp)
        # weights missing: finalizing without loading any
        assert lib.dsd_finalize_weights(hp) != 0
        assert b"missing keys" in lib.dsd_last_error(hp)
        # wrong handle kind: a separator handle on another family's entry point, and the reverse
        assert lib.dsd_set_lengths(hp, None, 1, None) != 0
        assert b"dsd_set_lengths: this handle is a harmonic-noise separator" in lib.dsd_last_error(hp)
        mc = _lib.DsdMelConfig(C.sizeof(_lib.DsdMelConfig), 44100, 2048, 2048, 512, 128, 40.0, 16000.0, 1e-5, 0)
        mh = C.c_void_p()
        assert lib.dsd_mel_create(C.byref(mc), C.byref(mh)) == 0
        try:
            rc = lib.dsd_variance_curves(mh, C.c_void_p(x.data_ptr()), None, None, 1, 1000, (C.c_int64 * 1)(1000), 128, 512,
                                         (C.c_int64 * 1)(8), 2, 1, C.c_void_p(x.data_ptr()), None, None, None, 8, None)
            assert rc != 0 and b"dsd_variance_curves: this handle is a mel analysis handle" in lib.dsd_last_error(mh)
        finally:
            lib.dsd_destroy(mh)
        # a requested curve without its input signal
        rc = lib.dsd_variance_curves(hp, None, None, None, 1, 1000, (C.c_int64 * 1)(1000), 128, 512, (C.c_int64 * 1)(8), 2, 1,
                                     C.c_void_p(x.data_ptr()), None, None, None, 8, None)
        assert rc != 0
    finally:
        lib.dsd_destroy(hp)
    assert lib.dsd_hnsep_num_frames(0, 512) < 0
    # a hop past win_size / 2: the Nuttall window-square envelope can reach 0 (torch.istft raises there)
    sp, _, _ = sep_of("small", 1900)
    h = np.zeros(4000, np.float32)
    with pytest.raises(_lib.NativeLibraryError, match="hop_size"):
        sp.base_harmonic_ragged([h], [np.full(4000 // 300 + 1, 200.0)], SR, 300, 512)


def test_predict_from_audio_mono(g19):
    """HnSep.predict_from_audio on [B, 1, T] -> [B, 1, T], as nets.py:148-166 (G19's mono case and the float64 oracle)."""
    i = 1
    name, wseed, x = case(g19, i)
    sp, sd, cfg = sep_of(name, wseed)
    fl_h = float(g19[f"c{i}_floor"][0])
    got = sp.predict_from_audio(torch.from_numpy(x)[None, None])
    assert got.shape == (1, 1, len(x))
    got = got[0, 0].cpu().numpy()
    assert np.abs(got - g19[f"c{i}_harmonic"]).max() <= 3 * fl_h
    want, _ = hnsep_ref.separate(hnsep_ref.model64(sd, cfg), x, cfg)
    assert np.abs(got - want).max() <= 2 * fl_h
    with pytest.raises(ValueError, match=r"\[B, 1, T\]"):
        sp.predict_from_audio(torch.from_numpy(np.stack([x, x]))[None])


def test_predict_from_audio_stereo(g19):
    """a stereo model on real two-channel audio: each channel its own STFT, the network on both jointly, [B, 2, T] out,
    against the torch mirror in float64; its floor is the mirror's own fp32 error on the same input.  The same model on
    a clip repeated to both channels, averaged, is DecomposedWaveformVocalRemover._infer: separate_ragged."""
    i = 4
    name, wseed, x = case(g19, i)
    sp, sd, cfg = sep_of(name, wseed)
    x2 = mel_ref.waveform(1999, len(x), SR).astype(np.float32)
    xs = np.stack([x, x2])[None]
    got = sp.predict_from_audio(torch.from_numpy(xs))
    assert got.shape == (1, 2, len(x))
    got = got.cpu().numpy()
    with torch.no_grad():
        h64 = hnsep_ref.model64(sd, cfg).predict_from_audio(torch.from_numpy(xs.astype(np.float64))).numpy()
        h32 = hnsep_ref.model64(sd, cfg).float().predict_from_audio(torch.from_numpy(xs)).numpy()
    floor = float(np.abs(h32 - h64).max())
    assert np.abs(got - h64).max() <= 2 * floor, (np.abs(got - h64).max(), floor)
    assert np.abs(got[0, 0] - got[0, 1]).max() > 1e-3      # the channels are separated apart, not mixed
    rep = sp.predict_from_audio(torch.from_numpy(np.stack([x, x])[None])).cpu().numpy()
    mean = sp.separate_ragged([x])[0].cpu().numpy()
    assert np.abs(0.5 * (rep[0, 0] + rep[0, 1]) - mean).max() <= 1e-6
    with pytest.raises(ValueError, match=r"\[B, 2, T\]"):
        sp.predict_from_audio(torch.from_numpy(x)[None, None])


def test_binarizer_chain():
    """one 44.1-kHz clip all on the GPU: RMVPE f0, f0 * ~uv into DecomposedWaveform, then all four curves, each finite and
    of length `length`."""
    from diffsinger_amd.pitch import RMVPE
    pe = RMVPE(synth.rmvpe_state_dict(seed=1800, with_tf=True, **synth.RMVPE_SMALL))
    sp, _, _ = sep_of("prod", 1902)
    hop, win = 512, 2048
    x = mel_ref.waveform(1995, 3 * SR, SR).astype(np.float32)
    length = int(np.ceil(len(x) / hop))
    f0, uv = pe.get_pitch(x, SR, length, hop_size=hop, interp_uv=True)
    d = hnsep.DecomposedWaveform(x, SR, f0 * ~uv, hop_size=hop, fft_size=win, win_size=win, algorithm="vr", model=sp)
    curves = dict(energy=hnsep.get_energy_librosa(x, length, hop_size=hop, win_size=win, model=sp),
                  breathiness=hnsep.get_breathiness(d, SR, f0, length),
                  voicing=hnsep.get_voicing(d, SR, f0, length),
                  tension=hnsep.get_tension_base_harmonic(d, SR, f0, length))
    for k, v in curves.items():
        assert v.shape == (length,), k
        assert np.isfinite(v).all(), k
