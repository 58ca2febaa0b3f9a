"""CPU checks of RMVPE pitch extraction: the float64 restatement (tests/rmvpe_ref.py) against G18, the HTK mel bank
(the library's host restatement and rmvpe_ref's) against transformers', the resampler's known answers, the frame count,
and the state_dict names.  No GPU."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import rmvpe_ref
from diffsinger_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FLOOR = 1.1e-6          # the reference's fp32 vs float64, max over the G18 cases (tests/test_gpu_rmvpe.py)
CONFIGS = [dict(n_blocks=4, n_gru=1, en_de_layers=5, inter_layers=4, en_out_channels=16), dict(synth.RMVPE_SMALL),
           dict(synth.RMVPE_SMALL, n_gru=0)]


def g18():
    return np.load(os.path.join(GOLDEN, "g18_rmvpe.npz"))


@pytest.mark.parametrize("i", [0, 2, 3])
def test_oracle_reproduces_g18(i):
    import sys
    sys.path.insert(0, GOLDEN)
    from make_golden_rmvpe import waveform
    z = g18()
    wseed, yseed, n, ci = (int(v) for v in z[f"c{i}_meta"])
    sd = synth.rmvpe_state_dict(seed=wseed, with_tf=True, **CONFIGS[ci])
    y = waveform(yseed, n)
    mel = rmvpe_ref.log_mel(y)
    assert np.abs(mel - z[f"c{i}_mel"]).max() < 1e-4
    h = rmvpe_ref.mel2hidden(mel, sd)
    assert np.abs(h - z[f"c{i}_hidden"]).max() <= FLOOR
    assert np.array_equal(rmvpe_ref.decode(h) > 0, z[f"c{i}_f0"] > 0) or np.abs(z[f"c{i}_max"] - 0.03).min() < FLOOR


def test_g18_is_non_degenerate():
    z = g18()
    mx = np.concatenate([z[f"c{i}_max"] for i in range(int(z["n_cases"]))])
    am = np.concatenate([z[f"c{i}_argmax"] for i in range(int(z["n_cases"]))])
    assert (mx < 0.03).any() and (mx > 0.03).any()
    assert am.min() < 60 and am.max() > 300


def test_decode_matches_reference_on_crafted_rows():
    z = g18()
    np.testing.assert_allclose(rmvpe_ref.decode(z["dec_hidden"]), z["dec_f0"], rtol=2e-6)


def test_htk_filterbank_matches_transformers():
    audio_utils = pytest.importorskip("transformers.audio_utils")
    from diffsinger_amd import _lib
    want = audio_utils.mel_filter_bank(num_frequency_bins=513, num_mel_filters=128, min_frequency=30, max_frequency=8000,
                                       sampling_rate=16000, norm="slaney", mel_scale="htk").T.astype(np.float32)
    got = np.zeros((128, 513), dtype=np.float32)
    assert _lib.lib().dsd_rmvpe_filterbank(got.ctypes.data_as(C.POINTER(C.c_float))) == 0
    np.testing.assert_allclose(got, want, rtol=2e-6, atol=1e-9)
    np.testing.assert_allclose(rmvpe_ref.htk_filterbank(), want, rtol=2e-6, atol=1e-9)


@pytest.mark.parametrize("sr", [44100, 48000, 22050])
def test_resampler_known_answers(sr):
    """Stand-ins for parity with torchaudio itself (not installed): the output length, unit DC gain, a tone below the
    rolloff (0.99 * 8 kHz) passes, one above 8 kHz is stopped."""
    n = sr // 2 + 37
    assert len(rmvpe_ref.resample(np.zeros(n), sr)) == math.ceil(16000 * n / sr) == rmvpe_ref.resampled_length(n, sr)
    k, width, orig, new = rmvpe_ref.resample_kernel(sr, 16000)
    assert k.dtype == np.float32 and k.shape == (new, 2 * width + orig)
    if sr == 44100:
        assert k.shape == (160, 1155)
    dc = rmvpe_ref.resample(np.ones(n), sr)
    mid = dc[len(dc) // 4: 3 * len(dc) // 4]
    assert np.abs(mid - 1).max() < 2e-3
    t = np.arange(n) / sr
    for f, lo, hi in ((1000.0, 0.99, 1.01), (7000.0, 0.98, 1.02), (9000.0, 0.0, 1e-3)):
        y = rmvpe_ref.resample(np.sin(2 * np.pi * f * t), sr)
        amp = np.sqrt(2 * np.mean(y[len(y) // 4: 3 * len(y) // 4] ** 2))
        assert lo <= amp <= hi, (f, amp)


def test_num_frames():
    from diffsinger_amd import _lib
    lib = _lib.lib()
    for n, sr in ((513, 16000), (16000, 16000), (160000, 16000), (44100 * 3 + 7, 44100), (48000, 48000), (22050, 22050)):
        n16 = n if sr == 16000 else math.ceil(16000 * n / sr)
        assert lib.dsd_rmvpe_num_frames(n, sr) == 1 + n16 // 160 == rmvpe_ref.num_frames(n, sr)
    assert lib.dsd_rmvpe_num_frames(512, 16000) < 0 and lib.dsd_rmvpe_num_frames(1000, 0) < 0


def test_state_dict_names_match_the_reference():
    """G18 stores the reference E2E0(4, 1, (2, 2))'s full key set (TimbreFilter included): synth's table is that set."""
    z = g18()
    shapes = synth.rmvpe_param_shapes(with_tf=True)
    assert list(shapes) == list(z["keys"])
    assert [",".join(map(str, s)) for s in shapes.values()] == list(z["key_shapes"])


def test_initialize_pe_rejects_cpu_extractors():
    from diffsinger_amd.pitch import initialize_pe
    for pe in ("parselmouth", "harvest"):
        with pytest.raises(NotImplementedError, match="reference"):
            initialize_pe({"pe": pe, "pe_ckpt": None})
    with pytest.raises(ValueError):
        initialize_pe({"pe": "crepe", "pe_ckpt": None})
