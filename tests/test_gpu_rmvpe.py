"""-m gpu: RMVPE pitch extraction (dsd_rmvpe_*, diffsinger_amd.pitch.RMVPE) against the reference's fp32 RMVPE (G18) and
the float64 restatement in tests/rmvpe_ref.py.

Tolerances are stated from measurement.  The reference's own fp32 CPU path sits within FLOOR = 1.1e-6 of the float64
restatement in the sigmoid output (max over the G18 cases: 1.1e-7 on the small configuration, 6.9e-7 on the production
one, 1.1e-6 on the Linear head; tests/golden/make_golden_rmvpe.py prints them).  The HIP hidden must stay within 2 FLOOR
of the float64 oracle and within FLOOR + 2 FLOOR of G18.  The argmax and f0 must be equal except on frames whose top-2
margin is below that bound (either candidate is accepted there), and voiced / unvoiced equal except where |max - thred|
is below it.  Ragged items must be bit-identical to their lone calls."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rmvpe_ref  # noqa: E402
from diffsinger_amd import synth  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FLOOR = 1.1e-6
BAR = 2 * FLOOR
FLOOR_10S = 1.4e-6          # the reference's fp32 error on test_production_10s's clip
CONFIGS = [dict(n_blocks=4, n_gru=1, en_de_layers=5, inter_layers=4, en_out_channels=16), dict(synth.RMVPE_SMALL),
           dict(synth.RMVPE_SMALL, n_gru=0)]
CONFIG_OF_META = {0: 0, 1: 1, 2: 2}      # make_golden_rmvpe.CONFIGS order: prod, small, small0


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"


_PE = {}


def pe_of(cfg_idx, seed):
    from diffsinger_amd.pitch import RMVPE
    key = (cfg_idx, seed)
    if key not in _PE:
        sd = synth.rmvpe_state_dict(seed=seed, with_tf=True, **CONFIGS[cfg_idx])
        _PE[key] = (RMVPE(sd), sd)
    return _PE[key]


def waveform(seed, n, sr=16000):
    import sys
    sys.path.insert(0, GOLDEN)
    from make_golden_rmvpe import waveform as wf
    if sr == 16000:
        return wf(seed, n)
    import mel_ref
    return mel_ref.waveform(seed, n, sr)


def check_decoded(f0, want_f0, hidden_ref, bound, thred=0.03):
    """f0 equal (to fp32 rounding of the cents) except where the top-2 margin or |max - thred| is within `bound`."""
    srt = np.sort(hidden_ref, axis=1)
    margin = srt[:, -1] - srt[:, -2]
    mx = srt[:, -1]
    ambiguous_uv = np.abs(mx - thred) <= bound
    voiced_got, voiced_want = f0 > 0, want_f0 > 0
    assert np.array_equal(voiced_got[~ambiguous_uv], voiced_want[~ambiguous_uv])
    both = voiced_got & voiced_want & (margin > bound)
    rel = np.abs(f0[both] - want_f0[both]) / want_f0[both]
    assert rel.size == 0 or rel.max() < 1e-4, rel.max()


def g18():
    return np.load(os.path.join(GOLDEN, "g18_rmvpe.npz"))


@pytest.mark.parametrize("i", range(5))
def test_g18_case(i):
    z = g18()
    wseed, yseed, n, ci = (int(v) for v in z[f"c{i}_meta"])
    pe, sd = pe_of(CONFIG_OF_META[ci], wseed)
    y = waveform(yseed, n)
    f0s = pe.infer_from_audio_ragged([y], 16000, want_hidden=True)
    f0, hid = f0s[0]
    h64 = rmvpe_ref.mel2hidden(rmvpe_ref.log_mel(y), sd)
    assert hid.shape == h64.shape and np.isfinite(hid).all()
    err = float(np.abs(hid - h64).max())
    assert err <= BAR, err
    if f"c{i}_hidden" in z:
        assert float(np.abs(hid - z[f"c{i}_hidden"]).max()) <= FLOOR + BAR
    check_decoded(f0, z[f"c{i}_f0"], h64, BAR)
    check_decoded(f0, rmvpe_ref.decode(h64), h64, BAR)
    lone = pe.infer_from_audio(y, 16000)
    assert np.array_equal(lone, f0)


@pytest.mark.parametrize("i", [0, 1, 2, 3])
def test_g18_mel2hidden(i):
    """The network alone, from the reference's own fp32 log-mel."""
    z = g18()
    wseed, yseed, n, ci = (int(v) for v in z[f"c{i}_meta"])
    pe, sd = pe_of(CONFIG_OF_META[ci], wseed)
    mel = z[f"c{i}_mel"]
    got = pe.mel2hidden(torch.from_numpy(mel)[None].cuda())[0].cpu().numpy()
    h64 = rmvpe_ref.mel2hidden(mel.astype(np.float64), sd)
    assert float(np.abs(got - h64).max()) <= BAR
    assert float(np.abs(got - z[f"c{i}_hidden"]).max()) <= FLOOR + BAR


def test_decode_crafted():
    z = g18()
    pe, _ = pe_of(1, 1800)
    h = z["dec_hidden"]
    got = pe.decode(torch.from_numpy(h)[None].cuda())
    want = z["dec_f0"]
    assert got[0] == 0 and want[0] == 0                       # all below the threshold
    np.testing.assert_allclose(got, want, rtol=2e-6)
    np.testing.assert_allclose(got, rmvpe_ref.decode(h), rtol=2e-6)
    with pytest.raises(NotImplementedError):
        pe.decode(torch.from_numpy(h)[None].cuda(), use_viterbi=True)


def test_production_10s():
    """1001 frames through the production network.  The floor is the reference's own fp32 error on this very clip
    (measured with tests/golden/make_golden_rmvpe.py's setup: 1.4e-6, the 1024-step GRU's longer tail than G18's)."""
    pe, sd = pe_of(0, 1802)
    y = waveform(1851, 160000)
    f0, hid = pe.infer_from_audio_ragged([y], 16000, want_hidden=True)[0]
    h64 = rmvpe_ref.mel2hidden(rmvpe_ref.log_mel(y), sd)
    assert float(np.abs(hid - h64).max()) <= 2 * FLOOR_10S
    check_decoded(f0, rmvpe_ref.decode(h64), h64, 2 * FLOOR_10S)


def test_ragged_batch_matches_lone_calls():
    """8 clips over several Tp classes (one shorter than 32 frames, one exactly at a multiple of 32) in one call."""
    pe, _ = pe_of(1, 1800)
    lens = [16000 * 3 + 11, 2000, 63 * 160 + 5, 16000 + 999, 513, 16000 * 2, 7000, 31 * 160]
    ys = [waveform(1860 + k, n) for k, n in enumerate(lens)]
    got = pe.infer_from_audio_ragged(ys, 16000, want_hidden=True)
    tps = {32 * -(-rmvpe_ref.num_frames(n) // 32) for n in lens}
    assert len(tps) >= 5 and min(rmvpe_ref.num_frames(n) for n in lens) < 32
    for y, (f0, hid) in zip(ys, got):
        f0_1, hid_1 = pe.infer_from_audio_ragged([y], 16000, want_hidden=True)[0]
        assert np.array_equal(hid, hid_1) and np.array_equal(f0, f0_1)


def test_44k_resample_and_get_pitch():
    pe, sd = pe_of(0, 1802)
    y = waveform(1870, 44100 * 2 + 123, 44100)
    f0 = pe.infer_from_audio(y, 44100)
    y16 = rmvpe_ref.resample(y, 44100)
    assert len(f0) == rmvpe_ref.num_frames(len(y), 44100) == 1 + len(y16) // 160
    h64 = rmvpe_ref.mel2hidden(rmvpe_ref.log_mel(y16), sd)
    want = rmvpe_ref.decode(h64)
    check_decoded(f0, want, h64, BAR)
    # the resampled audio itself, through the ragged call's hidden: within the bound of the float64 resampler's
    _, hid = pe.infer_from_audio_ragged([y], 44100, want_hidden=True)[0]
    assert float(np.abs(hid - h64).max()) <= BAR
    for speed in (1, 1.25):
        length = int(np.ceil(len(y) / round(512 * speed)))
        for interp in (False, True):
            f0r, uvr = pe.get_pitch(y, 44100, length, hop_size=512, speed=speed, interp_uv=interp)
            wf, wuv = rmvpe_ref.get_pitch_post(want.astype(np.float32), 44100, length, 512, speed, interp)
            assert f0r.shape == (length,) and uvr.dtype == bool
            ok = np.abs(f0r - wf) <= 1e-3 * np.maximum(wf, 1)
            assert ok.mean() > 0.97, ok.mean()


def test_g18_get_pitch():
    z = g18()
    wseed, yseed, n, ci = (int(v) for v in z["c4_meta"])
    pe, _ = pe_of(CONFIG_OF_META[ci], wseed)
    y = waveform(yseed, n)
    for k in range(int(z["n_pitch"])):
        hop, speed, interp, length = z[f"p{k}_args"]
        f0r, uvr = pe.get_pitch(y, 16000, int(length), hop_size=int(hop), speed=speed, interp_uv=bool(interp))
        assert f0r.shape == z[f"p{k}_f0"].shape
        assert (uvr == z[f"p{k}_uv"]).mean() > 0.97
        ok = np.abs(f0r - z[f"p{k}_f0"]) <= 1e-3 * np.maximum(z[f"p{k}_f0"], 1)
        assert ok.mean() > 0.97


def test_resynthesis_smoke():
    """44.1 kHz waveform -> diffsinger_amd.mel + RMVPE.get_pitch -> dsd_vocode (synthetic vocoder weights): finite, the
    expected length."""
    import mel_ref
    from diffsinger_amd.mel import STFT
    from test_gpu_vocoder import build
    c = mel_ref.PROD
    gen, h, _ = build({}, 430)
    y = mel_ref.waveform(12, 30000, c["sr"])
    mel = STFT(c["sr"], c["n_mels"], c["n_fft"], c["win_size"], c["hop"], c["fmin"], c["fmax"]).get_mel(torch.from_numpy(y)[None].cuda())
    t_len = mel.shape[2]
    pe, _ = pe_of(0, 1802)
    f0, uv = pe.get_pitch(y, c["sr"], t_len, hop_size=c["hop"], interp_uv=True)
    assert f0.shape == (t_len,) and (f0 > 0).all()
    with torch.no_grad():
        wav = gen(mel, torch.from_numpy(f0.astype(np.float32))[None].cuda())
    assert wav.shape[-1] == t_len * 512 and torch.isfinite(wav).all()
    gen.release_native()


def test_errors_and_handle_kinds():
    import ctypes as C
    from diffsinger_amd import _lib
    lib = _lib.lib()
    pe, _ = pe_of(1, 1800)
    st = _lib.DsdStats()
    assert lib.dsd_get_stats(pe._h, C.byref(st)) == -2
    assert lib.dsd_set_lengths(pe._h, None, 1, None) == -2
    x = torch.zeros(1, 128, 8, device="cuda")
    assert lib.dsd_mel_analyze(pe._h, C.c_void_p(x.data_ptr()), 1, 8, 8, None, 0.0, 1.0, C.c_void_p(x.data_ptr()), 1, 1, 1, None) == -2
    cfg = _lib.DsdMelConfig(C.sizeof(_lib.DsdMelConfig), 16000, 1024, 1024, 160, 128, 30.0, 8000.0, 1e-5, 0)
    mh = C.c_void_p()
    assert lib.dsd_mel_create(C.byref(cfg), C.byref(mh)) == 0
    out = torch.zeros(1, 8, 360, device="cuda")
    assert lib.dsd_rmvpe_mel_to_hidden(mh, C.c_void_p(x.data_ptr()), 1, 8, 1024, 8, 1, None, C.c_void_p(out.data_ptr()), 2880, 360, None) == -2
    lib.dsd_destroy(mh)
    rc = _lib.DsdRmvpeConfig(C.sizeof(_lib.DsdRmvpeConfig), 1, 1, 5, 1, 16, 0)
    h = C.c_void_p()
    assert lib.dsd_rmvpe_create(C.byref(rc), C.byref(h)) == 0
    assert lib.dsd_rmvpe_mel_to_hidden(h, C.c_void_p(x.data_ptr()), 1, 8, 1024, 8, 1, None, C.c_void_p(out.data_ptr()), 2880, 360, None) == -2
    one = np.ones(4, dtype=np.float32)
    shp = (C.c_int64 * 1)(4)
    ptr = one.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.dsd_load_weight(h, b"unet.tf.layers.0.conv.0.conv.0.weight", ptr, shp, 1, 0) == 0     # ignored
    assert lib.dsd_load_weight(h, b"unet.encoder.bn.num_batches_tracked", ptr, shp, 0, 0) == 0        # ignored
    assert lib.dsd_load_weight(h, b"fc.2.weight", ptr, shp, 1, 0) == -5                                # DSD_ENOTFOUND
    assert lib.dsd_load_weight(h, b"unet.encoder.bn.weight", ptr, shp, 1, 0) == -1                     # shape [1]
    assert lib.dsd_finalize_weights(h) == -2                                                           # keys missing
    lib.dsd_destroy(h)
    with pytest.raises(ValueError):
        pe.infer_from_audio(np.zeros(400, dtype=np.float32))
