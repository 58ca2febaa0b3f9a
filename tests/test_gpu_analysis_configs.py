"""-m gpu: RMVPE and the VR separator with the variance curves at the edges of what dsd_rmvpe_create, dsd_hnsep_create and
dsd_base_harmonic accept (the cases of tests/analysis_config_cases.py; test_analysis_configs_host.py checks the cases
themselves).  test_gpu_rmvpe.py and test_gpu_hnsep.py run en_de_layers 5 / en_out_channels 16 and hop == n_fft / 4 only.

Every result is compared with a float64 oracle recomputed from the seeds: the torch mirror E2E0 in float64 (tied to the numpy
restatement by the host test), hnsep_ref.separate, hnsep_ref.base_harmonic, hnsep_ref.energy / tension.  The bar of a case is
2 max(family floor, the case's own fp32-mirror floor), separately for RMVPE's hidden, the separator's harmonic part and its
mask: both terms come from the reference side (analysis_config_cases.py says why a case's own floor alone is no bound).  The
base harmonic's bar is twice the float32 restatement's own error, as test_gpu_hnsep.py states it; the curves keep that file's
bars.  Ragged items must be bit-identical to their lone calls.  Every test prints what it measured (DESIGN.md sections 4g
and 4h carry the tables)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import analysis_config_cases as ac  # noqa: E402
import hnsep_ref  # noqa: E402
import mel_ref  # noqa: E402
import rmvpe_ref  # noqa: E402
from diffsinger_amd import _lib, hnsep, synth  # noqa: E402
from test_gpu_hnsep import CURVE_DB_BAR, TENSION_BAR  # noqa: E402
from test_gpu_rmvpe import BAR, check_decoded  # noqa: E402

SR = ac.SR
DSD_EINVAL = -1


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"


# ------------------------------------------------------------------------------------------------------------------ RMVPE
@pytest.mark.parametrize("tag", list(ac.RMVPE))
def test_rmvpe_config(tag):
    from diffsinger_amd.pitch import RMVPE
    c = ac.RMVPE[tag]
    sd = ac.rmvpe_sd(tag)
    m64, m32 = ac.rmvpe_mirror(sd, c["cfg"]), ac.rmvpe_mirror(sd, c["cfg"], torch.float32)
    clips = ac.rmvpe_clips(tag)
    mels = [rmvpe_ref.log_mel(y) for y in clips]
    h64 = [ac.rmvpe_hidden(m64, mel) for mel in mels]
    floor = max(float(np.abs(ac.rmvpe_hidden(m32, mel.astype(np.float32)) - h).max()) for mel, h in zip(mels, h64))
    bar = 2 * max(ac.RMVPE_FLOOR, floor)
    pe = RMVPE(sd)              # released by __del__ when the test returns
    assert pe.config == c["cfg"]
    rag = pe.infer_from_audio_ragged(clips, 16000, want_hidden=True)
    for y, mel, want, (f0, hid) in zip(clips, mels, h64, rag):
        assert hid.shape == want.shape and np.isfinite(hid).all()
        err = float(np.abs(hid - want).max())
        # the network alone, from the oracle's log-mel rounded to float32: a front-end error and a network error show apart
        mel32 = mel.astype(np.float32)
        net = pe.mel2hidden(torch.from_numpy(mel32)[None].cuda())[0].cpu().numpy()
        err_net = float(np.abs(net - ac.rmvpe_hidden(m64, mel32.astype(np.float64))).max())
        print(f"{tag}, {len(want)} frames: waveform -> hidden {err:.3g}, mel -> hidden {err_net:.3g}, fp32 mirror floor "
              f"{floor:.3g}, bar {bar:.3g}")
        assert err_net <= bar, (err_net, bar)
        assert err <= bar, (err, bar)
        check_decoded(f0, rmvpe_ref.decode(want), want, bar)
        f0_1, hid_1 = pe.infer_from_audio_ragged([y], 16000, want_hidden=True)[0]
        assert np.array_equal(hid, hid_1) and np.array_equal(f0, f0_1)
        assert np.array_equal(pe.infer_from_audio(y, 16000), f0)


@pytest.fixture(scope="module")
def pe_small():
    from diffsinger_amd.pitch import RMVPE
    sd = synth.rmvpe_state_dict(seed=ac.RESAMPLE_WSEED, with_tf=True, **synth.RMVPE_SMALL)
    pe = RMVPE(sd)
    yield pe, ac.rmvpe_mirror(sd, synth.RMVPE_SMALL)
    del pe


@pytest.mark.parametrize("sr", ac.RESAMPLE_RATES)
def test_resample_rate(pe_small, sr):
    """as test_gpu_rmvpe.test_44k_resample_and_get_pitch: the hidden within BAR of the oracle on the float64-resampled
    audio, the frame count, the decoded f0.  The four rates share one handle: its table cache grows by one per rate."""
    pe, m64 = pe_small
    y = ac.resample_clip(sr)
    f0, hid = pe.infer_from_audio_ragged([y], sr, want_hidden=True)[0]
    y16 = rmvpe_ref.resample(y, sr)
    assert len(f0) == rmvpe_ref.num_frames(len(y), sr) == 1 + len(y16) // 160
    h64 = ac.rmvpe_hidden(m64, rmvpe_ref.log_mel(y16))
    err = float(np.abs(hid - h64).max())
    print(f"{sr} Hz, {len(f0)} frames: waveform -> hidden {err:.3g}, bar {BAR:.3g}")
    assert err <= BAR, err
    check_decoded(f0, rmvpe_ref.decode(h64), h64, BAR)
    assert np.array_equal(pe.infer_from_audio(y, sr), f0)


# -------------------------------------------------------------------------------------------------------------- separator
@pytest.mark.parametrize("tag", list(ac.HNSEP))
def test_hnsep_config(tag):
    c = ac.HNSEP[tag]
    cfg, sd = c["cfg"], ac.hnsep_sd(tag)
    fam_h, fam_m = ac.g19_family_floors()
    m64, m32 = ac.hnsep_models(sd, cfg)
    clips = ac.hnsep_clips(tag)
    sp = hnsep.HnSep(sd, cfg)   # released by __del__ when the test returns
    rag = sp.separate_ragged(clips)
    for x, r in zip(clips, rag):
        assert torch.equal(r, sp.separate_ragged([x])[0])
        want, mk64 = hnsep_ref.separate(m64, x, cfg)
        h32, mk32 = ac.hnsep_mirror32(m32, cfg, x)
        fl_h, fl_m = float(np.abs(h32 - want).max()), float(np.abs(mk32 - mk64).max())
        bar_h, bar_m = 2 * max(fam_h, fl_h), 2 * max(fam_m, fl_m)
        got = r.cpu().numpy()
        gm = sp.mask(torch.from_numpy(ac.hnsep_spec(x, cfg)[None].astype(np.complex64))).cpu().numpy()[0]
        assert got.shape == want.shape and gm.shape == mk64.shape and np.isfinite(got).all() and np.isfinite(gm).all()
        err_h, err_m = float(np.abs(got - want).max()), float(np.abs(gm - mk64).max())
        print(f"{tag}, {len(x)} samples: harmonic {err_h:.3g} (fp32 mirror floor {fl_h:.3g}, bar {bar_h:.3g}), mask "
              f"{err_m:.3g} (floor {fl_m:.3g}, bar {bar_m:.3g})")
        assert err_m <= bar_m, (err_m, bar_m)
        assert err_h <= bar_h, (err_h, bar_h)
        if not cfg["is_mono"]:
            assert np.abs(gm[0] - gm[1]).max() > 1e-3          # the two channels' masks differ


@pytest.fixture(scope="module")
def sp_small():
    """dsd_base_harmonic and dsd_variance_curves use no weights: any separator handle serves"""
    sp = hnsep.HnSep(synth.hnsep_state_dict(synth.HNSEP_SMALL, 1900), dict(synth.HNSEP_SMALL))
    yield sp
    del sp


@pytest.mark.parametrize("win,hop", list(ac.BASE_HARMONIC))
def test_base_harmonic_config(sp_small, win, hop):
    lens = ac.BASE_HARMONIC[(win, hop)]
    hs = [ac.base_clip(win, hop, i) for i in range(len(lens))]
    f0s = [ac.base_f0(win, n // hop + 1, i) for i, n in enumerate(lens)]
    rag = sp_small.base_harmonic_ragged(hs, f0s, SR, hop, win)
    for h, f0, r in zip(hs, f0s, rag):
        assert torch.equal(r, sp_small.base_harmonic_ragged([h], [f0], SR, hop, win)[0])
        want = hnsep_ref.base_harmonic(h, f0, SR, hop, win)
        floor = float(np.abs(hnsep_ref.base_harmonic(h, f0, SR, hop, win, dtype=np.float32) - want).max())
        err = float(np.abs(r.cpu().numpy() - want).max())
        print(f"base harmonic ({win}, {hop}), {len(h)} samples: error {err:.3g}, float32 restatement {floor:.3g}, peak "
              f"{np.abs(want).max():.3g}")
        assert np.abs(want).max() > 0.01 and floor > 0
        assert err <= 2 * floor, (err, floor)


@pytest.mark.parametrize("win,hop", ac.CURVES)
def test_variance_curves_config(sp_small, win, hop):
    """the four curves at the limits of win_size, in one ragged call: a clip shorter than win / 2 (its frames hold zero
    padding on both sides) and `frames` both past the natural frame count (the pad, then the top-db clamp) and short of it
    (the crop)."""
    lens = (12 * hop + hop // 3, win // 2 - 5)
    xs = [mel_ref.waveform(2450 + i, n, SR).astype(np.float32) for i, n in enumerate(lens)]
    hs = [(0.7 * mel_ref.waveform(2460 + i, n, SR)).astype(np.float32) for i, n in enumerate(lens)]
    bs = [(0.6 * h).astype(np.float32) for h in hs]
    natural = [n // hop + 1 for n in lens]
    for frames in ([natural[0] + 7, max(natural[1] - 1, 1)], [natural[0] - 5, natural[1] + 3]):
        cv = sp_small.curves_ragged(xs, hs, bs, frames, hop, win, domain="ratio")
        for i, (x, h, b, length) in enumerate(zip(xs, hs, bs, frames)):
            ref = dict(energy=hnsep_ref.energy(x, length, hop, win), breathiness=hnsep_ref.energy(x - h, length, hop, win),
                       voicing=hnsep_ref.energy(h, length, hop, win))
            for k, v in ref.items():
                assert cv[k][i].shape == (length,)
                err = float(np.abs(cv[k][i] - v).max())
                assert err <= CURVE_DB_BAR, (k, i, err)
            err_t = float(np.abs(cv["tension"][i] - hnsep_ref.tension(h, b, length, hop, win, "ratio")).max())
            print(f"curves ({win}, {hop}), {len(x)} samples, {length} frames (natural {natural[i]}): tension {err_t:.3g}")
            assert err_t <= TENSION_BAR, (i, err_t)
            if length > natural[i]:          # the padded frames: amin's -100 dB under the top-db clamp
                assert cv["energy"][i][-1] == pytest.approx(max(cv["energy"][i].max() - 80.0, -100.0), abs=1e-3)
            lone = sp_small.curves_ragged([x], [h], [b], [length], hop, win, domain="ratio")
            for k in lone:
                assert np.array_equal(cv[k][i], lone[k][0]), k


# ------------------------------------------------------------------------------------------------- rejected configurations
RMVPE_OK = dict(n_blocks=1, n_gru=1, en_de_layers=5, inter_layers=1, en_out_channels=16)
RMVPE_REJECTED = [dict(en_out_channels=4), dict(en_out_channels=12), dict(en_out_channels=72), dict(en_de_layers=0),
                  dict(en_de_layers=6), dict(inter_layers=0), dict(n_blocks=0), dict(n_gru=2)]
HNSEP_OK = dict(n_fft=512, hop_length=128, nout=8, nout_lstm=16, is_mono=1)
HNSEP_REJECTED = [dict(n_fft=64, hop_length=16), dict(n_fft=96, hop_length=24), dict(n_fft=4160), dict(hop_length=0),
                  dict(hop_length=257), dict(nout=0), dict(nout=6), dict(nout=68), dict(nout_lstm=0), dict(nout_lstm=12),
                  dict(nout_lstm=136), dict(is_mono=2)]


def test_the_accepted_configurations_next_to_the_rejected_ones():
    """the base of every rejected case below is itself accepted: each rejection is the one changed field's"""
    lib = _lib.lib()
    for cfg in (_lib.DsdRmvpeConfig(C.sizeof(_lib.DsdRmvpeConfig), *RMVPE_OK.values(), 0),
                _lib.DsdHnsepConfig(C.sizeof(_lib.DsdHnsepConfig), *HNSEP_OK.values(), 0)):
        hp = C.c_void_p()
        create = lib.dsd_rmvpe_create if isinstance(cfg, _lib.DsdRmvpeConfig) else lib.dsd_hnsep_create
        assert create(C.byref(cfg), C.byref(hp)) == 0 and hp.value
        lib.dsd_destroy(hp)


@pytest.mark.parametrize("change", RMVPE_REJECTED, ids=lambda d: "-".join(f"{k}{v}" for k, v in d.items()))
def test_rmvpe_create_rejects(change):
    c = dict(RMVPE_OK, **change)
    cfg = _lib.DsdRmvpeConfig(C.sizeof(_lib.DsdRmvpeConfig), c["n_blocks"], c["n_gru"], c["en_de_layers"], c["inter_layers"],
                              c["en_out_channels"], 0)
    hp = C.c_void_p()
    assert _lib.lib().dsd_rmvpe_create(C.byref(cfg), C.byref(hp)) == DSD_EINVAL
    assert hp.value is None
    assert b"dsd_rmvpe_create" in _lib.lib().dsd_last_error(None)


@pytest.mark.parametrize("change", HNSEP_REJECTED, ids=lambda d: "-".join(f"{k}{v}" for k, v in d.items()))
def test_hnsep_create_rejects(change):
    c = dict(HNSEP_OK, **change)
    cfg = _lib.DsdHnsepConfig(C.sizeof(_lib.DsdHnsepConfig), c["n_fft"], c["hop_length"], c["nout"], c["nout_lstm"],
                              c["is_mono"], 0)
    hp = C.c_void_p()
    assert _lib.lib().dsd_hnsep_create(C.byref(cfg), C.byref(hp)) == DSD_EINVAL
    assert hp.value is None
    assert b"dsd_hnsep_create" in _lib.lib().dsd_last_error(None)


@pytest.mark.parametrize("win,hop", [(48, 12), (4128, 1000), (512, 257), (64, 33)])
def test_base_harmonic_rejects(sp_small, win, hop):
    h = np.zeros(6000, np.float32)
    with pytest.raises(_lib.NativeLibraryError, match=r"dsd_base_harmonic failed \(-1\)"):
        sp_small.base_harmonic_ragged([h], [np.full(6000 // hop + 1, 300.0)], SR, hop, win)
