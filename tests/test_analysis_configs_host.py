"""The cases of tests/analysis_config_cases.py themselves, without a GPU and without the native library: what the GPU tests of
test_gpu_analysis_configs.py compare against, and whether each case could see an error.

- Oracle ties: the float64 torch mirror E2E0 equals the numpy restatement rmvpe_ref.mel2hidden within 1e-12 on the two
  cheapest RMVPE cases, which licenses the mirror as the oracle of the wide ones (the restatement takes 6 .. 13 s there).  The
  separator's oracle is hnsep_ref.model64 already.
- Floors: |fp32 mirror - oracle| of every case is at most twice the floor its family records (RMVPE 1.1e-6; the largest
  harmonic and mask floors of G19), so no new case is harder than the merged ones.  Measured with 8 and with 1 CPU threads:
  RMVPE 2.6e-8 .. 1.3e-6 (the 24-channel Linear-head network), separator harmonic 1.8e-8 .. 6.5e-7, mask 3.9e-7 .. 8.1e-6.
- Each case can see an error: RMVPE's frame maximum stays below 0.99 with at least 4 argmax classes over the case's clips;
  the separator's harmonic peak is at least 0.05 with at least 10 % of the mask magnitudes in (0.1, 0.9).
- At most 10 % of an RMVPE case's frames are ones check_decoded skips as ambiguous (a condition on the inputs).
- Every oracle takes under 3 s (the shorter of two runs; measured 0.03 .. 0.9 s, the nout 64 separator the slowest)."""
import time

import numpy as np
import pytest
import torch

import analysis_config_cases as ac
import hnsep_ref
import rmvpe_ref

ORACLE_SECONDS = 3.0


def timed(fn):
    """fn's result and the shorter of two run times, for every case alike: the limit is on what the oracle costs, and the
    first run also pays for thread start-up and cold caches"""
    times = []
    for _ in range(2):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return out, min(times)


@pytest.mark.parametrize("tag", ac.RMVPE_TIE)
def test_rmvpe_mirror_is_the_numpy_oracle(tag):
    c = ac.RMVPE[tag]
    sd = ac.rmvpe_sd(tag)
    m64 = ac.rmvpe_mirror(sd, c["cfg"])
    assert rmvpe_ref.config_of(sd) == tuple(c["cfg"][k] for k in ("n_blocks", "n_gru", "en_de_layers", "inter_layers",
                                                                   "en_out_channels"))
    for y in ac.rmvpe_clips(tag):
        mel = rmvpe_ref.log_mel(y)
        err = float(np.abs(ac.rmvpe_hidden(m64, mel) - rmvpe_ref.mel2hidden(mel, sd)).max())
        print(f"{tag}: float64 mirror vs numpy restatement {err:.3g}")
        assert err <= 1e-12, err


@pytest.mark.parametrize("tag", list(ac.RMVPE))
def test_rmvpe_case(tag):
    c = ac.RMVPE[tag]
    sd = ac.rmvpe_sd(tag)
    m64, m32 = ac.rmvpe_mirror(sd, c["cfg"]), ac.rmvpe_mirror(sd, c["cfg"], torch.float32)
    clips = ac.rmvpe_clips(tag)
    frames = [rmvpe_ref.num_frames(len(y)) for y in clips]
    assert frames[0] <= 32 < frames[1] <= 64            # Tp 32 and 64
    hid, floor, seconds = [], 0.0, 0.0
    for y in clips:
        mel = rmvpe_ref.log_mel(y)
        h64, sec = timed(lambda: ac.rmvpe_hidden(m64, mel))
        seconds = max(seconds, sec)
        floor = max(floor, float(np.abs(ac.rmvpe_hidden(m32, mel.astype(np.float32)) - h64).max()))
        hid.append(h64)
    hid = np.concatenate(hid)
    bar = 2 * max(ac.RMVPE_FLOOR, floor)
    amb = ac.ambiguous_share(hid, bar)
    print(f"{tag}: fp32 mirror floor {floor:.3g}, frame max {hid.max():.3f}, {len(set(hid.argmax(1)))} argmax classes, "
          f"{np.mean(hid.max(1) > 0.03):.2f} voiced, {amb:.3f} ambiguous, oracle {seconds:.2f} s")
    assert floor <= 2 * ac.RMVPE_FLOOR, floor
    assert hid.max() < 0.99
    assert len(set(hid.argmax(1))) >= 4
    assert amb <= 0.10, amb
    assert seconds < ORACLE_SECONDS, seconds


@pytest.mark.parametrize("sr", ac.RESAMPLE_RATES)
def test_resample_case(sr):
    """the polyphase table of each rate is another one, and the clip is long enough for RMVPE's reflect pad"""
    k, width, orig, new = rmvpe_ref.resample_kernel(sr, 16000)
    assert (orig, new, width) == {48000: (3, 1, 388), 24000: (3, 2, 194), 22050: (441, 320, 179), 8000: (1, 2, 130)}[sr]
    assert new <= 320
    y = ac.resample_clip(sr)
    assert rmvpe_ref.num_frames(len(y), sr) == 1 + len(rmvpe_ref.resample(y, sr)) // 160 >= 28


@pytest.mark.parametrize("tag", list(ac.HNSEP))
def test_hnsep_case(tag):
    c = ac.HNSEP[tag]
    cfg, sd = c["cfg"], ac.hnsep_sd(tag)
    fam_h, fam_m = ac.g19_family_floors()
    m64, m32 = ac.hnsep_models(sd, cfg)
    from diffsinger_amd import hnsep
    want_frames = (32 if cfg["hop_length"] == 1 else 64, 32)
    for x, nfr in zip(ac.hnsep_clips(tag), want_frames):
        assert hnsep.padding(len(x), cfg["hop_length"])[2] == nfr
        (h64, mk64), seconds = timed(lambda: hnsep_ref.separate(m64, x, cfg))
        h32, mk32 = ac.hnsep_mirror32(m32, cfg, x)
        fl_h, fl_m = float(np.abs(h32 - h64).max()), float(np.abs(mk32 - mk64).max())
        a = np.abs(mk64)
        mid = float(np.mean((a > 0.1) & (a < 0.9)))
        print(f"{tag}, {len(x)} samples: fp32 mirror floor harmonic {fl_h:.3g} mask {fl_m:.3g}, peak {np.abs(h64).max():.3f}, "
              f"|mask| in (0.1, 0.9) {mid:.2f}, oracle {seconds:.2f} s")
        assert fl_h <= 2 * fam_h and fl_m <= 2 * fam_m, (fl_h, fl_m)
        assert np.abs(h64).max() >= 0.05
        assert mid >= 0.10, mid
        if not cfg["is_mono"]:
            assert np.abs(mk64[0] - mk64[1]).max() > 1e-3
        assert seconds < ORACLE_SECONDS, seconds


@pytest.mark.parametrize("win,hop", list(ac.BASE_HARMONIC))
def test_base_harmonic_case(win, hop):
    """the f0 track crosses centre = 1 and has an unvoiced gap; the clip's last frame lies partly past its end; the float32
    restatement has an error to state the bar from, and the base harmonic is not silence"""
    for i, n in enumerate(ac.BASE_HARMONIC[(win, hop)]):
        assert n > win // 2 and (hop == 1 or n % hop != 0)
        f0 = ac.base_f0(win, n // hop + 1, i)
        centre = f0 * win / ac.SR
        assert (f0 == 0).any() and ((centre > 0) & (centre < 1)).any() and (centre > 1).any() and len(f0) < n // hop + 1
        edges = np.concatenate([hnsep_ref.base_f0(f0, n, hop) * win / ac.SR + d for d in (-3.5, 3.5, 0.0)])
        assert np.abs(edges - np.round(edges)).min() > 1e-4        # no band edge (and no centre == 1) on a bin: no fp32 / float64 tie
        h = ac.base_clip(win, hop, i)
        want = hnsep_ref.base_harmonic(h, f0, ac.SR, hop, win)
        floor = float(np.abs(hnsep_ref.base_harmonic(h, f0, ac.SR, hop, win, dtype=np.float32) - want).max())
        print(f"base harmonic ({win}, {hop}), {n} samples: float32 restatement {floor:.3g}, peak {np.abs(want).max():.3g}")
        assert floor > 0 and 0.01 < np.abs(want).max() < 1.5
