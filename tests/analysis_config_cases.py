"""The cases of the analysis configuration suite: RMVPE (dsd_rmvpe_*) and the VR separator with the variance curves
(dsd_hnsep_*, dsd_base_harmonic, dsd_variance_curves) at the edges of what their create calls accept.  Shared by the host
tests (test_analysis_configs_host.py: the cases themselves, from the oracle and the fp32 torch mirror alone) and the GPU tests
(test_gpu_analysis_configs.py), so that both build the same seeded weights and signals (diffsinger_amd/synth.py,
make_golden_rmvpe.waveform, mel_ref.waveform).  Nothing is stored: every reference is recomputed from the seeds.

Oracles.  RMVPE: the torch mirror diffsinger_amd.pitch.E2E0 in float64 (the numpy restatement rmvpe_ref.mel2hidden takes
6 .. 13 s on the wide networks; the host test ties the two within 1e-12 on the two cheapest cases).  Separator:
hnsep_ref.model64 / hnsep_ref.separate, as in test_gpu_hnsep.py.

Bars.  The floor of a case is |fp32 mirror - float64 oracle| on the CPU; it moves by a factor of two or more with the thread
count and the torch build (another summation order), so a case's own floor is a sample and not a bound.  The bar of a case
is 2 max(family floor, the case's own floor): the family floors are the ones the merged tests record (RMVPE FLOOR = 1.1e-6;
the largest harmonic and mask floors of G19), and the factor 2 is theirs.  Both terms come from the reference side."""
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

import hnsep_ref
import mel_ref
import rmvpe_ref
from diffsinger_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SR = 44100


def _rmvpe_waveform(seed, n):
    if GOLDEN not in sys.path:
        sys.path.insert(0, GOLDEN)
    from make_golden_rmvpe import waveform
    return waveform(seed, n)


# ------------------------------------------------------------------------------------------------------------------ RMVPE
RMVPE_FLOOR = 1.1e-6            # the reference's fp32 against float64, max over G18 (tests/test_gpu_rmvpe.py)
RMVPE_SHORT = 160 * 20 + 3      # 21 frames: Tp = 32, so five levels leave one frame at the bottom (the odd-Tl quad)
RMVPE_LONG = 160 * 40 + 7       # 41 frames: Tp = 64


def _rm(n_blocks, n_gru, en_de_layers, inter_layers, en_out_channels, wseed, yseeds, reaches):
    return dict(cfg=dict(n_blocks=n_blocks, n_gru=n_gru, en_de_layers=en_de_layers, inter_layers=inter_layers,
                         en_out_channels=en_out_channels), wseed=wseed, yseeds=yseeds, lens=(RMVPE_SHORT, RMVPE_LONG),
                reaches=reaches)


# tag: configuration, weight seed, waveform seeds of the short and the long clip, what rmvpe_run / rm_conv3_kernel /
# rm_tconv_kernel path only this row reaches
RMVPE = OrderedDict(
    e1_c8=_rm(1, 1, 1, 1, 8, 2201, (2251, 2252),
              "one level: 64 bins at the bottom, one 8-channel group in blockIdx.y, the GRU input (1536 floats per frame) "
              "is the largest tensor of the scratch rotation"),
    e2_c24_lin=_rm(2, 0, 2, 2, 24, 2232, (2253, 2254),
                   "24 / 48 / 96 channels (no power of two) through the CIV == 4 loads of a concatenated source, two blocks "
                   "per layer and two inter layers (identity and 1x1-shortcut residuals both), the Linear head"),
    e3_c8=_rm(1, 1, 3, 1, 8, 2203, (2255, 2256), "odd depth: 16 bins at the bottom, three skip tensors"),
    e4_c16_b3=_rm(3, 1, 4, 3, 16, 2204, (2257, 2258),
                  "three blocks per layer (two identity residuals after the shortcut one), three inter layers"),
    e5_c40_lin=_rm(1, 0, 5, 1, 40, 2205, (2259, 2260),
                   "the widest non-power-of-two network: 1280 channels at the bottom, where the short clip has one frame"),
    e2_c64=_rm(1, 1, 2, 1, 64, 2206, (2261, 2262), "the accepted maximum width: 64 / 128 / 256 channels, 8 .. 32 groups"),
)
RMVPE_TIE = ("e1_c8", "e3_c8")      # the two cheapest in the numpy restatement

# rates whose gcd with 16000 gives another polyphase table: (orig, new, width) = (3, 1, 388), (3, 2, 194), (441, 320, 179)
# and the upsampling (1, 2, 130).  No rate coprime to 16000: its table would hold 16000 phases
RESAMPLE_RATES = (48000, 24000, 22050, 8000)
RESAMPLE_WSEED = 1800               # test_gpu_rmvpe.py's RMVPE_SMALL network


def rmvpe_sd(tag):
    c = RMVPE[tag]
    return synth.rmvpe_state_dict(seed=c["wseed"], with_tf=True, **c["cfg"])


def rmvpe_clips(tag):
    c = RMVPE[tag]
    return [_rmvpe_waveform(s, n) for s, n in zip(c["yseeds"], c["lens"])]


def resample_clip(sr):
    """about 0.3 s at `sr`, with the near-silent middle fifth of the RMVPE clips"""
    n = int(0.3 * sr) + 11
    x = mel_ref.waveform(2270 + RESAMPLE_RATES.index(sr), n, sr).astype(np.float64)
    a, b = 2 * n // 5, 3 * n // 5
    x[a:b] = 0.003 * np.random.default_rng(2280 + sr % 97).standard_normal(b - a)
    return x.astype(np.float32)


def rmvpe_mirror(sd, cfg, dtype=torch.float64):
    from diffsinger_amd.pitch import E2E0
    m = E2E0(cfg["n_blocks"], cfg["n_gru"], (2, 2), cfg["en_de_layers"], cfg["inter_layers"], 1, cfg["en_out_channels"])
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m.to(dtype).eval()


def rmvpe_hidden(model, mel):
    """RMVPE.mel2hidden (inference.py:24-29) on the torch mirror: mel [128, T] -> hidden [T, 360] in the model's dtype."""
    dtype = next(model.parameters()).dtype
    t = mel.shape[1]
    x = torch.from_numpy(np.ascontiguousarray(mel)).to(dtype)[None]
    x = torch.nn.functional.pad(x, (0, 32 * ((t - 1) // 32 + 1) - t), mode="constant")
    with torch.no_grad():
        return model(x)[0, :t].numpy()


def ambiguous_share(hidden, bound, thred=0.03):
    """the share of frames test_gpu_rmvpe.check_decoded skips: top-2 margin or |max - thred| within `bound`"""
    srt = np.sort(hidden, axis=1)
    return float(np.mean((srt[:, -1] - srt[:, -2] <= bound) | (np.abs(srt[:, -1] - thred) <= bound)))


# -------------------------------------------------------------------------------------------------------------- separator
def _hs(n_fft, hop, nout, nout_lstm, mono, n, n2, wseed, yseed, reaches):
    return dict(cfg=dict(n_fft=n_fft, hop_length=hop, nout=nout, nout_lstm=nout_lstm, is_mono=mono), wseed=wseed,
                yseeds=(yseed, yseed + 50), lens=(n, n2), reaches=reaches)


# tag: configuration, samples of the main clip (64 spectrogram frames; 32 for hop 1) and of the short second clip of the ragged
# call (32 frames), weight seed, waveform seed, what hs_* path only this row reaches
HNSEP = OrderedDict(
    f128_h32_n4=_hs(128, 32, 4, 8, True, 1293, 300, 2301, 2351,
                    "64 bins drop to 4 (2 in the bands) at the bottom: the ASPP taps at dilation 4 / 8 / 12 read padding, the "
                    "bilinear sources run at Fs = 2; nout 4: couts 1 .. 32 and the co >= cout skip; LSTM H = 4 and 2"),
    f128_h64_n4_st=_hs(128, 64, 4, 8, False, 2573, 700, 2302, 2352, "hop == n_fft / 2, the accepted limit; stereo at nout 4"),
    f192_h40_n12=_hs(192, 40, 12, 24, True, 1613, 400, 2303, 2353,
                     "97 bins against the 64-row DFT tile; hop 40 does not divide 192; couts 3 .. 96, no multiple of 16; "
                     "LSTM H = 12 and 6"),
    f320_h100_n8=_hs(320, 100, 8, 40, True, 4013, 1000, 2304, 2354, "hop 100 does not divide 320 (3 or 4 frames per sample); "
                     "LSTM H = 20 and 10"),
    f512_h1_n8=_hs(512, 1, 8, 16, True, 20, 7, 2305, 2355, "hop 1: every sample under all of a clip's 32 frames"),
    f512_h256_n20=_hs(512, 256, 20, 16, True, 10253, 3000, 2306, 2356, "hop == n_fft / 2; nout 20: couts 5 .. 160"),
    f512_h77_n8_st=_hs(512, 77, 8, 128, False, 3093, 800, 2307, 2357,
                       "hop 77 (6 or 7 frames per sample); LSTM H = 64 fills sW exactly, next to H = 32; stereo"),
    f1024_h300_n64=_hs(1024, 300, 64, 8, True, 12013, 3000, 2308, 2358, "the widest network (cout up to 512) on the narrowest "
                       "LSTM; hop 300"),
    f4096_h1000_n4=_hs(4096, 1000, 4, 8, True, 40013, 9000, 2319, 2359, "the largest DFT (2049 bins, 65 row tiles); hop 1000"),
)

# dsd_base_harmonic (win, hop): the limits of win_size, hop 1, and a hop that divides nothing -> the samples of the two clips of
# the ragged call (no multiple of the hop: the last frame lies partly past the end).  At hop == win / 2 the samples past the
# last frame's centre lie under that frame alone, where istft divides by the Nuttall window's square on its way to 0 (1e-5 at
# the frame's end): a remainder of 5 or 6 samples keeps the divisor above 0.9, so that the float32 floor is a rounding
# error and not the window's conditioning (at 1500 samples, remainder 28, the oracle itself peaks at 15)
BASE_HARMONIC = OrderedDict([((64, 32), (1509, 1030)), ((4096, 1000), (30011, 9013)), ((512, 1), (700, 419)),
                             ((320, 77), (5003, 2011))])
CURVES = ((64, 32), (4096, 1000))


def hnsep_sd(tag):
    c = HNSEP[tag]
    return synth.hnsep_state_dict(c["cfg"], c["wseed"])


def hnsep_clips(tag):
    c = HNSEP[tag]
    return [mel_ref.waveform(s, n, SR).astype(np.float32) for s, n in zip(c["yseeds"], c["lens"])]


def hnsep_spec(x, cfg):
    """predict_from_audio's spectrogram of a mono clip on every channel of the model: [C, bins, frames] complex128"""
    s, _ = hnsep_ref.spec_of(x, cfg)
    return np.stack([s] * (1 if cfg["is_mono"] else 2))


def hnsep_models(sd, cfg):
    """the float64 oracle network and its fp32 mirror (one construction: the nout 64 network holds 58 M weights)"""
    import copy
    m64 = hnsep_ref.model64(sd, cfg)
    return m64, copy.deepcopy(m64).float()


def hnsep_mirror32(m32, cfg, x):
    """the fp32 torch mirror on the clip (a stereo model sees it on both channels, averaged) -> harmonic part, mask"""
    c = 1 if cfg["is_mono"] else 2
    with torch.no_grad():
        h = m32.predict_from_audio(torch.from_numpy(np.stack([x] * c))[None])[0].mean(0).numpy()
        mk = m32(torch.from_numpy(hnsep_spec(x, cfg)[None].astype(np.complex64)))[0].numpy()
    return h, mk


def g19_family_floors():
    """the largest harmonic and mask floors G19 records (the reference's own fp32 run against the float64 oracle)"""
    z = np.load(os.path.join(GOLDEN, "g19_hnsep.npz"))
    fl = np.array([z[f"c{i}_floor"][:2] for i in range(int(z["n_cases"]))])
    return float(fl[:, 0].max()), float(fl[:, 1].max())


def base_f0(win, n_frames, seed):
    """an f0 track for _kth_harmonic at window `win`: around max(220 Hz, centre bin 5.5) with a 27 % swing (the band's edges
    cross bins; the phase keeps every frame's band edges centre +- 3.5 off the integers, which the host test asserts:
    on an edge the float32 and float64 masks may differ by a whole bin), a stretch on both sides of centre = 1 (masked out below it), an unvoiced gap (interp_f0 fills it), and four
    frames short of the clip so that the edge pad runs"""
    m = n_frames - 4
    one = SR / win                                  # the f0 whose centre bin is 1
    f0 = max(220.0, 5.5 * one) * (1.0 + 0.27 * np.sin(np.arange(m) / 9.0 + seed + 0.3))
    k = max(m // 6, 1)
    f0[k:2 * k] = 0.0
    f0[3 * k:3 * k + (k + 1) // 2] = one * 0.998
    f0[3 * k + (k + 1) // 2:4 * k + 1] = one * 1.002
    return f0


def base_clip(win, hop, i):
    n = BASE_HARMONIC[(win, hop)][i]
    return mel_ref.waveform(2400 + win % 89 + i, n, SR).astype(np.float32)
