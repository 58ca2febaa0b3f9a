"""The cases of the vocoder configuration suite: the NSF-HiFiGAN generator (dsd_vocoder_create / dsd_vocode / dsd_vocode_ragged)
at the edges of what check_vocoder_config (api.hip) accepts.  Shared by the generator of G28
(tests/golden/make_golden_vocoder_configs.py), the host tests (test_vocoder_configs_host.py), the GPU tests
(test_gpu_vocoder_configs.py) and tools/bf16x3_vocoder_tolerance.py, so that all build the same seeded weights
(synth.synth_state_dict, one seed per case) and inputs (built as vocoder_x3_cases.inputs builds them, the source's width
following harmonic_num).  Sampling rate 44100 throughout.

Each case names what it reaches (`reaches`; api.hip = build_packed_voc / make_gemm / vocode_impl).  `accepts(h)` is the Python
mirror of check_vocoder_config: the whole predicate, same order, a fragment of the library's message as the reason.

Bound: TOL = 5e-5 of the waveform range against the float64 oracle (test_gpu_vocoder.py's bound) where the case's floor - the
fp32 oracle against the float64 oracle on the same inputs - is at most TOL / 2, else 2 x floor (the rule of
encoder_size_cases.py).  FLOORS below are printed by

    python -m pytest tests/test_vocoder_configs_host.py -s -k floors

("floor <tag> <B> <T> <value>") and, for the G28 forms, by the fixture generator."""
import functools
from collections import OrderedDict

import numpy as np

from diffsinger_amd import synth
from oracle import vocoder as ov

TOL = 5e-5
SAME = 1e-5         # a ragged item against its lone call: test_gpu_vocoder_ragged.py's rule, relative to max(1, max |wav|)
GAIN = 0.7
MAX_LDS = 160 * 1024

_KEQU = dict(upsample_rates=[4, 2], upsample_kernel_sizes=[4, 2], upsample_initial_channel=64, resblock_kernel_sizes=[3],
             resblock_dilation_sizes=[[1]])
_NW = dict(upsample_rates=[2, 8, 8], upsample_kernel_sizes=[4, 16, 16], resblock_kernel_sizes=[3], resblock_dilation_sizes=[[1]])

# tag: over (config over synth.NSF_HIFIGAN_DEFAULT), dense shapes [(B, T)], weight seed, gain
CASES = OrderedDict(
    # k = u: D = 0 in build_packed_voc (api.hip, the `voc_up_taps` loop) - the transposed conv is a 1-tap scatter GEMM (HL = 0);
    # stages of 32 / 16 channels: residual blocks and conv_post on tconv.hip
    k_eq_u=dict(over=_KEQU, shapes=[(2, 37), (1, 1)], wseed=2801, gain=GAIN,
                reaches="D = 0: 1-tap scatter GEMM; 32 / 16 channels on tconv.hip"),
    # k = 8u: D = 4, 9-tap phase rows, most taps of most phases zero
    k_8u=dict(over=dict(upsample_rates=[2, 2], upsample_kernel_sizes=[16, 16], upsample_initial_channel=128),
              shapes=[(2, 37), (1, 1)], wseed=2802, gain=GAIN, reaches="D = 4: 9-tap phase rows; widths 64 / 32"),
    # between the two: k = 4u is D = 2 (5 taps), k = 6u is D = 3 (7 taps) - every tap count of build_packed_voc has a case
    k_4u_6u=dict(over=dict(upsample_rates=[2, 2], upsample_kernel_sizes=[8, 12], upsample_initial_channel=128,
                           resblock_kernel_sizes=[3], resblock_dilation_sizes=[[1]]),
                 shapes=[(2, 37)], wseed=2814, gain=GAIN, reaches="D = 2 and D = 3: 5- and 7-tap phase rows"),
    # odd rates: u * ch = 144 / 120 / 24 rows, no multiple of 64 - the scatter epilogue's 64-row tile is cut inside a phase;
    # num_mels 20: Kreal = 20 of K = 32 in conv_pre; k = 1 (HL = 0) and k = 15 (reach 7 and 42) residual convs on the GEMM
    # path at widths 48 / 24 / 12 (K = 48 / 32 / 16 with Kreal 24 and 12); pre-noise on
    odd_rates=dict(over=dict(num_mels=20, upsample_rates=[3, 5, 2], upsample_kernel_sizes=[9, 5, 16], upsample_initial_channel=96,
                             resblock="2", resblock_kernel_sizes=[1, 15], resblock_dilation_sizes=[[1, 3], [1, 6]],
                             noise_sigma=0.25),
                   shapes=[(2, 37)], wseed=2803, gain=GAIN,
                   reaches="u * ch = 144 / 120 / 24 rows; Kreal 20 of 32; k = 1 and k = 15 on the GEMM path; widths 48 / 24 / 12"),
    # n_ups = 1: the only noise conv is the k = 1 one at the output rate; 32 channels on tconv.hip at its widest reach
    # (k 13 x dilation 8 = 48) with 4 dilations per block
    one_up=dict(over=dict(num_mels=80, upsample_rates=[4], upsample_kernel_sizes=[4], upsample_initial_channel=64,
                          resblock_kernel_sizes=[13], resblock_dilation_sizes=[[1, 2, 4, 8]]),
                shapes=[(2, 37)], wseed=2804, gain=GAIN, g28_gain=0.5,       # the three-dilation G28 form saturates at 0.7
                reaches="n_ups = 1: only the k = 1 noise conv; tconv.hip at reach 48 with 4 dilations"),
    # thin stages: widths 24 / 12 / 6 / 3 (K = 32 / 16 / 16 / 16 padded rows), voc_noise_conv_kernel with 256 / 24 = 10 and
    # 256 / 3 = 85 frame groups (threads past groups * C idle), conv_post on 3 channels, num_mels 17, k = u / 2u / 3u / 8u
    # (1 / 3 / 3 / 9 taps)
    thin=dict(over=dict(num_mels=17, upsample_rates=[2, 2, 2, 2], upsample_kernel_sizes=[2, 4, 6, 16], upsample_initial_channel=48,
                        resblock_kernel_sizes=[3, 5, 7], resblock_dilation_sizes=[[1], [2], [3]]),
              shapes=[(2, 37)], wseed=2805, gain=GAIN,
              reaches="widths 24 / 12 / 6 / 3; noise conv with 10 and 85 frame groups; conv_post on 3 channels"),
    # the layer counts at their maxima: 8 stages, 8 kernels per stage (every odd k to 15), widths 256 .. 2
    max_counts=dict(over=dict(upsample_rates=[2] * 8, upsample_kernel_sizes=[4] * 8, upsample_initial_channel=512,
                              resblock_kernel_sizes=[1, 3, 5, 7, 9, 11, 13, 15], resblock_dilation_sizes=[[1]] * 8),
                    shapes=[(1, 5)], wseed=2806, gain=GAIN, reaches="8 stages, 8 kernels per stage, widths 256 .. 2"),
    # the acceptance limits (what dsd_vocoder_create accepts runs): ups.0 with K = 848 resident at 3 taps, 848 x 48 x 4 =
    # 162 816 of 163 840 bytes; a residual conv at width 272 and reach 48, 272 x 144 x 4 = 156 672 bytes
    wide_limit=dict(over=dict(upsample_rates=[2, 2], upsample_kernel_sizes=[4, 4], upsample_initial_channel=848, resblock="2",
                              resblock_kernel_sizes=[3], resblock_dilation_sizes=[[1]]),
                    shapes=[(1, 9)], wseed=2807, gain=0.55,       # at 0.7 a fifth of the samples sit in tanh's saturation
                    reaches="ups.0 at 848 x 48 x 4 = 162 816 of 163 840 bytes"),
    reach_limit=dict(over=dict(upsample_rates=[2, 2], upsample_kernel_sizes=[4, 4], upsample_initial_channel=544, resblock="2",
                               resblock_kernel_sizes=[9], resblock_dilation_sizes=[[12]]),
                     shapes=[(1, 70)], wseed=2808, gain=GAIN, reaches="width 272 at reach 48: 156 672 bytes"),
    # voc_noise_conv_kernel's source window beyond the default 64 KiB of dynamic LDS: C = 16, sf = 64, k = 128 is
    # (16 x 16 - 1) x 64 + 128 floats = 65 792 bytes (the raised limit); C0 = 8: C = 4 would need 262 KiB with its 64 groups,
    # voc_noise_groups caps them at 39; widths 4 / 2 / 1
    noise_window=dict(over=dict(_NW, upsample_initial_channel=32), shapes=[(1, 5)], wseed=2809, gain=GAIN,
                      reaches="noise conv window of 65 792 bytes"),
    noise_window_c4=dict(over=dict(_NW, upsample_initial_channel=8), shapes=[(1, 5)], wseed=2810, gain=GAIN,
                         reaches="noise conv window beyond the CU's LDS: capped groups; widths 4 / 2 / 1"),
    # mini_nsf with exactly two stages: source_conv (k = 1) lands on the last stage, the source rate is the output rate; an odd
    # last rate is allowed here; k = 3u at u = 5 (D = 1, three taps in every phase), k = u = 3
    mini_two=dict(over=dict(mini_nsf=True, upsample_rates=[5, 3], upsample_kernel_sizes=[15, 3], upsample_initial_channel=128,
                            resblock_kernel_sizes=[3, 7], resblock_dilation_sizes=[[1, 3], [2, 5]]),
                  shapes=[(2, 37)], wseed=2811, gain=GAIN, reaches="mini with two stages; odd last rate; widths 64 / 32"),
    # voc_source_kernel at dim = 1 (the fundamental alone, rand_ini unused) and dim = 16 (VOC_MAXDIM)
    harm0=dict(over=dict(_KEQU, harmonic_num=0), shapes=[(1, 12)], wseed=2812, gain=GAIN, reaches="voc_source_kernel at dim 1"),
    harm15=dict(over=dict(_KEQU, harmonic_num=15), shapes=[(1, 12)], wseed=2813, gain=GAIN, reaches="voc_source_kernel at dim 16"),
)

# ragged: these cases at T = 37 with these lengths through forward(lengths=)
RAGGED = ("odd_rates", "thin")
RAGGED_T, RAGGED_LENGTHS = 37, [37, 1, 16, 22]

# split-bf16 (set_precision("bf16x3"), voc_x3.hip): taps 1 / 13 / 15 and C = 192 / 160 (3 row blocks per wave, the rows above
# C zero; 160 = 5 k32 chunks) - the rates of vocoder_x3_cases._A
_A = dict(num_mels=32, upsample_rates=[4, 2, 2], upsample_kernel_sizes=[8, 4, 4])
X3 = OrderedDict(
    x3_c384=dict(over=dict(_A, upsample_initial_channel=384, resblock_kernel_sizes=[1, 13],
                           resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5]]), shapes=[(1, 33)], wseed=2821, gain=GAIN,
                 reaches="voc_x3.hip at taps 1 / 13, C = 192 and 96"),
    x3_c320=dict(over=dict(_A, upsample_initial_channel=320, resblock_kernel_sizes=[15], resblock_dilation_sizes=[[1, 3]]),
                 shapes=[(1, 33)], wseed=2822, gain=GAIN, reaches="voc_x3.hip at taps 15, C = 160"),
)
ALL = OrderedDict(list(CASES.items()) + list(X3.items()))

# G28: the reference Generator on these cases at B = 1, T = 12.  The reference's ResBlock1 is written out for exactly three
# dilations and its ResBlock2 for exactly two (models.py:40-47, :80-85: fewer raise, more are ignored), so it cannot build
# k_eq_u (one), one_up (four) or mini_two (ResBlock1 with two) as they stand: the fixture holds the "g28:<tag>" form of a case,
# the same config with every dilation list cut, or padded with its last value, to the length the reference's block takes.
# What G28 is there for - the transposed convolutions at k != 2u and odd rates, the noise convs at those rates, a two-stage
# mini_nsf - is the same in both forms.
G28 = ("k_eq_u", "k_8u", "odd_rates", "one_up", "mini_two")
G28_SHAPE = (1, 12)


def g28_dilations(h):
    n = 3 if str(h.get("resblock", "1")) == "1" else 2
    return [(list(d) + [d[-1]] * n)[:n] for d in h["resblock_dilation_sizes"]]

# (tag, B, T) -> fp32 oracle vs float64 oracle, max |difference| / max |float64 result|
FLOORS = {
    ('k_eq_u', 2, 37): 6.18e-07, ('k_eq_u', 1, 1): 2.79e-07, ('k_8u', 2, 37): 1.11e-06, ('k_8u', 1, 1): 1.13e-07,
    ('k_4u_6u', 2, 37): 7.63e-07, ('odd_rates', 2, 37): 6.55e-07, ('one_up', 2, 37): 9.68e-07, ('thin', 2, 37): 3.67e-07,
    ('max_counts', 1, 5): 2.18e-07, ('wide_limit', 1, 9): 7.22e-07, ('reach_limit', 1, 70): 2.03e-06,
    ('noise_window', 1, 5): 4.13e-07, ('noise_window_c4', 1, 5): 2.73e-07, ('mini_two', 2, 37): 6.7e-07,
    ('harm0', 1, 12): 5.99e-07, ('harm15', 1, 12): 6.03e-07, ('x3_c384', 1, 33): 9.05e-07, ('x3_c320', 1, 33): 5.59e-07,
}

# fp32 oracle vs the reference Generator on the G28 forms (test_vocoder_configs_host.py prints "g28 <tag> <value>")
G28_ORACLE_ERR = {
    'k_eq_u': 6.67e-07, 'k_8u': 7.33e-07, 'odd_rates': 8.14e-07, 'one_up': 3.89e-07, 'mini_two': 1.02e-06,
}


def config(tag):
    """the config of a case, or - "g28:<tag>" - of its G28 form"""
    base = tag.split(":")[-1]
    h = dict(synth.NSF_HIFIGAN_DEFAULT)
    h.update(ALL[base]["over"])
    h["hop_size"] = int(np.prod(h["upsample_rates"]))
    if tag.startswith("g28:"):
        h["resblock_dilation_sizes"] = g28_dilations(h)
    return h


@functools.lru_cache(maxsize=None)
def weights(tag):
    c = ALL[tag.split(":")[-1]]
    gain = c.get("g28_gain", c["gain"]) if tag.startswith("g28:") else c["gain"]
    return synth.synth_state_dict(synth.nsf_hifigan_param_shapes(config(tag)), seed=c["wseed"], gain=gain)


def make_inputs(h, bsz, t_len):
    """vocoder_x3_cases.inputs for any config: -> dict(mel [B, M, T] ln-mel, f0 [B, T], rand_ini [dim], noise [B, T upp, dim],
    pre_noise [B, C0, T]), dim = harmonic_num + 1; every 7th frame unvoiced"""
    upp, dim = int(np.prod(h["upsample_rates"])), ov.harmonic_num_of(h) + 1
    rng = np.random.Generator(np.random.PCG64(t_len))
    mel = (synth.synth_normal((bsz, h["num_mels"], t_len), 411) * 3.0 - 11.0).astype(np.float32)
    f0 = (150.0 * 2.0 ** rng.uniform(-1, 2, (bsz, t_len))).astype(np.float32)
    f0[:, ::7] = 0.0
    return dict(mel=mel, f0=f0, rand_ini=rng.random(dim).astype(np.float32), noise=synth.synth_normal((bsz, t_len * upp, dim), 412),
                pre_noise=synth.synth_normal((bsz, h["upsample_initial_channel"], t_len), 413))


@functools.lru_cache(maxsize=None)
def inputs(tag, bsz, t_len):
    return make_inputs(config(tag), bsz, t_len)


def item_inputs(tag, bsz, t_len, b, n):
    """item b of inputs(tag, bsz, t_len) alone, cut to its first n frames (what a ragged call computes for it)"""
    i = inputs(tag, bsz, t_len)
    upp = int(np.prod(config(tag)["upsample_rates"]))
    return dict(mel=i["mel"][b:b + 1, :, :n], f0=i["f0"][b:b + 1, :n], rand_ini=i["rand_ini"], noise=i["noise"][b:b + 1, :n * upp],
                pre_noise=i["pre_noise"][b:b + 1, :, :n])


def oracle(tag, i, dtype=np.float32):
    return ov.generator_forward(weights(tag), config(tag), i["mel"], i["f0"], i["rand_ini"], i["noise"], i["pre_noise"], dtype=dtype)


@functools.lru_cache(maxsize=None)
def reference(tag, bsz, t_len, dtype=np.float64):
    """the oracle's waveform of a dense case (read-only: computed once per process, shared by the tests)"""
    want = oracle(tag, inputs(tag, bsz, t_len), dtype)
    want.setflags(write=False)
    return want


@functools.lru_cache(maxsize=None)
def ragged_reference(tag, b, dtype=np.float64):
    want = oracle(tag, item_inputs(tag, len(RAGGED_LENGTHS), RAGGED_T, b, RAGGED_LENGTHS[b]), dtype)
    want.setflags(write=False)
    return want


def floor_of(got32, want64):
    want64 = np.asarray(want64)
    assert want64.dtype == np.float64 and got32.shape == want64.shape
    return float(np.abs(np.asarray(got32, np.float64) - want64).max() / max(np.abs(want64).max(), 1e-30))


def bound(tag, bsz, t_len):
    """TOL, or 2 x floor where the case's recorded floor exceeds TOL / 2"""
    floor = FLOORS[(tag, bsz, t_len)]
    return TOL if floor <= TOL / 2 else 2 * floor


# ------------------------------------------------------------------------------------------------ the accepted space
def _round_up(a, b):
    return (a + b - 1) // b * b


def gemm_tile_bytes(cin, taps, dil, bn=32):
    """gemm_generic_lds_bytes (api.hip): LDS of one bn-frame tile of a conv on the generic GEMM path - all round_up(cin, 16)
    input rows resident (a 1x1 walks chunks of 256), row stride = bn + 2 halo rounded up to 16 mod 32 floats"""
    k = _round_up(cin, 16)
    hl = _round_up((taps // 2) * dil, 4) if taps > 1 else 0
    s = bn + 2 * hl
    while s % 32 != 16:
        s += 4
    return (k if taps > 1 else min(k, 256)) * s * 4


def up_taps(u, k):
    """voc_up_taps (api.hip): taps of the phase-row GEMM of ConvTranspose1d(k, stride u, padding (k - u) / 2)"""
    pad, d = (k - u) // 2, 0
    for r in range(u):
        k0, e = (r + pad) % u, (r + pad) // u
        d = max(d, e, (k - 1 - k0) // u - e)
    return 2 * d + 1


def noise_groups(c, sf, ksz):
    """voc_noise_groups (vocoder_kernels.hip): frame groups per workgroup of the noise conv, 0: not even one window fits"""
    cpb = min(c, 256)
    room = MAX_LDS // 4 - ksz
    if room < 15 * sf:
        return 0
    return min(256 // cpb, (room // sf + 1) // 16)


def accepts(h):
    """check_vocoder_config (api.hip) on a config dict (the keys Generator reads) -> (True, "") or (False, reason): the reason is
    a fragment of the message dsd_vocoder_create leaves in dsd_last_error"""
    rates, ks = list(h["upsample_rates"]), list(h["upsample_kernel_sizes"])
    rk, rd = list(h["resblock_kernel_sizes"]), [list(d) for d in h["resblock_dilation_sizes"]]
    c0, mini = h["upsample_initial_channel"], bool(h.get("mini_nsf", False))
    n_ups, n_k = len(rates), len(rk)
    sigma = h.get("noise_sigma", None) or 0.0
    if (h["num_mels"] < 1 or h["sampling_rate"] < 1 or not 1 <= n_ups <= 8 or not 1 <= n_k <= 8 or len(ks) != n_ups or
            len(rd) != n_k or str(h.get("resblock", "1")) not in ("1", "2")):
        return False, "bad layer counts"
    if not 0 <= ov.harmonic_num_of(h) <= 15:
        return False, "harmonic_num must be in [0, 15]"
    if not sigma >= 0:
        return False, "noise_sigma must be >= 0"
    if mini and n_ups < 2:
        return False, "mini_nsf needs at least two upsampling stages"
    if c0 % (1 << n_ups) != 0 or (c0 >> n_ups) < 1:
        return False, "upsample_initial_channel must be divisible by 2^n_ups"
    for i, (u, k) in enumerate(zip(rates, ks)):
        if u < 1 or k < u or (k - u) % 2 != 0 or k > 8 * u:
            return False, f"upsample stage {i} (rate {u}, kernel {k}) is not supported"
    for j in range(n_k):
        if rk[j] < 1 or rk[j] % 2 == 0 or rk[j] > 15 or not 1 <= len(rd[j]) <= 4:
            return False, f"residual block {j}: odd kernel <= 15 and 1..4 dilations"
        for d, dil in enumerate(rd[j]):
            if dil < 1 or dil * (rk[j] // 2) > 48:
                return False, f"residual block {j} dilation {d} reaches beyond 48 frames"
    if not mini and n_ups >= 2 and rates[-1] % 2 != 0:
        return False, f"the last upsample rate ({rates[-1]}) must be even unless mini_nsf"

    def fits(layer, cin, taps, dil):
        n = gemm_tile_bytes(cin, taps, dil)
        return None if n <= MAX_LDS else f"{layer} ({cin} input channels, k = {taps} taps, dilation {dil}) needs {n} bytes of LDS"
    bad = fits("conv_pre", h["num_mels"], 7, 1)
    if bad:
        return False, bad
    for i in range(n_ups):
        ch = c0 >> (i + 1)
        bad = fits(f"ups.{i}", 2 * ch, up_taps(rates[i], ks[i]), 1)
        if bad:
            return False, bad
        if not mini and i + 1 < n_ups:
            sf = int(np.prod(rates[i + 1:], dtype=np.int64))
            if sf > (1 << 28) or noise_groups(ch, sf, 2 * sf) == 0:
                return False, f"noise_convs.{i} (stride {sf}, kernel {2 * sf}) needs a source window of {17 * sf * 4} bytes of LDS"
        if ch in (16, 32):
            continue
        for j in range(n_k):
            for dil in rd[j]:
                bad = fits(f"resblocks.{i * n_k + j}", ch, rk[j], dil)
                if bad:
                    return False, bad
    bad = fits("conv_post", c0 >> n_ups, 7, 1)
    if bad:
        return False, bad
    return True, ""


def over_default(**over):
    h = dict(synth.NSF_HIFIGAN_DEFAULT)
    h.update(over)
    return h


_TWO = dict(upsample_rates=[2, 2], upsample_kernel_sizes=[4, 4])
# what dsd_vocoder_create refuses: (config over the default, a fragment of dsd_last_error)
REFUSE = [
    # the LDS rule, decided at create time ("Vocoder configurations")
    (dict(upsample_initial_channel=1024), "ups.0 (1024 input channels, k = 3 taps, dilation 1) needs 196608 bytes of LDS"),
    (dict(_TWO, upsample_initial_channel=576, resblock_kernel_sizes=[9], resblock_dilation_sizes=[[12]]),
     "resblocks.0 (288 input channels, k = 9 taps, dilation 12) needs 165888 bytes of LDS"),
    (dict(num_mels=864), "conv_pre (864 input channels, k = 7 taps, dilation 1) needs 165888 bytes of LDS"),
    (dict(_TWO, upsample_initial_channel=864), "ups.0 (864 input channels, k = 3 taps, dilation 1) needs 165888 bytes of LDS"),
    (dict(upsample_rates=[2, 50, 50], upsample_kernel_sizes=[4, 100, 100], upsample_initial_channel=64),
     "noise_convs.0 (stride 2500, kernel 5000) needs a source window of 170000 bytes of LDS"),
    # configurations the reference cannot run (models.py:239-245)
    (dict(upsample_rates=[2, 3], upsample_kernel_sizes=[4, 3]), "the last upsample rate (3) must be even unless mini_nsf"),
    (dict(upsample_rates=[3, 5, 7], upsample_kernel_sizes=[3, 5, 7], upsample_initial_channel=64),
     "the last upsample rate (7) must be even unless mini_nsf"),
    # what it refused before
    (dict(num_mels=0), "bad layer counts"),
    (dict(upsample_rates=[], upsample_kernel_sizes=[]), "bad layer counts"),
    (dict(upsample_rates=[2] * 9, upsample_kernel_sizes=[4] * 9, upsample_initial_channel=1024), "bad layer counts"),
    (dict(resblock_kernel_sizes=[], resblock_dilation_sizes=[]), "bad layer counts"),
    (dict(resblock_kernel_sizes=[3] * 9, resblock_dilation_sizes=[[1]] * 9), "bad layer counts"),
    (dict(harmonic_num=16), "harmonic_num must be in [0, 15]"),
    (dict(harmonic_num=-1), "harmonic_num must be in [0, 15]"),
    (dict(noise_sigma=-0.5), "noise_sigma must be >= 0"),
    (dict(mini_nsf=True, upsample_rates=[4], upsample_kernel_sizes=[8]), "mini_nsf needs at least two upsampling stages"),
    (dict(upsample_initial_channel=48), "upsample_initial_channel must be divisible by 2^n_ups"),
    (dict(_TWO, upsample_initial_channel=0), "upsample_initial_channel must be divisible by 2^n_ups"),
    (dict(upsample_rates=[8, 8, 2, 2, 0], upsample_kernel_sizes=[16, 16, 4, 4, 0]), "upsample stage 4 (rate 0, kernel 0) is not supported"),
    (dict(_TWO, upsample_kernel_sizes=[4, 3]), "upsample stage 1 (rate 2, kernel 3) is not supported"),
    (dict(_TWO, upsample_kernel_sizes=[1, 4]), "upsample stage 0 (rate 2, kernel 1) is not supported"),
    (dict(_TWO, upsample_kernel_sizes=[18, 4]), "upsample stage 0 (rate 2, kernel 18) is not supported"),
    (dict(resblock_kernel_sizes=[3, 4, 11]), "residual block 1: odd kernel <= 15 and 1..4 dilations"),
    (dict(resblock_kernel_sizes=[3, 7, 17]), "residual block 2: odd kernel <= 15 and 1..4 dilations"),
    (dict(resblock_dilation_sizes=[[1, 3, 5], [], [1, 3, 5]]), "residual block 1: odd kernel <= 15 and 1..4 dilations"),
    (dict(resblock_dilation_sizes=[[1, 2, 3, 4, 5], [1], [1]]), "residual block 0: odd kernel <= 15 and 1..4 dilations"),
    (dict(resblock_dilation_sizes=[[1, 3, 5], [1, 3, 17], [1, 3, 5]]), "residual block 1 dilation 2 reaches beyond 48 frames"),
    (dict(resblock_dilation_sizes=[[1, 3, 0], [1, 3, 5], [1, 3, 5]]), "residual block 0 dilation 2 reaches beyond 48 frames"),
]
# beside the limits, accepted: the widest of each kind (wide_limit and reach_limit run; these are only created)
ACCEPT_EDGE = [
    dict(num_mels=848),
    dict(_TWO, upsample_initial_channel=704, resblock_kernel_sizes=[11], resblock_dilation_sizes=[[5]]),      # width 352, k 11 / d 5
    dict(_TWO, upsample_initial_channel=736, resblock_kernel_sizes=[7], resblock_dilation_sizes=[[4]]),       # width 368, halo 12
    dict(upsample_rates=[2, 49, 49], upsample_kernel_sizes=[4, 49, 49], upsample_initial_channel=64, mini_nsf=True),
    dict(upsample_rates=[2, 48, 50], upsample_kernel_sizes=[4, 96, 100], upsample_initial_channel=64),       # sf 2400: 163 200 bytes
]


def native_config(h, device=0):
    """DsdVocoderConfig of a config dict as Generator._config fills it, but of ANY dict: counts beyond the struct's arrays
    (n_ups = 9, 5 dilations) are passed as counts, the arrays hold what fits"""
    import ctypes as C
    from diffsinger_amd import _lib
    cfg = _lib.DsdVocoderConfig()
    cfg.struct_size = C.sizeof(_lib.DsdVocoderConfig)
    cfg.num_mels, cfg.sampling_rate, cfg.upsample_initial_channel = h["num_mels"], h["sampling_rate"], h["upsample_initial_channel"]
    rates, ks = list(h["upsample_rates"]), list(h["upsample_kernel_sizes"])
    cfg.n_ups = len(rates)
    for i, (u, k) in enumerate(list(zip(rates, ks))[:8]):
        cfg.upsample_rates[i], cfg.upsample_kernel_sizes[i] = u, k
    cfg.resblock = 1 if str(h.get("resblock", "1")) == "1" else 2
    rk, rd = list(h["resblock_kernel_sizes"]), [list(d) for d in h["resblock_dilation_sizes"]]
    cfg.n_kernels = len(rk)
    for j, (k, ds) in enumerate(list(zip(rk, rd))[:8]):
        cfg.resblock_kernel_sizes[j], cfg.n_dilations[j] = k, len(ds)
        for d, dv in enumerate(ds[:4]):
            cfg.resblock_dilation_sizes[j][d] = dv
    cfg.harmonic_num = int(h.get("harmonic_num", 8))
    cfg.mini_nsf = int(bool(h.get("mini_nsf", False)))
    cfg.noise_sigma = float(h.get("noise_sigma", None) or 0.0)
    cfg.device = device
    return cfg
