"""The NSF-HiFiGAN vocoder at every configuration dsd_vocoder_create accepts, without a GPU (cases: vocoder_config_cases.py).

G28 (tests/golden/g28_vocoder_configs.npz, generator make_golden_vocoder_configs.py) holds the reference Generator's own fp32
waveforms at k = u, k = 8u, odd rates, one stage and a two-stage mini_nsf.  The fp32 numpy oracle is checked against it within
the project's stated oracle-vs-reference figure (TOL = 5e-5 of the waveform range, test_gpu_vocoder.py), which pins
oracle/vocoder.py for transposed convolutions other than k = 2u: tests/test_gpu_vocoder_configs.py uses its float64 mode as
the reference.

The boundary: dsd_vocoder_create validates before it selects a device, so everything it refuses - the layer-count rules, the LDS
rule of the resident k-tap convolutions, the configurations the reference cannot run - is checked here against the library
itself and against the Python mirror `accepts()`."""
import ctypes as C
import os

import numpy as np
import pytest

import vocoder_config_cases as cc
from oracle import vocoder as ov

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_SENTINEL = 0x5A5A5A50
DENSE = [(tag, b, t) for tag, c in cc.ALL.items() for b, t in c["shapes"]]


def load():
    return np.load(os.path.join(GOLDEN, "g28_vocoder_configs.npz"))


def g28_inputs(g, tag):
    """the G28 form's inputs at G28_SHAPE; f0 and rand_ini come from numpy's generator, the fixture holds what it gave"""
    i = cc.inputs("g28:" + tag, *cc.G28_SHAPE)
    assert np.array_equal(i["rand_ini"], g[f"{tag}_rand_ini"]) and np.array_equal(i["f0"], g[f"{tag}_f0"])
    return i


@pytest.mark.parametrize("tag", cc.G28)
def test_g28_oracle_vs_reference(tag):
    g = load()
    from diffsinger_amd import synth
    assert synth.state_dict_digest(cc.weights("g28:" + tag)) == str(g[f"{tag}_digest"])
    assert cc.accepts(cc.config("g28:" + tag)) == (True, "")
    got = cc.oracle("g28:" + tag, g28_inputs(g, tag))
    want = g[f"{tag}_wav"]
    err = cc.floor_of(got, np.asarray(want, np.float64))
    print(f"g28 {tag} {err:.3g}")
    assert got.shape == want.shape == (cc.G28_SHAPE[0], 1, cc.G28_SHAPE[1] * int(np.prod(cc.config(tag)["upsample_rates"])))
    assert err < cc.TOL, (tag, err)
    assert np.abs(want).max() >= 0.05 and want.std() >= 0.02 and float((np.abs(want) > 0.99).mean()) <= 0.01
    assert abs(err - cc.G28_ORACLE_ERR[tag]) <= 0.5 * cc.G28_ORACLE_ERR[tag] + 1e-7      # the recorded figure is this one


def test_floors_are_the_recorded_ones():
    """fp32 oracle vs float64 oracle of every dense case and every ragged item: what FLOORS records (within 25 %: the
    matmul's summation order is the BLAS build's) and what the GPU test's bound is made of"""
    for tag, b, t in DENSE:
        floor = cc.floor_of(cc.reference(tag, b, t, np.float32), cc.reference(tag, b, t))
        print(f"floor {tag} {b} {t} {floor:.3g}")
        rec = cc.FLOORS[(tag, b, t)]
        assert abs(floor - rec) <= 0.25 * rec + 5e-8, (tag, b, t, floor, rec)
        assert cc.bound(tag, b, t) == (cc.TOL if rec <= cc.TOL / 2 else 2 * rec)
    for tag in cc.RAGGED:
        for b, n in enumerate(cc.RAGGED_LENGTHS):
            floor = cc.floor_of(cc.ragged_reference(tag, b, np.float32), cc.ragged_reference(tag, b))
            print(f"floor {tag} ragged item {b} (T = {n}) {floor:.3g}")
            assert floor <= cc.TOL / 2        # the ragged items are held to TOL itself


@pytest.mark.parametrize("tag,bsz,t_len", DENSE)
def test_case_meets_the_conditions(tag, bsz, t_len):
    """on the reference side alone: the waveform is neither silent nor saturated (a saturated tanh hides errors), and every
    item has voiced and unvoiced frames"""
    wav = cc.reference(tag, bsz, t_len, np.float32)
    f0 = cc.inputs(tag, bsz, t_len)["f0"]
    sat = float((np.abs(wav) > 0.99).mean())
    print(f"{tag} ({bsz}, {t_len}): peak {np.abs(wav).max():.2f} std {wav.std():.3f} saturated {100 * sat:.2f} %")
    assert np.isfinite(wav).all()
    assert np.abs(wav).max() >= 0.05 and wav.std() >= 0.02 and sat <= 0.01
    if t_len > 1:
        assert ((f0 > 0).any(axis=1) & (f0 == 0).any(axis=1)).all()
    assert t_len <= 70 and wav.shape[2] <= 17000


def test_ragged_items_meet_the_conditions():
    for tag in cc.RAGGED:
        for b, n in enumerate(cc.RAGGED_LENGTHS):
            wav = cc.ragged_reference(tag, b, np.float32)
            assert np.abs(wav).max() >= 0.05 and wav.std() >= 0.02 and float((np.abs(wav) > 0.99).mean()) <= 0.01, (tag, b)


def test_float32_mode_is_the_old_path():
    """dtype=np.float32 is the oracle as it was, bit for bit, on a merged layout (vocoder_x3_cases "B": ResBlock2, reach 48): the
    default argument, the explicit one, and the old code written out below with float32 spelled in every place"""
    import vocoder_x3_cases as x3
    i = x3.inputs("B", 2, 70)
    args = (x3.weights("B"), x3.config("B"), i["mel"], i["f0"], i["rand_ini"], i["noise"], i["pre_noise"])
    old = ov.generator_forward(*args)
    new = ov.generator_forward(*args, dtype=np.float32)
    assert old.dtype == new.dtype == np.float32 and np.array_equal(old, new)
    assert np.array_equal(old, _frozen_fp32_forward(*args))
    wide = ov.generator_forward(*args, dtype=np.float64)
    assert wide.dtype == np.float64 and 0 < cc.floor_of(old, wide) < cc.TOL / 2


def _frozen_fp32_forward(p, h, mel, f0, rand_ini, noise, pre_noise):
    """The fp32 generator as oracle/vocoder.py spelled it before it took a dtype, for a non-mini layout: written out with
    explicit float32 so that a change of the shared helpers' default shows."""
    F32 = np.float32

    def lrelu(x, s):
        return np.where(x >= 0, x, x * F32(s)).astype(F32)

    def conv(x, w, b, dilation=1, padding=0, stride=1):
        bsz, ci, t = x.shape
        co, _, k = w.shape
        xp = np.zeros((bsz, ci, t + 2 * padding), dtype=F32)
        xp[:, :, padding:padding + t] = x
        to = (t + 2 * padding - dilation * (k - 1) - 1) // stride + 1
        y = np.zeros((bsz, co, to), dtype=F32)
        for j in range(k):
            y += np.matmul(np.ascontiguousarray(w[:, :, j]), xp[:, :, j * dilation: j * dilation + (to - 1) * stride + 1: stride])
        return (y + b[None, :, None]).astype(F32)

    def tconv(x, w, b, stride, padding):
        bsz, ci, t = x.shape
        _, co, k = w.shape
        full = np.zeros((bsz, co, (t - 1) * stride + k), dtype=F32)
        for j in range(k):
            full[:, :, j: j + (t - 1) * stride + 1: stride] += np.matmul(np.ascontiguousarray(w[:, :, j]).T, x)
        return (full[:, :, padding: full.shape[2] - padding] + b[None, :, None]).astype(F32)

    rates, ksz = h["upsample_rates"], h["upsample_kernel_sizes"]
    rk, rd = h["resblock_kernel_sizes"], h["resblock_dilation_sizes"]
    assert not h.get("mini_nsf") and str(h["resblock"]) == "2"
    har = ov.sine_source(p, f0, int(np.prod(rates)), h["sampling_rate"], rand_ini, noise)
    x = conv(np.asarray(mel, dtype=F32), p["conv_pre.weight"], p["conv_pre.bias"], padding=3)
    if h.get("noise_sigma"):
        x = (x + F32(h["noise_sigma"]) * np.asarray(pre_noise, dtype=F32)).astype(F32)
    for i, (u, k) in enumerate(zip(rates, ksz)):
        x = tconv(lrelu(x, 0.1), p[f"ups.{i}.weight"], p[f"ups.{i}.bias"], u, (k - u) // 2)
        if i + 1 < len(rates):
            sf = int(np.prod(rates[i + 1:]))
            x = (x + conv(har, p[f"noise_convs.{i}.weight"], p[f"noise_convs.{i}.bias"], stride=sf, padding=sf // 2)).astype(F32)
        else:
            x = (x + conv(har, p[f"noise_convs.{i}.weight"], p[f"noise_convs.{i}.bias"])).astype(F32)
        acc = None
        for j in range(len(rk)):
            y = x
            for n, d in enumerate(rd[j]):
                pre = f"resblocks.{i * len(rk) + j}.convs.{n}."
                y = (conv(lrelu(y, 0.1), p[pre + "weight"], p[pre + "bias"], dilation=d, padding=(rk[j] * d - d) // 2) + y).astype(F32)
            acc = y if acc is None else (acc + y).astype(F32)
        x = (acc / F32(len(rk))).astype(F32)
    return np.tanh(conv(lrelu(x, 0.01), p["conv_post.weight"], p["conv_post.bias"], padding=3)).astype(F32)


def test_harmonic_num_is_read_from_the_config():
    from diffsinger_amd import synth
    from diffsinger_amd.vocoder import Generator
    for tag, dim in (("k_eq_u", 9), ("harm0", 1), ("harm15", 16)):
        h = cc.config(tag)
        assert ov.harmonic_num_of(h) == dim - 1
        assert synth.nsf_hifigan_param_shapes(h)["m_source.l_linear.weight"] == (1, dim)
        gen = Generator(h)
        assert gen.harmonic_num == dim - 1 and tuple(gen.m_source.l_linear.weight.shape) == (1, dim)
        assert gen._config(0).harmonic_num == dim - 1
        i = cc.inputs(tag, 1, 12)
        assert i["rand_ini"].shape == (dim,) and i["noise"].shape[2] == dim
    # the default is the reference's 8 and the shapes of an existing config are what they were
    assert "harmonic_num" not in synth.NSF_HIFIGAN_DEFAULT
    assert synth.nsf_hifigan_param_shapes(dict(synth.NSF_HIFIGAN_DEFAULT))["m_source.l_linear.weight"] == (1, 9)
    # the harmonics are really there: the three sources differ
    hs = [ov.sine_source(cc.weights(t), cc.inputs(t, 1, 12)["f0"], 8, 44100, cc.inputs(t, 1, 12)["rand_ini"],
                         cc.inputs(t, 1, 12)["noise"], harmonic_num=n) for t, n in (("harm0", 0), ("k_eq_u", 8), ("harm15", 15))]
    assert not np.array_equal(hs[0], hs[1]) and not np.array_equal(hs[1], hs[2])


# ------------------------------------------------------------------------------------------------ the accepted space
def test_accepts_every_case():
    for tag in cc.ALL:
        assert cc.accepts(cc.config(tag)) == (True, ""), tag
    for over in cc.ACCEPT_EDGE:
        assert cc.accepts(cc.over_default(**over)) == (True, ""), over
    # the figures the cases are named for
    assert cc.gemm_tile_bytes(848, 3, 1) == 162816 and cc.gemm_tile_bytes(272, 9, 12) == 156672
    assert cc.gemm_tile_bytes(864, 3, 1) > cc.MAX_LDS >= cc.gemm_tile_bytes(352, 11, 5) and cc.gemm_tile_bytes(288, 9, 12) > cc.MAX_LDS
    assert [cc.up_taps(u, k) for u, k in ((4, 4), (2, 2), (8, 16), (2, 4), (2, 16), (3, 9), (5, 5), (5, 15), (2, 6), (2, 8), (2, 12))] == \
        [1, 1, 3, 3, 9, 3, 1, 3, 3, 5, 7]
    assert {cc.up_taps(u, k) for c in cc.CASES.values() for u, k in zip(c["over"]["upsample_rates"],
                                                                        c["over"]["upsample_kernel_sizes"])} == {1, 3, 5, 7, 9}
    assert cc.noise_groups(16, 64, 128) == 16 and ((16 * 16 - 1) * 64 + 128) * 4 == 65792      # noise_window: uncapped, 65 792 bytes
    assert cc.noise_groups(4, 64, 128) == 39 and ((39 * 16 - 1) * 64 + 128) * 4 <= cc.MAX_LDS < ((40 * 16 - 1) * 64 + 128) * 4
    assert cc.noise_groups(24, 8, 16) == 10 and cc.noise_groups(3, 1, 1) == 85                  # thin: 10 and 85 groups


@pytest.mark.parametrize("over,fragment", cc.REFUSE, ids=[str(sorted(o.items())) for o, _ in cc.REFUSE])
def test_accepts_and_create_refuse(over, fragment):
    """the mirror and the library give the same verdict with the same reason; nothing is written to *out"""
    from diffsinger_amd import _lib
    h = cc.over_default(**over)
    ok, reason = cc.accepts(h)
    assert not ok and fragment in reason, (ok, reason)
    out = C.c_void_p(_SENTINEL)
    rc = _lib.lib().dsd_vocoder_create(C.byref(cc.native_config(h)), C.byref(out))
    msg = _lib.lib().dsd_last_error(None).decode()
    assert rc == -1, f"rc = {rc}: {msg}"               # DSD_EINVAL
    assert out.value == _SENTINEL, "*out was written on a failed create"
    assert msg.startswith("dsd_vocoder_create: ") and fragment in msg and reason in msg, (fragment, reason, msg)


def test_create_accepts_what_the_mirror_accepts():
    """every case and every edge passes validation: with a GPU the handle is made, without one the error is the missing device"""
    import torch
    from diffsinger_amd import _lib
    lib = _lib.lib()
    for h in [cc.config(tag) for tag in cc.ALL] + [cc.over_default(**over) for over in cc.ACCEPT_EDGE]:
        out = C.c_void_p()
        rc = lib.dsd_vocoder_create(C.byref(cc.native_config(h)), C.byref(out))
        if torch.cuda.is_available():
            assert rc == 0, lib.dsd_last_error(None)
            lib.dsd_destroy(out)
        else:
            assert rc < 0 and b"no HIP device" in lib.dsd_last_error(None), (h, lib.dsd_last_error(None))


def test_oracle_agrees_that_an_odd_last_rate_cannot_run():
    """finding 3: rates [2, 3] - the reference's noise_convs.0 gives one frame too few and `x + x_source` raises; the oracle's
    shape check says so, for the float64 mode too, and a mini_nsf generator with the same rates runs"""
    from diffsinger_amd import synth
    h = cc.over_default(upsample_rates=[2, 3], upsample_kernel_sizes=[4, 3], upsample_initial_channel=64, num_mels=20)
    assert cc.accepts(h)[0] is False
    p = synth.synth_state_dict(synth.nsf_hifigan_param_shapes(h), seed=2830, gain=cc.GAIN)
    i = cc.make_inputs(h, 2, 37)
    for dt in (np.float32, np.float64):
        with pytest.raises(ValueError, match=r"noise_convs\.0 gives 73 frames for the stage's 74"):
            ov.generator_forward(p, h, i["mel"], i["f0"], i["rand_ini"], i["noise"], i["pre_noise"], dtype=dt)
    hm = dict(h, mini_nsf=True)
    assert cc.accepts(hm) == (True, "")
    pm = synth.synth_state_dict(synth.nsf_hifigan_param_shapes(hm), seed=2830, gain=cc.GAIN)
    assert ov.generator_forward(pm, hm, i["mel"], i["f0"]).shape == (2, 1, 37 * 6)


def test_split_bf16_layouts_within_the_margin():
    """tools/bf16x3_vocoder_tolerance.py on the two new layouts: the emulated split-bf16 arithmetic stays below 0.6 TOL of the
    fp32 oracle (the margin test_vocoder_x3_host.py documents), and the layouts reach what they are there for"""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import bf16x3_vocoder_tolerance as emu
    widths = {tag: [cc.config(tag)["upsample_initial_channel"] >> (i + 1) for i in range(3)] for tag in cc.X3}
    assert widths == {"x3_c384": [192, 96, 48], "x3_c320": [160, 80, 40]}
    assert emu.eligible(192, 192) and emu.eligible(96, 96) and emu.eligible(160, 160) and not emu.eligible(80, 80)
    for label, tag, inp, want in emu.config_cases():
        err = emu.rel(emu.emulate(tag, inp, cases=cc), want)
        print(f"{label}: split-bf16 emulation vs fp32 oracle {err:.3e} (cap {0.6 * cc.TOL:.0e})")
        assert 0.0 < err < 0.6 * cc.TOL, (label, err)
