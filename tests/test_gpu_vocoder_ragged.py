"""-m gpu: ragged vocoder batches (dsd_vocode_ragged, Generator.forward(lengths=...)).  Item b of a zero-padded batch must
come out as the same segment vocoded alone at T = lengths[b] with the same draws, for every G10 configuration shape (GEMM
path, tconv.hip, both source kinds, noise_sigma); the harness vocodes each group of a project in one such call."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from diffsinger_amd import synth  # noqa: E402
from gpu_util import dev  # noqa: E402
from oracle import vocoder as ov  # noqa: E402
from test_gpu_vocoder import GAIN, GOLDEN, OVER, TOL, build  # noqa: E402

SAME = 1e-5         # ragged vs alone with the same draws, relative to max(1, max|wav|)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"


def inputs(h, lens, t_len, seed):
    """A padded batch: item b's frames past lens[b] hold junk (not zeros), as a careless caller's buffer would."""
    bsz, upp, c0 = len(lens), int(np.prod(h["upsample_rates"])), h["upsample_initial_channel"]
    rng = np.random.Generator(np.random.PCG64(seed))
    mel = (synth.synth_normal((bsz, h["num_mels"], t_len), seed + 1) * 3.0 - 11.0).astype(np.float32)
    f0 = (150.0 * 2.0 ** rng.uniform(-1, 2, (bsz, t_len))).astype(np.float32)
    f0[:, ::7] = 0.0
    rand_ini = rng.random((bsz, 9)).astype(np.float32)
    noise = synth.synth_normal((bsz, t_len * upp, 9), seed + 2)
    pre = synth.synth_normal((bsz, c0, t_len), seed + 3)
    for b, n in enumerate(lens):            # junk past the end: must not reach the item's valid samples
        mel[b, :, n:] = 40.0
        f0[b, n:] = 3000.0
        noise[b, n * upp:] = 50.0
        pre[b, :, n:] = -50.0
    return mel, f0, rand_ini, noise, pre


def alone(gen, mel, f0, rand_ini, noise, pre, b, n, upp):
    with torch.no_grad():
        return gen(dev(mel[b:b + 1, :, :n]), dev(f0[b:b + 1, :n]), rand_ini=dev(rand_ini[b]),
                   noise=dev(noise[b:b + 1, :n * upp]), pre_noise=dev(pre[b:b + 1, :, :n]))[0, 0]


# lengths: full, one frame, a third, one short; then one frame before / on / after the 32- and 64-frame GEMM tile edges at
# the mel rate (on the small configurations every stage of tconv.hip also ends inside a 256-frame tile for most of them)
CASES = [(tag, 70, [70, 1, 23, 69, 31, 32, 33, 63, 64, 65]) for tag in sorted(OVER)] + [
    ("mini_small", 2100, [2100, 5, 2049, 2048]),         # the phase scan's 2048-frame pieces
    ("small_rb2", 130, [17, 130, 129, 100]),              # the longest item not first
]


@pytest.mark.parametrize("tag,t_len,lens", CASES)
def test_ragged_equals_alone(tag, t_len, lens):
    gen, h, params = build(OVER[tag], 430)
    upp = int(np.prod(h["upsample_rates"]))
    mel, f0, rand_ini, noise, pre = inputs(h, lens, t_len, 431)
    with torch.no_grad():
        got = gen(dev(mel), dev(f0), lengths=lens, rand_ini=dev(rand_ini), noise=dev(noise), pre_noise=dev(pre))
    assert tuple(got.shape) == (len(lens), 1, t_len * upp)
    for b, n in enumerate(lens):
        want = alone(gen, mel, f0, rand_ini, noise, pre, b, n, upp)
        scale = max(1.0, float(want.abs().max()))
        assert float((got[b, 0, :n * upp] - want).abs().max()) <= SAME * scale, (tag, b, n)
        assert not got[b, 0, n * upp:].any()                # zeroed past the item's end
        if t_len <= 130:
            ref = ov.generator_forward(params, h, mel[b:b + 1, :, :n], f0[b:b + 1, :n], rand_ini[b], noise[b:b + 1, :n * upp],
                                       pre[b:b + 1, :, :n])
            ref = torch.from_numpy(np.ascontiguousarray(ref.reshape(-1))).to(got.device)
            assert float((got[b, 0, :n * upp] - ref).abs().max()) / max(float(ref.abs().max()), 1e-6) < TOL, (tag, b, n)
    # the test is not empty: a dense batch of the same padded items is wrong near a short item's end
    b, n = 2, lens[2]
    with torch.no_grad():
        dense = gen(dev(mel[b:b + 1]), dev(f0[b:b + 1]), rand_ini=dev(rand_ini[b]), noise=dev(noise[b:b + 1]),
                    pre_noise=dev(pre[b:b + 1]))[0, 0, :n * upp]
    want = alone(gen, mel, f0, rand_ini, noise, pre, b, n, upp)
    assert float((dense - want).abs().max()) > 1e3 * SAME * max(1.0, float(want.abs().max()))
    gen.release_native()


@pytest.mark.parametrize("tag", ["default", "mini_small", "small_sigma", "mini_sigma"])
def test_ragged_device_draws_match_lone_calls(tag):
    """Draws made by forward(lengths=...): per item, in order, as lone calls make them - same waves, same RNG state."""
    gen, h, _ = build(OVER[tag], 440)
    upp = int(np.prod(h["upsample_rates"]))
    lens, t_len = [40, 7, 40, 33], 40
    mel, f0, _, _, _ = inputs(h, lens, t_len, 441)
    with torch.no_grad():
        torch.cuda.manual_seed(1234)
        got = gen(dev(mel), dev(f0), lengths=torch.tensor(lens))
        state_ragged = torch.cuda.get_rng_state()
        torch.cuda.manual_seed(1234)
        lone = [gen(dev(mel[b:b + 1, :, :n]), dev(f0[b:b + 1, :n]))[0, 0] for b, n in enumerate(lens)]
        state_lone = torch.cuda.get_rng_state()
    assert torch.equal(state_ragged, state_lone)
    for b, n in enumerate(lens):
        assert float((got[b, 0, :n * upp] - lone[b]).abs().max()) <= SAME * max(1.0, float(lone[b].abs().max())), (tag, b)
        assert not got[b, 0, n * upp:].any()
    gen.release_native()


def test_ragged_errors():
    from diffsinger_amd import _lib
    gen, h, _ = build(OVER["small_rb2"], 450)
    x = torch.zeros(2, 32, 4).cuda()
    f = torch.zeros(2, 4).cuda()
    ri = torch.zeros(2, 9).cuda()
    nz = torch.zeros(2, 64, 9).cuda()
    o = torch.zeros(2, 64).cuda()
    hd = gen.native_handle(x.device)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def call(lens, rand_ini=ri, noise=nz):
        lc = (C.c_int32 * 2)(*lens)
        _lib.check(hd, _lib.lib().dsd_vocode_ragged(hd, p(x), 2, 4, 128, 4, 1, lc, p(f), rand_ini if rand_ini is None else p(rand_ini),
                                                    noise if noise is None else p(noise), None, p(o), None), "dsd_vocode_ragged")
    call([4, 2])
    with pytest.raises(RuntimeError, match=r"lengths\[1\] = 0"):
        call([4, 0])
    with pytest.raises(RuntimeError, match=r"lengths\[0\] = 5"):
        call([5, 2])
    with pytest.raises(RuntimeError, match="rand_ini and noise are required"):
        call([4, 2], rand_ini=None)
    with torch.no_grad():
        with pytest.raises(ValueError, match="lengths"):
            gen(x, f, lengths=[4, 5])
    # dsd_set_lengths keeps rejecting vocoder handles
    assert _lib.lib().dsd_set_lengths(hd, (C.c_int32 * 2)(4, 2), 2, None) != 0
    gen.release_native()


def _project_harness():
    from diffsinger_amd import harness
    from diffsinger_amd.hparams import hparams
    from diffsinger_amd.toplevel import DiffSingerAcoustic
    from diffsinger_amd.vocoder import Generator, NsfHifiGAN
    hparams.clear()
    hparams.update(hop_size=512, audio_sample_rate=44100, hidden_size=256, enc_layers=2, enc_ffn_kernel_size=3, ffn_act="gelu",
                   dropout=0.1, num_heads=2, use_pos_embed=True, rel_pos=True, use_rope=True, use_spk_id=True, num_spk=3,
                   use_lang_id=False, num_lang=1, use_energy_embed=True, use_key_shift_embed=True, use_speed_embed=True,
                   augmentation_args=dict(random_pitch_shifting=dict(range=[-5.0, 5.0]),
                                          random_time_stretching=dict(range=[0.5, 2.0])),
                   schedule_type="linear", use_shallow_diffusion=True, diffusion_type="reflow", T_start=0.4, T_start_infer=0.4,
                   time_scale_factor=1000, sampling_algorithm="euler", sampling_steps=8, timesteps=1000, K_step=400,
                   K_step_infer=400, backbone_type="wavenet",
                   backbone_args=dict(num_layers=2, num_channels=64, dilation_cycle_length=2), spec_min=[-12.0], spec_max=[0.0],
                   shallow_diffusion_args=dict(aux_decoder_arch="convnext", val_gt_start=False,
                                               aux_decoder_args=dict(num_channels=64, num_layers=2, kernel_size=7)))
    table = harness.SimplePhonemeTable(["a", "b", "c", "d", "e"])
    model = DiffSingerAcoustic(len(table), 128)
    sd = dict(model.state_dict())
    sd.update({"fs2." + k: torch.from_numpy(v) for k, v in synth.synth_state_dict(synth.fs2_acoustic_param_shapes(
        len(table), enc_layers=2, num_spk=3, variances=("energy",), key_shift=True, speed=True), seed=500).items()})
    sd.update({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(synth.convnext_param_shapes(
        256, 128, num_channels=64, num_layers=2, prefix="aux_decoder.decoder."), seed=501).items()})
    sd.update({"diffusion.velocity_fn." + k: torch.from_numpy(v) for k, v in synth.synth_state_dict(
        synth.backbone_param_shapes("wavenet", 128, 1, hidden_size=256, num_layers=2, num_channels=64,
                                    dilation_cycle_length=2), seed=502).items()})
    model.load_state_dict(sd, strict=True)
    vh = dict(synth.NSF_HIFIGAN_DEFAULT, upsample_initial_channel=64, noise_sigma=0.1)
    gen = Generator(vh)
    gen.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(
        synth.nsf_hifigan_param_shapes(vh), seed=503, gain=GAIN).items()}, strict=True)
    return harness.AcousticHarness(model.cuda().eval(), NsfHifiGAN(gen.cuda().eval()), table,
                                   spk_map={"alice": 0, "bob": 1, "carol": 2}, device="cuda")


def test_project_in_one_ragged_vocoder_call():
    from diffsinger_amd import harness
    from diffsinger_amd.hparams import hparams
    saved = dict(hparams)
    try:
        h = _project_harness()
        segs = harness.load_ds(os.path.join(GOLDEN, "g11_segments.ds"))
        track = h.run_inference(segs)
        calls = []
        real = h.run_vocoder_batch
        h.run_vocoder_batch = lambda *a: calls.append(len(a[0])) or real(*a)
        batched = h.run_inference(segs, batch_size=len(segs))
        h.run_vocoder_batch = real
        assert calls == [len(segs)]                              # the whole project: one ragged vocoder call
        # the existing harness test's bounds (the acoustic model's padded batch rounds differently, see test_gpu_vocoder)
        assert batched.shape == track.shape and np.abs(batched - track).max() < 2e-2 and \
            np.abs(batched - track).mean() < 1e-3
        # the vocoder part alone: the same mels and draws in, one ragged call vs one call per segment
        mels = h.run_inference(segs, save_mel=True)
        gen = h.vocoder.model
        batches = [h.preprocess_input(s, idx=i) for i, s in enumerate(segs)]
        draws = []
        for s, b in zip(segs, batches):
            h._draw_noise(s, -1, int(b["mel2ph"].size(1)))
            draws.append(gen.draw(int(b["mel2ph"].size(1)), h.device))
        mel_d = [m["mel"].cuda() for m in mels]
        got = h.run_vocoder_batch(mel_d, [b["f0"] for b in batches], draws)
        for m, b, d, g in zip(mel_d, batches, draws, got):
            want = h.run_vocoder(m, f0=b["f0"], rand_ini=d[0], noise=d[1], pre_noise=d[2])[0]
            assert g.shape == want.shape
            assert float((g - want).abs().max()) <= SAME * float(want.abs().max())
    finally:
        hparams.clear()
        hparams.update(saved)
