#!/usr/bin/env python3
"""Timing of the pitch pre-process stage: `DiffSingerVarianceDeploy.forward_pitch_preprocess` at
B = 1, T = 1000 (no melody encoder, so the stage is the duration-to-frame work and one assembly) against the same stage
written with the torch ops the `.ds` harness uses for it today on the same GPU - the searchsorted length regulator (which reads
the frame total back), gather, replicate pad + conv1d, the retake blend, embedding lookups and broadcast adds.  Both are expected to be bound by
launches, not by arithmetic.  Device-event times, warm-up, median of several repeats; GPU box only.  Prints one JSON line;
`--out FILE` also writes it there.

`--variance`: instead, every non-sampler stage of the variance twin at the sizes of a configs/variance.yaml segment (hidden
256, 120 tokens, 60 notes, `--frames` frames, B = 1 and 8), the Python twin's stage (`deploy.DiffSingerVarianceDeploy`) and
the C stage (`dsd_variance_*` through `cvariance.Variance`, on a model file packed from the same weights) in this one process
on the same inputs.  Per stage and batch size: device-event time of one call, and the host time one
call takes to issue (wall clock over back-to-back calls, the device drained before and after).  One JSON line.

`--acoustic`: the same for the acoustic twin at the sizes of a configs/acoustic.yaml segment (hidden
256, 128 mel bins, 120 tokens, `--frames` frames, B = 1 and 8, shallow DDPM with every embedding): `condition`
(forward_fs2_aux against dsd_acoustic_condition), `start` (the twin's norm_spec + q_sample against dsd_acoustic_start) and
`sample` (forward_shallow_diffusion at depth 0.4 in 10 steps against dsd_acoustic_sample), `deploy.DiffSingerAcousticDeploy`
against `cacoustic.Acoustic` on a model file packed from the same weights, in this one process."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import deploy_cases as dc  # noqa: E402
from diffsinger_amd import deploy  # noqa: E402
from diffsinger_amd.harness import length_regulator  # noqa: E402
from diffsinger_amd.hparams import hparams  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=50)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--frames", type=int, default=1000)
ap.add_argument("--out")
ap.add_argument("--variance", action="store_true")
ap.add_argument("--acoustic", action="store_true")
args = ap.parse_args()
assert torch.cuda.is_available(), "time_stages.py needs the MI355X"


def timed(fn):
    for _ in range(args.warmup):
        fn()
    times = []
    for _ in range(args.repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def host_ms(fn, calls=20):
    """wall-clock time to issue one call: `calls` back-to-back, the device idle before the first and drained after the last"""
    import time
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return (t1 - t0) / calls * 1e3


def variance_stages():
    import tempfile
    from diffsinger_amd import cvariance, modelfile
    hp = dict(dc.BASE_HP)
    hp.update(dc.VARIANCE_HP, hidden_size=256, enc_layers=4, predict_dur=True, predict_pitch=True, use_melody_encoder=True,
              use_glide_embed=True, predict_energy=True, predict_breathiness=True, use_spk_id=True, num_spk=4, use_lang_id=True,
              num_lang=2, diffusion_type="reflow", melody_encoder_args=dict(hidden_size=128, enc_layers=4),
              dur_prediction_args=dict(dc.VARIANCE_HP["dur_prediction_args"], hidden_size=512, num_layers=5),
              pitch_prediction_args=dict(dc.VARIANCE_HP["pitch_prediction_args"], repeat_bins=64),
              variances_prediction_args=dict(dc.VARIANCE_HP["variances_prediction_args"], total_repeat_bins=48))
    hparams.clear()
    hparams.update(hp, infer=True)
    vocab, n_ph, n_word, n_note, t_len, h = 60, 120, 40, 60, args.frames, 256
    torch.manual_seed(2450)
    model = deploy.DiffSingerVarianceDeploy(vocab, cross_lingual_token_idx=list(range(2, vocab, 3))).cuda().eval()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "variance.dsdm")
        modelfile.write(path, modelfile.variance_sections("var", model))
        with modelfile.open(path) as f:
            v = cvariance.Variance(f, "var", "cuda")
    rng = np.random.default_rng(2451)
    names = v.names
    res = {"T": t_len, "tokens": n_ph, "words": n_word, "notes": n_note, "hidden": h, "K": int(v.cfg.smooth_width), "stages": {}}
    for bsz in (1, 8):
        def ints(lo, hi, shape):
            return torch.from_numpy(rng.integers(lo, hi, shape).astype(np.int64)).cuda()

        def split(total, parts):
            return torch.from_numpy(np.stack([rng.multinomial(total, np.ones(parts) / parts) for _ in range(bsz)])).cuda()
        tokens, languages, ph_midi = ints(1, vocab, (bsz, n_ph)), ints(1, 3, (bsz, n_ph)), ints(40, 80, (bsz, n_ph))
        word_div, ph_dur, note_dur = split(n_ph, n_word), split(t_len, n_ph), split(t_len, n_note)
        word_dur = ints(10, 40, (bsz, n_word))
        note_midi = torch.from_numpy(rng.uniform(48, 72, (bsz, n_note)).astype(np.float32)).cuda()
        note_rest, note_glide = torch.rand(bsz, n_note, device="cuda") < 0.2, ints(0, 3, (bsz, n_note))
        pitch = torch.from_numpy((60 + rng.normal(0, 3, (bsz, t_len))).astype(np.float32)).cuda()
        expr, retake = torch.rand(bsz, t_len, device="cuda"), torch.rand(bsz, t_len, device="cuda") < 0.5
        spk = torch.randn(bsz, 1, h, device="cuda")
        curves = {n: torch.from_numpy(rng.uniform(-60, -10, (bsz, t_len)).astype(np.float32)).cuda() for n in names}
        var_retake = torch.rand(bsz, t_len, len(names), device="cuda") < 0.5
        raw_pitch = torch.randn(bsz, t_len, v.cfg.pitch_repeat_bins, device="cuda")
        raw_var = torch.randn(bsz, len(names), t_len, v.cfg.var_repeat_bins, device="cuda") * 30 - 40
        enc, masks = v.encode(tokens, word_div=word_div, word_dur=word_dur, languages=languages)
        _, base = v.pitch_cond(enc, ph_dur, note_midi, note_rest, note_dur, note_glide=note_glide, pitch=pitch, expr=expr, retake=retake,
                               spk_embed=spk)
        note = dict(note_midi=note_midi, note_rest=note_rest, note_dur=note_dur, note_glide=note_glide, pitch=pitch, expr=expr,
                    retake=retake, spk_embed=spk)
        pairs = {
            "encode": (lambda: model.forward_linguistic_encoder_word(tokens, word_div, word_dur, languages=languages),
                       lambda: v.encode(tokens, word_div=word_div, word_dur=word_dur, languages=languages)),
            "dur": (lambda: model.forward_dur_predictor(enc, masks, ph_midi, spk_embed=spk), lambda: v.dur(enc, masks, ph_midi, spk_embed=spk)),
            "pitch_cond": (lambda: model.forward_pitch_preprocess(enc, ph_dur, **note), lambda: v.pitch_cond(enc, ph_dur, **note)),
            "cond": (lambda: model.forward_variance_preprocess(enc, ph_dur, pitch, variances=curves, retake=var_retake, spk_embed=spk),
                     lambda: v.cond(enc, ph_dur, pitch, curves, var_retake, spk_embed=spk)),
            "pitch_post": (lambda: model.forward_pitch_postprocess(raw_pitch.mean(-1), base), lambda: v.pitch_post(raw_pitch, base)),
            "post": (lambda: model.forward_variance_postprocess(raw_var.mean(-1)), lambda: v.post(raw_var)),
        }
        for stage, (twin, c_call) in pairs.items():
            res["stages"][f"{stage}_b{bsz}"] = {"python_device_ms": timed(twin), "c_device_ms": timed(c_call),
                                                "python_host_ms": host_ms(twin), "c_host_ms": host_ms(c_call)}
    v.close()
    return res


def acoustic_stages():
    import tempfile
    from diffsinger_amd import _lib, cacoustic, modelfile
    from diffsinger_amd.diffusion import _to_bfmt
    graph_flags = _lib.DSD_SAMPLE_GRAPH | _lib.DSD_SAMPLE_GRAPH_LAZY
    vocab, n_ph, t_len, h, m = 60, 120, args.frames, 256, 128
    hp = dict(dc.BASE_HP)
    hp.update(dc.ACOUSTIC_HP, hidden_size=256, enc_layers=4, use_shallow_diffusion=True, diffusion_type="ddpm", K_step=400,
              use_key_shift_embed=True, use_speed_embed=True, use_energy_embed=True, use_breathiness_embed=True, use_spk_id=True,
              num_spk=4, use_lang_id=True, num_lang=2, spec_min=[-12.0], spec_max=[0.0],
              backbone_args=dict(num_layers=20, num_channels=256, dilation_cycle_length=4),
              shallow_diffusion_args=dict(dc.ACOUSTIC_HP["shallow_diffusion_args"],
                                          aux_decoder_args=dict(num_channels=512, num_layers=6, kernel_size=7, dropout_rate=0.1)))
    hparams.clear()
    hparams.update(hp, infer=True)
    torch.manual_seed(2460)
    model = deploy.DiffSingerAcousticDeploy(vocab, m, cross_lingual_token_idx=list(range(2, vocab, 3))).cuda().eval()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "acoustic.dsdm")
        modelfile.write(path, modelfile.acoustic_sections("ac", model))
        with modelfile.open(path) as f:
            a = cacoustic.Acoustic(f, "ac", "cuda")
    rng = np.random.default_rng(2461)
    depth, steps = 0.4, 10
    plan = a.plan(depth, steps)
    res = {"T": t_len, "tokens": n_ph, "hidden": h, "mel_bins": m, "depth": depth, "steps": steps, "t_max": int(plan.t_max),
           "speedup": int(plan.speedup), "stages": {}}
    diff = model.diffusion
    k, mid = (diff.spec_max - diff.spec_min) / 2., (diff.spec_max + diff.spec_min) / 2.
    for bsz in (1, 8):
        def f32(lo, hi, shape):
            return torch.from_numpy(rng.uniform(lo, hi, shape).astype(np.float32)).cuda()
        tokens = torch.from_numpy(rng.integers(1, vocab, (bsz, n_ph)).astype(np.int64)).cuda()
        languages = torch.from_numpy(rng.integers(1, 3, (bsz, n_ph)).astype(np.int64)).cuda()
        durations = torch.from_numpy(np.stack([rng.multinomial(t_len, np.ones(n_ph) / n_ph) for _ in range(bsz)])).cuda()
        f0 = f32(110, 440, (bsz, t_len))
        curves = dict(energy=f32(-60, -10, (bsz, t_len)), breathiness=f32(-60, -10, (bsz, t_len)))
        kw = dict(gender=f32(-1.2, 1.2, (bsz, t_len)), velocity=f32(0.4, 2.2, (bsz, t_len)), spk_embed=torch.randn(bsz, 1, h, device="cuda"),
                  languages=languages)
        noise = torch.randn(bsz, 1, m, t_len, device="cuda")
        cond, aux = a.condition(tokens, durations, f0, curves, **kw)
        x = a.start(plan, source=aux, noise=noise)
        depth_t = torch.tensor(depth, dtype=torch.float32)
        pairs = {
            "condition": (lambda: model.forward_fs2_aux(tokens, durations, f0, curves, **kw), lambda: a.condition(tokens, durations, f0, curves, **kw)),
            "start": (lambda: diff._start_state(plan.t_max, _to_bfmt((aux - mid) / k, 1), noise, bsz, aux.device),
                      lambda: a.start(plan, source=aux, noise=noise)),
            "sample": (lambda: model.forward_shallow_diffusion(cond, aux, depth_t, steps, noise=noise), lambda: a.sample(plan, cond, x, flags=graph_flags)),     # the twin's own graph policy ("lazy")
        }
        for stage, (twin, c_call) in pairs.items():
            res["stages"][f"{stage}_b{bsz}"] = {"python_device_ms": timed(twin), "c_device_ms": timed(c_call),
                                                "python_host_ms": host_ms(twin), "c_host_ms": host_ms(c_call)}
    a.close()
    return res


if args.variance or args.acoustic:
    with torch.no_grad():
        line = json.dumps(variance_stages() if args.variance else acoustic_stages())
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    sys.exit(0)

hp = dict(dc.BASE_HP)
hp.update(dc.VARIANCE_HP, hidden_size=256, predict_pitch=True, diffusion_type="reflow")
hparams.clear()
hparams.update(hp, infer=True)
model = deploy.DiffSingerVarianceDeploy(40).cuda().eval()
model.build_smooth_op()
rng = np.random.default_rng(2295)
t_len, n_ph, n_note, h = args.frames, 60, 40, 256
ph_dur = torch.from_numpy(rng.multinomial(t_len, np.ones(n_ph) / n_ph)[None]).cuda()
note_dur = torch.from_numpy(rng.multinomial(t_len, np.ones(n_note) / n_note)[None]).cuda()
note_midi = torch.from_numpy(rng.uniform(48, 72, (1, n_note)).astype(np.float32)).cuda()
enc = torch.randn(1, n_ph, h, device="cuda")
pitch = torch.from_numpy((60 + rng.normal(0, 3, (1, t_len))).astype(np.float32)).cuda()
expr = torch.rand(1, t_len, device="cuda")
retake = torch.zeros(1, t_len, dtype=torch.bool, device="cuda")
retake[:, t_len // 3: 2 * t_len // 3] = True
taps = model.smooth[1].cuda()


def staged():
    return model.forward_pitch_preprocess(enc, ph_dur, note_midi=note_midi, note_dur=note_dur, pitch=pitch, expr=expr, retake=retake)


def torch_ops():
    mel2ph, mel2note = length_regulator(ph_dur), length_regulator(note_dur)
    cond = torch.gather(F.pad(enc, [0, 0, 1, 0]), 1, mel2ph[..., None].expand(-1, -1, h))
    e = (expr * retake)[:, :, None]
    cond = cond + e * model.pitch_retake_embed.weight[1] + (1. - e) * model.pitch_retake_embed.weight[0]
    frame_midi = torch.gather(F.pad(note_midi, [1, 0]), 1, mel2note)
    k = taps.numel()
    left = (k - 1) // 2
    base = F.conv1d(F.pad(frame_midi[:, None, :], [left, k - 1 - left], mode='replicate'), taps[None, None])[:, 0]
    base = base * retake + pitch * ~retake
    return cond + model.base_pitch_embed(base[:, :, None]), base


with torch.no_grad():
    a, b = staged(), torch_ops()
    res = {"B": 1, "T": t_len, "tokens": n_ph, "notes": n_note, "K": int(taps.numel()),
           "cond_max_abs_diff": float((a[0] - b[0]).abs().max()), "base_max_abs_diff": float((a[1] - b[1]).abs().max()),
           "staged_ms": timed(staged), "torch_ops_ms": timed(torch_ops),
           "length_regulate_ms": timed(lambda: deploy.length_regulate(ph_dur, t_len)),
           "torch_length_regulator_ms": timed(lambda: length_regulator(ph_dur)),
           "frame_curve_ms": timed(lambda: deploy.frame_curve(note_midi, deploy.length_regulate(note_dur, t_len), pitch, retake,
                                                              model.smooth[1]))}
line = json.dumps(res)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
