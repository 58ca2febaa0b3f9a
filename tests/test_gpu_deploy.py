"""-m gpu parity of the staged deployment entry points (diffsinger_amd/deploy.py on dsd_length_regulate /
dsd_frame_curve and the existing encoders, assembler and samplers) against G22, the reference's own deployment twins run
stage by stage on the CPU (tests/golden/make_golden_deploy.py), on the cases of tests/deploy_cases.py.

Tolerances.  Integer outputs are exact.  Encoder outputs, conditions, durations and sampler outputs are held to what
tests/test_gpu_variance.py applies to the same quantities (it states them inline, so they are named here with their
lines) and tests/test_gpu_encoder.py's TOL for the acoustic condition.  The smoothed base pitch has a bar of its own:
the reference's fp32 Conv1d sits within SMOOTH_FLOOR = 1.06e-5 semitones of an fp64 restatement with the same taps (max over
the pitch cases: 6.1e-6 at K = 5, 1.05e-5 at K = 21, 3.0e-6 at K = 4; make_golden_deploy.py prints them), and the kernel
must stay within twice that of the reference.  Every figure is printed before it is asserted."""
import os

import numpy as np
import pytest
import torch

import deploy_cases as dc
import variance_cases as vc
from diffsinger_amd import synth
from diffsinger_amd.hparams import hparams
from gpu_util import dev, rel_err
from test_gpu_encoder import TOL as ACOUSTIC_COND_TOL

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g22_deploy.npz")
ENC_TOL = 2e-4          # of max |want|: encoder outputs and conditions (test_gpu_variance.py:116,130)
DUR_TOL = 5e-5          # of max(1, max |want|): predicted durations vs the reference (test_gpu_variance.py:70)
SAMPLE_TOL = 2e-4       # of max(1, max |want|): a full sampler run with x_T passed in (test_gpu_variance.py:76,82)
ALONE_TOL = 5e-5        # of max(1, max |want|): batch against alone (test_gpu_variance.py:328)
AUX_TOL = 2e-5          # of max |want|: the aux decoder's mel behind the acoustic encoder (test_gpu_encoder.py:221)
SMOOTH_FLOOR = 1.06e-5
SMOOTH_BAR = 2 * SMOOTH_FLOOR


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    yield
    hparams.clear()
    hparams.update(hidden_size=256)


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


def release(model):
    for m in model.modules():
        if hasattr(m, "release_native"):
            m.release_native()


def load(model, seed):
    shapes = dc.sorted_param_shapes(model.named_parameters())
    res = model.load_state_dict({k: torch.from_numpy(v) for k, v in dc.synth_weights(shapes, seed).items()}, strict=False)
    assert not res.unexpected_keys and not set(res.missing_keys) & set(shapes)
    return model.cuda().eval()


def close(got, want, tol, floor_one, what):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = float(np.abs(got - want).max())
    ref = float(np.abs(want).max())
    bound = tol * (max(1.0, ref) if floor_one else ref)
    print(f"{what}: max |err| {err:.3e}, bound {bound:.3e} ({err / max(ref, 1e-30):.2e} of max |want| {ref:.3f})")
    assert err <= bound, (what, err, bound)


# ------------------------------------------------------------------------------------------------ dsd_length_regulate
@pytest.mark.parametrize("tag", list(dc.LR_CASES))
def test_length_regulator_vs_golden(g, tag):
    from diffsinger_amd.deploy import length_regulate
    dur, want = dc.lr_durations(tag), g[f"lr_{tag}"]
    assert np.array_equal(length_regulate(dev(dur)).cpu().numpy(), want)                      # the reference's own T
    assert np.array_equal(length_regulate(dev(dur), want.shape[1]).cpu().numpy(), want)       # the caller's T
    longer = length_regulate(dev(dur), want.shape[1] + 300).cpu().numpy()                     # frames past the total: 0
    assert np.array_equal(longer[:, :want.shape[1]], want) and not longer[:, want.shape[1]:].any()


def test_length_regulator_random_rows_vs_numpy():
    """A few hundred seeded rows against the numpy restatement: many zero durations, T below, at and above the totals,
    one lane per token up to eight tokens per lane."""
    from diffsinger_amd.deploy import length_regulate
    rng = np.random.Generator(np.random.PCG64(2290))
    for n_tok, hi, rows in ((1, 9, 16), (37, 6, 120), (256, 4, 60), (257, 4, 60), (1000, 3, 40), (2048, 3, 8)):
        dur = rng.integers(0, hi, (rows, n_tok)).astype(np.int64)
        dur[rng.random(dur.shape) < 0.3] = 0
        dur[0] = 0                                                      # an item with no frames at all
        totals = dur.sum(1)
        for t_len in sorted({1, max(1, int(np.median(totals))), int(totals.max()), int(totals.max()) + 257}):
            got = length_regulate(dev(dur), t_len).cpu().numpy()
            assert np.array_equal(got, dc.length_regulate_numpy(dur, t_len)), (n_tok, t_len)


def test_length_regulator_ragged_items_equal_their_lone_runs(g):
    from diffsinger_amd.deploy import length_regulate
    dur = dc.lr_durations("ragged3")
    batch = length_regulate(dev(dur)).cpu().numpy()
    assert np.array_equal(batch, g["lr_ragged3"])
    for b in range(3):
        alone = length_regulate(dev(dur[b:b + 1])).cpu().numpy()
        assert alone.shape[1] == dur[b].sum()
        assert np.array_equal(batch[b:b + 1, :alone.shape[1]], alone) and not batch[b, alone.shape[1]:].any()


# ------------------------------------------------------------------------------------------------ dsd_frame_curve
def _curve_reference(note_midi, mel2note, pitch, retake, taps, length):
    """toplevel.py:251-258 for one item cut to its own length, restated in fp64 with the given fp32 taps (the padding rule
    itself - (K - 1) // 2 in front - is torch's, which the K = 4 case of G22 pins)."""
    k = len(taps)
    left = (k - 1) // 2
    frame = np.pad(note_midi.astype(np.float64), (1, 0))[mel2note[:length]]
    x = np.pad(frame, (left, k - 1 - left), mode="edge")
    base = np.array([np.dot(taps.astype(np.float64), x[t:t + k]) for t in range(length)])
    p, r = pitch[:length].astype(np.float64), retake[:length]
    return base, base * r + p * ~r, (p - base) * ~r


@pytest.mark.parametrize("k", [1, 2, 4, 5, 21, 255])
def test_frame_curve_vs_torch_and_ragged_items_bit_equal_alone(k):
    """Three items of 700 / 300 / 2 frames (more than one 256-frame block, a block edge inside the taps' reach, a clip
    shorter than any K > 2) against an fp64 restatement, and each item of the batch bit for bit against its lone run.  The
    kernel sums in fp64 and rounds once, so it sits within half an ulp of the curve (3.8e-6 at 64 <= v < 128) of the fp64
    value: inside SMOOTH_BAR at every K, which is why this test may hold the wide K = 255 to the bar of the narrow ones."""
    from diffsinger_amd.deploy import frame_curve, smooth_kernel
    rng = np.random.Generator(np.random.PCG64(2280 + k))
    lens, t_len, n_note = [700, 300, 2], 700, 9
    note_midi = torch.from_numpy(rng.uniform(40, 80, (3, n_note)).astype(np.float32))
    mel2note = torch.zeros((3, t_len), dtype=torch.int64)
    for b, n in enumerate(lens):
        mel2note[b, :n] = torch.from_numpy(np.sort(rng.integers(0 if b == 0 else 1, n_note + 1, n)))     # item 0: index 0 too
    pitch = torch.from_numpy(rng.uniform(40, 80, (3, t_len)).astype(np.float32))
    retake = torch.from_numpy(rng.random((3, t_len)) < 0.5)
    taps = smooth_kernel(k) if k > 1 else torch.ones(1)                # the reference's own K = 1 tap is NaN (G22 covers it)
    got = [x.cpu() for x in frame_curve(note_midi.cuda(), mel2note.cuda(), pitch.cuda(), retake.cuda(), taps, lens)]
    worst = 0.0
    for b, n in enumerate(lens):
        want = _curve_reference(note_midi[b].numpy(), mel2note[b].numpy(), pitch[b].numpy(), retake[b].numpy(), taps.numpy(), n)
        alone = frame_curve(note_midi[b:b + 1].cuda(), mel2note[b:b + 1, :n].cuda(), pitch[b:b + 1, :n].cuda(),
                            retake[b:b + 1, :n].cuda(), taps)
        for x, w, a in zip(got, want, alone):
            assert torch.equal(x[b:b + 1, :n], a.cpu())
            assert not x[b, n:].any()
            worst = max(worst, float(np.abs(x[b, :n].numpy() - w).max()))
    print(f"K = {k}: max |err| vs fp64 {worst:.3e}, bar {SMOOTH_BAR:.3e}")
    assert worst <= SMOOTH_BAR


# ------------------------------------------------------------------------------------------------ variance twin
def build_variance(tag):
    from diffsinger_amd.deploy import DiffSingerVarianceDeploy
    c = dc.VAR_CASES[tag]
    hp = dc.variance_hparams(tag)
    hparams.clear()
    hparams.update(hp, infer=True)
    return load(DiffSingerVarianceDeploy(dc.VOCAB, cross_lingual_token_idx=c.get("cross")), c["seed"] + 1), hp, c


@pytest.mark.parametrize("tag", list(dc.VAR_CASES))
def test_variance_stages_vs_golden(g, tag):
    model, hp, c = build_variance(tag)
    inp = {k: dev(v) for k, v in dc.variance_inputs(tag).items()}
    noise = {k: dev(synth.synth_normal(s, c["seed"] + 2 + i)) for i, (k, s) in enumerate(dc.variance_noise_shapes(tag).items())}
    with torch.no_grad():
        if hp["predict_dur"]:
            enc, x_masks = model.forward_linguistic_encoder_word(inp["tokens"], inp["word_div"], inp["word_dur"],
                                                                 languages=inp.get("languages"))
            from diffsinger_amd.deploy import length_regulate
            assert np.array_equal(length_regulate(inp["word_div"], c["n_ph"]).cpu().numpy(), g[f"{tag}_ph2word"])
            dur = model.forward_dur_predictor(enc, x_masks, inp["ph_midi"], spk_embed=inp.get("spk_embed"))
            close(dur, g[f"{tag}_dur_pred"], DUR_TOL, True, "dur_pred")
        else:
            enc, x_masks = model.forward_linguistic_encoder_phoneme(inp["tokens"], inp["ph_dur"], languages=inp.get("languages"))
        assert np.array_equal(x_masks.cpu().numpy(), g[f"{tag}_x_masks"])
        close(enc, g[f"{tag}_enc"], ENC_TOL, False, "encoder_out")
        from diffsinger_amd.deploy import length_regulate
        assert np.array_equal(length_regulate(inp["ph_dur"], c["t_len"]).cpu().numpy(), g[f"{tag}_mel2ph"])
        if hp["predict_pitch"]:
            assert np.array_equal(length_regulate(inp["note_dur"], c["t_len"]).cpu().numpy(), g[f"{tag}_mel2note"])
            assert np.array_equal(model.forward_mel2x_gather(inp["note_midi"], inp["note_dur"]).cpu().numpy(),
                                  np.pad(dc.variance_inputs(tag)["note_midi"], [(0, 0), (1, 0)])[0][g[f"{tag}_mel2note"]])
            cond, base = model.forward_pitch_preprocess(
                enc, inp["ph_dur"], note_midi=inp["note_midi"], note_rest=inp["note_rest"], note_dur=inp["note_dur"],
                note_glide=inp.get("note_glide"), pitch=inp["pitch"], expr=inp.get("expr"), retake=inp["retake"],
                spk_embed=inp.get("spk_embed"))
            want = g[f"{tag}_base_pitch"]
            if dc.smooth_width(hp) == 1:        # the reference's operator is 0 / 0: NaN everywhere, and so is this one
                assert np.isnan(want).all() and torch.isnan(base).all() and tuple(base.shape) == want.shape
            else:
                err = float(np.abs(base.cpu().numpy() - want).max())
                print(f"base_pitch (K = {dc.smooth_width(hp)}): max |err| {err:.3e}, bar {SMOOTH_BAR:.3e}")
                assert err <= SMOOTH_BAR
                close(cond, g[f"{tag}_pitch_cond"], ENC_TOL, False, "pitch_cond")
            if c["steps"]:
                # the sampler stage on the reference's own condition: the stage under test, not the chain before it
                x_pred = model.forward_pitch_reflow(dev(g[f"{tag}_pitch_cond"]), steps=c["steps"], noise=noise["pitch"])
                close(x_pred, g[f"{tag}_x_pred"], SAMPLE_TOL, True, "x_pred")
                close(model.forward_pitch_postprocess(x_pred, dev(want)), g[f"{tag}_pitch_pred"], SAMPLE_TOL, True, "pitch_pred")
                chained = model.forward_pitch_reflow(cond, steps=c["steps"], noise=noise["pitch"])
                close(chained, g[f"{tag}_x_pred"], SAMPLE_TOL, True, "x_pred, chained")
        names = dc.variance_names(hp)
        if names:
            cond = model.forward_variance_preprocess(enc, inp["ph_dur"], inp["pitch"], variances={n: inp["var_" + n] for n in names},
                                                     retake=inp["var_retake"], spk_embed=inp.get("spk_embed"))
            close(cond, g[f"{tag}_var_cond"], ENC_TOL, False, "variance_cond")
            xs_pred = model.forward_variance_reflow(cond, steps=c["steps"], noise=noise["variance"])
            close(xs_pred, g[f"{tag}_xs_pred"], SAMPLE_TOL, True, "xs_pred")
            outs = model.forward_variance_postprocess(xs_pred)
            assert len(outs) == len(names)
            for n, v in zip(names, outs):
                close(v, g[f"{tag}_out_{n}"], SAMPLE_TOL, True, n)
    release(model)


def test_delta_pitch_of_the_melody_form_vs_golden(g):
    """With a melody encoder the twin embeds (pitch - base) * ~retake and returns the smoothed base itself: the kernel's third
    output against the same expression on the fixture's base pitch."""
    from diffsinger_amd.deploy import frame_curve, length_regulate, smooth_kernel
    for tag in ("word_melody", "melody_even", "short_clip"):
        hp, inp = dc.variance_hparams(tag), dc.variance_inputs(tag)
        mel2note = length_regulate(dev(inp["note_dur"]), inp["retake"].shape[1])
        base, _, delta = frame_curve(dev(inp["note_midi"]), mel2note, dev(inp["pitch"]), dev(inp["retake"]),
                                     smooth_kernel(dc.smooth_width(hp)))
        want = (inp["pitch"] - g[f"{tag}_base_pitch"]) * ~inp["retake"]
        err = max(float(np.abs(delta.cpu().numpy() - want).max()), float(np.abs(base.cpu().numpy() - g[f"{tag}_base_pitch"]).max()))
        print(f"{tag}: delta / base max |err| {err:.3e}, bar {SMOOTH_BAR:.3e}")
        assert err <= SMOOTH_BAR


def test_stages_chained_equal_the_one_call_model():
    """The stages chained on the word_reflow case of tests/variance_cases.py (durations predicted and aligned to the
    words, pitch, two variances) against DiffSingerVariance.forward on the same inputs, weights and x_T."""
    from diffsinger_amd.deploy import DiffSingerVarianceDeploy
    tag = "word_reflow"
    c, hp = vc.CASES[tag], vc.case_hparams(tag)
    hparams.clear()
    hparams.update(hp, infer=True, hop_size=512, audio_sample_rate=44100, midi_smooth_width=0.06)
    model = DiffSingerVarianceDeploy(c["vocab"])
    shapes = vc.sorted_param_shapes(model.named_parameters())
    model.load_state_dict({k: torch.from_numpy(v) for k, v in vc.synth_weights(shapes, c["seed"] + 1).items()}, strict=False)
    model = model.cuda().eval()
    inp = {k: v[:1] for k, v in vc.case_inputs(tag).items()}                           # the unpadded item, alone
    t_len, steps = c["t_len"], hp["sampling_steps"]
    word_div = np.bincount(inp["ph2word"][0], minlength=c["n_word"] + 1)[None, 1:].astype(np.int64)
    rng = np.random.Generator(np.random.PCG64(5))
    note_midi = rng.uniform(50, 70, (1, 6)).astype(np.float32)
    note_dur = np.array([[9, 11, 7, 13, 8, t_len - 48]], dtype=np.int64)
    names = model.variance_prediction_list
    pn = dev(synth.synth_normal((1, 1, hp["pitch_prediction_args"]["repeat_bins"], t_len), 31))
    vn = dev(synth.synth_normal((1, len(names), hp["variances_prediction_args"]["total_repeat_bins"] // len(names), t_len), 32))
    all_true = torch.ones((1, t_len), dtype=torch.bool, device="cuda")
    with torch.no_grad():
        enc, x_masks = model.forward_linguistic_encoder_word(dev(inp["txt_tokens"]), dev(word_div), dev(inp["word_dur"]))
        dur = model.forward_dur_predictor(enc, x_masks, dev(inp["midi"]))
        ph_dur = model.rr(dur, dev(inp["ph2word"]), dev(inp["word_dur"]))
        cond, base = model.forward_pitch_preprocess(enc, ph_dur, note_midi=dev(note_midi), note_dur=dev(note_dur),
                                                    pitch=torch.zeros((1, t_len), device="cuda"), retake=all_true)
        pitch = model.forward_pitch_postprocess(model.forward_pitch_reflow(cond, steps=steps, noise=pn), base)
        zeros = {n: torch.zeros((1, t_len), device="cuda") for n in names}
        var_cond = model.forward_variance_preprocess(enc, ph_dur, pitch, variances=zeros,
                                                     retake=all_true[:, :, None].expand(1, t_len, len(names)))
        outs = model.forward_variance_postprocess(model.forward_variance_reflow(var_cond, steps=steps, noise=vn))
        dur1, pitch1, var1 = model(dev(inp["txt_tokens"]), dev(inp["midi"]), dev(inp["ph2word"]), word_dur=dev(inp["word_dur"]),
                                   base_pitch=base, infer=True, pitch_noise=pn, variance_noise=vn)
    close(dur, dur1.cpu().numpy(), ALONE_TOL, True, "durations")
    close(pitch, (base + pitch1).cpu().numpy(), ALONE_TOL, True, "pitch")
    assert list(var1) == names
    for n, v in zip(names, outs):
        close(v, var1[n].cpu().numpy(), ALONE_TOL, True, n)
    release(model)


# ------------------------------------------------------------------------------------------------ acoustic twin
@pytest.mark.parametrize("tag", list(dc.AC_CASES))
def test_acoustic_stages_vs_golden(g, tag):
    from diffsinger_amd.deploy import DiffSingerAcousticDeploy
    c, hp = dc.AC_CASES[tag], dc.acoustic_hparams(tag)
    hparams.clear()
    hparams.update(hp, infer=True)
    model = load(DiffSingerAcousticDeploy(dc.VOCAB, dc.M_BINS, cross_lingual_token_idx=c.get("cross")), c["seed"] + 1)
    inp = {k: dev(v) for k, v in dc.acoustic_inputs(tag).items()}
    with torch.no_grad():
        res = model.forward_fs2_aux(inp["tokens"], inp["durations"], inp["f0"],
                                    {k[4:]: v for k, v in inp.items() if k.startswith("var_")}, gender=inp.get("gender"),
                                    velocity=inp.get("velocity"), spk_embed=inp.get("spk_embed"), languages=inp.get("languages"))
        if hp["use_shallow_diffusion"]:
            cond, aux = res
            err = rel_err(aux, g[f"{tag}_aux"])
            print(f"aux_mel_pred: {err:.3e} of max |want|, bound {AUX_TOL:.1e}")
            assert err < AUX_TOL
        else:
            cond, aux = res, None
        err = rel_err(cond, g[f"{tag}_cond"])
        print(f"condition: {err:.3e} of max |want|, bound {ACOUSTIC_COND_TOL:.1e}")
        assert err < ACOUSTIC_COND_TOL
        t_len = cond.shape[1]
        for i, (stage, depth) in enumerate(c["stages"]):
            noise = dev(synth.synth_normal((1, 1, dc.M_BINS, t_len), c["seed"] + 2 + i))
            if depth is None:
                mel = getattr(model, stage)(cond, steps=c["steps"], noise=noise)
            else:
                mel = getattr(model, stage)(cond, aux, torch.tensor(depth, dtype=torch.float32), steps=c["steps"], noise=noise)
            close(mel, g[f"{tag}_{stage}"], SAMPLE_TOL, True, stage)
    release(model)


def test_example_script_renders_a_segment_stage_by_stage(tmp_path):
    """examples/ds_stages.py as a user would run it, on the synthetic experiment examples/ds_variance.py is tested with."""
    import json
    import subprocess
    import sys
    import yaml
    from diffsinger_amd.variance import DiffSingerVariance
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exp = tmp_path / "exp"
    exp.mkdir()
    hp = vc.case_hparams("word_reflow")
    hp.update(vc.HARNESS_HP, hidden_size=256, use_melody_encoder=True, num_spk=3)
    (exp / "config.yaml").write_text(yaml.safe_dump(hp))
    (exp / "dictionary.txt").write_text("ab\ta b\ncd\tc d\ne\te\n", encoding="utf8")
    (exp / "spk_map.json").write_text(json.dumps(vc.HARNESS_SPK))
    hparams.clear()
    hparams.update(hp, infer=True)
    model = DiffSingerVariance(8)
    shapes = vc.sorted_param_shapes(model.named_parameters())
    sd = dict(model.state_dict())
    sd.update({k: torch.from_numpy(v) for k, v in vc.synth_weights(shapes, 88).items()})
    torch.save({"state_dict": {"model." + k: v for k, v in sd.items()}, "category": "variance"}, exp / "model_ckpt_steps_7.ckpt")
    proj = tmp_path / "song.ds"
    proj.write_text(json.dumps(vc.make_variance_segments()))
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "ds_stages.py"), str(exp), str(proj), "--segment", "1",
                        "--steps", "3"], capture_output=True, text=True, timeout=300, cwd=root, env=dict(os.environ, PYTHONPATH=root))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "| done" in r.stdout and "| pitch: first pass" in r.stdout and "| energy:" in r.stdout, r.stdout
