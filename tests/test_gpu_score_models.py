"""-m gpu: `forward_score` of the top-level models and the scorers of validate.py against G25 - the reference's own
DiffSingerVariance.forward(infer=False) (two configurations of tests/variance_cases.py) and the `else` branch of
DiffSingerAcoustic.forward on a given condition (aux decoder + DDPM under shallow diffusion), with the draws the reference
made stored in the fixture and handed over.

Tolerances are the suite's existing ones for the same chains: the duration predictor and the denoisers behind the variance
encoders as tests/test_gpu_variance.py states them against G12 (5e-5 and 2e-4 of the largest reference value: there after
several evaluations, here after one), the aux decoder and one backbone evaluation as tests/test_gpu_width.py does (2e-5).
Targets and t are compared bit for bit.  The scorers are pinned in two steps: their dict is exactly the loss modules on
`forward_score`'s outputs with the task's lambdas, and the loss modules on the REFERENCE's outputs meet the fixture's
distance rule (tests/test_gpu_score.py)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import score_cases as sc  # noqa: E402
import variance_cases as vc  # noqa: E402
from diffsinger_amd import losses, validate  # noqa: E402
from diffsinger_amd.hparams import hparams  # noqa: E402
from gpu_util import check, dev, set_hp  # noqa: E402
from test_gpu_score import assert_scalar  # noqa: E402

TOL_NFE = TOL_AUX = 2e-5
TOL_DUR, TOL_CHAIN = 5e-5, 2e-4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g25_score.npz")


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


@pytest.fixture(autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    yield
    set_hp()


def release(model):
    for m in model.modules():
        if hasattr(m, "release_native"):
            m.release_native()
        twin = m.__dict__.get("_raw_twin")
        if twin is not None:
            twin.release_native()


def to_dev(d):
    return {k: ({n: dev(a) for n, a in v.items()} if isinstance(v, dict) else v if isinstance(v, int) else dev(v)) for k, v in d.items()}


def build_variance(tag):
    from diffsinger_amd.variance import DiffSingerVariance
    hp = sc.variance_hparams(tag)
    hparams.clear()
    hparams.update(hp, infer=False)
    c = vc.CASES[tag]
    model = DiffSingerVariance(c["vocab"])
    shapes = vc.sorted_param_shapes(model.named_parameters())
    params = vc.synth_weights(shapes, c["seed"] + 1)
    res = model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=False)
    assert not res.unexpected_keys and not set(res.missing_keys) & set(shapes)
    return model.cuda().eval(), hp


def variance_draws(g, tag, names):
    d = dict(pitch_t=dev(g[f"v_{tag}_pitch_t"]), pitch_noise=dev(g[f"v_{tag}_pitch_noise"]))
    if names:
        d.update(variance_t=dev(g[f"v_{tag}_variance_t"]), variance_noise=dev(g[f"v_{tag}_variance_noise"]))
    return d


def near(got, want, tol, what):
    got = got.cpu().numpy()
    err = np.abs(got - want).max() / max(1.0, np.abs(want).max())
    print(f"{what}: {err:.3g}")
    assert got.shape == want.shape and err < tol, (what, err, tol)


@pytest.mark.parametrize("tag", sc.VARIANCE_TAGS)
def test_variance_forward_score_vs_golden(g, tag):
    model, hp = build_variance(tag)
    sample, retakes, names = sc.variance_sample(tag)
    s, r = to_dev(sample), to_dev(retakes)
    scorer = validate.VarianceScorer(model)
    assert scorer.variance_prediction_list == names
    draws = variance_draws(g, tag, names)
    dur, pitch, var = scorer.run_model(s, **r, **draws)
    ddpm = hp["diffusion_type"] == "ddpm"
    # the pitch predictor: network output, target and t as the reference returns them
    assert len(pitch) == (2 if ddpm else 3)
    near(pitch[0], g[f"v_{tag}_pitch_pred"], TOL_CHAIN, (tag, "pitch"))
    assert np.array_equal(pitch[1].cpu().numpy(), g[f"v_{tag}_pitch_target"])
    if not ddpm:
        assert np.array_equal(pitch[2].cpu().numpy(), g[f"v_{tag}_pitch_t"])
    if names:
        near(var[0], g[f"v_{tag}_var_pred"], TOL_CHAIN, (tag, "variances"))
        assert np.array_equal(var[1].cpu().numpy(), g[f"v_{tag}_var_target"])
    else:
        assert var is None
    if hp["predict_dur"]:
        want = g[f"v_{tag}_dur"]
        assert (want < 0).any()                                         # the fixture has raw predictions below zero
        near(dur, want, TOL_DUR, (tag, "raw durations"))
        # against dsd_predict_dur: equal wherever that is positive, at or below zero where it clamps, exp(0) - offset at padding
        with torch.no_grad():
            _, clamped = model.fs2(s["tokens"], midi=s["midi"], ph2word=s["ph2word"], ph_dur=s["ph_dur"])
        pos = clamped > 0
        assert torch.equal(dur[pos], clamped[pos]) and bool((dur[~pos] <= 0).all()) and bool((~pos).any())
        pad = s["tokens"] == 0
        assert bool(pad.any()) and bool((dur[pad] == 1.0 - hp["dur_prediction_args"]["log_offset"]).all())
    else:
        assert dur is None
    # the scorer's dict: the loss modules on these outputs with the task's lambdas, and nothing else
    got = scorer.losses(s, **r, **draws)
    npad = (s["mel2ph"] > 0).unsqueeze(-1)
    main = losses.DiffusionLoss("l2") if ddpm else losses.RectifiedFlowLoss("l2", log_norm=True)

    def apply(o):
        return main(o[0], o[1], non_padding=npad) if ddpm else main(o[0], o[1], t=o[2], non_padding=npad)

    want = {"pitch_loss": hp["lambda_pitch_loss"] * apply(pitch)}
    if names:
        want["var_loss"] = hp["lambda_var_loss"] * apply(var)
    if hp["predict_dur"]:
        d = hp["dur_prediction_args"]
        mod = losses.DurationLoss(d["log_offset"], d["loss_type"], d["lambda_pdur_loss"], d["lambda_wdur_loss"], d["lambda_sdur_loss"])
        want["dur_loss"] = hp["lambda_dur_loss"] * mod(dur, s["ph_dur"], ph2word=s["ph2word"])
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dim() == 0 and got[k].dtype == torch.float32 and torch.equal(got[k], want[k]), k
        print(f"{tag} {k}: {float(got[k]):.9g} (reference {float(g[f'v_{tag}_{k}_ref32']):.9g})")
    # ... and the loss modules on the REFERENCE's outputs, under the fixture's distance rule
    t = None if ddpm else dev(g[f"v_{tag}_pitch_t"])
    ref = (dev(g[f"v_{tag}_pitch_pred"]), dev(g[f"v_{tag}_pitch_target"]), t)
    assert_scalar(g, f"v_{tag}_pitch_loss", apply(ref))
    if names:
        ref = (dev(g[f"v_{tag}_var_pred"]), dev(g[f"v_{tag}_var_target"]), dev(g[f"v_{tag}_variance_t"]))
        assert_scalar(g, f"v_{tag}_var_loss", apply(ref))
    if hp["predict_dur"]:
        assert_scalar(g, f"v_{tag}_dur_loss", mod(dev(g[f"v_{tag}_dur"]), s["ph_dur"], ph2word=s["ph2word"]))
    release(model)


def test_variance_scorer_seeded_and_refusals():
    tag = "word_reflow"
    model, hp = build_variance(tag)
    sample, retakes, names = sc.variance_sample(tag)
    s, r = to_dev(sample), to_dev(retakes)
    scorer = validate.VarianceScorer(model)
    a, b = scorer.losses(s, **r, seed=[41, 42]), scorer.losses(s, **r, seed=[41, 42])
    assert all(torch.equal(a[k], b[k]) for k in a)                      # the same seeds, the same losses
    other = scorer.losses(s, **r, seed=[43, 44])
    assert float(other["pitch_loss"]) != float(a["pitch_loss"]) and float(other["var_loss"]) != float(a["var_loss"])
    assert torch.equal(other["dur_loss"], a["dur_loss"])                # no draw in it
    # the two predictors do not share their draws under one seed
    _, pitch, var = scorer.run_model(s, **r, seed=7)
    assert not torch.equal(pitch[2], var[2])
    # default draws: torch's generator, random retake masks
    torch.manual_seed(5)
    x = scorer.losses(s)
    torch.manual_seed(5)
    y = scorer.losses(s)
    assert sorted(x) == ["dur_loss", "pitch_loss", "var_loss"] and all(torch.equal(x[k], y[k]) for k in x)
    assert sorted(scorer.build_metrics()) == ["breathiness_r2", "energy_r2", "ph_dur_acc", "pitch_acc", "pitch_r2", "rhythm_corr"]
    m = validate.retake_masks(64, 50, torch.device("cuda"))
    assert m.dtype == torch.bool and tuple(m.shape) == (64, 50) and 0.2 < float(m.float().mean()) < 0.8
    with pytest.raises(ValueError, match="seed"):
        scorer.losses(s, **r, seed=3, pitch_t=torch.rand(2, device="cuda"))
    # what stays refused
    with torch.no_grad(), pytest.raises(NotImplementedError):
        model(s["tokens"], midi=s["midi"], ph2word=s["ph2word"], ph_dur=s["ph_dur"], mel2ph=s["mel2ph"], infer=False)
    with torch.no_grad(), pytest.raises(NotImplementedError):
        model.fs2(s["tokens"], midi=s["midi"], ph2word=s["ph2word"], ph_dur=s["ph_dur"], infer=False)
    with pytest.raises(RuntimeError, match="inference-only"):           # outside no_grad on parameters that require grad
        model(s["tokens"], midi=s["midi"], ph2word=s["ph2word"], ph_dur=s["ph_dur"], mel2ph=s["mel2ph"])
    model.train()
    with pytest.raises(RuntimeError, match=r"eval\(\)"):
        scorer.losses(s, **r, seed=1)
    release(model)


def build_acoustic():
    from diffsinger_amd.toplevel import AcousticDecoder
    hp = sc.acoustic_hparams()
    hparams.clear()
    hparams.update(hp, infer=False)
    model = AcousticDecoder(sc.ACOUSTIC["M"])
    aux_sd, net_sd = sc.acoustic_weights()
    full = dict(model.state_dict())
    full.update({f"aux_decoder.{k}": torch.from_numpy(v) for k, v in aux_sd.items()})
    full.update({f"diffusion.denoise_fn.{k}": torch.from_numpy(v) for k, v in net_sd.items()})
    model.load_state_dict(full, strict=True)
    return model.cuda().eval(), hp


def test_acoustic_forward_score_vs_golden(g):
    model, hp = build_acoustic()
    sample, draws = sc.acoustic_sample()
    s, d = to_dev(sample), to_dev(draws)
    out = model.forward_score(s["condition"], s["mel"], **d)
    # the aux decoder's raw output (the reference's went through the aux_decoder_grad mix of the condition: the identity up
    # to its fp32 rounding, 3e-7 of the output's range in the fixture's generator log)
    check(out.aux_out, g["ac_aux_out"], TOL_AUX, what="aux_out")
    x_recon, noise = out.diff_out
    check(x_recon, g["ac_x_recon"], TOL_NFE, what="x_recon")
    assert torch.equal(noise, d["noise"])
    scorer = validate.AcousticScorer(model)
    got = scorer.losses(s, **d)
    npad = (s["mel2ph"] > 0).unsqueeze(-1).float()
    want = {"aux_mel_loss": hp["lambda_aux_mel_loss"] * losses.L1Loss()(out.aux_out, model.aux_decoder.norm_spec(s["mel"])),
            "mel_loss": losses.DiffusionLoss("l2")(x_recon, noise, non_padding=npad)}
    assert sorted(got) == sorted(want) and all(torch.equal(got[k], want[k]) for k in want)
    for k in got:
        print(f"acoustic {k}: {float(got[k]):.9g} (reference {float(g[f'ac_{k}_ref32']):.9g})")
    # the loss modules on the reference's outputs under the fixture's distance rule
    ref_aux = hp["lambda_aux_mel_loss"] * losses.L1Loss()(dev(g["ac_aux_out"]), model.aux_decoder.norm_spec(s["mel"]))
    assert_scalar(g, "ac_aux_mel_loss", ref_aux)
    assert_scalar(g, "ac_mel_loss", losses.DiffusionLoss("l2")(dev(g["ac_x_recon"]), d["noise"], non_padding=npad))
    # seeded: t stays below K_step, the same seed scores the same
    a, b = scorer.losses(s, seed=9), scorer.losses(s, seed=9)
    assert all(torch.equal(a[k], b[k]) for k in a) and float(scorer.losses(s, seed=10)["mel_loss"]) != float(a["mel_loss"])
    assert torch.equal(a["aux_mel_loss"], got["aux_mel_loss"])
    # one branch switched off, as the reference's shallow_diffusion_args allow
    model.shallow_args["train_diffusion"] = False
    assert sorted(scorer.losses(s, seed=9)) == ["aux_mel_loss"]
    model.shallow_args["train_diffusion"], model.shallow_args["train_aux_decoder"] = True, False
    assert sorted(scorer.losses(s, seed=9)) == ["mel_loss"]
    model.shallow_args["train_aux_decoder"] = True
    with torch.no_grad(), pytest.raises(NotImplementedError):
        model(s["condition"], s["mel2ph"], gt_mel=s["mel"], infer=False)
    model.train()
    with pytest.raises(RuntimeError, match=r"eval\(\)"):
        model.forward_score(s["condition"], s["mel"], seed=1)
    release(model)
