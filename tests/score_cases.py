"""The cases of G25 (tests/golden/g25_score.npz): validation scoring.  Shared by the generator
(tests/golden/make_golden_score.py), the host tests and the GPU tests, so that all three build the same seeded weights and
inputs (diffsinger_amd/synth.py).  Small on purpose: B = 3, 8-16 bins, T <= 70, L <= 12; the top-level variance cases are
those of tests/variance_cases.py (B = 2, T <= 57)."""
import numpy as np

HIDDEN = 256
B = 3
WN = dict(num_layers=4, num_channels=64, dilation_cycle_length=2)
LX = dict(num_layers=2, num_channels=64, expansion_factor=2, kernel_size=31, activation="PReLU", strong_cond=False)

# tag: wrapper class, its family, backbone, constructor arguments, frames, weight seed, data seed
WRAPPERS = {
    # a spectrogram under DDPM on a WaveNet: T = 67 is no multiple of 4 (scalar path of dsd_diffuse)
    "ddpm_wn": dict(cls="GaussianDiffusion", family="ddpm", backbone="wavenet", args=WN, T=67, wseed=2501, seed=2510,
                    kw=dict(out_dims=16, num_feats=1, timesteps=1000, k_step=1000)),
    # a spectrogram under rectified flow on a LYNXNet: T = 64 (vector path)
    "reflow_lx": dict(cls="RectifiedFlow", family="reflow", backbone="lynxnet", args=LX, T=64, wseed=2502, seed=2520,
                      kw=dict(out_dims=16, num_feats=1, t_start=0.0, time_scale_factor=1000)),
    # the pitch predictor's codec: one clamped curve in 8 repeated bins
    "pitch_ddpm": dict(cls="PitchDiffusion", family="ddpm", backbone="wavenet", args=WN, T=50, wseed=2503, seed=2530,
                       kw=dict(vmin=-8.0, vmax=8.0, cmin=-6.0, cmax=6.0, repeat_bins=8, timesteps=1000, k_step=1000)),
    # the variance predictor's codec: two curves, one of them clamped
    "multi_reflow": dict(cls="MultiVarianceRectifiedFlow", family="reflow", backbone="lynxnet", args=LX, T=70, wseed=2504,
                         seed=2540, kw=dict(ranges=[(-96.0, -12.0), (-10.0, 10.0)], clamps=[(-96.0, -16.0), None],
                                            repeat_bins=8, time_scale_factor=1000)),
}
SPEC_MIN, SPEC_MAX = -12.0, 0.5      # of the two spectrogram cases: one value for every bin


def wrapper_kwargs(tag):
    c = WRAPPERS[tag]
    kw = dict(c["kw"], backbone_type=c["backbone"], backbone_args=dict(c["args"]))
    if c["cls"] in ("GaussianDiffusion", "RectifiedFlow"):
        kw.update(spec_min=[SPEC_MIN], spec_max=[SPEC_MAX])
    return kw


def dims(tag):
    """(num_feats, bins) of the backbone"""
    kw = WRAPPERS[tag]["kw"]
    if "ranges" in kw:
        return len(kw["ranges"]), kw["repeat_bins"]
    if "repeat_bins" in kw:
        return 1, kw["repeat_bins"]
    return kw["num_feats"], kw["out_dims"]


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def wrapper_inputs(tag):
    """condition [B, T, H]; gt (a spectrogram [B, T, M], a curve [B, T] or a list of curves); t [B]; noise [B, F, M, T];
    non_padding [B, T, 1] with item 1 cut short; for the reflow cases `torch_seed` replaces `noise` in the generator (the
    reference draws x_start itself) and the drawn tensor is stored in the fixture."""
    c = WRAPPERS[tag]
    t_len, seed = c["T"], c["seed"]
    f, m = dims(tag)
    r = _rng(seed)
    cond = r.standard_normal((B, t_len, HIDDEN), dtype=np.float32)
    cls = c["cls"]
    if cls in ("GaussianDiffusion", "RectifiedFlow"):
        gt = (SPEC_MIN + (SPEC_MAX - SPEC_MIN) * r.random((B, t_len, m), dtype=np.float32)).astype(np.float32)
    elif cls.startswith("Pitch"):
        gt = (7.5 * r.standard_normal((B, t_len), dtype=np.float32)).astype(np.float32)        # some of it beyond the clamp
    else:
        gt = [(-54.0 + 30.0 * r.standard_normal((B, t_len), dtype=np.float32)).astype(np.float32),
              (4.0 * r.standard_normal((B, t_len), dtype=np.float32)).astype(np.float32)]
    if c["family"] == "ddpm":
        t = np.array([3, 499, 998], np.int64)
    else:
        t = np.array([0.02, 0.5, 0.97], np.float32)
    noise = r.standard_normal((B, f, m, t_len), dtype=np.float32)
    non_padding = np.ones((B, t_len, 1), np.float32)
    non_padding[1, t_len - 9:] = 0.0
    return dict(cond=cond, gt=gt, t=t, noise=noise, non_padding=non_padding, torch_seed=seed + 1)


# ---- the loss modules and metrics on seeded inputs
def loss_inputs():
    r = _rng(2550)
    pred = r.standard_normal((B, 1, 12, 37), dtype=np.float32)
    target = r.standard_normal((B, 1, 12, 37), dtype=np.float32)
    non_padding = np.ones((B, 37, 1), np.float32)
    non_padding[0, 30:] = 0.0
    non_padding[2] = 0.0                            # an all-padding item
    t = np.array([1e-9, 0.3, 0.999], np.float32)    # the first one is clipped
    return dict(pred=pred, target=target, non_padding=non_padding, t=t)


def curve_inputs():
    r = _rng(2560)
    target = (60.0 + 5.0 * r.standard_normal((B, 70), dtype=np.float32)).astype(np.float32)
    pred = (target + 0.6 * r.standard_normal((B, 70), dtype=np.float32)).astype(np.float32)
    mask = r.random((B, 70)) < 0.8
    mask[1] = False
    return dict(pred=pred, target=target, mask=mask, tolerance=0.5)


def dur_inputs():
    """L = 12 phonemes; word 0 is padding.  Item 2 has a trailing pad and a word of one phoneme."""
    r = _rng(2570)
    length = 12
    ph2word = np.array([[1, 1, 2, 2, 2, 3, 4, 4, 5, 5, 5, 6],
                        [1, 2, 2, 3, 3, 3, 3, 4, 5, 5, 6, 6],
                        [1, 1, 1, 2, 3, 3, 4, 4, 4, 0, 0, 0]], np.int64)
    dur_gt = r.integers(2, 40, size=(B, length)).astype(np.float32) * (ph2word > 0)
    raw = (dur_gt * (1.0 + 0.15 * r.standard_normal((B, length))) + r.standard_normal((B, length))).astype(np.float32)
    raw[0, 3] = -0.25                               # a negative raw prediction (still above -offset)
    raw = (raw * (ph2word > 0) + (ph2word == 0) * 0.0).astype(np.float32)
    mask = ph2word > 0
    return dict(dur_pred_raw=raw, dur_pred=np.rint(np.maximum(raw, 0)).astype(np.int64), dur_gt=dur_gt.astype(np.float32),
                ph2word=ph2word, mask=mask, offset=1.0, lambdas=(0.6, 0.3, 0.1), rhythm_tolerance=0.05, pdur_tolerance=0.2)


# ---- the top-level models: DiffSingerVariance (configurations of tests/variance_cases.py) and the acoustic decoder
SCORE_HP = dict(main_loss_type="l2", main_loss_log_norm=True, lambda_dur_loss=1.0, lambda_pitch_loss=1.0, lambda_var_loss=1.0,
                lambda_aux_mel_loss=0.2)
DUR_LAMBDAS = dict(lambda_pdur_loss=0.3, lambda_wdur_loss=1.0, lambda_sdur_loss=3.0)
VARIANCE_TAGS = ("word_reflow", "melody_ddim")


def variance_hparams(tag):
    import variance_cases as vc
    hp = vc.case_hparams(tag)
    hp.update(SCORE_HP)
    hp["dur_prediction_args"] = dict(hp["dur_prediction_args"], **DUR_LAMBDAS)
    return hp


def variance_sample(tag):
    """A collated validation batch (the keys of variance_task.py:162-182) on the inputs of variance_cases.case_inputs, with
    what training has and inference lacks: the true phoneme durations with their mel2ph, the true curves, retake masks."""
    import variance_cases as vc
    c, hp, inp = vc.CASES[tag], variance_hparams(tag), vc.case_inputs(tag)
    bsz, n_ph, t_len = c["bsz"], c["n_ph"], c["t_len"]
    r = _rng(c["seed"] + 50)
    tokens = inp["txt_tokens"]
    if "ph_dur" in inp:
        ph_dur, mel2ph = inp["ph_dur"], inp["mel2ph"]
    else:
        ph_dur = np.zeros((bsz, n_ph), np.int64)
        mel2ph = np.zeros((bsz, t_len), np.int64)
        for b in range(bsz):
            n = int((tokens[b] > 0).sum())
            w = r.random(n) + 0.3
            ph_dur[b, :n] = np.maximum(1, np.floor(w / w.sum() * (t_len - 5 * b)).astype(np.int64))
            seq = np.repeat(np.arange(1, n + 1), ph_dur[b, :n])
            mel2ph[b, :len(seq)] = seq[:t_len]
    s = dict(size=bsz, tokens=tokens, ph_dur=ph_dur, ph2word=inp["ph2word"], midi=inp["midi"], mel2ph=mel2ph,
             base_pitch=inp["base_pitch"])
    for k in ("note_midi", "note_rest", "note_dur", "note_glide", "mel2note", "languages"):
        if k in inp:
            s[k] = inp[k]
    if "spk_id" in inp:
        s["spk_ids"] = inp["spk_id"]
    s["pitch"] = (inp["base_pitch"] + r.normal(0, 0.7, (bsz, t_len))).astype(np.float32)
    names = [n for n in ("energy", "breathiness", "voicing", "tension") if hp.get("predict_" + n)]
    for n in names:
        s[n] = (r.uniform(-5, 5, (bsz, t_len)) if n == "tension" else r.uniform(-70, -8, (bsz, t_len))).astype(np.float32)
    retakes = dict(pitch_retake=r.random((bsz, t_len)) < 0.5)
    if names:
        retakes["variance_retake"] = {n: r.random((bsz, t_len)) < 0.5 for n in names}
    return s, retakes, names


# the acoustic decoder under shallow diffusion: ConvNeXt aux decoder + DDPM on a WaveNet, K_step 400
ACOUSTIC = dict(M=16, T=45, wseed=2580, seed=2590,
                aux_args=dict(num_channels=64, num_layers=2, kernel_size=7, dropout_rate=0.1))


def acoustic_hparams():
    hp = dict(hidden_size=HIDDEN, schedule_type="linear", diffusion_type="ddpm", use_shallow_diffusion=True, timesteps=1000,
              K_step=400, T_start=0.4, time_scale_factor=1000, backbone_type="wavenet", backbone_args=dict(WN),
              spec_min=[SPEC_MIN], spec_max=[SPEC_MAX], diff_speedup=10, diff_accelerator="ddim",
              shallow_diffusion_args=dict(aux_decoder_arch="convnext", aux_decoder_args=dict(ACOUSTIC["aux_args"]),
                                          train_aux_decoder=True, train_diffusion=True, aux_decoder_grad=0.1, val_gt_start=False))
    hp.update(SCORE_HP)
    return hp


def acoustic_sample():
    a = ACOUSTIC
    r = _rng(a["seed"])
    cond = r.standard_normal((B, a["T"], HIDDEN), dtype=np.float32)
    mel = (SPEC_MIN + (SPEC_MAX - SPEC_MIN) * r.random((B, a["T"], a["M"]), dtype=np.float32)).astype(np.float32)
    mel2ph = np.tile(np.arange(1, a["T"] + 1, dtype=np.int64) // 5 + 1, (B, 1))
    mel2ph[2, a["T"] - 11:] = 0
    return dict(size=B, condition=cond, mel=mel, mel2ph=mel2ph), dict(t=np.array([0, 123, 399], np.int64),
                                                                       noise=r.standard_normal((B, 1, a["M"], a["T"]), dtype=np.float32))


def acoustic_weights():
    from diffsinger_amd import synth
    a = ACOUSTIC
    aux = synth.synth_state_dict(synth.convnext_param_shapes(HIDDEN, a["M"], num_channels=a["aux_args"]["num_channels"],
                                                             num_layers=a["aux_args"]["num_layers"],
                                                             kernel_size=a["aux_args"]["kernel_size"], prefix="decoder."),
                                 seed=a["wseed"])
    net = synth.synth_state_dict(synth.backbone_param_shapes("wavenet", a["M"], 1, hidden_size=HIDDEN, **WN), seed=a["wseed"] + 1)
    return aux, net
