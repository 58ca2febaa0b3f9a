"""The cases of the twin configuration suite: dsd_acoustic_open / dsd_variance_open on model shapes other than the one
tests/deploy_cases.py, cacoustic_cases.py and cvariance_cases.py share (hidden 64, two heads, a 64-channel WaveNet, 16 bins,
the linear schedule).  Shared by the generator of G31 (tests/golden/make_golden_twin_configs.py, which runs the reference's
deployment twins on them, on the CPU), the host tests (test_twin_configs_host.py) and the GPU tests
(test_gpu_twin_configs.py), so that all three build the same seeded weights and inputs; only the reference's outputs are stored.

One utterance per case unless it says `lengths`; 5 .. 9 tokens; 70 frames (over the 64-frame tile and the 32-frame transpose
tile, inside one 256-frame block) or 41; samplers of 2 .. 4 steps.  `reaches` names the lines a case is there for.

Bounds are the ones tests/test_gpu_deploy.py applies to the same quantities (BOUNDS below names them).  FLOORS holds, per
case and quantity, the reference's own fp32 result against a float64 evaluation of the same stage as the generator printed it
("floor <case> <quantity> <value>"): where a floor exceeds half the bound, the bound of that case and quantity is 2 x floor
(`bound_for`), the rule of tests/encoder_size_cases.py.  Nothing here is derived from what the library computes."""
from collections import OrderedDict

import numpy as np

import deploy_cases as dc

VOCAB = dc.VOCAB
LYNX = dict(num_layers=2, num_channels=90, expansion_factor=3, kernel_size=7, activation="SiLU", strong_cond=True, dropout=0.0)
LYNX_PITCH = dict(num_layers=2, num_channels=90, expansion_factor=2, kernel_size=7, activation="PReLU", strong_cond=False, dropout=0.0)
LYNX_VAR = dict(num_layers=2, num_channels=90, expansion_factor=2, kernel_size=7, activation="ReLU", strong_cond=False, dropout=0.0)
CURVES = dc.VARIANCE_NAMES                                              # energy, breathiness, voicing, tension: the bit order
EMBEDS = CURVES + ("key_shift", "speed")

# ------------------------------------------------------------------------------------------------ acoustic twin
_H96 = dict(hidden_size=96, num_heads=4)
_LYNX_REFLOW_HP = dict(_H96, use_shallow_diffusion=True, diffusion_type="reflow", backbone_type="lynxnet", backbone_args=LYNX)


def _alone(name, seed):
    return dict(hp={f"use_{name}_embed": True, "diffusion_type": "reflow"}, m_bins=16, n_ph=5 + seed % 5, t_len=70, stages=[], seed=seed,
                reaches=f"acoustic_api.hip dsd_acoustic_condition: the `{name}` slot alone (curves[] / gender / velocity -> dsd_encode_extras), "
                        f"modelfile.acoustic_config embed_flags with one bit set")


# stages: (the twin's method, depth or None for the full stage, steps)
AC_CASES = OrderedDict(
    lynx_reflow=dict(hp=_LYNX_REFLOW_HP, m_bins=80, n_ph=7, t_len=70, seed=3100,
                     stages=[("forward_shallow_reflow", 0.5, 3), ("forward_reflow", None, 2)],
                     reaches="dsd_acoustic_open: a DSD_BACKBONE_LYNXNET denoiser section, 90 channels run at 96, fed a condition of width "
                             "H = 96; ac_source_kernel at M = 80 (a partial second tile of bins) with T = 70 through dsd_acoustic_start; "
                             "k / mid at 80 floats (mid_off = 128); the ConvNeXt aux decoder at H = 96, M = 80"),
    lynx_ddpm_cosine=dict(hp=dict(use_shallow_diffusion=True, diffusion_type="ddpm", schedule_type="cosine", K_step=400,
                                  backbone_type="lynxnet", backbone_args=LYNX), m_bins=16, n_ph=6, t_len=70, seed=3110,
                          stages=[("forward_shallow_diffusion", 0.3, 3), ("forward_shallow_diffusion", 0.004, 4),
                                  ("forward_shallow_diffusion", 0.0, 3), ("forward_diffusion", None, 3)],
                          reaches="dsd_ddpm_tables_fill(cosine) behind both dsd_acoustic_plan (src_scale / noise_scale) and programs_of "
                                  "(DDIM t_max 300 speed-up 100; ancestral t_max 4 with step noise; the empty loop from the source; "
                                  "DDIM from noise over [0, 400) at speed-up 250): MIX, MIX, SOURCE, NOISE"),
    wn_cosine=dict(hp=dict(diffusion_type="ddpm", schedule_type="cosine", K_step=1000), m_bins=16, n_ph=7, t_len=70, seed=3120,
                   stages=[("forward_diffusion", None, 2)],
                   reaches="the cosine tables with the WaveNet of deploy_cases.plain_ddpm: tells `cosine` from `LYNXNet` if lynx_ddpm_cosine fails"),
    wn_h32_m5=dict(hp=dict(hidden_size=32, num_heads=4, use_shallow_diffusion=True, diffusion_type="reflow"), m_bins=5, n_ph=5, t_len=41,
                   seed=3130, stages=[("forward_shallow_reflow", 0.5, 2), ("forward_reflow", None, 3)],
                   reaches="H = 32 with head width 8 (the encoder's smallest); k / mid of 5 floats inside one 64-float unit (mid_off = 64); "
                           "ac_source_kernel with a single partial tile of bins; ac_mel_base at n = 205 (the scalar path)"),
    alone_energy=_alone("energy", 3140), alone_breathiness=_alone("breathiness", 3141), alone_voicing=_alone("voicing", 3142),
    alone_tension=_alone("tension", 3143), alone_key_shift=_alone("key_shift", 3144), alone_speed=_alone("speed", 3145),
    pairs=dict(hp=dict(use_breathiness_embed=True, use_voicing_embed=True, use_tension_embed=True, use_speed_embed=True,
                       diffusion_type="reflow"), m_bins=16, n_ph=8, t_len=70, stages=[], seed=3150,
               reaches="embed_flags 0x2e: curves[1..3] without curves[0], speed without key shift"),
    all_h96=dict(hp=dict(_H96, use_energy_embed=True, use_breathiness_embed=True, use_voicing_embed=True, use_tension_embed=True,
                         use_key_shift_embed=True, use_speed_embed=True, use_spk_id=True, num_spk=3, use_lang_id=True, num_lang=2,
                         f0_embed_type="discrete", diffusion_type="reflow"),
                 cross=[1, 4, 6, 9], m_bins=16, n_ph=9, t_len=70, stages=[], seed=3160,
                 reaches="every term of the condition stage at H = 96: embed_flags 0x3f, a per-frame speaker embedding "
                         "(spk_mix_tstride = 96), the language mask, the discrete f0 gather of dsd_cond_assemble at H = 96, f0_coarse"),
    lynx_ragged=dict(hp=_LYNX_REFLOW_HP, m_bins=80, n_ph=6, t_len=70, seed=3100, lengths=[70, 1, 33],
                     stages=[("forward_shallow_reflow", 0.5, 3)],
                     reaches="dsd_acoustic_set_lengths passed on to a LYNXNet denoiser handle and the aux decoder: B = 3, lengths 70, 1, 33"),
)


def acoustic_hparams(tag):
    c = AC_CASES[tag]
    hp = dict(dc.BASE_HP)
    hp.update(dc.ACOUSTIC_HP)
    hp.update(c["hp"])
    rng = np.random.Generator(np.random.PCG64(99))                        # deploy_cases.acoustic_hparams at M bins
    hp["spec_min"] = (-12.0 + rng.random(c["m_bins"])).round(3).tolist()
    hp["spec_max"] = (0.0 + rng.random(c["m_bins"])).round(3).tolist()
    return hp


def _frame_inputs(rng, hp, bsz, t_len, n_ph, out):
    """the optional inputs of the condition stage, in a fixed order; every curve from the case's own stream"""
    for n in CURVES:
        if hp[f"use_{n}_embed"]:
            lo, hi = (-5, 5) if n == "tension" else (-60, -10)
            out["var_" + n] = rng.uniform(lo, hi, (bsz, t_len)).astype(np.float32)
    if hp["use_key_shift_embed"]:
        out["gender"] = rng.uniform(-1.3, 1.3, (bsz, t_len)).astype(np.float32)          # beyond [-1, 1]: clipped
    if hp["use_speed_embed"]:
        out["velocity"] = rng.uniform(0.3, 2.4, (bsz, t_len)).astype(np.float32)         # beyond [0.5, 2]: clipped
    if hp["use_spk_id"]:
        out["spk_embed"] = rng.standard_normal((bsz, t_len, hp["hidden_size"])).astype(np.float32)
    if hp["use_lang_id"]:
        out["languages"] = rng.integers(1, hp["num_lang"] + 1, (bsz, n_ph)).astype(np.int64)
    return out


def acoustic_inputs(tag):
    """Seeded inputs of a one-utterance acoustic case (deploy_cases.acoustic_inputs at the case's own sizes): numpy, B = 1."""
    c, hp = AC_CASES[tag], acoustic_hparams(tag)
    assert "lengths" not in c
    rng = np.random.Generator(np.random.PCG64(c["seed"]))
    n_ph, t_len = c["n_ph"], c["t_len"]
    tokens = rng.integers(1, VOCAB, (1, n_ph)).astype(np.int64)
    tokens[0, -1] = 0                                                     # a padding token: its duration is masked away
    durations = np.append(dc._split(rng, t_len, n_ph - 1), 3)             # the reference needs sum(masked durations) == T
    out = dict(tokens=tokens, durations=durations[None], f0=(220.0 * 2.0 ** rng.uniform(-1, 1, (1, t_len))).astype(np.float32))
    out["f0"][0, 5:8] = 0.0                                               # unvoiced frames
    return _frame_inputs(rng, hp, 1, t_len, n_ph, out)


def acoustic_batch_inputs(tag):
    """The padded batch of a `lengths` case, built like cacoustic_cases.batch_inputs: B = 3; item 0 fills every frame; item 1
    has a padding token with a non-zero duration (masked away) and a single real frame; item 2 ends in two padding tokens.
    f0 holds junk past every item's end.  -> numpy dict with `lengths`."""
    c, hp = AC_CASES[tag], acoustic_hparams(tag)
    lens, n_ph, t_len = c["lengths"], c["n_ph"], c["t_len"]
    rng = np.random.Generator(np.random.PCG64(c["seed"] + 50))
    tokens = rng.integers(1, VOCAB, (3, n_ph)).astype(np.int64)
    tokens[1, 2] = 0
    tokens[2, -2:] = 0
    durations = np.zeros((3, n_ph), dtype=np.int64)
    durations[0] = dc._split(rng, lens[0], n_ph)
    durations[1, [0, 1, 3, 4, 5]] = dc._split(rng, lens[1], 5)
    durations[1, 2] = 9
    durations[2, :n_ph - 2] = dc._split(rng, lens[2], n_ph - 2)
    durations[2, n_ph - 2] = 5
    out = dict(lengths=np.array(lens, dtype=np.int32), tokens=tokens, durations=durations,
               f0=(220.0 * 2.0 ** rng.uniform(-1, 1, (3, t_len))).astype(np.float32))
    out["f0"][:, 5:8] = 0.0
    _frame_inputs(rng, hp, 3, t_len, n_ph, out)
    for b, n in enumerate(lens):
        out["f0"][b, n:] = 3000.0
    return out


FRAME_LEVEL = ("f0", "gender", "velocity", "spk_embed", "pitch", "expr", "retake")


def item_of(inp, b, n):
    """item `b` of a padded batch cut to its own `n` frames, as a batch of one"""
    return {k: (v[b:b + 1, :n] if k in FRAME_LEVEL or k.startswith("var_") else v[b:b + 1]) for k, v in inp.items() if k != "lengths"}


def stage_seed(tag, i):
    """the x_T seed of stage i of an acoustic case; an ancestral stage's step noise takes the seeds after it"""
    return AC_CASES[tag]["seed"] + 100 * (i + 1)


def stage_noise(tag, i):
    """the arrays stage i of an acoustic case draws, [B, 1, M, T] each (B = 3 for a `lengths` case): x_T, then one per step of
    the ancestral sampler (a DDPM stage whose speed-up is 1 draws t_max of them, the last one unused)"""
    from diffsinger_amd import synth
    c, hp = AC_CASES[tag], acoustic_hparams(tag)
    _, depth, steps = c["stages"][i]
    seed = stage_seed(tag, i)
    shape = (len(c.get("lengths", [0])), 1, c["m_bins"], c["t_len"])
    arrays = [synth.synth_normal(shape, seed)]
    if hp["diffusion_type"] == "ddpm" and depth is not None:
        depth_i = min(int(np.round(np.float32(depth) * np.float32(hp["timesteps"]))), hp["K_step"])      # diffusion.py:117-119
        if max(1, depth_i // steps) == 1:
            arrays += [synth.synth_normal(shape, seed + 1 + j) for j in range(depth_i)]
    return arrays


# ------------------------------------------------------------------------------------------------ variance twin
def _dur(chans, layers, ks):
    return dict(arch="fs2", hidden_size=chans, dropout=0.1, num_layers=layers, kernel_size=ks, log_offset=1.0, loss_type="mse")


_LYNX_PITCH_HP = dict(_H96, predict_dur=True, predict_pitch=True, use_melody_encoder=True, use_glide_embed=True, diffusion_type="reflow",
                      melody_encoder_args=dict(hidden_size=64, enc_layers=2),
                      pitch_prediction_args=dict(pitd_norm_min=-8.0, pitd_norm_max=8.0, pitd_clip_min=-12.0, pitd_clip_max=12.0,
                                                 repeat_bins=5, backbone_type="lynxnet", backbone_args=LYNX_PITCH))

# deploy_cases.VARIANCE_HP gives energy and voicing one range; a range of its own per curve lets a swapped slot show
_OWN_RANGES = dict(voicing_db_min=-90.0, voicing_db_max=-15.0, breathiness_db_min=-100.0)

# the form of deploy_cases.VAR_CASES, so that deploy_cases.variance_inputs(tag, VAR_CASES) builds the inputs
VAR_CASES = OrderedDict(
    # the clamps are the reference's own (param_adaptor.py:35-64 sets one per curve from hparams; none can be switched off there)
    four_curves=dict(hp=dict(_OWN_RANGES, predict_energy=True, predict_breathiness=True, predict_voicing=True, predict_tension=True, diffusion_type="reflow",
                             variances_prediction_args=dict(total_repeat_bins=20, backbone_type="wavenet", backbone_args=dc.NET)),
                     steps=3, n_ph=8, n_word=3, n_note=0, t_len=70, seed=3300,
                     reaches="variance_api.hip: n_feats = 4 and a repeat-bin count of 5; var_slot for every bit; the post kernel's four rows"),
    two_late=dict(hp=dict(_OWN_RANGES, predict_breathiness=True, predict_voicing=True, diffusion_type="reflow"),
                  steps=2, n_ph=7, n_word=3, n_note=0, t_len=70, seed=3310,
                  reaches="var_slot / modelfile.variance_config: rows 0 and 1 of the sample are slots 1 and 2 of the tables; curves[1..2] alone"),
    lynx_pitch=dict(hp=_LYNX_PITCH_HP, glide=True, expr=True, retake="mixed", steps=3, n_ph=9, n_word=4, n_note=5, t_len=70, seed=3320,
                    reaches="dsd_variance_open: a LYNXNet pitch predictor (90 channels) at H = 96, pitch_repeat_bins = 5, a melody encoder "
                            "of hidden size 64 inside a model of 96 (out_proj 64 -> 96), glides"),
    lynx_variances_ddpm=dict(hp=dict(predict_energy=True, predict_tension=True, use_spk_id=True, num_spk=2, diffusion_type="ddpm",
                                     variances_prediction_args=dict(total_repeat_bins=12, backbone_type="lynxnet", backbone_args=LYNX_VAR)),
                             steps=2, n_ph=8, n_word=3, n_note=0, t_len=70, seed=3330,
                             reaches="a LYNXNet variance predictor of two features (6 bins each) in the DDPM twin, run on the borrowed handle by the "
                                     "DDIM program of dsd_program_build: slots 0 and 3, the speaker embedding"),
    dur_wide=dict(hp=dict(_H96, predict_dur=True, diffusion_type="reflow", enc_ffn_kernel_size=9, ffn_act="swiglu", use_rope=False, rel_pos=True,
                          dur_prediction_args=_dur(40, 1, 5)),
                  steps=0, n_ph=9, n_word=4, n_note=0, t_len=70, seed=3340,
                  reaches="the linguistic encoder at H = 96 with a k = 9 swiglu FFN and relative positions; a one-layer duration predictor "
                          "of 40 channels, kernel 5; a model of the encoder and the duration predictor only"),
    lynx_ragged_var=dict(hp=_LYNX_PITCH_HP, steps=3, n_ph=6, n_word=3, n_note=4, t_len=70, seed=3320, lengths=[70, 1, 41],
                         reaches="dsd_variance_set_lengths passed on to a LYNXNet pitch predictor handle: B = 3, lengths 70, 1, 41"),
)


def variance_hparams(tag):
    return dc.variance_hparams(tag, VAR_CASES)


def variance_inputs(tag):
    assert "lengths" not in VAR_CASES[tag]
    return dc.variance_inputs(tag, VAR_CASES)


def variance_noise_shapes(tag):
    return dc.variance_noise_shapes(tag, VAR_CASES)


def variance_batch_inputs(tag):
    """The padded batch of a `lengths` case, built like cvariance_cases.batch_inputs at T = 70: item 0 fills every length;
    item 1 has one real phoneme, one note and one frame; item 2 has a zero in word_div, a phoneme without frames and a padding
    token at its end.  Frames past an item's length hold zeros."""
    c = VAR_CASES[tag]
    lens, n_ph, n_word, n_note, t_len = c["lengths"], c["n_ph"], c["n_word"], c["n_note"], c["t_len"]
    rng = np.random.Generator(np.random.PCG64(c["seed"] + 50))
    tokens = rng.integers(1, VOCAB, (3, n_ph)).astype(np.int64)
    tokens[1, 1:] = 0
    tokens[2, -1] = 0
    word_div = np.array([[2, 2, 2], [1, 0, 0], [3, 0, 2]], dtype=np.int64)
    ph_dur = np.zeros((3, n_ph), dtype=np.int64)
    ph_dur[0] = dc._split(rng, lens[0], n_ph)
    ph_dur[1, 0] = lens[1]
    ph_dur[2, :5] = dc._split(rng, lens[2], 5)
    ph_dur[2, 0] += ph_dur[2, 1]
    ph_dur[2, 1] = 0
    word_dur = np.zeros((3, n_word), dtype=np.int64)
    for b in range(3):
        edges = np.concatenate([[0], np.cumsum(word_div[b])])
        word_dur[b] = [ph_dur[b, edges[i]:edges[i + 1]].sum() for i in range(n_word)]
    note_dur = np.zeros((3, n_note), dtype=np.int64)
    note_midi = rng.uniform(48, 72, (3, n_note)).astype(np.float32)
    for b, n in enumerate((4, 1, 3)):
        note_dur[b, :n] = dc._split(rng, lens[b], n)
        note_midi[b, n:] = -1.0                                           # padding notes
    out = dict(lengths=np.array(lens, dtype=np.int32), tokens=tokens, word_div=word_div, word_dur=word_dur, ph_dur=ph_dur,
               ph_midi=rng.integers(40, 80, (3, n_ph)).astype(np.int64),
               note_midi=note_midi, note_rest=rng.random((3, n_note)) < 0.25, note_dur=note_dur,
               note_glide=rng.integers(0, 3, (3, n_note)).astype(np.int64),
               pitch=(60.0 + 6.0 * np.sin(np.arange(t_len)[None] / 5.0) + rng.normal(0, 0.5, (3, t_len))).astype(np.float32),
               expr=rng.random((3, t_len)).astype(np.float32), retake=rng.random((3, t_len)) < 0.5)
    for b in range(3):
        for k in ("pitch", "expr", "retake"):
            out[k][b, lens[b]:] = 0
    return out


def variance_item(batch, b):
    """item `b` of variance_batch_inputs as the reference takes it -> (inputs, the count of phonemes its words cover).  Cut to
    its own frames, but not to its own phonemes: the reference's encoder is not blind to padding tokens (EncSALayer zeroes
    the padding rows and then runs LayerNorm over them, so the k = 3 FFN conv reads LayerNorm's bias, not zeros, behind the
    last real phoneme: 2 % of the output's range here), and the library, like the Python twin, computes that padded form.  The
    reference's regulator needs word_div to total L, so the padding tokens are counted into the last word; what they embed
    there is masked before anything reads it."""
    out = item_of(batch, b, int(batch["lengths"][b]))
    n_real = int(batch["word_div"][b].sum())
    out["word_div"] = out["word_div"].copy()
    out["word_div"][0, -1] += out["tokens"].shape[1] - n_real
    return out, n_real


# ------------------------------------------------------------------------------------------------ models
def build_acoustic(tag, cuda):
    """-> (DiffSingerAcousticDeploy with the case's seeded weights, hparams of the case); hparams stay set to the case."""
    import torch
    from diffsinger_amd.deploy import DiffSingerAcousticDeploy
    from diffsinger_amd.hparams import hparams
    c, hp = AC_CASES[tag], acoustic_hparams(tag)
    hparams.clear()
    hparams.update(hp, infer=True)
    model = DiffSingerAcousticDeploy(VOCAB, c["m_bins"], cross_lingual_token_idx=c.get("cross"))
    return _load(model, c["seed"] + 1, cuda, torch), hp


def build_variance(tag, cuda, over=None):
    """-> (DiffSingerVarianceDeploy with the case's seeded weights, hparams); `over`: hparams changed on top of the case's."""
    import torch
    from diffsinger_amd.deploy import DiffSingerVarianceDeploy
    from diffsinger_amd.hparams import hparams
    c, hp = VAR_CASES[tag], variance_hparams(tag)
    hp.update(over or {})
    hparams.clear()
    hparams.update(hp, infer=True)
    model = DiffSingerVarianceDeploy(VOCAB, cross_lingual_token_idx=c.get("cross"))
    return _load(model, c["seed"] + 1, cuda, torch), hp


def _load(model, seed, cuda, torch):
    shapes = dc.sorted_param_shapes(model.named_parameters())
    res = model.load_state_dict({k: torch.from_numpy(v) for k, v in dc.synth_weights(shapes, seed).items()}, strict=False)
    assert not res.unexpected_keys and not set(res.missing_keys) & set(shapes)
    model = model.eval()
    return model.cuda() if cuda else model


# ------------------------------------------------------------------------------------------------ what the fixture holds
def acoustic_keys(tag):
    """name -> shape of every array G31 holds for an acoustic case (items of a `lengths` case: `<tag>_i<b>_...` at their own T)"""
    c, hp = AC_CASES[tag], acoustic_hparams(tag)
    h, m = hp["hidden_size"], c["m_bins"]
    out = OrderedDict()
    for pre, t in ([(f"{tag}_i{b}", n) for b, n in enumerate(c["lengths"])] if "lengths" in c else [(tag, c["t_len"])]):
        out[f"{pre}_cond"] = (1, t, h)
        if hp["use_shallow_diffusion"]:
            out[f"{pre}_aux"] = (1, t, m)
        for i in range(len(c["stages"])):
            out[f"{pre}_s{i}"] = (1, t, m)
    return out


def variance_keys(tag):
    c, hp = VAR_CASES[tag], variance_hparams(tag)
    h = hp["hidden_size"]
    names = dc.variance_names(hp)
    out = OrderedDict()
    if "lengths" in c:
        real = variance_batch_inputs(tag)["word_div"].sum(1)
        items = [(f"{tag}_i{b}", n, int(real[b])) for b, n in enumerate(c["lengths"])]
    else:
        items = [(tag, c["t_len"], c["n_ph"])]
    for pre, t, n_ph in items:
        out[f"{pre}_enc"], out[f"{pre}_x_masks"] = (1, n_ph, h), (1, n_ph)
        if hp["predict_dur"]:
            out[f"{pre}_dur_pred"] = (1, n_ph)
        if hp["predict_pitch"]:
            out[f"{pre}_pitch_cond"], out[f"{pre}_base_pitch"] = (1, t, h), (1, t)
            if c["steps"]:
                out[f"{pre}_x_pred"], out[f"{pre}_pitch_pred"] = (1, t), (1, t)
        if names:
            out[f"{pre}_var_cond"] = (1, t, h)
            out[f"{pre}_xs_pred"] = (1, t) if len(names) == 1 else (1, len(names), t)
            for n in names:
                out[f"{pre}_out_{n}"] = (1, t)
    return out


# ------------------------------------------------------------------------------------------------ what the library refuses
# Configurations that pack and pass the checks between the sections, and that the library refuses by design when it creates
# the inner handle; the case named runs at the nearest accepted value.  (what, the hparams over the named case, the section whose dsd_model_create refuses, a fragment of the message)
REFUSED = [
    ("a melody encoder of hidden size 48 (lynx_pitch runs it at 64)", "lynx_pitch", dict(melody_encoder_args=dict(hidden_size=48, enc_layers=2)),
     ".melody", "dsd_token_encoder_create: hidden_size must be a multiple of 32 and of 2 * num_heads"),
]

# ------------------------------------------------------------------------------------------------ bounds and floors
# quantity -> (the bound's name in tests/test_gpu_deploy.py, its value, its unit: "rel" of max |want|, "one" of max(1, max |want|),
# "abs" semitones)
BOUNDS = dict(cond=("ACOUSTIC_COND_TOL", 2e-5, "rel"), aux=("AUX_TOL", 2e-5, "rel"), mel=("SAMPLE_TOL", 2e-4, "one"),
              enc=("ENC_TOL", 2e-4, "rel"), dur_pred=("DUR_TOL", 5e-5, "one"), pitch_cond=("ENC_TOL", 2e-4, "rel"),
              base_pitch=("SMOOTH_BAR", 2.12e-5, "abs"), var_cond=("ENC_TOL", 2e-4, "rel"), x_pred=("SAMPLE_TOL", 2e-4, "one"),
              pitch_pred=("SAMPLE_TOL", 2e-4, "one"), xs_pred=("SAMPLE_TOL", 2e-4, "one"), out=("SAMPLE_TOL", 2e-4, "one"))

# fixture key -> floor, as the generator printed it; in the units of the quantity's bound.  No floor reaches half its bound (the
# largest: base_pitch 6.28e-6 of 2.12e-5 semitones, aux 8.55e-7 of 2e-5, dur_pred 1.05e-6 of 5e-5), so the 2 x floor rule raises
# no bound: every case runs under the bounds of tests/test_gpu_deploy.py as they stand.
FLOORS = {
    "lynx_reflow_cond": 2.65e-07, "lynx_reflow_aux": 5.11e-07, "lynx_reflow_s0": 3.14e-07, "lynx_reflow_s1": 4.43e-07,
    "lynx_ddpm_cosine_cond": 2.24e-07, "lynx_ddpm_cosine_aux": 8.55e-07, "lynx_ddpm_cosine_s0": 8.83e-07,
    "lynx_ddpm_cosine_s1": 9.53e-07, "lynx_ddpm_cosine_s2": 9.15e-07, "lynx_ddpm_cosine_s3": 1.39e-07,
    "wn_cosine_cond": 2.93e-07, "wn_cosine_s0": 4.26e-07, "wn_h32_m5_cond": 2.53e-07, "wn_h32_m5_aux": 4.46e-07,
    "wn_h32_m5_s0": 5.09e-07, "wn_h32_m5_s1": 2.47e-07, "alone_energy_cond": 1.32e-07, "alone_breathiness_cond": 1.58e-07,
    "alone_voicing_cond": 1.49e-07, "alone_tension_cond": 3.15e-07, "alone_key_shift_cond": 2.65e-07,
    "alone_speed_cond": 1.97e-07, "pairs_cond": 1.68e-07, "all_h96_cond": 1.85e-07, "lynx_ragged_i0_cond": 2.72e-07,
    "lynx_ragged_i0_aux": 3.85e-07, "lynx_ragged_i0_s0": 5.07e-07, "lynx_ragged_i1_cond": 2.36e-07,
    "lynx_ragged_i1_aux": 8.76e-08, "lynx_ragged_i1_s0": 1.96e-07, "lynx_ragged_i2_cond": 3.55e-07,
    "lynx_ragged_i2_aux": 5.25e-07, "lynx_ragged_i2_s0": 2.97e-07, "four_curves_enc": 2.7e-07,
    "four_curves_var_cond": 1.58e-07, "four_curves_xs_pred": 1.6e-07, "four_curves_out_energy": 1.94e-07,
    "four_curves_out_breathiness": 1.86e-07, "four_curves_out_voicing": 1.29e-07, "four_curves_out_tension": 5.13e-07,
    "two_late_enc": 2.82e-07, "two_late_var_cond": 1.59e-07, "two_late_xs_pred": 1.14e-07,
    "two_late_out_breathiness": 1.13e-07, "two_late_out_voicing": 1.22e-07, "lynx_pitch_dur_pred": 9.85e-07,
    "lynx_pitch_enc": 2.03e-07, "lynx_pitch_pitch_cond": 3.89e-07, "lynx_pitch_base_pitch": 6.28e-06,
    "lynx_pitch_x_pred": 4.75e-07, "lynx_pitch_pitch_pred": 7.78e-08, "lynx_variances_ddpm_enc": 2.44e-07,
    "lynx_variances_ddpm_var_cond": 1.55e-07, "lynx_variances_ddpm_xs_pred": 6.61e-07,
    "lynx_variances_ddpm_out_energy": 8.58e-07, "lynx_variances_ddpm_out_tension": 1.99e-06, "dur_wide_dur_pred": 4.61e-07,
    "dur_wide_enc": 1.95e-07, "lynx_ragged_var_i0_dur_pred": 1.05e-06, "lynx_ragged_var_i0_enc": 2.3e-07,
    "lynx_ragged_var_i0_pitch_cond": 3.57e-07, "lynx_ragged_var_i0_base_pitch": 6.01e-06,
    "lynx_ragged_var_i0_x_pred": 3.84e-07, "lynx_ragged_var_i0_pitch_pred": 9.46e-08, "lynx_ragged_var_i1_dur_pred": 7.14e-07,
    "lynx_ragged_var_i1_enc": 2.14e-07, "lynx_ragged_var_i1_pitch_cond": 1.63e-07, "lynx_ragged_var_i1_base_pitch": 1.2e-06,
    "lynx_ragged_var_i1_x_pred": 1.56e-07, "lynx_ragged_var_i1_pitch_pred": 3.8e-08, "lynx_ragged_var_i2_dur_pred": 4.48e-07,
    "lynx_ragged_var_i2_enc": 2.61e-07, "lynx_ragged_var_i2_pitch_cond": 2.22e-07, "lynx_ragged_var_i2_base_pitch": 2.68e-06,
    "lynx_ragged_var_i2_x_pred": 3.22e-07, "lynx_ragged_var_i2_pitch_pred": 9e-08,
}


def quantity_of(key, tag):
    """the BOUNDS entry of a fixture key of case `tag`"""
    q = key[len(tag) + 1:]
    if q[0] == "i" and q[1].isdigit():
        q = q.split("_", 1)[1]
    if q[0] == "s" and q[1:].isdigit():
        return "mel"
    return "out" if q.startswith("out_") else q


def bound_for(tag, key):
    """-> (bound, its unit, floor): the project's bound, or 2 x floor where the floor exceeds half of it"""
    _, tol, unit = BOUNDS[quantity_of(key, tag)]
    floor = FLOORS[key]
    if floor > tol / 2:
        tol = 2 * floor
    return tol, unit, floor


def scale_of(unit, want):
    """what a bound of `unit` multiplies: max |want|, max(1, that), or 1"""
    ref = float(np.abs(want).max())
    return {"rel": max(ref, 1e-30), "one": max(1.0, ref), "abs": 1.0}[unit]
