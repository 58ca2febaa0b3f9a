"""Configurations and seeded inputs of the G22 fixture (the staged entry points of the deployment twins,
deployment/modules/toplevel.py and fastspeech2.py), shared by tests/golden/make_golden_deploy.py (which runs the
reference's twins on them, on the CPU) and the host / GPU tests (which rebuild inputs and weights from the same seeds;
only the reference's outputs are stored).  Every case is as small as it can be and still go wrong: hidden size 64, two
encoder layers, two-layer denoisers, 2 or 3 sampler steps, one utterance per call as the twins are exported."""
from collections import OrderedDict

import numpy as np

HIDDEN = 64
NET = dict(num_layers=2, num_channels=64, dilation_cycle_length=2)
BASE_HP = dict(hidden_size=HIDDEN, enc_layers=2, enc_ffn_kernel_size=3, ffn_act="gelu", dropout=0.1, num_heads=2,
               use_pos_embed=True, rel_pos=True, use_rope=True, use_spk_id=False, num_spk=1, use_lang_id=False, num_lang=1,
               timesteps=1000, K_step=1000, time_scale_factor=1000, schedule_type="linear", max_beta=0.02,
               audio_sample_rate=44100, hop_size=512, midi_smooth_width=0.06)
VARIANCE_HP = dict(predict_dur=False, predict_pitch=False, predict_energy=False, predict_breathiness=False,
                   predict_voicing=False, predict_tension=False, use_melody_encoder=False, use_glide_embed=False,
                   glide_types=["up", "down"], glide_embed_scale=11.313708498984760,
                   energy_db_min=-96.0, energy_db_max=-12.0, breathiness_db_min=-96.0, breathiness_db_max=-20.0,
                   voicing_db_min=-96.0, voicing_db_max=-12.0, tension_logit_min=-10.0, tension_logit_max=10.0,
                   dur_prediction_args=dict(arch="fs2", hidden_size=48, dropout=0.1, num_layers=2, kernel_size=3,
                                            log_offset=1.0, loss_type="mse"),
                   melody_encoder_args=dict(hidden_size=32, enc_layers=2),
                   pitch_prediction_args=dict(pitd_norm_min=-8.0, pitd_norm_max=8.0, pitd_clip_min=-12.0, pitd_clip_max=12.0,
                                              repeat_bins=8, backbone_type="wavenet", backbone_args=NET),
                   variances_prediction_args=dict(total_repeat_bins=12, backbone_type="wavenet", backbone_args=NET))
VARIANCE_NAMES = ("energy", "breathiness", "voicing", "tension")        # param_adaptor.py:10

# ------------------------------------------------------------------------------------------------ the length regulator alone
LR_CASES = OrderedDict(
    one_token=dict(dur=[[5]]),
    zeros_inside=dict(dur=[[2, 0, 0, 3, 0, 1, 4]]),
    leading_zero=dict(dur=[[0, 2, 3]]),
    trailing_zero=dict(dur=[[2, 3, 0]]),
    all_in_one=dict(dur=[[0, 0, 7, 0]]),
    one_frame=dict(dur=[[0, 1, 0]]),                                  # T = 1
    ragged3=dict(dur=[[3, 1, 0, 4, 2], [1, 1, 1, 0, 0], [0, 6, 0, 0, 0]]),     # totals 10, 3, 6
    l2048=dict(seed=2200, n_tok=2048),                                # the encoders' limit: every lane scans 8 tokens
)


def lr_durations(tag):
    c = LR_CASES[tag]
    if "dur" in c:
        return np.array(c["dur"], dtype=np.int64)
    rng = np.random.Generator(np.random.PCG64(c["seed"]))
    return rng.integers(0, 4, (1, c["n_tok"])).astype(np.int64)


def length_regulate_numpy(dur, t_len):
    """LengthRegulator.forward (fastspeech2.py:31-40) restated: frame p holds i + 1 for cumsum[i - 1] <= p < cumsum[i]."""
    out = np.zeros((dur.shape[0], t_len), dtype=np.int64)
    for b, row in enumerate(dur):
        seq = np.repeat(np.arange(1, len(row) + 1), row)[:t_len]
        out[b, :len(seq)] = seq
    return out


# ------------------------------------------------------------------------------------------------ variance twin
# retake: 'all' true, 'none', or 'mixed'; glide / expr: given or None; width: midi_smooth_width (K = round(width * 44100 / hop))
VAR_CASES = OrderedDict(
    # word-level encoder + duration predictor, melody encoder with glides, expr curve, mixed retake, speaker + language; K = 5
    word_melody=dict(hp=dict(predict_dur=True, predict_pitch=True, use_melody_encoder=True, use_glide_embed=True,
                             use_spk_id=True, num_spk=2, use_lang_id=True, num_lang=2, diffusion_type="reflow"),
                     cross=[2, 3, 5, 7], glide=True, expr=True, retake="mixed", steps=3, n_ph=9, n_word=4, n_note=5,
                     t_len=37, seed=2210),
    # no melody encoder, retake everything, DDPM twin, hop 128: K = 21
    word_base=dict(hp=dict(predict_dur=True, predict_pitch=True, diffusion_type="ddpm", hop_size=128),
                   glide=False, expr=False, retake="all", steps=2, n_ph=7, n_word=3, n_note=4, t_len=45, seed=2220),
    # melody encoder with a glide embedding but no glides given, nothing retaken, an even K = 4
    melody_even=dict(hp=dict(predict_dur=True, predict_pitch=True, use_melody_encoder=True, use_glide_embed=True,
                             diffusion_type="reflow", midi_smooth_width=0.0464),
                     glide=False, expr=False, retake="none", steps=2, n_ph=6, n_word=3, n_note=4, t_len=23, seed=2230),
    # K = 1: the reference's single tap is sin(0) / sin(0), so its base pitch is NaN everywhere; the curve only
    k_one=dict(hp=dict(predict_pitch=True, diffusion_type="reflow", midi_smooth_width=0.0116),
               glide=False, expr=True, retake="mixed", steps=0, n_ph=5, n_word=2, n_note=3, t_len=11, seed=2240),
    # a clip shorter than K = 5: replicate padding covers every tap
    short_clip=dict(hp=dict(predict_pitch=True, use_melody_encoder=True, diffusion_type="reflow"),
                    glide=False, expr=False, retake="mixed", steps=2, n_ph=4, n_word=2, n_note=2, t_len=3, seed=2250),
    # variance stages: one variance, phoneme-level encoder
    var_one=dict(hp=dict(predict_energy=True, diffusion_type="reflow"),
                 steps=3, n_ph=8, n_word=3, n_note=0, t_len=29, seed=2260),
    # three variances, DDPM twin, speaker embedding
    var_three=dict(hp=dict(predict_energy=True, predict_voicing=True, predict_tension=True, use_spk_id=True, num_spk=2,
                           diffusion_type="ddpm"),
                   steps=2, n_ph=8, n_word=3, n_note=0, t_len=33, seed=2270),
)
VOCAB = 12


def variance_hparams(tag, cases=None):
    hp = dict(BASE_HP)
    hp.update(VARIANCE_HP)
    hp.update((cases or VAR_CASES)[tag]["hp"])
    return hp


def smooth_width(hp):
    return round(hp["midi_smooth_width"] * hp["audio_sample_rate"] / hp["hop_size"])


def variance_names(hp):
    return [n for n in VARIANCE_NAMES if hp.get("predict_" + n)]


def _split(rng, total, parts):
    """`parts` non-negative integers summing to `total`; every part >= 1 when total allows, zeros otherwise."""
    floor = 1 if total >= 2 * parts else 0
    return (rng.multinomial(total - floor * parts, np.ones(parts) / parts) + floor).astype(np.int64)


def variance_inputs(tag, cases=None):
    """Seeded stage inputs of a variance case: a dict of numpy arrays (B = 1).  `cases`: another table of the same form
    (tests/twin_config_cases.py), VAR_CASES when left out."""
    c, hp = (cases or VAR_CASES)[tag], variance_hparams(tag, cases)
    rng = np.random.Generator(np.random.PCG64(c["seed"]))
    n_ph, n_word, t_len = c["n_ph"], c["n_word"], c["t_len"]
    out = dict(tokens=rng.integers(1, VOCAB, (1, n_ph)).astype(np.int64))
    word_div = _split(rng, n_ph, n_word)
    ph_dur = _split(rng, t_len, n_ph)
    if t_len >= 2 * n_ph:                                             # a phoneme with no frames of its own
        k = int(rng.integers(1, n_ph))
        ph_dur[k - 1] += ph_dur[k]
        ph_dur[k] = 0
    word_dur = np.add.reduceat(ph_dur, np.concatenate([[0], np.cumsum(word_div)[:-1]]))
    out.update(word_div=word_div[None], ph_dur=ph_dur[None], word_dur=word_dur[None].astype(np.int64),
               ph_midi=rng.integers(40, 80, (1, n_ph)).astype(np.int64))
    if hp["use_lang_id"]:
        out["languages"] = rng.integers(1, hp["num_lang"] + 1, (1, n_ph)).astype(np.int64)
    if hp["use_spk_id"]:
        out["spk_embed"] = rng.standard_normal((1, 1, hp["hidden_size"])).astype(np.float32)
    out["pitch"] = (60.0 + 6.0 * np.sin(np.arange(t_len)[None] / 5.0) + rng.normal(0, 0.5, (1, t_len))).astype(np.float32)
    if hp["predict_pitch"]:
        n_note = c["n_note"]
        out["note_midi"] = rng.uniform(48, 72, (1, n_note)).astype(np.float32)
        out["note_rest"] = rng.random((1, n_note)) < 0.25
        out["note_dur"] = _split(rng, t_len, n_note)[None]
        if c["glide"]:
            out["note_glide"] = rng.integers(0, 3, (1, n_note)).astype(np.int64)
        if c["expr"]:
            out["expr"] = rng.random((1, t_len)).astype(np.float32)
        retake = np.zeros((1, t_len), dtype=bool)
        if c["retake"] == "all":
            retake[:] = True
        elif c["retake"] == "mixed":
            retake[:, t_len // 3: max(2 * t_len // 3, t_len // 3 + 1)] = True
        out["retake"] = retake
    names = variance_names(hp)
    if names:
        for n in names:
            lo, hi = (-5, 5) if n == "tension" else (-60, -10)
            out["var_" + n] = rng.uniform(lo, hi, (1, t_len)).astype(np.float32)
        out["var_retake"] = rng.random((1, t_len, len(names))) < 0.5
    return out


def variance_noise_shapes(tag, cases=None):
    """x_T shapes of the case's samplers, in the order the stages draw them: pitch first, then the variances."""
    c, hp = (cases or VAR_CASES)[tag], variance_hparams(tag, cases)
    shapes = {}
    if hp["predict_pitch"] and c["steps"]:
        shapes["pitch"] = (1, 1, hp["pitch_prediction_args"]["repeat_bins"], c["t_len"])
    names = variance_names(hp)
    if names:
        shapes["variance"] = (1, len(names), hp["variances_prediction_args"]["total_repeat_bins"] // len(names), c["t_len"])
    return shapes


# ------------------------------------------------------------------------------------------------ acoustic twin
M_BINS = 16
AUX_ARGS = dict(num_channels=32, num_layers=2, kernel_size=7, dropout_rate=0.1)
ACOUSTIC_HP = dict(use_energy_embed=False, use_breathiness_embed=False, use_voicing_embed=False, use_tension_embed=False,
                   use_key_shift_embed=False, use_speed_embed=False, use_shallow_diffusion=False,
                   backbone_type="wavenet", backbone_args=NET, T_start=0.4, K_step=400,
                   augmentation_args=dict(random_pitch_shifting=dict(range=[-5.0, 5.0]),
                                          random_time_stretching=dict(range=[0.5, 2.0])),
                   shallow_diffusion_args=dict(aux_decoder_arch="convnext", aux_decoder_args=AUX_ARGS, val_gt_start=False,
                                               train_aux_decoder=True, train_diffusion=True, aux_decoder_grad=0.1))
# stages: (name, depth or None) run after forward_fs2_aux; depth None = the full stage
AC_CASES = OrderedDict(
    aux_ddpm=dict(hp=dict(use_shallow_diffusion=True, diffusion_type="ddpm"),
                  stages=[("forward_shallow_diffusion", 0.3), ("forward_diffusion", None)], steps=3, seed=2300),
    aux_reflow=dict(hp=dict(use_shallow_diffusion=True, diffusion_type="reflow"),
                    stages=[("forward_shallow_reflow", 0.5), ("forward_reflow", None)], steps=3, seed=2310),
    plain_ddpm=dict(hp=dict(diffusion_type="ddpm", K_step=1000), stages=[("forward_diffusion", None)], steps=2, seed=2320),
    # gender -> key shift, velocity -> speed, a variance embedding, speaker embedding, the language mask
    gender_velocity=dict(hp=dict(diffusion_type="reflow", use_key_shift_embed=True, use_speed_embed=True,
                                 use_energy_embed=True, use_spk_id=True, num_spk=2, use_lang_id=True, num_lang=2),
                         cross=[1, 4, 6], stages=[], steps=0, seed=2330),
    # the legacy f0 embedding: an Embedding(300, H) over f0_to_coarse
    discrete_f0=dict(hp=dict(diffusion_type="reflow", f0_embed_type="discrete"), stages=[], steps=0, seed=2340),
)
AC_SHAPE = dict(n_ph=7, t_len=41)


def acoustic_hparams(tag):
    hp = dict(BASE_HP)
    hp.update(ACOUSTIC_HP)
    hp.update(AC_CASES[tag]["hp"])
    rng = np.random.Generator(np.random.PCG64(99))
    hp["spec_min"] = (-12.0 + rng.random(M_BINS)).round(3).tolist()
    hp["spec_max"] = (0.0 + rng.random(M_BINS)).round(3).tolist()
    return hp


def acoustic_inputs(tag):
    c, hp = AC_CASES[tag], acoustic_hparams(tag)
    rng = np.random.Generator(np.random.PCG64(c["seed"]))
    n_ph, t_len = AC_SHAPE["n_ph"], AC_SHAPE["t_len"]
    tokens = rng.integers(1, VOCAB, (1, n_ph)).astype(np.int64)
    tokens[0, -1] = 0                                                 # a padding token: its duration is masked away
    durations = np.append(_split(rng, t_len, n_ph - 1), 3)            # the reference needs sum(masked durations) == T
    out = dict(tokens=tokens, durations=durations[None],
               f0=(220.0 * 2.0 ** rng.uniform(-1, 1, (1, t_len))).astype(np.float32))
    out["f0"][0, 5:8] = 0.0                                           # unvoiced frames
    if hp["use_energy_embed"]:
        out["var_energy"] = rng.uniform(-60, -10, (1, t_len)).astype(np.float32)
    if hp["use_key_shift_embed"]:
        out["gender"] = rng.uniform(-1.3, 1.3, (1, t_len)).astype(np.float32)     # beyond [-1, 1]: clipped
    if hp["use_speed_embed"]:
        out["velocity"] = rng.uniform(0.3, 2.4, (1, t_len)).astype(np.float32)    # beyond [0.5, 2]: clipped
    if hp["use_spk_id"]:
        out["spk_embed"] = rng.standard_normal((1, t_len, HIDDEN)).astype(np.float32)
    if hp["use_lang_id"]:
        out["languages"] = rng.integers(1, hp["num_lang"] + 1, (1, n_ph)).astype(np.int64)
    return out


# ------------------------------------------------------------------------------------------------ weights
def sorted_param_shapes(named_parameters):
    return OrderedDict(sorted((n, tuple(int(s) for s in p.shape)) for n, p in named_parameters))


def synth_weights(shapes, seed):
    """The G12 recipe (tests/variance_cases.py): seeded normals, the Linear(1, H) embeddings of large inputs scaled down."""
    import variance_cases as vc
    sd = vc.synth_weights(shapes, seed)
    for name, w in sd.items():
        if name.endswith(("fs2.dur_embed.weight", "key_shift_embed.weight", "speed_embed.weight")):
            sd[name] = (w * np.float32(0.05)).astype(np.float32)
    return sd
