"""The cases of the encoder size suite: the FastSpeech2 acoustic encoder (dsd_encode), the token encoder and the duration
predictor (dsd_token_encode / dsd_predict_dur) at the edges of what dsd_encoder_create / dsd_token_encoder_create accept.
Shared by the generator of G21 (tests/golden/make_golden_encoder_sizes.py), the host tests (test_encoder_sizes_host.py) and
the GPU tests (test_gpu_encoder_sizes.py), so that all three build the same seeded weights and inputs (diffsinger_amd/synth.py).

Each case names the lines of encoder_kernels.hip / gemm.hip / api.hip it reaches (`reaches`).  Bounds: the acoustic encoder
2e-5 of the output range, the token encoder and the duration predictor 2e-4 of max |want| (max(1, .) for durations) - the
bounds of test_gpu_encoder.py and test_gpu_variance.py.  `floor`: the reference's own fp32 error against the float64 oracle
on the G21 form of the case, as make_golden_encoder_sizes.py prints it (the source of every figure below)."""
from collections import OrderedDict

import numpy as np

TOL_ACOUSTIC = 2e-5
TOL_TOKEN = 2e-4

ENC_HP = dict(hidden_size=256, enc_layers=1, enc_ffn_kernel_size=3, ffn_act="gelu", dropout=0.1, num_heads=2,
              use_pos_embed=True, rel_pos=True, use_rope=True, use_spk_id=False, num_spk=1, use_lang_id=False, num_lang=1)
VOCAB = 50
_REL = dict(use_rope=False, rel_pos=True)
_SIN = dict(use_rope=False, rel_pos=False)
_FULL_HP = dict(use_spk_id=True, num_spk=3, use_lang_id=True, num_lang=2, use_energy_embed=True, use_breathiness_embed=True,
                use_key_shift_embed=True, use_speed_embed=True)
_FULL_SKW = dict(num_spk=3, num_lang=2, variances=("energy", "breathiness"), key_shift=True, speed=True)


def _hp(hidden, heads, ks, act, layers, **kw):
    return dict(hidden_size=hidden, num_heads=heads, enc_ffn_kernel_size=ks, ffn_act=act, enc_layers=layers, **kw)


# tag: hp (over ENC_HP), skw (synth.fs2_acoustic_param_shapes arguments beyond the sizes), weight seed,
#      inputs [(tokens per item, frames per item)]: item 0 sets (L, T), item 1 is shorter
ACOUSTIC = OrderedDict(
    # smallest accepted model: D = 8; ffn k = 1 is a 1x1 GEMM (taps == 1: HL = 0, no halo) and K = 32 is no multiple of the
    # fast path's 64-row chunk: the generic walk; one row tile cut at 32 (o_proj, ffn_2: M = 32); L = 1 and L = 5
    h32_k1=dict(hp=_hp(32, 4, 1, "relu", 1), skw={}, wseed=2101, inputs=[([1], [3]), ([5, 3], [9, 6])]),
    # widest halo: HL = 8 per side (taps / 2 = 7 rounded to 4), L = 70: two key chunks, two LayerNorm column blocks
    h32_k15=dict(hp=_hp(32, 2, 15, "gelu", 1), skw={}, wseed=2102, inputs=[([70, 41], [150, 90])]),
    # K = 96: generic staging with kcn = 96 (one and a half 64-row chunks of the walk); 3H = 288 and 4H = 384 row tiles
    h96_k3=dict(hp=_hp(96, 4, 3, "gelu", 2), skw={}, wseed=2103, inputs=[([70, 41], [150, 90])]),
    # 8H = 768 rows of ffn_1, enc_swiglu_kernel at half = 384, ffn_2 reading the first 4H rows of an 8H-row buffer
    h96_swiglu=dict(hp=_hp(96, 2, 5, "swiglu", 1), skw=dict(ffn_act="swiglu"), wseed=2104, inputs=[([33], [40])]),
    # D = 80: the `dd` loop of enc_attention_kernel and the `qs` fill take a partial second pass (lanes 0..15)
    h160_d80=dict(hp=_hp(160, 2, 3, "swish", 2), skw={}, wseed=2105, inputs=[([65, 40], [130, 77])]),
    # enc_layernorm_kernel nper = 34: two iterations of each re-read loop, every wave active in both
    h544=dict(hp=_hp(544, 4, 3, "gelu", 1), skw={}, wseed=2106, inputs=[([65, 33], [100, 61])]),
    # nper = 48; K = 768 resident with a 4-column halo per side of a 32-frame tile: 768 * 48 * 4 = 147456 of 163840 bytes
    h768_k9=dict(hp=_hp(768, 8, 9, "gelu", 1), skw={}, wseed=2107, inputs=[([130, 100], [260, 190])]),
    # D = 256 (four passes of the P.V loop) with three heads; L = 64 is exactly one key chunk
    h768_d256=dict(hp=_hp(768, 3, 1, "relu", 1), skw={}, wseed=2108, inputs=[([64], [64])]),
    # pre-rotary layouts: enc_relpos_kernel / enc_sinpos_kernel at C = 96 and 544
    rel96=dict(hp=_hp(96, 2, 3, "gelu", 1, **_REL), skw=dict(rope=False), wseed=2109, inputs=[([40, 23], [80, 47])]),
    rel544=dict(hp=_hp(544, 4, 3, "gelu", 1, **_REL), skw=dict(rope=False), wseed=2110, inputs=[([40, 23], [80, 47])]),
    sin96=dict(hp=_hp(96, 2, 3, "gelu", 1, **_SIN), skw=dict(rope=False, sinpos=True), wseed=2111, inputs=[([40, 23], [80, 47])]),
    sin544=dict(hp=_hp(544, 4, 3, "gelu", 1, **_SIN), skw=dict(rope=False, sinpos=True), wseed=2112,
                inputs=[([40, 23], [80, 47])]),
    # every optional term of enc_embed_kernel / enc_expand_kernel at H = 96 (the `full` configuration of test_gpu_encoder.py)
    full96=dict(hp=_hp(96, 2, 3, "gelu", 1, **_FULL_HP), skw=_FULL_SKW, wseed=2113, inputs=[([40, 23], [80, 47])]),
    # the acceptance limits ("Encoder sizes"): what dsd_encoder_create accepts runs for every (B, L)
    h1024_k1=dict(hp=_hp(1024, 4, 1, "relu", 1), skw={}, wseed=2114, inputs=[([40], [60])]),
    h768_k15=dict(hp=_hp(768, 8, 15, "gelu", 1), skw={}, wseed=2115, inputs=[([40], [60])]),
    # the widest hidden size a k > 1 FFN conv can run at: 832 * 48 * 4 = 159744 of 163840 bytes
    h832_k3=dict(hp=_hp(832, 4, 3, "gelu", 1), skw={}, wseed=2116, inputs=[([40], [60])]),
)

# G21 holds these configurations on a small batch (outputs are [2, 40, H]: the fixture stays well under 1 MiB)
G21_ACOUSTIC = ("h96_k3", "h160_d80", "h544", "h768_k9")
G21_INPUT = ([24, 13], [40, 22])

# floors of the G21 forms, (tag, index into G21's <tag>_floor) -> value (make_golden_encoder_sizes.py prints
# "floor <tag> <output> <value>"; variance cases: enc, dur).  With --all the generator printed for the GPU inputs of ACOUSTIC:
# 1.1e-7 .. 3.6e-7 for the rotary and sinusoidal cases, rel96 5.97e-6 and rel544 2.57e-6 (fp32 angles near 4999 rad in
# RelPositionalEncoding) - every one below TOL_ACOUSTIC / 2, so no case needs the 2 x floor rule
FLOORS = {
    ("h96_k3", 0): 2.22e-07, ("h160_d80", 0): 2.55e-07, ("h544", 0): 2.58e-07, ("h768_k9", 0): 2.5e-07,
    ("d100", 0): 2.44e-07, ("d100", 1): 8.89e-07, ("d520", 0): 2.74e-07, ("d520", 1): 4.45e-07, ("melody96", 0): 3e-07,
}


def acoustic_hp(tag):
    hp = dict(ENC_HP)
    hp.update(ACOUSTIC[tag]["hp"])
    return hp


def acoustic_params(tag):
    from diffsinger_amd import synth
    hp, c = acoustic_hp(tag), ACOUSTIC[tag]
    shapes = synth.fs2_acoustic_param_shapes(VOCAB, hidden_size=hp["hidden_size"], enc_layers=hp["enc_layers"],
                                             num_heads=hp["num_heads"], ffn_kernel_size=hp["enc_ffn_kernel_size"], **c["skw"])
    return synth.synth_state_dict(shapes, seed=c["wseed"])


def padded_inputs(n_tok, n_fr, seed, vocab=VOCAB):
    """tests/test_gpu_encoder.py::padded_inputs at (L, T) = item 0's sizes."""
    from test_gpu_encoder import padded_inputs as make
    return make(list(n_tok), list(n_fr), max(n_tok), max(n_fr), seed, vocab)


def acoustic_inputs(tag, which):
    """-> tokens, mel2ph, f0, extras (the keyword inputs of the `full` configuration, else {}) of input `which` of a case;
    which = "g21": the small batch of the fixture."""
    c = ACOUSTIC[tag]
    n_tok, n_fr = G21_INPUT if which == "g21" else c["inputs"][which]
    seed = c["wseed"] * 10 + (9 if which == "g21" else which)
    tokens, mel2ph, f0 = padded_inputs(n_tok, n_fr, seed)
    extras = {}
    if c["skw"].get("num_spk"):
        rng = np.random.Generator(np.random.PCG64(seed + 100))
        bsz, t_mel = mel2ph.shape
        extras = dict(key_shift=rng.uniform(-5, 5, (bsz, t_mel)).astype(np.float32),
                      speed=rng.uniform(0.5, 2.0, (bsz, t_mel)).astype(np.float32),
                      energy=rng.uniform(-60, -10, (bsz, t_mel)).astype(np.float32),
                      breathiness=rng.uniform(-80, -20, (bsz, t_mel)).astype(np.float32),
                      languages=(rng.integers(1, 3, tokens.shape) * (tokens > 0)).astype(np.int64),
                      spk_embed_id=rng.integers(0, 3, (bsz,)).astype(np.int64))
    return tokens, mel2ph, f0, extras


def acoustic_oracle(tag, params, tokens, mel2ph, f0, extras):
    from oracle import encoder as oe
    hp = acoustic_hp(tag)
    pos = "rope" if hp["use_rope"] else ("rel" if hp["rel_pos"] else "sin")
    return oe.fs2_acoustic_forward(params, tokens, mel2ph, f0, num_heads=hp["num_heads"], pos=pos, ffn_act=hp["ffn_act"], **extras)


# ------------------------------------------------------------------------------------------------ token encoder, durations
def _dur(chans, layers, ks):
    return dict(arch="fs2", hidden_size=chans, dropout=0.1, num_layers=layers, kernel_size=ks, log_offset=1.0, loss_type="mse")


# tag: hidden, heads, duration predictor (channels, layers, kernel), item lengths (item 0 sets L), weight seed
VARIANCE = OrderedDict(
    # LayerNorm over one channel: (x - mean) = 0 exactly, the output is beta * mask as in torch; enc_dur_head_kernel at C = 1;
    # a k = 1 duration conv (no halo); the last item has a single real token
    d1=dict(hidden=64, heads=2, dur=(1, 1, 1), lens=(70, 41, 1), wseed=2201),
    # Kreal = 100 inside K = 112 for layers 1 and 2 (row_ok of the generic staging, the clamped channel read), the second
    # 64-row output tile cut at 36 rows, LayerNorm's `c < C` guard at C % 16 = 4 (nper = 7, waves 4..15 idle in the last round)
    d100=dict(hidden=96, heads=2, dur=(100, 3, 5), lens=(130, 77), wseed=2202),
    # LayerNorm nper = 33: one re-read iteration in which only waves 0..7 hold a channel (c = wave + 512 < 520)
    d520=dict(hidden=544, heads=4, dur=(520, 2, 3), lens=(65, 40), wseed=2203),
    # widest halo on the duration convs (HL = 8), K = 64 then 48
    dk15=dict(hidden=64, heads=2, dur=(48, 2, 15), lens=(70, 41), wseed=2204),
    # acceptance limit: K = 528 resident at k = 15 (528 * 48 * 4 = 101376 bytes)
    d520_k15=dict(hidden=64, heads=2, dur=(520, 2, 15), lens=(40,), wseed=2205),
)
G21_VARIANCE = ("d100", "d520")
G21_VARIANCE_LENS = (24, 13)
VAR_VOCAB = 30

# MelodyEncoder at hidden 96 inside a model of hidden 96 (out_proj: 96 -> 96)
MELODY = dict(hidden=96, heads=2, notes=(40, 23), wseed=2206)
G21_MELODY_NOTES = (24, 13)

# out_proj through the C ABI (hparams tie MelodyEncoder's out_dims to the model's hidden size): hidden 96, out_dims ->
# M = 1 and M = 30 (M % 4 != 0, one row tile cut at 1 / 30 rows), 4 * hidden = 384 (the e_mid buffer to its full extent)
OUT_DIMS = dict(hidden=96, heads=2, out_dims=(0, 1, 30, 384), lens=(70, 41, 1), wseed=2207)


def variance_hp(c, melody=False):
    import variance_cases as vc
    hp = dict(vc.ENC_HP)
    hp.update(hidden_size=c["hidden"], num_heads=c["heads"], enc_layers=1, diffusion_type="reflow")
    if melody:
        hp.update(predict_pitch=True, use_melody_encoder=True, use_glide_embed=True, sampling_algorithm="euler", sampling_steps=2,
                  melody_encoder_args=dict(hidden_size=c["hidden"], enc_layers=1))
    else:
        hp.update(predict_dur=True, dur_prediction_args=_dur(*c["dur"]))
    return hp


def variance_params(model, seed):
    """Seeded weights over the NAME-sorted parameters of a DiffSingerVariance (the reference's or diffsinger_amd's)."""
    import variance_cases as vc
    shapes = vc.sorted_param_shapes(model.named_parameters())
    return vc.synth_weights(shapes, seed)


def variance_inputs(lens, seed, vocab=VAR_VOCAB):
    """A zero-padded word-mode batch: tokens, midi, ph2word, word_dur."""
    rng = np.random.Generator(np.random.PCG64(seed))
    bsz, n_ph = len(lens), max(lens)
    tokens = rng.integers(1, vocab, (bsz, n_ph)).astype(np.int64)
    ph2word = np.zeros((bsz, n_ph), np.int64)
    for b, n in enumerate(lens):
        tokens[b, n:] = 0
        ph2word[b, :n] = np.cumsum(rng.random(n) < 0.4) + 1
    midi = rng.integers(30, 90, (bsz, n_ph)).astype(np.int64) * (tokens > 0)
    word_dur = rng.integers(1, 40, (bsz, int(ph2word.max()))).astype(np.int64)
    return tokens, midi, ph2word, word_dur


def melody_inputs(notes, seed):
    """note_midi (-1: padding), note_rest, note_dur, glide of a zero-padded batch of notes."""
    rng = np.random.Generator(np.random.PCG64(seed))
    bsz, n_note = len(notes), max(notes)
    note_midi = rng.uniform(48, 72, (bsz, n_note)).astype(np.float32)
    note_rest = rng.random((bsz, n_note)) < 0.25
    for b, n in enumerate(notes):
        note_midi[b, n:] = -1.0
    note_dur = rng.integers(1, 30, (bsz, n_note)).astype(np.int64) * (note_midi >= 0)
    glide = rng.integers(0, 3, (bsz, n_note)).astype(np.int64) * (note_midi >= 0)
    return note_midi, note_rest, note_dur, glide


def token_encoder_shapes(hidden, heads, ks=3, out_dims=0, dur=None):
    """The tensors dsd_token_encoder_create's handle loads, under the names of FastSpeech2Encoder / MelodyEncoder.out_proj /
    DurationPredictor (rotary configuration)."""
    from diffsinger_amd import synth
    full = synth.fs2_acoustic_param_shapes(2, hidden_size=hidden, enc_layers=1, num_heads=heads, ffn_kernel_size=ks)
    shapes = OrderedDict((k, v) for k, v in full.items() if k.startswith("encoder."))
    if out_dims:
        shapes["out_proj.weight"] = (out_dims, hidden)
        shapes["out_proj.bias"] = (out_dims,)
    if dur:
        chans, layers, kd = dur
        for l in range(layers):
            shapes[f"dur_predictor.conv.{l}.1.weight"] = (chans, hidden if l == 0 else chans, kd)
            shapes[f"dur_predictor.conv.{l}.1.bias"] = (chans,)
            shapes[f"dur_predictor.conv.{l}.3.weight"] = (chans,)
            shapes[f"dur_predictor.conv.{l}.3.bias"] = (chans,)
        shapes["dur_predictor.linear.weight"] = (1, chans)
        shapes["dur_predictor.linear.bias"] = (1,)
    return shapes


def token_oracle(params, embed, pad, heads, out_dims=0):
    """dsd_token_encode on a ready-made embedding: FastSpeech2Encoder on x = embed (main_embed = 0), then out_proj."""
    from oracle import encoder as oe
    enc = oe.fs2_encoder(params, np.zeros_like(embed), embed, pad, heads)
    if out_dims:
        enc = (enc @ params["out_proj.weight"].T + params["out_proj.bias"]).astype(np.float32)
    return enc


# ------------------------------------------------------------------------------------------------ what create refuses
# (DsdEncoderConfig / DsdTokenEncoderConfig field overrides, a fragment of dsd_last_error)
REJECT_ACOUSTIC = [
    (dict(hidden_size=48), "hidden_size must be a multiple of 32"),
    (dict(hidden_size=32, num_heads=3), "multiple of 32 and of 2 * num_heads"),
    (dict(hidden_size=32, num_heads=8), "head dimension must be a multiple of 8, at most 256"),
    (dict(hidden_size=544, num_heads=2), "head dimension must be a multiple of 8, at most 256"),
    (dict(ffn_kernel_size=4), "enc_ffn_kernel_size must be odd and <= 15"),
    (dict(ffn_kernel_size=17), "enc_ffn_kernel_size must be odd and <= 15"),
    (dict(struct_size=44), "struct_size 44 != 48"),
    # the LDS rule, decided at create time: a k > 1 FFN conv keeps all hidden_size input channels of a 32-frame tile resident
    (dict(hidden_size=1024, num_heads=4, ffn_kernel_size=15), "at most 832 with enc_ffn_kernel_size > 1"),
    (dict(hidden_size=864, num_heads=4, ffn_kernel_size=3), "at most 832 with enc_ffn_kernel_size > 1"),
]
REJECT_TOKEN = [
    (dict(hidden_size=48), "hidden_size must be a multiple of 32"),
    (dict(hidden_size=32, num_heads=3), "multiple of 32 and of 2 * num_heads"),
    (dict(hidden_size=32, num_heads=8), "head dimension must be a multiple of 8, at most 256"),
    (dict(hidden_size=544, num_heads=2), "head dimension must be a multiple of 8, at most 256"),
    (dict(ffn_kernel_size=4), "enc_ffn_kernel_size must be odd and <= 15"),
    (dict(ffn_kernel_size=17), "enc_ffn_kernel_size must be odd and <= 15"),
    (dict(dur_layers=2, dur_chans=64, dur_kernel_size=2), "odd kernel size <= 15"),
    (dict(dur_layers=2, dur_chans=64, dur_kernel_size=17), "odd kernel size <= 15"),
    (dict(dur_layers=2, dur_chans=0, dur_kernel_size=3), "channels >= 1"),
    (dict(hidden_size=64, out_dims=257), "out_dims above 4 * hidden_size"),
    (dict(struct_size=48), "struct_size 48 != 52"),
    (dict(hidden_size=1024, num_heads=4, ffn_kernel_size=15), "at most 832 with enc_ffn_kernel_size > 1"),
    (dict(dur_layers=2, dur_chans=900, dur_kernel_size=3), "at most 848 input channels"),
    (dict(hidden_size=1024, num_heads=4, ffn_kernel_size=1, dur_layers=1, dur_chans=64, dur_kernel_size=3),
     "at most 848 input channels"),
]
