"""What tests/test_cvariance_host.py and tests/test_gpu_cvariance.py share: the Python twin of a tests/deploy_cases.py
variance case (or of the seeded batch case below) with its synthetic weights, packed into a model file under a prefix."""
import numpy as np
import torch

import deploy_cases as dc
from diffsinger_amd import modelfile
from diffsinger_amd.hparams import hparams

PREFIX = "var"

# The seeded batch beyond G22: B = 3, padded.  Two models, so that both encoder forms, both pitch forms, a cross-lingual
# list that masks some tokens and an empty one are met; K = 5 (the default width).
BATCH_CASES = dict(
    word=dict(hp=dict(predict_dur=True, predict_pitch=True, use_melody_encoder=True, use_glide_embed=True, use_spk_id=True,
                      num_spk=2, use_lang_id=True, num_lang=2, predict_energy=True, predict_tension=True, diffusion_type="reflow"),
              cross=[2, 3, 5, 7], seed=2410),
    phoneme=dict(hp=dict(predict_pitch=True, use_spk_id=True, num_spk=2, use_lang_id=True, num_lang=2, predict_breathiness=True,
                         diffusion_type="reflow"),
                 cross=[], seed=2420),
)
BATCH_SHAPE = dict(n_ph=6, n_word=3, n_note=4, t_len=300)          # more than one 256-frame block


def library_taps(k):
    """The K smoothing taps as dsd_variance_open computes them (include/dsdenoise.h), restated: np.linspace(0, 1, K) rounded
    to fp32 times fp32 pi, the C library's double sine of that fp32 argument rounded to fp32, the sum added in double in
    order and rounded once, an fp32 division.  K = 1: 0 / 0."""
    import math
    x = np.linspace(0, 1, k).astype(np.float32) * np.float32(np.pi)
    w = np.array([math.sin(float(a)) for a in x], dtype=np.float64).astype(np.float32)
    total = 0.0
    for a in w:
        total += float(a)
    with np.errstate(invalid="ignore", divide="ignore"):
        return torch.from_numpy(w / np.float32(total))


def case_hparams(tag):
    if tag in dc.VAR_CASES:
        return dc.variance_hparams(tag), dc.VAR_CASES[tag]
    c = BATCH_CASES[tag]
    hp = dict(dc.BASE_HP)
    hp.update(dc.VARIANCE_HP)
    hp.update(c["hp"])
    return hp, c


def build_model(tag, cuda):
    """-> (DiffSingerVarianceDeploy with the case's seeded weights, hparams of the case); hparams stay set to the case."""
    from diffsinger_amd.deploy import DiffSingerVarianceDeploy
    hp, c = case_hparams(tag)
    hparams.clear()
    hparams.update(hp, infer=True)
    model = DiffSingerVarianceDeploy(dc.VOCAB, cross_lingual_token_idx=c.get("cross"))
    shapes = dc.sorted_param_shapes(model.named_parameters())
    res = model.load_state_dict({k: torch.from_numpy(v) for k, v in dc.synth_weights(shapes, c["seed"] + 1).items()}, strict=False)
    assert not res.unexpected_keys and not set(res.missing_keys) & set(shapes)
    model = model.eval()
    return (model.cuda() if cuda else model), hp


def pack(path, model, prefix=PREFIX, edit=None):
    """writes the model's sections (after `edit(sections)`, which may change the list in place) -> the sections"""
    sections = modelfile.variance_sections(prefix, model)
    if edit is not None:
        edit(sections)
    modelfile.write(path, sections, {"kind": "variance"})
    return sections


def batch_inputs(tag):
    """Seeded inputs of a batch case, numpy, B = 3 and padded: item 0 fills every length; item 1 has L = 1 real phoneme
    (the rest padding tokens with zero durations) and durations that total less than T; item 2 has a zero in word_div, a
    phoneme without frames and a padding token at its end."""
    hp, c = case_hparams(tag)
    s = BATCH_SHAPE
    n_ph, n_word, n_note, t_len = s["n_ph"], s["n_word"], s["n_note"], s["t_len"]
    rng = np.random.Generator(np.random.PCG64(c["seed"]))
    lens = np.array([t_len, 41, 257], dtype=np.int32)
    tokens = rng.integers(1, dc.VOCAB, (3, n_ph)).astype(np.int64)
    tokens[1, 1:] = 0
    tokens[2, -1] = 0
    word_div = np.array([[2, 2, 2], [1, 0, 0], [3, 0, 2]], dtype=np.int64)
    ph_dur = np.zeros((3, n_ph), dtype=np.int64)
    ph_dur[0] = dc._split(rng, t_len, n_ph)
    ph_dur[1, 0] = lens[1]
    ph_dur[2, :5] = dc._split(rng, int(lens[2]), 5)
    ph_dur[2, 0] += ph_dur[2, 1]
    ph_dur[2, 1] = 0
    word_dur = np.zeros((3, n_word), dtype=np.int64)
    for b in range(3):
        edges = np.concatenate([[0], np.cumsum(word_div[b])])
        word_dur[b] = [ph_dur[b, edges[i]:edges[i + 1]].sum() for i in range(n_word)]
    note_dur = np.zeros((3, n_note), dtype=np.int64)
    note_midi = rng.uniform(48, 72, (3, n_note)).astype(np.float32)
    for b, n in enumerate((4, 1, 3)):
        note_dur[b, :n] = dc._split(rng, int(lens[b]), n)
        note_midi[b, n:] = -1.0                                           # padding notes
    retake = rng.random((3, t_len)) < 0.5
    out = dict(lengths=lens, tokens=tokens, word_div=word_div, word_dur=word_dur, ph_dur=ph_dur,
               ph_midi=rng.integers(40, 80, (3, n_ph)).astype(np.int64),
               languages=rng.integers(1, hp["num_lang"] + 1, (3, n_ph)).astype(np.int64),
               spk_one=rng.standard_normal((3, 1, dc.HIDDEN)).astype(np.float32),
               spk_ph=rng.standard_normal((3, n_ph, dc.HIDDEN)).astype(np.float32),
               spk_frames=rng.standard_normal((3, t_len, dc.HIDDEN)).astype(np.float32),
               note_midi=note_midi, note_rest=rng.random((3, n_note)) < 0.25, note_dur=note_dur,
               note_glide=rng.integers(0, 3, (3, n_note)).astype(np.int64),
               pitch=(60.0 + 6.0 * np.sin(np.arange(t_len)[None] / 5.0) + rng.normal(0, 0.5, (3, t_len))).astype(np.float32),
               expr=rng.random((3, t_len)).astype(np.float32), retake=retake)
    names = dc.variance_names(hp)
    for n in names:
        lo, hi = (-5, 5) if n == "tension" else (-60, -10)
        out["var_" + n] = rng.uniform(lo, hi, (3, t_len)).astype(np.float32)
    out["var_retake"] = rng.random((3, t_len, len(names))) < 0.5
    for b in range(3):                      # a padded batch: frames past an item's length hold zeros
        for k in ["pitch", "expr", "retake", "var_retake"] + ["var_" + n for n in names]:
            out[k][b, lens[b]:] = 0
    return out
