"""What tests/test_cacoustic_host.py and tests/test_gpu_cacoustic.py share: the Python twin of a tests/deploy_cases.py
acoustic case (or of the seeded cases below) with its synthetic weights, packed into a model file under a prefix."""
import numpy as np
import torch

import deploy_cases as dc
from diffsinger_amd import modelfile
from diffsinger_amd.hparams import hparams

PREFIX = "ac"

# Beyond G22.  `batch`: every embedding the condition stage has, DDPM with shallow diffusion, B = 3 and padded (batch_inputs).
# `frozen`: the same model with the two frozen_* attributes set.  `ancestral`: DDPM, shallow, for depths whose speed-up is 1.
# `base10`: a reflow model whose mel is log10 (the default mel_base): the sampler stage ends in the in-place scale.
EXTRA_CASES = dict(
    batch=dict(hp=dict(use_shallow_diffusion=True, diffusion_type="ddpm", use_key_shift_embed=True, use_speed_embed=True,
                       use_energy_embed=True, use_tension_embed=True, use_spk_id=True, num_spk=2, use_lang_id=True, num_lang=2,
                       mel_base="e"),
               cross=[1, 4, 6], seed=2510),
    frozen=dict(hp=dict(use_shallow_diffusion=True, diffusion_type="reflow", use_key_shift_embed=True, use_speed_embed=True,
                        use_spk_id=True, num_spk=2, mel_base="e"),
                cross=None, seed=2520, frozen=True),
    ancestral=dict(hp=dict(use_shallow_diffusion=True, diffusion_type="ddpm", mel_base="e"), cross=None, seed=2530),
    base10=dict(hp=dict(use_shallow_diffusion=True, diffusion_type="reflow"), cross=None, seed=2540),
)
BATCH_SHAPE = dict(n_ph=6, t_len=70)


def case_hparams(tag):
    if tag in dc.AC_CASES:
        return dc.acoustic_hparams(tag), dc.AC_CASES[tag]
    c = EXTRA_CASES[tag]
    hp = dict(dc.BASE_HP)
    hp.update(dc.ACOUSTIC_HP)
    hp.update(c["hp"])
    base = dc.acoustic_hparams("aux_ddpm")
    hp["spec_min"], hp["spec_max"] = base["spec_min"], base["spec_max"]
    return hp, c


def build_model(tag, cuda):
    """-> (DiffSingerAcousticDeploy with the case's seeded weights, hparams of the case); hparams stay set to the case."""
    from diffsinger_amd.deploy import DiffSingerAcousticDeploy
    hp, c = case_hparams(tag)
    hparams.clear()
    hparams.update(hp, infer=True)
    model = DiffSingerAcousticDeploy(dc.VOCAB, dc.M_BINS, cross_lingual_token_idx=c.get("cross"))
    shapes = dc.sorted_param_shapes(model.named_parameters())
    res = model.load_state_dict({k: torch.from_numpy(v) for k, v in dc.synth_weights(shapes, c["seed"] + 1).items()}, strict=False)
    assert not res.unexpected_keys and not set(res.missing_keys) & set(shapes)
    model = model.eval()
    if c.get("frozen"):
        rng = np.random.Generator(np.random.PCG64(c["seed"] + 7))
        model.frozen_spk_embed = torch.from_numpy(rng.standard_normal((1, 1, dc.HIDDEN)).astype(np.float32))
        model.frozen_key_shift = torch.tensor([2.75], dtype=torch.float32)
    return (model.cuda() if cuda else model), hp


def pack(path, model, prefix=PREFIX, edit=None):
    """writes the model's sections (after `edit(sections)`, which may change the list in place) -> the sections"""
    sections = modelfile.acoustic_sections(prefix, model)
    if edit is not None:
        edit(sections)
    modelfile.write(path, sections, {"kind": "acoustic"})
    return sections


def batch_inputs(tag="batch"):
    """Seeded inputs of the padded batch, numpy, B = 3: item 0 fills every frame; item 1 has a padding token in the middle with
    a non-zero duration (masked away) and durations that total less than T (41 real frames); item 2 ends in two padding tokens
    and totals 57.  `lengths` holds the real frame counts."""
    hp, c = case_hparams(tag)
    n_ph, t_len = BATCH_SHAPE["n_ph"], BATCH_SHAPE["t_len"]
    rng = np.random.Generator(np.random.PCG64(c["seed"]))
    lens = np.array([t_len, 41, 57], dtype=np.int32)
    tokens = rng.integers(1, dc.VOCAB, (3, n_ph)).astype(np.int64)
    tokens[1, 2] = 0
    tokens[2, -2:] = 0
    durations = np.zeros((3, n_ph), dtype=np.int64)
    durations[0] = dc._split(rng, t_len, n_ph)
    durations[1, [0, 1, 3, 4, 5]] = dc._split(rng, int(lens[1]), 5)
    durations[1, 2] = 9                                                   # on a padding token: tokens > 0 masks it
    durations[2, :4] = dc._split(rng, int(lens[2]), 4)
    durations[2, 4] = 5                                                   # likewise
    out = dict(lengths=lens, tokens=tokens, durations=durations,
               f0=(220.0 * 2.0 ** rng.uniform(-1, 1, (3, t_len))).astype(np.float32),
               var_energy=rng.uniform(-60, -10, (3, t_len)).astype(np.float32),
               var_tension=rng.uniform(-5, 5, (3, t_len)).astype(np.float32),
               gender=rng.uniform(-1.3, 1.3, (3, t_len)).astype(np.float32),
               velocity=rng.uniform(0.3, 2.4, (3, t_len)).astype(np.float32),
               spk_one=rng.standard_normal((3, 1, dc.HIDDEN)).astype(np.float32),
               spk_frames=rng.standard_normal((3, t_len, dc.HIDDEN)).astype(np.float32),
               languages=rng.integers(1, hp["num_lang"] + 1, (3, n_ph)).astype(np.int64))
    out["f0"][:, 5:8] = 0.0
    return out
