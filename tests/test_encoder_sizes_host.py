"""The encoder family at sizes that are not multiples of 64, without a GPU.

G21 (tests/golden/g21_encoder_sizes.npz, generator make_golden_encoder_sizes.py) holds the reference's own fp32 output of
FastSpeech2Acoustic at hidden 96 / 160 / 544 / 768, of FastSpeech2Variance with duration predictors of 100 and 520 channels and
of MelodyEncoder at hidden 96.  The numpy oracle is checked against it at the levels tests/test_oracle_golden.py uses for G8 /
G12, which pins oracle/encoder.py and oracle/variance.py at these sizes: tests/test_gpu_encoder_sizes.py uses them as its
reference.

The boundary: dsd_encoder_create / dsd_token_encoder_create validate before they select a device, so everything they refuse -
the size rules and the LDS rule of the k-tap convolutions - is checked here too."""
import ctypes as C
import os

import numpy as np
import pytest

import encoder_size_cases as ec
from diffsinger_amd import synth
from oracle import variance as ovar

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load():
    return np.load(os.path.join(GOLDEN, "g21_encoder_sizes.npz"))


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.mark.parametrize("tag", ec.G21_ACOUSTIC)
def test_g21_oracle_acoustic_encoder(tag):
    g = load()
    params = ec.acoustic_params(tag)
    assert synth.state_dict_digest(params) == str(g[f"{tag}_digest"])
    tokens, mel2ph, f0, extras = ec.acoustic_inputs(tag, "g21")
    assert (tokens == 0).any() and (mel2ph == 0).any()
    cond = ec.acoustic_oracle(tag, params, tokens, mel2ph, f0, extras)
    err = rel_err(cond, g[f"{tag}_cond"])
    print(f"G21 {tag}: oracle vs reference {err:.3g} (floor {float(g[f'{tag}_floor'][0]):.3g})")
    assert err < 2e-5, (tag, err)


def _variance_model(c, melody=False):
    from diffsinger_amd.hparams import hparams
    from diffsinger_amd.variance import DiffSingerVariance
    hp = ec.variance_hp(c, melody=melody)
    hparams.clear()
    hparams.update(hp, infer=True)
    model = DiffSingerVariance(ec.VAR_VOCAB)
    return hp, ec.variance_params(model, c["wseed"])


@pytest.mark.parametrize("tag", ec.G21_VARIANCE)
def test_g21_oracle_variance_encoder_and_durations(tag):
    g = load()
    c = ec.VARIANCE[tag]
    hp, params = _variance_model(c)
    assert synth.state_dict_digest(params) == str(g[f"{tag}_digest"])
    assert params["fs2.dur_predictor.conv.1.1.weight"].shape == (c["dur"][0], c["dur"][0], c["dur"][2])
    tokens, midi, ph2word, word_dur = ec.variance_inputs(ec.G21_VARIANCE_LENS, c["wseed"] + 50)
    enc, dur = ovar.fs2_variance_forward(ovar.sub(params, "fs2."), hp, tokens, midi, ph2word, word_dur=word_dur)
    e_enc = rel_err(enc, g[f"{tag}_enc"])
    want = g[f"{tag}_dur"]
    e_dur = float(np.abs(dur - want).max() / max(1.0, np.abs(want).max()))
    print(f"G21 {tag}: oracle vs reference enc {e_enc:.3g} dur {e_dur:.3g} (floors {g[f'{tag}_floor'].tolist()})")
    assert (want > 0).any()             # the predictor is not clamped to zero everywhere
    assert e_enc < 2e-5 and e_dur < 2e-5, (tag, e_enc, e_dur)


def test_g21_oracle_melody_encoder():
    g = load()
    c = ec.MELODY
    hp, params = _variance_model(c, melody=True)
    assert synth.state_dict_digest(params) == str(g["melody96_digest"])
    note_midi, note_rest, note_dur, glide = ec.melody_inputs(ec.G21_MELODY_NOTES, c["wseed"] + 50)
    out = ovar.melody_encoder(ovar.sub(params, "melody_encoder."), hp, note_midi, note_rest, note_dur, glide=glide)
    err = rel_err(out, g["melody96_out"])
    print(f"G21 melody96: oracle vs reference {err:.3g} (floor {float(g['melody96_floor'][0]):.3g})")
    assert err < 2e-5, err


def test_floors_in_the_case_table_are_the_generators():
    g = load()
    for key, val in ec.FLOORS.items():
        tag, k = key
        assert float(g[f"{tag}_floor"][k]) == pytest.approx(val, rel=5e-3), key


# --------------------------------------------------------------------------- the boundary
def acoustic_cfg(_lib, **kw):
    f = dict(struct_size=C.sizeof(_lib.DsdEncoderConfig), vocab_size=50, hidden_size=64, enc_layers=1, num_heads=2,
             ffn_kernel_size=3, num_spk=0, num_lang=0, embed_flags=0, pos_mode=_lib.POS_ROPE, device=0, ffn_act=0)
    f.update(kw)
    return _lib.DsdEncoderConfig(**f)


def token_cfg(_lib, **kw):
    f = dict(struct_size=C.sizeof(_lib.DsdTokenEncoderConfig), hidden_size=64, enc_layers=1, num_heads=2, ffn_kernel_size=3,
             out_dims=0, dur_layers=0, dur_chans=0, dur_kernel_size=0, dur_offset=1.0, pos_mode=_lib.POS_ROPE, device=0, ffn_act=0)
    f.update(kw)
    return _lib.DsdTokenEncoderConfig(**f)


_SENTINEL = 0x5A5A5A5A


def _rejected(create, cfg, fragment, _lib):
    h = C.c_void_p(_SENTINEL)
    rc = create(C.byref(cfg), C.byref(h))
    msg = _lib.lib().dsd_last_error(None).decode()
    assert rc != 0, f"accepted; expected an error with {fragment!r}"
    assert h.value == _SENTINEL, "*out was written on a failed create"
    assert fragment in msg, (fragment, msg)


@pytest.mark.parametrize("over,fragment", ec.REJECT_ACOUSTIC, ids=[str(sorted(o.items())) for o, _ in ec.REJECT_ACOUSTIC])
def test_encoder_create_rejects(over, fragment):
    from diffsinger_amd import _lib
    _rejected(_lib.lib().dsd_encoder_create, acoustic_cfg(_lib, **over), "dsd_encoder_create: ", _lib)
    _rejected(_lib.lib().dsd_encoder_create, acoustic_cfg(_lib, **over), fragment, _lib)


@pytest.mark.parametrize("over,fragment", ec.REJECT_TOKEN, ids=[str(sorted(o.items())) for o, _ in ec.REJECT_TOKEN])
def test_token_encoder_create_rejects(over, fragment):
    from diffsinger_amd import _lib
    _rejected(_lib.lib().dsd_token_encoder_create, token_cfg(_lib, **over), "dsd_token_encoder_create: ", _lib)
    _rejected(_lib.lib().dsd_token_encoder_create, token_cfg(_lib, **over), fragment, _lib)


ACCEPTED = [
    ("acoustic", dict(hidden_size=32, num_heads=4, ffn_kernel_size=1)),
    ("acoustic", dict(hidden_size=832, num_heads=4, ffn_kernel_size=15)),
    ("acoustic", dict(hidden_size=1024, num_heads=4, ffn_kernel_size=1)),
    ("token", dict(hidden_size=96, out_dims=384)),
    ("token", dict(dur_layers=1, dur_chans=1, dur_kernel_size=1)),
    ("token", dict(dur_layers=2, dur_chans=848, dur_kernel_size=15)),
    ("token", dict(dur_layers=1, dur_chans=4000, dur_kernel_size=3)),          # one layer: nothing reads dur_chans channels
    ("token", dict(hidden_size=1024, num_heads=4, ffn_kernel_size=1, dur_layers=2, dur_chans=2000, dur_kernel_size=1)),
]


@pytest.mark.parametrize("kind,over", ACCEPTED, ids=[f"{k}-{sorted(o.items())}" for k, o in ACCEPTED])
def test_sizes_at_the_limits_get_past_validation(kind, over):
    """Without a GPU "past validation" is the no-device failure; with one, a handle."""
    import torch
    from diffsinger_amd import _lib
    lib = _lib.lib()
    h = C.c_void_p()
    if kind == "acoustic":
        rc = lib.dsd_encoder_create(C.byref(acoustic_cfg(_lib, **over)), C.byref(h))
    else:
        rc = lib.dsd_token_encoder_create(C.byref(token_cfg(_lib, **over)), C.byref(h))
    if torch.cuda.is_available():
        assert rc == 0, lib.dsd_last_error(None)
        lib.dsd_destroy(h)
    else:
        assert rc < 0 and b"no HIP device" in lib.dsd_last_error(None), lib.dsd_last_error(None)
