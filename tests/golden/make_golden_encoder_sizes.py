"""Generator of G21 (tests/golden/g21_encoder_sizes.npz): the reference's own FastSpeech2Acoustic (modules/fastspeech/
acoustic_encoder.py), FastSpeech2Variance with its DurationPredictor and MelodyEncoder (modules/fastspeech/variance_encoder.py,
through DiffSingerVariance) at hidden sizes and predictor widths that are not multiples of 64, run in fp32 on the CPU with the
seeded weights and inputs of tests/encoder_size_cases.py.  Only outputs, weight digests and floors are stored.

The floor of an output is the reference's fp32 result against the numpy oracle evaluated in float64 on the same weights and
inputs (every `F32` of oracle/{backbones,encoder,variance}.py replaced by float64), max |difference| over max |float64 result|:
how far fp32 arithmetic alone moves this output.  One line per output is printed as "floor <tag> <output> <value>"; with --all the
floors of every acoustic GPU case of encoder_size_cases.ACOUSTIC are printed too (nothing more is stored).

Runs on a machine with the reference tree; the tests only read the .npz.  `lightning` (imported by utils/training_utils.py, never
executed on this path) is stubbed.

    python tests/golden/make_golden_encoder_sizes.py /path/to/reference [--all]
"""
import contextlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import encoder_size_cases as ec  # noqa: E402
from diffsinger_amd import synth  # noqa: E402
from make_golden_width import _stub_lightning, to_t  # noqa: E402


@contextlib.contextmanager
def oracle_in_float64():
    from oracle import backbones, encoder, variance
    mods = (backbones, encoder, variance)
    try:
        for m in mods:
            m.F32 = np.float64
        yield
    finally:
        for m in mods:
            m.F32 = np.float32


def f64(params):
    return {k: np.asarray(v, np.float64) for k, v in params.items()}


def floor_of(ref32, want64):
    want64 = np.asarray(want64, np.float64)
    assert want64.dtype == np.float64 and ref32.shape == want64.shape
    return float(np.abs(np.asarray(ref32, np.float64) - want64).max() / max(np.abs(want64).max(), 1e-30))


def main(ref_root, all_cases):
    _stub_lightning()
    sys.path.insert(0, ref_root)
    from utils.hparams import hparams
    from modules.fastspeech.acoustic_encoder import FastSpeech2Acoustic
    from modules.toplevel import DiffSingerVariance
    from oracle import variance as ovar
    torch.set_num_threads(8)

    def set_hp(hp):
        hparams.clear()
        hparams.update(hp, infer=True)

    out = {}

    def acoustic(tag, which):
        set_hp(ec.acoustic_hp(tag))
        m = FastSpeech2Acoustic(ec.VOCAB)
        params = ec.acoustic_params(tag)
        m.load_state_dict({k: to_t(v) for k, v in params.items()}, strict=True)
        m.eval()
        tokens, mel2ph, f0, extras = ec.acoustic_inputs(tag, which)
        with torch.no_grad():
            cond = m(to_t(tokens), to_t(mel2ph), to_t(f0), **{k: to_t(v) for k, v in extras.items()}).numpy()
        with oracle_in_float64():
            want = ec.acoustic_oracle(tag, f64(params), tokens, mel2ph, f0.astype(np.float64),
                                      {k: (v.astype(np.float64) if v.dtype == np.float32 else v) for k, v in extras.items()})
        fl = floor_of(cond, want)
        print(f"floor {tag} {'cond' if which == 'g21' else 'cond[%d]' % which} {fl:.3g}   (shape {cond.shape}, absmax {np.abs(cond).max():.3f})")
        return params, cond, fl

    for tag in ec.G21_ACOUSTIC:
        params, cond, fl = acoustic(tag, "g21")
        out[f"{tag}_digest"] = np.array(synth.state_dict_digest(params))
        out[f"{tag}_cond"] = cond
        out[f"{tag}_floor"] = np.array([fl])
    if all_cases:
        for tag, c in ec.ACOUSTIC.items():
            for which in range(len(c["inputs"])):
                acoustic(tag, which)

    for tag in ec.G21_VARIANCE:
        c = ec.VARIANCE[tag]
        hp = ec.variance_hp(c)
        set_hp(hp)
        model = DiffSingerVariance(ec.VAR_VOCAB)
        params = ec.variance_params(model, c["wseed"])
        model.load_state_dict({k: to_t(v) for k, v in params.items()}, strict=False)
        model.eval()
        tokens, midi, ph2word, word_dur = ec.variance_inputs(ec.G21_VARIANCE_LENS, c["wseed"] + 50)
        with torch.no_grad():
            enc, dur = model.fs2(to_t(tokens), midi=to_t(midi), ph2word=to_t(ph2word), word_dur=to_t(word_dur), infer=True)
        enc, dur = enc.numpy(), dur.numpy()
        with oracle_in_float64():
            w_enc, w_dur = ovar.fs2_variance_forward(f64(ovar.sub(params, "fs2.")), hp, tokens, midi, ph2word, word_dur=word_dur)
        fl_e = floor_of(enc, w_enc)
        fl_d = float(np.abs(dur - w_dur).max() / max(1.0, np.abs(w_dur).max()))
        print(f"floor {tag} enc {fl_e:.3g}   (shape {enc.shape}, absmax {np.abs(enc).max():.3f})")
        print(f"floor {tag} dur {fl_d:.3g}   (max {dur.max():.3f})")
        out[f"{tag}_digest"] = np.array(synth.state_dict_digest(params))
        out[f"{tag}_enc"], out[f"{tag}_dur"] = enc, dur
        out[f"{tag}_floor"] = np.array([fl_e, fl_d])

    c = ec.MELODY
    hp = ec.variance_hp(c, melody=True)
    set_hp(hp)
    model = DiffSingerVariance(ec.VAR_VOCAB)
    params = ec.variance_params(model, c["wseed"])
    model.load_state_dict({k: to_t(v) for k, v in params.items()}, strict=False)
    model.eval()
    note_midi, note_rest, note_dur, glide = ec.melody_inputs(ec.G21_MELODY_NOTES, c["wseed"] + 50)
    with torch.no_grad():
        mel = model.melody_encoder(to_t(note_midi), to_t(note_rest), to_t(note_dur), glide=to_t(glide)).numpy()
    with oracle_in_float64():
        want = ovar.melody_encoder(f64(ovar.sub(params, "melody_encoder.")), hp, note_midi.astype(np.float64), note_rest, note_dur,
                                   glide=glide)
    fl = floor_of(mel, want)
    print(f"floor melody96 out {fl:.3g}   (shape {mel.shape}, absmax {np.abs(mel).max():.3f})")
    out["melody96_digest"] = np.array(synth.state_dict_digest(params))
    out["melody96_out"] = mel
    out["melody96_floor"] = np.array([fl])

    path = os.path.join(HERE, "g21_encoder_sizes.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main(sys.argv[1], "--all" in sys.argv[2:])
