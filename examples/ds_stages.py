#!/usr/bin/env python3
"""One `.ds` segment rendered stage by stage, the way an editor drives the exported variance model: linguistic encoder,
duration predictor, pitch pre-process / sampler / post-process, variance pre-process / sampler / post-process - then the
pitch of the middle third of the segment is re-rendered (`retake`) while the rest keeps the first pass, on the HIP library
only.

    python examples/ds_stages.py checkpoints/my_variance_exp song.ds [--segment 0] [--steps 10] [--seed 42]

The experiment needs `predict_dur` and `predict_pitch`; variance curves are rendered when the model predicts any.
"""
import argparse
import json
import pathlib

import torch

from diffsinger_amd import harness
from diffsinger_amd.deploy import DiffSingerVarianceDeploy
from diffsinger_amd.hparams import hparams, load_config
from diffsinger_amd.variance_harness import VarianceHarness


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("exp", type=pathlib.Path, help="experiment (work) directory")
    ap.add_argument("proj", type=pathlib.Path, help=".ds project")
    ap.add_argument("--segment", type=int, default=0)
    ap.add_argument("--ckpt", type=int, default=None, help="checkpoint step (default: the latest)")
    ap.add_argument("--steps", type=int, default=10, help="sampler steps of the pitch and variance stages")
    ap.add_argument("--seed", type=int, default=42)
    args = ap.parse_args()

    load_config(args.exp / "config.yaml", overrides=dict(infer=True, work_dir=str(args.exp)))
    dictionary = harness.load_phoneme_dictionary()
    spk_path = args.exp / "spk_map.json"
    spk_map = json.loads(spk_path.read_text(encoding="utf8")) if spk_path.exists() else {}
    model = DiffSingerVarianceDeploy(len(dictionary)).cuda().eval()
    print(f"| variance model: {harness.load_ckpt(model, args.exp, ckpt_steps=args.ckpt, prefix_in_ckpt='model', strict=True)}")
    assert model.predict_dur and model.predict_pitch, "this walk-through needs predict_dur and predict_pitch"
    # the harness turns the segment's text into the tensors an editor would hold: tokens, ph_num, notes, word durations
    h = VarianceHarness(model, dictionary, spk_map=spk_map, device="cuda")
    seg = harness.load_ds(args.proj)[args.segment]
    batch = h.preprocess_input(seg, idx=args.segment, verbose=True)
    tokens, note_dur = batch["tokens"], batch["note_dur"]
    word_div = torch.tensor([[int(v) for v in seg["ph_num"].split()]], device="cuda")
    t_len = batch["mel2note"].shape[1]
    ph_spk = spk = None
    if hparams["use_spk_id"]:                       # speaker mixes become plain embeddings, per token and per frame
        ph_spk = (model.spk_embed(batch["ph_spk_mix_id"]) * batch["ph_spk_mix_value"].unsqueeze(3)).sum(dim=2).detach()
        spk = (model.spk_embed(batch["spk_mix_id"]) * batch["spk_mix_value"].unsqueeze(3)).sum(dim=2).detach()
    gen = torch.Generator(device="cuda").manual_seed(args.seed)
    notes = dict(note_midi=batch["note_midi"], note_rest=batch["note_rest"], note_dur=note_dur, note_glide=batch["note_glide"])

    with torch.no_grad():
        enc, x_masks = model.forward_linguistic_encoder_word(tokens, word_div, batch["word_dur"])
        dur = model.forward_dur_predictor(enc, x_masks, batch["midi"], spk_embed=ph_spk)
        ph_dur = model.rr(dur, batch["ph2word"], batch["word_dur"])          # align to the words, as the editor does
        print(f"| durations: {ph_dur[0].tolist()} frames ({int(ph_dur.sum())} of {t_len})")

        def render_pitch(pitch, retake):
            cond, base = model.forward_pitch_preprocess(enc, ph_dur, pitch=pitch, retake=retake, spk_embed=spk, **notes)
            bins = model.pitch_predictor.repeat_bins
            x_t = torch.randn((1, 1, bins, t_len), device="cuda", generator=gen)
            return model.forward_pitch_postprocess(model.forward_pitch_reflow(cond, steps=args.steps, noise=x_t), base)

        everything = torch.ones((1, t_len), dtype=torch.bool, device="cuda")
        first = render_pitch(torch.zeros((1, t_len), device="cuda"), everything)
        middle = torch.zeros_like(everything)
        middle[:, t_len // 3: 2 * t_len // 3] = True
        second = render_pitch(first, middle)
        moved = (second - first).abs()
        print(f"| pitch: first pass {first.min():.2f}..{first.max():.2f} MIDI; retake of frames {t_len // 3}..{2 * t_len // 3}: "
              f"moved {moved[middle].max():.3f} inside, {moved[~middle].max():.3f} outside")
        if model.predict_variances:
            names = model.variance_prediction_list
            zeros = {n: torch.zeros((1, t_len), device="cuda") for n in names}
            cond = model.forward_variance_preprocess(enc, ph_dur, second, variances=zeros, spk_embed=spk,
                                                     retake=torch.ones((1, t_len, len(names)), dtype=torch.bool, device="cuda"))
            vp = model.variance_predictor
            x_t = torch.randn((1, vp.num_feats, vp.repeat_bins, t_len), device="cuda", generator=gen)
            curves = model.forward_variance_postprocess(model.forward_variance_reflow(cond, steps=args.steps, noise=x_t))
            for n, c in zip(names, curves):
                print(f"| {n}: {c.min():.2f}..{c.max():.2f}")
    print("| done")


if __name__ == "__main__":
    main()
