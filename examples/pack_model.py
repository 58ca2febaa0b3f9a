#!/usr/bin/env python3
"""A trained acoustic experiment and an NSF-HiFiGAN vocoder -> ONE model file that a process without Python opens
(include/dsdenoise.h: dsd_model_open, dsd_model_create; examples/c_abi_model.c reads one).

    python examples/pack_model.py checkpoints/my_exp nsf_hifigan/model.ckpt -o my_voice.dsdm [--ckpt 160000] [--twin ac]
                                  [--variance checkpoints/my_variance_exp [--variance-prefix var] [--variance-ckpt N]]

checkpoints/my_exp holds what a training run leaves there: config.yaml, model_ckpt_steps_<N>.ckpt, dictionary-<lang>.txt
(or dictionary.txt); config.json lies beside the vocoder checkpoint.  Sections written: "encoder" (the FastSpeech2
acoustic encoder), "denoiser" (the WaveNet / LYNXNet backbone), "aux_decoder" (with shallow diffusion), "vocoder", "mel"
(the analysis that matches the vocoder).  Metadata: what a caller needs besides weights - the diffusion schedule's sizes,
spec_min / spec_max, hop size, sample rate, the phoneme list - as plain strings (numbers in decimal, lists space-separated).
`--variance` adds a variance experiment (the same layout) under a prefix, as dsd_variance_open looks for it
(examples/c_abi_variance.c drives one): "<prefix>.tables" - the embedding tables of the staged twin, its constants and the
mask of the dictionary's cross-lingual phonemes - and "<prefix>.fs2", ".melody", ".pitch", ".variances", the inner handles.
`--twin PREFIX` writes the acoustic experiment once more as dsd_acoustic_open looks for it (examples/c_abi_acoustic.c
drives one): "<prefix>.tables" - the staged twin's constants, spec_min / spec_max and the cross-lingual mask - and
"<prefix>.fs2", ".aux", ".denoiser"; without it the output is what it was.
Needs no GPU: the wrappers are built on the CPU and only their parameters are read.
"""
import argparse
import pathlib

from diffsinger_amd import harness, modelfile
from diffsinger_amd.hparams import hparams, load_config
from diffsinger_amd.mel import STFT
from diffsinger_amd.toplevel import DiffSingerAcoustic


def _numbers(values):
    return " ".join(repr(float(v)) for v in values)


def variance_sections(exp, prefix, ckpt_steps):
    """the sections of a variance experiment's staged twin; hparams are the variance experiment's afterwards"""
    from diffsinger_amd.deploy import DiffSingerVarianceDeploy
    load_config(exp / "config.yaml", overrides=dict(infer=True, work_dir=str(exp)))
    dictionary = harness.load_phoneme_dictionary()
    cross = sorted({dictionary.encode_one(p) for p in dictionary.cross_lingual_phonemes})
    model = DiffSingerVarianceDeploy(len(dictionary), cross_lingual_token_idx=cross).eval()
    ckpt = harness.load_ckpt(model, exp, ckpt_steps=ckpt_steps, prefix_in_ckpt="model", strict=True)
    print(f"| variance model: {ckpt} ({len(cross)} cross-lingual tokens)")
    return modelfile.variance_sections(prefix, model)


def twin_sections(exp, prefix, ckpt_steps):
    """the sections of the acoustic experiment's staged twin; hparams are the acoustic experiment's afterwards"""
    from diffsinger_amd.deploy import DiffSingerAcousticDeploy
    load_config(exp / "config.yaml", overrides=dict(infer=True, work_dir=str(exp)))
    dictionary = harness.load_phoneme_dictionary()
    cross = sorted({dictionary.encode_one(p) for p in dictionary.cross_lingual_phonemes})
    model = DiffSingerAcousticDeploy(len(dictionary), hparams["audio_num_mel_bins"], cross_lingual_token_idx=cross).eval()
    ckpt = harness.load_ckpt(model, exp, ckpt_steps=ckpt_steps, prefix_in_ckpt="model", strict=True)
    print(f"| acoustic twin: {ckpt} ({len(cross)} cross-lingual tokens)")
    return modelfile.acoustic_sections(prefix, model)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("exp", type=pathlib.Path, help="experiment (work) directory")
    ap.add_argument("vocoder", type=pathlib.Path, help="NSF-HiFiGAN generator checkpoint (config.json beside it)")
    ap.add_argument("-o", "--out", type=pathlib.Path, required=True)
    ap.add_argument("--ckpt", type=int, default=None, help="checkpoint step (default: the latest)")
    ap.add_argument("--twin", metavar="PREFIX", default=None,
                    help="also write the acoustic experiment as a staged twin under this section name prefix (dsd_acoustic_open)")
    ap.add_argument("--variance", type=pathlib.Path, default=None, help="variance experiment (work) directory")
    ap.add_argument("--variance-prefix", default="var", help="section name prefix of the variance model (default: var)")
    ap.add_argument("--variance-ckpt", type=int, default=None, help="variance checkpoint step (default: the latest)")
    args = ap.parse_args()

    load_config(args.exp / "config.yaml", overrides=dict(infer=True, work_dir=str(args.exp)))
    dictionary = harness.load_phoneme_dictionary()
    model = DiffSingerAcoustic(len(dictionary), hparams["audio_num_mel_bins"]).eval()
    ckpt = harness.load_ckpt(model, args.exp, ckpt_steps=args.ckpt, prefix_in_ckpt="model", strict=True)
    print(f"| acoustic model: {ckpt}")
    vocoder = harness.load_vocoder(args.vocoder, device="cpu")
    gen = vocoder.model

    sections = [modelfile.section_of("encoder", model.fs2), modelfile.section_of("denoiser", model.diffusion._backbone())]
    if model.use_shallow_diffusion:
        sections.append(modelfile.section_of("aux_decoder", model.aux_decoder.decoder))
    sections.append(modelfile.section_of("vocoder", gen))
    sections.append(modelfile.section_of("mel", STFT(hparams["audio_sample_rate"], hparams["audio_num_mel_bins"], hparams["fft_size"],
                                                     hparams["win_size"], hparams["hop_size"], hparams["fmin"], hparams["fmax"])))
    meta = {
        "diffusion_type": str(hparams.get("diffusion_type", "ddpm")),
        "timesteps": str(hparams.get("timesteps", 1000)),
        "K_step": str(hparams.get("K_step", hparams.get("timesteps", 1000))),
        "K_step_infer": str(hparams.get("K_step_infer", hparams.get("K_step", hparams.get("timesteps", 1000)))),
        "T_start": repr(float(hparams.get("T_start", 0.0))),
        "time_scale_factor": repr(float(hparams.get("time_scale_factor", 1000))),
        "schedule_type": str(hparams.get("schedule_type", "linear")),
        "max_beta": repr(float(hparams.get("max_beta", 0.02))),
        "spec_min": _numbers(hparams["spec_min"]),
        "spec_max": _numbers(hparams["spec_max"]),
        "hop_size": str(hparams["hop_size"]),
        "audio_sample_rate": str(hparams["audio_sample_rate"]),
        "audio_num_mel_bins": str(hparams["audio_num_mel_bins"]),
        "mel_base": str(hparams.get("mel_base", "10")),
        "use_shallow_diffusion": str(int(bool(model.use_shallow_diffusion))),
        "phonemes": dictionary.decode(range(1, len(dictionary))),         # id order, ids from 1 (0 = padding)
    }
    if args.twin is not None:
        sections += twin_sections(args.exp, args.twin, args.ckpt)
    if args.variance is not None:
        sections += variance_sections(args.variance, args.variance_prefix, args.variance_ckpt)
    size = modelfile.write(args.out, sections, meta)
    with modelfile.open(args.out) as f:          # the C reader has the last word
        for s in f.sections:
            print(f"| section {s.name!r}: kind {s.kind}, {s.n_tensors} tensors, {s.total_floats} floats")
    print(f"| wrote {args.out}: {size} bytes, {len(meta)} metadata entries")


if __name__ == "__main__":
    main()
