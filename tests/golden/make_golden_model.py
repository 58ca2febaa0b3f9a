"""G29: tests/golden/g29_model_v1.dsdm, the pin of model file format version 1.

    python tests/golden/make_golden_model.py            # writes the file; run ONCE per format version

One section, "denoiser": a WaveNet of in_dims 4, 1 layer, 4 channels, dilation cycle 1, hidden 4 with
synth.synth_state_dict(seed=SEED) weights and the SinusoidalPosEmb frequency table the wrapper uploads; two metadata
entries.  About 3 KiB.  The file is written by diffsinger_amd.modelfile.write and never regenerated for as long as version
1 is read: tests/test_modelfile_host.py holds a fresh write() of `content()` byte-identical to it, opens it through the C
reader and checks its CRC with zlib - so a change to the writer OR the reader that moves a byte of version 1 shows.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "g29_model_v1.dsdm")
SEED = 2901
IN_DIMS, HIDDEN = 4, 4
ARGS = dict(num_layers=1, num_channels=4, dilation_cycle_length=1)
META = {"timesteps": "1000", "phonemes": "AP SP a i u"}


def weights():
    from diffsinger_amd import synth
    return synth.synth_state_dict(synth.backbone_param_shapes("wavenet", IN_DIMS, 1, hidden_size=HIDDEN, **ARGS), seed=SEED)


def content():
    """-> (sections, meta) of the pinned file"""
    import torch
    from diffsinger_amd import modelfile
    from diffsinger_amd.backbones import build_backbone
    from diffsinger_amd.hparams import hparams
    saved = dict(hparams)
    hparams.update(hidden_size=HIDDEN)
    try:
        net = build_backbone(IN_DIMS, 1, "wavenet", ARGS)
    finally:
        hparams.clear()
        hparams.update(saved)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in weights().items()}, strict=True)
    return [modelfile.section_of("denoiser", net)], dict(META)


if __name__ == "__main__":
    from diffsinger_amd import modelfile
    sections, meta = content()
    print(PATH, modelfile.write(PATH, sections, meta), "bytes")
