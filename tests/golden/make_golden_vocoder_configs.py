"""Generator of G28 (tests/golden/g28_vocoder_configs.npz): the reference's own NSF-HiFiGAN Generator
(modules/nsf_hifigan/models.py) in fp32 on the CPU at configurations away from k = 2u - k = u, k = 8u, odd rates, one stage, a
two-stage mini_nsf - with the seeded weights and inputs of tests/vocoder_config_cases.py (the "g28:<tag>" forms of G28 at G28_SHAPE: the
reference's residual blocks take exactly three / two dilations) and SineGen's draws
injected, as g10_vocoder() of make_golden.py injects them.  Stored per case: the waveform, the weights' digest, and the two
inputs that come from numpy's generator rather than from synth's seeds (f0, rand_ini).

Prints, per case, "floor <tag> <value>" - the reference's fp32 waveform against the float64 oracle, max |difference| over
max |float64 waveform| - and "range <tag> peak <p> std <s> saturated <share>".

Runs on a machine with the reference tree; the tests only read the .npz.  `lightning` (imported by models.py for a log call,
never executed on this path) is stubbed.

    python tests/golden/make_golden_vocoder_configs.py /path/to/reference
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import vocoder_config_cases as cc  # noqa: E402
from diffsinger_amd import synth  # noqa: E402
from make_golden_width import _stub_lightning, to_t  # noqa: E402


def main(ref_root):
    _stub_lightning()
    sys.path.insert(0, ref_root)
    from modules.nsf_hifigan.env import AttrDict
    from modules.nsf_hifigan.models import Generator
    torch.set_num_threads(8)
    out = {}
    for case in cc.G28:
        tag = "g28:" + case         # the form of the case the reference's fixed-length residual blocks can build
        h, i = cc.config(tag), cc.inputs(tag, *cc.G28_SHAPE)
        assert cc.accepts(h) == (True, "")
        gen = Generator(AttrDict(h))
        gen.remove_weight_norm()
        gen.load_state_dict({k: to_t(v) for k, v in cc.weights(tag).items()}, strict=True)
        gen.eval()
        dim = i["rand_ini"].shape[0]
        orig_rand, orig_randn_like = torch.rand, torch.randn_like
        torch.rand = lambda *a, **k: to_t(i["rand_ini"]).reshape(1, 1, dim).clone()
        torch.randn_like = lambda x, **k: to_t(i["noise"] if x.shape[-1] == dim else i["pre_noise"]).clone()
        try:
            with torch.no_grad():
                wav = gen(to_t(i["mel"]), to_t(i["f0"])).numpy()
        finally:
            torch.rand, torch.randn_like = orig_rand, orig_randn_like
        want64 = cc.reference(tag, *cc.G28_SHAPE)
        assert wav.shape == want64.shape, (wav.shape, want64.shape)
        tag = case
        print(f"floor {tag} {cc.floor_of(wav, want64):.3g}")
        print(f"range {tag} peak {np.abs(wav).max():.3f} std {wav.std():.4f} saturated {float((np.abs(wav) > 0.99).mean()):.4f}")
        out[f"{tag}_wav"] = wav
        out[f"{tag}_f0"], out[f"{tag}_rand_ini"] = i["f0"], i["rand_ini"]
        out[f"{tag}_digest"] = np.array(synth.state_dict_digest(cc.weights("g28:" + tag)))
    path = os.path.join(HERE, "g28_vocoder_configs.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv[1])
