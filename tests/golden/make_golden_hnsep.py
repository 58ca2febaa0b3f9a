"""Generator of G19 (tests/golden/g19_hnsep.npz): the reference's own VR separator (modules/hnsep/vr/: CascadedNet) and
DecomposedWaveformVocalRemover (utils/decomposed_waveform.py: harmonic(), aperiodic(), _kth_harmonic(0)), run in fp32 on
the CPU with seeded synthetic weights (diffsinger_amd.synth.hnsep_state_dict - regenerated from the seeds, not stored) on
seeded waveforms (mel_ref.waveform).

Runs on a machine with the reference tree.  pyworld is stubbed (the 'vr' path never calls it), the reference's heavy
utils/__init__ is bypassed (hparams is a plain dict), and the reference's checkpoint loader is bypassed by placing the
model in DecomposedWaveformVocalRemover's module-level cache.  librosa is not needed: the curves are compared against the
float64 restatement only (tests/hnsep_ref.py).  Prints the reference's own fp32 error against that float64 oracle per
case (the tolerances of tests/test_gpu_hnsep.py) and the share of mask magnitudes in (0.1, 0.9).

    python tests/golden/make_golden_hnsep.py /path/to/reference
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import hnsep_ref  # noqa: E402
import mel_ref  # noqa: E402
from diffsinger_amd import synth  # noqa: E402

SR = 44100
CONFIGS = {"small": dict(synth.HNSEP_SMALL), "stereo": dict(synth.HNSEP_SMALL, is_mono=False), "prod": dict(synth.HNSEP_PROD)}
# (config, weight seed, waveform seed, samples, store the mask)
CASES = [("small", 1900, 1911, 200, True),          # one 32-frame block
         ("small", 1900, 1912, 5127, True),
         ("small", 1900, 1913, 16000, False),
         ("stereo", 1901, 1914, 200, True),
         ("stereo", 1901, 1915, 5127, False),
         ("stereo", 1901, 1916, 16000, False),
         ("prod", 1902, 1917, 66150, False)]       # 1.5 s at 44.1 kHz
BASE_CASE = 2           # _kth_harmonic(0) on this case's harmonic part
BASE_HOP, BASE_WIN = 128, 512


def base_f0(n_frames):
    """f0 with unvoiced gaps (interp_f0 fills them) and values on both sides of center = f0 win / sr = 1 (86.13 Hz at
    win 512), shorter than n_samples // hop + 1 so the edge pad runs."""
    t = np.arange(n_frames)
    f0 = 180.0 + 40.0 * np.sin(t / 9.0)
    f0[12:20] = 0.0
    f0[30:36] = 86.0
    f0[36:40] = 86.3
    f0[70:75] = 0.0
    return f0[:-4].astype(np.float32)


def _stub_imports(ref_root):
    pw = types.ModuleType("pyworld")
    sys.modules["pyworld"] = pw
    sys.path.insert(0, ref_root)
    for name, path in (("modules", "modules"), ("utils", "utils")):
        pk = types.ModuleType(name)
        pk.__path__ = [os.path.join(ref_root, path)]
        sys.modules[name] = pk
    sys.modules["utils"].hparams = {"hnsep_ckpt": None}


def main(ref_root):
    _stub_imports(ref_root)
    from modules.hnsep.vr.nets import CascadedNet
    import utils.decomposed_waveform as dw
    torch.set_num_threads(8)
    out = {}
    for i, (name, wseed, yseed, n, keep_mask) in enumerate(CASES):
        cfg = CONFIGS[name]
        sd = synth.hnsep_state_dict(cfg, wseed)
        model = CascadedNet(cfg["n_fft"], cfg["hop_length"], cfg["nout"], cfg["nout_lstm"], True, is_mono=cfg["is_mono"]).eval()
        model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
        dw.SEP_MODEL = model
        x = mel_ref.waveform(yseed, n, SR).astype(np.float32)
        f0 = base_f0(n // BASE_HOP + 1)
        d = dw.DecomposedWaveform(x, SR, f0, hop_size=BASE_HOP, fft_size=BASE_WIN, win_size=BASE_WIN, algorithm="vr",
                                  device="cpu")
        h, ap = d.harmonic(), d.aperiodic()
        assert np.array_equal(ap, x - h)
        c = 1 if cfg["is_mono"] else 2
        spec, _ = hnsep_ref.spec_of(x, cfg)
        spec = np.stack([spec] * c)
        with torch.no_grad():
            m32 = model(torch.from_numpy(spec[None].astype(np.complex64)))[0].numpy()
        m64 = hnsep_ref.model64(sd, cfg)
        h64, mk64 = hnsep_ref.separate(m64, x, cfg)
        fl_h, fl_m = float(np.abs(h - h64).max()), float(np.abs(m32 - mk64).max())
        a = np.abs(mk64)
        mid = float(np.mean((a > 0.1) & (a < 0.9)))
        print(f"case {i}: {name} L {n} frames {spec.shape[-1]}: fp32 vs float64 harmonic {fl_h:.3g} (peak {np.abs(h64).max():.3f}), "
              f"mask {fl_m:.3g}; |mask| in (0.1, 0.9): {mid:.2f}")
        out[f"c{i}_meta"] = np.array([wseed, yseed, n, list(CONFIGS).index(name)], dtype=np.int64)
        out[f"c{i}_harmonic"] = h.astype(np.float32)
        out[f"c{i}_floor"] = np.array([fl_h, fl_m, mid])
        if keep_mask:
            out[f"c{i}_mask"] = m32.astype(np.complex64)
        if i == BASE_CASE:
            b0 = d.harmonic(0)
            b64 = hnsep_ref.base_harmonic(h, f0, SR, BASE_HOP, BASE_WIN)
            fl_b = float(np.abs(b0 - b64).max())
            print(f"  _kth_harmonic(0): fp32 vs float64 {fl_b:.3g} (peak {np.abs(b64).max():.3f})")
            out["base_f0"] = f0
            out["base_harmonic"] = b0.astype(np.float32)
            out["base_floor"] = np.array([fl_b])
    out["n_cases"] = np.array(len(CASES))
    sd = synth.hnsep_state_dict(CONFIGS["prod"], 1902)
    out["keys"] = np.array(list(sd))
    out["key_shapes"] = np.array([",".join(map(str, np.shape(v))) for v in sd.values()])
    path = os.path.join(HERE, "g19_hnsep.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("DSD_REFERENCE", "../reference"))
