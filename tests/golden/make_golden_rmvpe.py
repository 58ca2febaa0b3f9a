"""Generator of G18 (tests/golden/g18_rmvpe.npz): the reference's own RMVPE (modules/pe/rmvpe/: E2E0, MelSpectrogram,
RMVPE.mel2hidden / decode / infer_from_audio at sample_rate 16000, get_pitch), run in fp32 on the CPU with seeded
synthetic weights (diffsinger_amd.synth.rmvpe_state_dict - regenerated from the seeds, not stored) on seeded waveforms
(waveform() below).

Runs on a machine with the reference tree and transformers; the tests only read the .npz.  librosa is not needed:
`librosa.filters.mel(htk=True)` is stubbed by transformers' mel_filter_bank(norm="slaney", mel_scale="htk") cast to
float32, which is what spec.py stores.  torchaudio is stubbed: at 16 kHz infer_from_audio never reaches Resample.  The
reference's package __init__ files (lightning, the hparams loader) are bypassed; only the modules named above run.

    python tests/golden/make_golden_rmvpe.py /path/to/reference
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import mel_ref  # noqa: E402
import rmvpe_ref  # noqa: E402
from diffsinger_amd import synth  # noqa: E402

PROD = dict(n_blocks=4, n_gru=1, en_de_layers=5, inter_layers=4, en_out_channels=16)
SMALL = dict(synth.RMVPE_SMALL)
SMALL0 = dict(SMALL, n_gru=0)
CONFIGS = {"prod": PROD, "small": SMALL, "small0": SMALL0}
# (config, weight seed, waveform seed, samples at 16 kHz, store hidden)
CASES = [("small", 1800, 1811, 63 * 160 + 17, True),      # T = 64: a multiple of 32
         ("small", 1800, 1812, 16000 + 3300, True),       # T = 121
         ("small", 1800, 1813, 513, True),                # the shortest legal clip: T = 4
         ("small0", 1801, 1814, 8000 + 77, True),         # the Linear(384, 360) head, T = 51
         ("prod", 1802, 1815, 16000 + 4000, False)]       # T = 126
PITCH_CASE = 4          # get_pitch on this case's clip: hop 160 / 512, speed 1 / 1.25, interp_uv both ways


def waveform(seed, n):
    """mel_ref.waveform with a stretch of near silence (noise 50 dB down) over its middle fifth: unvoiced frames."""
    x = mel_ref.waveform(seed, n, 16000).astype(np.float64)
    a, b = 2 * n // 5, 3 * n // 5
    x[a:b] = 0.003 * np.random.default_rng(seed + 7).standard_normal(b - a)
    return x.astype(np.float32)


def crafted_hidden():
    """decode cases: all below threshold, argmax at class 0 and at class 359, exact ties (first index wins), a flat row."""
    rng = np.random.default_rng(1890)
    h = rng.uniform(0.0, 0.02, (6, 360)).astype(np.float32)
    h[1, 0], h[1, 1:4] = 0.9, 0.5
    h[2, 359], h[2, 355:359] = 0.8, 0.4
    h[3, 100], h[3, 200] = 0.7, 0.7
    h[4, :] = 0.25
    h[5, 180], h[5, 176:185] = 0.0301, 0.02
    h[5, 180] = 0.0301
    return h


def _stub_imports(ref_root):
    from transformers.audio_utils import mel_filter_bank

    def mel(sr, n_fft, n_mels, fmin, fmax, htk=False):
        fb = mel_filter_bank(num_frequency_bins=n_fft // 2 + 1, num_mel_filters=n_mels, min_frequency=fmin,
                             max_frequency=fmax, sampling_rate=sr, norm="slaney", mel_scale="htk" if htk else "slaney")
        return fb.T.astype(np.float32)
    lib = types.ModuleType("librosa")
    lib.filters = types.ModuleType("librosa.filters")
    lib.filters.mel = mel
    sys.modules["librosa"], sys.modules["librosa.filters"] = lib, lib.filters
    ta = types.ModuleType("torchaudio")
    ta.transforms = types.ModuleType("torchaudio.transforms")
    ta.transforms.Resample = None
    sys.modules["torchaudio"], sys.modules["torchaudio.transforms"] = ta, ta.transforms
    sc = types.ModuleType("scipy")
    sc.io = types.ModuleType("scipy.io")
    sc.io.wavfile = None
    sys.modules.setdefault("scipy", sc)
    sys.modules.setdefault("scipy.io", sc.io)
    sys.path.insert(0, ref_root)
    for name, path in (("modules", "modules"), ("modules.pe", "modules/pe"), ("utils", "utils")):
        pk = types.ModuleType(name)
        pk.__path__ = [os.path.join(ref_root, path)]
        sys.modules[name] = pk


def main(ref_root):
    _stub_imports(ref_root)
    from modules.pe.rmvpe import E2E0, MelSpectrogram
    from modules.pe.rmvpe.inference import RMVPE
    torch.set_num_threads(4)
    out = {}
    pes = {}
    for name, cfg in CONFIGS.items():
        pes[name] = None
    for i, (name, wseed, yseed, n, keep_hidden) in enumerate(CASES):
        cfg = CONFIGS[name]
        sd = synth.rmvpe_state_dict(seed=wseed, with_tf=True, **cfg)
        model = E2E0(cfg["n_blocks"], cfg["n_gru"], (2, 2), cfg["en_de_layers"], cfg["inter_layers"], 1,
                     cfg["en_out_channels"]).eval()
        model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
        pe = RMVPE.__new__(RMVPE)            # RMVPE.__init__ reads a checkpoint file and always builds E2E0(4, 1, (2, 2))
        pe.resample_kernel, pe.device, pe.model = {}, "cpu", model
        pe.mel_extractor = MelSpectrogram(128, 16000, 1024, 160, None, 30, 8000)
        y = waveform(yseed, n)
        with torch.no_grad():
            mel = pe.mel_extractor(torch.from_numpy(y)[None], center=True)
            hidden = pe.mel2hidden(mel)[0].numpy()
        f0 = pe.decode(torch.from_numpy(hidden)[None])
        f0_audio = pe.infer_from_audio(y, sample_rate=16000)
        assert np.array_equal(f0, f0_audio)
        h64 = rmvpe_ref.mel2hidden(rmvpe_ref.log_mel(y), sd)
        floor = float(np.abs(hidden - h64).max())
        mx = hidden.max(axis=1)
        print(f"case {i}: {name} L {n} T {hidden.shape[0]}: fp32 vs float64 {floor:.3g}, max {mx.min():.3f}..{mx.max():.3f}, "
              f"voiced {np.mean(mx >= 0.03):.2f}, argmax {np.percentile(hidden.argmax(1), [0, 50, 100])}")
        out[f"c{i}_meta"] = np.array([wseed, yseed, n, list(CONFIGS).index(name)], dtype=np.int64)
        out[f"c{i}_f0"] = f0.astype(np.float32)
        out[f"c{i}_max"] = mx.astype(np.float32)
        out[f"c{i}_argmax"] = hidden.argmax(axis=1).astype(np.int16)
        out[f"c{i}_mel"] = mel[0].numpy().astype(np.float32)[:, :4] if not keep_hidden else mel[0].numpy().astype(np.float32)
        if keep_hidden:
            out[f"c{i}_hidden"] = hidden.astype(np.float32)
        if i == PITCH_CASE:
            k = 0
            for hop in (160, 512):
                for speed in (1, 1.25):
                    for interp in (False, True):
                        length = int(np.ceil(n / round(hop * speed))) + 2
                        f0r, uvr = pe.get_pitch(y, 16000, length, hop_size=hop, speed=speed, interp_uv=interp)
                        out[f"p{k}_args"] = np.array([hop, speed, int(interp), length], dtype=np.float64)
                        out[f"p{k}_f0"], out[f"p{k}_uv"] = f0r.astype(np.float32), uvr
                        k += 1
            out["n_pitch"] = np.array(k)
    out["n_cases"] = np.array(len(CASES))
    hc = crafted_hidden()
    out["dec_hidden"] = hc
    out["dec_f0"] = RMVPE.decode(None, torch.from_numpy(hc)[None]).astype(np.float32)
    shapes = synth.rmvpe_param_shapes(with_tf=True, **PROD)
    out["keys"] = np.array(list(shapes))
    out["key_shapes"] = np.array([",".join(map(str, s)) for s in shapes.values()])
    path = os.path.join(HERE, "g18_rmvpe.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("DSD_REFERENCE", "../reference"))
