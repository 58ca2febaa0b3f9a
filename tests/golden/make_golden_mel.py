"""Generator of G17 (tests/golden/g17_mel.npz): the reference's own STFT.get_mel (modules/nsf_hifigan/nvSTFT.py), run in
fp32 on the CPU on seeded waveforms (tests/mel_ref.py:waveform - regenerated from the seeds, not stored).

Runs on a machine with the reference tree and transformers; the tests only read the .npz.  librosa is not needed:
`librosa.filters.mel` is stubbed by transformers' Slaney filterbank (mel_filter_bank(norm="slaney", mel_scale="slaney"),
documented equal to librosa's) cast to float32, which is what nvSTFT.py:47-48 stores.

    python tests/golden/make_golden_mel.py /path/to/reference
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import mel_ref  # noqa: E402

# (config, seed, seconds or samples, keyshift, speed)
CASES = [("prod", 1701, 1.5, 0, 1), ("prod", 1702, 1.5, 3, 1), ("prod", 1703, 1.5, -5.5, 1), ("prod", 1704, 1.5, 12, 1),
         ("prod", 1705, 1.5, 0, 1.25), ("prod", 1706, 1.5, 2, 0.8),
         ("small", 1711, 1.0, 0, 1), ("small", 1712, 1.0, -2, 1.1),
         ("prod", 1721, 772, 0, 1)]          # 4 samples above the reflect limit (pad 768 < L)


def _stub_librosa():
    from transformers.audio_utils import mel_filter_bank

    def mel(sr, n_fft, n_mels, fmin, fmax):
        fb = mel_filter_bank(num_frequency_bins=n_fft // 2 + 1, num_mel_filters=n_mels, min_frequency=fmin,
                             max_frequency=fmax, sampling_rate=sr, norm="slaney", mel_scale="slaney")
        return fb.T.astype(np.float32)
    lib = types.ModuleType("librosa")
    lib.filters = types.ModuleType("librosa.filters")
    lib.filters.mel = mel
    sys.modules["librosa"] = lib
    sys.modules["librosa.filters"] = lib.filters


def main(ref_root):
    _stub_librosa()
    sys.path.insert(0, ref_root)
    from modules.nsf_hifigan.nvSTFT import STFT
    torch.set_num_threads(1)
    out = {}
    for i, (name, seed, length, ks, speed) in enumerate(CASES):
        c = mel_ref.PROD if name == "prod" else mel_ref.SMALL
        n = int(length) if isinstance(length, int) else int(round(length * c["sr"]))
        y = mel_ref.waveform(seed, n, c["sr"])
        stft = STFT(c["sr"], c["n_mels"], c["n_fft"], c["win_size"], c["hop"], c["fmin"], c["fmax"], device="cpu")
        with torch.no_grad():
            mel = stft.get_mel(torch.from_numpy(y)[None], keyshift=ks, speed=speed)[0].numpy()
        out[f"c{i}_meta"] = np.array([seed, n, ks, speed, 0 if name == "prod" else 1], dtype=np.float64)
        out[f"c{i}_mel"] = mel.astype(np.float32)
        print(f"case {i}: {name} seed {seed} L {n} keyshift {ks} speed {speed} -> {mel.shape}")
    out["n_cases"] = np.array(len(CASES))
    path = os.path.join(HERE, "g17_mel.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("DSD_REFERENCE", "../reference"))
