"""Generator of G26 (tests/golden/g26_mel_configs.npz): the reference's own STFT.get_mel (modules/nsf_hifigan/nvSTFT.py),
run in fp32 on the CPU with one thread, on every row of tests/mel_config_cases.py (the waveforms are regenerated from
the seeds, not stored).  Per row: c{i}_meta = (seed, samples, keyshift, speed, clip_val) and c{i}_mel = the reference's
output; `tags` = the rows' names in order.

Runs on a machine with the reference tree and transformers; the tests only read the .npz.  librosa is stubbed as in
make_golden_mel.py (transformers' Slaney filterbank cast to float32; at an odd n_fft on librosa's bin centres, _mel_odd).

    python tests/golden/make_golden_mel_configs.py /path/to/reference
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import mel_config_cases as mc  # noqa: E402
from make_golden_mel import _stub_librosa  # noqa: E402


def _mel_odd(sr, n_fft, n_mels, fmin, fmax):
    """transformers' mel_filter_bank places the bin centres at linspace(0, sr // 2, bins), which is librosa's
    fft_frequencies (np.fft.rfftfreq: k sr / n_fft) only at an even n_fft.  At an odd one: transformers' own Slaney scale,
    triangles and norm, put together as mel_filter_bank does, on librosa's bin centres."""
    from transformers import audio_utils as au
    mel_freqs = np.linspace(au.hertz_to_mel(fmin, mel_scale="slaney"), au.hertz_to_mel(fmax, mel_scale="slaney"), n_mels + 2)
    filter_freqs = au.mel_to_hertz(mel_freqs, mel_scale="slaney")
    fb = au._create_triangular_filter_bank(np.fft.rfftfreq(n=n_fft, d=1.0 / sr), filter_freqs)
    fb *= np.expand_dims(2.0 / (filter_freqs[2: n_mels + 2] - filter_freqs[:n_mels]), 0)
    return fb.T.astype(np.float32)


def main(ref_root):
    _stub_librosa()
    even = sys.modules["librosa"].filters.mel
    sys.modules["librosa"].filters.mel = lambda sr, n_fft, n_mels, fmin, fmax: (
        _mel_odd if n_fft % 2 else even)(sr, n_fft, n_mels, fmin, fmax)
    sys.path.insert(0, ref_root)
    from modules.nsf_hifigan.nvSTFT import STFT
    torch.set_num_threads(1)
    warnings.filterwarnings("ignore", message=".*mel filter has all zero values.*")
    out = {}
    for i, (tag, c) in enumerate(mc.CASES.items()):
        cfg = c["cfg"]
        y = mc.clip_wave(tag)
        stft = STFT(cfg["sr"], cfg["n_mels"], cfg["n_fft"], cfg["win_size"], cfg["hop"], cfg["fmin"], cfg["fmax"],
                    clip_val=cfg["clip"], device="cpu")
        with torch.no_grad():
            mel = stft.get_mel(torch.from_numpy(y)[None], keyshift=c["ks"], speed=c["sp"])[0].numpy()
        out[f"c{i}_meta"] = np.array([c["seed"], c["n"], c["ks"], c["sp"], cfg["clip"]], dtype=np.float64)
        out[f"c{i}_mel"] = mel.astype(np.float32)
        print(f"case {i}: {tag} L {c['n']} keyshift {c['ks']} speed {c['sp']} -> {mel.shape}")
    out["tags"] = np.array(list(mc.CASES))
    path = mc.G26
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("DSD_REFERENCE", "../reference"))
