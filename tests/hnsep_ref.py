"""Float64 restatement of the VR separation chain and the variance curves (the oracle of tests/test_gpu_hnsep.py).

- The network: the torch mirror diffsinger_amd.hnsep.CascadedNet run in float64 on the CPU with the same weights.
- predict_from_audio's padding, the STFT (periodic Hann, center=True, zero pad) and torch.istft's overlap-add and
  window-square envelope: numpy float64 (np.fft).
- _kth_harmonic(0): the Nuttall window, the f0 bin mask, reflect padding, the iSTFT with length = n_samples.
- librosa 0.9.2 feature.rms (center=True, pad_mode="constant") and amplitude_to_db (ref 1, amin 1e-5, top_db 80), restated
  from that release's documented definitions; not compared against librosa itself (not installed).
"""
import numpy as np
import torch

from diffsinger_amd import hnsep
from diffsinger_amd.variance_harness import interp_f0


def model64(sd, cfg):
    m = hnsep.CascadedNet(**cfg)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return m.double().eval()


def hann(n):
    return 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)


def nuttall(n):
    ph = np.arange(n) / n * 2 * np.pi
    return 0.355768 - 0.487396 * np.cos(ph) + 0.144232 * np.cos(2 * ph) - 0.012604 * np.cos(3 * ph)


def stft(x, n_fft, hop, win, mode, dtype=np.float64):
    """torch.stft(center=True): pad n_fft / 2 (mode 'constant' or 'reflect'), frames of hop -> [bins, frames] complex.
    dtype float32: the same steps in single precision (numpy's pocketfft keeps float32 input in float32)."""
    xp = np.pad(np.asarray(x, dtype), n_fft // 2, mode=mode)
    win = np.asarray(win, dtype)
    n = 1 + (len(xp) - n_fft) // hop
    fr = np.stack([xp[t * hop:t * hop + n_fft] * win for t in range(n)])
    spec = np.fft.rfft(fr, axis=1).T
    assert spec.dtype == np.result_type(dtype, np.complex64), spec.dtype
    return spec


def istft(spec, n_fft, hop, win, length=None, dtype=np.float64):
    """torch.istft(center=True): irfft, window, overlap-add / sum of window^2, trim n_fft / 2 (and to `length`)."""
    win = np.asarray(win, dtype)
    fr = np.fft.irfft(spec.T, n=n_fft, axis=1) * win
    assert fr.dtype == dtype, fr.dtype
    n = spec.shape[1]
    total = n_fft + hop * (n - 1)
    y, env = np.zeros(total, dtype), np.zeros(total, dtype)
    for t in range(n):
        y[t * hop:t * hop + n_fft] += fr[t]
        env[t * hop:t * hop + n_fft] += win ** 2
    start = n_fft // 2
    end = start + length if length is not None else total - n_fft // 2
    y = np.pad(y, (0, max(0, end - total)))
    env = np.pad(env, (0, max(0, end - total)), constant_values=1.0)
    return y[start:end] / env[start:end]


def spec_of(x, cfg):
    """predict_from_audio's zero padding and STFT of a mono clip -> [bins, frames] complex, left pad."""
    pl, pr, _ = hnsep.padding(len(x), cfg["hop_length"])
    xp = np.pad(np.asarray(x, np.float64), (pl, pr))
    return stft(xp, cfg["n_fft"], cfg["hop_length"], hann(cfg["n_fft"]), "constant"), pl


def mask(model, spec):
    """CascadedNet.forward in float64: spec [C, bins, frames] complex -> mask, same shape."""
    with torch.no_grad():
        return model(torch.from_numpy(spec[None]).to(torch.complex128))[0].numpy()


def separate(model, x, cfg):
    """DecomposedWaveformVocalRemover._infer: the harmonic part of a mono clip (a stereo model sees it twice, averaged)."""
    c = 1 if cfg["is_mono"] else 2
    s, pl = spec_of(x, cfg)
    spec = np.stack([s] * c)
    m = mask(model, spec)
    ys = [istft(spec[i] * m[i], cfg["n_fft"], cfg["hop_length"], hann(cfg["n_fft"]))[pl:pl + len(x)] for i in range(c)]
    return np.mean(ys, axis=0), m


def base_f0(f0, n_samples, hop):
    """_kth_harmonic's host part: edge pad to n_samples // hop + 1 frames, interpolate unvoiced frames."""
    f0 = np.asarray(f0, dtype=np.float64).copy()
    pad = n_samples // hop - len(f0) + 1
    if pad > 0:
        f0 = np.pad(f0, (0, pad), mode="constant", constant_values=(f0[0], f0[-1]))
    return interp_f0(f0)[0]


def base_harmonic(h, f0, sr, hop, win_size, f0_interp=None, dtype=np.float64):
    """_kth_harmonic(0) on the harmonic part h (float64; dtype float32: STFT and iSTFT in single precision with the same
    bin mask, the floor a float32 implementation is measured against)."""
    n = len(h)
    f0 = base_f0(f0, n, hop) if f0_interp is None else np.asarray(f0_interp, np.float64)
    w = nuttall(win_size)
    spec = stft(h, win_size, hop, w, "reflect", dtype)
    nb, nt = spec.shape
    idx = np.arange(nb)[None]
    center = (f0 * win_size / sr)[:, None]
    m = (center >= 1) & (idx >= np.maximum(center - 3.5, 0)) & (idx < np.minimum(center + 3.5, nb))
    mk = np.zeros((nt, nb), bool)
    k = min(nt, len(f0))
    mk[:k] = m[:k]
    return istft(spec * mk.T, win_size, hop, w, length=n, dtype=dtype)


def rms(y, hop, win):
    """librosa 0.9.2 feature.rms(y, frame_length=win, hop_length=hop)[0] with that release's defaults.  The signature
    restated (librosa/feature/spectral.py, release 0.9.2):

        def rms(*, y=None, S=None, frame_length=2048, hop_length=512, center=True, pad_mode="constant"):

    with `center`: y padded by frame_length // 2 on both sides with np.pad(mode=pad_mode), then util.frame and
    sqrt(mean(|x|^2)) per frame.  Written from that release's source; not checked against an installed librosa."""
    yp = np.pad(np.asarray(y, np.float64), (win // 2, win // 2), mode="constant")
    n = 1 + (len(yp) - win) // hop
    return np.array([np.sqrt(np.mean(yp[t * hop:t * hop + win] ** 2)) for t in range(n)])


def amplitude_to_db(a, amin=1e-5, top_db=80.0):
    """librosa 0.9.2 amplitude_to_db(S, ref=1.0, amin, top_db) = power_to_db(|S|^2, ref=1, amin=amin^2, top_db)."""
    db = 10.0 * np.log10(np.maximum(amin ** 2, np.abs(a) ** 2))
    return np.maximum(db, db.max() - top_db)


def energy(y, length, hop, win, domain="db"):
    e = rms(y, hop, win)
    e = np.pad(e, (0, max(0, length - len(e))))[:length]
    return amplitude_to_db(e) if domain == "db" else e


def tension(h, base, length, hop, win, domain="logit"):
    eb, eh = energy(base, length, hop, win, "amplitude"), energy(h, length, hop, win, "amplitude")
    t = np.sqrt(np.clip(eh ** 2 - eb ** 2, 0, None)) / (eh + 1e-5)
    if domain == "ratio":
        return np.clip(t, 0, 1)
    if domain == "db":
        return amplitude_to_db(np.clip(t, 1e-5, 1))
    t = np.clip(t, 1e-4, 1 - 1e-4)
    return np.log(t / (1 - t))
