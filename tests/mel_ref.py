"""Float64 restatement of STFT.get_mel (modules/nsf_hifigan/nvSTFT.py:50-87, center=False) for the mel tests: numpy
reflect padding, frames, the periodic Hann window centred in the N'-sample frame, np.fft.rfft, |X|, the keyshift bin
rule, the mel projection, log(clamp).  Also the Slaney filterbank restated from librosa.filters.mel's definition, and
the seeded test waveforms G17 is recorded on."""
import numpy as np

PROD = dict(sr=44100, n_fft=2048, win_size=2048, hop=512, n_mels=128, fmin=40.0, fmax=16000.0)
SMALL = dict(sr=22050, n_fft=1024, win_size=800, hop=256, n_mels=80, fmin=0.0, fmax=8000.0)


def _hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    f_sp, min_log_hz, logstep = 200.0 / 3, 1000.0, np.log(6.4) / 27.0
    mels = f / f_sp
    return np.where(f >= min_log_hz, min_log_hz / f_sp + np.log(np.maximum(f, 1e-300) / min_log_hz) / logstep, mels)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    f_sp, min_log_hz, logstep = 200.0 / 3, 1000.0, np.log(6.4) / 27.0
    return np.where(m >= min_log_hz / f_sp, min_log_hz * np.exp(logstep * (m - min_log_hz / f_sp)), f_sp * m)


def filterbank(sr, n_fft, n_mels, fmin, fmax):
    """librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax) (Slaney scale, Slaney norm, float32)."""
    fft_f = np.fft.rfftfreq(n=n_fft, d=1.0 / sr)
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = np.subtract.outer(mel_f, fft_f)
    w = np.zeros((n_mels, len(fft_f)), dtype=np.float32)
    for i in range(n_mels):
        w[i] = np.maximum(0, np.minimum(-ramps[i] / fdiff[i], ramps[i + 2] / fdiff[i + 1]))
    w *= (2.0 / (mel_f[2: n_mels + 2] - mel_f[:n_mels]))[:, None]
    return w


def geometry(n_fft, win_size, hop, keyshift=0, speed=1):
    factor = 2 ** (keyshift / 12)
    n = int(np.round(n_fft * factor))
    w = int(np.round(win_size * factor))
    h = int(np.round(hop * speed))
    return n, w, h, (w - h) // 2, (w - h + 1) // 2


def num_frames(n_samples, n_fft, win_size, hop, keyshift=0, speed=1):
    n, w, h, pl, pr = geometry(n_fft, win_size, hop, keyshift, speed)
    if pl >= n_samples or pr >= n_samples or n_samples + pl + pr < n:
        return None
    return 1 + (n_samples + pl + pr - n) // h


def get_mel(y, cfg, keyshift=0, speed=1, fb=None, linear=False, clip=1e-5):
    """y [L] -> [n_mels, T] float64 (natural-log mel clamped at `clip`; linear=True: before the clamp and log)."""
    n, w, h, pl, pr = geometry(cfg["n_fft"], cfg["win_size"], cfg["hop"], keyshift, speed)
    y = np.asarray(y, dtype=np.float64)
    y = np.pad(y, (max(pl, 0), max(pr, 0)), mode="reflect")
    y = y[max(-pl, 0): len(y) - max(-pr, 0)]
    t = 1 + (len(y) - n) // h
    win = np.zeros(n)
    off = (n - w) // 2
    # torch.hann_window(w): periodic, and [1.] at w == 1 (where the formula would give 0)
    win[off: off + w] = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(w) / w) if w > 1 else 1.0
    spec = np.empty((n // 2 + 1, t))                              # [bins, T], in pieces of 1024 frames
    for t0 in range(0, t, 1024):
        nt = min(1024, t - t0)
        frames = np.lib.stride_tricks.as_strided(y[t0 * h:], (nt, n), (y.strides[0] * h, y.strides[0]))
        spec[:, t0: t0 + nt] = np.abs(np.fft.rfft(frames * win, axis=1)).T
    if keyshift != 0:
        size = cfg["n_fft"] // 2 + 1
        if spec.shape[0] < size:
            spec = np.pad(spec, ((0, size - spec.shape[0]), (0, 0)))
        spec = spec[:size] * cfg["win_size"] / w
    if fb is None:
        fb = filterbank(cfg["sr"], cfg["n_fft"], cfg["n_mels"], cfg["fmin"], cfg["fmax"])
    mel = fb.astype(np.float64) @ spec
    return mel if linear else np.log(np.maximum(mel, clip))


def waveform(seed, n_samples, sr):
    """A sung-vowel-like test signal: 24 harmonics of a gliding, vibrato f0 with a 1/h roll-off, an amplitude envelope and
    white noise 40 dB down; peak 0.8.  float32."""
    rng = np.random.default_rng(seed)
    t = np.arange(n_samples) / sr
    f0 = rng.uniform(110, 440) * 2 ** (rng.uniform(-0.5, 0.5) * t / max(t[-1], 1e-9) + 0.02 * np.sin(2 * np.pi * 5.5 * t))
    phase = 2 * np.pi * np.cumsum(f0) / sr
    x = np.zeros(n_samples)
    for k in range(1, 25):
        x += np.sin(k * phase + rng.uniform(0, 2 * np.pi)) / k * (k * f0 < sr / 2)
    x *= 0.6 + 0.4 * np.sin(2 * np.pi * rng.uniform(0.2, 1.0) * t + rng.uniform(0, 2 * np.pi))
    x = 0.8 * x / np.max(np.abs(x))
    x += 0.008 * rng.standard_normal(n_samples)
    return np.clip(x, -1, 1).astype(np.float32)
