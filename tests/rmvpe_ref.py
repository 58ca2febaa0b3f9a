"""Float64 numpy restatement of RMVPE (modules/pe/rmvpe/) for the pitch tests: torchaudio's sinc_interp_hann resampler,
the HTK mel bank, MelSpectrogram(center=True), E2E0 with BatchNorm unfolded, the BiGRU, to_local_average_f0 and
get_pitch's post-processing.  Weights are a state_dict of numpy arrays under the reference's names."""
import math

import numpy as np

N_CLASS, N_MELS, CONST = 360, 128, 1997.3794084376191


# ---------------------------------------------------------------------------------------------------------------- front end
def resample_kernel(orig, new, lowpass_filter_width=128, rolloff=0.99):
    """torchaudio.functional._get_sinc_resample_kernel (sinc_interp_hann, dtype None): float64 except the phase term
    (an int64 arange / new: float32), stored as float32.  -> (kernel [new, K] float32, width, orig, new) after the gcd."""
    g = math.gcd(int(orig), int(new))
    orig, new = int(orig) // g, int(new) // g
    base = min(orig, new) * rolloff
    width = math.ceil(lowpass_filter_width * orig / base)
    idx = np.arange(-width, width + orig, dtype=np.float64)[None, :] / orig
    t = (np.arange(0, -new, -1).astype(np.float32) / np.float32(new)).astype(np.float64)[:, None] + idx
    t *= base
    t = np.clip(t, -lowpass_filter_width, lowpass_filter_width)
    window = np.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t *= math.pi
    scale = base / orig
    with np.errstate(invalid="ignore", divide="ignore"):
        k = np.where(t == 0, 1.0, np.sin(t) / t)
    k *= window * scale
    return k.astype(np.float32), width, orig, new


def resample(x, sr, new=16000):
    """torchaudio Resample(sr, new, lowpass_filter_width=128)(x) in float64 on the float32 kernel."""
    if sr == new:
        return np.asarray(x, dtype=np.float64)
    k, width, orig, nw = resample_kernel(sr, new)
    x = np.asarray(x, dtype=np.float64)
    L = len(x)
    xp = np.pad(x, (width, width + orig))
    nblk = (len(xp) - k.shape[1]) // orig + 1
    frames = np.lib.stride_tricks.as_strided(xp, (nblk, k.shape[1]), (xp.strides[0] * orig, xp.strides[0]))
    y = (frames @ k.astype(np.float64).T).reshape(-1)
    return y[: math.ceil(nw * L / orig)]


def resampled_length(n, sr):
    if sr == 16000:
        return n
    g = math.gcd(int(sr), 16000)
    return -(-(16000 // g) * n // (sr // g))


def num_frames(n, sr=16000):
    n16 = resampled_length(n, sr)
    return None if n16 <= 512 else 1 + n16 // 160


def htk_filterbank(sr=16000, n_fft=1024, n_mels=128, fmin=30.0, fmax=8000.0):
    """librosa.filters.mel(..., htk=True): HTK scale, Slaney area norm, float32."""
    fft_f = np.fft.rfftfreq(n=n_fft, d=1.0 / sr)
    to_mel = lambda f: 2595.0 * np.log10(1.0 + np.asarray(f, dtype=np.float64) / 700.0)  # noqa: E731
    mel_f = 700.0 * (10.0 ** (np.linspace(to_mel(fmin), to_mel(fmax), n_mels + 2) / 2595.0) - 1.0)
    fdiff = np.diff(mel_f)
    ramps = np.subtract.outer(mel_f, fft_f)
    w = np.zeros((n_mels, len(fft_f)), dtype=np.float32)
    for i in range(n_mels):
        w[i] = np.maximum(0, np.minimum(-ramps[i] / fdiff[i], ramps[i + 2] / fdiff[i + 1]))
    w *= (2.0 / (mel_f[2: n_mels + 2] - mel_f[:n_mels]))[:, None]
    return w


def log_mel(y16, fb=None):
    """MelSpectrogram(128, 16000, 1024, 160, None, 30, 8000)(y, center=True): [128, T] float64."""
    y = np.pad(np.asarray(y16, dtype=np.float64), (512, 512), mode="reflect")
    t = 1 + (len(y) - 1024) // 160
    win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(1024) / 1024)
    frames = np.lib.stride_tricks.as_strided(y, (t, 1024), (y.strides[0] * 160, y.strides[0]))
    mag = np.abs(np.fft.rfft(frames * win, axis=1)).T
    fb = htk_filterbank() if fb is None else fb
    return np.log(np.maximum(fb.astype(np.float64) @ mag, 1e-5))


# ---------------------------------------------------------------------------------------------------------------- network
def _bn(sd, p, x):
    g, b, m, v = (np.asarray(sd[f"{p}.{k}"], dtype=np.float64) for k in ("weight", "bias", "running_mean", "running_var"))
    return (x - m) / np.sqrt(v + 1e-5) * g + b


def _conv3(x, w, bias=None):
    """x [T, F, Cin], w [Cout, Cin, 3, 3] -> [T, F, Cout] (padding 1)."""
    T, F, _ = x.shape
    w = np.asarray(w, dtype=np.float64)
    xp = np.pad(x, ((1, 1), (1, 1), (0, 0)))
    out = np.zeros((T, F, w.shape[0]))
    for kt in range(3):
        for kf in range(3):
            out += xp[kt: kt + T, kf: kf + F, :] @ w[:, :, kt, kf].T
    return out if bias is None else out + np.asarray(bias, dtype=np.float64)


def _tconv(x, w):
    """ConvTranspose2d(3x3, stride 2, padding 1, output_padding 1): x [T, F, Cin], w [Cin, Cout, 3, 3] -> [2T, 2F, Cout]."""
    T, F, _ = x.shape
    w = np.asarray(w, dtype=np.float64)
    buf = np.zeros((2 * T + 2, 2 * F + 2, w.shape[1]))
    for kt in range(3):
        for kf in range(3):
            buf[kt: kt + 2 * T: 2, kf: kf + 2 * F: 2] += x @ w[:, :, kt, kf]
    return buf[1: 2 * T + 1, 1: 2 * F + 1]


def _block(sd, p, x):
    h = np.maximum(_bn(sd, f"{p}.conv.1", _conv3(x, sd[f"{p}.conv.0.weight"])), 0)
    h = np.maximum(_bn(sd, f"{p}.conv.4", _conv3(h, sd[f"{p}.conv.3.weight"])), 0)
    if f"{p}.shortcut.weight" in sd:
        w = np.asarray(sd[f"{p}.shortcut.weight"], dtype=np.float64)[:, :, 0, 0]
        return h + x @ w.T + np.asarray(sd[f"{p}.shortcut.bias"], dtype=np.float64)
    return h + x


def _gru(x, sd, sfx, reverse):
    wi, wh = (np.asarray(sd[f"fc.0.gru.{k}_l0{sfx}"], dtype=np.float64) for k in ("weight_ih", "weight_hh"))
    bi, bh = (np.asarray(sd[f"fc.0.gru.{k}_l0{sfx}"], dtype=np.float64) for k in ("bias_ih", "bias_hh"))
    gi = x @ wi.T + bi
    h = np.zeros(256)
    out = np.zeros((len(x), 256))
    for t in (range(len(x) - 1, -1, -1) if reverse else range(len(x))):
        gh = wh @ h + bh
        r = 1 / (1 + np.exp(-(gi[t, :256] + gh[:256])))
        z = 1 / (1 + np.exp(-(gi[t, 256:512] + gh[256:512])))
        n = np.tanh(gi[t, 512:] + r * gh[512:])
        h = (1 - z) * n + z * h
        out[t] = h
    return out


def config_of(sd):
    """(n_blocks, n_gru, en_de_layers, inter_layers, en_out_channels) read off a state_dict."""
    E = len({k.split(".")[3] for k in sd if k.startswith("unet.encoder.layers.")})
    nb = len({k.split(".")[5] for k in sd if k.startswith("unet.encoder.layers.0.conv.")})
    inter = len({k.split(".")[3] for k in sd if k.startswith("unet.intermediate.layers.")})
    return nb, int("fc.0.gru.weight_ih_l0" in sd), E, inter, int(sd["cnn.weight"].shape[1])


def mel2hidden(mel, sd):
    """RMVPE.mel2hidden: mel [128, T] -> hidden [T, 360] float64 (padding to 32 ceil(T / 32) frames before the network)."""
    nb, n_gru, E, inter, _ = config_of(sd)
    T = mel.shape[1]
    Tp = 32 * ((T - 1) // 32 + 1)
    x = np.pad(np.asarray(mel, dtype=np.float64), ((0, 0), (0, Tp - T))).T[:, :, None]      # [Tp, 128, 1]
    x = _bn(sd, "unet.encoder.bn", x)
    skips = []
    for l in range(E):
        for k in range(nb):
            x = _block(sd, f"unet.encoder.layers.{l}.conv.{k}", x)
        skips.append(x)
        x = x.reshape(x.shape[0] // 2, 2, x.shape[1] // 2, 2, x.shape[2]).mean(axis=(1, 3))
    for i in range(inter):
        for k in range(nb):
            x = _block(sd, f"unet.intermediate.layers.{i}.conv.{k}", x)
    for i in range(E):
        p = f"unet.decoder.layers.{i}"
        x = np.maximum(_bn(sd, f"{p}.conv1.1", _tconv(x, sd[f"{p}.conv1.0.weight"])), 0)
        x = np.concatenate([x, skips[-1 - i]], axis=2)
        for k in range(nb):
            x = _block(sd, f"{p}.conv2.{k}", x)
    x = _conv3(x, sd["cnn.weight"], sd["cnn.bias"])                  # [Tp, 128, 3]
    x = x.transpose(0, 2, 1).reshape(Tp, 3 * N_MELS)                   # transpose(1, 2).flatten(-2): c * 128 + f
    if n_gru:
        x = np.concatenate([_gru(x, sd, "", False), _gru(x, sd, "_reverse", True)], axis=1)
        w, b = sd["fc.1.weight"], sd["fc.1.bias"]
    else:
        w, b = sd["fc.0.weight"], sd["fc.0.bias"]
    y = x @ np.asarray(w, dtype=np.float64).T + np.asarray(b, dtype=np.float64)
    return (1 / (1 + np.exp(-y)))[:T]


def decode(hidden, thred=0.03):
    """to_local_average_f0: hidden [T, 360] -> f0 [T] float64."""
    hidden = np.asarray(hidden, dtype=np.float64)
    c = np.argmax(hidden, axis=1)
    idx = np.arange(N_CLASS)[None, :]
    mask = (idx >= np.maximum(c - 4, 0)[:, None]) & (idx < np.minimum(c + 5, N_CLASS)[:, None])
    w = hidden * mask
    ps = (w * (idx * 20 + CONST)).sum(axis=1)
    ws = w.sum(axis=1)
    f0 = 10 * 2 ** (ps / (ws + (ws == 0)) / 1200)
    return f0 * ~(hidden.max(axis=1) < thred)


def infer_from_audio(audio, sd, sample_rate=16000, thred=0.03):
    return decode(mel2hidden(log_mel(resample(audio, sample_rate)), sd), thred)


def interp_f0(f0):
    uv = f0 == 0
    f = np.log2(f0 + uv)
    f[uv] = -np.inf
    if uv.any() and not uv.all():
        f[uv] = np.interp(np.where(uv)[0], np.where(~uv)[0], f[~uv])
    return 2 ** f, uv


def resample_align_curve(points, original_timestep, target_timestep, align_length):
    t_max = (len(points) - 1) * original_timestep
    curve = np.interp(np.arange(0, t_max, target_timestep), original_timestep * np.arange(len(points)), points).astype(points.dtype)
    d = align_length - len(curve)
    if d < 0:
        return curve[:align_length]
    if d > 0:
        return np.concatenate((curve, np.full(d, fill_value=curve[-1])), axis=0)
    return curve


def get_pitch_post(f0, samplerate, length, hop_size, speed=1, interp_uv=False):
    """RMVPE.get_pitch after infer_from_audio (inference.py:53-70)."""
    f0, uv = interp_f0(np.asarray(f0))
    hop = int(np.round(hop_size * speed))
    ts = hop / samplerate
    f0_res = resample_align_curve(f0, 0.01, ts, length)
    uv_res = resample_align_curve(uv.astype(np.float32), 0.01, ts, length) > 0.5
    if not interp_uv:
        f0_res[uv_res] = 0
    return f0_res, uv_res
