"""Numpy restatement of the reference's to_viterbi_f0 (modules/pe/rmvpe/utils.py:26-43) and of the
librosa.sequence.viterbi it calls, as in librosa 0.9.2 (the reference pins librosa < 0.10): parity unpinned against librosa
itself, which is not installed where these tests run.  No import from the product.

viterbi_path(hidden, chain): chain="ref" forms prob and log_prob in float32, as the reference does (hidden.cpu().numpy()
is float32, so librosa.util.tiny(prob) is the float32 tiny); chain="f64" forms them in float64 from the float32 hidden
with the same eps.  Either way value, the transition terms and every comparison are float64, first index on ties."""
import numpy as np

N_CLASS, CONST = 360, 1997.3794084376191
EPS = np.finfo(np.float32).tiny          # librosa.util.tiny of a float32 array: 1.1754944e-38, log = -87.3365


def transition():
    """utils.py:29-31: rows divided by their own sums (smaller near both ends: not Toeplitz)."""
    xx, yy = np.meshgrid(range(N_CLASS), range(N_CLASS))
    tr = np.maximum(30 - abs(xx - yy), 0)
    return tr / tr.sum(axis=1, keepdims=True)


_LOG_TRANS = np.log(transition() + np.float64(EPS))
_LOG_P_INIT = np.log(np.float64(1.0 / N_CLASS) + np.float64(EPS))


def log_prob(hidden, chain="ref"):
    hidden = np.asarray(hidden, dtype=np.float32)
    if chain == "ref":
        prob = hidden.T
        prob = prob / prob.sum(axis=0)                    # float32 (utils.py:35-37)
        return np.log(prob.T + EPS).astype(np.float64)    # float32 log, then value[t] = log_prob[t] + ... in float64
    assert chain == "f64"
    h = hidden.astype(np.float64)
    return np.log(h / h.sum(axis=1, keepdims=True) + np.float64(EPS))


def _forward(lp):
    T = lp.shape[0]
    value = np.zeros((T, N_CLASS))
    ptr = np.zeros((T, N_CLASS), dtype=np.int64)
    value[0] = lp[0] + _LOG_P_INIT
    for t in range(1, T):
        trans_out = value[t - 1][:, None] + _LOG_TRANS       # [k, j]
        ptr[t] = np.argmax(trans_out, axis=0)                 # first index on ties
        value[t] = lp[t] + trans_out[ptr[t], np.arange(N_CLASS)]
    return value, ptr


def _backtrack(value, ptr):
    T = value.shape[0]
    state = np.zeros(T, dtype=np.int64)
    state[-1] = np.argmax(value[-1])
    for t in range(T - 2, -1, -1):
        state[t] = ptr[t + 1, state[t + 1]]
    return state


def viterbi_path(hidden, chain="ref"):
    """hidden [T, 360] float32 -> the state sequence [T] int64 of librosa.sequence.viterbi(prob, transition)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return _backtrack(*_forward(log_prob(hidden, chain)))


def on_path_margin(hidden, chain="ref"):
    """The smallest gap between the best and the second-best predecessor along the chosen path, and between the two
    largest final values: how far the recursion is from choosing another path."""
    value, ptr = _forward(log_prob(hidden, chain))
    state = _backtrack(value, ptr)
    top = np.sort(value[-1])
    margin = top[-1] - top[-2]
    for t in range(1, len(state)):
        cand = np.sort(value[t - 1] + _LOG_TRANS[:, state[t]])
        margin = min(margin, cand[-1] - cand[-2])
    return float(margin)


def path_score(hidden, state, chain="f64"):
    """log p_init + sum of log_prob on the path + sum of log_trans along it."""
    lp = log_prob(hidden, chain)
    state = np.asarray(state)
    s = _LOG_P_INIT + lp[np.arange(len(state)), state].sum()
    return float(s + _LOG_TRANS[state[:-1], state[1:]].sum())


def to_local_average_f0(hidden, center=None, thred=0.03):
    """utils.py:8-23 in float64: hidden [T, 360], center [T] (None: the argmax) -> f0 [T]."""
    hidden = np.asarray(hidden, dtype=np.float64)
    c = np.argmax(hidden, axis=1) if center is None else np.asarray(center)
    idx = np.arange(N_CLASS)[None, :]
    mask = (idx >= np.clip(c - 4, 0, None)[:, None]) & (idx < np.clip(c + 5, None, N_CLASS)[:, None])
    w = hidden * mask
    ps = (w * (idx * 20 + CONST)).sum(axis=1)
    ws = w.sum(axis=1)
    f0 = 10 * 2 ** (ps / (ws + (ws == 0)) / 1200)
    return f0 * ~(hidden.max(axis=1) < thred)


def to_viterbi_f0(hidden, thred=0.03, chain="ref"):
    return to_local_average_f0(hidden, viterbi_path(hidden, chain), thred)


# ---------------------------------------------------------------------------------------------------------------- inputs
def melody(T, seed, kind=1):
    """A Gaussian ridge (sigma 2 classes, height 0.9) on 180 + 60 sin(t / 17) plus jitter; on 12 % of the frames a stronger
    ridge 60 classes up (the octave errors of a per-frame argmax); uniform noise of 0.02.  kind 2: five unvoiced frames
    (everything below thred) as well.  -> hidden [T, 360] float32."""
    rng = np.random.default_rng(seed)
    t = np.arange(T)
    mu = 180 + 60 * np.sin(t / 17.0) + rng.normal(0, 0.7, T)
    idx = np.arange(N_CLASS)[None, :]
    h = 0.9 * np.exp(-0.5 * ((idx - mu[:, None]) / 2.0) ** 2)
    octave = rng.random(T) < 0.12
    if T >= 2 and not octave.any():
        octave[rng.integers(T)] = True
    h += octave[:, None] * 0.97 * np.exp(-0.5 * ((idx - (mu[:, None] + 60)) / 2.0) ** 2)
    h += rng.random((T, N_CLASS)) * 0.02
    if kind == 2 and T > 8:
        lo = int(rng.integers(1, T - 6))
        h[lo: lo + 5] *= 0.02
    return np.clip(h, 0, 1).astype(np.float32)


# (name, T, seed, kind): every length class of the kernel - one frame, two, below / across the 32-row chunks of the backtrack
# (33, 37, 64), several chunks (200), a 10-s clip (1001)
MELODIES = [("t1", 1, 11, 1), ("t2", 2, 12, 1), ("t33", 33, 13, 1), ("t37", 37, 14, 2), ("t64", 64, 15, 1),
            ("t200", 200, 16, 2), ("t1001", 1001, 23, 1)]


def zero_probability():
    """12 frames of exact zeros except 0.8 at class 100 (frames 0-5) and class 200 (frames 6-11): the path jumps once, outside
    the band, at the price log(eps)."""
    h = np.zeros((12, N_CLASS), dtype=np.float32)
    h[:6, 100] = 0.8
    h[6:, 200] = 0.8
    return h, np.array([100] * 6 + [200] * 6)


def edge_rows():
    """20 frames at 0.01 with 0.9 at class 2 (frames 0-9) and class 357 (frames 10-19): the row-normalised transitions at
    the ends make the path [359] * 10 + [357] * 10."""
    h = np.full((20, N_CLASS), 0.01, dtype=np.float32)
    h[:10, 2] = 0.9
    h[10:, 357] = 0.9
    return h, np.array([359] * 10 + [357] * 10)


def cases():
    """name -> hidden, every host case."""
    out = {name: melody(T, seed, kind) for name, T, seed, kind in MELODIES}
    out["zero_probability"] = zero_probability()[0]
    out["edge_rows"] = edge_rows()[0]
    return out
