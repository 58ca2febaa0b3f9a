"""numpy restatement of validation scoring (include/dsdenoise.h, "Validation scoring") under its rounding rule: a term
is formed in fp32 wherever only IEEE add / sub / mul / div is involved (numpy float32 arrays: every operation rounded on its
own), whatever goes through log / exp is evaluated in float64 from the fp32 input, and the terms are summed in float64
(math.fsum: the correctly rounded sum, so any fixed double summation order of the library is within a few ulps of it).

The two noising formulas are restated in fp32 and are meant to be matched bit for bit.
"""
import math

import numpy as np

f32 = np.float32


def _a(x, dt=np.float32):
    return np.ascontiguousarray(np.asarray(x), dtype=dt)


def _bcast(v, x):
    return _a(v).reshape((-1,) + (1,) * (x.ndim - 1))


# ------------------------------------------------------------------------------------------- noising
def diffuse_ddpm(x0, eps, a, c):
    """ddpm.py:206-210 -> (x_t, target): fl(fl(a x0) + fl(c eps)), eps"""
    x0, eps = _a(x0), _a(eps)
    return _bcast(a, x0) * x0 + _bcast(c, x0) * eps, eps


def diffuse_reflow(x0, eps, t):
    """reflow.py:38,41 -> (x_t, target): target = fl(x0 - eps), x_t = fl(eps + fl(t target))"""
    x0, eps = _a(x0), _a(eps)
    target = x0 - eps
    return eps + _bcast(t, x0) * target, target


def seeded_t_ddpm(u, k_step):
    return np.minimum(k_step - 1, np.floor(_a(u).astype(np.float64) * k_step)).astype(np.int64)


def seeded_t_reflow(u, t_start):
    return (f32(t_start) + f32(1.0 - t_start) * _a(u)).astype(np.float32)


# ------------------------------------------------------------------------------------------- losses
def lognorm_weight(t):
    """reflow_loss.py:26-34 in float64 from the fp32 t"""
    t = np.clip(_a(t).astype(np.float64), 1e-7, 1.0 - 1e-7)
    l = np.log(t / (1.0 - t))
    return 0.398942 / t / (1.0 - t) * np.exp(-0.5 * (l * l)) + 1e-7


def masked_loss(kind, pred, target, non_padding=None, t=None):
    """-> (sum, mean over all elements).  pred, target [B, ..., T]; non_padding [B, T]; t [B]"""
    pred, target = _a(pred), _a(target)
    b, cols = pred.shape[0], pred.shape[-1]
    p3, t3 = pred.reshape(b, -1, cols), target.reshape(b, -1, cols)
    if non_padding is not None:
        m = _a(non_padding).reshape(b, 1, cols)
        p3, t3 = p3 * m, t3 * m
    d = p3 - t3
    term = (np.abs(d) if kind == "l1" else d * d).astype(np.float64)
    if t is not None:
        term = term * lognorm_weight(t).reshape(b, 1, 1)
    s = math.fsum(term.reshape(-1).tolist())
    return s, s / pred.size


# ------------------------------------------------------------------------------------------- curve metrics
def curve_stats(pred, target, mask=None, tolerance=0.0):
    pred, target = _a(pred).reshape(-1), _a(target).reshape(-1)
    if mask is not None:
        keep = np.asarray(mask).reshape(-1).astype(bool)
        pred, target = pred[keep], target[keep]
    r = target - pred
    return {"close": int(np.count_nonzero(np.abs(pred - target) <= f32(tolerance))), "total": int(pred.size),
            "sum_target": math.fsum(target.astype(np.float64).tolist()),
            "sum_target_sq": math.fsum((target * target).astype(np.float64).tolist()),
            "sum_residual_sq": math.fsum((r * r).astype(np.float64).tolist())}


def curve_accuracy(s):
    return s["close"] / s["total"]


def curve_r2(s):
    return 1 - s["sum_residual_sq"] / (s["sum_target_sq"] - s["sum_target"] ** 2 / s["total"])


# ------------------------------------------------------------------------------------------- durations
def word_sums(values, ph2word, n_words):
    """[B, n_words - 1] fp32: the values of each word added in phoneme order (torch's CPU scatter_add)[:, 1:]"""
    values, ph2word = _a(values), np.asarray(ph2word)
    out = np.zeros((values.shape[0], n_words), np.float32)
    for b in range(values.shape[0]):
        for l in range(values.shape[1]):
            w = int(ph2word[b, l])
            if 0 <= w < n_words:
                out[b, w] = out[b, w] + values[b, l]
    return out[:, 1:]


def _seq_sum(values):
    out = np.zeros(values.shape[0], np.float32)
    for l in range(values.shape[1]):
        out = out + values[:, l]
    return out


def _dur_terms(x, y, offset, kind):
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.log((_a(x) + f32(offset)).astype(np.float64)) - np.log((_a(y) + f32(offset)).astype(np.float64))
    if kind == "mse":
        return d * d
    ad = np.abs(d)
    return np.where(ad < 1.0, 0.5 * (d * d), ad - 0.5)


def dur_score(dur_pred, dur_gt, ph2word, mask=None, n_words=None, offset=1.0, loss_type="mse", rhythm_tolerance=0.05,
              pdur_tolerance=0.2):
    dur_pred, dur_gt, ph2word = _a(dur_pred), _a(dur_gt), np.asarray(ph2word).astype(np.int64)
    if n_words is None:
        n_words = int(ph2word.max()) + 1
    b, length = dur_pred.shape
    clamped = np.where(dur_pred < 0, f32(0), dur_pred).astype(np.float32)
    wp, wg = word_sums(clamped, ph2word, n_words), word_sums(dur_gt, ph2word, n_words)
    sums = [math.fsum(_dur_terms(dur_pred, dur_gt, offset, loss_type).reshape(-1).tolist()),
            math.fsum(_dur_terms(wp, wg, offset, loss_type).reshape(-1).tolist()),
            math.fsum(_dur_terms(_seq_sum(clamped), _seq_sum(dur_gt), offset, loss_type).reshape(-1).tolist())]
    means = [sums[0] / (b * length), sums[1] / (b * (n_words - 1)), sums[2] / b]
    # RhythmCorrectness (duration.py:41-59)
    if mask is None:
        wmask = np.ones(wp.shape, bool)
        pmask = np.ones(dur_pred.shape, bool)
    else:
        pmask = np.asarray(mask).astype(bool)
        wmask = word_sums(pmask.astype(np.float32), ph2word, n_words) > 0
    correct = (np.abs(wp - wg) <= wg * f32(rhythm_tolerance)) & wmask
    # PhonemeDurationAccuracy (duration.py:83-94) through RhythmRegulator (tts_modules.py:267-275)
    inw = (ph2word >= 1) & (ph2word < n_words)
    pd = (clamped * (ph2word > 0).astype(np.float32)).astype(np.float32)
    alpha_w = (wg / np.maximum(wp, f32(1e-5))).astype(np.float32)
    alpha = np.zeros(dur_pred.shape, np.float32)
    for i in range(b):
        for l in range(length):
            if inw[i, l]:
                alpha[i, l] = alpha_w[i, ph2word[i, l] - 1]
    align = np.rint(pd * alpha).astype(np.float32)
    accurate = (np.abs(align - dur_gt) <= dur_gt * f32(pdur_tolerance)) & pmask
    return {"sums": sums, "means": means, "wdur_pred": wp, "wdur_gt": wg,
            "counts": [int(correct.sum()), int(wmask.sum()), int(accurate.sum()), int(pmask.sum())]}


def dur_loss(res, lambda_pdur=0.6, lambda_wdur=0.3, lambda_sdur=0.1):
    m = res["means"]
    return lambda_pdur * m[0] + lambda_wdur * m[1] + lambda_sdur * m[2]
