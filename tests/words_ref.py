"""The variance front end's score algebra restated in numpy, one fp32 operation at a time in index order: the oracle of
dsd_word_dur, dsd_group_midi and dsd_rhythm_align (include/dsdenoise.h states the same sequences).  Loops over rows and
entries: the rows are at most 2048 long and the fixtures small.  tests/test_words_host.py holds it against the reference's own
results (G30: RhythmRegulator and the ds_variance.py expressions on the CPU; G13: preprocess_input)."""
import numpy as np

F = np.float32


def word_dur(dur, n_words, index=None, slur=None, totals=None):
    """dur [B, N] int64, index [B, N] (0 = padding) or slur [B, N] bool -> (word_dur [B, W] int64, index [B, N] int64)"""
    dur = np.asarray(dur, np.int64)
    assert (index is None) != (slur is None)
    if slur is not None:
        index = np.cumsum(~np.asarray(slur, bool), axis=1)
    index = np.asarray(index, np.int64)
    out = np.zeros((dur.shape[0], n_words), np.int64)
    for b in range(dur.shape[0]):
        for i in range(dur.shape[1]):
            if 1 <= index[b, i] <= n_words:
                out[b, index[b, i] - 1] += dur[b, i]
        if totals is not None:
            total = int(totals[b])
            raw = out[b].copy()
            c = np.minimum(np.cumsum(np.clip(raw, 0, None)), total)
            out[b] = np.diff(c, prepend=0)
            nz = np.nonzero(raw > 0)[0]
            if len(nz):
                out[b, nz[-1]] += total - c[-1]
    return out, index


def owners(dur, n_frames):
    """LengthRegulator at T = n_frames: frame -> 1-based owner, 0 at or past the total"""
    c = np.minimum(np.cumsum(np.clip(np.asarray(dur, np.int64), 0, n_frames)), n_frames)
    return np.array([(np.searchsorted(c, p, side="right") + 1) if p < c[-1] else 0 for p in range(n_frames)], np.int64)


def group_midi(note_midi, note_dur, group_dur, n_frames, ph2word=None):
    """-> [B, G] int64, or [B, L] gathered through ph2word"""
    note_midi, group_dur = np.asarray(note_midi, F), np.asarray(group_dur, np.int64)
    bsz, n_groups = group_dur.shape
    r = np.zeros((bsz, n_groups + 1), np.int64)
    for b in range(bsz):
        frame_midi = np.concatenate([np.zeros(1, F), note_midi[b]])[owners(note_dur[b], n_frames)]
        mel2g = owners(group_dur[b], n_frames)
        sums = np.zeros(n_groups + 1, F)
        for p in range(n_frames):
            g = mel2g[p]
            if g:
                sums[g] = F(sums[g] + F(frame_midi[p] / F(group_dur[b, g - 1])))
        r[b] = np.rint(sums).astype(np.int64)
        r[b, 0] = 0
    if ph2word is None:
        return r[:, 1:]
    ph2word = np.asarray(ph2word, np.int64)
    idx = np.where((ph2word >= 1) & (ph2word <= n_groups), ph2word, 0)
    return np.take_along_axis(r, idx, axis=1)


def rhythm_align(ph_dur_pred, ph2word, word_dur_, eps=1e-5):
    pred, ph2word, word_dur_ = np.asarray(ph_dur_pred, F), np.asarray(ph2word, np.int64), np.asarray(word_dur_, np.int64)
    bsz, n_ph = pred.shape
    n_words = word_dur_.shape[1]
    out = np.zeros((bsz, n_ph), np.int64)
    for b in range(bsz):
        d = pred[b] * (ph2word[b] > 0).astype(F)
        s = np.zeros(n_words + 1, F)
        for i in range(n_ph):
            if 1 <= ph2word[b, i] <= n_words:
                s[ph2word[b, i]] = F(s[ph2word[b, i]] + d[i])
        alpha = np.zeros(n_words + 1, F)
        alpha[1:] = word_dur_[b].astype(F) / np.maximum(s[1:], F(eps))
        for i in range(n_ph):
            if 1 <= ph2word[b, i] <= n_words:
                out[b, i] = np.int64(np.rint(F(d[i] * alpha[ph2word[b, i]])))
    return out
