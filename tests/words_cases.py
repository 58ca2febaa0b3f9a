"""The inputs of the score-algebra checks (dsd_word_dur, dsd_group_midi, dsd_rhythm_align), shared by the generator of G30
(tests/golden/make_golden_words.py: the reference's results), tests/test_words_host.py (the numpy oracle against G30) and
tests/test_gpu_words.py (the kernels against the oracle).  Every case is a dict of padded numpy arrays plus `sizes`, the
real counts of each item; padding is what the interface says it is: ph2word 0, slur 1 with dur 0, durations 0.  All values
are in the normal fp32 range.  The cases marked `oracle_only` use what the interface defines beyond the reference (an index
outside the words, totals that differ between notes and groups) and are not in G30."""
import numpy as np

F = np.float32


def _pad(rows, dtype, fill=0):
    n = max(len(r) for r in rows)
    out = np.full((len(rows), n), fill, dtype)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out


def _split(total, parts, rng, zeros=0):
    """`parts` non-negative ints summing to `total`, `zeros` of them 0"""
    live = parts - zeros
    cuts = np.sort(rng.choice(np.arange(1, total), live - 1, replace=False)) if live > 1 else np.array([], np.int64)
    d = np.diff(np.concatenate([[0], cuts, [total]])).astype(np.int64)
    out = np.zeros(parts, np.int64)
    out[np.sort(rng.choice(parts, live, replace=False))] = d
    return out


def rhythm_cases():
    rng = np.random.default_rng(3001)
    cases = {}

    def add(name, pred, ph2word, word_dur, **kw):
        cases[name] = dict(pred=_pad(pred, F), ph2word=_pad(ph2word, np.int64), word_dur=_pad(word_dur, np.int64),
                           sizes=[(len(p), len(w)) for p, w in zip(ph2word, word_dur)], **kw)

    add("single", [[3.25]], [[1]], [[7]])
    add("one_word", [[1.5, 2.25, 0.75, 4.0, 3.5, 1.25, 2.0]], [[1] * 7], [[41]])
    # word 2's predictions are all 0 (the eps branch), word 3 has duration 0, the last phone is padding with a prediction
    add("eps_zero_pad", [[2.0, 3.0, 0.0, 0.0, 5.0, 1.0, 9.5]], [[1, 1, 2, 2, 3, 4, 0]], [[10, 6, 0, 3]])
    # 1 * (3 / 2) = 1.5 -> 2 and 1 * (2 / 4) = 0.5 -> 0: ties go to even, up and down
    add("ties", [[1.0, 1.0], [1.0, 1.0, 1.0, 1.0]], [[1, 1], [1, 1, 1, 1]], [[3], [2]])
    add("unsorted", [[1.5, 2.5, 0.5, 3.0, 2.0, 1.0, 4.5, 2.75]], [[3, 1, 2, 3, 1, 0, 2, 3]], [[12, 9, 20]])
    sizes = [(9, 4), (17, 7), (5, 2)]
    pred, p2w, wd = [], [], []
    for n_ph, n_w in sizes:
        div = _split(n_ph, n_w, rng) if n_w > 1 else np.array([n_ph])
        div = np.maximum(div, 1)
        div[-1] += n_ph - div.sum()
        p2w.append(np.repeat(np.arange(1, n_w + 1), div))
        pred.append(rng.uniform(0.5, 30.0, n_ph).astype(F))
        wd.append(rng.integers(1, 60, n_w))
    add("batch3", pred, p2w, wd)
    div = np.ones(2048, np.int64)
    add("largest", [rng.uniform(0.5, 30.0, 2048).astype(F)], [np.repeat(np.arange(1, 2049), div)], [rng.integers(0, 9, 2048)])
    # 2048 phones in 300 words of uneven size: long in-order sums
    div = np.maximum(_split(2048, 300, rng), 1)
    div[np.argmax(div)] -= div.sum() - 2048
    add("long_words", [rng.uniform(0.5, 30.0, 2048).astype(F)], [np.repeat(np.arange(1, 301), div)], [rng.integers(1, 400, 300)])
    add("outside", [[1.5, 2.5, 3.5, 4.5]], [[1, 5, 2, -3]], [[4, 6]], oracle_only=True)
    return cases


def word_cases():
    rng = np.random.default_rng(3002)
    cases = {}
    # from ph2word: B = 3, padded; the phones' totals are 30, 51, 12
    p2w = [[1, 1, 2, 3, 3, 3], [1, 2, 2, 3, 4, 4, 5, 5, 5], [1, 1]]
    dur = [[4, 6, 5, 3, 7, 5], [9, 2, 8, 1, 6, 5, 7, 3, 10], [5, 7]]
    base = dict(dur=_pad(dur, np.int64), index=_pad(p2w, np.int64), W=5, sizes=[(6, 3), (9, 5), (2, 1)])
    cases["index_plain"] = dict(base, totals=None)
    cases["index_totals"] = dict(base, totals=np.array([30, 44, 19], np.int64))           # equal, smaller, larger
    # from slurs: a leading slur (dropped), a slur run, padding notes (slur 1, dur 0); totals larger, smaller, equal
    slur = [[1, 0, 1, 1, 0, 0, 1], [0, 0, 1, 0], [0, 1, 1, 1, 1, 0, 0, 1, 0]]
    dur = [[3, 10, 4, 2, 8, 6, 5], [7, 9, 11, 4], [5, 3, 2, 6, 1, 9, 12, 2, 8]]
    base = dict(dur=_pad(dur, np.int64), slur=_pad(slur, np.uint8, 1), W=5, sizes=[(7, 3), (4, 3), (9, 4)])
    cases["slur_plain"] = dict(base, totals=None)
    cases["slur_totals"] = dict(base, totals=np.array([40, 20, 48], np.int64))
    # a zero word at the end: the rest goes to the last word with a non-zero duration, not to the last word
    cases["rest_skips_zero"] = dict(dur=np.array([[5, 0, 7, 0]], np.int64), index=np.array([[1, 2, 3, 4]], np.int64), W=4,
                                    sizes=[(4, 4)], totals=np.array([20], np.int64))
    d = _split(4096, 2048, rng, zeros=100)
    cases["largest"] = dict(dur=d[None], slur=np.zeros((1, 2048), np.uint8), W=2048, sizes=[(2048, 2048)],
                            totals=np.array([4096], np.int64))
    d = _split(4096, 2048, rng, zeros=60)
    cases["largest_index"] = dict(dur=d[None], index=rng.permutation(np.arange(1, 2049))[None].astype(np.int64), W=2048,
                                  sizes=[(2048, 2048)], totals=np.array([4000], np.int64), oracle_only=True)
    return cases


def midi_cases():
    rng = np.random.default_rng(3003)
    cases = {}

    def notes(n, total):
        return rng.integers(96, 320, n).astype(F) / F(4), _split(total, n, rng)        # quarter tones: some means tie at .5

    # phones as groups: B = 3 with different note, phone and frame counts; item 0 has a group of 300 frames across several
    # notes and a zero-frame group between two others
    t_len = [420, 131, 77]
    n_notes, n_groups = [9, 5, 3], [6, 11, 2]
    midi, ndur, gdur = [], [], []
    for b in range(3):
        m, d = notes(n_notes[b], t_len[b])
        midi.append(m)
        ndur.append(d)
        gdur.append(np.array([40, 300, 0, 25, 30, 25], np.int64) if b == 0 else _split(t_len[b], n_groups[b], rng))
    base = dict(note_midi=_pad(midi, F), note_dur=_pad(ndur, np.int64), group_dur=_pad(gdur, np.int64), T=420, t_len=t_len,
                sizes=list(zip(n_notes, n_groups)))
    cases["phones"] = dict(base, ph2word=None)
    # words as groups, gathered to phones
    p2w = [[1, 1, 2, 2, 2, 3, 4, 5, 5, 6], [1, 2, 3, 3, 4, 5, 6, 7, 8, 9, 10, 11, 11], [1, 2, 2]]
    cases["words"] = dict(base, ph2word=_pad(p2w, np.int64), n_ph=[len(p) for p in p2w])
    cases["one_group"] = dict(note_midi=np.array([[61.5, 64.0, 59.25]], F), note_dur=np.array([[3, 5, 2]], np.int64),
                              group_dur=np.array([[10]], np.int64), T=10, t_len=[10], sizes=[(3, 1)], ph2word=None)
    m, d = notes(2048, 4096)
    cases["largest"] = dict(note_midi=m[None], note_dur=d[None], group_dur=_split(4096, 2048, rng, zeros=31)[None], T=4096,
                            t_len=[4096], sizes=[(2048, 2048)], ph2word=rng.integers(0, 2049, (1, 2048)).astype(np.int64),
                            n_ph=[2048])
    # beyond the reference: the groups reach past the notes' total (those frames' MIDI is 0), the notes past T, an index past G
    cases["mismatch"] = dict(note_midi=np.array([[60.0, 67.5, 72.25]], F), note_dur=np.array([[10, 6, 30]], np.int64),
                             group_dur=np.array([[7, 0, 12, 40]], np.int64), T=30, t_len=[30], sizes=[(3, 4)],
                             ph2word=np.array([[1, 9, 3, 4, 0, -1]], np.int64), n_ph=[6], oracle_only=True)
    return cases
