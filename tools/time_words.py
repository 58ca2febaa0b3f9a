"""What the variance front end's score algebra costs for one segment: the three device entries (diffsinger_amd/words.py:
dsd_word_dur, dsd_group_midi, dsd_rhythm_align) against the torch expressions of variance_harness.preprocess_input and
variance.RhythmRegulator on the GPU, in one process.  The harness's word_dur path sizes mel2word by a read-back, as the
reference does; the entries read nothing back.  Nothing is asserted; one JSON line.  These run once per segment, so the
figures say what the interface costs, not where a render's time goes.

    python tools/time_words.py [--seconds 11.6] [--repeat 50]

Every timing is wall-clock around the call with a device synchronisation on both sides, the median of `--repeat` runs
after 5 warm-up runs.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffsinger_amd import words  # noqa: E402
from diffsinger_amd.harness import length_regulator  # noqa: E402
from diffsinger_amd.variance import RhythmRegulator  # noqa: E402
from diffsinger_amd.variance_harness import VarianceHarness, mel2ph_to_dur  # noqa: E402

HOP = 512 / 44100


def timed(fn, repeat):
    for _ in range(5):
        fn()
    ms = []
    for _ in range(repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ms), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=11.6)
    ap.add_argument("--repeat", type=int, default=50)
    args = ap.parse_args()
    rng = np.random.Generator(np.random.PCG64(3100))
    n_frames = int(args.seconds / HOP)
    n_word = max(1, int(args.seconds / 0.36))
    n_ph, n_note = 2 * n_word, n_word + n_word // 3          # two phones a word; every third word has a slurred note
    cuts = np.sort(rng.choice(np.arange(1, n_frames), n_note - 1, replace=False))
    note_dur = torch.from_numpy(np.diff(np.concatenate([[0], cuts, [n_frames]]))[None]).cuda()
    slur = np.zeros(n_note, bool)
    slur[np.arange(n_word // 3) * 4 + 1] = True
    is_slur = torch.from_numpy(slur[None]).cuda()
    note_midi = torch.from_numpy(rng.uniform(48, 72, (1, n_note)).astype(np.float32)).cuda()
    ph2word = torch.arange(1, n_word + 1, device="cuda").repeat_interleave(2)[None]
    pred = torch.from_numpy(rng.uniform(1, 30, (1, n_ph)).astype(np.float32)).cuda()
    rr = RhythmRegulator()

    def torch_word_dur():
        note2word = torch.cumsum(~is_slur, dim=1)
        word_dur = note_dur.new_zeros(1, n_word + 1).scatter_add(1, note2word, note_dur)[:, 1:]
        mel2word = length_regulator(word_dur)
        if mel2word.shape[1] != n_frames:
            mel2word = F.pad(mel2word, [0, n_frames - mel2word.shape[1]], value=mel2word[0, -1])
            word_dur = mel2ph_to_dur(mel2word, n_word)
        return word_dur, mel2word

    word_dur, mel2word = torch_word_dur()
    mel2note = length_regulator(note_dur)

    def torch_midi():
        frame_midi = torch.gather(F.pad(note_midi, [1, 0]), 1, mel2note)
        w_midi = VarianceHarness._per_group_mean(frame_midi, mel2word, word_dur, n_word)
        return torch.gather(F.pad(w_midi, [1, 0]), 1, ph2word).round().long()

    out = {"seconds": args.seconds, "repeat": args.repeat, "frames": n_frames, "phones": n_ph, "words": n_word, "notes": n_note}
    got = words.word_dur(note_dur, n_word, slur=is_slur, totals=[n_frames])
    out["word_dur_equal"] = bool(torch.equal(got, word_dur))
    out["midi_mismatches"] = int((words.group_midi(note_midi, note_dur, word_dur, n_frames, ph2word=ph2word) != torch_midi()).sum())
    out["rhythm_mismatches"] = int((words.rhythm_align(pred, ph2word, word_dur) != rr(pred, ph2word, word_dur)).sum())
    out["word_dur_torch_ms"] = timed(torch_word_dur, args.repeat)
    out["word_dur_entry_ms"] = timed(lambda: words.word_dur(note_dur, n_word, slur=is_slur, totals=[n_frames]), args.repeat)
    out["group_midi_torch_ms"] = timed(torch_midi, args.repeat)
    out["group_midi_entry_ms"] = timed(lambda: words.group_midi(note_midi, note_dur, word_dur, n_frames, ph2word=ph2word), args.repeat)
    out["rhythm_torch_ms"] = timed(lambda: rr(pred, ph2word, word_dur), args.repeat)
    out["rhythm_entry_ms"] = timed(lambda: words.rhythm_align(pred, ph2word, word_dur), args.repeat)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
