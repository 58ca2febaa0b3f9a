"""Generator of G30 (tests/golden/g30_words.npz): the reference's own results for the cases of tests/words_cases.py, in fp32
on the CPU - RhythmRegulator.forward (modules/fastspeech/tts_modules.py) on the padded batches as they stand, and, item by
item at the item's own sizes as the reference's front end runs (B = 1, nothing padded), its expressions for word_dur and for
the `midi` input (inference/ds_variance.py, preprocess_input) on the reference's LengthRegulator and mel2ph_to_dur.  Only
results are stored, padded with zeros to the case's batch; the tests rebuild the inputs from tests/words_cases.py.

Runs on a machine with the reference tree; the tests only read the .npz.  `utils/training_utils.py` on the import path pulls
in `lightning`, which is never executed here and is stubbed as tests/golden/make_golden_deploy.py does.

    python tests/golden/make_golden_words.py /path/to/reference
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import words_cases as wc  # noqa: E402
from make_golden_deploy import _stub_lightning  # noqa: E402


def main(ref_root):
    _stub_lightning()
    sys.path.insert(0, ref_root)
    from modules.fastspeech.tts_modules import LengthRegulator, RhythmRegulator, mel2ph_to_dur
    torch.set_num_threads(1)
    lr, rr = LengthRegulator(), RhythmRegulator()
    out = {}

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(a))

    def aligned(word_dur, n_words, n_frames):
        mel2word = lr(word_dur)
        if mel2word.shape[1] != n_frames:
            mel2word = F.pad(mel2word, [0, n_frames - mel2word.shape[1]], value=mel2word[0, -1])
            word_dur = mel2ph_to_dur(mel2word, n_words)
        return word_dur

    for name, c in wc.rhythm_cases().items():
        if not c.get("oracle_only"):
            out[f"rhythm_{name}"] = rr(t(c["pred"]), t(c["ph2word"]), t(c["word_dur"])).numpy()

    for name, c in wc.word_cases().items():
        if c.get("oracle_only"):
            continue
        res = np.zeros((len(c["sizes"]), c["W"]), np.int64)
        for b, (n, n_words) in enumerate(c["sizes"]):
            dur = t(c["dur"][b:b + 1, :n])
            index = t(c["index"][b:b + 1, :n]) if "index" in c else torch.cumsum(~t(c["slur"][b:b + 1, :n]).bool(), dim=1)
            word_dur = dur.new_zeros(1, n_words + 1).scatter_add(1, index, dur)[:, 1:]
            if c["totals"] is not None:
                word_dur = aligned(word_dur, n_words, int(c["totals"][b]))
            res[b, :n_words] = word_dur[0].numpy()
        out[f"word_{name}"] = res

    for name, c in wc.midi_cases().items():
        if c.get("oracle_only"):
            continue
        by_word = c["ph2word"] is not None
        bsz = len(c["sizes"])
        res = np.zeros((bsz, c["ph2word"].shape[1] if by_word else c["group_dur"].shape[1]), np.int64)
        for b, (n_notes, n_groups) in enumerate(c["sizes"]):
            note_midi, note_dur = t(c["note_midi"][b:b + 1, :n_notes]), t(c["note_dur"][b:b + 1, :n_notes])
            group_dur = t(c["group_dur"][b:b + 1, :n_groups])
            mel2note, mel2group = lr(note_dur), lr(group_dur)
            assert mel2note.shape[1] == mel2group.shape[1] == c["t_len"][b]
            frame_midi = torch.gather(F.pad(note_midi, [1, 0]), 1, mel2note)
            mel2dur = torch.gather(F.pad(group_dur, [1, 0], value=1), 1, mel2group)
            g_midi = frame_midi.new_zeros(1, n_groups + 1).scatter_add(1, mel2group, frame_midi / mel2dur)[:, 1:]
            if by_word:
                n_ph = c["n_ph"][b]
                g_midi = torch.gather(F.pad(g_midi, [1, 0]), 1, t(c["ph2word"][b:b + 1, :n_ph]))
            r = g_midi.round().long()[0].numpy()
            res[b, :len(r)] = r
        out[f"midi_{name}"] = res

    path = os.path.join(HERE, "g30_words.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main(sys.argv[1])
