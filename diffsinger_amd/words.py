"""The variance front end's score algebra on the device (include/dsdenoise.h: dsd_word_dur, dsd_group_midi,
dsd_rhythm_align), on torch tensors: word durations from ph2word or from the note slurs, the `midi` input of the variance
model, and the rhythm regulator that turns predicted phone durations into integer ones.  One function per C call.  Every
array is a device tensor but `totals`, which is a host list; nothing is read back, so each call can be captured in a graph
(the tensors given must then stay alive: the caller keeps them).  No CPU path.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib


def _dev(t, who):
    if not torch.is_tensor(t) or t.device.type != "cuda":
        raise RuntimeError(f"diffsinger_amd.words.{who} runs only on an MI355X (HIP) device tensor. There is no CPU path.")
    return t.device


def _as(t, dtype, device):
    return None if t is None else t.detach().to(device=device, dtype=dtype).contiguous()


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def word_dur(dur, n_words, index=None, slur=None, totals=None, want_index=False, out=None):
    """dur [B, N]; index [B, N] (ph2word, 0 = padding) or slur [B, N] bool; totals: B host ints or None
    -> word_dur [B, n_words] int64 (, index [B, N] int64)"""
    d = _dev(dur, "word_dur")
    dur, index, slur = _as(dur, torch.int64, d), _as(index, torch.int64, d), _as(slur, torch.uint8, d)
    bsz, n = dur.shape
    out = torch.empty((bsz, int(n_words)), device=d, dtype=torch.int64) if out is None else out
    idx_out = torch.empty((bsz, n), device=d, dtype=torch.int64) if want_index else None
    tot = None
    if totals is not None:
        vals = [int(v) for v in (totals.tolist() if torch.is_tensor(totals) else totals)]
        if len(vals) != bsz:
            raise ValueError(f"totals holds {len(vals)} values for a batch of {bsz}")
        tot = (C.c_int64 * bsz)(*vals)
    a = _lib.DsdWordDurArgs(C.sizeof(_lib.DsdWordDurArgs), bsz, n, int(n_words), _ptr(dur), _ptr(index), _ptr(slur), tot, _ptr(out),
                            _ptr(idx_out))
    _lib.check(None, _lib.lib().dsd_word_dur(d.index, C.byref(a), _stream(d)), "dsd_word_dur")
    return (out, idx_out) if want_index else out


def group_midi(note_midi, note_dur, group_dur, n_frames, ph2word=None, out=None):
    """note_midi [B, Nn] fp32 (rests filled), note_dur [B, Nn], group_dur [B, G] (ph_dur, or the aligned word_dur)
    -> midi [B, G] int64, or [B, L] gathered through ph2word [B, L]"""
    d = _dev(note_midi, "group_midi")
    note_midi, note_dur = _as(note_midi, torch.float32, d), _as(note_dur, torch.int64, d)
    group_dur, ph2word = _as(group_dur, torch.int64, d), _as(ph2word, torch.int64, d)
    bsz, n_notes = note_midi.shape
    n_groups = group_dur.shape[1]
    n_ph = 0 if ph2word is None else ph2word.shape[1]
    out = torch.empty((bsz, n_ph or n_groups), device=d, dtype=torch.int64) if out is None else out
    a = _lib.DsdGroupMidiArgs(C.sizeof(_lib.DsdGroupMidiArgs), bsz, n_notes, n_groups, n_ph, int(n_frames), _ptr(note_midi),
                              _ptr(note_dur), _ptr(group_dur), _ptr(ph2word), _ptr(out))
    _lib.check(None, _lib.lib().dsd_group_midi(d.index, C.byref(a), _stream(d)), "dsd_group_midi")
    return out


def rhythm_align(ph_dur_pred, ph2word, word_dur_, out=None):
    """RhythmRegulator: ph_dur_pred [B, L] fp32, ph2word [B, L], word_dur [B, W] -> ph_dur [B, L] int64"""
    d = _dev(ph_dur_pred, "rhythm_align")
    pred, ph2word, word_dur_ = _as(ph_dur_pred, torch.float32, d), _as(ph2word, torch.int64, d), _as(word_dur_, torch.int64, d)
    bsz, n_ph = pred.shape
    out = torch.empty((bsz, n_ph), device=d, dtype=torch.int64) if out is None else out
    a = _lib.DsdRhythmAlignArgs(C.sizeof(_lib.DsdRhythmAlignArgs), bsz, n_ph, word_dur_.shape[1], _ptr(pred), _ptr(ph2word),
                                _ptr(word_dur_), _ptr(out))
    _lib.check(None, _lib.lib().dsd_rhythm_align(d.index, C.byref(a), _stream(d)), "dsd_rhythm_align")
    return out
