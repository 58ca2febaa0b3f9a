"""On the MI355X: the score algebra of the variance front end from C - dsd_word_dur, dsd_group_midi, dsd_rhythm_align against
the numpy oracle of tests/words_ref.py (which tests/test_words_host.py holds against the reference's own results, G30 and
G13) with torch.equal: the outputs are integers and the fp32 sequence is fixed, so there is no tolerance.  Item b of a
padded batch against its lone call, each entry captured in a graph and replayed twice, the refusals with nothing launched;
dsd_variance_set_lengths at B = 3 against every item's lone run through the same C calls (ALONE_TOL, as
tests/test_gpu_cvariance.py and tests/test_gpu_cproject.py hold batches against items alone); and
examples/c_abi_variance_project.c compiled with gcc and run once."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cvariance_cases as cc
import deploy_cases as dc
import words_cases as wc
import words_ref as wr
from diffsinger_amd import _lib, modelfile, noise as seeded, words
from diffsinger_amd.hparams import hparams
from gpu_util import dev
from test_gpu_deploy import ALONE_TOL, close, release

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESTATE = -1, _lib.DSD_ESTATE


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    yield
    hparams.clear()
    hparams.update(hidden_size=256)


def t_int(a):
    return dev(np.asarray(a, np.int64))


# ------------------------------------------------------------------------------------------------ the three entries
def run_rhythm(c, sl=slice(None), n_ph=None, n_words=None):
    return words.rhythm_align(dev(c["pred"][sl, :n_ph]), t_int(c["ph2word"][sl, :n_ph]), t_int(c["word_dur"][sl, :n_words]))


def run_word(c, sl=slice(None), n=None, n_words=None, want_index=False):
    kw = dict(index=t_int(c["index"][sl, :n])) if "index" in c else dict(slur=dev(c["slur"][sl, :n]))
    totals = None if c["totals"] is None else c["totals"][sl].tolist()
    return words.word_dur(t_int(c["dur"][sl, :n]), c["W"] if n_words is None else n_words, totals=totals, want_index=want_index, **kw)


def run_midi(c, sl=slice(None), n_notes=None, n_groups=None, n_ph=None, t_len=None):
    p2w = None if c["ph2word"] is None else t_int(c["ph2word"][sl, :n_ph])
    return words.group_midi(dev(c["note_midi"][sl, :n_notes]), t_int(c["note_dur"][sl, :n_notes]), t_int(c["group_dur"][sl, :n_groups]),
                            c["T"] if t_len is None else t_len, ph2word=p2w)


@pytest.mark.parametrize("name", list(wc.rhythm_cases()))
def test_rhythm_align_equals_the_oracle_and_items_alone(name):
    c = wc.rhythm_cases()[name]
    want = torch.from_numpy(wr.rhythm_align(c["pred"], c["ph2word"], c["word_dur"]))
    got = run_rhythm(c).cpu()
    assert got.dtype == torch.int64 and torch.equal(got, want), (name, int((got != want).sum()))
    if len(c["sizes"]) > 1:
        for b, (n_ph, n_words) in enumerate(c["sizes"]):
            alone = run_rhythm(c, slice(b, b + 1), n_ph, n_words).cpu()
            assert torch.equal(alone, got[b:b + 1, :n_ph]), (name, b)
            assert not got[b, n_ph:].any()                              # padding phones: duration 0


@pytest.mark.parametrize("name", list(wc.word_cases()))
def test_word_dur_equals_the_oracle_and_items_alone(name):
    c = wc.word_cases()[name]
    want, want_index = wr.word_dur(c["dur"], c["W"], index=c.get("index"), slur=c.get("slur"), totals=c["totals"])
    got, index = run_word(c, want_index=True)
    got, index = got.cpu(), index.cpu()
    assert torch.equal(got, torch.from_numpy(want)), (name, got.tolist())
    assert torch.equal(index, torch.from_numpy(want_index)), name
    if c["totals"] is not None:
        for b in range(got.shape[0]):
            assert int(got[b].sum()) == int(c["totals"][b])
    if len(c["sizes"]) > 1:
        for b, (n, n_words) in enumerate(c["sizes"]):
            alone = run_word(c, slice(b, b + 1), n, n_words).cpu()
            assert torch.equal(alone, got[b:b + 1, :n_words]), (name, b)
            assert not got[b, n_words:].any()


@pytest.mark.parametrize("name", list(wc.midi_cases()))
def test_group_midi_equals_the_oracle_and_items_alone(name):
    c = wc.midi_cases()[name]
    want = torch.from_numpy(wr.group_midi(c["note_midi"], c["note_dur"], c["group_dur"], c["T"], c["ph2word"]))
    got = run_midi(c).cpu()
    assert got.dtype == torch.int64 and torch.equal(got, want), (name, int((got != want).sum()))
    if len(c["sizes"]) > 1:
        for b, (n_notes, n_groups) in enumerate(c["sizes"]):
            n_ph = None if c["ph2word"] is None else c["n_ph"][b]
            alone = run_midi(c, slice(b, b + 1), n_notes, n_groups, n_ph, c["t_len"][b]).cpu()
            assert torch.equal(alone, got[b:b + 1, :(n_groups if n_ph is None else n_ph)]), (name, b)


def test_word_dur_in_more_items_than_one_launch_carries_totals_for():
    """B = 130 with totals: three launches of 64, 64 and 2 items"""
    rng = np.random.default_rng(3004)
    dur = rng.integers(0, 30, (130, 11))
    slur = rng.random((130, 11)) < 0.4
    totals = rng.integers(0, 400, 130)
    want, _ = wr.word_dur(dur, 7, slur=slur, totals=totals)
    got = words.word_dur(t_int(dur), 7, slur=dev(slur), totals=totals.tolist()).cpu()
    assert torch.equal(got, torch.from_numpy(want))


def test_each_entry_captured_in_a_graph_and_replayed_twice():
    """the entries read nothing back and keep no memory: captured once, replayed over inputs written in place"""
    rc, wcase, mc = wc.rhythm_cases()["batch3"], wc.word_cases()["slur_totals"], wc.midi_cases()["words"]
    pred, p2w, wd = dev(rc["pred"]), t_int(rc["ph2word"]), t_int(rc["word_dur"])
    ndur, slur = t_int(wcase["dur"]), dev(wcase["slur"])
    midi, mnd, mgd, mp2w = dev(mc["note_midi"]), t_int(mc["note_dur"]), t_int(mc["group_dur"]), t_int(mc["ph2word"])
    outs = dict(rhythm=torch.empty(pred.shape, device="cuda", dtype=torch.int64),
                word=torch.empty((3, wcase["W"]), device="cuda", dtype=torch.int64),
                midi=torch.empty(mp2w.shape, device="cuda", dtype=torch.int64))

    def chain():
        words.rhythm_align(pred, p2w, wd, out=outs["rhythm"])
        words.word_dur(ndur, wcase["W"], slur=slur, totals=wcase["totals"].tolist(), out=outs["word"])
        words.group_midi(midi, mnd, mgd, mc["T"], ph2word=mp2w, out=outs["midi"])

    def oracle(scale, shift):
        return dict(rhythm=wr.rhythm_align(rc["pred"] * np.float32(scale), rc["ph2word"], rc["word_dur"]),
                    word=wr.word_dur(wcase["dur"] + shift, wcase["W"], slur=wcase["slur"], totals=wcase["totals"])[0],
                    midi=wr.group_midi(mc["note_midi"] + np.float32(shift), mc["note_dur"], mc["group_dur"], mc["T"], mc["ph2word"]))
    chain()                                         # eager first
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    for scale, shift in ((1.0, 0), (1.75, 3)):
        pred.copy_(dev(rc["pred"] * np.float32(scale)))
        ndur.copy_(t_int(wcase["dur"] + shift))
        midi.copy_(dev(mc["note_midi"] + np.float32(shift)))
        for x in outs.values():
            x.fill_(-77)
        graph.replay()
        torch.cuda.synchronize()
        want = oracle(scale, shift)
        for k in outs:
            assert torch.equal(outs[k].cpu(), torch.from_numpy(want[k])), (k, scale)


def test_refusals_launch_nothing():
    lib = _lib.lib()
    buf = torch.full((4096,), -77, device="cuda", dtype=torch.int64)
    p = C.c_void_p(buf.data_ptr())

    def msg():
        return lib.dsd_last_error(None).decode()

    def make(cls, values, **kw):
        a = cls(C.sizeof(cls), *values)
        for k, x in kw.items():
            setattr(a, k, x)
        return a
    word = (_lib.DsdWordDurArgs, (2, 8, 4, p, p, None, None, p, p))
    midi = (_lib.DsdGroupMidiArgs, (2, 3, 4, 5, 9, p, p, p, p, p))
    rhythm = (_lib.DsdRhythmAlignArgs, (2, 5, 3, p, p, p, p))
    for fn, base, kw, text in ((lib.dsd_word_dur, word, dict(struct_size=8), "struct_size"), (lib.dsd_word_dur, word, dict(slur=p), "exactly one"),
                               (lib.dsd_word_dur, word, dict(index=None), "exactly one"), (lib.dsd_word_dur, word, dict(N=2049), "N = 2049"),
                               (lib.dsd_word_dur, word, dict(W=0), "W = 0"), (lib.dsd_word_dur, word, dict(B=65536), "B = 65536"),
                               (lib.dsd_word_dur, word, dict(totals=(C.c_int64 * 2)(4, -1)), "totals[1] = -1"),
                               (lib.dsd_word_dur, word, dict(word_dur=None), "NULL"),
                               (lib.dsd_group_midi, midi, dict(T=0), "T = 0"), (lib.dsd_group_midi, midi, dict(G=2049), "G = 2049"),
                               (lib.dsd_group_midi, midi, dict(ph2word=None), "without ph2word"), (lib.dsd_group_midi, midi, dict(midi=None), "NULL"),
                               (lib.dsd_group_midi, midi, dict(Nn=0), "Nn = 0"), (lib.dsd_group_midi, midi, dict(B=0), "B = 0"),
                               (lib.dsd_rhythm_align, rhythm, dict(L=2049), "L = 2049"), (lib.dsd_rhythm_align, rhythm, dict(W=-1), "W = -1"),
                               (lib.dsd_rhythm_align, rhythm, dict(ph2word=None), "NULL"), (lib.dsd_rhythm_align, rhythm, dict(struct_size=0), "struct_size")):
        assert fn(0, C.byref(make(*base, **kw)), None) == EINVAL and text in msg(), (text, msg())
    for fn in (lib.dsd_word_dur, lib.dsd_group_midi, lib.dsd_rhythm_align):
        assert fn(0, None, None) == EINVAL and "NULL args" in msg()
    assert lib.dsd_rhythm_align(99, C.byref(make(*rhythm)), None) != 0                 # no such device: refused by select_device
    torch.cuda.synchronize()
    assert bool((buf == -77).all())                                                    # nothing was launched


# ------------------------------------------------------------------------------------------------ lengths through the object
class World:
    """the Python twin of the seeded 'word' case (both predictors, speakers), its model file, and the C object opened from it"""

    def __init__(self, directory):
        from diffsinger_amd.cvariance import Variance
        self.model, self.hp = cc.build_model("word", cuda=True)
        self.path = os.path.join(str(directory), "word.dsdm")
        cc.pack(self.path, self.model)
        with modelfile.open(self.path) as f:
            self.v = Variance(f, cc.PREFIX, "cuda")

    def close(self):
        self.v.close()
        release(self.model)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    w = World(tmp_path_factory.mktemp("words"))
    yield w
    w.close()


LENS, T_LEN, STEPS = [70, 23, 33], 70, 4


def ragged_inputs(hp):
    """B = 3, T = 70, lengths [70, 23, 33]: the token-level inputs of tests/cvariance_cases.py's batch, durations that fill
    each item's own frames, and junk - not zeros - past every end in every frame-level input"""
    rng = np.random.default_rng(3005)
    base = cc.batch_inputs("word")
    n_ph, n_note = base["tokens"].shape[1], base["note_midi"].shape[1]
    ph_dur, note_dur = np.zeros((3, n_ph), np.int64), np.zeros((3, n_note), np.int64)
    note_midi = base["note_midi"].copy()
    for b, (live_ph, live_notes) in enumerate(((6, 4), (1, 1), (5, 3))):
        ph_dur[b, :live_ph] = dc._split(rng, LENS[b], live_ph)
        note_dur[b, :live_notes] = dc._split(rng, LENS[b], live_notes)
    names = dc.variance_names(hp)
    out = dict(tokens=base["tokens"], word_div=base["word_div"], languages=base["languages"], spk=base["spk_one"], ph_dur=ph_dur,
               note_midi=note_midi, note_rest=base["note_rest"], note_dur=note_dur, note_glide=base["note_glide"],
               pitch=rng.uniform(50, 70, (3, T_LEN)).astype(np.float32), expr=rng.random((3, T_LEN)).astype(np.float32),
               retake=rng.random((3, T_LEN)) < 0.5, var_retake=rng.random((3, T_LEN, len(names))) < 0.5)
    word_dur = np.zeros((3, 3), np.int64)
    for b in range(3):
        edges = np.concatenate([[0], np.cumsum(base["word_div"][b])])
        word_dur[b] = [ph_dur[b, edges[i]:edges[i + 1]].sum() for i in range(3)]
    out["word_dur"] = word_dur
    for n in names:
        out["var_" + n] = rng.uniform(-40, -10, (3, T_LEN)).astype(np.float32)
    return out


def render(v, hp, inp, sl, t, seeds):
    """the frame-level half of the chain through the C calls on items `sl`, cut to `t` frames: pitch condition, base pitch,
    pitch, variance condition, curves"""
    names = v.names
    note = dict(note_midi=inp["note_midi"][sl], note_rest=inp["note_rest"][sl], note_dur=inp["note_dur"][sl])
    if hp["use_glide_embed"]:
        note["note_glide"] = inp["note_glide"][sl]
    bsz = inp["tokens"][sl].shape[0]
    out = {}
    enc, _ = v.encode(inp["tokens"][sl], word_div=inp["word_div"][sl], word_dur=inp["word_dur"][sl], languages=inp["languages"][sl])
    out["pitch_cond"], out["base_pitch"] = v.pitch_cond(enc, inp["ph_dur"][sl], pitch=inp["pitch"][sl, :t], expr=inp["expr"][sl, :t],
                                                        retake=inp["retake"][sl, :t], spk_embed=inp["spk"][sl], **note)
    x_t = seeded.fill((1, bsz, v.cfg.pitch_repeat_bins, t), seeds, seeded.PITCH_X_T, device=torch.device("cuda"))
    out["pitch"] = v.pitch_post(v.sample(_lib.DSD_VAR_PITCH, out["pitch_cond"], STEPS, x_t.view(bsz, 1, -1, t)), out["base_pitch"])
    curves = {n: inp["var_" + n][sl, :t] for n in names}
    out["variance_cond"] = v.cond(enc, inp["ph_dur"][sl], out["pitch"], curves, inp["var_retake"][sl, :t], spk_embed=inp["spk"][sl])
    x_t = seeded.fill((1, bsz, len(names) * v.cfg.var_repeat_bins, t), seeds, seeded.VARIANCE_X_T, device=torch.device("cuda"))
    out.update(v.post(v.sample(_lib.DSD_VAR_VARIANCES, out["variance_cond"], STEPS, x_t.view(bsz, len(names), -1, t))))
    torch.cuda.synchronize()
    return out


def test_set_lengths_gives_every_item_as_if_alone(world):
    v, hp = world.v, world.hp
    inp = {k: dev(x) for k, x in ragged_inputs(hp).items()}
    seeds = [41, 42, 43]
    with torch.no_grad():
        dense = render(v, hp, inp, slice(0, 3), T_LEN, seeds)
        v.set_lengths(LENS)
        ragged = render(v, hp, inp, slice(0, 3), T_LEN, seeds)
        v.set_lengths(None)
        again = render(v, hp, inp, slice(0, 3), T_LEN, seeds)
        for k in dense:                                             # set_lengths(NULL): the dense bits are back
            assert torch.equal(dense[k], again[k]), k
        for b, n in enumerate(LENS):
            alone = render(v, hp, inp, slice(b, b + 1), n, seeds[b:b + 1])
            for k in ragged:
                close(ragged[k][b:b + 1, :n], alone[k].cpu().numpy(), ALONE_TOL, True, f"item {b} of the ragged batch vs alone, {k}")
        # without lengths the batch is another computation: item 1's last frames see what lies past its end
        n = LENS[1]
        for k in ("base_pitch", "pitch"):
            tail_dense, tail_ragged = dense[k][1, n - 2:n], ragged[k][1, n - 2:n]
            print(f"{k}: item 1's last frames, dense {tail_dense.tolist()} vs with lengths {tail_ragged.tolist()}")
            assert float((tail_dense - tail_ragged).abs().max()) > 100 * ALONE_TOL * float(tail_ragged.abs().max()), k


def test_set_lengths_rules_from_all_four_stage_calls(world):
    v, hp = world.v, world.hp
    lib = _lib.lib()
    inp = {k: dev(x) for k, x in ragged_inputs(hp).items()}
    buf = torch.zeros(3 * T_LEN * 64, device="cuda")
    p = C.c_void_p(buf.data_ptr())

    def msg():
        return lib.dsd_last_error(None).decode()
    lens3 = (C.c_int32 * 3)(*LENS)
    for bad, text in (((C.c_int32 * 3)(70, -1, 33), "lengths[1] = -1 is negative"),):
        assert lib.dsd_variance_set_lengths(v._v, bad, 3, None) == EINVAL and text in msg()
    assert lib.dsd_variance_set_lengths(v._v, lens3, 0, None) == EINVAL and "B = 0" in msg()
    assert lib.dsd_variance_set_lengths(v._v, lens3, 65536, None) == EINVAL and "B = 65536" in msg()
    v.set_lengths(LENS)
    try:
        def pit(bsz, t, lengths=None):
            return _lib.DsdVariancePitchCondArgs(C.sizeof(_lib.DsdVariancePitchCondArgs), bsz, 6, 4, t, p, p, p, p, p, None, p, None, p, None, 0,
                                                 lengths, p, p)

        def cnd(bsz, t):
            return _lib.DsdVarianceCondArgs(C.sizeof(_lib.DsdVarianceCondArgs), bsz, 6, t, p, p, p, (C.c_void_p * 4)(*[p.value] * 4), p, None, 0, p)
        four = ((lambda b, t: lib.dsd_variance_pitch_cond(v._v, C.byref(pit(b, t)), None), "dsd_variance_pitch_cond"),
                (lambda b, t: lib.dsd_variance_cond(v._v, C.byref(cnd(b, t)), None), "dsd_variance_cond"),
                (lambda b, t: lib.dsd_variance_pitch_post(v._v, p, p, b, t, p, None), "dsd_variance_pitch_post"),
                (lambda b, t: lib.dsd_variance_post(v._v, p, b, t, (C.c_void_p * 4)(*[p.value] * 4), None), "dsd_variance_post"))
        for call, name in four:
            assert call(2, T_LEN) == ESTATE and msg().startswith(name) and "gave 3 lengths but this call runs a batch of 2" in msg(), msg()
            assert call(3, 69) == EINVAL and msg().startswith(name) and "lengths[0] = 70 exceeds T = 69" in msg(), msg()
        other = (C.c_int32 * 3)(70, 23, 32)
        assert lib.dsd_variance_pitch_cond(v._v, C.byref(pit(3, T_LEN, other)), None) == EINVAL
        assert "lengths[2] = 32, but dsd_variance_set_lengths gave 33" in msg()
        torch.cuda.synchronize()
        assert not buf.any()                                        # nothing was launched
        with torch.no_grad():                                       # the same lengths in the args are fine, and change nothing
            enc, _ = v.encode(inp["tokens"], word_div=inp["word_div"], word_dur=inp["word_dur"], languages=inp["languages"])
            kw = dict(note_midi=inp["note_midi"], note_rest=inp["note_rest"], note_dur=inp["note_dur"], note_glide=inp["note_glide"],
                      pitch=inp["pitch"], expr=inp["expr"], retake=inp["retake"], spk_embed=inp["spk"])
            a = v.pitch_cond(enc, inp["ph_dur"], **kw)
            b = v.pitch_cond(enc, inp["ph_dur"], lengths=LENS, **kw)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
            v.set_lengths(None)                                     # ... and are what the args alone gave before this call
            c = v.pitch_cond(enc, inp["ph_dur"], lengths=LENS, **kw)
            assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    finally:
        v.set_lengths(None)


# ------------------------------------------------------------------------------------------------ the C example
def example_inputs(v):
    """examples/c_abi_variance_project.c's project, restated"""
    cfg = v.cfg
    n_ph, n_word, n_note = [6, 3, 5], [3, 1, 2], [5, 2, 4]
    word_div = np.array([[2, 1, 3], [3, 0, 0], [2, 3, 0]], np.int64)
    seconds = [[0.21, 0.17, 0.30, 0.12, 0.26], [0.25, 0.19], [0.15, 0.22, 0.11, 0.33]]
    slur = np.array([[0, 1, 0, 0, 1], [0, 1, 1, 1, 1], [0, 0, 1, 1, 1]], np.uint8)
    note_midi = np.array([[60.0, 62.0, 64.5, 59.0, 57.0], [67.0, 65.5, -1, -1, -1], [55.0, 58.0, 60.0, 62.0, -1]], np.float32)
    note_dur, lens = np.zeros((3, 5), np.int64), []
    for b in range(3):
        sec = (C.c_float * n_note[b])(*seconds[b])
        frames, total = (C.c_int64 * n_note[b])(), C.c_int64()
        _lib.check(None, _lib.lib().dsd_seconds_to_frames(sec, n_note[b], 512.0 / 44100.0, frames, C.byref(total)), "dsd_seconds_to_frames")
        note_dur[b, :n_note[b]] = list(frames)
        lens.append(int(total.value))
    t_len = max(lens)
    tokens, languages = np.zeros((3, 6), np.int64), np.zeros((3, 6), np.int64)
    glide, rest = np.zeros((3, 5), np.int64), np.zeros((3, 5), np.uint8)
    for b in range(3):
        for i in range(n_ph[b]):
            tokens[b, i] = 1 + (3 * i + 5 * b) % (cfg.vocab_size - 1)
            languages[b, i] = 1 + (i + b) % cfg.num_lang if cfg.num_lang > 0 else 0
        for k in range(n_note[b]):
            glide[b, k] = (k + b) % cfg.glide_rows if cfg.glide_rows > 0 else 0
            rest[b, k] = (k + b) % 4 == 3
    t = np.arange(t_len)
    pitch = np.stack([np.float32(60.0) + np.float32(0.03125) * ((t + 7 * b) % 96).astype(np.float32) for b in range(3)])
    spk_w = np.array([[[0.25 * (b + 1), 1.0 - 0.25 * (b + 1)]] for b in range(3)], np.float32)
    ids = [[0, 1 if cfg.num_spk > 1 else 0]] * 3
    return dict(n_ph=n_ph, n_word=n_word, n_note=n_note, lens=lens, t_len=t_len, word_div=word_div, slur=slur, note_midi=note_midi,
                note_dur=note_dur, tokens=tokens, languages=languages, glide=glide, rest=rest, pitch=pitch, spk_w=spk_w, ids=ids)


def project(v, e, sl, seeds):
    """the example's nine steps through the bindings on the segments `sl`: at the project's padded phone, word and note counts
    (padding is tokens == 0, as for the items alone of tests/test_gpu_cvariance.py) and the segments' own frame count"""
    items = list(range(3))[sl]
    lens = [e["lens"][b] for b in items]
    t = max(lens)
    n_ph, n_word, n_note = (max(e[k]) for k in ("n_ph", "n_word", "n_note"))
    d = lambda k, n: dev(e[k][sl, :n])       # noqa: E731
    names = v.names
    out = {}
    note_dur, note_midi = d("note_dur", n_note), d("note_midi", n_note)
    out["word_dur"] = word_dur = words.word_dur(note_dur, n_word, slur=d("slur", n_note), totals=lens)
    tokens, languages = d("tokens", n_ph), d("languages", n_ph)
    out["encoder_out"], masks, ph2word = v.encode(tokens, word_div=d("word_div", n_word), word_dur=word_dur, languages=languages, want_ph2word=True)
    out["ph_midi"] = ph_midi = words.group_midi(note_midi, note_dur, word_dur, t, ph2word=ph2word)
    spk = v.spk_mix([e["ids"][b] for b in items], dev(e["spk_w"][sl])) if v.cfg.use_spk_id else None
    out["ph_dur_pred"] = pred = v.dur(out["encoder_out"], masks, ph_midi, spk_embed=spk)
    out["ph_dur"] = ph_dur = words.rhythm_align(pred, ph2word, word_dur)
    v.set_lengths(lens)
    try:
        all_true = torch.ones((len(items), t), dtype=torch.uint8, device="cuda")
        kw = dict(note_glide=d("glide", n_note)) if v.cfg.use_glide_embed else {}
        out["pitch_cond"], out["base_pitch"] = v.pitch_cond(out["encoder_out"], ph_dur, note_midi, d("rest", n_note), note_dur, pitch=d("pitch", t),
                                                            retake=all_true, spk_embed=spk, **kw)
        x_t = seeded.fill((1, len(items), v.cfg.pitch_repeat_bins, t), seeds, seeded.PITCH_X_T, device=torch.device("cuda"))
        out["pitch_pred"] = v.pitch_post(v.sample(_lib.DSD_VAR_PITCH, out["pitch_cond"], 4, x_t.view(len(items), 1, -1, t)), out["base_pitch"])
        zeros = {n: torch.zeros((len(items), t), device="cuda") for n in names}
        retake = torch.ones((len(items), t, len(names)), dtype=torch.bool, device="cuda")
        out["variance_cond"] = v.cond(out["encoder_out"], ph_dur, out["pitch_pred"], zeros, retake, spk_embed=spk)
        x_t = seeded.fill((1, len(items), len(names) * v.cfg.var_repeat_bins, t), seeds, seeded.VARIANCE_X_T, device=torch.device("cuda"))
        out.update(v.post(v.sample(_lib.DSD_VAR_VARIANCES, out["variance_cond"], 4, x_t.view(len(items), len(names), -1, t))))
        torch.cuda.synchronize()
    finally:
        v.set_lengths(None)
    return out


def test_c_example_renders_the_project_as_the_bindings_do_and_each_segment_as_alone(world, tmp_path):
    """examples/c_abi_variance_project.c compiled with gcc and run once on the packed model: every figure it prints - one per
    stage and segment, over the segment's own phones or frames - equals the same sum over the chain through the bindings, and
    every segment of that chain equals its lone render (B = 1, its own frame count) within ALONE_TOL; the integer stages exactly."""
    v = world.v
    exe = tmp_path / "c_abi_variance_project"
    libdir = os.path.join(ROOT, "diffsinger_amd")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "c_abi_variance_project.c"), "-L" + libdir, "-ldsdenoise", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True, timeout=300)
    r = subprocess.run([str(exe), world.path, cc.PREFIX], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    got = {}
    for line in r.stdout.splitlines():
        if line.startswith("sum "):
            _, name, b, value = line.split()
            got[name, int(b)] = float(value)
    e = example_inputs(v)
    seeds = [2025, 2026, 2027]
    rows = dict(word_dur="n_word", encoder_out="n_ph", ph_midi="n_ph", ph_dur_pred="n_ph", ph_dur="n_ph")
    with torch.no_grad():
        batch = project(v, e, slice(0, 3), seeds)
        assert {k for k, _ in got} == set(batch), (sorted({k for k, _ in got}), sorted(batch))
        for b in range(3):
            for k, x in batch.items():
                n = e[rows[k]][b] if k in rows else e["lens"][b]
                s = float(x[b, :n].double().sum())
                print(f"{k} of segment {b}: C example {got[k, b]!r}, bindings {s!r}")
                assert got[k, b] == pytest.approx(s, rel=0, abs=1e-9 * max(1.0, abs(s))), (k, b)      # %.17g of the same double sum
            alone = project(v, e, slice(b, b + 1), seeds[b:b + 1])
            for k, x in batch.items():
                n = e[rows[k]][b] if k in rows else e["lens"][b]
                if x.dtype == torch.int64:
                    assert torch.equal(x[b:b + 1, :n], alone[k][:, :n]), (k, b)
                else:
                    close(x[b:b + 1, :n], alone[k][:, :n].cpu().numpy(), ALONE_TOL, True, f"segment {b} of the batch vs alone, {k}")
        assert int(batch["word_dur"].sum()) == sum(e["lens"])
