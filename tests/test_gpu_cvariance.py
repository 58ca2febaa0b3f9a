"""-m gpu: the variance model's staged twin driven through the C calls (dsd_variance_open .. dsd_variance_post, by way
of diffsinger_amd/cvariance.py) on a model file, against

  * G22 (tests/golden/g22_deploy.npz, the reference's own deployment twins) on the cases of tests/deploy_cases.py, with the
    tolerances tests/test_gpu_deploy.py applies to the same quantities;
  * `deploy.DiffSingerVarianceDeploy`, the Python twin, with the same weights: the four front stages run the same kernels
    on the same operands in the same order and must be bit-identical; the two post stages sum the bins in another order
    than torch's mean and are held to ALONE_TOL.

Every figure is printed before it is asserted."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import cvariance_cases as cc
import deploy_cases as dc
from diffsinger_amd import _lib, modelfile, synth
from diffsinger_amd.hparams import hparams
from gpu_util import dev
from test_gpu_deploy import ALONE_TOL, DUR_TOL, ENC_TOL, GOLDEN, SAMPLE_TOL, SMOOTH_BAR, close, release

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    yield
    hparams.clear()
    hparams.update(hidden_size=256)


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


class World:
    """the Python twin of a case, its model file, and the C object opened from it"""

    def __init__(self, tag, directory, edit=None):
        from diffsinger_amd.cvariance import Variance
        self.model, self.hp = cc.build_model(tag, cuda=True)
        self.path = os.path.join(str(directory), tag + ".dsdm")
        cc.pack(self.path, self.model, edit=edit)
        with modelfile.open(self.path) as f:
            self.v = Variance(f, cc.PREFIX, "cuda")         # the object keeps nothing of the file

    def close(self):
        self.v.close()
        release(self.model)


@pytest.fixture
def world(tmp_path):
    made = []

    def make(tag, edit=None):
        made.append(World(tag, tmp_path, edit))
        return made[-1]
    yield make
    for w in made:
        w.close()


def same(got, want, what):
    """bit-identical, a NaN equal to a NaN (the K = 1 case)"""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    a, b = got.contiguous().view(-1), want.contiguous().view(-1)
    differ = int((a.view(torch.int32) != b.view(torch.int32)).sum()) if a.dtype == torch.float32 else int((a != b).sum())
    worst = float((a.float() - b.float()).abs().nan_to_num(0).max()) if a.numel() else 0.0
    print(f"{what}: {differ} of {a.numel()} elements differ from the Python twin's (max |diff| {worst:.3e})")
    assert differ == 0, (what, differ, worst)


def raw_sample(predictor, cond, steps, noise):
    """the twin's sampler stage before the mean over the bins: [B, T, M] / [B, F, T, M], denormalised"""
    from diffsinger_amd.deploy import _sample
    predictor._reduce_bins = lambda x: x
    try:
        return _sample(predictor, cond, steps, noise, None)
    finally:
        del predictor._reduce_bins


# ------------------------------------------------------------------------------------------------ G22 and the twin
@pytest.mark.parametrize("tag", list(dc.VAR_CASES))
def test_stages_vs_golden_and_python_twin(g, world, tag):
    w = world(tag)
    model, hp, v, c = w.model, w.hp, w.v, dc.VAR_CASES[tag]
    inp = {k: dev(x) for k, x in dc.variance_inputs(tag).items()}
    noise = {k: dev(synth.synth_normal(s, c["seed"] + 2 + i)) for i, (k, s) in enumerate(dc.variance_noise_shapes(tag).items())}
    spk = inp.get("spk_embed")
    with torch.no_grad():
        if hp["predict_dur"]:
            enc, x_masks, ph2word = v.encode(inp["tokens"], word_div=inp["word_div"], word_dur=inp["word_dur"],
                                             languages=inp.get("languages"), want_ph2word=True)
            assert np.array_equal(ph2word.cpu().numpy(), g[f"{tag}_ph2word"])
            want_enc, want_masks = model.forward_linguistic_encoder_word(inp["tokens"], inp["word_div"], inp["word_dur"],
                                                                         languages=inp.get("languages"))
            dur = v.dur(enc, x_masks, inp["ph_midi"], spk_embed=spk)
            close(dur, g[f"{tag}_dur_pred"], DUR_TOL, True, "dur_pred")
            same(dur, model.forward_dur_predictor(want_enc, want_masks, inp["ph_midi"], spk_embed=spk), "ph_dur_pred")
        else:
            enc, x_masks = v.encode(inp["tokens"], ph_dur=inp["ph_dur"], languages=inp.get("languages"))
            want_enc, want_masks = model.forward_linguistic_encoder_phoneme(inp["tokens"], inp["ph_dur"], languages=inp.get("languages"))
        assert np.array_equal(x_masks.cpu().numpy(), g[f"{tag}_x_masks"])
        close(enc, g[f"{tag}_enc"], ENC_TOL, False, "encoder_out")
        same(enc, want_enc, "encoder_out")
        same(x_masks, want_masks, "x_masks")
        if hp["predict_pitch"]:
            args = dict(note_midi=inp["note_midi"], note_rest=inp["note_rest"], note_dur=inp["note_dur"], note_glide=inp.get("note_glide"),
                        pitch=inp["pitch"], expr=inp.get("expr"), retake=inp["retake"], spk_embed=spk)
            cond, base = v.pitch_cond(enc, inp["ph_dur"], **args)          # against the twin: the two tests below
            gold = g[f"{tag}_base_pitch"]
            if dc.smooth_width(hp) == 1:        # the reference's operator is 0 / 0: NaN everywhere, and so is this one
                assert np.isnan(gold).all() and torch.isnan(base).all() and tuple(base.shape) == gold.shape
            else:
                err = float(np.abs(base.cpu().numpy() - gold).max())
                print(f"base_pitch (K = {dc.smooth_width(hp)}): max |err| {err:.3e}, bar {SMOOTH_BAR:.3e}")
                assert err <= SMOOTH_BAR
                close(cond, g[f"{tag}_pitch_cond"], ENC_TOL, False, "pitch_cond")
            if c["steps"]:
                # the post stage on the twin's own sample of the reference's condition: the stage under test alone
                raw = raw_sample(model.pitch_predictor, dev(g[f"{tag}_pitch_cond"]), c["steps"], noise["pitch"])
                close(raw.mean(-1), g[f"{tag}_x_pred"], SAMPLE_TOL, True, "x_pred")
                pred = v.pitch_post(raw, dev(gold))
                close(pred, g[f"{tag}_pitch_pred"], SAMPLE_TOL, True, "pitch_pred")
                close(pred, model.forward_pitch_postprocess(raw.mean(-1), dev(gold)).cpu().numpy(), ALONE_TOL, True, "pitch_pred vs the twin")
                if hp["diffusion_type"] == "reflow":        # and the sampler stage as a C caller runs it, on the borrowed handle
                    mine = v.sample(_lib.DSD_VAR_PITCH, dev(g[f"{tag}_pitch_cond"]), c["steps"], noise["pitch"])
                    same(mine, raw, "the pitch sample on the borrowed handle")
        names = dc.variance_names(hp)
        assert v.names == names
        if names:
            curves = {n: inp["var_" + n] for n in names}
            cond = v.cond(enc, inp["ph_dur"], inp["pitch"], curves, inp["var_retake"], spk_embed=spk)
            close(cond, g[f"{tag}_var_cond"], ENC_TOL, False, "variance_cond")
            same(cond, model.forward_variance_preprocess(enc, inp["ph_dur"], inp["pitch"], variances=curves, retake=inp["var_retake"],
                                                         spk_embed=spk), "variance_cond")
            raw = raw_sample(model.variance_predictor, cond, c["steps"], noise["variance"])
            close(raw.mean(-1), g[f"{tag}_xs_pred"], SAMPLE_TOL, True, "xs_pred")
            outs = v.post(raw)
            twin = model.forward_variance_postprocess(raw.mean(-1))
            assert list(outs) == names and len(twin) == len(names)
            for n, t in zip(names, twin):
                close(outs[n], g[f"{tag}_out_{n}"], SAMPLE_TOL, True, n)
                close(outs[n], t.cpu().numpy(), ALONE_TOL, True, n + " vs the twin")
            if hp["diffusion_type"] == "reflow":
                same(v.sample(_lib.DSD_VAR_VARIANCES, cond, c["steps"], noise["variance"]), raw, "the variance sample on the borrowed handle")


PITCH_TAGS = [t for t in dc.VAR_CASES if dc.variance_hparams(t)["predict_pitch"]]


def _pitch_cond_pair(w, tag, taps=None):
    """(pitch_cond, base_pitch) of the C stage and of the Python twin on the case's inputs and the C stage's encoder output;
    `taps`: installed in the twin in place of its own"""
    model, v = w.model, w.v
    inp = {k: dev(x) for k, x in dc.variance_inputs(tag).items()}
    with torch.no_grad():
        if w.hp["predict_dur"]:
            enc, _ = v.encode(inp["tokens"], word_div=inp["word_div"], word_dur=inp["word_dur"], languages=inp.get("languages"))
        else:
            enc, _ = v.encode(inp["tokens"], ph_dur=inp["ph_dur"], languages=inp.get("languages"))
        args = dict(note_midi=inp["note_midi"], note_rest=inp["note_rest"], note_dur=inp["note_dur"], note_glide=inp.get("note_glide"),
                    pitch=inp["pitch"], expr=inp.get("expr"), retake=inp["retake"], spk_embed=inp.get("spk_embed"))
        if taps is not None:
            model.smooth = (len(taps), taps)
        return v.pitch_cond(enc, inp["ph_dur"], **args), model.forward_pitch_preprocess(enc, inp["ph_dur"], **args)


@pytest.mark.parametrize("tag", PITCH_TAGS)
def test_pitch_cond_is_bit_identical_to_the_python_twins(world, tag):
    """pitch_cond and base_pitch against the unmodified Python twin, bit for bit, K = 4 and the NaN tap of K = 1 included.
    The kernels, operands and their order are the twin's; the K taps are the twin's too, because the tables section carries
    them (`smooth_taps`, what `deploy.smooth_kernel` gives on the packing host - the reference bakes its own into the
    exported graph in the same way)."""
    (cond, base), (want_cond, want_base) = _pitch_cond_pair(world(tag), tag)
    same(base, want_base, "base_pitch")
    same(cond, want_cond, "pitch_cond")


@pytest.mark.parametrize("tag", PITCH_TAGS)
def test_pitch_cond_without_stored_taps_takes_the_librarys_own(world, tag):
    """A tables section without `smooth_taps`: dsd_variance_open computes the taps itself (include/dsdenoise.h; restated in
    tests/cvariance_cases.py).  Those are not torch's bits for every K - torch's CPU sine is accurate to one ulp, not correctly
    rounded, and its sum order follows the host's vector width; with its own taps the library's `melody_even` (K = 4) base
    pitch sits one fp32 ulp, 7.63e-6 semitones, from the twin's in 23 of 23 frames - so the twin is given the restated taps,
    and then every case is bit-identical: the fallback computes exactly what the header says."""
    w = world(tag, lambda sections: sections[0].tensors.pop("smooth_taps"))
    (cond, base), (want_cond, want_base) = _pitch_cond_pair(w, tag, cc.library_taps(dc.smooth_width(w.hp)))
    same(base, want_base, "base_pitch")
    same(cond, want_cond, "pitch_cond")


def test_post_stage_row_counts_clamps_and_nan(world):
    """The post kernel on rows that are no multiple of the four a workgroup takes (3 x 3 x 7), with the clamp binding on
    either side and a NaN in one bin (torch.clamp keeps it, and so does the kernel)."""
    w = world("var_three")
    v = w.v
    rng = np.random.Generator(np.random.PCG64(2430))
    raw = torch.from_numpy(rng.uniform(-120, 30, (3, 3, 7, 4)).astype(np.float32)).cuda()
    raw[0, :, 0, :], raw[0, :, 1, :] = -150.0, 50.0                       # a row below every clamp, one above
    raw[1, 2, 3, 1] = float("nan")
    outs = v.post(raw)
    twin = w.model.forward_variance_postprocess(raw.mean(-1))
    for n, t in zip(v.names, twin):
        got, want = outs[n].cpu().numpy(), t.cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got).sum() == (1 if n == v.names[2] else 0)
        err = float(np.nanmax(np.abs(got - want)))
        print(f"{n}: max |err| {err:.3e}, bound {ALONE_TOL * max(1.0, float(np.nanmax(np.abs(want)))):.3e}")
        assert err <= ALONE_TOL * max(1.0, float(np.nanmax(np.abs(want))))
        lo = -96.0 if n != "tension" else -10.0
        hi = 0.0 if n != "tension" else 10.0
        assert np.nanmin(got) >= lo and np.nanmax(got) <= hi and (got == lo).any() and (got == hi).any()


# ------------------------------------------------------------------------------------------------ a seeded, padded batch
@pytest.mark.parametrize("tag,spk", [("word", "one"), ("word", "per_row"), ("phoneme", "one"), ("phoneme", "per_row")])
def test_padded_batch_vs_python_twin_and_items_alone(world, tag, spk):
    """B = 3 (tests/cvariance_cases.py): an item with one real phoneme, a zero in word_div, a phoneme without frames,
    padding tokens at the end of two items, durations that total less than T with `lengths` given, spk_embed as
    [B, 1, H] and per row, a cross-lingual list that masks some tokens ('word') and an empty one ('phoneme').  Every stage
    against the Python twin, bit for bit, and every item against the same item run alone (B = 1, its own frame count)."""
    w = world(tag)
    model, hp, v = w.model, w.hp, w.v
    inp = {k: dev(x) for k, x in cc.batch_inputs(tag).items()}
    lens = [int(x) for x in inp["lengths"].tolist()]
    t_len = inp["retake"].shape[1]
    spk_ph = inp["spk_one"] if spk == "one" else inp["spk_ph"]
    spk_fr = inp["spk_one"] if spk == "one" else inp["spk_frames"]
    names = v.names
    curves = {n: inp["var_" + n] for n in names}
    note = dict(note_midi=inp["note_midi"], note_rest=inp["note_rest"], note_dur=inp["note_dur"])
    if hp["use_glide_embed"]:
        note["note_glide"] = inp["note_glide"]

    def stages(obj, sl, t, spk_p, spk_f, lengths):
        """every front stage on the items `sl`, cut to `t` frames; obj: the C object or the Python twin"""
        c_side = obj is v
        out = {}
        if hp["predict_dur"]:
            enc_args = (inp["tokens"][sl],), dict(word_div=inp["word_div"][sl], word_dur=inp["word_dur"][sl], languages=inp["languages"][sl])
            fn = v.encode if c_side else lambda tok, **kw: model.forward_linguistic_encoder_word(tok, kw["word_div"], kw["word_dur"],
                                                                                                 languages=kw["languages"])
        else:
            enc_args = (inp["tokens"][sl],), dict(ph_dur=inp["ph_dur"][sl], languages=inp["languages"][sl])
            fn = v.encode if c_side else lambda tok, **kw: model.forward_linguistic_encoder_phoneme(tok, kw["ph_dur"], languages=kw["languages"])
        out["encoder_out"], out["x_masks"] = fn(*enc_args[0], **enc_args[1])
        enc = batch["encoder_out"][sl] if batch else out["encoder_out"]      # later stages: on the batch's own encoder output
        if hp["predict_dur"]:
            out["ph_dur_pred"] = (v.dur if c_side else model.forward_dur_predictor)(enc, out["x_masks"], inp["ph_midi"][sl], spk_embed=spk_p)
        kw = dict({k: x[sl] for k, x in note.items()}, pitch=inp["pitch"][sl, :t], expr=inp["expr"][sl, :t], retake=inp["retake"][sl, :t],
                  spk_embed=spk_f, lengths=lengths)
        out["pitch_cond"], out["base_pitch"] = (v.pitch_cond if c_side else model.forward_pitch_preprocess)(enc, inp["ph_dur"][sl], **kw)
        cv, rt = {n: x[sl, :t] for n, x in curves.items()}, inp["var_retake"][sl, :t]
        if c_side:
            out["variance_cond"] = v.cond(enc, inp["ph_dur"][sl], inp["pitch"][sl, :t], cv, rt, spk_embed=spk_f)
        else:
            out["variance_cond"] = model.forward_variance_preprocess(enc, inp["ph_dur"][sl], inp["pitch"][sl, :t], variances=cv, retake=rt,
                                                                     spk_embed=spk_f)
        return out

    with torch.no_grad():
        batch = None
        batch = stages(v, slice(0, 3), t_len, spk_ph, spk_fr, lens)
        twin = stages(model, slice(0, 3), t_len, spk_ph, spk_fr, lens)
        for k in batch:
            same(batch[k], twin[k], k)
        assert batch["x_masks"].cpu().numpy().tolist() == (cc.batch_inputs(tag)["tokens"] == 0).tolist()
        for b in range(3):
            sl, n = slice(b, b + 1), lens[b]
            alone = stages(v, sl, n, spk_ph[sl], spk_fr[sl] if spk == "one" else spk_fr[sl, :n], None)
            for k in batch:
                frames = k in ("pitch_cond", "base_pitch", "variance_cond")
                same(alone[k], batch[k][sl, :n] if frames else batch[k][sl], f"item {b} alone, {k}")
            assert not batch["base_pitch"][b, n:].any()                  # frames past the item's length


def test_encode_at_the_token_limit(world):
    """L = 2048, the encoders' limit (eight tokens per lane in the regulator, eight workgroups of the index kernel): the
    padding mask and ph2word only."""
    w = world("word_base")
    rng = np.random.Generator(np.random.PCG64(2440))
    n_ph, n_word = 2048, 700
    tokens = rng.integers(0, dc.VOCAB, (1, n_ph)).astype(np.int64)
    word_div = rng.integers(0, 5, (1, n_word)).astype(np.int64)
    word_div[0, -1] += max(0, n_ph - 100 - int(word_div.sum()))          # the words cover all but about a hundred phonemes
    word_dur = rng.integers(1, 40, (1, n_word)).astype(np.int64)
    with torch.no_grad():
        _, x_masks, ph2word = w.v.encode(dev(tokens), word_div=dev(word_div), word_dur=dev(word_dur), want_ph2word=True)
    assert np.array_equal(x_masks.cpu().numpy(), tokens == 0) and (tokens == 0).any()
    want = dc.length_regulate_numpy(word_div, n_ph)
    assert np.array_equal(ph2word.cpu().numpy(), want) and (want == 0).any() and want.max() == n_word


# ------------------------------------------------------------------------------------------------ refusals with an object
def test_stage_calls_refuse_before_any_launch(world):
    lib = _lib.lib()
    word, plain = world("word_melody"), world("var_one")         # word form, speaker, pitch  /  phoneme form, one variance, no speaker
    buf = torch.zeros(4096, device="cuda")
    p = C.c_void_p(buf.data_ptr())

    def msg():
        return lib.dsd_last_error(None).decode()

    def enc(**kw):
        a = _lib.DsdVarianceEncodeArgs(C.sizeof(_lib.DsdVarianceEncodeArgs), 1, 4, 2, p, p, p, None, p, p, p, None)
        for k, x in kw.items():
            setattr(a, k, x)
        return a
    for v, a, words in ((word.v, enc(B=0), "B = 0"), (word.v, enc(L=0), "L = 0"), (word.v, enc(L=2049), "L = 2049"), (word.v, enc(W=2049), "W = 2049"),
                        (word.v, enc(W=0), "W = 0"), (word.v, enc(tokens=None), "NULL tokens"), (word.v, enc(word_dur=None), "NULL word_div or word_dur"),
                        (word.v, enc(ph_dur=p), "ph_dur is the phoneme form's input"), (word.v, enc(languages=None), "languages is required"),
                        (word.v, enc(struct_size=8), "struct_size"), (plain.v, enc(), "the word form's inputs"),
                        (plain.v, enc(W=0, word_div=None, word_dur=None), "NULL ph_dur"),
                        (plain.v, enc(W=0, word_div=None, word_dur=None, ph_dur=p, ph2word=p), "no ph2word to write")):
        assert lib.dsd_variance_encode(v._v, C.byref(a), None) == -1 and words in msg(), (words, msg())
    assert lib.dsd_variance_encode(word.v._v, None, None) == -1 and "NULL args" in msg()

    def dur(**kw):
        a = _lib.DsdVarianceDurArgs(C.sizeof(_lib.DsdVarianceDurArgs), 1, 4, p, p, p, None, 0, p)
        for k, x in kw.items():
            setattr(a, k, x)
        return a
    for v, a, words in ((plain.v, dur(), "no duration predictor"), (word.v, dur(L=0), "L = 0"), (word.v, dur(ph_midi=None), "NULL"),
                        (word.v, dur(spk_embed=p, spk_rows=3), "spk_rows = 3 is neither 1 nor L = 4")):
        assert lib.dsd_variance_dur(v._v, C.byref(a), None) == -1 and words in msg(), (words, msg())

    def pit(**kw):
        a = _lib.DsdVariancePitchCondArgs(C.sizeof(_lib.DsdVariancePitchCondArgs), 1, 4, 3, 9, p, p, p, p, p, None, p, None, p, None, 0, None, p, p)
        for k, x in kw.items():
            setattr(a, k, x)
        return a
    for v, a, words in ((plain.v, pit(), "no pitch predictor"), (word.v, pit(T=0), "T = 0"), (word.v, pit(N=0), "N = 0"), (word.v, pit(N=2049), "N = 2049"),
                        (word.v, pit(note_rest=None), "NULL note_rest"), (word.v, pit(retake=None), "NULL"),
                        (word.v, pit(spk_embed=p, spk_rows=2), "spk_rows = 2 is neither 1 nor T = 9"),
                        (word.v, pit(lengths=(C.c_int32 * 1)(10)), "lengths[0] = 10 outside [0, T = 9]"),
                        (word.v, pit(lengths=(C.c_int32 * 1)(-1)), "lengths[0] = -1")):
        assert lib.dsd_variance_pitch_cond(v._v, C.byref(a), None) == -1 and words in msg(), (words, msg())

    def cond(**kw):
        a = _lib.DsdVarianceCondArgs(C.sizeof(_lib.DsdVarianceCondArgs), 1, 4, 9, p, p, p, (C.c_void_p * 4)(p.value), p, None, 0, p)
        for k, x in kw.items():
            setattr(a, k, x)
        return a
    for v, a, words in ((word.v, cond(), "predicts no variance"), (plain.v, cond(T=0), "T = 0"), (plain.v, cond(curves=(C.c_void_p * 4)()), "NULL curves[0] (energy)"),
                        (plain.v, cond(spk_embed=p, spk_rows=1), "no speaker embedding")):
        assert lib.dsd_variance_cond(v._v, C.byref(a), None) == -1 and words in msg(), (words, msg())
    assert lib.dsd_variance_pitch_post(plain.v._v, p, p, 1, 4, p, None) == -1 and "no pitch predictor" in msg()
    assert lib.dsd_variance_pitch_post(word.v._v, p, None, 1, 4, p, None) == -1 and "NULL" in msg()
    assert lib.dsd_variance_pitch_post(word.v._v, p, p, 1, 0, p, None) == -1 and "T = 0" in msg()
    assert lib.dsd_variance_post(word.v._v, p, 1, 4, (C.c_void_p * 4)(p.value), None) == -1 and "predicts no variance" in msg()
    assert lib.dsd_variance_post(plain.v._v, p, 1, 4, (C.c_void_p * 4)(), None) == -1 and "NULL curves_out[0] (energy)" in msg()
    h = C.c_void_p(1)
    assert lib.dsd_variance_backbone(plain.v._v, _lib.DSD_VAR_PITCH, C.byref(h)) == -1 and h.value is None and "no pitch predictor" in msg()
    assert lib.dsd_variance_backbone(plain.v._v, 2, C.byref(h)) == -1 and "which = 2" in msg()
    assert lib.dsd_variance_backbone(plain.v._v, _lib.DSD_VAR_VARIANCES, C.byref(h)) == 0 and h.value
    cfg = _lib.DsdVarianceConfig()
    assert lib.dsd_variance_info(word.v._v, C.byref(cfg)) == 0 and bytes(cfg) == bytes(modelfile.variance_config(word.model))
    torch.cuda.synchronize()
    assert not buf.any()                                                    # nothing was launched


# ------------------------------------------------------------------------------------------------ capture
def test_captured_pitch_chain_replays_what_the_eager_run_gives(world):
    """pitch-cond -> dsd_prepare_cond + dsd_sample on the borrowed handle -> pitch-post, captured in one HIP graph after
    an eager run at the same sizes (which sized every workspace), replayed twice over inputs written in place."""
    w = world("word_melody")
    v, c = w.v, dc.VAR_CASES["word_melody"]
    inp = {k: dev(x) for k, x in dc.variance_inputs("word_melody").items()}
    noise = dev(synth.synth_normal(dc.variance_noise_shapes("word_melody")["pitch"], c["seed"] + 2))
    with torch.no_grad():
        enc, _ = v.encode(inp["tokens"], word_div=inp["word_div"], word_dur=inp["word_dur"], languages=inp["languages"])
        args = dict(note_midi=inp["note_midi"], note_rest=inp["note_rest"].to(torch.uint8), note_dur=inp["note_dur"],
                    note_glide=inp["note_glide"], pitch=inp["pitch"].clone(), expr=inp["expr"], retake=inp["retake"].to(torch.uint8),
                    spk_embed=inp["spk_embed"])
        t_len, m = c["t_len"], w.hp["pitch_prediction_args"]["repeat_bins"]
        bufs = dict(cond=torch.empty((1, t_len, dc.HIDDEN), device="cuda"), base=torch.empty((1, t_len), device="cuda"),
                    raw=torch.empty((1, t_len, m), device="cuda"), pred=torch.empty((1, t_len), device="cuda"))

        def chain():
            v.pitch_cond(enc, inp["ph_dur"], out=(bufs["cond"], bufs["base"]), **args)
            v.sample(_lib.DSD_VAR_PITCH, bufs["cond"], c["steps"], noise, out=bufs["raw"])
            v.pitch_post(bufs["raw"], bufs["base"], out=bufs["pred"])

        def eager(pitch):
            args["pitch"].copy_(pitch)
            chain()
            torch.cuda.synchronize()
            return {k: x.clone() for k, x in bufs.items()}
        first = eager(inp["pitch"])
        other = eager(inp["pitch"] + 1.5)
        assert not torch.equal(first["pred"], other["pred"])
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            chain()
        for pitch, want in ((inp["pitch"], first), (inp["pitch"] + 1.5, other)):
            args["pitch"].copy_(pitch)
            for x in bufs.values():
                x.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            for k in bufs:
                assert torch.equal(bufs[k], want[k]), k


# ------------------------------------------------------------------------------------------------ the C example
def test_c_example_prints_the_python_twins_checksums(world, tmp_path):
    """examples/c_abi_variance.c compiled and run on a packed model: one file -> word-form encode -> durations -> pitch
    cond -> reflow program -> sample -> pitch post -> variance cond -> sample -> post, x_T from dsd_noise_fill.  The sums it
    prints are held against two references on the same file, inputs and seed: the Python twin (`DiffSingerVarianceDeploy`) for
    the four front stages, the variance condition on the example's own pitch (equal sums: the outputs are bit-identical)
    and the pitch (ALONE_TOL: torch's mean); and the same chain through cvariance for every printed sum, the variance curves
    included - that half shows the example's plumbing, not the stages."""
    from diffsinger_amd import noise as seeded
    w = world("word")
    exe = tmp_path / "c_abi_variance"
    libdir = os.path.join(ROOT, "diffsinger_amd")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "c_abi_variance.c"), "-L" + libdir, "-ldsdenoise", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True, timeout=300)
    r = subprocess.run([str(exe), w.path, cc.PREFIX], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    got = {}
    for line in r.stdout.splitlines():
        if line.startswith("sum "):
            _, name, value = line.split()
            got[name] = float(value)
    # the example's own inputs, restated (examples/c_abi_variance.c: fill_inputs)
    v = w.v
    n_ph, n_word, n_note, t_len, steps, seed = 6, 3, 4, 120, 4, 2025
    tokens = torch.tensor([[1 + (3 * i) % 11 for i in range(n_ph)]], device="cuda")
    word_div = torch.tensor([[2, 1, 3]], device="cuda")
    word_dur = torch.tensor([[50, 30, 40]], device="cuda")
    languages = torch.tensor([[1 + i % 2 for i in range(n_ph)]], device="cuda")
    ph_midi = torch.tensor([[60 + i for i in range(n_ph)]], device="cuda")
    ph_dur = torch.tensor([[25, 25, 30, 10, 0, 30]], device="cuda")
    note_midi = torch.tensor([[60.0, 62.5, 64.0, 59.0]], device="cuda")
    note_rest = torch.tensor([[0, 0, 1, 0]], dtype=torch.uint8, device="cuda")
    note_dur = torch.tensor([[30, 30, 20, 40]], device="cuda")
    note_glide = torch.tensor([[0, 1, 2, 0]], device="cuda")
    frames = torch.arange(t_len, device="cuda", dtype=torch.float32)
    pitch = (60.0 + 0.03125 * frames)[None]
    retake = ((torch.arange(t_len, device="cuda") // 16) % 2 == 0)[None]
    spk = (0.015625 * (torch.arange(dc.HIDDEN, device="cuda", dtype=torch.float32) % 7.0 - 3.0))[None, None]
    with torch.no_grad():
        enc, masks = v.encode(tokens, word_div=word_div, word_dur=word_dur, languages=languages)
        dur = v.dur(enc, masks, ph_midi, spk_embed=spk)
        cond, base = v.pitch_cond(enc, ph_dur, note_midi, note_rest, note_dur, note_glide=note_glide, pitch=pitch, retake=retake, spk_embed=spk)
        x_t_pitch = x_t = seeded.fill((1, 1, v.cfg.pitch_repeat_bins, t_len), [seed], seeded.PITCH_X_T, device=torch.device("cuda"))
        pred = v.pitch_post(v.sample(_lib.DSD_VAR_PITCH, cond, steps, x_t.view(1, 1, -1, t_len)), base)
        zeros = {n: torch.zeros((1, t_len), device="cuda") for n in v.names}
        all_true = torch.ones((1, t_len, len(v.names)), dtype=torch.bool, device="cuda")
        var_cond = v.cond(enc, ph_dur, pred, zeros, all_true, spk_embed=spk)
        n_var = len(v.names)
        x_t = seeded.fill((1, 1, n_var * v.cfg.var_repeat_bins, t_len), [seed], seeded.VARIANCE_X_T, device=torch.device("cuda"))
        outs = v.post(v.sample(_lib.DSD_VAR_VARIANCES, var_cond, steps, x_t.view(1, n_var, -1, t_len)))
        # the Python twin on the same inputs: its front stages are bit-identical, so their sums are the example's too
        model = w.model
        t_enc, t_masks = model.forward_linguistic_encoder_word(tokens, word_div, word_dur, languages=languages)
        t_dur = model.forward_dur_predictor(t_enc, t_masks, ph_midi, spk_embed=spk)
        t_cond, t_base = model.forward_pitch_preprocess(t_enc, ph_dur, note_midi=note_midi, note_rest=note_rest.bool(), note_dur=note_dur,
                                                        note_glide=note_glide, pitch=pitch, retake=retake, spk_embed=spk)
        t_pred = model.forward_pitch_postprocess(model.forward_pitch_reflow(t_cond, steps=steps, noise=x_t_pitch.view(1, 1, -1, t_len)), t_base)
        t_var_cond = model.forward_variance_preprocess(t_enc, ph_dur, pred, variances=zeros, retake=all_true, spk_embed=spk)
    twin = dict(encoder_out=t_enc, ph_dur_pred=t_dur, pitch_cond=t_cond, base_pitch=t_base, variance_cond=t_var_cond)
    for k, t in twin.items():
        s = float(t.double().sum())
        print(f"{k}: C example {got[k]!r}, Python twin {s!r}")
        assert got[k] == pytest.approx(s, rel=0, abs=1e-9 * max(1.0, abs(s))), k
    # the twin's pitch: torch's mean adds the bins in another order (ALONE_TOL per frame, summed over the frames)
    s = float(t_pred.double().sum())
    print(f"pitch_pred: C example {got['pitch_pred']!r}, Python twin {s!r}")
    assert abs(got["pitch_pred"] - s) <= ALONE_TOL * float(t_pred.abs().max()) * t_len
    want = dict(encoder_out=enc, ph_dur_pred=dur, pitch_cond=cond, base_pitch=base, pitch_pred=pred, variance_cond=var_cond, **outs)
    assert set(got) == set(want), (sorted(got), sorted(want))
    for k, t in want.items():
        s = float(t.double().sum())
        print(f"{k}: C example {got[k]!r}, Python {s!r}")
        assert got[k] == pytest.approx(s, rel=0, abs=1e-9 * max(1.0, abs(s))), k         # %.17g of the same double sum
