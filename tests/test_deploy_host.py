"""CPU-side checks of the staged deployment entry points (diffsinger_amd/deploy.py, dsd_length_regulate,
dsd_frame_curve): the G22 fixture agrees with tests/deploy_cases.py, the classes add no parameters to their parents, the
two C entries reject bad shapes before they touch a device, and CPU tensors are refused.  No compute calls."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import deploy_cases as dc
from diffsinger_amd.hparams import hparams

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g22_deploy.npz")


@pytest.fixture(autouse=True)
def _restore_hparams():
    yield
    hparams.clear()
    hparams.update(hidden_size=256)


def expected_keys():
    keys = {f"lr_{tag}" for tag in dc.LR_CASES}
    for tag, c in dc.VAR_CASES.items():
        hp = dc.variance_hparams(tag)
        keys |= {f"{tag}_{k}" for k in ("params", "enc", "x_masks", "mel2ph")}
        if hp["predict_dur"]:
            keys |= {f"{tag}_ph2word", f"{tag}_dur_pred"}
        if hp["predict_pitch"]:
            keys |= {f"{tag}_{k}" for k in ("mel2note", "pitch_cond", "base_pitch")}
            if c["steps"]:
                keys |= {f"{tag}_x_pred", f"{tag}_pitch_pred"}
        names = dc.variance_names(hp)
        if names:
            keys |= {f"{tag}_var_cond", f"{tag}_xs_pred"} | {f"{tag}_out_{n}" for n in names}
    for tag, c in dc.AC_CASES.items():
        keys |= {f"{tag}_params", f"{tag}_cond"} | {f"{tag}_{stage}" for stage, _ in c["stages"]}
        if dc.acoustic_hparams(tag)["use_shallow_diffusion"]:
            keys.add(f"{tag}_aux")
    return keys


def test_fixture_keys_and_shapes_agree_with_the_cases():
    g = np.load(GOLDEN)
    assert set(g.files) == expected_keys()
    for tag in dc.LR_CASES:
        dur = dc.lr_durations(tag)
        want = g[f"lr_{tag}"]
        assert want.dtype == np.int64 and want.shape == (dur.shape[0], int(dur.sum(1).max()))
        assert np.array_equal(want, dc.length_regulate_numpy(dur, want.shape[1]))
    assert g["lr_one_frame"].shape[1] == 1 and dc.lr_durations("l2048").shape[1] == 2048
    for tag, c in dc.VAR_CASES.items():
        hp, inp = dc.variance_hparams(tag), dc.variance_inputs(tag)
        assert g[f"{tag}_enc"].shape == (1, c["n_ph"], dc.HIDDEN)
        assert inp["ph_dur"].sum() == c["t_len"] and inp["word_div"].sum() == c["n_ph"]
        assert g[f"{tag}_mel2ph"].shape == (1, c["t_len"])
        if hp["predict_pitch"]:
            assert g[f"{tag}_base_pitch"].shape == (1, c["t_len"]) and inp["note_dur"].sum() == c["t_len"]
    widths = {tag: dc.smooth_width(dc.variance_hparams(tag)) for tag in dc.VAR_CASES}
    assert [widths[t] for t in ("word_melody", "word_base", "melody_even", "k_one", "short_clip")] == [5, 21, 4, 1, 5]
    assert dc.VAR_CASES["short_clip"]["t_len"] < widths["short_clip"]
    assert np.isnan(g["k_one_base_pitch"]).all()            # sin(0) / sin(0): the reference's K = 1 operator
    assert all(np.isfinite(g[k]).all() for k in g.files if g[k].dtype.kind == "f" and not k.startswith("k_one"))


def _variance_pair(tag):
    from diffsinger_amd.deploy import DiffSingerVarianceDeploy
    from diffsinger_amd.variance import DiffSingerVariance
    hparams.clear()
    hparams.update(dc.variance_hparams(tag), infer=True)
    return DiffSingerVarianceDeploy(dc.VOCAB, cross_lingual_token_idx=dc.VAR_CASES[tag].get("cross")), DiffSingerVariance(dc.VOCAB)


def _acoustic_pair(tag):
    from diffsinger_amd.deploy import DiffSingerAcousticDeploy
    from diffsinger_amd.toplevel import DiffSingerAcoustic
    hparams.clear()
    hparams.update(dc.acoustic_hparams(tag), infer=True)
    return (DiffSingerAcousticDeploy(dc.VOCAB, dc.M_BINS, cross_lingual_token_idx=dc.AC_CASES[tag].get("cross")),
            DiffSingerAcoustic(dc.VOCAB, dc.M_BINS))


@pytest.mark.parametrize("tag", ["word_melody", "word_base", "var_three"])
def test_variance_deploy_state_dict_is_the_parents_and_the_references(tag):
    g = np.load(GOLDEN)
    mine, parent = _variance_pair(tag)
    assert list(mine.state_dict()) == list(parent.state_dict())
    assert {k: tuple(v.shape) for k, v in mine.state_dict().items()} == {k: tuple(v.shape) for k, v in parent.state_dict().items()}
    shapes = dc.sorted_param_shapes(mine.named_parameters())
    assert [f"{n}:{'x'.join(map(str, sh))}" for n, sh in shapes.items()] == [str(s) for s in g[f"{tag}_params"]]
    assert "cross_lingual_token_idx" not in mine.state_dict()


@pytest.mark.parametrize("tag", ["aux_ddpm", "gender_velocity"])
def test_acoustic_deploy_state_dict_is_the_parents_and_the_references(tag):
    g = np.load(GOLDEN)
    mine, parent = _acoustic_pair(tag)
    assert list(mine.state_dict()) == list(parent.state_dict())
    shapes = dc.sorted_param_shapes(mine.named_parameters())
    assert [f"{n}:{'x'.join(map(str, sh))}" for n, sh in shapes.items()] == [str(s) for s in g[f"{tag}_params"]]


def test_discrete_f0_twin_has_the_references_parameters():
    g = np.load(GOLDEN)
    mine, _ = _acoustic_pair("discrete_f0")
    shapes = dc.sorted_param_shapes(mine.named_parameters())
    assert shapes["fs2.pitch_embed.weight"] == (300, dc.HIDDEN) and "fs2.pitch_embed.bias" not in shapes
    assert [f"{n}:{'x'.join(map(str, sh))}" for n, sh in shapes.items()] == [str(s) for s in g["discrete_f0_params"]]


def test_an_empty_cross_lingual_list_switches_the_language_embedding_off():
    mine, _ = _variance_pair("word_melody")
    assert mine.fs2.use_lang_id and mine.cross_lingual_token_idx.tolist() == [2, 3, 5, 7]
    from diffsinger_amd.deploy import DiffSingerVarianceDeploy
    assert not DiffSingerVarianceDeploy(dc.VOCAB, cross_lingual_token_idx=[]).fs2.use_lang_id


def test_length_regulate_rejects_bad_shapes():
    from diffsinger_amd import _lib
    lib = _lib.lib()
    buf = (C.c_int64 * 8)()
    ptr = C.cast(buf, C.c_void_p)
    for args, msg in (((0, None, 1, 4, 4, ptr, None), b"null argument"),
                      ((0, ptr, 0, 4, 4, ptr, None), b"must be positive"),
                      ((0, ptr, 1, -3, 4, ptr, None), b"must be positive"),         # a negative token count
                      ((0, ptr, 1, 2049, 4, ptr, None), b"exceeds the 2048 tokens"),
                      ((0, ptr, 1, 4, 0, ptr, None), b"T must be positive"),
                      ((0, ptr, 1, 4, -1, ptr, None), b"T must be positive")):
        assert lib.dsd_length_regulate(*args) == -1, args               # DSD_EINVAL
        assert msg in lib.dsd_last_error(None)


def test_frame_curve_rejects_bad_shapes():
    from diffsinger_amd import _lib
    lib = _lib.lib()
    buf = (C.c_float * 8)()
    ptr = C.cast(buf, C.c_void_p)
    w = (C.c_float * 256)()
    good = [0, ptr, ptr, ptr, ptr, 1, 2, 4, None, w, 5, ptr, ptr, ptr, None]

    def call(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return lib.dsd_frame_curve(*a)

    for kw, msg in ((dict(a1=None), b"null argument"), (dict(a13=None), b"null argument"), (dict(a9=None), b"null argument"),
                    (dict(a5=0), b"must be positive"), (dict(a6=0), b"must be positive"), (dict(a7=0), b"must be positive"),
                    (dict(a10=0), b"outside [1, 255]"), (dict(a10=256), b"outside [1, 255]"),
                    (dict(a8=(C.c_int32 * 1)(5)), b"outside [0, T = 4]"), (dict(a8=(C.c_int32 * 1)(-1)), b"outside [0, T = 4]")):
        assert call(**kw) == -1, kw
        assert msg in lib.dsd_last_error(None), kw


def test_cpu_tensors_are_refused():
    from diffsinger_amd import deploy
    with pytest.raises(RuntimeError, match="no CPU path"):
        deploy.length_regulate(torch.ones(1, 3, dtype=torch.long), 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        deploy.frame_curve(torch.zeros(1, 2), torch.ones(1, 4, dtype=torch.long), torch.zeros(1, 4),
                           torch.zeros(1, 4, dtype=torch.bool), deploy.smooth_kernel(5))
    mine, _ = _variance_pair("word_melody")
    inp = {k: torch.from_numpy(v) for k, v in dc.variance_inputs("word_melody").items()}
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU path"):
        mine.forward_linguistic_encoder_word(inp["tokens"], inp["word_div"], inp["word_dur"], languages=inp["languages"])
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU path"):
        mine.forward_pitch_preprocess(torch.zeros(1, 9, dc.HIDDEN), inp["ph_dur"], note_midi=inp["note_midi"],
                                      note_rest=inp["note_rest"], note_dur=inp["note_dur"], pitch=inp["pitch"],
                                      retake=inp["retake"])
    with pytest.raises(RuntimeError, match="inference-only"):
        mine.forward_linguistic_encoder_word(inp["tokens"], inp["word_div"], inp["word_dur"], languages=inp["languages"])
    ac, _ = _acoustic_pair("plain_ddpm")
    a = {k: torch.from_numpy(v) for k, v in dc.acoustic_inputs("plain_ddpm").items()}
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU path"):
        ac.forward_fs2_aux(a["tokens"], a["durations"], a["f0"], {})


def test_smoothing_taps_are_the_references():
    """build_smooth_op (toplevel.py:189-192): sin(pi * linspace(0, 1, K)) in fp32 over its fp32 sum."""
    from diffsinger_amd.deploy import smooth_kernel
    for k in (4, 5, 21):
        w = smooth_kernel(k)
        assert w.dtype == torch.float32 and w.shape == (k,) and abs(float(w.sum()) - 1.0) < 1e-6
        assert torch.allclose(w, w.flip(0), atol=1e-7) and float(w[0]) == 0.0
    assert torch.isnan(smooth_kernel(1)).all()


def test_exports_cover_the_new_entries():
    from diffsinger_amd import _lib
    from test_cabi_exports import header_functions
    assert {"dsd_length_regulate", "dsd_frame_curve"} <= set(_lib.EXPORTS)
    assert sorted(_lib.EXPORTS) == header_functions()
    assert _lib.lib().dsd_api_version() == 10
