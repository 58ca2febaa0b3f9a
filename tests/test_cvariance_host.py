"""The variance model's tables section and dsd_variance_open's host checks, without a GPU: the config struct's layout, the
round trip of modelfile.variance_sections through the C reader for every variance case of tests/deploy_cases.py, one case
per refusal of the section validation (each made by editing the sections of a valid model before they are written), the
DSD_EINVAL answers that need no object, dsd_model_create's refusal of the kind, and the stand-alone sanitizer run of the
validation code (tools/harness/variance_harness.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import cvariance_cases as cc
import deploy_cases as dc
from diffsinger_amd import _lib, modelfile
from diffsinger_amd.hparams import hparams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOTFOUND = -1, -5


@pytest.fixture(autouse=True)
def _restore_hparams():
    yield
    hparams.clear()
    hparams.update(hidden_size=256)


def c_variance_open(path, prefix=cc.PREFIX):
    """-> (rc, object pointer, message); the file is closed again (the object does not refer to it)"""
    lib = _lib.lib()
    with modelfile.open(path) as f:
        vp = C.c_void_p(1)
        rc = lib.dsd_variance_open(f._f, prefix.encode(), 0, C.byref(vp))
        return rc, vp, lib.dsd_last_error(None).decode("utf-8", "replace")


def test_config_struct_layout_is_pinned():
    c = _lib.DsdVarianceConfig
    assert C.sizeof(c) == 184
    want = dict(struct_size=0, hidden_size=4, vocab_size=8, num_lang=12, num_spk=16, predict_dur=20, predict_pitch=24,
                use_melody_encoder=28, use_glide_embed=32, use_lang_id=36, use_spk_id=40, variances=44, melody_hidden_size=48,
                glide_rows=52, glide_embed_scale=56, smooth_width=60, pitch_repeat_bins=64, pitd_norm_min=68, pitd_norm_max=72,
                pitd_clip_min=76, pitd_clip_max=80, var_repeat_bins=84, var_norm_min=88, var_norm_max=104, var_clamp_min=120,
                var_clamp_max=136, var_no_clamp=152, diffusion_type=168, timesteps=172, k_step=176, time_scale_factor=180)
    assert [n for n, _ in c._fields_] == list(want)
    assert {n: getattr(c, n).offset for n in want} == want
    assert all(getattr(c, n).size == (16 if n.startswith("var_") and n != "var_repeat_bins" else 4) for n in want)
    assert (_lib.DSD_VARIANCE_TABLES, _lib.DSD_VAR_PITCH, _lib.DSD_VAR_VARIANCES, _lib.DSD_VAR_MAX_CURVES) == (10, 0, 1, 4)
    assert 9 not in _lib.KIND_CONFIGS and _lib.KIND_CONFIGS[10] is c
    assert [C.sizeof(t) for t in (_lib.DsdVarianceEncodeArgs, _lib.DsdVarianceDurArgs, _lib.DsdVariancePitchCondArgs,
                                  _lib.DsdVarianceCondArgs)] == [80, 64, 136, 104]


@pytest.mark.parametrize("tag", list(dc.VAR_CASES))
def test_sections_round_trip_bit_for_bit(tmp_path, tag):
    model, hp = cc.build_model(tag, cuda=False)
    path = tmp_path / "v.dsdm"
    sections = cc.pack(path, model)
    want_names = [cc.PREFIX + s for s in [".tables", ".fs2"] + [".melody"] * bool(hp["use_melody_encoder"] and hp["predict_pitch"]) +
                  [".pitch"] * bool(hp["predict_pitch"]) + [".variances"] * bool(dc.variance_names(hp))]
    assert [s.name for s in sections] == want_names
    sd = model.state_dict()
    with modelfile.open(path) as f:
        assert [(s.name, s.kind) for s in f.sections] == [(s.name, s.kind) for s in sections]
        assert f.sections[0].kind == 10
        for i, s in enumerate(sections):
            assert bytes(f.config(i)) == bytes(s.cfg)
            got = f.tensors(i)
            assert list(got) == list(s.tensors)
            for k, v in s.tensors.items():
                assert got[k].shape == np.asarray(v).shape and got[k].tobytes() == np.asarray(v, np.float32).tobytes(), (s.name, k)
        tables = f.tensors(0)
        cfg = f.config(0)
    # the tables are the wrapper's own parameters under their own names, and the mask is its cross-lingual list
    for k, v in tables.items():
        if k not in ("cross_lingual_mask", "smooth_taps"):
            assert v.tobytes() == sd[k].detach().numpy().tobytes(), k
    assert sorted(np.nonzero(tables["cross_lingual_mask"])[0].tolist()) == sorted(dc.VAR_CASES[tag].get("cross") or [])
    assert set(np.unique(tables["cross_lingual_mask"])) <= {0.0, 1.0}
    if hp["predict_pitch"]:         # the taps of this host's build_smooth_op travel with the tables
        from diffsinger_amd.deploy import smooth_kernel
        assert tables["smooth_taps"].tobytes() == smooth_kernel(dc.smooth_width(hp)).numpy().tobytes()
    else:
        assert "smooth_taps" not in tables
    assert not any(k.startswith(("fs2.encoder.", "pitch_predictor.", "variance_predictor.")) for k in tables)
    # every constant of the stages
    assert (cfg.hidden_size, cfg.vocab_size) == (dc.HIDDEN, dc.VOCAB)
    assert (cfg.predict_dur, cfg.predict_pitch, cfg.use_spk_id) == (int(hp["predict_dur"]), int(hp["predict_pitch"]), int(hp["use_spk_id"]))
    assert cfg.variances == sum(_lib.EMBED_FLAGS[n] for n in dc.variance_names(hp))
    if hp["predict_pitch"]:
        assert cfg.smooth_width == dc.smooth_width(hp) and cfg.pitch_repeat_bins == 8
        assert (cfg.pitd_norm_min, cfg.pitd_norm_max, cfg.pitd_clip_min, cfg.pitd_clip_max) == (-8.0, 8.0, -12.0, 12.0)
        assert cfg.use_melody_encoder == int(hp["use_melody_encoder"])
        if hp["use_melody_encoder"]:
            assert cfg.melody_hidden_size == 32 and cfg.use_glide_embed == int(hp["use_glide_embed"])
            assert cfg.glide_rows == (3 if hp["use_glide_embed"] else 0)
    names = dc.variance_names(hp)
    if names:
        assert cfg.var_repeat_bins == 12 // len(names)
        for n in names:
            slot = dc.VARIANCE_NAMES.index(n)
            lo, hi = (hp["tension_logit_min"], hp["tension_logit_max"]) if n == "tension" else (hp[n + "_db_min"], hp[n + "_db_max"])
            assert (cfg.var_norm_min[slot], cfg.var_norm_max[slot], cfg.var_clamp_min[slot]) == (lo, hi, lo)
            assert cfg.var_clamp_max[slot] == (hi if n == "tension" else 0.0) and cfg.var_no_clamp[slot] == 0
    assert cfg.diffusion_type == (1 if hp["diffusion_type"] == "reflow" else 0)
    assert (cfg.timesteps, cfg.k_step, cfg.time_scale_factor) == (1000, 1000, 1000.0)
    # a valid file passes every host check: what stops the open on a machine without a GPU is the device
    rc, vp, msg = c_variance_open(path)
    if torch.cuda.is_available():
        assert rc == 0 and vp.value, msg
        _lib.lib().dsd_variance_close(vp)
    else:
        assert rc < 0 and vp.value is None and "no HIP device" in msg, msg


def _tables(sections):
    return sections[0]


def _set(sections, **fields):
    cfg = _lib.DsdVarianceConfig.from_buffer_copy(sections[0].cfg)
    for k, v in fields.items():
        setattr(cfg, k, v)
    sections[0] = sections[0]._replace(cfg=cfg)


def _inner(sections, name, **fields):
    i = [s.name for s in sections].index(cc.PREFIX + name)
    cfg = type(sections[i].cfg).from_buffer_copy(sections[i].cfg)
    for k, v in fields.items():
        setattr(cfg, k, v)
    sections[i] = sections[i]._replace(cfg=cfg)


def _drop(name):
    return lambda s: _tables(s).tensors.pop(name)


def _add(name, shape):
    return lambda s: _tables(s).tensors.__setitem__(name, np.zeros(shape, np.float32))


def _reshape(name, shape):
    return lambda s: _tables(s).tensors.__setitem__(name, np.zeros(shape, np.float32))


def _mask_value(s):
    _tables(s).tensors["cross_lingual_mask"][3] = 0.5


def _remove_section(name):
    def edit(s):
        del s[[x.name for x in s].index(cc.PREFIX + name)]
    return edit


def _tables_of_another_kind(s):
    s[0] = modelfile.Section(s[0].name, s[1].kind, s[1].cfg, s[1].tensors)


# on word_melody: every flag set, so every tensor family is present.  (edit, words the message must hold)
REFUSALS = {
    "missing_txt": (_drop("fs2.txt_embed.weight"), ["lacks", "fs2.txt_embed.weight"]),
    "missing_mask": (_drop("cross_lingual_mask"), ["lacks", "cross_lingual_mask"]),
    "missing_lang": (_drop("fs2.lang_embed.weight"), ["lacks", "fs2.lang_embed.weight"]),
    "missing_onset": (_drop("fs2.onset_embed.weight"), ["lacks", "fs2.onset_embed.weight"]),
    "missing_word_dur_bias": (_drop("fs2.word_dur_embed.bias"), ["lacks", "fs2.word_dur_embed.bias"]),
    "missing_midi": (_drop("fs2.midi_embed.weight"), ["lacks", "fs2.midi_embed.weight"]),
    "missing_spk": (_drop("spk_embed.weight"), ["lacks", "spk_embed.weight"]),
    "missing_note_midi": (_drop("melody_encoder.note_midi_embed.weight"), ["lacks", "melody_encoder.note_midi_embed.weight"]),
    "missing_note_dur": (_drop("melody_encoder.note_dur_embed.bias"), ["lacks", "melody_encoder.note_dur_embed.bias"]),
    "missing_glide": (_drop("melody_encoder.note_glide_embed.weight"), ["lacks", "melody_encoder.note_glide_embed.weight"]),
    "missing_retake": (_drop("pitch_retake_embed.weight"), ["lacks", "pitch_retake_embed.weight"]),
    "missing_delta": (_drop("delta_pitch_embed.weight"), ["lacks", "delta_pitch_embed.weight"]),
    "extra_ph_dur": (_add("fs2.ph_dur_embed.weight", (64, 1)), ["excludes", "fs2.ph_dur_embed.weight"]),
    "extra_base_pitch": (_add("base_pitch_embed.bias", (64,)), ["excludes", "base_pitch_embed.bias"]),
    "extra_pitch_embed": (_add("pitch_embed.weight", (64, 1)), ["excludes", "pitch_embed.weight"]),
    "extra_variance_embed": (_add("variance_embeds.energy.weight", (64, 1)), ["excludes", "variance_embeds.energy.weight"]),
    "extra_unknown": (_add("fs2.encoder.layer_norm.weight", (64,)), ["do not have", "fs2.encoder.layer_norm.weight"]),
    "shape_txt_rows": (_reshape("fs2.txt_embed.weight", (dc.VOCAB + 1, 64)), ["fs2.txt_embed.weight", "must be [12, 64]"]),
    "shape_lin1_weight": (_reshape("fs2.word_dur_embed.weight", (64,)), ["fs2.word_dur_embed.weight", "must be [64, 1]"]),
    "shape_melody_width": (_reshape("melody_encoder.note_dur_embed.bias", (64,)), ["melody_encoder.note_dur_embed.bias", "must be [32]"]),
    "shape_glide_rows": (_reshape("melody_encoder.note_glide_embed.weight", (2, 32)), ["note_glide_embed.weight", "must be [3, 32]"]),
    "shape_mask": (_reshape("cross_lingual_mask", (dc.VOCAB, 1)), ["cross_lingual_mask", "must be [12]"]),
    "shape_taps": (_reshape("smooth_taps", (4,)), ["smooth_taps", "must be [5]"]),
    "taps_not_finite": (lambda s: _tables(s).tensors["smooth_taps"].__setitem__(2, np.inf), ["smooth_taps[2] is not finite"]),
    "taps_sum": (lambda s: _tables(s).tensors.__setitem__("smooth_taps", np.full(5, 0.25, np.float32)), ["smooth_taps sum to 1.25"]),
    "mask_value": (_mask_value, ["cross_lingual_mask[3]", "neither 0 nor 1"]),
    "k_zero": (lambda s: _set(s, smooth_width=0), ["smooth_width K = 0", "[1, 255]"]),
    "k_256": (lambda s: _set(s, smooth_width=256), ["smooth_width K = 256", "[1, 255]"]),
    "flag_value": (lambda s: _set(s, predict_dur=2), ["predict_dur = 2", "neither 0 nor 1"]),
    "variance_bits": (lambda s: _set(s, variances=16), ["variances = 0x10"]),
    "glide_without_melody": (lambda s: _set(s, use_melody_encoder=0), ["use_glide_embed without use_melody_encoder"]),
    "inner_fs2_hidden": (lambda s: _inner(s, ".fs2", hidden_size=32), ["fs2.hidden_size = 32", "tables.hidden_size = 64"]),
    "inner_fs2_no_dur": (lambda s: _inner(s, ".fs2", dur_layers=0), ["fs2.dur_layers = 0", "tables.predict_dur = 1"]),
    "inner_melody_out": (lambda s: _inner(s, ".melody", out_dims=32), ["melody.out_dims = 32", "tables.hidden_size = 64"]),
    "inner_melody_hidden": (lambda s: _set(s, melody_hidden_size=16), []),          # the tables' own shapes fail first
    "inner_pitch_bins": (lambda s: _inner(s, ".pitch", in_dims=4), ["pitch.in_dims = 4", "tables.pitch_repeat_bins = 8"]),
    "inner_pitch_feats": (lambda s: _inner(s, ".pitch", n_feats=2), ["pitch.n_feats = 2"]),
    "inner_pitch_hidden": (lambda s: _inner(s, ".pitch", hidden_size=128), ["pitch.hidden_size = 128", "tables.hidden_size = 64"]),
    "no_tables_section": (_remove_section(".tables"), ['no section "var.tables"']),
    "no_melody_section": (_remove_section(".melody"), ['no section "var.melody"']),
    "no_pitch_section": (_remove_section(".pitch"), ['no section "var.pitch"']),
    "tables_of_another_kind": (_tables_of_another_kind, ["var.tables", "not DSD_VARIANCE_TABLES"]),
}


@pytest.fixture(scope="module")
def _melody_model():
    return cc.build_model("word_melody", cuda=False)


@pytest.fixture
def melody_model(_melody_model):
    """built once; the hparams its sections are made from are set again for every test"""
    model, hp = _melody_model
    hparams.clear()
    hparams.update(hp, infer=True)
    return model


@pytest.mark.parametrize("name", list(REFUSALS))
def test_open_refuses(tmp_path, melody_model, name):
    edit, words = REFUSALS[name]
    path = tmp_path / "bad.dsdm"
    cc.pack(path, melody_model, edit=edit)
    rc, vp, msg = c_variance_open(path)
    assert rc == (ENOTFOUND if name.startswith("no_") else EINVAL), (rc, msg)
    assert vp.value is None                                                 # *out = NULL
    assert msg.startswith("dsd_variance_open:") and all(w in msg for w in words), msg


def test_open_refuses_inner_mismatches_of_the_variance_predictor(tmp_path):
    model, _ = cc.build_model("var_three", cuda=False)
    for edit, words in ((lambda s: _inner(s, ".variances", in_dims=6), ["variances.in_dims = 6", "tables.var_repeat_bins = 4"]),
                        (lambda s: _inner(s, ".variances", n_feats=2), ["variances.n_feats = 2", "tables.variances"]),
                        (lambda s: _inner(s, ".fs2", dur_layers=2, dur_chans=48, dur_kernel_size=3),
                         ["fs2.dur_layers = 2", "tables.predict_dur = 0"]),
                        (_drop("variance_embeds.voicing.bias"), ["lacks", "variance_embeds.voicing.bias"]),
                        (_drop("fs2.ph_dur_embed.weight"), ["lacks", "fs2.ph_dur_embed.weight"]),
                        (_add("fs2.onset_embed.weight", (2, 64)), ["excludes", "fs2.onset_embed.weight"]),
                        (_add("pitch_retake_embed.weight", (2, 64)), ["excludes", "pitch_retake_embed.weight"]),
                        (_add("smooth_taps", (5,)), ["excludes", "smooth_taps"])):
        path = tmp_path / "bad.dsdm"
        cc.pack(path, model, edit=edit)
        rc, vp, msg = c_variance_open(path)
        assert rc == EINVAL and vp.value is None and all(w in msg for w in words), msg


def test_einval_without_an_object(tmp_path, melody_model):
    lib = _lib.lib()
    path = tmp_path / "ok.dsdm"
    cc.pack(path, melody_model)
    out = C.c_void_p(1)
    with modelfile.open(path) as f:
        for args in ((None, b"var", 0, C.byref(out)), (f._f, None, 0, C.byref(out)), (f._f, b"var", 0, None)):
            assert lib.dsd_variance_open(*args) == EINVAL and b"NULL argument" in lib.dsd_last_error(None)
        assert out.value is None
        assert lib.dsd_variance_open(f._f, b"x" * 250, 0, C.byref(out)) == EINVAL and b"prefix" in lib.dsd_last_error(None)
        assert lib.dsd_variance_open(f._f, b"other", 0, C.byref(out)) == ENOTFOUND
        assert b'no section "other.tables"' in lib.dsd_last_error(None)
    lib.dsd_variance_close(None)
    ptr = C.cast((C.c_float * 64)(), C.c_void_p)
    cfg = _lib.DsdVarianceConfig()
    assert lib.dsd_variance_info(None, C.byref(cfg)) == EINVAL and b"dsd_variance_info" in lib.dsd_last_error(None)
    assert lib.dsd_variance_backbone(None, 0, C.byref(out)) == EINVAL and b"dsd_variance_backbone" in lib.dsd_last_error(None)
    for name, cls in (("dsd_variance_encode", _lib.DsdVarianceEncodeArgs), ("dsd_variance_dur", _lib.DsdVarianceDurArgs),
                      ("dsd_variance_pitch_cond", _lib.DsdVariancePitchCondArgs), ("dsd_variance_cond", _lib.DsdVarianceCondArgs)):
        a = cls()
        a.struct_size = C.sizeof(cls)
        assert getattr(lib, name)(None, C.byref(a), None) == EINVAL
        assert lib.dsd_last_error(None).decode() == f"{name}: NULL object"
    assert lib.dsd_variance_pitch_post(None, ptr, ptr, 1, 4, ptr, None) == EINVAL
    assert lib.dsd_last_error(None) == b"dsd_variance_pitch_post: NULL object"
    assert lib.dsd_variance_post(None, ptr, 1, 4, (C.c_void_p * 4)(ptr.value), None) == EINVAL
    assert lib.dsd_last_error(None) == b"dsd_variance_post: NULL object"


def test_model_create_refuses_the_tables_kind(tmp_path, melody_model):
    lib = _lib.lib()
    path = tmp_path / "ok.dsdm"
    cc.pack(path, melody_model)
    with modelfile.open(path) as f:
        h = C.c_void_p(1)
        assert lib.dsd_model_create(f._f, f.index("var.tables"), 0, C.byref(h)) == EINVAL and h.value is None
        msg = lib.dsd_last_error(None).decode()
        assert "dsd_model_create" in msg and "var.tables" in msg and "dsd_variance_open" in msg


def test_variance_config_refuses_a_width_outside_the_kernel(melody_model):
    hparams.update(midi_smooth_width=3.0)                                # K = 258
    with pytest.raises(ValueError, match="outside"):
        modelfile.variance_config(melody_model)


def test_documented_taps_stay_close_to_torchs():
    """The taps dsd_variance_open computes for a section without `smooth_taps` (restated in cvariance_cases.library_taps; the
    sanitizer test below holds the C code's bits against it) against the Python twin's, which come out of torch's CPU sin and sum.  Bound: 2^-20 of the tap.  torch's fp32 sin is
    within one ulp of the rounded value the library takes (2^-23 of it); its fp32 sum of up to 255 terms, added in a
    machine-dependent cascade of about log2(255) = 8 roundings, is within 8 * 2^-24 = 2^-21 of the sum the library rounds
    once; each side's division rounds once more (2 * 2^-24): 0.75 * 2^-20 in all.  Equal bit for bit at the stock widths
    K = 5 (hop 512) and K = 21 (hop 128); NaN on both sides at K = 1."""
    from diffsinger_amd.deploy import smooth_kernel
    assert torch.isnan(cc.library_taps(1)).all() and torch.isnan(smooth_kernel(1)).all()
    worst, worst_ulp, differ = 0.0, 0.0, 0
    for k in range(2, 256):
        mine, theirs = cc.library_taps(k).numpy(), smooth_kernel(k).numpy()
        scale = np.maximum(np.abs(mine), np.abs(theirs))
        gap = np.abs(mine.astype(np.float64) - theirs)
        worst = max(worst, float((gap[scale > 0] / scale[scale > 0]).max()))
        worst_ulp = max(worst_ulp, float((gap / np.spacing(scale.astype(np.float32))).max()))
        differ += int(not np.array_equal(mine.view(np.uint32), theirs.view(np.uint32)))
    print(f"K = 2 .. 255: {differ} tap sets differ somewhere; max distance {worst:.3e} of the tap ({worst_ulp} ulp), bound {2.0 ** -20:.3e}")
    assert worst <= 2.0 ** -20
    for k in (5, 21):
        assert np.array_equal(cc.library_taps(k).numpy().view(np.uint32), smooth_kernel(k).numpy().view(np.uint32)), k


def test_pack_model_packs_a_variance_experiment(tmp_path):
    """examples/pack_model.py's variance half on a synthetic experiment directory (config.yaml, dictionary, checkpoint): the
    sections dsd_variance_open looks for, the checkpoint's own tables in them, and a file the C reader accepts."""
    import importlib.util
    import json
    import yaml
    import variance_cases as vc
    from diffsinger_amd.variance import DiffSingerVariance
    exp = tmp_path / "exp"
    exp.mkdir()
    hp = vc.case_hparams("word_reflow")
    hp.update(vc.HARNESS_HP, hidden_size=64, use_melody_encoder=True, num_spk=3)
    (exp / "config.yaml").write_text(yaml.safe_dump(hp))
    (exp / "dictionary.txt").write_text("ab\ta b\ncd\tc d\ne\te\n", encoding="utf8")
    (exp / "spk_map.json").write_text(json.dumps(vc.HARNESS_SPK))
    hparams.clear()
    hparams.update(hp, infer=True)
    model = DiffSingerVariance(8)
    sd = dict(model.state_dict())
    sd.update({k: torch.from_numpy(v) for k, v in vc.synth_weights(vc.sorted_param_shapes(model.named_parameters()), 89).items()})
    torch.save({"state_dict": {"model." + k: v for k, v in sd.items()}, "category": "variance"}, exp / "model_ckpt_steps_7.ckpt")
    spec = importlib.util.spec_from_file_location("pack_model", os.path.join(ROOT, "examples", "pack_model.py"))
    pack_model = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pack_model)
    sections = pack_model.variance_sections(exp, "singer", None)
    names = [s.name for s in sections]
    assert names[:2] == ["singer.tables", "singer.fs2"] and "singer.melody" in names and "singer.pitch" in names
    assert sections[0].kind == 10 and sections[0].cfg.hidden_size == 64 and sections[0].cfg.use_melody_encoder == 1
    for k in ("fs2.txt_embed.weight", "pitch_retake_embed.weight", "delta_pitch_embed.bias"):
        assert sections[0].tensors[k].tobytes() == sd[k].numpy().tobytes(), k
    assert not sections[0].tensors["cross_lingual_mask"].any()             # one language: nothing is cross-lingual
    path = tmp_path / "voice.dsdm"
    modelfile.write(path, sections)
    rc, vp, msg = c_variance_open(path, "singer")
    if torch.cuda.is_available():
        assert rc == 0, msg
        _lib.lib().dsd_variance_close(vp)
    else:
        assert "no HIP device" in msg, msg                                  # every host check passed


def test_validation_under_sanitizers(tmp_path):
    """tools/harness/variance_harness.cpp: the section validation, the inner-config check and the taps, compiled with the
    host compiler's address and undefined-behaviour sanitizers into a stand-alone program, on heap buffers of exact size."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = tmp_path / "variance_harness"
    # the sanitizer runtimes are linked into the program itself (g++ links them dynamically unless told otherwise; clang
    # links them statically and does not know -static-libubsan)
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) == "g++" else []
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static,
           "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tools", "harness", "variance_harness.cpp"), "-x", "c++",
           os.path.join(ROOT, "diffsinger_amd", "csrc", "variance_tables.hip"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert built.returncode == 0, built.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    assert "0 failed" in run.stdout, run.stdout
    # the C fallback's taps, bit for bit, against the restatement the other tests use (K = 1: a NaN on both sides)
    seen = []
    for line in run.stdout.splitlines():
        if line.startswith("taps "):
            words = line.split()
            k, got = int(words[1]), np.array([int(x, 16) for x in words[2:]], dtype=np.uint32).view(np.float32)
            want = cc.library_taps(k).numpy()
            assert got.shape == want.shape == (k,)
            assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(got)].view(np.uint32),
                                                                                     want[~np.isnan(want)].view(np.uint32)), k
            seen.append(k)
    assert seen == [1, 2, 3, 4, 5, 21, 64, 255]
