"""The acoustic model's tables section, dsd_acoustic_open's host checks and dsd_acoustic_plan, without a GPU: the layout of
the config and plan structs, the round trip of modelfile.acoustic_sections through the C reader for every acoustic case of
tests/deploy_cases.py, one case per refusal of the section validation (each made by editing the sections of a valid model
before they are written), dsd_model_create's refusal of the kind, the plan call against the Python twin's own rules
(schedule.onnx_ddpm_plan, GaussianDiffusion._start_state, RectifiedFlow.forward_onnx), its DSD_EINVAL answers, and the
stand-alone sanitizer run of the validation and plan code (tools/harness/acoustic_harness.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import cacoustic_cases as cc
import deploy_cases as dc
from diffsinger_amd import _lib, modelfile, schedule
from diffsinger_amd.hparams import hparams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOTFOUND = -1, -5
DEPTHS = (None, 0, 0.001, 0.004, 0.06, 0.3, 0.4, 0.9, 1)


@pytest.fixture(autouse=True)
def _restore_hparams():
    yield
    hparams.clear()
    hparams.update(hidden_size=256)


def c_acoustic_open(path, prefix=cc.PREFIX):
    """-> (rc, object pointer, message); the file is closed again (the object does not refer to it)"""
    lib = _lib.lib()
    with modelfile.open(path) as f:
        ap = C.c_void_p(1)
        rc = lib.dsd_acoustic_open(f._f, prefix.encode(), 0, C.byref(ap))
        return rc, ap, lib.dsd_last_error(None).decode("utf-8", "replace")


def c_plan(cfg, depth, steps):
    p = _lib.DsdAcousticPlan()
    rc = _lib.lib().dsd_acoustic_plan(C.byref(cfg), -1.0 if depth is None else float(depth), steps, C.byref(p))
    return rc, p, _lib.lib().dsd_last_error(None).decode()


def bits(x):
    return np.float32(x).view(np.uint32)


def test_struct_layouts_are_pinned():
    c = _lib.DsdAcousticConfig
    assert C.sizeof(c) == 96
    want = dict(struct_size=0, hidden_size=4, vocab_size=8, out_dims=12, num_lang=16, num_spk=20, use_lang_id=24, use_spk_id=28,
                embed_flags=32, f0_discrete=36, use_shallow_diffusion=40, shift_min=44, shift_max=48, speed_min=52, speed_max=56,
                mel_base_e=60, diffusion_type=64, timesteps=68, k_step=72, schedule_type=76, max_beta=80, t_start=88,
                time_scale_factor=92)
    assert [n for n, _ in c._fields_] == list(want)
    assert {n: getattr(c, n).offset for n in want} == want
    assert all(getattr(c, n).size == (8 if n == "max_beta" else 4) for n in want)
    p = _lib.DsdAcousticPlan
    want = dict(mode=0, start=4, t_max=8, speedup=12, t_start=16, n_step_noise=20, src_scale=24, noise_scale=28, steps=32)
    assert C.sizeof(p) == 36 and [n for n, _ in p._fields_] == list(want) and {n: getattr(p, n).offset for n in want} == want
    a = _lib.DsdAcousticConditionArgs
    assert C.sizeof(a) == 136 and (a.curves.offset, a.spk_rows.offset, a.languages.offset, a.f0_coarse.offset) == (40, 96, 104, 128)
    assert (_lib.DSD_ACOUSTIC_TABLES, _lib.DSD_AC_FS2, _lib.DSD_AC_AUX, _lib.DSD_AC_DENOISER) == (11, 0, 1, 2)
    assert (_lib.DSD_AC_START_NOISE, _lib.DSD_AC_START_MIX, _lib.DSD_AC_START_SOURCE) == (0, 1, 2)
    assert _lib.KIND_CONFIGS[11] is c and _lib.DSD_API_VERSION == 10 == _lib.lib().dsd_api_version()


@pytest.mark.parametrize("tag", list(dc.AC_CASES))
def test_sections_round_trip_bit_for_bit(tmp_path, tag):
    model, hp = cc.build_model(tag, cuda=False)
    c = dc.AC_CASES[tag]
    path = tmp_path / "a.dsdm"
    sections = cc.pack(path, model)
    shallow = bool(hp["use_shallow_diffusion"])
    assert [s.name for s in sections] == [cc.PREFIX + s for s in [".tables", ".fs2"] + [".aux"] * shallow + [".denoiser"]]
    with modelfile.open(path) as f:
        assert [(s.name, s.kind) for s in f.sections] == [(s.name, s.kind) for s in sections]
        assert [s.kind for s in f.sections] == [11, 3] + [2] * shallow + [0]
        for i, s in enumerate(sections):
            assert bytes(f.config(i)) == bytes(s.cfg)
            got = f.tensors(i)
            assert list(got) == list(s.tensors)
            for k, v in s.tensors.items():
                assert got[k].shape == np.asarray(v).shape and got[k].tobytes() == np.asarray(v, np.float32).tobytes(), (s.name, k)
        tables, cfg, fs2 = f.tensors(0), f.config(0), f.tensors(1)
    discrete = hp.get("f0_embed_type") == "discrete"
    assert list(tables) == ["cross_lingual_mask", "spec_min", "spec_max"] + ["fs2.pitch_embed.weight"] * discrete
    assert sorted(np.nonzero(tables["cross_lingual_mask"])[0].tolist()) == sorted(c.get("cross") or [])
    assert set(np.unique(tables["cross_lingual_mask"])) <= {0.0, 1.0}
    assert tables["spec_min"].tobytes() == np.float32(hp["spec_min"]).tobytes() and tables["spec_max"].tobytes() == np.float32(hp["spec_max"]).tobytes()
    if discrete:        # the lookup travels with the tables; the encoder's own Linear(1, H) pitch term is stored as zeros
        assert tables["fs2.pitch_embed.weight"].tobytes() == model.fs2.pitch_embed.weight.detach().numpy().tobytes()
        assert fs2["pitch_embed.weight"].shape == (dc.HIDDEN, 1) and not fs2["pitch_embed.weight"].any() and not fs2["pitch_embed.bias"].any()
    # every constant of the stages
    assert (cfg.hidden_size, cfg.vocab_size, cfg.out_dims) == (dc.HIDDEN, dc.VOCAB, dc.M_BINS)
    assert (cfg.use_lang_id, cfg.use_spk_id) == (int(hp["use_lang_id"]), int(hp["use_spk_id"]))
    assert (cfg.num_lang, cfg.num_spk) == (hp["num_lang"] if hp["use_lang_id"] else 0, hp["num_spk"] if hp["use_spk_id"] else 0)
    flags = sum(_lib.EMBED_FLAGS[n] for n in dc.VARIANCE_NAMES if hp[f"use_{n}_embed"])
    flags |= 16 * bool(hp["use_key_shift_embed"]) | 32 * bool(hp["use_speed_embed"])
    assert cfg.embed_flags == flags and cfg.f0_discrete == int(discrete) and cfg.use_shallow_diffusion == int(shallow)
    if hp["use_key_shift_embed"]:
        assert (cfg.shift_min, cfg.shift_max, cfg.speed_min, cfg.speed_max) == (-5.0, 5.0, 0.5, 2.0)
    assert cfg.mel_base_e == 0                                              # the cases leave mel_base at its default, '10'
    if hp["diffusion_type"] == "reflow":
        assert cfg.diffusion_type == 1 and cfg.time_scale_factor == 1000.0 and bits(cfg.t_start) == bits(0.4 if shallow else 0.0)
    else:
        assert (cfg.diffusion_type, cfg.timesteps, cfg.k_step, cfg.schedule_type, cfg.max_beta) == \
            (0, 1000, hp["K_step"] if shallow else 1000, 0, 0.01)
    # a valid file passes every host check: what stops the open on a machine without a GPU is the device
    rc, ap, msg = c_acoustic_open(path)
    if torch.cuda.is_available():
        assert rc == 0 and ap.value, msg
        _lib.lib().dsd_acoustic_close(ap)
    else:
        assert rc < 0 and ap.value is None and "no HIP device" in msg, msg


def _tables(sections):
    return sections[0]


def _set(sections, **fields):
    cfg = _lib.DsdAcousticConfig.from_buffer_copy(sections[0].cfg)
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


def _put(name, shape, value=0.0):
    return lambda s: _tables(s).tensors.__setitem__(name, np.full(shape, value, np.float32))


def _at(name, i, value):
    return lambda s: _tables(s).tensors[name].__setitem__(i, value)


def _remove_section(name):
    def edit(s):
        del s[[x.name for x in s].index(cc.PREFIX + name)]
    return edit


def _tables_of_another_kind(s):
    s[0] = modelfile.Section(s[0].name, s[1].kind, s[1].cfg, s[1].tensors)


def _section_of_another_kind(name):
    def edit(s):
        i = [x.name for x in s].index(cc.PREFIX + name)
        j = [x.name for x in s].index(cc.PREFIX + (".denoiser" if name != ".denoiser" else ".fs2"))
        s[i] = modelfile.Section(s[i].name, s[j].kind, s[j].cfg, s[j].tensors)
    return edit


# on the `batch` model: every embedding and shallow diffusion, so every rule applies.  (edit, words the message must hold)
REFUSALS = {
    "missing_mask": (_drop("cross_lingual_mask"), ["lacks", "cross_lingual_mask"]),
    "missing_spec_min": (_drop("spec_min"), ["lacks", "spec_min"]),
    "missing_spec_max": (_drop("spec_max"), ["lacks", "spec_max"]),
    "extra_pitch_embed": (_put("fs2.pitch_embed.weight", (300, 64)), ["excludes", "fs2.pitch_embed.weight"]),
    "extra_unknown": (_put("fs2.txt_embed.weight", (12, 64)), ["do not have", "fs2.txt_embed.weight"]),
    "shape_mask": (_put("cross_lingual_mask", (dc.VOCAB, 1)), ["cross_lingual_mask", "must be [12]"]),
    "shape_spec_min": (_put("spec_min", (1,), -12.0), ["spec_min", "must be [16]"]),
    "shape_spec_max": (_put("spec_max", (17,), 1.0), ["spec_max", "must be [16]"]),
    "shape_frozen_spk": (_put("frozen_spk_embed", (1, 64)), ["frozen_spk_embed", "must be [64]"]),
    "shape_frozen_key_shift": (_put("frozen_key_shift", (2,)), ["frozen_key_shift", "must be [1]"]),
    "mask_value": (_at("cross_lingual_mask", 3, 0.5), ["cross_lingual_mask[3]", "neither 0 nor 1"]),
    "spec_order": (_at("spec_max", 15, -20.0), ["spec_max[15]", "spec_min[15]"]),
    "spec_equal": (lambda s: _tables(s).tensors["spec_max"].__setitem__(0, _tables(s).tensors["spec_min"][0]), ["spec_max[0]"]),
    "flag_lang": (lambda s: _set(s, use_lang_id=2), ["use_lang_id = 2", "neither 0 nor 1"]),
    "flag_spk": (lambda s: _set(s, use_spk_id=-1), ["use_spk_id = -1", "neither 0 nor 1"]),
    "flag_discrete": (lambda s: _set(s, f0_discrete=3), ["f0_discrete = 3", "neither 0 nor 1"]),
    "flag_shallow": (lambda s: _set(s, use_shallow_diffusion=2), ["use_shallow_diffusion = 2", "neither 0 nor 1"]),
    "flag_mel_base": (lambda s: _set(s, mel_base_e=7), ["mel_base_e = 7", "neither 0 nor 1"]),
    "embed_bits": (lambda s: _set(s, embed_flags=64), ["embed_flags = 0x40"]),
    "shift_min_positive": (lambda s: _set(s, shift_min=0.5), ["shift_min = 0.5"]),
    "shift_max_negative": (lambda s: _set(s, shift_max=-0.5), ["shift_max = -0.5"]),
    "speed_min_zero": (lambda s: _set(s, speed_min=0.0), ["speed_min = 0"]),
    "speed_max_below_min": (lambda s: _set(s, speed_max=0.25), ["speed_max = 0.25"]),
    "diffusion_type": (lambda s: _set(s, diffusion_type=2), ["diffusion_type = 2"]),
    "k_step_above_timesteps": (lambda s: _set(s, k_step=1001), ["k_step = 1001"]),
    "discrete_without_table": (lambda s: _set(s, f0_discrete=1), ["lacks", "fs2.pitch_embed.weight"]),
    "inner_fs2_hidden": (lambda s: _inner(s, ".fs2", hidden_size=32), ["fs2.hidden_size = 32", "tables.hidden_size = 64"]),
    "inner_fs2_vocab": (lambda s: _inner(s, ".fs2", vocab_size=13), ["fs2.vocab_size = 13", "tables.vocab_size = 12"]),
    "inner_fs2_flags": (lambda s: _inner(s, ".fs2", embed_flags=1), ["fs2.embed_flags = 1", "tables.embed_flags = 57"]),
    "inner_fs2_spk": (lambda s: _inner(s, ".fs2", num_spk=3), ["fs2.num_spk = 3", "tables.num_spk = 2"]),
    "inner_fs2_lang": (lambda s: _inner(s, ".fs2", num_lang=1), ["fs2.num_lang = 1", "tables.num_lang = 2"]),
    "inner_denoiser_bins": (lambda s: _inner(s, ".denoiser", in_dims=80), ["denoiser.in_dims = 80", "tables.out_dims = 16"]),
    "inner_denoiser_feats": (lambda s: _inner(s, ".denoiser", n_feats=2), ["denoiser.n_feats = 2"]),
    "inner_denoiser_hidden": (lambda s: _inner(s, ".denoiser", hidden_size=128), ["denoiser.hidden_size = 128", "tables.hidden_size = 64"]),
    "inner_aux_bins": (lambda s: _inner(s, ".aux", in_dims=8), ["aux.in_dims = 8", "tables.out_dims = 16"]),
    "inner_aux_feats": (lambda s: _inner(s, ".aux", n_feats=2), ["aux.n_feats = 2"]),
    "inner_aux_hidden": (lambda s: _inner(s, ".aux", hidden_size=32), ["aux.hidden_size = 32", "tables.hidden_size = 64"]),
    "no_tables_section": (_remove_section(".tables"), ['no section "ac.tables"']),
    "no_fs2_section": (_remove_section(".fs2"), ['no section "ac.fs2"']),
    "no_aux_section": (_remove_section(".aux"), ['no section "ac.aux"']),
    "no_denoiser_section": (_remove_section(".denoiser"), ['no section "ac.denoiser"']),
    "tables_of_another_kind": (_tables_of_another_kind, ["ac.tables", "not DSD_ACOUSTIC_TABLES"]),
    "fs2_of_another_kind": (_section_of_another_kind(".fs2"), ["ac.fs2", "not an acoustic encoder"]),
    "aux_of_another_kind": (_section_of_another_kind(".aux"), ["ac.aux", "not an aux decoder"]),
    "denoiser_of_another_kind": (_section_of_another_kind(".denoiser"), ["ac.denoiser", "not a denoiser"]),
}


@pytest.fixture(scope="module")
def _batch_model():
    return cc.build_model("batch", cuda=False)


@pytest.fixture
def batch_model(_batch_model):
    """built once; the hparams its sections are made from are set again for every test"""
    model, hp = _batch_model
    hparams.clear()
    hparams.update(hp, infer=True)
    return model


@pytest.mark.parametrize("name", list(REFUSALS))
def test_open_refuses(tmp_path, batch_model, name):
    edit, words = REFUSALS[name]
    path = tmp_path / "bad.dsdm"
    cc.pack(path, batch_model, edit=edit)
    rc, ap, msg = c_acoustic_open(path)
    assert rc == (ENOTFOUND if name.startswith("no_") else EINVAL), (rc, msg)
    assert ap.value is None                                                 # *out = NULL
    assert msg.startswith("dsd_acoustic_open:") and all(w in msg for w in words), msg


def test_open_refuses_what_the_other_flags_exclude(tmp_path):
    """on the plain model: the frozen tensors need their embedding, and a model without shallow diffusion needs no aux section"""
    model, _ = cc.build_model("plain_ddpm", cuda=False)
    for edit, words in ((_put("frozen_spk_embed", (64,)), ["excludes", "frozen_spk_embed"]),
                        (_put("frozen_key_shift", (1,)), ["excludes", "frozen_key_shift"]),
                        (lambda s: _set(s, use_shallow_diffusion=1), ['no section "ac.aux"']),
                        (lambda s: _set(s, use_spk_id=1), ["use_spk_id = 1 with num_spk = 0"]),
                        (lambda s: _set(s, num_lang=2), ["use_lang_id = 0 with num_lang = 2"]),
                        (lambda s: _set(s, max_beta=1.5), ["max_beta = 1.5"]),
                        (lambda s: _set(s, schedule_type=2), ["schedule_type = 2"])):
        path = tmp_path / "bad.dsdm"
        cc.pack(path, model, edit=edit)
        rc, ap, msg = c_acoustic_open(path)
        assert rc < 0 and ap.value is None and all(w in msg for w in words), msg


def test_frozen_tensors_are_packed_and_accepted(tmp_path):
    model, _ = cc.build_model("frozen", cuda=False)
    path = tmp_path / "f.dsdm"
    sections = cc.pack(path, model)
    t = sections[0].tensors
    assert t["frozen_spk_embed"].shape == (dc.HIDDEN,) and t["frozen_key_shift"].tolist() == [2.75]
    assert t["frozen_spk_embed"].tobytes() == model.frozen_spk_embed.numpy().tobytes()
    rc, ap, msg = c_acoustic_open(path)
    if torch.cuda.is_available():
        assert rc == 0, msg
        _lib.lib().dsd_acoustic_close(ap)
    else:
        assert "no HIP device" in msg, msg                                  # every host check passed


def test_einval_without_an_object(tmp_path, batch_model):
    lib = _lib.lib()
    path = tmp_path / "ok.dsdm"
    cc.pack(path, batch_model)
    out = C.c_void_p(1)
    with modelfile.open(path) as f:
        for args in ((None, b"ac", 0, C.byref(out)), (f._f, None, 0, C.byref(out)), (f._f, b"ac", 0, None)):
            assert lib.dsd_acoustic_open(*args) == EINVAL and b"NULL argument" in lib.dsd_last_error(None)
        assert out.value is None
        assert lib.dsd_acoustic_open(f._f, b"x" * 250, 0, C.byref(out)) == EINVAL and b"prefix" in lib.dsd_last_error(None)
        assert lib.dsd_acoustic_open(f._f, b"other", 0, C.byref(out)) == ENOTFOUND
        assert b'no section "other.tables"' in lib.dsd_last_error(None)
    lib.dsd_acoustic_close(None)
    ptr = C.cast((C.c_float * 64)(), C.c_void_p)
    cfg, p = _lib.DsdAcousticConfig(), _lib.DsdAcousticPlan()
    assert lib.dsd_acoustic_info(None, C.byref(cfg)) == EINVAL and b"dsd_acoustic_info" in lib.dsd_last_error(None)
    assert lib.dsd_acoustic_handle(None, 0, C.byref(out)) == EINVAL and b"dsd_acoustic_handle" in lib.dsd_last_error(None)
    a = _lib.DsdAcousticConditionArgs()
    a.struct_size = C.sizeof(a)
    assert lib.dsd_acoustic_condition(None, C.byref(a), None) == EINVAL
    assert lib.dsd_last_error(None) == b"dsd_acoustic_condition: NULL object"
    assert lib.dsd_acoustic_start(None, C.byref(p), ptr, ptr, 1, 4, ptr, None) == EINVAL
    assert lib.dsd_last_error(None) == b"dsd_acoustic_start: NULL object"
    assert lib.dsd_acoustic_sample(None, C.byref(p), ptr, ptr, None, 1, 4, 0, ptr, None) == EINVAL
    assert lib.dsd_last_error(None) == b"dsd_acoustic_sample: NULL object"


def test_model_create_refuses_the_tables_kind(tmp_path, batch_model):
    lib = _lib.lib()
    path = tmp_path / "ok.dsdm"
    cc.pack(path, batch_model)
    with modelfile.open(path) as f:
        h = C.c_void_p(1)
        assert lib.dsd_model_create(f._f, f.index("ac.tables"), 0, C.byref(h)) == EINVAL and h.value is None
        msg = lib.dsd_last_error(None).decode()
        assert "dsd_model_create" in msg and "ac.tables" in msg and "use dsd_acoustic_open" in msg


# ------------------------------------------------------------------------------------------------ dsd_acoustic_plan
@pytest.mark.parametrize("k_step", [400, 1000])
def test_ddpm_plan_is_the_python_twins(k_step):
    """steps 1 .. 60 x the depths, against schedule.onnx_ddpm_plan (integers equal) and GaussianDiffusion._start_state's rule
    with the wrapper's own fp32 buffers (coefficients bit for bit)."""
    model, _ = cc.build_model("aux_ddpm", cuda=False)
    diff = model.diffusion
    cfg = modelfile.acoustic_config(model)
    assert (cfg.timesteps, cfg.k_step) == (1000, 400)
    cfg.k_step = k_step
    sa, s1 = diff.sqrt_alphas_cumprod.numpy(), diff.sqrt_one_minus_alphas_cumprod.numpy()
    seen = set()
    for steps in range(1, 61):
        for depth in DEPTHS:
            rc, p, msg = c_plan(cfg, depth, steps)
            assert rc == 0, (steps, depth, msg)
            t_max, speedup = schedule.onnx_ddpm_plan(1000, k_step, diff.timestep_factors, steps, depth)
            assert (p.mode, p.steps, p.t_max, p.speedup) == (0, steps, t_max, speedup), (steps, depth)
            assert p.n_step_noise == (t_max if speedup == 1 else 0), (steps, depth)        # _run_loop: ancestral at speed-up 1
            if depth is None or t_max >= 1000:          # forward_onnx: x = noise without a source; _start_state: t_max >= timesteps
                want = (_lib.DSD_AC_START_NOISE, bits(0.0), bits(1.0))
            elif t_max > 0:
                want = (_lib.DSD_AC_START_MIX, bits(sa[t_max - 1]), bits(s1[t_max - 1]))
            else:
                want = (_lib.DSD_AC_START_SOURCE, bits(1.0), bits(0.0))
            assert (p.start, bits(p.src_scale), bits(p.noise_scale)) == want, (steps, depth)
            seen.add((p.start, p.n_step_noise > 0))
    # the grid meets every start and both samplers
    assert {s for s, _ in seen} == {0, 1, 2} and {a for _, a in seen} == {False, True}


def test_reflow_plan_is_the_python_twins():
    """against RectifiedFlow.forward_onnx's rule - max(fp32(1 - depth), fp32(T_start)) and its three branches - for
    T_start = 0.4 (the cases') and 0 (where a depth of 1 lands on NOISE)."""
    model, _ = cc.build_model("aux_reflow", cuda=False)
    cfg = modelfile.acoustic_config(model)
    assert bits(cfg.t_start) == bits(0.4)
    seen = set()
    for t0 in (0.4, 0.0, 1.0):
        cfg.t_start = t0
        for steps in (0, 1, 3, 60):
            for depth in DEPTHS + (0.5, 0.6, 0.75, 2.0):
                rc, p, msg = c_plan(cfg, depth, steps)
                assert rc == 0, (t0, steps, depth, msg)
                if depth is None:
                    ts = 0.0
                else:
                    ts = float(torch.maximum(1 - torch.as_tensor(depth, dtype=torch.float32), torch.tensor(t0, dtype=torch.float32)))
                assert (p.mode, p.steps, p.t_max, p.speedup, p.n_step_noise) == (1, steps, 0, 0, 0)
                assert bits(p.t_start) == bits(ts), (t0, depth)
                if ts <= 0.0:
                    want = (_lib.DSD_AC_START_NOISE, bits(0.0), bits(1.0))
                elif ts >= 1.0:
                    want = (_lib.DSD_AC_START_SOURCE, bits(1.0), bits(0.0))
                else:                                   # ts * xe + (1 - ts) * noise with ts a Python float
                    want = (_lib.DSD_AC_START_MIX, bits(ts), bits(1 - ts))
                assert (p.start, bits(p.src_scale), bits(p.noise_scale)) == want, (t0, depth)
                seen.add(p.start)
    assert seen == {0, 1, 2}


def test_plan_refusals():
    model, _ = cc.build_model("aux_ddpm", cuda=False)
    cfg = modelfile.acoustic_config(model)
    lib = _lib.lib()
    p = _lib.DsdAcousticPlan()
    assert lib.dsd_acoustic_plan(None, 0.3, 4, C.byref(p)) == EINVAL and b"NULL argument" in lib.dsd_last_error(None)
    assert lib.dsd_acoustic_plan(C.byref(cfg), 0.3, 4, None) == EINVAL and b"NULL argument" in lib.dsd_last_error(None)
    for depth, steps, word in ((0.3, 0, "steps = 0"), (None, -1, "steps = -1"), (float("nan"), 4, "depth is NaN")):
        rc, _, msg = c_plan(cfg, depth, steps)
        assert rc == EINVAL and msg.startswith("dsd_acoustic_plan:") and word in msg, msg
    for field, value, word in (("struct_size", 92, "struct_size 92"), ("diffusion_type", 3, "diffusion_type = 3"),
                               ("timesteps", 0, "timesteps = 0"), ("k_step", -1, "k_step = -1"), ("k_step", 1001, "k_step = 1001")):
        bad = _lib.DsdAcousticConfig.from_buffer_copy(cfg)
        setattr(bad, field, value)
        rc, _, msg = c_plan(bad, 0.3, 4)
        assert rc == EINVAL and word in msg, msg
    bad = _lib.DsdAcousticConfig.from_buffer_copy(cfg)
    bad.schedule_type = 9                                # dsd_ddpm_tables_fill's refusal, where the plan reads the tables
    rc, _, msg = c_plan(bad, 0.3, 4)
    assert rc == EINVAL and "schedule" in msg, msg
    model, _ = cc.build_model("aux_reflow", cuda=False)
    cfg = modelfile.acoustic_config(model)
    rc, _, msg = c_plan(cfg, float("nan"), 4)
    assert rc == EINVAL and "depth is NaN" in msg
    assert c_plan(cfg, 0.5, 0)[0] == 0 and c_plan(cfg, None, -2)[0] == 0        # reflow: an empty loop, as the twin's


def test_acoustic_config_refuses_a_schedule_of_the_checkpoints_own():
    model, _ = cc.build_model("plain_ddpm", cuda=False)
    model.diffusion.sqrt_alphas_cumprod[10] += 1e-3
    with pytest.raises(ValueError, match="sqrt_alphas_cumprod"):
        modelfile.acoustic_config(model)


def test_pack_model_writes_the_twin_sections(tmp_path):
    """examples/pack_model.py --twin's half on a synthetic experiment directory: the sections dsd_acoustic_open looks for,
    the checkpoint's own weights in them, and a file the C reader and the host checks accept."""
    import importlib.util
    import yaml
    exp = tmp_path / "exp"
    exp.mkdir()
    hp, _ = cc.case_hparams("aux_reflow")
    hp = dict(hp, audio_num_mel_bins=dc.M_BINS, work_dir=str(exp))
    (exp / "config.yaml").write_text(yaml.safe_dump(hp))
    (exp / "dictionary.txt").write_text("ab\ta b\ncd\tc d\ne\te\n", encoding="utf8")
    hparams.clear()
    hparams.update(hp, infer=True)
    from diffsinger_amd.toplevel import DiffSingerAcoustic
    model = DiffSingerAcoustic(8, dc.M_BINS)
    sd = dict(model.state_dict())
    sd.update({k: torch.from_numpy(v) for k, v in dc.synth_weights(dc.sorted_param_shapes(model.named_parameters()), 91).items()})
    torch.save({"state_dict": {"model." + k: v for k, v in sd.items()}, "category": "acoustic"}, exp / "model_ckpt_steps_5.ckpt")
    spec = importlib.util.spec_from_file_location("pack_model", os.path.join(ROOT, "examples", "pack_model.py"))
    pack_model = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pack_model)
    sections = pack_model.twin_sections(exp, "singer", None)
    assert [s.name for s in sections] == ["singer.tables", "singer.fs2", "singer.aux", "singer.denoiser"]
    assert sections[0].kind == 11 and sections[0].cfg.out_dims == dc.M_BINS and sections[0].cfg.use_shallow_diffusion == 1
    assert sections[1].tensors["txt_embed.weight"].tobytes() == sd["fs2.txt_embed.weight"].numpy().tobytes()
    assert not sections[0].tensors["cross_lingual_mask"].any()             # one language: nothing is cross-lingual
    path = tmp_path / "voice.dsdm"
    modelfile.write(path, sections)
    rc, ap, msg = c_acoustic_open(path, "singer")
    if torch.cuda.is_available():
        assert rc == 0, msg
        _lib.lib().dsd_acoustic_close(ap)
    else:
        assert "no HIP device" in msg, msg


def test_validation_and_plan_under_sanitizers(tmp_path):
    """tools/harness/acoustic_harness.cpp: the section validation, the inner-config check and dsd_acoustic_plan over a grid of
    (depth, steps) for both diffusion types, compiled with the host compiler's address and undefined-behaviour sanitizers
    into a stand-alone program, on heap buffers of exact size."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = tmp_path / "acoustic_harness"
    # the sanitizer runtimes are linked into the program itself (g++ links them dynamically unless told otherwise; clang
    # links them statically and does not know -static-libubsan)
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) == "g++" else []
    csrc = os.path.join(ROOT, "diffsinger_amd", "csrc")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static,
           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "harness", "acoustic_harness.cpp"), "-x", "c++",
           os.path.join(csrc, "acoustic_tables.hip"), os.path.join(csrc, "program_api.hip"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert built.returncode == 0, built.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    assert "0 failed" in run.stdout, run.stdout
