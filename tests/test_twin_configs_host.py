"""No GPU: the cases of tests/twin_config_cases.py as far as a host can take them.  Every case builds its Python twin, packs
with modelfile.acoustic_sections / variance_sections, round-trips bit for bit through the C reader, passes every host check of
dsd_acoustic_open / dsd_variance_open (what stops the open on a machine without a GPU is the device, as in
test_cacoustic_host.py and test_cvariance_host.py) and the create-time validation of every inner section; the packed config
carries what the case set; G31 holds every key the case needs, at the shapes it implies, with a floor for each, and its
parameter lists are the Python twin's; what the library refuses is refused with its message; and, where the reference tree is
at hand (DIFFSINGER_REFERENCE), the generator reproduces the stored arrays."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import deploy_cases as dc
import twin_config_cases as tc
from diffsinger_amd import _lib, modelfile
from diffsinger_amd.hparams import hparams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g31_twin_configs.npz")
AC, VAR = "ac", "var"


@pytest.fixture(autouse=True)
def _restore_hparams():
    yield
    hparams.clear()
    hparams.update(hidden_size=256)


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


def packed(kind, tag, directory, over=None):
    """-> (model, hp, sections, path of the file written)"""
    if kind == AC:
        model, hp = tc.build_acoustic(tag, cuda=False)
        sections = modelfile.acoustic_sections(AC, model)
    else:
        model, hp = tc.build_variance(tag, cuda=False, over=over)
        sections = modelfile.variance_sections(VAR, model)
    path = os.path.join(str(directory), f"{tag}.dsdm")
    modelfile.write(path, sections, {"kind": "acoustic" if kind == AC else "variance"})
    return model, hp, sections, path


def check_round_trip_and_open(kind, sections, path):
    lib = _lib.lib()
    with modelfile.open(path) as f:
        assert [(s.name, s.kind) for s in f.sections] == [(s.name, s.kind) for s in sections]
        for i, s in enumerate(sections):
            assert bytes(f.config(i)) == bytes(s.cfg), s.name
            got = f.tensors(i)
            assert list(got) == list(s.tensors), s.name
            for k, v in s.tensors.items():
                want = modelfile._as_f32(v)
                assert got[k].shape == want.shape and got[k].tobytes() == want.tobytes(), (s.name, k)
        out = C.c_void_p(1)
        entry = lib.dsd_acoustic_open if kind == AC else lib.dsd_variance_open
        rc = entry(f._f, kind.encode(), 0, C.byref(out))
        msg = lib.dsd_last_error(None).decode("utf-8", "replace")
        if torch.cuda.is_available():
            assert rc == 0 and out.value, msg
            (lib.dsd_acoustic_close if kind == AC else lib.dsd_variance_close)(out)
            return
        # every host check passed: the tables' own, the inner sections' kinds, acoustic_inner_check / variance_inner_check
        assert rc < 0 and out.value is None and "no HIP device" in msg, msg
        for s in sections[1:]:          # and every inner config passes its create-time validation, which comes before the device
            with pytest.raises(_lib.NativeLibraryError, match="no HIP device"):
                f.create(s.name)


# ------------------------------------------------------------------------------------------------ acoustic
@pytest.mark.parametrize("tag", list(tc.AC_CASES))
def test_acoustic_case_packs_opens_and_carries_its_config(tmp_path, tag):
    c = tc.AC_CASES[tag]
    model, hp, sections, path = packed(AC, tag, tmp_path)
    shallow = bool(hp["use_shallow_diffusion"])
    assert [s.name for s in sections] == [AC + s for s in [".tables", ".fs2"] + [".aux"] * shallow + [".denoiser"]]
    check_round_trip_and_open(AC, sections, path)
    cfg, tables = sections[0].cfg, sections[0].tensors
    assert sections[-1].kind == _lib.BACKBONE_IDS[hp["backbone_type"]]
    den = sections[-1].cfg
    assert (den.hidden_size, den.in_dims, den.n_feats) == (hp["hidden_size"], c["m_bins"], 1)
    assert den.num_channels == hp["backbone_args"]["num_channels"] and den.num_layers == 2
    assert (cfg.hidden_size, cfg.vocab_size, cfg.out_dims) == (hp["hidden_size"], tc.VOCAB, c["m_bins"])
    # embed_flags, bit for bit against _lib.EMBED_FLAGS (the variance curves) and the two bits behind them
    flags = sum(_lib.EMBED_FLAGS[n] for n in tc.CURVES if hp[f"use_{n}_embed"])
    flags |= 16 * bool(hp["use_key_shift_embed"]) | 32 * bool(hp["use_speed_embed"])
    assert cfg.embed_flags == flags == sections[1].cfg.embed_flags
    assert [_lib.EMBED_FLAGS[n] for n in tc.CURVES] == [1, 2, 4, 8]
    if tag.startswith("alone_"):
        assert cfg.embed_flags == 1 << tc.EMBEDS.index(tag[6:])
    assert (cfg.use_spk_id, cfg.num_spk) == (int(hp["use_spk_id"]), hp["num_spk"] if hp["use_spk_id"] else 0)
    assert (cfg.use_lang_id, cfg.num_lang) == (int(hp["use_lang_id"]), hp["num_lang"] if hp["use_lang_id"] else 0)
    assert cfg.f0_discrete == int(hp.get("f0_embed_type") == "discrete") and cfg.use_shallow_diffusion == int(shallow)
    if hp["diffusion_type"] == "ddpm":
        assert (cfg.diffusion_type, cfg.timesteps, cfg.k_step) == (_lib.DSD_DIFFUSE_DDPM, 1000, hp["K_step"])
        assert cfg.schedule_type == _lib.SCHEDULE_IDS[hp["schedule_type"]] == _lib.SCHEDULE_IDS["cosine"] != _lib.SCHEDULE_IDS["linear"]
    else:
        assert cfg.diffusion_type == _lib.DSD_DIFFUSE_REFLOW and cfg.time_scale_factor == 1000.0
        assert np.float32(cfg.t_start) == np.float32(0.4 if shallow else 0.0)
    assert tables["spec_min"].shape == tables["spec_max"].shape == (c["m_bins"],)
    assert tables["spec_min"].tobytes() == np.float32(hp["spec_min"]).tobytes() and tables["spec_max"].tobytes() == np.float32(hp["spec_max"]).tobytes()
    assert sorted(np.nonzero(tables["cross_lingual_mask"])[0].tolist()) == sorted(c.get("cross") or [])


def test_the_ddpm_plan_reads_the_cosine_tables():
    """dsd_acoustic_plan (host only) on lynx_ddpm_cosine's config: t_max and speed-up are schedule.onnx_ddpm_plan's, the mix
    coefficients the Python twin's cosine buffers bit for bit - and not the linear schedule's; the stages meet NOISE, MIX and SOURCE."""
    from diffsinger_amd import cacoustic, cprogram, schedule
    tag = "lynx_ddpm_cosine"
    model, hp = tc.build_acoustic(tag, cuda=False)
    cfg, diff = modelfile.acoustic_config(model), model.diffusion
    sa, s1 = diff.sqrt_alphas_cumprod.numpy(), diff.sqrt_one_minus_alphas_cumprod.numpy()
    linear = cprogram.tables("linear", 1000, cfg.max_beta)
    starts = []
    for _, depth, steps in tc.AC_CASES[tag]["stages"]:
        p = cacoustic.plan(cfg, depth, steps)
        t_max, speedup = schedule.onnx_ddpm_plan(1000, hp["K_step"], diff.timestep_factors, steps, depth)
        assert (p.t_max, p.speedup, p.n_step_noise) == (t_max, speedup, t_max if speedup == 1 else 0)
        if p.start == _lib.DSD_AC_START_MIX:
            got = np.float32([p.src_scale, p.noise_scale])
            assert got.tobytes() == np.float32([sa[t_max - 1], s1[t_max - 1]]).tobytes(), (depth, steps)
            assert got[0] != linear.sqrt_alphas_cumprod[t_max - 1]
        starts.append(p.start)
    assert starts == [_lib.DSD_AC_START_MIX, _lib.DSD_AC_START_MIX, _lib.DSD_AC_START_SOURCE, _lib.DSD_AC_START_NOISE]


# ------------------------------------------------------------------------------------------------ variance
@pytest.mark.parametrize("tag", list(tc.VAR_CASES))
def test_variance_case_packs_opens_and_carries_its_config(tmp_path, tag):
    model, hp, sections, path = packed(VAR, tag, tmp_path)
    names = dc.variance_names(hp)
    want = [".tables", ".fs2"] + [".melody"] * bool(hp["use_melody_encoder"] and hp["predict_pitch"]) + [".pitch"] * bool(hp["predict_pitch"]) + \
        [".variances"] * bool(names)
    assert [s.name for s in sections] == [VAR + s for s in want]
    check_round_trip_and_open(VAR, sections, path)
    cfg = sections[0].cfg
    assert (cfg.hidden_size, cfg.vocab_size, cfg.predict_dur, cfg.predict_pitch) == (hp["hidden_size"], tc.VOCAB, int(hp["predict_dur"]), int(hp["predict_pitch"]))
    assert cfg.variances == sum(_lib.EMBED_FLAGS[n] for n in names)
    if hp["predict_dur"]:
        fs2, d = sections[1].cfg, hp["dur_prediction_args"]
        assert (fs2.dur_layers, fs2.dur_chans, fs2.dur_kernel_size) == (d["num_layers"], d["hidden_size"], d["kernel_size"])
        assert (fs2.hidden_size, fs2.ffn_kernel_size) == (hp["hidden_size"], hp["enc_ffn_kernel_size"])
    if hp["predict_pitch"]:
        ph = hp["pitch_prediction_args"]
        assert (cfg.pitch_repeat_bins, cfg.use_melody_encoder, cfg.melody_hidden_size) == (ph["repeat_bins"], 1, hp["melody_encoder_args"]["hidden_size"])
        assert (cfg.pitd_norm_min, cfg.pitd_norm_max, cfg.pitd_clip_min, cfg.pitd_clip_max) == (-8.0, 8.0, -12.0, 12.0)
        i = [s.name for s in sections].index(VAR + ".pitch")
        assert sections[i].kind == _lib.BACKBONE_IDS["lynxnet"] and sections[i].cfg.hidden_size == hp["hidden_size"]
        assert (sections[i].cfg.in_dims, sections[i].cfg.n_feats) == (ph["repeat_bins"], 1)
    if names:
        va = hp["variances_prediction_args"]
        assert cfg.var_repeat_bins == va["total_repeat_bins"] // len(names)
        den = sections[-1].cfg
        assert (den.in_dims, den.n_feats, den.hidden_size) == (cfg.var_repeat_bins, len(names), hp["hidden_size"])
        assert sections[-1].kind == _lib.BACKBONE_IDS[va["backbone_type"]]
        # every curve's range and clamp sits in the slot of its DSD_EMBED_* bit; the other slots stay zero
        for slot, n in enumerate(tc.CURVES):
            key = ("tension_logit", "tension_logit") if n == "tension" else (n + "_db", n + "_db")
            if n in names:
                lo, hi = hp[key[0] + "_min"], hp[key[1] + "_max"]
                assert (cfg.var_norm_min[slot], cfg.var_norm_max[slot]) == (lo, hi), n
                assert (cfg.var_no_clamp[slot], cfg.var_clamp_min[slot], cfg.var_clamp_max[slot]) == (0, lo, hi if n == "tension" else 0.0), n
            else:
                assert (cfg.var_norm_min[slot], cfg.var_norm_max[slot], cfg.var_clamp_min[slot], cfg.var_clamp_max[slot]) == (0.0, 0.0, 0.0, 0.0), n
    assert cfg.diffusion_type == (_lib.DSD_DIFFUSE_REFLOW if hp["diffusion_type"] == "reflow" else _lib.DSD_DIFFUSE_DDPM)


def test_the_curves_of_the_cases_have_ranges_of_their_own():
    """a swapped slot must show: no two of the four curves share a range and a clamp in the cases' hparams"""
    hp = tc.variance_hparams("four_curves")
    assert hp["voicing_db_max"] == tc.variance_hparams("two_late")["voicing_db_max"] != hp["energy_db_max"]
    ranges = {(hp["energy_db_min"], hp["energy_db_max"]), (hp["breathiness_db_min"], hp["breathiness_db_max"]),
              (hp["voicing_db_min"], hp["voicing_db_max"]), (hp["tension_logit_min"], hp["tension_logit_max"])}
    assert len(ranges) == 4


# ------------------------------------------------------------------------------------------------ the fixture
def _fixture_matches(g, tag, keys, model):
    for k, shape in keys.items():
        assert k in g.files and g[k].shape == shape, (k, shape, g[k].shape if k in g.files else None)
        if g[k].dtype == np.float32:
            assert np.isfinite(g[k]).all(), k
            floor = float(g[k + "_floor"][0])
            assert tc.FLOORS[k] == float(f"{floor:.3g}"), (k, floor, tc.FLOORS[k])     # the table states what the generator printed
            tol, unit, _ = tc.bound_for(tag, k)
            name, stated, _ = tc.BOUNDS[tc.quantity_of(k, tag)]
            assert tol == (stated if floor <= stated / 2 else 2 * tc.FLOORS[k]), (k, tol, name)
    shapes = dc.sorted_param_shapes(model.named_parameters())
    assert [f"{n}:{'x'.join(map(str, sh))}" for n, sh in shapes.items()] == [str(s) for s in g[f"{tag}_params"]]


@pytest.mark.parametrize("tag", list(tc.AC_CASES))
def test_fixture_holds_the_acoustic_case(g, tag):
    model, _ = tc.build_acoustic(tag, cuda=False)
    _fixture_matches(g, tag, tc.acoustic_keys(tag), model)


@pytest.mark.parametrize("tag", list(tc.VAR_CASES))
def test_fixture_holds_the_variance_case(g, tag):
    model, _ = tc.build_variance(tag, cuda=False)
    _fixture_matches(g, tag, tc.variance_keys(tag), model)


def test_fixture_holds_nothing_else_and_no_two_alone_cases_share_a_condition(g):
    want = set()
    for tag in tc.AC_CASES:
        want |= set(tc.acoustic_keys(tag)) | {tag + "_params"}
    for tag in tc.VAR_CASES:
        want |= set(tc.variance_keys(tag)) | {tag + "_params"}
    floors = {k for k in g.files if k.endswith("_floor")}
    assert set(g.files) - floors == want | {"oracle_pairs_cond"} and {k[:-6] for k in floors} == set(tc.FLOORS)
    # the cross-check of the float64 evaluation behind the floors: the numpy oracle in float64 gives the same figure for the one
    # quantity it can compute, on the same side of half the bound
    by_oracle, mine = float(g["oracle_pairs_cond"][0]), float(g["pairs_cond_floor"][0])
    assert by_oracle <= tc.BOUNDS["cond"][1] / 2 and mine / 2 <= by_oracle <= 2 * mine, (by_oracle, mine)
    assert os.path.getsize(GOLDEN) < 1 << 20
    alone = [t for t in tc.AC_CASES if t.startswith("alone_")]
    assert [t[6:] for t in alone] == list(tc.EMBEDS)
    for i, a in enumerate(alone):          # own seeds, own inputs: no case could pass with another's table
        for b in alone[i + 1:]:
            assert g[a + "_cond"].shape != g[b + "_cond"].shape or not np.array_equal(g[a + "_cond"], g[b + "_cond"])
            assert tc.AC_CASES[a]["seed"] != tc.AC_CASES[b]["seed"]


def test_bounds_are_the_projects_own():
    """BOUNDS restates tests/test_gpu_deploy.py's constants so that the generator can read them without a GPU module"""
    import test_gpu_deploy as d
    stated = {name: tol for name, tol, _ in tc.BOUNDS.values()}
    assert stated == {n: getattr(d, n) for n in ("ACOUSTIC_COND_TOL", "AUX_TOL", "SAMPLE_TOL", "ENC_TOL", "DUR_TOL", "SMOOTH_BAR")}
    # and the unit each is applied in there: `close(..., floor_one)` / rel_err / an absolute bar
    assert {q: u for q, (_, _, u) in tc.BOUNDS.items()} == dict(
        cond="rel", aux="rel", enc="rel", pitch_cond="rel", var_cond="rel", mel="one", dur_pred="one", x_pred="one", pitch_pred="one",
        xs_pred="one", out="one", base_pitch="abs")


def test_the_inputs_meet_what_the_cases_are_there_for():
    """properties of the seeded inputs the cases rest on"""
    inp, c = tc.acoustic_inputs("all_h96"), tc.AC_CASES["all_h96"]
    real = inp["tokens"][0][inp["tokens"][0] > 0]
    masked = np.isin(real, c["cross"])
    assert masked.any() and not masked.all(), real                          # the cross-lingual list masks some tokens, not all
    assert inp["spk_embed"].shape == (1, c["t_len"], 96)                    # a per-frame speaker embedding
    for tag in ("lynx_ragged", "lynx_ragged_var"):
        batch = tc.acoustic_batch_inputs(tag) if tag in tc.AC_CASES else tc.variance_batch_inputs(tag)
        dur = batch["durations"] * (batch["tokens"] > 0) if "durations" in batch else batch["ph_dur"]
        assert dur.sum(1).tolist() == batch["lengths"].tolist() == (tc.AC_CASES if tag in tc.AC_CASES else tc.VAR_CASES)[tag]["lengths"]
    for tag, c in tc.AC_CASES.items():
        assert c["t_len"] == (41 if tag == "wn_h32_m5" else 70) and 5 <= c["n_ph"] <= 9, tag


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("what,tag,over,section,fragment", tc.REFUSED, ids=[r[0] for r in tc.REFUSED])
def test_refused_configurations_are_refused_with_their_message(tmp_path, what, tag, over, section, fragment):
    """The Python twin builds and packs; the host checks of dsd_variance_open pass (they compare the sections with each other);
    the section's own create-time validation, which dsd_variance_open reaches through dsd_model_create, refuses."""
    _, _, sections, path = packed(VAR, tag, tmp_path, over=over)
    with modelfile.open(path) as f:
        with pytest.raises(_lib.NativeLibraryError) as e:
            f.create(VAR + section)
        assert fragment in str(e.value) and "(-1)" in str(e.value), str(e.value)
        if torch.cuda.is_available():
            out = C.c_void_p(1)
            assert _lib.lib().dsd_variance_open(f._f, VAR.encode(), 0, C.byref(out)) == -1 and out.value is None
            assert fragment in _lib.lib().dsd_last_error(None).decode()


# ------------------------------------------------------------------------------------------------ the generator
def reference_root():
    """DIFFSINGER_REFERENCE, or the checkout an importable reference package lives in -> path or None"""
    import importlib.util
    ref = os.environ.get("DIFFSINGER_REFERENCE", "")
    if not ref:
        try:
            spec = importlib.util.find_spec("deployment.modules.toplevel")
        except (ImportError, ValueError):
            spec = None
        if spec is not None and spec.origin:
            ref = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(spec.origin))))
    return ref if ref and os.path.isdir(os.path.join(ref, "deployment", "modules")) else None


def test_generator_reproduces_the_fixture():
    ref = reference_root()
    if ref is None:
        pytest.skip("the reference tree is not at hand (neither DIFFSINGER_REFERENCE nor an importable `deployment` package)")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_golden_twin_configs.py"), ref, "--check"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "arrays reproduce the stored ones" in r.stdout and "not:" not in r.stdout
