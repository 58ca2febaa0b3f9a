"""-m gpu: the acoustic model's staged twin driven through the C calls (dsd_acoustic_open .. dsd_acoustic_sample, by way
of diffsinger_amd/cacoustic.py) on a model file, against

  * G22 (tests/golden/g22_deploy.npz, the reference's own deployment twins) on the acoustic cases of tests/deploy_cases.py,
    with the tolerances tests/test_gpu_deploy.py applies to the same quantities;
  * `deploy.DiffSingerAcousticDeploy`, the Python twin, with the same weights: the condition stage and the start state run
    the same arithmetic on the same operands and must be bit-identical; the sampler stage is bit-identical where the
    library's program builder gives schedule.py's program, and within ALONE_TOL otherwise.

Every figure is printed before it is asserted."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import cacoustic_cases as cc
import deploy_cases as dc
from diffsinger_amd import _lib, cprogram, modelfile, schedule, synth
from diffsinger_amd import noise as seeded
from diffsinger_amd.hparams import hparams
from gpu_util import dev, rel_err
from test_gpu_deploy import ACOUSTIC_COND_TOL, ALONE_TOL, AUX_TOL, GOLDEN, SAMPLE_TOL, close, release

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


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

    def __init__(self, tag, directory, extra=()):
        from diffsinger_amd.cacoustic import Acoustic
        self.model, self.hp = cc.build_model(tag, cuda=True)
        self.path = os.path.join(str(directory), tag + ".dsdm")
        sections = modelfile.acoustic_sections(cc.PREFIX, self.model) + list(extra)
        modelfile.write(self.path, sections, {"kind": "acoustic"})
        with modelfile.open(self.path) as f:
            self.a = Acoustic(f, cc.PREFIX, "cuda")         # the object keeps nothing of the file

    def close(self):
        self.a.close()
        release(self.model)


@pytest.fixture
def world(tmp_path):
    made = []

    def make(tag, extra=()):
        made.append(World(tag, tmp_path, extra))
        return made[-1]
    yield make
    for w in made:
        w.close()


def same(got, want, what):
    """bit-identical"""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    a, b = got.contiguous().view(-1), want.contiguous().view(-1)
    differ = int((a.view(torch.int32) != b.view(torch.int32)).sum()) if a.dtype == torch.float32 else int((a != b).sum())
    worst = float((a.double() - b.double()).abs().nan_to_num(0).max()) if a.numel() else 0.0
    print(f"{what}: {differ} of {a.numel()} elements differ from the reference's (max |diff| {worst:.3e})")
    assert differ == 0, (what, differ, worst)


def twin_condition(model, inp, sl=slice(None), spk="spk_embed", t_len=None):
    cut = (lambda x: x[sl, :t_len]) if t_len else (lambda x: x[sl])
    variances = {k[4:]: cut(v) for k, v in inp.items() if k.startswith("var_")}
    return model.forward_fs2_aux(inp["tokens"][sl], inp["durations"][sl], cut(inp["f0"]), variances,
                                 gender=None if "gender" not in inp else cut(inp["gender"]),
                                 velocity=None if "velocity" not in inp else cut(inp["velocity"]),
                                 spk_embed=None if spk not in inp else (cut(inp[spk]) if inp[spk].shape[1] > 1 else inp[spk][sl]),
                                 languages=None if "languages" not in inp else inp["languages"][sl])


def c_condition(a, inp, sl=slice(None), spk="spk_embed", t_len=None, **kw):
    cut = (lambda x: x[sl, :t_len]) if t_len else (lambda x: x[sl])
    variances = {k[4:]: cut(v) for k, v in inp.items() if k.startswith("var_")}
    return a.condition(inp["tokens"][sl], inp["durations"][sl], cut(inp["f0"]), variances,
                       gender=None if "gender" not in inp else cut(inp["gender"]),
                       velocity=None if "velocity" not in inp else cut(inp["velocity"]),
                       spk_embed=None if spk not in inp else (cut(inp[spk]) if inp[spk].shape[1] > 1 else inp[spk][sl]),
                       languages=None if "languages" not in inp else inp["languages"][sl], **kw)


def twin_start(model, depth, steps, source, noise):
    """the start state of forward_onnx (diffusion.py), restated with the wrapper's own pieces -> (x, (t_max, speedup) or t_start)"""
    from diffsinger_amd.diffusion import _to_bfmt
    d = model.diffusion
    b, device = noise.shape[0], noise.device
    k, mid = (d.spec_max - d.spec_min) / 2., (d.spec_max + d.spec_min) / 2.
    if hasattr(d, "denoise_fn"):
        t_max, speedup = schedule.onnx_ddpm_plan(d.timesteps, d.k_step, d.timestep_factors.cpu(), steps, None if source is None else depth)
        if source is None:
            return noise, (t_max, speedup)
        return d._start_state(t_max, _to_bfmt((source - mid) / k, 1), noise, b, device), (t_max, speedup)
    if source is None:
        return noise, 0.0
    t_start = torch.maximum(1 - torch.as_tensor(depth, dtype=torch.float32).cpu(), torch.tensor(d.t_start, dtype=torch.float32))
    xe = _to_bfmt((source - mid) / k, 1)
    ts = float(t_start)
    if ts <= 0.:
        return noise, ts
    if ts >= 1.:
        return xe, ts
    return ts * xe + (1 - ts) * noise, ts


def twin_programs(model, plan_key, steps):
    """the schedule.py programs diffusion.py runs for a plan, in order"""
    d = model.diffusion
    if hasattr(d, "denoise_fn"):
        t_max, speedup = plan_key
        if speedup > 1 and t_max > 0:
            return [schedule.ddim_program(d._tables, t_max, speedup)]
        out, hi = [], t_max
        while hi > 0:
            lo = max(hi - d._ANCESTRAL_CHUNK, 0)
            out.append(schedule.ddpm_ancestral_program(d._tables, hi, lo))
            hi = lo
        return out
    if plan_key >= 1. or steps < 1:
        return []
    return [schedule.reflow_onnx_program(steps, torch.tensor(plan_key, dtype=torch.float32), d.time_scale_factor)]


def c_programs(a, p):
    """the programs dsd_acoustic_sample builds for a plan (dsd_program_build on the same specs), read back"""
    c = a.cfg
    if p.mode == _lib.DSD_DIFFUSE_REFLOW:
        if p.t_start >= 1. or p.steps < 1:
            return []
        return [cprogram.build(cprogram.spec("rf_euler_onnx", steps=p.steps, t_start=p.t_start, time_scale_factor=c.time_scale_factor))]
    kind = {v: k for k, v in _lib.SCHEDULE_IDS.items()}[c.schedule_type]
    tb = cprogram.tables(kind, c.timesteps, c.max_beta)
    if p.speedup > 1 and p.t_max > 0:
        return [cprogram.build(cprogram.spec("ddim", tb, t_max=p.t_max, speedup=p.speedup))]
    out, hi = [], p.t_max
    while hi > 0:
        lo = max(hi - 50, 0)
        out.append(cprogram.build(cprogram.spec("ddpm", tb, t_max=hi, speedup=1, t_lo=lo)))
        hi = lo
    return out


def run_stage(w, depth, steps, cond, aux, noise, step_noise=None, what="stage"):
    """one sampler stage on both sides -> (C mel, twin mel); x is held bit for bit on the way"""
    model, a = w.model, w.a
    source = None if depth is None else aux
    p = a.plan(depth, steps)
    x = a.start(p, source=source, noise=noise)
    want_x, key = twin_start(model, depth, steps, source, noise)
    same(x, want_x, f"{what}: x (start {p.start})")
    mel = a.sample(p, cond, x, step_noise=step_noise)
    d = model.diffusion
    if hasattr(d, "denoise_fn"):
        kw = dict(noise=noise, step_noise=step_noise)
    else:
        kw = dict(noise=noise)
    if source is None:
        want = model.ensure_mel_base(d.forward_onnx(cond, steps=steps, **kw))
    elif hasattr(d, "denoise_fn"):
        want = model.ensure_mel_base(d.forward_onnx(cond, x_start=source, depth=torch.tensor(depth, dtype=torch.float32), steps=steps, **kw))
    else:
        want = model.ensure_mel_base(d.forward_onnx(cond, x_end=source, depth=torch.tensor(depth, dtype=torch.float32), steps=steps, **kw))
    mine, theirs = [q.key() for q in c_programs(a, p)], [q.key() for q in twin_programs(model, key, steps)]
    close(mel, want.cpu().numpy(), ALONE_TOL, True, f"{what}: mel vs the twin")
    if mine == theirs:
        print(f"{what}: the library's builder gives schedule.py's program ({len(mine)} program(s)): the mel must be bit-identical")
        same(mel, want, f"{what}: mel")
    else:
        print(f"{what}: the library's builder and schedule.py differ in a coefficient's last bit: held to ALONE_TOL only")
    return mel, want, p


# ------------------------------------------------------------------------------------------------ G22 and the twin
@pytest.mark.parametrize("tag", list(dc.AC_CASES))
def test_stages_vs_golden_and_python_twin(g, world, tag):
    w = world(tag)
    model, hp, a, c = w.model, w.hp, w.a, dc.AC_CASES[tag]
    inp = {k: dev(x) for k, x in dc.acoustic_inputs(tag).items()}
    discrete = hp.get("f0_embed_type") == "discrete"
    with torch.no_grad():
        res = c_condition(a, inp, want_coarse=discrete)
        want = twin_condition(model, inp)
        if hp["use_shallow_diffusion"]:
            cond, aux = res[0], res[1]
            err = rel_err(aux, g[f"{tag}_aux"])
            print(f"aux_mel_pred: {err:.3e} of max |want|, bound {AUX_TOL:.1e}")
            assert err < AUX_TOL
            same(aux, want[1], "aux_mel")
            want_cond = want[0]
        else:
            cond, aux, want_cond = (res[0] if discrete else res), None, want
        err = rel_err(cond, g[f"{tag}_cond"])
        print(f"condition: {err:.3e} of max |want|, bound {ACOUSTIC_COND_TOL:.1e}")
        assert err < ACOUSTIC_COND_TOL
        same(cond, want_cond, "condition")
        if discrete:
            from diffsinger_amd.deploy import f0_to_coarse, length_regulate
            mel2ph = length_regulate(inp["durations"] * (inp["tokens"] > 0), inp["f0"].shape[1])
            coarse = f0_to_coarse(inp["f0"] * (mel2ph > 0))
            print(f"f0_coarse: {int((res[1] != coarse).sum())} of {coarse.numel()} frames differ; range {int(coarse.min())} .. {int(coarse.max())}")
            assert torch.equal(res[1], coarse) and int(coarse.max()) > 1
        for i, (stage, depth) in enumerate(c["stages"]):
            noise = dev(synth.synth_normal((1, 1, dc.M_BINS, cond.shape[1]), c["seed"] + 2 + i))
            mel, _, _ = run_stage(w, depth, c["steps"], cond, aux, noise, what=stage)
            close(mel, g[f"{tag}_{stage}"], SAMPLE_TOL, True, stage)


# ------------------------------------------------------------------------------------------------ the start state
@pytest.mark.parametrize("tag,depth,start", [("aux_ddpm", 0.3, 1), ("aux_ddpm", 1.0, 1), ("aux_ddpm", 0.0, 2), ("aux_ddpm", None, 0),
                                             ("aux_reflow", 0.5, 1), ("aux_reflow", 0.9, 1), ("aux_reflow", 0.0, 2), ("aux_reflow", None, 0)])
def test_start_state_is_the_python_twins(world, tag, depth, start):
    """DDPM MIX (q_sample at t_max - 1), reflow MIX, SOURCE and NOISE, bit for bit; and with noise == NULL followed by
    dsd_noise_fill in place, the twin's seeded start under the same seed."""
    from diffsinger_amd.diffusion import _to_bfmt
    w = world(tag)
    model, a, c = w.model, w.a, dc.AC_CASES[tag]
    inp = {k: dev(x) for k, x in dc.acoustic_inputs(tag).items()}
    t_len, steps, seed = inp["f0"].shape[1], 3, 77
    with torch.no_grad():
        cond, aux = c_condition(a, inp)
        noise = dev(synth.synth_normal((1, 1, dc.M_BINS, t_len), c["seed"] + 9))
        p = a.plan(depth, steps)
        assert p.start == start
        source = None if depth is None else aux
        x = a.start(p, source=source, noise=noise)
        want, key = twin_start(model, depth, steps, source, noise)
        same(x, want, f"x (start {start})")
        if start == _lib.DSD_AC_START_MIX:
            d = model.diffusion
            x = a.start(p, source=source, noise=None)
            k, mid = (d.spec_max - d.spec_min) / 2., (d.spec_max + d.spec_min) / 2.
            xs = _to_bfmt((source - mid) / k, 1)
            same(x, xs, "the normalised, transposed source alone")
            flat = x.view(1, 1, dc.M_BINS, t_len)
            seeded.fill((1, 1, dc.M_BINS, t_len), [seed], seeded.X_T, src=flat, src_scale=p.src_scale, scale=p.noise_scale, out=flat)
            if hasattr(d, "denoise_fn"):
                want = d._seeded_start(key[0], xs, [seed], seeded.X_T, 1, t_len, x.device)
            else:
                want = d._seeded_state([seed], seeded.X_T, 1, t_len, x.device, src=xs, src_scale=key, scale=1 - key)
            same(x, want, "x mixed in place with the seeded noise")


# ------------------------------------------------------------------------------------------------ the ancestral sampler
@pytest.mark.parametrize("depth,steps,n", [(0.004, 4, 4), (0.06, 60, 60)])
def test_ancestral_sampling_vs_python_twin(world, depth, steps, n):
    """speed-up 1: p_sample with one noise tensor per step, consumed in order; 60 steps cross one 50-step chunk boundary"""
    w = world("ancestral")
    model, a = w.model, w.a
    inp = {k: dev(x) for k, x in dc.acoustic_inputs("aux_ddpm").items()}
    t_len = inp["f0"].shape[1]
    with torch.no_grad():
        cond, aux = c_condition(a, inp)
        noise = dev(synth.synth_normal((1, 1, dc.M_BINS, t_len), 2531))
        step_noise = dev(synth.synth_normal((n, 1, 1, dc.M_BINS, t_len), 2532))
        mel, want, p = run_stage(w, depth, steps, cond, aux, noise, step_noise=step_noise, what=f"ancestral, {n} steps")
        assert (p.t_max, p.speedup, p.n_step_noise) == (n, 1, n)
        other = a.sample(p, cond, a.start(p, source=aux, noise=noise), step_noise=step_noise.flip(0))
        assert not torch.equal(other, mel)                               # the order of the step noise counts


# ------------------------------------------------------------------------------------------------ the kernels alone
def carrier(directory, m_bins, seed):
    """an object whose tables hold `m_bins` bins with uneven spec_min / spec_max - a reflow model of a log10 mel without an aux
    decoder, its weights as torch initialised them: the kernels under test do not read them -> (twin on the GPU, C object, hp)"""
    from diffsinger_amd.cacoustic import Acoustic
    from diffsinger_amd.deploy import DiffSingerAcousticDeploy
    hp, _ = cc.case_hparams("aux_reflow")
    rng = np.random.Generator(np.random.PCG64(seed))
    hp = dict(hp, spec_min=(-12.0 + 3 * rng.random(m_bins)).round(3).tolist(), spec_max=(0.5 + 2 * rng.random(m_bins)).round(3).tolist(),
              use_shallow_diffusion=False)
    hparams.clear()
    hparams.update(hp, infer=True)
    model = DiffSingerAcousticDeploy(dc.VOCAB, m_bins).eval().cuda()
    path = os.path.join(str(directory), f"m{m_bins}.dsdm")
    modelfile.write(path, modelfile.acoustic_sections(cc.PREFIX, model))
    with modelfile.open(path) as f:
        return model, Acoustic(f, cc.PREFIX, "cuda"), hp


@pytest.mark.parametrize("m_bins", [1, 16, 80, 128])
def test_source_kernel_vs_torch(tmp_path, m_bins):
    """ac_source_kernel through dsd_acoustic_start: B = 2, T over every tile edge (1, 31, 33, 64, 65, 257), with and without
    noise, x apart from source, bit for bit against torch's own (source - mid) / k transposed and
    src_scale * that + noise_scale * noise."""
    model, a, hp = carrier(tmp_path, m_bins, 2600 + m_bins)
    rng = np.random.Generator(np.random.PCG64(2650 + m_bins))
    try:
        lo, hi = dev(np.float32(hp["spec_min"])), dev(np.float32(hp["spec_max"]))
        k, mid = (hi - lo) / 2., (hi + lo) / 2.
        p = _lib.DsdAcousticPlan(mode=1, start=_lib.DSD_AC_START_MIX, t_start=0.625, src_scale=0.625, noise_scale=0.375, steps=2)
        for t_len in (1, 31, 33, 64, 65, 257):
            source = dev((rng.standard_normal((2, t_len, m_bins)) * 4 - 6).astype(np.float32))
            noise = dev(rng.standard_normal((2, 1, m_bins, t_len)).astype(np.float32))
            xs = ((source - mid) / k).transpose(1, 2)[:, None].contiguous()
            x = torch.full((2, 1, m_bins, t_len), float("nan"), device="cuda")
            a.start(p, source=source, noise=noise, out=x)
            same(x, 0.625 * xs + 0.375 * noise, f"M = {m_bins}, T = {t_len}: the mix")
            x.fill_(float("nan"))
            a.start(p, source=source, noise=None, out=x)
            same(x, xs, f"M = {m_bins}, T = {t_len}: the source alone")
            p.start = _lib.DSD_AC_START_SOURCE
            x.fill_(float("nan"))
            a.start(p, source=source, noise=noise, out=x)
            same(x, xs, f"M = {m_bins}, T = {t_len}: SOURCE does not read the noise")
            p.start = _lib.DSD_AC_START_MIX
    finally:
        a.close()
        release(model)


@pytest.mark.parametrize("m_bins,t_len,offset", [(5, 41, 0), (5, 41, 1), (5, 1, 2), (16, 40, 0), (16, 40, 3), (16, 1, 0), (16, 257, 0)])
def test_mel_base_scale_in_place(tmp_path, m_bins, t_len, offset):
    """the sampler stage of a log10 model ends in mel *= fp32(2.30259).  The empty loop (t_start = 1) leaves x * k + mid as the
    library's unpack forms it - the twin's own empty loop gives the same bits - so the stage's output is that times 2.30259:
    at odd counts (M = 5) and counts that are a multiple of 4, into an aligned and an unaligned `mel` pointer (the 16-byte
    path needs both; the others take the scalar one)."""
    from diffsinger_amd.diffusion import _expand_fm
    model, a, hp = carrier(tmp_path, m_bins, 2700 + m_bins)
    try:
        assert a.cfg.mel_base_e == 0
        rng = np.random.Generator(np.random.PCG64(2750 + t_len + offset))
        d = model.diffusion
        k, mid = ((d.spec_max - d.spec_min) / 2.).reshape(-1), ((d.spec_max + d.spec_min) / 2.).reshape(-1)
        x = dev(rng.standard_normal((1, 1, m_bins, t_len)).astype(np.float32))
        cond = dev(rng.standard_normal((1, t_len, dc.HIDDEN)).astype(np.float32))
        p = _lib.DsdAcousticPlan(mode=1, start=_lib.DSD_AC_START_SOURCE, t_start=1.0, src_scale=1.0, noise_scale=0.0, steps=3)
        n = t_len * m_bins
        store = torch.full((n + 8,), float("nan"), device="cuda")
        mel = store[offset:offset + n].view(1, t_len, m_bins)
        assert (mel.data_ptr() % 16 == 0) == (offset == 0)
        with torch.no_grad():
            a.sample(p, cond, x, out=mel)
            entry = d._cached_program(('noop',), lambda: schedule.Program(1, 0, []))
            base = d._run_program(entry, cond.transpose(1, 2), x, scale=_expand_fm(d, k), shift=_expand_fm(d, mid))
        close(base, (x[:, 0].transpose(1, 2) * k + mid).cpu().numpy(), 1e-6, True, "the empty loop is x * k + mid")
        same(mel, base * 2.30259, f"mel * 2.30259 (M = {m_bins}, T = {t_len}, offset {offset}: {'16-byte' if n % 4 == 0 and not offset else 'scalar'} path)")
        assert torch.isnan(store[:offset]).all() and torch.isnan(store[offset + n:]).all()       # nothing beside it was written
    finally:
        a.close()
        release(model)


# ------------------------------------------------------------------------------------------------ a padded batch
@pytest.mark.parametrize("spk", ["spk_one", "spk_frames"])
def test_padded_batch_vs_python_twin_and_items_alone(world, spk):
    """B = 3, T = 70 (tests/cacoustic_cases.py): a padding token with a non-zero duration, items whose durations total less
    than T, spk_embed as [B, 1, H] and per frame, every embedding of the condition stage.  Against the Python twin bit for
    bit; every item's real frames of the condition against its lone run at its own frame count, and its aux mel against its
    lone run at T (the aux decoder's convolutions see the padding frames' condition, which is not zero)."""
    w = world("batch")
    model, a = w.model, w.a
    raw = cc.batch_inputs()
    inp = {k: dev(x) for k, x in raw.items() if k != "lengths"}
    lens = raw["lengths"]
    with torch.no_grad():
        cond, aux = c_condition(a, inp, spk=spk)
        want_cond, want_aux = twin_condition(model, inp, spk=spk)
        same(cond, want_cond, "condition")
        same(aux, want_aux, "aux_mel")
        for b in range(3):
            sl, n = slice(b, b + 1), int(lens[b])
            lone_cond, _ = c_condition(a, inp, sl=sl, spk=spk, t_len=n)
            same(lone_cond, cond[sl, :n], f"item {b} alone at T = {n}: condition")
            full_cond, full_aux = c_condition(a, inp, sl=sl, spk=spk)
            same(full_cond, cond[sl], f"item {b} alone at T: condition")
            same(full_aux[:, :n], aux[sl, :n], f"item {b} alone at T: aux_mel")
        # the masked duration: item 1's padding token takes no frame, and its frames past 41 are padding (mel2ph 0)
        from diffsinger_amd.deploy import length_regulate
        mel2ph = length_regulate(inp["durations"] * (inp["tokens"] > 0), 70)
        assert not (mel2ph[1] == 3).any() and not mel2ph[1, 41:].any() and not mel2ph[2, 57:].any() and mel2ph[0].all()


# ------------------------------------------------------------------------------------------------ frozen tensors
def test_frozen_tensors_take_the_place_of_the_inputs(world):
    w = world("frozen")
    model, a = w.model, w.a
    inp = {k: dev(x) for k, x in dc.acoustic_inputs("gender_velocity").items() if k in ("tokens", "durations", "f0", "velocity")}
    with torch.no_grad():
        cond, aux = a.condition(inp["tokens"], inp["durations"], inp["f0"], velocity=inp["velocity"])
        want_cond, want_aux = model.forward_fs2_aux(inp["tokens"], inp["durations"], inp["f0"], {}, velocity=inp["velocity"])
        same(cond, want_cond, "condition with frozen_spk_embed and frozen_key_shift")
        same(aux, want_aux, "aux_mel")
        # a gender curve and a speaker mix are accepted and not read
        other = a.condition(inp["tokens"], inp["durations"], inp["f0"], velocity=inp["velocity"], gender=torch.full_like(inp["f0"], -0.7),
                            spk_embed=torch.ones((1, 1, dc.HIDDEN), device="cuda"))[0]
        same(other, want_cond, "condition, the caller's gender and spk_embed ignored")
        # and without the attributes the twin differs: the tensors are read
        del model.frozen_key_shift
        changed = model.forward_fs2_aux(inp["tokens"], inp["durations"], inp["f0"], {}, velocity=inp["velocity"],
                                        gender=torch.zeros_like(inp["f0"]))[0]
        assert not torch.equal(changed, want_cond)


# ------------------------------------------------------------------------------------------------ refusals
def test_stage_calls_refuse_before_any_launch(world):
    """every DSD_EINVAL of the three stage calls on two models (every embedding and shallow DDPM; the plain reflow model):
    the outputs keep their NaN fill, so nothing was launched."""
    lib = _lib.lib()
    wb, wp = world("batch"), world("discrete_f0")
    raw = cc.batch_inputs()
    inp = {k: dev(x) for k, x in raw.items() if k != "lengths"}
    b, n_ph, t_len, h, m = 3, cc.BATCH_SHAPE["n_ph"], cc.BATCH_SHAPE["t_len"], dc.HIDDEN, dc.M_BINS
    cond = torch.full((b, t_len, h), float("nan"), device="cuda")
    aux = torch.full((b, t_len, m), float("nan"), device="cuda")
    coarse = torch.zeros((b, t_len), dtype=torch.int64, device="cuda")

    def args(**over):
        a = _lib.DsdAcousticConditionArgs()
        a.struct_size, a.B, a.L, a.T = C.sizeof(a), b, n_ph, t_len
        a.tokens, a.durations, a.f0 = inp["tokens"].data_ptr(), inp["durations"].data_ptr(), inp["f0"].data_ptr()
        a.curves[0], a.curves[3] = inp["var_energy"].data_ptr(), inp["var_tension"].data_ptr()
        a.gender, a.velocity = inp["gender"].data_ptr(), inp["velocity"].data_ptr()
        a.spk_embed, a.spk_rows, a.languages = inp["spk_one"].data_ptr(), 1, inp["languages"].data_ptr()
        a.condition, a.aux_mel = cond.data_ptr(), aux.data_ptr()
        for k, v in over.items():
            if k.startswith("curve"):
                a.curves[int(k[5:])] = v
            else:
                setattr(a, k, v)
        return a

    def plain(**over):
        a = _lib.DsdAcousticConditionArgs()
        a.struct_size, a.B, a.L, a.T = C.sizeof(a), b, n_ph, t_len
        a.tokens, a.durations, a.f0, a.condition = inp["tokens"].data_ptr(), inp["durations"].data_ptr(), inp["f0"].data_ptr(), cond.data_ptr()
        for k, v in over.items():
            if k.startswith("curve"):
                a.curves[int(k[5:])] = v
            else:
                setattr(a, k, v)
        return a

    some = inp["f0"].data_ptr()
    refusals = [
        (wb, args(struct_size=132), "struct_size"), (wb, args(B=0), "B = 0"), (wb, args(B=65536), "B = 65536"),
        (wb, args(L=0), "L = 0"), (wb, args(L=2049), "L = 2049"), (wb, args(T=0), "T = 0"), (wb, args(T=-4), "T = -4"),
        (wb, args(tokens=None), "NULL tokens"), (wb, args(durations=None), "NULL tokens, durations"), (wb, args(f0=None), "f0"),
        (wb, args(condition=None), "condition"), (wb, args(curve0=None), "NULL curves[0] (energy)"),
        (wb, args(curve3=None), "NULL curves[3] (tension)"), (wb, args(curve1=some), "curves[1] (breathiness) given"),
        (wb, args(curve2=some), "curves[2] (voicing) given"), (wb, args(gender=None), "NULL gender"),
        (wb, args(spk_embed=None), "NULL spk_embed"), (wb, args(spk_rows=2), "spk_rows = 2"), (wb, args(spk_rows=0), "spk_rows = 0"),
        (wb, args(languages=None), "languages is required"), (wb, args(aux_mel=None), "NULL aux_mel"),
        (wb, args(f0_coarse=coarse.data_ptr()), "f0_coarse given"),
        (wp, plain(aux_mel=aux.data_ptr()), "aux_mel given"), (wp, plain(gender=some), "gender given"),
        (wp, plain(velocity=some), "velocity given"), (wp, plain(spk_embed=some, spk_rows=1), "spk_embed given"),
        (wp, plain(curve0=some), "curves[0] (energy) given"),
    ]
    for w, a, word in refusals:
        rc = lib.dsd_acoustic_condition(w.a._a, C.byref(a), None)
        msg = lib.dsd_last_error(None).decode()
        assert rc == EINVAL and msg.startswith("dsd_acoustic_condition:") and word in msg, (word, rc, msg)
    assert lib.dsd_acoustic_condition(wb.a._a, None, None) == EINVAL and b"NULL args" in lib.dsd_last_error(None)
    n_cond = len(refusals) + 1
    # the plain model takes its plain arguments (no languages: it has no lang_embed), and velocity may be left out on the other
    assert lib.dsd_acoustic_condition(wp.a._a, C.byref(plain()), None) == 0
    assert lib.dsd_acoustic_condition(wb.a._a, C.byref(args(velocity=None)), None) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(cond).all() and torch.isfinite(aux).all()
    cond.fill_(float("nan"))

    x = torch.full((b, 1, m, t_len), float("nan"), device="cuda")
    mel = torch.full((b, t_len, m), float("nan"), device="cuda")
    noise = torch.zeros((b, 1, m, t_len), device="cuda")
    aux.zero_()
    good = wb.a.plan(0.3, 4)

    def plan(**over):
        p = _lib.DsdAcousticPlan.from_buffer_copy(good)
        for k, v in over.items():
            setattr(p, k, v)
        return p
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    starts = [((plan(), aux, noise, 0, t_len, x), "B = 0"), ((plan(), aux, noise, b, 0, x), "T = 0"),
              ((plan(), aux, noise, b, t_len, None), "NULL plan or x"), ((None, aux, noise, b, t_len, x), "NULL plan or x"),
              ((plan(start=3), aux, noise, b, t_len, x), "plan->start = 3"), ((plan(start=-1), aux, noise, b, t_len, x), "plan->start = -1"),
              ((plan(), None, noise, b, t_len, x), "NULL source"), ((plan(start=2), None, noise, b, t_len, x), "NULL source"),
              ((plan(start=0), aux, None, b, t_len, x), "NULL noise"), ((plan(), aux, x, b, t_len, x), "must not alias"),
              ((plan(), x.view(b, t_len, m), noise, b, t_len, x), "must not alias")]
    for (p, source, eps, bb, tt, out), word in starts:
        rc = lib.dsd_acoustic_start(wb.a._a, None if p is None else C.byref(p), ptr(source), ptr(eps), bb, tt, ptr(out), None)
        msg = lib.dsd_last_error(None).decode()
        assert rc == EINVAL and msg.startswith("dsd_acoustic_start:") and word in msg, (word, rc, msg)
    x.zero_()
    samples = [((plan(), cond, x, None, 0, t_len, 0, mel), "B = 0"), ((plan(), cond, x, None, b, 0, 0, mel), "T = 0"),
               ((None, cond, x, None, b, t_len, 0, mel), "NULL plan"), ((plan(), None, x, None, b, t_len, 0, mel), "NULL plan, condition"),
               ((plan(), cond, None, None, b, t_len, 0, mel), "x or mel"), ((plan(), cond, x, None, b, t_len, 0, None), "x or mel"),
               ((plan(), cond, x, None, b, t_len, 2, mel), "flags = 0x2"), ((plan(), cond, x, None, b, t_len, 8, mel), "flags = 0x8"),
               ((plan(mode=1), cond, x, None, b, t_len, 0, mel), "plan->mode = 1"),
               ((plan(t_max=1001), cond, x, None, b, t_len, 0, mel), "plan->t_max = 1001"),
               ((plan(t_max=-1), cond, x, None, b, t_len, 0, mel), "plan->t_max = -1"),
               ((plan(speedup=0), cond, x, None, b, t_len, 0, mel), "plan->speedup = 0"),
               ((plan(n_step_noise=3), cond, x, None, b, t_len, 0, mel), "plan->n_step_noise = 3"),
               ((plan(t_max=4, speedup=1, n_step_noise=4), cond, x, None, b, t_len, 0, mel), "NULL step_noise")]
    for (p, cd, xx, sn, bb, tt, flags, out), word in samples:
        rc = lib.dsd_acoustic_sample(wb.a._a, None if p is None else C.byref(p), ptr(cd), ptr(xx), ptr(sn), bb, tt, flags, ptr(out), None)
        msg = lib.dsd_last_error(None).decode()
        assert rc == EINVAL and msg.startswith("dsd_acoustic_sample:") and word in msg, (word, rc, msg)
    rp = wp.a.plan(None, 3)
    for over, word in ((dict(t_start=-0.5), "plan->t_start = -0.5"), (dict(n_step_noise=1), "plan->n_step_noise = 1"), (dict(mode=0), "plan->mode = 0")):
        p = _lib.DsdAcousticPlan.from_buffer_copy(rp)
        for k, v in over.items():
            setattr(p, k, v)
        rc = lib.dsd_acoustic_sample(wp.a._a, C.byref(p), ptr(cond), ptr(x), None, b, t_len, 0, ptr(mel), None)
        msg = lib.dsd_last_error(None).decode()
        assert rc == EINVAL and word in msg, (word, rc, msg)
    hp_ = C.c_void_p(1)
    assert lib.dsd_acoustic_handle(wp.a._a, _lib.DSD_AC_AUX, C.byref(hp_)) == EINVAL and hp_.value is None
    assert lib.dsd_acoustic_handle(wb.a._a, 3, C.byref(hp_)) == EINVAL and b"which = 3" in lib.dsd_last_error(None)
    for which in (_lib.DSD_AC_FS2, _lib.DSD_AC_AUX, _lib.DSD_AC_DENOISER):
        assert wb.a.handle(which).value
    torch.cuda.synchronize()
    total = n_cond + len(starts) + len(samples) + 3 + 2
    print(f"{total} refusals")
    assert total >= 30 and torch.isnan(cond).all() and torch.isnan(mel).all()           # nothing was launched


# ------------------------------------------------------------------------------------------------ capture
def test_captured_chain_replays_what_the_eager_run_gives(world):
    """condition -> start -> sample, captured in one HIP graph after an eager run at the same sizes (which sized every
    workspace and built the program), replayed twice over inputs written in place."""
    w = world("aux_reflow")
    a, c = w.a, dc.AC_CASES["aux_reflow"]
    inp = {k: dev(x) for k, x in dc.acoustic_inputs("aux_reflow").items()}
    t_len = inp["f0"].shape[1]
    noise = dev(synth.synth_normal((1, 1, dc.M_BINS, t_len), c["seed"] + 2))
    f0 = inp["f0"].clone()
    p = a.plan(0.5, c["steps"])
    assert p.start == _lib.DSD_AC_START_MIX
    bufs = dict(cond=torch.empty((1, t_len, dc.HIDDEN), device="cuda"), aux=torch.empty((1, t_len, dc.M_BINS), device="cuda"),
                x=torch.empty((1, 1, dc.M_BINS, t_len), device="cuda"), mel=torch.empty((1, t_len, dc.M_BINS), device="cuda"))
    with torch.no_grad():
        def chain():
            a.condition(inp["tokens"], inp["durations"], f0, out=(bufs["cond"], bufs["aux"]))
            a.start(p, source=bufs["aux"], noise=noise, out=bufs["x"])
            a.sample(p, bufs["cond"], bufs["x"], out=bufs["mel"])

        def eager(values):
            f0.copy_(values)
            chain()
            torch.cuda.synchronize()
            return {k: x.clone() for k, x in bufs.items()}
        first = eager(inp["f0"])
        other = eager(inp["f0"] * 1.25)
        assert not torch.equal(first["mel"], other["mel"])
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            chain()
        for values, want in ((inp["f0"], first), (inp["f0"] * 1.25, other)):
            f0.copy_(values)
            for x in bufs.values():
                x.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            wrong = []
            for k in bufs:
                differ = int((bufs[k].view(torch.int32) != want[k].view(torch.int32)).sum())
                nans = int(torch.isnan(bufs[k]).sum())
                print(f"replayed {k}: {differ} of {bufs[k].numel()} elements differ from the eager run's ({nans} still NaN)")
                wrong += [k] * bool(differ)
            assert not wrong, wrong


# ------------------------------------------------------------------------------------------------ the C example
def test_c_example_prints_the_python_twins_checksums(world, tmp_path):
    """examples/c_abi_acoustic.c compiled and run on a packed model with a mini_nsf vocoder section: one file -> condition and
    aux mel -> plan -> x from dsd_acoustic_start and dsd_noise_fill -> sample -> mel -> dsd_vocode.  The sums it prints are
    held against the same chain through cacoustic.py on the same file, inputs and seed (every sum equal) and against the
    Python twin (condition, aux and x equal; the mel within ALONE_TOL per element, summed)."""
    import vocoder_config_cases as vcc
    from diffsinger_amd.diffusion import _to_bfmt
    from diffsinger_amd.vocoder import Generator
    from gpu_util import load_synth
    h = vcc.over_default(**dict(vcc.CASES["mini_two"]["over"], num_mels=dc.M_BINS))
    assert h["mini_nsf"] and vcc.accepts(h)[0]
    gen = load_synth(Generator(h), synth.synth_state_dict(synth.nsf_hifigan_param_shapes(h), seed=2811, gain=vcc.GAIN))
    w = world("batch", extra=[modelfile.section_of("vocoder", gen)])
    exe = tmp_path / "c_abi_acoustic"
    libdir = os.path.join(ROOT, "diffsinger_amd")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "c_abi_acoustic.c"), "-L" + libdir, "-ldsdenoise", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True, timeout=300)
    r = subprocess.run([str(exe), w.path, cc.PREFIX], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    got = {}
    for line in r.stdout.splitlines():
        if line.startswith("sum "):
            _, name, value = line.split()
            got[name] = float(value)
    # the example's own inputs, restated (examples/c_abi_acoustic.c)
    a, model = w.a, w.model
    n_ph, t_len, steps, depth, seed = 6, 96, 4, 0.375, 2026
    tokens = torch.tensor([[1 + (3 * i) % 11 for i in range(n_ph)]], device="cuda")
    tokens[0, -1] = 0
    languages = torch.tensor([[1 + i % 2 for i in range(n_ph)]], device="cuda")
    durations = torch.tensor([[20, 16, 0, 36, 24, 7]], device="cuda")
    t = torch.arange(t_len, device="cuda")
    f0 = torch.where((t >= 10) & (t < 14), 0.0, 180.0 + 0.5 * t.float())[None]
    curve = (-30.0 + 0.125 * (t % 16).float())[None]
    gender = (0.3125 * ((t % 9) - 4).float())[None]
    velocity = (0.25 + 0.125 * (t % 20).float())[None]
    spk = (0.015625 * (torch.arange(dc.HIDDEN, device="cuda", dtype=torch.float32) % 7.0 - 3.0))[None, None]
    variances = dict(energy=curve, tension=curve)
    with torch.no_grad():
        cond, aux = a.condition(tokens, durations, f0, variances, gender=gender, velocity=velocity, spk_embed=spk, languages=languages)
        p = a.plan(depth, steps)
        assert (p.start, p.t_max, p.speedup, p.n_step_noise) == (_lib.DSD_AC_START_MIX, 372, 93, 0)
        x = a.start(p, source=aux, noise=None)
        flat = x.view(1, 1, dc.M_BINS, t_len)
        seeded.fill((1, 1, dc.M_BINS, t_len), [seed], seeded.X_T, src=flat, src_scale=p.src_scale, scale=p.noise_scale, out=flat)
        mel = a.sample(p, cond, x)
        wav = gen(mel.transpose(1, 2), f0)
        # the Python twin
        t_cond, t_aux = model.forward_fs2_aux(tokens, durations, f0, variances, gender=gender, velocity=velocity, spk_embed=spk, languages=languages)
        d = model.diffusion
        k, mid = (d.spec_max - d.spec_min) / 2., (d.spec_max + d.spec_min) / 2.
        t_x = d._seeded_start(p.t_max, _to_bfmt((t_aux - mid) / k, 1), [seed], seeded.X_T, 1, t_len, x.device)
        eps = seeded.fill((1, 1, dc.M_BINS, t_len), [seed], seeded.X_T, device=x.device).view(1, 1, dc.M_BINS, t_len)
        t_mel = model.forward_shallow_diffusion(t_cond, t_aux, torch.tensor(depth, dtype=torch.float32), steps, noise=eps)
    assert a.cfg.mel_base_e == 1                                          # the case's mel is natural-log: the vocoder takes it as it is
    want = dict(condition=cond, aux_mel=aux, x=x, mel=mel, wav=wav)
    assert set(got) == set(want), (sorted(got), sorted(want))
    for name, tensor in want.items():
        s = float(tensor.double().sum())
        print(f"{name}: C example {got[name]!r}, cacoustic {s!r}")
        assert got[name] == pytest.approx(s, rel=0, abs=1e-9 * max(1.0, abs(s))), name         # %.17g of the same double sum
    for name, tensor in dict(condition=t_cond, aux_mel=t_aux, x=t_x).items():
        s = float(tensor.double().sum())
        print(f"{name}: C example {got[name]!r}, Python twin {s!r}")
        assert got[name] == pytest.approx(s, rel=0, abs=1e-9 * max(1.0, abs(s))), name
    close(mel, t_mel.cpu().numpy(), ALONE_TOL, True, "mel vs the twin")
    s = float(t_mel.double().sum())
    print(f"mel: C example {got['mel']!r}, Python twin {s!r}")
    assert abs(got["mel"] - s) <= ALONE_TOL * max(1.0, float(t_mel.abs().max())) * t_mel.numel()
    gen.release_native()
