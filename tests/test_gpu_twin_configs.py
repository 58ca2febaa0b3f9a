"""-m gpu: the staged C twins (dsd_acoustic_open .. dsd_acoustic_sample, dsd_variance_open .. dsd_variance_post) opened on
the model shapes of tests/twin_config_cases.py - LYNXNet denoisers, hidden sizes 32 and 96, 5 and 80 mel bins, the cosine
schedule, every embedding alone, four predicted variances, ragged batches through a LYNXNet - against

  * G31 (tests/golden/g31_twin_configs.npz, the reference's own deployment twins on the CPU) under the bounds
    tests/test_gpu_deploy.py applies to the same quantities, through twin_config_cases.bound_for (2 x floor where the
    reference's own fp32 error exceeds half a bound; no case needs it);
  * the Python twins (deploy.DiffSingerAcousticDeploy / DiffSingerVarianceDeploy) with the same weights: conditions, start
    states, f0_coarse and front stages bit for bit, the sampler stage bit for bit where the library's program keys equal
    schedule.py's and within ALONE_TOL otherwise, the post stages within ALONE_TOL (torch's mean adds in another order) -
    what tests/test_gpu_cacoustic.py and test_gpu_cvariance.py hold the one shape they know to.  The sampler stage of the
    variance twin runs on the handle dsd_variance_open made (`c_sample`), for the DDPM twin too, and its result is what meets
    G31 and feeds the post stage.

Every figure is printed before it is asserted."""
import os

import numpy as np
import pytest
import torch

import deploy_cases as dc
import twin_config_cases as tc
from diffsinger_amd import _lib, cprogram, modelfile, schedule
from diffsinger_amd.hparams import hparams
from gpu_util import dev
from test_gpu_cacoustic import World as AcousticWorldBase, c_condition, run_stage, same, twin_condition
from test_gpu_cvariance import World as VarianceWorldBase, raw_sample, same as same_or_nan
from test_gpu_deploy import ALONE_TOL, close

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g31_twin_configs.npz")
AC_SINGLE = [t for t, c in tc.AC_CASES.items() if "lengths" not in c]
VAR_SINGLE = [t for t, c in tc.VAR_CASES.items() if "lengths" not in c]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    yield
    hparams.clear()
    hparams.update(hidden_size=256)


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


class AcousticWorld(AcousticWorldBase):
    """test_gpu_cacoustic.World on a case of twin_config_cases"""

    def __init__(self, tag, directory):
        from diffsinger_amd.cacoustic import Acoustic
        self.model, self.hp = tc.build_acoustic(tag, cuda=True)
        self.path = os.path.join(str(directory), tag + ".dsdm")
        modelfile.write(self.path, modelfile.acoustic_sections("ac", self.model), {"kind": "acoustic"})
        with modelfile.open(self.path) as f:
            self.a = Acoustic(f, "ac", "cuda")


class VarianceWorld(VarianceWorldBase):
    """test_gpu_cvariance.World on a case of twin_config_cases"""

    def __init__(self, tag, directory):
        from diffsinger_amd.cvariance import Variance
        self.model, self.hp = tc.build_variance(tag, cuda=True)
        self.path = os.path.join(str(directory), tag + ".dsdm")
        modelfile.write(self.path, modelfile.variance_sections("var", self.model), {"kind": "variance"})
        with modelfile.open(self.path) as f:
            self.v = Variance(f, "var", "cuda")


@pytest.fixture
def world(tmp_path):
    made = []

    def make(kind, tag):
        made.append(kind(tag, tmp_path))
        return made[-1]
    yield make
    for w in made:
        w.close()


def golden(got, g, tag, key):
    """a stage output against G31 under the bound of its quantity"""
    want = g[key]
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    assert got.shape == want.shape, (key, got.shape, want.shape)
    tol, unit, floor = tc.bound_for(tag, key)
    name = tc.BOUNDS[tc.quantity_of(key, tag)][0]
    err, scale = float(np.abs(got - want).max()), tc.scale_of(unit, want)
    print(f"{key} vs the reference: max |err| {err:.3e} = {err / scale:.3e} ({unit}), bound {tol:.1e} ({name}), the reference's own floor {floor:.2e}")
    assert err <= tol * scale, (key, err, tol * scale)


def bits(x):
    return np.float32(x).view(np.uint32)


def c_sample(v, which, predictor, cond, steps, noise, what, schedule_type="linear"):
    """The sampler stage on the handle dsd_variance_open made, as a C caller runs it -> the denormalised sample before the
    mean over the bins.  Rectified flow: cvariance.Variance.sample.  DDPM: the plan of dsd_onnx_ddpm_plan, its DDIM program
    from dsd_program_build on dsd_ddpm_tables_fill's tables, dsd_prepare_cond + dsd_sample on the borrowed handle.  Held to
    `raw`, the Python twin's sample on its own handle: bit for bit where the program keys agree, within ALONE_TOL otherwise."""
    from diffsinger_amd.cvariance import _ptr, _stream
    raw = raw_sample(predictor, cond, steps, noise)
    if v.cfg.diffusion_type == _lib.DSD_DIFFUSE_REFLOW:
        mine = v.sample(which, cond, steps, noise)
        same_or_nan(mine, raw, f"{what}: the sample on the borrowed handle")
        return mine
    t_max, speedup = cprogram.onnx_ddpm_plan(v.cfg.timesteps, v.cfg.k_step, predictor.timestep_factors.cpu(), steps)
    assert (t_max, speedup) == schedule.onnx_ddpm_plan(predictor.timesteps, predictor.k_step, predictor.timestep_factors.cpu(), steps)
    assert speedup > 1 and t_max > 0, (t_max, speedup)                    # DDIM: no step noise
    spec, keep = cprogram.spec("ddim", cprogram.tables(schedule_type, v.cfg.timesteps), t_max=t_max, speedup=speedup)
    bsz, t_len, hid = cond.shape
    _, f, m, _ = noise.shape
    mine = torch.full((bsz, t_len, m) if f == 1 else (bsz, f, t_len, m), float("nan"), device="cuda")
    scale, shift = v.affine(which)
    h, st = v.backbone(which), _stream(v.device)
    with cprogram.built(spec) as prog:
        key = cprogram.from_c(prog.contents).key()
        _lib.check(h, _lib.lib().dsd_prepare_cond(h, _ptr(cond), bsz, t_len, t_len * hid, 1, hid, st), "dsd_prepare_cond")
        _lib.check(h, _lib.lib().dsd_sample(h, prog, _ptr(noise), None, _ptr(mine), _ptr(scale), _ptr(shift), _lib.DSD_SAMPLE_TRANSPOSE, st),
                   "dsd_sample")
        torch.cuda.synchronize()
    theirs = schedule.ddim_program(predictor._tables, t_max, speedup).key()
    print(f"{what}: DDIM t_max {t_max}, speed-up {speedup} on the borrowed handle (F = {f}, M = {m}, H = {hid})")
    close(mine, raw.cpu().numpy(), ALONE_TOL, True, f"{what}: the sample on the borrowed handle vs the twin")
    if key == theirs:
        print(f"{what}: the library's builder gives schedule.py's program: the sample must be bit-identical")
        same_or_nan(mine, raw, f"{what}: the sample on the borrowed handle")
    else:
        print(f"{what}: the library's builder and schedule.py differ in a coefficient's last bit: held to ALONE_TOL only")
    return mine


# ------------------------------------------------------------------------------------------------ acoustic, one utterance
@pytest.mark.parametrize("tag", AC_SINGLE)
def test_acoustic_stages_vs_golden_and_python_twin(g, world, tag):
    w = world(AcousticWorld, tag)
    model, hp, a, c = w.model, w.hp, w.a, tc.AC_CASES[tag]
    inp = {k: dev(x) for k, x in tc.acoustic_inputs(tag).items()}
    discrete = hp.get("f0_embed_type") == "discrete"
    assert (a.cfg.hidden_size, a.cfg.out_dims) == (hp["hidden_size"], c["m_bins"])
    with torch.no_grad():
        res = c_condition(a, inp, want_coarse=discrete)
        want = twin_condition(model, inp)
        if hp["use_shallow_diffusion"]:
            cond, aux, want_cond = res[0], res[1], want[0]
            golden(aux, g, tag, f"{tag}_aux")
            same(aux, want[1], "aux_mel")
        else:
            cond, aux, want_cond = (res[0] if discrete else res), None, want
        golden(cond, g, tag, f"{tag}_cond")
        same(cond, want_cond, "condition")
        if discrete:
            from diffsinger_amd.deploy import f0_to_coarse, length_regulate
            mel2ph = length_regulate(inp["durations"] * (inp["tokens"] > 0), inp["f0"].shape[1])
            coarse = f0_to_coarse(inp["f0"] * (mel2ph > 0))
            print(f"f0_coarse: {int((res[1] != coarse).sum())} of {coarse.numel()} frames differ; range {int(coarse.min())} .. {int(coarse.max())}")
            assert torch.equal(res[1], coarse) and int(coarse.max()) > 1
        # an embedding that is there is live: the condition moves when its curve alone is zeroed
        live = [k for k in inp if k.startswith("var_") or k in ("gender", "velocity")]
        for key in live if tag.startswith("alone_") or tag == "pairs" else []:
            other = c_condition(a, dict(inp, **{key: torch.zeros_like(inp[key])}))
            moved = float((other - cond).abs().max())
            print(f"{key} zeroed: the condition moves by {moved:.3e}")
            assert moved > 1e-3 * float(cond.abs().max()), key
        if tag.startswith("alone_"):
            assert live == [{"key_shift": "gender", "speed": "velocity"}.get(tag[6:], "var_" + tag[6:])]
        starts = []
        for i, (stage, depth, steps) in enumerate(c["stages"]):
            arrays = tc.stage_noise(tag, i)
            noise = dev(arrays[0])
            step_noise = dev(np.stack(arrays[1:])) if len(arrays) > 1 else None
            mel, _, p = run_stage(w, depth, steps, cond, aux, noise, step_noise=step_noise, what=f"{stage} (depth {depth}, {steps} steps)")
            golden(mel, g, tag, f"{tag}_s{i}")
            starts.append(p.start)
            if hp["diffusion_type"] == "ddpm":      # the plan against schedule.py and the Python twin's own tables
                d = model.diffusion
                t_max, speedup = schedule.onnx_ddpm_plan(d.timesteps, d.k_step, d.timestep_factors.cpu(), steps, depth)
                print(f"plan: t_max {p.t_max}, speedup {p.speedup}, start {p.start}, src_scale {p.src_scale!r}, noise_scale {p.noise_scale!r}")
                assert (p.t_max, p.speedup, p.n_step_noise) == (t_max, speedup, len(arrays) - 1)
                if p.start == _lib.DSD_AC_START_MIX:
                    sa, s1 = float(d.sqrt_alphas_cumprod[t_max - 1]), float(d.sqrt_one_minus_alphas_cumprod[t_max - 1])
                    assert (bits(p.src_scale), bits(p.noise_scale)) == (bits(sa), bits(s1))
        if tag == "lynx_ddpm_cosine":
            assert sorted(set(starts)) == [_lib.DSD_AC_START_NOISE, _lib.DSD_AC_START_MIX, _lib.DSD_AC_START_SOURCE]
            assert a.cfg.schedule_type == _lib.SCHEDULE_IDS["cosine"]


# ------------------------------------------------------------------------------------------------ acoustic, ragged
def test_ragged_batch_through_a_lynxnet_denoiser(g, world):
    """lynx_ragged: B = 3, lengths 70, 1, 33 through dsd_acoustic_set_lengths.  The dense condition stage against the Python
    twin bit for bit; under the lengths every item against its lone run at its own frame count - the condition bit for bit (the
    encoder does not read the lengths), aux mel and mel within ALONE_TOL, as tests/test_gpu_cproject.py holds the WaveNet
    case - and against the reference's run of that item alone."""
    tag = "lynx_ragged"
    w = world(AcousticWorld, tag)
    model, a, c = w.model, w.a, tc.AC_CASES[tag]
    raw = tc.acoustic_batch_inputs(tag)
    inp = {k: dev(x) for k, x in raw.items() if k != "lengths"}
    lens = [int(n) for n in raw["lengths"]]
    (_, depth, steps), noise = c["stages"][0], dev(tc.stage_noise(tag, 0)[0])
    with torch.no_grad():
        p = a.plan(depth, steps)
        assert p.start == _lib.DSD_AC_START_MIX
        dense_cond, dense_aux = c_condition(a, inp)
        want_cond, want_aux = twin_condition(model, inp)
        same(dense_cond, want_cond, "dense condition")
        same(dense_aux, want_aux, "dense aux_mel")
        a.set_lengths(lens)
        try:
            cond, aux = c_condition(a, inp)
            x = a.start(p, source=aux, noise=noise)
            mel = a.sample(p, cond, x)
        finally:
            a.set_lengths(None)
        same(cond, dense_cond, "condition under the lengths")
        for b, n in enumerate(lens):
            sl = slice(b, b + 1)
            lone_cond, lone_aux = c_condition(a, inp, sl=sl, t_len=n)
            lone_x = a.start(p, source=lone_aux, noise=noise[sl, :, :, :n].contiguous())
            lone_mel = a.sample(p, lone_cond, lone_x)
            same(lone_cond, cond[sl, :n], f"item {b} alone at T = {n}: condition")
            same(lone_x, x[sl, :, :, :n].contiguous(), f"item {b} alone at T = {n}: x")
            close(aux[sl, :n], lone_aux.cpu().numpy(), ALONE_TOL, True, f"item {b} ({n} frames): aux_mel against its lone run")
            close(mel[sl, :n], lone_mel.cpu().numpy(), ALONE_TOL, True, f"item {b} ({n} frames): mel against its lone run")
            golden(cond[sl, :n], g, tag, f"{tag}_i{b}_cond")
            golden(aux[sl, :n], g, tag, f"{tag}_i{b}_aux")
            golden(mel[sl, :n], g, tag, f"{tag}_i{b}_s0")
        # not vacuous: without the lengths item 2's last frames see the junk f0 past its end through the aux decoder's convolutions
        n = lens[2]
        gap = float((dense_aux[2, n - 3:n] - aux[2, n - 3:n]).abs().max())
        print(f"item 2's last 3 frames of aux_mel, dense against under the lengths: {gap:.3e}")
        assert gap > ALONE_TOL * max(1.0, float(aux[2, :n].abs().max()))


# ------------------------------------------------------------------------------------------------ acoustic, capture
def test_captured_chain_with_a_lynxnet_replays_what_the_eager_run_gives(world):
    """condition -> start -> sample on lynx_reflow, captured in one HIP graph after an eager run at the same sizes, replayed
    twice over inputs written in place: test_gpu_cacoustic.py's captured chain with a LYNXNet, H = 96 and M = 80 inside."""
    tag = "lynx_reflow"
    w = world(AcousticWorld, tag)
    a, c, hp = w.a, tc.AC_CASES[tag], w.hp
    inp = {k: dev(x) for k, x in tc.acoustic_inputs(tag).items()}
    t_len, m, h = c["t_len"], c["m_bins"], hp["hidden_size"]
    _, depth, steps = c["stages"][0]
    noise = dev(tc.stage_noise(tag, 0)[0])
    f0 = inp["f0"].clone()
    p = a.plan(depth, steps)
    assert p.start == _lib.DSD_AC_START_MIX
    bufs = dict(cond=torch.empty((1, t_len, h), device="cuda"), aux=torch.empty((1, t_len, m), device="cuda"),
                x=torch.empty((1, 1, m, t_len), device="cuda"), mel=torch.empty((1, t_len, m), device="cuda"))
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
                print(f"replayed {k}: {differ} of {bufs[k].numel()} elements differ from the eager run's ({int(torch.isnan(bufs[k]).sum())} still NaN)")
                wrong += [k] * bool(differ)
            assert not wrong, wrong


# ------------------------------------------------------------------------------------------------ variance, one utterance
@pytest.mark.parametrize("tag", VAR_SINGLE)
def test_variance_stages_vs_golden_and_python_twin(g, world, tag):
    w = world(VarianceWorld, tag)
    model, hp, v, c = w.model, w.hp, w.v, tc.VAR_CASES[tag]
    inp = {k: dev(x) for k, x in tc.variance_inputs(tag).items()}
    shapes = tc.variance_noise_shapes(tag) if c["steps"] else {}
    from diffsinger_amd import synth
    noise = {k: dev(synth.synth_normal(s, c["seed"] + 2 + i)) for i, (k, s) in enumerate(shapes.items())}
    spk = inp.get("spk_embed")
    assert v.cfg.hidden_size == hp["hidden_size"]
    with torch.no_grad():
        if hp["predict_dur"]:
            enc, x_masks = v.encode(inp["tokens"], word_div=inp["word_div"], word_dur=inp["word_dur"], languages=inp.get("languages"))
            want_enc, want_masks = model.forward_linguistic_encoder_word(inp["tokens"], inp["word_div"], inp["word_dur"],
                                                                         languages=inp.get("languages"))
            dur = v.dur(enc, x_masks, inp["ph_midi"], spk_embed=spk)
            golden(dur, g, tag, f"{tag}_dur_pred")
            same_or_nan(dur, model.forward_dur_predictor(want_enc, want_masks, inp["ph_midi"], spk_embed=spk), "ph_dur_pred")
        else:
            enc, x_masks = v.encode(inp["tokens"], ph_dur=inp["ph_dur"], languages=inp.get("languages"))
            want_enc, want_masks = model.forward_linguistic_encoder_phoneme(inp["tokens"], inp["ph_dur"], languages=inp.get("languages"))
        assert np.array_equal(x_masks.cpu().numpy(), g[f"{tag}_x_masks"])
        golden(enc, g, tag, f"{tag}_enc")
        same_or_nan(enc, want_enc, "encoder_out")
        same_or_nan(x_masks, want_masks, "x_masks")
        if hp["predict_pitch"]:
            args = dict(note_midi=inp["note_midi"], note_rest=inp["note_rest"], note_dur=inp["note_dur"], note_glide=inp.get("note_glide"),
                        pitch=inp["pitch"], expr=inp.get("expr"), retake=inp["retake"], spk_embed=spk)
            cond, base = v.pitch_cond(enc, inp["ph_dur"], **args)
            want_cond, want_base = model.forward_pitch_preprocess(enc, inp["ph_dur"], **args)
            golden(base, g, tag, f"{tag}_base_pitch")
            golden(cond, g, tag, f"{tag}_pitch_cond")
            same_or_nan(base, want_base, "base_pitch")
            same_or_nan(cond, want_cond, "pitch_cond")
            assert v.cfg.pitch_repeat_bins == noise["pitch"].shape[2]
            # the sampler and the post stage of the C twin on the reference's condition: the stages under test, not the chain before
            gold_cond, gold_base = dev(g[f"{tag}_pitch_cond"]), dev(g[f"{tag}_base_pitch"])
            raw = c_sample(v, _lib.DSD_VAR_PITCH, model.pitch_predictor, gold_cond, c["steps"], noise["pitch"], "pitch", hp["schedule_type"])
            golden(raw.mean(-1), g, tag, f"{tag}_x_pred")
            pred = v.pitch_post(raw, gold_base)
            golden(pred, g, tag, f"{tag}_pitch_pred")
            close(pred, model.forward_pitch_postprocess(raw.mean(-1), gold_base).cpu().numpy(), ALONE_TOL, True, "pitch_pred vs the twin")
        names = dc.variance_names(hp)
        assert v.names == names
        if names:
            curves = {n: inp["var_" + n] for n in names}
            cond = v.cond(enc, inp["ph_dur"], inp["pitch"], curves, inp["var_retake"], spk_embed=spk)
            golden(cond, g, tag, f"{tag}_var_cond")
            same_or_nan(cond, model.forward_variance_preprocess(enc, inp["ph_dur"], inp["pitch"], variances=curves, retake=inp["var_retake"],
                                                                spk_embed=spk), "variance_cond")
            assert tuple(noise["variance"].shape[1:3]) == (len(names), v.cfg.var_repeat_bins)
            raw = c_sample(v, _lib.DSD_VAR_VARIANCES, model.variance_predictor, cond, c["steps"], noise["variance"], "variances", hp["schedule_type"])
            golden(raw.mean(-1), g, tag, f"{tag}_xs_pred")
            outs = v.post(raw)
            twin = model.forward_variance_postprocess(raw.mean(-1))
            assert list(outs) == names and len(twin) == len(names)
            for n, t in zip(names, twin):
                golden(outs[n], g, tag, f"{tag}_out_{n}")
                close(outs[n], t.cpu().numpy(), ALONE_TOL, True, n + " vs the twin")
            for i, n in enumerate(names):           # a curve is live in its own slot: zeroing it alone moves the condition
                other = v.cond(enc, inp["ph_dur"], inp["pitch"], dict(curves, **{n: torch.zeros_like(curves[n])}), inp["var_retake"], spk_embed=spk)
                moved = float((other - cond).abs().max())
                print(f"{n} zeroed: the variance condition moves by {moved:.3e}")
                assert moved > 1e-3 * float(cond.abs().max()), n


# ------------------------------------------------------------------------------------------------ variance, ragged
def test_ragged_batch_through_a_lynxnet_pitch_predictor(g, world):
    """lynx_ragged_var: B = 3, padded, lengths 70, 1, 41.  The front stages against the Python twin and every item against its
    lone run, bit for bit, with base_pitch zero past every length (tests/test_gpu_cvariance.py's padded batch); the sampler and
    the post stage under dsd_variance_set_lengths against every item's lone run within ALONE_TOL (tests/test_gpu_words.py);
    and every item against the reference's run of that item alone."""
    from diffsinger_amd import synth
    tag = "lynx_ragged_var"
    w = world(VarianceWorld, tag)
    model, hp, v, c = w.model, w.hp, w.v, tc.VAR_CASES[tag]
    raw_inp = tc.variance_batch_inputs(tag)
    inp = {k: dev(x) for k, x in raw_inp.items() if k != "lengths"}
    lens, real = [int(n) for n in raw_inp["lengths"]], [int(n) for n in raw_inp["word_div"].sum(1)]
    t_len, steps, h = c["t_len"], c["steps"], hp["hidden_size"]
    noise = dev(synth.synth_normal((3,) + tc.variance_noise_shapes(tag)["pitch"][1:], c["seed"] + 2))

    def front(obj, sl, t, lengths, enc_from=None):
        c_side = obj is v
        out = {}
        if c_side:
            out["encoder_out"], out["x_masks"] = v.encode(inp["tokens"][sl], word_div=inp["word_div"][sl], word_dur=inp["word_dur"][sl])
        else:
            out["encoder_out"], out["x_masks"] = model.forward_linguistic_encoder_word(inp["tokens"][sl], inp["word_div"][sl], inp["word_dur"][sl])
        enc = out["encoder_out"] if enc_from is None else enc_from[sl]
        out["ph_dur_pred"] = (v.dur if c_side else model.forward_dur_predictor)(enc, out["x_masks"], inp["ph_midi"][sl])
        kw = dict(note_midi=inp["note_midi"][sl], note_rest=inp["note_rest"][sl], note_dur=inp["note_dur"][sl], note_glide=inp["note_glide"][sl],
                  pitch=inp["pitch"][sl, :t], expr=inp["expr"][sl, :t], retake=inp["retake"][sl, :t], lengths=lengths)
        out["pitch_cond"], out["base_pitch"] = (v.pitch_cond if c_side else model.forward_pitch_preprocess)(enc, inp["ph_dur"][sl], **kw)
        return out

    def sampled(cond, base, eps, lengths):
        v.set_lengths(lengths)
        try:
            raw = v.sample(_lib.DSD_VAR_PITCH, cond, steps, eps)
            return raw, v.pitch_post(raw, base)
        finally:
            v.set_lengths(None)

    with torch.no_grad():
        everything = slice(0, 3)
        batch = front(v, everything, t_len, lens)
        twin = front(model, everything, t_len, lens, enc_from=batch["encoder_out"])
        for k in batch:
            same_or_nan(batch[k], twin[k], k)
        raw, pred = sampled(batch["pitch_cond"], batch["base_pitch"], noise, lens)
        # the sampler on the reference's own conditions, padded with zeros: the stage under test, not the chain before it
        gold_cond, gold_base = torch.zeros((3, t_len, h), device="cuda"), torch.zeros((3, t_len), device="cuda")
        for b, n in enumerate(lens):
            gold_cond[b, :n], gold_base[b, :n] = dev(g[f"{tag}_i{b}_pitch_cond"])[0], dev(g[f"{tag}_i{b}_base_pitch"])[0]
        gold_raw, gold_pred = sampled(gold_cond, gold_base, noise, lens)
        for b, n in enumerate(lens):
            sl = slice(b, b + 1)
            alone = front(v, sl, n, None, enc_from=batch["encoder_out"])
            for k in batch:
                frames = k in ("pitch_cond", "base_pitch")
                same_or_nan(alone[k], batch[k][sl, :n] if frames else batch[k][sl], f"item {b} alone, {k}")
            assert not batch["base_pitch"][b, n:].any()                  # frames past the item's length
            lone_raw, lone_pred = sampled(alone["pitch_cond"], alone["base_pitch"], noise[sl, :, :, :n].contiguous(), None)
            close(raw[sl, :n], lone_raw.cpu().numpy(), ALONE_TOL, True, f"item {b} ({n} frames): the pitch sample against its lone run")
            close(pred[sl, :n], lone_pred.cpu().numpy(), ALONE_TOL, True, f"item {b} ({n} frames): pitch_pred against its lone run")
            pre = f"{tag}_i{b}"
            golden(batch["encoder_out"][sl, :real[b]], g, tag, pre + "_enc")
            golden(batch["ph_dur_pred"][sl, :real[b]], g, tag, pre + "_dur_pred")
            assert np.array_equal(batch["x_masks"][sl, :real[b]].cpu().numpy(), g[pre + "_x_masks"]) and bool(batch["x_masks"][b, real[b]:].all())
            golden(batch["pitch_cond"][sl, :n], g, tag, pre + "_pitch_cond")
            golden(batch["base_pitch"][sl, :n], g, tag, pre + "_base_pitch")
            golden(gold_raw[sl, :n].mean(-1), g, tag, pre + "_x_pred")
            golden(gold_pred[sl, :n], g, tag, pre + "_pitch_pred")
