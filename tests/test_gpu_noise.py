"""-m gpu: seeded draws on the device (dsd_noise_fill, noise.fill, the seed= arguments) against the numpy restatement of
the generator (tests/noise_ref.py).

Uniform draws are bitwise the oracle's.  Normal draws are within 1e-5 absolute of the float64 Box-Muller on the same
uniforms: the fp32 angle 2 pi u carries at most ~3e-7 absolute error, times r <= 5.77, plus a few ulp of logf, sqrtf
and sincosf - about 2e-6; the same fp32 evaluation in numpy measured 1.5e-6 (cos) / 1.7e-6 (sin) over 2 M draws; 1e-5
leaves 5x over that.  Everything else - layout independence, capture, seed= against the explicit noise= - is bitwise:
both sides get the same tensors, so any difference is a wiring error.
"""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import noise_ref  # noqa: E402
from diffsinger_amd import noise, synth  # noqa: E402
from gpu_util import dev, load_synth, make_backbone, set_hp, synth_params  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORMAL_ATOL = 1e-5
HIGH = 0x9e3779b97f4a7c15           # a seed with a non-zero high word
ARGS = dict(num_layers=2, num_channels=64, dilation_cycle_length=2)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"


def same_as_oracle(got, want64, kind):
    got = got.cpu().numpy()
    assert got.shape == want64.shape and got.dtype == np.float32
    if kind == "uniform":
        assert np.array_equal(got.astype(np.float64), want64)
    else:
        err = float(np.abs(got.astype(np.float64) - want64).max())
        print(f"normal: max |device - float64 oracle| = {err:.3e} over {got.size} draws")
        assert err <= NORMAL_ATOL, err


# [n, B, rows, cols], seeds: the scalar path with a tail; the vector path; one column, one block of four, a block and a
# tail; more than one workgroup (1000 threads); more items than one launch carries (64); a seed with a high word
SHAPES = [((2, 2, 3, 9), [11, HIGH]), ((1, 1, 5, 64), [12]), ((1, 1, 4, 1), [13]), ((1, 2, 3, 4), [14, 15]), ((1, 1, 3, 5), [HIGH]),
          ((1, 1, 40, 100), [16]), ((2, 1, 37, 27), [17]), ((1, 70, 2, 4), list(range(100, 170))), ((1, 66, 1, 3), list(range(66)))]


@pytest.mark.parametrize("kind", ["uniform", "normal"])
@pytest.mark.parametrize("shape,seeds", SHAPES, ids=["x".join(map(str, s)) for s, _ in SHAPES])
def test_fill_equals_oracle(shape, seeds, kind):
    got = noise.fill(shape, seeds, noise.STEP, first_stream=3, kind=kind)
    same_as_oracle(got, noise_ref.fill(shape, seeds, noise_ref.STEP, first_stream=3, kind=kind), kind)


@pytest.mark.parametrize("kind", ["uniform", "normal"])
def test_unaligned_out_takes_the_scalar_path(kind):
    """cols = 8 but `out` one float past a 16-byte boundary: a 16-byte store there would fault or land four bytes off."""
    buf = torch.full((1 + 2 * 3 * 8 + 3,), -7.0, device="cuda")
    assert buf.data_ptr() % 16 == 0
    out = buf[1:1 + 48]
    noise.fill((1, 2, 3, 8), [21, HIGH], noise.X_T, kind=kind, out=out)
    same_as_oracle(out.view(1, 2, 3, 8), noise_ref.fill((1, 2, 3, 8), [21, HIGH], noise_ref.X_T, kind=kind), kind)
    assert float(buf[0]) == -7.0 and bool((buf[49:] == -7.0).all())        # nothing outside the view was written


def test_layout_independence_is_bitwise():
    seeds = [31, HIGH, 33]
    for kind in ("normal", "uniform"):
        wide = noise.fill((1, 3, 6, 40), seeds, noise.X_T, kind=kind)               # vector path, B = 3
        lone = noise.fill((1, 1, 6, 17), [seeds[1]], noise.X_T, kind=kind)          # scalar path with a tail, B = 1
        assert torch.equal(wide[0, 1, :, :17], lone[0, 0])
        whole = noise.fill((5, 2, 4, 12), seeds[:2], noise.STEP, first_stream=0, kind=kind)
        head = noise.fill((2, 2, 4, 12), seeds[:2], noise.STEP, first_stream=0, kind=kind)
        tail = noise.fill((3, 2, 4, 12), seeds[:2], noise.STEP, first_stream=2, kind=kind)
        assert torch.equal(whole, torch.cat([head, tail]))
        base = noise.fill((1, 1, 4, 12), [31], noise.X_T, kind=kind)
        assert not (noise.fill((1, 1, 4, 12), [31], noise.STEP, kind=kind) == base).any()       # another domain
        assert not (noise.fill((1, 1, 4, 12), [32], noise.X_T, kind=kind) == base).any()        # another seed
        assert not (noise.fill((1, 1, 4, 12), [31 + (1 << 32)], noise.X_T, kind=kind) == base).any()    # the high word counts
        assert torch.equal(noise.fill((1, 2, 4, 12), 31, noise.X_T, kind=kind)[0, 1], base[0, 0])      # an int: every item


@pytest.mark.parametrize("shape", [(2, 2, 3, 9), (1, 2, 5, 16)], ids=["scalar", "vector"])
def test_affine_form(shape):
    """src_scale * src + scale * eps with the bitwise-known (uniform) eps: two products and a sum, each rounded once, of
    positive terms - at most 1.5 ulp of the result from the exact value; the bound is 2 ulp."""
    seeds, a, b = [41, HIGH], 0.8125, 0.3
    src = torch.rand(shape, device="cuda") + 0.5
    got = noise.fill(shape, seeds, noise.X_T, kind="uniform", src=src, src_scale=a, scale=b).cpu().numpy()
    eps = noise_ref.fill(shape, seeds, noise_ref.X_T, kind="uniform")
    want = float(np.float32(a)) * src.cpu().numpy().astype(np.float64) + float(np.float32(b)) * eps
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    assert float((np.abs(got.astype(np.float64) - want) / ulp).max()) <= 2.0
    # ... and it is bitwise what torch forms from the same eps in three kernels (the samplers' start mix)
    e32 = noise.fill(shape, seeds, noise.X_T, kind="uniform")
    assert torch.equal(torch.from_numpy(got).cuda(), a * src + b * e32)
    # in place: out may be src
    x = src.clone()
    noise.fill(shape, seeds, noise.X_T, kind="uniform", src=x, src_scale=a, scale=b, out=x)
    assert torch.equal(x.cpu(), torch.from_numpy(got))


def test_fill_is_capturable():
    shape, seeds = (3, 2, 5, 24), [51, HIGH]
    eager = noise.fill(shape, seeds, noise.STEP, first_stream=7)
    out = torch.zeros(shape, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        noise.fill(shape, seeds, noise.STEP, first_stream=7, out=out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


# ---- the samplers: seed= against the same tensors passed in -------------------------------------------------------------
def _x_t(seeds, b, m, t, domain=noise.X_T):
    return noise.fill((1, b, m, t), seeds, domain).view(b, 1, m, t)


def test_ddim_seed_equals_explicit_noise():
    from diffsinger_amd.diffusion import GaussianDiffusion
    set_hp(diff_accelerator="ddim", diff_speedup=100, K_step_infer=1000)
    d = GaussianDiffusion(32, 1, timesteps=1000, k_step=1000, backbone_type="wavenet", backbone_args=ARGS,
                          spec_min=[-8.0], spec_max=[0.0])
    load_synth(d.denoise_fn, synth_params("wavenet", 32, 1, ARGS, 60))
    d = d.cuda().eval()
    b, t, seeds = 2, 90, [61, HIGH]
    cond = dev(synth.synth_normal((b, t, 256), 3))
    with torch.no_grad():
        seeded = d(cond, infer=True, seed=seeds).clone()
        explicit = d(cond, infer=True, noise=_x_t(seeds, b, 32, t))
        assert torch.equal(seeded, explicit) and torch.isfinite(seeded).all()
        # item 1 of the batch drew what it draws alone; one int seeds every item alike
        alone = noise.fill((1, 1, 32, t), [HIGH], noise.X_T)
        assert torch.equal(_x_t(seeds, b, 32, t)[1], alone[0])
        assert not torch.equal(d(cond, infer=True, seed=62), seeded)
        # the variance pair's domains give other draws under the same seed
        assert not torch.equal(d(cond, infer=True, seed=seeds, noise_domain=noise.PITCH_X_T), seeded)
    d.denoise_fn.release_native()


def test_reflow_shallow_seed_equals_explicit_noise():
    from diffsinger_amd.diffusion import RectifiedFlow
    set_hp(use_shallow_diffusion=True, sampling_algorithm="euler", sampling_steps=6, T_start_infer=0.4)
    r = RectifiedFlow(32, 1, t_start=0.4, time_scale_factor=1000, backbone_type="wavenet", backbone_args=ARGS,
                      spec_min=[-12.0], spec_max=[0.0])
    load_synth(r.velocity_fn, synth_params("wavenet", 32, 1, ARGS, 61))
    r = r.cuda().eval()
    b, t, seeds = 2, 75, [71, HIGH]
    cond = dev(synth.synth_normal((b, t, 256), 5))
    src = dev((synth.synth_normal((b, t, 32), 6) * 1.5 - 6.0).astype(np.float32))
    with torch.no_grad():
        seeded = r(cond, src_spec=src, infer=True, seed=seeds).clone()
        explicit = r(cond, src_spec=src, infer=True, noise=_x_t(seeds, b, 32, t))
    assert torch.equal(seeded, explicit) and torch.isfinite(seeded).all()
    r.velocity_fn.release_native()


def test_ancestral_seed_equals_explicit_noise_and_reuses_its_graphs():
    """t_max = 60: two chunks (50 + 10 steps), the stream numbers running on across the boundary; the shallow start mix
    in the fill's own launch.  The step noise lives in one buffer, so the second run finds both chunks' graphs."""
    from diffsinger_amd.diffusion import GaussianDiffusion
    set_hp(use_shallow_diffusion=True, diff_speedup=1, K_step_infer=60)
    d = GaussianDiffusion(32, 1, timesteps=1000, k_step=60, backbone_type="wavenet", backbone_args=ARGS,
                          spec_min=[-12.0], spec_max=[0.0])
    load_synth(d.denoise_fn, synth_params("wavenet", 32, 1, ARGS, 62))
    d = d.cuda().eval()
    d.use_graph = True
    b, t, seeds = 2, 48, [81, HIGH]
    cond = dev(synth.synth_normal((b, t, 256), 7))
    src = dev((synth.synth_normal((b, t, 32), 8) * 1.5 - 6.0).astype(np.float32))
    cached = lambda: d.denoise_fn.stats()["graphs_cached"]  # noqa: E731
    with torch.no_grad():
        seeded = d(cond, src_spec=src, infer=True, seed=seeds).clone()
        graphs = cached()
        assert graphs == 2                                  # one per chunk
        again = d(cond, src_spec=src, infer=True, seed=seeds).clone()
        assert cached() == graphs and torch.equal(seeded, again)
        step = noise.fill((60, b, 32, t), seeds, noise.STEP).view(60, b, 1, 32, t)
        explicit = d(cond, src_spec=src, infer=True, noise=_x_t(seeds, b, 32, t), step_noise=step)
    assert torch.equal(seeded, explicit) and torch.isfinite(seeded).all()
    d.denoise_fn.release_native()


# ---- the vocoder ------------------------------------------------------------------------------------------------------
def test_vocoder_seed_equals_explicit_draws():
    from test_gpu_vocoder import OVER, build
    from test_gpu_vocoder_ragged import SAME
    gen, h, _ = build(OVER["small_sigma"], 470)             # every draw: phases, source noise, noise_sigma normals
    upp, c0, t = int(np.prod(h["upsample_rates"])), h["upsample_initial_channel"], 40
    rng = np.random.Generator(np.random.PCG64(5))
    mel = dev((synth.synth_normal((2, h["num_mels"], t), 471) * 3.0 - 11.0).astype(np.float32))
    f0 = dev((150.0 * 2.0 ** rng.uniform(-1, 2, (2, t))).astype(np.float32))
    with torch.no_grad():
        # dense: one seed, one draw of the phases
        s = 91
        seeded = gen(mel, f0, seed=s)
        ini = noise.fill((1, 1, 1, 9), [s], noise.VOC_PHASE, kind="uniform").view(9)
        src = noise.fill((1, 2, t * upp, 9), [s, s], noise.VOC_SOURCE)[0]
        pre = noise.fill((1, 2, c0, t), [s, s], noise.VOC_PRE)[0]
        assert torch.equal(seeded, gen(mel, f0, rand_ini=ini, noise=src, pre_noise=pre))
        assert torch.isfinite(seeded).all() and not torch.equal(seeded, gen(mel, f0, seed=s + 1))
        # ragged: one seed per item
        seeds, lens = [92, HIGH], [t, t - 3]
        ragged = gen(mel, f0, lengths=lens, seed=seeds)
        ini = noise.fill((1, 2, 1, 9), seeds, noise.VOC_PHASE, kind="uniform").view(2, 9)
        src = noise.fill((1, 2, t * upp, 9), seeds, noise.VOC_SOURCE)[0]
        pre = noise.fill((1, 2, c0, t), seeds, noise.VOC_PRE)[0]
        assert torch.equal(ragged, gen(mel, f0, lengths=lens, rand_ini=ini, noise=src, pre_noise=pre))
        # the shorter item is the one it is alone with its seed (the bound of test_gpu_vocoder_ragged)
        n = lens[1]
        alone = gen(mel[1:2, :, :n].contiguous(), f0[1:2, :n].contiguous(), seed=seeds[1])[0, 0]
        assert float((ragged[1, 0, :n * upp] - alone).abs().max()) <= SAME * max(1.0, float(alone.abs().max()))
        assert not ragged[1, 0, n * upp:].any()
    gen.release_native()


# ---- a project through the harness ------------------------------------------------------------------------------------
def test_harness_device_noise():
    from diffsinger_amd import harness
    from diffsinger_amd.hparams import hparams
    from test_gpu_vocoder import GOLDEN
    from test_gpu_vocoder_ragged import _project_harness
    saved = dict(hparams)
    try:
        h = _project_harness()
        segs = harness.load_ds(os.path.join(GOLDEN, "g11_segments.ds"))[:2]
        calls = []
        real = h._seed
        h._seed = lambda v: calls.append(v) or real(v)
        one = h.run_inference(segs, device_noise=True)
        again = h.run_inference(segs, device_noise=True)
        batched = h.run_inference(segs, device_noise=True, batch_size=2)
        assert calls == []                                  # torch's generators are never reseeded on this path
        assert one.tobytes() == again.tobytes()
        assert np.isfinite(one).all() and one.std() > 0
        # the bounds of the existing ragged-harness tests (the padded batch rounds differently through the encoder)
        assert batched.shape == one.shape and np.abs(batched - one).max() < 2e-2 and np.abs(batched - one).mean() < 1e-3
        assert batched.tobytes() == h.run_inference(segs, device_noise=True, batch_size=2).tobytes()
        other = h.run_inference([dict(s, seed=s["seed"] + 1) for s in segs], device_noise=True)
        assert not np.array_equal(other, one)
        default = h.run_inference(segs)                     # the default path: unchanged, reseeds per segment
        assert calls == [s["seed"] for s in segs] and not np.array_equal(default, one)
    finally:
        hparams.clear()
        hparams.update(saved)


def test_variance_harness_device_noise():
    """The variance pair under device_noise: no reseeding, the same completed project twice, and a ragged batch within the
    bound of test_gpu_variance's batched run (2e-3 of the curve: the padded batch rounds differently through the encoder)."""
    import copy
    import variance_cases as vc
    from diffsinger_amd.harness import SimplePhonemeTable
    from diffsinger_amd.hparams import hparams
    from diffsinger_amd.variance import DiffSingerVariance
    from diffsinger_amd.variance_harness import VarianceHarness
    saved = dict(hparams)
    try:
        hp = vc.case_hparams("word_reflow")
        hp.update(vc.HARNESS_HP, hidden_size=256, use_melody_encoder=True, num_spk=3, infer=True)
        hparams.clear()
        hparams.update(hp)
        table = SimplePhonemeTable(vc.HARNESS_PHONES)
        model = DiffSingerVariance(len(table))
        shapes = vc.sorted_param_shapes(model.named_parameters())
        model.load_state_dict({k: torch.from_numpy(v) for k, v in vc.synth_weights(shapes, 77).items()}, strict=False)
        model = model.cuda().eval()
        h = VarianceHarness(model, table, spk_map=vc.HARNESS_SPK, device="cuda")
        segs = vc.make_variance_segments()
        calls = []
        real = h._seed
        h._seed = lambda v: calls.append(v) or real(v)
        a = h.run_inference(copy.deepcopy(segs), seed=5, device_noise=True)[0]
        b = h.run_inference(copy.deepcopy(segs), seed=5, device_noise=True)[0]
        assert a == b and calls == []
        assert a != h.run_inference(copy.deepcopy(segs), seed=6, device_noise=True)[0]
        seen = []
        fmb = h.forward_model_batch
        h.forward_model_batch = lambda samples, noises, seeds=None: (seen.append((len(samples), seeds)), fmb(samples, noises, seeds=seeds))[1]
        c = h.run_inference(copy.deepcopy(segs), seed=5, batch_size=4, device_noise=True)[0]
        assert [n for n, _ in seen] == [2] and len(seen[0][1]) == 2         # one ragged launch, one seed per segment
        for one, bat in zip(a, c):
            assert one.keys() == bat.keys()
            for key in one:
                if key in ("ph_dur", "f0_seq", "energy", "breathiness") and isinstance(one[key], str):
                    x, y = np.array(one[key].split(), float), np.array(bat[key].split(), float)
                    assert x.shape == y.shape and np.abs(x - y).max() <= 2e-3 * max(1.0, np.abs(x).max()), key
                else:
                    assert one[key] == bat[key], key
        h.forward_model_batch = fmb
        h.run_inference(copy.deepcopy(segs), seed=5)        # the default path still reseeds torch, once per segment
        assert calls == [s.get("seed", 5) for s in segs]
        for m in model.modules():
            if hasattr(m, "release_native"):
                m.release_native()
    finally:
        hparams.clear()
        hparams.update(saved)


# ---- a plain-C caller --------------------------------------------------------------------------------------------------
def test_c_example_draws_the_oracle_values(tmp_path):
    from diffsinger_amd import _lib, schedule
    from diffsinger_amd.diffusion import _SamplerMixin
    exe = tmp_path / "c_abi_seeded"
    libdir = os.path.join(ROOT, "diffsinger_amd")
    cmd = ["gcc", "-std=c99", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "examples", "c_abi_seeded.c"), "-L" + libdir, "-ldsdenoise", "-L/opt/rocm/lib", "-lamdhip64",
           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)]
    subprocess.run(cmd, check=True)
    set_hp()
    args = dict(num_layers=4, num_channels=64, dilation_cycle_length=2)
    bsz, t_len, hidden, bins = 2, 150, 256, 32
    seeds = [0x123456789abcdef0, 42]
    net, params = make_backbone("wavenet", bins, 1, args, 45)
    with open(tmp_path / "weights.bin", "wb") as f:
        f.write(struct.pack("<i", len(params)))
        for name, arr in params.items():
            nb = name.encode()
            f.write(struct.pack("<i", len(nb)) + nb + struct.pack("<i", arr.ndim) + struct.pack(f"<{arr.ndim}q", *arr.shape))
            f.write(np.ascontiguousarray(arr, np.float32).tobytes())
    cond = synth.synth_normal((bsz, hidden, t_len), 1)
    with open(tmp_path / "inputs.bin", "wb") as f:
        f.write(struct.pack("<4i", bsz, t_len, hidden, bins) + struct.pack(f"<{bsz}Q", *seeds) + cond.tobytes())
    env = dict(os.environ, HIP_FORCE_DEV_KERNARG="1")
    res = subprocess.run([str(exe), str(tmp_path / "weights.bin"), str(tmp_path / "inputs.bin"), str(tmp_path / "out.bin")],
                         capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.splitlines()
    printed = [float(v) for v in lines[0].split()[1:]]
    want = noise_ref.draw(seeds[0], noise_ref.X_T, 0, bins, t_len)
    assert lines[0].startswith("x_T ") and len(printed) == 4
    assert np.abs(np.array(printed) - want[0, :4]).max() <= NORMAL_ATOL
    assert lines[1].startswith("sample checksum ") and np.isfinite(float(lines[1].split()[2]))
    # the whole x_T, and the sample against the Python side on the same seeds: the same library, the same draws
    got = np.fromfile(tmp_path / "out.bin", dtype=np.float32).reshape(2, bsz, 1, bins, t_len)
    assert np.array_equal(got[0], noise.fill((1, bsz, bins, t_len), seeds, noise.X_T).view(bsz, 1, bins, t_len).cpu().numpy())
    f32 = lambda v: float(np.float32(v))  # noqa: E731
    evals = []
    for k in range(6):
        terms = [(0, f32(np.float32(0.95) + np.float32(0.005) * np.float32(k))),
                 (_lib.DSD_SRC_MODEL, f32(np.float32(-0.15) + np.float32(0.02) * np.float32(k)))]
        if k < 5:
            terms.append((_lib.DSD_SRC_NOISE_BASE - k, f32(np.float32(0.1) - np.float32(0.015) * np.float32(k))))
        evals.append(schedule.Eval(0, 50.0 - 10.0 * k, [(0, terms)]))
    prog = schedule.Program(1, 0, evals, n_noise=6)
    runner = type("R", (_SamplerMixin,), {})()
    runner.denoise_fn = net
    x_t = noise.fill((1, bsz, bins, t_len), seeds, noise.X_T).view(bsz, 1, bins, t_len)
    step = noise.fill((6, bsz, bins, t_len), seeds, noise.STEP).view(6, bsz, 1, bins, t_len)
    want_samp = runner._run_program((prog,) + _lib.program_to_c(prog), dev(cond), x_t, noise=step, transpose=False).cpu().numpy()
    np.testing.assert_allclose(got[1], want_samp, rtol=0, atol=1e-5 * np.abs(want_samp).max())      # test_gpu_c_abi's bound
    net.release_native()
