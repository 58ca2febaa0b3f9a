"""-m gpu: model files end to end.  For each of the eight kinds of handle that have weights, wrapper A (seeded weights) runs as
it does today and its section goes into a file; wrapper B - the same configuration, OTHER seeded weights - is put on a handle
that dsd_model_create made from that file (modelfile.attach), and must then give A's output exactly: the same library, the
same bytes, the same launch plan, so torch.equal and no tolerance.  (Every family here is held to run-to-run equality by its
own tests: test_gpu_fused / _lynx_small / _width / _encoder_sizes / _vocoder_configs / _rmvpe / _hnsep / _mel.)  Small
shapes: B = 2, T = 40 frames or 0.3 s of audio.  Then the mel section, attach's and dsd_model_create's refusals, and
examples/c_abi_model.c from one file to a waveform in a process without Python."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import encoder_size_cases as ec  # noqa: E402
import vocoder_config_cases as vcc  # noqa: E402
import width_cases as wc  # noqa: E402
from diffsinger_amd import _lib, modelfile, synth  # noqa: E402
from diffsinger_amd.hparams import hparams  # noqa: E402
from gpu_util import dev, load_synth, set_hp  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BSZ, T_LEN = 2, 40


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    yield
    set_hp()


def through_file(tmp_path, name, a, b, run, native_of=lambda m: m):
    """A's section -> file -> B attached; -> (A's output, B's output before, B's output after)"""
    with torch.no_grad():
        want, before = run(a), run(b)
    path = tmp_path / f"{name}.dsdm"
    modelfile.write(path, [modelfile.section_of(name, native_of(a))], {"kind": name})
    with modelfile.open(path) as f:
        modelfile.attach(native_of(b), f, name, "cuda")
    with torch.no_grad():           # the file is closed: the handle holds its own copy
        got = run(b)
    torch.cuda.synchronize()
    return want, before, got


def assert_same(want, before, got, what):
    want, before, got = [x if isinstance(x, (tuple, list)) else (x,) for x in (want, before, got)]
    for k, (w, b0, g) in enumerate(zip(want, before, got)):
        w, b0, g = [torch.as_tensor(x) for x in (w, b0, g)]
        assert torch.isfinite(w).all() and float(w.abs().max()) > 0, (what, k)
        assert not torch.equal(b0, w), (what, k, "B's own weights give A's output: the case shows nothing")
        print(f"{what}[{k}] {tuple(w.shape)}: max |B - A| = {float((g - w).abs().max()):.3g}")
        assert torch.equal(g, w), (what, k)


def assert_backbone_clean(a, b):
    """B runs on the installed handle, uploaded nothing, and its Python mirror holds the file's values"""
    assert b._weights_dirty is False and b._handle is not None
    sa, sb = a.state_dict(), b.state_dict()
    for k in a._native_state():
        assert torch.equal(sa[k].cpu(), sb[k].cpu()), k


# ------------------------------------------------------------------------------------------------ one case per kind
def backbone_pair(kind, in_dims, n_feats, args, seed):
    from diffsinger_amd.backbones import build_backbone
    set_hp()
    nets = []
    for s in (seed, seed + 1):
        params = synth.synth_state_dict(synth.backbone_param_shapes(kind, in_dims, n_feats, hidden_size=256, **args), seed=s)
        nets.append(load_synth(build_backbone(in_dims, n_feats, kind, args), params))
    return nets


@pytest.mark.parametrize("kind,in_dims,n_feats,args,seed", [
    ("wavenet", 32, 1, dict(num_layers=4, num_channels=64, dilation_cycle_length=2), 2921),
    ("lynxnet",) + wc.LYNX_EVALS["c90"][:3] + (2922,),       # 90 channels: the handle runs at 96, the file holds true-width tensors
], ids=["wavenet", "lynxnet_c90"])
def test_denoisers(tmp_path, kind, in_dims, n_feats, args, seed):
    a, b = backbone_pair(kind, in_dims, n_feats, args, seed)
    x = dev(synth.synth_normal((BSZ, n_feats, in_dims, T_LEN), 11))
    cond = dev(synth.synth_normal((BSZ, 256, T_LEN), 12))
    t = dev(np.array([400.0, 30.5], np.float32))
    assert_same(*through_file(tmp_path, kind, a, b, lambda m: m(x, t, cond)), kind)
    assert_backbone_clean(a, b)
    if kind == "lynxnet":
        assert b.stats()["weight_bytes"] == a.stats()["weight_bytes"]
    a.release_native(), b.release_native()


def test_aux_decoder(tmp_path):
    from diffsinger_amd.aux_decoder import build_aux_decoder
    hsz, m, args, _, _, wseed = wc.AUX["a75"]
    set_hp()
    decs = []
    for s in (wseed, wseed + 1000):
        shapes = synth.convnext_param_shapes(hsz, m, num_channels=args["num_channels"], num_layers=args["num_layers"],
                                             kernel_size=args["kernel_size"])
        decs.append(load_synth(build_aux_decoder(hsz, m, "convnext", dict(args)), synth.synth_state_dict(shapes, seed=s)))
    a, b = decs
    cond = dev(synth.synth_normal((BSZ, T_LEN, hsz), 21))
    assert_same(*through_file(tmp_path, "aux", a, b, lambda d: d(cond, infer=True)), "aux a75")
    assert_backbone_clean(a, b)
    a.release_native(), b.release_native()


def test_acoustic_encoder(tmp_path):
    from test_gpu_encoder import build
    tag = "h96_k3"
    c = ec.ACOUSTIC[tag]
    a, _, _ = build(ec.VOCAB, ec.acoustic_hp(tag), c["skw"], c["wseed"])
    b, _, _ = build(ec.VOCAB, ec.acoustic_hp(tag), c["skw"], c["wseed"] + 1000)
    tokens, mel2ph, f0, _ = ec.acoustic_inputs(tag, "g21")         # [2, 24] tokens over [2, 40] frames
    assert mel2ph.shape == (BSZ, T_LEN)
    assert_same(*through_file(tmp_path, "fs2", a, b, lambda m: m(dev(tokens), dev(mel2ph), dev(f0))), "fs2 h96_k3")
    assert_backbone_clean(a, b)
    a.release_native(), b.release_native()


def test_token_encoder_and_duration_predictor(tmp_path):
    """The handle of FastSpeech2Variance loads `encoder.*` and `dur_predictor.*`; its embeddings are torch parameters that
    feed dsd_cond_assemble and are no part of the section, so B keeps A's embeddings and differs in what the handle holds."""
    from test_gpu_encoder_sizes import build_variance
    c = ec.VARIANCE["d100"]
    ma, _, _ = build_variance(c)
    mb, _, _ = build_variance(dict(c, wseed=c["wseed"] + 1000))
    a, b = ma.fs2, mb.fs2
    native = set(a._native_state())
    res = b.load_state_dict({k: v for k, v in a.state_dict().items() if k not in native}, strict=False)
    assert set(res.missing_keys) == native and not res.unexpected_keys
    tokens, midi, ph2word, word_dur = ec.variance_inputs(ec.G21_VARIANCE_LENS, c["wseed"] + 61)

    def run(m):
        return m(dev(tokens), midi=dev(midi), ph2word=dev(ph2word), word_dur=dev(word_dur))
    assert_same(*through_file(tmp_path, "variance_fs2", a, b, run), "token encoder d100")
    assert_backbone_clean(a, b)
    a.release_native(), b.release_native()


def test_vocoder(tmp_path):
    from diffsinger_amd.vocoder import Generator
    tag = min(vcc.CASES, key=lambda t: sum(int(np.prod(s)) for s in synth.nsf_hifigan_param_shapes(vcc.config(t)).values()))
    h = vcc.config(tag)
    gens = []
    for seed in (vcc.CASES[tag]["wseed"], 2923):
        gens.append(load_synth(Generator(h), synth.synth_state_dict(synth.nsf_hifigan_param_shapes(h), seed=seed, gain=vcc.GAIN)))
    a, b = gens
    i = {k: dev(v) for k, v in vcc.make_inputs(h, BSZ, T_LEN).items()}

    def run(g):
        return g(i["mel"], i["f0"], rand_ini=i["rand_ini"], noise=i["noise"], pre_noise=i["pre_noise"])
    assert_same(*through_file(tmp_path, "vocoder", a, b, run), f"vocoder {tag}")
    assert_backbone_clean(a, b)
    a.release_native(), b.release_native()


def test_rmvpe(tmp_path):
    from diffsinger_amd.pitch import RMVPE
    a = RMVPE(synth.rmvpe_state_dict(seed=2924, with_tf=True, **synth.RMVPE_SMALL))
    b = RMVPE(synth.rmvpe_state_dict(seed=2925, with_tf=True, **synth.RMVPE_SMALL))
    mel = dev((synth.synth_normal((BSZ, 128, T_LEN), 31) * 2.0 - 6.0).astype(np.float32))
    assert_same(*through_file(tmp_path, "rmvpe", a, b, lambda pe: pe.mel2hidden(mel)), "rmvpe small")
    assert set(b._native_tensors()) == set(a._native_tensors())


def test_hnsep(tmp_path):
    from diffsinger_amd.hnsep import HnSep
    import mel_ref
    cfg = dict(synth.HNSEP_SMALL)
    a = HnSep(synth.hnsep_state_dict(cfg, seed=2926), cfg)
    b = HnSep(synth.hnsep_state_dict(cfg, seed=2927), cfg)
    x = torch.from_numpy(np.stack([mel_ref.waveform(2928 + k, 4800, 16000).astype(np.float32) for k in range(BSZ)])[:, None])
    assert_same(*through_file(tmp_path, "hnsep", a, b, lambda sp: sp.predict_from_audio(x)), "hnsep small")


def test_mel_section(tmp_path):
    """A mel section has no tensors: dsd_model_create stops after dsd_mel_create, and dsd_mel_analyze on that handle gives
    what the STFT wrapper's own handle gives."""
    from diffsinger_amd.mel import STFT
    import mel_ref
    args = (16000, 40, 512, 400, 128, 40, 7600)
    a, b = STFT(*args), STFT(*args)
    y = dev(np.stack([mel_ref.waveform(2930 + k, 4800, 16000).astype(np.float32) for k in range(BSZ)]))
    want = a.get_mel(y, keyshift=1.5)
    path = tmp_path / "mel.dsdm"
    modelfile.write(path, [modelfile.section_of("mel", a)])
    with modelfile.open(path) as f:
        assert f.sections[0].kind == 6 and f.sections[0].n_tensors == 0
        modelfile.attach(b, f, "mel", "cuda")
        installed = b._handles[torch.cuda.current_device()].value
        with pytest.raises(ValueError, match="hop_size"):
            modelfile.attach(STFT(16000, 40, 512, 400, 160, 40, 7600), f, "mel", "cuda")
    got = b.get_mel(y, keyshift=1.5)
    assert b._handles[torch.cuda.current_device()].value == installed
    assert torch.isfinite(want).all() and torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ refusals
def test_attach_refuses_another_config_and_create_a_missing_tensor(tmp_path):
    from diffsinger_amd.backbones import build_backbone
    args = dict(num_layers=2, num_channels=64, dilation_cycle_length=2)
    a, _ = backbone_pair("wavenet", 32, 1, args, 2931)
    sec = modelfile.section_of("denoiser", a)
    dropped = "residual_layers.1.dilated_conv.bias"
    fewer = sec._replace(name="fewer", tensors={k: v for k, v in sec.tensors.items() if k != dropped})
    path = tmp_path / "two.dsdm"
    modelfile.write(path, [sec, fewer])
    lib = _lib.lib()
    with modelfile.open(path) as f:
        other = build_backbone(32, 1, "wavenet", dict(args, num_layers=3)).cuda()
        with pytest.raises(ValueError, match="differ in num_layers"):
            modelfile.attach(other, f, "denoiser", "cuda")
        assert other._handle is None and other._weights_dirty
        from diffsinger_amd.mel import STFT
        with pytest.raises(ValueError, match="DsdConfig"):
            modelfile.attach(STFT(), f, "denoiser", "cuda")
        h = C.c_void_p(1)
        rc = lib.dsd_model_create(f._f, f.index("fewer"), 0, C.byref(h))
        msg = lib.dsd_last_error(None).decode()
        assert rc == _lib.DSD_ESTATE and not h.value, (rc, msg)          # no handle is left
        assert dropped in msg and 'section "fewer"' in msg, msg
        with pytest.raises(_lib.NativeLibraryError, match=dropped):
            f.create("fewer")
        # a tensor the model does not know: the failing dsd_load_weight is named
        extra = sec._replace(name="extra", tensors=dict(sec.tensors, **{"no.such.weight": np.zeros(3, np.float32)}))
        modelfile.write(tmp_path / "extra.dsdm", [extra])
        with modelfile.open(tmp_path / "extra.dsdm") as g:
            rc = lib.dsd_model_create(g._f, 0, 0, C.byref(h))
            msg = lib.dsd_last_error(None).decode()
            assert rc == _lib.DSD_ENOTFOUND and not h.value and 'tensor "no.such.weight"' in msg, (rc, msg)
            assert lib.dsd_model_create(g._f, 0, 99, C.byref(h)) == _lib.DSD_EINVAL and "device 99" in lib.dsd_last_error(None).decode()
        # the whole section still opens and runs
        hp = f.create("denoiser")
        assert hp.value
        lib.dsd_destroy(hp)
    a.release_native()


# ------------------------------------------------------------------------------------------------ plain C
def test_c_example_from_one_file_to_a_waveform(tmp_path):
    """examples/c_abi_model.c (gcc -std=c99, no Python / torch in the process) on a file with a WaveNet and a mini_nsf
    vocoder against the Python wrappers on the same inputs.  Equality: both sides run the same library on the same weight
    bytes - the file also carries the SinusoidalPosEmb table the wrapper uploads, the one thing test_gpu_c_abi.py has to
    allow 2e-6 for - and nothing in either kernel path depends on the process."""
    from diffsinger_amd.vocoder import Generator
    exe = tmp_path / "c_abi_model"
    libdir = os.path.join(ROOT, "diffsinger_amd")
    cmd = ["gcc", "-std=c99", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "examples", "c_abi_model.c"), "-L" + libdir, "-ldsdenoise", "-L/opt/rocm/lib", "-lamdhip64",
           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)]
    subprocess.run(cmd, check=True)
    bins, hidden = 32, 256
    net, _ = backbone_pair("wavenet", bins, 1, dict(num_layers=4, num_channels=64, dilation_cycle_length=2), 2941)
    h = vcc.over_default(**dict(vcc.CASES["mini_two"]["over"], num_mels=bins))
    assert h["mini_nsf"] and vcc.accepts(h)[0]
    gen = load_synth(Generator(h), synth.synth_state_dict(synth.nsf_hifigan_param_shapes(h), seed=2942, gain=vcc.GAIN))
    upp = int(np.prod(h["upsample_rates"]))
    meta = {"timesteps": "1000", "hop_size": str(upp), "audio_sample_rate": str(h["sampling_rate"]), "phonemes": "AP SP a i u"}
    modelfile.write(tmp_path / "model.dsdm", [modelfile.section_of("denoiser", net), modelfile.section_of("vocoder", gen)], meta)
    cond = synth.synth_normal((BSZ, hidden, T_LEN), 41)
    x = synth.synth_normal((BSZ, 1, bins, T_LEN), 42)
    t = np.array([400.0, 30.5], np.float32)
    f0 = vcc.make_inputs(h, BSZ, T_LEN)["f0"]
    with open(tmp_path / "inputs.bin", "wb") as f:
        f.write(struct.pack("<2i", BSZ, T_LEN) + cond.tobytes() + x.tobytes() + t.tobytes() + f0.tobytes())
    env = dict(os.environ, HIP_FORCE_DEV_KERNARG="1")
    res = subprocess.run([str(exe), str(tmp_path / "model.dsdm"), str(tmp_path / "inputs.bin"), str(tmp_path / "out.bin")],
                         capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 0, res.stderr
    out = res.stdout
    n_den = sum(int(np.asarray(v).size) for v in modelfile.section_of("denoiser", net).tensors.values())
    assert f"api v{_lib.lib().dsd_api_version()}  2 sections  4 metadata entries" in out
    assert f'section 0: "denoiser" kind 0, {len(net.state_dict()) + 1} tensors, {n_den} floats' in out
    assert f'section 1: "vocoder" kind 4, {len(gen.state_dict())} tensors' in out
    for k, v in meta.items():
        assert f'meta "{k}" = "{v}"' in out
    assert f"denoiser: in_dims {bins} hidden_size {hidden}  vocoder: num_mels {bins} hop {upp}" in out
    got = np.fromfile(tmp_path / "out.bin", dtype=np.float32)
    n_x = BSZ * bins * T_LEN
    assert got.size == n_x + BSZ * T_LEN * upp
    with torch.no_grad():
        want_den = net(dev(x), dev(t), dev(cond))
        want_wav = gen(want_den[:, 0], dev(f0))
    want_den, want_wav = want_den.cpu().numpy(), want_wav.cpu().numpy()
    got_den, got_wav = got[:n_x].reshape(want_den.shape), got[n_x:].reshape(want_wav.shape)
    assert np.isfinite(want_wav).all() and np.abs(want_wav).max() > 0
    print(f"C vs Python: denoised {np.abs(got_den - want_den).max():.3g}, waveform {np.abs(got_wav - want_wav).max():.3g}")
    assert np.array_equal(got_den, want_den)
    assert np.array_equal(got_wav, want_wav)
    net.release_native(), gen.release_native()
