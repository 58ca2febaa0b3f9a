"""-m gpu: mel analysis (dsd_mel_analyze, diffsinger_amd.mel.STFT) against the reference's fp32 STFT.get_mel (G17) and
the float64 restatement in tests/mel_ref.py.

Tolerances are stated from measurement.  The reference's own fp32 CPU path sits within FLOOR_LOG = 7.6e-5 in log-mel and
FLOOR_LIN = 2.8e-7 of the item's peak mel (linear) of the float64 restatement on the G17 cases; the HIP result must stay
within twice that floor of the float64 oracle, and within floor + bar of G17 itself.  Ragged items must be bit-identical
to their lone calls.  On the 5-minute clips the floor is the reference's own error on those clips (measured with
tests/golden/make_golden_mel.py's setup: 1.3e-4 in log-mel, 2.9e-7 linear)."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mel_ref  # noqa: E402
from diffsinger_amd import synth  # noqa: E402
from gpu_util import dev, rel_err  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FLOOR_LOG, FLOOR_LIN = 7.6e-5, 2.8e-7       # measured: reference fp32 vs float64 over the G17 cases (max)
TOL_LOG, TOL_LIN = 2 * FLOOR_LOG, 2 * FLOOR_LIN
# the 5-minute clips: the reference's fp32 path measured on these very clips (25 839 frames: a longer tail than G17's)
FLOOR_LOG_5MIN = {0.0: 1.30e-4, -3.7: 1.26e-4}
_MEASURED = os.environ.get("DSD_MEL_ERRORS_LOG")     # optional: a JSON-lines file that collects the measured errors


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"


def stft_of(c):
    from diffsinger_amd.mel import STFT
    return STFT(c["sr"], c["n_mels"], c["n_fft"], c["win_size"], c["hop"], c["fmin"], c["fmax"])


def errors(got, y, c, ks, sp, tag):
    """(log-mel error, linear error / peak) of a HIP result against the float64 oracle; appended to $DSD_MEL_ERRORS_LOG
    when that is set (the DESIGN table)."""
    got = got.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(got) else got
    lin = mel_ref.get_mel(y, c, ks, sp, linear=True)
    e_log = float(np.abs(got - np.log(np.maximum(lin, 1e-5))).max())
    e_lin = float(np.abs(np.exp(got) - np.maximum(lin, 1e-5)).max() / lin.max())
    _record(dict(case=tag, log=e_log, lin_peak=e_lin))
    return e_log, e_lin


def _record(row):
    if _MEASURED:
        with open(_MEASURED, "a") as f:
            f.write(json.dumps(row) + "\n")


def g17_cases():
    z = np.load(os.path.join(GOLDEN, "g17_mel.npz"))
    return [(i, z[f"c{i}_meta"], z[f"c{i}_mel"]) for i in range(int(z["n_cases"]))]


@pytest.mark.parametrize("i", range(9))
def test_g17_case(i):
    _, meta, want = g17_cases()[i]
    seed, n, ks, sp, small = meta
    c = mel_ref.SMALL if small else mel_ref.PROD
    y = mel_ref.waveform(int(seed), int(n), c["sr"])
    got = stft_of(c).get_mel(dev(y)[None], keyshift=float(ks), speed=float(sp))[0]
    assert tuple(got.shape) == want.shape
    e_log, e_lin = errors(got, y, c, float(ks), float(sp), f"g17_{i}")
    assert e_log <= TOL_LOG and e_lin <= TOL_LIN, (e_log, e_lin)
    assert float((got.cpu() - torch.from_numpy(want)).abs().max()) <= FLOOR_LOG + TOL_LOG


@pytest.mark.parametrize("ks", [0.0, -3.7])
def test_five_minute_clip(ks):
    c = mel_ref.PROD
    y = mel_ref.waveform(51 + int(ks), 13_230_000, c["sr"])
    got = stft_of(c).get_mel(dev(y)[None], keyshift=ks)[0]
    assert got.shape[1] == mel_ref.num_frames(len(y), 2048, 2048, 512, ks, 1)
    e_log, e_lin = errors(got, y, c, ks, 1.0, f"5min_ks{ks}")
    assert e_log <= 2 * FLOOR_LOG_5MIN[ks] and e_lin <= TOL_LIN, (e_log, e_lin)


def test_ragged_batch_matches_lone_calls():
    c, sp, ks = mel_ref.PROD, 1.1, 0.0
    rng = np.random.default_rng(7)
    secs = [1, 60, 2.5, 17, 800, 33, 5, 1.2, 48, 9, 3.3, 26, 12, 7.7, 41, 2]       # 800: samples, T_b = 1 at speed 1.1
    lens = [int(s) if s == 800 else int(s * c["sr"]) for s in secs]
    waves = [mel_ref.waveform(100 + b, n, c["sr"]) for b, n in enumerate(lens)]
    stft = stft_of(c)
    assert stft.num_frames(800, ks, sp) == 1
    # a padded batch with junk (not zeros) past every item's end, through the raw entry point
    pad = np.full((len(lens), max(lens)), 0.0, np.float32)
    for b, w in enumerate(waves):
        pad[b, : len(w)] = w
        pad[b, len(w):] = rng.uniform(-1, 1, max(lens) - len(w)).astype(np.float32) * 0.9
    frames = [stft.num_frames(n, ks, sp) for n in lens]
    yb = dev(pad)
    out = torch.full((len(lens), c["n_mels"], max(frames)), float("nan"), device=yb.device)
    with torch.no_grad():
        stft._analyze(yb, lens, ks, sp, out)
    listed = stft.get_mel_ragged([dev(w) for w in waves], keyshift=ks, speed=sp)
    for b, w in enumerate(waves):
        lone = stft.get_mel(dev(w)[None], keyshift=ks, speed=sp)[0]
        assert torch.equal(out[b, :, : frames[b]], lone), b
        assert torch.equal(listed[b], lone), b
        if b in (0, 3, 4, 13):
            e_log, e_lin = errors(lone, w, c, ks, sp, f"ragged_{b}")
            assert e_log <= TOL_LOG and e_lin <= TOL_LIN, (b, e_log, e_lin)


def test_output_strides_and_determinism():
    c = mel_ref.SMALL
    y = np.stack([mel_ref.waveform(s, 30000, c["sr"]) for s in (3, 4)])
    stft = stft_of(c)
    a = stft.get_mel(dev(y), keyshift=1.5, speed=0.9)
    b = stft.get_mel(dev(y), keyshift=1.5, speed=0.9)
    t = a.shape[2]
    btm = torch.empty(2, t, c["n_mels"], device=a.device)
    stft.get_mel(dev(y), keyshift=1.5, speed=0.9, out=btm.transpose(1, 2))
    assert torch.equal(a, b)
    assert torch.equal(a, btm.transpose(1, 2))
    # a strided input view (every other row of a larger buffer) is read through its stride
    big = torch.zeros(4, 30000, device=a.device)
    big[0::2] = dev(y)
    assert torch.equal(stft.get_mel(big[0::2], keyshift=1.5, speed=0.9), a)


def test_errors_and_handle_kinds():
    import ctypes as C
    from diffsinger_amd import _lib
    c = mel_ref.PROD
    stft = stft_of(c)
    with pytest.raises(ValueError):
        stft.get_mel(torch.zeros(1, 700, device="cuda"))              # reflect pad 768 >= L
    lib = _lib.lib()
    h = stft._handle(torch.device("cuda"))
    assert lib.dsd_finalize_weights(h) == -2
    assert lib.dsd_vocode(h, C.c_void_p(1), 1, 1, 1, 1, 1, C.c_void_p(1), None, None, None, C.c_void_p(1), None) == -2
    assert lib.dsd_set_lengths(h, None, 0, None) == -2
    st = _lib.DsdStats()
    assert lib.dsd_get_stats(h, C.byref(st)) == -2
    assert lib.dsd_kernel_timing(h, 1) == -2
    assert lib.dsd_set_precision(h, 0) == -2
    # and the mel entry point on another kind of handle
    from test_gpu_vocoder import OVER, build
    gen, _, _ = build(OVER["small_rb2"], 5)
    vh = gen.native_handle(torch.device("cuda"))
    y = torch.zeros(1, 4096, device="cuda")
    out = torch.empty(1, 128, 8, device="cuda")
    assert lib.dsd_mel_analyze(vh, C.c_void_p(y.data_ptr()), 1, 4096, 4096, None, 0.0, 1.0, C.c_void_p(out.data_ptr()),
                               1024, 8, 1, None) == -2
    gen.release_native()


def test_get_mel_torch_dropin():
    from diffsinger_amd.mel import get_mel_torch
    y = mel_ref.waveform(11, 30000, 44100)
    got = get_mel_torch(y, 44100, keyshift=0.5, speed=1.05)
    assert got.shape == (mel_ref.num_frames(30000, 2048, 2048, 512, 0.5, 1.05), 128) and got.dtype == np.float32
    e_log, e_lin = errors(got.T, y, mel_ref.PROD, 0.5, 1.05, "get_mel_torch")
    assert e_log <= TOL_LOG and e_lin <= TOL_LIN


def test_resynthesis_through_vocoder():
    """wav -> STFT.get_mel -> Generator.forward (synthetic G10 weights) against the oracle vocoder on the oracle mel."""
    from oracle import vocoder as ov
    from test_gpu_vocoder import build
    c = mel_ref.PROD
    gen, h, params = build({}, 430)
    y = mel_ref.waveform(12, 20000, c["sr"])
    mel = stft_of(c).get_mel(dev(y)[None])
    want_mel = mel_ref.get_mel(y, c)[None].astype(np.float32)
    t_len = mel.shape[2]
    rng = np.random.Generator(np.random.PCG64(430))
    f0 = (220.0 * 2.0 ** rng.uniform(-0.5, 0.5, (1, t_len))).astype(np.float32)
    rand_ini = rng.random(9).astype(np.float32)
    noise = synth.synth_normal((1, t_len * 512, 9), 431)
    pre = synth.synth_normal((1, h["upsample_initial_channel"], t_len), 432)
    with torch.no_grad():
        got = gen(mel, dev(f0), rand_ini=dev(rand_ini), noise=dev(noise), pre_noise=dev(pre))
    want = ov.generator_forward(params, h, want_mel, f0, rand_ini, noise, pre)
    err = rel_err(got, want)
    _record(dict(case="resynthesis", rel=err))
    assert err < 5e-5, err          # the vocoder suite's own tolerance; measured 2.4e-6
    gen.release_native()
