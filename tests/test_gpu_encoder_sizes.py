"""-m gpu parity of the encoder family - the kernels of encoder_kernels.hip, the generic instantiations of gemm.hip they drive,
pack / unpack at the boundary - at the edges of what dsd_encoder_create / dsd_token_encoder_create accept, against the numpy
oracle (pinned to the reference at these sizes by G21, tests/test_encoder_sizes_host.py).  The cases and what each reaches:
tests/encoder_size_cases.py.  Every element of every output is compared, padding positions included.

Bounds: the acoustic encoder 2e-5 of the output range (test_gpu_encoder.py), the token encoder and the duration predictor 2e-4
of max |want|, max(1, .) for durations (test_gpu_variance.py).  The reference's own fp32 error against the float64 oracle on
these cases is 1e-7 .. 6e-6 (encoder_size_cases.FLOORS), so no case needs a bound of its own."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import encoder_size_cases as ec  # noqa: E402
from diffsinger_amd import synth  # noqa: E402
from diffsinger_amd.hparams import hparams  # noqa: E402
from gpu_util import check, dev, rel_err, set_hp  # noqa: E402
from oracle import variance as ovar  # noqa: E402
from test_gpu_encoder import build as build_acoustic  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    yield
    set_hp()


def run_acoustic(m, tokens, mel2ph, f0, extras):
    with torch.no_grad():
        return m(dev(tokens), dev(mel2ph), dev(f0), **{k: dev(v) for k, v in extras.items()})


# --------------------------------------------------------------------------- dsd_encode
@pytest.mark.parametrize("tag", list(ec.ACOUSTIC))
def test_acoustic_encoder_sizes_vs_oracle(tag):
    c = ec.ACOUSTIC[tag]
    m, params, _ = build_acoustic(ec.VOCAB, ec.acoustic_hp(tag), c["skw"], c["wseed"])
    for which in range(len(c["inputs"])):
        tokens, mel2ph, f0, extras = ec.acoustic_inputs(tag, which)
        want = ec.acoustic_oracle(tag, params, tokens, mel2ph, f0, extras)
        got = run_acoustic(m, tokens, mel2ph, f0, extras)
        err = check(got, want, ec.TOL_ACOUSTIC, what=(tag, which))
        print(f"{tag}[{which}] {tuple(got.shape)}: {err:.3g}")
    m.release_native()


# --------------------------------------------------------------------------- dsd_token_encode / dsd_predict_dur
def build_variance(c, melody=False):
    from diffsinger_amd.variance import DiffSingerVariance
    hp = ec.variance_hp(c, melody=melody)
    hparams.clear()
    hparams.update(hp, infer=True)
    model = DiffSingerVariance(ec.VAR_VOCAB)
    params = ec.variance_params(model, c["wseed"])
    res = model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=False)
    assert not res.unexpected_keys and not set(res.missing_keys) & set(params)
    return model.cuda().eval(), hp, params


def check_dur(got, want, what):
    rel_err(got, want)                  # into the parity record
    err = float(np.abs(got.cpu().numpy() - want).max() / max(1.0, np.abs(want).max()))
    print(f"{what} dur: {err:.3g}")
    assert err < ec.TOL_TOKEN, (what, err)


@pytest.mark.parametrize("tag", list(ec.VARIANCE))
def test_duration_predictor_sizes_vs_oracle(tag):
    c = ec.VARIANCE[tag]
    model, hp, params = build_variance(c)
    tokens, midi, ph2word, word_dur = ec.variance_inputs(c["lens"], c["wseed"] + 60)
    want_enc, want_dur = ovar.fs2_variance_forward(ovar.sub(params, "fs2."), hp, tokens, midi, ph2word, word_dur=word_dur)
    with torch.no_grad():
        enc, dur = model.fs2(dev(tokens), midi=dev(midi), ph2word=dev(ph2word), word_dur=dev(word_dur))
    assert (want_dur > 0).any()
    err = check(enc, want_enc, ec.TOL_TOKEN, what=(tag, "enc"))
    print(f"{tag} enc {tuple(enc.shape)}: {err:.3g}")
    check_dur(dur, want_dur, tag)
    if c["dur"][0] == 1:                # LayerNorm over one channel is beta * mask: the head sees nothing of the input
        p = ovar.sub(params, "fs2.dur_predictor.")
        v = np.float32(p["conv.0.3.bias"][0] * p["linear.weight"][0, 0] + p["linear.bias"][0])
        exact = np.where(tokens == 0, np.float32(0), np.maximum(np.exp(v, dtype=np.float32) - np.float32(1), 0)).astype(np.float32)
        assert np.abs(dur.cpu().numpy() - exact).max() <= 2e-6 * max(1.0, float(exact.max()))
    model.fs2.release_native()


def test_melody_encoder_hidden_96_vs_oracle():
    c = ec.MELODY
    model, hp, params = build_variance(c, melody=True)
    note_midi, note_rest, note_dur, glide = ec.melody_inputs(c["notes"], c["wseed"] + 60)
    want = ovar.melody_encoder(ovar.sub(params, "melody_encoder."), hp, note_midi, note_rest, note_dur, glide=glide)
    with torch.no_grad():
        got = model.melody_encoder(dev(note_midi), dev(note_rest), dev(note_dur), glide=dev(glide))
    check(got, want, ec.TOL_TOKEN, what="melody96")
    model.melody_encoder.release_native()


class TokenHandle:
    """dsd_token_encoder_create -> dsd_load_weight -> dsd_token_encode / dsd_predict_dur through the C ABI, for sizes the
    hparams cannot express (MelodyEncoder's out_dims is the model's hidden size)."""

    def __init__(self, params, hidden, heads, ks=3, out_dims=0, dur=None):
        from diffsinger_amd import _lib
        self._lib, self.lib = _lib, _lib.lib()
        chans, layers, kd = dur or (0, 0, 0)
        cfg = _lib.DsdTokenEncoderConfig(C.sizeof(_lib.DsdTokenEncoderConfig), hidden, 1, heads, ks, out_dims, layers, chans, kd,
                                         1.0, _lib.POS_ROPE, torch.cuda.current_device(), 0)
        self.h = C.c_void_p()
        rc = self.lib.dsd_token_encoder_create(C.byref(cfg), C.byref(self.h))
        assert rc == 0, self.lib.dsd_last_error(None)
        _lib.load_state_dict(self.h, params)
        self.hidden, self.out = hidden, out_dims or hidden

    def _call(self, fn, what, x, pad, out):
        mask = dev(pad.astype(np.uint8))
        xd = dev(x)
        stream = torch.cuda.current_stream().cuda_stream
        self._lib.check(self.h, fn(self.h, C.c_void_p(xd.data_ptr()), C.c_void_p(mask.data_ptr()), x.shape[0], x.shape[1],
                                   C.c_void_p(out.data_ptr()), C.c_void_p(stream)), what)
        torch.cuda.synchronize()
        return out

    def encode(self, embed, pad):
        out = torch.empty((*embed.shape[:2], self.out), device="cuda", dtype=torch.float32)
        return self._call(self.lib.dsd_token_encode, "dsd_token_encode", embed, pad, out)

    def predict_dur(self, cond, pad):
        out = torch.empty(cond.shape[:2], device="cuda", dtype=torch.float32)
        return self._call(self.lib.dsd_predict_dur, "dsd_predict_dur", cond, pad, out)

    def release(self):
        if self.h:
            self.lib.dsd_destroy(self.h)
            self.h = None


def token_inputs(lens, hidden, seed, scale=1.0):
    """Two [B, L, H] inputs (embedding, duration condition) that are NOT zero at padding, and the padding mask."""
    bsz, n = len(lens), max(lens)
    pad = np.arange(n)[None, :] >= np.asarray(lens)[:, None]
    embed = (synth.synth_normal((bsz, n, hidden), seed) * np.float32(scale)).astype(np.float32)
    cond = (synth.synth_normal((bsz, n, hidden), seed + 1) * np.float32(scale)).astype(np.float32)
    return embed, cond, pad


@pytest.mark.parametrize("out_dims", ec.OUT_DIMS["out_dims"])
def test_out_proj_sizes_vs_oracle(out_dims):
    c = ec.OUT_DIMS
    params = synth.synth_state_dict(ec.token_encoder_shapes(c["hidden"], c["heads"], out_dims=out_dims), seed=c["wseed"])
    embed, _, pad = token_inputs(c["lens"], c["hidden"], c["wseed"] + 60)
    want = ec.token_oracle(params, embed, pad, c["heads"], out_dims)
    t = TokenHandle(params, c["hidden"], c["heads"], out_dims=out_dims)
    got = t.encode(embed, pad)
    assert tuple(got.shape) == (len(c["lens"]), max(c["lens"]), out_dims or c["hidden"])
    check(got, want, ec.TOL_TOKEN, what=("out_dims", out_dims))
    t.release()


# --------------------------------------------------------------------------- a handle's history
# "nan": dirt only - every float input NaN (tokens, mel2ph and the masks stay valid; encoder_kernels.hip uses the floats only
# arithmetically), at a's shape so that the next call reuses the arena untouched; its own NaN result is not compared
HISTORY = [("a", (70, 41)), ("b", (5,)), ("big", (70, 41)), ("a", (70, 41)), ("c", (130, 77, 1)), ("nan", (70, 41)), ("a", (70, 41))]


def test_acoustic_results_do_not_depend_on_the_handles_history():
    """enc_workspace keeps its arena while (B, L) repeats and re-lays it out otherwise; whatever a call left in the padding
    columns, in e_mid or in a re-laid-out arena never reaches a later result: each equals a fresh handle's, bit for bit."""
    tag = "h96_k3"
    c = ec.ACOUSTIC[tag]
    inputs = {}
    for k, (name, lens) in enumerate(HISTORY):
        if name not in inputs:
            tokens, mel2ph, f0 = ec.padded_inputs(lens, [2 * n + 3 for n in lens], 3000 + k)
            if name == "big":
                f0 = f0 * np.float32(1e3)
            if name == "nan":
                f0 = np.full_like(f0, np.nan)
            inputs[name] = (tokens, mel2ph, f0, {})
    old, _, _ = build_acoustic(ec.VOCAB, ec.acoustic_hp(tag), c["skw"], c["wseed"])
    for k, (name, _) in enumerate(HISTORY):
        got = run_acoustic(old, *inputs[name])
        if name == "nan":
            assert torch.isnan(got).any()
            continue
        fresh, _, _ = build_acoustic(ec.VOCAB, ec.acoustic_hp(tag), c["skw"], c["wseed"])
        want = run_acoustic(fresh, *inputs[name])
        fresh.release_native()
        assert torch.isfinite(want).all()
        assert torch.equal(got, want), (k, name, float((got - want).abs().max()))
    old.release_native()


def test_token_encoder_results_do_not_depend_on_the_handles_history():
    """The same on a token encoder with a duration predictor, dsd_predict_dur interleaved with dsd_token_encode (they share the
    arena); the `big` inputs are 1e3 times larger and not zero at padding."""
    hidden, heads, dur = 96, 2, (100, 2, 3)
    params = synth.synth_state_dict(ec.token_encoder_shapes(hidden, heads, dur=dur), seed=2208)
    inputs = {}
    for k, (name, lens) in enumerate(HISTORY):
        if name not in inputs:
            inputs[name] = token_inputs(lens, hidden, 3100 + 2 * k, scale=1e3 if name == "big" else np.nan if name == "nan" else 1.0)
    old = TokenHandle(params, hidden, heads, dur=dur)
    for k, (name, _) in enumerate(HISTORY):
        embed, cond, pad = inputs[name]
        got_e, got_d = old.encode(embed, pad), old.predict_dur(cond, pad)
        if name == "nan":
            assert torch.isnan(got_e).any()         # (the duration head ends in a clamp, which may swallow its NaN)
            continue
        fresh = TokenHandle(params, hidden, heads, dur=dur)
        want_d = fresh.predict_dur(cond, pad)
        fresh.release()
        fresh = TokenHandle(params, hidden, heads, dur=dur)
        want_e = fresh.encode(embed, pad)
        fresh.release()
        assert torch.isfinite(want_e).all() and torch.isfinite(want_d).all()
        assert torch.equal(got_e, want_e), (k, name, "enc", float((got_e - want_e).abs().max()))
        assert torch.equal(got_d, want_d), (k, name, "dur", float((got_d - want_d).abs().max()))
    old.release()
