"""-m gpu: what lets a C process render a multi-speaker project in one ragged, seeded batch.

  * dsd_vocode_seeded (Generator.forward_seeded) against the path it replaces - three dsd_noise_fill calls, then dsd_vocode /
    dsd_vocode_ragged - bit for bit, and every ragged item against its lone seeded call within SAME;
  * dsd_acoustic_spk_mix / dsd_variance_spk_mix against a numpy fp32 restatement that adds in index order (bit for bit) and
    against torch's own expression;
  * dsd_acoustic_set_lengths: every item of a padded batch against its lone run through the same C calls, within ALONE_TOL;
  * examples/c_abi_project.c against the same chain through the Python bindings.

Every figure is printed before it is asserted."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import cacoustic_cases as cc
import deploy_cases as dc
from diffsinger_amd import _lib, modelfile, synth, track
from diffsinger_amd import noise as seeded
from diffsinger_amd.hparams import hparams
from gpu_util import dev
from test_gpu_cacoustic import World, c_condition, same
from test_gpu_cvariance import World as VarWorld
from test_gpu_deploy import ALONE_TOL, close
from test_gpu_vocoder import GAIN, OVER, build
from test_gpu_vocoder_ragged import SAME

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESTATE = -1, -2

# OVER has no source of one or of four harmonics (dim 1: rand_ini unused; dim 4: exactly one Philox block): built as
# tests/vocoder_config_cases.py builds its harm0 / harm15, on the small two-block configuration
CONFIGS = dict(OVER, harm0=dict(OVER["small_rb2"], harmonic_num=0), harm3=dict(OVER["small_rb2"], harmonic_num=3))
# dim 9 at production width; dim 9 small; pre-noise with a SineGen source; no draws; pre-noise alone; dim 1; dim 4
TAGS = ["default", "small_rb2", "small_sigma", "mini_small", "mini_sigma", "harm0", "harm3"]
SEEDS = [2026, 7, 0x123456789ABCDEF0, 2 ** 64 - 1]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    yield
    hparams.clear()
    hparams.update(hidden_size=256)


# ------------------------------------------------------------------------------------------------ the seeded vocoder
def voc_inputs(h, lens, t_len, seed):
    """a padded batch as tests/test_gpu_vocoder_ragged.py's: junk, not zeros, past every item's end"""
    bsz = len(lens)
    rng = np.random.Generator(np.random.PCG64(seed))
    mel = (synth.synth_normal((bsz, h["num_mels"], t_len), seed + 1) * 3.0 - 11.0).astype(np.float32)
    f0 = (150.0 * 2.0 ** rng.uniform(-1, 2, (bsz, t_len))).astype(np.float32)
    f0[:, ::7] = 0.0
    for b, n in enumerate(lens):
        mel[b, :, n:] = 40.0
        f0[b, n:] = 3000.0
    return dev(mel), dev(f0)


def draws(gen):
    return not gen.mini_nsf or bool(gen.noise_sigma and gen.noise_sigma > 0)


def differing(got, want):
    return int((got.contiguous().view(torch.int32) != want.contiguous().view(torch.int32)).sum())


@pytest.mark.parametrize("t_len", [5, 70])
@pytest.mark.parametrize("tag", TAGS)
def test_seeded_dense_is_fill_then_vocode_bit_for_bit(tag, t_len):
    """B = 2.  T = 5: a partial Philox block in the pre-noise, a source length that is no multiple of 256."""
    gen, h, _ = build(CONFIGS[tag], 510)
    mel, f0 = voc_inputs(h, [t_len, t_len], t_len, 511)
    seeds = SEEDS[:2]
    with torch.no_grad():
        if draws(gen):
            want = gen(mel, f0, seed=seeds)             # _seeded_draws: three dsd_noise_fill calls, then dsd_vocode
            got = gen.forward_seeded(mel, f0, seeds)
            other = gen.forward_seeded(mel, f0, seeds[::-1])
            assert not torch.equal(other, got)          # the seeds are read
        else:
            want = gen(mel, f0)                         # nothing to draw: dsd_vocode with NULLs
            got = gen.forward_seeded(mel, f0, None)
            assert torch.equal(gen.forward_seeded(mel, f0, seeds), got)
    n = differing(got, want)
    print(f"{tag}, T = {t_len}: {n} of {got.numel()} samples differ from fill-then-vocode (max |wav| {float(want.abs().max()):.3f})")
    assert n == 0 and torch.equal(got, want) and float(want.abs().max()) > 1e-3
    gen.release_native()


@pytest.mark.parametrize("tag", TAGS)
def test_seeded_ragged_is_fill_then_vocode_and_items_alone(tag):
    gen, h, _ = build(CONFIGS[tag], 520)
    t_len, lens = 70, [70, 1, 23, 33]
    upp = int(np.prod(h["upsample_rates"]))
    mel, f0 = voc_inputs(h, lens, t_len, 521)
    seeds = SEEDS if draws(gen) else None
    with torch.no_grad():
        want = gen(mel, f0, lengths=lens, seed=SEEDS) if draws(gen) else gen(mel, f0, lengths=lens)
        got = gen.forward_seeded(mel, f0, seeds, lengths=lens)
        n = differing(got, want)
        print(f"{tag}: {n} of {got.numel()} samples differ from fill-then-vocode-ragged")
        assert n == 0 and torch.equal(got, want)
        for b, m in enumerate(lens):
            alone = gen.forward_seeded(mel[b:b + 1, :, :m], f0[b:b + 1, :m], None if seeds is None else [seeds[b]])[0, 0]
            scale = max(1.0, float(alone.abs().max()))
            err = float((got[b, 0, :m * upp] - alone).abs().max())
            print(f"{tag}: item {b} ({m} frames) against its lone seeded call: max |err| {err:.3e}, bound {SAME * scale:.3e}")
            assert err <= SAME * scale, (tag, b, m)
            assert not got[b, 0, m * upp:].any()
    gen.release_native()


def test_seeds_cross_one_launch_chunk():
    """B = 65, T = 2: the seeds travel 64 per launch, so item 64 rides in the second launch of both seeded kernels and of the
    phase draw - dense (one phase row from seeds[0]) and ragged (a row per item)."""
    gen, h, _ = build(CONFIGS["small_sigma"], 530)
    lens = [2 - (b % 3 == 1) for b in range(65)]
    mel, f0 = voc_inputs(h, lens, 2, 531)
    seeds = [1000003 * b + 17 for b in range(65)]
    with torch.no_grad():
        for lengths in (None, lens):
            kw = {} if lengths is None else dict(lengths=lengths)
            want = gen(mel, f0, seed=seeds, **kw)
            got = gen.forward_seeded(mel, f0, seeds, **kw)
            n = differing(got, want)
            print(f"B = 65, {'ragged' if lengths else 'dense'}: {n} of {got.numel()} samples differ; item 64 max |wav| {float(got[64].abs().max()):.3f}")
            assert n == 0 and float(got[64].abs().max()) > 1e-3
        moved = list(seeds)
        moved[64] += 1
        assert not torch.equal(gen.forward_seeded(mel, f0, moved, lengths=lens)[64], got[64])       # item 64's own seed is read
    gen.release_native()


@pytest.mark.parametrize("lens", [None, [70, 1, 23, 33]])
def test_seeded_call_replays_from_a_graph(lens):
    gen, h, _ = build(CONFIGS["small_sigma"], 540)
    bsz = 4 if lens else 2
    mel, f0 = voc_inputs(h, lens or [70, 70], 70, 541)
    seeds = SEEDS[:bsz]
    upp = int(np.prod(h["upsample_rates"]))
    out = torch.empty((bsz, 1, 70 * upp), device="cuda")
    with torch.no_grad():
        eager = gen.forward_seeded(mel, f0, seeds, lengths=lens)           # the warm-up: sizes the workspace, uploads the tile lists
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out.copy_(gen.forward_seeded(mel, f0, seeds, lengths=lens))
        for k in range(2):
            out.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            n = differing(out, eager)
            print(f"replay {k}: {n} of {out.numel()} samples differ from the eager call")
            assert n == 0
    gen.release_native()


def test_seeded_vocoder_refusals():
    """nothing launched: wav keeps its NaN fill"""
    lib = _lib.lib()
    gen, h, _ = build(CONFIGS["small_sigma"], 550)
    mini, _, _ = build(CONFIGS["mini_small"], 551)
    bsz, t_len = 2, 9
    upp = int(np.prod(h["upsample_rates"]))
    mel, f0 = voc_inputs(h, [t_len] * bsz, t_len, 552)
    wav = torch.full((bsz, t_len * upp), float("nan"), device="cuda")
    voc, mini_h = gen.native_handle(mel.device), mini.native_handle(mel.device)
    seeds = (C.c_uint64 * bsz)(3, 4)

    def args(**over):
        a = _lib.DsdVocodeSeededArgs()
        a.struct_size, a.B, a.T, a.vocoder = C.sizeof(a), bsz, t_len, voc
        a.mel, (a.stride_b, a.stride_m, a.stride_t) = mel.data_ptr(), mel.stride()
        a.f0, a.seeds, a.wav_out = f0.data_ptr(), seeds, wav.data_ptr()
        for k, v in over.items():
            setattr(a, k, v)
        return a
    lens = lambda *v: (C.c_int32 * bsz)(*v)  # noqa: E731
    refusals = [(args(vocoder=None), "null argument"), (args(mel=None), "null argument"), (args(f0=None), "null argument"),
                (args(wav_out=None), "null argument"), (args(seeds=None), "null seeds"), (args(B=0), "B and T must be positive"),
                (args(T=0), "B and T must be positive"), (args(T=-3), "B and T must be positive"),
                (args(lengths=lens(9, 0)), "lengths[1] = 0"), (args(lengths=lens(10, 9)), "lengths[0] = 10"),
                (args(lengths=lens(9, -1)), "lengths[1] = -1"), (args(stride_m=3, stride_t=2), "contiguous along T"),
                (args(struct_size=80), "struct_size")]
    for a, word in refusals:
        rc = lib.dsd_vocode_seeded(C.byref(a), None)
        msg = lib.dsd_last_error(None if word == "struct_size" else a.vocoder).decode()     # the struct is refused before its handle is read
        print(f"{word!r}: {rc} {msg}")
        assert rc == EINVAL and msg.startswith("dsd_vocode_seeded:") and word in msg, (word, rc, msg)
    # a handle of another kind: the entry check's message, on that handle
    w_hp = cc.build_model("aux_reflow", cuda=True)[0]
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "m.dsdm")
        cc.pack(path, w_hp)
        from diffsinger_amd.cacoustic import Acoustic
        with modelfile.open(path) as f:
            ac = Acoustic(f, cc.PREFIX, "cuda")
    for which, what in ((_lib.DSD_AC_DENOISER, "a "), (_lib.DSD_AC_AUX, "an aux decoder"), (_lib.DSD_AC_FS2, "an acoustic encoder")):
        other = ac.handle(which)
        rc = lib.dsd_vocode_seeded(C.byref(args(vocoder=other)), None)
        msg = lib.dsd_last_error(other).decode()
        print(f"{what}: {rc} {msg}")
        assert rc == ESTATE and msg.startswith("dsd_vocode_seeded: this handle is " + what), (rc, msg)
    torch.cuda.synchronize()
    assert torch.isnan(wav).all()
    # and what is in order runs: seeds may be NULL exactly where nothing is drawn
    mmel, mf0 = voc_inputs(mini.h, [t_len] * bsz, t_len, 553)
    mwav = torch.full((bsz, t_len * mini.upp), float("nan"), device="cuda")
    ok = args(vocoder=mini_h, seeds=None, mel=mmel.data_ptr(), f0=mf0.data_ptr(), wav_out=mwav.data_ptr())
    ok.stride_b, ok.stride_m, ok.stride_t = mmel.stride()
    assert lib.dsd_vocode_seeded(C.byref(ok), None) == 0
    assert lib.dsd_vocode_seeded(C.byref(args()), None) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(wav).all() and torch.isfinite(mwav).all()
    ac.close()
    from test_gpu_deploy import release
    release(w_hp)
    gen.release_native()
    mini.release_native()


# ------------------------------------------------------------------------------------------------ speaker mixes
def mix_ref(table, ids, values, normalize):
    """the specification restated in numpy fp32: every product, sum and division rounded on its own, sums in index order"""
    v = np.asarray(values, np.float32)
    w = v
    if normalize:
        s = v[..., 0].copy()
        for n in range(1, v.shape[2]):
            s = (s + v[..., n]).astype(np.float32)
        with np.errstate(invalid="ignore", divide="ignore"):
            w = (v / s[..., None]).astype(np.float32)
    acc = None
    for n in range(v.shape[2]):
        t = (w[:, :, n, None] * table[ids[:, n]][:, None, :]).astype(np.float32)
        acc = t if acc is None else (acc + t).astype(np.float32)
    return acc, w


def table_of(model):
    (name, p), = [(k, q) for k, q in model.named_parameters() if k.endswith("spk_embed.weight")]
    return p.detach()


def mix_cases(rng, num_spk, lengths):
    """(N, rows, normalize, ids [3, N], values [3, rows, N]): N in {1, 2, 5}, rows in {1} + lengths, both normalize"""
    for n in (1, 2, 5):
        for rows in sorted({1} | set(lengths)):
            for normalize in (0, 1):
                ids = rng.integers(0, num_spk, (3, n)).astype(np.int32)
                values = rng.random((3, rows, n)).astype(np.float32) + np.float32(0.0625)
                if n > 1:
                    values[1, :, 1] = 0.0               # a padding speaker
                yield n, rows, normalize, ids, values


def check_mix(obj, table, n, rows, normalize, ids, values, unaligned=False):
    hidden = table.shape[1]
    want, w = mix_ref(table.cpu().numpy(), ids, values, normalize)
    out = None
    if unaligned:                                       # the scalar path: H = 64 in every builder, so an out pointer off by 4 bytes
        store = torch.full((3 * rows * hidden + 4,), float("nan"), device="cuda")
        out = store[1:1 + 3 * rows * hidden].view(3, rows, hidden)
        assert out.data_ptr() % 16 == 4
    got = obj.spk_mix(ids, dev(values), normalize=bool(normalize), out=out)
    what = f"N = {n}, rows = {rows}, normalize = {normalize}{', unaligned out' if unaligned else ''}"
    same(got, dev(want), what + ": against the numpy restatement")
    if unaligned:
        assert torch.isnan(store[:1]).all() and torch.isnan(store[-3:]).all()
    tw = dev(w)                                         # torch's expression on the same weights
    mixed = torch.sum(table[torch.from_numpy(ids.astype(np.int64)).cuda()][:, None] * tw.unsqueeze(3), dim=2)
    if n <= 2:                                          # addition commutes: any order gives these bits
        if normalize and n == 2:
            v = dev(values)
            tw = v / v.sum(dim=2, keepdim=True)
            mixed = torch.sum(table[torch.from_numpy(ids.astype(np.int64)).cuda()][:, None] * tw.unsqueeze(3), dim=2)
        same(got, mixed, what + ": against torch.sum(table[ids] * values.unsqueeze(3), dim=2)")
    else:       # two summation orders of the same N products: first-order bound 2 (N - 1) 2^-24 sum_n |w_n E_n| per element
        mag = np.abs(w[:, :, :, None].astype(np.float64) * table.cpu().numpy()[ids][:, None].astype(np.float64)).sum(axis=2)
        bound = 2 * (n - 1) * 2.0 ** -24 * mag
        err = np.abs(got.cpu().numpy().astype(np.float64) - mixed.cpu().numpy().astype(np.float64))
        print(f"{what}: against torch, max err / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
        assert (err <= bound).all()
    return got, mixed


def test_acoustic_spk_mix_and_its_condition(tmp_path):
    w = World("batch", tmp_path)
    try:
        a, model = w.a, w.model
        table = table_of(model)
        assert tuple(table.shape) == (2, dc.HIDDEN)
        raw = cc.batch_inputs()
        inp = {k: dev(x) for k, x in raw.items() if k != "lengths"}
        rng = np.random.Generator(np.random.PCG64(2560))
        count = 0
        with torch.no_grad():
            for n, rows, normalize, ids, values in mix_cases(rng, 2, (33, 70)):
                got, mixed = check_mix(a, table, n, rows, normalize, ids, values)
                count += 1
                if rows == 33:
                    check_mix(a, table, n, rows, normalize, ids, values, unaligned=True)
                elif n <= 2:        # rows 1 or T = 70: what the condition stage takes, against the same call fed torch's mix
                    cond, aux = c_condition(a, dict(inp, spk_embed=got), spk="spk_embed")
                    want_cond, want_aux = c_condition(a, dict(inp, spk_embed=mixed), spk="spk_embed")
                    same(cond, want_cond, f"condition from the mix (N = {n}, rows = {rows}, normalize = {normalize})")
                    same(aux, want_aux, "aux_mel from the mix")
        assert count == 18
    finally:
        w.close()


def test_variance_spk_mix_and_its_stages(tmp_path):
    import cvariance_cases as cv
    w = VarWorld("word", tmp_path)
    try:
        v, model = w.v, w.model
        table = table_of(model)
        raw = cv.batch_inputs("word")
        inp = {k: dev(x) for k, x in raw.items() if k != "lengths"}
        n_ph, t_len = cv.BATCH_SHAPE["n_ph"], cv.BATCH_SHAPE["t_len"]
        rng = np.random.Generator(np.random.PCG64(2570))
        names = v.names
        with torch.no_grad():
            enc, masks = v.encode(inp["tokens"], word_div=inp["word_div"], word_dur=inp["word_dur"], languages=inp["languages"])
            for n, rows, normalize, ids, values in mix_cases(rng, 2, (n_ph, t_len)):
                got, mixed = check_mix(v, table, n, rows, normalize, ids, values)
                if n > 2:
                    continue
                if rows in (1, n_ph):
                    same(v.dur(enc, masks, inp["ph_midi"], spk_embed=got), v.dur(enc, masks, inp["ph_midi"], spk_embed=mixed),
                         f"ph_dur_pred from the mix (N = {n}, rows = {rows}, normalize = {normalize})")
                if rows in (1, t_len):
                    curves = {k: inp["var_" + k] for k in names}
                    same(v.cond(enc, inp["ph_dur"], inp["pitch"], curves, inp["var_retake"], spk_embed=got),
                         v.cond(enc, inp["ph_dur"], inp["pitch"], curves, inp["var_retake"], spk_embed=mixed),
                         f"variance_cond from the mix (N = {n}, rows = {rows}, normalize = {normalize})")
    finally:
        w.close()


def test_spk_mix_refusals(tmp_path):
    """every DSD_EINVAL of section 2, nothing launched: out keeps its NaN fill"""
    lib = _lib.lib()
    wb, wf, wp = World("batch", tmp_path), World("frozen", tmp_path), World("aux_reflow", tmp_path)
    wv, wn = VarWorld("word", tmp_path), VarWorld("k_one", tmp_path)
    try:
        rows, n = 4, 2
        values = torch.full((1, rows, n), 0.5, device="cuda")
        out = torch.full((1, rows, dc.HIDDEN), float("nan"), device="cuda")

        def args(ids=(0, 1), **over):
            a = _lib.DsdSpkMixArgs()
            keep = None if ids is None else (C.c_int32 * len(ids))(*ids)
            a.struct_size, a.B, a.rows, a.N, a.ids = C.sizeof(a), 1, rows, n, keep
            a.values, a.normalize, a.out = values.data_ptr(), 1, out.data_ptr()
            for k, v in over.items():
                setattr(a, k, v)
            return a, keep
        cases = [(args(struct_size=40), "struct_size"), (args(ids=(0, 2)), "ids[1] = 2"), (args(ids=(-1, 0)), "ids[0] = -1"),
                 (args(N=0), "must be positive"), (args(rows=0), "must be positive"), (args(B=0), "B = 0"), (args(ids=None), "NULL ids"),
                 (args(values=None), "NULL ids, values"), (args(out=None), "values or out")]
        total = 0
        for (entry, name), objs in (((lib.dsd_acoustic_spk_mix, "dsd_acoustic_spk_mix"), (wb.a._a, wp.a._a, wf.a._a)),
                                    ((lib.dsd_variance_spk_mix, "dsd_variance_spk_mix"), (wv.v._v, wn.v._v, None))):
            for (a, keep), word in cases:
                rc = entry(objs[0], C.byref(a), None)
                msg = lib.dsd_last_error(None).decode()
                assert rc == EINVAL and msg.startswith(name + ":") and word in msg, (name, word, rc, msg)
                total += 1
            assert entry(objs[0], None, None) == EINVAL and b"NULL args" in lib.dsd_last_error(None)
            a, keep = args()
            assert entry(objs[1], C.byref(a), None) == EINVAL and b"use_spk_id = 0" in lib.dsd_last_error(None)
            if objs[2] is not None:
                assert entry(objs[2], C.byref(a), None) == EINVAL and b"frozen_spk_embed" in lib.dsd_last_error(None)
            total += 3
        torch.cuda.synchronize()
        print(f"{total} refusals")
        assert torch.isnan(out).all()
        for entry, obj in ((lib.dsd_acoustic_spk_mix, wb.a._a), (lib.dsd_variance_spk_mix, wv.v._v)):
            a, keep = args()
            assert entry(obj, C.byref(a), None) == 0
            torch.cuda.synchronize()
            assert torch.isfinite(out).all()
            out.fill_(float("nan"))
    finally:
        for w in (wb, wf, wp, wv, wn):
            w.close()


# ------------------------------------------------------------------------------------------------ lengths through the object
LENS = [70, 23, 33]


def ragged_inputs(tag, seed):
    """B = 3, T = 70, LENS: every item's durations total its length; item 1 has a padding token with a duration (masked away);
    f0 and every curve hold junk past each item's end."""
    hp, _ = cc.case_hparams(tag)
    n_ph, t_len = 6, 70
    rng = np.random.Generator(np.random.PCG64(seed))
    tokens = rng.integers(1, dc.VOCAB, (3, n_ph)).astype(np.int64)
    durations = np.zeros((3, n_ph), dtype=np.int64)
    durations[0] = dc._split(rng, LENS[0], n_ph)
    tokens[1, 2] = 0
    durations[1, [0, 1, 3, 4, 5]] = dc._split(rng, LENS[1], 5)
    durations[1, 2] = 9
    tokens[2, -2:] = 0
    durations[2, :4] = dc._split(rng, LENS[2], 4)
    out = dict(tokens=tokens, durations=durations, f0=(220.0 * 2.0 ** rng.uniform(-1, 1, (3, t_len))).astype(np.float32))
    out["f0"][:, 5:8] = 0.0
    junk = dict(f0=3000.0)
    if hp.get("use_energy_embed"):
        out["var_energy"], junk["var_energy"] = rng.uniform(-60, -10, (3, t_len)).astype(np.float32), 99.0
    if hp.get("use_tension_embed"):
        out["var_tension"], junk["var_tension"] = rng.uniform(-5, 5, (3, t_len)).astype(np.float32), -99.0
    if hp.get("use_key_shift_embed"):
        out["gender"], junk["gender"] = rng.uniform(-1.3, 1.3, (3, t_len)).astype(np.float32), -7.0
    if hp.get("use_speed_embed"):
        out["velocity"], junk["velocity"] = rng.uniform(0.3, 2.4, (3, t_len)).astype(np.float32), 50.0
    if hp.get("use_spk_id"):
        out["spk_embed"] = rng.standard_normal((3, t_len, dc.HIDDEN)).astype(np.float32)
    if hp.get("use_lang_id"):
        out["languages"] = rng.integers(1, hp["num_lang"] + 1, (3, n_ph)).astype(np.int64)
    for b, n in enumerate(LENS):
        for k, v in junk.items():
            out[k][b, n:] = v
    return {k: dev(v) for k, v in out.items()}


def run_chain(a, inp, p, sl, t_len, x_of, step_noise=None, flags=0):
    """condition -> start -> sample through the C calls on items `sl` cut to `t_len` frames; x_of(source, sl, t_len) -> x"""
    cond, aux = c_condition(a, inp, sl=sl, t_len=t_len)
    x = x_of(aux, sl, t_len)
    sn = None if step_noise is None else step_noise[:, sl, :, :, :t_len].contiguous()
    mel = a.sample(p, cond, x, step_noise=sn, flags=flags)
    return dict(condition=cond, aux_mel=aux, mel=mel)


def against_alone(a, inp, p, batch, x_of, step_noise, what):
    a.set_lengths(None)
    for b, n in enumerate(LENS):
        lone = run_chain(a, inp, p, slice(b, b + 1), n, x_of, step_noise)
        for k in ("condition", "aux_mel", "mel"):
            close(batch[k][b:b + 1, :n], lone[k].cpu().numpy(), ALONE_TOL, True, f"{what}: item {b} ({n} frames) {k} against its lone run")
    return lone


@pytest.mark.parametrize("tag", ["batch", "base10"])
def test_lengths_through_the_acoustic_object(tmp_path, tag):
    """the shallow-DDPM case with every embedding, and a reflow case (a log10 mel: the in-place scale runs too)"""
    w = World(tag, tmp_path)
    try:
        a = w.a
        inp = ragged_inputs(tag, 2580)
        m, seeds = dc.M_BINS, [11, 12, 13]
        noise = dev(synth.synth_normal((3, 1, m, 70), 2581))
        p = a.plan(0.3, 4)
        assert p.start == _lib.DSD_AC_START_MIX and p.n_step_noise == 0
        print(f"{tag}: plan start {p.start}, t_max {p.t_max}, speedup {p.speedup}, t_start {p.t_start}")

        def passed_in(source, sl, t_len):
            return a.start(p, source=source, noise=noise[sl, :, :, :t_len].contiguous())

        def drawn_in_place(source, sl, t_len):
            x = a.start(p, source=source, noise=None)
            bsz = x.shape[0]
            flat = x.view(1, bsz, m, t_len)
            seeded.fill((1, bsz, m, t_len), seeds[sl], seeded.X_T, src=flat, src_scale=p.src_scale, scale=p.noise_scale, out=flat)
            return x
        everything = slice(0, 3)
        with torch.no_grad():
            dense = run_chain(a, inp, p, everything, 70, passed_in)
            a.set_lengths(LENS)
            ragged = run_chain(a, inp, p, everything, 70, passed_in)
            against_alone(a, inp, p, ragged, passed_in, None, f"{tag}, x passed in")
            # not vacuous: without the lengths the padding frames' condition (junk f0, junk curves) reaches item 1's last frames
            # through the aux decoder's convolutions.  Item 1 (23 frames: its end falls inside the first 32-frame tile)
            lone = run_chain(a, inp, p, slice(1, 2), LENS[1], passed_in)
            gap = float((dense["aux_mel"][1:2, LENS[1] - 3:LENS[1]] - lone["aux_mel"][:, -3:]).abs().max())
            bound = ALONE_TOL * max(1.0, float(lone["aux_mel"].abs().max()))
            print(f"{tag}: the dense batch's aux mel differs from item 1's lone run by {gap:.3e} in its last 3 frames (bound {bound:.3e})")
            assert gap > bound
            gap = float((dense["mel"][1:2, :LENS[1]] - lone["mel"]).abs().max())
            print(f"{tag}: and its mel by {gap:.3e}")
            assert gap > ALONE_TOL * max(1.0, float(lone["mel"].abs().max()))
            # NULL: the dense result, bit for bit
            again = run_chain(a, inp, p, everything, 70, passed_in)
            for k in dense:
                same(again[k], dense[k], f"{tag}: {k} after set_lengths(NULL)")
            # x drawn by dsd_noise_fill in place: element (m, t) of x_T does not depend on T
            a.set_lengths(LENS)
            drawn = run_chain(a, inp, p, everything, 70, drawn_in_place)
            assert not torch.equal(drawn["mel"], ragged["mel"])
            # DSD_SAMPLE_GRAPH once: the graph key holds the lengths
            graphed = run_chain(a, inp, p, everything, 70, drawn_in_place, flags=_lib.DSD_SAMPLE_GRAPH)
            for b, n in enumerate(LENS):
                close(graphed["mel"][b, :n], drawn["mel"][b, :n].cpu().numpy(), ALONE_TOL, True,
                      f"{tag}: item {b}'s mel through DSD_SAMPLE_GRAPH against the eager run")
            against_alone(a, inp, p, drawn, drawn_in_place, None, f"{tag}, x drawn in place")
            against_alone(a, inp, p, graphed, drawn_in_place, None, f"{tag}, x drawn in place, DSD_SAMPLE_GRAPH")
    finally:
        w.close()


def test_lengths_with_the_ancestral_sampler(tmp_path):
    """4 steps of p_sample: the step noise of a padded batch under lengths"""
    w = World("ancestral", tmp_path)
    try:
        a = w.a
        inp = ragged_inputs("ancestral", 2590)
        m = dc.M_BINS
        noise = dev(synth.synth_normal((3, 1, m, 70), 2591))
        step_noise = dev(synth.synth_normal((4, 3, 1, m, 70), 2592))
        p = a.plan(0.004, 4)
        assert (p.t_max, p.speedup, p.n_step_noise) == (4, 1, 4)

        def passed_in(source, sl, t_len):
            return a.start(p, source=source, noise=noise[sl, :, :, :t_len].contiguous())
        with torch.no_grad():
            a.set_lengths(LENS)
            ragged = run_chain(a, inp, p, slice(0, 3), 70, passed_in, step_noise)
            against_alone(a, inp, p, ragged, passed_in, step_noise, "ancestral")
    finally:
        w.close()


def test_set_lengths_rules(tmp_path):
    lib = _lib.lib()
    w = World("batch", tmp_path)
    try:
        a = w.a
        inp = ragged_inputs("batch", 2600)
        p = a.plan(0.3, 4)
        noise = dev(synth.synth_normal((3, 1, dc.M_BINS, 70), 2601))
        with torch.no_grad():
            a.set_lengths(LENS)
            cond, aux = c_condition(a, inp)
            x = a.start(p, source=aux, noise=noise)
            # a stage call at another B: DSD_ESTATE, from each of the three
            for call in (lambda: c_condition(a, inp, sl=slice(0, 2)), lambda: a.start(p, source=aux[:2], noise=noise[:2]),
                         lambda: a.sample(p, cond[:2], x[:2])):
                with pytest.raises(_lib.NativeLibraryError, match=r"\(-2\).*gave 3 lengths but this call runs a batch of 2"):
                    call()
            # a length above that call's T: DSD_EINVAL
            for call in (lambda: c_condition(a, inp, t_len=41), lambda: a.start(p, source=aux[:, :41], noise=noise[..., :41]),
                         lambda: a.sample(p, cond[:, :41], x[..., :41])):
                with pytest.raises(_lib.NativeLibraryError, match=r"\(-1\).*exceeds T = 41"):
                    call()
            # a negative length: DSD_EINVAL, and the lengths set before stay
            bad = (C.c_int32 * 3)(70, -1, 33)
            assert lib.dsd_acoustic_set_lengths(a._a, bad, 3, None) == EINVAL and b"lengths[1] = -1 is negative" in lib.dsd_last_error(None)
            assert lib.dsd_acoustic_set_lengths(a._a, bad, 0, None) == EINVAL and b"B = 0" in lib.dsd_last_error(None)
            with pytest.raises(_lib.NativeLibraryError, match=r"\(-2\)"):
                c_condition(a, inp, sl=slice(0, 2))
            same(c_condition(a, inp)[1], aux, "aux_mel after the refused calls")
            a.set_lengths(None)
            c_condition(a, inp, sl=slice(0, 2))         # dense again: any B
    finally:
        w.close()


# ------------------------------------------------------------------------------------------------ the C example
def test_c_example_renders_the_project(tmp_path):
    """examples/c_abi_project.c compiled and run on a packed multi-speaker model with a SineGen vocoder section, noise_sigma > 0.
    Its sums against the same chain through the Python bindings (every sum equal), and every segment against the same segment
    rendered alone through the same calls (mel within ALONE_TOL, samples within SAME)."""
    import vocoder_config_cases as vcc
    from diffsinger_amd.vocoder import Generator
    from gpu_util import load_synth
    h = vcc.over_default(**dict(OVER["small_sigma"], num_mels=dc.M_BINS))
    assert not h["mini_nsf"] and h["noise_sigma"] > 0 and vcc.accepts(h)[0]
    gen = load_synth(Generator(h), synth.synth_state_dict(synth.nsf_hifigan_param_shapes(h), seed=2821, gain=GAIN))
    w = World("batch", tmp_path, extra=[modelfile.section_of("vocoder", gen)])
    try:
        exe, pcm_path = tmp_path / "c_abi_project", tmp_path / "project.s16"
        libdir = os.path.join(ROOT, "diffsinger_amd")
        subprocess.run(["gcc", "-std=c99", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "c_abi_project.c"), "-L" + libdir, "-ldsdenoise", "-L/opt/rocm/lib", "-lamdhip64",
                        "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True, timeout=300)
        r = subprocess.run(["timeout", "-k", "10", "120", str(exe), w.path, cc.PREFIX, str(pcm_path)], capture_output=True, text=True, timeout=150)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
        got = {}
        for line in r.stdout.splitlines():
            parts = line.split() or [""]
            if parts[0] == "sum":
                got[parts[1]] = float(parts[2])
            elif parts[0] in ("total", "peak", "checksum"):
                got[parts[0]] = float(parts[1])
        # the example's own inputs, restated (examples/c_abi_project.c)
        a = w.a
        bsz, n_ph, t_len, steps, depth = 3, 6, 48, 4, 0.375
        lens, seeds = [48, 17, 30], [2026, 7, 0x123456789ABCDEF]
        upp, rate = gen.upp, gen.sampling_rate
        vocab, num_lang, num_spk = a.cfg.vocab_size, a.cfg.num_lang, a.cfg.num_spk
        tokens = torch.tensor([[1 + (3 * i + b) % (vocab - 1) for i in range(n_ph)] for b in range(bsz)], device="cuda")
        tokens[1, 2] = 0
        tokens[1, 4:] = 0
        tokens[2, 5] = 0
        languages = torch.tensor([[1 + (i + b) % num_lang for i in range(n_ph)] for b in range(bsz)], device="cuda")
        durations = torch.tensor([[10, 8, 6, 12, 7, 5], [5, 4, 9, 8, 0, 0], [6, 6, 6, 6, 6, 0]], device="cuda")
        t = torch.arange(t_len, device="cuda")[None]
        b = torch.arange(bsz, device="cuda")[:, None]
        valid = t < torch.tensor(lens, device="cuda")[:, None]
        f0 = torch.where(valid, torch.where((t >= 10) & (t < 14), 0.0, 160.0 + 20.0 * b.float() + 0.5 * t.float()), 3000.0)
        curve = torch.where(valid, -30.0 + 0.125 * ((t + b) % 16).float(), 99.0)
        gender = torch.where(valid, 0.3125 * (((t + b) % 9) - 4).float(), -7.0)
        velocity = torch.where(valid, 0.25 + 0.125 * ((t + b) % 20).float(), 50.0)
        ids = [[0, num_spk - 1], [num_spk - 1, 0], [num_spk - 1, 0]]
        tf = t[0].float()
        mix = torch.stack([torch.stack([torch.ones_like(tf), 3 * torch.ones_like(tf)], 1), torch.stack([t_len - tf, tf], 1),
                           torch.stack([2 * torch.ones_like(tf), torch.zeros_like(tf)], 1)])
        variances = dict(energy=curve, tension=curve)
        offsets = [0.0, 0.85 * (lens[0] * upp) / rate]
        offsets.append(offsets[1] + 1.2 * (lens[1] * upp) / rate)

        def render(sl, n, lengths):
            """the example's chain on items `sl` cut to n frames"""
            k = len(range(*sl.indices(bsz)))
            a.set_lengths(lengths)
            spk = a.spk_mix(ids[sl], mix[sl, :n], normalize=True)
            cond, aux = a.condition(tokens[sl], durations[sl], f0[sl, :n], {kk: v[sl, :n] for kk, v in variances.items()}, gender=gender[sl, :n],
                                    velocity=velocity[sl, :n], spk_embed=spk, languages=languages[sl])
            p = a.plan(depth, steps)
            assert p.start == _lib.DSD_AC_START_MIX and p.n_step_noise == 0
            x = a.start(p, source=aux, noise=None)
            flat = x.view(1, k, dc.M_BINS, n)
            seeded.fill((1, k, dc.M_BINS, n), seeds[sl], seeded.X_T, src=flat, src_scale=p.src_scale, scale=p.noise_scale, out=flat)
            mel = a.sample(p, cond, x)
            wav = gen.forward_seeded(mel.transpose(1, 2), f0[sl, :n], seeds[sl], lengths=lengths)
            return dict(spk_mix=spk, condition=cond, aux_mel=aux, mel=mel, wav=wav[:, 0].reshape(k, n, upp))
        with torch.no_grad():
            batch = render(slice(0, 3), t_len, lens)
            layout = track.plan(offsets, [n * upp for n in lens], rate)
            tr = track.Track(layout.total, "cuda", layout)
            for k, n in enumerate(lens):
                tr.place(k, batch["wav"][k, :n].reshape(-1))
            peak = float(tr.compute_peak().cpu())
            pcm = tr.export("pcm", norm=True).cpu().numpy()
            want = {k: float(sum(v[i, :n].double().sum() for i, n in enumerate(lens))) for k, v in batch.items()}
            want.update(total=float(layout.total), peak=peak, checksum=float(np.abs(pcm.astype(np.int64)).sum()))
            assert set(got) == set(want), (sorted(got), sorted(want))
            for name, s in want.items():
                print(f"{name}: C example {got[name]!r}, Python bindings {s!r}")
                assert got[name] == pytest.approx(s, rel=0, abs=1e-9 * max(1.0, abs(s))), name
            written = np.fromfile(str(pcm_path), dtype="<i2")
            assert written.shape == pcm.shape and np.array_equal(written, pcm) and int(np.abs(pcm).max()) > 1000
            for i, n in enumerate(lens):                # every segment alone through the same calls
                lone = render(slice(i, i + 1), n, None)
                for k in ("condition", "aux_mel", "mel"):
                    close(batch[k][i:i + 1, :n], lone[k].cpu().numpy(), ALONE_TOL, True, f"segment {i} ({n} frames) {k} against its lone render")
                # the vocoder alone on the batch's own mel: SAME is the bound of vocoding ragged against alone
                alone = gen.forward_seeded(batch["mel"][i:i + 1, :n].transpose(1, 2), f0[i:i + 1, :n], [seeds[i]])[0, 0]
                err = float((batch["wav"][i, :n].reshape(-1) - alone).abs().max())
                scale = max(1.0, float(alone.abs().max()))
                print(f"segment {i}: samples against the segment vocoded alone: max |err| {err:.3e}, bound {SAME * scale:.3e}")
                assert err <= SAME * scale
    finally:
        w.close()
        gen.release_native()
