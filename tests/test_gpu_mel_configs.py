"""-m gpu: mel analysis (dsd_mel_analyze, diffsinger_amd.mel.STFT) at the edges of what dsd_mel_create accepts: the rows of
tests/mel_config_cases.py against the float64 restatement (tests/mel_ref.py) and the reference's own fp32 STFT.get_mel (G26).

Bars.  A row's floor is G26 against mel_ref in float64, computed here from the committed fixture; its bar is
2 max(family floor, row floor) with test_gpu_mel.py's family floors and factor, and the result must also lie within
floor + bar of G26.  No figure of the HIP result enters a bar.  Where the item's peak is 0 every value must be
log(float32(clip)) within 1e-6 instead.  Every row meets its log-mel bar over all of its entries: none is restricted to
the larger values.

Beyond the rows: frame-tile edges and negative pads in ragged NaN-padded calls, the basis cache cycled past its four slots,
two calls on one stream with no host sync between them, the output forms at an odd geometry, and dsd_mel_analyze's
refusals (which must leave the output untouched)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mel_config_cases as mc  # noqa: E402
import mel_ref  # noqa: E402
from gpu_util import dev  # noqa: E402
from test_gpu_mel import FLOOR_LIN, FLOOR_LOG, TOL_LIN, TOL_LOG, _record  # noqa: E402

assert (FLOOR_LOG, FLOOR_LIN) == (mc.FLOOR_LOG, mc.FLOOR_LIN)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"


def stft_of(c):
    from diffsinger_amd.mel import STFT
    return STFT(c["sr"], c["n_mels"], c["n_fft"], c["win_size"], c["hop"], c["fmin"], c["fmax"], clip_val=c.get("clip", 1e-5))


def assert_within(got, lin, clip, bar_log, bar_lin, name):
    """the errors of test_gpu_mel.errors (log-mel maximum, linear error over the item's peak) of `got` against the float64
    linear mel `lin`, recorded, printed and then held against the bars"""
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
    assert got.shape == lin.shape, (name, got.shape, lin.shape)
    assert np.isfinite(got).all(), name
    e_log, e_lin = mc.errors_of(got, lin, clip)
    row = dict(case=name, log=e_log, lin_peak=e_lin, bar_log=bar_log, bar_lin=bar_lin)
    _record(row)
    print(row)
    assert e_log <= bar_log and e_lin <= bar_lin, row
    return e_log, e_lin


_results = {}


def run_case(tag):
    """the row's HIP result [n_mels, T] as float32 numpy, computed once"""
    if tag not in _results:
        k = mc.CASES[tag]
        got = stft_of(k["cfg"]).get_mel(dev(mc.clip_wave(tag))[None], keyshift=float(k["ks"]), speed=float(k["sp"]))[0]
        _results[tag] = got.cpu().numpy()
    return _results[tag]


# ------------------------------------------------------------------------------------------------------------------ a
@pytest.mark.parametrize("tag", mc.TAGS)
def test_case(tag):
    k = mc.CASES[tag]
    clip = k["cfg"]["clip"]
    want, got, lin = mc.g26(tag), run_case(tag), mc.oracle_linear(tag)
    assert got.shape == want.shape and got.dtype == np.float32
    if tag in mc.DEAD:
        assert lin.max() == 0.0
        _record(dict(case=f"cfg_{tag}", dead=float(np.abs(got - np.log(np.float32(clip))).max())))
        assert np.abs(got.astype(np.float64) - np.log(np.float32(clip))).max() <= 1e-6
        return
    f_log, f_lin = mc.floors(tag)
    bar_log, bar_lin = mc.bars(tag)
    _record(dict(case=f"cfg_{tag}_floor", log=f_log, lin_peak=f_lin))
    assert_within(got, lin, clip, bar_log, bar_lin, f"cfg_{tag}")
    d = np.abs(got.astype(np.float64) - want).max()
    print(dict(case=tag, to_g26=float(d), allowed=f_log + bar_log))
    assert d <= f_log + bar_log, (tag, d, f_log + bar_log)


# ------------------------------------------------------------------------------------------------------------------ b
@pytest.mark.parametrize("tag", ["mels1024", "over_nyquist"])
def test_empty_filter_rows(tag):
    live = mc.live_filters(tag)
    got = run_case(tag)
    assert (~live).sum() == {"mels1024": 253, "over_nyquist": 6}[tag]
    assert np.abs(got[~live].astype(np.float64) - np.log(np.float32(mc.CASES[tag]["cfg"]["clip"]))).max() <= 1e-6
    assert (got[live].max(axis=1) > np.log(np.float32(1e-5)) + 1e-3).all()         # and every live row rises above the clamp


# --------------------------------------------------------------------------------------------------------------- c, d
def length_for(c, t, ks=0, sp=1, extra=0):
    """the shortest clip of `t` frames, plus up to `extra` samples that leave the count alone"""
    n = next(n for n in range(1, 1 << 20) if mel_ref.num_frames(n, c["n_fft"], c["win_size"], c["hop"], ks, sp) == t)
    while extra and mel_ref.num_frames(n + extra, c["n_fft"], c["win_size"], c["hop"], ks, sp) != t:
        extra -= 1
    return n + extra


def ragged_check(tag, lens, seed):
    """one ragged call through STFT._analyze on a NaN-padded buffer into a NaN-filled output: every item bit-equal to its
    lone call and within the row's bars, NaN past T_b and none before"""
    k = mc.CASES[tag]
    c, ks, sp = k["cfg"], float(k["ks"]), float(k["sp"])
    stft = stft_of(c)
    waves = [mel_ref.waveform(seed + b, n, c["sr"]) for b, n in enumerate(lens)]
    frames = [mel_ref.num_frames(n, c["n_fft"], c["win_size"], c["hop"], ks, sp) for n in lens]
    pad = np.full((len(lens), max(lens)), np.nan, np.float32)
    for b, w in enumerate(waves):
        pad[b, : len(w)] = w
    out = torch.full((len(lens), c["n_mels"], max(frames)), float("nan"), device="cuda")
    with torch.no_grad():
        stft._analyze(dev(pad), lens, ks, sp, out)
    bar_log, bar_lin = mc.bars(tag)
    for b, w in enumerate(waves):
        lone = stft.get_mel(dev(w)[None], keyshift=ks, speed=sp)[0]
        assert lone.shape[1] == frames[b]
        assert not torch.isnan(out[b, :, : frames[b]]).any(), b
        assert torch.equal(out[b, :, : frames[b]], lone), b
        assert torch.isnan(out[b, :, frames[b]:]).all(), b
        lin = mel_ref.get_mel(w, c, ks, sp, linear=True)
        assert_within(lone, lin, c["clip"], bar_log, bar_lin, f"ragged_{tag}_{b}_T{frames[b]}")
    return frames


def test_tile_edges_ragged():
    c = mc.TINY
    want = [1, 63, 64, 65, 128, 129]
    lens = [length_for(c, t, extra=(5 * i) % 16) for i, t in enumerate(want)]
    assert ragged_check("tiny", lens, 2640) == want


def test_negative_pads_ragged():
    c = mc.HOP_GT_WIN_ODD
    shortest = length_for(c, 1)
    assert shortest == 256 + 86 + 85 and mel_ref.num_frames(shortest - 1, c["n_fft"], c["win_size"], c["hop"]) is None
    assert ragged_check("hop_gt_win_odd", [3011, shortest, 20000], 2650) == [9, 1, 66]


# ------------------------------------------------------------------------------------------------------------------ e
def test_basis_cache_cycles():
    """six (N', W') through the four slots of one handle, two of them re-created, then hits that rotate: every repeat is
    bit-equal to its first result, and each first result meets the family's bars"""
    c = mel_ref.SMALL
    y = mel_ref.waveform(2630, 12000, c["sr"])
    yd = dev(y)[None]
    order = [0, 1, 2, 3, 4, 5, 0, 1, 5, 4, 5]
    assert len({mel_ref.geometry(c["n_fft"], c["win_size"], c["hop"], ks)[:2] for ks in order}) == 6
    stft = stft_of(c)
    first = {}
    for i, ks in enumerate(order):
        got = stft.get_mel(yd, keyshift=float(ks))[0]
        if ks not in first:
            first[ks] = got.clone()
            assert_within(got, mel_ref.get_mel(y, c, ks, 1, linear=True), 1e-5, TOL_LOG, TOL_LIN, f"cache_ks{ks}")
        else:
            assert torch.equal(got, first[ks]), (i, ks)


# ------------------------------------------------------------------------------------------------------------------ f
def test_two_calls_without_host_sync():
    """call A (about 4060 work entries) and call B right behind it on the same stream, results read only after both are
    issued: each bit-equal to the same call made alone between synchronisations (the work list of A must not be the one B
    refills)"""
    c = mc.HOP1
    ya, yb = dev(mel_ref.waveform(2660, 260000, c["sr"]))[None], dev(mel_ref.waveform(2661, 5000, c["sr"]))[None]
    stft = stft_of(c)
    ta, tb = stft.num_frames(260000), stft.num_frames(5000)
    stft.get_mel(yb)                                              # the handle, its buffers and the basis exist
    alone = []
    for y in (ya, yb):
        torch.cuda.synchronize()
        alone.append(stft.get_mel(y).clone())
        torch.cuda.synchronize()
    oa = torch.full((1, c["n_mels"], ta), float("nan"), device="cuda")
    ob = torch.full((1, c["n_mels"], tb), float("nan"), device="cuda")
    torch.cuda.synchronize()
    stft.get_mel(ya, out=oa)
    stft.get_mel(yb, out=ob)
    torch.cuda.synchronize()
    assert torch.equal(oa, alone[0]) and torch.equal(ob, alone[1])
    assert not torch.isnan(oa).any() and not torch.isnan(ob).any()


# ------------------------------------------------------------------------------------------------------------------ g
def test_output_forms_at_odd_geometry():
    tag = "oddwin_dn"
    k = mc.CASES[tag]
    c, ks, sp = k["cfg"], float(k["ks"]), float(k["sp"])
    y = np.stack([mc.clip_wave(tag), mel_ref.waveform(2670, k["n"], c["sr"])])
    stft = stft_of(c)
    a = stft.get_mel(dev(y), keyshift=ks, speed=sp)
    assert np.array_equal(a[0].cpu().numpy(), run_case(tag))      # an item of a batch is its lone call
    t = a.shape[2]
    btm = torch.full((2, t, c["n_mels"]), float("nan"), device=a.device)
    stft.get_mel(dev(y), keyshift=ks, speed=sp, out=btm.transpose(1, 2))
    assert torch.equal(a, btm.transpose(1, 2))
    big = torch.full((4, k["n"] + 37), float("nan"), device=a.device)      # rows two apart in a wider buffer
    big[0::2, : k["n"]] = dev(y)
    view = big[0::2, : k["n"]]
    assert view.stride(0) == 2 * (k["n"] + 37)
    out = torch.empty_like(a)
    with torch.no_grad():
        stft._analyze(view, None, ks, sp, out)
    assert torch.equal(out, a)


# ------------------------------------------------------------------------------------------------------------------ h
def test_analyze_refusals_leave_output_untouched():
    from diffsinger_amd import _lib
    lib = _lib.lib()
    c = mel_ref.PROD
    stft = stft_of(c)
    h = stft._handle(torch.device("cuda"))
    n = 4096
    y = torch.zeros(2, n, device="cuda")
    out = torch.full((2, c["n_mels"], 8), float("nan"), device="cuda")
    so = out.stride()

    def call(handle, wav, b, n_samples, stride_b, lens, ks, sp):
        arr = None if lens is None else (C.c_int64 * len(lens))(*lens)
        rc = lib.dsd_mel_analyze(handle, C.c_void_p(wav.data_ptr()), b, n_samples, stride_b, arr, ks, sp,
                                 C.c_void_p(out.data_ptr()), so[0], so[1], so[2], None)
        torch.cuda.synchronize()
        return rc, lib.dsd_last_error(handle)

    refused = [("lengths[b] of 0", (h, y, 2, n, n, [n, 0], 0.0, 1.0), b"lengths[1]"),
               ("lengths[b] above n_samples", (h, y, 2, n, n, [n + 1, n], 0.0, 1.0), b"lengths[0]"),
               ("B = 2 with wav_stride_b < n_samples", (h, y, 2, n, n - 1, None, 0.0, 1.0), b"wav_stride_b"),
               ("B = 0", (h, y, 0, n, n, None, 0.0, 1.0), b"positive"),
               ("speed = 0", (h, y, 1, n, n, None, 0.0, 0.0), b"speed"),
               ("N' > 32768", (h, y, 1, n, n, None, 49.0, 1.0), b"keyshift")]
    assert mel_ref.geometry(2048, 2048, 512, 49.0)[0] > 32768 >= mel_ref.geometry(2048, 2048, 512, 48.0)[0]
    for what, args, word in refused:
        rc, msg = call(*args)
        assert rc == -1 and word in msg, (what, rc, msg)
        assert torch.isnan(out).all(), what
    # an item one sample too short for hop_gt_win's geometry (pads -86 / -86: 256 + 172 samples fill one frame)
    g = mc.HOP_GT_WIN
    s2 = stft_of(g)
    h2 = s2._handle(torch.device("cuda"))
    out = torch.full((2, g["n_mels"], 2), float("nan"), device="cuda")
    so = out.stride()
    y2 = dev(np.stack([mel_ref.waveform(2680 + b, 800, g["sr"]) for b in range(2)]))
    rc, msg = call(h2, y2, 2, 800, 800, [800, 427], 0.0, 1.0)
    assert rc == -1 and b"too short" in msg and b"item 1" in msg, (rc, msg)
    assert torch.isnan(out).all()
    rc, msg = call(h2, y2, 2, 800, 800, [800, 428], 0.0, 1.0)
    assert rc == 0, msg
    assert not torch.isnan(out[0]).any() and not torch.isnan(out[1, :, 0]).any() and torch.isnan(out[1, :, 1]).all()
    assert torch.equal(out[1, :, :1], s2.get_mel(y2[1:, :428])[0])
