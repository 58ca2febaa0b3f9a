"""CPU-side checks of the seeded generator: the oracle (tests/noise_ref.py) against the specification's known answers
and statistics, the C-ABI boundary of dsd_noise_fill (export, struct layout, every DSD_EINVAL case - all refused before
any device work, so no GPU is needed), and the shims' refusal of seed= together with explicit noise."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import noise_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KNOWN = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,want", KNOWN)
def test_philox_known_answers(counter, key, want):
    got = noise_ref.philox4x32_10([np.uint64(c) for c in counter], key)
    assert tuple(int(w) for w in got) == want


def test_addressing_is_counter_col4_row_stream_domain():
    seed, domain, stream = 0x299f31d0a4093822, 0x03707344, 0x13198a2e
    rows, cols = 0x85a308d3 % 7 + 1, 9
    w = noise_ref.words(seed, domain, stream, rows, cols)
    assert w.shape == (rows, 3, 4)
    one = noise_ref.philox4x32_10([np.uint64(2), np.uint64(rows - 1), np.uint64(stream), np.uint64(domain)],
                                  (seed & 0xffffffff, seed >> 32))
    assert [int(v) for v in w[rows - 1, 2]] == [int(v) for v in one]
    u = noise_ref.draw(seed, domain, stream, rows, cols, "uniform")
    assert u.shape == (rows, cols) and u[rows - 1, 8] == noise_ref.uniform(one[0])      # column 8 = word 0 of block 2


def test_uniform_is_fp32_exact_and_open():
    edge = noise_ref.uniform(np.array([0, 0x1ff, 0x200, 0xffffffff, 0xfffffe00], dtype=np.uint64))
    u = np.concatenate([edge, noise_ref.draw(7, 1, 0, 64, 1024, "uniform").ravel()])
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)
    assert u.min() > 0.0 and u.max() < 1.0 and np.float32(u.max()) < np.float32(1.0)
    assert edge[0] == 2.0 ** -24 and edge[3] == 1.0 - 2.0 ** -24


def test_normal_statistics():
    n = 1 << 20
    z = noise_ref.draw(0x1234567800000042, noise_ref.X_T, 3, 1024, 1024).ravel()
    assert z.size == n
    assert abs(z.mean()) < 5 / np.sqrt(n)
    assert abs(z.var() - 1) < 5 * np.sqrt(2 / n)
    assert np.abs(z).max() <= 5.7682
    # the largest draw the generator can make: u0 = 2^-24
    assert np.sqrt(-2 * np.log(2.0 ** -24)) <= 5.7682


def test_streams_domains_and_seeds_are_apart():
    base = noise_ref.draw(5, 1, 0, 4, 8)
    for other in (noise_ref.draw(5, 1, 1, 4, 8), noise_ref.draw(5, 2, 0, 4, 8), noise_ref.draw(6, 1, 0, 4, 8),
                  noise_ref.draw(5 + (1 << 32), 1, 0, 4, 8)):
        assert not np.any(other == base)
    assert np.array_equal(noise_ref.fill((2, 2, 4, 8), [5, 6], 1, first_stream=3)[1, 1], noise_ref.draw(6, 1, 4, 4, 8))


def test_symbol_struct_and_domains():
    from diffsinger_amd import _lib, noise
    assert "dsd_noise_fill" in _lib.EXPORTS and hasattr(C.CDLL(_lib.LIB_PATH), "dsd_noise_fill")
    s = _lib.DsdNoiseSpec
    # the header's field order on an LP64 target: 8 int32-sized fields, a pointer, float (+ 4 padding), a pointer, float (+ 4)
    assert C.sizeof(s) == 64
    assert [(n, getattr(s, n).offset) for n, _ in s._fields_] == [
        ("struct_size", 0), ("kind", 4), ("domain", 8), ("first_stream", 12), ("n", 16), ("B", 20), ("rows", 24), ("cols", 28),
        ("seeds", 32), ("scale", 40), ("src", 48), ("src_scale", 56)]
    header = open(os.path.join(ROOT, "include", "dsdenoise.h")).read()
    body = re.search(r"typedef struct dsd_noise_spec \{(.*?)\} dsd_noise_spec;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert names == [n for n, _ in s._fields_]
    assert "#define DSD_NOISE_NORMAL 0" in header and "#define DSD_NOISE_UNIFORM 1" in header
    assert (_lib.DSD_NOISE_NORMAL, _lib.DSD_NOISE_UNIFORM) == (0, 1)
    assert (noise.X_T, noise.STEP, noise.VOC_SOURCE, noise.VOC_PRE, noise.VOC_PHASE, noise.PITCH_X_T, noise.VARIANCE_X_T) == \
        (1, 2, 3, 4, 5, 6, 7) == (noise_ref.X_T, noise_ref.STEP, noise_ref.VOC_SOURCE, noise_ref.VOC_PRE, noise_ref.VOC_PHASE,
                                  noise_ref.PITCH_X_T, noise_ref.VARIANCE_X_T)


def _spec(**over):
    from diffsinger_amd import _lib
    seeds = (C.c_uint64 * 4)(1, 2, 3, 4)
    s = _lib.DsdNoiseSpec()
    s.struct_size, s.kind, s.domain, s.first_stream = C.sizeof(_lib.DsdNoiseSpec), 0, 1, 0
    s.n, s.B, s.rows, s.cols = 1, 1, 2, 4
    s.seeds = C.cast(seeds, C.POINTER(C.c_uint64))
    s.scale, s.src_scale = 1.0, 1.0
    for k, v in over.items():
        setattr(s, k, v)
    return s, seeds


EINVAL = [
    ("struct_size", dict(struct_size=60), b"struct_size"),
    ("n", dict(n=0), b"positive"), ("B", dict(B=0), b"positive"), ("rows", dict(rows=-1), b"positive"), ("cols", dict(cols=0), b"positive"),
    ("kind", dict(kind=2), b"unknown kind"), ("kind_negative", dict(kind=-1), b"unknown kind"),
    ("too_many", dict(n=2, B=1, rows=1 << 15, cols=1 << 15), b"2^31 - 1"),
    ("far_too_many", dict(n=(1 << 31) - 1, B=(1 << 31) - 1, rows=(1 << 31) - 1, cols=(1 << 31) - 1), b"2^31 - 1"),
    ("null_seeds", dict(seeds=C.POINTER(C.c_uint64)()), b"null"),
]


@pytest.mark.parametrize("name,over,message", EINVAL, ids=[e[0] for e in EINVAL])
def test_einval_before_any_device_work(name, over, message):
    """A host pointer stands in for `out`: every case is refused before anything could touch it or a device."""
    from diffsinger_amd import _lib
    lib = _lib.lib()
    host = (C.c_float * 8)()
    spec, _keep = _spec(**over)
    assert lib.dsd_noise_fill(0, C.byref(spec), C.cast(host, C.c_void_p), None) == -1
    err = lib.dsd_last_error(None)
    assert b"dsd_noise_fill" in err and message in err, err
    assert not any(host)


def test_null_spec_and_out_are_einval():
    from diffsinger_amd import _lib
    lib = _lib.lib()
    host = (C.c_float * 8)()
    spec, _keep = _spec()
    assert lib.dsd_noise_fill(0, None, C.cast(host, C.c_void_p), None) == -1
    assert lib.dsd_noise_fill(0, C.byref(spec), None, None) == -1
    assert b"dsd_noise_fill: null argument" in lib.dsd_last_error(None)


def test_largest_legal_count_passes_the_argument_check():
    """2^31 - 1 elements is legal: the call gets past the argument check and stops at the device (index -1 exists nowhere)."""
    from diffsinger_amd import _lib
    lib = _lib.lib()
    host = (C.c_float * 8)()
    spec, _keep = _spec(n=1, B=1, rows=1, cols=(1 << 31) - 1)
    assert lib.dsd_noise_fill(-1, C.byref(spec), C.cast(host, C.c_void_p), None) < 0
    err = lib.dsd_last_error(None)
    assert b"2^31" not in err and (b"no HIP device" in err or b"device -1 out of range" in err), err


def test_seed_together_with_noise_raises():
    """The refusal comes before anything touches a device, so CPU tensors do."""
    import torch
    from diffsinger_amd.diffusion import GaussianDiffusion, RectifiedFlow
    from diffsinger_amd.hparams import hparams
    from diffsinger_amd.vocoder import Generator
    from diffsinger_amd import noise, synth
    saved = dict(hparams)
    try:
        hparams.clear()
        hparams.update(hidden_size=256, schedule_type="linear", use_shallow_diffusion=False, diff_speedup=10,
                       diff_accelerator="ddim", infer=False, sampling_algorithm="euler", sampling_steps=4)
        args = dict(num_layers=2, num_channels=64, dilation_cycle_length=2)
        cond, x = torch.zeros(1, 8, 256), torch.zeros(1, 1, 16, 8)
        d = GaussianDiffusion(16, 1, backbone_type="wavenet", backbone_args=args, spec_min=[-8.0], spec_max=[0.0])
        r = RectifiedFlow(16, 1, backbone_type="wavenet", backbone_args=args, spec_min=[-8.0], spec_max=[0.0])
        with pytest.raises(ValueError, match="either seed or noise"):
            d(cond, infer=True, seed=1, noise=x)
        with pytest.raises(ValueError, match="either seed or noise"):
            d(cond, infer=True, seed=1, step_noise=x[None])
        with pytest.raises(ValueError, match="either seed or noise"):
            r(cond, infer=True, seed=1, noise=x)
        with pytest.raises(ValueError, match="1 ints expected"):
            d(cond, infer=True, seed=[1, 2])
        g = Generator(dict(synth.NSF_HIFIGAN_DEFAULT))
        with torch.no_grad(), pytest.raises(ValueError, match="either seed or rand_ini"):
            g(torch.zeros(1, g.num_mels, 4), torch.zeros(1, 4), seed=3, rand_ini=torch.zeros(9))
        with pytest.raises(ValueError):
            noise.as_seeds(-1, 1)
        with pytest.raises(ValueError):
            noise.as_seeds(1 << 64, 1)
        assert noise.as_seeds(np.int64(7), 2) == [7, 7] and noise.as_seeds((1 << 64) - 1, 1) == [(1 << 64) - 1]
    finally:
        hparams.clear()
        hparams.update(saved)
