"""Model files on the host (no GPU): the pure-Python writer (diffsinger_amd/modelfile.py) against the C reader
(csrc/model_file.hip) - two independent statements of DESIGN.md section 4n.  Round trip bit for bit, one case per refusal
of dsd_model_open (each made by patching a valid file, the CRC recomputed here so that the named check is the one reached),
every prefix of the pinned file, and the pin of format version 1 (tests/golden/g29_model_v1.dsdm)."""
import ctypes as C
import os
import struct
import sys
import zlib

import numpy as np
import pytest
import torch

from diffsinger_amd import _lib, modelfile, synth
from diffsinger_amd.hparams import hparams

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PINNED = os.path.join(GOLDEN, "g29_model_v1.dsdm")
EINVAL, ESTATE, ENOTFOUND, EIO = -1, -2, -5, -6


def golden_module():
    sys.path.insert(0, GOLDEN)
    import make_golden_model
    return make_golden_model


def wavenet(in_dims, hidden, args, seed):
    from diffsinger_amd.backbones import build_backbone
    saved = dict(hparams)
    hparams.update(hidden_size=hidden)
    try:
        net = build_backbone(in_dims, 1, "wavenet", args)
    finally:
        hparams.clear()
        hparams.update(saved)
    params = synth.synth_state_dict(synth.backbone_param_shapes("wavenet", in_dims, 1, hidden_size=hidden, **args), seed=seed)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    return net, params


def smallest_vocoder_case():
    import vocoder_config_cases as vcc
    return min(vcc.CASES, key=lambda t: sum(int(np.prod(s)) for s in synth.nsf_hifigan_param_shapes(vcc.config(t)).values()))


def c_open(path):
    fp = C.c_void_p()
    rc = _lib.lib().dsd_model_open(str(path).encode(), C.byref(fp))
    return rc, fp, _lib.lib().dsd_last_error(None).decode("utf-8", "replace")


# ------------------------------------------------------------------------------------------------ round trip
def test_round_trip_bit_for_bit(tmp_path):
    import vocoder_config_cases as vcc
    from diffsinger_amd.mel import STFT
    from diffsinger_amd.vocoder import Generator
    net, params = wavenet(32, 256, dict(num_layers=2, num_channels=64, dilation_cycle_length=2), 2911)
    tag = smallest_vocoder_case()
    gen = Generator(vcc.config(tag))
    gen.load_state_dict({k: torch.from_numpy(v) for k, v in vcc.weights(tag).items()}, strict=True)
    stft = STFT(44100, 128, 2048, 2048, 512, 40, 16000)
    den = modelfile.section_of("denoiser", net)
    den.tensors["a_scalar"] = np.float32(-2.5)                  # a 0-dim tensor
    den.tensors["a_4d"] = synth.synth_normal((2, 3, 1, 5), 7)
    sections = [den, modelfile.section_of("vocoder", gen), modelfile.section_of("mel", stft)]
    meta = {"empty": "", "big": "0123456789abcdef" * 4480, "ключ": "значение ♪", "timesteps": "1000"}
    assert len(meta["big"]) > 70000
    path = tmp_path / "three.dsdm"
    size = modelfile.write(path, sections, meta)
    assert size == os.path.getsize(path)

    lib = _lib.lib()
    rc, fp, msg = c_open(path)
    assert rc == 0, msg
    try:
        ns, nm = C.c_int32(), C.c_int32()
        assert lib.dsd_model_count(fp, C.byref(ns), C.byref(nm)) == 0 and (ns.value, nm.value) == (3, 4)
        info, t = _lib.DsdModelSectionInfo(), _lib.DsdModelTensorInfo()
        for i, s in enumerate(sections):
            assert lib.dsd_model_section(fp, i, C.byref(info)) == 0
            assert info.name.decode() == s.name and info.kind == s.kind == (0, 4, 6)[i]
            assert info.config_size == C.sizeof(s.cfg) and info.n_tensors == len(s.tensors)
            assert info.total_floats == sum(int(np.asarray(v).size) for v in s.tensors.values())
            assert lib.dsd_model_find(fp, s.name.encode()) == i
            cfg = type(s.cfg)()
            assert lib.dsd_model_config(fp, i, C.byref(cfg), C.sizeof(cfg)) == 0 and bytes(cfg) == bytes(s.cfg)
            assert lib.dsd_model_config(fp, i, C.byref(cfg), C.sizeof(cfg) - 4) == EINVAL
            for j, (name, want) in enumerate(s.tensors.items()):            # names AND order
                want = np.asarray(want, np.float32)
                assert lib.dsd_model_tensor(fp, i, j, C.byref(t)) == 0
                assert t.name.decode() == name and t.ndim == want.ndim and t.count == want.size
                assert tuple(t.shape) == tuple(want.shape) + (0,) * (4 - want.ndim)
                assert C.addressof(t.data.contents) % 64 == 0
                got = np.ctypeslib.as_array(t.data, shape=(want.size,))
                assert got.tobytes() == want.tobytes(), name
        key, value = C.c_char_p(), C.c_char_p()
        for k, (mk, mv) in enumerate(meta.items()):
            assert lib.dsd_model_meta_at(fp, k, C.byref(key), C.byref(value)) == 0
            assert key.value == mk.encode("utf-8") and value.value == mv.encode("utf-8")
            assert lib.dsd_model_meta(fp, mk.encode("utf-8")) == mv.encode("utf-8")
        assert lib.dsd_model_meta(fp, b"missing") is None
        assert lib.dsd_model_find(fp, b"missing") == ENOTFOUND
        assert "missing" in lib.dsd_last_error(None).decode()
        # an index out of range, NULL arguments
        assert lib.dsd_model_section(fp, 3, C.byref(info)) == EINVAL and lib.dsd_model_section(fp, -1, C.byref(info)) == EINVAL
        assert "out of range" in lib.dsd_last_error(None).decode()
        assert lib.dsd_model_tensor(fp, 0, len(den.tensors), C.byref(t)) == EINVAL and lib.dsd_model_tensor(fp, 2, 0, C.byref(t)) == EINVAL
        assert lib.dsd_model_config(fp, 3, C.byref(cfg), C.sizeof(cfg)) == EINVAL
        assert lib.dsd_model_meta_at(fp, 4, C.byref(key), C.byref(value)) == EINVAL
        assert lib.dsd_model_section(fp, 0, None) == EINVAL and lib.dsd_model_tensor(fp, 0, 0, None) == EINVAL
        assert lib.dsd_model_config(fp, 0, None, 52) == EINVAL and lib.dsd_model_meta_at(fp, 0, None, C.byref(value)) == EINVAL
        assert lib.dsd_model_find(fp, None) == EINVAL and lib.dsd_model_find(None, b"x") == EINVAL
        assert lib.dsd_model_count(None, C.byref(ns), C.byref(nm)) == EINVAL
        assert lib.dsd_model_create(None, 0, 0, C.byref(C.c_void_p())) == EINVAL and lib.dsd_model_create(fp, 0, 0, None) == EINVAL
    finally:
        lib.dsd_model_close(fp)
    lib.dsd_model_close(None)

    # the same through the Python face of the reader
    with modelfile.open(path) as f:
        assert [(s.name, s.kind, s.n_tensors) for s in f.sections] == [(s.name, s.kind, len(s.tensors)) for s in sections]
        assert dict(f.meta) == meta and list(f.meta) == list(meta)
        got = f.tensors("denoiser")
        assert list(got) == list(den.tensors) and got["a_scalar"].shape == () and got["a_4d"].shape == (2, 3, 1, 5)
        assert all(np.array_equal(got[k], params[k]) for k in params)
        assert bytes(f.config("vocoder")) == bytes(sections[1].cfg) and f.tensors("mel") == {}
        with pytest.raises(_lib.NativeLibraryError, match="no section is called"):
            f.index("missing")


def test_open_refuses_paths_and_null():
    lib = _lib.lib()
    rc, fp, msg = c_open("/no/such/directory/model.dsdm")
    assert rc == EIO and not fp.value and "cannot open" in msg
    rc, fp, msg = c_open(GOLDEN)                                   # a directory
    assert rc == EIO and not fp.value
    assert lib.dsd_model_open(None, C.byref(fp)) == EINVAL and lib.dsd_model_open(PINNED.encode(), None) == EINVAL
    with pytest.raises(_lib.NativeLibraryError, match=r"\(-6\)"):
        modelfile.open("/no/such/directory/model.dsdm")


# ------------------------------------------------------------------------------------------------ refusals
class Layout:
    """A third, minimal reading of the tables (struct only): where each field of a valid file sits."""

    def __init__(self, raw):
        self.n_sections, self.n_meta, self.section_table, self.meta_table = struct.unpack_from("<IIQQ", raw, 32)
        self.size = len(raw)

    def section(self, i, field):
        return self.section_table + 40 * i + dict(name=0, config=8, tensors=16, name_len=24, kind=28, config_size=32, n_tensors=36)[field]

    def tensor(self, raw, i, j, field):
        table, = struct.unpack_from("<Q", raw, self.section(i, "tensors"))
        return table + 64 * j + dict(name=0, data=8, count=16, name_len=24, ndim=28, shape=32)[field]

    def meta(self, k, field):
        return self.meta_table + 32 * k + dict(key=0, value=8, value_len=16, key_len=24)[field]


@pytest.fixture(scope="module")
def valid(tmp_path_factory):
    """A small valid file: the pinned WaveNet as "denoiser" (a [1] bias, [4, 4, 3] and [4, 4, 1] weights) and a mel section"""
    from diffsinger_amd.mel import STFT
    sections, meta = golden_module().content()
    sections.append(modelfile.section_of("mel", STFT()))
    path = tmp_path_factory.mktemp("modelfile") / "valid.dsdm"
    modelfile.write(path, sections, dict(meta, note="hello"))
    raw = path.read_bytes()
    rc, fp, msg = c_open(path)
    assert rc == 0, msg
    _lib.lib().dsd_model_close(fp)
    return raw


def _p32(off, v):
    return lambda raw, L: struct.pack_into("<I", raw, off(raw, L) if callable(off) else off, v & 0xFFFFFFFF)


def _p64(off, v):
    return lambda raw, L: struct.pack_into("<Q", raw, off(raw, L), (v(raw, L) if callable(v) else v) & 0xFFFFFFFFFFFFFFFF)


def _copy_field(dst, src, fmt):
    return lambda raw, L: struct.pack_into(fmt, raw, dst(raw, L), *struct.unpack_from(fmt, raw, src(raw, L)))


def _both(*patches):
    def run(raw, L):
        for p in patches:
            p(raw, L)
    return run


def _u64(raw, off):
    return struct.unpack_from("<Q", raw, off)[0]


# name: (patch(raw, L), recompute the CRC, code, message fragment)
REFUSALS = {
    "bad_magic": (lambda raw, L: raw.__setitem__(0, raw[0] ^ 1), True, EINVAL, "bad magic"),
    "unknown_version": (_p32(8, 2), True, EINVAL, "format version 2 is unknown"),
    "recorded_size_larger": (_p64(lambda raw, L: 16, lambda raw, L: L.size + 1), True, EINVAL, "the header records"),
    "recorded_size_smaller": (_p64(lambda raw, L: 16, lambda raw, L: L.size - 1), True, EINVAL, "the header records"),
    "crc_mismatch": (lambda raw, L: raw.__setitem__(L.size - 1, raw[L.size - 1] ^ 0x40), False, EINVAL, "CRC mismatch"),
    "crc_field": (_p32(24, 0), False, EINVAL, "CRC mismatch"),
    "sections_over_limit": (_p32(32, 65), True, EINVAL, "65 sections are over the limit of 64"),
    "meta_over_limit": (_p32(36, 65537), True, EINVAL, "metadata entries are over the limit"),
    "tensors_over_limit": (_p32(lambda raw, L: L.section(0, "n_tensors"), 65537), True, EINVAL, "65537 tensors are over the limit of 65536"),
    "section_table_past_end": (_p64(lambda raw, L: 40, lambda raw, L: L.size - 8), True, EINVAL, "the section table"),
    "section_table_wraps": (_p64(lambda raw, L: 40, 2 ** 64 - 8), True, EINVAL, "the section table"),
    "meta_table_past_end": (_p64(lambda raw, L: 48, lambda raw, L: L.size - 31), True, EINVAL, "the metadata table"),
    "tensor_table_past_end": (_p64(lambda raw, L: L.section(0, "tensors"), lambda raw, L: L.size - 63), True, EINVAL, "the tensor table"),
    "config_past_end": (_p64(lambda raw, L: L.section(0, "config"), lambda raw, L: L.size - 51), True, EINVAL, "the config"),
    "name_past_end": (_p64(lambda raw, L: L.section(0, "name"), lambda raw, L: L.size - 2), True, EINVAL, "past the end of the file"),
    "data_past_end": (_p64(lambda raw, L: L.tensor(raw, 0, 0, "data"), lambda raw, L: (L.size + 63) // 64 * 64), True, EINVAL,
                      "is past the end of the file"),
    "data_offset_wraps": (_p64(lambda raw, L: L.tensor(raw, 0, 0, "data"), 2 ** 64 - 64), True, EINVAL, "is past the end of the file"),
    "meta_value_length_past_end": (_p64(lambda raw, L: L.meta(0, "value_len"), lambda raw, L: L.size), True, EINVAL, "the value"),
    "meta_value_length_wraps": (_p64(lambda raw, L: L.meta(0, "value_len"), 2 ** 64 - 1), True, EINVAL, "the value"),
    "unaligned_data": (_p64(lambda raw, L: L.tensor(raw, 0, 0, "data"), lambda raw, L: _u64(raw, L.tensor(raw, 0, 0, "data")) + 4), True,
                       EINVAL, "is not 64-byte aligned"),
    "count_differs": (_p64(lambda raw, L: L.tensor(raw, 0, 0, "count"), lambda raw, L: _u64(raw, L.tensor(raw, 0, 0, "count")) + 1), True,
                      EINVAL, "differs from the stored count"),
    "shape_differs": (_p64(lambda raw, L: L.tensor(raw, 0, 0, "shape"), lambda raw, L: _u64(raw, L.tensor(raw, 0, 0, "shape")) + 1), True,
                      EINVAL, "differs from the stored count"),
    "shape_product_overflows": (_both(_p32(lambda raw, L: L.tensor(raw, 0, 0, "ndim"), 4),
                                      *[_p64(lambda raw, L, d=d: L.tensor(raw, 0, 0, "shape") + 8 * d, 2 ** 62) for d in range(4)]),
                                True, EINVAL, "the shape product overflows 64 bits"),
    "negative_dim": (_p64(lambda raw, L: L.tensor(raw, 0, 0, "shape"), 2 ** 64 - 1), True, EINVAL, "negative dim -1"),
    "ndim_5": (_p32(lambda raw, L: L.tensor(raw, 0, 0, "ndim"), 5), True, EINVAL, "ndim 5 > 4"),
    "section_name_empty": (_p32(lambda raw, L: L.section(0, "name_len"), 0), True, EINVAL, "section 0: the name is empty"),
    "tensor_name_empty": (_p32(lambda raw, L: L.tensor(raw, 0, 1, "name_len"), 0), True, EINVAL, "section 0 tensor 1: the name is empty"),
    "name_over_255": (_p32(lambda raw, L: L.tensor(raw, 0, 0, "name_len"), 256), True, EINVAL, "is longer than 255 bytes"),
    "name_holds_nul": (lambda raw, L: raw.__setitem__(_u64(raw, L.tensor(raw, 0, 0, "name")) + 2, 0), True, EINVAL, "holds a NUL"),
    "name_not_terminated": (_p32(lambda raw, L: L.section(0, "name_len"), 4), True, EINVAL, "is not NUL-terminated"),
    "key_empty": (_p32(lambda raw, L: L.meta(0, "key_len"), 0), True, EINVAL, "metadata entry 0: the key is empty"),
    "two_sections_one_name": (_both(_copy_field(lambda raw, L: L.section(1, "name"), lambda raw, L: L.section(0, "name"), "<Q"),
                                    _copy_field(lambda raw, L: L.section(1, "name_len"), lambda raw, L: L.section(0, "name_len"), "<I")),
                              True, EINVAL, 'two sections are called "denoiser"'),
    "two_tensors_one_name": (_both(_copy_field(lambda raw, L: L.tensor(raw, 0, 3, "name"), lambda raw, L: L.tensor(raw, 0, 1, "name"), "<Q"),
                                   _copy_field(lambda raw, L: L.tensor(raw, 0, 3, "name_len"), lambda raw, L: L.tensor(raw, 0, 1, "name_len"), "<I")),
                             True, EINVAL, "two tensors are called"),
    "two_keys_one_name": (_both(_copy_field(lambda raw, L: L.meta(1, "key"), lambda raw, L: L.meta(0, "key"), "<Q"),
                                _copy_field(lambda raw, L: L.meta(1, "key_len"), lambda raw, L: L.meta(0, "key_len"), "<I")),
                          True, EINVAL, "two metadata entries have the key"),
    "unknown_kind": (_p32(lambda raw, L: L.section(0, "kind"), 9), True, EINVAL, "unknown kind 9"),
    "config_size_not_sizeof": (_p32(lambda raw, L: L.section(0, "config_size"), 56), True, EINVAL, "config size 56 is not sizeof(dsd_config) = 52"),
    "kind_of_another_struct": (_p32(lambda raw, L: L.section(0, "kind"), 7), True, EINVAL, "is not sizeof(dsd_rmvpe_config) = 28"),
    "stored_struct_size": (lambda raw, L: struct.pack_into("<i", raw, _u64(raw, L.section(0, "config")), 48), True, EINVAL,
                           "the stored struct_size 48 disagrees with the config size 52"),
    "backbone_is_not_the_kind": (_p32(lambda raw, L: L.section(0, "kind"), 1), True, EINVAL, "is of kind 1, its dsd_config says backbone 0"),
    "tensor_on_a_mel_section": (_p32(lambda raw, L: L.section(1, "n_tensors"), 1), True, EINVAL, "a mel analysis section has no tensors"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusal(valid, tmp_path, name):
    patch, fix_crc, code, fragment = REFUSALS[name]
    raw = bytearray(valid)
    patch(raw, Layout(valid))
    if fix_crc:
        struct.pack_into("<I", raw, 24, zlib.crc32(bytes(raw[32:])) & 0xFFFFFFFF)
    path = tmp_path / "patched.dsdm"
    path.write_bytes(raw)
    rc, fp, msg = c_open(path)
    assert rc == code and not fp.value, (rc, msg)
    assert fragment in msg, msg


def test_refuses_a_longer_file(valid, tmp_path):
    """the other direction of the size check: bytes behind the recorded end"""
    path = tmp_path / "longer.dsdm"
    path.write_bytes(valid + b"\0")
    rc, fp, msg = c_open(path)
    assert rc == EINVAL and not fp.value and "the header records" in msg, msg


def test_every_prefix_is_refused(tmp_path):
    raw = open(PINNED, "rb").read()
    path = tmp_path / "prefix.dsdm"
    for n in range(len(raw)):
        path.write_bytes(raw[:n])
        rc, fp, _ = c_open(path)
        assert rc < 0 and not fp.value, n


# ------------------------------------------------------------------------------------------------ the pin of version 1
def test_format_pin(tmp_path):
    g = golden_module()
    raw = open(PINNED, "rb").read()
    assert len(raw) < 16384
    magic, version, api, size, crc = struct.unpack_from("<8sIIQI", raw, 0)
    assert (magic, version, api, size) == (b"DSDMODEL", 1, 10, len(raw))
    assert crc == zlib.crc32(raw[32:]) & 0xFFFFFFFF
    with modelfile.open(PINNED) as f:
        assert [(s.name, s.kind) for s in f.sections] == [("denoiser", 0)]
        assert dict(f.meta) == g.META
        cfg = f.config(0)
        assert (cfg.in_dims, cfg.num_layers, cfg.num_channels, cfg.hidden_size, cfg.dilation_cycle_length, cfg.device) == (4, 1, 4, 4, 1, 0)
        got, want = f.tensors(0), g.weights()
        assert set(want) < set(got) and set(got) - set(want) == {"diffusion_embedding.freqs"}
        for k, v in want.items():
            assert got[k].shape == v.shape and got[k].tobytes() == v.tobytes(), k
    fresh = tmp_path / "fresh.dsdm"
    modelfile.write(fresh, *g.content())
    assert fresh.read_bytes() == raw


def test_create_without_gpu_says_so():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    lib = _lib.lib()
    rc, fp, msg = c_open(PINNED)
    assert rc == 0, msg
    try:
        h = C.c_void_p(1)
        rc = lib.dsd_model_create(fp, 0, 0, C.byref(h))
        assert rc < 0 and not h.value
        msg = lib.dsd_last_error(None)
        assert b"no HIP device" in msg and b'section "denoiser"' in msg
        assert lib.dsd_model_create(fp, 1, 0, C.byref(h)) == EINVAL          # an index out of range
    finally:
        lib.dsd_model_close(fp)
