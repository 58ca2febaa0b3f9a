"""-m gpu: which handle may call what.  One handle of each of the nine kinds, no weights loaded; every exported call that
takes a handle is made on every kind it does not take, and - where it needs weights - on its own kind, and must answer
DSD_ESTATE (-2).  Every call made here is refused on the host before anything is launched: no call that could pass the
entry check is made, so the buffers below are never read or written.

The table in calls() is written from include/dsdenoise.h and the "Which handle takes which call" table of INTEGRATION.md,
not read from the library."""
import ctypes as C
from types import SimpleNamespace

import pytest

pytestmark = pytest.mark.gpu

from diffsinger_amd import _lib  # noqa: E402

DSD_ESTATE = -2

# kind -> what the library calls it in "<call>: this handle is <what> (use <calls>)"
WHAT = {
    "wavenet": "a WaveNet denoiser",
    "lynxnet": "a LYNXNet denoiser",
    "aux": "an aux decoder",
    "enc": "an acoustic encoder",
    "voc": "a vocoder",
    "tok": "a token encoder",
    "mel": "a mel analysis handle",
    "pe": "an RMVPE pitch extractor",
    "hs": "a harmonic-noise separator",
}
KINDS = tuple(WHAT)
DENOISERS = {"wavenet", "lynxnet"}
ANALYSIS = {"mel", "pe", "hs"}
MODELS = set(KINDS) - ANALYSIS          # everything dsd_get_stats and the timing hooks describe
WEIGHTS = set(KINDS) - {"mel"}          # everything with a state dict


def calls(p):
    """One row per exported handle-taking call: name -> (arguments after the handle, the kinds it takes, what it needs on
    its own kind: "weights" (finalized weights), "cond" (a dsd_prepare_cond, which needs the weights) or None).  `p` holds
    the buffers: f / g floats (in / out), i64, i32, u8, and host arrays."""
    one_i32, one_i64 = (C.c_int32 * 1)(4), (C.c_int64 * 1)(8)
    prog = _lib.DsdProgram(1, 0, 0, 0, None)
    stats, kt = _lib.DsdStats(), (_lib.DsdKernelTime * 1)()
    d0, d1, n64, n32 = C.c_double(), C.c_double(), C.c_int64(), C.c_int32()
    shape = (C.c_int64 * 1)(4)
    return {
        "dsd_load_weight": ((b"x.weight", p.host_f, shape, 1, 0), WEIGHTS, None),
        "dsd_finalize_weights": ((), WEIGHTS, None),
        "dsd_prepare_cond": ((p.f, 1, 4, 128, 4, 1, None), DENOISERS, "weights"),
        "dsd_denoise": ((p.f, p.f, 1, p.g, None), DENOISERS, "cond"),
        "dsd_sample": ((C.byref(prog), p.f, None, p.g, None, None, 0, None), DENOISERS, "cond"),
        "dsd_aux_decode": ((p.f, 1, 4, 128, 4, 1, p.g, None, None, None), {"aux"}, "weights"),
        "dsd_encode": ((p.i64, p.i64, p.f, 1, 2, 4, None, p.g, None), {"enc"}, "weights"),
        "dsd_token_encode": ((p.f, p.u8, 1, 2, p.g, None), {"tok"}, "weights"),
        "dsd_predict_dur": ((p.f, p.u8, 1, 2, p.g, None), {"tok"}, "weights"),
        "dsd_vocode": ((p.f, 1, 4, 128, 4, 1, p.f, p.f, p.f, p.f, p.g, None), {"voc"}, "weights"),
        "dsd_vocode_ragged": ((p.f, 1, 4, 128, 4, 1, one_i32, p.f, p.f, p.f, p.f, p.g, None), {"voc"}, "weights"),
        "dsd_set_lengths": ((one_i32, 1, None), DENOISERS | {"aux"}, None),
        "dsd_set_precision": ((0,), DENOISERS | {"voc"}, None),
        "dsd_get_stats": ((C.byref(stats),), MODELS, None),
        "dsd_kernel_timing": ((0,), MODELS, None),
        "dsd_kernel_timing_read": ((C.byref(d0), C.byref(d1), C.byref(n64)), MODELS, None),
        "dsd_kernel_timing_classes": ((kt, 1, C.byref(n32), C.byref(d0)), MODELS, None),
        "dsd_mel_analyze": ((p.f, 1, 4096, 4096, None, 0.0, 1.0, p.g, 1024, 8, 1, None), {"mel"}, None),
        "dsd_rmvpe_mel_to_hidden": ((p.f, 1, 8, 1024, 8, 1, None, p.g, 2880, 360, None), {"pe"}, "weights"),
        "dsd_rmvpe_decode": ((p.f, 1, 4, 1440, 360, 0.03, p.g, 4, None), {"pe"}, None),
        "dsd_rmvpe_decode_at": ((p.f, p.i32, 1, 4, 1440, 360, 4, 0.03, p.g, 4, None), {"pe"}, None),
        "dsd_rmvpe_decode_viterbi": ((p.f, 1, 4, 1440, 360, None, 0.03, p.g, 4, None, 0, None), {"pe"}, None),
        "dsd_rmvpe_infer": ((p.f, 1, 4096, 4096, None, 16000, 0.03, p.g, 64, None, 0, 0, None), {"pe"}, "weights"),
        "dsd_hnsep_mask": ((p.f, 1, 16, 2080, 0, 32, 2, None, p.g, 2080, 0, 32, 2, None), {"hs"}, "weights"),
        "dsd_hnsep_separate": ((p.f, 1, 1000, 1000, 0, None, p.g, 1000, 0, None), {"hs"}, "weights"),
        "dsd_base_harmonic": ((p.f, 1, 1000, 1000, None, p.f, 8, one_i64, 44100, 128, 512, p.g, 1000, None), {"hs"}, None),
        "dsd_variance_curves": ((p.f, None, None, 1, 1000, (C.c_int64 * 1)(1000), 128, 512, one_i64, 2, 1, p.g, None, None, None,
                                 8, None), {"hs"}, None),
    }


# the same table without buffers, for the parametrisation: (call, kind) pairs the entry check must refuse
_TABLE = calls(SimpleNamespace(f=None, g=None, i64=None, i32=None, u8=None, host_f=None))
WRONG_KIND = [(c, k) for c, (_, takes, _) in _TABLE.items() for k in KINDS if k not in takes]
OWN_KIND = [(c, k) for c, (_, takes, needs) in _TABLE.items() if needs for k in KINDS if k in takes]


def configs():
    """The smallest configuration each create accepts."""
    sz = C.sizeof
    voc = _lib.DsdVocoderConfig()
    voc.struct_size, voc.num_mels, voc.sampling_rate, voc.upsample_initial_channel = sz(voc), 8, 16000, 32
    voc.n_ups, voc.upsample_rates[0], voc.upsample_kernel_sizes[0] = 1, 2, 4
    voc.resblock, voc.n_kernels, voc.resblock_kernel_sizes[0], voc.n_dilations[0] = 2, 1, 3, 1
    voc.resblock_dilation_sizes[0][0] = 1
    voc.harmonic_num = 0
    return {
        "wavenet": ("dsd_create", _lib.DsdConfig(sz(_lib.DsdConfig), 0, 8, 1, 1, 32, 32, 1, 0, 0, 0, 0, 0)),
        "lynxnet": ("dsd_create", _lib.DsdConfig(sz(_lib.DsdConfig), 1, 8, 1, 1, 32, 32, 0, 1, 3, 0, 0, 0)),
        "aux": ("dsd_create", _lib.DsdConfig(sz(_lib.DsdConfig), 2, 8, 1, 1, 32, 32, 0, 0, 7, 0, 0, 0)),
        "enc": ("dsd_encoder_create", _lib.DsdEncoderConfig(sz(_lib.DsdEncoderConfig), 4, 32, 1, 1, 1, 0, 0, 0, 0, 0, 0)),
        "voc": ("dsd_vocoder_create", voc),
        "tok": ("dsd_token_encoder_create",
                _lib.DsdTokenEncoderConfig(sz(_lib.DsdTokenEncoderConfig), 32, 1, 1, 1, 0, 1, 32, 3, 1.0, 0, 0, 0)),
        "mel": ("dsd_mel_create", _lib.DsdMelConfig(sz(_lib.DsdMelConfig), 16000, 64, 64, 16, 4, 0.0, 8000.0, 1e-5, 0)),
        "pe": ("dsd_rmvpe_create", _lib.DsdRmvpeConfig(sz(_lib.DsdRmvpeConfig), 1, 1, 5, 1, 16, 0)),
        "hs": ("dsd_hnsep_create", _lib.DsdHnsepConfig(sz(_lib.DsdHnsepConfig), 128, 64, 4, 8, 1, 0)),
    }


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"


@pytest.fixture(scope="module")
def world():
    """Nine creates, nine destroys, and the buffers the argument tuples point into."""
    import torch
    lib = _lib.lib()
    bufs = [torch.zeros(8192, device="cuda"), torch.zeros(8192, device="cuda"), torch.zeros(64, dtype=torch.int64, device="cuda"),
            torch.zeros(64, dtype=torch.int32, device="cuda"), torch.zeros(64, dtype=torch.uint8, device="cuda")]
    host_f = (C.c_float * 4)()
    p = SimpleNamespace(host_f=C.cast(host_f, C.c_void_p),
                        **{n: C.c_void_p(b.data_ptr()) for n, b in zip(("f", "g", "i64", "i32", "u8"), bufs)})
    handles = {}
    try:
        for kind, (create, cfg) in configs().items():
            h = C.c_void_p()
            assert getattr(lib, create)(C.byref(cfg), C.byref(h)) == 0, (kind, lib.dsd_last_error(None))
            handles[kind] = h
        yield SimpleNamespace(lib=lib, handles=handles, table=calls(p), keep=(bufs, host_f))
        torch.cuda.synchronize()
    finally:
        for h in handles.values():
            lib.dsd_destroy(h)


def _call(world, call, kind):
    return getattr(world.lib, call)(world.handles[kind], *world.table[call][0])


def test_tables_cover_every_export():
    """Every export of the header whose first parameter is a handle has a row (dsd_destroy and dsd_last_error take any)."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dsdenoise.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    taking = set(re.findall(r"\b(dsd_[a-z_]+)\s*\(\s*(?:const\s+)?dsd_handle\s*\*", src))
    assert taking - {"dsd_destroy", "dsd_last_error"} == set(_TABLE)
    assert len(WRONG_KIND) + len(OWN_KIND) > 150


@pytest.mark.parametrize("call,kind", WRONG_KIND, ids=[f"{c}-{k}" for c, k in WRONG_KIND])
def test_wrong_kind_is_estate(world, call, kind):
    assert _call(world, call, kind) == DSD_ESTATE


@pytest.mark.parametrize("call,kind", OWN_KIND, ids=[f"{c}-{k}" for c, k in OWN_KIND])
def test_own_kind_without_weights_is_estate(world, call, kind):
    """Nothing is loaded: a call that needs weights stops there; dsd_denoise / dsd_sample stop at the missing dsd_prepare_cond."""
    assert _call(world, call, kind) == DSD_ESTATE


@pytest.mark.parametrize("call,kind", WRONG_KIND + OWN_KIND, ids=[f"{c}-{k}" for c, k in WRONG_KIND + OWN_KIND])
def test_refusal_message(world, call, kind):
    """dsd_last_error names the call; for a wrong kind it says what the handle is and a call that takes it."""
    assert _call(world, call, kind) == DSD_ESTATE
    msg = world.lib.dsd_last_error(world.handles[kind]).decode()
    assert msg.startswith(call + ":"), msg
    if kind not in _TABLE[call][1]:
        assert WHAT[kind] in msg, msg
        assert any(c in msg for c, (_, takes, _) in _TABLE.items() if kind in takes), msg
