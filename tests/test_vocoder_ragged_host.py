"""CPU-side checks of the ragged vocoder batch (dsd_vocode_ragged): the entry point is declared, exported and bound, its
argument checks that run before any HIP call reject bad calls, and Generator.forward takes `lengths`.  No compute calls."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DSD_EINVAL = -1


def test_header_declares_and_lib_exports_vocode_ragged():
    from diffsinger_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dsdenoise.h")).read(), flags=re.S)
    decl = re.search(r"int\s+dsd_vocode_ragged\s*\(([^)]*)\)\s*;", src)
    assert decl is not None
    args = [a.strip() for a in decl.group(1).split(",")]
    assert len(args) == 14 and args[7] == "const int32_t* lengths"
    assert "dsd_vocode_ragged" in _lib.EXPORTS
    assert len(_lib.lib().dsd_vocode_ragged.argtypes) == 14
    assert _lib.lib().dsd_api_version() == 10        # additive: the version stays


def test_vocode_ragged_rejects_null_handle_and_null_lengths():
    from diffsinger_amd import _lib
    lib = _lib.lib()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    lens = (C.c_int32 * 2)(4, 2)
    assert lib.dsd_vocode_ragged(None, p, 2, 4, 128, 1, 32, lens, p, p, p, None, p, None) == DSD_EINVAL
    assert b"null" in lib.dsd_last_error(None)
    assert lib.dsd_vocode_ragged(None, p, 2, 4, 128, 1, 32, None, p, p, p, None, p, None) == DSD_EINVAL
    assert b"lengths" in lib.dsd_last_error(None)


def test_generator_forward_accepts_lengths():
    import torch
    from diffsinger_amd import synth
    from diffsinger_amd.vocoder import Generator
    sig = inspect.signature(Generator.forward)
    assert "lengths" in sig.parameters and sig.parameters["lengths"].kind == inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters["lengths"].default is None
    h = dict(synth.NSF_HIFIGAN_DEFAULT, num_mels=32, upsample_rates=[4, 2, 2], upsample_kernel_sizes=[8, 4, 4],
             upsample_initial_channel=64, resblock_kernel_sizes=[3], resblock_dilation_sizes=[[1]], hop_size=16)
    gen = Generator(h)
    with torch.no_grad():
        with pytest.raises(ValueError, match="lengths"):          # checked before any device work
            gen(torch.zeros(2, 32, 4), torch.zeros(2, 4), lengths=[4, 5])
        with pytest.raises(ValueError, match="lengths"):
            gen(torch.zeros(2, 32, 4), torch.zeros(2, 4), lengths=[4])
        with pytest.raises(ValueError, match="lengths"):
            gen(torch.zeros(2, 32, 4), torch.zeros(2, 4), lengths=[0, 4])
        if not torch.cuda.is_available():
            with pytest.raises(RuntimeError, match="no CPU path"):
                gen(torch.zeros(2, 32, 4), torch.zeros(2, 4), lengths=[4, 2])
