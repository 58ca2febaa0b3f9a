"""No GPU: the boundary of the three entries that let a C process render a project - dsd_acoustic_set_lengths,
dsd_acoustic_spk_mix / dsd_variance_spk_mix, dsd_vocode_seeded.  The two new structs against their ctypes mirrors (pinned
numbers, and what a C compiler makes of the header), the exports, and the refusals that need no device."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from diffsinger_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
NEW = ("dsd_acoustic_set_lengths", "dsd_acoustic_spk_mix", "dsd_variance_spk_mix", "dsd_vocode_seeded")
MIX = dict(struct_size=0, B=4, rows=8, N=12, ids=16, values=24, normalize=32, out=40)
VOC = dict(struct_size=0, B=4, T=8, vocoder=16, mel=24, stride_b=32, stride_m=40, stride_t=48, lengths=56, f0=64, seeds=72, wav_out=80)


def test_struct_layouts_are_pinned():
    for mirror, want, size in ((_lib.DsdSpkMixArgs, MIX, 48), (_lib.DsdVocodeSeededArgs, VOC, 88)):
        assert C.sizeof(mirror) == size
        assert [n for n, _ in mirror._fields_] == list(want)
        assert {n: getattr(mirror, n).offset for n in want} == want


def test_struct_layouts_match_what_a_c_compiler_sees(tmp_path):
    """sizeof and offsetof of every field, printed by a C99 program that includes the header alone"""
    assert shutil.which("gcc"), "the layout check compiles the header"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dsdenoise.h"', 'int main(void) {']
    for struct, want in (("dsd_spk_mix_args", MIX), ("dsd_vocode_seeded_args", VOC)):
        lines.append(f'    printf("{struct} sizeof %zu\\n", sizeof({struct}));')
        lines += [f'    printf("{struct} {n} %zu\\n", offsetof({struct}, {n}));' for n in want]
    lines.append('    printf("domains %d %d %d %d %d\\n", DSD_DOMAIN_X_T, DSD_DOMAIN_STEP, DSD_DOMAIN_VOC_SOURCE, DSD_DOMAIN_VOC_PRE, '
                 'DSD_DOMAIN_VOC_PHASE);')
    lines += ['    return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, timeout=120)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.split("\n")
    got = {}
    for line in out:
        if line and not line.startswith("domains"):
            struct, name, value = line.split()
            got.setdefault(struct, {})[name] = int(value)
    for struct, mirror in (("dsd_spk_mix_args", _lib.DsdSpkMixArgs), ("dsd_vocode_seeded_args", _lib.DsdVocodeSeededArgs)):
        fields = got[struct]
        assert fields.pop("sizeof") == C.sizeof(mirror), struct
        assert fields == {n: getattr(mirror, n).offset for n, _ in mirror._fields_}, struct
    from diffsinger_amd import noise
    assert [line for line in out if line.startswith("domains")] == ["domains 1 2 3 4 5"]
    assert (noise.X_T, noise.STEP, noise.VOC_SOURCE, noise.VOC_PRE, noise.VOC_PHASE) == (1, 2, 3, 4, 5)
    assert (_lib.DSD_DOMAIN_X_T, _lib.DSD_DOMAIN_STEP, _lib.DSD_DOMAIN_VOC_SOURCE, _lib.DSD_DOMAIN_VOC_PRE, _lib.DSD_DOMAIN_VOC_PHASE) == \
        (1, 2, 3, 4, 5)


def test_new_names_are_exported_and_the_version_stays():
    lib = C.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert n in _lib.EXPORTS and hasattr(lib, n), n
    assert _lib.DSD_API_VERSION == 10 == _lib.lib().dsd_api_version() and _lib.DSD_MODEL_FORMAT_VERSION == 1
    header = open(os.path.join(ROOT, "include", "dsdenoise.h")).read()
    for n in NEW:
        assert f"int {n}(" in header, n


def test_refusals_that_need_no_device():
    lib = _lib.lib()
    assert lib.dsd_vocode_seeded(None, None) == EINVAL
    assert lib.dsd_last_error(None) == b"dsd_vocode_seeded: null args"
    a = _lib.DsdVocodeSeededArgs()
    for size in (0, C.sizeof(a) - 8, C.sizeof(a) + 8):
        a.struct_size = size
        assert lib.dsd_vocode_seeded(C.byref(a), None) == EINVAL
        assert b"dsd_vocode_seeded: struct_size" in lib.dsd_last_error(None)
    a.struct_size = C.sizeof(a)                     # the struct in order, its handle NULL: dsd_vocode's own refusal
    assert lib.dsd_vocode_seeded(C.byref(a), None) == EINVAL and b"dsd_vocode_seeded: null argument" in lib.dsd_last_error(None)
    m = _lib.DsdSpkMixArgs()
    m.struct_size = C.sizeof(m)
    lens = (C.c_int32 * 2)(3, 4)
    for call, args in ((lib.dsd_acoustic_spk_mix, (C.byref(m), None)), (lib.dsd_variance_spk_mix, (C.byref(m), None)),
                       (lib.dsd_acoustic_set_lengths, (lens, 2, None))):
        assert call(None, *args) == EINVAL
        assert b"NULL object" in lib.dsd_last_error(None)
