"""No GPU: the boundary of the score algebra - dsd_word_dur, dsd_group_midi, dsd_rhythm_align, dsd_variance_set_lengths.  The
exports and the three args structs (pinned numbers, and what a C compiler makes of the header), every DSD_EINVAL that needs
no device, the numpy oracle of tests/words_ref.py against the reference's own results (G30: RhythmRegulator and the
ds_variance.py expressions; G13: preprocess_input's word_dur and midi of every segment in all three modes), the kernel
file under the resource and store-hazard checks, and the stand-alone sanitizer run of the host code
(tools/harness/words_harness.cpp)."""
import ctypes as C
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from diffsinger_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
sys.path.insert(0, HERE)
import words_cases as wc  # noqa: E402
import words_ref as wr  # noqa: E402

EINVAL = -1
NEW = ("dsd_word_dur", "dsd_group_midi", "dsd_rhythm_align", "dsd_variance_set_lengths")
WORD = dict(struct_size=0, B=4, N=8, W=12, dur=16, index=24, slur=32, totals=40, word_dur=48, index_out=56)
MIDI = dict(struct_size=0, B=4, Nn=8, G=12, L=16, T=20, note_midi=24, note_dur=32, group_dur=40, ph2word=48, midi=56)
RHYTHM = dict(struct_size=0, B=4, L=8, W=12, ph_dur_pred=16, ph2word=24, word_dur=32, ph_dur=40)
STRUCTS = (("dsd_word_dur_args", _lib.DsdWordDurArgs, WORD, 64), ("dsd_group_midi_args", _lib.DsdGroupMidiArgs, MIDI, 64),
           ("dsd_rhythm_align_args", _lib.DsdRhythmAlignArgs, RHYTHM, 48))


def test_new_names_are_exported_and_the_version_stays():
    lib = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "dsdenoise.h")).read()
    for n in NEW:
        assert n in _lib.EXPORTS and hasattr(lib, n), n
        assert f"int {n}(" in header, n
    assert _lib.DSD_API_VERSION == 10 == _lib.lib().dsd_api_version()


def test_struct_layouts_are_pinned_and_match_what_a_c_compiler_sees(tmp_path):
    for _, mirror, want, size in STRUCTS:
        assert C.sizeof(mirror) == size
        assert [n for n, _ in mirror._fields_] == list(want)
        assert {n: getattr(mirror, n).offset for n in want} == want
    assert shutil.which("gcc"), "the layout check compiles the header"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dsdenoise.h"', 'int main(void) {']
    for struct, _, want, _ in STRUCTS:
        lines.append(f'    printf("{struct} sizeof %zu\\n", sizeof({struct}));')
        lines += [f'    printf("{struct} {n} %zu\\n", offsetof({struct}, {n}));' for n in want]
    lines += ['    return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, timeout=120)
    got = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.split("\n"):
        if line:
            struct, name, value = line.split()
            got.setdefault(struct, {})[name] = int(value)
    for struct, mirror, _, _ in STRUCTS:
        fields = got[struct]
        assert fields.pop("sizeof") == C.sizeof(mirror), struct
        assert fields == {n: getattr(mirror, n).offset for n, _ in mirror._fields_}, struct


# ---- refusals: every check stands before the device is selected, so none of these touches one -----------------------------
def _word(**kw):
    a = _lib.DsdWordDurArgs(C.sizeof(_lib.DsdWordDurArgs), 2, 8, 4, 0x1000, 0x1000, None, None, 0x1000, None)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _midi(**kw):
    a = _lib.DsdGroupMidiArgs(C.sizeof(_lib.DsdGroupMidiArgs), 2, 3, 4, 5, 9, 0x1000, 0x1000, 0x1000, 0x1000, 0x1000)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _rhythm(**kw):
    a = _lib.DsdRhythmAlignArgs(C.sizeof(_lib.DsdRhythmAlignArgs), 2, 5, 3, 0x1000, 0x1000, 0x1000, 0x1000)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


BAD_COUNTS = (0, -1, 2049, -2**31, 2**31 - 1)
BAD_B = (0, -1, 65536, -2**31)


def _refusals():
    out = []
    for make, name, ptrs, counts in ((_word, "dsd_word_dur", ("dur", "word_dur"), ("N", "W")),
                                     (_midi, "dsd_group_midi", ("note_midi", "note_dur", "group_dur", "midi"), ("Nn", "G", "L")),
                                     (_rhythm, "dsd_rhythm_align", ("ph_dur_pred", "ph2word", "word_dur", "ph_dur"), ("L", "W"))):
        out += [(name, make(struct_size=s), "struct_size") for s in (0, 8, 4096)]
        out += [(name, make(**{p: None}), "NULL") for p in ptrs]
        out += [(name, make(B=b), "B = ") for b in BAD_B]
        out += [(name, make(**{c: v}), f"{c} = ") for c in counts for v in BAD_COUNTS]
    out.append(("dsd_word_dur", _word(index=None), "exactly one of index and slur"))
    out.append(("dsd_word_dur", _word(slur=0x1000), "exactly one of index and slur"))
    for t in (-1, 2**31, -2**63, 2**63 - 1):
        out.append(("dsd_word_dur", _word(totals=(C.c_int64 * 2)(7, t)), "totals[1]"))
    out.append(("dsd_group_midi", _midi(ph2word=None), "without ph2word"))
    out += [("dsd_group_midi", _midi(T=t), "T = ") for t in (0, -1, -2**31)]
    return out


def test_every_einval_without_a_device():
    lib = _lib.lib()
    for name in NEW[:3]:
        assert getattr(lib, name)(0, None, None) == EINVAL
        assert lib.dsd_last_error(None) == f"{name}: NULL args".encode()
    cases = _refusals()
    assert len(cases) == 76
    for name, args, text in cases:
        assert getattr(lib, name)(0, C.byref(args), None) == EINVAL, (name, text)
        msg = lib.dsd_last_error(None).decode()
        assert msg.startswith(name + ": ") and text in msg, (name, text, msg)
    lens = (C.c_int32 * 2)(3, 4)
    assert lib.dsd_variance_set_lengths(None, lens, 2, None) == EINVAL
    assert lib.dsd_last_error(None) == b"dsd_variance_set_lengths: NULL object"
    assert lib.dsd_variance_set_lengths(None, None, 0, None) == EINVAL


# ---- the oracle against the reference's results --------------------------------------------------------------------
@pytest.fixture(scope="module")
def g30():
    return np.load(os.path.join(GOLDEN, "g30_words.npz"))


def test_oracle_equals_g30(g30):
    seen = 0
    for name, c in wc.rhythm_cases().items():
        if not c.get("oracle_only"):
            assert np.array_equal(wr.rhythm_align(c["pred"], c["ph2word"], c["word_dur"]), g30[f"rhythm_{name}"]), name
            seen += 1
    for name, c in wc.word_cases().items():
        if not c.get("oracle_only"):
            got, _ = wr.word_dur(c["dur"], c["W"], index=c.get("index"), slur=c.get("slur"), totals=c["totals"])
            assert np.array_equal(got, g30[f"word_{name}"]), name
            seen += 1
    for name, c in wc.midi_cases().items():
        if not c.get("oracle_only"):
            got = wr.group_midi(c["note_midi"], c["note_dur"], c["group_dur"], c["T"], c["ph2word"])
            assert np.array_equal(got, g30[f"midi_{name}"]), name
            seen += 1
    assert seen == len(g30.files) == 18
    # the ties the cases were built for: 1.5 -> 2 and 0.5 -> 0
    assert g30["rhythm_ties"].tolist() == [[2, 2, 0, 0], [0, 0, 0, 0]]
    assert g30["word_rest_skips_zero"].tolist() == [[5, 0, 15, 0]]


def test_oracle_equals_g13():
    """the reference's preprocess_input: word_dur and midi of every segment in all three modes"""
    with open(os.path.join(GOLDEN, "g13_variance_segments.ds"), encoding="utf8") as f:
        segs = json.load(f)
    g = np.load(os.path.join(GOLDEN, "g13_variance_harness.npz"))
    seen = {True: 0, False: 0}
    for mode in ("auto", "pitch_only", "dur_energy"):
        for i, seg in enumerate(segs):
            k = f"{mode}_seg{i}_"
            want_wd, want_midi, ph2word = g[k + "word_dur"], g[k + "midi"], g[k + "ph2word"]
            note_midi, note_dur = g[k + "note_midi"], g[k + "note_dur"]
            n_frames, n_words = g[k + "mel2note"].shape[1], want_wd.shape[1]
            with_dur = k + "ph_dur" in g.files
            if with_dur:
                ph_dur = g[k + "ph_dur"]
                wd, _ = wr.word_dur(ph_dur, n_words, index=ph2word, totals=[n_frames])
                midi = wr.group_midi(note_midi, note_dur, ph_dur, n_frames)
            else:
                slur = np.array([[int(s) for s in seg["note_slur"].split()]], bool)
                wd, _ = wr.word_dur(note_dur, n_words, slur=slur, totals=[n_frames])
                midi = wr.group_midi(note_midi, note_dur, wd, n_frames, ph2word)
            assert np.array_equal(wd, want_wd), k
            assert np.array_equal(midi, want_midi), k
            seen[with_dur] += 1
    assert seen[True] >= 2 and seen[False] >= 2


# ---- the kernel file and the host code ---------------------------------------------------------------------------
def test_kernel_resources_and_store_hazard():
    """words_kernels.hip and frames_kernels.hip (they share the prefix sum of dsd_device.h) stay in registers, and the new file
    has no store / VALU-overwrite pair (hipcc cross-compiles; no GPU)."""
    for tool, files in (("check_resources.py", ["words_kernels.hip", "frames_kernels.hip"]), ("check_store_hazard.py", ["words_kernels.hip"])):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), *files], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
        assert "words_kernels.hip" in r.stdout


def test_lds_is_static_and_small():
    """every kernel of the file keeps its rows in static LDS, far below 64 KiB, and is launched with plain <<<>>> (no dynamic
    LDS, nothing for the kernel registry)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_resources
    ks = check_resources.analyse(os.path.join(ROOT, "diffsinger_amd", "csrc", "words_kernels.hip"))
    assert len(ks) == 3
    for k in ks:
        assert 0 < int(k["LDS Size"]) <= 28 * 1024, k
    text = open(os.path.join(ROOT, "diffsinger_amd", "csrc", "words_kernels.hip")).read()
    assert text.count("<<<") == 3 and "launch_timed" not in text and "extern __shared__" not in text


def test_host_code_under_sanitizers(tmp_path):
    """tools/harness/words_harness.cpp: the three entries' argument checks and a loop restatement of their kernels on heap
    arrays of exact size, compiled with the host compiler's address and undefined-behaviour sanitizers into a stand-alone
    program."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = tmp_path / "words_harness"
    # the sanitizer runtimes are linked into the program itself (g++ links them dynamically unless told otherwise; clang
    # links them statically and does not know -static-libubsan)
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) == "g++" else []
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static,
           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "harness", "words_harness.cpp"), "-x", "c++",
           os.path.join(ROOT, "diffsinger_amd", "csrc", "words_api.hip"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert built.returncode == 0, built.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "0 unexpected results" in r.stdout and "words_harness:" in r.stdout
