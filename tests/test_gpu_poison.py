"""-m gpu: what a call may read.  Every handle keeps its device workspace between calls; the library's contract is

  1. what a call leaves in the workspace never reaches a later result (halo columns past T, the tiles a ragged call skips, the
     guard floats, the rows of a padded width, the state buffers and step tables of dsd_sample),
  2. what the caller has past an item's end in a ragged batch never reaches that item's valid frames,
  3. a handle's result does not depend on the calls before it.

On finite O(1) leftovers a mask written as a multiply, or a read of a column nobody wrote, passes every comparison with an
oracle.  Here the leftovers are NaN (and the caller's padding NaN, then +inf), and every comparison is torch.equal /
np.array_equal between two runs of the same kernels on the same valid inputs, on the frames the caller keeps: the whole tensor
of a dense call, per item its valid frames of a ragged one.  No tolerances.

Part A  every case of kernel_ledger_cases.CASES (all 293 instantiations, under the switches that select each), on one handle:
        clean -> ref (finite); a dense all-NaN call at the case's (B, T), the diffusion step NaN too; clean again == ref;
        ragged cases: NaN, then +inf past every item's end == ref on the valid frames.  The ledger is zeroed before each compared
        call and the case's targets must be among what ran: the poison met the form under test.
Part B  dsd_sample on program_cases' two graph rows: a NaN run (x_T, step noise and cond, written in place: the noise pointer is
        part of the graph key), then eager, captured, a NaN replay of the cached graph and a clean replay, each clean result equal
        to a fresh rig's; gen8 after the 64-buffer program and its NaN run.
Part C  one used handle per family walks a list of calls with natural plans (no switches) - a shape, a smaller one (the arena is
        re-carved and cleared on the stream), NaN dirt, a ragged call right after dense dirt, a larger shape (the arena is
        reallocated), split-bf16 and back - and after every call a fresh handle given the same call returns the same bits;
        repeats of a call equal each other.  A dirt call's own output is NaN and is not compared.

Where NaN may go.  Read for a data value that becomes an index, a trip count or a bound ((int) of a float, lrintf, floorf feeding
an address, a loop bounded by a value):
  denoisers, aux decoder    the GEMM paths, the fused / row-split / edge / resident layer kernels and dwconv_* use data only
                            arithmetically; the diffusion step feeds sinf / cosf only: NaN.
  vocoder                   voc_phase_kernel / voc_source_kernel: fmodf, sinf and `f0 > 0` on the data, every index from the sample
                            number: NaN.
  mel analysis              mel_kernels.hip indexes by frame and bin only; the clamp is fmaxf on the value: NaN.
  separator and its curves  hnsep_kernels.hip: the f0 bin mask compares `(float)bin` with bounds computed from f0 (no conversion), the
                            network, the RMS and the curve kernels are arithmetic and compares: NaN in the waveforms.  f0 itself stays
                            valid: base_harmonic interpolates it on the host before the call.
  RMVPE                     the decode, local-average and Viterbi kernels choose indices by comparing values, and the Viterbi
                            backtrace reads a stored state as the next index (rmvpe_kernels.hip, `state = min((int)rows[..], ..)`):
                            loud finite dirt instead - the waveforms times 1e4 at another length.
The point is unmasked reads, not odd control flow."""
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import analysis_config_cases as ac  # noqa: E402
import kernel_ledger_cases as lc  # noqa: E402
import mel_config_cases as mc  # noqa: E402
import mel_ref  # noqa: E402
import poison_cases as pz  # noqa: E402
import program_cases as pc  # noqa: E402
import test_gpu_programs as tp  # noqa: E402
from diffsinger_amd import _lib, hnsep  # noqa: E402
from gpu_util import set_hp  # noqa: E402
from test_gpu_first_capture import SWITCHES  # noqa: E402
from test_kernel_registry import demangle  # noqa: E402

NAN, INF = float("nan"), float("inf")


@pytest.fixture(autouse=True)
def _clean_env():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    set_hp()
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    yield
    for k in SWITCHES:
        os.environ.pop(k, None)
        if saved[k] is not None:
            os.environ[k] = saved[k]


@pytest.fixture(scope="module")
def names():
    """the ledger's entries in registry order, as 'kernel<template arguments>'"""
    rows = _lib.kernel_ledger()
    assert rows and all(sym for sym, _, _ in rows)
    return [re.sub(r"^void dsd::|\(.*$", "", n) for n in demangle([sym for sym, _, _ in rows])]


def ran(names):
    return {n for n, (_, _, count) in zip(names, _lib.kernel_ledger()) if count}


_handles = {}       # poison_cases.handle_key -> Handle, shared by the cases of part A


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    for h in _handles.values():
        pz.release(h)
    _handles.clear()


def kept(case, out):
    """the frames the caller keeps: the whole tensor of a dense call, per item its valid frames of a ragged one"""
    lengths = pz.grid(case)[2]
    return [out] if lengths is None else [pz.valid(case, out, b, n) for b, n in enumerate(lengths)]


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def worst(a, b):
    return max(float((x - y).abs().nan_to_num(nan=INF).max()) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ part A: every instantiation
@pytest.mark.parametrize("case", lc.CASES, ids=[c.id for c in lc.CASES])
def test_part_a_case_survives_a_poisoned_workspace_and_padding(case, names):
    os.environ.update(case.env)
    key = pz.handle_key(case)
    if key not in _handles:
        _handles[key] = pz.make_handle(case)
    h = _handles[key]
    lengths = pz.grid(case)[2]
    clean = pz.clean(case)
    pz.set_precision(h, case.precision)
    try:
        if lengths is not None:         # as in test_gpu_kernel_ledger.py: the skipped tiles hold a dense call's values
            pz.call(h, clean)
        ref = kept(case, pz.call(h, clean, lengths))
        assert all(torch.isfinite(r).all() for r in ref), case.id

        pz.call(h, pz.all_of(case, NAN))            # dense, at the case's (B, T): every float the workspace holds is dirty
        runs = [("clean after an all-NaN call", clean)]
        if lengths is not None:
            runs += [("NaN past every item's end", pz.padded_with(case, NAN)), ("+inf past every item's end", pz.padded_with(case, INF))]
        for what, inputs in runs:
            got = kept(case, pz.call(h, inputs, lengths, _lib.kernel_ledger_reset))
            launched = ran(names)
            missing = [t for t in case.targets if t not in launched]
            assert not missing, (case.id, what, "did not run", missing, "ran", sorted(launched))
            assert same(got, ref), (case.id, what, [int((~torch.isfinite(g)).sum()) for g in got], worst(got, ref))
    finally:
        pz.set_precision(h, "f32")


# ------------------------------------------------------------------------------------------------ part B: dsd_sample
def _poison_rig(row, tag):
    rig = tp.make_rig(row.net)
    rig.name = f"{row.net}#poison-{tag}"        # its own device inputs: they are overwritten in place here
    return rig


def _drop(rig):
    rig.net.release_native()
    for k in [k for k in tp._inputs if k[0] == rig.name]:
        del tp._inputs[k]


def _fill(i, value=None):
    """NaN (or `value`) into x_T, the step noise and the cond in place; None: the clean values back"""
    for d, host in ((i.xd, i.x), (i.cd, i.cond), (i.nd, i.noise)):
        if value is None:
            d.copy_(torch.from_numpy(np.ascontiguousarray(host)))
        else:
            d.fill_(value)
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", ["gen8", "noise3", "bufs64"])
@pytest.mark.parametrize("row_id", tp.GRAPH_ROWS)
def test_part_b_sample_after_nan_runs_eager_captured_and_replayed(row_id, name):
    row, prog = tp.ROW[row_id], pc.PROGRAMS[name]
    grid = row.dense
    os.environ.update(row.env)
    fresh, used = _poison_rig(row, "fresh"), _poison_rig(row, "used")
    try:
        want = tp.sample(fresh, prog, grid)
        assert torch.isfinite(want).all()
        i = tp.inputs(used, grid[0], grid[1])
        cached = lambda: used.net.stats()["graphs_cached"]  # noqa: E731

        _fill(i, NAN)                                                   # 1
        assert not torch.isfinite(tp.sample(used, prog, grid)).any()
        _fill(i)                                                        # 2
        got = tp.sample(used, prog, grid)
        assert torch.equal(got, want), (row_id, name, "eager after a NaN run", worst([got], [want]))
        c0 = cached()                                                   # 3
        got = tp.sample(used, prog, grid, graph=True)
        assert cached() == c0 + 1
        assert torch.equal(got, want), (row_id, name, "captured", worst([got], [want]))
        _fill(i, NAN)                                                   # 4
        assert not torch.isfinite(tp.sample(used, prog, grid, graph=True)).any()
        _fill(i)                                                        # 5
        got = tp.sample(used, prog, grid, graph=True)
        assert cached() == c0 + 1, "steps 4 and 5 replay the graph of step 3"
        assert torch.equal(got, want), (row_id, name, "replayed after a NaN replay", worst([got], [want]))

        if name == "bufs64":                                            # 6
            _fill(i, NAN)
            for b in pc.compared(prog):
                tp.sample(used, prog, grid, b)
            _fill(i)
            gen8, fresh8 = pc.PROGRAMS["gen8"], _poison_rig(row, "fresh8")
            try:
                for b in pc.compared(gen8):
                    got, want8 = tp.sample(used, gen8, grid, b), tp.sample(fresh8, gen8, grid, b)
                    assert torch.isfinite(want8).all()
                    assert torch.equal(got, want8), (row_id, "gen8 after bufs64 and its NaN run, buffer", b, worst([got], [want8]))
            finally:
                _drop(fresh8)
    finally:
        _drop(fresh)
        _drop(used)


# ------------------------------------------------------------------------------------------------ part C: a handle's history
def walk(make, release, steps):
    """steps: [(label, call(handle) -> list of tensors, dirt)].  After every call that is no dirt a fresh handle given the same
    call returns the same bits, and calls with the same label return the same bits."""
    used, seen = make(), {}
    try:
        for k, (label, call, dirt) in enumerate(steps):
            got = [g.clone() for g in call(used)]
            if dirt:
                continue
            fresh = make()
            try:
                want = [w.clone() for w in call(fresh)]
            finally:
                release(fresh)
            assert all(torch.isfinite(w).all() for w in want), (k, label)
            assert same(got, want), (k, label, "differs from a fresh handle's", worst(got, want))
            assert same(got, seen.setdefault(label, got)), (k, label, "differs from the same call earlier")
        assert any(dirt for _, _, dirt in steps) and len(seen) < sum(not dirt for _, _, dirt in steps)
    finally:
        release(used)


def ledger_family_steps(kind, key, shapes, ragged, x3):
    """the list of the issue for a family of the ledger table: shapes = (a, smaller, larger) as (B, T); ragged: lengths at a"""
    def case(shape, lengths=None, precision="f32"):
        spec = (key + shape + (lengths,)) if kind == "vocoder" else (key,) + shape + (lengths,)
        return lc.Case(f"history-{shape[0]}x{shape[1]}", (), kind, spec, {}, precision, ())

    def step(label, c, build=pz.clean, dirt=False):
        def call(h):
            pz.set_precision(h, c.precision)
            return kept(c, pz.call(h, build(c), pz.grid(c)[2]))
        return label, call, dirt

    a, small, large = (case(s) for s in shapes)
    rag = case(shapes[0], ragged)
    nan = lambda c: pz.all_of(c, NAN)  # noqa: E731
    steps = [step("a", a), step("small", small), step("a", a), step("nan", a, nan, True), step("a", a),
             step("nan", a, nan, True), step("a ragged", rag), step("a ragged", rag, lambda c: pz.padded_with(c, NAN)),
             step("large", large), step("a", a)]
    if x3:
        steps += [step("a bf16x3", case(shapes[0], None, "bf16x3")), step("a", a), step("nan", case(shapes[0], None, "bf16x3"), nan, True),
                  step("a ragged bf16x3", case(shapes[0], ragged, "bf16x3")), step("a", a)]
    return steps


BACKBONE_SHAPES = ((2, 70), (1, 5), (4, 211))
LEDGER_FAMILIES = {
    "wn256": ("wavenet", "wn256", BACKBONE_SHAPES, [70, 33], True),
    "lx512_e2": ("lynxnet", "lx512_e2", BACKBONE_SHAPES, [70, 33], True),
    "aux256": ("aux", "aux256", BACKBONE_SHAPES, [70, 33], False),
    "aux72": ("aux", "aux72", BACKBONE_SHAPES, [70, 33], False),
    # vocoder_config_cases' x3_c320: three stages, the first (160 channels) on the split-bf16 kernels when asked
    "vocoder": ("vocoder", ("configs", "x3_c320"), ((2, 37), (1, 5), (4, 130)), [37, 16], True),
}


@pytest.mark.parametrize("family", list(LEDGER_FAMILIES))
def test_part_c_result_does_not_depend_on_the_handles_history(family):
    kind, key, shapes, ragged, x3 = LEDGER_FAMILIES[family]
    steps = ledger_family_steps(kind, key, shapes, ragged, x3)
    probe = lc.Case("history", (), kind, (key + shapes[0] + (None,)) if kind == "vocoder" else (key,) + shapes[0] + (None,), {}, "f32", ())
    walk(lambda: pz.make_handle(probe), pz.release, steps)


# ---- the analysis families: DevBuf::reserve never clears, a fresh handle starts on whatever hipMalloc returned
def _dev(y):
    return torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32)).cuda()


def test_part_c_mel_analysis_history():
    """mel_config_cases' `tiny` configuration (33 bins, 16-sample hop): shortest items first, then longest, then ragged"""
    from diffsinger_amd.mel import STFT
    c = mc.TINY
    make = lambda: STFT(c["sr"], c["n_mels"], c["n_fft"], c["win_size"], c["hop"], c["fmin"], c["fmax"], clip_val=c["clip"])  # noqa: E731
    wave = lambda seed, n: mel_ref.waveform(seed, n, c["sr"])  # noqa: E731
    short, long_, rag = [wave(2651, 200), wave(2652, 150)], [wave(2653, 1200), wave(2654, 1100)], [wave(2653, 1200), wave(2655, 80), wave(2656, 500)]

    def step(label, clips, dirt=False, **kw):
        def call(st):
            ys = [_dev(np.full_like(y, NAN) if dirt else y) for y in clips]
            out = st.get_mel_ragged(ys, **kw)
            torch.cuda.synchronize()
            return out
        return label, call, dirt

    def dense(label, clips):
        def call(st):
            out = st.get_mel(torch.stack([_dev(y[:1100]) for y in clips]))
            torch.cuda.synchronize()
            return [out]
        return label, call, False

    walk(make, lambda st: None, [
        step("short", short), step("long", long_), step("short", short), step("nan", long_, True), step("long", long_),
        step("nan", long_, True), step("ragged", rag), dense("dense", long_), step("nan", rag, True), step("shifted", rag, keyshift=2.5, speed=0.9),
        step("ragged", rag), step("short", short)])


@pytest.mark.parametrize("use_viterbi", [False, True], ids=["argmax", "viterbi"])
def test_part_c_rmvpe_history(use_viterbi):
    """analysis_config_cases' e1_c8 network on its 21- and 41-frame clips; the dirt is loud and finite (the module docstring)"""
    from diffsinger_amd.pitch import RMVPE
    tag = "e1_c8"
    sd = ac.rmvpe_sd(tag)
    short, long_ = ac.rmvpe_clips(tag)
    other = ac._rmvpe_waveform(2291, 160 * 30 + 1)             # another length: 31 frames

    def step(label, clips, dirt=False):
        def call(pe):
            res = pe.infer_from_audio_ragged([np.asarray(y, np.float32) * np.float32(1e4 if dirt else 1) for y in clips], 16000,
                                             want_hidden=True, use_viterbi=use_viterbi)
            torch.cuda.synchronize()
            return [torch.from_numpy(np.ascontiguousarray(v)) for f0, hid in res for v in (f0, hid)]
        return label, call, dirt

    loud = [other, other[:160 * 9 + 5]]
    walk(lambda: RMVPE(sd), lambda pe: None, [
        step("short", [short]), step("long", [long_, long_[::-1].copy()]), step("short", [short]), step("loud", loud, True),
        step("long", [long_, long_[::-1].copy()]), step("loud", loud, True), step("ragged", [long_, short, short[:160 * 6 + 1]]),
        step("short", [short]), step("ragged", [long_, short, short[:160 * 6 + 1]])])


def test_part_c_separator_and_curves_history():
    """analysis_config_cases' f128_h32_n4 separator (1293- and 300-sample clips), with dsd_base_harmonic and dsd_variance_curves at
    (win, hop) = (64, 32) interleaved on the same handle: the three share its workspace"""
    tag, win, hop = "f128_h32_n4", 64, 32
    cfg, sd = ac.HNSEP[tag]["cfg"], ac.hnsep_sd(tag)
    long_, short = ac.hnsep_clips(tag)
    hs = [ac.base_clip(win, hop, i) for i in range(2)]
    f0s = [ac.base_f0(win, len(h) // hop + 1, i) for i, h in enumerate(hs)]
    frames = [len(h) // hop + 1 for h in hs]
    poison = lambda ys, dirt: [np.full_like(y, NAN) if dirt else y for y in ys]  # noqa: E731

    def sep(label, clips, dirt=False):
        def call(sp):
            out = sp.separate_ragged(poison(clips, dirt))
            torch.cuda.synchronize()
            return out
        return label, call, dirt

    def base(label, dirt=False):
        def call(sp):
            out = sp.base_harmonic_ragged(poison(hs, dirt), f0s, ac.SR, hop, win)
            torch.cuda.synchronize()
            return out
        return label, call, dirt

    def curves(label, dirt=False):
        def call(sp):
            xs, hh = poison(hs, dirt), poison([(0.7 * h).astype(np.float32) for h in hs], dirt)
            cv = sp.curves_ragged(xs, hh, poison([(0.6 * h).astype(np.float32) for h in hh], dirt), frames, hop, win, domain="ratio")
            torch.cuda.synchronize()
            return [torch.from_numpy(v) for k in sorted(cv) for v in cv[k]]
        return label, call, dirt

    walk(lambda: hnsep.HnSep(sd, cfg), lambda sp: None, [
        sep("short", [short]), sep("long", [long_]), sep("short", [short]), sep("nan", [long_], True), sep("long", [long_]),
        sep("nan", [long_, long_], True), sep("ragged", [long_, short]), base("base"), curves("curves"), base("nan", True),
        curves("curves"), curves("nan", True), base("base"), sep("ragged", [long_, short]), sep("nan", [long_, short], True),
        curves("curves"), sep("short", [short])])
