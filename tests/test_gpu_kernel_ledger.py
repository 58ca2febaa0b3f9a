"""Every kernel instantiation the library can launch, run by a case that passed its comparison with the oracle.

The hot path is a few heavily templated kernels and the host picks one instantiation per launch - from the grid, the channel
count, the dilation, dense or ragged, the precision and the path switches.  The rest of the suite compares models with the
oracle at many shapes, but nothing there says WHICH instantiation a shape ran, so a form no test reaches, or a ragged twin that
is wrong only in its length mask, would go unnoticed.  The launch ledger (dsd_kernel_ledger: one launch counter per entry of the
kernel registry) says it.

Per case of kernel_ledger_cases.py: build (or reuse) the handle, for a ragged case run the dense call first, zero the ledger,
run the case's one call, compare it with the family's numpy oracle at the tolerance the family's own test uses (imported from
there, not restated: TOL_NFE of test_gpu_config_sweep.py for one backbone evaluation, split-bf16 included as in
test_gpu_bf16x3.py; the bound of vocoder_config_cases.py / TOL of test_gpu_vocoder_x3.py for the vocoder; a ragged batch per
item on its valid frames against the oracle run alone at that length), then read the instantiations with a non-zero count.
They are credited to the case only now, after the comparison, and the case's targets must be among them.

Completeness, per kernel group: the union of what the group's cases were credited with is the group's whole ledger - no
allowlist.  The test fails, naming them, if a case of the group did not run or did not pass (so `-k` on a few cases cannot make
it pass over a subset), and lists the uncredited instantiations otherwise.  An instantiation nothing can reach is to be deleted
from the dispatch code, not excused here.

All four groups are complete.  The vocoder's generic-path GEMM forms on 64-frame tiles need a stage with 512 workgroups of 64
frames; the thin late stages of vocoder_config_cases.py's configurations (2 to 12 channels: one row tile, but thousands of
samples) get there at a few hundred mel frames, where the float64 oracle still takes a second or two."""
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_ledger_cases as lc  # noqa: E402
import poison_cases as pz  # noqa: E402
import vocoder_config_cases as vcc  # noqa: E402
import vocoder_x3_cases as vx3  # noqa: E402
from diffsinger_amd import _lib  # noqa: E402
from gpu_util import check, rel_err, set_hp  # noqa: E402
from oracle import aux_decoder as oa  # noqa: E402
from oracle import backbones as ob  # noqa: E402
from test_gpu_aux_decoder import TOL_AUX  # noqa: E402
from test_gpu_config_sweep import TOL_NFE  # noqa: E402
from test_gpu_first_capture import SWITCHES  # noqa: E402
from test_gpu_vocoder_x3 import TOL as TOL_VOCODER_X3  # noqa: E402
from test_kernel_registry import demangle  # noqa: E402

# KernelGroup of dsd_internal.h: every group
COMPLETE_GROUPS = (lc.KG_GEMM, lc.KG_WAVENET, lc.KG_LYNXNET, lc.KG_VOCODER)
CREDIT = {}         # case id -> the instantiations it ran, once its comparison has passed


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
def ledger():
    """-> (names, groups) of the ledger's entries in registry order; names as 'kernel<template arguments>'"""
    rows = _lib.kernel_ledger()
    assert rows and all(sym for sym, _, _ in rows)
    names = [re.sub(r"^void dsd::|\(.*$", "", n) for n in demangle([sym for sym, _, _ in rows])]
    assert len(set(names)) == len(names)
    return names, [g for _, g, _ in rows]


def _ran(ledger):
    return {n for n, (_, _, count) in zip(ledger[0], _lib.kernel_ledger()) if count}


# ------------------------------------------------------------------------------------------------ handles, shared by cases
_handles = {}       # poison_cases.handle_key -> poison_cases.Handle


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    for h in _handles.values():
        pz.release(h)
    _handles.clear()


def _handle(case):
    key = pz.handle_key(case)
    if key not in _handles:
        _handles[key] = pz.make_handle(case)
    return _handles[key]


# ------------------------------------------------------------------------------------------------ one call of each family
# (poison_cases.py has the inputs, the handles and the call itself: test_gpu_poison.py runs the same calls)
def run_backbone(case, reset):
    net_name, bsz, t_len, lengths = case.spec
    kind, in_dims, n_feats, args, _ = lc.NETS[net_name]
    h = _handle(case)
    net, params = h.net, h.params
    i = pz.clean(case)
    x, t, cond = i["x"], i["t"], i["cond"]
    if kind == "wavenet":
        fwd = lambda xx, tt, cc: ob.wavenet_forward(params, xx, tt, cc, dilation_cycle_length=args["dilation_cycle_length"])  # noqa: E731
    else:
        fwd = lambda xx, tt, cc: ob.lynxnet_forward(params, xx, tt, cc, activation=args["activation"], strong_cond=args["strong_cond"])  # noqa: E731
    net.set_precision(case.precision)
    try:
        if lengths is not None:         # the tiles the ragged call skips hold this call's values
            pz.call(h, i)
        out = pz.call(h, i, lengths, reset).cpu().numpy()
        if any("_x3_" in t for t in case.targets) or case.precision == "f32":     # (bf16x3 without a split-bf16 kernel on the
            assert net.stats()["precision"] == (1 if case.precision == "bf16x3" else 0), net.stats()      # plan reports fp32)
        if lengths is None:
            check(out, fwd(x, t, cond), TOL_NFE, what=(case.id,))
        else:                               # frames past an item's end are the caller's to mask
            for b, n in enumerate(lengths):
                check(out[b:b + 1, :, :, :n], fwd(x[b:b + 1, :, :, :n], t[b:b + 1], cond[b:b + 1, :, :n]), TOL_NFE, what=(case.id, b))
    finally:
        net.set_precision("f32")


def run_vocoder(case, reset):
    which, tag, bsz, t_len, lengths = case.spec
    module = pz.voc_module(which)
    x3 = case.precision == "bf16x3"
    h = _handle(case)
    gen, upp = h.net, h.upp
    gen.set_precision(case.precision)
    try:
        i = pz.clean(case)
        if lengths is None:
            got = pz.call(h, i, None, reset)
            assert tuple(got.shape) == (bsz, 1, t_len * upp)
            if which == "configs":          # test_gpu_vocoder_configs.py: the case's bound in fp32, TOL in split-bf16
                # (a shape vocoder_config_cases.FLOORS does not list: TOL itself, which bound() never goes below)
                listed = (tag, bsz, t_len) in vcc.FLOORS
                assert rel_err(got, vcc.reference(tag, bsz, t_len)) < (vcc.bound(tag, bsz, t_len) if listed and not x3 else vcc.TOL), case.id
            else:
                assert rel_err(got, vx3.reference(tag, bsz, t_len)) < TOL_VOCODER_X3, case.id
        else:
            own = lengths != "cases"        # "cases": the module's ragged lengths, whose references the suite shares
            lens = pz.grid(case)[2]
            assert bsz == len(lens) and (which == "configs" if own else t_len == module.RAGGED_T and (which == "configs" or tag == vx3.RAGGED_LAYOUT))
            pz.call(h, i)
            got = pz.call(h, i, lens, reset)
            for b, n in enumerate(lens):
                if own:
                    want = vcc.oracle(tag, vcc.item_inputs(tag, bsz, t_len, b, n), np.float64)
                else:
                    want = vcc.ragged_reference(tag, b) if which == "configs" else vx3.ragged_reference(b)
                assert rel_err(got[b:b + 1, :, :n * upp], want) < (vcc.TOL if which == "configs" else TOL_VOCODER_X3), (case.id, b)
                assert not got[b, 0, n * upp:].any()
        assert gen.stats()["precision"] == (1 if x3 else 0)
    finally:
        gen.set_precision("f32")


def run_aux(case, reset):
    net_name, bsz, t_len, lengths = case.spec
    m = lc.AUX_NETS[net_name][1]
    h = _handle(case)
    params, smin, smax = h.params, h.smin, h.smax
    i = pz.clean(case)
    cond = i["cond"]
    if lengths is not None:
        pz.call(h, i)
    got = pz.call(h, i, lengths, reset).cpu().numpy()
    if lengths is None:
        assert rel_err(got, oa.aux_adaptor_forward(params, cond, m, 1, smin, smax, infer=True)) < TOL_AUX, case.id
    else:
        for b, n in enumerate(lengths):
            assert rel_err(got[b:b + 1, :n], oa.aux_adaptor_forward(params, cond[b:b + 1, :n], m, 1, smin, smax, infer=True)) < TOL_AUX, (case.id, b)


RUNNERS = dict(wavenet=run_backbone, lynxnet=run_backbone, vocoder=run_vocoder, aux=run_aux)


@pytest.mark.parametrize("case", lc.CASES, ids=[c.id for c in lc.CASES])
def test_case_runs_its_instantiations_and_agrees_with_the_oracle(case, ledger):
    os.environ.update(case.env)
    RUNNERS[case.kind](case, _lib.kernel_ledger_reset)          # raises unless the comparison passed
    ran = _ran(ledger)
    print(case.id, "ran", sorted(ran))
    missing = [t for t in case.targets if t not in ran]
    assert not missing, (case.id, "did not run", missing, "ran", sorted(ran))
    CREDIT[case.id] = ran


def test_ledger_counts_launches_and_resets(ledger):
    """the counters themselves: a call adds to the entries it launches and to no other, a reset zeroes them"""
    case = next(c for c in lc.CASES if c.kind == "wavenet" and c.spec[3] is None)
    os.environ.update(case.env)
    run_backbone(case, _lib.kernel_ledger_reset)
    once = {n: c for n, (_, _, c) in zip(ledger[0], _lib.kernel_ledger()) if c}
    assert set(case.targets) <= set(once) and len(once) < len(ledger[0])
    run_backbone(case, lambda: None)
    twice = {n: c for n, (_, _, c) in zip(ledger[0], _lib.kernel_ledger()) if c}
    assert set(twice) == set(once) and all(twice[n] == 2 * once[n] for n in case.targets), (once, twice)
    _lib.kernel_ledger_reset()
    assert not _ran(ledger)


@pytest.mark.parametrize("group", COMPLETE_GROUPS, ids=[f"group{g}" for g in COMPLETE_GROUPS])
def test_every_instantiation_of_the_group_is_credited(group, ledger):
    cases = [c for c in lc.CASES if group in c.groups]
    assert cases
    absent = [c.id for c in cases if c.id not in CREDIT]
    assert not absent, f"group {group}: these cases did not run or did not pass, so nothing is asserted over the rest: {absent}"
    entries = {n for n, g in zip(*ledger) if g == group}
    credited = set().union(*(CREDIT[c.id] for c in cases)) & entries
    assert len(entries) > 0 and len(credited) == len(entries), (
        f"group {group}: {len(entries)} instantiations registered, {len(credited)} credited; no case that passed its "
        f"comparison ran {sorted(entries - credited)}")
