"""CPU: the builders of tests/poison_cases.py and the coverage of tests/test_gpu_poison.py, without a GPU.

* every ragged case of kernel_ledger_cases.CASES has an item shorter than T: otherwise its padding test poisons nothing;
* padded_with changes exactly the elements past each item's end of the per-frame float inputs (the masks are restated here from
  the lengths by broadcasting, not taken from poison_cases.FRAME_AXES' loop), all_of every float element, and neither writes
  into what clean returns (the vocoder modules share those arrays with the whole suite);
* part A of test_gpu_poison.py is parametrised over every case id of the table, in order, and carries no skip or xfail mark."""
import numpy as np
import pytest

import kernel_ledger_cases as lc
import poison_cases as pz

RAGGED = [c for c in lc.CASES if pz.grid(c)[2] is not None]


def _inputs_key(c):
    """what the builders' results depend on: the family, the grid, and the shapes of the inputs (not the switches, the precision,
    the targets or the weights)"""
    bsz, t_len, lengths = pz.grid(c)
    dims = lc.NETS[c.spec[0]][1:3] if c.kind in ("wavenet", "lynxnet") else lc.AUX_NETS[c.spec[0]][0] if c.kind == "aux" else c.spec[:2]
    return c.kind, dims, bsz, t_len, tuple(lengths or ())


BUILDER_CASES = list({_inputs_key(c): c for c in reversed(lc.CASES)}.values())[::-1]        # the first case of each key


def bits(a):
    return a.view(np.uint32)


def past_end(case, name, shape):
    """the elements of input `name` past each item's end, from the issue's table: x[b, :, :, n:], cond[b, :, n:] (denoisers),
    cond[b, n:] (aux), mel[b, :, n:], f0[b, n:], noise[b, n * upp:], pre_noise[b, :, n:]; nothing of t and rand_ini"""
    _, t_len, lengths = pz.grid(case)
    upp = pz.upp_of(case)
    n = np.asarray(lengths)
    if case.kind in ("wavenet", "lynxnet"):
        m = {"x": (np.arange(t_len)[None, None, None, :] >= n[:, None, None, None]),
             "cond": (np.arange(t_len)[None, None, :] >= n[:, None, None])}.get(name)
    elif case.kind == "aux":
        m = (np.arange(t_len)[None, :, None] >= n[:, None, None]) if name == "cond" else None
    else:
        m = {"mel": (np.arange(t_len)[None, None, :] >= n[:, None, None]),
             "f0": (np.arange(t_len)[None, :] >= n[:, None]),
             "noise": (np.arange(t_len * upp)[None, :, None] >= (n * upp)[:, None, None]),
             "pre_noise": (np.arange(t_len)[None, None, :] >= n[:, None, None])}.get(name)
    return np.zeros(shape, bool) if m is None else np.broadcast_to(m, shape)


def test_the_table_has_ragged_cases_of_every_family():
    assert {c.kind for c in RAGGED} == {"wavenet", "lynxnet", "aux", "vocoder"}
    assert {c.kind for c in BUILDER_CASES if pz.grid(c)[2] is not None} == {"wavenet", "lynxnet", "aux", "vocoder"}


@pytest.mark.parametrize("case", RAGGED, ids=[c.id for c in RAGGED])
def test_every_ragged_case_has_padding(case):
    bsz, t_len, lengths = pz.grid(case)
    assert len(lengths) == bsz and all(1 <= n <= t_len for n in lengths)
    assert min(lengths) < t_len, (case.id, "no item is shorter than T: padded_with would change nothing")


@pytest.mark.parametrize("case", BUILDER_CASES, ids=[c.id for c in BUILDER_CASES])
def test_builders_change_exactly_what_they_claim(case):
    ref = pz.clean(case)
    keep = {k: v.copy() for k, v in ref.items()}
    assert all(v.dtype == np.float32 for v in ref.values()), "an integer input: the builders must leave it alone"
    again = pz.clean(case)
    assert ref.keys() == again.keys() and all(np.array_equal(bits(ref[k]), bits(again[k])) for k in ref)
    assert all(np.isfinite(v).all() for v in ref.values())

    for value in (np.nan, np.inf):
        everything = pz.all_of(case, value)
        assert everything.keys() == ref.keys()
        for k, v in everything.items():
            assert v.shape == ref[k].shape and v.dtype == ref[k].dtype
            assert (np.isnan(v) if np.isnan(value) else v == value).all(), k
    if case.kind in ("wavenet", "lynxnet"):
        assert np.isnan(pz.all_of(case, np.nan)["t"]).all()         # the step tables get dirty too

    if pz.grid(case)[2] is not None:
        touched = 0
        for value in (np.nan, np.inf, np.float32(-3.5)):
            padded = pz.padded_with(case, value)
            assert padded.keys() == ref.keys()
            for k, v in padded.items():
                mask = past_end(case, k, v.shape)
                assert v.shape == ref[k].shape and v.dtype == ref[k].dtype
                hit = np.isnan(v) if np.isnan(value) else v == value
                assert np.array_equal(hit & mask, mask), (case.id, k, "an element past an item's end kept its value")
                assert np.array_equal(bits(v)[~mask], bits(ref[k])[~mask]), (case.id, k, "a valid element changed")
                touched += int(mask.sum())
        assert touched > 0
        for k in ("t", "rand_ini"):
            if k in ref:
                assert not past_end(case, k, ref[k].shape).any()
    else:
        with pytest.raises(AssertionError):
            pz.padded_with(case, np.nan)
    assert all(np.array_equal(bits(ref[k]), bits(keep[k])) for k in ref), "a builder wrote into clean()'s arrays"
    assert all(np.array_equal(bits(pz.clean(case)[k]), bits(keep[k])) for k in ref)


def test_valid_selects_an_items_frames():
    for case in BUILDER_CASES:
        bsz, t_len, lengths = pz.grid(case)
        if lengths is None:
            continue
        upp = pz.upp_of(case)
        shape = {"aux": (bsz, t_len, 3), "vocoder": (bsz, 1, t_len * upp)}.get(case.kind, (bsz, 2, 3, t_len))
        out = np.arange(int(np.prod(shape))).reshape(shape)
        for b, n in enumerate(lengths):
            want = out[b, :n] if case.kind == "aux" else out[b, :, :n * upp] if case.kind == "vocoder" else out[b, :, :, :n]
            assert np.array_equal(pz.valid(case, out, b, n), want) and want.size > 0


def test_part_a_of_the_gpu_test_runs_every_case_of_the_table():
    import test_gpu_poison as tp
    marks = [m for m in tp.test_part_a_case_survives_a_poisoned_workspace_and_padding.pytestmark if m.name == "parametrize"]
    assert len(marks) == 1 and marks[0].args[0] == "case"
    params = list(marks[0].args[1])
    assert [c.id for c in params] == [c.id for c in lc.CASES] and list(marks[0].kwargs["ids"]) == [c.id for c in lc.CASES]
    assert all(a is b for a, b in zip(params, lc.CASES)), "a case of the table was replaced"
    assert not any(hasattr(p, "marks") for p in params), "pytest.param with marks: no case may be skipped or xfailed"
    names = {m.name for m in tp.test_part_a_case_survives_a_poisoned_workspace_and_padding.pytestmark}
    assert not names & {"skip", "skipif", "xfail"}, names
    assert not hasattr(tp, "SKIP") and not hasattr(tp, "XFAIL")
