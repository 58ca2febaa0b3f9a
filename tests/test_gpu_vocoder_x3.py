"""-m gpu: the vocoder's opt-in split-bf16 precision mode (voc_x3.hip, dsd_set_precision on a vocoder handle) - the residual-block
convolutions of the stages with 64 .. 256 channels with every operand split into two bf16 values, three bf16 MFMAs per fp32 one,
fp32 accumulation; everything else fp32.  Stated tolerance = the fp32 vocoder's own, TOL = 5e-5 of the waveform range against
the numpy oracle (tests/test_gpu_vocoder.py); tests/test_vocoder_x3_host.py shows on the CPU that the arithmetic alone stays
below 0.6 TOL for every case here.  Every test fails without the mode: set_precision("bf16x3") raises on a vocoder there."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vocoder_x3_cases as cases  # noqa: E402
from diffsinger_amd import _lib  # noqa: E402
from gpu_util import dev, rel_err  # noqa: E402

TOL = 5e-5
X3 = "voc_conv_x3_kernel<"
SWITCHES = ("DSD_PRECISION", "DSD_X3_WIDE")


@pytest.fixture(autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    yield
    for k in SWITCHES:
        os.environ.pop(k, None)
        if saved[k] is not None:
            os.environ[k] = saved[k]


def build(layout):
    from diffsinger_amd.vocoder import Generator
    g = Generator(cases.config(layout))
    g.load_state_dict({k: torch.from_numpy(v) for k, v in cases.weights(layout).items()}, strict=True)
    return g.cuda().eval()


def run(gen, i, lengths=None):
    with torch.no_grad():
        out = gen(dev(i["mel"]), dev(i["f0"]), lengths=lengths, rand_ini=dev(i["rand_ini"]), noise=dev(i["noise"]),
                  pre_noise=dev(i["pre_noise"]))
    torch.cuda.synchronize()
    return out


def x3_classes(gen):
    return sorted(c["name"] for c in gen.kernel_classes() if c["name"].startswith(X3))


@pytest.mark.parametrize("layout,bsz,t_len", [c for c in cases.PARITY if c[0] != "F"])
def test_x3_vs_oracle(layout, bsz, t_len):
    gen = build(layout)
    gen.set_precision("bf16x3")
    gen.kernel_timing(True)
    got = run(gen, cases.inputs(layout, bsz, t_len))
    names = x3_classes(gen)
    upp = int(np.prod(cases.config(layout)["upsample_rates"]))
    assert tuple(got.shape) == (bsz, 1, t_len * upp)
    # all three eligible widths ran: 256 -> 4 row blocks per wave, 128 -> 2, 64 -> 1; dense launches
    assert {n.split("<")[1].split(",")[0] for n in names} == {"4", "2", "1"} and all(n.endswith(" 0>") for n in names), names
    assert gen.stats()["precision"] == 1
    err = rel_err(got, cases.reference(layout, bsz, t_len))
    print(f"{layout} ({bsz}, {t_len}): bf16x3 vs oracle {err:.3e}; {names}")
    assert err < TOL
    gen.release_native()


def test_x3_ragged_items_equal_lone_items():
    layout, t_len, lens = cases.RAGGED_LAYOUT, cases.RAGGED_T, cases.RAGGED_LENGTHS
    gen = build(layout)
    gen.set_precision("bf16x3")
    upp = int(np.prod(cases.config(layout)["upsample_rates"]))
    i = cases.inputs(layout, len(lens), t_len)
    batch = dict(i, rand_ini=np.repeat(i["rand_ini"][None], len(lens), 0))     # the ragged call takes one row of phases per item
    gen.kernel_timing(True)
    got = run(gen, batch, lengths=lens)
    names = x3_classes(gen)
    assert names and all(n.endswith(" 1>") for n in names), names      # the ragged instantiations
    assert gen.stats()["precision"] == 1
    gen.kernel_timing(False)
    for b, n in enumerate(lens):
        alone = run(gen, cases.item_inputs(layout, len(lens), t_len, b, n))
        assert torch.equal(got[b:b + 1, :, :n * upp], alone), (b, n)
        err = rel_err(alone, cases.ragged_reference(b))
        print(f"ragged item {b} (T = {n}): bf16x3 vs oracle {err:.3e}")
        assert err < TOL
    gen.release_native()


@pytest.mark.parametrize("layout,bsz,t_len,lengths", [("A", 3, 130, None), ("B", 2, 70, None), ("A", 4, 130, cases.RAGGED_LENGTHS)])
def test_x3_tile_width_does_not_change_a_bit(layout, bsz, t_len, lengths):
    """The library takes 64-frame tiles once they give every CU a workgroup (thousands of frames per stage) and 32-frame tiles
    below that; DSD_X3_WIDE forces either at these sizes.  The K walk is the weight stream's, so both give the same bits - and
    a cut last tile, a lone-frame item and the 32-frame-only reach-48 convolution at C = 256 are covered at both widths."""
    gen = build(layout)
    gen.set_precision("bf16x3")
    inp = cases.inputs(layout, bsz, t_len)
    if lengths:
        inp = dict(inp, rand_ini=np.repeat(inp["rand_ini"][None], bsz, 0))
    outs = {}
    for wide in ("0", "1"):
        os.environ["DSD_X3_WIDE"] = wide
        gen.kernel_timing(True)
        outs[wide] = run(gen, inp, lengths=lengths)
        names = x3_classes(gen)
        widths = {(n.split("<")[1].split(",")[0], n.split(", ")[1]) for n in names}
        if wide == "0":
            assert {w for _, w in widths} == {"2"}, names
        else:       # everything on 64-frame tiles but the convolutions whose images do not fit: C = 256 beyond a reach of 28
            assert {("1", "4"), ("2", "4"), ("4", "4")} <= widths, names
            assert (("4", "2") in widths) == (layout == "B"), names
    if lengths:
        upp = int(np.prod(cases.config(layout)["upsample_rates"]))
        for b, n in enumerate(lengths):
            assert torch.equal(outs["0"][b, :, :n * upp], outs["1"][b, :, :n * upp]), b
    else:
        assert torch.equal(outs["0"], outs["1"])
        assert rel_err(outs["1"], cases.reference(layout, bsz, t_len)) < TOL
    gen.release_native()


def test_x3_fallback_is_visible():
    # 96 / 48 / 24 channels: the 96-channel stage is eligible (2 row blocks per wave, the rows above 96 zero), the others are not
    gen = build("F")
    inp = cases.inputs("F", 1, 33)
    f32 = run(gen, inp)
    gen.set_precision("bf16x3")
    gen.kernel_timing(True)
    got = run(gen, inp)
    names = x3_classes(gen)
    assert names and all(n.startswith(X3 + "2,") for n in names), names
    assert gen.stats()["precision"] == 1
    assert not torch.equal(got, f32)
    err = rel_err(got, cases.reference("F", 1, 33))
    print(f"F (1, 33): bf16x3 vs oracle {err:.3e}; {names}")
    assert err < TOL
    gen.release_native()
    # 32 / 16 / 8 channels: nothing is eligible - the mode is accepted, no split-bf16 kernel runs, and the stats say so
    small = build("small")
    inp = cases.inputs("small", 1, 9)
    a = run(small, inp)
    small.set_precision("bf16x3")
    small.kernel_timing(True)
    b = run(small, inp)
    assert torch.equal(a, b) and x3_classes(small) == [] and small.stats()["precision"] == 0
    assert rel_err(b, cases.reference("small", 1, 9)) < TOL
    small.release_native()


def test_x3_round_trip_to_f32():
    gen = build("A")
    inp = cases.inputs("A", 1, 33)
    before = run(gen, inp)
    assert gen.stats()["precision"] == 0
    gen.set_precision("bf16x3")
    x3 = run(gen, inp)
    assert gen.stats()["precision"] == 1
    gen.set_precision("f32")
    gen.kernel_timing(True)
    after = run(gen, inp)
    assert x3_classes(gen) == [] and gen.stats()["precision"] == 0
    assert torch.equal(before, after)
    assert not torch.equal(x3, before)          # the mode really was on
    want = cases.reference("A", 1, 33)
    assert rel_err(x3, want) < TOL and rel_err(before, want) < TOL
    gen.release_native()


@pytest.mark.parametrize("layout,bsz,t_len", [("A", 3, 130), ("B", 2, 70)])
def test_x3_repeatable(layout, bsz, t_len):
    gen = build(layout)
    gen.set_precision("bf16x3")
    inp = cases.inputs(layout, bsz, t_len)
    first = run(gen, inp)
    for _ in range(3):
        assert torch.equal(run(gen, inp), first)
    assert rel_err(first, cases.reference(layout, bsz, t_len)) < TOL
    gen.release_native()


def test_x3_errors_and_environment():
    gen = build("A")
    inp = cases.inputs("A", 1, 1)
    f32 = run(gen, inp)
    lib = _lib.lib()
    assert lib.dsd_set_precision(gen._handle, 7) == -1                  # DSD_EINVAL: unknown mode
    assert b"unknown mode" in lib.dsd_last_error(gen._handle)
    with pytest.raises(ValueError):
        gen.set_precision("bf16")
    assert gen.stats()["precision"] == 0 and torch.equal(run(gen, inp), f32)
    gen.release_native()
    os.environ["DSD_PRECISION"] = "1"           # the environment switch is the denoisers': a vocoder takes the explicit call only
    env = build("A")
    env.native_handle(torch.device("cuda", torch.cuda.current_device()))
    env.kernel_timing(True)
    got = run(env, inp)
    assert env.stats()["precision"] == 0 and x3_classes(env) == []
    assert torch.equal(got, f32)
    env.release_native()
