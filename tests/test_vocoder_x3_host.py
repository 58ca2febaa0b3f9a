"""The arithmetic of the vocoder's split-bf16 mode on the CPU (tools/bf16x3_vocoder_tolerance.py: the numpy oracle with the
products of the eligible residual-block convolutions evaluated as hi.hi + hi.lo + lo.hi over bf16 halves): for every layout and
size that tests/test_gpu_vocoder_x3.py runs, the emulated result stays within 3e-5 = 0.6 TOL of the fp32 oracle, which leaves
the GPU tests' fp32 tolerance (TOL = 5e-5) room for the fp32 path's own 5.7e-6 and the accumulation order.  This is the
condition that keeps the GPU bar honest; no GPU is needed."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import bf16x3_vocoder_tolerance as emu  # noqa: E402
import vocoder_x3_cases as cases  # noqa: E402

CAP = 3e-5
LABELS = [f"{la}-{b}-{t}" for la, b, t in cases.PARITY] + [f"ragged-item{b}-{n}" for b, n in enumerate(cases.RAGGED_LENGTHS)]


def test_cases_cover_the_kernel_paths():
    """what the sizes are chosen for: every MBW of voc_x3.hip the layouts reach, a reach that forces 32-frame tiles at C = 256,
    an all-halo utterance and one with several tiles and a cut last tile at both widths"""
    chans = {cases.config(la)["upsample_initial_channel"] >> (i + 1) for la, _, _ in cases.PARITY for i in range(3)}
    assert {256, 128, 64, 96} <= chans and {48, 24} <= chans
    hb = cases.config("B")
    assert max((k // 2) * d for k, ds in zip(hb["resblock_kernel_sizes"], hb["resblock_dilation_sizes"]) for d in ds) == 48
    assert ("A", 1, 1) in cases.PARITY and ("A", 3, 130) in cases.PARITY and (130 * 4) % 64 != 0 and (130 * 4) % 32 != 0
    assert all(emu.eligible(c, c) == (c in (256, 128, 64, 96)) for c in (256, 128, 96, 64, 48, 32, 24, 16, 512))


@pytest.mark.parametrize("idx", range(len(LABELS)), ids=LABELS)
def test_emulated_split_bf16_within_cap(idx):
    label, layout, inp, want = list(emu.all_cases())[idx]
    got = emu.emulate(layout, inp)
    err = emu.rel(got, want)
    print(f"{label}: split-bf16 emulation vs fp32 oracle {err:.3e} (cap {CAP:.0e})")
    assert got.shape == want.shape
    assert 0.0 < err < CAP       # > 0: the emulation really replaced products


def test_emulation_restores_the_oracle():
    from oracle import vocoder as ov
    before = (ov.conv1d, ov.resblock1, ov.resblock2)
    emu.emulate("A", cases.inputs("A", 1, 1))
    assert (ov.conv1d, ov.resblock1, ov.resblock2) == before
