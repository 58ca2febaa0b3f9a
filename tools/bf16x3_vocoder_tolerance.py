#!/usr/bin/env python3
"""What the split-bf16 ("bf16x3") mode of the vocoder costs in accuracy - CPU emulation on the numpy oracle, no GPU.

Inside the residual blocks every Conv1d(C -> C) that voc_x3.hip takes (C a multiple of 32, 64 <= C <= 256) is evaluated tap by
tap with `matmul3` of tools/bf16x3_tolerance.py - operands split hi = bf16(x), lo = bf16(x - hi), product hi.hi + hi.lo + lo.hi
in fp32 - and everything else (conv_pre, the transposed convolutions, the 16- / 32-channel stages, conv_post, the source) is the
plain fp32 oracle.  Prints, for every case of tests/vocoder_x3_cases.py and every split-bf16 layout of tests/vocoder_config_cases.py, max |diff| / max |want| against the fp32 oracle, and the
same with plain bf16 operands for scale.  DESIGN.md section 4d quotes the table; tests/test_vocoder_x3_host.py asserts it."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bf16x3_tolerance import F32, bf16, matmul3  # noqa: E402
from oracle import vocoder as ov  # noqa: E402


def eligible(c_out, c_in):
    return c_out == c_in and c_in % 32 == 0 and 64 <= c_in <= 256


def emulate(layout, inp, product=matmul3, cases=None):
    """generator_forward of oracle/vocoder.py with the eligible residual-block convolutions' products replaced by `product`;
    `cases`: the module whose oracle(layout, inp) is evaluated (default tests/vocoder_x3_cases.py)"""
    if cases is None:
        import vocoder_x3_cases as cases
    plain = (ov.conv1d, ov.resblock1, ov.resblock2)
    in_block = [False]

    def conv1d(x, w, b, dilation=1, padding=0, stride=1, **kw):
        # kw: the oracle's optional `dt`, handed on as given, so that an oracle whose conv1d has no such argument still works
        if not in_block[0] or stride != 1 or not eligible(w.shape[0], w.shape[1]):
            return plain[0](x, w, b, dilation=dilation, padding=padding, stride=stride, **kw)
        assert kw.get("dt", F32) is F32        # the emulation is of the fp32 mode's arithmetic
        bsz, ci, t = x.shape
        k = w.shape[2]
        xp = np.zeros((bsz, ci, t + 2 * padding), dtype=F32)
        xp[:, :, padding:padding + t] = x
        to = t + 2 * padding - dilation * (k - 1)
        y = np.zeros((bsz, w.shape[0], to), dtype=F32)
        for j in range(k):
            y += product(np.ascontiguousarray(w[:, :, j]), xp[:, :, j * dilation:j * dilation + to])
        return (y + b[None, :, None]).astype(F32)

    def block(fn):
        def run(*a, **k):
            in_block[0] = True
            try:
                return fn(*a, **k)
            finally:
                in_block[0] = False
        return run

    ov.conv1d, ov.resblock1, ov.resblock2 = conv1d, block(plain[1]), block(plain[2])
    try:
        return cases.oracle(layout, inp)
    finally:
        ov.conv1d, ov.resblock1, ov.resblock2 = plain


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / np.abs(b).max())


def all_cases():
    """(label, layout, inputs, fp32 oracle result) of every dense case and every item of the ragged batch"""
    import vocoder_x3_cases as cases
    for layout, bsz, t_len in cases.PARITY:
        yield f"{layout} ({bsz}, {t_len})", layout, cases.inputs(layout, bsz, t_len), cases.reference(layout, bsz, t_len)
    for b, n in enumerate(cases.RAGGED_LENGTHS):
        inp = cases.item_inputs(cases.RAGGED_LAYOUT, len(cases.RAGGED_LENGTHS), cases.RAGGED_T, b, n)
        yield f"{cases.RAGGED_LAYOUT} ragged item {b} (1, {n})", cases.RAGGED_LAYOUT, inp, cases.ragged_reference(b)


def config_cases():
    """the same of the split-bf16 layouts of tests/vocoder_config_cases.py (taps 1 / 13 / 15, C = 192 / 160)"""
    import vocoder_config_cases as cc
    for tag, c in cc.X3.items():
        for bsz, t_len in c["shapes"]:
            yield f"{tag} ({bsz}, {t_len})", tag, cc.inputs(tag, bsz, t_len), cc.reference(tag, bsz, t_len, np.float32)


def main():
    print(f"{'case':28s} {'split-bf16 vs fp32':>20s} {'plain bf16 operands':>20s}")
    import vocoder_config_cases as cc
    for label, layout, inp, want, cases in [c + (None,) for c in all_cases()] + [c + (cc,) for c in config_cases()]:
        x3 = rel(emulate(layout, inp, cases=cases), want)
        b1 = rel(emulate(layout, inp, lambda a, b: np.matmul(bf16(a), bf16(b)).astype(F32), cases=cases), want)
        print(f"{label:28s} {x3:20.2e} {b1:20.2e}", flush=True)


if __name__ == "__main__":
    main()
