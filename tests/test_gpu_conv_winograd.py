"""The row-split conv on Winograd F(2,3) operands (wn_rowsplit.hip, wn_conv_wq_kernel; DSD_RS_CONV_Q=2 forces it on every layer
of dilation <= 8): one evaluation against the numpy oracle at shapes chosen for where the pairing (frame t with t + d) and the
padding can go wrong, against the direct K-quarter kernel (DSD_RS_CONV_Q=1), and on the grid where the library picks it itself.
The kernel classes of a timing pass (dsd_kernel_timing_classes) say which conv ran.

Grids below ~16 tiles never reach the row-split pair by the library's own rule (they run 16-frame GEMM tiles), so the small
cases go through the mixed-plan test hook (DSD_WN_PLAN=2 + DSD_RS_ROWS=64: the first half of the tiles, rounded down, on the
fused layer kernel, the rest on the row-split pair): T = 32 and T = 7 put their only tile on the kernel under test, T = 37 its
cut second tile, T = 70 the middle and the cut last tile, B = 2 the second item, the ragged batch the items of 33 and 5 frames."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from diffsinger_amd import synth  # noqa: E402
from gpu_util import check, dev, make_backbone, set_hp  # noqa: E402
from oracle import backbones as ob  # noqa: E402

TOL_NFE = 2e-5
# Winograd against the direct K-quarter kernel: twice what tests/test_gpu_rowsplit.py allows two summation orders of the same
# products (2e-6), each transformed operand adding one rounding
TOL_VS_DIRECT = 4e-6
SWITCHES = ("DSD_RS_CONV_Q", "DSD_WN_PLAN", "DSD_RS_ROWS", "DSD_FUSED_LAYER", "DSD_ROWSPLIT")
HOOK = {"DSD_WN_PLAN": "2", "DSD_RS_ROWS": "64"}
ACOUSTIC = dict(num_layers=4, num_channels=256, dilation_cycle_length=4)        # d = 1, 2, 4, 8 once each
PITCH = dict(num_layers=5, num_channels=256, dilation_cycle_length=5)           # ... and d = 16


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


def _run(env, in_dims, args, bsz, t_len, lengths=None):
    """-> (out, kernel class names of one more pass, params, x, t, cond)"""
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        net, params = make_backbone("wavenet", in_dims, 1, args, 42)
        x = synth.synth_normal((bsz, 1, in_dims, t_len), 21)
        cond = synth.synth_normal((bsz, 256, t_len), 22)
        t = (np.arange(bsz) * 211.5 + 3.25).astype(np.float32)
        xd = dev(x)
        if lengths is not None:
            net.set_lengths(lengths, xd.device)
        with torch.no_grad():
            out = net(xd, dev(t), dev(cond))
            again = net(xd, dev(t), dev(cond))
            torch.cuda.synchronize()
            assert torch.equal(out, again)
            net.kernel_timing(True)
            net(xd, dev(t), dev(cond))
            torch.cuda.synchronize()
            names = [k["name"] for k in net.kernel_classes()]
            net.kernel_timing(False)
        net.release_native()
        return out.cpu().numpy(), names, params, x, t, cond
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)


def _vs_oracle(out, params, x, t, cond, cyc, lengths, what):
    if lengths is None:
        check(out, ob.wavenet_forward(params, x, t, cond, dilation_cycle_length=cyc), TOL_NFE, what=what)
        return
    for b, n in enumerate(lengths):               # frames past an item's end are the caller's to mask
        want_b = ob.wavenet_forward(params, x[b:b + 1, :, :, :n], t[b:b + 1], cond[b:b + 1, :, :n], dilation_cycle_length=cyc)
        check(out[b:b + 1, :, :, :n], want_b, TOL_NFE, what=(what, b))


def _wq(names):
    return [n for n in names if n.startswith("wn_conv_wq_kernel")]


CASES = {
    "T32": (128, ACOUSTIC, 1, 32, None),                        # exactly one full tile; the halo is all padding
    "T37": (128, ACOUSTIC, 1, 37, None),                        # second tile cut at 5 frames (< d = 8); a partner past the end
    "T70": (128, ACOUSTIC, 1, 70, None),                        # three tiles; real halos on both sides of the middle one; last cut at 6
    "T7": (128, ACOUSTIC, 1, 7, None),                          # shorter than the largest dilation
    "B2_T70": (128, ACOUSTIC, 2, 70, None),                     # batch stride
    "ragged_B3_T70": (128, ACOUSTIC, 3, 70, [70, 33, 5]),       # tile list and per-item ends inside a tile
    "pitch_T70": (64, PITCH, 1, 70, None),                      # the d = 16 layer stays on the direct kernel
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_winograd_forced_vs_oracle(name):
    in_dims, args, bsz, t_len, lengths = CASES[name]
    out, names, params, x, t, cond = _run(dict(HOOK, DSD_RS_CONV_Q="2"), in_dims, args, bsz, t_len, lengths)
    assert _wq(names), names
    direct = [n for n in names if n.startswith(("wn_conv_rq_kernel", "wn_conv_rs_kernel"))]
    if args is PITCH:
        assert direct and all("80, 16" in n or n.startswith("wn_conv_rs_kernel<80") for n in direct), names
    else:
        assert not direct, names
    _vs_oracle(out, params, x, t, cond, args["dilation_cycle_length"], lengths, ("Winograd conv", name))


def test_direct_switch_keeps_winograd_out():
    in_dims, args, bsz, t_len, lengths = CASES["T70"]
    out, names, params, x, t, cond = _run(dict(HOOK, DSD_RS_CONV_Q="1"), in_dims, args, bsz, t_len, lengths)
    assert not _wq(names) and any(n.startswith("wn_conv_rq_kernel") for n in names), names
    _vs_oracle(out, params, x, t, cond, 4, None, "direct K quarters, T = 70")
    wino = _run(dict(HOOK, DSD_RS_CONV_Q="2"), in_dims, args, bsz, t_len, lengths)[0]
    check(wino, out, TOL_VS_DIRECT, what="Winograd vs direct K quarters, T = 70")


def test_natural_plan_T1000():
    """One utterance of 1000 frames (8 layers): 256 workgroups - the library's own choice is the Winograd conv on every layer; and
    it agrees with the direct K-quarter kernel and the oracle."""
    args = dict(num_layers=8, num_channels=256, dilation_cycle_length=4)
    out, names, params, x, t, cond = _run({}, 128, args, 1, 1000)
    assert _wq(names) and not any(n.startswith(("wn_conv_rq_kernel", "wn_conv_rs_kernel")) for n in names), names
    _vs_oracle(out, params, x, t, cond, 4, None, "natural plan, T = 1000")
    forced, fnames = _run({"DSD_RS_CONV_Q": "2"}, 128, args, 1, 1000)[:2]
    assert _wq(fnames), fnames
    assert np.array_equal(forced, out)
    direct, dnames = _run({"DSD_RS_CONV_Q": "1"}, 128, args, 1, 1000)[:2]
    assert not _wq(dnames) and any(n.startswith("wn_conv_rq_kernel<2") for n in dnames), dnames
    check(out, direct, TOL_VS_DIRECT, what="Winograd vs direct K quarters, T = 1000")
