"""wn_conv_wq_kernel forms its Winograd operands G1, G2 from the three tap blocks of the direct packed matrix: cases that tell
the taps apart.  Same hook as tests/test_gpu_conv_winograd.py (DSD_WN_PLAN=2 + DSD_RS_ROWS=64 puts the later tiles of a short
utterance on the row-split pair, DSD_RS_CONV_Q=2 forces the Winograd conv), one evaluation at T = 70 against the numpy oracle:
  * one tap scaled by 8 (g1, then g0, then g2): a swapped or mis-signed tap is then far above the tolerance;
  * a 250-channel network, which the loader pads to 256;
  * bf16x3 and back to f32 on one handle: re-finalisation keeps the operand, bit-equal to a fresh f32 handle;
  * every result twice, bit-equal."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from diffsinger_amd import synth  # noqa: E402
from diffsinger_amd.backbones import build_backbone  # noqa: E402
from gpu_util import check, dev, load_synth, set_hp, synth_params  # noqa: E402
from oracle import backbones as ob  # noqa: E402

TOL_NFE = 2e-5
SWITCHES = ("DSD_RS_CONV_Q", "DSD_WN_PLAN", "DSD_RS_ROWS", "DSD_FUSED_LAYER", "DSD_ROWSPLIT")
FORCED = {"DSD_WN_PLAN": "2", "DSD_RS_ROWS": "64", "DSD_RS_CONV_Q": "2"}
IN_DIMS, T_LEN = 128, 70


@pytest.fixture(autouse=True)
def _env():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    set_hp()
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(FORCED)
    yield
    for k in SWITCHES:
        os.environ.pop(k, None)
        if saved[k] is not None:
            os.environ[k] = saved[k]


@pytest.fixture(scope="module")
def inputs():
    return (synth.synth_normal((1, 1, IN_DIMS, T_LEN), 21), np.asarray([3.25], np.float32), synth.synth_normal((1, 256, T_LEN), 22))


def _params(channels, scale_tap=None):
    args = dict(num_layers=4, num_channels=channels, dilation_cycle_length=4)        # d = 1, 2, 4, 8 once each
    params = synth_params("wavenet", IN_DIMS, 1, args, 42)
    if scale_tap is not None:
        for l in range(4):
            params[f"residual_layers.{l}.dilated_conv.weight"][:, :, scale_tap] *= np.float32(8.0)
    return args, params


def _eval(net, inputs, classes=True):
    """-> (out, kernel class names of a timing pass); the result is run twice and must repeat bit for bit"""
    x, t, cond = inputs
    with torch.no_grad():
        out = net(dev(x), dev(t), dev(cond))
        again = net(dev(x), dev(t), dev(cond))
        torch.cuda.synchronize()
        assert torch.equal(out, again)
        names = []
        if classes:
            net.kernel_timing(True)
            net(dev(x), dev(t), dev(cond))
            torch.cuda.synchronize()
            names = [k["name"] for k in net.kernel_classes()]
            net.kernel_timing(False)
    return out.cpu().numpy(), names


def _only_winograd(names):
    assert [n for n in names if n.startswith("wn_conv_wq_kernel")], names
    assert not [n for n in names if n.startswith(("wn_conv_rq_kernel", "wn_conv_rs_kernel"))], names


@pytest.mark.parametrize("tap", [1, 0, 2])
def test_one_tap_dominates(tap, inputs):
    args, params = _params(256, scale_tap=tap)
    net = load_synth(build_backbone(IN_DIMS, 1, "wavenet", args), params)
    out, names = _eval(net, inputs)
    net.release_native()
    _only_winograd(names)
    x, t, cond = inputs
    check(out, ob.wavenet_forward(params, x, t, cond, dilation_cycle_length=4), TOL_NFE, what=("tap x 8", tap))


def test_250_channels_padded_to_256(inputs):
    args, params = _params(250)
    net = load_synth(build_backbone(IN_DIMS, 1, "wavenet", args), params)
    out, names = _eval(net, inputs)
    net.release_native()
    _only_winograd(names)
    x, t, cond = inputs
    check(out, ob.wavenet_forward(params, x, t, cond, dilation_cycle_length=4), TOL_NFE, what="C = 250")


def test_precision_round_trip_keeps_the_operand(inputs):
    args, params = _params(256)
    fresh = load_synth(build_backbone(IN_DIMS, 1, "wavenet", args), params)
    want, names = _eval(fresh, inputs)
    fresh.release_native()
    _only_winograd(names)
    net = load_synth(build_backbone(IN_DIMS, 1, "wavenet", args), params)
    net.set_precision("bf16x3")
    _eval(net, inputs, classes=False)              # one evaluation on the re-finalised bf16x3 weights
    net.set_precision("f32")
    got, names = _eval(net, inputs)
    net.release_native()
    _only_winograd(names)
    assert np.array_equal(got, want)
    x, t, cond = inputs
    check(got, ob.wavenet_forward(params, x, t, cond, dilation_cycle_length=4), TOL_NFE, what="f32 after bf16x3")
