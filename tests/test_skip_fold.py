"""The skip projection folded into the layers' skip rows (build_packed in csrc/api.hip), as host arithmetic.

wavenet.py:96-98 computes  h = relu(W1 (sum_l (Ws_l z_l + bs_l)) / sqrt(L) + b1).  The library's fp32 path instead lets layer l
accumulate V_l z_l + c_l with  V_l = W1 Ws_l / sqrt(L),  c_l = W1 bs_l / sqrt(L)  (+ b1 on layer 0), formed in double and rounded
to fp32 once, and takes relu of the sum.  Here both are run in fp32 on the SAME gated tiles z_l (the oracle's own layer loop, z_l
kept) and measured against float64 on those tiles: the fold may be no farther from float64 than 1.5 x today's arithmetic - the
measure is the reference arithmetic itself, not a constant - and the two outputs may differ by 2e-6 of the range, the bound
tests/test_gpu_edge.py holds between the two forms of the edge."""
import math

import numpy as np
import pytest

from diffsinger_amd import synth
from oracle import backbones as ob

F32, F64 = np.float32, np.float64


def _params(in_dims, n_feats, args, seed=42):
    return synth.synth_state_dict(synth.backbone_param_shapes("wavenet", in_dims, n_feats, hidden_size=256, **args), seed=seed)


def gated_tiles(p, spec, step, cond, cycle):
    """wavenet_forward's layer loop (oracle/backbones.py) up to each layer's gate: the fp32 z_l every form below is fed"""
    bsz, n_feats, in_dims, t_len = spec.shape
    c, n_layers, _, _ = ob.wavenet_config(p)
    x = np.maximum(ob._conv1x1(ob._flatten_spec(spec), p["input_projection.weight"], p["input_projection.bias"]), F32(0))
    e = ob.sinusoidal_pos_emb(ob._broadcast_step(step, bsz), c)
    e = ob._linear(ob._mish(ob._linear(e, p["mlp.0.weight"], p["mlp.0.bias"])), p["mlp.2.weight"], p["mlp.2.bias"])
    zs = []
    for l in range(n_layers):
        pre = f"residual_layers.{l}."
        d = ob._linear(e, p[pre + "diffusion_projection.weight"], p[pre + "diffusion_projection.bias"])
        y = ob._dilated_conv3((x + d[:, :, None]).astype(F32), p[pre + "dilated_conv.weight"], p[pre + "dilated_conv.bias"],
                              2 ** (l % cycle))
        y = (y + ob._conv1x1(cond, p[pre + "conditioner_projection.weight"], p[pre + "conditioner_projection.bias"])).astype(F32)
        z = (ob._sigmoid(y[:, :c]) * np.tanh(y[:, c:])).astype(F32)
        zs.append(z)
        o = ob._conv1x1(z, p[pre + "output_projection.weight"], p[pre + "output_projection.bias"])
        x = ((x + o[:, :c]) / F32(math.sqrt(2.0))).astype(F32)
    return zs


def fold(p):
    """(V_l, c_l) as build_packed forms them: products and 1 / sqrt(L) in double, one rounding to fp32"""
    c, n_layers, _, _ = ob.wavenet_config(p)
    w1 = p["skip_projection.weight"][:, :, 0].astype(F64)
    inv = 1.0 / math.sqrt(float(n_layers))
    vs, cs = [], []
    for l in range(n_layers):
        pre = f"residual_layers.{l}.output_projection."
        v = (w1 @ p[pre + "weight"][c:, :, 0].astype(F64)) * inv
        b = (w1 @ p[pre + "bias"][c:].astype(F64)) * inv
        if l == 0:
            b = b + p["skip_projection.bias"].astype(F64)
        vs.append(v.astype(F32))
        cs.append(b.astype(F32))
    return vs, cs


def tails(p, zs):
    """(h, out) of the evaluation's end on the tiles zs: today's fp32 arithmetic, the folded fp32 arithmetic, float64"""
    c, n_layers, _, _ = ob.wavenet_config(p)
    wo, bo = p["output_projection.weight"], p["output_projection.bias"]
    # today: the oracle's own lines (backbones.py:163-178)
    skip_sum = np.zeros_like(zs[0])
    for l, z in enumerate(zs):
        pre = f"residual_layers.{l}.output_projection."
        skip_sum += ob._conv1x1(z, p[pre + "weight"], p[pre + "bias"])[:, c:]
    x = (skip_sum / F32(math.sqrt(n_layers))).astype(F32)
    h_today = np.maximum(ob._conv1x1(x, p["skip_projection.weight"], p["skip_projection.bias"]), F32(0))
    out_today = ob._conv1x1(h_today, wo, bo)
    # folded: fp32 products, fp32 accumulation over the layers; layer 0 writes the rows, the others add to them
    vs, cs = fold(p)
    acc = None
    for l, z in enumerate(zs):
        s = (np.matmul(vs[l], z) + cs[l][None, :, None]).astype(F32)
        acc = s if acc is None else (acc + s).astype(F32)
    h_fold = np.maximum(acc, F32(0))
    out_fold = ob._conv1x1(h_fold, wo, bo)
    # float64 on the same tiles
    s64 = np.zeros(zs[0].shape, F64)
    for l, z in enumerate(zs):
        pre = f"residual_layers.{l}.output_projection."
        s64 += np.matmul(p[pre + "weight"][c:, :, 0].astype(F64), z.astype(F64)) + p[pre + "bias"][c:].astype(F64)[None, :, None]
    x64 = np.matmul(p["skip_projection.weight"][:, :, 0].astype(F64), s64 / math.sqrt(float(n_layers)))
    h64 = np.maximum(x64 + p["skip_projection.bias"].astype(F64)[None, :, None], 0.0)
    out64 = np.matmul(wo[:, :, 0].astype(F64), h64) + bo.astype(F64)[None, :, None]
    return (h_today, out_today), (h_fold, out_fold), (h64, out64)


def _err(a, ref):
    return float(np.abs(a.astype(F64) - ref).max() / np.abs(ref).max())


CASES = {
    "acoustic_20x256_T96": (128, 1, dict(num_layers=20, num_channels=256, dilation_cycle_length=4), 96),
    "variance_10x192_T40": (24, 2, dict(num_layers=10, num_channels=192, dilation_cycle_length=4), 40),
    "c250_T40": (128, 1, dict(num_layers=4, num_channels=250, dilation_cycle_length=4), 40),           # channels the kernels pad
    "three_layers_T40": (128, 1, dict(num_layers=3, num_channels=256, dilation_cycle_length=4), 40),   # fewer than one cycle
}


@pytest.fixture(scope="module", params=sorted(CASES))
def case(request):
    in_dims, n_feats, args, t_len = CASES[request.param]
    p = _params(in_dims, n_feats, args)
    spec = synth.synth_normal((1, n_feats, in_dims, t_len), 11)
    cond = synth.synth_normal((1, 256, t_len), 12)
    zs = gated_tiles(p, spec, np.asarray([417.25], F32), cond, args["dilation_cycle_length"])
    return request.param, p, tails(p, zs)


def test_fold_no_farther_from_float64_than_todays_arithmetic(case):
    name, _, ((h_t, o_t), (h_f, o_f), (h64, o64)) = case
    eh_t, eh_f, eo_t, eo_f = _err(h_t, h64), _err(h_f, h64), _err(o_t, o64), _err(o_f, o64)
    print(f"{name}: h today {eh_t:.2e} folded {eh_f:.2e}; output today {eo_t:.2e} folded {eo_f:.2e}")
    assert eh_f <= 1.5 * eh_t, (name, eh_f, eh_t)
    assert eo_f <= 1.5 * eo_t, (name, eo_f, eo_t)


def test_fold_against_todays_output(case):
    name, _, ((_, o_t), (_, o_f), _) = case
    d = float(np.abs(o_f.astype(F64) - o_t.astype(F64)).max() / np.abs(o_t).max())
    print(f"{name}: folded vs today's output {d:.2e}")
    assert d <= 2e-6, (name, d)


def test_bias_fold_adds_b1_once(case):
    _, p, _ = case
    c, n_layers, _, _ = ob.wavenet_config(p)
    _, cs = fold(p)
    w1 = p["skip_projection.weight"][:, :, 0].astype(F64)
    b1 = p["skip_projection.bias"].astype(F64)
    inv = 1.0 / math.sqrt(float(n_layers))
    for l in range(n_layers):
        want = (w1 @ p[f"residual_layers.{l}.output_projection.bias"][c:].astype(F64)) * inv + (b1 if l == 0 else 0.0)
        assert np.array_equal(cs[l], want.astype(F32)), l
    # all-zero tiles: what the layers leave in the skip rows is W1 (sum_l bs_l) / sqrt(L) + b1, with b1 in it exactly once
    bs = sum(p[f"residual_layers.{l}.output_projection.bias"][c:].astype(F64) for l in range(n_layers))
    total = np.sum(np.stack(cs).astype(F64), axis=0)
    want = w1 @ bs * inv + b1
    assert np.abs(total - want).max() <= 4 * n_layers * np.finfo(F32).eps * np.abs(want).max()
    assert np.abs(total - (want + b1)).max() > 1e-3 * np.abs(b1).max()


def test_padding_after_forming_equals_forming_from_padded():
    """C = 250 runs as 256 channels whose extra rows and columns are zero (pad_weights): zero-extending V_l formed at the caller's
    width gives, bit for bit, what forming it from the zero-extended matrices gives - extra terms of the sums are exact zeros"""
    in_dims, n_feats, args, _ = CASES["c250_T40"]
    p = _params(in_dims, n_feats, args)
    c, cp = 250, 256
    vs, cs = fold(p)
    q = dict(p)
    w1 = np.zeros((cp, cp, 1), F32)
    w1[:c, :c] = p["skip_projection.weight"]
    b1 = np.zeros(cp, F32)
    b1[:c] = p["skip_projection.bias"]
    q["skip_projection.weight"], q["skip_projection.bias"] = w1, b1
    q["input_projection.weight"] = np.zeros((cp, in_dims * n_feats, 1), F32)       # (wavenet_config reads C from it)
    for l in range(args["num_layers"]):
        pre = f"residual_layers.{l}.output_projection."
        w = np.zeros((2 * cp, cp, 1), F32)
        w[:c, :c], w[cp:cp + c, :c] = p[pre + "weight"][:c], p[pre + "weight"][c:]       # halves extended on their own
        b = np.zeros(2 * cp, F32)
        b[:c], b[cp:cp + c] = p[pre + "bias"][:c], p[pre + "bias"][c:]
        q[pre + "weight"], q[pre + "bias"] = w, b
    vq, cq = fold(q)
    for l in range(args["num_layers"]):
        want_v = np.zeros((cp, cp), F32)
        want_v[:c, :c] = vs[l]
        want_c = np.zeros(cp, F32)
        want_c[:c] = cs[l]
        assert np.array_equal(vq[l], want_v) and np.array_equal(cq[l], want_c), l
