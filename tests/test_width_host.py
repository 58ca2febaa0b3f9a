"""LYNXNet and the ConvNeXt aux decoder at widths that are not multiples of 32, without a GPU.

G20 (tests/golden/g20_width.npz, generator make_golden_width.py) holds the reference's outputs at num_channels 500 / 1000 / 90 / 6
(LYNXNet), one RectifiedFlow run at 500 and AuxDecoderAdaptor at 500 / 75.  The numpy oracle is checked against it at the levels
tests/test_oracle_golden.py uses for G3 / G5 / G7, which pins the oracle at these widths: the larger GPU cases of
tests/test_gpu_width.py use it as their reference.

The boundary: dsd_create_any_width validates before it selects a device, so its width rules are checked here too; dsd_create keeps
its own (tests/test_cabi_exports.py::test_bad_config_rejected)."""
import ctypes as C
import os

import numpy as np
import pytest

import width_cases as wc
from diffsinger_amd import synth
from oracle import aux_decoder as oa
from oracle import backbones as ob
from oracle import diffusion as od

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load():
    return np.load(os.path.join(GOLDEN, "g20_width.npz"))


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def lynx_params(in_dims, n_feats, args, seed):
    shapes = synth.backbone_param_shapes("lynxnet", in_dims, n_feats, hidden_size=256, **args)
    return synth.synth_state_dict(shapes, seed=seed)


@pytest.mark.parametrize("tag", sorted(wc.LYNX_EVALS))
def test_g20_oracle_lynxnet_single_nfe(tag):
    in_dims, n_feats, args, wseed, cases = wc.LYNX_EVALS[tag]
    g = load()
    params = lynx_params(in_dims, n_feats, args, wseed)
    assert synth.state_dict_digest(params) == str(g[f"{tag}_digest"])
    for ci, (bsz, t_len, _) in enumerate(cases):
        xs, cs, _ = wc.eval_seeds(ci)
        x = synth.synth_normal((bsz, n_feats, in_dims, t_len), xs)
        cond = synth.synth_normal((bsz, 256, t_len), cs)
        out = ob.lynxnet_forward(params, x, g[f"{tag}_c{ci}_t"], cond, activation=args["activation"], strong_cond=args["strong_cond"])
        err = rel_err(out, g[f"{tag}_c{ci}_out"])
        print(f"G20 {tag} case {ci}: oracle vs reference {err:.3g}")
        assert err < 2e-5, (tag, ci, err)


def test_g20_oracle_lynxnet_sampler():
    s = wc.SAMPLER
    g = load()
    params = lynx_params(s["in_dims"], s["n_feats"], s["args"], s["wseed"])
    assert synth.state_dict_digest(params) == str(g["rf_digest"])
    fn = lambda x, t, c: ob.lynxnet_forward(params, x, t, c, activation=s["args"]["activation"], strong_cond=s["args"]["strong_cond"])   # noqa: E731
    cond = synth.synth_normal((s["bsz"], s["t_len"], 256), s["cond_seed"])
    r = od.RectifiedFlow(fn, s["in_dims"], s["n_feats"], spec_min=[-12.0], spec_max=[0.0])
    out = r.forward(cond, synth.synth_normal((s["bsz"], s["n_feats"], s["in_dims"], s["t_len"]), s["noise_seed"]),
                    sampling_algorithm="euler", sampling_steps=s["steps"])
    err = rel_err(out, g["rf_euler10_out"])
    print(f"G20 reflow euler: oracle vs reference {err:.3g}")
    assert err < 5e-5, err


@pytest.mark.parametrize("tag", sorted(wc.AUX))
def test_g20_oracle_aux_decoder(tag):
    hsz, m, args, bsz, t_len, wseed = wc.AUX[tag]
    g = load()
    shapes = synth.convnext_param_shapes(hsz, m, num_channels=args["num_channels"], num_layers=args["num_layers"],
                                         kernel_size=args["kernel_size"], prefix="decoder.")
    params = synth.synth_state_dict(shapes, seed=wseed)
    assert synth.state_dict_digest(params) == str(g[f"{tag}_digest"])
    cond = synth.synth_normal((bsz, t_len, hsz), wseed + 100)
    raw = oa.aux_adaptor_forward(params, cond, m, 1, g[f"{tag}_smin"], g[f"{tag}_smax"], infer=False)
    mel = oa.aux_adaptor_forward(params, cond, m, 1, g[f"{tag}_smin"], g[f"{tag}_smax"], infer=True)
    e_raw, e_mel = rel_err(raw, g[f"{tag}_raw"]), rel_err(mel, g[f"{tag}_mel"])
    print(f"G20 aux {tag}: oracle vs reference raw {e_raw:.3g} mel {e_mel:.3g}")
    assert e_raw < 2e-5 and e_mel < 2e-5, (tag, e_raw, e_mel)


# --------------------------------------------------------------------------- the boundary
def _lynx_cfg(_lib, channels, expansion=2, kernel=31):
    return _lib.DsdConfig(C.sizeof(_lib.DsdConfig), 1, 128, 1, 6, channels, 256, 0, expansion, kernel, 0, 0, 0)


def _aux_cfg(_lib, channels):
    return _lib.DsdConfig(C.sizeof(_lib.DsdConfig), 2, 128, 1, 3, channels, 256, 0, 0, 7, 0, 0, 0)


@pytest.mark.parametrize("channels", (501, 2))
def test_any_width_rejects_what_the_reference_cannot_build(channels):
    from diffsinger_amd import _lib
    h = C.c_void_p()
    assert _lib.lib().dsd_create_any_width(C.byref(_lynx_cfg(_lib, channels)), C.byref(h)) == -1
    msg = _lib.lib().dsd_last_error(None)
    assert b"even and >= 4" in msg and b"reference cannot build" in msg and b"SinusoidalPosEmb" in msg, msg


def test_any_width_keeps_the_other_rules():
    from diffsinger_amd import _lib
    h = C.c_void_p()
    lib = _lib.lib()
    assert lib.dsd_create_any_width(C.byref(_lynx_cfg(_lib, 500, kernel=30)), C.byref(h)) == -1      # even kernel: T + 1 frames
    assert b"odd kernel_size" in lib.dsd_last_error(None)
    assert lib.dsd_create_any_width(C.byref(_lynx_cfg(_lib, 500, expansion=0)), C.byref(h)) == -1
    assert lib.dsd_create_any_width(C.byref(_aux_cfg(_lib, 0)), C.byref(h)) == -1
    assert b"positive" in lib.dsd_last_error(None)
    cfg = _lib.DsdConfig(C.sizeof(_lib.DsdConfig), 0, 128, 1, 20, 251, 256, 4, 0, 0, 0, 0, 0)           # WaveNet: as dsd_create
    assert lib.dsd_create_any_width(C.byref(cfg), C.byref(h)) == -1
    assert b"must be even" in lib.dsd_last_error(None)


@pytest.mark.parametrize("which", ("lynx250", "lynx90x3", "aux75", "aux1"))
def test_any_width_gets_past_validation(which):
    """Without a GPU "past validation" is the no-device failure of test_create_fails_loudly_without_gpu; with one, a handle."""
    import torch
    from diffsinger_amd import _lib
    lib = _lib.lib()
    cfg = {"lynx250": lambda: _lynx_cfg(_lib, 250), "lynx90x3": lambda: _lynx_cfg(_lib, 90, expansion=3, kernel=7),
           "aux75": lambda: _aux_cfg(_lib, 75), "aux1": lambda: _aux_cfg(_lib, 1)}[which]()
    h = C.c_void_p()
    rc = lib.dsd_create_any_width(C.byref(cfg), C.byref(h))
    if torch.cuda.is_available():
        assert rc == 0, lib.dsd_last_error(None)
        lib.dsd_destroy(h)
    else:
        assert rc < 0
        assert b"no HIP device" in lib.dsd_last_error(None) and b"dsd_create_any_width" in lib.dsd_last_error(None)


def test_create_keeps_its_contract():
    from diffsinger_amd import _lib
    lib = _lib.lib()
    h = C.c_void_p()
    assert lib.dsd_create(C.byref(_lynx_cfg(_lib, 250)), C.byref(h)) == -1
    assert b"dsd_create: num_channels must be a positive multiple of 32 (got 250)" in lib.dsd_last_error(None)
    assert lib.dsd_create(C.byref(_aux_cfg(_lib, 75)), C.byref(h)) == -1
    assert b"multiple of 32" in lib.dsd_last_error(None)
    assert lib.dsd_create(C.byref(_lynx_cfg(_lib, 48, expansion=1)), C.byref(h)) == -1
    assert b"multiple of 32" in lib.dsd_last_error(None)
    assert lib.dsd_api_version() == 10 and C.sizeof(_lib.DsdConfig) == 13 * 4


def test_shims_reject_through_the_library():
    """backbones.LYNXNet keeps its constructor; the width rule is the library's, met when the native handle is made (on a GPU:
    tests/test_gpu_width.py).  The shim builds the reference's state_dict at any width."""
    from diffsinger_amd.aux_decoder import build_aux_decoder
    from diffsinger_amd.backbones import build_backbone
    from diffsinger_amd.hparams import hparams
    hparams.update(hidden_size=256)
    for tag, (in_dims, n_feats, args, _, _) in wc.LYNX_EVALS.items():
        sd = build_backbone(in_dims, n_feats, "lynxnet", args).state_dict()
        shapes = synth.backbone_param_shapes("lynxnet", in_dims, n_feats, hidden_size=256, **args)
        assert set(sd) == set(shapes) and all(tuple(sd[k].shape) == tuple(v) for k, v in shapes.items()), tag
    for tag, (hsz, m, args, _, _, _) in wc.AUX.items():
        sd = build_aux_decoder(hsz, m, "convnext", dict(args)).state_dict()
        shapes = synth.convnext_param_shapes(hsz, m, num_channels=args["num_channels"], num_layers=args["num_layers"],
                                             kernel_size=args["kernel_size"])
        assert set(sd) == set(shapes) and all(tuple(sd[k].shape) == tuple(v) for k, v in shapes.items()), tag
