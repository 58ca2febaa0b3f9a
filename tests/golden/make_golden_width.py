"""Generator of G20 (tests/golden/g20_width.npz): the reference's own LYNXNet (modules/backbones/lynxnet.py), RectifiedFlow
(modules/core/reflow.py) and AuxDecoderAdaptor (modules/aux_decoder) at channel counts that are not multiples of 32, run in fp32
on the CPU with the seeded weights and inputs of diffsinger_amd/synth.py (the cases: tests/width_cases.py).  Only outputs, t values,
seeds and the weight digests are stored, as G2 / G3 / G5 / G7 do.

Runs on a machine with the reference tree; the tests only read the .npz.  `lightning` (imported by utils/training_utils.py, never
executed on this path) is stubbed, and torch.randn is replaced while the sampler runs so that x_T is the seed-derived tensor the
oracle and the library are fed later.

    python tests/golden/make_golden_width.py /path/to/reference
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import width_cases as wc  # noqa: E402
from diffsinger_amd import synth  # noqa: E402


def _stub_lightning():
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m

    class _Dummy:
        def __init__(self, *a, **k):
            pass

    stub("lightning")
    stub("lightning.pytorch", LightningModule=_Dummy, Trainer=_Dummy, Callback=_Dummy)
    stub("lightning.fabric")
    stub("lightning.fabric.loggers")
    stub("lightning.fabric.loggers.tensorboard", _TENSORBOARD_AVAILABLE=False)
    stub("lightning.pytorch.callbacks", ModelCheckpoint=_Dummy, TQDMProgressBar=_Dummy)
    stub("lightning.pytorch.loggers", TensorBoardLogger=_Dummy)
    stub("lightning.pytorch.utilities")
    stub("lightning.pytorch.utilities.rank_zero", rank_zero_info=print, rank_zero_only=lambda f: f, rank_zero_debug=print)


def to_t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def main(ref_root):
    _stub_lightning()
    sys.path.insert(0, ref_root)
    from utils.hparams import hparams
    from modules.backbones import build_backbone
    from modules.core import reflow as ref_reflow
    from modules.aux_decoder import AuxDecoderAdaptor
    torch.set_num_threads(8)

    def set_hp(**kw):
        hparams.clear()
        hparams.update(hidden_size=256, schedule_type="linear", use_shallow_diffusion=False, diff_speedup=10,
                       diff_accelerator="ddim", infer=False, sampling_algorithm="euler", sampling_steps=20)
        hparams.update(kw)

    def load_synth(module, in_dims, n_feats, args, seed):
        shapes = synth.backbone_param_shapes("lynxnet", in_dims, n_feats, hidden_size=hparams["hidden_size"], **args)
        sd = synth.synth_state_dict(shapes, seed=seed)
        module.load_state_dict({k: to_t(v) for k, v in sd.items()}, strict=True)
        module.eval()
        return synth.state_dict_digest(sd)

    out = {}
    set_hp()
    for tag, (in_dims, n_feats, args, wseed, cases) in wc.LYNX_EVALS.items():
        net = build_backbone(in_dims, n_feats, "lynxnet", args)
        out[f"{tag}_digest"] = np.array(load_synth(net, in_dims, n_feats, args, wseed))
        for ci, (bsz, t_len, tkind) in enumerate(cases):
            xs, cs, ts = wc.eval_seeds(ci)
            x = synth.synth_normal((bsz, n_feats, in_dims, t_len), xs)
            cond = synth.synth_normal((bsz, 256, t_len), cs)
            t = wc.make_t(tkind, bsz, ts)
            with torch.no_grad():
                y = net(to_t(x), to_t(t), to_t(cond)).numpy()
            out[f"{tag}_c{ci}_t"] = t
            out[f"{tag}_c{ci}_out"] = y
            print(f"lynxnet {tag} case {ci}: out {y.shape} absmax {np.abs(y).max():.3f}")

    s = wc.SAMPLER
    set_hp(sampling_algorithm="euler", sampling_steps=s["steps"], T_start_infer=0.0)
    r = ref_reflow.RectifiedFlow(s["in_dims"], s["n_feats"], t_start=0.0, time_scale_factor=1000, backbone_type="lynxnet",
                                 backbone_args=s["args"], spec_min=[-12.0], spec_max=[0.0])
    out["rf_digest"] = np.array(load_synth(r.velocity_fn, s["in_dims"], s["n_feats"], s["args"], s["wseed"]))
    cond = synth.synth_normal((s["bsz"], s["t_len"], 256), s["cond_seed"])
    orig, calls = torch.randn, []

    def fake(*size, **kw):
        if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
            size = tuple(size[0])
        calls.append(size)
        return to_t(synth.synth_normal(tuple(int(v) for v in size), s["noise_seed"] + len(calls) - 1))

    torch.randn = fake
    try:
        with torch.no_grad():
            y = r(to_t(cond), infer=True).numpy()
    finally:
        torch.randn = orig
    assert len(calls) == 1, calls          # euler draws x_T only
    out["rf_euler10_out"] = y
    print(f"reflow euler{s['steps']}: out {y.shape} absmax {np.abs(y).max():.3f}")

    set_hp()
    for tag, (hsz, m, args, bsz, t_len, wseed) in wc.AUX.items():
        rng = np.random.Generator(np.random.PCG64(wseed))
        smin = (-12.0 + rng.random(m)).astype(np.float32)
        smax = (0.0 + rng.random(m)).astype(np.float32)
        a = AuxDecoderAdaptor(hsz, m, 1, smin.tolist(), smax.tolist(), "convnext", dict(args))
        shapes = synth.convnext_param_shapes(hsz, m, num_channels=args["num_channels"], num_layers=args["num_layers"],
                                             kernel_size=args["kernel_size"], prefix="decoder.")
        sd = synth.synth_state_dict(shapes, seed=wseed)
        a.load_state_dict({k: to_t(v) for k, v in sd.items()}, strict=True)
        a.eval()
        cond = synth.synth_normal((bsz, t_len, hsz), wseed + 100)
        with torch.no_grad():
            raw = a(to_t(cond), infer=False).numpy()
            mel = a(to_t(cond), infer=True).numpy()
        out[f"{tag}_digest"] = np.array(synth.state_dict_digest(sd))
        out[f"{tag}_smin"], out[f"{tag}_smax"] = smin, smax
        out[f"{tag}_raw"], out[f"{tag}_mel"] = raw, mel
        print(f"aux {tag}: raw absmax {np.abs(raw).max():.3f} mel range ({mel.min():.2f}, {mel.max():.2f})")

    path = os.path.join(HERE, "g20_width.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main(sys.argv[1])
