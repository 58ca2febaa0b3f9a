"""Generator of G25 (tests/golden/g25_score.npz): the reference's own validation scoring, run in fp32 on the CPU on the
cases of tests/score_cases.py with the seeded weights of diffsinger_amd/synth.py -
  - GaussianDiffusion.p_losses (modules/core/ddpm.py) with explicit t and noise, RectifiedFlow.p_losses
    (modules/core/reflow.py) under a recorded torch.manual_seed (its x_start is redrawn under the same seed and stored),
    on a WaveNet and a LYNXNet, one repeat-bins pitch codec and one multi-curve codec;
  - DiffusionLoss, RectifiedFlowLoss, DurationLoss (modules/losses/), the aux decoders' L1 loss and the four metrics of
    modules/metrics/ on seeded inputs and on the p_losses outputs;
  - DiffSingerVariance.forward(infer=False) (modules/toplevel.py) on two configurations of tests/variance_cases.py, the draws
    it made recorded (RecordDraws), with the variance task's loss terms; and the `else` branch of DiffSingerAcoustic.forward
    on a given condition - AuxDecoderAdaptor(infer=False) behind the aux_decoder_grad mix and GaussianDiffusion.p_losses at
    K_step 400 - with the acoustic task's loss terms.
For every scalar the reference's fp32 value (`*_ref32`) and the float64 value of tests/score_ref.py on the same inputs
(`*_ref64`) are stored: their distance is the reference's own rounding, which the GPU tests' bound is made of.

Data only.  Runs on a machine with the reference tree; the tests only read the .npz.  `lightning` (imported by
utils/training_utils.py, never executed on this path) is stubbed as in make_golden_width.py; `modules/metrics` imports
torchmetrics, which is absent: a stand-in `torchmetrics.Metric` (only `__init__` and `add_state`) is placed in
sys.modules - the `update` / `compute` code that runs is the reference's own.

    python tests/golden/make_golden_score.py /path/to/reference
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import score_cases as sc  # noqa: E402
import score_ref as sr  # noqa: E402
from diffsinger_amd import synth  # noqa: E402


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m


def _stub_lightning():
    class _Dummy:
        def __init__(self, *a, **k):
            pass

    _stub("lightning")
    _stub("lightning.pytorch", LightningModule=_Dummy, Trainer=_Dummy, Callback=_Dummy)
    _stub("lightning.fabric")
    _stub("lightning.fabric.loggers")
    _stub("lightning.fabric.loggers.tensorboard", _TENSORBOARD_AVAILABLE=False)
    _stub("lightning.pytorch.callbacks", ModelCheckpoint=_Dummy, TQDMProgressBar=_Dummy)
    _stub("lightning.pytorch.loggers", TensorBoardLogger=_Dummy)
    _stub("lightning.pytorch.utilities")
    _stub("lightning.pytorch.utilities.rank_zero", rank_zero_info=print, rank_zero_only=lambda f: f, rank_zero_debug=print)


def _stub_torchmetrics():
    class Metric:
        def __init__(self, **kwargs):
            pass

        def add_state(self, name, default, dist_reduce_fx=None):
            setattr(self, name, default.clone())

    _stub("torchmetrics", Metric=Metric)


def to_t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


class RecordDraws:
    """Inside the block torch.randint / torch.rand / torch.randn_like still draw what they draw, and every result is kept
    in call order: the reference's forward(infer=False) takes no t or noise, so what it drew is stored and handed to
    forward_score by the tests."""

    def __enter__(self):
        self.saved = torch.randint, torch.rand, torch.randn_like
        self.calls = []

        def wrap(name, fn):
            def inner(*a, **k):
                v = fn(*a, **k)
                self.calls.append((name, v.clone()))
                return v
            return inner

        torch.randint, torch.rand, torch.randn_like = (wrap(n, f) for n, f in zip(("randint", "rand", "randn_like"), self.saved))
        return self

    def __exit__(self, *exc):
        torch.randint, torch.rand, torch.randn_like = self.saved


def main(ref_root):
    _stub_lightning()
    _stub_torchmetrics()
    sys.path.insert(0, ref_root)
    from utils.hparams import hparams
    from modules.core import ddpm as ref_ddpm, reflow as ref_reflow
    from modules.losses import DiffusionLoss, DurationLoss, RectifiedFlowLoss
    from modules.metrics import PhonemeDurationAccuracy, RawCurveAccuracy, RawCurveR2Score, RhythmCorrectness
    from modules.aux_decoder import build_aux_loss
    torch.set_num_threads(8)
    hparams.clear()
    hparams.update(hidden_size=sc.HIDDEN, schedule_type="linear", use_shallow_diffusion=False, diff_speedup=10,
                   diff_accelerator="ddim", infer=False, sampling_algorithm="euler", sampling_steps=20)
    out = {}

    def scalar(name, ref32, ref64):
        out[f"{name}_ref32"] = np.float32(ref32)
        out[f"{name}_ref64"] = np.float64(ref64)
        print(f"  {name}: ref32 {float(ref32):.9g}  ref64 {float(ref64):.17g}  |d| {abs(float(ref32) - float(ref64)):.3g}")

    # ---- p_losses of the two wrappers and their codecs
    for tag, c in sc.WRAPPERS.items():
        mod = ref_ddpm if c["family"] == "ddpm" else ref_reflow
        w = getattr(mod, c["cls"])(**sc.wrapper_kwargs(tag))
        net = w.denoise_fn if c["family"] == "ddpm" else w.velocity_fn
        f, m = sc.dims(tag)
        sd = synth.synth_state_dict(synth.backbone_param_shapes(c["backbone"], m, f, hidden_size=sc.HIDDEN, **c["args"]),
                                    seed=c["wseed"])
        net.load_state_dict({k: to_t(v) for k, v in sd.items()}, strict=True)
        w.eval()
        out[f"{tag}_digest"] = np.array(synth.state_dict_digest(sd))
        inp = sc.wrapper_inputs(tag)
        gt = [to_t(g) for g in inp["gt"]] if isinstance(inp["gt"], list) else to_t(inp["gt"])
        cond = to_t(inp["cond"]).transpose(1, 2)
        t = to_t(inp["t"])
        non_padding = to_t(inp["non_padding"])
        with torch.no_grad():
            spec = w.norm_spec(gt).transpose(-2, -1)
            if w.num_feats == 1:
                spec = spec[:, None, :, :]
            if c["family"] == "ddpm":
                noise = to_t(inp["noise"])
                x_t = w.q_sample(x_start=spec, t=t, noise=noise)
                pred, target = w.p_losses(spec, t, cond=cond, noise=noise)
            else:
                torch.manual_seed(inp["torch_seed"])
                noise = torch.randn_like(spec)                  # what p_losses draws as x_start under the same seed
                x_t = noise + t[:, None, None, None] * (spec - noise)
                torch.manual_seed(inp["torch_seed"])
                pred, target = w.p_losses(spec, t, cond=cond)
                assert torch.equal(target, spec - noise)
            out[f"{tag}_spec"], out[f"{tag}_noise"], out[f"{tag}_x_t"] = spec.numpy().copy(), noise.numpy(), x_t.numpy()
            out[f"{tag}_pred"], out[f"{tag}_target"] = pred.numpy(), target.numpy()
            print(f"{tag}: spec {tuple(spec.shape)} pred absmax {pred.abs().max():.3f}")
            npad = inp["non_padding"][..., 0]
            for kind in ("l1", "l2"):
                if c["family"] == "ddpm":
                    v = DiffusionLoss(kind)(pred, target, non_padding=non_padding)
                    scalar(f"{tag}_{kind}", v, sr.masked_loss(kind, pred.numpy(), target.numpy(), npad)[1])
                else:
                    v = RectifiedFlowLoss(kind, log_norm=True)(pred, target, t=t, non_padding=non_padding)
                    scalar(f"{tag}_{kind}", v, sr.masked_loss(kind, pred.numpy(), target.numpy(), npad, inp["t"])[1])

    # ---- the loss modules on seeded inputs
    with torch.no_grad():
        li = sc.loss_inputs()
        p, g, npad, t = (to_t(li[k]) for k in ("pred", "target", "non_padding", "t"))
        npad2 = li["non_padding"][..., 0]
        for kind in ("l1", "l2"):
            scalar(f"diff_{kind}_masked", DiffusionLoss(kind)(p, g, non_padding=npad), sr.masked_loss(kind, li["pred"], li["target"], npad2)[1])
            scalar(f"diff_{kind}", DiffusionLoss(kind)(p, g), sr.masked_loss(kind, li["pred"], li["target"])[1])
            scalar(f"rf_{kind}_lognorm_masked", RectifiedFlowLoss(kind, log_norm=True)(p, g, t=t, non_padding=npad),
                   sr.masked_loss(kind, li["pred"], li["target"], npad2, li["t"])[1])
            scalar(f"rf_{kind}_plain", RectifiedFlowLoss(kind, log_norm=False)(p, g, t=t),
                   sr.masked_loss(kind, li["pred"], li["target"])[1])
        scalar("aux_l1", build_aux_loss("convnext")(p[:, 0].transpose(1, 2), g[:, 0].transpose(1, 2)),
               sr.masked_loss("l1", li["pred"], li["target"])[1])
        out["rf_weights_ref32"] = RectifiedFlowLoss.get_weights(t).reshape(-1).numpy()
        out["rf_weights_ref64"] = sr.lognorm_weight(li["t"])

        di = sc.dur_inputs()
        raw, gt, p2w = to_t(di["dur_pred_raw"]), to_t(di["dur_gt"]), to_t(di["ph2word"])
        lp, lw, ls = di["lambdas"]
        for kind in ("mse", "huber"):
            v = DurationLoss(di["offset"], kind, lambda_pdur=lp, lambda_wdur=lw, lambda_sdur=ls)(raw, gt, ph2word=p2w)
            res = sr.dur_score(di["dur_pred_raw"], di["dur_gt"], di["ph2word"], offset=di["offset"], loss_type=kind)
            scalar(f"dur_{kind}", v, sr.dur_loss(res, lp, lw, ls))
        shape = (sc.B, int(di["ph2word"].max()) + 1)
        out["dur_wdur_pred"] = raw.clamp(min=0.).new_zeros(*shape).scatter_add(1, p2w, raw.clamp(min=0.))[:, 1:].numpy()
        out["dur_wdur_gt"] = gt.new_zeros(*shape).scatter_add(1, p2w, gt)[:, 1:].numpy()

        # ---- the metrics
        pred_i, mask = to_t(di["dur_pred"]), to_t(di["mask"])
        for name, mk in (("nomask", None), ("mask", mask)):
            res = sr.dur_score(di["dur_pred"], di["dur_gt"], di["ph2word"], mask=None if mk is None else di["mask"],
                               rhythm_tolerance=di["rhythm_tolerance"], pdur_tolerance=di["pdur_tolerance"])
            rc = RhythmCorrectness(tolerance=di["rhythm_tolerance"])
            rc.update(pred_i, gt.long(), p2w, mask=mk)
            out[f"rhythm_{name}_counts"] = np.array([int(rc.correct), int(rc.total)], np.int64)
            assert [int(rc.correct), int(rc.total)] == res["counts"][:2], (name, res["counts"])
            scalar(f"rhythm_{name}", rc.compute(), res["counts"][0] / res["counts"][1])
            pa = PhonemeDurationAccuracy(tolerance=di["pdur_tolerance"])
            pa.update(pred_i, gt.long(), p2w, mask=mk)
            out[f"pdur_{name}_counts"] = np.array([int(pa.accurate), int(pa.total)], np.int64)
            assert [int(pa.accurate), int(pa.total)] == res["counts"][2:], (name, res["counts"])
            scalar(f"pdur_{name}", pa.compute(), res["counts"][2] / res["counts"][3])

        ci = sc.curve_inputs()
        cp, cg, cm = to_t(ci["pred"]), to_t(ci["target"]), to_t(ci["mask"])
        for name, mk in (("nomask", None), ("mask", cm)):
            st = sr.curve_stats(ci["pred"], ci["target"], None if mk is None else ci["mask"], ci["tolerance"])
            acc = RawCurveAccuracy(tolerance=ci["tolerance"])
            acc.update(cp, cg, mask=mk)
            assert (int(acc.close), int(acc.total)) == (st["close"], st["total"]), (name, st)
            out[f"curve_{name}_counts"] = np.array([int(acc.close), int(acc.total)], np.int64)
            scalar(f"curve_acc_{name}", acc.compute(), sr.curve_accuracy(st))
            r2 = RawCurveR2Score()
            r2.update(cp, cg, mask=mk)
            scalar(f"curve_r2_{name}", r2.compute(), sr.curve_r2(st))
            out[f"curve_{name}_sums64"] = np.array([st["sum_target"], st["sum_target_sq"], st["sum_residual_sq"]])

    # ---- the top-level variance model, forward(infer=False) and the task's loss terms (variance_task.py:216-249)
    from modules.toplevel import DiffSingerVariance
    import variance_cases as vc
    for tag in sc.VARIANCE_TAGS:
        hp = sc.variance_hparams(tag)
        hparams.clear()
        hparams.update(hp, infer=False)
        c = vc.CASES[tag]
        model = DiffSingerVariance(c["vocab"])
        shapes = vc.sorted_param_shapes(model.named_parameters())
        sd = vc.synth_weights(shapes, c["seed"] + 1)
        model.load_state_dict({k: to_t(v) for k, v in sd.items()}, strict=False)
        model.eval()
        sample, retakes, names = sc.variance_sample(tag)
        kw = {k: to_t(v) for k, v in sample.items() if k not in ("size", "tokens", "spk_ids")}
        kw.update(pitch_retake=to_t(retakes["pitch_retake"]), spk_id=to_t(sample["spk_ids"]) if "spk_ids" in sample else None)
        if names:
            kw["variance_retake"] = {n: to_t(v) for n, v in retakes["variance_retake"].items()}
        torch.manual_seed(c["seed"] + 60)
        with RecordDraws() as rec, torch.no_grad():
            dur, pitch, var = model(to_t(sample["tokens"]), infer=False, **kw)
        kinds = [n for n, _ in rec.calls]
        first = "rand" if hp["diffusion_type"] == "reflow" else "randint"
        assert kinds == [first, "randn_like"] * (1 + bool(names)), kinds
        out[f"v_{tag}_pitch_t"], out[f"v_{tag}_pitch_noise"] = rec.calls[0][1].numpy(), rec.calls[1][1].contiguous().numpy()
        if hp["diffusion_type"] == "reflow":    # t = t_start + (1 - t_start) * rand with t_start = 0: the draw itself
            assert torch.equal(pitch[2], rec.calls[0][1])
        non_padding = (to_t(sample["mel2ph"]) > 0).unsqueeze(-1)
        npad = (sample["mel2ph"] > 0).astype(np.float32)
        mk = (lambda: DiffusionLoss("l2")) if hp["diffusion_type"] == "ddpm" else (lambda: RectifiedFlowLoss("l2", log_norm=True))

        def main_loss(o):
            with torch.no_grad():
                if hp["diffusion_type"] == "ddpm":
                    return mk()(o[0], o[1], non_padding=non_padding), sr.masked_loss("l2", o[0].numpy(), o[1].numpy(), npad)[1]
                return (mk()(o[0], o[1], t=o[2], non_padding=non_padding),
                        sr.masked_loss("l2", o[0].numpy(), o[1].numpy(), npad, o[2].numpy())[1])

        out[f"v_{tag}_pitch_pred"], out[f"v_{tag}_pitch_target"] = pitch[0].numpy(), pitch[1].numpy()
        scalar(f"v_{tag}_pitch_loss", *main_loss(pitch))
        if names:
            out[f"v_{tag}_variance_t"], out[f"v_{tag}_variance_noise"] = rec.calls[2][1].numpy(), rec.calls[3][1].contiguous().numpy()
            out[f"v_{tag}_var_pred"], out[f"v_{tag}_var_target"] = var[0].numpy(), var[1].numpy()
            scalar(f"v_{tag}_var_loss", *main_loss(var))
        else:
            assert var is None
        if hp["predict_dur"]:
            d = hp["dur_prediction_args"]
            out[f"v_{tag}_dur"] = dur.numpy()
            lam = (d["lambda_pdur_loss"], d["lambda_wdur_loss"], d["lambda_sdur_loss"])
            with torch.no_grad():
                v = DurationLoss(d["log_offset"], d["loss_type"], *lam)(dur, to_t(sample["ph_dur"]), ph2word=to_t(sample["ph2word"]))
            res = sr.dur_score(dur.numpy(), sample["ph_dur"], sample["ph2word"], offset=d["log_offset"], loss_type=d["loss_type"])
            scalar(f"v_{tag}_dur_loss", v, sr.dur_loss(res, *lam))
            print(f"  raw durations: min {float(dur.min()):.3f} (negative: {int((dur < 0).sum())}), at padding {dur[-1, -1]:.3f}")
        else:
            assert dur is None

    # ---- the acoustic decoder under shallow diffusion: the else branch of toplevel.py:106-122 on a given condition
    from modules.aux_decoder import AuxDecoderAdaptor
    hp = sc.acoustic_hparams()
    hparams.clear()
    hparams.update(hp, infer=False)
    a = sc.ACOUSTIC
    sh = hp["shallow_diffusion_args"]
    aux = AuxDecoderAdaptor(in_dims=sc.HIDDEN, out_dims=a["M"], num_feats=1, spec_min=hp["spec_min"], spec_max=hp["spec_max"],
                            aux_decoder_arch=sh["aux_decoder_arch"], aux_decoder_args=sh["aux_decoder_args"])
    diff = ref_ddpm.GaussianDiffusion(out_dims=a["M"], num_feats=1, timesteps=hp["timesteps"], k_step=hp["K_step"],
                                      backbone_type="wavenet", backbone_args=dict(sc.WN), spec_min=hp["spec_min"],
                                      spec_max=hp["spec_max"])
    aux_sd, net_sd = sc.acoustic_weights()
    aux.load_state_dict({k: to_t(v) for k, v in aux_sd.items()}, strict=True)
    diff.denoise_fn.load_state_dict({k: to_t(v) for k, v in net_sd.items()}, strict=True)
    aux.eval(), diff.eval()
    sample, draws = sc.acoustic_sample()
    cond, mel = to_t(sample["condition"]), to_t(sample["mel"])
    with torch.no_grad():
        g_ = sh["aux_decoder_grad"]
        aux_out = aux(cond * g_ + cond.detach() * (1 - g_), infer=False)
        aux_plain = aux(cond, infer=False)
        spec = diff.norm_spec(mel).transpose(-2, -1)[:, None]
        x_recon, noise = diff.p_losses(spec, to_t(draws["t"]), cond=cond.transpose(1, 2), noise=to_t(draws["noise"]))
        out["ac_aux_out"], out["ac_x_recon"] = aux_out.numpy(), x_recon.numpy()
        print(f"acoustic: aux_out absmax {aux_out.abs().max():.3f}, the grad mix moves it by {(aux_out - aux_plain).abs().max():.3g}")
        norm_gt = aux.norm_spec(mel)
        scalar("ac_aux_mel_loss", hp["lambda_aux_mel_loss"] * build_aux_loss("convnext")(aux_out, norm_gt),
               hp["lambda_aux_mel_loss"] * sr.masked_loss("l1", aux_out.numpy(), norm_gt.numpy())[1])
        non_padding = (to_t(sample["mel2ph"]) > 0).unsqueeze(-1).float()
        scalar("ac_mel_loss", DiffusionLoss("l2")(x_recon, noise, non_padding=non_padding),
               sr.masked_loss("l2", x_recon.numpy(), noise.numpy(), (sample["mel2ph"] > 0).astype(np.float32))[1])

    # ---- the public layout: signatures and state names (lists of names, compared by tests/test_score_host.py)
    import inspect
    for cls, methods in ((DiffusionLoss, ("__init__", "forward")), (RectifiedFlowLoss, ("__init__", "forward", "get_weights")),
                         (DurationLoss, ("__init__", "forward", "linear2log")),
                         (RawCurveAccuracy, ("__init__", "update", "compute")), (RawCurveR2Score, ("__init__", "update", "compute")),
                         (RhythmCorrectness, ("__init__", "update", "compute")),
                         (PhonemeDurationAccuracy, ("__init__", "update", "compute"))):
        for meth in methods:
            params = inspect.signature(getattr(cls, meth)).parameters.values()
            out[f"sig_{cls.__name__}_{meth}"] = np.array([f"{q.name}:{q.kind.name}:{'' if q.default is q.empty else repr(q.default)}"
                                                          for q in params])
    for name, obj in (("RawCurveAccuracy", RawCurveAccuracy(tolerance=0.5)), ("RawCurveR2Score", RawCurveR2Score()),
                      ("RhythmCorrectness", RhythmCorrectness(tolerance=0.05)),
                      ("PhonemeDurationAccuracy", PhonemeDurationAccuracy(tolerance=0.2))):
        out[f"states_{name}"] = np.array(sorted(k for k, v in vars(obj).items() if torch.is_tensor(v)))

    path = os.path.join(HERE, "g25_score.npz")
    np.savez_compressed(path, **out)
    print(f"wrote g25_score.npz ({os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays)")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("DIFFSINGER_REFERENCE", ""))
