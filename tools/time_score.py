#!/usr/bin/env python3
"""One validation scoring step, timed: `forward_score` + the loss of the fork's default acoustic
denoiser (DDPM, WaveNet 20 x 256, 128 bins) and of its pitch predictor (PitchDiffusion, 64 repeated bins, WaveNet 20 x
256) at B = 8, T = 1000 with seeded weights, split into the noising step, the denoiser evaluation and the loss; and each
reduction beside torch's own ops on the GPU at the same shape - DiffusionLoss / RectifiedFlowLoss against the masked
`.mean()` expression, RawCurveR2Score against its five torch reductions, DurationLoss against the scatter_add / log / mse
chain.  Device-event times, 10 warm-up calls, the median of 50, all in one process; GPU box only.  Nothing is asserted.
Prints one JSON line; `--out FILE` also writes it there."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from diffsinger_amd import losses, metrics, score, synth  # noqa: E402
from diffsinger_amd.diffusion import GaussianDiffusion, PitchDiffusion  # noqa: E402
from diffsinger_amd.hparams import hparams  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=50)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--frames", type=int, default=1000)
ap.add_argument("--out")
args = ap.parse_args()
assert torch.cuda.is_available(), "time_score.py needs the MI355X"
B, T = args.batch, args.frames


def timed(fn):
    for _ in range(args.warmup):
        fn()
    times = []
    for _ in range(args.repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def dev(a):
    return torch.from_numpy(a).cuda()


hparams.clear()
hparams.update(hidden_size=256, schedule_type="linear", use_shallow_diffusion=False, diff_speedup=10, diff_accelerator="ddim")
args_wn = dict(num_layers=20, num_channels=256, dilation_cycle_length=4)
res = {"B": B, "T": T}
with torch.no_grad():
    cond = dev(synth.synth_normal((B, T, 256), 1))
    npad = torch.ones((B, T, 1), device="cuda")
    npad[-1, T - T // 4:] = 0
    seeds = list(range(B))
    for tag, w, gt in (
            ("acoustic", GaussianDiffusion(128, 1, backbone_type="wavenet", backbone_args=args_wn, spec_min=[-12.0], spec_max=[0.0]),
             -6.0 + 3.0 * dev(synth.synth_normal((B, T, 128), 2))),
            ("pitch", PitchDiffusion(-8.0, 8.0, -12.0, 12.0, 64, backbone_type="wavenet", backbone_args=args_wn),
             3.0 * dev(synth.synth_normal((B, T), 3)))):
        m = w.out_dims
        sd = synth.synth_state_dict(synth.backbone_param_shapes("wavenet", m, 1, hidden_size=256, **args_wn), seed=11)
        w.denoise_fn.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        w = w.cuda().eval()
        loss = losses.DiffusionLoss("l2")
        spec = w.norm_spec(gt).transpose(-2, -1)[:, None].contiguous()
        t = torch.randint(0, 1000, (B,), device="cuda")
        a, c = w.sqrt_alphas_cumprod[t], w.sqrt_one_minus_alphas_cumprod[t]
        x_t, eps = score.diffuse("ddpm", spec, a, c, seeds=seeds)
        pred = w.denoise_fn(x_t, t, cond.transpose(1, 2))
        res[f"{tag}_step_ms"] = timed(lambda: loss(*w.forward_score(cond, gt, seed=seeds), non_padding=npad))
        res[f"{tag}_diffuse_seeded_ms"] = timed(lambda: score.diffuse("ddpm", spec, a, c, seeds=seeds))
        res[f"{tag}_diffuse_given_ms"] = timed(lambda: score.diffuse("ddpm", spec, a, c, eps=eps, want_target=False))
        res[f"{tag}_torch_q_sample_ms"] = timed(lambda: w.q_sample(spec, t, torch.randn_like(spec)))
        res[f"{tag}_denoise_ms"] = timed(lambda: w.denoise_fn(x_t, t, cond.transpose(1, 2)))
        res[f"{tag}_loss_ms"] = timed(lambda: loss(pred, eps, non_padding=npad))
        mask = npad.transpose(1, 2).unsqueeze(1)
        res[f"{tag}_torch_loss_ms"] = timed(lambda: ((pred * mask - eps * mask) ** 2).mean())
        rf = losses.RectifiedFlowLoss("l2")
        tf = torch.rand(B, device="cuda")
        res[f"{tag}_lognorm_loss_ms"] = timed(lambda: rf(pred, eps, tf, non_padding=npad))
        res[f"{tag}_torch_lognorm_loss_ms"] = timed(lambda: (rf.get_weights(tf) * (pred * mask - eps * mask) ** 2).mean())
        w.denoise_fn.release_native()
    # curve metric and duration loss against their torch ops
    tgt = 60.0 + 5.0 * dev(synth.synth_normal((B, T), 4))
    prd = tgt + 0.5 * dev(synth.synth_normal((B, T), 5))
    cm = npad[..., 0] > 0
    r2 = metrics.RawCurveR2Score()

    def torch_r2():
        p, g = prd[cm], tgt[cm]
        r = g - p
        return torch.sum(g), torch.sum(g * g), torch.sum(r * r), cm.sum()

    res["curve_r2_update_ms"] = timed(lambda: r2.update(prd, tgt, mask=cm))
    res["torch_curve_r2_update_ms"] = timed(torch_r2)
    n_ph, n_word = 120, 40
    p2w = (torch.arange(n_ph, device="cuda") // 3 + 1)[None].expand(B, n_ph).contiguous()
    dgt = torch.randint(2, 30, (B, n_ph), device="cuda").float()
    dpr = dgt + dev(synth.synth_normal((B, n_ph), 6))
    dl = losses.DurationLoss(1.0, "mse")

    def torch_dur():
        lg = lambda v: torch.log(v + 1.0)       # noqa: E731
        mse = torch.nn.functional.mse_loss
        c = dpr.clamp(min=0.)
        wp = c.new_zeros(B, n_word + 1).scatter_add(1, p2w, c)[:, 1:]
        wg = dgt.new_zeros(B, n_word + 1).scatter_add(1, p2w, dgt)[:, 1:]
        return 0.6 * mse(lg(dpr), lg(dgt)) + 0.3 * mse(lg(wp), lg(wg)) + 0.1 * mse(lg(c.sum(1)), lg(dgt.sum(1)))

    res["dur_loss_ms"] = timed(lambda: score.dur_score(dpr, dgt, p2w, n_words=n_word + 1))
    res["dur_loss_module_ms"] = timed(lambda: dl(dpr, dgt, p2w))     # reads ph2word.max() back, as the reference does
    res["torch_dur_loss_ms"] = timed(torch_dur)
line = json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()})
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
