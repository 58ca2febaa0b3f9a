#!/usr/bin/env python3
"""Seeded draws on the device, timed and measured: noise.fill against torch.randn of the same
shape for x_T [1, 1, 128, 1000], a 50-step chunk of it and the vocoder's source noise [1, 512000, 9] - one call between
two device events, which at these sizes is mostly the launch, and 20 back-to-back calls between two events divided by 20,
which is the kernel; a seeded against a default ancestral-DDPM run of 100 steps at T = 1000 (WaveNet 20 x 256, shallow
start, the default lazy hipGraph policy: the seeded run keeps its noise pointer, so its chunks replay from captured
graphs); and the largest deviation of 2 M device normals from the float64 oracle (tests/noise_ref.py).  Device-event
times, 10 warm-up calls, the median of 50, all in one process; GPU box only.  Prints one JSON line; `--out FILE` also
writes it there."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import noise_ref  # noqa: E402
from diffsinger_amd import noise, synth  # noqa: E402
from diffsinger_amd.diffusion import GaussianDiffusion  # noqa: E402
from diffsinger_amd.hparams import hparams  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=50)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--out")
args = ap.parse_args()
assert torch.cuda.is_available(), "time_noise.py needs the MI355X"


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


res = {}
with torch.no_grad():
    # fill against torch.randn, both into a preallocated tensor (the allocator is not what is compared)
    for tag, shape in (("x_T_1x128x1000", (1, 1, 128, 1000)), ("chunk_50x128x1000", (50, 1, 128, 1000)),
                       ("voc_source_512000x9", (1, 1, 512000, 9))):
        out = torch.empty(shape, device="cuda")
        res[f"{tag}_fill_ms"] = timed(lambda: noise.fill(shape, [7], noise.STEP, out=out))
        res[f"{tag}_randn_ms"] = timed(lambda: torch.randn(shape, device="cuda", out=out))
        res[f"{tag}_fill_x20_ms_per_call"] = timed(lambda: [noise.fill(shape, [7], noise.STEP, out=out) for _ in range(20)]) / 20
        res[f"{tag}_randn_x20_ms_per_call"] = timed(lambda: [torch.randn(shape, device="cuda", out=out) for _ in range(20)]) / 20
        res[f"{tag}_elements"] = int(out.numel())
    out = torch.empty((1, 1, 1, 9), device="cuda")
    res["voc_phase_uniform_fill_ms"] = timed(lambda: noise.fill((1, 1, 1, 9), [7], noise.VOC_PHASE, kind="uniform", out=out))
    res["voc_phase_rand_ms"] = timed(lambda: torch.rand(9, device="cuda"))

    # exactness: 2 M normals and uniforms against the oracle
    shape = (1, 1, 2048, 1024)
    seed = 0x9e3779b97f4a7c15
    z = noise.fill(shape, [seed], noise.X_T).cpu().numpy().astype(np.float64)
    res["normal_max_abs_dev_2M"] = float(np.abs(z - noise_ref.fill(shape, [seed], noise_ref.X_T)).max())
    res["normal_mean_2M"], res["normal_var_2M"], res["normal_max_abs_2M"] = float(z.mean()), float(z.var()), float(np.abs(z).max())
    u = noise.fill(shape, [seed], noise.X_T, kind="uniform").cpu().numpy().astype(np.float64)
    res["uniform_bitwise_2M"] = bool(np.array_equal(u, noise_ref.fill(shape, [seed], noise_ref.X_T, kind="uniform")))

    # ancestral DDPM, 100 steps (two 50-step chunks) at T = 1000: seed= against the default torch.randn path
    hparams.clear()
    hparams.update(hidden_size=256, schedule_type="linear", use_shallow_diffusion=True, diff_speedup=1, K_step_infer=100,
                   diff_accelerator="ddim", infer=False)
    bargs = dict(num_layers=20, num_channels=256, dilation_cycle_length=4)
    d = GaussianDiffusion(128, 1, timesteps=1000, k_step=100, backbone_type="wavenet", backbone_args=bargs,
                          spec_min=[-12.0], spec_max=[0.0])
    d.denoise_fn.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(
        synth.backbone_param_shapes("wavenet", 128, 1, hidden_size=256, **bargs), seed=42).items()}, strict=True)
    d = d.cuda().eval()
    cond = torch.from_numpy(synth.synth_normal((1, 1000, 256), 1)).cuda()
    src = torch.from_numpy((synth.synth_normal((1, 1000, 128), 2) * 1.5 - 6.0).astype(np.float32)).cuda()
    stats = lambda: d.denoise_fn.stats()["graphs_cached"]  # noqa: E731
    res["ancestral100_seeded_ms"] = timed(lambda: d(cond, src_spec=src, infer=True, seed=11))
    res["ancestral100_seeded_graphs_cached"] = stats()
    res["ancestral100_default_ms"] = timed(lambda: d(cond, src_spec=src, infer=True))
    res["ancestral100_default_graphs_cached"] = stats()
    d.denoise_fn.release_native()
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
