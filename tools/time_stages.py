#!/usr/bin/env python3
"""Timing of the pitch pre-process stage: `DiffSingerVarianceDeploy.forward_pitch_preprocess` at
B = 1, T = 1000 (no melody encoder, so the stage is the duration-to-frame work and one assembly) against the same stage
written with the torch ops the `.ds` harness uses for it today on the same GPU - the searchsorted length regulator (which reads
the frame total back), gather, replicate pad + conv1d, the retake blend, embedding lookups and broadcast adds.  Both are expected to be bound by
launches, not by arithmetic.  Device-event times, warm-up, median of several repeats; GPU box only.  Prints one JSON line;
`--out FILE` also writes it there."""
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
import torch.nn.functional as F  # noqa: E402

import deploy_cases as dc  # noqa: E402
from diffsinger_amd import deploy  # noqa: E402
from diffsinger_amd.harness import length_regulator  # noqa: E402
from diffsinger_amd.hparams import hparams  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=50)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--frames", type=int, default=1000)
ap.add_argument("--out")
args = ap.parse_args()
assert torch.cuda.is_available(), "time_stages.py needs the MI355X"


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


hp = dict(dc.BASE_HP)
hp.update(dc.VARIANCE_HP, hidden_size=256, predict_pitch=True, diffusion_type="reflow")
hparams.clear()
hparams.update(hp, infer=True)
model = deploy.DiffSingerVarianceDeploy(40).cuda().eval()
model.build_smooth_op()
rng = np.random.default_rng(2295)
t_len, n_ph, n_note, h = args.frames, 60, 40, 256
ph_dur = torch.from_numpy(rng.multinomial(t_len, np.ones(n_ph) / n_ph)[None]).cuda()
note_dur = torch.from_numpy(rng.multinomial(t_len, np.ones(n_note) / n_note)[None]).cuda()
note_midi = torch.from_numpy(rng.uniform(48, 72, (1, n_note)).astype(np.float32)).cuda()
enc = torch.randn(1, n_ph, h, device="cuda")
pitch = torch.from_numpy((60 + rng.normal(0, 3, (1, t_len))).astype(np.float32)).cuda()
expr = torch.rand(1, t_len, device="cuda")
retake = torch.zeros(1, t_len, dtype=torch.bool, device="cuda")
retake[:, t_len // 3: 2 * t_len // 3] = True
taps = model.smooth[1].cuda()


def staged():
    return model.forward_pitch_preprocess(enc, ph_dur, note_midi=note_midi, note_dur=note_dur, pitch=pitch, expr=expr, retake=retake)


def torch_ops():
    mel2ph, mel2note = length_regulator(ph_dur), length_regulator(note_dur)
    cond = torch.gather(F.pad(enc, [0, 0, 1, 0]), 1, mel2ph[..., None].expand(-1, -1, h))
    e = (expr * retake)[:, :, None]
    cond = cond + e * model.pitch_retake_embed.weight[1] + (1. - e) * model.pitch_retake_embed.weight[0]
    frame_midi = torch.gather(F.pad(note_midi, [1, 0]), 1, mel2note)
    k = taps.numel()
    left = (k - 1) // 2
    base = F.conv1d(F.pad(frame_midi[:, None, :], [left, k - 1 - left], mode='replicate'), taps[None, None])[:, 0]
    base = base * retake + pitch * ~retake
    return cond + model.base_pitch_embed(base[:, :, None]), base


with torch.no_grad():
    a, b = staged(), torch_ops()
    res = {"B": 1, "T": t_len, "tokens": n_ph, "notes": n_note, "K": int(taps.numel()),
           "cond_max_abs_diff": float((a[0] - b[0]).abs().max()), "base_max_abs_diff": float((a[1] - b[1]).abs().max()),
           "staged_ms": timed(staged), "torch_ops_ms": timed(torch_ops),
           "length_regulate_ms": timed(lambda: deploy.length_regulate(ph_dur, t_len)),
           "torch_length_regulator_ms": timed(lambda: length_regulator(ph_dur)),
           "frame_curve_ms": timed(lambda: deploy.frame_curve(note_midi, deploy.length_regulate(note_dur, t_len), pitch, retake,
                                                              model.smooth[1]))}
line = json.dumps(res)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
