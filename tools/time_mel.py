#!/usr/bin/env python3
"""Mel analysis timings: dsd_mel_analyze at the production configuration (44.1 kHz, 2048 / 2048 /
512, 128 mels, 40-16000 Hz) on one 60-s clip at keyshift 0 and 3 (the basis of each size is built once, at warm-up), a
ragged batch of 16 clips of 2-20 s against 16 lone calls, the same mels through a torch-on-GPU restatement (reflect pad,
torch.stft, abs, matmul, clamp, log), and dsd_vocode of the 60-s mel for the cost ratio.  Device-event times, warm-up,
median of several repeats; GPU box only.  Prints one JSON line; `--out FILE` also writes it there."""
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

import mel_ref  # noqa: E402
from diffsinger_amd import synth  # noqa: E402
from diffsinger_amd.mel import STFT, mel_filterbank  # noqa: E402
from diffsinger_amd.vocoder import Generator  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out")
args = ap.parse_args()
assert torch.cuda.is_available(), "time_mel.py needs the MI355X"


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


c = mel_ref.PROD
stft = STFT(c["sr"], c["n_mels"], c["n_fft"], c["win_size"], c["hop"], c["fmin"], c["fmax"])
basis = torch.from_numpy(mel_filterbank(c["sr"], c["n_fft"], c["n_mels"], c["fmin"], c["fmax"])).cuda()


def torch_mel(y, keyshift=0, speed=1):
    """nvSTFT.py:50-87 on torch's GPU ops (the path a user of the reference runs)."""
    n, w, h, pl, pr = mel_ref.geometry(c["n_fft"], c["win_size"], c["hop"], keyshift, speed)
    yp = F.pad(y.unsqueeze(1), (pl, pr), mode="reflect").squeeze(1)
    spec = torch.stft(yp, n, hop_length=h, win_length=w, window=torch.hann_window(w, device=y.device), center=False,
                      normalized=False, onesided=True, return_complex=True).abs()
    if keyshift != 0:
        size = c["n_fft"] // 2 + 1
        if spec.size(1) < size:
            spec = F.pad(spec, (0, 0, 0, size - spec.size(1)))
        spec = spec[:, :size, :] * c["win_size"] / w
    return torch.log(torch.clamp(torch.matmul(basis, spec), min=1e-5))


res = {"config": "44.1 kHz, n_fft 2048, win 2048, hop 512, 128 mels"}
with torch.no_grad():
    y60 = torch.from_numpy(mel_ref.waveform(60, 60 * c["sr"], c["sr"])).cuda()[None]
    t60 = stft.num_frames(y60.shape[1])
    res["frames_60s"] = t60
    for ks in (0, 3):
        ms = timed(lambda: stft.get_mel(y60, keyshift=ks))
        mt = timed(lambda: torch_mel(y60, keyshift=ks))
        a, b = stft.get_mel(y60, keyshift=ks), torch_mel(y60, keyshift=ks)
        res[f"clip60_ks{ks}_ms"] = ms
        res[f"clip60_ks{ks}_ms_per_1000_frames"] = ms * 1000 / t60
        res[f"clip60_ks{ks}_torch_ms"] = mt
        res[f"clip60_ks{ks}_hip_vs_torch_max_abs_log"] = float((a - b).abs().max())
    rng = np.random.default_rng(16)
    lens = [int(s * c["sr"]) for s in rng.uniform(2, 20, 16)]
    waves = [torch.from_numpy(mel_ref.waveform(200 + i, n, c["sr"])).cuda() for i, n in enumerate(lens)]
    frames = sum(stft.num_frames(n) for n in lens)
    res["ragged16_seconds"] = round(sum(lens) / c["sr"], 2)
    res["ragged16_frames"] = frames
    res["ragged16_one_call_ms"] = timed(lambda: stft.get_mel_ragged(waves))
    res["ragged16_lone_calls_ms"] = timed(lambda: [stft.get_mel(w[None]) for w in waves])
    res["ragged16_torch_lone_calls_ms"] = timed(lambda: [torch_mel(w[None]) for w in waves])
    # the vocoder on the 60-s mel: the cost the analysis is compared with
    h = dict(synth.NSF_HIFIGAN_DEFAULT)
    gen = Generator(h)
    gen.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(
        synth.nsf_hifigan_param_shapes(h), seed=45, gain=0.7).items()}, strict=True)
    gen = gen.cuda().eval()
    mel = stft.get_mel(y60)
    f0 = torch.full((1, t60), 220.0, device="cuda")
    rand_ini = torch.rand(9, device="cuda")
    noise = torch.randn(1, t60 * gen.upp, 9, device="cuda")
    mv = timed(lambda: gen(mel, f0, rand_ini=rand_ini, noise=noise))
    res["vocode60_ms"] = mv
    res["vocode_ms_per_1000_frames"] = mv * 1000 / t60
    res["analysis_over_vocode_ks0"] = res["clip60_ks0_ms"] / mv
    res["analysis_over_vocode_ks3"] = res["clip60_ks3_ms"] / mv
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
