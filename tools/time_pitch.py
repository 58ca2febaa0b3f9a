#!/usr/bin/env python3
"""RMVPE pitch extraction timings: dsd_rmvpe_infer with the production E2E0(4, 1, (2, 2)) on
synthetic weights, one 10-s and one 60-s clip at B = 1 (16 kHz and 44.1 kHz input), a ragged batch of 16 clips of 2-12 s
against 16 lone calls, the network alone (dsd_rmvpe_mel_to_hidden) for the front end's share, and the same weights in the
torch restatement (diffsinger_amd.pitch.E2E0: nn.Conv2d / BatchNorm2d / nn.GRU) on the same GPU.  The Viterbi decode
(dsd_rmvpe_decode_viterbi) is timed alone on the hidden of the 10-s and 60-s clips and of the ragged batch, beside the
local-average decode (dsd_rmvpe_decode) and the numpy oracle of tests/viterbi_ref.py on the host.  The per-kernel split
(resample + mel / U-Net / GRU / decode) comes from a rocprofv3 --kernel-trace --stats run of `--quick`.  Device-event
times, warm-up, median of several repeats; GPU box only.  Prints one JSON line; `--out FILE` also writes it there."""
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

import ctypes as C  # noqa: E402
import time  # noqa: E402

import mel_ref  # noqa: E402
import viterbi_ref  # noqa: E402
from diffsinger_amd import _lib  # noqa: E402
from diffsinger_amd import synth  # noqa: E402
from diffsinger_amd.pitch import E2E0, RMVPE  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--quick", action="store_true", help="one 10-s call per path (for a profiler run)")
ap.add_argument("--out")
args = ap.parse_args()
assert torch.cuda.is_available(), "time_pitch.py needs the MI355X"
if args.quick:
    args.repeats, args.warmup = 1, 1

PROD = dict(n_blocks=4, n_gru=1, en_de_layers=5, inter_layers=4, en_out_channels=16)
# U-Net convolutions: ~69 MFLOP per 10-ms frame (torch.utils.flop_counter on the reference model); peak fp32 from
# MI355X_MICROARCH.md (157.3 TFLOP/s dense fp32, vector or MFMA)
UNET_FLOP_PER_FRAME, FP32_PEAK = 69e6, 157.3e12


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


def decode_times(hid, lengths, tag):
    """Decode alone on a device hidden [B, T, 360]: the Viterbi decode, the local-average decode, the numpy oracle."""
    b, t, _ = hid.shape
    f0 = torch.zeros(b, t, device="cuda")
    res[f"viterbi_decode_{tag}"] = timed(lambda: pe._viterbi(hid, lengths, 0.03, f0))
    res[f"local_decode_{tag}"] = timed(lambda: _lib.check(pe._h, _lib.lib().dsd_rmvpe_decode(
        pe._h, C.c_void_p(hid.data_ptr()), b, t, t * 360, 360, 0.03, C.c_void_p(f0.data_ptr()), t, pe._stream()), "decode"))
    host = hid.cpu().numpy()
    t0 = time.perf_counter()
    for i in range(b):
        viterbi_ref.to_viterbi_f0(host[i, : (t if lengths is None else lengths[i])])
    res[f"numpy_viterbi_{tag}"] = (time.perf_counter() - t0) * 1e3


sd = synth.rmvpe_state_dict(seed=1802, **PROD)
pe = RMVPE(sd)
res = {"config": "E2E0(4, 1, (2, 2)), synthetic weights"}
secs = [10] if args.quick else [10, 60]
for s in secs:
    for sr in (16000, 44100):
        y = mel_ref.waveform(1900 + s, s * sr, sr)
        wav = torch.from_numpy(y).cuda()[None]
        lens = [wav.shape[1]]
        ms = timed(lambda: pe._infer(wav, lens, sr, 0.03))
        res[f"infer_{s}s_{sr}"] = ms
        if sr == 16000:
            res[f"infer_viterbi_{s}s_{sr}"] = timed(lambda: pe._infer(wav, lens, sr, 0.03, use_viterbi=True))
            decode_times(pe._infer(wav, lens, sr, 0.03, want_hidden=True)[1], None, f"{s}s")
    frames = 1 + s * 100
    mel = torch.randn(1, 128, frames, device="cuda") - 4
    ms = timed(lambda: pe.mel2hidden(mel))
    res[f"mel2hidden_{s}s"] = ms
    res[f"unet_share_of_fp32_peak_{s}s_upper_bound"] = UNET_FLOP_PER_FRAME * frames / (ms * 1e-3) / FP32_PEAK
    net = E2E0(4, 1, (2, 2)).cuda().eval()
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items() if not k.startswith("unet.tf.")},
                        strict=False)
    tp = 32 * ((frames - 1) // 32 + 1)
    melp = torch.nn.functional.pad(mel, (0, tp - frames))
    with torch.no_grad():
        res[f"torch_mel2hidden_{s}s"] = timed(lambda: net(melp))
        feat = torch.randn(1, tp, 384, device="cuda")
        res[f"torch_gru_{s}s"] = timed(lambda: net.fc[0](feat))
        x = melp.transpose(-1, -2).unsqueeze(1)
        res[f"torch_unet_{s}s"] = timed(lambda: net.cnn(net.unet(x)))
if not args.quick:
    rng = np.random.default_rng(1950)
    clips = [mel_ref.waveform(1960 + k, int(rng.uniform(2, 12) * 16000), 16000) for k in range(16)]
    res["ragged16_s"] = sum(len(c) for c in clips) / 16000
    res["ragged16_ms"] = timed(lambda: pe.infer_from_audio_ragged(clips, 16000))
    res["lone16_ms"] = timed(lambda: [pe.infer_from_audio(c, 16000) for c in clips])
    res["ragged16_viterbi_ms"] = timed(lambda: pe.infer_from_audio_ragged(clips, 16000, use_viterbi=True))
    wav16 = torch.zeros(16, max(len(c) for c in clips), device="cuda")
    for i, c in enumerate(clips):
        wav16[i, : len(c)] = torch.from_numpy(c).cuda()
    _, hid16, frames16 = pe._infer(wav16, [len(c) for c in clips], 16000, 0.03, want_hidden=True)
    decode_times(hid16, frames16, "ragged16")
line = json.dumps(res)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
