#!/usr/bin/env python3
"""VR harmonic-noise separation timings: dsd_hnsep_separate with the production layout (n_fft 2048,
hop 512, nout 32, nout_lstm 128, mono) on synthetic weights, one 10-s and one 60-s 44.1-kHz clip at B = 1, a ragged batch
of 16 clips of 2-12 s against 16 lone calls, the base harmonic and the four curves of a 10-s clip, and the same weights
in the torch mirror (diffsinger_amd.hnsep.CascadedNet: nn.Conv2d / MIOpen, nn.LSTM, torch.stft) on the same GPU.
Device-event times, warm-up, median of several repeats; GPU box only.  Prints one JSON line; `--out FILE` also writes it.

The per-kernel split (STFT / iSTFT, convs, LSTM, curves) and the convs' fraction of the fp32 MFMA peak come from a
rocprofv3 --kernel-trace --stats run of `--quick` (one 10-s separation): pass its kernel_stats.csv, or the rocpd database
(results.db) rocprofv3 writes by default, with `--stats FILE`; this step needs no GPU."""
import argparse
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mel_ref  # noqa: E402
from diffsinger_amd import hnsep, synth  # noqa: E402

SR = 44100
PEAK_F32_MFMA = 157.3e12            # MI355X fp32 matrix peak (spec), FLOP/s

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--quick", action="store_true", help="one 10-s separation (for a profiler run)")
ap.add_argument("--stats", help="rocprofv3 kernel_stats.csv or results.db of a --quick run: per-kernel split and conv "
                                "MFMA fraction")
ap.add_argument("--out")
args = ap.parse_args()

cfg = dict(synth.HNSEP_PROD)
sd = synth.hnsep_state_dict(cfg, 1902)


def conv_macs(n_samples):
    """MACs of every Conv2d of the mirror on one clip (forward hooks, shapes only: the model on the meta device)."""
    m = hnsep.CascadedNet(**cfg).to("meta")
    total = [0]

    def hook(mod, inp, out):
        if isinstance(mod, torch.nn.Conv2d):
            total[0] += out.numel() * mod.in_channels * mod.kernel_size[0] * mod.kernel_size[1]
    for mod in m.modules():
        mod.register_forward_hook(hook)
    _, _, frames = hnsep.padding(n_samples, cfg["hop_length"])
    with torch.no_grad():
        m(torch.zeros(1, 1, cfg["n_fft"] // 2 + 1, frames, dtype=torch.complex64, device="meta"))
    return total[0]


if args.stats:
    groups = {"stft / istft / overlap-add": ("hs_dft", "hs_ola", "hs_basis"), "convs": ("hs_conv",), "lstm": ("hs_lstm",),
              "mask / bin mean": ("hs_mask", "hs_binmean"), "curves": ("hs_rms", "hs_curves")}
    split = {k: 0.0 for k in groups}
    rows = []                               # (kernel name, total ms)
    if args.stats.endswith(".db"):
        import sqlite3
        with sqlite3.connect(args.stats) as db:
            rows = [(n, us / 1e3) for n, us in db.execute("select name, total_duration from top_kernels")]
    else:
        with open(args.stats) as f:
            rows = [(r.get("Name") or r.get("KernelName") or "", float(r.get("TotalDurationNs") or 0) / 1e6)
                    for r in csv.DictReader(f)]
    for name, ms in rows:
        for k, pre in groups.items():
            if any(p in name for p in pre):
                split[k] += ms
    macs = conv_macs(10 * SR)
    res = {"split_ms_10s": split, "conv_gmac_10s": macs / 1e9,
           "conv_fraction_of_fp32_mfma_peak": 2 * macs / (split["convs"] / 1e3) / PEAK_F32_MFMA if split["convs"] else None}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res) + "\n")
    sys.exit(0)

assert torch.cuda.is_available(), "time_hnsep.py needs the MI355X"
dev = torch.device("cuda")
sep = hnsep.HnSep(sd, cfg)
if args.quick:
    x = mel_ref.waveform(5, 10 * SR, SR).astype(np.float32)
    sep.separate_ragged([x])
    torch.cuda.synchronize()
    sys.exit(0)


def timed(fn):
    for _ in range(args.warmup):
        fn()
    ts = []
    for _ in range(args.repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


res = {"layout": cfg}
clips = {s: torch.from_numpy(mel_ref.waveform(10 + s, s * SR, SR).astype(np.float32)).to(dev) for s in (10, 60)}
for s, x in clips.items():
    res[f"separate_{s}s_ms"] = timed(lambda: sep.separate_ragged([x]))
rng = np.random.default_rng(7)
rag = [torch.from_numpy(mel_ref.waveform(100 + i, int(rng.uniform(2, 12) * SR), SR).astype(np.float32)).to(dev) for i in range(16)]
res["ragged16_total_s"] = sum(len(v) for v in rag) / SR
res["ragged16_one_call_ms"] = timed(lambda: sep.separate_ragged(rag))
res["ragged16_lone_calls_ms"] = timed(lambda: [sep.separate_ragged([v]) for v in rag])
x10 = clips[10]
h10 = sep.separate_ragged([x10])[0]
f0 = np.full(10 * SR // 512 + 1, 220.0)
res["base_harmonic_10s_ms"] = timed(lambda: sep.base_harmonic_ragged([h10], [f0], SR, 512, 2048))
b10 = sep.base_harmonic_ragged([h10], [f0], SR, 512, 2048)[0]
res["curves_10s_ms"] = timed(lambda: sep.curves_ragged([x10], [h10], [b10], [len(f0)], 512, 2048))
mirror = hnsep.CascadedNet(**cfg)
mirror.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
mirror = mirror.to(dev).eval()
with torch.no_grad():
    for s, x in clips.items():
        res[f"torch_mirror_{s}s_ms"] = timed(lambda: mirror.predict_from_audio(x[None, None]))
res["conv_gmac_10s"] = conv_macs(10 * SR) / 1e9
print(json.dumps(res))
if args.out:
    with open(args.out, "w") as f:
        f.write(json.dumps(res) + "\n")
