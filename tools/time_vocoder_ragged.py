#!/usr/bin/env python3
"""Several segments through the NSF-HiFiGAN vocoder (the default 44.1 kHz / hop 512 / 512-channel layout, synthetic
weights): one call per segment (what the reference does) against ONE ragged call (dsd_vocode_ragged) and against one dense
call over the padded batch (wrong near the short items' ends: the cost of padding, not an option).  Device-event times,
warm-up, median of several repeats; GPU box only.  `--trace MIX` runs that mix's ragged call once and then its dense padded call
once, nothing else (for a rocprofv3 kernel trace)."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from diffsinger_amd import synth  # noqa: E402
from diffsinger_amd.vocoder import Generator  # noqa: E402

rng = np.random.Generator(np.random.PCG64(5))
MIXES = {
    "a": ("8 segments of 480-1000 frames", [1000, 930, 850, 760, 700, 640, 560, 480]),
    "b": ("16 segments of 120-400 frames", sorted((int(v) for v in rng.integers(120, 401, 16)), reverse=True)),
    "c": ("one of 4000 frames + seven of 300", [4000] + [300] * 7),
}

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--trace", choices=sorted(MIXES))
args = ap.parse_args()

h = dict(synth.NSF_HIFIGAN_DEFAULT)
gen = Generator(h)
gen.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(
    synth.nsf_hifigan_param_shapes(h), seed=45, gain=0.7).items()}, strict=True)
gen = gen.cuda().eval()
upp, dim, c0 = gen.upp, gen.harmonic_num + 1, gen.upsample_initial_channel


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


with torch.no_grad():
    for key, (what, lens) in MIXES.items():
        if args.trace and key != args.trace:
            continue
        n, t_max = len(lens), max(lens)
        mel = torch.from_numpy(synth.synth_normal((n, 128, t_max), 1) * 1.5 - 5.0).float().cuda()
        f0 = torch.from_numpy((180.0 * 2.0 ** rng.uniform(-1, 1, (n, t_max))).astype(np.float32)).cuda()
        rand_ini = torch.rand((n, dim), device="cuda")
        noise = torch.randn((n, t_max * upp, dim), device="cuda")
        singles = [(mel[i:i + 1, :, :t].contiguous(), f0[i:i + 1, :t].contiguous(), rand_ini[i],
                    noise[i:i + 1, :t * upp].contiguous()) for i, t in enumerate(lens)]

        def one_by_one():
            return [gen(m, f, rand_ini=r, noise=z) for m, f, r, z in singles]

        def ragged():
            return gen(mel, f0, lengths=lens, rand_ini=rand_ini, noise=noise)

        def dense():
            return gen(mel, f0, rand_ini=rand_ini[0], noise=noise)

        if args.trace:
            ragged()
            torch.cuda.synchronize()
            dense()
            torch.cuda.synchronize()
            print(f"mix ({key}) {what}: one ragged call, then one dense padded call")
            continue
        a, b = one_by_one(), ragged()
        worst = max(float((x[0, 0] - b[i, 0, :t * upp]).abs().max()) for i, (x, t) in enumerate(zip(a, lens)))
        res = {"one by one": timed(one_by_one), "ragged": timed(ragged), "dense padded": timed(dense)}
        print(f"mix ({key}) {what}: {sum(lens)} frames, padded {n} x {t_max} = {n * t_max}; max |ragged - alone| {worst:.2e}")
        for name, ms in res.items():
            print(f"  {name:13s} {ms:8.2f} ms  {sum(lens) / ms:8.1f} frames/ms")
        print(f"  ragged vs one by one {res['one by one'] / res['ragged']:.2f}x, vs dense padded "
              f"{res['dense padded'] / res['ragged']:.2f}x", flush=True)
