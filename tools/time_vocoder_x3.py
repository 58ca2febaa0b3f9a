#!/usr/bin/env python3
"""The NSF-HiFiGAN vocoder (default 44.1 kHz / hop 512 / 512-channel layout, synthetic weights) in fp32 and in the split-bf16
mode (Generator.set_precision("bf16x3"), voc_x3.hip), in ONE process: one utterance of B = 1 / T = 1000 and the ragged mix (b)
of tools/time_vocoder_ragged.py (16 segments of 120-400 frames, one dsd_vocode_ragged call).  Each workload is measured fp32,
then bf16x3, then fp32 again - device events around one call, 10 warm-up calls, the median of 20 - so the two fp32 legs bracket
the bf16x3 one on the same device in the same minute; their spread is the noise the ratio has to clear.  Prints one JSON line:
per workload the three times (ms), ratio = mean of the fp32 legs / bf16x3, f32_spread = |leg 1 - leg 3|, faster = bf16x3 below
both fp32 legs by more than that spread, the max |bf16x3 - fp32| / max |fp32| of the outputs, and the mean time per launch of
the split-bf16 kernel classes of one call.  GPU box only."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from diffsinger_amd import synth  # noqa: E402
from diffsinger_amd.vocoder import Generator  # noqa: E402

WARMUP, REPEATS = 10, 20
rng = np.random.Generator(np.random.PCG64(5))
MIX_B = sorted((int(v) for v in rng.integers(120, 401, 16)), reverse=True)      # the draw of time_vocoder_ragged.py's mix (b)


def timed(fn):
    for _ in range(WARMUP):
        fn()
    times = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def main():
    h = dict(synth.NSF_HIFIGAN_DEFAULT)
    gen = Generator(h)
    gen.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(
        synth.nsf_hifigan_param_shapes(h), seed=45, gain=0.7).items()}, strict=True)
    gen = gen.cuda().eval()
    upp, dim = gen.upp, gen.harmonic_num + 1
    result = {"warmup": WARMUP, "repeats": REPEATS}
    with torch.no_grad():
        for name, lens in (("b1_t1000", None), ("ragged_16x120_400", MIX_B)):
            n, t_max = (1, 1000) if lens is None else (len(lens), max(lens))
            mel = torch.from_numpy(synth.synth_normal((n, 128, t_max), 1) * 1.5 - 5.0).float().cuda()
            f0 = torch.from_numpy((180.0 * 2.0 ** rng.uniform(-1, 1, (n, t_max))).astype(np.float32)).cuda()
            rand_ini = torch.rand((n, dim), device="cuda")
            noise = torch.randn((n, t_max * upp, dim), device="cuda")

            def call():
                if lens is None:
                    return gen(mel, f0, rand_ini=rand_ini[0], noise=noise)
                return gen(mel, f0, lengths=lens, rand_ini=rand_ini, noise=noise)

            gen.set_precision("f32")
            ref = call()
            f32_a = timed(call)
            gen.set_precision("bf16x3")
            out = call()
            assert gen.stats()["precision"] == 1, "no split-bf16 kernel ran"
            x3 = timed(call)
            gen.kernel_timing(True)
            call()
            torch.cuda.synchronize()
            classes = {c["name"]: {"mean_ms": round(c["mean_ms"], 4), "launches": c["launches"]} for c in gen.kernel_classes()
                       if c["name"].startswith("voc_conv_x3_kernel<")}
            gen.kernel_timing(False)
            gen.set_precision("f32")
            f32_b = timed(call)
            spread = abs(f32_a - f32_b)
            result[name] = {"frames": t_max if lens is None else sum(lens), "f32_ms": round(f32_a, 4), "bf16x3_ms": round(x3, 4),
                            "f32_again_ms": round(f32_b, 4), "ratio": round(0.5 * (f32_a + f32_b) / x3, 4),
                            "f32_spread_ms": round(spread, 4), "faster": bool(min(f32_a, f32_b) - x3 > spread),
                            "max_rel_diff": float((out - ref).abs().max() / ref.abs().max()), "x3_classes": classes}
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
