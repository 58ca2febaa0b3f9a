#!/usr/bin/env python3
"""dsd_vocode_seeded against the path it replaces, in ONE process: the NSF-HiFiGAN vocoder at its production shape (default
44.1 kHz / hop 512 / 512-channel layout, 8 harmonics, synthetic weights; noise_sigma set above 0 so that all three draws are
made) on B = 8 segments of T = 1000 frames, one seed per segment.

  fill_then_vocode   three dsd_noise_fill calls (rand_ini [B, 9], noise [B, T * 512, 9], pre_noise [B, 512, T]) plus
                     dsd_vocode_ragged: Generator.forward(lengths=, seed=)
  seeded             dsd_vocode_seeded: Generator.forward_seeded

Device events around one call, 10 warm-up calls, the median of 50, the legs in the order seeded, fill_then_vocode, seeded
again (the two seeded legs bracket the other; their spread is the noise a ratio has to clear).  Device memory from
hipMemGetInfo (torch.cuda.mem_get_info) around the FIRST call of each path, the caching allocator emptied before: the seeded
path is called first and pays the handle's workspace, the other then adds only what it allocates beyond that - the draws.
Prints one JSON line.  GPU box only."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from diffsinger_amd import synth  # noqa: E402
from diffsinger_amd.vocoder import Generator  # noqa: E402

WARMUP, REPEATS = 10, 50
B, T = 8, 1000


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


def first_call_bytes(fn):
    """device memory taken by one call and still held after it (the allocator's cache keeps the call's peak)"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free0 = torch.cuda.mem_get_info()[0]
    out = fn()
    torch.cuda.synchronize()
    taken = free0 - torch.cuda.mem_get_info()[0]
    return out, taken


def main():
    h = dict(synth.NSF_HIFIGAN_DEFAULT, noise_sigma=0.05)
    gen = Generator(h)
    gen.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(
        synth.nsf_hifigan_param_shapes(h), seed=45, gain=0.7).items()}, strict=True)
    gen = gen.cuda().eval()
    rng = np.random.Generator(np.random.PCG64(5))
    lens, seeds = [T] * B, [1000 + b for b in range(B)]
    with torch.no_grad():
        mel = torch.from_numpy(synth.synth_normal((B, 128, T), 1) * 1.5 - 5.0).float().cuda()
        f0 = torch.from_numpy((180.0 * 2.0 ** rng.uniform(-1, 1, (B, T))).astype(np.float32)).cuda()
        gen.native_handle(mel.device)                   # weights on the device before any measurement

        def seeded():
            return gen.forward_seeded(mel, f0, seeds, lengths=lens)

        def fill_then_vocode():
            return gen(mel, f0, lengths=lens, seed=seeds)

        got, seeded_bytes = first_call_bytes(seeded)
        del got
        want, extra_bytes = first_call_bytes(fill_then_vocode)
        got = seeded()
        same = bool(torch.equal(got, want))
        out_bytes = want.numel() * 4
        del got, want
        a = timed(seeded)
        other = timed(fill_then_vocode)
        b = timed(seeded)
    spread = abs(a - b)
    draws = 4 * (B * gen.upp * T * (gen.harmonic_num + 1) + B * gen.upsample_initial_channel * T + B * (gen.harmonic_num + 1))
    print(json.dumps({"B": B, "T": T, "warmup": WARMUP, "repeats": REPEATS, "bit_identical": same,
                      "seeded_ms": round(a, 4), "fill_then_vocode_ms": round(other, 4), "seeded_again_ms": round(b, 4),
                      "seeded_spread_ms": round(spread, 4), "ratio": round(other / (0.5 * (a + b)), 4),
                      "seeded_faster": bool(other - max(a, b) > spread),
                      "seeded_first_call_bytes": int(seeded_bytes), "fill_then_vocode_extra_bytes": int(extra_bytes),
                      "output_bytes": int(out_bytes), "draw_tensor_bytes": int(draws)}), flush=True)


if __name__ == "__main__":
    main()
