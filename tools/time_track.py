#!/usr/bin/env python3
"""The track of a project assembled on the host (the default) and on the device (`run_inference(device_mix=True)`), in
one process on the 8-segment project of tools/time_project.py: wall time of the whole `run_inference`, median of 7 after
a warm-up that has captured the graphs, at batch_size 1 and 8, with an output file (int16 through `save_wav` / through
the PCM export) and without; and the device time of the track's own launches - place x 8, then peak + PCM export - between
events on the stream, median of 7."""
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from diffsinger_amd import track  # noqa: E402
from diffsinger_amd.hparams import hparams  # noqa: E402
from time_project import build_project  # noqa: E402

RUNS = 7


def wall(fn):
    times = []
    for _ in range(RUNS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return statistics.median(times) * 1e3


def main():
    h, segs, seconds = build_project()
    with tempfile.TemporaryDirectory() as tmp:
        for bs in (1, 8):
            for mix in (False, True):                               # warm-up: every graph of this batch size is captured
                for _ in range(2):
                    h.run_inference(segs, batch_size=bs, device_noise=True, seed=1, device_mix=mix)
            for out in (None, os.path.join(tmp, "t.wav")):
                ms = {mix: wall(lambda: h.run_inference(segs, batch_size=bs, device_noise=True, seed=1, device_mix=mix, out_path=out))
                      for mix in (False, True)}
                print(f"batch_size={bs} {'with a .wav' if out else 'no file   '}: host mix {ms[False]:8.2f} ms, device mix {ms[True]:8.2f} ms "
                      f"({ms[True] - ms[False]:+.2f} ms) for {seconds:.1f} s of audio in {len(segs)} segments", flush=True)

    # the track's own launches on segments of the project's lengths
    sr, hop = hparams["audio_sample_rate"], hparams["hop_size"]
    lengths = [int(h.preprocess_input(s, idx=i)["mel2ph"].size(1)) * hop for i, s in enumerate(segs)]
    layout = track.plan([s["offset"] for s in segs], lengths, sr)
    wavs = [torch.rand(n, device="cuda") - 0.5 for n in lengths]
    t = track.Track(layout.total, "cuda", layout)
    pcm = torch.empty(layout.total, dtype=torch.int16, device="cuda")
    place_ms, export_ms = [], []
    for _ in range(RUNS + 2):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        for k, w in enumerate(wavs):
            t.place(k, w)
        ev[1].record()
        t.export("pcm", norm=True, out=pcm)
        ev[2].record()
        torch.cuda.synchronize()
        place_ms.append(ev[0].elapsed_time(ev[1]))
        export_ms.append(ev[1].elapsed_time(ev[2]))
    place, export = statistics.median(place_ms[2:]), statistics.median(export_ms[2:])
    moved = sum(lengths) * 12 + (layout.total - sum(lengths)) * 8           # 4 in + 8 out per sample, 8 per gap sample
    print(f"track of {layout.total} samples ({layout.total / sr:.1f} s): place x {len(wavs)} {place * 1e3:.0f} us on the device "
          f"({moved / place / 1e6:.0f} GB/s over the launches and the gaps between them), peak + pcm export {export * 1e3:.0f} us", flush=True)


if __name__ == "__main__":
    main()
