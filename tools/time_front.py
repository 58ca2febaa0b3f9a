"""What the segment front end costs: `AcousticHarness.preprocess_input` on the host path (np.interp per curve, one upload
per tensor, the cumsum / round / diff and the length regulator's read-back) against `device_front=True` (front.py: one
upload, dsd_length_regulate, one dsd_curve_resample), per segment and over a project, and the same for the variance
harness's `load_dur` / `load_pitch` inputs.  No model runs: the front end needs none.  Nothing is asserted; one JSON line.

    python tools/time_front.py [--segments 8] [--seconds 11.6] [--repeat 30]

Every timing is wall-clock around the call with a device synchronisation on both sides, the median of `--repeat` runs
after 5 warm-up runs.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffsinger_amd import harness, variance_harness  # noqa: E402
from diffsinger_amd.hparams import hparams  # noqa: E402

HOP = 512 / 44100
PHONES = ["a", "b", "c", "d", "e"]


def make_segment(rng, seconds):
    n_ph = max(2, int(seconds / 0.18))
    dur = rng.uniform(0.05, 0.3, n_ph)
    dur *= seconds / dur.sum()
    total = float(dur.sum())
    text = lambda v, digits: " ".join(str(x) for x in np.round(v, digits))     # noqa: E731
    n_f0 = int(total / 0.005) + 1
    f0 = 220.0 * 2.0 ** rng.uniform(-0.5, 0.5, n_f0)
    f0[rng.random(n_f0) < 0.1] = 0.0
    n_note = max(1, n_ph // 2)
    note_dur = rng.uniform(0.1, 0.6, n_note)
    note_dur *= total / note_dur.sum()
    return {"offset": 0.0, "ph_seq": " ".join(PHONES[int(k)] for k in rng.integers(0, 5, n_ph)), "ph_dur": text(dur, 6),
            "ph_num": " ".join(["2"] * (n_ph // 2) + (["1"] if n_ph % 2 else [])),
            "note_seq": " ".join(["C4", "D4", "E4", "rest"][int(k)] for k in rng.integers(0, 4, n_note)), "note_dur": text(note_dur, 6),
            "note_slur": " ".join(["0"] * n_note),
            "f0_seq": text(f0, 1), "f0_timestep": "0.005",
            "energy": text(rng.uniform(-60, -10, n_f0 // 2), 2), "energy_timestep": "0.01",
            "breathiness": text(rng.uniform(-70, -20, n_f0 // 2), 2), "breathiness_timestep": "0.01",
            "gender": text(rng.uniform(-1, 1, 64), 3), "gender_timestep": str(total / 63),
            "velocity": text(rng.uniform(0.4, 2.2, 64), 3), "velocity_timestep": str(total / 63)}


def timed(fn, repeat):
    for _ in range(5):
        fn()
    ms = []
    for _ in range(repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ms), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=11.6)
    ap.add_argument("--repeat", type=int, default=30)
    args = ap.parse_args()
    rng = np.random.Generator(np.random.PCG64(2750))
    segs = [make_segment(rng, args.seconds * (0.6 + 0.8 * k / max(1, args.segments - 1))) for k in range(args.segments)]
    one = make_segment(rng, args.seconds)
    out = {"segments": args.segments, "seconds": args.seconds, "repeat": args.repeat}

    hparams.clear()
    hparams.update(hop_size=512, audio_sample_rate=44100, use_spk_id=False, use_lang_id=False, use_energy_embed=True,
                   use_breathiness_embed=True, use_key_shift_embed=True, use_speed_embed=True,
                   augmentation_args=dict(random_pitch_shifting=dict(range=[-5.0, 5.0]),
                                          random_time_stretching=dict(range=[0.5, 2.0])))
    h = harness.AcousticHarness(None, None, harness.SimplePhonemeTable(PHONES), device="cuda")
    out["frames"] = int(h.preprocess_input(one)["mel2ph"].size(1))
    out["acoustic_segment_host_ms"] = timed(lambda: h.preprocess_input(one), args.repeat)
    out["acoustic_segment_front_ms"] = timed(lambda: h.preprocess_input(one, device_front=True), args.repeat)
    out["acoustic_project_host_ms"] = timed(lambda: [h.preprocess_input(s) for s in segs], args.repeat)
    out["acoustic_project_front_ms"] = timed(lambda: [h.preprocess_input(s, device_front=True) for s in segs], args.repeat)
    out["acoustic_project_front_group_ms"] = timed(lambda: h.preprocess_group(segs), args.repeat)

    class Flags:            # what the variance harness reads of its model before the forward pass
        predict_dur = predict_pitch = predict_variances = True
        variance_prediction_list = ["energy", "breathiness"]

    hparams.clear()
    hparams.update(hop_size=512, audio_sample_rate=44100, midi_smooth_width=0.06, use_spk_id=False, use_lang_id=False,
                   predict_dur=True, predict_pitch=True, use_glide_embed=False)
    v = variance_harness.VarianceHarness(Flags(), harness.SimplePhonemeTable(PHONES), device="cuda")
    kw = dict(load_dur=True, load_pitch=True)
    out["variance_segment_host_ms"] = timed(lambda: v.preprocess_input(one, **kw), args.repeat)
    out["variance_segment_front_ms"] = timed(lambda: v.preprocess_input(one, device_front=True, **kw), args.repeat)
    out["variance_project_host_ms"] = timed(lambda: [v.preprocess_input(s, **kw) for s in segs], args.repeat)
    out["variance_project_front_ms"] = timed(lambda: [v.preprocess_input(s, device_front=True, **kw) for s in segs], args.repeat)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
