"""Layouts, sizes and inputs shared by the split-bf16 vocoder tests (test_vocoder_x3_host.py on the CPU, test_gpu_vocoder_x3.py
on the GPU) and tools/bf16x3_vocoder_tolerance.py: synthetic weights (seed 410, gain 0.7) and the inputs of
test_gpu_vocoder.py::test_vocoder_vs_oracle_sizes; every fp32 oracle result is computed once per process and shared."""
import functools

import numpy as np

from diffsinger_amd import synth
from oracle import vocoder as ov

WSEED, GAIN = 410, 0.7
_A = dict(num_mels=32, upsample_rates=[4, 2, 2], upsample_kernel_sizes=[8, 4, 4], upsample_initial_channel=512, hop_size=16)
LAYOUTS = {
    "default": dict(),                                                       # 256 / 128 / 64 on voc_x3.hip, 32 / 16 on tconv.hip
    "A": dict(_A),                                                           # 256 / 128 / 64, ResBlock1, k 3 / 7 / 11, d 1 / 3 / 5
    "B": dict(_A, resblock="2", resblock_kernel_sizes=[3, 9], resblock_dilation_sizes=[[1, 2], [12, 6]]),    # reach 48
    "A_mini_sigma": dict(_A, mini_nsf=True, noise_sigma=0.2),
    "F": dict(_A, upsample_initial_channel=192),                             # 96 on voc_x3.hip (zero row blocks), 48 / 24 fp32
    "small": dict(_A, upsample_initial_channel=64, resblock="2", resblock_kernel_sizes=[3, 5],
                  resblock_dilation_sizes=[[1, 2], [2, 6]]),                 # 32 / 16 / 8: nothing for voc_x3.hip
}
PARITY = [("A", 1, 1), ("A", 1, 33), ("A", 3, 130), ("B", 2, 70), ("default", 1, 33), ("A_mini_sigma", 1, 5), ("F", 1, 33)]
RAGGED_LAYOUT, RAGGED_T, RAGGED_LENGTHS = "A", 130, [130, 1, 33, 64]


def config(layout):
    h = dict(synth.NSF_HIFIGAN_DEFAULT)
    h.update(LAYOUTS[layout])
    return h


@functools.lru_cache(maxsize=None)
def weights(layout):
    return synth.synth_state_dict(synth.nsf_hifigan_param_shapes(config(layout)), seed=WSEED, gain=GAIN)


@functools.lru_cache(maxsize=None)
def inputs(layout, bsz, t_len):
    """-> dict(mel [B, M, T] ln-mel, f0 [B, T], rand_ini [9], noise [B, T upp, 9], pre_noise [B, C0, T])"""
    h = config(layout)
    upp = int(np.prod(h["upsample_rates"]))
    rng = np.random.Generator(np.random.PCG64(t_len))
    mel = (synth.synth_normal((bsz, h["num_mels"], t_len), 411) * 3.0 - 11.0).astype(np.float32)
    f0 = (150.0 * 2.0 ** rng.uniform(-1, 2, (bsz, t_len))).astype(np.float32)
    f0[:, ::7] = 0.0
    return dict(mel=mel, f0=f0, rand_ini=rng.random(9).astype(np.float32), noise=synth.synth_normal((bsz, t_len * upp, 9), 412),
                pre_noise=synth.synth_normal((bsz, h["upsample_initial_channel"], t_len), 413))


def item_inputs(layout, bsz, t_len, b, n):
    """item b of inputs(layout, bsz, t_len) alone, cut to its first n frames (what a ragged call computes for it)"""
    i = inputs(layout, bsz, t_len)
    upp = int(np.prod(config(layout)["upsample_rates"]))
    return dict(mel=i["mel"][b:b + 1, :, :n], f0=i["f0"][b:b + 1, :n], rand_ini=i["rand_ini"], noise=i["noise"][b:b + 1, :n * upp],
                pre_noise=i["pre_noise"][b:b + 1, :, :n])


def oracle(layout, i):
    return ov.generator_forward(weights(layout), config(layout), i["mel"], i["f0"], i["rand_ini"], i["noise"], i["pre_noise"])


@functools.lru_cache(maxsize=None)
def reference(layout, bsz, t_len):
    """the fp32 oracle's waveform of a dense case (read-only: shared by the tests of a process)"""
    want = oracle(layout, inputs(layout, bsz, t_len))
    want.setflags(write=False)
    return want


@functools.lru_cache(maxsize=None)
def ragged_reference(b):
    want = oracle(RAGGED_LAYOUT, item_inputs(RAGGED_LAYOUT, len(RAGGED_LENGTHS), RAGGED_T, b, RAGGED_LENGTHS[b]))
    want.setflags(write=False)
    return want
