"""Inputs, handles and the one call per family of the launch-ledger cases (tests/kernel_ledger_cases.py), shared by
tests/test_gpu_kernel_ledger.py (a case against the oracle) and tests/test_gpu_poison.py (a case against itself after the
workspace and the caller's padding were poisoned); tests/test_poison_cases_host.py vets the builders on the CPU.

Builders (numpy, name -> array; every input of these families is float32, an integer input would be left alone):
  clean(case)               the inputs test_gpu_kernel_ledger.py compares with the oracle, seeds included
  padded_with(case, value)  `value` in every per-frame float input past each item's end, the valid part bit-identical:
                            denoisers x[b, :, :, n:] and cond[b, :, n:]; aux decoder cond[b, n:]; vocoder mel[b, :, n:],
                            f0[b, n:], noise[b, n * upp:], pre_noise[b, :, n:]  (t and rand_ini have no frame axis)
  all_of(case, value)       every float input set to `value`, the diffusion step t and the initial phases included

Handles and calls need the GPU; they import torch and the library when called."""
from collections import namedtuple

import numpy as np

import kernel_ledger_cases as lc
import vocoder_config_cases as vcc
import vocoder_x3_cases as vx3
from diffsinger_amd import synth

# what a handle carries besides the module: the weights as numpy (the oracle's), and the aux adaptor's mel range
Handle = namedtuple("Handle", "kind net params smin smax upp")

# name -> (frame axis, elements per frame along it in units of `upp`: 0 = one per frame, 1 = upp per frame)
FRAME_AXES = {
    "wavenet": {"x": (3, 0), "cond": (2, 0)},
    "lynxnet": {"x": (3, 0), "cond": (2, 0)},
    "aux": {"cond": (1, 0)},
    "vocoder": {"mel": (2, 0), "f0": (1, 0), "noise": (1, 1), "pre_noise": (2, 0)},
}


def voc_module(which):
    return vcc if which == "configs" else vx3


def grid(case):
    """(B, T, lengths or None) of a case; the vocoder's "cases" are its module's shared ragged lengths"""
    if case.kind == "vocoder":
        which, _, bsz, t_len, lengths = case.spec
        if lengths == "cases":
            lengths = voc_module(which).RAGGED_LENGTHS
    else:
        _, bsz, t_len, lengths = case.spec
    return bsz, t_len, None if lengths is None else [int(n) for n in lengths]


def upp_of(case):
    """samples per frame of a vocoder case's output and noise (1 for the other families)"""
    if case.kind != "vocoder":
        return 1
    which, tag = case.spec[:2]
    return int(np.prod(voc_module(which).config(tag)["upsample_rates"]))


def handle_key(case):
    return case.spec[:2] if case.kind == "vocoder" else case.spec[0]


# ------------------------------------------------------------------------------------------------ inputs
def clean(case):
    bsz, t_len, _ = grid(case)
    if case.kind in ("wavenet", "lynxnet"):
        _, in_dims, n_feats, _, _ = lc.NETS[case.spec[0]]
        return dict(x=synth.synth_normal((bsz, n_feats, in_dims, t_len), 21), cond=synth.synth_normal((bsz, 256, t_len), 22),
                    t=((np.arange(bsz) * 173.25 + 7.5) % 1000.0).astype(np.float32))       # diffusion steps: [0, 1000)
    if case.kind == "aux":
        return dict(cond=synth.synth_normal((bsz, t_len, lc.AUX_NETS[case.spec[0]][0]), 900 + t_len))
    which, tag = case.spec[:2]
    return dict(voc_module(which).inputs(tag, bsz, t_len))        # (the module shares the arrays: never written in place)


def _is_float(a):
    return a.dtype.kind == "f"


def padded_with(case, value):
    _, t_len, lengths = grid(case)
    assert lengths is not None, case.id
    upp, out = upp_of(case), {k: v.copy() for k, v in clean(case).items()}
    for name, (axis, per_upp) in FRAME_AXES[case.kind].items():
        a = out[name]
        assert _is_float(a) and a.shape[axis] == t_len * (upp if per_upp else 1), (case.id, name, a.shape)
        for b, n in enumerate(lengths):
            idx = [slice(None)] * a.ndim
            idx[0], idx[axis] = b, slice(n * (upp if per_upp else 1), None)
            a[tuple(idx)] = value
    return out


def all_of(case, value):
    return {k: np.full_like(v, value) if _is_float(v) else v.copy() for k, v in clean(case).items()}


def valid(case, out, b, n):
    """item b's n valid frames of a call's output (tensor or array)"""
    if case.kind == "aux":
        return out[b, :n]
    return out[b, ..., :n * upp_of(case)]


# ------------------------------------------------------------------------------------------------ handles
def aux_range(m):
    rng = np.random.Generator(np.random.PCG64(5))
    return (-12.0 + rng.random(m)).astype(np.float32), rng.random(m).astype(np.float32)


def make_handle(case):
    """a new handle of the case's network with its synthetic weights (shared by every case with the same handle_key)"""
    import torch
    if case.kind in ("wavenet", "lynxnet"):
        from gpu_util import make_backbone
        kind, in_dims, n_feats, args, seed = lc.NETS[case.spec[0]]
        net, params = make_backbone(kind, in_dims, n_feats, args, seed)
        return Handle(case.kind, net, params, None, None, 1)
    if case.kind == "aux":
        from test_gpu_aux_decoder import make_adaptor
        hsz, m, c, nl, ks, wseed = lc.AUX_NETS[case.spec[0]]
        smin, smax = aux_range(m)
        a, params = make_adaptor(hsz, m, c, nl, ks, wseed, smin, smax)
        return Handle("aux", a, params, smin, smax, 1)
    from diffsinger_amd.vocoder import Generator
    which, tag = case.spec[:2]
    module = voc_module(which)
    g = Generator(module.config(tag))
    g.load_state_dict({k: torch.from_numpy(v) for k, v in module.weights(tag).items()}, strict=True)
    return Handle("vocoder", g.cuda().eval(), None, None, None, upp_of(case))


def release(handle):
    getattr(handle.net, "decoder", handle.net).release_native()


def set_precision(handle, precision):
    """the aux decoder has no split-bf16 path and no switch"""
    if handle.kind != "aux":
        handle.net.set_precision(precision)


# ------------------------------------------------------------------------------------------------ one call of each family
def call(handle, inputs, lengths=None, reset=None):
    """one call of the family on `inputs` (a builder's dict), ragged with `lengths`; `reset` runs after the lengths are set and the
    device is idle, right before the call (the ledger's zeroing) -> the output on the device, the stream synchronised"""
    import torch
    from gpu_util import dev
    reset = reset or (lambda: None)
    net = handle.net
    with torch.no_grad():
        if handle.kind == "aux":
            cd = dev(inputs["cond"])
            torch.cuda.synchronize()
            reset()
            out = net(cd, infer=True, lengths=lengths)
        elif handle.kind == "vocoder":
            i = {k: dev(v) for k, v in inputs.items()}
            if lengths is not None:         # one row of phases per item
                i["rand_ini"] = i["rand_ini"][None].repeat(len(lengths), 1)
            torch.cuda.synchronize()
            reset()
            out = net(i["mel"], i["f0"], lengths=lengths, rand_ini=i["rand_ini"], noise=i["noise"], pre_noise=i["pre_noise"])
        else:
            xd, td, cd = dev(inputs["x"]), dev(inputs["t"]), dev(inputs["cond"])
            try:
                net.set_lengths(lengths, xd.device)
                torch.cuda.synchronize()
                reset()
                out = net(xd, td, cd)
            finally:
                net.set_lengths(None, xd.device)
    torch.cuda.synchronize()
    return out
