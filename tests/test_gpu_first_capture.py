"""A kernel form whose FIRST launch in the process happens under stream capture.

Every hand-written kernel needs its dynamic-LDS limit raised before its first launch, and that call is not allowed inside a
capture; dsd_sample captures hipGraphs.  The create functions raise the limits of every kernel their family can launch
(dsd_internal.h, KernelReg; api.hip, prepare_kernels), so a capture may be the first thing that launches a form.  The rest of
the suite cannot show that: it runs in one process, where an eager test of the same kernels has always come first.

So this test starts fresh child processes (this file run as a script), one per backbone, one after the other.  A child builds
one handle and walks a list of forms, each selected by the path switches.  Per form: first a 2-step DDIM dsd_sample with
use_graph = True (not "lazy": the first call captures), then the same call eagerly on the same handle under the timing hook,
which also names the kernels that ran.  The order guarantees the property by construction, and the child asserts it: each
form names the kernels that are NEW with it, those must be among the kernels its eager pass reports, and none of them may have
been reported by an earlier form of the process - so their first launch was the captured one.  (Creating a handle launches
nothing; dsd_prepare_cond and the step tables run gemm.hip kernels only.)

Criterion: the one tests/test_gpu_parity.py holds its use_graph cases to (1.5e-5, max and rms), captured against eager, on
the valid frames of each item.  Shapes: B = 2, T = 70 - two whole 32-frame tiles and a cut one - and the ragged lengths
[70, 33]; grids this small reach the row-split pair only through the mixed-plan hook the Winograd tests use (DSD_WN_PLAN=2 +
DSD_RS_ROWS=64: the first half of the tiles on the fused kernel, the rest on the pair)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_SAMPLER = 1.5e-5
B, T, LENGTHS = 2, 70, [70, 33]
SWITCHES = ("DSD_FUSED_LAYER", "DSD_FUSED16", "DSD_WN_PLAN", "DSD_ROWSPLIT", "DSD_RS_CONV_Q", "DSD_RS_ROWS", "DSD_EDGE",
            "DSD_LYNX_RESIDENT", "DSD_LYNX_PW1P", "DSD_LYNX_PW2Q", "DSD_PRECISION", "DSD_X3_WIDE")
PAIR = dict(DSD_WN_PLAN="2", DSD_RS_ROWS="64")

# (name, switches, precision, kernels that are new with the form: prefixes of dsd_kernel_timing_classes names).  Each form
# runs dense, then ragged; the ragged kernels are instantiations of their own (last template argument 1).
WAVENET = dict(
    kind="wavenet", args=dict(num_layers=2, num_channels=256, dilation_cycle_length=2),
    forms=[
        ("fused", dict(DSD_FUSED_LAYER="1"), "f32", ["wn_layer_kernel<"]),
        ("fused16", dict(DSD_FUSED16="1"), "f32", ["wn_layer16_kernel<"]),
        ("rows128", dict(DSD_RS_ROWS="128"), "f32", ["wn_conv_rw_kernel<2,", "wn_out_rw_kernel<2,"]),
        ("rows256", dict(DSD_RS_ROWS="256"), "f32", ["wn_conv_rw_kernel<4,", "wn_out_rw_kernel<4,"]),
        ("pair_winograd", PAIR, "f32", ["wn_conv_wq_kernel<", "wn_out_rs_kernel<2,"]),       # the one-utterance default's pair
        ("pair_halves", dict(PAIR, DSD_RS_CONV_Q="0"), "f32", ["wn_conv_rs_kernel<"]),
        ("pair_quarters", dict(PAIR, DSD_RS_CONV_Q="1"), "f32", ["wn_conv_rq_kernel<2,"]),
        ("edge", dict(DSD_EDGE="1"), "f32", ["wn_edge_kernel<"]),
        ("fused_bf16x3", dict(DSD_FUSED_LAYER="1"), "bf16x3", ["wn_layer_x3_kernel<"]),
    ])
# C = 512, inner = 1024 at 6 (5) frame tiles: with DSD_LYNX_RESIDENT=1 the planner's own rule gives pw2 to the 128-row kernel,
# so DSD_LYNX_PW2Q=1 comes first and the switch-less form after it launches nothing new (it is still run and compared)
LYNXNET = dict(
    kind="lynxnet", args=dict(num_layers=2, num_channels=512, expansion_factor=2, kernel_size=31, activation="PReLU", strong_cond=False),
    forms=[
        ("pw2q", dict(DSD_LYNX_RESIDENT="1", DSD_LYNX_PW2Q="1"), "f32", ["lx_pw1", "lx_pw2q_kernel<"]),
        ("resident", dict(DSD_LYNX_RESIDENT="1"), "f32", []),
        ("pw2d", dict(DSD_LYNX_RESIDENT="1", DSD_LYNX_PW2Q="0"), "f32", ["lx_pw2d_kernel<"]),
        ("bf16x3", dict(DSD_LYNX_RESIDENT="1"), "bf16x3", ["lx_x3_kernel<"]),
    ])
FAMILIES = dict(wavenet=WAVENET, lynxnet=LYNXNET)


def child(family):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from diffsinger_amd import synth
    from diffsinger_amd.diffusion import GaussianDiffusion
    from gpu_util import check, dev, load_synth, set_hp, synth_params
    fam = FAMILIES[family]
    for k in SWITCHES:
        os.environ.pop(k, None)
    set_hp(diff_accelerator="ddim", diff_speedup=500, K_step_infer=1000)        # 2 steps
    d = GaussianDiffusion(128, 1, timesteps=1000, k_step=1000, backbone_type=fam["kind"], backbone_args=fam["args"],
                          spec_min=[-12.0], spec_max=[0.0])
    load_synth(d.denoise_fn, synth_params(fam["kind"], 128, 1, fam["args"], 45))
    d = d.cuda().eval()
    net = d.denoise_fn
    cond = dev(synth.synth_normal((B, T, 256), 71))
    noise = dev(synth.synth_normal((B, 1, 128, T), 72))
    seen = set()
    for name, switches, precision, new in fam["forms"]:
        for lengths in (None, LENGTHS):
            what = (family, name, "ragged" if lengths else "dense")
            os.environ.update(switches)
            net.set_precision(precision)
            net.set_lengths(lengths, cond.device)           # kept until the next form: dsd_get_stats reports the current plan
            d.use_graph = True
            captured = d(cond, infer=True, noise=noise).clone()
            st = net.stats()
            d.use_graph = False
            net.kernel_timing(True)
            eager = d(cond, infer=True, noise=noise).clone()
            names = {k["name"] for k in net.kernel_classes()}
            net.kernel_timing(False)
            torch.cuda.synchronize()
            tiles = lambda bn: sum((n + bn - 1) // bn for n in (lengths or [T] * B))      # noqa: E731
            if name in ("fused", "fused_bf16x3"):           # as tests/test_gpu_fused.py asserts of its forced plans
                assert st["layer_launches"] == 1 and st["fused_tiles"] == tiles(32) and st["split_tiles"] == 0, (what, st)
            if name == "fused16":
                assert st["layer_launches"] == 1 and st["fused_tiles"] == tiles(16) and st["split_tiles"] == 0, (what, st)
            assert st["precision"] == (1 if precision == "bf16x3" else 0), (what, st)
            first = set()
            for prefix in new:
                hit = {n for n in names if n.startswith(prefix)}
                assert hit, (what, "did not run", prefix, sorted(names))
                first |= hit
            assert not (first & seen), (what, "ran eagerly before their capture", sorted(first & seen))
            seen |= names
            for b, n in enumerate(lengths or [T] * B):      # [B, T, M]: the valid frames of each item
                mx = check(captured[b, :n], eager[b, :n].cpu().numpy(), TOL_SAMPLER, what=what + (b,))
                print(what, b, "max_rel", mx, "equal", bool(torch.equal(captured[b, :n], eager[b, :n])), flush=True)
            assert np.isfinite(eager.cpu().numpy()[0]).all()
            for k in switches:
                os.environ.pop(k)
    net.set_precision("f32")
    net.release_native()
    print("__FIRST_CAPTURE_OK__", family, flush=True)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_first_launch_of_each_form_is_a_captured_one(family):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), family], env=env, cwd=ROOT,
                       capture_output=True, text=True)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and "__FIRST_CAPTURE_OK__ " + family in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])


if __name__ == "__main__":
    child(sys.argv[1])
