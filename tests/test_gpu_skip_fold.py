"""The skip projection folded into the layers' skip rows (build_packed / run_wavenet in csrc/api.hip) on the GPU.

An fp32 evaluation that does not end in the edge kernel runs its layers on a second out-proj pack whose skip rows carry
W1 Ws_l / sqrt(L), launches no skip-projection GEMM, and lets the output projection stage max(skip, 0) itself (gemm.hip, ST_RELU).
Every layer form reads that pack, so one evaluation is put against the numpy oracle under each form the path switches can force
(the row-split pair in its three conv layouts as the second segment of a DSD_WN_PLAN=2 plan - the only way onto it at these
sizes - wn_rows.hip, the gemm.hip pair, fused segments with the edge off), at the tolerance of tests/test_gpu_rowsplit.py.  Sampler
loops, eager and replayed from their graph, are put against DSD_EDGE=1 on the same handle: the edge kernel reads the unfolded
weights, and 2e-6 of the range is the bound tests/test_gpu_edge.py holds between the two.  Precision changes and reloaded
weights must rebuild the folded pack."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from diffsinger_amd import synth  # noqa: E402
from gpu_util import check, dev, load_synth, make_backbone, set_hp, synth_params  # noqa: E402
from oracle import backbones as ob  # noqa: E402

TOL_NFE = 2e-5      # tests/test_gpu_rowsplit.py
SWITCHES = ("DSD_FUSED_LAYER", "DSD_WN_PLAN", "DSD_ROWSPLIT", "DSD_RS_CONV_Q", "DSD_RS_ROWS", "DSD_EDGE")

FORMS = {
    "default": {},
    "gemm_pair": dict(DSD_ROWSPLIT="0", DSD_FUSED_LAYER="0"),
    "rowsplit_halves": dict(DSD_WN_PLAN="2", DSD_RS_CONV_Q="0"),
    "rowsplit_quarters": dict(DSD_WN_PLAN="2", DSD_RS_CONV_Q="1"),
    "rowsplit_winograd": dict(DSD_WN_PLAN="2", DSD_RS_CONV_Q="2"),
    "rows128": dict(DSD_FUSED_LAYER="0", DSD_RS_ROWS="128"),
    "rows256": dict(DSD_FUSED_LAYER="0", DSD_RS_ROWS="256"),
    "fused_edge_off": dict(DSD_FUSED_LAYER="1", DSD_EDGE="0"),
}

ACOUSTIC = (128, 1, dict(num_layers=20, num_channels=256, dilation_cycle_length=4))
# name -> ((in_dims, n_feats, args), B, T, lengths)
SHAPES = {
    "acoustic_T20": (ACOUSTIC, 1, 20, None),                  # one cut tile
    "acoustic_T70": (ACOUSTIC, 1, 70, None),                  # three tiles
    "acoustic_T7": (ACOUSTIC, 1, 7, None),                    # T < dilation 8
    "acoustic_ragged_B2": (ACOUSTIC, 2, 70, [70, 33]),
    "c250": ((128, 1, dict(num_layers=4, num_channels=250, dilation_cycle_length=4)), 1, 70, None),      # runs as 256 channels
    "three_layers": ((128, 1, dict(num_layers=3, num_channels=256, dilation_cycle_length=4)), 1, 70, None),
    "pitch_cycle5": ((64, 1, dict(num_layers=5, num_channels=256, dilation_cycle_length=5)), 1, 70, None),   # dilation 16 in layer 4
    "variance_10x192": ((24, 2, dict(num_layers=10, num_channels=192, dilation_cycle_length=4)), 1, 70, None),
}


class _env:
    def __init__(self, kv):
        self.kv = kv

    def __enter__(self):
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k in self.kv:
            os.environ.pop(k, None)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    saved = {k: os.environ.get(k) for k in SWITCHES}
    set_hp()
    yield
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


_nets = {}


@pytest.fixture(scope="module")
def nets():
    """one network (and its parameters) per configuration, shared by the shapes that use it"""
    def get(cfg):
        key = repr(cfg)
        if key not in _nets:
            in_dims, n_feats, args = cfg
            _nets[key] = make_backbone("wavenet", in_dims, n_feats, args, 42)
        return _nets[key]
    yield get
    for net, _ in _nets.values():
        net.release_native()
    _nets.clear()


def _oracle(params, args, x, t, cond, lengths):
    cyc = args["dilation_cycle_length"]
    if lengths is None:
        return [ob.wavenet_forward(params, x, t, cond, dilation_cycle_length=cyc)]
    return [ob.wavenet_forward(params, x[b:b + 1, :, :, :n], t[b:b + 1], cond[b:b + 1, :, :n], dilation_cycle_length=cyc)
            for b, n in enumerate(lengths)]


def _items(out, lengths):
    if lengths is None:
        return [out]
    return [out[b:b + 1, :, :, :n] for b, n in enumerate(lengths)]


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_folded_evaluation_vs_oracle_under_every_layer_form(name, nets):
    cfg, bsz, t_len, lengths = SHAPES[name]
    in_dims, n_feats, args = cfg
    net, params = nets(cfg)
    x = synth.synth_normal((bsz, n_feats, in_dims, t_len), 31)
    cond = synth.synth_normal((bsz, 256, t_len), 32)
    t = (np.arange(bsz) * 211.5 + 3.25).astype(np.float32)
    want = _oracle(params, args, x, t, cond, lengths)
    xd, td, cd = dev(x), dev(t), dev(cond)
    net.set_lengths(lengths, xd.device)
    try:
        for form, kv in FORMS.items():
            with _env(kv):
                with torch.no_grad():
                    out = net(xd, td, cd)
                    again = net(xd, td, cd)
                torch.cuda.synchronize()
                stats = net.stats()
            assert torch.equal(out, again), (name, form)
            if args["num_channels"] == 256:          # the forced form really ran (192 channels: the gemm.hip pair is the only one)
                tiles = sum((n + 31) // 32 for n in (lengths or [t_len] * bsz))
                if form.startswith("rowsplit"):
                    assert stats["fused_tiles"] == tiles // 2 and stats["split_tiles"] == tiles - tiles // 2, (name, form, stats)
                elif form == "fused_edge_off":
                    assert stats["fused_tiles"] == tiles and stats["layer_launches"] == 1, (name, form, stats)
                elif form == "gemm_pair":
                    assert stats["fused_tiles"] == 0 and stats["layer_launches"] == 2, (name, form, stats)
            for b, (g, w) in enumerate(zip(_items(out.cpu().numpy(), lengths), want)):
                check(g, w, TOL_NFE, what=("folded evaluation", name, form, b))
    finally:
        net.set_lengths(None, xd.device)


def _sampler_vs_edge(d, net, call, what):
    """the folded GEMM path (DSD_EDGE=0: eager, then captured and replayed) against the edge kernel on the same handle"""
    with _env(dict(DSD_EDGE="1")):
        ref = call()
        ref = [r.cpu().numpy() for r in (ref if isinstance(ref, (tuple, list)) else [ref])]
    with _env(dict(DSD_EDGE="0")):
        runs = [call() for _ in range(3)]
        assert net.stats()["kernels_per_nfe"] > 0
    runs = [list(r) if isinstance(r, (tuple, list)) else [r] for r in runs]
    for k, r in enumerate(runs):
        for g, w in zip(r, ref):
            check(g, w, 2e-6, what=(what, "run", k))
    for r in runs[1:]:
        for g, g0 in zip(r, runs[0]):
            assert torch.equal(g, g0), what
    net.release_native()


def test_dpm_solver_loop_folded_vs_edge_kernel():
    from diffsinger_amd.diffusion import GaussianDiffusion
    set_hp(K_step_infer=1000, diff_accelerator="dpm-solver", diff_speedup=100)          # 10 evaluations
    args = dict(num_layers=4, num_channels=256, dilation_cycle_length=4)
    d = GaussianDiffusion(128, 1, backbone_type="wavenet", backbone_args=args, spec_min=[-12.0], spec_max=[0.0])
    load_synth(d.denoise_fn, synth_params("wavenet", 128, 1, args, 42))
    d = d.cuda().eval()
    cond = dev(synth.synth_normal((2, 150, 256), 40))
    noise = dev(synth.synth_normal((2, 1, 128, 150), 41))
    _sampler_vs_edge(d, d.denoise_fn, lambda: d(cond, infer=True, noise=noise), "DPM-Solver++ 10 steps")


def test_euler_reflow_loop_folded_vs_edge_kernel():
    from diffsinger_amd.diffusion import PitchRectifiedFlow
    set_hp(sampling_algorithm="euler", sampling_steps=10)
    args = dict(num_layers=6, num_channels=256, dilation_cycle_length=5)          # dilation 16 in layer 4
    d = PitchRectifiedFlow(vmin=-8.0, vmax=8.0, cmin=-12.0, cmax=12.0, repeat_bins=64, backbone_type="wavenet", backbone_args=args)
    load_synth(d.velocity_fn, synth_params("wavenet", 64, 1, args, 42))
    d = d.cuda().eval()
    cond = dev(synth.synth_normal((2, 133, 256), 50))
    noise = dev(synth.synth_normal((2, 1, 64, 133), 51))
    _sampler_vs_edge(d, d.velocity_fn, lambda: d(cond, infer=True, noise=noise), "euler reflow 10 steps")


def test_precision_round_trip_rebuilds_the_folded_pack():
    args = dict(num_layers=4, num_channels=256, dilation_cycle_length=4)
    net, params = make_backbone("wavenet", 128, 1, args, 42)
    x = synth.synth_normal((1, 1, 128, 70), 31)
    cond = synth.synth_normal((1, 256, 70), 32)
    t = np.asarray([3.25], np.float32)
    want = ob.wavenet_forward(params, x, t, cond, dilation_cycle_length=4)
    xd, td, cd = dev(x), dev(t), dev(cond)
    with _env({}), torch.no_grad():
        first = net(xd, td, cd)
        net.set_precision("bf16x3")
        x3 = net(xd, td, cd)
        net.set_precision("f32")
        back = net(xd, td, cd)
    check(first, want, TOL_NFE, what="f32, folded")
    check(x3, want, TOL_NFE, what="bf16x3 mode (unfolded weights)")
    assert torch.equal(first, back)
    net.release_native()


def test_reloaded_skip_projection_changes_the_output():
    args = dict(num_layers=4, num_channels=256, dilation_cycle_length=4)
    net, params = make_backbone("wavenet", 128, 1, args, 42)
    x = synth.synth_normal((1, 1, 128, 70), 31)
    cond = synth.synth_normal((1, 256, 70), 32)
    t = np.asarray([3.25], np.float32)
    xd, td, cd = dev(x), dev(t), dev(cond)
    with _env({}), torch.no_grad():
        before = net(xd, td, cd)
        changed = dict(params)
        changed["skip_projection.weight"] = (params["skip_projection.weight"][::-1] * np.float32(1.25)).copy()
        with torch.no_grad():
            net.skip_projection.weight.copy_(dev(changed["skip_projection.weight"]))
        net.refresh_native()                  # dsd_load_weight of every tensor + dsd_finalize_weights
        after = net(xd, td, cd)
    assert not torch.equal(before, after)
    check(before, ob.wavenet_forward(params, x, t, cond, dilation_cycle_length=4), TOL_NFE, what="before the reload")
    check(after, ob.wavenet_forward(changed, x, t, cond, dilation_cycle_length=4), TOL_NFE, what="after the reload")
    net.release_native()
