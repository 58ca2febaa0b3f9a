"""LYNXNet and the ConvNeXt aux decoder at widths that are not multiples of 32 (dsd_create_any_width): the network runs at the
next multiple with the extra channels exactly zero and every LayerNorm taken over the true channel count.

Against G20 (the reference at num_channels 500 / 1000 / 90 / 6, a RectifiedFlow run, AuxDecoderAdaptor at 500 / 75) and, for the
larger grids, against the numpy oracle that tests/test_width_host.py pins to G20 at these widths.  A LayerNorm over the padded
count misstates the variance by ~2.4 % at 500 and ~6.7 % at 90, orders of magnitude above the tolerances, which are the project's
existing ones.  Every frame and channel of every case is compared; every run is repeated and must be bit-equal to itself.

The resident kernels (lynx_layer.hip, lynx_x3.hip) must serve 500 / 1000 exactly as they serve 512 / 1024: forced on small grids
in every form that writes or merges LayerNorm partials, and by the library's own plan, whose kernel classes and launch counts must
equal those of the padded twin."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import width_cases as wc  # noqa: E402
from diffsinger_amd import synth  # noqa: E402
from gpu_util import check, dev, load_synth, make_backbone, set_hp, synth_params  # noqa: E402
from oracle import backbones as ob  # noqa: E402

TOL_NFE = 2e-5
TOL_SAMPLER = 1.5e-5
TOL_AUX = 2e-5
SWITCHES = ("DSD_LYNX_RESIDENT", "DSD_LYNX_PW2Q", "DSD_LYNX_PW1P")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load():
    return np.load(os.path.join(GOLDEN, "g20_width.npz"))


@pytest.fixture(autouse=True)
def _clean_env():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    set_hp()
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    yield
    for k in SWITCHES:
        os.environ.pop(k, None)
        if saved[k] is not None:
            os.environ[k] = saved[k]


def _run(net, x, t, cond, lengths=None):
    xd = dev(x)
    net.set_lengths(lengths, xd.device)
    with torch.no_grad():
        out = net(xd, dev(t), dev(cond))
        again = net(xd, dev(t), dev(cond))
    torch.cuda.synchronize()
    assert torch.equal(out, again)
    return out.cpu().numpy()


def _classes(net, x, t, cond, lengths=None):
    """(class names, launches of the timed classes) of one more pass"""
    net.kernel_timing(True)
    xd = dev(x)
    net.set_lengths(lengths, xd.device)
    with torch.no_grad():
        net(xd, dev(t), dev(cond))
    torch.cuda.synchronize()
    ks = net.kernel_classes()
    net.kernel_timing(False)
    return [k["name"] for k in ks], sum(k["launches"] for k in ks)


def _oracle(params, args):
    return lambda xx, tt, cc: ob.lynxnet_forward(params, xx, tt, cc, activation=args["activation"], strong_cond=args["strong_cond"])


def _check_items(out, fwd, x, t, cond, lengths, what):
    if lengths is None:
        check(out, fwd(x, t, cond), TOL_NFE, what=what)
        return
    for b, n in enumerate(lengths):
        check(out[b:b + 1, :, :, :n], fwd(x[b:b + 1, :, :, :n], t[b:b + 1], cond[b:b + 1, :, :n]), TOL_NFE, what=(what, b))


# --------------------------------------------------------------------------- G20: the reference itself
@pytest.mark.parametrize("tag", sorted(wc.LYNX_EVALS))
def test_lynxnet_evaluations_vs_golden(tag):
    in_dims, n_feats, args, wseed, cases = wc.LYNX_EVALS[tag]
    g = load()
    net, params = make_backbone("lynxnet", in_dims, n_feats, args, wseed)
    assert synth.state_dict_digest(params) == str(g[f"{tag}_digest"])
    for ci, (bsz, t_len, _) in enumerate(cases):
        xs, cs, _ = wc.eval_seeds(ci)
        x = synth.synth_normal((bsz, n_feats, in_dims, t_len), xs)
        cond = synth.synth_normal((bsz, 256, t_len), cs)
        out = _run(net, x, g[f"{tag}_c{ci}_t"], cond)
        mx = check(out, g[f"{tag}_c{ci}_out"], TOL_NFE, what=("G20", tag, ci))
        print(f"G20 {tag} case {ci}: {mx:.3g}")
    net.release_native()


@pytest.mark.parametrize("use_graph", [False, True])
def test_lynxnet_sampler_vs_golden(use_graph):
    from diffsinger_amd.diffusion import RectifiedFlow
    s = wc.SAMPLER
    g = load()
    set_hp(sampling_algorithm="euler", sampling_steps=s["steps"])
    r = RectifiedFlow(s["in_dims"], s["n_feats"], backbone_type="lynxnet", backbone_args=s["args"], spec_min=[-12.0], spec_max=[0.0])
    load_synth(r.velocity_fn, synth_params("lynxnet", s["in_dims"], s["n_feats"], s["args"], s["wseed"]))
    r = r.cuda().eval()
    r.use_graph = use_graph
    cond = dev(synth.synth_normal((s["bsz"], s["t_len"], 256), s["cond_seed"]))
    noise = dev(synth.synth_normal((s["bsz"], s["n_feats"], s["in_dims"], s["t_len"]), s["noise_seed"]))
    out = r(cond, infer=True, noise=noise)
    again = r(cond, infer=True, noise=noise)        # (use_graph: the second run of a program is the captured one)
    third = r(cond, infer=True, noise=noise)
    torch.cuda.synchronize()
    assert torch.equal(out, again) and torch.equal(out, third)
    mx = check(out, g["rf_euler10_out"], TOL_SAMPLER, what=("G20 reflow euler", use_graph))
    print(f"G20 reflow euler, graph {use_graph}: {mx:.3g}")
    r.velocity_fn.release_native()


@pytest.mark.parametrize("tag", sorted(wc.AUX))
def test_aux_decoder_vs_golden(tag):
    from diffsinger_amd.aux_decoder import AuxDecoderAdaptor
    hsz, m, args, bsz, t_len, wseed = wc.AUX[tag]
    g = load()
    a = AuxDecoderAdaptor(hsz, m, 1, list(map(float, g[f"{tag}_smin"])), list(map(float, g[f"{tag}_smax"])), "convnext", dict(args))
    shapes = synth.convnext_param_shapes(hsz, m, num_channels=args["num_channels"], num_layers=args["num_layers"],
                                         kernel_size=args["kernel_size"], prefix="decoder.")
    params = synth.synth_state_dict(shapes, seed=wseed)
    assert synth.state_dict_digest(params) == str(g[f"{tag}_digest"])
    a.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    a = a.cuda().eval()
    cond = dev(synth.synth_normal((bsz, t_len, hsz), wseed + 100))
    with torch.no_grad():
        raw, mel = a(cond, infer=False), a(cond, infer=True)
        raw2, mel2 = a(cond, infer=False), a(cond, infer=True)
    torch.cuda.synchronize()
    assert torch.equal(raw, raw2) and torch.equal(mel, mel2)
    e1 = check(raw, g[f"{tag}_raw"], TOL_AUX, what=("G20 aux raw", tag))
    e2 = check(mel, g[f"{tag}_mel"], TOL_AUX, what=("G20 aux mel", tag))
    print(f"G20 aux {tag}: raw {e1:.3g} mel {e2:.3g}")
    a.decoder.release_native()


# --------------------------------------------------------------------------- the resident kernels, forced
NETS = {
    "c1000_strong": dict(num_layers=3, num_channels=1000, expansion_factor=2, kernel_size=31, activation="PReLU", strong_cond=True),
    "c500_default": dict(num_layers=3, num_channels=500, expansion_factor=2, kernel_size=31, activation="PReLU", strong_cond=False),
}
GRIDS = {"dense_T211_B2": (2, 211, None), "dense_T96_B1": (1, 96, None), "ragged_B3": (3, 200, [200, 77, 141])}
# (grid, DSD_LYNX_PW2Q, DSD_LYNX_PW1P): both pw2 forms (0: lx_pw2d_kernel, 1: lx_pw2q_kernel) and pw1 as lx_pw1_kernel (0), as
# lx_pw1p_kernel in 2 row-tile groups and by the library's choice (-1), each on a grid with cut tiles and on the ragged one
FORCED = [("dense_T211_B2", 1, 0), ("dense_T211_B2", 0, 2), ("dense_T96_B1", 0, 0), ("dense_T96_B1", 1, 2),
          ("ragged_B3", 1, -1), ("ragged_B3", 0, 0)]


@pytest.mark.parametrize("grid,pw2q,pw1p", FORCED)
@pytest.mark.parametrize("net_name", sorted(NETS))
def test_resident_kernels_forced_vs_oracle(net_name, grid, pw2q, pw1p):
    args = NETS[net_name]
    bsz, t_len, lengths = GRIDS[grid]
    os.environ["DSD_LYNX_RESIDENT"] = "1"
    os.environ["DSD_LYNX_PW2Q"] = str(pw2q)
    if pw1p >= 0:
        os.environ["DSD_LYNX_PW1P"] = str(pw1p)
    net, params = make_backbone("lynxnet", 128, 1, args, 61)
    x = synth.synth_normal((bsz, 1, 128, t_len), 21)
    cond = synth.synth_normal((bsz, 256, t_len), 22)
    t = (np.arange(bsz) * 173.25 + 7.5).astype(np.float32)
    out = _run(net, x, t, cond, lengths)
    names, _ = _classes(net, x, t, cond, lengths)
    assert any(n.startswith("lx_pw1") for n in names) and any(n.startswith("lx_pw2") for n in names), names
    assert not any("gemm_kernel" in n for n in names), names
    assert any(n.startswith("lx_pw2q_kernel" if pw2q else "lx_pw2d_kernel") for n in names), names
    if pw1p >= 0:
        assert any(n.startswith("lx_pw1_kernel" if pw1p == 0 else "lx_pw1p_kernel") for n in names), names
    _check_items(out, _oracle(params, args), x, t, cond, lengths, ("resident forced", net_name, grid, pw2q, pw1p))
    net.release_native()


@pytest.mark.parametrize("net_name", sorted(NETS))
def test_split_bf16_forced_vs_oracle(net_name):
    args = NETS[net_name]
    bsz, t_len = 2, 211
    os.environ["DSD_LYNX_RESIDENT"] = "1"
    net, params = make_backbone("lynxnet", 128, 1, args, 62)
    x = synth.synth_normal((bsz, 1, 128, t_len), 21)
    cond = synth.synth_normal((bsz, 256, t_len), 22)
    t = (np.arange(bsz) * 173.25 + 7.5).astype(np.float32)
    f32 = _run(net, x, t, cond)
    net.set_precision("bf16x3")
    out = _run(net, x, t, cond)
    assert net.stats()["precision"] == 1 and not np.array_equal(out, f32)
    names, _ = _classes(net, x, t, cond)
    assert any(n.startswith("lx_x3_kernel") for n in names) and not any("gemm_kernel" in n for n in names), names
    check(out, _oracle(params, args)(x, t, cond), TOL_NFE, what=("bf16x3", net_name))
    net.set_precision("f32")
    assert np.array_equal(_run(net, x, t, cond), f32)
    net.release_native()


# --------------------------------------------------------------------------- the library's own plan
@pytest.mark.parametrize("odd,twin,layers,strong,bsz,t_len", [(1000, 1024, 2, True, 1, 1000), (500, 512, 3, False, 8, 200)])
def test_natural_plan_equals_the_padded_twin(odd, twin, layers, strong, bsz, t_len):
    x = synth.synth_normal((bsz, 1, 128, t_len), 31)
    cond = synth.synth_normal((bsz, 256, t_len), 32)
    t = (np.arange(bsz) * 101.5 + 12.0).astype(np.float32)
    seen = {}
    for c in (odd, twin):
        args = dict(num_layers=layers, num_channels=c, expansion_factor=2, kernel_size=31, activation="PReLU", strong_cond=strong)
        net, params = make_backbone("lynxnet", 128, 1, args, 63)
        out = _run(net, x, t, cond)
        names, launches = _classes(net, x, t, cond)
        seen[c] = (sorted(names), launches, net.stats()["workspace_bytes"], net.stats()["weight_bytes"])
        if c == odd:
            assert any(n.startswith("lx_pw1") for n in names) and any(n.startswith("lx_pw2") for n in names), names
            check(out, _oracle(params, args)(x, t, cond), TOL_NFE, what=("natural plan", c, bsz, t_len))
        net.release_native()
    assert seen[odd] == seen[twin], seen


# --------------------------------------------------------------------------- rejections through the shim
@pytest.mark.parametrize("channels", (501, 2))
def test_shim_raises_with_the_librarys_message(channels):
    from diffsinger_amd import _lib
    from diffsinger_amd.backbones import build_backbone
    net = build_backbone(32, 1, "lynxnet", dict(num_layers=2, num_channels=channels, expansion_factor=2, kernel_size=7,
                                                activation="SiLU")).cuda().eval()
    with torch.no_grad(), pytest.raises(_lib.NativeLibraryError, match="reference cannot build"):
        net(torch.zeros(1, 1, 32, 8, device="cuda"), torch.zeros(1, device="cuda"), torch.zeros(1, 256, 8, device="cuda"))
    assert net._handle is None          # no handle, so nothing was loaded or launched
