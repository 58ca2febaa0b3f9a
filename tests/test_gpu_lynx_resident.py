"""Every fp32 form of LYNXNet's two pointwise GEMMs in lynx_layer.hip against the numpy oracle (oracle.backbones.lynxnet_forward),
in the style of test_gpu_fused.py.

plan_denoise (api.hip) and launch_lx_layer pick the forms from the grid and the CU count, so the small grids the oracle handles
would reach few of them by themselves: the path switches are snapshotted on each C-ABI call, and these tests force every form
on them - pw1: DSD_LYNX_PW1P=0 (lx_pw1_kernel, one row tile per workgroup) or g = 1 / 2 / 4 row-tile groups (lx_pw1p_kernel);
pw2: DSD_LYNX_PW2Q=0 (lx_pw2d_kernel<NP> for inner 1024 / 2048, lx_pw2_kernel<512> for inner 512) or 1 (lx_pw2q_kernel) - on
four 3-layer nets (a pw2 feeds the next layer's pw1; the last pw2 has none), dense and ragged grids.  Every case reads the kernel
classes of a timing pass back (dsd_kernel_timing_classes) and asserts the exact instantiation of both GEMMs and no other lx_ or
gemm.hip pw1 / pw2 class, so a silent fallback fails.  Tolerance 2e-5 (max and RMS, gpu_util.check); ragged grids per item on
its valid frames, once more with the caller's padding poisoned with NaN (an item computes as if it ran alone).

Bit identity across forms: lx_pw1p_kernel runs the same per-row-tile code whatever the group count - only the workgroup that
runs a row tile changes - and lx_pw1_kernel shares its statistics merge (lx_merge_stats), staging, K walk (k_phase) and SwiGLU
epilogue arithmetic, so PW1P = 0 / 1 / 2 / 4 must agree bit for bit: a forced group count that decoded its (group, frame tile)
wrongly cannot hide inside the tolerance.

Then the natural grids, no switches: resident pw1 + the gemm.hip pw2 (EP_LYNX_NEXT) of one-utterance grids, config 3's own grid
(6 x 1024, B = 8, T = 1000) dense and ragged, and config 3's DDIM sampler at that grid (5 NFE) against oracle.diffusion."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from diffsinger_amd import synth  # noqa: E402
from diffsinger_amd._lib import NativeLibraryError  # noqa: E402
from gpu_util import check, dev, load_synth, make_backbone, set_hp, synth_params  # noqa: E402
from oracle import backbones as ob  # noqa: E402
from oracle import diffusion as od  # noqa: E402

TOL_NFE = 2e-5
TOL_SAMPLER = 1.5e-5
SWITCHES = ("DSD_LYNX_RESIDENT", "DSD_LYNX_PW1P", "DSD_LYNX_PW2Q", "DSD_PRECISION", "DSD_X3_WIDE")


def _net(c, e, act, strong, layers=3):
    return dict(num_layers=layers, num_channels=c, expansion_factor=e, kernel_size=31, activation=act, strong_cond=strong)


# name -> (backbone args, weight seed).  Row tiles of pw1 = 2 inner / 512: 8, 4, 4, 2
NETS = {
    "c1024_e2": (_net(1024, 2, "PReLU", True), 61),     # the fork's net: pw2 on lx_pw2d<4> / lx_pw2q<512>
    "c512_e2": (_net(512, 2, "SiLU", False), 62),       # the class default: lx_pw2d<2> / lx_pw2q<256>
    "c1024_e1": (_net(1024, 1, "ReLU", True), 63),      # inner 1024 at C = 1024: lx_pw2d<2>, no 128-row form
    "c512_e1": (_net(512, 1, "PReLU", False), 64),      # inner 512: lx_pw2_kernel<512> (one resident phase)
}
# (B, T, lengths)
GRIDS = {
    "dense_T211_B2": (2, 211, None),            # 7 tiles per item, the last cut at 19 frames
    "dense_T13_B3": (3, 13, None),              # T below the depthwise half-window (15): every item one partial tile
    "ragged_B3": (3, 200, [200, 77, 141]),      # item ends inside tiles, different tile counts
    "ragged_short": (3, 64, [1, 64, 33]),       # a 1-frame item, a tile-exact one, one that ends 1 frame into its second tile
}


def _inner(args):
    return args["num_channels"] * args["expansion_factor"]


def _pw1_values(args):
    """DSD_LYNX_PW1P values valid for the net: 0, and every g that divides the 2 inner / 512 row tiles and is below their count"""
    mt = 2 * _inner(args) // 512
    return [0] + [g for g in (1, 2, 4) if g < mt and mt % g == 0]


def _pw2q_values(args):
    return [0, 1] if (args["num_channels"], _inner(args)) in ((1024, 2048), (512, 1024)) else [0]


def _pw1_class(args, pw1p, rag):
    return f"lx_pw1_kernel<{args['num_channels']}, {rag}>" if pw1p == 0 else f"lx_pw1p_kernel<{args['num_channels']}, {rag}>"


def _pw2_class(args, pw2q, rag):
    inner = _inner(args)
    if pw2q == 1:
        return f"lx_pw2q_kernel<{inner // 4}, {rag}>"
    return f"lx_pw2d_kernel<{inner // 512}, {rag}>" if inner >= 1024 else f"lx_pw2_kernel<{inner}, {rag}>"


def _gemm_classes(names):
    """the pointwise GEMMs' classes on the timed launches: lx_* kernels and gemm.hip's pw1 (ST_LN, EP_SWIGLU) / pw2 (EP_LYNX_NEXT)"""
    return sorted(n for n in names if n.startswith("lx_") or n.startswith("gemm_kernel<2, 1, 4,") or n.startswith("gemm_kernel<0, 1, 7,"))


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


def _set(**kw):
    for k, v in kw.items():
        name = "DSD_LYNX_" + k.upper()
        if v is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = str(v)


def _inputs(bsz, t_len, seed):
    x = synth.synth_normal((bsz, 1, 128, t_len), seed)
    cond = synth.synth_normal((bsz, 256, t_len), seed + 1)
    t = (np.arange(bsz) * 173.25 + 7.5).astype(np.float32)
    return x, t, cond


def _items(out, lengths):
    """the frames the caller keeps: the whole batch (dense), or per item its valid frames (ragged)"""
    return [out] if lengths is None else [out[b:b + 1, :, :, :n] for b, n in enumerate(lengths)]


def _run(net, x, t, cond, lengths):
    """one evaluation, twice back to back: the same bits both times (on the frames the caller keeps)"""
    xd = dev(x)
    net.set_lengths(lengths, xd.device)
    with torch.no_grad():
        out = net(xd, dev(t), dev(cond)).cpu().numpy()
        again = net(xd, dev(t), dev(cond)).cpu().numpy()
    for a, b in zip(_items(out, lengths), _items(again, lengths)):
        assert np.array_equal(a, b), "two back-to-back calls differ"
    return out


def _classes(net, x, t, cond, lengths):
    net.kernel_timing(True)
    _run(net, x, t, cond, lengths)
    names = [k["name"] for k in net.kernel_classes()]
    net.kernel_timing(False)
    return names


def _oracle(params, args, x, t, cond, lengths):
    fwd = lambda xx, tt, cc: ob.lynxnet_forward(params, xx, tt, cc, activation=args["activation"], strong_cond=args["strong_cond"])  # noqa: E731
    if lengths is None:
        return [fwd(x, t, cond)]
    return [fwd(x[b:b + 1, :, :, :n], t[b:b + 1], cond[b:b + 1, :, :n]) for b, n in enumerate(lengths)]


def _check(out, want, lengths, what):
    for b, (a, w) in enumerate(zip(_items(out, lengths), want)):
        check(a, w, TOL_NFE, what=what + (b,))


@pytest.mark.parametrize("grid", sorted(GRIDS))
@pytest.mark.parametrize("net_name", sorted(NETS))
def test_pointwise_forms_forced_vs_oracle(net_name, grid):
    """every (pw1, pw2) form of the net on this grid: classes asserted, against the oracle, PW1P forms bit-identical; ragged grids
    again with NaN in the caller's padding"""
    args, seed = NETS[net_name]
    bsz, t_len, lengths = GRIDS[grid]
    rag = 0 if lengths is None else 1
    net, params = make_backbone("lynxnet", 128, 1, args, seed)
    x, t, cond = _inputs(bsz, t_len, 21)
    want = _oracle(params, args, x, t, cond, lengths)
    if lengths is not None:
        xp, cp = x.copy(), cond.copy()
        for b, n in enumerate(lengths):
            xp[b, :, :, n:] = np.nan
            cp[b, :, n:] = np.nan
    _set(resident=1)
    for pw2q in _pw2q_values(args):
        first = None
        for pw1p in _pw1_values(args):
            form = (net_name, grid, f"PW1P={pw1p}", f"PW2Q={pw2q}")
            _set(pw1p=pw1p, pw2q=pw2q)
            out = _run(net, x, t, cond, lengths)
            names = _classes(net, x, t, cond, lengths)
            assert _gemm_classes(names) == sorted([_pw1_class(args, pw1p, rag), _pw2_class(args, pw2q, rag)]), (form, names)
            _check(out, want, lengths, form)
            if first is None:
                first = (pw1p, out)
            else:
                for a, b in zip(_items(out, lengths), _items(first[1], lengths)):
                    assert np.array_equal(a, b), (form, f"differs from PW1P={first[0]}")
            if lengths is not None:       # NaN past every item's end: the valid frames do not see it
                poisoned = _run(net, xp, t, cp, lengths)
                _check(poisoned, want, lengths, form + ("NaN padding",))
                for a, b in zip(_items(poisoned, lengths), _items(out, lengths)):
                    assert np.array_equal(a, b), (form, "NaN padding changed valid frames")
    net.release_native()


@pytest.mark.parametrize("net_name,bsz", [("c1024_e2", 1), ("c512_e2", 2)])
def test_natural_t1000_resident_pw1_gemm_pw2_vs_oracle(net_name, bsz):
    """natural_T1000: DSD_LYNX_RESIDENT and DSD_LYNX_PW1P unset, PW2Q=0 - the resident pw1 on the grid's own row-tile choice, pw2
    on gemm.hip's EP_LYNX_NEXT GEMM (too few frame tiles for the 512-row form): the only plan where a LayerNorm partial written by
    the GEMM (layers 1 on) feeds a resident pw1"""
    args, seed = NETS[net_name]
    net, params = make_backbone("lynxnet", 128, 1, args, seed)
    x, t, cond = _inputs(bsz, 1000, 41)
    _set(pw2q=0)
    out = _run(net, x, t, cond, None)
    names = _gemm_classes(_classes(net, x, t, cond, None))
    c = args["num_channels"]
    assert len(names) == 2 and names[1] in (f"lx_pw1_kernel<{c}, 0>", f"lx_pw1p_kernel<{c}, 0>"), names
    assert names[0].startswith("gemm_kernel<0, 1, 7,"), names
    _check(out, _oracle(params, args, x, t, cond, None), None, ("natural T = 1000", net_name, bsz))
    net.release_native()


def test_pw1p_group_count_rejected():
    """DSD_LYNX_PW1P=3 does not divide the 8 row tiles of inner 2048: the call fails on the host, before any launch, naming the
    switch - and the handle runs the next call normally"""
    args, seed = NETS["c1024_e2"]
    net, params = make_backbone("lynxnet", 128, 1, args, seed)
    x, t, cond = _inputs(2, 211, 51)
    _set(resident=1, pw1p=3)
    with pytest.raises(RuntimeError, match="DSD_LYNX_PW1P") as ei:
        _run(net, x, t, cond, None)
    assert isinstance(ei.value, NativeLibraryError)
    for bad in (8, -2):                 # the row-tile count itself (one row tile per group: that is PW1P=0) / below -1
        _set(pw1p=bad)
        with pytest.raises(RuntimeError, match="DSD_LYNX_PW1P"):
            _run(net, x, t, cond, None)
    _set(pw1p=4)
    out = _run(net, x, t, cond, None)
    _check(out, _oracle(params, args, x, t, cond, None), None, ("after a rejected PW1P",))
    net.release_native()


# ------------------------------------------------------------------------------------------------------------------------------
# config 3's own grid: LYNXNet 6 x 1024, k = 31, strong_cond, PReLU; B = 8, T = 1000; no switches
# ------------------------------------------------------------------------------------------------------------------------------
C3 = _net(1024, 2, "PReLU", True, layers=6)


@pytest.mark.parametrize("lengths", [None, [1000, 977, 640, 1, 513, 1000, 33, 800]], ids=["dense", "ragged"])
def test_config3_grid_one_evaluation_vs_oracle(lengths):
    """one evaluation at config 3's grid on the library's own plan: both pointwise GEMMs on lynx_layer.hip (dense: lx_pw1p_kernel
    <1024, 0> with all 8 row tiles per workgroup and lx_pw2d_kernel<4, 0>; ragged: the RAG = 1 forms the rounds pick for its 160
    frame tiles), no gemm.hip pw1 / pw2; against the oracle (~10 s of host time), per item when ragged"""
    net, params = make_backbone("lynxnet", 128, 1, C3, 77)
    x, t, cond = _inputs(8, 1000, 71)
    out = _run(net, x, t, cond, lengths)
    names = _gemm_classes(_classes(net, x, t, cond, lengths))
    if lengths is None:
        assert names == ["lx_pw1p_kernel<1024, 0>", "lx_pw2d_kernel<4, 0>"], names
    else:
        assert len(names) == 2 and names[0].startswith("lx_pw1") and names[1].startswith("lx_pw2"), names
        assert all(n.endswith(", 1>") for n in names), names
    _check(out, _oracle(params, C3, x, t, cond, lengths), lengths, ("config 3 grid", "dense" if lengths is None else "ragged"))
    net.release_native()


def test_config3_ddim_full_grid_vs_oracle():
    """config 3's sampler at its real grid: DDIM (speed-up 200: 5 NFE) on 8 utterances of 1000 frames through the 6 x 1024 net,
    GaussianDiffusion against oracle.diffusion.GaussianDiffusion (~50 s of host time); tolerance TOL_SAMPLER = 1.5e-5"""
    from diffsinger_amd.diffusion import GaussianDiffusion
    set_hp(diff_accelerator="ddim", diff_speedup=200, K_step_infer=1000)
    d = GaussianDiffusion(128, 1, timesteps=1000, k_step=1000, backbone_type="lynxnet", backbone_args=C3,
                          spec_min=[-12.0], spec_max=[0.0])
    params = synth_params("lynxnet", 128, 1, C3, 78)
    load_synth(d.denoise_fn, params)
    d = d.cuda().eval()
    bsz, t_len = 8, 1000
    cond = synth.synth_normal((bsz, t_len, 256), 72)
    noise = synth.synth_normal((bsz, 1, 128, t_len), 73)
    out = d(dev(cond), infer=True, noise=dev(noise))
    fn = lambda x, t, c: ob.lynxnet_forward(params, x, t, c, activation="PReLU", strong_cond=True)   # noqa: E731
    o = od.GaussianDiffusion(fn, 128, 1, spec_min=[-12.0], spec_max=[0.0])
    want = o.forward(cond, noise, diff_accelerator="ddim", diff_speedup=200, K_step_infer=1000)
    check(out, want, TOL_SAMPLER, what="config 3 DDIM 5 NFE, B = 8, T = 1000")
    d.denoise_fn.release_native()
