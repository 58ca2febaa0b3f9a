"""The case table of tests/test_gpu_kernel_ledger.py: one case = one call of one model family at one small shape, under the
path switches that select one kernel form, with the instantiations it is there to run (`targets`, as the launch ledger names
them: kernel<template arguments>, demangled).  A case is credited with everything the ledger counted during its call once its
comparison with the oracle has passed; the targets are what it must have run, so that a case which silently takes another
path fails instead of passing for the wrong reason.

Where the forms come from (api.hip: plan_denoise, make_gemm; the launchers at the end of each kernel file):
  WaveNet layer kernels   wn_layer_kernel<C/64, S, RAG> (DSD_FUSED_LAYER=1), wn_layer16_kernel (DSD_FUSED16=1),
                          wn_layer_x3_kernel<halo, RAG> (fused + bf16x3), the row-split pair as the second segment of a
                          DSD_WN_PLAN=2 plan in its three conv layouts (DSD_RS_CONV_Q=0 / 1 / 2: wn_conv_rs / rq / wq, the
                          Winograd form only up to dilation 8) with wn_out_rs_kernel, the wide row tiles (DSD_RS_ROWS=128 / 256:
                          wn_conv_rw / wn_out_rw<2 | 4>), the three-chunk row-split forms of a one-utterance grid (<3, ..>: T = 1500,
                          no switch, no ragged twin compiled), wn_edge_kernel<C/64, F*M/16, 2, RAG> (DSD_EDGE=1).
                          S = 48 up to dilation 8, 80 at dilation 16: every net here has a cycle of 5.
  LYNXNet                 DSD_LYNX_RESIDENT=1 with DSD_LYNX_PW1P = 0 (lx_pw1_kernel<C>) or a group count (lx_pw1p_kernel<C>) and
                          DSD_LYNX_PW2Q = 0 (lx_pw2d_kernel<inner/512>, inner = 512: lx_pw2_kernel<512>) or 1 (lx_pw2q_kernel<inner/4>);
                          bf16x3: lx_x3_kernel<0 = pw1 | 1 = pw2, K, RAG, 2 | 4 = 32- | 64-frame tiles (DSD_X3_WIDE)>, pw2 only on
                          grids that give it half a chip of workgroups (2 x 1000 frames at C = 1024, 5 x 1000 at C = 512).
  vocoder                 tconv_kernel<C, C, RAG> for the 32- and 16-channel stages, voc_noise_conv_kernel<RAG>,
                          voc_conv_x3_kernel<row blocks per wave (C = 64: 1, 128: 2, 160 / 192: 3, 256: 4), 2 | 4, RAG> (bf16x3).

  gemm.hip                the sections at the end of this file.

Ragged lengths sit on a tile boundary, one frame below and one above it, with a one-frame item; the ragged call follows a dense
call on the same handle, so the tiles it skips hold that call's values and not a fresh arena's zeros."""
from collections import namedtuple

# kind: "wavenet" / "lynxnet": spec = (net, B, T, lengths); "vocoder": spec = (module, tag, B, T, lengths)
Case = namedtuple("Case", "id groups kind spec env precision targets")

KG_GEMM, KG_WAVENET, KG_LYNXNET, KG_VOCODER = 1, 2, 4, 8


def _wn(c, cyc, layers, in_dims, n_feats=1):
    return ("wavenet", in_dims, n_feats, dict(num_layers=layers, num_channels=c, dilation_cycle_length=cyc), 42)


def _lx(c, e, act, strong, layers, seed):
    return ("lynxnet", 128, 1, dict(num_layers=layers, num_channels=c, expansion_factor=e, kernel_size=31, activation=act,
                                    strong_cond=strong), seed)


# name -> (kind, in_dims, n_feats, backbone args, weight seed); hidden size 256 throughout
NETS = {
    "wn256": _wn(256, 5, 5, 64),            # dilations 1, 2, 4, 8, 16
    "wn192": _wn(192, 5, 5, 24, 2),
    "wn128": _wn(128, 5, 5, 80),
    "wn256_mel": _wn(256, 5, 5, 128),
    # the GEMM path of gemm.hip: K = C = 256 (fast, resident up to K = 256), 512 (fast, pipelined), 96 (no multiple of 64: generic);
    # dilations to 32 (S = 48 / 80 / 112 and the generic halos); F*M = 512 / 80: an in-proj with K > 256 / on the generic path
    "wn256_L6": _wn(256, 6, 6, 128),
    "wn512": _wn(512, 5, 5, 128),
    "wn96": _wn(96, 5, 5, 80),
    "wn256_fm512": _wn(256, 1, 1, 512),
    "wn256_L1": _wn(256, 1, 1, 128),
    "wn512_L1": _wn(512, 1, 1, 128),
    "wn96_L1": _wn(96, 1, 1, 80),
    "lx256": _lx(256, 2, "SiLU", False, 2, 65),
    "lx512_L1": _lx(512, 2, "SiLU", False, 1, 67),
    "lx256_L1": _lx(256, 2, "SiLU", False, 1, 68),
    "lx96_L1": _lx(96, 1, "SiLU", False, 1, 69),         # K = C = inner = 96: both pointwise GEMMs and the output GEMM generic
    "lx1024_e2": _lx(1024, 2, "PReLU", True, 3, 61),
    "lx512_e2": _lx(512, 2, "SiLU", False, 3, 62),
    "lx512_e1": _lx(512, 1, "PReLU", False, 3, 64),
    "lx1024_x3": _lx(1024, 2, "PReLU", True, 2, 59),
    "lx512_x3": _lx(512, 2, "SiLU", False, 3, 59),
}
# wn_edge_kernel<C/64, F*M/16, 2, RAG>: every C with every F*M the kernel has (48 = two features of 24 bins)
EDGE_SHAPES = [(c, fm) for c in (128, 192, 256) for fm in (48, 64, 80, 128)]
for _c, _fm in EDGE_SHAPES:
    NETS[f"wn{_c}_fm{_fm}"] = _wn(_c, 3, 3, 24 if _fm == 48 else _fm, 2 if _fm == 48 else 1)

# ConvNeXt aux decoder: name -> (hidden size, mel bins, channels, layers, kernel size, weight seed).  pw1 has K = C, pw2 K = 4 C
AUX_NETS = {
    "aux256": (256, 128, 256, 1, 7, 81),        # pw1 fast and resident, pw2 (K = 1024) fast and pipelined
    "aux64": (256, 128, 64, 1, 7, 82),          # pw2 with K = 256: resident
    "aux512": (256, 128, 512, 1, 7, 83),        # pw1 with K = 512: pipelined
    "aux72": (256, 128, 72, 1, 7, 84),          # K = 72 and 288, no multiples of 64: both generic
}

CASES = []


def _add(cid, groups, kind, spec, env, targets, precision="f32"):
    assert all(c.id != cid for c in CASES), cid
    CASES.append(Case(cid, tuple(groups), kind, spec, dict(env), precision, tuple(targets)))


def _both(cid, groups, kind, dense, ragged, env, targets, precision="f32"):
    """the dense case and its ragged twin: `targets` with {r} for the RAG template argument"""
    for r, spec in ((0, dense), (1, ragged)):
        if spec is not None:
            _add(f"{cid}-{'ragged' if r else 'dense'}", groups, kind, spec, env, [t.format(r=r) for t in targets], precision)


# ------------------------------------------------------------------------------------------------ WaveNet (group 2)
G12 = (KG_GEMM, KG_WAVENET)
_D70, _R70 = (1, 70, None), (3, 70, [64, 65, 1])            # three 32-frame tiles, the last cut at 6 frames
_D96, _R160 = (1, 96, None), (4, 160, [160, 96, 97, 1])     # whole tiles; a mixed plan's boundary inside an item
PLAN2 = dict(DSD_WN_PLAN="2")           # the first half of the tiles on the fused kernel, the rest on the row-split pair


def _wavenet(cid, net, dense, ragged, env, targets, precision="f32", groups=G12):
    _both("wn-" + cid, groups, "wavenet", dense and (net,) + dense, ragged and (net,) + ragged, env, targets, precision)


for _n, _m in (("wn256", 4), ("wn192", 3), ("wn128", 2)):
    _wavenet(f"fused-{_n}", _n, _D70, _R70, dict(DSD_FUSED_LAYER="1"), [f"wn_layer_kernel<{_m}, 48, {{r}}>", f"wn_layer_kernel<{_m}, 80, {{r}}>"])
for _n, _m in (("wn256", 4), ("wn192", 3)):
    _wavenet(f"fused16-{_n}", _n, _D96, _R160, dict(DSD_FUSED16="1"), [f"wn_layer16_kernel<{_m}, 48, {{r}}>", f"wn_layer16_kernel<{_m}, 80, {{r}}>"])
_wavenet("fused-bf16x3", "wn256", _D70, _R70, dict(DSD_FUSED_LAYER="1"), ["wn_layer_x3_kernel<8, {r}>", "wn_layer_x3_kernel<16, {r}>"],
         precision="bf16x3")
_wavenet("pair-halves", "wn256", _D70, _R70, dict(PLAN2, DSD_RS_CONV_Q="0"),
         ["wn_conv_rs_kernel<48, {r}>", "wn_conv_rs_kernel<80, {r}>", "wn_out_rs_kernel<2, {r}>"])
_wavenet("pair-quarters", "wn256", _D70, _R70, dict(PLAN2, DSD_RS_CONV_Q="1"),
         ["wn_conv_rq_kernel<2, 48, 8, {r}>", "wn_conv_rq_kernel<2, 80, 16, {r}>", "wn_out_rs_kernel<2, {r}>"])
_wavenet("pair-winograd", "wn256", _D70, _R70, dict(PLAN2, DSD_RS_CONV_Q="2"),
         ["wn_conv_wq_kernel<1, {r}>", "wn_conv_wq_kernel<2, {r}>", "wn_conv_wq_kernel<4, {r}>", "wn_conv_wq_kernel<8, {r}>"])
for _rows, _m in (("128", 2), ("256", 4)):
    _wavenet(f"rows{_rows}", "wn256", _D70, _R70, dict(DSD_FUSED_LAYER="0", DSD_RS_ROWS=_rows),
             [f"wn_conv_rw_kernel<{_m}, 48, 8, {{r}}>", f"wn_conv_rw_kernel<{_m}, 80, 16, {{r}}>", f"wn_out_rw_kernel<{_m}, {{r}}>"])
# one utterance of 1500 frames, no switch: 47 tiles as the three-chunk row-split pair (no ragged twin is compiled)
_wavenet("one-utterance-T1500", "wn256_mel", (1, 1500, None), None, {},
         ["wn_conv_rq_kernel<3, 80, 8, 0>", "wn_conv_rq_kernel<3, 80, 16, 0>", "wn_out_rs_kernel<3, 0>"])
for _c, _fm in EDGE_SHAPES:
    _wavenet(f"edge-c{_c}-fm{_fm}", f"wn{_c}_fm{_fm}", (2, 77, None), (3, 77, [64, 65, 1]), dict(DSD_EDGE="1"),
             [f"wn_edge_kernel<{_c // 64}, {_fm // 16}, 2, {{r}}>"])

# ------------------------------------------------------------------------------------------------ LYNXNet (group 4)
G14 = (KG_GEMM, KG_LYNXNET)
_LD, _LR = (3, 13, None), (4, 65, [64, 65, 63, 1])          # T below the depthwise half-window; item ends around a tile end


def _lynx(cid, net, dense, ragged, env, targets, precision="f32"):
    _both("lx-" + cid, G14, "lynxnet", dense and (net,) + dense, ragged and (net,) + ragged, dict(env, DSD_LYNX_RESIDENT="1"), targets,
          precision)


_lynx("c512-pw1-pw2d", "lx512_e2", _LD, _LR, dict(DSD_LYNX_PW1P="0", DSD_LYNX_PW2Q="0"), ["lx_pw1_kernel<512, {r}>", "lx_pw2d_kernel<2, {r}>"])
_lynx("c512-pw1p-pw2q", "lx512_e2", _LD, _LR, dict(DSD_LYNX_PW1P="2", DSD_LYNX_PW2Q="1"), ["lx_pw1p_kernel<512, {r}>", "lx_pw2q_kernel<256, {r}>"])
_lynx("c1024-pw1-pw2d", "lx1024_e2", _LD, _LR, dict(DSD_LYNX_PW1P="0", DSD_LYNX_PW2Q="0"), ["lx_pw1_kernel<1024, {r}>", "lx_pw2d_kernel<4, {r}>"])
_lynx("c1024-pw1p-pw2q", "lx1024_e2", _LD, _LR, dict(DSD_LYNX_PW1P="4", DSD_LYNX_PW2Q="1"), ["lx_pw1p_kernel<1024, {r}>", "lx_pw2q_kernel<512, {r}>"])
_lynx("c512-inner512-pw2", "lx512_e1", _LD, _LR, dict(DSD_LYNX_PW1P="0", DSD_LYNX_PW2Q="0"), ["lx_pw1_kernel<512, {r}>", "lx_pw2_kernel<512, {r}>"])
# split-bf16 pw1 on small forced grids: tiles cut inside the first and the second 32-frame half of a 64-frame tile
_XD, _XR = (2, 211, None), (4, 200, [192, 193, 191, 1])
for _net, _c in (("lx512_x3", 512), ("lx1024_x3", 1024)):
    for _wide, _w in (("0", 2), ("1", 4)):
        _lynx(f"c{_c}-x3-pw1-w{_w}", _net, _XD, _XR, dict(DSD_X3_WIDE=_wide), [f"lx_x3_kernel<0, {_c}, {{r}}, {_w}>"], precision="bf16x3")
# ... and both GEMMs on the grids that give pw2 half a chip of workgroups (no switch but the tile width)
for _net, _c, _dense, _ragged in (("lx1024_x3", 1024, (2, 1000, None), (3, 1000, [1000, 961, 1])),
                                  ("lx512_x3", 512, (5, 1000, None), (6, 1000, [1000, 961, 960, 959, 1000, 1]))):
    for _wide, _w in (("0", 2), ("1", 4)):
        _both(f"lx-c{_c}-x3-pw2-w{_w}", G14, "lynxnet", (_net,) + _dense, (_net,) + _ragged, dict(DSD_X3_WIDE=_wide),
              [f"lx_x3_kernel<0, {_c}, {{r}}, {_w}>", f"lx_x3_kernel<1, {2 * _c}, {{r}}, {_w}>"], precision="bf16x3")

# ------------------------------------------------------------------------------------------------ vocoder (group 8)
G18 = (KG_GEMM, KG_VOCODER)
# vocoder_config_cases: k_eq_u has stages of 32 and 16 channels (tconv.hip); x3_c320 one of 160 channels (3 row blocks per wave)
_both("voc-tconv", G18, "vocoder", ("configs", "k_eq_u", 2, 37, None), ("configs", "k_eq_u", 4, 37, "cases"), {},
      ["tconv_kernel<32, 32, {r}>", "tconv_kernel<16, 16, {r}>", "voc_noise_conv_kernel<{r}>"])
for _wide, _w in (("0", 2), ("1", 4)):
    _both(f"voc-x3-c160-w{_w}", G18, "vocoder", ("configs", "x3_c320", 1, 33, None), ("configs", "x3_c320", 4, 37, "cases"),
          dict(DSD_X3_WIDE=_wide), [f"voc_conv_x3_kernel<3, {_w}, {{r}}>"], precision="bf16x3")
    # vocoder_x3_cases, layout A: stages of 256 / 128 / 64 channels (4 / 2 / 1 row blocks per wave)
    _both(f"voc-x3-A-w{_w}", G18, "vocoder", ("x3", "A", 3, 130, None), ("x3", "A", 4, 130, "cases"), dict(DSD_X3_WIDE=_wide),
          [f"voc_conv_x3_kernel<{m}, {_w}, {{r}}>" for m in (1, 2, 4)], precision="bf16x3")

# ------------------------------------------------------------------------------------------------ gemm.hip (group 1)
# gemm_kernel<STAGE, TAPS, EPI, NB, SW, RES, WN, RAG> under the backbones, every layer on the GEMM pair (WaveNet: DSD_ROWSPLIT=0,
# DSD_FUSED_LAYER=0, DSD_EDGE=0; LYNXNet: DSD_LYNX_RESIDENT=0).  make_gemm picks the tile width from the workgroup count
# batch * ceil(T / width) * row tiles: narrow 16-frame tiles (NB 1, SW 16 / 48, WN 1) while 32-frame tiles give at most 192
# workgroups, 64-frame tiles (NB 2) from 512 workgroups, 32-frame tiles between - so the 2C-row GEMMs (conv, out-proj: 8 row
# tiles at C = 256) change over at smaller batches than the C-row ones (4) and the F*M-row output GEMM (2), and a ladder of
# B x 1000 frames (1000 = 31 x 32 + 8 = 15 x 64 + 40: the last tile is cut at either width) walks every GEMM through its widths.
# SW: the fast path's LDS row stride (48 / 80 / 112 by halo; 0 = generic: K no multiple of 64, or a dilation-32 halo); RES 1: all
# K <= 256 resident.  Families: (0,1,0) in-proj and conditioner projection, (1,3,1) FiLM conv + gate, (0,1,2) out-proj with
# residual and skip, (5,1,3) output GEMM on the folded skip sum; a split-bf16 handle keeps the skip projection apart: (3,1,0)
# ST_SCALE skip projection and (0,1,3) output GEMM.  LYNXNet: (0,1,7) in-proj / pw2 with the next layer's transition, (2,1,4)
# LayerNorm -> pw1 -> SwiGLU, (2,1,3) final LayerNorm -> output GEMM.
GEMM_PAIR = dict(DSD_ROWSPLIT="0", DSD_FUSED_LAYER="0", DSD_EDGE="0")
_L8 = [1000, 961, 960, 959, 1, 1000, 33, 800]           # on, above and below a tile end (960 = 30 x 32 = 15 x 64), one frame
_RAGGED = {(3, 70): (3, 70, [64, 65, 1]), (1, 1000): (1, 1000, [961]), (2, 1000): (2, 1000, [1000, 961]),
           (4, 1000): (4, 1000, [1000, 961, 960, 1]), (8, 1000): (8, 1000, _L8), (16, 1000): (16, 1000, _L8 + _L8)}
# (net, B, T, dense / ragged, precision, the forms the case is there for)
GEMM_ROWS = [
    ("wn256_L6", 1, 1000, "r", "f32", ["0, 1, 0, 1, 16, 1, 1, 1", "0, 1, 2, 1, 48, 1, 2, 1", "1, 3, 1, 1, 0, 0, 2, 1", "1, 3, 1, 1, 48, 0, 2, 1", "1, 3, 1, 1, 80, 0, 2, 1", "5, 1, 3, 1, 16, 1, 1, 1"]),
    ("wn256_L6", 2, 1000, "d", "f32", ["0, 1, 0, 1, 16, 0, 1, 0", "0, 1, 0, 1, 16, 1, 1, 0", "0, 1, 0, 1, 48, 1, 2, 0", "0, 1, 0, 2, 80, 0, 2, 0", "0, 1, 2, 1, 48, 1, 2, 0", "1, 3, 1, 1, 0, 0, 2, 0", "1, 3, 1, 1, 48, 0, 2, 0", "1, 3, 1, 1, 80, 0, 2, 0", "5, 1, 3, 1, 16, 1, 1, 0"]),
    ("wn256_L6", 4, 1000, "d", "f32", ["0, 1, 2, 2, 80, 0, 2, 0", "1, 3, 1, 2, 112, 0, 2, 0", "1, 3, 1, 2, 80, 0, 2, 0", "5, 1, 3, 1, 48, 1, 2, 0"]),
    ("wn256_L6", 4, 1000, "r", "f32", ["0, 1, 0, 1, 48, 1, 2, 1", "0, 1, 2, 2, 80, 0, 2, 1", "1, 3, 1, 2, 0, 0, 2, 1", "1, 3, 1, 2, 112, 0, 2, 1", "1, 3, 1, 2, 80, 0, 2, 1", "5, 1, 3, 1, 48, 1, 2, 1"]),
    ("wn512", 1, 1000, "d", "f32", ["0, 1, 2, 1, 48, 0, 2, 0", "5, 1, 3, 1, 16, 0, 1, 0"]),
    ("wn512", 1, 1000, "r", "f32", ["0, 1, 2, 1, 48, 0, 2, 1", "5, 1, 3, 1, 16, 0, 1, 1"]),
    ("wn512", 4, 1000, "d", "f32", ["5, 1, 3, 1, 48, 0, 2, 0"]),
    ("wn512", 4, 1000, "r", "f32", ["5, 1, 3, 1, 48, 0, 2, 1"]),
    ("wn96", 1, 70, "d", "f32", ["5, 1, 3, 1, 0, 0, 2, 0"]),
    ("wn96", 3, 70, "r", "f32", ["5, 1, 3, 1, 0, 0, 2, 1"]),
    ("wn256_fm512", 3, 70, "r", "f32", ["0, 1, 0, 1, 16, 0, 1, 1"]),
    ("wn256_fm512", 4, 1000, "d", "f32", ["0, 1, 0, 1, 48, 0, 2, 0", "5, 1, 3, 2, 80, 0, 2, 0"]),
    ("wn256_fm512", 4, 1000, "r", "f32", ["0, 1, 0, 1, 48, 0, 2, 1", "5, 1, 3, 2, 80, 0, 2, 1"]),
    ("wn256_L1", 1, 70, "d", "bf16x3", ["0, 1, 2, 1, 16, 1, 1, 0", "0, 1, 3, 1, 16, 1, 1, 0", "1, 3, 1, 1, 48, 0, 1, 0", "3, 1, 0, 1, 16, 1, 1, 0"]),
    ("wn256_L1", 3, 70, "r", "bf16x3", ["0, 1, 2, 1, 16, 1, 1, 1", "0, 1, 3, 1, 16, 1, 1, 1", "1, 3, 1, 1, 48, 0, 1, 1", "3, 1, 0, 1, 16, 1, 1, 1"]),
    ("wn256_L1", 2, 1000, "r", "bf16x3", ["3, 1, 0, 1, 48, 1, 2, 1"]),
    ("wn256_L1", 4, 1000, "d", "bf16x3", ["0, 1, 3, 1, 48, 1, 2, 0", "3, 1, 0, 1, 48, 1, 2, 0"]),
    ("wn256_L1", 8, 1000, "r", "bf16x3", ["0, 1, 0, 2, 80, 0, 2, 1", "0, 1, 3, 1, 48, 1, 2, 1", "3, 1, 0, 2, 80, 0, 2, 1"]),
    ("wn256_L1", 16, 1000, "d", "bf16x3", ["0, 1, 3, 2, 80, 0, 2, 0", "3, 1, 0, 2, 80, 0, 2, 0"]),
    ("wn256_L1", 16, 1000, "r", "bf16x3", ["0, 1, 3, 2, 80, 0, 2, 1"]),
    ("wn512_L1", 1, 70, "d", "bf16x3", ["0, 1, 2, 1, 16, 0, 1, 0", "0, 1, 3, 1, 16, 0, 1, 0", "3, 1, 0, 1, 16, 0, 1, 0"]),
    ("wn512_L1", 3, 70, "r", "bf16x3", ["0, 1, 2, 1, 16, 0, 1, 1", "0, 1, 3, 1, 16, 0, 1, 1", "3, 1, 0, 1, 16, 0, 1, 1"]),
    ("wn512_L1", 1, 1000, "d", "bf16x3", ["3, 1, 0, 1, 48, 0, 2, 0"]),
    ("wn512_L1", 1, 1000, "r", "bf16x3", ["3, 1, 0, 1, 48, 0, 2, 1"]),
    ("wn512_L1", 4, 1000, "d", "bf16x3", ["0, 1, 3, 1, 48, 0, 2, 0"]),
    ("wn512_L1", 4, 1000, "r", "bf16x3", ["0, 1, 3, 1, 48, 0, 2, 1"]),
    ("wn96_L1", 1, 70, "d", "bf16x3", ["0, 1, 2, 1, 0, 0, 2, 0", "0, 1, 3, 1, 0, 0, 2, 0", "3, 1, 0, 1, 0, 0, 2, 0"]),
    ("wn96_L1", 3, 70, "r", "bf16x3", ["0, 1, 0, 1, 0, 0, 2, 1", "0, 1, 2, 1, 0, 0, 2, 1", "0, 1, 3, 1, 0, 0, 2, 1", "3, 1, 0, 1, 0, 0, 2, 1"]),
    ("wn96_L1", 16, 1000, "d", "bf16x3", ["0, 1, 0, 1, 0, 0, 2, 0", "0, 1, 0, 2, 0, 0, 2, 0", "0, 1, 2, 2, 0, 0, 2, 0", "0, 1, 3, 2, 0, 0, 2, 0", "1, 3, 1, 2, 0, 0, 2, 0", "3, 1, 0, 2, 0, 0, 2, 0"]),
    ("wn96_L1", 16, 1000, "r", "bf16x3", ["0, 1, 0, 2, 0, 0, 2, 1", "0, 1, 2, 2, 0, 0, 2, 1", "0, 1, 3, 2, 0, 0, 2, 1", "3, 1, 0, 2, 0, 0, 2, 1"]),
    ("wn96_L1", 16, 1000, "d", "f32", ["5, 1, 3, 2, 0, 0, 2, 0"]),
    ("wn96_L1", 16, 1000, "r", "f32", ["5, 1, 3, 2, 0, 0, 2, 1"]),
    ("lx256", 1, 70, "d", "f32", ["0, 1, 7, 1, 48, 0, 2, 0", "2, 1, 3, 1, 48, 1, 2, 0", "2, 1, 4, 1, 48, 1, 2, 0"]),
    ("lx256", 3, 70, "r", "f32", ["0, 1, 7, 1, 48, 0, 2, 1", "2, 1, 3, 1, 48, 1, 2, 1", "2, 1, 4, 1, 48, 1, 2, 1"]),
    ("lx512_L1", 1, 70, "d", "f32", ["2, 1, 4, 1, 48, 0, 2, 0"]),
    ("lx512_L1", 3, 70, "r", "f32", ["2, 1, 4, 1, 48, 0, 2, 1"]),
    ("lx512_L1", 4, 1000, "d", "f32", ["0, 1, 7, 2, 80, 0, 2, 0", "2, 1, 3, 1, 48, 0, 2, 0", "2, 1, 4, 2, 80, 0, 2, 0"]),
    ("lx512_L1", 4, 1000, "r", "f32", ["0, 1, 7, 2, 80, 0, 2, 1", "2, 1, 3, 1, 48, 0, 2, 1", "2, 1, 4, 2, 80, 0, 2, 1"]),
    ("lx256_L1", 16, 1000, "d", "f32", ["2, 1, 3, 2, 80, 0, 2, 0"]),
    ("lx256_L1", 16, 1000, "r", "f32", ["2, 1, 3, 2, 80, 0, 2, 1"]),
    ("lx96_L1", 1, 70, "d", "f32", ["2, 1, 4, 1, 0, 0, 2, 0", "0, 1, 7, 1, 0, 0, 2, 0", "2, 1, 3, 1, 0, 0, 2, 0"]),
    ("lx96_L1", 3, 70, "r", "f32", ["2, 1, 4, 1, 0, 0, 2, 1", "0, 1, 7, 1, 0, 0, 2, 1", "2, 1, 3, 1, 0, 0, 2, 1"]),
    ("lx96_L1", 16, 1000, "d", "f32", ["2, 1, 4, 2, 0, 0, 2, 0", "0, 1, 7, 2, 0, 0, 2, 0", "2, 1, 3, 2, 0, 0, 2, 0"]),
    ("lx96_L1", 16, 1000, "r", "f32", ["2, 1, 4, 2, 0, 0, 2, 1", "0, 1, 7, 2, 0, 0, 2, 1", "2, 1, 3, 2, 0, 0, 2, 1"]),
]
for _net, _b, _t, _dr, _prec, _forms in GEMM_ROWS:
    _kind = NETS[_net][0]
    _add(f"gemm-{_net}-{_b}x{_t}-{'ragged' if _dr == 'r' else 'dense'}-{_prec}", (KG_GEMM,), _kind,
         (_net,) + (_RAGGED[(_b, _t)] if _dr == "r" else (_b, _t, None)), GEMM_PAIR if _kind == "wavenet" else dict(DSD_LYNX_RESIDENT="0"),
         [f"gemm_kernel<{f}>" for f in _forms], _prec)

# the ConvNeXt aux decoder (dsd_aux_decode): (0,0,0) the k = 7 input conv and the output conv, (2,1,0) LayerNorm -> pw1 -> GELU,
# (0,1,5) pw2 + layer scale + residual, on the same ladder of grids (64-frame tiles from 4 x 1000 frames at C = 512)
AUX_ROWS = [
    ("aux256", 1, 70, "d", ["0, 1, 5, 1, 16, 0, 1, 0", "2, 1, 0, 1, 48, 1, 2, 0"]),
    ("aux256", 1, 1000, "r", ["0, 1, 5, 1, 16, 0, 1, 1", "2, 1, 0, 1, 48, 1, 2, 1"]),
    ("aux64", 1, 70, "d", ["0, 1, 5, 1, 16, 1, 1, 0"]),
    ("aux64", 1, 1000, "r", ["0, 1, 5, 1, 16, 1, 1, 1"]),
    ("aux64", 8, 1000, "d", ["0, 1, 5, 1, 48, 1, 2, 0"]),
    ("aux64", 8, 1000, "r", ["0, 1, 5, 1, 48, 1, 2, 1"]),
    ("aux512", 1, 70, "d", ["2, 1, 0, 1, 48, 0, 2, 0"]),
    ("aux512", 3, 70, "r", ["2, 1, 0, 1, 48, 0, 2, 1"]),
    ("aux512", 4, 1000, "d", ["0, 0, 0, 2, 0, 0, 2, 0", "0, 1, 5, 2, 80, 0, 2, 0", "2, 1, 0, 2, 80, 0, 2, 0"]),
    ("aux512", 4, 1000, "r", ["0, 0, 0, 2, 0, 0, 2, 1", "0, 1, 5, 2, 80, 0, 2, 1", "2, 1, 0, 2, 80, 0, 2, 1"]),
    ("aux72", 4, 1000, "d", ["0, 1, 5, 1, 48, 0, 2, 0", "2, 1, 0, 1, 0, 0, 2, 0"]),
    ("aux72", 4, 1000, "r", ["0, 1, 5, 1, 48, 0, 2, 1", "2, 1, 0, 1, 0, 0, 2, 1"]),
    ("aux72", 8, 1000, "d", ["2, 1, 0, 2, 0, 0, 2, 0"]),
    ("aux72", 8, 1000, "r", ["2, 1, 0, 2, 0, 0, 2, 1"]),
]
for _net, _b, _t, _dr, _forms in AUX_ROWS:
    _add(f"gemm-{_net}-{_b}x{_t}-{'ragged' if _dr == 'r' else 'dense'}", (KG_GEMM,), "aux",
         (_net,) + (_RAGGED[(_b, _t)] if _dr == "r" else (_b, _t, None)), {}, [f"gemm_kernel<{f}>" for f in _forms])
# NSF-HiFiGAN with ResBlock2 at widths 48 / 24 / 12: leaky-ReLU staged convs with the residual epilogue, on the GEMM path
_both("gemm-voc-resblock2", (KG_GEMM,), "vocoder", ("configs", "odd_rates", 2, 37, None), ("configs", "odd_rates", 4, 37, "cases"), {},
      ["gemm_kernel<4, 0, 5, 1, 0, 0, 2, {r}>", "gemm_kernel<4, 0, 6, 1, 0, 0, 2, {r}>", "gemm_kernel<4, 0, 0, 1, 0, 0, 2, {r}>"])
# ... and with ResBlock1 at kernel size 1 (widths 192 / 96 / 48, fp32): its second conv is the 1x1 EP_BIAS_RES form on the generic path -
# the only ragged call that reaches it (the aux decoder's pw2 has K = 4 C, a multiple of 128: always the fast path)
_both("gemm-voc-resblock1-k1", (KG_GEMM,), "vocoder", ("configs", "x3_c384", 1, 33, None), ("configs", "x3_c384", 4, 37, "cases"), {},
      ["gemm_kernel<0, 1, 5, 1, 0, 0, 2, {r}>"])
# 64-frame tiles (NB = 2) on the vocoder's generic path: make_gemm counts batch * ceil(T_stage / 64) * row tiles >= 512 at the stage's own
# rate (a ragged call: its valid tiles), and a thin late stage has one row tile but T * upp samples.  max_counts (ResBlock1, kernel
# sizes 1 .. 15, upp 256, last widths 4 / 2): 2 x 128 frames are 2 x 256 tiles at the last transposed conv and 2 x 512 at the last
# stage's convs and conv_post; ragged: 256 + 254 + 192 + 2 = 704 and twice that.  odd_rates (ResBlock2, upp 30, last width 12): 8 x 280
# frames are 8 x 66 tiles at the last transposed conv's input rate (15); ragged lengths 279 / 256 / 1: 256 x 15 = 60 x 64 sits on a tile
# end.  thin (widths 24 .. 3, upp 16): 8 x 260 frames are 8 x 65 tiles; 257 / 256 / 1: one frame past a tile end, on it, one frame.
_both("gemm-voc-resblock1-64", (KG_GEMM,), "vocoder", ("configs", "max_counts", 2, 128, None), ("configs", "max_counts", 4, 128, [128, 127, 96, 1]), {},
      ["gemm_kernel<0, 1, 5, 2, 0, 0, 2, {r}>", "gemm_kernel<0, 0, 5, 2, 0, 0, 2, {r}>", "gemm_kernel<4, 0, 0, 2, 0, 0, 2, {r}>",
       "gemm_kernel<4, 0, 6, 2, 0, 0, 2, {r}>"])
_both("gemm-voc-resblock2-64", (KG_GEMM,), "vocoder", ("configs", "odd_rates", 8, 280, None),
      ("configs", "odd_rates", 10, 280, [280] * 7 + [279, 256, 1]), {},
      ["gemm_kernel<4, 0, 5, 2, 0, 0, 2, {r}>", "gemm_kernel<4, 0, 0, 2, 0, 0, 2, {r}>", "gemm_kernel<4, 0, 6, 2, 0, 0, 2, {r}>"])
_both("gemm-voc-thin-64", (KG_GEMM,), "vocoder", ("configs", "thin", 8, 260, None), ("configs", "thin", 10, 260, [260] * 7 + [257, 256, 1]), {},
      ["gemm_kernel<0, 0, 5, 2, 0, 0, 2, {r}>", "gemm_kernel<4, 0, 0, 2, 0, 0, 2, {r}>"])
