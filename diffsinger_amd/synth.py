"""Deterministic synthetic weights and inputs (numpy only).

There are no checkpoints in the build container or on the GPU box, so every
test, fixture and benchmark regenerates its weights from a seed.  The state
dict names and shapes are exactly those of the reference modules
(`modules/backbones/wavenet.py:22-31,56-72`, `modules/backbones/lynxnet.py:52-62,
71-74,104-124`), so the same dict loads with `strict=True` into the reference
`WaveNet` / `LYNXNet`, into this package's shims and into the numpy oracle.

`output_projection.weight` is zero-initialised by the reference
(`wavenet.py:73`, `lynxnet.py:126`); here it gets fan-in scaled normals like
every other layer, otherwise the network output would be its bias only.
"""
from __future__ import annotations

import hashlib
from collections import OrderedDict

import numpy as np


def wavenet_param_shapes(in_dims, n_feats, num_layers=20, num_channels=256, hidden_size=256):
    c, m, h = num_channels, in_dims * n_feats, hidden_size
    shapes = OrderedDict()
    shapes["input_projection.weight"] = (c, m, 1)
    shapes["input_projection.bias"] = (c,)
    shapes["mlp.0.weight"] = (4 * c, c)
    shapes["mlp.0.bias"] = (4 * c,)
    shapes["mlp.2.weight"] = (c, 4 * c)
    shapes["mlp.2.bias"] = (c,)
    for l in range(num_layers):
        p = f"residual_layers.{l}."
        shapes[p + "dilated_conv.weight"] = (2 * c, c, 3)
        shapes[p + "dilated_conv.bias"] = (2 * c,)
        shapes[p + "diffusion_projection.weight"] = (c, c)
        shapes[p + "diffusion_projection.bias"] = (c,)
        shapes[p + "conditioner_projection.weight"] = (2 * c, h, 1)
        shapes[p + "conditioner_projection.bias"] = (2 * c,)
        shapes[p + "output_projection.weight"] = (2 * c, c, 1)
        shapes[p + "output_projection.bias"] = (2 * c,)
    shapes["skip_projection.weight"] = (c, c, 1)
    shapes["skip_projection.bias"] = (c,)
    shapes["output_projection.weight"] = (m, c, 1)
    shapes["output_projection.bias"] = (m,)
    return shapes


def lynxnet_param_shapes(in_dims, n_feats, num_layers=6, num_channels=512, expansion_factor=2,
                         kernel_size=31, activation="PReLU", hidden_size=256):
    c, m, h = num_channels, in_dims * n_feats, hidden_size
    inner = c * expansion_factor
    shapes = OrderedDict()
    shapes["input_projection.weight"] = (c, m, 1)
    shapes["input_projection.bias"] = (c,)
    shapes["diffusion_embedding.1.weight"] = (4 * c, c)
    shapes["diffusion_embedding.1.bias"] = (4 * c,)
    shapes["diffusion_embedding.3.weight"] = (c, 4 * c)
    shapes["diffusion_embedding.3.bias"] = (c,)
    for l in range(num_layers):
        p = f"residual_layers.{l}."
        shapes[p + "diffusion_projection.weight"] = (c, c, 1)
        shapes[p + "diffusion_projection.bias"] = (c,)
        shapes[p + "conditioner_projection.weight"] = (c, h, 1)
        shapes[p + "conditioner_projection.bias"] = (c,)
        shapes[p + "convmodule.net.0.weight"] = (c,)
        shapes[p + "convmodule.net.0.bias"] = (c,)
        shapes[p + "convmodule.net.2.weight"] = (2 * inner, c, 1)
        shapes[p + "convmodule.net.2.bias"] = (2 * inner,)
        shapes[p + "convmodule.net.4.weight"] = (inner, 1, kernel_size)
        shapes[p + "convmodule.net.4.bias"] = (inner,)
        if activation == "PReLU":
            shapes[p + "convmodule.net.5.weight"] = (inner,)
        shapes[p + "convmodule.net.6.weight"] = (c, inner, 1)
        shapes[p + "convmodule.net.6.bias"] = (c,)
    shapes["norm.weight"] = (c,)
    shapes["norm.bias"] = (c,)
    shapes["output_projection.weight"] = (m, c, 1)
    shapes["output_projection.bias"] = (m,)
    return shapes


def convnext_param_shapes(in_dims, out_dims, num_channels=512, num_layers=6, kernel_size=7, prefix=""):
    """state_dict of modules/aux_decoder/convnext.py:58-76 (ConvNeXtDecoder); `prefix="decoder."` gives the
    AuxDecoderAdaptor layout (aux_decoder/__init__.py:33-37)."""
    c = num_channels
    shapes = OrderedDict()
    shapes[prefix + "inconv.weight"] = (c, in_dims, kernel_size)
    shapes[prefix + "inconv.bias"] = (c,)
    for l in range(num_layers):
        p = f"{prefix}conv.{l}."
        shapes[p + "gamma"] = (c,)
        shapes[p + "dwconv.weight"] = (c, 1, 7)
        shapes[p + "dwconv.bias"] = (c,)
        shapes[p + "norm.weight"] = (c,)
        shapes[p + "norm.bias"] = (c,)
        shapes[p + "pwconv1.weight"] = (4 * c, c)
        shapes[p + "pwconv1.bias"] = (4 * c,)
        shapes[p + "pwconv2.weight"] = (c, 4 * c)
        shapes[p + "pwconv2.bias"] = (c,)
    shapes[prefix + "outconv.weight"] = (out_dims, c, kernel_size)
    shapes[prefix + "outconv.bias"] = (out_dims,)
    return shapes


def fs2_acoustic_param_shapes(vocab_size, hidden_size=256, enc_layers=4, num_heads=2, ffn_kernel_size=3,
                              num_spk=0, num_lang=0, variances=(), key_shift=False, speed=False, rope=True, sinpos=False,
                              ffn_act="gelu"):
    """state_dict of modules/fastspeech/acoustic_encoder.py:14-63 (FastSpeech2Acoustic) in its rotary-embedding
    configuration (`use_rope: true`): tts_modules.py:353-383, common_layers.py:120-234.  The rotary frequency
    table is an (untrained) nn.Parameter of the shared RotaryEmbedding and shows up once per layer.  `rope=False`:
    the pre-rotary layout, torch.nn.MultiheadAttention(bias=False) (common_layers.py:222-226)."""
    h = hidden_size
    shapes = OrderedDict()
    shapes["txt_embed.weight"] = (vocab_size, h)
    if num_lang:
        shapes["lang_embed.weight"] = (num_lang + 1, h)
    shapes["dur_embed.weight"] = (h, 1)
    shapes["dur_embed.bias"] = (h,)
    for l in range(enc_layers):
        p = f"encoder.layers.{l}.op."
        shapes[p + "layer_norm1.weight"] = (h,)
        shapes[p + "layer_norm1.bias"] = (h,)
        if rope:
            shapes[p + "self_attn.in_proj.weight"] = (3 * h, h)
            shapes[p + "self_attn.out_proj.weight"] = (h, h)
            shapes[p + "self_attn.rotary_embed.freqs"] = (h // num_heads // 2,)
        else:
            shapes[p + "self_attn.in_proj_weight"] = (3 * h, h)
            shapes[p + "self_attn.out_proj.weight"] = (h, h)
        shapes[p + "layer_norm2.weight"] = (h,)
        shapes[p + "layer_norm2.bias"] = (h,)
        f1 = (8 if ffn_act == "swiglu" else 4) * h          # SwiGLU: out and gate halves (common_layers.py:132-134)
        shapes[p + "ffn.ffn_1.weight"] = (f1, h, ffn_kernel_size)
        shapes[p + "ffn.ffn_1.bias"] = (f1,)
        shapes[p + "ffn.ffn_2.weight"] = (h, 4 * h)
        shapes[p + "ffn.ffn_2.bias"] = (h,)
    shapes["encoder.layer_norm.weight"] = (h,)
    shapes["encoder.layer_norm.bias"] = (h,)
    if sinpos:       # SinusoidalPositionalEmbedding's marker buffer (common_layers.py:59): a value nobody reads
        shapes["encoder.embed_positions._float_tensor"] = (1,)
    shapes["pitch_embed.weight"] = (h, 1)
    shapes["pitch_embed.bias"] = (h,)
    for v in variances:
        shapes[f"variance_embeds.{v}.weight"] = (h, 1)
        shapes[f"variance_embeds.{v}.bias"] = (h,)
    if key_shift:
        shapes["key_shift_embed.weight"] = (h, 1)
        shapes["key_shift_embed.bias"] = (h,)
    if speed:
        shapes["speed_embed.weight"] = (h, 1)
        shapes["speed_embed.bias"] = (h,)
    if num_spk:
        shapes["spk_embed.weight"] = (num_spk, h)
    return shapes


NSF_HIFIGAN_DEFAULT = dict(       # the openvpi 44.1 kHz / hop 512 NSF-HiFiGAN layout (config.json ships with the checkpoint)
    sampling_rate=44100, num_mels=128, hop_size=512, upsample_rates=[8, 8, 2, 2, 2],
    upsample_kernel_sizes=[16, 16, 4, 4, 4], upsample_initial_channel=512, resblock="1",
    resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]], mini_nsf=False,
    noise_sigma=0.0)


def nsf_hifigan_param_shapes(h):
    """state_dict of modules/nsf_hifigan/models.py:207-260 (Generator, mini_nsf = False) in its inference form,
    i.e. after `remove_weight_norm()`: plain `weight` / `bias` everywhere."""
    shapes = OrderedDict()
    mini = bool(h.get("mini_nsf", False))
    if not mini:
        shapes["m_source.l_linear.weight"] = (1, int(h.get("harmonic_num", 8)) + 1)      # optional key, the reference's 8
        shapes["m_source.l_linear.bias"] = (1,)
    ch = h["upsample_initial_channel"]
    rates = list(h["upsample_rates"])
    noise = OrderedDict()
    ups = OrderedDict()
    res = OrderedDict()
    nk = len(h["resblock_kernel_sizes"])
    for i, (u, k) in enumerate(zip(rates, h["upsample_kernel_sizes"])):
        ch //= 2
        ups[f"ups.{i}.weight"] = (2 * ch, ch, k)
        ups[f"ups.{i}.bias"] = (ch,)
        for j, (rk, rd) in enumerate(zip(h["resblock_kernel_sizes"], h["resblock_dilation_sizes"])):
            pre = f"resblocks.{i * nk + j}."
            if str(h.get("resblock", "1")) == "1":
                for grp in ("convs1", "convs2"):
                    for d in range(len(rd)):
                        res[f"{pre}{grp}.{d}.weight"] = (ch, ch, rk)
                        res[f"{pre}{grp}.{d}.bias"] = (ch,)
            else:
                for d in range(len(rd)):
                    res[f"{pre}convs.{d}.weight"] = (ch, ch, rk)
                    res[f"{pre}convs.{d}.bias"] = (ch,)
        if mini:
            if i == 1:
                noise["source_conv.weight"] = (ch, 1, 1)
                noise["source_conv.bias"] = (ch,)
        else:
            if i + 1 < len(rates):
                sf = int(np.prod(rates[i + 1:]))
                noise[f"noise_convs.{i}.weight"] = (ch, 1, sf * 2)
            else:
                noise[f"noise_convs.{i}.weight"] = (ch, 1, 1)
            noise[f"noise_convs.{i}.bias"] = (ch,)
    shapes.update(noise)
    shapes["conv_pre.weight"] = (h["upsample_initial_channel"], h["num_mels"], 7)
    shapes["conv_pre.bias"] = (h["upsample_initial_channel"],)
    shapes.update(ups)
    shapes.update(res)
    shapes["conv_post.weight"] = (1, ch, 7)
    shapes["conv_post.bias"] = (1,)
    return shapes


def backbone_param_shapes(kind, in_dims, n_feats, hidden_size=256, **args):
    if kind == "wavenet":
        return wavenet_param_shapes(in_dims, n_feats, num_layers=args.get("num_layers", 20),
                                    num_channels=args.get("num_channels", 256), hidden_size=hidden_size)
    if kind == "lynxnet":
        return lynxnet_param_shapes(in_dims, n_feats, num_layers=args.get("num_layers", 6),
                                    num_channels=args.get("num_channels", 512),
                                    expansion_factor=args.get("expansion_factor", 2),
                                    kernel_size=args.get("kernel_size", 31),
                                    activation=args.get("activation", "PReLU") or "PReLU",
                                    hidden_size=hidden_size)
    raise KeyError(kind)


def synth_state_dict(shapes, seed=42, gain=1.0):
    """name -> float32 ndarray.  Fan-in scaled normals for matrices (times `gain`: < 1 keeps deep residual stacks
    such as the vocoder's in the O(1) range), N(0, 0.1) biases, LayerNorm gains around 1, PReLU slopes around 0.25."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = OrderedDict()
    for name, shape in shapes.items():
        z = rng.standard_normal(shape, dtype=np.float32)
        leaf = name.rsplit(".", 1)[-1]
        is_ln = (name.startswith("norm.") or ".convmodule.net.0." in name or ".norm." in name
                 or ".layer_norm" in name)
        if is_ln and leaf == "weight":
            w = 1.0 + 0.1 * z
        elif ".convmodule.net.5." in name:
            w = 0.25 + 0.05 * z
        elif leaf == "freqs":                      # rotary table: the reference's own values (rotary_embedding_torch.py:119)
            d = 2 * shape[0]
            w = (1.0 / (10000.0 ** (np.arange(0, d, 2, dtype=np.float32) / np.float32(d)))).astype(np.float32)
        elif name.endswith("_embed.weight") and len(shape) == 2 and shape[1] > 1 and "variance" not in name:
            w = z / np.sqrt(np.float32(shape[1]))      # embedding tables: N(0, H^-0.5) (common_layers.py:24)
            if name.startswith(("txt_embed", "lang_embed")):
                w[0] = 0.0                             # padding_idx row
        elif leaf == "gamma":                      # ConvNeXt layer scale (reference init 1e-6; O(1) here so it matters)
            w = 0.5 + 0.1 * z
        elif leaf == "bias":
            w = 0.1 * z
        else:
            fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else shape[0]
            w = np.float32(gain) * z / np.sqrt(np.float32(fan_in))
        out[name] = np.ascontiguousarray(w, dtype=np.float32)
    return out


def state_dict_digest(sd):
    h = hashlib.sha256()
    for name, arr in sd.items():
        h.update(name.encode())
        h.update(np.ascontiguousarray(arr, dtype=np.float32).tobytes())
    return h.hexdigest()


def synth_normal(shape, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.standard_normal(shape, dtype=np.float32)


def rmvpe_param_shapes(n_blocks=4, n_gru=1, en_de_layers=5, inter_layers=4, en_out_channels=16, with_tf=False):
    """The state_dict of E2E0(n_blocks, n_gru, (2, 2), en_de_layers, inter_layers, 1, en_out_channels)
    (modules/pe/rmvpe/model.py): name -> shape, `num_batches_tracked` as () and, with `with_tf`, the TimbreFilter
    (`unet.tf.*`) the checkpoint carries but forward never calls.  The defaults are the production RMVPE."""
    shapes = OrderedDict()

    def bn(p, c):
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            shapes[f"{p}.{leaf}"] = (c,)
        shapes[f"{p}.num_batches_tracked"] = ()

    def block(p, cin, cout):
        shapes[f"{p}.conv.0.weight"] = (cout, cin, 3, 3)
        bn(f"{p}.conv.1", cout)
        shapes[f"{p}.conv.3.weight"] = (cout, cout, 3, 3)
        bn(f"{p}.conv.4", cout)
        if cin != cout:
            shapes[f"{p}.shortcut.weight"] = (cout, cin, 1, 1)
            shapes[f"{p}.shortcut.bias"] = (cout,)

    E, C = en_de_layers, en_out_channels
    bn("unet.encoder.bn", 1)
    for l in range(E):
        cin, cout = (1 if l == 0 else C << (l - 1)), C << l
        for k in range(n_blocks):
            block(f"unet.encoder.layers.{l}.conv.{k}", cout if k else cin, cout)
    for i in range(inter_layers):
        cin, cout = (C << (E - 1) if i == 0 else C << E), C << E
        for k in range(n_blocks):
            block(f"unet.intermediate.layers.{i}.conv.{k}", cout if k else cin, cout)
    if with_tf:
        for l in range(E):
            block(f"unet.tf.layers.{l}", C << l, C << l)
    for i in range(E):
        cin = C << (E - i)
        cout = cin // 2
        shapes[f"unet.decoder.layers.{i}.conv1.0.weight"] = (cin, cout, 3, 3)
        bn(f"unet.decoder.layers.{i}.conv1.1", cout)
        for k in range(n_blocks):
            block(f"unet.decoder.layers.{i}.conv2.{k}", cout if k else 2 * cout, cout)
    shapes["cnn.weight"] = (3, C, 3, 3)
    shapes["cnn.bias"] = (3,)
    if n_gru:
        for sfx in ("", "_reverse"):
            shapes[f"fc.0.gru.weight_ih_l0{sfx}"] = (768, 384)
            shapes[f"fc.0.gru.weight_hh_l0{sfx}"] = (768, 256)
            shapes[f"fc.0.gru.bias_ih_l0{sfx}"] = (768,)
            shapes[f"fc.0.gru.bias_hh_l0{sfx}"] = (768,)
        shapes["fc.1.weight"] = (360, 512)
        shapes["fc.1.bias"] = (360,)
    else:
        shapes["fc.0.weight"] = (360, 384)
        shapes["fc.0.bias"] = (360,)
    return shapes


RMVPE_SMALL = dict(n_blocks=1, n_gru=1, en_de_layers=5, inter_layers=1, en_out_channels=16)


def rmvpe_state_dict(seed=1800, with_tf=False, **cfg):
    """Seeded synthetic RMVPE weights (float32; num_batches_tracked int64 0) whose sigmoid output is non-degenerate on the
    test signals: voiced and unvoiced frames, the frame maximum on both sides of thred = 0.03, argmax spread over the 360
    classes.  Statistics:
      conv weights         N(0, 2 / fan_in) (He), the second conv of every ConvBlockRes and the shortcut times 0.5
      BatchNorm            weight 1 + 0.1 N, bias 0.1 N, running_mean 0.1 N, running_var 1 + 0.25 U(0, 1); the input
                           BatchNorm: running_mean -5, running_var 9 (log-mel values of -11.5 .. 2 come out as O(1))
      cnn                  N(0, 1 / fan_in), bias 0.1 N
      GRU                  weights U(-1, 1) / 16 (torch's init: U(-1 / sqrt(256), 1 / sqrt(256))), biases the same
      fc (Linear -> 360)   N(0, 9 / fan_in), bias -6 + 0.5 N (sigmoid(-6) = 0.0025 < 0.03)"""
    shapes = rmvpe_param_shapes(with_tf=with_tf, **cfg)
    rng = np.random.Generator(np.random.PCG64(seed))
    out = OrderedDict()
    for name, shape in shapes.items():
        leaf = name.rsplit(".", 1)[-1]
        if leaf == "num_batches_tracked":
            out[name] = np.zeros((), dtype=np.int64)
            continue
        z = rng.standard_normal(shape)
        fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else shape[0]
        is_bn = len(shape) == 1 and leaf in ("weight", "bias", "running_mean", "running_var") and not name.startswith(("cnn", "fc"))
        is_bn = is_bn and not name.endswith(("shortcut.bias",))
        if name.startswith("unet.encoder.bn."):
            w = {"weight": 1.0 + 0.1 * z, "bias": 0.1 * z, "running_mean": np.full(shape, -5.0),
                 "running_var": np.full(shape, 9.0)}[leaf]
        elif is_bn:
            w = {"weight": 1.0 + 0.1 * z, "bias": 0.1 * z, "running_mean": 0.1 * z,
                 "running_var": 1.0 + 0.25 * rng.uniform(0, 1, shape)}[leaf]
        elif name.startswith("fc.0.gru."):
            w = rng.uniform(-1, 1, shape) / 16.0
        elif name.startswith("fc."):
            w = (-6.0 + 0.5 * z) if leaf == "bias" else 3.0 * z / np.sqrt(fan_in)
        elif name.startswith("cnn."):
            w = 0.1 * z if leaf == "bias" else z / np.sqrt(fan_in)
        elif leaf == "bias":
            w = 0.1 * z
        else:
            w = np.sqrt(2.0 / fan_in) * z
            if ".conv.3." in name or ".shortcut." in name:
                w = 0.5 * w
        out[name] = np.ascontiguousarray(w, dtype=np.float32)
    return out


HNSEP_SMALL = dict(n_fft=512, hop_length=128, nout=8, nout_lstm=16, is_mono=True)
HNSEP_PROD = dict(n_fft=2048, hop_length=512, nout=32, nout_lstm=128, is_mono=True)


def hnsep_state_dict(cfg=None, seed=1900, out_scale=0.5):
    """Seeded synthetic CascadedNet weights (float32; num_batches_tracked int64 0) for the layout `cfg` (CascadedNet's
    arguments).  Statistics:
      conv weights   N(0, 2 / fan_in) (He)
      BatchNorm      weight 1 + 0.1 N, bias 0.1 N, running_mean 0.1 N, running_var 1 + 0.25 U(0, 1) (non-trivial, so the
                     folding into the conv weights is exercised)
      LSTM           U(-1, 1) / sqrt(hidden) (torch's init), Linear N(0, 1 / fan_in), bias 0.1 N
      out            N(0, 1 / fan_in) times out_scale: the bounded mask's magnitudes spread over (0, 1) instead of
                     saturating at tanh's ceiling on the test signals"""
    from .hnsep import CascadedNet
    cfg = dict(HNSEP_SMALL if cfg is None else cfg)
    shapes = OrderedDict((k, tuple(v.shape)) for k, v in CascadedNet(**cfg).state_dict().items())
    rng = np.random.Generator(np.random.PCG64(seed))
    out = OrderedDict()
    for name, shape in shapes.items():
        leaf = name.rsplit(".", 1)[-1]
        if leaf == "num_batches_tracked":
            out[name] = np.zeros((), dtype=np.int64)
            continue
        z = rng.standard_normal(shape)
        fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else shape[0]
        if ".lstm." in name:
            hid = shapes[name.replace("ih", "hh").replace("bias_hh", "weight_hh").replace("bias_ih", "weight_hh")][1]
            w = rng.uniform(-1, 1, shape) / np.sqrt(hid)
        elif len(shape) == 1 and ".dense.0." in name:
            w = 0.1 * z
        elif len(shape) == 1:
            w = {"weight": 1.0 + 0.1 * z, "bias": 0.1 * z, "running_mean": 0.1 * z,
                 "running_var": 1.0 + 0.25 * rng.uniform(0, 1, shape)}[leaf]
        elif ".dense.0." in name:
            w = z / np.sqrt(fan_in)
        elif name in ("out.weight", "aux_out.weight"):
            w = out_scale * z / np.sqrt(fan_in)
        else:
            w = np.sqrt(2.0 / fan_in) * z
        out[name] = np.ascontiguousarray(w, dtype=np.float32)
    return out
