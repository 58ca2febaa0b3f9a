"""Model files: every model of a render in one file that a process without Python can open (include/dsdenoise.h,
dsd_model_open .. dsd_model_create; the byte layout is DESIGN.md section 4n).

Two independent halves.  `write(path, sections, meta)` is a pure-Python writer on struct / numpy / zlib: it shares no code
with the C reader, so each is the other's check.  `open(path)` goes through the C reader (dsd_model_open validates the
whole file) and hands back what it stores: `.sections`, `.meta`, `.config(i)`, `.tensors(i)`, and `.create(i, device)`,
the raw handle of dsd_model_create.

`section_of(name, module)` takes any wrapper of this package - WaveNet, LYNXNet, the ConvNeXt aux decoder, the FS2
acoustic encoder, the token encoders of variance.py, the vocoder Generator, pitch.RMVPE, hnsep.HnSep, the mel STFT - and
gives the section its native handle is made of: the config of `_config()`, the tensors of `_native_state()` plus
`_extra_weights()` in fp32.  `attach(module, file, section, device)` is the way back: the wrapper then runs on a handle
made from the file, and uploads nothing itself.  `variance_sections(prefix, model)` gives the sections of a staged variance
twin (`deploy.DiffSingerVarianceDeploy`) as dsd_variance_open looks for them: its embedding tables and constants in a
section of their own kind, and the inner handles' sections; `acoustic_sections(prefix, model)` does
the same for a staged acoustic twin (`deploy.DiffSingerAcousticDeploy`) and dsd_acoustic_open (section 4p).
"""
from __future__ import annotations

import builtins
import ctypes as C
import struct
import zlib
from collections import OrderedDict, namedtuple

import numpy as np

from . import _lib

MAGIC = b"DSDMODEL"
HEADER_BYTES, DIRECTORY_END = 32, 64        # the CRC covers [HEADER_BYTES, file size)
SECTION_BYTES, TENSOR_BYTES, META_BYTES = 40, 64, 32

Section = namedtuple("Section", "name kind cfg tensors")
"""name: str; kind: the DSD_* enum (0 .. 8), DSD_VARIANCE_TABLES (10) or DSD_ACOUSTIC_TABLES (11); cfg: the kind's ctypes config struct (or its
bytes); tensors: an ordered mapping name -> array (anything numpy or torch, written as fp32)."""
SectionInfo = namedtuple("SectionInfo", "name kind config_size n_tensors total_floats")


def _as_f32(v):
    """the values in fp32, C order, at the shape given (a 0-dim tensor stays 0-dim, as _NativeBackbone.native_handle
    uploads it)"""
    if hasattr(v, "detach"):
        v = v.detach().cpu().numpy()
    return np.require(np.asarray(v, dtype="<f4"), requirements="C")


def _name_bytes(name, what):
    b = name.encode("utf-8") if isinstance(name, str) else bytes(name)
    if not 1 <= len(b) <= _lib.DSD_MODEL_MAX_NAME or b"\0" in b:
        raise ValueError(f"{what} {name!r}: 1 .. {_lib.DSD_MODEL_MAX_NAME} bytes without a NUL")
    return b


def write(path, sections, meta=None):
    """Writes format version 1.  The bytes depend on the arguments alone (no time stamp, no padding left undefined), so the
    same content gives the same file.  -> the file's size."""
    sections = [Section(*s) for s in sections]
    meta = list((meta or {}).items())
    if len(sections) > _lib.DSD_MODEL_MAX_SECTIONS or len(meta) > _lib.DSD_MODEL_MAX_META:
        raise ValueError(f"at most {_lib.DSD_MODEL_MAX_SECTIONS} sections and {_lib.DSD_MODEL_MAX_META} metadata entries")
    if len({s.name for s in sections}) != len(sections):
        raise ValueError("two sections with one name")
    prepared = []
    for s in sections:
        if s.kind not in _lib.KIND_CONFIGS:
            raise ValueError(f"section {s.name!r}: unknown kind {s.kind}")
        cfg = bytes(s.cfg)
        if len(cfg) != C.sizeof(_lib.KIND_CONFIGS[s.kind]):
            raise ValueError(f"section {s.name!r}: {len(cfg)} config bytes, {_lib.KIND_CONFIGS[s.kind].__name__} has "
                             f"{C.sizeof(_lib.KIND_CONFIGS[s.kind])}")
        tensors = [(_name_bytes(k, "tensor"), _as_f32(v)) for k, v in (s.tensors or {}).items()]
        if len(tensors) > _lib.DSD_MODEL_MAX_TENSORS or any(a.ndim > 4 for _, a in tensors):
            raise ValueError(f"section {s.name!r}: at most {_lib.DSD_MODEL_MAX_TENSORS} tensors of at most 4 dimensions")
        if s.kind == 6 and tensors:
            raise ValueError(f"section {s.name!r}: a mel analysis section has no tensors")
        prepared.append((_name_bytes(s.name, "section"), s.kind, cfg, tensors))

    # pass 1: where everything goes.  Tables first, then the strings, the configs, the values, the data.
    pos = DIRECTORY_END
    section_table = pos
    pos += SECTION_BYTES * len(prepared)
    tensor_tables = []
    for _, _, _, tensors in prepared:
        tensor_tables.append(pos)
        pos += TENSOR_BYTES * len(tensors)
    meta_table = pos
    pos += META_BYTES * len(meta)
    blobs = []

    def put(data, align=1):
        nonlocal pos
        pos = -(-pos // align) * align
        blobs.append((pos, data))
        pos += len(data)
        return blobs[-1][0]

    names = [(put(n + b"\0"), [put(tn + b"\0") for tn, _ in tensors]) for n, _, _, tensors in prepared]
    keys = [put(_name_bytes(k, "metadata key") + b"\0") for k, _ in meta]
    configs = [put(cfg, 8) for _, _, cfg, _ in prepared]
    values = []
    for k, v in meta:
        v = v.encode("utf-8") if isinstance(v, str) else bytes(v)
        if b"\0" in v:
            raise ValueError(f"metadata {k!r}: the value holds a NUL")
        values.append((put(v + b"\0"), len(v)))
    datas = [[put(a.tobytes(), _lib.DSD_MODEL_ALIGN) for _, a in tensors] for _, _, _, tensors in prepared]
    total = pos

    # pass 2: the bytes
    buf = bytearray(total)
    for off, data in blobs:
        buf[off:off + len(data)] = data
    struct.pack_into("<IIQQQ", buf, HEADER_BYTES, len(prepared), len(meta), section_table, meta_table, 0)
    for i, (n, kind, cfg, tensors) in enumerate(prepared):
        struct.pack_into("<QQQIIII", buf, section_table + SECTION_BYTES * i, names[i][0], configs[i], tensor_tables[i], len(n), kind,
                         len(cfg), len(tensors))
        for j, (tn, a) in enumerate(tensors):
            shape = list(a.shape) + [0] * (4 - a.ndim)
            struct.pack_into("<QQQII4q", buf, tensor_tables[i] + TENSOR_BYTES * j, names[i][1][j], datas[i][j], a.size, len(tn), a.ndim,
                             *shape)
    for k, (key, _) in enumerate(meta):
        struct.pack_into("<QQQII", buf, meta_table + META_BYTES * k, keys[k], values[k][0], values[k][1],
                         len(_name_bytes(key, "metadata key")), 0)
    crc = zlib.crc32(memoryview(buf)[HEADER_BYTES:]) & 0xFFFFFFFF
    struct.pack_into("<8sIIQII", buf, 0, MAGIC, _lib.DSD_MODEL_FORMAT_VERSION, _lib.DSD_API_VERSION, total, crc, 0)
    with builtins.open(path, "wb") as f:
        f.write(buf)
    return total


# ------------------------------------------------------------------------------------------------ wrapper -> section
def _zero_device(cfg):
    out = type(cfg).from_buffer_copy(cfg)
    out.device = 0
    return out


def _field_bytes(cfg):
    raw = bytes(cfg)
    return {n: raw[getattr(type(cfg), n).offset:getattr(type(cfg), n).offset + getattr(type(cfg), n).size] for n, _ in cfg._fields_}


def _kind_of(cfg):
    if isinstance(cfg, _lib.DsdConfig):
        return int(cfg.backbone)
    for kind, cls in _lib.KIND_CONFIGS.items():
        if kind > 2 and isinstance(cfg, cls):
            return kind
    raise TypeError(f"not a config struct of the library: {type(cfg).__name__}")


def _module_config(module, device_index=0):
    """the config struct the wrapper creates its handle with"""
    from .backbones import _NativeBackbone
    from .mel import STFT
    if isinstance(module, _NativeBackbone):
        return module._config(device_index)
    if isinstance(module, STFT):
        return module._cfg(device_index)
    if hasattr(module, "_native_config"):          # pitch.RMVPE, hnsep.HnSep
        return module._native_config(device_index)
    raise TypeError(f"{type(module).__name__} has no native handle")


def _module_tensors(module):
    """name -> fp32 array of what the wrapper's handle loads, in load order"""
    from .backbones import _NativeBackbone
    from .mel import STFT
    if isinstance(module, STFT):
        return OrderedDict()
    if isinstance(module, _NativeBackbone):
        tensors = module._native_state()
        tensors.update(module._extra_weights())
    else:       # pitch.RMVPE, hnsep.HnSep load through _lib.load_state_dict, which passes a 0-dim buffer as [1]
        return OrderedDict((k, np.ascontiguousarray(_as_f32(v))) for k, v in module._native_tensors().items())
    return OrderedDict((k, _as_f32(v)) for k, v in tensors.items())


def section_of(name, module):
    """The section a wrapper's native handle is made of (its `device` field 0: a file does not say where it runs)."""
    cfg = _zero_device(_module_config(module))
    return Section(name, _kind_of(cfg), cfg, _module_tensors(module))


def _backbone_of(predictor):
    return predictor.denoise_fn if hasattr(predictor, "denoise_fn") else predictor.velocity_fn


def variance_config(model):
    """The dsd_variance_config of a `deploy.DiffSingerVarianceDeploy` (include/dsdenoise.h): every constant its stages read
    from hparams or from the predictors, so that a C caller has none in its source."""
    from .hparams import hparams
    c = _lib.DsdVarianceConfig()
    c.struct_size = C.sizeof(c)
    fs2 = model.fs2
    c.hidden_size, c.vocab_size = model.hidden_size, fs2.txt_embed.num_embeddings
    c.predict_dur, c.predict_pitch = int(bool(model.predict_dur)), int(bool(model.predict_pitch))
    c.use_lang_id = int(hasattr(fs2, "lang_embed"))
    c.num_lang = fs2.lang_embed.num_embeddings - 1 if c.use_lang_id else 0
    c.use_spk_id = int(bool(model.use_spk_id))
    c.num_spk = model.spk_embed.num_embeddings if c.use_spk_id else 0
    for name in model.variance_prediction_list:
        c.variances |= _lib.EMBED_FLAGS[name]
    if c.predict_pitch:
        c.use_melody_encoder = int(bool(model.use_melody_encoder))
        if c.use_melody_encoder:
            me = model.melody_encoder
            c.melody_hidden_size = me._hidden
            c.use_glide_embed = int(bool(me.use_glide_embed))
            if c.use_glide_embed:
                c.glide_rows, c.glide_embed_scale = me.note_glide_embed.num_embeddings, float(me.glide_embed_scale)
        k = round(hparams['midi_smooth_width'] * hparams['audio_sample_rate'] / hparams['hop_size'])
        if not 1 <= k <= 255:
            raise ValueError(f"midi smoothing kernel of {k} frames is outside [1, 255]")
        p = model.pitch_predictor
        c.smooth_width, c.pitch_repeat_bins = k, p.repeat_bins
        c.pitd_norm_min, c.pitd_norm_max, c.pitd_clip_min, c.pitd_clip_max = p.vmin, p.vmax, p.cmin, p.cmax
    if c.variances:
        p = model.variance_predictor
        c.var_repeat_bins = p.repeat_bins
        lo, hi = p.spec_min.reshape(-1).tolist(), p.spec_max.reshape(-1).tolist()
        for i, name in enumerate(model.variance_prediction_list):
            slot = list(_lib.EMBED_FLAGS).index(name)
            c.var_norm_min[slot], c.var_norm_max[slot] = lo[i], hi[i]
            if p.clamps[i] is None:
                c.var_no_clamp[slot] = 1
            else:
                c.var_clamp_min[slot], c.var_clamp_max[slot] = p.clamps[i]
    c.diffusion_type = _lib.DSD_DIFFUSE_REFLOW if model.diffusion_type == 'reflow' else _lib.DSD_DIFFUSE_DDPM
    c.timesteps = int(hparams.get('timesteps') or 0)
    c.k_step = int(hparams.get('K_step') or c.timesteps)
    c.time_scale_factor = float(hparams.get('time_scale_factor') or 0)
    return c


def variance_sections(prefix, model):
    """The sections dsd_variance_open looks for under `prefix`, for a `deploy.DiffSingerVarianceDeploy`: `<prefix>.tables`
    (kind DSD_VARIANCE_TABLES: the embedding tables under the wrapper's own state_dict names, the mask of its
    `cross_lingual_token_idx` and the smoothing taps of its `build_smooth_op`), `<prefix>.fs2`, `<prefix>.melody`, `<prefix>.pitch` and `<prefix>.variances`."""
    cfg = variance_config(model)
    sd = model.state_dict()
    inner = ("fs2.encoder.", "fs2.dur_predictor.", "melody_encoder.encoder.", "melody_encoder.out_proj.", "pitch_predictor.",
             "variance_predictor.")
    tensors = OrderedDict((k, _as_f32(v)) for k, v in sd.items() if not k.startswith(inner))
    mask = np.zeros(cfg.vocab_size, dtype="<f4")
    idx = np.asarray(model.cross_lingual_token_idx.cpu().numpy(), dtype=np.int64)
    mask[idx[(idx >= 0) & (idx < cfg.vocab_size)]] = 1.0
    tensors["cross_lingual_mask"] = mask
    if cfg.predict_pitch:       # build_smooth_op's taps as this host's torch computes them: the reference's export bakes them in too
        from .deploy import smooth_kernel
        tensors["smooth_taps"] = _as_f32(smooth_kernel(cfg.smooth_width))
    out = [Section(prefix + ".tables", _lib.DSD_VARIANCE_TABLES, cfg, tensors), section_of(prefix + ".fs2", model.fs2)]
    if cfg.use_melody_encoder:
        out.append(section_of(prefix + ".melody", model.melody_encoder))
    if cfg.predict_pitch:
        out.append(section_of(prefix + ".pitch", _backbone_of(model.pitch_predictor)))
    if cfg.variances:
        out.append(section_of(prefix + ".variances", _backbone_of(model.variance_predictor)))
    return out


def acoustic_config(model):
    """The dsd_acoustic_config of a `deploy.DiffSingerAcousticDeploy` (include/dsdenoise.h): every constant its stages and
    its sampler plan read from hparams or from the wrapper, so that a C caller has none in its source."""
    import inspect
    from . import cprogram, schedule
    c = _lib.DsdAcousticConfig()
    c.struct_size = C.sizeof(c)
    fs2, diff = model.fs2, model.diffusion
    c.hidden_size, c.vocab_size, c.out_dims = fs2._hidden, fs2.vocab_size, diff.out_dims
    c.use_lang_id, c.num_lang = int(bool(fs2.use_lang_id)), fs2.num_lang
    c.use_spk_id, c.num_spk = int(bool(fs2.use_spk_id)), fs2.num_spk
    c.embed_flags = fs2._config(0).embed_flags
    c.f0_discrete = int(model.f0_embed_type == 'discrete')
    c.use_shallow_diffusion = int(bool(model.use_shallow_diffusion))
    if fs2.use_key_shift_embed:
        c.shift_min, c.shift_max = float(model.shift_min), float(model.shift_max)
    if fs2.use_speed_embed:
        c.speed_min, c.speed_max = float(model.speed_min), float(model.speed_max)
    c.mel_base_e = int(model.mel_base == 'e')
    if model.diffusion_type == 'reflow':
        c.diffusion_type = _lib.DSD_DIFFUSE_REFLOW
        c.t_start, c.time_scale_factor = float(diff.t_start), float(diff.time_scale_factor)
    else:
        from .hparams import hparams
        c.diffusion_type = _lib.DSD_DIFFUSE_DDPM
        c.timesteps, c.k_step = int(diff.timesteps), int(diff.k_step)
        kind = hparams['schedule_type']
        c.schedule_type = _lib.SCHEDULE_IDS[kind]
        # the wrapper's constructor calls the schedule function with its default max_beta; the buffers are persistent, so a
        # checkpoint may carry another schedule - which a config of (schedule_type, max_beta) cannot describe
        c.max_beta = float(inspect.signature(schedule.linear_beta_schedule).parameters['max_beta'].default)
        mine = cprogram.tables(kind, c.timesteps, c.max_beta)
        for name in ("sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod", "betas"):
            if getattr(mine, name).tobytes() != getattr(diff, name).detach().cpu().numpy().tobytes():
                raise ValueError(f"the model's `{name}` buffer is not the {kind} schedule of {c.timesteps} steps (max_beta {c.max_beta}): "
                                 "a checkpoint with a schedule of its own cannot be packed as an acoustic twin")
    return c


def acoustic_sections(prefix, model):
    """The sections dsd_acoustic_open looks for under `prefix`, for a `deploy.DiffSingerAcousticDeploy`: `<prefix>.tables`
    (kind DSD_ACOUSTIC_TABLES: the mask of its `cross_lingual_token_idx`, spec_min / spec_max broadcast to the mel bins, the
    discrete f0 embedding and the two `frozen_*` tensors where the model has them), `<prefix>.fs2`, `<prefix>.aux` (with shallow
    diffusion) and `<prefix>.denoiser`."""
    cfg = acoustic_config(model)
    tensors = OrderedDict()
    mask = np.zeros(cfg.vocab_size, dtype="<f4")
    idx = np.asarray(model.cross_lingual_token_idx.cpu().numpy(), dtype=np.int64)
    mask[idx[(idx >= 0) & (idx < cfg.vocab_size)]] = 1.0
    tensors["cross_lingual_mask"] = mask
    for name in ("spec_min", "spec_max"):
        v = _as_f32(getattr(model.diffusion, name)).reshape(-1)
        if v.size not in (1, cfg.out_dims):
            raise ValueError(f"{name} has {v.size} values for {cfg.out_dims} mel bins")
        tensors[name] = np.array(np.broadcast_to(v, (cfg.out_dims,)))      # a copy: the caller may edit it
    if cfg.f0_discrete:
        tensors["fs2.pitch_embed.weight"] = _as_f32(model.fs2.pitch_embed.weight)
    for name in ("frozen_spk_embed", "frozen_key_shift"):
        v = model._frozen(name)
        if v is not None:
            tensors[name] = np.ascontiguousarray(_as_f32(v).reshape(-1))
    out = [Section(prefix + ".tables", _lib.DSD_ACOUSTIC_TABLES, cfg, tensors), section_of(prefix + ".fs2", model.fs2)]
    if cfg.use_shallow_diffusion:
        out.append(section_of(prefix + ".aux", model.aux_decoder.decoder))
    out.append(section_of(prefix + ".denoiser", _backbone_of(model.diffusion)))
    return out


# ------------------------------------------------------------------------------------------------ the C reader
class ModelFile:
    """An open model file (dsd_model_open).  Sections are addressed by index or by name."""

    def __init__(self, path):
        self._f = None
        fp = C.c_void_p()
        rc = _lib.lib().dsd_model_open(str(path).encode(), C.byref(fp))
        if rc != 0:
            raise _lib.NativeLibraryError(f"dsd_model_open failed ({rc}): {_lib.lib().dsd_last_error(None).decode('utf-8', 'replace')}")
        self._f = fp
        self.path = str(path)

    def close(self):
        if self._f is not None:
            _lib.lib().dsd_model_close(self._f)
            self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:      # interpreter shutdown
            pass

    def _check(self, rc, what):
        if rc < 0:
            raise _lib.NativeLibraryError(f"{what} failed ({rc}): {_lib.lib().dsd_last_error(None).decode('utf-8', 'replace')}")
        return rc

    def _counts(self):
        ns, nm = C.c_int32(), C.c_int32()
        self._check(_lib.lib().dsd_model_count(self._f, C.byref(ns), C.byref(nm)), "dsd_model_count")
        return ns.value, nm.value

    def index(self, section):
        if isinstance(section, str):
            return self._check(_lib.lib().dsd_model_find(self._f, section.encode()), f"dsd_model_find({section})")
        return int(section)

    def _info(self, i):
        info = _lib.DsdModelSectionInfo()
        self._check(_lib.lib().dsd_model_section(self._f, i, C.byref(info)), "dsd_model_section")
        return info

    @property
    def sections(self):
        out = []
        for i in range(self._counts()[0]):
            info = self._info(i)
            out.append(SectionInfo(info.name.decode("utf-8"), info.kind, info.config_size, info.n_tensors, info.total_floats))
        return out

    @property
    def meta(self):
        out = OrderedDict()
        key, value = C.c_char_p(), C.c_char_p()
        for k in range(self._counts()[1]):
            self._check(_lib.lib().dsd_model_meta_at(self._f, k, C.byref(key), C.byref(value)), "dsd_model_meta_at")
            out[key.value.decode("utf-8")] = value.value.decode("utf-8")
        return out

    def config(self, section):
        """the stored config as the ctypes struct of the section's kind (a copy)"""
        i = self.index(section)
        cfg = _lib.KIND_CONFIGS[self._info(i).kind]()
        self._check(_lib.lib().dsd_model_config(self._f, i, C.byref(cfg), C.sizeof(cfg)), "dsd_model_config")
        return cfg

    def tensors(self, section):
        """name -> numpy copy, in file order"""
        i = self.index(section)
        out = OrderedDict()
        t = _lib.DsdModelTensorInfo()
        for j in range(self._info(i).n_tensors):
            self._check(_lib.lib().dsd_model_tensor(self._f, i, j, C.byref(t)), "dsd_model_tensor")
            shape = tuple(t.shape[d] for d in range(t.ndim))
            data = np.ctypeslib.as_array(t.data, shape=(t.count,)).copy() if t.count else np.zeros(0, np.float32)
            out[t.name.decode("utf-8")] = data.reshape(shape)
        return out

    def create(self, section, device=0):
        """dsd_model_create: the raw handle (release it with dsd_destroy)"""
        hp = C.c_void_p()
        self._check(_lib.lib().dsd_model_create(self._f, self.index(section), int(device), C.byref(hp)), "dsd_model_create")
        return hp


def open(path):        # noqa: A001  (the module's verb, as in gzip.open)
    return ModelFile(path)


# ------------------------------------------------------------------------------------------------ file -> wrapper
def attach(module, file, section, device):
    """Makes an existing wrapper run on a handle made by dsd_model_create from `file`'s `section`.  Refuses unless the
    section's config equals the wrapper's own (apart from `device`); then copies the tensors the wrapper holds under its
    own state_dict names from the file, so that its Python mirror agrees with the handle; then installs the handle with the
    weights marked clean: the wrapper uploads nothing."""
    import torch
    from .backbones import _NativeBackbone
    from .mel import STFT
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"diffsinger_amd.modelfile.attach needs an MI355X (HIP) device; got {dev.type}. There is no CPU path.")
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    i = file.index(section)
    want, got = _zero_device(_module_config(module)), _zero_device(file.config(i))
    if type(want) is not type(got):
        raise ValueError(f"section {file.sections[i].name!r} holds a {type(got).__name__}, this {type(module).__name__} "
                         f"is made from a {type(want).__name__}")
    if bytes(want) != bytes(got):
        a, b = _field_bytes(want), _field_bytes(got)
        raise ValueError(f"section {file.sections[i].name!r} holds another model than this {type(module).__name__}: "
                         f"the configs differ in {', '.join(n for n in a if a[n] != b[n])}")
    if isinstance(module, STFT):
        old = module._handles.pop(idx, None)
        if old is not None:
            _lib.lib().dsd_destroy(old)
        module._handles[idx] = file.create(i, idx)
        return module
    tensors = file.tensors(i)
    if not isinstance(module, _NativeBackbone):     # pitch.RMVPE, hnsep.HnSep: the state dict is their mirror
        module._install_native(file.create(i, idx), tensors, torch.device("cuda", idx))
        return module
    missing = [k for k in module._native_state() if k not in tensors]
    if missing:
        raise ValueError(f"section {file.sections[i].name!r} lacks {', '.join(missing[:4])}")
    handle = file.create(i, idx)
    with torch.no_grad():
        for k, v in module.state_dict().items():
            if k in tensors:
                v.copy_(torch.from_numpy(tensors[k]).reshape(v.shape))
    module.release_native()
    module._handle, module._handle_device = handle, idx
    module._weights_dirty = False
    module._cond_key = None
    return module
