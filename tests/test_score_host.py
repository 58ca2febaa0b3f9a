"""Host-side checks of validation scoring (no GPU): every DSD_EINVAL of the handle-free calls, tests/score_ref.py against
G25 (tests/golden/g25_score.npz: the reference's p_losses, losses and metrics), the seeded `t` rule, and the public layout
of losses.py / metrics.py against the reference's.  The C99 check of the header (tests/test_cabi_exports.py) covers the new
declarations as it covers the others; it is repeated here on the scoring structs' sizes."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

import score_cases as sc
import score_ref as sr
from diffsinger_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DSD_EINVAL, DSD_EHIP = -1, -3


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(ROOT, "tests", "golden", "g25_score.npz"))


def ref_distance(g, name):
    """The bound of a 0-dim fp32 result against the reference's fp32 scalar: the reference's own rounding distance twice, and
    one fp32 ulp (2^-23 relative) for the result's own rounding.  Both quantities come from the fixture."""
    r32, r64 = float(g[f"{name}_ref32"]), float(g[f"{name}_ref64"])
    return r32, 2.0 * abs(r64 - r32) + 2.0 ** -23 * abs(r64)


# ------------------------------------------------------------------------------------------- argument checks
class _Args:
    """Host buffers standing in for device memory: every call below is refused before anything is read."""

    def __init__(self):
        self.buf = (C.c_double * 64)()
        self.p = C.cast(self.buf, C.c_void_p).value                 # 16-byte aligned in practice; checked below
        self.seeds = (C.c_uint64 * 4)(1, 2, 3, 4)

    def ptr(self, off=0):
        return C.c_void_p(self.p + off)


def _diffuse_spec(a, /, **kw):
    s = _lib.DsdDiffuseSpec()
    s.struct_size, s.kind, s.B, s.rows, s.cols, s.domain = C.sizeof(s), 0, 2, 3, 5, 9
    s.x0, s.eps, s.a, s.c = a.p + 64, a.p + 128, a.p + 192, a.p + 256
    s.seeds = C.cast(a.seeds, C.POINTER(C.c_uint64))
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _loss_spec(a, /, **kw):
    s = _lib.DsdLossSpec()
    s.struct_size, s.kind, s.B, s.rows, s.cols = C.sizeof(s), 0, 2, 3, 5
    s.pred, s.target = a.p + 64, a.p + 128
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _dur_spec(a, /, **kw):
    s = _lib.DsdDurSpec()
    s.struct_size, s.kind, s.B, s.L, s.n_words = C.sizeof(s), 0, 2, 4, 3
    s.offset, s.rhythm_tolerance, s.pdur_tolerance = 1.0, 0.05, 0.2
    s.dur_pred, s.dur_gt, s.ph2word = a.p + 64, a.p + 128, a.p + 192
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _einval(rc, needle):
    assert rc == DSD_EINVAL, rc
    msg = _lib.lib().dsd_last_error(None).decode()
    assert needle in msg, msg


def test_diffuse_einval():
    lib, a = _lib.lib(), _Args()
    xt, tg = a.ptr(320), a.ptr(384)
    call = lambda s, x=xt, t=tg: lib.dsd_diffuse(0, None if s is None else C.byref(s), x, t, None)  # noqa: E731
    _einval(call(None), "null argument")
    _einval(call(_diffuse_spec(a), x=None), "null argument")
    _einval(call(_diffuse_spec(a, struct_size=8)), "struct_size")
    _einval(call(_diffuse_spec(a, kind=2)), "unknown kind")
    _einval(call(_diffuse_spec(a, x0=None)), "null x0 or a")
    _einval(call(_diffuse_spec(a, a=None)), "null x0 or a")
    _einval(call(_diffuse_spec(a, c=None)), "needs c")
    _einval(call(_diffuse_spec(a, eps=None, seeds=C.POINTER(C.c_uint64)())), "neither eps nor seeds")
    _einval(call(_diffuse_spec(a, eps=None), t=None), "target may be NULL only")
    _einval(call(_diffuse_spec(a, kind=1, c=None), t=None), "target may be NULL only")
    for dim in ("B", "rows", "cols"):
        _einval(call(_diffuse_spec(a, **{dim: 0})), "must be positive")
    _einval(call(_diffuse_spec(a, B=1 << 11, rows=1 << 10, cols=1 << 10)), "more than 2^31 - 1")
    _einval(call(_diffuse_spec(a), x=a.ptr(64)), "must not be an input")            # x_t == x0
    _einval(call(_diffuse_spec(a), t=a.ptr(128)), "must not be an input")           # target == eps
    _einval(call(_diffuse_spec(a), x=tg), "must not be an input")                   # x_t == target
    _einval(call(_diffuse_spec(a), x=a.ptr(322)), "4-byte aligned")


def test_masked_loss_einval():
    lib, a = _lib.lib(), _Args()
    ws, out = a.ptr(320), a.ptr(384)
    call = lambda s, w=ws, o=out: lib.dsd_masked_loss(0, None if s is None else C.byref(s), w, o, None)  # noqa: E731
    _einval(call(None), "null argument")
    _einval(call(_loss_spec(a), w=None), "null argument")
    _einval(call(_loss_spec(a), o=None), "null argument")
    _einval(call(_loss_spec(a, struct_size=0)), "struct_size")
    _einval(call(_loss_spec(a, kind=-1)), "unknown kind")
    _einval(call(_loss_spec(a, pred=None)), "null pred or target")
    _einval(call(_loss_spec(a, target=None)), "null pred or target")
    for dim in ("B", "rows", "cols"):
        _einval(call(_loss_spec(a, **{dim: -3})), "must be positive")
    _einval(call(_loss_spec(a, B=3, rows=1 << 15, cols=1 << 15)), "more than 2^31 - 1")
    _einval(call(_loss_spec(a), w=a.ptr(324)), "aligned")
    _einval(call(_loss_spec(a, t=a.p + 2)), "aligned")


def test_curve_stats_einval():
    lib, a = _lib.lib(), _Args()
    call = lambda p=a.ptr(64), t=a.ptr(128), n=7, w=a.ptr(320), o=a.ptr(384): lib.dsd_curve_stats(  # noqa: E731
        0, p, t, None, n, 0.5, w, o, None)
    for kw in (dict(p=None), dict(t=None), dict(w=None), dict(o=None)):
        _einval(call(**kw), "null argument")
    _einval(call(n=0), "outside [1, 2^31 - 1]")
    _einval(call(n=1 << 31), "outside [1, 2^31 - 1]")
    _einval(call(o=a.ptr(388)), "aligned")


def test_dur_score_einval():
    lib, a = _lib.lib(), _Args()
    wp, wg, ws, out = a.ptr(256), a.ptr(288), a.ptr(320), a.ptr(384)

    def call(s, wp=wp, wg=wg, ws=ws, out=out):
        return lib.dsd_dur_score(0, None if s is None else C.byref(s), wp, wg, ws, out, None)

    _einval(call(None), "null argument")
    for kw in (dict(wp=None), dict(wg=None), dict(ws=None), dict(out=None)):
        _einval(call(_dur_spec(a), **kw), "null argument")
    _einval(call(_dur_spec(a, struct_size=4)), "struct_size")
    _einval(call(_dur_spec(a, kind=2)), "unknown kind")
    for f in ("dur_pred", "dur_gt", "ph2word"):
        _einval(call(_dur_spec(a, **{f: None})), "null dur_pred, dur_gt or ph2word")
    _einval(call(_dur_spec(a, B=0)), "must be positive")
    _einval(call(_dur_spec(a, L=0)), "must be positive")
    _einval(call(_dur_spec(a, n_words=1)), "n_words")
    _einval(call(_dur_spec(a, B=1 << 20, L=1 << 11)), "more than 2^31 - 1")
    _einval(call(_dur_spec(a), wg=wp), "must not be an input")
    _einval(call(_dur_spec(a), wp=a.ptr(64)), "must not be an input")
    _einval(call(_dur_spec(a, ph2word=a.p + 196)), "aligned")


def test_valid_arguments_pass_every_check():
    """With nothing wrong the calls get as far as selecting the device - which, without one, is DSD_EHIP: the EINVAL cases
    above are refused for the reason each names, not for one common to them all.  (With a GPU the calls would launch on
    these host buffers: nothing is called then; tests/test_gpu_score.py makes the valid calls.)"""
    if torch.cuda.is_available():
        return
    lib, a = _lib.lib(), _Args()
    assert lib.dsd_diffuse(0, C.byref(_diffuse_spec(a)), a.ptr(320), a.ptr(384), None) == DSD_EHIP
    assert lib.dsd_masked_loss(0, C.byref(_loss_spec(a)), a.ptr(320), a.ptr(384), None) == DSD_EHIP
    assert lib.dsd_curve_stats(0, a.ptr(64), a.ptr(128), None, 7, 0.5, a.ptr(320), a.ptr(384), None) == DSD_EHIP
    assert lib.dsd_dur_score(0, C.byref(_dur_spec(a)), a.ptr(256), a.ptr(288), a.ptr(320), a.ptr(384), None) == DSD_EHIP


def test_constants_and_struct_sizes_match_header():
    src = open(os.path.join(ROOT, "include", "dsdenoise.h")).read()
    assert f"#define DSD_SCORE_WORKSPACE_BYTES {_lib.DSD_SCORE_WORKSPACE_BYTES}" in src
    for name, val in (("DSD_DIFFUSE_DDPM", 0), ("DSD_DIFFUSE_REFLOW", 1), ("DSD_LOSS_L1", 0), ("DSD_LOSS_L2", 1), ("DSD_DUR_MSE", 0),
                      ("DSD_DUR_HUBER", 1)):
        assert f"#define {name} {val}" in src
    assert (_lib.DSD_DIFFUSE_DDPM, _lib.DSD_DIFFUSE_REFLOW) == (0, 1)
    assert _lib.LOSS_IDS == {"l1": 0, "l2": 1} and _lib.DUR_LOSS_IDS == {"mse": 0, "huber": 1}
    # the library refuses any other struct_size (the EINVAL tests), so these are the header's sizes
    assert [C.sizeof(c) for c in (_lib.DsdDiffuseSpec, _lib.DsdLossSpec, _lib.DsdDurSpec)] == [64, 56, 64]
    assert C.sizeof(_lib.DsdCurveResult) == 40 and C.sizeof(_lib.DsdDurResult) == 80
    from diffsinger_amd import noise
    assert (noise.SCORE_T, noise.SCORE_NOISE) == (8, 9)
    assert "8 = the scoring step's t, 9 = the scoring step's noise" in src


def test_header_with_scoring_is_plain_c99(tmp_path):
    """A C99 translation unit that fills the scoring structs and names the four calls compiles with -pedantic -Werror."""
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    c = tmp_path / "use.c"
    c.write_text('#include "dsdenoise.h"\n'
                 "int use(void* ws, float* x, double* out, dsd_curve_result* cr, dsd_dur_result* dr) {\n"
                 "    dsd_diffuse_spec d = {0}; dsd_loss_spec l = {0}; dsd_dur_spec u = {0};\n"
                 "    char fits[DSD_SCORE_WORKSPACE_BYTES == 65536 ? 1 : -1];\n"
                 "    (void)fits; d.struct_size = (int32_t)sizeof d; l.struct_size = (int32_t)sizeof l; u.struct_size = (int32_t)sizeof u;\n"
                 "    return dsd_diffuse(0, &d, x, x, 0) + dsd_masked_loss(0, &l, ws, out, 0)\n"
                 "         + dsd_curve_stats(0, x, x, 0, 1, 0.5f, ws, cr, 0) + dsd_dur_score(0, &u, x, x, ws, dr, 0);\n"
                 "}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I",
                    os.path.join(ROOT, "include"), str(c)], check=True)


# ------------------------------------------------------------------------------------------- score_ref.py against G25
LOSS_SCALARS = ["diff_l1_masked", "diff_l1", "rf_l1_lognorm_masked", "rf_l1_plain", "diff_l2_masked", "diff_l2", "rf_l2_lognorm_masked",
                "rf_l2_plain", "aux_l1"]


def _ref_loss(name):
    li = sc.loss_inputs()
    kind = "l2" if "_l2" in name else "l1"
    npad = li["non_padding"][..., 0] if "masked" in name else None
    t = li["t"] if "lognorm" in name else None
    return sr.masked_loss(kind, li["pred"], li["target"], npad, t)[1]


@pytest.mark.parametrize("name", LOSS_SCALARS)
def test_ref_losses_vs_golden(g, name):
    v = _ref_loss(name)
    assert v == float(g[f"{name}_ref64"])                           # the restatement, exactly
    r32, bound = ref_distance(g, name)
    assert abs(np.float32(v) - r32) <= bound, (name, v, r32, bound)


@pytest.mark.parametrize("tag", sorted(sc.WRAPPERS))
def test_ref_p_losses_vs_golden(g, tag):
    """The noising formulas in fp32 against the reference's x_t and target bit for bit, and the losses on its outputs."""
    c, inp = sc.WRAPPERS[tag], sc.wrapper_inputs(tag)
    spec, noise = g[f"{tag}_spec"], g[f"{tag}_noise"]
    if c["family"] == "ddpm":
        assert np.array_equal(noise, inp["noise"])
        from diffsinger_amd import schedule
        tb = schedule.DDPMTables(schedule.BETA_SCHEDULE["linear"](1000))
        x_t, target = sr.diffuse_ddpm(spec, noise, tb.sqrt_alphas_cumprod[inp["t"]], tb.sqrt_one_minus_alphas_cumprod[inp["t"]])
    else:
        x_t, target = sr.diffuse_reflow(spec, noise, inp["t"])
    assert np.array_equal(x_t, g[f"{tag}_x_t"]) and np.array_equal(target, g[f"{tag}_target"])
    npad = inp["non_padding"][..., 0]
    for kind in ("l1", "l2"):
        v = sr.masked_loss(kind, g[f"{tag}_pred"], g[f"{tag}_target"], npad, None if c["family"] == "ddpm" else inp["t"])[1]
        assert v == float(g[f"{tag}_{kind}_ref64"])
        r32, bound = ref_distance(g, f"{tag}_{kind}")
        assert abs(np.float32(v) - r32) <= bound, (tag, kind, v, r32, bound)


def test_ref_lognorm_weights_vs_golden(g):
    w = sr.lognorm_weight(sc.loss_inputs()["t"])
    assert np.array_equal(w, g["rf_weights_ref64"])
    # fp32 evaluation of log / exp / two divisions: a few fp32 ulps, away from the clipped ends (t[0] is clipped: the fp32
    # reference clips to fl32(1e-7), the restatement to the double 1e-7 - 1.2e-8 relative apart - where w = 1e-7 + tiny)
    assert np.allclose(g["rf_weights_ref32"], w, rtol=2e-6, atol=0)


def test_ref_durations_vs_golden(g):
    di = sc.dur_inputs()
    lp, lw, ls = di["lambdas"]
    for kind in ("mse", "huber"):
        res = sr.dur_score(di["dur_pred_raw"], di["dur_gt"], di["ph2word"], offset=di["offset"], loss_type=kind)
        v = sr.dur_loss(res, lp, lw, ls)
        assert v == float(g[f"dur_{kind}_ref64"])
        r32, bound = ref_distance(g, f"dur_{kind}")
        assert abs(np.float32(v) - r32) <= bound, (kind, v, r32, bound)
        # the word sums: torch's CPU scatter_add, bit for bit
        assert np.array_equal(res["wdur_pred"], g["dur_wdur_pred"]) and np.array_equal(res["wdur_gt"], g["dur_wdur_gt"])
    for name, mask in (("nomask", None), ("mask", di["mask"])):
        res = sr.dur_score(di["dur_pred"], di["dur_gt"], di["ph2word"], mask=mask, rhythm_tolerance=di["rhythm_tolerance"],
                           pdur_tolerance=di["pdur_tolerance"])
        assert res["counts"][:2] == g[f"rhythm_{name}_counts"].tolist()
        assert res["counts"][2:] == g[f"pdur_{name}_counts"].tolist()
        for key, (num, den) in (("rhythm", res["counts"][:2]), ("pdur", res["counts"][2:])):
            assert num / den == float(g[f"{key}_{name}_ref64"])
            r32, bound = ref_distance(g, f"{key}_{name}")
            assert abs(np.float32(num / den) - r32) <= bound


def test_ref_curves_vs_golden(g):
    ci = sc.curve_inputs()
    for name, mask in (("nomask", None), ("mask", ci["mask"])):
        st = sr.curve_stats(ci["pred"], ci["target"], mask, ci["tolerance"])
        assert [st["close"], st["total"]] == g[f"curve_{name}_counts"].tolist()
        assert [st["sum_target"], st["sum_target_sq"], st["sum_residual_sq"]] == g[f"curve_{name}_sums64"].tolist()
        for key, v in (("curve_acc", sr.curve_accuracy(st)), ("curve_r2", sr.curve_r2(st))):
            assert v == float(g[f"{key}_{name}_ref64"])
            r32, bound = ref_distance(g, f"{key}_{name}")
            assert abs(np.float32(v) - r32) <= bound, (key, name, v, r32, bound)


# ------------------------------------------------------------------------------------------- the seeded t rule
def test_seeded_t_rule():
    from diffsinger_amd.diffusion import seeded_t_ddpm, seeded_t_reflow
    top = np.float32(1.0) - np.float32(2.0 ** -24)                  # the largest draw: ((2^23 - 1) + 0.5) * 2^-23
    u = np.array([top, 2.0 ** -24, 0.5, 0.4999999, 0.9985, 0.9990001, 1.5e-3], np.float32)
    t = seeded_t_ddpm(torch.from_numpy(u), 1000)
    assert t.dtype == torch.int64
    assert t.tolist() == [999, 0, 500, 499, 998, 999, 1]
    assert int(t[0]) == 999                                         # the largest draw stays inside [0, k_step)
    assert t.tolist() == sr.seeded_t_ddpm(u, 1000).tolist()
    for k in (1, 7, 100, 1000, 4000):
        tk = seeded_t_ddpm(torch.from_numpy(u), k)
        assert int(tk.min()) >= 0 and int(tk.max()) == k - 1
        assert tk.tolist() == [min(k - 1, int(np.floor(float(v) * k))) for v in u]
    for t_start in (0.0, 0.25, 0.6):
        r = seeded_t_reflow(torch.from_numpy(u), t_start)
        assert r.dtype == torch.float32
        assert np.array_equal(r.numpy(), sr.seeded_t_reflow(u, t_start))
        assert np.array_equal(r.numpy(), np.float32(t_start) + np.float32(1.0 - t_start) * u)
        assert float(r.min()) >= t_start and float(r.max()) <= 1.0


# ------------------------------------------------------------------------------------------- the public layout
def _sig(fn):
    return [f"{q.name}:{q.kind.name}:{'' if q.default is q.empty else repr(q.default)}" for q in inspect.signature(fn).parameters.values()]


def test_losses_and_metrics_layout_matches_reference(g):
    from diffsinger_amd import losses, metrics
    for key in g.files:
        if key.startswith("sig_"):
            _, cls, meth = key.split("_", 2)
            mod = losses if hasattr(losses, cls) else metrics
            assert _sig(getattr(getattr(mod, cls), meth)) == g[key].tolist(), key
    assert isinstance(inspect.getattr_static(losses.RectifiedFlowLoss, "get_weights"), staticmethod)
    made = {"RawCurveAccuracy": metrics.RawCurveAccuracy(tolerance=0.5), "RawCurveR2Score": metrics.RawCurveR2Score(),
            "RhythmCorrectness": metrics.RhythmCorrectness(tolerance=0.05),
            "PhonemeDurationAccuracy": metrics.PhonemeDurationAccuracy(tolerance=0.2)}
    for name, obj in made.items():
        states = sorted(k for k, v in vars(obj).items() if torch.is_tensor(v))
        assert states == g[f"states_{name}"].tolist(), name
        for s in states:        # int64 counts, float64 sums
            assert getattr(obj, s).dtype == (torch.int64 if s in ("close", "total", "correct", "accurate") else torch.float64)
        assert callable(obj.reset)
    with pytest.raises(AssertionError):
        metrics.RhythmCorrectness(tolerance=1.5)
    for bad in ("l3", "mse"):
        with pytest.raises(NotImplementedError):
            losses.DiffusionLoss(bad)
    with pytest.raises(NotImplementedError):
        losses.DurationLoss(1.0, "l1")
    w = losses.RectifiedFlowLoss.get_weights(torch.from_numpy(sc.loss_inputs()["t"]))
    assert tuple(w.shape) == (3, 1, 1, 1) and np.array_equal(w.reshape(-1).numpy(), g["rf_weights_ref32"])


def test_linguistic_checks_kept():
    from diffsinger_amd.metrics import linguistic_checks
    ok = torch.ones(2, 3)
    p2w = torch.tensor([[1, 1, 2], [1, 2, 0]])
    linguistic_checks(ok, ok, p2w)
    for args in ((ok, ok, torch.zeros(2, 3, dtype=torch.long)), (ok, ok, -p2w), (-ok, ok, p2w), (ok, -ok, p2w),
                 (ok, ok[:, :2], p2w), (ok, ok, p2w * 9), (ok[0], ok[0], p2w[0])):
        with pytest.raises(AssertionError):
            linguistic_checks(*args)


def test_cpu_tensors_raise_not_fall_back():
    from diffsinger_amd import losses, metrics
    x = torch.zeros(1, 1, 4, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        losses.DiffusionLoss("l1")(x, x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        metrics.RawCurveR2Score().update(x, x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        losses.DurationLoss(1.0, "mse")(torch.ones(1, 3), torch.ones(1, 3), torch.tensor([[1, 1, 2]]))
