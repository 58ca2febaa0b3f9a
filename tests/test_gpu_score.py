"""-m gpu: validation scoring - dsd_diffuse, dsd_masked_loss, dsd_curve_stats, dsd_dur_score, the loss modules and metrics
built on them, and `forward_score` of the two diffusion wrappers and their codecs.

What is compared with what:
  * the noising step: bit for bit with the numpy fp32 formulas of tests/score_ref.py and with the reference's own x_t (G25);
    the in-launch draw bit for bit with noise.fill;
  * every reduction: relative 1e-12 on each double against score_ref.py (float64, correctly rounded sums), integer counts
    equal, the word sums bit for bit torch's CPU scatter_add; two runs give identical bits;
  * a 0-dim fp32 result against the reference's recorded fp32 scalar: |gpu - ref32| <= 2 |ref64 - ref32| + 2^-23 |ref64|,
    both quantities from the fixture (the reference's own rounding distance, a factor two, and one fp32 ulp for the
    result's own rounding) - not a number measured on the code under test;
  * forward_score's network output against the reference's at the suite's single-evaluation tolerance (TOL_NFE), through
    `check`; target and t as the reference returns them, bit for bit.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import score_cases as sc  # noqa: E402
import score_ref as sr  # noqa: E402
from diffsinger_amd import _lib, losses, metrics, noise, score, synth  # noqa: E402
from gpu_util import check, dev, load_synth, set_hp  # noqa: E402

TOL_NFE = 2e-5          # tests/test_gpu_parity.py, tests/test_gpu_width.py: one evaluation of a backbone
REL = 1e-12
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g25_score.npz")
SPAN, MAX_BLOCKS = 2048, 1024       # a workgroup's share of a reduction, and the grid's cap (include/dsdenoise.h)


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


@pytest.fixture(autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    set_hp()


def ref_bound(g, name):
    r32, r64 = float(g[f"{name}_ref32"]), float(g[f"{name}_ref64"])
    return r32, 2.0 * abs(r64 - r32) + 2.0 ** -23 * abs(r64)


def assert_scalar(g, name, value):
    assert value.dim() == 0 and value.dtype == torch.float32 and value.device.type == "cuda", name
    r32, bound = ref_bound(g, name)
    v = float(value)
    print(f"{name}: gpu {v:.9g} ref32 {r32:.9g} |d| {abs(v - r32):.3g} bound {bound:.3g}")
    assert abs(v - r32) <= bound, (name, v, r32, bound)


def close(a, b):
    return abs(a - b) <= REL * abs(b)


def offset_copy(a, off):
    """`a` on the device at a pointer `off` floats past a 16-byte boundary (off = 0: aligned)"""
    a = np.ascontiguousarray(a)
    buf = torch.empty(a.size + 4, dtype=torch.from_numpy(a).dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    return view


def raw_diffuse(kind, x0, a, c, eps, x_t, target, seeds=None, domain=noise.SCORE_NOISE):
    """dsd_diffuse on exactly these tensors (score.diffuse allocates its outputs, which are then always aligned)"""
    b, cols = x0.shape[0], x0.shape[-1]
    spec = _lib.DsdDiffuseSpec()
    spec.struct_size, spec.kind, spec.B, spec.rows, spec.cols = C.sizeof(spec), score.KINDS[kind], b, x0.numel() // (b * cols), cols
    spec.domain, spec.x0, spec.a = domain, x0.data_ptr(), a.data_ptr()
    if c is not None:
        spec.c = c.data_ptr()
    keep = None
    if eps is not None:
        spec.eps = eps.data_ptr()
    else:
        keep = (C.c_uint64 * b)(*seeds)
        spec.seeds = C.cast(keep, C.POINTER(C.c_uint64))
    rc = _lib.lib().dsd_diffuse(0, C.byref(spec), C.c_void_p(x_t.data_ptr()), None if target is None else C.c_void_p(target.data_ptr()),
                                C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _lib.lib().dsd_last_error(None)


def coefficients(kind, b, seed):
    r = np.random.Generator(np.random.PCG64(seed))
    a = r.random(b, dtype=np.float32)                       # distinct per item
    return a, (np.sqrt(1 - a.astype(np.float64) ** 2).astype(np.float32) if kind == "ddpm" else None)


# ------------------------------------------------------------------------------------------- dsd_diffuse
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "plus4bytes"])
@pytest.mark.parametrize("shape", [(3, 3, 5), (2, 8, 67), (1, 16, 64)], ids=str)
@pytest.mark.parametrize("kind", ["ddpm", "reflow"])
def test_diffuse_bitwise(kind, shape, off):
    x0, eps = synth.synth_normal(shape, 2601), synth.synth_normal(shape, 2602)
    a, c = coefficients(kind, shape[0], 2603)
    want_x, want_t = sr.diffuse_ddpm(x0, eps, a, c) if kind == "ddpm" else sr.diffuse_reflow(x0, eps, a)
    dx0, deps = offset_copy(x0, off), offset_copy(eps, off)
    x_t, target = offset_copy(np.zeros(shape, np.float32), off), offset_copy(np.zeros(shape, np.float32), off)
    raw_diffuse(kind, dx0, dev(a), None if c is None else dev(c), deps, x_t, target)
    torch.cuda.synchronize()
    assert np.array_equal(x_t.cpu().numpy(), want_x) and np.array_equal(target.cpu().numpy(), want_t)
    if kind == "ddpm":      # target may be NULL: x_t alone, the same bits
        x2 = offset_copy(np.zeros(shape, np.float32), off)
        raw_diffuse(kind, dx0, dev(a), dev(c), deps, x2, None)
        assert torch.equal(x2, x_t)
    # the module-level binding (it allocates the outputs itself)
    bx, bt = score.diffuse(kind, dx0, dev(a), None if c is None else dev(c), eps=deps)
    assert torch.equal(bx, x_t) and torch.equal(bt, target)


@pytest.mark.parametrize("tag", sorted(sc.WRAPPERS))
def test_diffuse_vs_golden_x_t(g, tag):
    """the reference's own q_sample / x_start + t * (x_end - x_start), on its normalised spectrogram and noise"""
    c, inp = sc.WRAPPERS[tag], sc.wrapper_inputs(tag)
    spec, eps = dev(g[f"{tag}_spec"]), dev(g[f"{tag}_noise"])
    if c["family"] == "ddpm":
        from diffsinger_amd import schedule
        tb = schedule.DDPMTables(schedule.BETA_SCHEDULE["linear"](1000))
        x_t, target = score.diffuse("ddpm", spec, dev(tb.sqrt_alphas_cumprod[inp["t"]]), dev(tb.sqrt_one_minus_alphas_cumprod[inp["t"]]),
                                    eps=eps)
    else:
        x_t, target = score.diffuse("reflow", spec, dev(inp["t"]), eps=eps)
    assert np.array_equal(x_t.cpu().numpy(), g[f"{tag}_x_t"]) and np.array_equal(target.cpu().numpy(), g[f"{tag}_target"])


@pytest.mark.parametrize("shape", [(3, 3, 5), (3, 8, 64)], ids=str)
@pytest.mark.parametrize("kind", ["ddpm", "reflow"])
def test_diffuse_in_launch_draw(kind, shape):
    seeds = [71, (1 << 63) + 5, 73]
    x0 = synth.synth_normal(shape, 2611)
    a, c = coefficients(kind, shape[0], 2612)
    eps = noise.fill((1,) + shape, seeds, noise.SCORE_NOISE)[0]
    x_t, target = score.diffuse(kind, dev(x0), dev(a), None if c is None else dev(c), seeds=seeds)
    e = eps.cpu().numpy()
    want_x, want_t = sr.diffuse_ddpm(x0, e, a, c) if kind == "ddpm" else sr.diffuse_reflow(x0, e, a)
    assert np.array_equal(x_t.cpu().numpy(), want_x) and np.array_equal(target.cpu().numpy(), want_t)
    if kind == "ddpm":
        assert torch.equal(target, eps)
    other = score.diffuse(kind, dev(x0), dev(a), None if c is None else dev(c), seeds=seeds, domain=noise.X_T)[1]
    assert not torch.equal(other, target)
    for b in range(shape[0]):           # item b of the batch is a lone call with seeds[b]
        lx, lt = score.diffuse(kind, dev(x0[b:b + 1]), dev(a[b:b + 1]), None if c is None else dev(c[b:b + 1]), seeds=[seeds[b]])
        assert torch.equal(lx[0], x_t[b]) and torch.equal(lt[0], target[b])


def test_scoring_calls_are_capturable():
    """dsd_diffuse (drawing inside the launch), dsd_masked_loss, dsd_curve_stats and dsd_dur_score inside a captured graph
    give the bits they give outside."""
    shape, seeds = (3, 8, 67), [5, 6, 7]
    x0 = dev(synth.synth_normal(shape, 2621))
    a, c = (dev(v) for v in coefficients("ddpm", 3, 2622))
    di = sc.dur_inputs()
    dp, dg, p2w = dev(di["dur_pred_raw"]), dev(di["dur_gt"]), dev(di["ph2word"])
    x_e, t_e = score.diffuse("ddpm", x0, a, c, seeds=seeds)
    loss_e = score.masked_loss("l2", x_e, t_e).clone()
    cnt_e, sum_e = (v.clone() for v in score.curve_stats(x_e, t_e, tolerance=0.5))
    dur_e = {k: v.clone() for k, v in score.dur_score(dp, dg, p2w, n_words=7).items()}
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        x_g, t_g = score.diffuse("ddpm", x0, a, c, seeds=seeds)
        loss_g = score.masked_loss("l2", x_g, t_g)
        cnt_g, sum_g = score.curve_stats(x_g, t_g, tolerance=0.5)
        dur_g = score.dur_score(dp, dg, p2w, n_words=7)
    for v in (x_g, t_g, loss_g, cnt_g, sum_g):
        v.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(x_g, x_e) and torch.equal(t_g, t_e) and torch.equal(loss_g, loss_e)
    assert torch.equal(cnt_g, cnt_e) and torch.equal(sum_g, sum_e)
    for k in dur_e:
        assert torch.equal(dur_g[k], dur_e[k]), k


# ------------------------------------------------------------------------------------------- dsd_masked_loss
def _loss_case(shape, seed, mask, with_t):
    r = np.random.Generator(np.random.PCG64(seed))
    pred, target = r.standard_normal(shape, dtype=np.float32), r.standard_normal(shape, dtype=np.float32)
    npad = None
    if mask:
        npad = (r.random((shape[0], shape[-1])) < 0.7).astype(np.float32)       # holes
        npad[-1] = 0.0                                                           # an all-padding item
    t = None
    if with_t:
        t = r.random(shape[0], dtype=np.float32)
        t[0] = 0.0                                                               # clipped
    return pred, target, npad, t


# one element; one more than a workgroup's share; cols no multiple of 4; more spans than the grid has workgroups
LOSS_SHAPES = [(1, 1, 1), (1, 1, SPAN + 1), (3, 5, 67), (2, 3, 2, 7), (2, 16, MAX_BLOCKS * SPAN // 32 + 1)]


@pytest.mark.parametrize("with_t", [False, True], ids=["plain", "lognorm"])
@pytest.mark.parametrize("mask", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=str)
@pytest.mark.parametrize("kind", ["l1", "l2"])
def test_masked_loss_vs_ref(kind, shape, mask, with_t):
    pred, target, npad, t = _loss_case(shape, 2630 + len(shape) + shape[-1] % 97, mask, with_t)
    want = sr.masked_loss(kind, pred, target, npad, t)
    args = (kind, dev(pred), dev(target), None if npad is None else dev(npad), None if t is None else dev(t))
    out = score.masked_loss(*args).clone()
    again = score.masked_loss(*args)
    torch.cuda.synchronize()
    assert out.dtype == torch.float64 and torch.equal(out, again)           # identical bits run to run
    got = out.tolist()
    print(f"{kind} {shape} mask={mask} t={with_t}: sum {got[0]:.17g} vs {want[0]:.17g}")
    assert close(got[0], want[0]) and close(got[1], want[1]), (got, want)
    if mask and not with_t and shape[0] > 1:     # the all-padding item adds exactly nothing
        alone = score.masked_loss(kind, dev(pred[:-1]), dev(target[:-1]), dev(npad[:-1])).tolist()
        assert close(alone[0], got[0])


# ------------------------------------------------------------------------------------------- dsd_curve_stats
@pytest.mark.parametrize("mask", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("n", [1, SPAN + 1, 5003, MAX_BLOCKS * SPAN + SPAN + 3])
def test_curve_stats_vs_ref(n, mask):
    r = np.random.Generator(np.random.PCG64(2640 + n % 89))
    target = (60.0 + 5.0 * r.standard_normal(n, dtype=np.float32)).astype(np.float32)
    pred = (target + 0.6 * r.standard_normal(n, dtype=np.float32)).astype(np.float32)
    m = None
    if mask:
        m = r.random(n) < 0.7
        m[0] = True
    want = sr.curve_stats(pred, target, m, 0.5)
    args = (dev(pred), dev(target), None if m is None else dev(m), 0.5)
    counts, sums = (v.clone() for v in score.curve_stats(*args))
    counts2, sums2 = score.curve_stats(*args)
    torch.cuda.synchronize()
    assert torch.equal(counts, counts2) and torch.equal(sums, sums2)
    assert counts.tolist() == [want["close"], want["total"]]
    for got, key in zip(sums.tolist(), ("sum_target", "sum_target_sq", "sum_residual_sq")):
        assert close(got, want[key]), (key, got, want[key])


def test_curve_tolerance_edge_is_inclusive():
    """|pred - target| exactly the tolerance counts; one ulp more does not; one ulp less does"""
    tol = np.float32(0.5)
    up, down = np.nextafter(tol, np.float32(1)), np.nextafter(tol, np.float32(0))
    target = np.array([0, 0, 0, 64, 64, 64, 0, 0, 0], np.float32)
    pred = np.array([tol, up, down, 64.5, np.nextafter(np.float32(64.5), np.float32(65)), np.nextafter(np.float32(64.5), np.float32(64)),
                     -tol, -up, -down], np.float32)
    counts, _ = score.curve_stats(dev(pred), dev(target), None, float(tol))
    assert counts.tolist() == [6, 9]
    assert sr.curve_stats(pred, target, None, tol)["close"] == 6
    acc = metrics.RawCurveAccuracy(tolerance=0.5)
    acc.update(dev(pred), dev(target))
    acc.update(dev(pred), dev(target), mask=dev(np.arange(9) < 3))
    assert (int(acc.close), int(acc.total)) == (8, 12) and float(acc.compute()) == np.float32(8) / np.float32(12)


# ------------------------------------------------------------------------------------------- dsd_dur_score
def _dur_case(b, length, max_words, seed, negative=True):
    r = np.random.Generator(np.random.PCG64(seed))
    steps = (r.random((b, length)) < (max_words / length)).astype(np.int64)
    steps[:, 0] = 1
    ph2word = np.cumsum(steps, axis=1)
    pad = r.integers(0, max(length // 3, 1), size=b)
    for i in range(b):
        if pad[i]:
            ph2word[i, length - pad[i]:] = 0
    gt = (r.integers(1, 40, size=(b, length)) * (ph2word > 0)).astype(np.float32)
    raw = (gt * (1.0 + 0.2 * r.standard_normal((b, length))) + 0.5 * r.standard_normal((b, length))).astype(np.float32)
    raw = np.where(ph2word > 0, raw, 0).astype(np.float32)
    if negative:
        raw[0, 0] = -0.5
    mask = (r.random((b, length)) < 0.8) & (ph2word > 0)
    return raw, gt, ph2word, mask


def _check_dur(res, want):
    for k in ("sums", "means"):
        for got, w in zip(res[k].tolist(), want[k]):
            assert close(got, w), (k, got, w)
    assert res["counts"].tolist() == want["counts"]
    assert np.array_equal(res["wdur_pred"].cpu().numpy(), want["wdur_pred"])
    assert np.array_equal(res["wdur_gt"].cpu().numpy(), want["wdur_gt"])


def _scatter_words(values, ph2word):
    v, w = torch.from_numpy(values), torch.from_numpy(ph2word)
    return v.new_zeros(v.shape[0], int(w.max()) + 1).scatter_add(1, w, v)[:, 1:].numpy()


@pytest.mark.parametrize("loss_type", ["mse", "huber"])
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("case", ["g25", "one_word", "padded_item", "spans"])
def test_dur_score_vs_ref(case, masked, loss_type):
    if case == "g25":
        di = sc.dur_inputs()
        raw, gt, p2w, mask = di["dur_pred_raw"], di["dur_gt"], di["ph2word"], di["mask"]
    elif case == "one_word":                    # n_words - 1 == 1
        raw, gt, p2w, mask = _dur_case(2, 5, 1, 2651)
        p2w = (p2w > 0).astype(np.int64)
    elif case == "padded_item":                 # an item that is all padding, among real ones
        raw, gt, p2w, mask = _dur_case(3, 9, 4, 2652)
        p2w[1], gt[1], raw[1], mask[1] = 0, 0, 0, False
    else:                                       # more than one workgroup's share of phonemes
        raw, gt, p2w, mask = _dur_case(41, 61, 20, 2653)
        assert raw.size > SPAN
    m = mask if masked else None
    want = sr.dur_score(raw, gt, p2w, mask=m, loss_type=loss_type)
    args = (dev(raw), dev(gt), dev(p2w), None if m is None else dev(m))
    res = {k: v.clone() for k, v in score.dur_score(*args, loss_type=loss_type).items()}
    again = score.dur_score(*args, n_words=int(p2w.max()) + 1, loss_type=loss_type)
    torch.cuda.synchronize()
    for k in res:
        assert torch.equal(res[k], again[k]), k
    _check_dur(res, want)
    # the word sums are torch's CPU scatter_add, bit for bit
    assert np.array_equal(res["wdur_pred"].cpu().numpy(), _scatter_words(np.maximum(raw, 0), p2w))
    assert np.array_equal(res["wdur_gt"].cpu().numpy(), _scatter_words(gt, p2w))


def test_dur_tolerance_edges_are_inclusive():
    """one-phoneme words: |wdur_pred - wdur_gt| against fl(wdur_gt * tolerance) at the edge and one ulp either side"""
    f = np.float32
    assert f(20) * f(0.05) == f(1)              # the rhythm edge: 20 * fl32(0.05) rounds to 1
    assert f(10) * f(0.2) == f(2)               # the phoneme edge
    gt = np.array([[20, 20, 20, 20, 10, 10, 10, 10]], np.float32)
    pred = np.array([[21, np.nextafter(f(21), f(22)), np.nextafter(f(21), f(20)), 19, 12, 13, 8, 7]], np.float32)
    p2w = np.arange(1, 9, dtype=np.int64)[None]
    want = sr.dur_score(pred, gt, p2w)
    # rhythm: 21 yes, 21+ no, 21- yes, 19 yes; 12 (|2| <= 0.5) no ...; phonemes: align = round(pred * gt / pred)
    res = score.dur_score(dev(pred), dev(gt), dev(p2w))
    assert res["counts"].tolist() == want["counts"]
    assert want["counts"][0] == 3 and want["counts"][1] == 8
    # every word is one phoneme: the regulator maps each prediction onto its target, so all eight are accurate
    assert want["counts"][2:] == [8, 8]
    # phoneme edge without the regulator's help: two phonemes share a word
    gt2 = np.array([[10, 10, 10, 10]], np.float32)
    pred2 = np.array([[12, 8, 13, 7]], np.float32)
    p2w2 = np.array([[1, 1, 2, 2]], np.int64)
    want2 = sr.dur_score(pred2, gt2, p2w2)
    assert want2["counts"][2:] == [2, 4]        # |12 - 10| <= 2 and |8 - 10| <= 2; |13 - 10| and |7 - 10| are not
    assert score.dur_score(dev(pred2), dev(gt2), dev(p2w2))["counts"].tolist() == want2["counts"]


# ------------------------------------------------------------------------------------------- modules vs the reference's scalars
def test_loss_modules_vs_golden(g):
    li = {k: dev(v) for k, v in sc.loss_inputs().items()}
    p, t_, npad, t = li["pred"], li["target"], li["non_padding"], li["t"]
    for kind in ("l1", "l2"):
        assert_scalar(g, f"diff_{kind}_masked", losses.DiffusionLoss(kind)(p, t_, non_padding=npad))
        assert_scalar(g, f"diff_{kind}", losses.DiffusionLoss(kind)(p, t_))
        assert_scalar(g, f"rf_{kind}_lognorm_masked", losses.RectifiedFlowLoss(kind, log_norm=True)(p, t_, t=t, non_padding=npad))
        assert_scalar(g, f"rf_{kind}_plain", losses.RectifiedFlowLoss(kind, log_norm=False)(p, t_, t=t))
    from diffsinger_amd.aux_decoder import build_aux_loss
    assert_scalar(g, "aux_l1", build_aux_loss("convnext")(p[:, 0].transpose(1, 2), t_[:, 0].transpose(1, 2)))
    di = sc.dur_inputs()
    lp, lw, ls = di["lambdas"]
    for kind in ("mse", "huber"):
        mod = losses.DurationLoss(di["offset"], kind, lambda_pdur=lp, lambda_wdur=lw, lambda_sdur=ls)
        assert_scalar(g, f"dur_{kind}", mod(dev(di["dur_pred_raw"]), dev(di["dur_gt"]), ph2word=dev(di["ph2word"])))


def test_metrics_vs_golden(g):
    di, ci = sc.dur_inputs(), sc.curve_inputs()
    pred, gt, p2w = dev(di["dur_pred"]), dev(di["dur_gt"]).long(), dev(di["ph2word"])
    for name, mask in (("nomask", None), ("mask", dev(di["mask"]))):
        rc = metrics.RhythmCorrectness(tolerance=di["rhythm_tolerance"])
        rc.update(pred, gt, p2w, mask=mask)
        assert [int(rc.correct), int(rc.total)] == g[f"rhythm_{name}_counts"].tolist()
        assert_scalar(g, f"rhythm_{name}", rc.compute())
        pa = metrics.PhonemeDurationAccuracy(tolerance=di["pdur_tolerance"])
        pa.update(pred, gt, p2w, mask=mask)
        assert [int(pa.accurate), int(pa.total)] == g[f"pdur_{name}_counts"].tolist()
        assert_scalar(g, f"pdur_{name}", pa.compute())
        rc.update(pred, gt, p2w, mask=mask)             # states accumulate; reset returns to the defaults
        assert int(rc.total) == 2 * int(g[f"rhythm_{name}_counts"][1])
        rc.reset()
        assert int(rc.total) == 0 and int(rc.correct) == 0
    cp, cg = dev(ci["pred"]), dev(ci["target"])
    for name, mask in (("nomask", None), ("mask", dev(ci["mask"]))):
        acc = metrics.RawCurveAccuracy(tolerance=ci["tolerance"])
        acc.update(cp, cg, mask=mask)
        assert [int(acc.close), int(acc.total)] == g[f"curve_{name}_counts"].tolist()
        assert_scalar(g, f"curve_acc_{name}", acc.compute())
        r2 = metrics.RawCurveR2Score()
        r2.update(cp, cg, mask=mask)
        got = [float(r2.sum_error), float(r2.sum_squared_error), float(r2.residual)]
        for a, b in zip(got, g[f"curve_{name}_sums64"].tolist()):
            assert close(a, b)
        assert_scalar(g, f"curve_r2_{name}", r2.compute())
    with pytest.raises(AssertionError):
        metrics.RhythmCorrectness(tolerance=0.05).update(-pred.float(), gt, p2w)


# ------------------------------------------------------------------------------------------- forward_score
def make_wrapper(tag, g=None):
    from diffsinger_amd import diffusion
    c = sc.WRAPPERS[tag]
    w = getattr(diffusion, c["cls"])(**sc.wrapper_kwargs(tag))
    f, m = sc.dims(tag)
    params = synth.synth_state_dict(synth.backbone_param_shapes(c["backbone"], m, f, hidden_size=sc.HIDDEN, **c["args"]), seed=c["wseed"])
    if g is not None:
        assert synth.state_dict_digest(params) == str(g[f"{tag}_digest"])
    load_synth(w._backbone(), params)
    return w.cuda().eval()


def wrapper_args(tag):
    inp = sc.wrapper_inputs(tag)
    gt = [dev(v) for v in inp["gt"]] if isinstance(inp["gt"], list) else dev(inp["gt"])
    return inp, dev(inp["cond"]), gt


@pytest.mark.parametrize("tag", sorted(sc.WRAPPERS))
def test_forward_score_vs_golden(g, tag):
    c = sc.WRAPPERS[tag]
    w = make_wrapper(tag, g)
    inp, cond, gt = wrapper_args(tag)
    t, eps = dev(inp["t"]), dev(g[f"{tag}_noise"])
    out = w.forward_score(cond, gt, t=t, noise=eps)
    again = w.forward_score(cond, gt, t=t, noise=eps)
    torch.cuda.synchronize()
    assert len(out) == (2 if c["family"] == "ddpm" else 3)
    assert all(torch.equal(a, b) for a, b in zip(out, again))
    pred, target = out[0], out[1]
    assert not pred.requires_grad
    mx = check(pred, g[f"{tag}_pred"], TOL_NFE, what=("G25", tag))
    print(f"G25 {tag}: {mx:.3g}")
    assert np.array_equal(target.cpu().numpy(), g[f"{tag}_target"])         # as the reference returns it
    if c["family"] == "reflow":
        assert out[2].dtype == torch.float32 and np.array_equal(out[2].cpu().numpy(), inp["t"])
    # the loss modules on the REFERENCE's outputs: the fixture's distance rule ...
    npad = dev(inp["non_padding"])
    rp, rt = dev(g[f"{tag}_pred"]), dev(g[f"{tag}_target"])
    for kind in ("l1", "l2"):
        mod = losses.DiffusionLoss(kind) if c["family"] == "ddpm" else losses.RectifiedFlowLoss(kind, log_norm=True)
        extra = {} if c["family"] == "ddpm" else {"t": t}
        assert_scalar(g, f"{tag}_{kind}", mod(rp, rt, non_padding=npad, **extra))
        # ... and on forward_score's own: the network output is within delta = TOL_NFE * max|ref| of the reference's, so
        # with w_max the largest log-norm weight (1 for DDPM) the mean moves by at most w_max * delta (l1) or
        # w_max * (2 delta sqrt(mean d^2) + delta^2) (l2, Cauchy-Schwarz; mean d^2 <= the unweighted l2 loss)
        mine = float(mod(pred, target, non_padding=npad, **extra))
        delta = TOL_NFE * float(np.abs(g[f"{tag}_pred"]).max())
        w_max = 1.0 if c["family"] == "ddpm" else float(sr.lognorm_weight(inp["t"]).max())
        d2 = sr.masked_loss("l2", g[f"{tag}_pred"], g[f"{tag}_target"], inp["non_padding"][..., 0])[1]
        room = w_max * (delta if kind == "l1" else 2 * delta * np.sqrt(d2) + delta * delta)
        r32, bound = ref_bound(g, f"{tag}_{kind}")
        assert abs(mine - r32) <= bound + room, (tag, kind, mine, r32, bound, room)
    w._backbone().release_native()


@pytest.mark.parametrize("tag", ["ddpm_wn", "reflow_lx"])
def test_forward_score_default_draws_are_torchs_in_the_references_order(tag):
    """t first, then the noise, each where and as the reference draws it"""
    c = sc.WRAPPERS[tag]
    w = make_wrapper(tag)
    inp, cond, gt = wrapper_args(tag)
    torch.manual_seed(77)
    out = w.forward_score(cond, gt)
    torch.manual_seed(77)
    if c["family"] == "ddpm":
        t = torch.randint(0, w.k_step, (sc.B,), device="cuda").long()
    else:
        t = w.t_start + (1.0 - w.t_start) * torch.rand((sc.B,), device="cuda")
    # randn_like on the normalised spectrogram as the wrappers hold it: [B, 1, M, T], a transposed view of [B, T, M]
    eps = torch.randn_like(torch.empty((sc.B, c["T"], 16), device="cuda").transpose(-2, -1)[:, None])
    want = w.forward_score(cond, gt, t=t, noise=eps)
    assert all(torch.equal(a, b) for a, b in zip(out, want))
    if c["family"] == "ddpm":
        assert torch.equal(out[1], eps)
    w._backbone().release_native()


@pytest.mark.parametrize("tag", ["ddpm_wn", "multi_reflow"])
def test_forward_score_seeded(tag):
    c = sc.WRAPPERS[tag]
    w = make_wrapper(tag)
    inp, cond, gt = wrapper_args(tag)
    npad = dev(inp["non_padding"])
    mod = losses.DiffusionLoss("l2") if c["family"] == "ddpm" else losses.RectifiedFlowLoss("l2")

    def loss(out):
        return mod(out[0], out[1], non_padding=npad) if c["family"] == "ddpm" else mod(out[0], out[1], out[2], non_padding=npad)

    seeds = [11, 12, (1 << 40) + 13]
    a, b = w.forward_score(cond, gt, seed=seeds), w.forward_score(cond, gt, seed=seeds)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and torch.equal(loss(a), loss(b))      # the same seed, the same loss
    other = w.forward_score(cond, gt, seed=[21, 22, 23])
    assert not torch.equal(other[1], a[1]) and float(loss(other)) != float(loss(a))
    same = w.forward_score(cond, gt, seed=11)                   # an int: every item under it
    assert torch.equal(same[1][0], a[1][0])
    # item b does not depend on the batch it is scored in
    for i in range(sc.B):
        gi = [v[i:i + 1] for v in gt] if isinstance(gt, list) else gt[i:i + 1]
        lone = w.forward_score(cond[i:i + 1], gi, seed=seeds[i])
        assert torch.equal(lone[1][0], a[1][i])                 # the target: bit for bit
        if c["family"] == "reflow":
            assert torch.equal(lone[2][0], a[2][i])
        check(lone[0][0], a[0][i].cpu().numpy(), TOL_NFE, what=("lone item", tag, i))
    # the t rule on the device's own uniform draw
    u = noise.fill((1, sc.B, 1, 1), seeds, noise.SCORE_T, kind="uniform").reshape(-1).cpu().numpy()
    if c["family"] == "reflow":
        assert np.array_equal(a[2].cpu().numpy(), sr.seeded_t_reflow(u, w.t_start))
    else:
        t = dev(sr.seeded_t_ddpm(u, w.k_step))
        eps = noise.fill((1, sc.B, 16, c["T"]), seeds, noise.SCORE_NOISE)[0].view(sc.B, 1, 16, c["T"])
        explicit = w.forward_score(cond, gt, t=t, noise=eps)
        assert torch.equal(explicit[0], a[0]) and torch.equal(explicit[1], a[1])
    for kw in (dict(t=dev(inp["t"])), dict(noise=a[1])):
        with pytest.raises(ValueError, match="seed"):
            w.forward_score(cond, gt, seed=3, **kw)
    w._backbone().release_native()


def test_refusals_stand():
    """forward(infer=False) and p_losses still raise; a backbone call outside no_grad on parameters that require grad still
    raises "inference-only"."""
    for tag in ("ddpm_wn", "reflow_lx"):
        w = make_wrapper(tag)
        inp, cond, gt = wrapper_args(tag)
        with pytest.raises(NotImplementedError, match="inference-only"):
            w(cond, gt_spec=gt, infer=False)
        with pytest.raises(NotImplementedError):
            w.p_losses(gt, dev(inp["t"]), cond)
        net = w._backbone()
        assert any(p.requires_grad for p in net.parameters())
        with pytest.raises(RuntimeError, match="inference-only"):
            net(torch.zeros(1, 1, 16, 8, device="cuda"), torch.zeros(1, device="cuda"), torch.zeros(1, 256, 8, device="cuda"))
        net.release_native()
