"""-m gpu: dsd_sample as the public interpreter of dsd_program, on programs at the limits of the format.

The rest of the suite runs only the nine built-in samplers' programs through dsd_sample; tests/program_cases.py has what those
never contain (8-term combinations, exactly 8 and 9 state terms over three outputs, several noise terms in several outputs, the
model term twice, swaps, 64 buffers, a model-free output as the next input, ...), each vetted on the CPU by
tests/test_program_cases_host.py: every term of every program is live, so a kernel that drops or misreads one fails here.

Every program runs on every row of program_cases.ROWS -the four pieces of device code that implement the format: wn_edge_kernel, and
gemm_kernel<S, 1, EP_LINCOMB = 3, ..> behind WaveNet's folded fp32 staging (S = 5), the split-bf16 handle's plain staging (0) and
LYNXNet's LayerNorm staging (2), on the fast and the generic path and at both tile widths - dense and ragged, and is compared
with tests/prog_sim.py on the oracle backbone over EVERY buffer it wrote and buffer 0 (one device run per buffer, result_buf
set to it), at test_gpu_parity's full-sampler tolerance, max and RMS.  A ragged batch is compared per item on its valid frames
with the program run alone at that length on the same slices of the noise.  Which kernel ended each evaluation is read from the
launch ledger: the edge kernel exactly the evaluations run_wavenet's rule gives it (no noise term, at most 8 state terms), the
row's EP_LINCOMB instantiation all the others.  On the edge rows the same program also runs with DSD_EDGE=0 and the two paths
agree to the 2e-6 of test_gpu_edge.py.

Then: eager = graph = lazy graph bit for bit; the graph cache's key (a coefficient, a time, result_buf, the noise pointer, the
lengths); no leftovers from a 64-buffer program; and one refused call per fail() of dsd_sample's validation block, the duplicate
destination included - DSD_EINVAL (DSD_ESTATE before dsd_prepare_cond), the field named, nothing launched, the handle usable.
"""
import copy
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_ledger_cases as lc  # noqa: E402
import program_cases as pc  # noqa: E402
from diffsinger_amd import _lib  # noqa: E402
from diffsinger_amd.diffusion import _SamplerMixin  # noqa: E402
from gpu_util import check, dev, make_backbone, set_hp  # noqa: E402
from prog_sim import run_program  # noqa: E402
from test_gpu_first_capture import SWITCHES  # noqa: E402
from test_gpu_parity import TOL_SAMPLER  # noqa: E402
from test_kernel_registry import demangle  # noqa: E402

TOL_EDGE = 2e-6         # test_gpu_edge.py: the edge kernel against the three GEMMs, a whole loop (the model term joins the sum last)
DSD_EINVAL, DSD_ESTATE = -1, -2
LINCOMB = re.compile(r"gemm_kernel<\d+, 1, 3,")         # any EP_LINCOMB instantiation
EDGE = "wn_edge_kernel<"

ROWS, ROW = pc.ROWS, pc.ROW
MAIN = [(r.id, mode, name) for r in ROWS for mode in ("dense", "ragged")
        for name in (r.programs or tuple(pc.HAND)) + (tuple(pc.GENERATED) if r.seeds else ())]


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


@pytest.fixture(scope="module")
def names():
    """the ledger's entries in registry order, as 'kernel<template arguments>'"""
    rows = _lib.kernel_ledger()
    assert rows and all(sym for sym, _, _ in rows)
    return [re.sub(r"^void dsd::|\(.*$", "", n) for n in demangle([sym for sym, _, _ in rows])]


def launches(names):
    return {n: c for n, (_, _, c) in zip(names, _lib.kernel_ledger()) if c}


# ------------------------------------------------------------------------------------------------ handles, inputs, references
_handles, _inputs, _refs = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    for rig in _handles.values():
        rig.net.release_native()
    _handles.clear()
    _inputs.clear()
    _refs.clear()


def make_rig(net_name):
    kind, in_dims, n_feats, args, seed = lc.NETS[net_name]
    net, _params = make_backbone(kind, in_dims, n_feats, args, seed)
    runner = type("R", (_SamplerMixin,), {})()
    runner.denoise_fn = net
    oracle, fm = pc.oracle_of(net_name)         # the same synthetic weights (gpu_util.synth_params)
    return SimpleNamespace(name=net_name, net=net, runner=runner, oracle=oracle, fm=fm)


def rig_of(net_name, purpose="main-f32"):
    """one handle per (net, purpose): the main comparisons share theirs, the graph tests have their own (their cache counts)"""
    if (net_name, purpose) not in _handles:
        _handles[(net_name, purpose)] = make_rig(net_name)
    return _handles[(net_name, purpose)]


def inputs(rig, bsz, t_len):
    """x [B, F, M, T], cond [B, 256, T], noise 3 x [B, F, M, T]: numpy, and on the device (kept: prepare_cond keys on the pointer)"""
    key = (rig.name, bsz, t_len)
    if key not in _inputs:
        x, cond, noise = pc.host_inputs(rig.fm, bsz, t_len)
        _inputs[key] = SimpleNamespace(x=x, cond=cond, noise=noise, xd=dev(x), cd=dev(cond), nd=dev(noise))
    return _inputs[key]


def reference(rig, name, grid, prog=None):
    """prog_sim on the oracle backbone, computed once per (net, program, grid) and shared: dense -> the list of all buffers; ragged
    -> per item, the buffers of the program run alone on the item's valid frames with the noise sliced the same way"""
    bsz, t_len, lengths = grid
    key = (rig.name, name, grid)
    if key not in _refs:
        prog = prog or pc.PROGRAMS[name]
        i = inputs(rig, bsz, t_len)
        if lengths is None:
            _refs[key] = run_program(prog, rig.oracle, i.x, i.cond, i.noise, all_bufs=True)
        else:
            _refs[key] = [run_program(prog, rig.oracle, i.x[b:b + 1, ..., :n], i.cond[b:b + 1, :, :n], i.noise[:, b:b + 1, ..., :n], all_bufs=True)
                          for b, n in enumerate(lengths)]
    return _refs[key]


def sample(rig, prog, grid, buf=None, graph=False, noise=None, **kw):
    """one dsd_sample call of `prog` with result_buf = buf on the grid's inputs (the handle's lengths are the caller's to set)"""
    i = inputs(rig, grid[0], grid[1])
    rig.runner.use_graph = graph
    p = prog if buf is None else pc.with_result(prog, buf)
    out = rig.runner._run_program((p,) + _lib.program_to_c(p), i.cd, i.xd, noise=i.nd if noise is None else noise, **{"transpose": False, **kw})
    torch.cuda.synchronize()            # the C program is freed on return
    return out.clone()


class lengths_set:
    def __init__(self, rig, grid):
        self.rig, self.lengths = rig, grid[2]

    def __enter__(self):
        self.rig.net.set_lengths(None if self.lengths is None else list(self.lengths), torch.device("cuda"))

    def __exit__(self, *a):
        self.rig.net.set_lengths(None, torch.device("cuda"))


def items(grid):
    """(slice over the batch, valid frames) of what a comparison covers: the whole dense batch, or each item of a ragged one"""
    bsz, t_len, lengths = grid
    return [(slice(0, bsz), t_len)] if lengths is None else [(slice(b, b + 1), n) for b, n in enumerate(lengths)]


def compare(got, want, grid, tol, what):
    """got [B, F, M, T] against the dense reference buffer, or per item against the list of the items' references (numpy)"""
    for k, (bs, n) in enumerate(items(grid)):
        check(got[bs, ..., :n], (want if grid[2] is None else want[k])[..., :n], tol, what=what + (k,))


def equal_on_valid(a, b, grid):
    return all(torch.equal(a[bs, ..., :n], b[bs, ..., :n]) for bs, n in items(grid))


# ------------------------------------------------------------------------------------------------ every program on every path
@pytest.mark.parametrize("row_id,mode,name", MAIN, ids=["-".join(c) for c in MAIN])
def test_program_on_path_vs_prog_sim_with_the_ledger(row_id, mode, name, names):
    row, prog = ROW[row_id], pc.PROGRAMS[name]
    grid = row.dense if mode == "dense" else row.ragged
    rig = rig_of(row.net, "main-" + row.precision)          # (a split-bf16 handle stays one: switching re-packs the weights)
    os.environ.update(row.env)
    rig.net.set_precision(row.precision)
    if grid[2] is not None:        # the tiles the ragged call skips hold a dense call's values, not a fresh arena's zeros
        sample(rig, prog, grid)
    with lengths_set(rig, grid):
        bufs = pc.compared(prog)
        _lib.kernel_ledger_reset()
        got = {bufs[0]: sample(rig, prog, grid, bufs[0])}
        ran = launches(names)
        got.update((b, sample(rig, prog, grid, b)) for b in bufs[1:])
        want = reference(rig, name, grid)
        for b in bufs:
            compare(got[b], want[b] if grid[2] is None else [w[b] for w in want], grid, TOL_SAMPLER, (row_id, mode, name, "buffer", b))
        if 0 not in pc.written(prog):           # ... and the start comes back as it went in
            assert equal_on_valid(got[0], inputs(rig, grid[0], grid[1]).xd, grid)

        # which kernel ended the evaluations
        n_edge = sum(c for n, c in ran.items() if n.startswith(EDGE))
        lin = {n: c for n, c in ran.items() if LINCOMB.match(n)}
        print(row_id, mode, name, "edge launches", n_edge, "EP_LINCOMB", lin)
        if row.form is None:
            takes = sum(pc.edge_takes(ev) for ev in prog.evals)
            assert n_edge == takes and sum(lin.values()) == len(prog.evals) - takes, (ran, takes)
            assert any(n.startswith(EDGE) for n in ran) or takes == 0
            if any(pc.noise_terms(ev) for ev in prog.evals):
                assert lin, "a noise term goes to the GEMMs"
            if name == "edge_over":
                assert not any(n.startswith(EDGE) for n in ran), ran
            if name == "edge_full":
                assert n_edge == len(prog.evals) and not lin, ran
        else:
            assert n_edge == 0 and lin and all(n.startswith(row.form) for n in lin), (row.form, ran)
            assert sum(lin.values()) == len(prog.evals), lin
            assert all(n.endswith(f", {0 if grid[2] is None else 1}>") for n in lin), lin         # the dense / the ragged twin

        if row.form is None:        # the same program on the three GEMMs
            os.environ["DSD_EDGE"] = "0"
            _lib.kernel_ledger_reset()
            for b in bufs:
                gemm = sample(rig, prog, grid, b).cpu().numpy()
                compare(got[b], gemm if grid[2] is None else [gemm[bs] for bs, _ in items(grid)], grid, TOL_EDGE,
                        (row_id, mode, name, "edge kernel vs GEMMs, buffer", b))
            assert not any(n.startswith(EDGE) for n in launches(names))


@pytest.mark.parametrize("mode", ["dense", "ragged"])
@pytest.mark.parametrize("name", sorted(pc.HAND))
def test_transposed_output_with_per_row_scale_and_shift(name, mode):
    """DSD_SAMPLE_TRANSPOSE on F = 2 features of 24 bins: out [B, F, T, M] = sample * out_scale[f * M + m] + out_shift[f * M + m]"""
    row, prog = ROW["edge-c192-fm48"], pc.PROGRAMS[name]
    grid = row.dense if mode == "dense" else row.ragged
    rig = rig_of(row.net)
    os.environ.update(row.env)
    f, m = rig.fm
    rng = np.random.Generator(np.random.PCG64(7))
    scale, shift = (0.5 + rng.random(f * m)).astype(np.float32), rng.standard_normal(f * m).astype(np.float32)
    with lengths_set(rig, grid):
        got = sample(rig, prog, grid, transpose=True, scale=dev(scale), shift=dev(shift))
    assert tuple(got.shape) == (grid[0], f, grid[1], m)
    want = reference(rig, name, grid)
    for k, (bs, n) in enumerate(items(grid)):
        ref = (want if grid[2] is None else want[k])[prog.result_buf]
        ref = np.swapaxes(ref * scale.reshape(1, f, m, 1) + shift.reshape(1, f, m, 1), 2, 3)
        check(got[bs, :, :n], ref, TOL_SAMPLER, what=("transposed", name, mode, k))


# ------------------------------------------------------------------------------------------------ eager, graph, lazy graph
GRAPH_ROWS = ("edge-c256", "gemm-folded")


@pytest.mark.parametrize("name", sorted(pc.PROGRAMS))
@pytest.mark.parametrize("row_id", GRAPH_ROWS)
def test_graph_and_lazy_graph_equal_eager(row_id, name):
    row, prog = ROW[row_id], pc.PROGRAMS[name]
    grid = row.dense
    rig = rig_of(row.net, "graph-" + row_id)
    os.environ.update(row.env)
    bufs = pc.compared(prog)
    eager = {b: sample(rig, prog, grid, b) for b in bufs}
    cached = lambda: rig.net.stats()["graphs_cached"]  # noqa: E731
    c0 = cached()
    first = sample(rig, prog, grid, bufs[0], graph="lazy")         # first sight: runs eagerly
    c1 = cached()
    second = sample(rig, prog, grid, bufs[0], graph="lazy")        # comes back: captured and launched
    c2 = cached()
    assert c1 == c0 and c2 == (c0 + 1 if c0 < 16 else 1), (c0, c1, c2)
    assert torch.equal(first, eager[bufs[0]]) and torch.equal(second, eager[bufs[0]])
    for b in bufs:                      # result_buf is not part of the key: replays of the one graph
        assert torch.equal(sample(rig, prog, grid, b, graph=True), eager[b]), (row_id, name, b)
    assert cached() == c2


def _last_writer(prog):
    """(evaluation, output) of the last write to result_buf, which must have a model term: its coefficients and its t show there"""
    i, o = [(i, o) for i, ev in enumerate(prog.evals) for o, (d, _) in enumerate(ev.outs) if d == prog.result_buf][-1]
    assert any(s == pc.M for s, _ in prog.evals[i].outs[o][1])
    return i, o


def _other_coef(prog):
    p = copy.deepcopy(prog)
    i, o = _last_writer(p)
    ts = p.evals[i].outs[o][1]
    ts[-1] = (ts[-1][0], float(np.float32(-0.75 * ts[-1][1])))
    return p


def _other_t(prog):
    p = copy.deepcopy(prog)
    ev = p.evals[_last_writer(p)[0]]
    ev.t = float(np.float32(ev.t * 0.5 + 17.0))
    return p


@pytest.mark.parametrize("name", ["noise3", "gen8"])
@pytest.mark.parametrize("row_id", GRAPH_ROWS)
def test_graph_key_tells_programs_noise_and_lengths_apart(row_id, name):
    """back to back on one handle with DSD_SAMPLE_GRAPH: whatever the key misses replays the wrong graph"""
    row, prog = ROW[row_id], pc.PROGRAMS[name]
    dense, rag1, rag2 = (3,) + row.ragged[1:2] + (None,), row.ragged, (3, row.ragged[1], (33, row.ragged[1], 2))
    rig = rig_of(row.net, "graph-" + row_id)
    os.environ.update(row.env)
    i = inputs(rig, 3, row.ragged[1])
    other_buf = next(b for b in pc.compared(prog) if b != prog.result_buf)
    variants = [("program", prog), ("one coefficient changed", _other_coef(prog)), ("one t changed", _other_t(prog)),
                ("result_buf changed", pc.with_result(prog, other_buf))]
    eager = {what: sample(rig, p, dense) for what, p in variants}
    outs = list(eager.values())
    assert not any(torch.equal(a, b) for k, a in enumerate(outs) for b in outs[k + 1:]), "the variants must differ in their results"
    eager_rag = {}
    for g in (rag1, rag2):
        with lengths_set(rig, g):
            eager_rag[g] = sample(rig, prog, g)

    for what, p in variants:
        assert torch.equal(sample(rig, p, dense, graph=True), eager[what]), (row_id, name, what)
    # the same values in a newly allocated tensor, the old tensor (still alive: another address) overwritten
    old = i.nd.clone()
    assert torch.equal(sample(rig, prog, dense, graph=True, noise=old), eager["program"])
    fresh = old.clone()
    old.copy_(torch.flip(old, dims=(0,)) * 3.0 + 1.0)
    assert fresh.data_ptr() != old.data_ptr()
    assert torch.equal(sample(rig, prog, dense, graph=True, noise=fresh), eager["program"]), (row_id, name, "noise pointer")
    # two sets of lengths, back to the first, and back to dense
    for g in (rag1, rag2, rag1):
        with lengths_set(rig, g):
            assert equal_on_valid(sample(rig, prog, g, graph=True), eager_rag[g], g), (row_id, name, g)
    assert torch.equal(sample(rig, prog, dense, graph=True), eager["program"]), (row_id, name, "dense after ragged")


@pytest.mark.parametrize("row_id", GRAPH_ROWS)
def test_no_leftovers_of_a_64_buffer_program(row_id):
    """bufs64 and then swap on one handle give the bits of swap on a fresh handle"""
    row = ROW[row_id]
    os.environ.update(row.env)
    used, fresh = make_rig(row.net), make_rig(row.net)
    try:
        for b in pc.compared(pc.HAND["bufs64"]):
            sample(used, pc.HAND["bufs64"], row.dense, b)
        for b in pc.compared(pc.HAND["swap"]):
            assert torch.equal(sample(used, pc.HAND["swap"], row.dense, b), sample(fresh, pc.HAND["swap"], row.dense, b)), (row_id, b)
    finally:
        used.net.release_native()
        fresh.net.release_native()


# ------------------------------------------------------------------------------------------------ refusals before any launch
def _set(path, value):
    """a mutation of the C program: path = attribute names / indices from the DsdProgram or ('ev', i, ...) from evaluation i"""
    def mutate(p, evals):
        obj, steps = (evals, path[1:]) if path[0] == "ev" else (p, path)
        for step in steps[:-1]:
            obj = obj[step] if isinstance(step, int) else getattr(obj, step)
        setattr(obj, steps[-1], value)
    return mutate


def _null_evals(p, evals):
    p.evals = C.POINTER(_lib.DsdEval)()


NB = pc.HAND["noise3"].n_bufs
NOISE_BASE = _lib.DSD_SRC_NOISE_BASE
# (id, mutation, pass the noise tensors, the field dsd_last_error must name)
REFUSALS = [
    ("n_bufs-0", _set(("n_bufs",), 0), True, "n_bufs"),
    ("n_bufs-65", _set(("n_bufs",), 65), True, "n_bufs"),
    ("n_evals-negative", _set(("n_evals",), -1), True, "n_evals"),
    ("evals-null", _null_evals, True, "evals == null"),
    ("result_buf-high", _set(("result_buf",), NB), True, "result_buf"),
    ("result_buf-negative", _set(("result_buf",), -1), True, "result_buf"),
    ("x_buf-high", _set(("ev", 1, "x_buf"), NB), True, "x_buf"),
    ("x_buf-negative", _set(("ev", 0, "x_buf"), -1), True, "x_buf"),
    ("n_out-0", _set(("ev", 1, "n_out"), 0), True, "n_out"),
    ("n_out-4", _set(("ev", 1, "n_out"), 4), True, "n_out"),
    ("dst-high", _set(("ev", 1, "out", 1, "dst"), NB), True, "dst"),
    ("dst-negative", _set(("ev", 0, "out", 0, "dst"), -1), True, "dst"),
    ("dst-duplicate", _set(("ev", 1, "out", 1, "dst"), 3), True, "duplicate dst"),
    ("n_terms-0", _set(("ev", 2, "out", 0, "n_terms"), 0), True, "n_terms"),
    ("n_terms-9", _set(("ev", 0, "out", 1, "n_terms"), 9), True, "n_terms"),
    ("src-buffer-high", _set(("ev", 2, "out", 0, "terms", 1, "src"), NB), True, "src"),
    ("src-noise-index-high", _set(("ev", 0, "out", 0, "terms", 2, "src"), NOISE_BASE - 3), True, "src"),
    ("src-between-model-and-noise", _set(("ev", 0, "out", 0, "terms", 0, "src"), -2), True, "src"),
    ("src-just-above-noise-base", _set(("ev", 1, "out", 0, "terms", 3, "src"), NOISE_BASE + 1), True, "src"),
    ("noise-null", None, False, "noise == null"),
]


def _raw_sample(rig, handle, cprog, i, with_noise=True):
    out = torch.empty_like(i.xd)
    rc = _lib.lib().dsd_sample(handle, C.byref(cprog), C.c_void_p(i.xd.data_ptr()), C.c_void_p(i.nd.data_ptr()) if with_noise else None,
                               C.c_void_p(out.data_ptr()), None, None, 0, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, _lib.lib().dsd_last_error(handle).decode("utf-8", "replace"), out


@pytest.fixture(scope="module")
def good():
    """noise3 on the first row, checked against prog_sim once: what a valid call after a refused one must give again"""
    row = ROW["edge-c256"]
    set_hp()
    saved = os.environ.get("DSD_EDGE")
    os.environ["DSD_EDGE"] = "1"
    try:
        rig = rig_of(row.net)
        out = sample(rig, pc.HAND["noise3"], row.dense)
        compare(out, reference(rig, "noise3", row.dense)[0], row.dense, TOL_SAMPLER, ("refusals: the valid call",))
    finally:
        os.environ.pop("DSD_EDGE", None)
        if saved is not None:
            os.environ["DSD_EDGE"] = saved
    return out


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_malformed_program_is_refused_before_any_launch(case, good, names):
    _, mutate, with_noise, field = case
    row, prog = ROW["edge-c256"], pc.HAND["noise3"]
    rig = rig_of(row.net)
    os.environ.update(row.env)
    i = inputs(rig, row.dense[0], row.dense[1])
    handle = rig.net.prepare_cond(i.cd)
    cprog, evals = _lib.program_to_c(prog)
    if mutate:
        mutate(cprog, evals)
    torch.cuda.synchronize()
    _lib.kernel_ledger_reset()
    rc, msg, _ = _raw_sample(rig, handle, cprog, i, with_noise)
    assert rc == DSD_EINVAL, (rc, msg)
    assert field in msg.lower(), msg
    assert not launches(names), launches(names)
    assert torch.equal(sample(rig, prog, row.dense), good)


def test_sample_before_prepare_cond_is_refused(good, names):
    row, prog = ROW["edge-c256"], pc.HAND["noise3"]
    os.environ.update(row.env)
    rig = make_rig(row.net)
    try:
        i = inputs(rig, row.dense[0], row.dense[1])
        handle = rig.net.native_handle(torch.device("cuda"))
        cprog, _evals = _lib.program_to_c(prog)
        torch.cuda.synchronize()
        _lib.kernel_ledger_reset()
        rc, msg, _ = _raw_sample(rig, handle, cprog, i)
        assert rc == DSD_ESTATE and "dsd_prepare_cond" in msg, (rc, msg)
        assert not launches(names), launches(names)
        assert torch.equal(sample(rig, prog, row.dense), good)
    finally:
        rig.net.release_native()
