"""Programs at the limits of the dsd_program format (include/dsdenoise.h), as plain schedule.Program / schedule.Eval data: the
cases of tests/test_gpu_programs.py, vetted on the CPU by tests/test_program_cases_host.py.

The nine built-in samplers' programs stay well inside the format: at most 6 terms per combination, at most 7 state terms in an
evaluation the edge kernel takes, one noise term in one output, 7 buffers, the model term once.  The programs here go to the
format's edges.  They are built term by term, not through schedule.Lin, which merges duplicate sources.

* gen(seed): random programs - x_buf drawn from the buffers defined so far (buffer 0 on entry, the others once written: a
  program never reads a buffer it has not written, the library does not clear them between calls), t in [0, 1000), 1-3 outputs
  with distinct destinations, 1-8 distinct sources each from {MODEL, defined buffers, noise 0 .. n_noise-1}, coefficients of
  magnitude in [0.05, 1] with a random sign, scaled to unit 2-norm per combination and rounded to fp32.  SEEDS lists the seeds
  whose programs have every term live (test_program_cases_host.py asserts it: dropping any one term moves a compared buffer by
  1e-3 of its peak); the seeds between them have terms whose result is overwritten unread, and a comparison proves nothing
  about those.
* HAND: named limit programs of 2-4 evaluations; the docstring line of each says what it pins, FEATURES states it as a
  predicate over the program, and the host test asserts that the list as a whole has every feature.

* ROWS: the paths the programs run on - net, grids, path switches and the EP_LINCOMB instantiation that must end the evaluations.

A test compares every buffer a program wrote, and buffer 0 (compared()): on the device by running the program once per such
buffer with result_buf set to it (with_result).
"""
import copy
from collections import namedtuple

import numpy as np

from diffsinger_amd.schedule import MODEL, NOISE_BASE, Eval, Program, noise_src

M = MODEL
N0, N1, N2 = noise_src(0), noise_src(1), noise_src(2)
MAX_TERMS, MAX_OUT, MAX_BUFS, EDGE_MAX_STATE = 8, 3, 64, 8        # DSD_MAX_TERMS, DSD_MAX_OUT, n_bufs <= 64, kEdgeMaxTerms


def _f32(c):
    return float(np.float32(c))


def unit(*terms):
    """[(src, coef)] scaled to unit 2-norm, coefficients rounded to fp32"""
    n = float(np.sqrt(sum(c * c for _, c in terms)))
    return [(s, _f32(c / n)) for s, c in terms]


def raw(*terms):
    return [(s, _f32(c)) for s, c in terms]


# ------------------------------------------------------------------------------------------------ inspection
def is_noise(src):
    return src <= NOISE_BASE


def state_terms(ev):
    """terms of all outputs that read a state buffer: what the edge kernel holds at most EDGE_MAX_STATE of"""
    return sum(1 for _, ts in ev.outs for s, _ in ts if s >= 0)


def noise_terms(ev):
    return sum(1 for _, ts in ev.outs for s, _ in ts if is_noise(s))


def edge_takes(ev):
    """run_wavenet's rule: no caller-noise term and at most EDGE_MAX_STATE state terms, else the GEMMs of gemm.hip"""
    return noise_terms(ev) == 0 and state_terms(ev) <= EDGE_MAX_STATE


def written(prog):
    return sorted({d for ev in prog.evals for d, _ in ev.outs})


def compared(prog):
    """the buffers a test compares: every buffer the program wrote, and buffer 0"""
    return sorted(set(written(prog)) | {0})


def with_result(prog, buf):
    p = copy.copy(prog)
    p.result_buf = buf
    return p


def all_terms(prog):
    """[(eval, output, term)] of every term"""
    return [(i, o, k) for i, ev in enumerate(prog.evals) for o, (_, ts) in enumerate(ev.outs) for k in range(len(ts))]


def without_term(prog, i, o, k):
    """the program with one term's coefficient set to zero (the structure stays: a one-term combination keeps its term)"""
    p = copy.deepcopy(prog)
    ts = p.evals[i].outs[o][1]
    ts[k] = (ts[k][0], 0.0)
    return p


def well_formed(prog):
    """what the generator promises and dsd_sample's validation block requires; reads only written buffers"""
    assert 1 <= prog.n_bufs <= MAX_BUFS and 0 <= prog.result_buf < prog.n_bufs
    defined = {0}
    for ev in prog.evals:
        assert ev.x_buf in defined and 0.0 <= ev.t < 1000.0
        assert 1 <= len(ev.outs) <= MAX_OUT and len({d for d, _ in ev.outs}) == len(ev.outs)
        for dst, ts in ev.outs:
            assert 0 <= dst < prog.n_bufs and 1 <= len(ts) <= MAX_TERMS
            for s, c in ts:
                assert s == M or s in defined or (is_noise(s) and NOISE_BASE - s < prog.n_noise), (s, sorted(defined))
                assert c == _f32(c)
        defined |= {d for d, _ in ev.outs}
    return True


# ------------------------------------------------------------------------------------------------ generated programs
def gen(seed, n_bufs=8, n_evals=5, n_noise=3):
    rng = np.random.Generator(np.random.PCG64(seed))
    defined, evals = [0], []
    for _ in range(n_evals):
        x_buf = defined[int(rng.integers(len(defined)))]
        ev = Eval(x_buf, _f32(rng.uniform(0.0, 1000.0)))
        pool = [M] + defined + [noise_src(k) for k in range(n_noise)]
        dsts = [int(d) for d in rng.choice(n_bufs, size=int(rng.integers(1, MAX_OUT + 1)), replace=False)]
        for dst in dsts:
            n_terms = int(rng.integers(1, min(MAX_TERMS, len(pool)) + 1))
            srcs = [pool[int(j)] for j in rng.choice(len(pool), size=n_terms, replace=False)]
            coefs = rng.uniform(0.05, 1.0, size=n_terms) * rng.choice([-1.0, 1.0], size=n_terms)
            ev.outs.append((dst, unit(*zip(srcs, coefs))))
        defined = sorted(set(defined) | set(dsts))
        evals.append(ev)
    return Program(n_bufs, defined[int(rng.integers(len(defined)))], evals, n_noise)


# Of seeds 0-39, 27 give a program with every term live.  These eight have between them combinations of 8 terms, evaluations of
# 1, 2 and 3 outputs, up to 9 noise terms in one evaluation, evaluations of 8, 9 and 10 state terms, and evaluations without a
# noise term (which the edge kernel takes where it is on) between ones with.
SEEDS = (2, 3, 8, 10, 12, 29, 31, 38)


# ------------------------------------------------------------------------------------------------ hand-written limit programs
def terms8():
    """one combination of DSD_MAX_TERMS = 8 terms, the model output and 7 buffers: a loop that drops its last term shows"""
    return Program(8, 0, [
        Eval(0, 800.0, [(1, unit((M, 1.0))), (2, unit((0, 0.6), (M, 0.8))), (3, unit((0, 0.8), (M, -0.6)))]),
        Eval(2, 600.0, [(4, unit((M, 0.7), (1, 0.7))), (5, unit((M, -0.5), (3, 0.8))), (6, unit((2, 0.6), (0, -0.5), (M, 0.6)))]),
        Eval(4, 400.0, [(7, unit((M, 0.8), (5, 0.4), (6, -0.4)))]),
        Eval(7, 200.0, [(0, unit((M, 0.5), (1, 0.3), (2, -0.35), (3, 0.4), (4, -0.3), (5, 0.35), (6, 0.3), (7, -0.45)))]),
    ])


def _edge_limit(third):
    # (buffers 1 and 2 are 0.8 M + 0.6 x and 0.6 M - 0.8 x: taken with opposite signs in output 5, so that x - the large part of
    # both - stays in the sum.  With equal signs x cancels, the buffer is a small difference of large ones, and the fp32
    # reference's own rounding error on it, against the same reference in float64, is 8.6e-6 of its peak - more than half
    # the tolerance before the device has rounded anything; test_program_cases_host.py holds every program to that half)
    return [
        Eval(1, 450.0, [(4, unit((M, 0.5), (0, 0.5), (1, -0.5), (2, 0.5))), (5, unit((M, -0.6), (1, 0.4), (2, -0.4), (3, 0.5))),
                        (6, unit(*third))]),
    ]


def edge_full():
    """3 outputs whose state terms total exactly kEdgeMaxTerms = 8 (twice): the most the edge kernel holds, and it must take it"""
    return Program(8, 0, [
        Eval(0, 900.0, [(1, unit((M, 0.8), (0, 0.6))), (2, unit((M, 0.6), (0, -0.8))), (3, unit((M, 1.0)))]),
        *_edge_limit([(0, 0.7), (3, -0.7)]),
        Eval(4, 50.0, [(0, unit((M, 0.5), (0, 0.3), (1, -0.3), (2, 0.35), (3, 0.4), (4, -0.3), (5, 0.35), (6, 0.3))), (7, unit((4, 1.0)))]),
    ])


def edge_over():
    """the same with 9 state terms in every evaluation (buffer 0 listed three times where nothing else is defined yet): one
    more than the edge kernel holds, so every evaluation falls back to the GEMMs"""
    return Program(8, 0, [
        Eval(0, 900.0, [(1, unit((M, 0.8), (0, 0.6), (0, 0.2), (0, -0.3))), (2, unit((M, 0.6), (0, -0.5), (0, -0.2), (0, -0.3))),
                        (3, unit((0, 0.5), (0, 0.25), (0, 0.4)))]),
        *_edge_limit([(0, 0.7), (3, -0.7), (1, 0.4)]),
        Eval(4, 50.0, [(0, unit((M, 0.5), (0, 0.3), (1, -0.3), (2, 0.35), (3, 0.4), (4, -0.3), (5, 0.35), (6, 0.3))),
                       (7, unit((4, 0.8), (5, 0.6)))]),
    ])


def swap():
    """output 0 writes buffer 1 from buffer 2 and output 1 writes buffer 2 from buffer 1 in one evaluation, a third output reads
    both: every output reads the values from before the evaluation"""
    return Program(4, 0, [
        Eval(0, 700.0, [(1, unit((M, 0.8), (0, 0.6))), (2, unit((M, -0.6), (0, 0.8)))]),
        Eval(1, 350.0, [(1, unit((M, 0.3), (2, 0.9))), (2, unit((1, 0.8), (M, -0.5))), (3, unit((1, 0.6), (2, -0.6), (0, 0.5)))]),
        Eval(3, 120.0, [(0, unit((M, 0.5), (1, 0.5), (2, 0.5), (3, -0.5)))]),
    ])


def copy_next():
    """an output without a model term (cm = 0) is the next evaluation's x_buf: the edge kernel fuses the input projection from
    a pure state combination"""
    return Program(4, 0, [
        Eval(0, 650.0, [(1, unit((M, 0.6), (0, 0.8)))]),
        Eval(1, 300.0, [(2, unit((0, 0.6), (1, -0.8))), (3, unit((M, 0.7), (1, 0.7)))]),
        Eval(2, 80.0, [(0, unit((M, 0.6), (2, 0.5), (3, 0.6)))]),
    ])


def model_twice():
    """MODEL listed twice in one combination, with coefficients 0.3 and 0.4: the edge kernel sums them into cm, the GEMM
    epilogue adds them one by one"""
    return Program(3, 0, [
        Eval(0, 500.0, [(1, raw((M, 0.3), (0, 0.8), (M, 0.4)))]),
        Eval(1, 250.0, [(0, raw((M, 0.3), (M, 0.4), (1, 0.6), (0, 0.4))), (2, raw((M, 0.3), (M, 0.4)))]),
    ])


def stay():
    """consecutive evaluations read the same x_buf unchanged (no fused input projection, and the edge kernel's note of what it
    projected must not carry over); the last evaluation overwrites its own x_buf in place"""
    return Program(4, 3, [
        Eval(0, 900.0, [(1, unit((M, 0.6), (0, 0.8)))]),
        Eval(1, 600.0, [(2, unit((M, 0.8), (1, 0.6)))]),
        Eval(1, 300.0, [(3, unit((M, 0.5), (1, 0.6), (2, -0.6)))]),
        Eval(3, 100.0, [(3, unit((M, 0.6), (3, 0.8)))]),
    ])


def noise3():
    """three noise terms in one combination, the same noise tensor in two outputs of one evaluation, indices 0 and 2 used and 1
    not; the last evaluation has no noise term, so where the edge kernel is on it takes that one and the GEMMs the others"""
    return Program(4, 0, [
        Eval(0, 700.0, [(1, unit((M, 0.5), (0, 0.6), (N0, 0.4), (N2, -0.4), (N0, 0.25))), (2, unit((0, 0.8), (N2, 0.6)))]),
        Eval(1, 400.0, [(3, unit((M, 0.6), (1, 0.5), (2, -0.4), (N2, 0.5))), (0, unit((M, -0.5), (1, 0.7), (N0, 0.5)))]),
        Eval(3, 100.0, [(0, unit((M, 0.6), (3, 0.6), (0, 0.5)))]),
    ], n_noise=3)


def bufs64():
    """n_bufs = 64, the most the format allows, using buffers 0, 31 and 63"""
    return Program(64, 0, [
        Eval(0, 550.0, [(31, unit((M, 0.6), (0, 0.8))), (63, unit((M, 0.8), (0, -0.6)))]),
        Eval(63, 150.0, [(0, unit((M, 0.6), (31, 0.5), (63, 0.6))), (31, unit((63, 0.6), (0, 0.6), (M, -0.5)))]),
    ])


def untouched():
    """n_evals > 0 and result_buf = 0, which no evaluation writes: the call returns x_init"""
    return Program(3, 0, [
        Eval(0, 500.0, [(1, unit((M, 0.6), (0, 0.8)))]),
        Eval(1, 200.0, [(2, unit((M, 0.6), (1, 0.6), (0, -0.5)))]),
    ])


HAND_BUILDERS = (terms8, edge_full, edge_over, swap, copy_next, model_twice, stay, noise3, bufs64, untouched)
HAND = {b.__name__: b() for b in HAND_BUILDERS}
GENERATED = {f"gen{seed}": gen(seed) for seed in SEEDS}
PROGRAMS = {**HAND, **GENERATED}


# ------------------------------------------------------------------------------------------------ the paths the programs run on
# (net: a name of kernel_ledger_cases.NETS; dense / ragged: (B, T, lengths); env: the path switches)
# form: the prefix every EP_LINCOMB instantiation the row launches must have (None: an edge row - the edge kernel where
# run_wavenet's rule allows it, any EP_LINCOMB form for the rest); programs: None = every hand-written one; seeds: the generated too
Row = namedtuple("Row", "id net dense ragged env precision form programs seeds")
_R77, _R70 = (3, 77, (64, 65, 1)), (3, 70, (64, 65, 1))         # on a tile end, one frame past it, one frame; T ends in a cut tile
ROWS = [
    Row("edge-c256", "wn256_fm128", (2, 77, None), _R77, dict(DSD_EDGE="1"), "f32", None, None, True),
    Row("edge-c192-fm48", "wn192_fm48", (2, 77, None), _R77, dict(DSD_EDGE="1"), "f32", None, None, False),
    Row("gemm-folded", "wn256_fm128", (1, 70, None), _R70, dict(DSD_EDGE="0"), "f32", "gemm_kernel<5, 1, 3,", None, True),
    Row("gemm-bf16x3", "wn256_L1", (1, 70, None), _R70, dict(DSD_EDGE="0"), "bf16x3", "gemm_kernel<0, 1, 3,", None, False),
    Row("gemm-generic", "wn96_L1", (1, 70, None), _R70, dict(DSD_EDGE="0"), "f32", "gemm_kernel<5, 1, 3, 1, 0,", None, False),     # K = 96
    Row("lynx-gemm", "lx256", (1, 70, None), _R70, dict(DSD_LYNX_RESIDENT="0"), "f32", "gemm_kernel<2, 1, 3,", None, True),
    Row("lynx-resident", "lx256", (1, 70, None), _R70, dict(DSD_LYNX_RESIDENT="1"), "f32", "gemm_kernel<2, 1, 3,", None, True),
    # 64-frame tiles (NB = 2); 961 is odd: the noise rows of stride T are not 16-byte aligned
    Row("gemm-nb2", "wn256_fm512", (4, 1000, None), (4, 1000, (1000, 961, 960, 1)), dict(DSD_EDGE="0"), "f32", "gemm_kernel<5, 1, 3, 2,",
        ("noise3", "terms8"), False),
]
ROW = {r.id: r for r in ROWS}


def oracle_of(net):
    """(model(x, t, cond) on the numpy oracle, (F, M)) of a net of kernel_ledger_cases.NETS with its synthetic weights"""
    import kernel_ledger_cases as lc
    from diffsinger_amd import synth
    from oracle import backbones as ob
    kind, in_dims, n_feats, args, seed = lc.NETS[net]
    params = synth.synth_state_dict(synth.backbone_param_shapes(kind, in_dims, n_feats, hidden_size=256, **args), seed=seed)
    if kind == "wavenet":
        model = lambda x, t, c: ob.wavenet_forward(params, x, t, c, dilation_cycle_length=args["dilation_cycle_length"])  # noqa: E731
    else:
        model = lambda x, t, c: ob.lynxnet_forward(params, x, t, c, activation=args["activation"], strong_cond=args["strong_cond"])  # noqa: E731
    return model, (n_feats, in_dims)


def host_inputs(fm, bsz, t_len):
    """x [B, F, M, T], cond [B, 256, T], noise 3 x [B, F, M, T] of a grid: the same on the host and on the device"""
    from diffsinger_amd import synth
    f, m = fm
    return (synth.synth_normal((bsz, f, m, t_len), 21), synth.synth_normal((bsz, 256, t_len), 22),
            np.stack([synth.synth_normal((bsz, f, m, t_len), 23 + k) for k in range(3)]))


# ------------------------------------------------------------------------------------------------ the limit table as predicates
def _combos(p):
    return [ts for ev in p.evals for _, ts in ev.outs]


def _swap(p):
    for ev in p.evals:
        reads = {d: {s for s, _ in ts} for d, ts in ev.outs}
        for a in reads:
            for b in reads:
                if a != b and b in reads[a] and a in reads[b] and a not in reads[a] and b not in reads[b]:
                    if any({a, b} <= r for d, r in reads.items() if d not in (a, b)):
                        return True
    return False


def _copy_next(p):
    return any(dst == nxt.x_buf and all(s != M for s, _ in ts) for ev, nxt in zip(p.evals, p.evals[1:]) for dst, ts in ev.outs)


def _stay(p):
    same = any(nxt.x_buf == ev.x_buf and all(d != ev.x_buf for d, _ in ev.outs) for ev, nxt in zip(p.evals, p.evals[1:]))
    fused_before = any(ev.x_buf != nxt.x_buf and any(d == nxt.x_buf for d, _ in ev.outs) and nxt2.x_buf == nxt.x_buf and
                       all(d != nxt.x_buf for d, _ in nxt.outs) for ev, nxt, nxt2 in zip(p.evals, p.evals[1:], p.evals[2:]))
    return same and fused_before and any(d == ev.x_buf for ev in p.evals for d, _ in ev.outs)


def _noise3(p):
    used = {NOISE_BASE - s for ts in _combos(p) for s, _ in ts if is_noise(s)}
    three = any(sum(is_noise(s) for s, _ in ts) >= 3 for ts in _combos(p))
    shared = any(len([1 for _, ts in ev.outs if any(s == n for s, _ in ts)]) >= 2
                 for ev in p.evals for n in {s for _, ts in ev.outs for s, _ in ts if is_noise(s)})
    return (p.n_noise == 3 and used == {0, 2} and three and shared and noise_terms(p.evals[-1]) == 0 and edge_takes(p.evals[-1]) and
            all(noise_terms(ev) > 0 for ev in p.evals[:-1]))


FEATURES = {
    "terms8": lambda p: any(len(ts) == 8 and [s for s, _ in ts].count(M) == 1 and len({s for s, _ in ts if s >= 0}) == 7 for ts in _combos(p)),
    "edge_full": lambda p: all(edge_takes(ev) for ev in p.evals) and any(len(ev.outs) == 3 and state_terms(ev) == EDGE_MAX_STATE for ev in p.evals),
    "edge_over": lambda p: (all(noise_terms(ev) == 0 and state_terms(ev) == EDGE_MAX_STATE + 1 for ev in p.evals) and
                            all(len(ev.outs) == 3 for ev in p.evals[:-1])),
    "swap": _swap,
    "copy_next": _copy_next,
    "model_twice": lambda p: any(sorted(c for s, c in ts if s == M) == [_f32(0.3), _f32(0.4)] for ts in _combos(p)),
    "stay": _stay,
    "noise3": _noise3,
    "bufs64": lambda p: p.n_bufs == 64 and {0, 31, 63} <= set(compared(p)) | {ev.x_buf for ev in p.evals},
    "untouched": lambda p: len(p.evals) > 0 and p.result_buf == 0 and 0 not in written(p),
}
