"""Host checks (no GPU) of the library's program builder - dsd_ddpm_tables_fill, dsd_program_build / dsd_program_free,
dsd_onnx_ddpm_plan - against diffsinger_amd/schedule.py, the yardstick.

Bit equality (fp32 coefficients and fp32 times alike) wherever only IEEE + - * / sqrt stand between the inputs and the
program: the twelve tables, DDIM, PLMS, the four rectified-flow integrators, the ONNX euler, dsd_onnx_ddpm_plan, and -
for every sampler - the evaluation times and the structure (buffer ids, counts, term order).

The coefficients of the ancestral sampler (sigma = exp(0.5 * log variance)), DPM-Solver++ and UniPC pass through fp32
exp / log / expm1, which the library takes from the C math library and schedule.py from torch (SLEEF) and numpy: equality
to the last bit is not promised there.  The test prints, per case, how many coefficients differ and the largest relative
difference (run with -s; DESIGN.md section 5 has the table), and ASSERTS on the sample: the C-built program run through
tests/prog_sim with the oracle WaveNet meets the reference's goldens (g5_samplers) at the bars test_schedule_programs
applies to the Python-built programs, and lies within the full-sampler fp32 tolerance (1.5e-5, max and RMS) of the
Python-built program's sample.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from diffsinger_amd import _lib, cprogram, schedule, synth
from oracle import backbones as ob
from prog_sim import finish, run_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SN_ARGS = dict(num_layers=4, num_channels=64, dilation_cycle_length=2)
TOL_SAMPLER = 1.5e-5


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def structure(prog):
    return (prog.n_bufs, prog.result_buf, prog.n_noise,
            tuple((e.x_buf, tuple((d, tuple(s for s, _ in ts)) for d, ts in e.outs)) for e in prog.evals))


def times(prog):
    return bits([e.t for e in prog.evals]).tolist()


def coefficients(prog):
    return np.array([c for e in prog.evals for _, ts in e.outs for _, c in ts], dtype=np.float32)


@pytest.fixture(scope="module")
def tb():
    return schedule.DDPMTables(schedule.linear_beta_schedule(1000))


# ---- the boundary --------------------------------------------------------------------------------------------------------
def test_symbols_and_struct():
    names = ["dsd_ddpm_tables_fill", "dsd_program_build", "dsd_program_free", "dsd_onnx_ddpm_plan"]
    lib = C.CDLL(_lib.LIB_PATH)
    for n in names:
        assert n in _lib.EXPORTS and hasattr(lib, n), n
    s = _lib.DsdSamplerSpec
    assert C.sizeof(s) == 56
    assert [(n, getattr(s, n).offset) for n, _ in s._fields_] == [
        ("struct_size", 0), ("sampler", 4), ("timesteps", 8), ("t_max", 12), ("speedup", 16), ("t_lo", 20), ("noise_index0", 24),
        ("steps", 28), ("tables", 32), ("t_start", 40), ("time_scale_factor", 48)]
    header = open(os.path.join(ROOT, "include", "dsdenoise.h")).read()
    body = re.search(r"typedef struct dsd_sampler_spec \{(.*?)\} dsd_sampler_spec;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert [re.findall(r"(\w+)\s*$", d.strip())[0] for d in body.split(";") if d.strip()] == [n for n, _ in s._fields_]
    ids = dict(re.findall(r"DSD_SAMPLER_(\w+) = (\d+)", header))
    assert {k: int(v) for k, v in ids.items()} == {"DDPM": 0, "DDIM": 1, "PLMS": 2, "DPM_SOLVER_PP": 3, "UNIPC": 4, "RF_EULER": 5,
                                                   "RF_RK2": 6, "RF_RK4": 7, "RF_RK5": 8, "RF_EULER_ONNX": 9}
    assert sorted(_lib.SAMPLER_IDS.values()) == list(range(10))
    assert "#define DSD_SCHEDULE_LINEAR 0" in header and "#define DSD_SCHEDULE_COSINE 1" in header
    assert f"#define DSD_DDPM_TABLES {len(schedule.DDPMTables.NAMES)}" in header


# ---- tables --------------------------------------------------------------------------------------------------------------
TABLE_CASES = [("linear", t, mb) for t in (1000, 100, 4) for mb in (0.01, 0.02, 0.06)] + [("cosine", 1000, 0.01)]


@pytest.mark.parametrize("kind,timesteps,max_beta", TABLE_CASES, ids=[f"{k}-{t}-{m}" for k, t, m in TABLE_CASES])
def test_tables_bit_equal(kind, timesteps, max_beta):
    betas = schedule.linear_beta_schedule(timesteps, max_beta) if kind == "linear" else schedule.cosine_beta_schedule(timesteps)
    want, got = schedule.DDPMTables(betas), cprogram.tables(kind, timesteps, max_beta)
    for name in schedule.DDPMTables.NAMES:
        differing = np.flatnonzero(bits(getattr(want, name)) != bits(getattr(got, name)))
        assert differing.size == 0, (name, differing[:8])


def test_tables_equal_the_reference_golden():
    g = np.load(os.path.join(GOLDEN, "g4_schedules.npz"))
    got = cprogram.tables("linear", 1000, 0.01)
    for k in ("betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod",
              "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_variance",
              "posterior_log_variance_clipped", "posterior_mean_coef1", "posterior_mean_coef2"):
        assert np.array_equal(bits(getattr(got, k)), bits(g[k])), k
    assert np.array_equal(bits(cprogram.tables("cosine", 1000).betas), bits(g["cosine_betas"]))


def test_tables_one_step_and_errors():
    one = cprogram.tables("linear", 1, 0.02)            # numpy's linspace of one point is its start
    assert np.array_equal(bits(one.betas), bits(schedule.DDPMTables(schedule.linear_beta_schedule(1, 0.02)).betas))
    lib = _lib.lib()
    out = (C.c_float * 48)()
    for args, message in (((0, 4, 0.01, None), b"null"), ((2, 4, 0.01, out), b"unknown schedule_type"),
                          ((-1, 4, 0.01, out), b"unknown schedule_type"), ((0, 0, 0.01, out), b"positive")):
        assert lib.dsd_ddpm_tables_fill(*args) == -1
        err = lib.dsd_last_error(None)
        assert b"dsd_ddpm_tables_fill" in err and message in err, err
    assert not any(out)


# ---- programs that are bit-equal -----------------------------------------------------------------------------------------
# (t_max, speedup); the issue's pairs read either as that or as (t_max, steps): both readings are here
GRID = [(1000, 10), (1000, 100), (200, 10), (200, 20), (400, 20), (20, 20), (20, 1), (1000, 7), (1000, 1000), (999, 10)]


@pytest.mark.parametrize("t_max,speedup", GRID)
def test_ddim_and_plms_bit_equal(tb, t_max, speedup):
    assert cprogram.build(cprogram.spec("ddim", tb, t_max, speedup)).key() == schedule.ddim_program(tb, t_max, speedup).key()
    assert cprogram.build(cprogram.spec("pndm", tb, t_max, speedup)).key() == schedule.plms_program(tb, t_max, speedup).key()


def test_tables_from_a_checkpoint_are_read_as_they_stand():
    """`tables` need not come from the fill call (DDPMTables.from_arrays): another schedule, cut to 300 steps."""
    other = schedule.DDPMTables(schedule.cosine_beta_schedule(300))
    assert cprogram.build(cprogram.spec("ddim", other, 300, 10)).key() == schedule.ddim_program(other, 300, 10).key()
    assert cprogram.build(cprogram.spec("pndm", other, 120, 5)).key() == schedule.plms_program(other, 120, 5).key()


@pytest.mark.parametrize("t_start", [0.0, 0.4])
@pytest.mark.parametrize("steps", [1, 3, 20])
@pytest.mark.parametrize("algorithm", cprogram.RF_ALGORITHMS)
def test_reflow_bit_equal(algorithm, steps, t_start):
    got = cprogram.build(cprogram.spec("rf_" + algorithm, steps=steps, t_start=t_start, time_scale_factor=1000))
    assert got.key() == schedule.reflow_program(algorithm, steps, t_start, 1000).key()


@pytest.mark.parametrize("t_start", [0.0, 0.4, 0.123456789])
@pytest.mark.parametrize("steps", [1, 3, 7, 20])
def test_reflow_onnx_bit_equal(steps, t_start):
    got = cprogram.build(cprogram.spec("rf_euler_onnx", steps=steps, t_start=t_start, time_scale_factor=1000))
    assert got.key() == schedule.reflow_onnx_program(steps, t_start, 1000).key()
    # the twin's t_start is an fp32 value: 0.4 gives other times than reflow.py's Python-float arithmetic
    if steps == 20 and t_start == 0.4:
        assert times(got) != times(schedule.reflow_program("euler", steps, t_start, 1000))


def test_empty_programs(tb):
    for name in ("ddpm", "ddim", "pndm", "dpm-solver", "unipc"):
        assert cprogram.build(cprogram.spec(name, tb, 0, 10)).key() == schedule.Program(1, 0, []).key()
    assert cprogram.build(cprogram.spec("rf_rk4", steps=0)).key() == schedule.reflow_program("rk4", 0, 0.0, 1000).key()
    _lib.lib().dsd_program_free(None)               # like free()


# ---- the ONNX twins' plan -------------------------------------------------------------------------------------------------
def test_onnx_ddpm_plan_sweep():
    """steps 1..1000 without a depth, and steps 1..1000 x depth 0, 0.01 .. 1 with one: the whole product at k_step 1000,
    and at k_step 400 (the cap) for the steps up to 60 and every 37th after.  The library is called directly: the wrapper's
    array conversion would double the time of 10^5 calls."""
    timesteps = 1000
    factors = [i for i in range(1, timesteps + 1) if timesteps % i == 0]
    ft = torch.LongTensor(factors)
    lib, fc = _lib.lib(), (C.c_int64 * len(factors))(*factors)
    t, s = C.c_int32(), C.c_int32()

    def plan(k_step, steps, depth):
        assert lib.dsd_onnx_ddpm_plan(timesteps, k_step, fc, len(factors), steps, -1.0 if depth is None else depth,
                                      C.byref(t), C.byref(s)) == 0
        return t.value, s.value

    assert cprogram.onnx_ddpm_plan(timesteps, 400, factors, 7) == schedule.onnx_ddpm_plan(timesteps, 400, ft, 7) == plan(400, 7, None)
    assert cprogram.onnx_ddpm_plan(timesteps, 400, ft, 7, 0.37) == schedule.onnx_ddpm_plan(timesteps, 400, ft, 7, 0.37)
    depths = [0.01 * i for i in range(101)]
    ties = [0.0005, 0.0015, 0.0025, 0.3995, 0.4005]         # depth * 1000 lands on a half
    for steps in range(1, 1001):
        for k_step in (1000, 400):
            assert plan(k_step, steps, None) == schedule.onnx_ddpm_plan(timesteps, k_step, ft, steps)
        for depth in depths + ties:
            assert plan(1000, steps, depth) == schedule.onnx_ddpm_plan(timesteps, 1000, ft, steps, depth), (steps, depth)
        if steps <= 60 or steps % 37 == 0:
            for depth in depths + ties:
                assert plan(400, steps, depth) == schedule.onnx_ddpm_plan(timesteps, 400, ft, steps, depth), (steps, depth)


def test_onnx_ddpm_plan_errors():
    lib = _lib.lib()
    f = (C.c_int64 * 3)(1, 2, 4)
    t, s = C.c_int32(-7), C.c_int32(-7)
    cases = [((4, 4, f, 3, 2, -1.0, None, C.byref(s)), b"null"), ((0, 4, f, 3, 2, -1.0, C.byref(t), C.byref(s)), b"positive"),
             ((4, 4, f, 3, 0, 0.5, C.byref(t), C.byref(s)), b"positive"), ((4, 4, None, 0, 2, -1.0, C.byref(t), C.byref(s)), b"no factors"),
             ((4, 4, (C.c_int64 * 1)(3), 1, 2, -1.0, C.byref(t), C.byref(s)), b"no factor is <="),
             ((4, 4, f, 3, 2, float("nan"), C.byref(t), C.byref(s)), b"NaN")]
    for args, message in cases:
        assert lib.dsd_onnx_ddpm_plan(*args) == -1
        err = lib.dsd_last_error(None)
        assert b"dsd_onnx_ddpm_plan" in err and message in err, err
        assert (t.value, s.value) == (-7, -7)


# ---- programs that pass through exp / log / expm1 ----------------------------------------------------------------------
MATH = {
    "dpm20": (lambda tb: schedule.dpm_solver_pp_program(torch.from_numpy(tb.betas), 20), lambda tb: cprogram.spec("dpm-solver", tb, 1000, 50)),
    "dpm50": (lambda tb: schedule.dpm_solver_pp_program(torch.from_numpy(tb.betas), 50), lambda tb: cprogram.spec("dpm-solver", tb, 1000, 20)),
    "dpm5": (lambda tb: schedule.dpm_solver_pp_program(torch.from_numpy(tb.betas), 5), lambda tb: cprogram.spec("dpm-solver", tb, 1000, 200)),
    "dpm100": (lambda tb: schedule.dpm_solver_pp_program(torch.from_numpy(tb.betas), 100), lambda tb: cprogram.spec("dpm-solver", tb, 1000, 10)),
    "dpm_shallow": (lambda tb: schedule.dpm_solver_pp_program(torch.from_numpy(tb.betas[:400]), 20),
                    lambda tb: cprogram.spec("dpm-solver", tb, 400, 20)),
    "dpm_200_10": (lambda tb: schedule.dpm_solver_pp_program(torch.from_numpy(tb.betas[:200]), 20),
                   lambda tb: cprogram.spec("dpm-solver", tb, 200, 10)),
    "dpm_20_10": (lambda tb: schedule.dpm_solver_pp_program(torch.from_numpy(tb.betas[:20]), 2), lambda tb: cprogram.spec("dpm-solver", tb, 20, 10)),
    "dpm_200_20": (lambda tb: schedule.dpm_solver_pp_program(torch.from_numpy(tb.betas[:200]), 10),
                   lambda tb: cprogram.spec("dpm-solver", tb, 200, 20)),
    "dpm_20_1": (lambda tb: schedule.dpm_solver_pp_program(torch.from_numpy(tb.betas[:20]), 20), lambda tb: cprogram.spec("dpm-solver", tb, 20, 1)),
    "unipc_200_10": (lambda tb: schedule.unipc_program(torch.from_numpy(tb.betas[:200]), 20), lambda tb: cprogram.spec("unipc", tb, 200, 10)),
    "unipc_20_1": (lambda tb: schedule.unipc_program(torch.from_numpy(tb.betas[:20]), 20), lambda tb: cprogram.spec("unipc", tb, 20, 1)),
    "unipc20": (lambda tb: schedule.unipc_program(torch.from_numpy(tb.betas), 20), lambda tb: cprogram.spec("unipc", tb, 1000, 50)),
    "unipc50": (lambda tb: schedule.unipc_program(torch.from_numpy(tb.betas), 50), lambda tb: cprogram.spec("unipc", tb, 1000, 20)),
    "unipc100": (lambda tb: schedule.unipc_program(torch.from_numpy(tb.betas), 100), lambda tb: cprogram.spec("unipc", tb, 1000, 10)),
    "unipc_shallow": (lambda tb: schedule.unipc_program(torch.from_numpy(tb.betas[:400]), 20), lambda tb: cprogram.spec("unipc", tb, 400, 20)),
    "unipc_20_10": (lambda tb: schedule.unipc_program(torch.from_numpy(tb.betas[:20]), 2), lambda tb: cprogram.spec("unipc", tb, 20, 10)),
    "ddpm_20_8": (lambda tb: schedule.ddpm_ancestral_program(tb, 20, 8), lambda tb: cprogram.spec("ddpm", tb, 20, 1, 8)),
    "ddpm_8_0_from_12": (lambda tb: schedule.ddpm_ancestral_program(tb, 8, 0, 12), lambda tb: cprogram.spec("ddpm", tb, 8, 1, 0, 12)),
    "ddpm_1000_950": (lambda tb: schedule.ddpm_ancestral_program(tb, 1000, 950), lambda tb: cprogram.spec("ddpm", tb, 1000, 1, 950)),
}


@pytest.mark.parametrize("tag", sorted(MATH))
def test_math_dependent_programs_structure_and_times(tb, tag):
    want, got = MATH[tag][0](tb), cprogram.build(MATH[tag][1](tb))
    assert structure(got) == structure(want)
    assert times(got) == times(want)
    a, b = coefficients(want).astype(np.float64), coefficients(got).astype(np.float64)
    differing = int((bits(a) != bits(b)).sum())
    rel = float((np.abs(a - b) / np.maximum(np.abs(a), 1e-30)).max())
    print(f"{tag}: {differing} of {a.size} coefficients differ, largest relative difference {rel:.3g}")
    assert np.isfinite(b).all()         # the figures above are recorded, not barred: the samples are (below)


@pytest.fixture(scope="module")
def net():
    shapes = synth.backbone_param_shapes("wavenet", 32, 1, hidden_size=256, **SN_ARGS)
    params = synth.synth_state_dict(shapes, seed=45)
    return lambda x, t, c: ob.wavenet_forward(params, x, t, c, dilation_cycle_length=2)


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def near_python_built(tag, got, want):
    d = np.asarray(got, np.float64) - np.asarray(want, np.float64)
    mx = float(np.abs(d).max() / np.abs(want).max())
    rms = float(np.sqrt(np.mean(d * d)) / np.sqrt(np.mean(np.asarray(want, np.float64) ** 2)))
    print(f"{tag}: C-built vs Python-built sample: max {mx:.3g}, rms {rms:.3g} (bar {TOL_SAMPLER})")
    assert mx <= TOL_SAMPLER and rms <= TOL_SAMPLER, (tag, mx, rms)


def _inputs(g, tag, shallow_tb=None, t_max=None):
    from test_schedule_programs import _inputs as inputs
    return inputs(g, tag, shallow_tb, t_max)


@pytest.mark.parametrize("tag", ["dpm20", "dpm50", "dpm5", "unipc20", "unipc50"])
def test_math_dependent_samples_vs_golden(tb, net, tag):
    g = np.load(os.path.join(GOLDEN, "g5_samplers.npz"))
    _, _, _, _, cond, x = _inputs(g, tag)
    got = finish(run_program(cprogram.build(MATH[tag][1](tb)), net, x, cond))
    assert rel_err(got, g[f"{tag}_out"]) < 2e-4, tag
    near_python_built(tag, got, finish(run_program(MATH[tag][0](tb), net, x, cond)))


def test_shallow_samples_vs_golden(tb, net):
    g = np.load(os.path.join(GOLDEN, "g5_samplers.npz"))
    # ancestral DDPM from K_step_infer = 20 in chunks (20, 8) and (8, 0), each with its own noise tensors from 0
    bsz, t_len, nseed, n_randn, cond, x0 = _inputs(g, "ddpm_shallow20", tb, 20)
    noise = np.stack([synth.synth_normal((bsz, 1, 32, t_len), nseed + 1 + i) for i in range(n_randn - 1)])
    samples = []
    for build in (lambda hi, lo: cprogram.build(cprogram.spec("ddpm", tb, hi, 1, lo)),
                  lambda hi, lo: schedule.ddpm_ancestral_program(tb, hi, lo)):
        p1, p2 = build(20, 8), build(8, 0)
        assert p1.n_noise == 12 and p2.n_noise == 8
        samples.append(finish(run_program(p2, net, run_program(p1, net, x0, cond, noise[:12]), cond, noise[12:])))
    assert rel_err(samples[0], g["ddpm_shallow20_out"]) < 1e-4
    near_python_built("ddpm_shallow20", *samples)
    _, _, _, _, cond, x = _inputs(g, "dpm_shallow", tb, 400)
    got = finish(run_program(cprogram.build(MATH["dpm_shallow"][1](tb)), net, x, cond))
    assert rel_err(got, g["dpm_shallow_out"]) < 2e-4
    near_python_built("dpm_shallow", got, finish(run_program(MATH["dpm_shallow"][0](tb), net, x, cond)))


def test_reflow_sample_vs_golden(net):
    """Bit-equal programs give the same sample; one run shows the C-built one against the reference's golden all the same."""
    g = np.load(os.path.join(GOLDEN, "g5_samplers.npz"))
    _, _, _, _, cond, x = _inputs(g, "rf_rk4_20")
    got = finish(run_program(cprogram.build(cprogram.spec("rf_rk4", steps=20)), net, x, cond))
    assert rel_err(got, g["rf_rk4_20_out"]) < 5e-5


# ---- errors --------------------------------------------------------------------------------------------------------------
def _refused(sampler_spec, message):
    lib = _lib.lib()
    sentinel = C.cast(0x5a5a5a50, C.POINTER(_lib.DsdProgram))
    out = C.POINTER(_lib.DsdProgram)()
    C.memmove(C.byref(out), C.byref(sentinel), C.sizeof(out))
    assert lib.dsd_program_build(C.byref(sampler_spec) if sampler_spec is not None else None, C.byref(out)) == -1
    err = lib.dsd_last_error(None)
    assert b"dsd_program_build" in err and message in err, err
    assert C.cast(out, C.c_void_p).value == 0x5a5a5a50          # *out untouched


BUILD_EINVAL = [
    ("short_struct", "ddim", dict(t_max=1000, speedup=10), dict(struct_size=48), b"struct_size"),
    ("zero_struct", "ddim", dict(t_max=1000, speedup=10), dict(struct_size=0), b"struct_size"),
    ("unknown_sampler", "ddim", dict(t_max=1000, speedup=10), dict(sampler=10), b"unknown sampler"),
    ("negative_sampler", "ddim", dict(t_max=1000, speedup=10), dict(sampler=-1), b"unknown sampler"),
    ("dpm_one_step", "dpm-solver", dict(t_max=1000, speedup=1000), {}, b">= 2"),
    ("dpm_no_step", "dpm-solver", dict(t_max=10, speedup=20), {}, b">= 2"),
    ("unipc_one_step", "unipc", dict(t_max=1000, speedup=501), {}, b">= 2"),
    ("t_max_past_timesteps", "ddim", dict(t_max=1001, speedup=10), {}, b"t_max 1001"),
    ("t_max_negative", "ddpm", dict(t_max=-1, speedup=1), {}, b"t_max -1"),
    ("speedup_zero", "ddim", dict(t_max=1000, speedup=0), {}, b"speedup 0"),
    ("speedup_negative", "pndm", dict(t_max=1000, speedup=-3), {}, b"speedup -3"),
    ("null_tables", "ddim", dict(t_max=1000, speedup=10), dict(tables=C.POINTER(C.c_float)()), b"null tables"),
    ("no_timesteps", "ddim", dict(t_max=0, speedup=10), dict(timesteps=0), b"timesteps 0"),
    ("t_lo_past_t_max", "ddpm", dict(t_max=20, speedup=1, t_lo=21), {}, b"t_lo 21"),
    ("noise_index_negative", "ddpm", dict(t_max=20, speedup=1, noise_index0=-1), {}, b"noise_index0"),
    ("reflow_negative_steps", "rf_euler", dict(steps=-1), {}, b"steps -1"),
    ("reflow_nan", "rf_rk4", dict(steps=3, t_start=float("nan")), {}, b"NaN"),
]


@pytest.mark.parametrize("name,sampler,kw,over,message", BUILD_EINVAL, ids=[e[0] for e in BUILD_EINVAL])
def test_build_einval_leaves_out_untouched(tb, name, sampler, kw, over, message):
    s, _keep = cprogram.spec(sampler, None if sampler.startswith("rf_") else tb, **kw)
    for k, v in over.items():
        setattr(s, k, v)
    _refused(s, message)


def test_build_null_arguments():
    lib = _lib.lib()
    _refused(None, b"null argument")
    s, _keep = cprogram.spec("rf_euler", steps=3)
    assert lib.dsd_program_build(C.byref(s), None) == -1
    assert b"dsd_program_build: null argument" in lib.dsd_last_error(None)


def test_every_built_program_is_within_the_limits(tb):
    """DSD_MAX_TERMS / DSD_MAX_OUT: the builder refuses a program that would exceed them; none of the samplers it knows
    does (rk5's last stage is the widest with 6 terms, UniPC's evaluations the only ones with 3 outputs), so that refusal
    has no case that reaches it through the public struct - what is checked here is that the limits hold."""
    widest_terms = widest_outs = 0
    specs = [cprogram.spec(n, tb, 1000, 50) for n in ("ddim", "pndm", "dpm-solver", "unipc")] + \
            [cprogram.spec("ddpm", tb, 30, 1, 0, 5), cprogram.spec("dpm-solver", tb, 1000, 200)] + \
            [cprogram.spec("rf_" + a, steps=3, t_start=0.4) for a in cprogram.RF_ALGORITHMS] + [cprogram.spec("rf_euler_onnx", steps=3)]
    for s in specs:
        prog = cprogram.build(s)
        for ev in prog.evals:
            assert 1 <= len(ev.outs) <= _lib.DSD_MAX_OUT and 0 <= ev.x_buf < prog.n_bufs
            widest_outs = max(widest_outs, len(ev.outs))
            for dst, terms in ev.outs:
                assert 0 <= dst < prog.n_bufs and 1 <= len(terms) <= _lib.DSD_MAX_TERMS
                widest_terms = max(widest_terms, len(terms))
                assert all(c != 0.0 for _, c in terms)
    assert (widest_terms, widest_outs) == (6, 3)
