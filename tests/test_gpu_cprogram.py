"""-m gpu: the programs the library builds (dsd_program_build) run through dsd_sample.

The WaveNet of test_schedule_programs (4 layers x 64 channels, 32 bins, hidden 256) at B = 2, T = 33: one cut tile, the
smallest grid on which dsd_sample's buffer handling can go wrong.

* Programs that are bit-equal to schedule.py's (DDIM, PLMS, rectified flow, the ONNX euler): dsd_sample on the C struct AS
  BUILT - the pointer dsd_program_build returned, not a copy made in Python - gives bit-identical output to the Python-built
  program on the same handle, eagerly and from a hipGraph.
* Programs whose coefficients pass through the C math library (DPM-Solver++, UniPC, ancestral): against prog_sim.run_program
  of the PYTHON-built program on the oracle backbone, through gpu_util.check at test_gpu_parity's full-sampler tolerance
  (1.5e-5, max and RMS).
* examples/c_abi_sampler.c: compiled with gcc, run, and compared with the same sampler run from Python on the same seeds.
"""
import os
import struct
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from diffsinger_amd import _lib, cprogram, noise, schedule, synth  # noqa: E402
from diffsinger_amd.diffusion import _SamplerMixin  # noqa: E402
from gpu_util import check, dev, make_backbone, set_hp  # noqa: E402
from oracle import backbones as ob  # noqa: E402
from prog_sim import run_program  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = dict(num_layers=4, num_channels=64, dilation_cycle_length=2)
B, T, BINS, HIDDEN = 2, 33, 32, 256
TOL_SAMPLER = 1.5e-5            # test_gpu_parity.TOL_SAMPLER


@pytest.fixture(scope="module")
def rig():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    set_hp()
    net, params = make_backbone("wavenet", BINS, 1, ARGS, 45)
    runner = type("R", (_SamplerMixin,), {})()
    runner.denoise_fn = net
    cond = synth.synth_normal((B, HIDDEN, T), 11)
    x = synth.synth_normal((B, 1, BINS, T), 12)
    oracle = lambda xx, t, c: ob.wavenet_forward(params, xx, t, c, dilation_cycle_length=2)  # noqa: E731
    yield SimpleNamespace(net=net, runner=runner, cond=cond, x=x, oracle=oracle,
                          tb=schedule.DDPMTables(schedule.linear_beta_schedule(1000)))
    net.release_native()


def run_python_built(rig, prog, use_graph, x=None, step_noise=None):
    rig.runner.use_graph = use_graph
    entry = (prog,) + _lib.program_to_c(prog)
    return rig.runner._run_program(entry, dev(rig.cond), dev(rig.x if x is None else x), noise=step_noise, transpose=False).clone()


def run_c_built(rig, sampler_spec, use_graph, x=None, step_noise=None):
    """dsd_sample on the struct dsd_program_build allocated: `p.contents` is that memory, not a copy."""
    rig.runner.use_graph = use_graph
    with cprogram.built(sampler_spec[0]) as p:
        entry = (SimpleNamespace(n_noise=p.contents.n_noise), p.contents, None)
        out = rig.runner._run_program(entry, dev(rig.cond), dev(rig.x if x is None else x), noise=step_noise, transpose=False).clone()
        torch.cuda.synchronize()            # the program is freed on leaving the block
    return out


BIT_EQUAL = {
    "ddim_1000_10": (lambda tb: cprogram.spec("ddim", tb, 1000, 100), lambda tb: schedule.ddim_program(tb, 1000, 100)),
    "plms_1000_20": (lambda tb: cprogram.spec("pndm", tb, 1000, 50), lambda tb: schedule.plms_program(tb, 1000, 50)),
    "rf_rk4_3": (lambda tb: cprogram.spec("rf_rk4", steps=3, t_start=0.0, time_scale_factor=1000),
                 lambda tb: schedule.reflow_program("rk4", 3, 0.0, 1000)),
    "rf_euler_onnx": (lambda tb: cprogram.spec("rf_euler_onnx", steps=5, t_start=0.4, time_scale_factor=1000),
                      lambda tb: schedule.reflow_onnx_program(5, 0.4, 1000)),
}


@pytest.mark.parametrize("tag", sorted(BIT_EQUAL))
def test_bit_equal_programs_give_bit_identical_samples(rig, tag):
    c_spec, py_prog = BIT_EQUAL[tag][0](rig.tb), BIT_EQUAL[tag][1](rig.tb)
    assert cprogram.build(c_spec).key() == py_prog.key()
    # the C struct first in either mode: its graph is captured from the C struct, not found in the cache
    c_eager, py_eager = run_c_built(rig, c_spec, False), run_python_built(rig, py_prog, False)
    c_graph, py_graph = run_c_built(rig, c_spec, True), run_python_built(rig, py_prog, True)
    assert torch.isfinite(c_eager).all() and float(c_eager.abs().max()) > 0
    assert torch.equal(c_eager, py_eager), tag
    assert torch.equal(c_graph, py_graph), tag
    assert torch.equal(c_graph, c_eager), tag


MATH = {
    "dpm_1000_20": (lambda tb: cprogram.spec("dpm-solver", tb, 1000, 50),
                    lambda tb: schedule.dpm_solver_pp_program(torch.from_numpy(tb.betas), 20)),
    "dpm_400_20": (lambda tb: cprogram.spec("dpm-solver", tb, 400, 20),
                   lambda tb: schedule.dpm_solver_pp_program(torch.from_numpy(tb.betas[:400]), 20)),
    "unipc_1000_20": (lambda tb: cprogram.spec("unipc", tb, 1000, 50),
                      lambda tb: schedule.unipc_program(torch.from_numpy(tb.betas), 20)),
}


@pytest.mark.parametrize("tag", sorted(MATH))
def test_math_dependent_programs_vs_python_built_on_the_oracle(rig, tag):
    c_spec, py_prog = MATH[tag][0](rig.tb), MATH[tag][1](rig.tb)
    want = run_program(py_prog, rig.oracle, rig.x, rig.cond)
    check(run_c_built(rig, c_spec, False), want, TOL_SAMPLER, what=(tag, "eager"))
    check(run_c_built(rig, c_spec, True), want, TOL_SAMPLER, what=(tag, "graph"))


def test_ancestral_chunks_vs_python_built_on_the_oracle(rig):
    """t_max = 20 in chunks (20, 8) and (8, 0), each taking its own noise tensors from index 0, as diffusion.py runs them."""
    step = np.stack([synth.synth_normal((B, 1, BINS, T), 100 + i) for i in range(20)])
    x = run_program(schedule.ddpm_ancestral_program(rig.tb, 20, 8), rig.oracle, rig.x, rig.cond, step[:12])
    want = run_program(schedule.ddpm_ancestral_program(rig.tb, 8, 0), rig.oracle, x, rig.cond, step[12:])
    for use_graph in (False, True):
        mid = run_c_built(rig, cprogram.spec("ddpm", rig.tb, 20, 1, 8), use_graph, step_noise=dev(step[:12]))
        got = run_c_built(rig, cprogram.spec("ddpm", rig.tb, 8, 1, 0), use_graph, x=mid.cpu().numpy(), step_noise=dev(step[12:]))
        check(got, want, TOL_SAMPLER, what=("ancestral 20 -> 8 -> 0", use_graph))
    # one program for the second chunk that numbers its noise on from the first: the same tensors at indices 12..19
    whole = run_c_built(rig, cprogram.spec("ddpm", rig.tb, 8, 1, 0, noise_index0=12), False, x=mid.cpu().numpy(), step_noise=dev(step))
    assert torch.equal(whole, got)


def test_empty_program_returns_the_start(rig):
    out = run_c_built(rig, cprogram.spec("ddim", rig.tb, 0, 10), False)
    assert torch.equal(out, dev(rig.x))


def test_c_example_runs_the_sampler_the_library_built(tmp_path, rig):
    exe = tmp_path / "c_abi_sampler"
    libdir = os.path.join(ROOT, "diffsinger_amd")
    cmd = ["gcc", "-std=c99", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "examples", "c_abi_sampler.c"), "-L" + libdir, "-ldsdenoise", "-L/opt/rocm/lib", "-lamdhip64",
           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)]
    subprocess.run(cmd, check=True)
    params = synth.synth_state_dict(synth.backbone_param_shapes("wavenet", BINS, 1, hidden_size=HIDDEN, **ARGS), seed=45)
    seeds = [0x123456789abcdef0, 42]
    with open(tmp_path / "weights.bin", "wb") as f:
        f.write(struct.pack("<i", len(params)))
        for name, arr in params.items():
            nb = name.encode()
            f.write(struct.pack("<i", len(nb)) + nb + struct.pack("<i", arr.ndim) + struct.pack(f"<{arr.ndim}q", *arr.shape))
            f.write(np.ascontiguousarray(arr, np.float32).tobytes())
    with open(tmp_path / "inputs.bin", "wb") as f:
        f.write(struct.pack("<4i", B, T, HIDDEN, BINS) + struct.pack(f"<{B}Q", *seeds) + rig.cond.tobytes())
    env = dict(os.environ, HIP_FORCE_DEV_KERNARG="1")
    res = subprocess.run([str(exe), str(tmp_path / "weights.bin"), str(tmp_path / "inputs.bin"), str(tmp_path / "out.bin")],
                         capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.splitlines()
    assert lines[0] == "program 20 evaluations, 3 buffers"
    assert lines[1].startswith("sample checksum ") and np.isfinite(float(lines[1].split()[2]))
    got = np.fromfile(tmp_path / "out.bin", dtype=np.float32).reshape(2, B, 1, BINS, T)
    x_t = noise.fill((1, B, BINS, T), seeds, noise.X_T).view(B, 1, BINS, T)
    assert np.array_equal(got[0], x_t.cpu().numpy())
    # The same sampler from Python on the same seeds, within the full-sampler tolerance: with the program the library built
    # and with the one schedule.py builds.  (Not bitwise: the shim hands the library torch's SinusoidalPosEmb frequency table,
    # the C caller leaves it to the library's own expf - the bound of test_gpu_c_abi exists for the same reason.)
    x0 = x_t.cpu().numpy()
    check(got[1], run_c_built(rig, cprogram.spec("dpm-solver", rig.tb, 1000, 50), True, x=x0).cpu().numpy(), TOL_SAMPLER,
          what="c_abi_sampler.c vs the C-built DPM-Solver++ 1000 -> 20 from Python")
    py = run_python_built(rig, schedule.dpm_solver_pp_program(torch.from_numpy(rig.tb.betas), 20), True, x=x0)
    check(got[1], py.cpu().numpy(), TOL_SAMPLER, what="c_abi_sampler.c vs the Python-built DPM-Solver++ 1000 -> 20")
