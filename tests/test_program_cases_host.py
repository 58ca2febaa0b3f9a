"""Host checks (no GPU) of tests/program_cases.py: the programs tests/test_gpu_programs.py runs are fit to be compared.

On the WaveNet of test_gpu_cprogram.py (4 layers x 64 channels, 32 bins, hidden 256) at B = 2, T = 33, with the oracle backbone
under tests/prog_sim.py, for every listed program - generated and hand-written:

* every term is live: with any one term's coefficient set to zero, some compared buffer (every buffer the program wrote, and
  buffer 0) moves by at least 1e-3 of that buffer's peak in the reference - about 66 x the sampler tolerance of 1.5e-5 the device
  is held to.  A condition on the INPUTS of the GPU test: a kernel that dropped or misread the term would fail there;
* every compared buffer's rms stays in [0.1, 10]: no term is drowned by a buffer that grew, none is compared against ~0;
* the programs are well formed (what dsd_sample validates, and no read of a buffer the program has not written);
* the reference leaves the device room: on every path of program_cases.ROWS (its net, its dense grid, its programs) the fp32
  reference's own rounding error on every compared buffer - against the same oracle and the same interpreter run in float64 -
  is at most HALF the sampler tolerance.  The device rounds the same arithmetic in another order and is owed as much again;
  where the reference alone takes more than half, a failure on the device would say nothing about the device.  (One evaluation
  of these nets at t = 900 is 4e-6 to 6e-6 from float64 in the fp32 oracle - the sinusoidal embedding's argument t * freq is
  rounded at 900 - so the half is not generous: a buffer that is a small difference of large ones goes over it);
* taken together they have every feature of the limit table (program_cases.FEATURES: predicates over the programs, so that a
  later edit cannot quietly lose one), and each hand-written program has the feature of its name.
"""
import numpy as np
import pytest

import prog_sim
import program_cases as pc
from diffsinger_amd import synth
from oracle import backbones as ob
from prog_sim import run_program

ARGS = dict(num_layers=4, num_channels=64, dilation_cycle_length=2)
B, T, BINS, HIDDEN = 2, 33, 32, 256
LIVE = 1e-3
TOL_SAMPLER = 1.5e-5          # test_gpu_parity.TOL_SAMPLER, which test_gpu_programs.py imports


@pytest.fixture(scope="module")
def rig():
    params = synth.synth_state_dict(synth.backbone_param_shapes("wavenet", BINS, 1, hidden_size=HIDDEN, **ARGS), seed=45)
    cond = synth.synth_normal((B, HIDDEN, T), 11)
    x = synth.synth_normal((B, 1, BINS, T), 12)
    noise = np.stack([synth.synth_normal((B, 1, BINS, T), 100 + i) for i in range(3)])
    model = lambda xx, t, c: ob.wavenet_forward(params, xx, t, c, dilation_cycle_length=2)  # noqa: E731
    return lambda prog: run_program(prog, model, x, cond, noise, all_bufs=True)


def moved(bufs, ref, which):
    """the largest move of a compared buffer, relative to that buffer's peak in the reference"""
    return max(float(np.abs(bufs[b] - ref[b]).max() / np.abs(ref[b]).max()) for b in which)


@pytest.mark.parametrize("name", sorted(pc.PROGRAMS))
def test_every_term_is_live_and_every_buffer_in_range(rig, name):
    prog = pc.PROGRAMS[name]
    assert pc.well_formed(prog)
    which = pc.compared(prog)
    ref = rig(prog)
    for b in which:
        rms = float(np.sqrt(np.mean(np.square(ref[b], dtype=np.float64))))
        assert 0.1 <= rms <= 10.0, (name, "buffer", b, "rms", rms)
    dead = []
    for i, o, k in pc.all_terms(prog):
        m = moved(rig(pc.without_term(prog, i, o, k)), ref, which)
        if m < LIVE:
            dead.append((i, o, k, m))
    assert not dead, (name, "terms (eval, output, term, move) below", LIVE, dead)


def test_the_list_has_every_feature_of_the_limit_table():
    assert len(pc.SEEDS) >= 6 and len(set(pc.SEEDS)) == len(pc.SEEDS)
    assert set(pc.FEATURES) == set(pc.HAND)
    for feature, has in pc.FEATURES.items():
        assert has(pc.HAND[feature]), f"the hand-written program {feature} no longer has the feature of its name"
        assert any(has(p) for p in pc.PROGRAMS.values()), feature
    for name, prog in pc.HAND.items():
        assert 2 <= len(prog.evals) <= 4 and pc.HAND_BUILDERS[list(pc.HAND).index(name)].__doc__, name


def test_generated_programs_follow_the_generator_rules():
    for seed in pc.SEEDS:
        p = pc.gen(seed)
        assert p.key() == pc.gen(seed).key() == pc.PROGRAMS[f"gen{seed}"].key()          # seeded: the same program every time
        assert pc.well_formed(p) and p.n_bufs == 8 and len(p.evals) == 5 and p.n_noise == 3
        assert p.result_buf in pc.compared(p)
        for ev in p.evals:
            for _, ts in ev.outs:
                assert len({s for s, _ in ts}) == len(ts)                                   # distinct sources
                assert abs(sum(c * c for _, c in ts) - 1.0) < 1e-6                          # unit 2-norm
                assert all(0.05 / np.sqrt(8.0) - 1e-7 <= abs(c) <= 1.0 for _, c in ts)
    # what the built-in samplers never reach, reached by the generated programs together
    evs = [ev for seed in pc.SEEDS for ev in pc.gen(seed).evals]
    assert any(len(ts) >= 7 for ev in evs for _, ts in ev.outs)
    assert any(len(ev.outs) == 3 for ev in evs) and any(len(ev.outs) == 1 for ev in evs)
    assert any(pc.noise_terms(ev) >= 2 and len(ev.outs) >= 2 for ev in evs)
    assert any(pc.edge_takes(ev) for ev in evs) and any(not pc.edge_takes(ev) for ev in evs)


def test_without_term_and_with_result_leave_the_program_alone():
    prog = pc.HAND["swap"]
    key = prog.key()
    q = pc.without_term(prog, 1, 0, 1)
    assert q.evals[1].outs[0][1][1] == (2, 0.0) and pc.with_result(prog, 3).result_buf == 3
    assert prog.key() == key and pc.with_result(prog, 3).evals is prog.evals


PATHS = sorted({(r.net, r.dense[:2]) for r in pc.ROWS})


@pytest.mark.parametrize("net,grid", PATHS, ids=[f"{n}-{g[0]}x{g[1]}" for n, g in PATHS])
def test_the_fp32_reference_takes_at_most_half_the_tolerance(net, grid, monkeypatch):
    names = sorted({name for r in pc.ROWS if (r.net, r.dense[:2]) == (net, grid)
                    for name in (r.programs or tuple(pc.HAND)) + (tuple(pc.GENERATED) if r.seeds else ())})
    model, fm = pc.oracle_of(net)
    x, cond, noise = pc.host_inputs(fm, *grid)
    ref = {name: run_program(pc.PROGRAMS[name], model, x, cond, noise, all_bufs=True) for name in names}
    assert all(b.dtype == np.float32 for bufs in ref.values() for b in bufs)
    # the oracle and the interpreter name their float type in one place each: the same code in float64
    monkeypatch.setattr(ob, "F32", np.float64)
    monkeypatch.setattr(prog_sim, "F32", np.float64)
    worst = (0.0, None)
    for name in names:
        prog = pc.PROGRAMS[name]
        exact = run_program(prog, model, x.astype(np.float64), cond.astype(np.float64), noise.astype(np.float64), all_bufs=True)
        assert all(b.dtype == np.float64 for b in exact)
        for b in pc.compared(prog):
            err = float(np.abs(ref[name][b] - exact[b]).max() / np.abs(exact[b]).max())
            worst = max(worst, (err, (name, b)))
            assert err <= TOL_SAMPLER / 2, (net, grid, name, "buffer", b, err)
    print(net, grid, "fp32 reference vs float64, worst", worst)
