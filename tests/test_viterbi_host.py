"""CPU: the inputs of the Viterbi decode tests (tests/viterbi_ref.py), not the product.  tests/test_gpu_viterbi.py asks the
kernel for a path EQUAL to the oracle's; this file shows that its inputs admit no excuse: the float32 and the float64
formation of log_prob choose the same path, and that path is chosen with a margin (>= 1e-4) far above what a double
recursion can lose (value reaches 5.8e3 on 1001 frames, where a double ulp is 9e-13).  It also checks the oracle itself:
two crafted inputs with known paths, and the path's score against its neighbours'."""
import numpy as np
import pytest

import viterbi_ref as vr

MARGIN = 1e-4


@pytest.fixture(scope="module")
def hidden():
    return vr.cases()


@pytest.mark.parametrize("name,T,seed,kind", vr.MELODIES)
def test_melody_admits_one_path(hidden, name, T, seed, kind):
    h = hidden[name]
    assert h.shape == (T, vr.N_CLASS) and h.dtype == np.float32
    ref, f64 = vr.viterbi_path(h, "ref"), vr.viterbi_path(h, "f64")
    margin = min(vr.on_path_margin(h, "ref"), vr.on_path_margin(h, "f64"))
    differs = int((ref != h.argmax(axis=1)).sum())
    print(f"{name}: margin {margin:.3g}, path != argmax on {differs} frames")
    assert np.array_equal(ref, f64)
    assert margin >= MARGIN, margin
    if T == 1:
        assert ref[0] == h[0].argmax()
    else:
        assert differs >= 1
    if kind == 2:
        assert ((h.max(axis=1) < 0.03).sum()) == 5
        f0 = vr.to_viterbi_f0(h)
        assert (f0 == 0).sum() == 5


def test_zero_probability_jump_costs_the_float32_tiny(hidden):
    """Drops out for an oracle (or kernel) without the out-of-band term, or with the float64 tiny (log = -708)."""
    h, want = vr.zero_probability()
    for chain in ("ref", "f64"):
        assert np.array_equal(vr.viterbi_path(h, chain), want)
        # the final argmax decides between ending at 200 (one jump) and staying at 100 (six frames at probability zero)
        margin = vr.on_path_margin(h, chain)
        assert abs(margin - 87.34) < 0.01, margin
    assert abs(np.log(np.float64(vr.EPS)) + 87.3365) < 1e-4
    assert int((np.abs(np.diff(want)) >= 30).sum()) == 1


def test_edge_rows_pin_the_row_normalisation(hidden):
    h, want = vr.edge_rows()
    for chain in ("ref", "f64"):
        assert np.array_equal(vr.viterbi_path(h, chain), want)
        margin = vr.on_path_margin(h, chain)
        assert abs(margin - 0.059) < 0.002, margin
    tr = vr.transition()
    assert np.allclose(tr.sum(axis=1), 1) and tr[0, 0] > 1.9 * tr[180, 180] and (tr[0, 30:] == 0).all()
    assert int((tr[:, 180] > 0).sum()) == 59


@pytest.mark.parametrize("name", ["t33", "t37", "t200", "zero_probability", "edge_rows"])
def test_path_beats_argmax_and_perturbations(hidden, name):
    """Independent of the recursion: the returned path scores at least as high as the per-frame argmax path and as 100
    random single-frame perturbations of itself."""
    h = hidden[name]
    path = vr.viterbi_path(h, "f64")
    best = vr.path_score(h, path)
    assert best >= vr.path_score(h, h.argmax(axis=1))
    rng = np.random.default_rng(5)
    for _ in range(100):
        q = path.copy()
        t = int(rng.integers(len(q)))
        q[t] = int(np.clip(q[t] + rng.choice([-40, -3, -2, -1, 1, 2, 3, 40]), 0, vr.N_CLASS - 1))
        assert best >= vr.path_score(h, q)


def test_local_average_around_a_centre():
    """The window follows the centre, the threshold the frame maximum: a window of zeros on a voiced frame gives 10 Hz."""
    h = np.zeros((2, vr.N_CLASS), dtype=np.float32)
    h[:, 100] = 0.8
    f0 = vr.to_local_average_f0(h, np.array([100, 300]))
    assert abs(f0[0] - 10 * 2 ** ((100 * 20 + vr.CONST) / 1200)) < 1e-9 and f0[1] == 10.0
    assert np.array_equal(vr.to_local_average_f0(h), vr.to_local_average_f0(h, h.argmax(axis=1)))
