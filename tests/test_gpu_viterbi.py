"""-m gpu: the Viterbi decode of RMVPE (dsd_rmvpe_decode_viterbi / dsd_rmvpe_decode_at, RMVPE.decode_viterbi) against the
numpy restatement of to_viterbi_f0 and librosa.sequence.viterbi in tests/viterbi_ref.py.

The path is discrete, so it must be EQUAL to the oracle's: tests/test_viterbi_host.py shows that on these inputs the float32
and the float64 formation of log_prob agree and that the path is chosen with a margin of at least 1e-4, eight orders above
what the double recursion can lose.  f0 is the fp32 local average around that path: rtol 2e-6 of the float64 oracle, the
bound of tests/test_gpu_rmvpe.py::test_decode_crafted for the same kernel."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rmvpe_ref  # noqa: E402
import viterbi_ref as vr  # noqa: E402
from diffsinger_amd import synth  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WEIGHT_SEED, CLIP_SEED, CLIP_SAMPLES = 1800, 1880, 6500     # chosen on the CPU: the float64 hidden's on-path margin is 0.66
MAX_T = 131072                                              # the documented cap of include/dsdenoise.h


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"


@pytest.fixture(scope="module")
def pe():
    from diffsinger_amd.pitch import RMVPE
    sd = synth.rmvpe_state_dict(seed=WEIGHT_SEED, with_tf=True, **synth.RMVPE_SMALL)
    ext = RMVPE(sd)
    ext.sd = sd
    return ext


@pytest.fixture(scope="module")
def hidden():
    return vr.cases()


@pytest.fixture(scope="module")
def want(hidden):
    """name -> (path, f0) of the oracle, computed once."""
    out = {}
    for name, h in hidden.items():
        path = vr.viterbi_path(h, "ref")
        out[name] = (path, vr.to_local_average_f0(h, path))
    return out


CASES = [m[0] for m in vr.MELODIES] + ["zero_probability", "edge_rows"]


@pytest.mark.parametrize("name", CASES)
def test_path_equals_oracle(pe, hidden, want, name):
    h = hidden[name]
    f0, path = pe.decode_viterbi(torch.from_numpy(h)[None].cuda(), return_path=True)
    wpath, wf0 = want[name]
    assert path.shape == wpath.shape and path.dtype == np.int64
    wrong = np.nonzero(path != wpath)[0]
    voiced = wf0 > 0
    rel = float((np.abs(f0 - wf0)[voiced] / wf0[voiced]).max()) if voiced.any() else 0.0
    print(f"{name}: {len(wrong)} of {len(wpath)} states differ; f0 max rel err {rel:.3g}")
    assert wrong.size == 0, (wrong[:10], path[wrong[:10]], wpath[wrong[:10]])
    assert np.array_equal(f0 > 0, wf0 > 0)
    np.testing.assert_allclose(f0, wf0, rtol=2e-6)
    if name == "zero_probability":
        assert np.array_equal(path, vr.zero_probability()[1])
    if name == "edge_rows":
        assert np.array_equal(path, vr.edge_rows()[1])


@pytest.mark.parametrize("name", ["t37", "t200", "zero_probability"])
def test_decode_at_a_centre(pe, hidden, name):
    h = torch.from_numpy(hidden[name])[None].cuda()
    f0, path = pe.decode_viterbi(h, return_path=True)
    assert np.array_equal(pe.decode(h, center=path), f0)
    assert np.array_equal(pe.decode(h, center=torch.from_numpy(path).cuda()), f0)
    assert np.array_equal(pe.decode(h, center=hidden[name].argmax(axis=1)), pe.decode(h))
    # the window follows the centre, the threshold the frame's maximum: a window of zeros on a voiced frame gives 10 Hz
    if name == "zero_probability":
        far = pe.decode(h, center=np.full(len(path), 300))
        assert np.array_equal(far, np.full(len(path), 10.0, dtype=np.float32))


def test_ragged_items_equal_lone_calls(pe, hidden):
    names = ["t1", "t2", "t33", "t37", "t64", "t200"]
    lens = [len(hidden[n]) for n in names]
    tmax = max(lens)
    batch = torch.rand(len(names), tmax, vr.N_CLASS, generator=torch.Generator().manual_seed(3))     # past T_b: never read
    for i, n in enumerate(names):
        batch[i, : lens[i]] = torch.from_numpy(hidden[n])
    batch = batch.cuda()
    f0 = torch.full((len(names), tmax), -7.0, device="cuda")
    path = torch.full((len(names), tmax), -7, dtype=torch.int32, device="cuda")
    pe._viterbi(batch, lens, 0.03, f0, path)
    f0, path = f0.cpu().numpy(), path.cpu().numpy()
    lists = pe.decode_viterbi(batch, lengths=lens, return_path=True)
    for i, n in enumerate(names):
        f0_1, path_1 = pe.decode_viterbi(torch.from_numpy(hidden[n])[None].cuda(), return_path=True)
        assert np.array_equal(path[i, : lens[i]], path_1) and np.array_equal(f0[i, : lens[i]], f0_1)
        assert (f0[i, lens[i]:] == -7.0).all() and (path[i, lens[i]:] == -7).all()
        assert np.array_equal(lists[0][i], f0_1) and np.array_equal(lists[1][i], path_1)


@pytest.fixture(scope="module")
def clip():
    sys.path.insert(0, GOLDEN)
    from make_golden_rmvpe import waveform
    return waveform(CLIP_SEED, CLIP_SAMPLES)


@pytest.fixture(scope="module")
def end_to_end(pe, clip):
    """(f0 of infer_from_audio, (f0, hidden) of the ragged call), both with use_viterbi=True."""
    lone = pe.infer_from_audio(clip, 16000, use_viterbi=True)
    ragged = pe.infer_from_audio_ragged([clip], 16000, want_hidden=True, use_viterbi=True)[0]
    return lone, ragged


def test_end_to_end(pe, clip, end_to_end):
    lone, (f0, hid) = end_to_end
    assert hid.shape == (41, vr.N_CLASS) and lone.shape == (41,)
    assert np.array_equal(lone, f0)
    f0_d, path = pe.decode_viterbi(torch.from_numpy(hid)[None].cuda(), return_path=True)
    assert np.array_equal(f0_d, f0)
    # the clip and the weights were chosen on the CPU for a margin of 0.66 on the float64 hidden; the GPU's hidden is within
    # 2.2e-6 of that one (test_gpu_rmvpe.py), so the margin here can only miss 1e-4 if the seeds are wrong
    h64 = rmvpe_ref.mel2hidden(rmvpe_ref.log_mel(clip), {k: np.asarray(v) for k, v in pe.sd.items()})
    assert vr.on_path_margin(h64.astype(np.float32)) >= 1e-3
    margin = min(vr.on_path_margin(hid, "ref"), vr.on_path_margin(hid, "f64"))
    assert margin >= 1e-4, f"on-path margin {margin:.3g} on the GPU's hidden: choose another seed"
    wpath = vr.viterbi_path(hid, "ref")
    assert np.array_equal(path, wpath)
    assert (wpath != hid.argmax(axis=1)).any()            # the Viterbi decode is not the local-average one on this clip
    assert not np.array_equal(f0, pe.infer_from_audio(clip, 16000))
    np.testing.assert_allclose(f0, vr.to_local_average_f0(hid, wpath), rtol=2e-6)


@pytest.mark.parametrize("speed,interp", [(1, False), (1.25, True)])
def test_get_pitch_viterbi(pe, clip, end_to_end, speed, interp):
    f0 = end_to_end[0]
    length = int(np.ceil(len(clip) / round(128 * speed)))
    f0r, uvr = pe.get_pitch(clip, 16000, length, hop_size=128, speed=speed, interp_uv=interp, use_viterbi=True)
    wf, wuv = rmvpe_ref.get_pitch_post(f0, 16000, length, 128, speed, interp)
    assert f0r.shape == (length,) and uvr.dtype == bool
    assert np.array_equal(uvr, wuv)
    np.testing.assert_allclose(f0r, wf, rtol=1e-5)
    plain = pe.get_pitch(clip, 16000, length, hop_size=128, speed=speed, interp_uv=interp)[0]
    assert not np.array_equal(plain, f0r)


def test_limits_and_handle_kinds(pe):
    from diffsinger_amd import _lib
    lib = _lib.lib()
    h = torch.rand(1, 4, vr.N_CLASS, device="cuda")
    f0 = torch.zeros(1, 4, device="cuda")
    c = torch.zeros(1, 4, dtype=torch.int32, device="cuda")
    hp, fp, cp = (C.c_void_p(x.data_ptr()) for x in (h, f0, c))
    T = MAX_T + 1           # refused before any launch: the 4-frame buffers are never read
    assert lib.dsd_rmvpe_decode_viterbi(pe._h, hp, 1, T, T * 360, 360, None, 0.03, fp, T, None, 0, None) == -1     # DSD_EINVAL
    assert str(MAX_T).encode() in lib.dsd_last_error(pe._h)
    assert lib.dsd_rmvpe_decode_at(pe._h, hp, cp, 1, T, T * 360, 360, T, 0.03, fp, T, None) == -1
    assert str(MAX_T).encode() in lib.dsd_last_error(pe._h)
    assert lib.dsd_rmvpe_decode_viterbi(pe._h, hp, 16, MAX_T, MAX_T * 360, 360, None, 0.03, fp, MAX_T, None, 0, None) == -1
    assert b"1048576" in lib.dsd_last_error(pe._h)
    lens = (C.c_int64 * 1)(5)
    assert lib.dsd_rmvpe_decode_viterbi(pe._h, hp, 1, 4, 4 * 360, 360, lens, 0.03, fp, 4, None, 0, None) == -1
    with pytest.raises(NotImplementedError, match="decode_viterbi"):
        pe.decode(h, use_viterbi=True)
    cfg = _lib.DsdMelConfig(C.sizeof(_lib.DsdMelConfig), 16000, 1024, 1024, 160, 128, 30.0, 8000.0, 1e-5, 0)
    mh = C.c_void_p()
    assert lib.dsd_mel_create(C.byref(cfg), C.byref(mh)) == 0
    assert lib.dsd_rmvpe_decode_viterbi(mh, hp, 1, 4, 4 * 360, 360, None, 0.03, fp, 4, None, 0, None) == -2         # DSD_ESTATE
    assert lib.dsd_rmvpe_decode_at(mh, hp, cp, 1, 4, 4 * 360, 360, 4, 0.03, fp, 4, None) == -2
    lib.dsd_destroy(mh)


def test_all_zero_frame_returns_states(pe, hidden):
    """The reference's probabilities are NaN from such a frame on; here the call returns and every state is a state."""
    h = hidden["t64"].copy()
    h[20] = 0
    _, path = pe.decode_viterbi(torch.from_numpy(h)[None].cuda(), return_path=True)
    assert path.shape == (64,) and path.min() >= 0 and path.max() <= 359
