"""CPU checks of the VR separator and the variance curves: the torch mirror's state_dict against G19's reference layout,
the float64 oracle against G19, predict_from_audio's padding arithmetic, hand-checked RMS / dB values, the tension
domains, config.yaml loading, the ctypes struct, and the resource / store-hazard checks of hnsep_kernels.hip.  No GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import hnsep_ref
import mel_ref
from diffsinger_amd import _lib, hnsep, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def g19():
    return np.load(os.path.join(GOLDEN, "g19_hnsep.npz"))


def test_state_dict_names_and_shapes():
    z = g19()
    m = hnsep.CascadedNet(**synth.HNSEP_PROD)
    got = {k: ",".join(map(str, v.shape)) for k, v in m.state_dict().items()}
    assert list(got) == [str(k) for k in z["keys"]]
    assert list(got.values()) == [str(s) for s in z["key_shapes"]]
    n = sum(v.numel() for k, v in m.state_dict().items() if not k.endswith("num_batches_tracked"))
    assert 14e6 < n < 15.5e6            # ~14.7 M parameters at the production layout


@pytest.mark.parametrize("n,hop", [(200, 128), (5127, 128), (16000, 128), (441000, 512), (1, 512), (512 * 31 - 1, 512),
                                   (512 * 31, 512)])
def test_padding_arithmetic(n, hop):
    left, right, frames = hnsep.padding(n, hop)
    assert frames % 32 == 0 and left % hop == 0 and left >= 0 and right >= 0
    # torch.stft(center=True) of the padded clip has exactly `frames` frames
    assert (n + left + right) // hop + 1 == frames
    assert frames == 32 * ((n // hop + 1) // 32 + 1)
    assert _lib.lib().dsd_hnsep_num_frames(n, hop) == frames


def test_rms_and_db_by_hand():
    # a constant 0.5 over 8 samples, win 4, hop 2: zero-padded frames at both ends
    y = np.full(8, 0.5)
    r = hnsep_ref.rms(y, 2, 4)
    assert len(r) == 5
    assert r[0] == pytest.approx(np.sqrt(2 * 0.25 / 4)) and r[2] == pytest.approx(0.5)
    assert r[-1] == pytest.approx(np.sqrt(2 * 0.25 / 4))
    e = hnsep_ref.energy(y, 7, 2, 4)                     # padded to 7 frames with zeros
    assert len(e) == 7
    assert e[2] == pytest.approx(20 * np.log10(0.5))
    assert e[5] == pytest.approx(e.max() - 80.0)          # the zero frames sit at the top-db clamp
    assert len(hnsep_ref.energy(y, 3, 2, 4)) == 3         # cropped
    db = hnsep_ref.amplitude_to_db(np.array([1.0, 1e-7, 0.1]))
    assert db.tolist() == pytest.approx([0.0, -80.0, -20.0])   # amin 1e-5 -> -100 dB, then the clamp at max - 80


def test_tension_domains():
    h = np.sin(np.arange(4096) / 7.0)
    b = 0.6 * h
    r = hnsep_ref.tension(h, b, 10, 256, 1024, "ratio")
    assert r[4] == pytest.approx(0.8, abs=1e-3)           # sqrt(1 - 0.36)
    lg = hnsep_ref.tension(h, b, 10, 256, 1024, "logit")
    assert lg[4] == pytest.approx(np.log(r[4] / (1 - r[4])), abs=1e-9)
    db = hnsep_ref.tension(h, b, 10, 256, 1024, "db")
    assert db[4] == pytest.approx(20 * np.log10(r[4]), abs=1e-6)
    z = hnsep_ref.tension(h, h, 10, 256, 1024, "logit")  # no harmonics above the base: the lower clip
    assert z[4] == pytest.approx(np.log(1e-4 / (1 - 1e-4)))


def test_config_yaml_loading(tmp_path):
    cfg = dict(synth.HNSEP_SMALL)
    sd = synth.hnsep_state_dict(cfg, 1900)
    p = tmp_path / "model.pt"
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, p)
    (tmp_path / "config.yaml").write_text("n_fft: 512\nhop_length: 128\nn_out: 8\nn_out_lstm: 16\nis_mono: true\n")
    assert hnsep.read_config(p) == cfg
    m = hnsep.load_sep_model(p)
    assert not m.training
    assert torch.equal(m.state_dict()["out.weight"], torch.from_numpy(sd["out.weight"]))


def test_ctypes_struct():
    assert C.sizeof(_lib.DsdHnsepConfig) == 7 * 4
    assert [f[0] for f in _lib.DsdHnsepConfig._fields_] == ["struct_size", "n_fft", "hop_length", "nout", "nout_lstm",
                                                           "is_mono", "device"]


@pytest.mark.parametrize("i", [0, 3])
def test_oracle_reproduces_g19(i):
    """the float64 chain against the reference's fp32 run, within the fp32 floor G19 records."""
    z = g19()
    wseed, yseed, n, ci = (int(v) for v in z[f"c{i}_meta"])
    sys.path.insert(0, GOLDEN)
    import make_golden_hnsep
    cfg = list(make_golden_hnsep.CONFIGS.values())[ci]
    x = mel_ref.waveform(yseed, n, 44100).astype(np.float32)
    h, m = hnsep_ref.separate(hnsep_ref.model64(synth.hnsep_state_dict(cfg, wseed), cfg), x, cfg)
    fl_h, fl_m, mid = z[f"c{i}_floor"]
    assert np.abs(h - z[f"c{i}_harmonic"]).max() <= fl_h * 1.0001
    assert np.abs(m - z[f"c{i}_mask"]).max() <= fl_m * 1.0001
    assert mid > 0.1


def test_base_harmonic_oracle_g19():
    z = g19()
    sys.path.insert(0, GOLDEN)
    import make_golden_hnsep as g
    b = hnsep_ref.base_harmonic(z[f"c{g.BASE_CASE}_harmonic"], z["base_f0"], 44100, g.BASE_HOP, g.BASE_WIN)
    assert np.abs(b - z["base_harmonic"]).max() <= float(z["base_floor"][0]) * 1.0001


def test_world_stays_on_the_reference():
    with pytest.raises(NotImplementedError, match="world"):
        hnsep.DecomposedWaveform(np.zeros(1000, np.float32), 44100, np.zeros(3), hop_size=512, win_size=2048,
                                 algorithm="world")


def test_kernel_resources_and_store_hazard():
    """hnsep_kernels.hip stays in registers and has no store / VALU-overwrite pair (hipcc cross-compiles; no GPU)."""
    for tool in ("check_resources.py", "check_store_hazard.py"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), "hnsep_kernels.hip"], capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
        assert "hnsep_kernels.hip" in r.stdout
