"""-m gpu: the NSF-HiFiGAN vocoder at every configuration dsd_vocoder_create accepts (cases: vocoder_config_cases.py) - every
tap count of the phase-row packing (k = u .. 8u), odd rates, one stage and eight, stage widths down to 1, padded input rows,
the residual convolutions at k = 1 .. 15 on gemm.hip, tconv.hip and voc_x3.hip, the noise conv's window at and beyond the
default LDS limit, the source at 1 and 16 harmonics, and the acceptance limits themselves.

Reference: oracle/vocoder.py in its float64 mode (everything after the fp32 source in float64), which
test_vocoder_configs_host.py pins against the reference Generator (G28).  Bound: TOL = 5e-5 of the waveform range - every floor
(fp32 oracle vs float64 oracle, vocoder_config_cases.FLOORS) is below TOL / 2, so no case takes the 2 x floor rule.

What each part is there to catch (by the arithmetic, not by a mutated run): without voc_noise_groups' cap and the raised LDS
limit `noise_window*` ask for 65 792 / 262 400 bytes of dynamic LDS and cannot launch; `k_eq_u`, `k_4u_6u`, `k_8u` and
`odd_rates` are the only cases in the suite whose phase rows have other than 3 taps or a rate that does not divide the row tile,
so an error in k0 / e / D of build_packed_voc that k = 2u hides shows there; without the create-time checks the refusal table
fails."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vocoder_config_cases as cc  # noqa: E402
from gpu_util import dev, rel_err  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
X3 = "voc_conv_x3_kernel<"
_SENTINEL = 0x5A5A5A50
DENSE = [(tag, b, t) for tag, c in cc.CASES.items() for b, t in c["shapes"]]


@pytest.fixture(autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    saved = {k: os.environ.pop(k, None) for k in ("DSD_PRECISION", "DSD_X3_WIDE")}
    yield
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def build(tag):
    from diffsinger_amd.vocoder import Generator
    g = Generator(cc.config(tag))
    g.load_state_dict({k: torch.from_numpy(v) for k, v in cc.weights(tag).items()}, strict=True)
    return g.cuda().eval()


def run(gen, i, lengths=None, transposed=False):
    mel = dev(i["mel"])
    if transposed:          # [B, T, M] storage viewed as [B, M, T]
        mel = dev(np.ascontiguousarray(i["mel"].transpose(0, 2, 1))).transpose(1, 2)
    with torch.no_grad():
        out = gen(mel, dev(i["f0"]), lengths=lengths, rand_ini=dev(i["rand_ini"]), noise=dev(i["noise"]),
                  pre_noise=dev(i["pre_noise"]))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("tag,bsz,t_len", DENSE)
def test_config_vs_float64_oracle(tag, bsz, t_len):
    gen = build(tag)
    i = cc.inputs(tag, bsz, t_len)
    got = run(gen, i)
    upp = int(np.prod(cc.config(tag)["upsample_rates"]))
    assert tuple(got.shape) == (bsz, 1, t_len * upp)
    err = rel_err(got, cc.reference(tag, bsz, t_len))
    print(f"{tag} ({bsz}, {t_len}): vs float64 oracle {err:.3e} (floor {cc.FLOORS[(tag, bsz, t_len)]:.2e}, "
          f"bound {cc.bound(tag, bsz, t_len):.1e}); {cc.CASES[tag]['reaches']}")
    assert err < cc.bound(tag, bsz, t_len)
    assert torch.equal(run(gen, i, transposed=True), got)      # strided input: the same bits
    assert torch.equal(run(gen, i), got)                        # and again: nothing left over from the first call
    gen.release_native()


@pytest.mark.parametrize("tag", cc.G28)
def test_config_vs_reference_fixture(tag):
    """the G28 form of the case (the dilation lists the reference's residual blocks can build) against the reference
    Generator's own waveform"""
    g = np.load(os.path.join(GOLDEN, "g28_vocoder_configs.npz"))
    form = "g28:" + tag
    i = cc.inputs(form, *cc.G28_SHAPE)
    assert np.array_equal(i["f0"], g[f"{tag}_f0"]) and np.array_equal(i["rand_ini"], g[f"{tag}_rand_ini"])
    gen = build(form)
    got = run(gen, i)
    err = rel_err(got, g[f"{tag}_wav"])
    print(f"G28 {tag}: vs reference {err:.3e}")
    assert err < cc.TOL
    assert rel_err(got, cc.reference(form, *cc.G28_SHAPE)) < cc.TOL
    gen.release_native()


@pytest.mark.parametrize("tag", cc.RAGGED)
def test_ragged_items(tag):
    """forward(lengths=): each item against its lone call (test_gpu_vocoder_ragged.py's rule) and against the oracle"""
    lens, t_len = cc.RAGGED_LENGTHS, cc.RAGGED_T
    gen = build(tag)
    upp = int(np.prod(cc.config(tag)["upsample_rates"]))
    i = cc.inputs(tag, len(lens), t_len)
    batch = dict(i, rand_ini=np.repeat(i["rand_ini"][None], len(lens), 0))     # the ragged call takes one row of phases per item
    got = run(gen, batch, lengths=lens)
    assert tuple(got.shape) == (len(lens), 1, t_len * upp)
    for b, n in enumerate(lens):
        alone = run(gen, cc.item_inputs(tag, len(lens), t_len, b, n))
        scale = max(1.0, float(alone.abs().max()))
        assert float((got[b:b + 1, :, :n * upp] - alone).abs().max()) <= cc.SAME * scale, (tag, b, n)
        assert not got[b, 0, n * upp:].any()                # zeroed past the item's end
        err = rel_err(got[b:b + 1, :, :n * upp], cc.ragged_reference(tag, b))
        print(f"{tag} ragged item {b} (T = {n}): vs float64 oracle {err:.3e}")
        assert err < cc.TOL, (tag, b, n)
    gen.release_native()


@pytest.mark.parametrize("tag,mbw", [("x3_c384", {"3", "2"}), ("x3_c320", {"3"})])
def test_split_bf16_layouts(tag, mbw):
    """set_precision("bf16x3") at taps 1 / 13 / 15 and C = 192 / 96 / 160: voc_x3.hip really ran, at the row-block counts the
    widths mean (192 and 160 -> 3 per wave, 96 -> 2), and the result keeps the fp32 bound"""
    (bsz, t_len), = cc.X3[tag]["shapes"]
    gen = build(tag)
    i = cc.inputs(tag, bsz, t_len)
    f32 = run(gen, i)
    assert rel_err(f32, cc.reference(tag, bsz, t_len)) < cc.bound(tag, bsz, t_len)
    gen.set_precision("bf16x3")
    gen.kernel_timing(True)
    got = run(gen, i)
    names = sorted(c["name"] for c in gen.kernel_classes() if c["name"].startswith(X3))
    assert {n.split("<")[1].split(",")[0] for n in names} == mbw and all(n.endswith(" 0>") for n in names), names
    assert gen.stats()["precision"] == 1
    assert not torch.equal(got, f32)
    err = rel_err(got, cc.reference(tag, bsz, t_len))
    print(f"{tag} ({bsz}, {t_len}): bf16x3 vs float64 oracle {err:.3e}; {names}")
    assert err < cc.TOL
    gen.release_native()


@pytest.mark.parametrize("over,fragment", cc.REFUSE, ids=[str(sorted(o.items())) for o, _ in cc.REFUSE])
def test_create_refuses(over, fragment):
    """dsd_vocoder_create returns DSD_EINVAL with the layer named, before anything is launched or allocated; its verdict is
    accepts()'s"""
    from diffsinger_amd import _lib
    h = cc.over_default(**over)
    ok, reason = cc.accepts(h)
    out = C.c_void_p(_SENTINEL)
    rc = _lib.lib().dsd_vocoder_create(C.byref(cc.native_config(h, torch.cuda.current_device())), C.byref(out))
    msg = _lib.lib().dsd_last_error(None).decode()
    assert rc == -1 and not ok, (rc, ok, msg)
    assert out.value == _SENTINEL, "*out was written on a failed create"
    assert fragment in msg and reason in msg, (fragment, reason, msg)


def test_create_accepts_the_edges():
    """the widest of each kind next to the refusal table's rows: created, and the verdict is accepts()'s"""
    from diffsinger_amd import _lib
    lib = _lib.lib()
    for over in cc.ACCEPT_EDGE:
        h = cc.over_default(**over)
        out = C.c_void_p()
        rc = lib.dsd_vocoder_create(C.byref(cc.native_config(h, torch.cuda.current_device())), C.byref(out))
        assert rc == 0 and cc.accepts(h) == (True, ""), (over, lib.dsd_last_error(None))
        lib.dsd_destroy(out)
