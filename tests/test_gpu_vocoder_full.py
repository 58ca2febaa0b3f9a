"""-m gpu parity of the NSF-HiFiGAN generator at the lengths real projects vocode, against the numpy oracle.

test_gpu_vocoder.py holds dsd_vocode to the oracle at T <= 130 frames (and mini_small at 2100); the paths below only
open up at production lengths, so they were checked there for finiteness and ragged == alone only:

  * 64-frame GEMM tiles (make_gemm: `nb = 2` once batch * ceil(T_stage / 64) * row tiles >= 512; the vocoder's
    GEMMs are on the generic path, whose LDS rule still admits them up to 256 channels at k = 11, dilation 5).
    Default layout, resblock convs: stage 0 (256 channels, 4 row tiles, 8 T frames) counts 4 B ceil(T / 8) and switches
    at T >= 1017 for B = 1, at T >= 505 for B = 2; stages 1 (128 channels, 64 T frames) and 2 (64, 128 T) count 2 B T
    and switch at T >= 256 / B.  So B = 1 at T = 1100 runs the resblock convs of every GEMM stage on 64-frame tiles,
    and B = 2 at T = 480 runs stage 0 on 32-frame tiles and stages 1 and 2 on 64-frame ones (at T = 600, B = 2 would
    put stage 0 on 64-frame tiles as well).  A ragged batch counts its valid tiles (the shape B lone calls would take):
    lengths [1100, 1, 257, 1025, 640] take the 64-frame tiles in their RAG = 1 instantiations.  tconv.hip (the 32- and
    16-channel stages) walks ~2200 / ~4400 256-sample tiles per item there.  A kernel trace of this file shows
    gemm_kernel<ST_LRELU, 0, EP_BIAS_ACT | EP_SCATTER | EP_BIAS_RES, NB = 2, ...> and <ST_PLAIN, 0, EP_BIAS_RES, 2, ...>
    with RAG = 0 and 1, and the 9 residual-block GEMMs of each kind on NB = 1 that the B = 2, T = 480 call leaves on
    stage 0.
  * SineGen's running phase across voc_phase_kernel's 2048-frame pieces (thread 0 carries `run` from one piece to
    the next): T = 4500 is three pieces, ragged lengths 2048 / 2049 / 4097 end on and just past a piece edge.  The
    same lengths on mini_small go through voc_fast_phase_kernel's pieces.  With `run` restarted at every piece, both
    small_rb2 tests fail (max_rel 0.07) while every test of test_gpu_vocoder.py and test_gpu_vocoder_ragged.py passes.

f0 has voiced and unvoiced runs with pitches up to 1100 Hz: the ninth harmonic's sine argument reaches ~800 rad.  The
tolerance is test_gpu_vocoder.py's TOL of the waveform range, on the max and on the RMS error.  Every oracle result is
computed once per module and kept (measured: 54 s of numpy for all of them on 8 CPUs, 23 s of wall time for the
default-layout tests on 16); the ragged item 0 is the dense B = 1 case.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from diffsinger_amd import synth  # noqa: E402
from gpu_util import check, dev  # noqa: E402
from oracle import vocoder as ov  # noqa: E402
from test_gpu_vocoder import OVER, TOL, build  # noqa: E402

T_FULL = 1100
LENS_FULL = [T_FULL, 1, 257, 1025, 640]
T_PIECES = 4500
LENS_PIECES = [T_PIECES, 2048, 2049, 4097]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"


def f0_track(t_len, seed):
    """Voiced runs (80 .. 1100 Hz: glides with vibrato) alternating with unvoiced ones (f0 = 0), 3 .. 120 frames each;
    one 20-frame run held at 1100 Hz."""
    rng = np.random.Generator(np.random.PCG64(seed))
    f0 = np.zeros(t_len, np.float32)
    t, voiced = 0, True
    while t < t_len:
        n = min(int(rng.integers(3, 121)), t_len - t)
        if voiced:
            a, b = 80.0 * (1100.0 / 80.0) ** rng.random(2)
            vib = 1.0 + 0.03 * np.sin(np.arange(n) * rng.uniform(0.2, 0.9))
            f0[t:t + n] = np.minimum(np.geomspace(a, b, n) * vib, 1100.0)
        t, voiced = t + n, not voiced
    if t_len > 40:
        f0[t_len // 3: t_len // 3 + 20] = 1100.0
    return f0


def item(h, t_len, seed):
    """One utterance's inputs: mel [M, T] (ln-mel), f0 [T], rand_ini [9], noise [T * upp, 9]."""
    upp = int(np.prod(h["upsample_rates"]))
    mel = (synth.synth_normal((h["num_mels"], t_len), seed) * 3.0 - 11.0).astype(np.float32)
    rand_ini = np.random.Generator(np.random.PCG64(seed + 1)).random(9).astype(np.float32)
    return mel, f0_track(t_len, seed + 2), rand_ini, synth.synth_normal((t_len * upp, 9), seed + 3)


def batch(h, lens, t_len, seed):
    """Items seed + 10 b at their own lengths, padded to t_len with junk (as test_gpu_vocoder_ragged.inputs)."""
    bsz, upp = len(lens), int(np.prod(h["upsample_rates"]))
    mel = np.full((bsz, h["num_mels"], t_len), 40.0, np.float32)
    f0 = np.full((bsz, t_len), 3000.0, np.float32)
    rand_ini = np.zeros((bsz, 9), np.float32)
    noise = np.full((bsz, t_len * upp, 9), 50.0, np.float32)
    for b, n in enumerate(lens):
        mel[b, :, :n], f0[b, :n], rand_ini[b], noise[b, :n * upp] = item(h, n, seed + 10 * b)
    return mel, f0, rand_ini, noise


class Case:
    """A generator and one padded batch; the oracle's waveform of item b alone at its own length with item i's
    rand_ini, computed on first use and kept (the module-scoped fixtures below share it between tests)."""

    def __init__(self, tag, lens, t_len, wseed, seed):
        self.gen, self.h, self.params = build(OVER[tag], wseed)
        self.upp = int(np.prod(self.h["upsample_rates"]))
        self.lens, self.t_len = lens, t_len
        self.mel, self.f0, self.rand_ini, self.noise = batch(self.h, lens, t_len, seed)
        self._want = {}

    def want(self, b, ini=None):
        ini = b if ini is None else ini
        if (b, ini) not in self._want:
            n = self.lens[b]
            self._want[b, ini] = ov.generator_forward(self.params, self.h, self.mel[b:b + 1, :, :n], self.f0[b:b + 1, :n],
                                                      self.rand_ini[ini], self.noise[b:b + 1, :n * self.upp])[0, 0]
        return self._want[b, ini]

    def dense(self, items):
        """dsd_vocode on full-length items: one rand_ini per call, items[0]'s."""
        assert all(self.lens[b] == self.t_len for b in items)
        with torch.no_grad():
            got = self.gen(dev(self.mel[items]), dev(self.f0[items]), rand_ini=dev(self.rand_ini[items[0]]),
                           noise=dev(self.noise[items]))[:, 0]
        assert tuple(got.shape) == (len(items), self.t_len * self.upp)
        return got

    def ragged(self, items):
        """dsd_vocode_ragged on items (padded to t_len), each with its own rand_ini."""
        lens = [self.lens[b] for b in items]
        with torch.no_grad():
            got = self.gen(dev(self.mel[items]), dev(self.f0[items]), lengths=lens, rand_ini=dev(self.rand_ini[items]),
                           noise=dev(self.noise[items]))[:, 0]
        assert tuple(got.shape) == (len(items), self.t_len * self.upp)
        for k, n in enumerate(lens):
            assert not got[k, n * self.upp:].any()              # zeroed past the item's end
        return got


@pytest.fixture(scope="module")
def full():
    c = Case("default", LENS_FULL + [T_FULL], T_FULL, 700, 710)
    yield c
    c.gen.release_native()


@pytest.fixture(scope="module")
def pair():
    c = Case("default", [480, 480], 480, 720, 730)
    yield c
    c.gen.release_native()


@pytest.fixture(scope="module", params=["small_rb2", "mini_small"])
def pieces(request):
    c = Case(request.param, LENS_PIECES + [T_PIECES], T_PIECES, 740, 750)
    yield c
    c.gen.release_native()


def test_vocoder_full_length_dense(full):
    """B = 1, T = 1100, default layout: every GEMM stage on 64-frame tiles (stage 0 from T = 1024), RAG = 0."""
    check(full.dense([0])[0], full.want(0), TOL, what="B=1 T=1100")


def test_vocoder_full_length_dense_pair(pair):
    """B = 2, T = 480, default layout: stage 0's resblock convs on 32-frame tiles (2 * 60 * 4 = 480 < 512), stages
    1 and 2 on 64-frame ones (2 * 480 * 2 = 1920, 2 * 960 = 1920), one rand_ini for the batch."""
    got = pair.dense([0, 1])
    for b in range(2):
        check(got[b], pair.want(b, 0), TOL, what=("B=2 T=480", b))


def test_vocoder_full_length_ragged(full):
    """RAG = 1 twin of the dense case: lengths [1100, 1, 257, 1025, 640], junk past each end, every item against the
    oracle alone at its own length (item 0 is the dense B = 1 case's oracle)."""
    items = list(range(len(LENS_FULL)))
    got = full.ragged(items)
    for b in items:
        check(got[b, :LENS_FULL[b] * full.upp], full.want(b), TOL, what=("ragged", b, LENS_FULL[b]))


def test_vocoder_phase_across_pieces_dense(pieces):
    """T = 4500 = three 2048-frame pieces of the phase scan, B = 2 (voc_phase_kernel / voc_fast_phase_kernel, RAG = 0)."""
    k = len(LENS_PIECES)
    got = pieces.dense([0, k])
    check(got[0], pieces.want(0), TOL, what="dense 0")
    check(got[1], pieces.want(k, 0), TOL, what="dense 1")


def test_vocoder_phase_across_pieces_ragged(pieces):
    """Lengths [4500, 2048, 2049, 4097]: on and next to the pieces' edges (RAG = 1)."""
    items = list(range(len(LENS_PIECES)))
    got = pieces.ragged(items)
    for b in items:
        check(got[b, :LENS_PIECES[b] * pieces.upp], pieces.want(b), TOL, what=("ragged", b, LENS_PIECES[b]))
