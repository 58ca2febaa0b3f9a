"""Host-only: the index arithmetic of the Winograd F(2,3) conv of wn_rowsplit.hip (wn_conv_wq_kernel), in numpy, against the
oracle's _dilated_conv3.  The model follows the kernel: 32-frame tiles; pair p of a tile is frame f(p) = p + d (p // d) with its
partner at f(p) + d; the operands are zero outside [0, T) BEFORE the differences; G0 .. G3 as api.hip forms them; outputs past T
are dropped."""
import numpy as np
import pytest

from oracle import backbones as ob


def winograd_conv3(x, w, b, dil, dtype):
    bsz, cin, t_len = x.shape
    g0, g1, g2 = (w[:, :, k].astype(np.float64) for k in range(3))
    G = [m.astype(dtype) for m in (g0, 0.5 * (g0 + g1 + g2), 0.5 * (g0 - g1 + g2), g2)]
    tiles = (t_len + 31) // 32
    xp = np.zeros((bsz, cin, 32 * tiles + 32), dtype)          # frame f at column f + 8 (halo 8)
    xp[:, :, 8:8 + t_len] = x
    y = np.zeros((bsz, w.shape[0], 32 * tiles + 8), dtype)
    p = np.arange(16)
    for tile in range(tiles):
        f = 32 * tile + p + dil * (p // dil)                    # the pairs' first frames
        xm, x0, x1, x2 = (xp[:, :, f + 8 + s * dil] for s in (-1, 0, 1, 2))
        m = [np.matmul(Gi, Di) for Gi, Di in zip(G, (xm - x1, x0 + x1, x1 - x0, x0 - x2))]
        y[:, :, f] = m[0] + m[1] + m[2]
        y[:, :, f + dil] = m[1] - m[2] - m[3]
    return y[:, :, :t_len] + b[None, :, None].astype(dtype)


@pytest.mark.parametrize("t_len", [7, 37, 70])
@pytest.mark.parametrize("dil", [1, 2, 4, 8])
def test_pairing_covers_every_frame_once(dil, t_len):
    p = np.arange(16)
    f = p + dil * (p // dil)
    assert sorted(np.concatenate([f, f + dil]).tolist()) == list(range(32))
    rng = np.random.default_rng(100 * dil + t_len)
    x = rng.standard_normal((2, 24, t_len)).astype(np.float32)
    w = (rng.standard_normal((40, 24, 3)) / np.sqrt(72)).astype(np.float32)
    b = rng.standard_normal(40).astype(np.float32)
    want = ob._dilated_conv3(x, w, b, dil)
    # exact arithmetic apart from float64 rounding: any wrong index shows as an O(1) difference
    got64 = winograd_conv3(x.astype(np.float64), w, b, dil, np.float64)
    xp = np.zeros((2, 24, t_len + 2 * dil))
    xp[:, :, dil:dil + t_len] = x
    want64 = sum(np.matmul(w[:, :, k].astype(np.float64), xp[:, :, k * dil:k * dil + t_len]) for k in range(3)) + b[None, :, None]
    assert np.abs(got64 - want64).max() <= 1e-12 * np.abs(want64).max()
    # fp32 throughout, as the kernel computes: the same bound the GPU test allows Winograd against the direct kernel
    got32 = winograd_conv3(x, w, b, dil, np.float32)
    assert got32.dtype == np.float32
    assert np.abs(got32.astype(np.float64) - want).max() <= 4e-6 * np.abs(want).max()
