"""Numpy restatement of the seeded generator of dsd_noise_fill (specification: include/dsdenoise.h).

Philox4x32-10 in uint64 integer arithmetic; the uniform in exact arithmetic (every step is representable, so float64
holds it exactly and the fp32 cast changes nothing); the normal in float64 FROM those uniforms - the device evaluates
the same Box-Muller in fp32, and the tests bound the difference.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)

X_T, STEP, VOC_SOURCE, VOC_PRE, VOC_PHASE, PITCH_X_T, VARIANCE_X_T = 1, 2, 3, 4, 5, 6, 7


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (broadcastable), key: two ints -> four uint64 arrays holding 32-bit words."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def uniform(w):
    """((w >> 9) + 0.5) * 2^-23 as float64 (exact; equal to its own fp32 cast)."""
    return ((np.asarray(w, dtype=np.uint64) >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def words(seed, domain, stream, rows, cols):
    """-> uint64 [rows, ceil(cols / 4), 4]: the Philox words of one item's tensor."""
    ncb = (cols + 3) // 4
    r = np.arange(rows, dtype=np.uint64)[:, None]
    cb = np.arange(ncb, dtype=np.uint64)[None, :]
    w = philox4x32_10((cb, r, np.uint64(stream & 0xFFFFFFFF), np.uint64(domain)), (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(w, axis=-1)


def draw(seed, domain, stream, rows, cols, kind="normal"):
    """-> float64 [rows, cols]: element (row, col) of stream `stream` under (seed, domain)."""
    w = words(seed, domain, stream, rows, cols)
    if kind == "uniform":
        e = uniform(w)
    else:
        u = uniform(w)
        e = np.empty_like(u)
        for a in (0, 2):
            r = np.sqrt(-2.0 * np.log(u[..., a]))
            theta = 2.0 * np.pi * u[..., a + 1]
            e[..., a], e[..., a + 1] = r * np.cos(theta), r * np.sin(theta)
    return e.reshape(rows, -1)[:, :cols]


def fill(shape, seeds, domain, first_stream=0, kind="normal"):
    """-> float64 [n, B, rows, cols], as noise.fill lays it out."""
    n, b, rows, cols = shape
    seeds = [seeds] * b if isinstance(seeds, int) else list(seeds)
    return np.stack([np.stack([draw(seeds[i], domain, first_stream + k, rows, cols, kind) for i in range(b)])
                     for k in range(n)])
