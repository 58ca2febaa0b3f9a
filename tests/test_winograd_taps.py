"""Host-only: the walk of wn_conv_wq_kernel (wn_rowsplit.hip) over the DIRECT packed conv matrix, in numpy.

The kernel streams the three tap blocks of a k16 block ([chunk][tap][k16] packing, 12 blocks per chunk and 16-row block) and
walks a quarter (one 64-channel chunk) in groups of four steps - the four Winograd products of one k16 block in the order
G0 = g0, G3 = g2, G1, G2 - forming 2 G1 = s + g1, 2 G2 = s - g1, s = g0 + g2 in fp32 registers; the output transform halves the
two products (a factor 2 is exact in every product and sum, so this is G1 = (s + g1) / 2 bit for bit).  Modelled here:
  * the step -> (half, k16, product) map, the block offsets into the packing and the load schedule of the two-group ring;
  * the walk itself on a packed random matrix against a float64 convolution (any wrong block shows as an O(1) difference);
  * the forming identity: fp32-formed G1, G2 against the double-formed ones through one layer's convolution."""
import numpy as np
import pytest

NCH, NQ, NG, NS = 4, 16, 4, 48          # chunks of 64 channels; steps and groups per quarter; blocks per packed row block
PROD_OF_SLOT = [(0x2130 >> (4 * s)) & 3 for s in range(4)]          # the kernel's nibble tables
TAP_OF_ISSUE = [(0x120 >> (4 * s)) & 3 for s in range(3)]
LW, LB = 5, 6                            # late rows (channels [32, 64) of a chunk): written after step LW, barrier after LB
TAPS_OF_PRODUCT = {0: {0}, 1: {0, 1, 2}, 2: {0, 1, 2}, 3: {2}}


def step_map(t):
    g, slot = divmod(t, 4)
    return g // 2, g, PROD_OF_SLOT[slot]          # (32-channel half, k16 block of the chunk, product)


def load_schedule():
    """[(issuing step, k4 slot j, group, tap, row block)] of one wave; the prologue counts as step -1"""
    out = [(-1, 0, 0, 0, 0), (-1, 1, 0, 0, 1)]
    for t in range(NQ):
        g, slot = divmod(t, 4)
        for j in range(4):
            if t == 0:
                out.append((t, j, 0, 2 - j // 2, j & 1))
            elif g == 0 and j < 2:
                out.append((t, j, 1, TAP_OF_ISSUE[slot - 1], j))
            elif g >= 1 and g + 1 < NG and slot < 3 and j < 2:
                out.append((t, j, g + 1, TAP_OF_ISSUE[slot], j))
    return out


def block_index(mtile, wr, kq, g, tap, rb):
    """256-float block of the packed matrix: row block 4 mtile + 2 wr + rb, then [chunk kq][tap][k16 g]"""
    return (4 * mtile + 2 * wr + rb) * NS + 12 * kq + tap * 4 + g


def test_step_map():
    assert PROD_OF_SLOT == [0, 3, 1, 2] and TAP_OF_ISSUE == [0, 2, 1]
    seen = [step_map(t) for t in range(NQ)]
    assert sorted((k, p) for _, k, p in seen) == [(k, p) for k in range(4) for p in range(4)]        # every (k16, product) once
    assert all(h == k // 2 for h, k, _ in seen)
    assert [h for h, _, _ in seen] == [0] * 8 + [1] * 8       # steps 0 .. 7 read only channels [0, 32) of the chunk
    # the late rows are in LDS behind the barrier before step 7 fetches step 8's B fragments
    assert 2 <= LW <= LB <= 8 - 2


def test_blocks_hit_once_per_product_that_needs_them():
    sched = load_schedule()
    assert len(sched) == 6 * NG           # six loads per group where the four-matrix operand took eight
    for mtile in range(8):
        for wr in range(2):
            per_q = []
            for kq in range(NCH):
                loaded = {}
                for t, j, g, tap, rb in sched:
                    blk = block_index(mtile, wr, kq, g, tap, rb)
                    assert blk not in loaded
                    loaded[blk] = (t, j)
                # exactly the 12 blocks [chunk kq][tap][k16] of this wave's two row blocks
                want = {(4 * mtile + 2 * wr + rb) * NS + 12 * kq + tap * 4 + k for rb in range(2) for tap in range(3) for k in range(4)}
                assert set(loaded) == want
                # every step finds the tap blocks its product needs, each loaded once, issued before the step
                uses = {}
                for t in range(NQ):
                    _, k16, prod = step_map(t)
                    for tap in TAPS_OF_PRODUCT[prod]:
                        for rb in range(2):
                            blk = block_index(mtile, wr, kq, k16, tap, rb)
                            first_need = 4 * k16 + (0 if tap == 0 else 1)          # g0: product 0's step; g2, g1: product 3's (the forming)
                            assert loaded[blk][0] < first_need
                            uses.setdefault(blk, []).append(prod)
                for blk, prods in uses.items():
                    tap = ((blk % NS) % 12) // 4
                    assert sorted(prods) == sorted(p for p in range(4) if tap in TAPS_OF_PRODUCT[p])
                per_q.append(set(loaded))
            assert not set.intersection(*per_q) and len(set.union(*per_q)) == 2 * NS          # the quarters tile the two row blocks


def test_ring_of_two_groups():
    """group g + 1's blocks land in the registers of group g - 1: issued only after that group's last step, in the order of need"""
    sched = load_schedule()
    for t, j, g, tap, rb in sched:
        if g >= 2:
            assert t >= 4 * (g - 1)
    for g in range(NG):
        order = [tap for t, j, gg, tap, rb in sorted(sched) if gg == g and rb == 0]
        assert order == [0, 2, 1]
    burst = [s for s in sched if s[0] == -1]
    assert [(g, tap) for _, _, g, tap, _ in burst] == [(0, 0), (0, 0)]       # only group 0's g0 pair before the walk
    # no step issues more weight loads than before (4 in step 0, 2 elsewhere), and the last group issues none
    per_step = {}
    for t, *_ in sched:
        per_step[t] = per_step.get(t, 0) + 1
    assert per_step[0] == 4 and all(n == 2 for t, n in per_step.items() if t != 0) and max(per_step) < 4 * (NG - 1)


def _pack(w):
    """[2C, C, 3] -> [row block][chunk][tap][k16][16 rows][16 channels], the order of the packed matrix"""
    r, c, _ = w.shape
    return w.reshape(r // 16, 16, c // 64, 4, 16, 3).transpose(0, 2, 5, 3, 1, 4).copy()


def _form32(g0, g1, g2):
    s = g0 + g2
    return np.float32(0.5) * (s + g1), np.float32(0.5) * (s - g1)


def _input_transform(x, dil):
    """x [C, T] -> D [4][C, pairs], the pairs' first frames f, for whole 32-frame tiles (zero outside [0, T) before the differences)"""
    cin, t_len = x.shape
    tiles = (t_len + 31) // 32
    xp = np.zeros((cin, 32 * tiles + 32), x.dtype)
    xp[:, 8:8 + t_len] = x
    p = np.arange(16)
    f = np.concatenate([32 * tile + p + dil * (p // dil) for tile in range(tiles)])
    xm, x0, x1, x2 = (xp[:, f + 8 + s * dil] for s in (-1, 0, 1, 2))
    return [xm - x1, x0 + x1, x1 - x0, x0 - x2], f, tiles


def _output_transform(m, f, dil, tiles, t_len):
    y = np.zeros((m[0].shape[0], 32 * tiles + 8), m[0].dtype)
    y[:, f] = m[1] + (m[2] + m[0])
    y[:, f + dil] = m[1] - (m[2] + m[3])
    return y[:, :t_len]


@pytest.mark.parametrize("dil", [1, 8])
def test_walk_on_the_packed_matrix(dil):
    rng = np.random.default_rng(7 + dil)
    rows, cin, t_len = 64, 256, 70
    w = (rng.standard_normal((rows, cin, 3)) / np.sqrt(3 * cin)).astype(np.float32)
    x = rng.standard_normal((cin, t_len)).astype(np.float32)
    flat = _pack(w).reshape(-1, 16, 16)                           # blocks in packed order
    D, f, tiles = _input_transform(x.astype(np.float64), dil)
    m = [np.zeros((rows, len(f))) for _ in range(4)]
    for rblk in range(rows // 16):                                # (mtile, wr, rb) flattened: a 16-row block
        for kq in range(NCH):
            ring = {}
            sched = load_schedule()
            formed = None
            for t in range(NQ):
                for ts, j, g, tap, rb in sched:                   # loads issued before step t have landed (rb: both alike here)
                    if ts < t and rb == 0:
                        ring[(g % 2, tap)] = flat[rblk * NS + 12 * kq + tap * 4 + g].astype(np.float64)
                _, k16, prod = step_map(t)
                gp = (t // 4) % 2
                if t % 4 == 1:
                    s = ring[(gp, 0)] + ring[(gp, 2)]
                    formed = (s + ring[(gp, 1)], s - ring[(gp, 1)])           # 2 G1, 2 G2
                a = ring[(gp, 0)] if prod == 0 else ring[(gp, 2)] if prod == 3 else formed[prod - 1]
                ch = slice(64 * kq + 16 * k16, 64 * kq + 16 * k16 + 16)
                m[prod][16 * rblk:16 * rblk + 16] += a @ D[prod][ch]
    got = _output_transform([m[0], 0.5 * m[1], 0.5 * m[2], m[3]], f, dil, tiles, t_len)
    xp = np.zeros((cin, t_len + 2 * dil))
    xp[:, dil:dil + t_len] = x
    want = sum(w[:, :, k].astype(np.float64) @ xp[:, k * dil:k * dil + t_len] for k in range(3))
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_forming_in_fp32_matches_forming_in_double(seed):
    """One layer (C = 256, d = 4, 1024 frames), fp32 products and sums: G1, G2 formed in fp32 from the fp32 taps against the
    double-formed, once-rounded ones.  Measured, max |y - y64| / max |y64| over the three seeds: double-formed 5.7e-7 .. 6.9e-7,
    fp32-formed 5.7e-7 .. 7.2e-7.  Bound: twice the double-formed variant's own error - forming adds at most two roundings of 2^-24 relative to an
    operand whose product already carries the fp32 sum's error over K = 256."""
    rng = np.random.default_rng(seed)
    c, dil, t_len = 256, 4, 1024
    w = (rng.standard_normal((2 * c, c, 3)) / np.sqrt(3 * c)).astype(np.float32)
    x = rng.standard_normal((c, t_len)).astype(np.float32)
    g0, g1, g2 = (np.ascontiguousarray(w[:, :, k]) for k in range(3))
    d0, d1, d2 = (g.astype(np.float64) for g in (g0, g1, g2))
    G_double = [g0, (0.5 * (d0 + d1 + d2)).astype(np.float32), (0.5 * (d0 - d1 + d2)).astype(np.float32), g2]
    f1, f2 = _form32(g0, g1, g2)
    assert f1.dtype == np.float32 and f2.dtype == np.float32
    G_fp32 = [g0, f1, f2, g2]
    D, f, tiles = _input_transform(x, dil)
    xp = np.zeros((c, t_len + 2 * dil))
    xp[:, dil:dil + t_len] = x
    want = sum(w[:, :, k].astype(np.float64) @ xp[:, k * dil:k * dil + t_len] for k in range(3))
    err = {}
    for name, G in (("double", G_double), ("fp32", G_fp32)):
        m = [np.matmul(Gi, Di) for Gi, Di in zip(G, D)]
        assert all(mi.dtype == np.float32 for mi in m)
        y = _output_transform(m, f, dil, tiles, t_len)
        err[name] = float(np.abs(y.astype(np.float64) - want).max() / np.abs(want).max())
    # as the kernel carries them: 2 G1, 2 G2 through the products, halved in the output transform - the same bits
    s32 = g0 + g2
    m2x = [np.matmul(Gi, Di) for Gi, Di in zip([g0, s32 + g1, s32 - g1, g2], D)]
    y2x = _output_transform([m2x[0], np.float32(0.5) * m2x[1], np.float32(0.5) * m2x[2], m2x[3]], f, dil, tiles, t_len)
    assert y2x.dtype == np.float32 and np.array_equal(y2x, y)
    print(f"seed {seed}: double-formed {err['double']:.3e}, fp32-formed {err['fp32']:.3e}")
    assert err["fp32"] <= 2 * err["double"], err
    # the operands themselves: within one unit in the last place of each other
    for a, b in ((f1, G_double[1]), (f2, G_double[2])):
        assert np.abs(a.astype(np.float64) - b).max() <= 2.0 ** -23 * np.abs(b).max()
