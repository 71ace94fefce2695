"""The definition of the multi-scale flow pyramid (ofdg_flow_pyramid, include/ofdg.h) restated in numpy: float32 arrays,
reshaped to 2x2 blocks, the two additions in the stated order (numpy rounds every ufunc result to float32 and fuses nothing),
np.float32 division, astype(np.float16) for the binary16 output (to nearest even, an overflow becomes inf).  Shared by
tests/test_flow_pyramid.py and tests/test_gpu_flow_pyramid.py, which also take their planted tensors from here."""
import numpy as np

MAX_LEVELS = 6
SCALE = 1
LIMIT = np.float32(1048576.0)
BELOW_LIMIT = np.nextafter(LIMIT, np.float32(0))  # the largest float32 that is still usable
# the values planted in every sample-0 plane (float32; as float16 the limits overflow to inf and the denormals flush to 0)
SPECIALS = (np.nan, np.inf, -np.inf, LIMIT, -LIMIT, BELOW_LIMIT, -BELOW_LIMIT, -0.0, 65504.0, -65504.0, 65520.0, 1e-40, -1e-45,
            1.5 * 2.0 ** -126, 6e-8, 6.2e-5)


def max_levels(H, W):
    """The deepest pyramid H x W allows (6 at most)."""
    k = 0
    while k < MAX_LEVELS and H % (2 << k) == 0 and W % (2 << k) == 0:
        k += 1
    return k


def level0(flow, occ=None):
    """(S0 [n,2,H,W] float32, c0 [n,H,W] int64): unusable pixels as (+0, +0) with count 0."""
    f = flow.astype(np.float32)
    usable = (np.abs(f[:, 0]) < LIMIT) & (np.abs(f[:, 1]) < LIMIT)
    if occ is not None:
        usable &= occ[:, 0] == 0
    return np.where(usable[:, None], f, np.float32(0.0)), usable.astype(np.int64)


def blocks(a):
    """[..., h, w] -> the four children [..., h/2, w/2] of every 2x2 block: top left, top right, bottom left, bottom right."""
    h, w = a.shape[-2:]
    b = a.reshape(a.shape[:-2] + (h // 2, 2, w // 2, 2))
    return b[..., 0, :, 0], b[..., 0, :, 1], b[..., 1, :, 0], b[..., 1, :, 1]


def output(S, c, k, flags, out_dtype):
    """Level k's planes of its sums [n,2,h,w] and counts [n,h,w]."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        q = np.where(c[:, None] == 0, np.float32(0.0), S / c[:, None].astype(np.float32))
        assert q.dtype == np.float32
        if flags & SCALE:
            q = q * np.float32(2.0 ** -k)
        return q.astype(out_dtype)


def flow_pyramid(flow, levels, occ=None, flags=SCALE, out_dtype=None):
    """(the list of level arrays [n,2,H>>k,W>>k] of out_dtype, the list of weights [n,1,H>>k,W>>k] uint16), k = 1..levels."""
    out_dtype = flow.dtype if out_dtype is None else out_dtype
    S, c = level0(flow, occ)
    lv, wt = [], []
    for k in range(1, levels + 1):
        tl, tr, bl, br = blocks(S)
        S = (tl + tr) + (bl + br)  # the left-right pairs first, then top and bottom
        assert S.dtype == np.float32
        c = sum(blocks(c))
        lv.append(output(S, c, k, flags, out_dtype))
        wt.append(c[:, None].astype(np.uint16))
    return lv, wt


def running_sum_pyramid(flow, levels, occ=None, flags=SCALE, out_dtype=None):
    """The same with every cell summed pixel by pixel in row-major order instead: what a wrong tree would give."""
    out_dtype = flow.dtype if out_dtype is None else out_dtype
    S0, c0 = level0(flow, occ)
    n, _, H, W = S0.shape
    lv = []
    for k in range(1, levels + 1):
        e, h, w = 1 << k, H >> k, W >> k
        px = S0.reshape(n, 2, h, e, w, e).transpose(0, 1, 2, 4, 3, 5).reshape(n, 2, h, w, e * e)
        S = np.zeros((n, 2, h, w), np.float32)
        for j in range(e * e):
            S = S + px[..., j]
        c = c0.reshape(n, h, e, w, e).sum(axis=(2, 4))
        lv.append(output(S, c, k, flags, out_dtype))
    return lv


def assert_order_is_visible(flow, levels, occ=None):
    """A row-major running sum of this tensor differs from the definition in at least one cell of every level >= 2: without
    that a test on it could not tell a wrong summation tree from the right one."""
    want, _ = flow_pyramid(flow, levels, occ, SCALE, np.float32)
    other = running_sum_pyramid(flow, levels, occ, SCALE, np.float32)
    for k in range(2, levels + 1):
        assert want[k - 1].tobytes() != other[k - 1].tobytes(), "level %d of %s does not show the order of summation" % (k, flow.shape)


def planted(n, H, W, dtype=np.float32, seed=7, levels=None):
    """(flow [n,2,H,W] of dtype, occ bool [n,1,H,W]) with what the definition distinguishes planted.  Every sample: cells that mix
    values of about +-2^19 (+-2^14 for float16) with values of about 1e-3, so that the order of summation shows.  Sample 0:
    SPECIALS at random pixels of both planes (test_flow_pyramid.py checks that they meet every child position of every level),
    a 2x2 cell of float32 denormals whose mean and scaled mean are denormal, one around the binary16 subnormals, one around the
    binary16 overflow, one whole 4x4 block occluded.  Sample 1 % n: the first level-`levels` cell holds exactly one usable
    pixel.  Sample n - 1: the last level-`levels` cell holds none.  The map hides a fifth of the pixels besides."""
    levels = max_levels(H, W) if levels is None else levels
    rng = np.random.default_rng(seed)
    f = (rng.standard_normal((n, 2, H, W)) * 30.0).astype(np.float32)
    kind = rng.random((n, 2, H, W))
    big = np.float32(2.0 ** 14 if np.dtype(dtype) == np.float16 else 2.0 ** 19)
    f = np.where(kind < 0.3, (np.sign(f) * big * (1 + rng.random(f.shape))).astype(np.float32), f)
    f = np.where(kind > 0.7, (f * np.float32(1e-3 / 30)).astype(np.float32), f)
    occ = rng.random((n, 1, H, W)) < 0.2
    reps = max(1, min(6, H * W // 64))
    for j, value in enumerate(SPECIALS):
        for r in range(reps):
            y, x = int(rng.integers(H)), int(rng.integers(W))
            f[0, (j + r) % 2, y, x] = value
            occ[0, 0, y, x] = False
    f[0, 0, 2:4, 2:4] = [[1.5 * 2.0 ** -126, 2.0 ** -126], [1e-40, 3e-39]]
    f[0, 1, 2:4, 2:4] = [[-0.0, -0.0], [-0.0, -0.0]]
    f[0, 0, 2:4, 4:6] = [[3e-7, 5e-8], [1e-7, 7e-6]]
    f[0, 1, 2:4, 4:6] = [[6e-8, 6e-8], [6e-8, 2.9e-8]]
    f[0, 0, 2:4, 6:8] = [[65519.9, 65519.9], [65519.9, 65519.9]]
    f[0, 1, 2:4, 6:8] = [[65520.0, 65520.0], [65520.0, 65520.0]]
    occ[0, 0, 2:4, 2:8] = False
    occ[0, 0, 4:8, 4:8] = True
    e = 1 << levels
    one = 1 % n
    f[one, :, :e, :e] = np.where(rng.random((2, e, e)) < 0.5, np.nan, np.inf)
    f[one, :, e // 2, e - 1] = (3.0, -4.0)
    occ[one, 0, e // 2, e - 1] = False
    f[n - 1, 0, H - e:, W - e:] = np.nan
    f[n - 1, 1, H - e:, W - e:] = LIMIT
    with np.errstate(over="ignore", under="ignore"):  # (the limits become inf in a half: that is the point)
        out = f.astype(dtype)
    assert_order_is_visible(out, levels)
    assert_order_is_visible(out, levels, occ)
    return out, occ


def expect_equal(got, want, what=""):
    """Level for level, byte for byte; names the first cell that differs."""
    assert len(got) == len(want), (what, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want), 1):
        g = np.asarray(g)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            bits = {2: np.uint16, 4: np.uint32}[g.dtype.itemsize]
            at = np.argwhere(g.view(bits) != w.view(bits))
            i = tuple(at[0])
            raise AssertionError("%s level %d: %d cells differ, the first at %s: got %r, expected %r" % (what, k, len(at), i, g[i], w[i]))
