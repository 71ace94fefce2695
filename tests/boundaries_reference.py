"""numpy restatement of ofdg_boundaries (include/ofdg.h), written from the header text alone: what the CPU and GPU tests compare
ofdg_host_boundaries and the device with, byte for byte.  Every float32 operation is rounded through np.float32 on its own; the
distance is the brute-force minimum over the offsets of the disc.  Also the inputs both test files use."""
import functools

import numpy as np

F32, F16 = 0, 2                      # OFDG_FMT_F32, OFDG_FMT_F16
LABELS, MAX_RADIUS, FAR = 1, 15, 255  # OFDG_BND_LABELS, OFDG_BND_MAX_RADIUS, OFDG_BND_FAR
N = 3
SIZES = ((8, 2), (24, 6), (72, 40), (264, 200))  # (W, H)
RADII = (1, 4, 15)
MIN_STEPS = (0.0, 0.5, 3.0)
DTYPE = {F32: np.float32, F16: np.float16}


def _pair_step(up, vp, uq, vq, t2):
    """d2 > t2 of the header: du, dv, the two squares and their sum each rounded to float32; a NaN compares false"""
    with np.errstate(all="ignore"):
        du = np.subtract(up, uq, dtype=np.float32)
        dv = np.subtract(vp, vq, dtype=np.float32)
        a = np.multiply(du, du, dtype=np.float32)
        b = np.multiply(dv, dv, dtype=np.float32)
        d2 = np.add(a, b, dtype=np.float32)
        return d2 > t2


def edge_of(flow, label, min_step, labels):
    """edge uint8 [n,1,H,W] of flow [n,2,H,W] (float32 or float16) and label uint8 [n,H,W] (read with labels only)"""
    f = flow.astype(np.float32)  # (exact for binary16)
    u, v = f[:, 0], f[:, 1]
    t2 = np.float32(np.float32(min_step) * np.float32(min_step))
    edge = np.zeros(u.shape, bool)
    right = _pair_step(u[:, :, :-1], v[:, :, :-1], u[:, :, 1:], v[:, :, 1:], t2)
    down = _pair_step(u[:, :-1, :], v[:, :-1, :], u[:, 1:, :], v[:, 1:, :], t2)
    if labels:
        right &= label[:, :, :-1] != label[:, :, 1:]
        down &= label[:, :-1, :] != label[:, 1:, :]
    edge[:, :, :-1] |= right
    edge[:, :, 1:] |= right
    edge[:, :-1, :] |= down
    edge[:, 1:, :] |= down
    return edge.astype(np.uint8)[:, None]


def dist2_of(edge, radius):
    """dist2 uint8 [n,1,H,W] of edge [n,1,H,W]: for every offset (dx, dy) of the disc, the pixels whose neighbour at that offset
    is an edge pixel of the same plane take min(best, dx^2 + dy^2)"""
    n, _, H, W = edge.shape
    e = edge[:, 0] != 0
    best = np.full((n, H, W), FAR, np.uint8)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            d = dx * dx + dy * dy
            if d > radius * radius or abs(dy) >= H or abs(dx) >= W:
                continue
            # pixel (x, y) looks at (x + dx, y + dy): both inside the plane
            ys, yd = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))
            xs, xd = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
            view = best[:, yd, xd]
            np.minimum(view, np.where(e[:, ys, xs], np.uint8(d), np.uint8(FAR)), out=view)
    return best[:, None]


def _specials(dtype):
    tiny = [6e-8, -6e-8] if dtype == np.float16 else [1e-45, -1e-40, 6e-8]  # denormals of the format (and of binary16)
    return np.array([np.nan, np.inf, -np.inf, -0.0, 65504.0, -65504.0] + tiny, dtype)


def _frame(rng, W, H, dtype):
    """Piecewise-constant random blocks with matching labels; spikes; special values."""
    bw, bh = int(rng.integers(3, 12)), int(rng.integers(2, 9))
    gx, gy = (W + bw - 1) // bw, (H + bh - 1) // bh
    flow = np.zeros((N, 2, H, W), np.float32)
    label = np.zeros((N, H, W), np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for i in range(N):
        block = (yy // bh) * gx + (xx // bw)
        ids = rng.integers(1, 7, gx * gy).astype(np.uint8)           # few labels: neighbouring blocks often share one
        motions = rng.integers(-3, 4, (7, 2)).astype(np.float32) * 0.75  # a motion per label: multiples of 0.75 in [-2.25, 2.25]
        motions[5] = motions[4]                                     # two labels that move identically
        label[i] = ids[block]
        flow[i] = np.moveaxis(motions[label[i]], -1, 0)
        inner = rng.integers(0, 2, gx * gy).astype(bool)[block] & (xx % bw >= bw // 2)
        flow[i, 0][inner] += 1.5                                    # a flow step inside one label
    # one-pixel spikes: isolated ones, one at each corner and on each border
    spots = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 3), (H // 2, 0), (H // 3, W - 1)]
    spots += [(int(rng.integers(0, H)), int(rng.integers(0, W))) for _ in range(max(2, W * H // 400))]
    for k, (y, x) in enumerate(spots):
        flow[k % N, :, y, x] += (5.0, -2.5)
        if k % 2:
            label[k % N, y, x] = 9
    flow = flow.astype(dtype)
    sp = _specials(dtype)
    for i in (1, 2):  # sample 0 stays finite
        flat = flow[i].reshape(-1)
        at = np.arange(i, flat.size, 7)
        flat[at] = sp[(np.arange(at.size) + i) % sp.size]
    return flow, label


@functools.lru_cache(maxsize=None)
def inputs(W, H, fmt):
    """dict(flow, label, flow1, label1) of N samples; treat as read-only"""
    rng = np.random.default_rng(1000 * W + 10 * H + fmt)
    flow, label = _frame(rng, W, H, DTYPE[fmt])
    flow1, label1 = _frame(rng, W, H, DTYPE[fmt])
    out = dict(flow=flow, label=label, flow1=flow1, label1=label1)
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected(W, H, fmt, labels, radius, min_step):
    """dict(edge0, dist0, edge1, dist1) of inputs(W, H, fmt)"""
    src = inputs(W, H, fmt)
    out = {}
    for f, (fk, lk) in enumerate((("flow", "label"), ("flow1", "label1"))):
        out["edge%d" % f] = edge_of(src[fk], src[lk], min_step, labels)
        out["dist%d" % f] = dist2_of(out["edge%d" % f], radius)
    for a in out.values():
        a.setflags(write=False)
    return out


def expect_equal(got, want, what=""):
    for key in want:
        if key not in got:
            continue
        g, w = np.asarray(got[key]), np.asarray(want[key])
        assert g.shape == w.shape and g.dtype == w.dtype, "%s %s: %s %s against %s %s" % (what, key, g.dtype, g.shape, w.dtype, w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            at = tuple(bad[0])
            raise AssertionError("%s %s: %d of %d differ, first at %s: got %d, want %d" % (what, key, len(bad), g.size, at, g[at], w[at]))
