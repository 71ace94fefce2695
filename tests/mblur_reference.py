"""The definition of motion blur (ofdg_motion_blur, include/ofdg.h) restated in numpy from the header text: float32 arrays whose
every operation is one IEEE rounding (numpy fuses nothing) up to the half-displacement and the step, int64 arrays behind
them, Philox4x32-10 on uint64 arrays.  u(w), sym(w, a) and the byte of a float32 element are ofdg_photo's, so they are taken
from its restatement (tests/photo_reference.py).  No GPU, no library call."""
import functools

import numpy as np

import photo_reference as pr

F32 = np.float32
RANGES = ("prob", "shutter_min", "shutter_max", "pair_shutter")
MAX_SHUTTER, MAX_D, MAX_TAPS_SIDE = 2.0, 8192, 16
SIZES = [(8, 2), (24, 6), (72, 40), (264, 200)]  # W, H
FORMATS = [(s, d, f) for s in ("float32", "uint8") for d in ("float32", "uint8") for f in ("float32", "float16")]
N = 3
expect_equal, equal_bits = pr.expect_equal, pr.equal_bits

# the grid: every format at every size under the widest cap; the narrower caps where a case costs least
GRID = [(W, H, s, d, f, 16) for (W, H) in SIZES for (s, d, f) in FORMATS] + \
       [(W, H, s, d, f, t) for (W, H) in SIZES[:3] for (s, d, f) in (FORMATS[0], FORMATS[7], FORMATS[2]) for t in (1, 4)] + \
       [(264, 200, "uint8", "uint8", "float16", 4), (264, 200, "float32", "float32", "float32", 1)]
KNOWN = [  # (u, v), shutter, taps_side -> {(x, y): byte}, every other pixel 0
    ((4, 0), 1.0, 16, {(x, 3): 51 for x in range(8, 13)}),
    ((1, 0), 1.0, 16, {(9, 3): 42, (10, 3): 170, (11, 3): 42}),
    ((0, 3), 1.0, 16, {(10, 1): 25, (10, 2): 64, (10, 3): 77, (10, 4): 64, (10, 5): 25}),
    ((4, 4), 0.5, 16, {(9, 2): 85, (10, 3): 85, (11, 4): 85}),
    ((40, 0), 1.0, 4, {(x, 3): 28 for x in (0, 5, 10, 15, 20)}),
    ((-4, 0), 1.0, 16, {(x, 3): 51 for x in range(8, 13)}),  # the sign of the flow does not matter
]


# ---- 1. draw ---------------------------------------------------------------------------------------------------------------
def draw(seed, index, ranges=None):
    """the record float32 [4] of global sample `index`, not sanitised"""
    q = {k: F32((ranges or {}).get(k, 0.0)) for k in RANGES}
    w = [int(v) for v in pr.philox([0], 0, 0x0C76, 0, pr.key_of(seed, index))[0]]
    on = pr.unit(w[0]) < q["prob"]
    s0 = F32(q["shutter_min"] + F32(F32(q["shutter_max"] - q["shutter_min"]) * pr.unit(w[1])))
    s1 = F32(s0 + pr.sym(w[2], q["pair_shutter"]))
    return np.array([s0, s1, 0, 0] if on else [0, 0, 0, 0], np.float32)


def drawn_records(seed, first_index, n, ranges=None):
    return np.stack([draw(seed, first_index + i, ranges) for i in range(n)])


# ---- 2. sanitise -----------------------------------------------------------------------------------------------------------
def sanitise(recs):
    out = np.zeros((len(recs), 4), np.float32)
    for i, r in enumerate(np.asarray(recs, np.float32).reshape(-1, 4)):
        for f in range(2):
            s = r[f]
            out[i, f] = F32(0.0) if (np.isnan(s) or s <= 0) else F32(MAX_SHUTTER) if s > MAX_SHUTTER else s
    return out


# ---- 3. pixels -------------------------------------------------------------------------------------------------------------
def half_displacement(flow, s):
    """(Dx, Dy) int64 [H,W] of a flow [2,H,W] (float32 or float16) under the sanitised shutter s"""
    u, v = flow[0].astype(np.float32), flow[1].astype(np.float32)
    finite = np.isfinite(u) & np.isfinite(v)
    out = []
    for d in (u, v):
        with np.errstate(over="ignore", invalid="ignore"):
            a = (d * F32(s)).astype(np.float32)
            h = (a * F32(128.0)).astype(np.float32)
            h = np.where(finite, h, F32(0.0)).astype(np.float32)
            h = np.minimum(np.maximum(h, F32(-MAX_D)), F32(MAX_D))
        out.append(np.rint(h).astype(np.int64))
    return out


def taps(Dx, Dy, taps_side):
    """(m, sx, sy) int64 of half-displacements"""
    L = np.maximum(np.abs(Dx), np.abs(Dy))
    m = np.minimum(taps_side, (L + 255) >> 8)
    div = np.where(m > 0, m, 1).astype(np.float32)
    sx = np.rint((Dx.astype(np.float32) / div).astype(np.float32)).astype(np.int64)
    sy = np.rint((Dy.astype(np.float32) / div).astype(np.float32)).astype(np.int64)
    return m, np.where(m > 0, sx, 0), np.where(m > 0, sy, 0)


def blur_frame(img, flow, s, taps_side, stats=None):
    """the bytes int64 [3,H,W] of one frame [3,H,W] (uint8 or float32) along its flow [2,H,W] under the sanitised shutter s"""
    _, H, W = img.shape
    B = pr.index_of(img)
    Dx, Dy = half_displacement(flow, s)
    m, sx, sy = taps(Dx, Dy, taps_side)
    if stats is not None:
        stats.append((2 * m + 1).mean())
    w = 65536 // (2 * m + 1)
    centre = 65536 - 2 * m * w
    y, x = np.mgrid[0:H, 0:W]
    S = np.zeros((3, H, W), np.int64)
    for k in range(-int(m.max()), int(m.max()) + 1):
        Qx = np.clip(256 * x + k * sx, 0, 256 * (W - 1))
        Qy = np.clip(256 * y + k * sy, 0, 256 * (H - 1))
        ix, fx, iy, fy = Qx >> 8, Qx & 255, Qy >> 8, Qy & 255
        x0, x1, y0, y1 = np.clip(ix, 0, W - 1), np.clip(ix + 1, 0, W - 1), np.clip(iy, 0, H - 1), np.clip(iy + 1, 0, H - 1)
        T = (256 - fx) * (256 - fy) * B[:, y0, x0] + fx * (256 - fy) * B[:, y0, x1] + (256 - fx) * fy * B[:, y1, x0] + fx * fy * B[:, y1, x1]
        t = (T + 128) >> 8
        S += np.where(np.abs(k) <= m, (centre if k == 0 else w) * t, 0)
    assert S.max() < 2 ** 32 - 2 ** 23
    return (S + 2 ** 23) >> 24


def motion_blur(images, flow, recs, taps_side=8, dst_dtype=None, stats=None):
    """((out0, out1), sanitised records) of the frames images = (image0, image1), each [n,3,H,W] uint8 / float32 or None, along
    flow = (flow, flow1), each [n,2,H,W] float32 / float16 or None, under the records recs float32 [n,4]."""
    given = [t for t in images if t is not None]
    n = given[0].shape[0]
    dt = np.dtype(given[0].dtype if dst_dtype is None else dst_dtype)
    used = sanitise(recs)
    out = [None if t is None else np.zeros(t.shape, dt) for t in images]
    for f in range(2):
        if images[f] is None:
            continue
        for i in range(n):
            out[f][i] = blur_frame(images[f][i], flow[f][i], used[i][f], taps_side, stats).astype(dt)
    return tuple(out), used


# ---- test data -------------------------------------------------------------------------------------------------------------
def records():
    """N = 3 records: shutter 0, 0.5, and 2 with another shutter in frame 1"""
    return np.array([[0, 0, 0, 0], [0.5, 0.5, 0, 0], [2.0, 1.25, 0, 0]], np.float32)


def frames(W, H, dtype="uint8", n=N, seed=1):
    """(image0, image1) [n,3,H,W]: photo_reference's - every byte value; float32 with fractions, NaN, -3, 255.5, 1e9, infinities"""
    return pr.frames(W, H, dtype, n=n, seed=seed)


# (u, v) of the blocks, px: still, sub-pixel parts, ties of rintf at shutter 0.5 / 1.25 / 2, beyond the 32 px clamp on one axis
# and on both, beyond the tap cap, the smallest displacement that counts (0.004 at shutter 1; here through 0.0079 / 0.0078)
_VECTORS = [(0.0, 0.0), (4.25, 0.0), (-3.5, 2.75), (0.0, -7.125), (40.5, 0.3), (-70.0, 65.0), (0.0079, 0.0), (1.0, 1.0), (-12.3, -9.9),
            (33.0, -0.5), (2.5, -2.5), (0.0, 0.0078), (15.99, 16.01), (-0.00390625, 0.01171875), (100.0, -100.0), (0.5, 18.75), (-1.0, 0.0)]
_SPECIAL = [np.nan, np.inf, -np.inf, -0.0, 1e-40, -1e-40, 65504.0, -65504.0]
# the gentle set: no |u|, |v| above 15.5 px, so that under every shutter up to 2 every tap stays within 16 px of its pixel
# (D <= 3968, m |step| <= 3968 + m / 2 <= 4096) - sub-pixel parts, ties, both diagonals, the cap of 16 taps reached
_GENTLE = [(0.0, 0.0), (4.25, 0.0), (-3.5, 2.75), (0.0, -7.125), (15.5, 0.3), (-15.5, 15.5), (0.0079, 0.0), (1.0, 1.0), (-12.3, -9.9),
           (9.0, -0.5), (2.5, -2.5), (0.0, 0.0078), (7.99, 8.01), (-0.00390625, 0.01171875), (15.25, -15.25), (0.5, 13.75), (-1.0, 0.0)]
_PLANTS = {False: [(-20.5, -11.0), (31.0, -31.0), (-9.25, 9.25), (64.0, 64.0)], True: [(-10.5, -11.0), (15.0, -15.0), (-9.25, 9.25), (15.5, 15.5)]}


def flows(W, H, dtype="float32", n=N, seed=2, special=True, gentle=False):
    """(flow, flow1) [n,2,H,W]: piecewise-constant blocks of _VECTORS, another assignment per sample and frame; outward streaks
    at the four corners and along the four borders; at 264x200 the three streaks of a 64 x 16 tiling - across the tile corner at
    (64, 16), 50 px long around (100, 100), and a far one whose taps but the centre all lie 20 px and more away -; in
    samples 1 and 2 a special value at every 7th element but those (special=False: none - the +-65504 among them put a streak
    beyond every halo into every tile).  gentle=True: blocks of _GENTLE and corner streaks of at most 15.5 px, no special values
    and none of the three long streaks, so that no tap of any sample lies further than 16 px from its pixel - the set under
    which a tile stages its window also where the plane is smaller than the window (8x2, 24x6)."""
    table, special = (_GENTLE if gentle else _VECTORS), special and not gentle
    bw, bh = max(2, W // 6), max(1, H // 5)
    y, x = np.mgrid[0:H, 0:W]
    out = []
    for f in range(2):
        a = np.zeros((n, 2, H, W), np.float32)
        for i in range(n):
            idx = ((y // bh) * ((W + bw - 1) // bw) + x // bw + 5 * i + 3 * f + seed) % len(table)
            vec = np.array(table, np.float32)
            a[i, 0], a[i, 1] = vec[idx, 0], vec[idx, 1]
            if i > 0 and special:  # (the streaks planted below win over these)
                flat = a[i].reshape(-1)
                at = np.arange(3 + i, flat.size, 7)
                flat[at] = np.array(_SPECIAL, np.float32)[(np.arange(at.size) + i) % len(_SPECIAL)]
            c = max(1, min(3, W // 8, H // 2))
            corners = [np.array(v, np.float32)[:, None, None] for v in _PLANTS[bool(gentle)]]
            a[i, :, :c, :c], a[i, :, :c, -c:], a[i, :, -c:, :c], a[i, :, -c:, -c:] = corners
            a[i, :, H // 2, :1] = np.array([-6.0, 0.25], np.float32)[:, None]
            a[i, :, H // 2, -1:] = np.array([6.0, -0.25], np.float32)[:, None]
            a[i, :, :1, W // 2] = np.array([0.25, -6.0], np.float32)[:, None]
            a[i, :, -1:, W // 2] = np.array([-0.25, 6.0], np.float32)[:, None]
            if W >= 264 and H >= 200 and not gentle:
                a[i, :, 14:18, 62:66] = np.array([10.0, 10.0], np.float32)[:, None, None]
                a[i, :, 98:102, 98:102] = np.array([25.0, -3.0], np.float32)[:, None, None]
                a[i, :, 150:152, 200:202] = np.array([32.0, 32.0], np.float32)[:, None, None]
        with np.errstate(over="ignore"):
            out.append(a.astype(dtype))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def case(W, H, src_dtype, flow_dtype, taps_side, special=True, gentle=False):
    """(images, flows, records, {dst dtype: (out0, out1)}, sanitised records) of one cell of the grid, computed once; read only"""
    images, fl, recs = frames(W, H, src_dtype), flows(W, H, flow_dtype, special=special, gentle=gentle), records()
    want, used = motion_blur(images, fl, recs, taps_side, dst_dtype="float32")
    for t in images + fl + want + (recs, used):
        t.setflags(write=False)
    return images, fl, recs, {"float32": want, "uint8": tuple(t.astype(np.uint8) for t in want)}, used


def tile_paths(flow, s, taps_side, tile_w=64, tile_h=16, halo=16):
    """the path of every tile_w x tile_h tile of one sample's flow [2,H,W] under the sanitised shutter s, as the kernel chooses it
    (csrc/kernels.hip): "copy" - no pixel has a tap beside its centre -, "window" - m |step| <= 256 * halo on both axes for every
    pixel -, else "gather"; a list in tile order"""
    Dx, Dy = half_displacement(flow, s)
    m, sx, sy = taps(Dx, Dy, taps_side)
    far = (m * np.abs(sx) > 256 * halo) | (m * np.abs(sy) > 256 * halo)
    H, W = m.shape
    return ["gather" if far[y0:y0 + tile_h, x0:x0 + tile_w].any() else "window" if m[y0:y0 + tile_h, x0:x0 + tile_w].any() else "copy"
            for y0 in range(0, H, tile_h) for x0 in range(0, W, tile_w)]


def impulse(u, v, shutter, taps_side=16, W=24, H=6, at=(10, 3)):
    """the known-answer setup: (image uint8 [1,3,H,W] with one 255, flow float32 [1,2,H,W] constant, record [1,4])"""
    img = np.zeros((1, 3, H, W), np.uint8)
    img[:, :, at[1], at[0]] = 255
    fl = np.zeros((1, 2, H, W), np.float32)
    fl[:, 0], fl[:, 1] = u, v
    return img, fl, np.array([[shutter, shutter, 0, 0]], np.float32)
