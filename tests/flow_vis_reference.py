"""Two independent restatements of the flow visualisation (ofdg_flow_vis, include/ofdg.h), shared by tests/test_flow_vis.py
and tests/test_gpu_flow_vis.py: flow_vis() is the integer definition in numpy - no ctypes, the two tables rebuilt from their
formulas with math.atan -, middlebury() the published float algorithm (Baker et al.: atan2(-v, -u) / pi, floor(255 col)) in
float64.  Also the test flows, maps and sizes."""
import math

import numpy as np

N = 4
ALL_UNUSABLE, ALL_ZERO = 1, 2   # samples of flows(): every pixel unusable; every pixel exactly zero
FIXED_ENDS = (2.0 ** -8, 2.0 ** 20)   # both ends of max_flow: M = 1 and M = 2^28
SIZES = [(8, 2), (24, 6), (72, 40), (264, 200)]
ROW = np.dtype([("max_r2_q16", "<u8"), ("scale_q8", "<u4"), ("reserved", "<u4")])
SEGMENTS = (("RY", 15), ("YG", 6), ("GC", 4), ("CB", 11), ("BM", 13), ("MR", 6))
KNOWN = {(8, 0): (255, 0, 0), (0, 8): (255, 229, 0), (-8, 0): (0, 209, 255), (0, -8): (88, 0, 255), (0, 0): (255, 255, 255),
         (8, 8): (191, 86, 0), (-8, 8): (24, 191, 0)}   # max_flow = 8, as (R, G, B)


def atan_table():
    """A[k] = lrint(atan(k / 256) / (2 pi) * 2^24), k = 0..256"""
    return np.array([int(round(math.atan(k / 256.0) / (2.0 * math.pi) * 2.0 ** 24)) for k in range(257)], np.int64)


def wheel_table():
    """the 55 entries (R, G, B) of Baker et al."""
    rows = []
    for name, count in SEGMENTS:
        for i in range(count):
            up, down = 255 * i // count, 255 - 255 * i // count
            rows.append({"RY": (255, up, 0), "YG": (down, 255, 0), "GC": (0, 255, up), "CB": (0, down, 255), "BM": (up, 0, 255), "MR": (255, 0, down)}[name])
    return np.array(rows, np.int64)


_isqrt = np.frompyfunc(math.isqrt, 1, 1)


def isqrt(x):
    return _isqrt(np.asarray(x, np.int64).astype(object)).astype(np.int64)


def fixed(flow):
    """(usable, U, V): rule 1 and the Q8 components of step 2 (0 where unusable) of a [n,2,H,W] flow"""
    u, v = flow[:, 0].astype(np.float32), flow[:, 1].astype(np.float32)
    with np.errstate(invalid="ignore"):
        usable = (np.abs(u) < np.float32(1048576.0)) & (np.abs(v) < np.float32(1048576.0))
    U = np.rint(np.where(usable, u, 0).astype(np.float32) * np.float32(256.0)).astype(np.int64)
    V = np.rint(np.where(usable, v, 0).astype(np.float32) * np.float32(256.0)).astype(np.int64)
    return usable, U, V


def flow_vis(flow, occ=None, norm="sample", max_flow=None, layout="planar_bgr", dim_occ=False):
    """(picture, rows) by sections 1 to 8 of the definition"""
    A, wheel = atan_table(), wheel_table()
    flow = np.asarray(flow)
    n, _, H, W = flow.shape
    usable, U, V = fixed(flow)
    R2 = U * U + V * V
    Rq = isqrt(R2)
    rows = np.zeros(n, ROW)
    if norm == "fixed":
        M = np.full(n, int(np.rint(np.float32(max_flow) * np.float32(256.0))), np.int64)
    else:
        top = np.where(usable, R2, 0).reshape(n, -1).max(axis=1)
        if norm == "batch":
            top[:] = top.max()
        M = np.maximum(1, isqrt(top))
        rows["max_r2_q16"] = top
    rows["scale_q8"] = M
    rho = np.minimum((Rq << 16) // M[:, None, None], 65537)
    ax, ay = np.abs(U), np.abs(V)
    mx, mn = np.maximum(ax, ay), np.minimum(ax, ay)
    t = np.where(mx > 0, (mn << 16) // np.maximum(mx, 1), 0)
    i, fr = t >> 8, t & 255
    a24 = A[i] + (((A[np.minimum(i + 1, 256)] - A[i]) * fr + 128) >> 8)
    o = (a24 + 128) >> 8
    b = np.where(ax >= ay, o, 16384 - o)
    b = np.where(U < 0, 32768 - b, b)
    b = np.where(V < 0, (65536 - b) & 65535, b)
    fk = b * 54
    k0, f = fk >> 16, fk & 65535
    rgb = np.zeros((n, H, W, 3), np.int64)
    for c in range(3):
        c16 = wheel[k0, c] * (65536 - f) + wheel[k0 + 1, c] * f
        inside = ((16711680 << 16) - rho * (16711680 - c16)) >> 32
        rgb[..., c] = np.where(rho <= 65536, inside, (3 * c16) >> 18)
    if dim_occ:
        with np.errstate(invalid="ignore"):
            hidden = np.asarray(occ)[:, 0] != 0
        rgb = np.where(hidden[..., None], rgb >> 1, rgb)
    rgb = np.where(usable[..., None], rgb, 0).astype(np.uint8)
    if layout == "hwc_rgb":
        return np.ascontiguousarray(rgb), rows
    return np.ascontiguousarray(rgb[..., ::-1].transpose(0, 3, 1, 2)), rows


def middlebury(u, v, max_flow):
    """The published algorithm in float64 on arrays u, v: (R, G, B uint8 [..., 3], radius, turn fraction of the angle)"""
    wheel = wheel_table().astype(np.float64)
    u, v = np.asarray(u, np.float64) / max_flow, np.asarray(v, np.float64) / max_flow
    rad = np.sqrt(u * u + v * v)
    a = np.arctan2(-v, -u) / np.pi
    fk = (a + 1.0) / 2.0 * 54.0
    k0 = np.floor(fk).astype(np.int64)
    k1 = np.where(k0 + 1 == 55, 0, k0 + 1)
    f = fk - k0
    out = np.zeros(u.shape + (3,), np.uint8)
    for c in range(3):
        col = (1.0 - f) * wheel[k0, c] / 255.0 + f * wheel[k1, c] / 255.0
        col = np.where(rad <= 1.0, 1.0 - rad * (1.0 - col), col * 0.75)
        out[..., c] = np.floor(255.0 * col).astype(np.uint8)
    return out, rad, (a + 1.0) / 2.0


def flows(W, H, dtype, n=N):
    """Test flows [n,2,H,W]: sample 0 random with exact zeros, axis-aligned and diagonal vectors of all eight octants, NaN, +-inf,
    +-2^20, the largest usable value and - as binary16 - an overflowed half; sample 1 all unusable (M = 1, black); sample 2 all
    zero (usable, the maximum 0: M = 1, white); the last zero but for one large vector in its last pixel."""
    rng = np.random.RandomState(W * 1000 + H)
    f = np.zeros((n, 2, H, W), np.float32)
    f[0] = (rng.uniform(-1.0, 1.0, (2, H, W)) * rng.choice([0.01, 1.0, 30.0, 700.0], (1, H, W))).astype(np.float32)
    big = np.float32(1048576.0)
    special = [(0, 0), (3, 0), (-3, 0), (0, 3), (0, -3), (2, 2), (-2, 2), (2, -2), (-2, -2), (5, 1), (1, 5), (-1, 5), (-5, 1), (-5, -1), (-1, -5), (1, -5), (5, -1),
               (np.nan, 1), (1, np.nan), (np.inf, 0), (0, -np.inf), (big, 0), (0, -big), (np.nextafter(big, np.float32(0)), 0),
               (-np.nextafter(big, np.float32(0)), np.nextafter(big, np.float32(0))), (70000.0, 1.0), (0.001953125, -0.001953125), (0.5 / 256, 1.5 / 256),
               (-0.0, 8.0), (8.0, -0.0), (1e-30, -1e-30)]
    flat = f[0].reshape(2, -1)
    for k, (u, v) in enumerate(special[:flat.shape[1]]):
        flat[0, k], flat[1, k] = u, v
    f[1, 0], f[1, 1] = np.nan, np.inf
    f[1, 1, ::2] = -big
    f[n - 1, 0, -1, -1], f[n - 1, 1, -1, -1] = -900.0, 40.0
    with np.errstate(over="ignore"):
        return f.astype(dtype)   # (binary16: 70000 and 2^20 overflow to inf, 900 stays)


def occ_map(W, H, dtype, n=N):
    """[n,1,H,W] maps with zeros, ones, other non-zero values and - as float32 - NaN and -0.0"""
    rng = np.random.RandomState(7 * W + H)
    o = (rng.randint(0, 3, (n, 1, H, W)) * rng.randint(0, 2, (n, 1, H, W))).astype(dtype)
    if np.dtype(dtype) == np.float32:
        o[0, 0, 0, 0], o[0, 0, 0, 1], o[0, 0, 0, 2] = np.nan, -0.0, 1e-30
    else:
        o[0, 0, 0, 0], o[0, 0, 0, 1] = 255, 0
    return o


def cases():
    """(norm, max_flow) x layout x dimming of the matrix both test files walk"""
    for norm, max_flow in (("fixed", 8.0), ("sample", None), ("batch", None)):
        for layout in ("planar_bgr", "hwc_rgb"):
            for dim in (None, "uint8", "float32"):
                yield norm, max_flow, layout, dim


def equal_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
