"""numpy restatement of the camera (ofdg_camera, include/ofdg.h) - written from the header's text alone: the draw, the
sanitising, the tap table, the two blur passes on bytes, the mosaic and its bilinear demosaic - and the planes and records the
tests share."""
import numpy as np

from erase_reference import equal_bits, expect_equal, key_of, philox  # noqa: F401  (the Philox block and the comparisons)

F32 = np.float32
REC = np.dtype([("sigma_q8", "<i4", (2,)), ("bayer", "<i4"), ("radius", "<i4", (2,)), ("reserved", "<i4", (3,))])
N = 4
SIZES = [(8, 2), (24, 6), (72, 40), (264, 200)]
MAX_SIGMA, MAX_RADIUS = 1024, 12
DEFAULT = dict(sigma_min=0.3, sigma_max=1.5, sigma_delta=0.1, blur_prob=0.8, bayer_prob=0.5, pattern=-1)
# the header's known answers: sigma_q8 -> w[0..R]
KNOWN_TAPS = {1: [65536, 0], 85: [64160, 688], 86: [64012, 762, 0], 256: [26152, 15862, 3539, 291],
              1024: [6548, 6346, 5778, 4942, 3971, 2998, 2126, 1416, 886, 521, 288, 149, 73]}


# ---- 1. draw ---------------------------------------------------------------------------------------------------------------
def q8(px):
    return int(np.rint(F32(px) * F32(256.0)))       # (float32 product, to nearest even)


def unit(w):
    return F32(int(w) >> 8) * F32(2.0 ** -24)


def isym(w, A):
    return ((int(w) * (2 * A + 1)) >> 32) - A


def draw(seed, index, ranges):
    b = philox(np.arange(2), 0, 0x0C79, 0, key_of(seed, index))
    lo, hi, D = q8(ranges.get("sigma_min", 0.0)), q8(ranges.get("sigma_max", 0.0)), q8(ranges.get("sigma_delta", 0.0))
    pattern = int(ranges.get("pattern", -1))
    blurred = unit(b[0, 0]) < F32(ranges.get("blur_prob", 0.0))
    s0 = lo + ((int(b[0, 1]) * (hi - lo + 1)) >> 32)
    s1 = s0 + isym(b[0, 2], D)
    mosaic = unit(b[0, 3]) < F32(ranges.get("bayer_prob", 0.0))
    p = pattern if pattern >= 0 else int(b[1, 0]) >> 30
    r = np.zeros((), REC)
    r["sigma_q8"] = (s0, s1) if blurred else (0, 0)
    r["bayer"] = p if mosaic else -1
    return r


def drawn_records(seed, first_index, n, ranges):
    return np.array([draw(seed, first_index + i, ranges) for i in range(n)], REC)


# ---- 2. sanitise -----------------------------------------------------------------------------------------------------------
def radius_of(s):
    return np.minimum(MAX_RADIUS, (3 * np.asarray(s, np.int64) + 255) >> 8)


def sanitise(recs):
    out = np.zeros(recs.shape, REC)
    out["sigma_q8"] = np.clip(recs["sigma_q8"], 0, MAX_SIGMA)
    out["bayer"] = np.where((recs["bayer"] < -1) | (recs["bayer"] > 3), -1, recs["bayer"])
    out["radius"] = radius_of(out["sigma_q8"])
    return out


# ---- 3. taps ---------------------------------------------------------------------------------------------------------------
def taps(s, exp=np.exp):
    """w[0..R] of sigma_q8 = s in 1..1024, as python ints"""
    R = int(radius_of(s))
    e = [int(np.rint(exp(-float(k * k) * 32768.0 / float(s * s)) * 16777216.0)) for k in range(R + 1)]
    E = e[0] + 2 * sum(e[1:])
    w = [0] + [(e[k] * 65536 + E // 2) // E for k in range(1, R + 1)]
    w[0] = 65536 - 2 * sum(w[1:])
    return w


def taps13(s):
    w = taps(s)
    return np.array(w + [0] * (MAX_RADIUS + 1 - len(w)), np.uint32)


# ---- 4. blur, on int64 planes of bytes [.., H, W] ---------------------------------------------------------------------------
def shifted(a, k, axis, mode):
    """a at the coordinate + k along axis, clamped ("edge") or reflected without repeating the edge ("reflect")"""
    n = a.shape[axis]
    at = np.arange(n) + k
    if mode == "edge":
        at = np.clip(at, 0, n - 1)
    else:
        at = np.where(at < 0, -at, np.where(at >= n, 2 * n - 2 - at, at))
    return np.take(a, at, axis=axis)


def blur(a, s):
    if s == 0:
        return a
    w = taps(s)
    R = len(w) - 1
    h8 = (sum(w[abs(k)] * shifted(a, k, -1, "edge") for k in range(-R, R + 1)) + 128) >> 8
    return (sum(w[abs(k)] * shifted(h8, k, -2, "edge") for k in range(-R, R + 1)) + 8388608) >> 24


def blur_float(a, s):
    """the float64 separable convolution with the same truncated, normalised Gaussian, the edge replicated"""
    R = int(radius_of(s))
    g = np.exp(-np.arange(-R, R + 1, dtype=np.float64) ** 2 * 32768.0 / float(s * s))
    g /= g.sum()
    a = a.astype(np.float64)
    h = sum(g[k + R] * shifted(a, k, -1, "edge") for k in range(-R, R + 1))
    return sum(g[k + R] * shifted(h, k, -2, "edge") for k in range(-R, R + 1))


# ---- 5. mosaic and demosaic, on (B, G, R) int64 planes [.., H, W] -----------------------------------------------------------
def demosaic(B, G, R, p):
    H, W = B.shape[-2:]
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    a, b = (x + (p & 1)) & 1, (y + (p >> 1)) & 1
    m = np.where((a == 0) & (b == 0), R, np.where((a == 1) & (b == 1), B, G))     # the one sample a site has
    nb = lambda dx, dy: shifted(shifted(m, dx, -1, "reflect"), dy, -2, "reflect")  # noqa: E731
    hz = (nb(-1, 0) + nb(1, 0) + 1) >> 1
    vt = (nb(0, -1) + nb(0, 1) + 1) >> 1
    cr = (nb(-1, 0) + nb(1, 0) + nb(0, -1) + nb(0, 1) + 2) >> 2
    dg = (nb(-1, -1) + nb(1, -1) + nb(-1, 1) + nb(1, 1) + 2) >> 2
    r_site, b_site, g_r_row = (a == 0) & (b == 0), (a == 1) & (b == 1), (a == 1) & (b == 0)
    oR = np.where(r_site, m, np.where(b_site, dg, np.where(g_r_row, hz, vt)))
    oG = np.where(r_site | b_site, cr, m)
    oB = np.where(r_site, dg, np.where(b_site, m, np.where(g_r_row, vt, hz)))
    return oB, oG, oR


def to_bytes(frame):
    """the bytes of a frame [.., H, W] of uint8 or float32, as int64"""
    if frame.dtype == np.uint8:
        return frame.astype(np.int64)
    v = frame.astype(F32)
    v = np.where(v > 0, v, F32(0))       # (a NaN becomes 0)
    v = np.where(v < 255, v, F32(255))
    return np.rint(v).astype(np.int64)


# ---- the whole call --------------------------------------------------------------------------------------------------------
def camera(src, recs=None, seed=0, first_index=0, ranges=None, dst_dtype=None):
    """((out0, out1), records used) as the call leaves them"""
    given = [t for t in src if t is not None]
    n = given[0].shape[0]
    dt = np.dtype(given[0].dtype if dst_dtype is None else dst_dtype)
    if recs is None:
        recs = drawn_records(seed, first_index, n, ranges or {})
    used = sanitise(np.asarray(recs, REC))
    out = [None if t is None else np.zeros(t.shape, dt) for t in src]
    for i in range(n):
        for f in range(2):
            if src[f] is None:
                continue
            s, p = int(used[i]["sigma_q8"][f]), int(used[i]["bayer"])
            if s == 0 and p < 0 and src[f].dtype == dt:
                out[f][i] = src[f][i]        # (bit for bit)
                continue
            planes = [blur(to_bytes(src[f][i, c]), s) for c in range(3)]
            if p >= 0:
                planes = demosaic(*planes, p)
            for c in range(3):
                out[f][i, c] = planes[c].astype(dt)
    return tuple(out), used


# ---- what the tests share --------------------------------------------------------------------------------------------------
def frames(W, H, dtype="uint8", n=N, seed=1):
    """(image0, image1) [n,3,H,W]: blocks of flat colour with hard edges under noise, the first and last rows and columns
    saturated; a float32 frame also holds NaN, -3, 255.5, 1e9, infinities, a denormal and halves"""
    rng = np.random.RandomState(seed * 1000 + W)
    out = []
    for f in range(2):
        a = rng.randint(0, 256, (n, 3, H, W))
        blocks = rng.randint(0, 256, (n, 3, (H + 3) // 4, (W + 7) // 8))
        flat = np.repeat(np.repeat(blocks, 4, axis=2), 8, axis=3)[:, :, :H, :W]
        a[:, :, :, W // 2:] = flat[:, :, :, W // 2:]         # the right half: flat blocks, hard edges
        a[:, :, 0, :3] = 255
        a[:, :, -1, -3:] = (0, 255, 0)
        a = a.astype(dtype)
        if dtype == "float32":
            flat = a.reshape(-1)
            odd = np.array([np.nan, -3.0, 255.5, 1e9, np.inf, -np.inf, 1e-45, 0.5, 1.5, 254.5, 254.998], F32)
            at = rng.choice(flat.size, min(flat.size // 4, 44), replace=False)
            flat[at] = odd[np.arange(at.size) % odd.size]
        out.append(a)
    return tuple(out)


def rec_of(sigma_q8=0, bayer=-1):
    """one record; a pair sets the frames' sigmas apart"""
    r = np.zeros((), REC)
    r["sigma_q8"] = sigma_q8 if isinstance(sigma_q8, (tuple, list)) else (sigma_q8, sigma_q8)
    r["bayer"] = bayer
    return r


def record_sets():
    """three sets of n = 4 given records, which together hold: the identity; Bayer alone; blur alone with R = 1, 3 and 12; both;
    the two frames at different sigma (one of them 0); every pattern; a record that needs sanitising (sigmas and pattern out
    of range, radius and reserved words set)"""
    a = np.array([rec_of(), rec_of(bayer=2), rec_of(85), rec_of(256, bayer=0)], REC)
    b = np.array([rec_of(1024), rec_of((300, 0), bayer=1), rec_of((0, 700), bayer=3), rec_of((40, 1000))], REC)
    c = np.array([rec_of((-5, 2 ** 31 - 1), bayer=4), rec_of((1025, -2 ** 31), bayer=-2), rec_of(1, bayer=3), rec_of((600, 86), bayer=2 ** 31 - 1)], REC)
    c["radius"], c["reserved"] = 99, 7
    return [a, b, c]
