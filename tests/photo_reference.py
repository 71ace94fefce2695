"""The definition of the photometric augmentation (ofdg_photo, include/ofdg.h; the elementary functions of
include/ofdg_detmath.h) restated in numpy from the header text: fp64 / float32 arrays whose every operation is one IEEE
rounding (numpy fuses nothing), Philox4x32-10 on uint64 arrays.  No GPU, no library call."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
RANGES = ("gamma_log", "contrast_log", "brightness", "colour_log", "sigma_max",
          "pair_gamma_log", "pair_contrast_log", "pair_brightness", "pair_colour_log")
# a record as float32 [16]: gamma[2] contrast[2] brightness[2] gain[2][3] sigma[2] reserved[2]
GAMMA, CONTRAST, BRIGHTNESS, GAIN, SIGMA, RESERVED = 0, 2, 4, 6, 12, 14
IDENTITY = np.array([1, 1, 1, 1, 0, 0, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0], np.float32)
SIZES = [(8, 2), (160, 100), (264, 200)]  # W, H
PAIRS = [("float32", "float32"), ("float32", "uint8"), ("uint8", "float32"), ("uint8", "uint8")]
F32 = np.float32


# ---- include/ofdg_detmath.h ------------------------------------------------------------------------------------------------
def det_exp(x):
    """ofdg_det_exp on a float64 array (|x| <= 700 here)."""
    x = np.asarray(x, np.float64)
    ln2_hi, ln2_lo, inv_ln2, big = 6.93147180369123816490e-01, 1.90821492927058770002e-10, 1.44269504088896338700e+00, 6755399441055744.0
    fk = (x * inv_ln2 + big) - big
    r = (x - fk * ln2_hi) - fk * ln2_lo
    p = np.full_like(x, 1.0 / 6227020800.0)
    for d in (479001600.0, 39916800.0, 3628800.0, 362880.0, 40320.0, 5040.0, 720.0, 120.0, 24.0, 6.0):
        p = p * r + 1.0 / d
    p = p * r + 0.5
    p = p * r + 1.0
    p = p * r + 1.0
    k = fk.astype(np.int64)
    k1 = np.where(k < 0, -((-k) // 2), k // 2)  # C division: towards zero
    k2 = k - k1
    return (p * np.ldexp(1.0, k1)) * np.ldexp(1.0, k2)


def det_log(x):
    """ofdg_det_log on a float64 array of finite, normal, positive numbers."""
    x = np.ascontiguousarray(x, np.float64)
    ln2_hi, ln2_lo = 6.93147180369123816490e-01, 1.90821492927058770002e-10
    b = x.view(np.uint64)
    e = (b >> np.uint64(52)).astype(np.int64) - 1023
    m = ((b & np.uint64(0x000FFFFFFFFFFFFF)) | np.uint64(0x3FF0000000000000)).view(np.float64)
    up = m >= 1.41421356237309514547
    m = np.where(up, m * 0.5, m)
    e = e + up
    s = (m - 1.0) / (m + 1.0)
    z = s * s
    p = np.full_like(x, 1.0 / 23.0)
    for d in (21.0, 19.0, 17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0):
        p = p * z + 1.0 / d
    p = p * z + 1.0
    lm = (2.0 * s) * p
    fe = e.astype(np.float64)
    return fe * ln2_hi + (fe * ln2_lo + lm)


# ---- Philox4x32-10 ---------------------------------------------------------------------------------------------------------
def philox(c0, c1, c2, c3, key):
    """The blocks of the counters {c0[i], c1, c2, c3} under key (two ints): uint64 [len(c0), 4] holding 32-bit words."""
    x = np.asarray(c0, np.uint64).copy()
    y, z, w = (np.full_like(x, v) for v in (c1, c2, c3))
    k0, k1 = int(key[0]), int(key[1])
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * x, np.uint64(0xCD9E8D57) * z
        x, y, z, w = (p1 >> np.uint64(32)) ^ y ^ np.uint64(k0), p1 & M32, (p0 >> np.uint64(32)) ^ w ^ np.uint64(k1), p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack([x, y, z, w], axis=1)


def key_of(seed, index):
    g = index & 0xFFFFFFFFFFFFFFFF
    return ((seed ^ (((g >> 32) * 0x9E3779B9) & 0xFFFFFFFF)) & 0xFFFFFFFF, g & 0xFFFFFFFF)


# ---- 1. draw ---------------------------------------------------------------------------------------------------------------
def unit(w):
    return F32(int(w) >> 8) * F32(2.0 ** -24)


def sym(w, a):
    r = F32(a) * (F32(2.0) * unit(w) - F32(1.0))
    return F32(0.0) if r == 0 else r


def expf(l):
    return F32(det_exp(np.array([np.float64(l)]))[0])


def draw(seed, index, ranges):
    """The drawn record (not sanitised) of global sample `index`: float32 [16]."""
    q = {k: F32(ranges.get(k, 0.0)) for k in RANGES}
    blocks = philox([0, 1, 2], 0, 0x0C71, 0, key_of(seed, index))
    a, b, d = ([int(v) for v in blocks[j]] for j in range(3))
    lg0, lc0, b0 = sym(a[0], q["gamma_log"]), sym(a[1], q["contrast_log"]), sym(a[2], q["brightness"])
    sigma = q["sigma_max"] * unit(a[3])
    col = [sym(b[c], q["colour_log"]) for c in range(3)]
    dg, dc, db, dcol = sym(d[0], q["pair_gamma_log"]), sym(d[1], q["pair_contrast_log"]), sym(d[2], q["pair_brightness"]), sym(d[3], q["pair_colour_log"])
    r = np.zeros(16, np.float32)
    r[GAMMA:GAMMA + 2] = expf(lg0), expf(lg0 + dg)
    r[CONTRAST:CONTRAST + 2] = expf(lc0), expf(lc0 + dc)
    r[BRIGHTNESS:BRIGHTNESS + 2] = b0, b0 + db
    r[GAIN:GAIN + 3] = [expf(v) for v in col]
    r[GAIN + 3:GAIN + 6] = [expf(v + dcol) for v in col]
    r[SIGMA:SIGMA + 2] = sigma, sigma
    return r


def drawn_records(seed, first_index, n, ranges):
    return np.stack([draw(seed, first_index + i, ranges) for i in range(n)])


# ---- 2. sanitise -----------------------------------------------------------------------------------------------------------
def _clamp(x, lo, hi, identity):
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(x != x, F32(identity), np.where(x < F32(lo), F32(lo), np.where(x > F32(hi), F32(hi), x))).astype(np.float32)


def sanitise(recs):
    """float32 [..., 16] -> the records as they are used"""
    r = np.array(recs, np.float32)
    r[..., GAMMA:GAMMA + 2] = _clamp(r[..., GAMMA:GAMMA + 2], 0.125, 8.0, 1.0)
    r[..., CONTRAST:CONTRAST + 2] = _clamp(r[..., CONTRAST:CONTRAST + 2], 0.0, 4.0, 1.0)
    r[..., BRIGHTNESS:BRIGHTNESS + 2] = _clamp(r[..., BRIGHTNESS:BRIGHTNESS + 2], -1.0, 1.0, 0.0)
    r[..., GAIN:GAIN + 6] = _clamp(r[..., GAIN:GAIN + 6], 0.0, 8.0, 1.0)
    r[..., SIGMA:SIGMA + 2] = _clamp(r[..., SIGMA:SIGMA + 2], 0.0, 64.0, 0.0)
    r[..., RESERVED:RESERVED + 2] = 0.0
    return r


# ---- 3. table --------------------------------------------------------------------------------------------------------------
def table(rec):
    """float32 [2,3,256] of ONE record (sanitised here)"""
    r = sanitise(rec)
    k = np.arange(256, dtype=np.float64)
    x = k / 255.0
    out = np.zeros((2, 3, 256), np.float32)
    for f in range(2):
        gamma = np.float64(r[GAMMA + f])
        if r[GAMMA + f] == F32(1.0):
            p = x.copy()
        else:
            p = np.zeros(256)
            p[1:] = det_exp(gamma * det_log(x[1:]))
        p[0] = 0.0
        for c in range(3):
            t = p * np.float64(r[GAIN + 3 * f + c])
            t = t - 0.5
            t = t * np.float64(r[CONTRAST + f])
            t = t + 0.5
            t = t + np.float64(r[BRIGHTNESS + f])
            t = 255.0 * t
            t = np.where(t > 0.0, t, 0.0)
            t = np.where(t < 255.0, t, 255.0)
            out[f, c] = t.astype(np.float32)
    return out


# ---- 4. pixels -------------------------------------------------------------------------------------------------------------
def index_of(frame):
    """the table index of every element of a uint8 or float32 array"""
    if frame.dtype == np.uint8:
        return frame.astype(np.int64)
    with np.errstate(invalid="ignore"):
        e = np.where(frame > F32(0.0), frame, F32(0.0)).astype(np.float32)
        e = np.where(e < F32(255.0), e, F32(255.0)).astype(np.float32)
    return np.rint(e).astype(np.int64)


def photo(src, recs, seed=0, first_index=0, dst_dtype=None):
    """((image0, image1), sanitised records) of the frames src = (image0, image1), each [n,3,H,W] uint8 / float32 or None,
    under the records recs float32 [n,16] (drawn_records for a drawn call)."""
    given = [t for t in src if t is not None]
    n, _, H, W = given[0].shape
    dt = np.dtype(given[0].dtype if dst_dtype is None else dst_dtype)
    used = sanitise(recs)
    out = [None if t is None else np.zeros(t.shape, dt) for t in src]
    m = np.arange(3 * H * W, dtype=np.uint64)
    for i in range(n):
        T = table(used[i])
        key = key_of(seed, first_index + i)
        for f in range(2):
            if src[f] is None:
                continue
            k = index_of(src[f][i]).reshape(3, H * W)
            v = np.stack([T[f, c][k[c]] for c in range(3)]).reshape(-1).astype(np.float32)
            sigma = used[i][SIGMA + f]
            if sigma > 0:
                words = philox(np.arange((3 * H * W + 3) // 4, dtype=np.uint64), f, 0x0C72, 0, key).reshape(-1)[m]
                s = (words & np.uint64(255)) + ((words >> np.uint64(8)) & np.uint64(255)) + ((words >> np.uint64(16)) & np.uint64(255)) + (words >> np.uint64(24))
                scale = F32(sigma) / F32(147.80054)
                d = (scale * (s.astype(np.int64) - 510).astype(np.float32)).astype(np.float32)
                v = (v + d).astype(np.float32)
                v = np.where(v > F32(0.0), v, F32(0.0)).astype(np.float32)
                v = np.where(v < F32(255.0), v, F32(255.0)).astype(np.float32)
            o = v if dt == np.float32 else np.rint(v).astype(np.uint8)
            out[f][i] = o.reshape(3, H, W)
    return tuple(out), used


# ---- test data -------------------------------------------------------------------------------------------------------------
N = 12


def records():
    """N records [N,16]: identity; a plain one with noise; each clamp edge; beyond each edge; NaN everywhere; infinities; a
    non-zero reserved word and -0.0 fields; noise in frame 1 only."""
    r = np.tile(IDENTITY, (N, 1))
    r[1] = [0.8, 1.3, 1.2, 0.9, 0.05, -0.03, 1.1, 0.9, 1.05, 0.95, 1.2, 0.8, 6.0, 6.0, 0, 0]
    r[2] = [0.125, 8.0, 0.0, 4.0, -1.0, 1.0, 0.0, 8.0, 1.0, 8.0, 0.0, 1.0, 0.0, 64.0, 0, 0]
    r[3] = [8.0, 0.125, 4.0, 0.0, 1.0, -1.0, 8.0, 0.0, 0.5, 1.0, 2.0, 8.0, 64.0, 0.0, 0, 0]
    r[4] = [0.01, 100.0, -1.0, 9.0, -5.0, 5.0, -2.0, 20.0, 1.0, 1.0, 1.0, 1.0, -1.0, 1000.0, 0, 0]
    r[5] = [np.nan] * 14 + [0, 0]
    r[6] = [np.inf, -np.inf, np.inf, -np.inf, np.inf, -np.inf, np.inf, -np.inf, np.inf, 1.0, -np.inf, 1.0, np.inf, -np.inf, 0, 0]
    r[7] = [1.0, 1.0, -0.0, 1.0, -0.0, 0.0, -0.0, 1.0, 1.0, 1.0, 1.0, 1.0, -0.0, 0.0, 0, 0]
    r[7].view(np.int32)[RESERVED:] = (7, -1)
    r[8] = [2.2, 0.45, 0.7, 1.6, 0.2, -0.2, 1.5, 0.7, 1.0, 0.6, 1.4, 1.0, 0.0, 25.0, 0, 0]
    r[9] = [1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.5, 3.0, 0, 0]
    r[10] = [0.5, 2.0, 1.0, 1.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0, 0]
    r[11] = [1.0, 1.0, 3.0, 0.3, -0.4, 0.4, 1.0, 2.0, 0.5, 1.0, 1.0, 1.0, 12.0, 0.0, 0, 0]
    return r.astype(np.float32)


_SPECIAL = [np.nan, -3.0, 255.5, 1e9, -0.0, 0.5, 1.5, 2.5, 254.5, 254.49998, np.inf, -np.inf, 1e-40, 127.5, 128.5]


def frames(W, H, dtype="uint8", n=N, seed=1):
    """(image0, image1) [n,3,H,W]: every byte value occurs in every channel of a frame that has 256 elements and more;
    float32 frames hold the byte values (what the generator stores) with the special values planted at fixed places."""
    rng = np.random.RandomState(seed * 1000 + W + H)
    out = []
    for f in range(2):
        a = rng.randint(0, 256, size=(n, 3, H, W)).astype(np.uint8)
        flat = a.reshape(n, 3, -1)
        count = min(256, flat.shape[2])
        flat[:, :, :count] = (np.arange(count) + 37 * f) % 256
        if dtype == "float32":
            a = a.astype(np.float32)
            flat = a.reshape(n, 3, -1)
            size = flat.shape[2]
            for j, v in enumerate(_SPECIAL):  # (7 is coprime to every size here: distinct places; and once more near the end)
                flat[:, :, (3 + 7 * j) % size] = F32(v)
                if size > 256:
                    flat[:, :, size - 1 - 5 * j] = F32(v)
        out.append(a)
    return tuple(out)


def expect_equal(got, want, what=""):
    """byte for byte, frame by frame (NaNs compare as their bits)"""
    for f in range(2):
        assert (got[f] is None) == (want[f] is None), (what, f)
        if want[f] is None:
            continue
        a, b = np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f])
        assert a.dtype == b.dtype and a.shape == b.shape, (what, f, a.dtype, b.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            bad = np.argwhere(a.view(np.uint8 if a.dtype == np.uint8 else np.uint32) != b.view(np.uint8 if a.dtype == np.uint8 else np.uint32))
            first = tuple(bad[0])
            raise AssertionError("%s: image%d differs at %d elements, first %s: got %r, want %r" % (what, f, len(bad), first, a[first], b[first]))


def equal_bits(a, b):
    return np.ascontiguousarray(a, np.float32).tobytes() == np.ascontiguousarray(b, np.float32).tobytes()
