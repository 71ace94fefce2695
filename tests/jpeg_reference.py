"""numpy restatement of the block compression (ofdg_jpeg, include/ofdg.h) - written from the header's text alone: the draw, the
sanitising, the tables, the colour transforms, the block grid, the four integer passes and the quantiser, all blocks of a
plane at once - the orthonormal float64 codec the definition is measured against, and the planes and records the tests share."""
import numpy as np

from camera_reference import isym, to_bytes, unit  # noqa: F401  (u() and isym() of the jitter, the byte of a float32 element)
from erase_reference import equal_bits, expect_equal, key_of, philox  # noqa: F401  (the Philox block and the comparisons)

F32 = np.float32
REC = np.dtype([("quality", "<i4", (2,)), ("subsample", "<i4"), ("phase_x", "<i4"), ("phase_y", "<i4"), ("reserved", "<i4", (3,))])
N = 3
SIZES = [(8, 2), (24, 10), (40, 26), (72, 34)]   # (W, H) of the CPU tests
GPU_SIZES = SIZES + [(136, 18)]
PHASES = [(0, 0), (3, 5), (8, 8), (15, 1)]
DEFAULT = dict(prob=0.5, quality_min=30, quality_max=95, quality_delta=5, subsample=-1, sub_prob=0.5, phase=True)

# T.81 Annex K, Tables K.1 and K.2, [v][u]
K1 = np.array([[16, 11, 10, 16, 24, 40, 51, 61], [12, 12, 14, 19, 26, 58, 60, 55], [14, 13, 16, 24, 40, 57, 69, 56], [14, 17, 22, 29, 51, 87, 80, 62],
               [18, 22, 37, 56, 68, 109, 103, 77], [24, 35, 55, 64, 81, 104, 113, 92], [49, 64, 78, 87, 103, 121, 120, 101],
               [72, 92, 95, 98, 112, 100, 103, 99]], np.int64)
K2 = np.full((8, 8), 99, np.int64)
K2[:4, :4] = [[17, 18, 24, 47], [18, 21, 26, 66], [24, 26, 56, 99], [47, 66, 99, 99]]

# C[u][x]: the orthonormal DCT-II matrix; T = lrint(8192 C) = lrint(4096 s(u) cos((2 x + 1) u pi / 16))
_u, _x = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
C = np.where(_u == 0, np.sqrt(0.5), 1.0) * np.cos((2 * _x + 1) * _u * np.pi / 16) / 2
T = np.rint(8192 * C).astype(np.int64)
assert sorted(set(np.abs(T).reshape(-1).tolist())) == [799, 1567, 2276, 2896, 3406, 3784, 4017]


# ---- 1. draw ---------------------------------------------------------------------------------------------------------------
def draw(seed, index, ranges):
    b = philox(np.arange(2), 0, 0x0C7B, 0, key_of(seed, index))
    lo, hi, delta = int(ranges.get("quality_min", 75)), int(ranges.get("quality_max", 75)), int(ranges.get("quality_delta", 0))
    sub = int(ranges.get("subsample", -1))
    on = unit(b[0, 0]) < F32(ranges.get("prob", 0.0))
    q0 = lo + ((int(b[0, 1]) * (hi - lo + 1)) >> 32)
    q1 = min(100, max(1, q0 + isym(b[0, 2], delta)))
    r = np.zeros((), REC)
    r["quality"] = (q0, q1) if on else (0, 0)
    r["subsample"] = sub if sub >= 0 else int(unit(b[0, 3]) < F32(ranges.get("sub_prob", 0.0)))
    if ranges.get("phase", False):
        r["phase_x"], r["phase_y"] = int(b[1, 0]) >> 28, int(b[1, 1]) >> 28
    return r


def drawn_records(seed, first_index, n, ranges):
    return np.array([draw(seed, first_index + i, ranges) for i in range(n)], REC)


# ---- 2. sanitise -----------------------------------------------------------------------------------------------------------
def sanitise(recs):
    out = np.zeros(recs.shape, REC)
    out["quality"] = np.clip(recs["quality"], 0, 100)
    out["subsample"] = np.where(recs["subsample"] == 1, 1, 0)
    for k in ("phase_x", "phase_y"):
        out[k] = np.where((recs[k] < 0) | (recs[k] > 15), 0, recs[k])
    return out


# ---- 3. tables -------------------------------------------------------------------------------------------------------------
def tables(quality):
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((base * scale + 50) // 100, 1, 255) for base in (K1, K2))


# ---- 4. / 7. colour, on int64 planes ---------------------------------------------------------------------------------------
def to_ycc(B, G, R):
    return ((19595 * R + 38470 * G + 7471 * B + 32768) >> 16, (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16,
            (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16)


def to_bgr(Y, Cb, Cr):
    cb, cr = Cb - 128, Cr - 128
    return tuple(np.clip(v, 0, 255) for v in (Y + ((116130 * cb + 32768) >> 16), Y + ((-22554 * cb - 46802 * cr + 32768) >> 16), Y + ((91881 * cr + 32768) >> 16)))


# ---- 6. blocks [.., 8, 8] (y, x) of bytes as int64 -------------------------------------------------------------------------
def codec(blocks, Q):
    """(levels [.., v, u], decoded bytes [.., y, x]) of the integer definition"""
    p = blocks.astype(np.int64) - 128
    A1 = (p @ T.T + 256) >> 9                     # A[y][u] = sum_x T[u][x] p[y][x]
    F = T @ A1                                    # F[v][u] = sum_y T[v][y] A1[y][u]
    level = np.sign(F) * ((np.abs(F) + Q * 65536) // (Q * 131072))
    B1 = (T.T @ (level * Q) + 256) >> 9           # B[y][u] = sum_v T[v][y] D[v][u]
    P = B1 @ T                                    # P[y][x] = sum_u T[u][x] B1[y][u]
    return level, np.clip(((P + 65536) >> 17) + 128, 0, 255)


def codec_float(blocks, Q):
    """the same in float64: the orthonormal DCT, quantisation to nearest with halves away from zero, the inverse, to nearest"""
    p = blocks.astype(np.float64) - 128.0
    F = C @ p @ C.T
    level = np.sign(F) * np.floor(np.abs(F) / Q + 0.5)
    out = C.T @ (level * Q) @ C
    return level.astype(np.int64), np.clip(np.floor(out + 128.5), 0, 255).astype(np.int64)


# ---- 5. geometry -----------------------------------------------------------------------------------------------------------
def _blocks(a):
    h, w = a.shape
    return a.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)


def _plane(b):
    ny, nx = b.shape[:2]
    return b.transpose(0, 2, 1, 3).reshape(ny * 8, nx * 8)


def compress(B, G, R, quality, sub, phase_x, phase_y):
    """the three decoded planes of one frame's bytes [H, W] (int64)"""
    H, W = B.shape
    M = 16 if sub else 8
    px, py = (phase_x, phase_y) if sub else (phase_x & 7, phase_y & 7)
    ny, nx = (H + py + M - 1) // M, (W + px + M - 1) // M
    ys, xs = np.clip(np.arange(M * ny) - py, 0, H - 1), np.clip(np.arange(M * nx) - px, 0, W - 1)
    qy, qc = tables(quality)
    dec = []
    for c, comp in enumerate(to_ycc(B, G, R)):
        ext = comp[ys][:, xs]                    # the edge replicated on all four sides
        if sub and c > 0:
            cells = (ext[0::2, 0::2] + ext[0::2, 1::2] + ext[1::2, 0::2] + ext[1::2, 1::2] + 2) >> 2
            out = _plane(codec(_blocks(cells), qc)[1])
            out = np.repeat(np.repeat(out, 2, axis=0), 2, axis=1)
        else:
            out = _plane(codec(_blocks(ext), qc if c else qy)[1])
        dec.append(out[py:py + H, px:px + W])
    return to_bgr(*dec)


# ---- the whole call --------------------------------------------------------------------------------------------------------
def jpeg(src, recs=None, seed=0, first_index=0, ranges=None, dst_dtype=None):
    """((out0, out1), records used) as the copying call leaves them (the in-place form leaves the same in the sources)"""
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
            r = used[i]
            q = int(r["quality"][f])
            if q == 0 and src[f].dtype == dt:
                out[f][i] = src[f][i]        # (bit for bit)
                continue
            planes = [to_bytes(src[f][i, c]) for c in range(3)]
            if q > 0:
                planes = compress(*planes, q, int(r["subsample"]), int(r["phase_x"]), int(r["phase_y"]))
            for c in range(3):
                out[f][i, c] = planes[c].astype(dt)
    return tuple(out), used


# ---- what the tests share --------------------------------------------------------------------------------------------------
def frames(W, H, dtype="uint8", n=N, seed=1):
    """(image0, image1) [n,3,H,W]: smooth gradients with a flat rectangle and a hard, saturated edge under mild noise - what
    compression has something to do with -, one sample of plain noise; a float32 frame also holds NaN, -3, 255.5, 1e9,
    infinities, a denormal and halves"""
    rng = np.random.RandomState(seed * 1000 + W + H)
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    out = []
    for f in range(2):
        a = np.empty((n, 3, H, W), np.float64)
        for i in range(n):
            for c in range(3):
                a[i, c] = 128 + 100 * np.sin((x * (c + 1) + 2 * f) / 9.0 + i) * np.cos((y + f) / (5.0 + c))
            a[i, :, H // 3:, W // 2:] = rng.randint(0, 256, (3, 1, 1))
            a[i, 2, :, W // 4:W // 4 + 3] = 255
            a[i, 0, :, W // 4:W // 4 + 3] = 0
        a += rng.normal(0, 3, a.shape)
        a[n - 1] = rng.randint(0, 256, (3, H, W))
        a = np.clip(np.rint(a), 0, 255).astype(dtype)
        if dtype == "float32":
            flat = a.reshape(-1)
            odd = np.array([np.nan, -3.0, 255.5, 1e9, np.inf, -np.inf, 1e-45, 0.5, 1.5, 254.5, 254.998], F32)
            at = rng.choice(flat.size, min(flat.size // 4, 44), replace=False)
            flat[at] = odd[np.arange(at.size) % odd.size]
        out.append(a)
    return tuple(out)


def rec_of(quality=0, subsample=0, phase=(0, 0)):
    """one record; a pair sets the frames' qualities apart"""
    r = np.zeros((), REC)
    r["quality"] = quality if isinstance(quality, (tuple, list)) else (quality, quality)
    r["subsample"], r["phase_x"], r["phase_y"] = subsample, phase[0], phase[1]
    return r


def recs_of(quality, subsample=0, phase=(0, 0), n=N):
    return np.array([rec_of(quality, subsample, phase)] * n, REC)


def hostile_records():
    """n = 3 records that need sanitising: every field out of range on either side, reserved words set"""
    big, small = 2 ** 31 - 1, -2 ** 31
    c = np.array([rec_of((-5, big), 2, (16, -1)), rec_of((101, small), small, (big, small)), rec_of((60, 100), -1, (15, 15))], REC)
    c["reserved"] = 7
    return c


def synthetic(W=96, H=64, seed=5):
    """the picture of the comparison with Pillow, [3,H,W] uint8 B, G, R: gradients, two flat rectangles, noise of sigma 6"""
    rng = np.random.RandomState(seed)
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    a = np.stack([60 + 1.5 * x + 0.5 * y, 200 - 1.2 * x + 0.8 * y, 90 + 0.6 * x + 1.4 * y])
    a[:, 10:30, 12:40] = np.array([40.0, 170.0, 220.0])[:, None, None]
    a[:, 36:58, 50:90] = np.array([200.0, 60.0, 90.0])[:, None, None]
    a += rng.normal(0, 6, a.shape)
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)
