"""numpy restatement of the colour jitter (ofdg_jitter, include/ofdg.h) - written from the header's text alone: the draw, the
sanitising, the order's permutation, the four operations on bytes, the mean - and the planes and records the tests share."""
import itertools

import numpy as np

from erase_reference import equal_bits, expect_equal, key_of, philox  # noqa: F401  (the Philox block and the comparisons)

F32 = np.float32
ONE, TURN = 65536, 393216
REC = np.dtype([("brightness", "<i4", (2,)), ("contrast", "<i4", (2,)), ("saturation", "<i4", (2,)), ("hue", "<i4", (2,)), ("order", "<i4", (2,)),
                ("shared", "<i4"), ("mean", "<i4", (2,)), ("reserved", "<i4", (3,))])
FIELDS = ("brightness", "contrast", "saturation", "hue", "order")
PERMS = list(itertools.permutations(range(4)))   # of (brightness, contrast, saturation, hue), in lexicographic order
BRIGHTNESS, CONTRAST, SATURATION, HUE = range(4)
N = 4
SIZES = [(8, 2), (24, 6), (72, 40), (264, 200)]
RAFT = dict(brightness=0.4, contrast=0.4, saturation=0.4, hue=0.5 / 3.14, asym_prob=0.2)


# ---- 1. draw ---------------------------------------------------------------------------------------------------------------
def amp(rng, unit):
    return int(np.rint(F32(rng) * F32(unit)))       # (float32 product, to nearest even)


def isym(w, A):
    return ((int(w) * (2 * A + 1)) >> 32) - A


def draw(seed, index, ranges):
    b = philox(np.arange(3), 0, 0x0C78, 0, key_of(seed, index))
    A = [amp(ranges.get("brightness", 0.0), 65536.0), amp(ranges.get("contrast", 0.0), 65536.0), amp(ranges.get("saturation", 0.0), 65536.0),
         amp(ranges.get("hue", 0.0), 393216.0)]
    r = np.zeros((), REC)
    asym = F32(int(b[2, 0]) >> 8) * F32(2.0 ** -24) < F32(ranges.get("asym_prob", 0.0))
    for f in range(2):
        s = f if asym else 0
        r["brightness"][f], r["contrast"][f], r["saturation"][f] = (ONE + isym(b[s, k], A[k]) for k in range(3))
        r["hue"][f] = isym(b[s, 3], A[3])
        r["order"][f] = ((int(b[2, 1 + s]) >> 8) * 24) >> 24
    r["shared"] = 0 if asym else 1
    r["mean"] = -1
    return r


def drawn_records(seed, first_index, n, ranges):
    return np.array([draw(seed, first_index + i, ranges) for i in range(n)], REC)


# ---- 2. sanitise -----------------------------------------------------------------------------------------------------------
def sanitise(recs):
    out = np.zeros(recs.shape, REC)
    for k in ("brightness", "contrast", "saturation"):
        out[k] = np.clip(recs[k], 0, 4 * ONE)
    out["hue"] = np.clip(recs["hue"], -TURN // 2, TURN // 2)
    out["order"] = np.clip(recs["order"], 0, 23)
    same = np.all([out[k][..., 0] == out[k][..., 1] for k in FIELDS], axis=0)
    out["shared"] = ((recs["shared"] != 0) & same).astype(np.int32)
    out["mean"] = -1
    return out


# ---- 3. the operations, on int64 arrays of bytes ----------------------------------------------------------------------------
def lum(B, G, R):
    return (7471 * B + 38470 * G + 19595 * R + 32768) >> 16


def mix(a, m, q):
    return np.clip((q * a + (ONE - q) * m + 32768) >> 16, 0, 255)


def hue_shift(B, G, R, h):
    mx, mn = np.maximum(np.maximum(R, G), B), np.minimum(np.minimum(R, G), B)
    d = mx - mn
    # (largest, smallest, third) channel of sectors 0..5; the first that holds
    table = [(R, B, G), (G, B, R), (G, R, B), (B, R, G), (B, G, R), (R, G, B)]
    s = np.full(B.shape, 5, np.int64)
    for k in range(4, -1, -1):
        s = np.where((table[k][0] == mx) & (table[k][1] == mn), k, s)
    mid = np.choose(s, [t[2] for t in table])
    t = np.where(s & 1, d - (mid - mn), mid - mn)
    hq = (ONE * s + (ONE * t) // np.maximum(d, 1) + h) % TURN
    s2, f2 = hq >> 16, hq & 65535
    nm = mn + ((d * np.where(s2 & 1, ONE - f2, f2) + 32768) >> 16)
    place = lambda big, small: np.where(np.isin(s2, big), mx, np.where(np.isin(s2, small), mn, nm))  # noqa: E731
    nB, nG, nR = place((3, 4), (0, 1)), place((1, 2), (4, 5)), place((0, 5), (2, 3))
    keep = d == 0
    return np.where(keep, B, nB), np.where(keep, G, nG), np.where(keep, R, nR)


def apply_ops(bgr, fields, places, mean):
    """the operations at the first `places` places of the frame's order on bgr = (B, G, R); fields: the frame's five numbers"""
    b, c, s, h, order = (int(v) for v in fields)
    B, G, R = bgr
    for op in PERMS[order][:places]:
        if op == BRIGHTNESS:
            B, G, R = mix(B, 0, b), mix(G, 0, b), mix(R, 0, b)
        elif op == CONTRAST:
            B, G, R = mix(B, mean, c), mix(G, mean, c), mix(R, mean, c)
        elif op == SATURATION:
            l_ = lum(B, G, R)
            B, G, R = mix(B, l_, s), mix(G, l_, s), mix(R, l_, s)
        else:
            B, G, R = hue_shift(B, G, R, h)
    return B, G, R


def to_bytes(frame):
    """the bytes of a frame [.., H, W] of uint8 or float32, as int64"""
    if frame.dtype == np.uint8:
        return frame.astype(np.int64)
    v = frame.astype(F32)
    v = np.where(v > 0, v, F32(0))       # (a NaN becomes 0)
    v = np.where(v < 255, v, F32(255))
    return np.rint(v).astype(np.int64)


def mean_byte(S, P):
    return (2 * int(S) + int(P)) // (2 * int(P))


# ---- the whole call --------------------------------------------------------------------------------------------------------
def jitter(src, recs=None, seed=0, first_index=0, ranges=None, dst_dtype=None, in_place=False):
    """((image0, image1), records used) as the call leaves them; the inputs are not written (in_place only says that the
    destination is the source: an identity frame of equal formats keeps its bits either way)"""
    given = [t for t in src if t is not None]
    n, _, H, W = given[0].shape
    dt = np.dtype(given[0].dtype if dst_dtype is None else dst_dtype)
    if recs is None:
        recs = drawn_records(seed, first_index, n, ranges or {})
    used = sanitise(np.asarray(recs, REC))
    out = [None if t is None else np.zeros(t.shape, dt) for t in src]
    P = W * H
    for i in range(n):
        r = used[i]
        fields = [tuple(int(r[k][f]) for k in FIELDS) for f in range(2)]
        byts = [None if t is None else tuple(to_bytes(t[i, c]) for c in range(3)) for t in src]
        S = [0, 0]
        for f in range(2):
            if src[f] is not None and fields[f][1] != ONE:
                places = PERMS[fields[f][4]].index(CONTRAST)
                S[f] = int(lum(*apply_ops(byts[f], fields[f], places, 0)).sum())
        joint = bool(r["shared"]) and src[0] is not None and src[1] is not None
        for f in range(2):
            if src[f] is None:
                continue
            mean = -1
            if fields[f][1] != ONE:
                mean = mean_byte(S[0] + S[1], 2 * P) if joint else mean_byte(S[f], P)
            r["mean"][f] = mean
            b, c, s, h, _ = fields[f]
            if b == ONE and c == ONE and s == ONE and h == 0 and src[f].dtype == dt:
                out[f][i] = src[f][i]        # (bit for bit)
                continue
            for ch, v in enumerate(apply_ops(byts[f], fields[f], 4, mean)):
                out[f][i, ch] = v.astype(dt)
    return tuple(out), used


# ---- what the tests share --------------------------------------------------------------------------------------------------
def frames(W, H, dtype="uint8", n=N, seed=1):
    """(image0, image1) [n,3,H,W]: byte values, smooth enough to hold saturated and grey pixels; a float32 frame also holds NaN,
    -3, 255.5, 1e9, infinities, a denormal and halves"""
    rng = np.random.RandomState(seed * 1000 + W)
    out = []
    for f in range(2):
        a = rng.randint(0, 256, (n, 3, H, W))
        a[:, :, ::2, ::4] = a[:, :1, ::2, ::4]              # grey pixels (d = 0)
        a[:, 1, :, 1::4] = a[:, 0, :, 1::4]                 # ties of two channels
        a[:, 2, 1::2, 2::4] = a[:, 1, 1::2, 2::4]
        a = a.astype(dtype)
        if dtype == "float32":
            flat = a.reshape(-1)
            odd = np.array([np.nan, -3.0, 255.5, 1e9, np.inf, -np.inf, 1e-45, 0.5, 1.5, 254.5, 254.998], F32)
            at = rng.choice(flat.size, min(flat.size // 4, 44), replace=False)
            flat[at] = odd[np.arange(at.size) % odd.size]
        out.append(a)
    return tuple(out)


def rec_of(brightness=ONE, contrast=ONE, saturation=ONE, hue=0, order=0, shared=0):
    """one record; a pair sets the frames apart"""
    r = np.zeros((), REC)
    for k, v in zip(FIELDS, (brightness, contrast, saturation, hue, order)):
        r[k] = v if isinstance(v, (tuple, list)) else (v, v)
    r["shared"] = shared
    return r


def records():
    """n = 4 given records: the identity; one without a contrast (mean -1), shared; an asymmetric one that claims to be shared,
    with non-zero mean and reserved words; one at every clamp"""
    r = np.zeros((N,), REC)
    r[0] = rec_of()
    r[1] = rec_of(brightness=80000, saturation=30000, hue=-50000, order=17, shared=1)
    r[2] = rec_of(brightness=(52000, 70000), contrast=(90000, 40000), saturation=(100000, 65536), hue=(21845, -131072), order=(9, 20), shared=1)
    r[2]["mean"], r[2]["reserved"] = 77, 5
    r[3] = rec_of(brightness=(-5, 2 ** 31 - 1), contrast=(4 * ONE + 1, -2 ** 31), saturation=(2 ** 30, -1), hue=(-2 ** 31, 196609), order=(-1, 24), shared=-7)
    return r


def records_orders():
    """24 records, one per order, all four operations away from the identity, both frames alike and shared"""
    return np.array([rec_of(brightness=75000, contrast=110000, saturation=20000, hue=40000, order=k, shared=1) for k in range(24)], REC)


def cube(lo=0, n=16):
    """samples lo .. lo + n - 1 of the colour cube as sixteen [3,1024,1024] uint8 samples: pixel (y, x) of sample i holds B = 16 i
    + (y >> 6), G = (y & 63) * 4 + (x >> 8), R = x & 255 - every colour once"""
    y, x = np.meshgrid(np.arange(1024), np.arange(1024), indexing="ij")
    out = np.zeros((n, 3, 1024, 1024), np.uint8)
    for k in range(n):
        out[k, 0] = 16 * (lo + k) + (y >> 6)
        out[k, 1] = (y & 63) * 4 + (x >> 8)
        out[k, 2] = x & 255
    return out
