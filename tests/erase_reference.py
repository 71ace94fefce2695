"""numpy restatement of the occluder rectangles (ofdg_erase, include/ofdg.h) - written from the header's text alone: the draw,
the sanitising, the integer mean, the noise bytes and the occlusion rule - and the planes and records the tests share."""
import numpy as np

F32 = np.float32
M32 = np.uint64(0xFFFFFFFF)
REC = np.dtype([("count", "<i4"), ("rect", "<i4", (4, 5)), ("fill", "u1", (2, 3)), ("reserved", "u1", (6,))])
FRAME0, FRAME1, OCC = 1, 2, 4
MEAN, CONST, NOISE = 0, 1, 2
N = 3
SIZES = [(8, 2), (24, 6), (72, 40), (264, 200)]
RAFT = dict(prob=0.5, min_rects=1, max_rects=2, min_size=50, max_size=99)


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
def pick(w, lo, hi):
    return lo + ((int(w) * (hi - lo + 1)) >> 32)


def draw(seed, index, W, H, ranges, frames=(1,)):
    b = philox(np.arange(5), 0, 0x0C74, 0, key_of(seed, index))
    r = np.zeros((), REC)
    erased = F32(int(b[0, 0]) >> 8) * F32(2.0 ** -24) < F32(ranges["prob"])
    if not erased:
        return r
    r["count"] = pick(b[0, 1], ranges["min_rects"], ranges["max_rects"])
    for k in range(int(r["count"])):
        frame = (int(b[0, 2]) >> k) & 1 if len(frames) == 2 else frames[0]
        r["rect"][k] = (pick(b[k + 1, 2], 0, W - 1), pick(b[k + 1, 3], 0, H - 1), pick(b[k + 1, 0], ranges["min_size"], ranges["max_size"]),
                        pick(b[k + 1, 1], ranges["min_size"], ranges["max_size"]), frame)
    return r


def drawn_records(seed, first_index, n, W, H, ranges, frames=(1,)):
    return np.array([draw(seed, first_index + i, W, H, ranges, frames) for i in range(n)], REC)


# ---- 2. sanitise -----------------------------------------------------------------------------------------------------------
def sanitise(recs, W, H, frames=(1,)):
    out = np.zeros(recs.shape, REC)
    for i, r in enumerate(recs):
        kept = 0
        for k in range(min(max(int(r["count"]), 0), 4)):
            x0, y0, w, h, f = (int(v) for v in r["rect"][k])
            f &= 1
            cx0, cy0, cx1, cy1 = max(x0, 0), max(y0, 0), min(x0 + w, W), min(y0 + h, H)
            if f not in frames or w < 1 or h < 1 or cx1 <= cx0 or cy1 <= cy0:
                continue
            out[i]["rect"][kept] = (cx0, cy0, cx1 - cx0, cy1 - cy0, f)
            kept += 1
        out[i]["count"] = kept
    return out


# ---- 3. fill ---------------------------------------------------------------------------------------------------------------
def q8(channel):
    """the Q8 values of a channel (uint8 or float32) as uint64"""
    if channel.dtype == np.uint8:
        return channel.astype(np.uint64) * np.uint64(256)
    v = channel.astype(F32)
    v = np.where(v > 0, v, F32(0))       # (a NaN becomes 0)
    v = np.where(v < 255, v, F32(255))
    return np.rint(v * F32(256.0)).astype(np.uint64)


def mean_byte(S, P):
    mean_q8 = (2 * int(S) + int(P)) // (2 * int(P))
    return (mean_q8 + 128) >> 8


def noise_bytes(seed, index, f, elems):
    """the noise byte of each element number in `elems` (any shape) of frame f of global sample `index`"""
    e = np.asarray(elems, np.uint64)
    blocks = philox((e >> np.uint64(2)).reshape(-1), f, 0x0C75, 0, key_of(seed, index))
    word = blocks[np.arange(e.size), (e & np.uint64(3)).reshape(-1).astype(np.int64)]
    return (word >> np.uint64(24)).astype(np.uint8).reshape(e.shape)


# ---- 4. occlusion ----------------------------------------------------------------------------------------------------------
def _axis_inside(at, d, lo, length):
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.floor((at.astype(F32) + d.astype(F32)) + F32(0.5))
        return (t >= F32(lo)) & (t <= F32(lo + length - 1))


def marks(rec, f, cross, flow, W, H):
    """bool [H,W]: the elements of the map of frame f one sanitised record marks; flow [2,H,W] or None"""
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    hit = np.zeros((H, W), bool)
    for k in range(int(rec["count"])):
        x0, y0, w, h, fr = (int(v) for v in rec["rect"][k])
        if fr == f:
            hit[y0:y0 + h, x0:x0 + w] = True
        elif cross:
            hit |= _axis_inside(xs, flow[0], x0, w) & _axis_inside(ys, flow[1], y0, h)
    return hit


# ---- the whole call --------------------------------------------------------------------------------------------------------
def erase(images, occ=None, flow=None, recs=None, seed=0, first_index=0, ranges=None, fill=MEAN, color=(0, 0, 0), frames=(1,), mark_occ=None):
    """(images, occ, records used) as the call leaves them; the inputs are not written"""
    images = [None if t is None else np.array(t) for t in images]
    occ = [None, None] if occ is None else [None if t is None else np.array(t) for t in occ]
    flow = [None, None] if flow is None else list(flow)
    first = next(t for t in images if t is not None)
    n, _, H, W = first.shape
    if mark_occ is None:
        mark_occ = any(t is not None for t in occ)
    if recs is None:
        recs = drawn_records(seed, first_index, n, W, H, ranges, frames)
    used = sanitise(recs, W, H, frames)
    P = W * H
    for i, r in enumerate(used):
        rects = [tuple(int(v) for v in r["rect"][k]) for k in range(int(r["count"]))]
        for f in sorted({q[4] for q in rects}):
            img = images[f][i]
            if fill == MEAN:
                r["fill"][f] = [mean_byte(q8(img[c]).sum(dtype=np.uint64), P) for c in range(3)]
            elif fill == CONST:
                r["fill"][f] = color
            for x0, y0, w, h, fr in rects:
                if fr != f:
                    continue
                for c in range(3):
                    if fill == NOISE:
                        ys, xs = np.meshgrid(np.arange(y0, y0 + h), np.arange(x0, x0 + w), indexing="ij")
                        img[c, y0:y0 + h, x0:x0 + w] = noise_bytes(seed, first_index + i, f, c * P + ys * W + xs)
                    else:
                        img[c, y0:y0 + h, x0:x0 + w] = r["fill"][f][c]
        if mark_occ and rects:
            for f in range(2):
                if occ[f] is None:
                    continue
                cross = (1 - f) in frames
                fl = flow[f][i].astype(F32) if cross else None
                occ[f][i, 0][marks(r, f, cross, fl, W, H)] = 1
    return images, occ, used


# ---- what the tests share --------------------------------------------------------------------------------------------------
def records(W, H):
    """n = 3 given records for a W x H plane: none; one (the whole frame, frame 1); four, clipped at borders, overlapping, one
    entirely outside, with count 7 and non-zero fill / reserved bytes."""
    r = np.zeros((N,), REC)
    r[0]["count"] = -1
    r[0]["rect"][0] = (0, 0, W, H, 1)            # (count -1: not used)
    r[1]["count"] = 1
    r[1]["rect"][0] = (0, 0, W, H, 1)
    r[2]["count"] = 7
    r[2]["rect"] = [(-3, -1, 3 + W // 2, 2, 1), (W // 3, H // 2 - 1, W, H, 3), (W, 0, 4, 4, 1), (W // 4 + 1, 0, max(W // 3, 1), H, 0)]
    r[2]["fill"] = 9
    r[2]["reserved"] = 7
    return r


def records_edges(W, H):
    """n = 3: 1x1 rectangles and one full row; a rectangle clipped at each border; one at each corner"""
    r = np.zeros((N,), REC)
    r[0]["count"] = 4
    r[0]["rect"] = [(W - 1, H - 1, 1, 1, 1), (0, H // 2, W, 1, 1), (W // 2, 0, 1, 1, 0), (3, 1, 1, 1, 1)]
    r[1]["count"] = 4
    r[1]["rect"] = [(-2, H // 2, 4, 1, 1), (W - 2, 0, 9, 1, 1), (W // 2, -5, 2, 6, 0), (W // 2 + 1, H - 1, 3, 32767, 1)]
    r[2]["count"] = 4
    r[2]["rect"] = [(-1, -1, 3, 2, 1), (W - 2, -1, 3, 2, 0), (-1, H - 1, 3, 2, 0), (W - 2, H - 1, 2147483647, 2147483647, 1)]
    return r


def frames(W, H, dtype="uint8", n=N, seed=1):
    """(image0, image1) [n,3,H,W]: byte values; a float32 frame also holds NaN, -3, 255.5, 1e9, infinities and a denormal"""
    rng = np.random.RandomState(seed * 1000 + W)
    out = []
    for f in range(2):
        a = rng.randint(0, 256, (n, 3, H, W)).astype(dtype)
        if dtype == "float32":
            flat = a.reshape(-1)
            odd = np.array([np.nan, -3.0, 255.5, 1e9, np.inf, -np.inf, 1e-45, 0.001953125, 0.005859375, 254.998], F32)
            at = rng.choice(flat.size, min(flat.size // 4, 40), replace=False)
            flat[at] = odd[np.arange(at.size) % odd.size]
        out.append(a)
    return tuple(out)


def flows(W, H, dtype="float32", n=N, seed=2):
    """(flow, flow1) [n,2,H,W]: small displacements, ties of the + 0.5 rounding, NaN, infinities, -0.0 and +-65504"""
    rng = np.random.RandomState(seed * 1000 + W)
    out = []
    for f in range(2):
        a = (rng.randint(-8 * 4, 8 * 4 + 1, (n, 2, H, W)) / 4.0).astype(F32)   # (multiples of 1/4: exact in binary16, ties included)
        flat = a.reshape(-1)
        odd = np.array([np.nan, np.inf, -np.inf, -0.0, 65504.0, -65504.0, 0.5, -0.5, 1.5], F32)
        at = rng.choice(flat.size, min(flat.size // 3, 60), replace=False)
        flat[at] = odd[np.arange(at.size) % odd.size]
        out.append(a.astype(dtype))
    return tuple(out)


def maps(W, H, dtype="float32", n=N, seed=3):
    """(occ0, occ1) [n,1,H,W]: mostly 0, some 1 and some other non-zero values whose bits must stay"""
    rng = np.random.RandomState(seed * 1000 + W)
    out = []
    for f in range(2):
        a = (rng.randint(0, 8, (n, 1, H, W)) == 0).astype(dtype)
        flat = a.reshape(-1)
        at = rng.choice(flat.size, min(flat.size // 5, 30), replace=False)
        flat[at] = np.array([2, 0.5, 255, 3], F32).astype(dtype)[np.arange(at.size) % 4] if dtype == "float32" else np.array([2, 7, 255, 3], np.uint8)[np.arange(at.size) % 4]
        if dtype == "float32":
            flat[at[:2]] = np.array([np.nan, -0.0], F32)[:at[:2].size]
        out.append(a)
    return tuple(out)


def equal_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def expect_equal(got, want, what=""):
    """pairs of planes, compared bit for bit (None with None)"""
    for f, (g, w) in enumerate(zip(got, want)):
        if g is None or w is None:
            assert g is None and w is None, "%s [%d]: one side is None" % (what, f)
            continue
        if not equal_bits(g, w):
            bad = np.flatnonzero(np.ascontiguousarray(g).reshape(-1).view(np.uint8) != np.ascontiguousarray(w).reshape(-1).view(np.uint8))
            raise AssertionError("%s [%d]: %d bytes differ, the first at %d" % (what, f, bad.size, bad[0] if bad.size else -1))
