"""The spatial augmentation (ofdg_spatial, include/ofdg.h) restated in numpy from the header text, independent of the library:
Philox4x32-10, the draw of a record, its sanitising, the tap, the blend, the flow's transform, the labels and the occlusion
rule - plus the planes and records the CPU and the GPU tests share.  The scalar work of a record (draw, sanitise, inverse)
runs on Python floats, which are IEEE doubles rounded operation by operation; the pixels on float64 / float32 arrays (numpy
fuses nothing).  ofdg_det_exp and ofdg_det_sincos of include/ofdg_detmath.h are restated HERE, on Python floats: no entry
of the library is called.  No GPU."""
import math

import numpy as np

import crop_reference as cr

RANDOM_HFLIP, RANDOM_VFLIP, OCC_WINDOW = 4, 8, 16
PLANES = cr.PLANES
RANGES = ("zoom_log", "rot", "squeeze_log", "translate", "pair_zoom_log", "pair_rot", "pair_translate")
F32 = np.float32
NAN32, NAN16 = 0x7FC00000, 0x7E00
# W, H, out_w, out_h: a window inside the frame, one that is no multiple of 16 wide (units straddle rows) or 4 high, and an
# output larger than the source
SHAPES = [(72, 40, 40, 24), (160, 100, 136, 66), (40, 24, 72, 40)]
GPU_SHAPE = (264, 200, 248, 134)  # tiles partial on both axes, 31 runs of 8 per row
SUBSETS = [PLANES, ("image0", "image1"), ("flow",), ("flow1", "occ1", "label1"), ("occ0", "label0", "image1"), ("label0",)]


# ---- include/ofdg_detmath.h on Python floats -------------------------------------------------------------------------------
def det_exp(x):
    ln2_hi, ln2_lo, inv_ln2, big = 6.93147180369123816490e-01, 1.90821492927058770002e-10, 1.44269504088896338700e+00, 6755399441055744.0
    if x != x:
        return x
    if x > 709.78:
        return math.inf
    if x < -745.2:
        return 0.0
    fk = (x * inv_ln2 + big) - big
    r = (x - fk * ln2_hi) - fk * ln2_lo
    p = 1.0 / 6227020800.0
    for d in (479001600.0, 39916800.0, 3628800.0, 362880.0, 40320.0, 5040.0, 720.0, 120.0, 24.0, 6.0):
        p = p * r + 1.0 / d
    p = p * r + 0.5
    p = p * r + 1.0
    p = p * r + 1.0
    k = int(fk)
    k1 = -((-k) // 2) if k < 0 else k // 2  # C division: towards zero
    return (p * math.ldexp(1.0, k1)) * math.ldexp(1.0, k - k1)


def det_sincos(a):
    invpio2, pio2_1, pio2_2 = 6.36619772367581382433e-01, 1.57079632673412561417e+00, 6.07710050630396597660e-11
    pio2_3, pio2_3t, big = 2.02226624871116645580e-21, 8.47842766036889956997e-32, 6755399441055744.0
    S1, S2, S3 = -1.66666666666666324348e-01, 8.33333333332248946124e-03, -1.98412698298579493134e-04
    S4, S5, S6 = 2.75573137070700676789e-06, -2.50507602534068634195e-08, 1.58969099521155010221e-10
    C1, C2, C3 = 4.16666666666666019037e-02, -1.38888888888741095749e-03, 2.48015872894767294178e-05
    C4, C5, C6 = -2.75573143513906633035e-07, 2.08757232129817482790e-09, -1.13596475577881948265e-11
    if not abs(a) < 823549.6:
        return math.nan, math.nan
    fn = (a * invpio2 + big) - big
    t = a - fn * pio2_1
    w = fn * pio2_2
    r = t - w
    bb = r - t
    e = (t - (r - bb)) + (-w - bb)
    w3 = fn * pio2_3
    y0 = r - w3
    y1 = (((r - y0) - w3) + e) - fn * pio2_3t
    z = y0 * y0
    v = z * y0
    p = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)))
    ks = y0 - ((z * (0.5 * y1 - v * p) - y1) - v * S1)
    ww = z * z
    p = z * (C1 + z * (C2 + z * C3)) + (ww * ww) * (C4 + z * (C5 + z * C6))
    hz = 0.5 * z
    om = 1.0 - hz
    kc = om + (((1.0 - om) - hz) + (z * p - y0 * y1))
    n = int(fn) & 3
    return (ks, kc, -ks, -kc)[n], (kc, -ks, -kc, ks)[n]


# ---- draw ------------------------------------------------------------------------------------------------------------------
def unit(w):
    return F32(int(w) >> 8) * F32(2.0 ** -24)


def sym(w, a):
    r = F32(a) * (F32(2.0) * unit(w) - F32(1.0))
    return F32(0.0) if r == 0 else r


def _pz(x):
    return 0.0 if x == 0 else x


def _linear(lz, th, lq, h, v):
    gx, gy = det_exp(-float(F32(lz) + F32(lq))), det_exp(-float(F32(lz) - F32(lq)))
    s, c = det_sincos(float(th))
    return _pz(c * gx * h), _pz(-(s * gy) * v), _pz(s * gx * h), _pz(c * gy * v)


def draw(seed, index, W, H, out_w, out_h, ranges=None, flags=0, with_slack=False):
    """The drawn record (not sanitised) of global sample `index`: float64 [14]; with_slack: also (slack x, slack y) of frame 0."""
    q = {k: F32((ranges or {}).get(k, 0.0)) for k in RANGES}
    g = index & 0xFFFFFFFFFFFFFFFF
    key = ((seed ^ (((g >> 32) * 0x9E3779B9) & cr.M32)) & cr.M32, g & cr.M32)
    w0, w1, w2 = (cr.philox4x32((j, 0, 0x0C73, 0), key) for j in range(3))
    lz, th, lq = sym(w0[0], q["zoom_log"]), sym(w0[1], q["rot"]), sym(w0[2], q["squeeze_log"])
    h = -1.0 if (flags & RANDOM_HFLIP) and (w0[3] & 1) else 1.0
    v = -1.0 if (flags & RANDOM_VFLIP) and ((w0[3] >> 1) & 1) else 1.0
    tfx, tfy = F32(2.0) * unit(w1[0]) - F32(1.0), F32(2.0) * unit(w1[1]) - F32(1.0)
    dlz, dth = sym(w2[0], q["pair_zoom_log"]), sym(w2[1], q["pair_rot"])
    dtx, dty = sym(w2[2], q["pair_translate"]), sym(w2[3], q["pair_translate"])
    hw, hh = (out_w - 1) / 2.0, (out_h - 1) / 2.0
    a, b, d, e = _linear(lz, th, lq, h, v)
    centre, slack = [], []
    for side, p, r, tf in ((W, a, b, tfx), (H, d, e, tfy)):
        mid = (side - 1) / 2.0
        ex = abs(p) * hw + abs(r) * hh
        s = mid - ex
        s = s if s > 0 else 0.0
        slack.append(s)
        centre.append(mid + (float(tf) * float(q["translate"])) * s)
    rec = np.zeros(14, np.float64)
    rec[0:6] = a, b, centre[0] - (a * hw + b * hh), d, e, centre[1] - (d * hw + e * hh)
    a, b, d, e = _linear(F32(lz) + F32(dlz), F32(th) + F32(dth), lq, h, v)
    rec[6:12] = a, b, (centre[0] + float(dtx)) - (a * hw + b * hh), d, e, (centre[1] + float(dty)) - (d * hw + e * hh)
    return (rec, tuple(slack)) if with_slack else rec


def drawn_records(seed, first_index, n, W, H, out_w, out_h, ranges=None, flags=0):
    return np.stack([draw(seed, first_index + i, W, H, out_w, out_h, ranges, flags) for i in range(n)])


# ---- sanitise, inverse -----------------------------------------------------------------------------------------------------
def _det(m):
    return float(m[0]) * float(m[4]) - float(m[1]) * float(m[3])


def sanitise(rec, W, H, out_w, out_h):
    out = np.zeros(14, np.float64)
    for f in range(2):
        m = [float(v) for v in rec[6 * f:6 * f + 6]]
        ok = all(abs(m[k]) <= 64.0 for k in (0, 1, 3, 4)) and abs(m[2]) <= 2.0 ** 20 and abs(m[5]) <= 2.0 ** 20
        det = abs(_det(m))
        ok = ok and 2.0 ** -12 <= det <= 2.0 ** 12
        out[6 * f:6 * f + 6] = m if ok else [1.0, 0.0, float((W - out_w) // 2), 0.0, 1.0, float((H - out_h) // 2)]
    return out


def sanitise_all(recs, W, H, out_w, out_h):
    return np.stack([sanitise(r, W, H, out_w, out_h) for r in recs])


def inverse(m):
    det = _det(m)
    return float(m[4]) / det, -float(m[1]) / det, -float(m[3]) / det, float(m[0]) / det


# ---- pixels ----------------------------------------------------------------------------------------------------------------
def _fixed(q):
    t = np.floor(q * 256.0 + 0.5)
    return np.clip(t, -2.0 ** 30, 2.0 ** 30).astype(np.int64)


def _quiet32(v):
    v = np.ascontiguousarray(v, np.float32)
    v.view(np.uint32)[np.isnan(v)] = NAN32
    return v


def _store_flow(v, dtype):
    v = _quiet32(v)
    if np.dtype(dtype) == np.float32:
        return v
    with np.errstate(over="ignore"):
        h = v.astype(np.float16)
    h.view(np.uint16)[np.isnan(v)] = NAN16
    return h


def warp_frame(m, other, src, W, H, out_w, out_h, occ_window):
    """The planes of ONE frame of ONE sample: src maps "image" [3,H,W], "flow" [2,H,W], "occ" [H,W], "label" [H,W] (any subset)
    to arrays; m: the frame's own map (six floats), other: the other frame's.  Returns the same keys, out_h x out_w."""
    a, b, c, d, e, g = (float(v) for v in m)
    X = np.arange(out_w, dtype=np.float64)[None, :]
    Y = np.arange(out_h, dtype=np.float64)[:, None]
    qx, qy = ((a * X) + (b * Y)) + c, ((d * X) + (e * Y)) + g
    Qx, Qy = _fixed(qx), _fixed(qy)
    inside = (Qx >= 0) & (Qx <= (W - 1) * 256) & (Qy >= 0) & (Qy <= (H - 1) * 256)
    nx, ny = np.clip((Qx + 128) >> 8, 0, W - 1), np.clip((Qy + 128) >> 8, 0, H - 1)
    out = {}
    if "image" in src:
        fx, fy = Qx & 255, Qy & 255
        x0, x1 = np.clip(Qx >> 8, 0, W - 1), np.clip((Qx >> 8) + 1, 0, W - 1)
        y0, y1 = np.clip(Qy >> 8, 0, H - 1), np.clip((Qy >> 8) + 1, 0, H - 1)
        w00, w10 = ((256 - fx) * (256 - fy)).astype(F32), (fx * (256 - fy)).astype(F32)
        w01, w11 = ((256 - fx) * fy).astype(F32), (fx * fy).astype(F32)
        img = src["image"]
        res = np.zeros((3, out_h, out_w), img.dtype)
        with np.errstate(invalid="ignore", over="ignore"):
            for ch in range(3):
                p = img[ch]
                e00, e10, e01, e11 = (p[yy, xx].astype(F32) for yy, xx in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)))
                v = ((w00 * e00 + w10 * e10) + (w01 * e01 + w11 * e11)) * F32(2.0 ** -16)
                assert v.dtype == np.float32
                if img.dtype == np.float32:
                    res[ch] = _quiet32(v)
                else:
                    v = np.where(v > 0, v, F32(0))
                    v = np.where(v < 255, v, F32(255))
                    res[ch] = np.rint(v).astype(np.uint8)
        out["image"] = res
    px = py = None
    if "flow" in src:
        ia, ib, id_, ie = inverse(other)
        oc, og = float(other[2]), float(other[5])
        with np.errstate(invalid="ignore", over="ignore"):
            u = src["flow"][0][ny, nx].astype(F32).astype(np.float64)
            v = src["flow"][1][ny, nx].astype(F32).astype(np.float64)
            dx, dy = (qx + u) - oc, (qy + v) - og
            px, py = (ia * dx) + (ib * dy), (id_ * dx) + (ie * dy)
            out["flow"] = np.stack([_store_flow((px - X).astype(F32), src["flow"].dtype), _store_flow((py - Y).astype(F32), src["flow"].dtype)])
    if "occ" in src:
        with np.errstate(invalid="ignore"):
            hidden = (src["occ"][ny, nx] != 0) | ~inside
            if occ_window:
                tx, ty = np.floor(px + 0.5), np.floor(py + 0.5)
                hidden |= ~((tx >= 0) & (tx <= out_w - 1) & (ty >= 0) & (ty <= out_h - 1))
        out["occ"] = hidden.astype(src["occ"].dtype)
    if "label" in src:
        out["label"] = src["label"][ny, nx]
    return out


_FRAME_KEYS = (("image", "image0", "image1"), ("flow", "flow", "flow1"), ("occ", "occ0", "occ1"), ("label", "label0", "label1"))


def spatial(src, recs, out_w, out_h, occ_window=False):
    """(dst, sanitised records) of the planes in `src` (name -> array [n,C,H,W], labels [n,H,W]) under recs (float64 [n,14])."""
    first = next(iter(src.values()))
    n, (H, W) = first.shape[0], first.shape[-2:]
    used = np.stack([sanitise(r, W, H, out_w, out_h) for r in recs])
    dst = {name: np.zeros(a.shape[:-2] + (out_h, out_w), a.dtype) for name, a in src.items()}
    for i in range(n):
        for f in range(2):
            mine = {}
            for key, n0, n1 in _FRAME_KEYS:
                name = n1 if f else n0
                if name in src:
                    a = src[name][i]
                    mine[key] = a[0] if key == "occ" and a.ndim == 3 else a
            if not mine:
                continue
            res = warp_frame(used[i, 6 * f:6 * f + 6], used[i, 6 * (1 - f):6 * (1 - f) + 6], mine, W, H, out_w, out_h, occ_window)
            for key, n0, n1 in _FRAME_KEYS:
                if key in res:
                    dst[n1 if f else n0][i] = res[key]
    return dst, used


# ---- planes and records ----------------------------------------------------------------------------------------------------
def _centred(W, H, out_w, out_h, a, b, d, e, sx=0.0, sy=0.0):
    hw, hh = (out_w - 1) / 2.0, (out_h - 1) / 2.0
    return [a, b, (W - 1) / 2.0 + sx - (a * hw + b * hh), d, e, (H - 1) / 2.0 + sy - (d * hw + e * hh)]


def records(W, H, out_w, out_h):
    """The records of the restatement tests, float64 [N,14]: identity, integer and fractional shifts, both flips, rotations
    by 30 and 90 degrees, zoom 0.5 and 2, a squeeze, windows wholly and partly outside the frame, and the sanitise cases (NaN,
    infinite, singular, nearly singular, oversized entries); one carries non-zero reserved bytes."""
    x0, y0 = (W - out_w) // 2, (H - out_h) // 2
    c30, s30 = math.cos(math.pi / 6), math.sin(math.pi / 6)
    c32, s32 = math.cos(0.56), math.sin(0.56)
    ident = [1.0, 0.0, float(x0), 0.0, 1.0, float(y0)]
    rows = [
        ident + ident,
        [1.0, 0.0, 3.0, 0.0, 1.0, 2.0] + [1.0, 0.0, 5.0, 0.0, 1.0, 1.0],
        [1.0, 0.0, 2.37, 0.0, 1.0, 1.62] + [1.0, 0.0, 0.5, 0.0, 1.0, 0.25],
        [-1.0, 0.0, float(x0 + out_w - 1), 0.0, 1.0, float(y0)] * 2,
        [1.0, 0.0, float(x0), 0.0, -1.0, float(y0 + out_h - 1)] * 2,
        [-1.0, 0.0, float(x0 + out_w - 1), 0.0, -1.0, float(y0 + out_h - 1)] + [-1.0, 0.0, float(x0 + out_w), 0.0, -1.0, float(y0 + out_h - 2)],
        _centred(W, H, out_w, out_h, c30, -s30, s30, c30) + _centred(W, H, out_w, out_h, c32, -s32, s32, c32, 1.5, -0.75),
        _centred(W, H, out_w, out_h, 0.0, -1.0, 1.0, 0.0) + _centred(W, H, out_w, out_h, 0.0, -1.0, 1.0, 0.0, 1.0, 0.0),
        _centred(W, H, out_w, out_h, 0.5, 0.0, 0.0, 0.5) + _centred(W, H, out_w, out_h, 0.55, 0.0, 0.0, 0.55),
        _centred(W, H, out_w, out_h, 2.0, 0.0, 0.0, 2.0) + _centred(W, H, out_w, out_h, 2.0, 0.0, 0.0, 1.9),
        _centred(W, H, out_w, out_h, 1.25, 0.0, 0.0, 0.8) + _centred(W, H, out_w, out_h, 1.25, 0.03, -0.02, 0.8),
        [1.0, 0.0, float(W + 10), 0.0, 1.0, float(-H - out_h - 3)] + [1.0, 0.0, -1.0e5, 0.0, 1.0, 3.0e5],          # wholly outside
        [1.0, 0.0, -out_w / 2.0 + 0.3, 0.0, 1.0, H - out_h / 2.0] + _centred(W, H, out_w, out_h, c30, s30, -s30, c30, W / 2.0, 0.0),  # partly
        [math.nan, 0.0, 1.0, 0.0, 1.0, 1.0] + _centred(W, H, out_w, out_h, c30, -s30, s30, c30),
        _centred(W, H, out_w, out_h, 0.9, 0.0, 0.0, 0.9) + [1.0, 0.0, math.inf, 0.0, 1.0, 0.0],
        [0.5, 0.5, 3.0, 0.5, 0.5, 2.0] + [2.0 ** -7, 0.0, 3.0, 0.0, 2.0 ** -7, 2.0],                                # singular, |det| = 2^-14
        [65.0, 0.0, 3.0, 0.0, 1.0, 2.0] + [1.0, 0.0, 2.0 ** 20 + 1.0, 0.0, 1.0, 2.0],                               # oversized
        [64.0, 0.0, -3.0, 0.0, 64.0, 2.0] + [1.0, 0.0, -2.0 ** 20, 0.0, 1.0, 2.0 ** 20],                            # the bounds themselves, kept
    ]
    recs = np.zeros((len(rows), 14), np.float64)
    recs[:, :12] = rows
    recs[5, 12:].view(np.int32)[:] = [77, -1, 5, 1 << 30]
    return recs


N = 18
_planes = {}


def planes(W, H, image="float32", flow="float32", occ="float32", n=N):
    """The eight planes of n samples: those of the crop's tests (frames that encode their position, flows with NaN, +-inf and
    -0.0 planted all over, maps with values other than 1), and on top of them float32 frames with fractions and byte-like
    samples, and float32 maps with NaN and -0.0 elements."""
    key = (W, H, image, flow, occ, n)
    if key not in _planes:
        src = {k: np.array(v) for k, v in cr.planes(W, H, image, flow, occ, n).items()}
        if image == "float32":
            for k, name in enumerate(("image0", "image1")):
                src[name][1::3] = (src[name][1::3] % 256).astype(np.float32)          # byte values
                src[name][2::3] = src[name][2::3] * np.float32(0.37) - np.float32(1000.5 + k)  # fractions, negative ones too
        if occ == "float32":
            for name in ("occ0", "occ1"):
                flat = src[name].reshape(-1)
                flat[5::97] = np.nan
                flat[11::89] = -0.0
        for a in src.values():
            a.setflags(write=False)
        _planes[key] = src
    return _planes[key]


expect_equal = cr.expect_equal
