"""The definition of the splat (ofdg_splat, include/ofdg.h) restated in numpy from the header text, steps 1 to 6: float32
arrays whose every operation is one IEEE rounding up to the 24.8 displacement, int64 arrays behind it, np.maximum.at for the
scatter.  The displacement is ofdg_reproject's step 2 and the byte of a float32 element ofdg_photo's, so both are taken from
their restatements (tests/reproject_reference.py, tests/photo_reference.py).  No GPU, no library call: the draw takes the Philox
block function as an argument."""
import functools

import numpy as np

import photo_reference as pr
import reproject_reference as rr

F32 = np.float32
SIZES = [(8, 2), (24, 6), (72, 40), (264, 200)]  # W, H: the tile is 64 x 16, a lane holds 4 pixels, a uint8 store 8
FORMATS = [(s, d, f) for s in ("float32", "uint8") for d in ("float32", "uint8") for f in ("float32", "float16")]  # frames, image, both flows
TS = (0, 1, 77, 128, 255, 256)
PLANES = ("image", "to_own", "to_other", "mask", "fate")
N = 3
M = (1 << 24) - 1
FIELDS = ("n_bad", "n_outside", "n_inside", "n_filled", "n_holes", "n_covered", "n_covered_visible", "n_covered_hidden", "n_hole_other_visible",
          "n_hole_other_hidden", "t_q8", "reserved")
COUNTS = FIELDS[:-2]
ROW_DTYPE = np.dtype([(k, "<u4", (5,) if k == "reserved" else ()) for k in FIELDS])
expect_equal, equal_bits = pr.expect_equal, pr.equal_bits


def key(name, f):
    return "%s%d" % (name, f)


# ---- the definition --------------------------------------------------------------------------------------------------------
def draw(seed, g, t_min_q8, t_max_q8, philox):
    """step 1: the record [t, 256 - t, 0, 0] of global index g; philox(counter, key) -> 4 words"""
    w = philox((0, 0, 0x0C77, 0), ((seed ^ (((g >> 32) * 0x9E3779B9) & 0xFFFFFFFF)) & 0xFFFFFFFF, g & 0xFFFFFFFF))
    t = t_min_q8 + ((int(w[0]) * (t_max_q8 - t_min_q8 + 1)) >> 32)
    return [t, 256 - t, 0, 0]


def sanitise(rec):
    """step 2"""
    return [min(max(int(rec[0]), 0), 256), min(max(int(rec[1]), 0), 256), 0, 0]


def aim(flow, T):
    """steps 3a to 3d of one sample's frame: (bad, inside, Dx, Dy, rx, ry), [H,W] each"""
    _, H, W = flow.shape
    u, v = flow[0].astype(np.float32), flow[1].astype(np.float32)
    bad = ~(np.isfinite(u) & np.isfinite(v))
    Dx, Dy = rr.q8(u), rr.q8(v)
    y, x = np.mgrid[0:H, 0:W]
    Sx, Sy = (Dx * T + 128) >> 8, (Dy * T + 128) >> 8
    rx, ry = (256 * x + Sx + 128) >> 8, (256 * y + Sy + 128) >> 8
    inside = ~bad & (rx >= 0) & (rx < W) & (ry >= 0) & (ry < H)
    return bad, inside, Dx, Dy, rx, ry


def splat_frame(img, flow, label, occ_own, occ_other, T):
    """One sample, one frame: img [3,H,W] uint8 / float32 or None, flow [2,H,W], label [H,W] uint8 or None, occ_own / occ_other
    [1,H,W] or None, T the sanitised fraction.  Returns (planes, keys, row): planes a dict - "image" int64 [3,H,W], "to_own",
    "to_other" float32 [2,H,W], "mask", "fate" int64 [1,H,W] -, keys uint32 [H,W], row a dict of the block's fields."""
    _, H, W = flow.shape
    bad, inside, Dx, Dy, rx, ry = aim(flow, T)
    y, x = np.mgrid[0:H, 0:W]
    L = np.zeros((H, W), np.int64) if label is None else label.astype(np.int64)
    own_key = (L << 24) | (M - (y * W + x))
    assert (own_key > 0).all()
    keys = np.zeros(H * W, np.int64)
    tgt = (ry * W + rx)[inside]
    np.maximum.at(keys, tgt, own_key[inside])                       # step 3f
    K = keys.reshape(H, W)
    filled = K != 0
    s = np.where(filled, M - (K & M), 0)
    sy, sx = s // W, s % W
    image = np.zeros((3, H, W), np.int64)
    if img is not None:
        image = np.where(filled, pr.index_of(img).astype(np.int64)[:, sy, sx], 0)
    dx, dy = sx - x, sy - y
    zero = F32(0.0)
    to_own = np.stack([np.where(filled, dx.astype(np.float32), zero), np.where(filled, dy.astype(np.float32), zero)]).astype(np.float32)
    ox = ((256 * dx + Dx[sy, sx]).astype(np.float32) * F32(2.0 ** -8)).astype(np.float32)
    oy = ((256 * dy + Dy[sy, sx]).astype(np.float32) * F32(2.0 ** -8)).astype(np.float32)
    to_other = np.stack([np.where(filled, ox, zero), np.where(filled, oy, zero)]).astype(np.float32)
    shown = np.zeros((H, W), bool)
    shown[inside] = keys[tgt] == own_key[inside]                    # step 5
    covered = inside & ~shown
    fate = np.where(bad, 3, np.where(~inside, 2, np.where(covered, 1, 0)))
    row = {k: 0 for k in COUNTS}
    row["n_bad"], row["n_outside"], row["n_inside"] = int(bad.sum()), int((~bad & ~inside).sum()), int(inside.sum())
    row["n_filled"], row["n_holes"], row["n_covered"] = int(filled.sum()), int((~filled).sum()), int(covered.sum())
    if occ_own is not None:
        hid = occ_own[0] != 0
        row["n_covered_visible"], row["n_covered_hidden"] = int((covered & ~hid).sum()), int((covered & hid).sum())
    if occ_other is not None:
        hid = occ_other[0] != 0
        row["n_hole_other_visible"], row["n_hole_other_hidden"] = int((~filled & ~hid).sum()), int((~filled & hid).sum())
    row["t_q8"] = int(T)
    return {"image": image, "to_own": to_own, "to_other": to_other, "mask": filled.astype(np.int64)[None], "fate": fate[None]}, K.astype(np.uint32), row


def splat(images, flows, labels=None, occ=None, recs=None, frames=(0, 1), dst_dtype="float32", oflow_dtype="float32"):
    """(planes by name for every frame of `frames`, keys pair, rows structured [n,2]) of images = (image0, image1) or None, flows
    = (flow, flow1), labels = (label0, label1) or None, occ = (occ0, occ1) or None, any member None; recs [n][2]: t_q8 per
    sample and frame, sanitised here."""
    images, labels, occ = ((None, None) if pair is None else pair for pair in (images, labels, occ))
    n, _, H, W = next(t for t in flows if t is not None).shape
    rows = np.zeros((n, 2), ROW_DTYPE)
    out, keys = {}, [None, None]
    for f in frames:
        kinds = {"image": (3, dst_dtype), "to_own": (2, oflow_dtype), "to_other": (2, oflow_dtype), "mask": (1, np.uint8), "fate": (1, np.uint8)}
        for name, (ch, dt) in kinds.items():
            out[key(name, f)] = np.zeros((n, ch, H, W), dt)
        keys[f] = np.zeros((n, H, W), np.uint32)
        for i in range(n):
            pick = lambda t: None if t is None else t[i]  # noqa: E731
            planes, keys[f][i], row = splat_frame(pick(images[f]), flows[f][i], pick(labels[f]), pick(occ[f]), pick(occ[1 - f]), sanitise(recs[i])[f])
            with np.errstate(over="ignore"):
                for name in PLANES:
                    out[key(name, f)][i] = planes[name].astype(kinds[name][1])
            for k, val in row.items():
                rows[i, f][k] = val
    return out, tuple(keys), rows


def add_rows(a, b):
    """what OFDG_SPLAT_ACCUMULATE makes of rows a when b is reduced on top: the counts added, t_q8 overwritten"""
    out = a.copy()
    for k in COUNTS:
        out[k] = a[k] + b[k]
    out["t_q8"] = b["t_q8"]
    return out


def recs_of(T, n=N):
    """frame 0 goes forward by T, frame 1 comes back by the rest"""
    return np.array([[T, 256 - T, 0, 0]] * n, np.int32)


# ---- test data -------------------------------------------------------------------------------------------------------------
def frames(W, H, dtype="uint8", n=N, seed=1):
    """(image0, image1) [n,3,H,W]: photo_reference's - every byte value; float32 with fractions, NaN, -3, 255.5, 1e9, infinities"""
    return pr.frames(W, H, dtype, n=n, seed=seed)


maps = rr.maps
_SPECIAL = [np.nan, np.inf, -np.inf, -0.0, 1e-40, 5.0e6, -5.0e6, 65504.0, -65504.0, 3.0e38, -3.0e38]
_SMALL = [0.001953125, 0.005859375, -0.001953125, 0.01171875, -0.01171875, 0.00390625, -0.00390625, 1.0, -1.0, 1.5, -1.5, 0.5, -0.5]
LABELS = (0, 3, 7, 255)


def flows_and_labels(W, H, dtype="float32", n=N):
    """((flow, flow1) [n,2,H,W], (label0, label1) uint8 [n,H,W]).  Regions that do not fit a small plane are clipped away.
    Sample 0, targets that stay in their tile: still pixels of label 1; a zoom-out by 2 around (10, 6) (four sources a target,
    equal labels: the index decides); a stretch by 2 from column 2 that leaves every second column empty; a band of label 5
    that moves 4 px down onto a still band of label 9 (the higher label keeps the pixel against the lower source index), a
    band of label 9 that moves down onto a still band of label 5 (the reverse arrangement: the higher label arrives with the
    lower index), a band of label 255 that moves onto label 9; columns of _SMALL: +-1 and +-1.5 px, whose 24.8 value ends in .5
    px at T = 128 and T = 256, and ties of rintf at u 256 = 0.5, 1.5, -0.5, 3, -3.  Sample 1, sprayed: every pixel's target at
    T = 256 is a hashed pixel of the whole plane, labels hashed among LABELS, special values at every 7th element.  Sample 2:
    reproject_reference's blocks with column 0 / W - 1 and row 0 / H - 1 aimed at -1, 0, W - 1 and W (H) exactly at the rounding
    boundary, specials at every 11th element, labels in blocks.  Frame 1 holds the same with the signs turned."""
    base = rr.flows(W, H, "float32", n=n)
    y, x = np.mgrid[0:H, 0:W]
    spec = np.array(_SPECIAL, np.float32)
    fl, lab = [], []
    for f in range(2):
        a = np.array(base[f], np.float32)
        b = np.zeros((n, H, W), np.uint8)
        sign = F32(1.0 if f == 0 else -1.0)
        a[0] = 0.0
        b[0] = 1
        a[0, 0, 2:10, 2:18], a[0, 1, 2:10, 2:18] = (-(x - 10) * F32(0.5))[2:10, 2:18], (-(y - 6) * F32(0.5))[2:10, 2:18]
        a[0, 0, 12:18, 2:14] = ((x - 2) * F32(1.0))[12:18, 2:14]
        for (y0, xs, moving, still) in ((20, slice(2, 20), 5, 9), (30, slice(2, 20), 9, 5), (20, slice(22, 30), 255, 9)):
            a[0, 1, y0:y0 + 4, xs] = 4.0
            b[0, y0:y0 + 4, xs], b[0, y0 + 4:y0 + 8, xs] = moving, still
        for k, val in enumerate(_SMALL):
            a[0, 0, 2:10, 40 + k:41 + k] = val
            a[0, 1, 10:12, 40 + k:41 + k] = val
        a[0] *= sign
        tx, ty = (x * 7 + y * 13 + 3 + f) % W, (x * 5 + y * 11 + 1 + f) % H
        a[1, 0], a[1, 1] = (tx - x) + F32(0.37), (ty - y) - F32(0.21)
        flat = a[1].reshape(-1)
        at = np.arange(3, flat.size, 7)
        flat[at] = spec[np.arange(at.size) % len(spec)]
        b[1] = np.array(LABELS, np.uint8)[(x * 3 + y * 5 + (x * y) % 7 + f) % len(LABELS)]
        b[2] = ((x // 5 + 2 * (y // 3) + f) % 6).astype(np.uint8) * 40
        with np.errstate(over="ignore"):
            fl.append(a.astype(dtype))
        lab.append(b)
    return tuple(fl), tuple(lab)


@functools.lru_cache(maxsize=None)
def inputs(W, H, src_dtype, flow_dtype, occ_dtype="uint8"):
    images, (fl, lab), occ = frames(W, H, src_dtype), flows_and_labels(W, H, flow_dtype), maps(W, H, occ_dtype)
    for t in images + fl + lab + occ:
        t.setflags(write=False)
    return images, fl, lab, occ


@functools.lru_cache(maxsize=None)
def case(W, H, src_dtype, flow_dtype, occ_dtype="uint8", T=256):
    """(images, flows, labels, occ, recs, {(dst dtype, oflow dtype): planes by name}, keys, rows) of one cell of the grid, both
    frames, frame 0 at T and frame 1 at 256 - T, computed once; read only"""
    images, fl, lab, occ = inputs(W, H, src_dtype, flow_dtype, occ_dtype)
    recs = recs_of(T)
    want, keys, rows = splat(images, fl, lab, occ, recs, (0, 1), "float32", "float32")
    forms = {}
    with np.errstate(over="ignore"):
        for d in ("float32", "uint8"):
            for o in ("float32", "float16"):
                forms[d, o] = {k: (v.astype(d) if k.startswith("image") else v.astype(o) if k.startswith("to_") else v) for k, v in want.items()}
    for t in tuple(keys) + (rows, recs) + tuple(v for form in forms.values() for v in form.values()):
        t.setflags(write=False)
    return images, fl, lab, occ, recs, forms, keys, rows


def losers(flow, label, keys, T):
    """Of one sample's frame, per covered source: (winner's label, own label, winner's index, own index, target index), int64
    arrays - what the tie-break cases are asserted on."""
    _, H, W = flow.shape
    bad, inside, _, _, rx, ry = aim(flow, T)
    y, x = np.mgrid[0:H, 0:W]
    idx = y * W + x
    K = keys.astype(np.int64)[np.clip(ry, 0, H - 1), np.clip(rx, 0, W - 1)]
    L = label.astype(np.int64)
    lost = inside & (K != ((L << 24) | (M - idx)))
    return (K >> 24)[lost], L[lost], (M - (K & M))[lost], idx[lost], (ry * W + rx)[lost]


oracle_planes = rr.oracle_planes
PROPERTY_INPUTS = rr.PROPERTY_INPUTS
