"""The lens (ofdg_lens, include/ofdg.h) restated in numpy from the header text, independent of the library: the draw of a
record, its sanitising, the forward map, the taps, the frames with their fringes and vignette, the eight Newton steps of the
flow's inverse with their verdict, the labels and the occlusion rule - plus the planes and records the CPU and the GPU tests
share.  The scalar work of a record runs on Python floats, which are IEEE doubles rounded operation by operation; the pixels
on float64 / float32 arrays, one numpy operation per stated rounding (numpy fuses nothing).  The taps are the spatial
augmentation's, so its restatement's helpers (the 24.8 fixed point, the stores) are used as they are; Philox is the crop's.
No entry of the library is called.  No GPU."""
import numpy as np

import crop_reference as cr
import spatial_reference as sr

FILL, OCC_WINDOW = 1, 16
PLANES = cr.PLANES
RANGES = ("prob", "k1_range", "ca_range", "vig_max", "centre")
F32 = np.float32
SIZES = [(8, 2), (24, 10), (40, 26), (72, 34)]  # W, H
GPU_SIZES = SIZES + [(136, 18)]                 # several tiles across, an odd count of row pairs down
N = 3
SUBSETS = [PLANES] + [(name,) for name in PLANES]


# ---- a record ----------------------------------------------------------------------------------------------------------------
def half(W, H):
    return (W - 1) / 2.0, (H - 1) / 2.0


def inv_diag2(W, H):
    hw, hh = half(W, H)
    return 1.0 / ((hw * hw) + (hh * hh))


def identity(W, H):
    hw, hh = half(W, H)
    return np.array([0.0, 1.0, 0.0, 0.0, 0.0, hw, hh, 0.0], np.float64)


def _rho(dx, dy, inv):
    return ((dx * dx) + (dy * dy)) * inv


def draw(seed, index, W, H, ranges=None, flags=0):
    """The drawn record (not sanitised) of global sample `index`: float64 [8]."""
    q = {k: F32((ranges or {}).get(k, 0.0)) for k in RANGES}
    g = index & 0xFFFFFFFFFFFFFFFF
    key = ((seed ^ (((g >> 32) * 0x9E3779B9) & cr.M32)) & cr.M32, g & cr.M32)
    w0, w1 = (cr.philox4x32((j, 0, 0x0C7A, 0), key) for j in range(2))
    if not sr.unit(w0[0]) < q["prob"]:
        return identity(W, H)
    k1, ca_b, ca_r = (float(sr.sym(w0[k], q[name])) for k, name in ((1, "k1_range"), (2, "ca_range"), (3, "ca_range")))
    vig = float(sr.unit(w1[0]) * q["vig_max"])
    ox, oy = float(sr.sym(w1[1], q["centre"])), float(sr.sym(w1[2], q["centre"]))
    hw, hh = half(W, H)
    cx, cy = hw + (ox * hw), hh + (oy * hh)
    z = 1.0
    if flags & FILL:
        inv = inv_diag2(W, H)
        rc = max(_rho(X - cx, Y - cy, inv) for X in (0.0, float(W - 1)) for Y in (0.0, float(H - 1)))
        Lc = 1.0 + (k1 * rc)
        z = 1.0 / Lc if Lc > 1.0 else 1.0
    return np.array([k1, z, ca_b, ca_r, vig, cx, cy, 0.0], np.float64)


def drawn_records(seed, first_index, n, W, H, ranges=None, flags=0):
    return np.stack([draw(seed, first_index + i, W, H, ranges, flags) for i in range(n)])


def sanitise(rec, W, H):
    k1, z, ca_b, ca_r, vig, cx, cy = (float(v) for v in rec[:7])
    hw, hh = half(W, H)
    ok = all(np.isfinite([k1, z, ca_b, ca_r, vig, cx, cy]))
    ok = ok and abs(k1) <= 0.125 and 0.5 <= z <= 2.0 and abs(ca_b) <= 1.0 / 64 and abs(ca_r) <= 1.0 / 64 and 0.0 <= vig <= 0.5
    ok = ok and abs(cx - hw) <= hw / 4.0 and abs(cy - hh) <= hh / 4.0
    return np.array([k1, z, ca_b, ca_r, vig, cx, cy, 0.0], np.float64) if ok else identity(W, H)


# ---- pixels ------------------------------------------------------------------------------------------------------------------
def forward(rec, W, H, X, Y, m=None):
    """(qx, qy, rho) of destination positions X, Y (float64 arrays) under magnification m (default: z, the geometric map S)."""
    k1, z, cx, cy = float(rec[0]), float(rec[1]), float(rec[5]), float(rec[6])
    m = z if m is None else m
    dx, dy = X - cx, Y - cy
    rho = _rho(dx, dy, inv_diag2(W, H))
    L = 1.0 + (k1 * rho)
    return cx + ((m * L) * dx), cy + ((m * L) * dy), rho


def inverse(rec, W, H, tx, ty):
    """(px, py, solved) of targets tx, ty (float64 arrays): the eight Newton steps and their verdict."""
    k1, z, cx, cy = float(rec[0]), float(rec[1]), float(rec[5]), float(rec[6])
    with np.errstate(all="ignore"):
        dtx, dty = tx - cx, ty - cy
        s = np.full(np.shape(tx), 1.0 / z)
        solved = np.ones(np.shape(tx), bool)
        if k1 != 0.0:
            ru = _rho(dtx, dty, inv_diag2(W, H))
            k3 = 3.0 * k1

            def residual(s):
                a = (ru * s) * s
                return ((z * s) * (1.0 + (k1 * a))) - 1.0, 1.0 + (k3 * a)

            for _ in range(8):
                g, D = residual(s)
                s = s - (g / (z * D))
            g, D = residual(s)
            solved = (ru <= 16.0) & (np.abs(g) <= 2.0 ** -30) & (D >= 0.25) & (s > 0.0)
        return cx + (s * dtx), cy + (s * dty), solved


def _taps(qx, qy, W, H):
    Qx, Qy = sr._fixed(qx), sr._fixed(qy)
    return Qx, Qy


def bend_frame(rec, src, W, H, occ_window):
    """The planes of ONE frame of ONE sample under a sanitised record: src maps "image" [3,H,W], "flow" [2,H,W], "occ" [H,W],
    "label" [H,W] (any subset) to arrays.  Returns the same keys, and "solved" [H,W] when there is a flow."""
    k1, z, ca_b, ca_r, vig = (float(v) for v in rec[:5])
    X = np.arange(W, dtype=np.float64)[None, :] + np.zeros((H, 1))
    Y = np.arange(H, dtype=np.float64)[:, None] + np.zeros((1, W))
    qx, qy, rho = forward(rec, W, H, X, Y)
    Qx, Qy = _taps(qx, qy, W, H)
    inside = (Qx >= 0) & (Qx <= (W - 1) * 256) & (Qy >= 0) & (Qy <= (H - 1) * 256)
    nx, ny = np.clip((Qx + 128) >> 8, 0, W - 1), np.clip((Qy + 128) >> 8, 0, H - 1)
    out = {}
    if "image" in src:
        img = src["image"]
        res = np.zeros((3, H, W), img.dtype)
        gain = (1.0 - (vig * rho)).astype(F32)
        with np.errstate(invalid="ignore", over="ignore"):
            for ch, ca in enumerate((ca_b, 0.0, ca_r)):
                zc = z * (1.0 + ca)
                cqx, cqy, _ = forward(rec, W, H, X, Y, zc)
                Cx, Cy = _taps(cqx, cqy, W, H)
                fx, fy = Cx & 255, Cy & 255
                x0, x1 = np.clip(Cx >> 8, 0, W - 1), np.clip((Cx >> 8) + 1, 0, W - 1)
                y0, y1 = np.clip(Cy >> 8, 0, H - 1), np.clip((Cy >> 8) + 1, 0, H - 1)
                w00, w10 = ((256 - fx) * (256 - fy)).astype(F32), (fx * (256 - fy)).astype(F32)
                w01, w11 = ((256 - fx) * fy).astype(F32), (fx * fy).astype(F32)
                p = img[ch]
                e00, e10, e01, e11 = (p[yy, xx].astype(F32) for yy, xx in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)))
                v = ((w00 * e00 + w10 * e10) + (w01 * e01 + w11 * e11)) * F32(2.0 ** -16)
                if vig != 0.0:
                    v = v * gain
                assert v.dtype == np.float32
                if img.dtype == np.float32:
                    res[ch] = sr._quiet32(v)
                else:
                    v = np.where(v > 0, v, F32(0))
                    v = np.where(v < 255, v, F32(255))
                    res[ch] = np.rint(v).astype(np.uint8)
        out["image"] = res
    px = py = None
    solved = np.ones((H, W), bool)
    if "flow" in src:
        with np.errstate(invalid="ignore", over="ignore"):
            u = src["flow"][0][ny, nx].astype(F32).astype(np.float64)
            v = src["flow"][1][ny, nx].astype(F32).astype(np.float64)
            px, py, solved = inverse(rec, W, H, qx + u, qy + v)
            fu = np.where(solved, (px - X).astype(F32), F32(np.nan))
            fv = np.where(solved, (py - Y).astype(F32), F32(np.nan))
        out["flow"] = np.stack([sr._store_flow(fu, src["flow"].dtype), sr._store_flow(fv, src["flow"].dtype)])
        out["solved"] = solved
    if "occ" in src:
        with np.errstate(invalid="ignore"):
            hidden = (src["occ"][ny, nx] != 0) | ~inside | ~solved
            if occ_window:
                tx, ty = np.floor(px + 0.5), np.floor(py + 0.5)
                hidden |= ~((tx >= 0) & (tx <= W - 1) & (ty >= 0) & (ty <= H - 1))
        out["occ"] = hidden.astype(src["occ"].dtype)
    if "label" in src:
        out["label"] = src["label"][ny, nx]
    out["inside"] = inside
    return out


_FRAME_KEYS = (("image", "image0", "image1"), ("flow", "flow", "flow1"), ("occ", "occ0", "occ1"), ("label", "label0", "label1"))


def lens(src, recs, occ_window=False, extra=None):
    """(dst, sanitised records) of the planes in `src` (name -> array [n,C,H,W], labels [n,H,W]) under recs (float64 [n,8]).
    extra: a dict that receives "inside" and "solved0" / "solved1" as bool [n,H,W]."""
    first = next(iter(src.values()))
    n, (H, W) = first.shape[0], first.shape[-2:]
    used = np.stack([sanitise(r, W, H) for r in recs])
    dst = {name: np.zeros(a.shape, a.dtype) for name, a in src.items()}
    if extra is not None:
        extra.update(inside=np.zeros((n, H, W), bool), solved0=np.ones((n, H, W), bool), solved1=np.ones((n, H, W), bool))
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
            res = bend_frame(used[i], mine, W, H, occ_window)
            for key, n0, n1 in _FRAME_KEYS:
                if key in res:
                    dst[n1 if f else n0][i] = res[key]
            if extra is not None:
                extra["inside"][i] = res["inside"]
                if "solved" in res:
                    extra["solved%d" % f][i] = res["solved"]
    return dst, used


# ---- planes and records ------------------------------------------------------------------------------------------------------
_planes = {}


def planes(W, H, image="float32", flow="float32", occ="float32", n=N):
    """The eight planes of n samples from a seeded generator: byte-valued frames, flows with zeros, sub-pixel values, targets
    outside the frame, one NaN and one 1e30 per plane, maps that are non-zero in places (values other than 1 among them),
    labels."""
    key = (W, H, image, flow, occ, n)
    if key in _planes:
        return _planes[key]
    rng = np.random.default_rng(20240607 + W * 131 + H)
    src = {}
    for name in ("image0", "image1"):
        src[name] = rng.integers(0, 256, (n, 3, H, W)).astype(image)
    for name in ("flow", "flow1"):
        kind = rng.integers(0, 4, (n, 1, H, W))
        f = np.where(kind == 0, 0.0, np.where(kind == 1, rng.uniform(-1, 1, (n, 2, H, W)),
                     np.where(kind == 2, rng.uniform(-6, 6, (n, 2, H, W)), rng.uniform(-1.5, 1.5, (n, 2, H, W)) * (W + H))))
        f = f.astype(np.float32)
        f[0, 0, H // 2, W // 2] = np.nan
        f[n - 1, 1, 0, 1] = 1e30
        with np.errstate(over="ignore"):
            src[name] = f.astype(flow)
    for name in ("occ0", "occ1"):
        o = rng.integers(0, 6, (n, 1, H, W))
        src[name] = np.where(o == 0, 1, np.where(o == 1, 3, 0)).astype(occ)
    for name in ("label0", "label1"):
        src[name] = rng.integers(0, 251, (n, H, W)).astype(np.uint8)
    for a in src.values():
        a.setflags(write=False)
    _planes[key] = src
    return src


K1S = (-0.125, -0.03, 0.0, 0.04, 0.125)


def records(W, H, fill):
    """The records of the restatement tests, float64 [15,8]: every k1 of K1S plain, with an off-centre centre, and with fringes
    and a vignette on top; fill: z as OFDG_LENS_FILL would draw it."""
    hw, hh = half(W, H)
    inv = inv_diag2(W, H)
    rows = []
    for k1 in K1S:
        for cx, cy, ca_b, ca_r, vig in ((hw, hh, 0.0, 0.0, 0.0), (hw + hw / 5, hh - hh / 4, 0.0, 0.0, 0.0),
                                        (hw - hw / 8, hh + hh / 7, 0.01, -1.0 / 64, 0.3)):
            z = 1.0
            if fill:
                rc = max(_rho(X - cx, Y - cy, inv) for X in (0.0, float(W - 1)) for Y in (0.0, float(H - 1)))
                Lc = 1.0 + (k1 * rc)
                z = 1.0 / Lc if Lc > 1.0 else 1.0
            rows.append([k1, z, ca_b, ca_r, vig, cx, cy, 0.0])
    return np.array(rows, np.float64)


expect_equal = cr.expect_equal
