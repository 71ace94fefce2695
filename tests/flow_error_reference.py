"""Two independent restatements of the flow error (ofdg_flow_error, include/ofdg.h), shared by tests/test_flow_error.py and
tests/test_gpu_flow_error.py: flow_error() is the integer definition in numpy - no ctypes -, float_metrics() the published
metrics in float64: the end-point error, KITTI's Fl rule (E > 3 px and E / |gt| > 5 %) and the KITTI devkit's colour rule
(min(E / 3, 20 E / |gt|) against the edges 1/16 ... 16).  Also the test inputs, maps and sizes."""
import functools
import math

import numpy as np

N = 4
ALL_BAD_GT, EST_IS_GT = 1, 2   # samples of inputs(): every gt pixel unusable; the estimate equals the ground truth
SIZES = [(8, 2), (24, 6), (72, 40), (264, 200)]
CELL = np.dtype([("sum_epe_q8", "<u8"), ("n", "<u4"), ("n_1px", "<u4"), ("n_3px", "<u4"), ("n_5px", "<u4"), ("n_fl", "<u4"), ("reserved", "<u4")])
ROW = np.dtype([("cell", CELL, (2, 3, 3)), ("hist", "<u4", (16,)), ("max_key", "<u8"), ("n_bad_gt", "<u4"), ("n_bad_est", "<u4"), ("reserved", "<u4", (4,))])
COLOURS = np.array([(49, 54, 149), (69, 117, 180), (116, 173, 209), (171, 217, 233), (224, 243, 248), (254, 224, 144), (253, 174, 97), (244, 109, 67),
                    (215, 48, 39), (165, 0, 38)], np.int64)   # (R, G, B) of bins 0..9
# gt, est -> (Eq, colour bin, in n_3px, in n_fl), est_scale 1
KNOWN = [((10, 0), (10, 0), 0, 0, False, False), ((0, 0), (3, 0), 768, 5, False, False), ((100, 0), (104, 0), 1024, 4, True, False),
         ((100, 0), (106, 0), 1536, 5, True, True)]
BIG = np.float32(1048576.0)
COUNTS = ("n", "n_1px", "n_3px", "n_5px", "n_fl")


def isqrt(x):
    """floor(sqrt(x)) of an int64 array, 0 <= x < 2^60: the float64 root, then one exact step either way"""
    x = np.asarray(x, np.int64)
    r = np.floor(np.sqrt(x.astype(np.float64))).astype(np.int64)
    r = r - (r * r > x)
    return r + ((r + 1) * (r + 1) <= x)


def isqrt_python(x):
    return np.array([math.isqrt(int(v)) for v in np.asarray(x).reshape(-1)], np.int64).reshape(np.shape(x))


def to_bf16_bits(a):
    """float32 -> bfloat16 bit patterns (uint16), to nearest even; a NaN stays a NaN"""
    bits = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    rounded = ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(a), np.uint16(0x7FC0), rounded)


def widen(a):
    """a plane as float32: float32 and float16 by value, uint16 as bfloat16 bit patterns"""
    a = np.asarray(a)
    if a.dtype == np.uint16:
        return (a.astype(np.uint32) << 16).view(np.float32)
    return a.astype(np.float32)


def pixels(gt, est, est_scale=1.0):
    """Steps 1 to 5: (bad_gt, bad_est, Eq, Gq) as [n,H,W] arrays; Eq and Gq are 0 where the pixel is unusable"""
    g, e = widen(gt), widen(est)
    with np.errstate(invalid="ignore", over="ignore"):
        e = (e * np.float32(est_scale)).astype(np.float32)
        gt_ok = (np.abs(g[:, 0]) < BIG) & (np.abs(g[:, 1]) < BIG)
        est_ok = (np.abs(e[:, 0]) < BIG) & (np.abs(e[:, 1]) < BIG)
    ok = gt_ok & est_ok

    def q8(a):
        return np.rint(np.where(ok, a, 0).astype(np.float32) * np.float32(256.0)).astype(np.int64)

    Ug, Vg, Ue, Ve = q8(g[:, 0]), q8(g[:, 1]), q8(e[:, 0]), q8(e[:, 1])
    return ~gt_ok, gt_ok & ~est_ok, isqrt((Ue - Ug) ** 2 + (Ve - Vg) ** 2), isqrt(Ug * Ug + Vg * Vg)


def colour_bin(Eq, Gq):
    return sum(((Eq >= (48 << j)) & (320 * Eq >= (Gq << j))).astype(np.int64) for j in range(9))


def hist_bin(Eq):
    return sum((Eq >= (16 << k)).astype(np.int64) for k in range(15))


def flow_error(gt, est, occ=None, dist2=None, outputs=("rows",), epe_dtype=np.float32, est_scale=1.0, speed_px=(10, 40), dist2_edges=(26, 101),
               layout="planar_bgr", dim_occ=False, one_row=False, px=None):
    """The dict of rows (ROW, zeroed first), epe and picture by steps 1 to 10 of the definition; px: pixels() of the same gt,
    est and est_scale, when the caller has it already"""
    bad_gt, bad_est, Eq, Gq = pixels(gt, est, est_scale) if px is None else px
    n, H, W = Eq.shape
    ok = ~(bad_gt | bad_est)
    if occ is None:
        hidden = np.zeros((n, H, W), bool)
    else:
        with np.errstate(invalid="ignore"):
            hidden = np.asarray(occ)[:, 0] != 0
    out = {}
    if "rows" in outputs:
        S = [int(np.rint(np.float32(s) * np.float32(256.0))) for s in speed_px]
        sb = (Gq >= S[0]).astype(np.int64) + (Gq >= S[1])
        db = np.zeros((n, H, W), np.int64) if dist2 is None else sum((np.asarray(dist2)[:, 0].astype(np.int64) >= int(e)).astype(np.int64) for e in dist2_edges)
        cell = (hidden * 3 + sb) * 3 + db
        flags = {"n": ok, "n_1px": Eq > 256, "n_3px": Eq > 768, "n_5px": Eq > 1280, "n_fl": (Eq > 768) & (20 * Eq > Gq)}
        idx = np.arange(n * H * W, dtype=np.int64).reshape(n, H, W) if one_row else np.broadcast_to(np.arange(H * W, dtype=np.int64).reshape(1, H, W), (n, H, W))
        key = (Eq.astype(np.uint64) << np.uint64(32)) | (0xFFFFFFFF - idx).astype(np.uint64)
        rows = np.zeros(1 if one_row else n, ROW)
        for r, which in enumerate([slice(None)] if one_row else [slice(i, i + 1) for i in range(n)]):
            m = ok[which]
            flat = rows[r]["cell"].reshape(18)
            for name, flag in flags.items():
                flat[name] = np.bincount(cell[which][m & flag[which]], minlength=18)
            flat["sum_epe_q8"] = np.bincount(cell[which][m], weights=Eq[which][m].astype(np.float64), minlength=18).astype(np.uint64)  # (exact: below 2^53)
            rows[r]["hist"] = np.bincount(hist_bin(Eq[which][m]), minlength=16)
            rows[r]["max_key"] = key[which][m].max() if m.any() else 0
            rows[r]["n_bad_gt"], rows[r]["n_bad_est"] = bad_gt[which].sum(), bad_est[which].sum()
        out["rows"] = rows
    if "epe" in outputs:
        epe = np.where(ok, Eq.astype(np.float32) * np.float32(0.00390625), np.float32(-1.0)).astype(np.float32)
        with np.errstate(over="ignore"):
            out["epe"] = np.ascontiguousarray(epe[:, None].astype(epe_dtype))
    if "picture" in outputs:
        rgb = COLOURS[colour_bin(Eq, Gq)]
        if dim_occ:
            rgb = np.where(hidden[..., None], rgb >> 1, rgb)
        rgb = np.where(ok[..., None], rgb, 0).astype(np.uint8)
        out["picture"] = np.ascontiguousarray(rgb if layout == "hwc_rgb" else rgb[..., ::-1].transpose(0, 3, 1, 2))
    return out


def float_metrics(gt, est):
    """The published metrics in float64 of float32 planes (est_scale 1), per pixel: (E, |gt|, E > 1, E > 3, E > 5, KITTI's Fl
    outlier, the devkit's colour bin)"""
    g, e = np.asarray(gt, np.float64), np.asarray(est, np.float64)
    E = np.sqrt((e[:, 0] - g[:, 0]) ** 2 + (e[:, 1] - g[:, 1]) ** 2)
    G = np.sqrt(g[:, 0] ** 2 + g[:, 1] ** 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(G > 0, E / G, np.inf)
    val = np.minimum(E / 3.0, 20.0 * rel)
    return E, G, E > 1.0, E > 3.0, E > 5.0, (E > 3.0) & (rel > 0.05), sum((val >= 2.0 ** j).astype(np.int64) for j in range(-4, 5))


def threshold_distance(E, G):
    """How far, in pixels of E, every pixel is from the thresholds the counts and the colours compare E with, LESS what the
    definition may move that comparison by: E against 1, 3, 5 px and the colour edges 3 * 2^j / 16 px, where Eq / 256 is within
    2.5 / 256 of E - allowed 3 / 256 -, and E against f |gt| for f = 1 / 20 (Fl) and f = 2^j / 320 (the colours' relative
    edges), where Gq / 256 is within (1 + sqrt(2) / 2) / 256 < 2 / 256 of |gt| as well - allowed (3 + 2 f) / 256.  Fl and every
    colour edge ask for an absolute AND a relative comparison: a pixel safely below one of the two is safe whatever the other
    says.  A pixel is safe when the result is >= 0."""
    def both(t, f):
        a, r = np.abs(E - t) - 3.0 / 256.0, np.abs(E - f * G) - (3.0 + 2.0 * f) / 256.0
        return np.where(((E < t) & (a >= 0)) | ((E < f * G) & (r >= 0)), np.inf, np.minimum(a, r))

    d = np.full(E.shape, np.inf)
    for t in (1.0, 3.0, 5.0):
        d = np.minimum(d, np.abs(E - t) - 3.0 / 256.0)
    d = np.minimum(d, both(3.0, 1.0 / 20.0))
    for j in range(9):
        d = np.minimum(d, both(3.0 * 2.0 ** j / 16.0, 2.0 ** j / 320.0))
    return d


def safe_inputs(W=264, H=200, seed=5):
    """float32 (gt, est) [N,2,H,W] that stay away from every threshold (threshold_distance >= 0, asserted here): random speeds
    and errors over all bands, and a pixel that comes too close to a threshold gets est = gt, which is E = 0 - 1/16 px and more
    below every threshold."""
    rng = np.random.RandomState(seed)
    turn, speed = rng.uniform(0, 2 * np.pi, (N, H, W)), rng.choice([0.0, 0.5, 6.0, 25.0, 90.0, 400.0], (N, H, W)) * rng.uniform(0.5, 1.5, (N, H, W))
    gt = np.stack([speed * np.cos(turn), speed * np.sin(turn)], axis=1).astype(np.float32)
    turn, err = rng.uniform(0, 2 * np.pi, (N, H, W)), 2.0 ** rng.uniform(-6.0, 8.0, (N, H, W))
    est = (gt + np.stack([err * np.cos(turn), err * np.sin(turn)], axis=1)).astype(np.float32)
    E, G = float_metrics(gt, est)[:2]
    near = threshold_distance(E, G) < 0
    est = np.where(near[:, None], gt, est)
    E, G = float_metrics(gt, est)[:2]
    assert (threshold_distance(E, G) >= 0).all() and near.mean() < 0.2
    return gt, est


@functools.lru_cache(maxsize=None)
def _float_inputs(W, H):
    rng = np.random.RandomState(W * 1000 + H)
    n = N
    turn, speed = rng.uniform(0, 2 * np.pi, (n, H, W)), rng.choice([0.0, 0.5, 6.0, 25.0, 90.0, 600.0], (n, H, W)) * rng.uniform(0.6, 1.4, (n, H, W))
    gt = np.stack([speed * np.cos(turn), speed * np.sin(turn)], axis=1).astype(np.float32)
    turn, err = rng.uniform(0, 2 * np.pi, (n, H, W)), 2.0 ** rng.uniform(-8.0, 11.5, (n, H, W))
    est = (gt + np.stack([err * np.cos(turn), err * np.sin(turn)], axis=1)).astype(np.float32)
    top = np.nextafter(BIG, np.float32(0))
    # (gt, est) of the first pixels of sample 0: the known answers; unusable ground truth; NaN and inf estimates; an estimate
    # that overflows binary16 (and, as float32, only errs by 70000 px); the largest usable values, opposite: Eq near 2^29.5
    special = [(k[0], k[1]) for k in KNOWN] + [((np.nan, 1), (1, 1)), ((1, np.inf), (1, 1)), ((BIG, 0), (0, 0)), ((0, -BIG), (np.nan, 0)),
                                              ((1, 1), (np.nan, 1)), ((1, 1), (1, -np.inf)), ((2, 2), (BIG, 0)), ((3, 1), (70000.0, 1.0)),
                                              ((top, -top), (-top, top)), ((0.5 / 256, 1.5 / 256), (-0.5 / 256, 2.5 / 256)), ((-0.0, 0.0), (0.0, -0.0)),
                                              ((0, 0), (1e-30, -1e-30))]
    g0, e0 = gt[0].reshape(2, -1), est[0].reshape(2, -1)
    for k, (g, e) in enumerate(special[:g0.shape[1]]):
        g0[:, k], e0[:, k] = g, e
    gt[ALL_BAD_GT, 0], gt[ALL_BAD_GT, 1] = np.nan, np.inf
    gt[ALL_BAD_GT, 1, ::2] = -BIG
    gt[EST_IS_GT] = rng.randint(-127, 128, (2, H, W)) / 4.0   # (exact as bfloat16 too: the estimate equals it in every format)
    est[EST_IS_GT] = gt[EST_IS_GT]
    gt[n - 1, :, -1, -1], est[n - 1, :, -1, -1] = (-2500.0, 40.0), (2500.0, 40.0)   # the last pixel of the last sample: 5000 px, the largest
    return gt, est


def inputs(W, H, gt_dtype="float32", est_dtype="float32", n=N):
    """(gt, est) [n,2,H,W]: sample 0 random over every band with the special pixels of _float_inputs in front, sample 1 with all
    ground truth unusable, sample 2 with est equal to gt, the last random with a 5000 px error, its largest, in its last pixel.  est_dtype
    "bfloat16": uint16 bit patterns.  binary16: 70000 and 2^20 overflow to inf."""
    gt, est = _float_inputs(W, H)
    with np.errstate(over="ignore"):
        gt = gt.astype(gt_dtype)
        if est_dtype == "bfloat16":
            est = to_bf16_bits(est)
        else:
            est = est.astype(est_dtype)
    return gt[:n].copy(), est[:n].copy()


def occ_map(W, H, dtype, n=N):
    """[n,1,H,W] maps with zeros, ones, other non-zero values and - as float32 - NaN and -0.0"""
    rng = np.random.RandomState(7 * W + H)
    o = (rng.randint(0, 3, (n, 1, H, W)) * rng.randint(0, 2, (n, 1, H, W))).astype(dtype)
    if np.dtype(dtype) == np.float32:
        o[0, 0, 0, 0], o[0, 0, 0, 1], o[0, 0, 0, 2] = np.nan, -0.0, 1e-30
    else:
        o[0, 0, 0, 0], o[0, 0, 0, 1] = 255, 0
    return o


def dist2_map(W, H, n=N):
    """[n,1,H,W] uint8 as ofdg_boundaries writes dist2: squared distances with both default edges, their neighbours, 0 and FAR"""
    rng = np.random.RandomState(11 * W + H)
    return rng.choice(np.array([0, 1, 4, 25, 26, 27, 50, 100, 101, 102, 200, 255], np.uint8), (n, 1, H, W))


def cases():
    """gt format x est format x map x dist2 x layout of the matrix both test files walk"""
    for gt_dtype in ("float32", "float16"):
        for est_dtype in ("float32", "float16", "bfloat16"):
            for occ in (None, "uint8", "float32"):
                for dist in (False, True):
                    for layout in ("planar_bgr", "hwc_rgb"):
                        yield gt_dtype, est_dtype, occ, dist, layout


def equal_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def add_rows(rows, plane=None):
    """One row that is the field-wise sum of rows; the key: the maximum, re-indexed with plane= (H * W) as OFDG_ERR_ONE_ROW
    indexes - sample r's idx becomes r * plane + idx"""
    out = np.zeros(1, ROW)
    for name in CELL.names:
        out["cell"][name][0] = rows["cell"][name].sum(axis=0, dtype=np.uint64)
    out["hist"][0] = rows["hist"].sum(axis=0, dtype=np.uint64)
    out["n_bad_gt"][0], out["n_bad_est"][0] = rows["n_bad_gt"].sum(), rows["n_bad_est"].sum()
    keys = []
    for r, key in enumerate(rows["max_key"].tolist()):
        if key:
            idx = 0xFFFFFFFF - (key & 0xFFFFFFFF) + (r * plane if plane is not None else 0)
            keys.append((key >> 32 << 32) | (0xFFFFFFFF - idx))
    out["max_key"][0] = max(keys) if keys else 0
    return out
