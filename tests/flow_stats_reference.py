"""The definition of the per-sample flow statistics (ofdg_flow_stats, include/ofdg.h) restated in numpy: float32 arithmetic op
by op (numpy rounds every ufunc result to float32 and fuses nothing), np.rint / np.sqrt on float32 (nearest even / correctly
rounded), integers for everything that is summed.  Shared by tests/test_flow_stats.py and tests/test_gpu_flow_stats.py, which
also take their planted tensors from here."""
import numpy as np

BINS = 64
ACCUMULATE, VISIBLE_ONLY, ONE_ROW = 1, 2, 4
FIELDS = ("hist", "n_counted", "n_bad", "n_occluded", "reserved", "sum_u_q8", "sum_v_q8", "sum_mag_q8", "max_key")
LIMIT = np.float32(1048576.0)
BELOW_LIMIT = np.nextafter(LIMIT, np.float32(0))  # the largest float32 that still counts


def edges2(bin_px):
    """edge2[k] = fl32(fl32(k * bin_px)^2), k = 0..63."""
    e = np.arange(BINS, dtype=np.float32) * np.float32(bin_px)
    return e * e


def zero_rows(m):
    return [dict(hist=[0] * BINS, n_counted=0, n_bad=0, n_occluded=0, reserved=0, sum_u_q8=0, sum_v_q8=0, sum_mag_q8=0, max_key=0)
            for _ in range(m)]


def flow_stats(flow, occ=None, bin_px=2.0, flags=0, rows=None):
    """Rows (dicts of Python integers, one per sample or one in all) of flow [n,2,H,W] float32 / float16 and occ None or
    [n,1,H,W] float32 / uint8.  rows: what to add to with ACCUMULATE."""
    n, _, H, W = flow.shape
    one = bool(flags & ONE_ROW)
    if not flags & ACCUMULATE:
        rows = zero_rows(1 if one else n)
    e2 = edges2(bin_px)
    for i in range(n):
        r = rows[0 if one else i]
        u = flow[i, 0].astype(np.float32).reshape(-1)
        v = flow[i, 1].astype(np.float32).reshape(-1)
        idx = np.arange(H * W, dtype=np.int64) + (i * H * W if one else 0)
        look = np.ones(H * W, bool)
        if occ is not None:
            hidden = occ[i, 0].reshape(-1) != 0
            r["n_occluded"] += int(hidden.sum())
            if flags & VISIBLE_ONLY:
                look = ~hidden
        good = (np.abs(u) < LIMIT) & (np.abs(v) < LIMIT)
        r["n_bad"] += int((look & ~good).sum())
        c = look & good
        r["n_counted"] += int(c.sum())
        u, v, idx = u[c], v[c], idx[c]
        m2 = u * u + v * v  # (two float32 products, one float32 sum)
        assert m2.dtype == np.float32
        b = np.searchsorted(e2[1:], m2, side="right")  # the number of k in 1..63 with edge2[k] <= m2
        for k, cnt in zip(*np.unique(b, return_counts=True)):
            r["hist"][int(k)] += int(cnt)
        r["sum_u_q8"] += int(np.rint(u * np.float32(256)).astype(np.int64).sum())
        r["sum_v_q8"] += int(np.rint(v * np.float32(256)).astype(np.int64).sum())
        r["sum_mag_q8"] += int(np.rint(np.sqrt(m2) * np.float32(256)).astype(np.int64).sum())
        if len(m2):
            key = (m2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - idx.astype(np.uint64))
            r["max_key"] = max(r["max_key"], int(key.max()))
    return rows


def rows_of(structured):
    """A FLOW_STATS_DTYPE array as the same list of dicts of Python integers."""
    return [{f: ([int(x) for x in row[f]] if f == "hist" else int(row[f])) for f in FIELDS} for row in structured]


def expect_equal(got, want, what=""):
    """Field for field, bit for bit."""
    got = rows_of(got)
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        for f in FIELDS:
            assert g[f] == w[f], "%s row %d field %s: got %s, expected %s" % (what, i, f, g[f], w[f])


def expect_invariants(rows, H, W, samples_per_row=1, visible_only=False):
    for r in rows:
        assert sum(r["hist"]) == r["n_counted"]
        assert r["n_counted"] + r["n_bad"] + (r["n_occluded"] if visible_only else 0) == samples_per_row * H * W


def planted(n, H, W, bin_px, dtype=np.float32, seed=7):
    """Random flow of scale ~30 px with the special pixels of the definition planted in every sample (float32 values; as float16
    the limits overflow to inf and count as bad, and an edge stays an edge only where k * bin_px is a half), and an occlusion
    map (bool [n,1,H,W]) that hides some ordinary pixels, one bad pixel and one of the two maxima of sample 1."""
    rng = np.random.default_rng(seed)
    f = (rng.standard_normal((n, 2, H, W)) * 30.0).astype(np.float32)
    occ = rng.random((n, 1, H, W)) < 0.2
    bp = np.float32(bin_px)
    for i in range(n):
        u, v = f[i, 0].reshape(-1), f[i, 1].reshape(-1)
        o = occ[i, 0].reshape(-1)
        p = 5 + 3 * i  # (a different place in every sample)
        u[p], u[p + 1], v[p + 2] = np.nan, np.inf, -np.inf
        u[p + 3], v[p + 4] = LIMIT, -LIMIT                      # bad
        u[p + 5], v[p + 5] = BELOW_LIMIT, -BELOW_LIMIT          # counted: the open last bin, and the largest m2 there can be
        u[p + 6], v[p + 6] = -0.0, -0.0
        for j, k in enumerate((1, 2, 7, 31, 63)):                # exactly on an edge: belongs to bin k
            u[p + 7 + j], v[p + 7 + j] = (np.float32(k) * bp, 0.0) if j % 2 == 0 else (-0.0, -np.float32(k) * bp)
        u[p + 12], v[p + 12] = np.float32(64.5) * bp, 0.0        # the open last bin
        u[p + 13], v[p + 13] = 1e-20, 0.0                        # m2 is a float32 subnormal
        o[p:p + 14] = False
        o[p + 1] = True                                          # an occluded bad pixel
    # sample 1: no pixel at the limit; two pixels share the largest m2 instead (the lower index must win), a third, occluded
    # one in front of them holds it too (and wins unless VISIBLE_ONLY)
    if n > 1:
        u, v = f[1, 0].reshape(-1), f[1, 1].reshape(-1)
        o = occ[1, 0].reshape(-1)
        u[8 + 5], v[8 + 5] = 3.0, 4.0
        top = np.float32(900.0)
        for q, hide in ((H * W // 3, True), (H * W // 2 + 1, False), (H * W - 2, False)):
            u[q], v[q], o[q] = top, -top, hide
    with np.errstate(over="ignore"):  # (the limits become inf in a half: that is the point)
        return f.astype(dtype), occ
