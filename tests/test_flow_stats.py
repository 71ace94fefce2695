"""Host-side tests of the per-sample flow statistics (ofdg_flow_stats_row, ofdg_flow_stats, ofdg_host_flow_stats in
include/ofdg.h): the layout in header / ctypes / numpy, ofdg_host_flow_stats against the numpy restatement of the definition
(tests/flow_stats_reference.py) field for field and bit for bit on tensors with every special pixel planted, the options, and
the refusals.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import flow_stats_reference as fsr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N, H, W = 3, 40, 72
FILL = 0xA5
FIELDS = [("hist", 0, 256), ("n_counted", 256, 4), ("n_bad", 260, 4), ("n_occluded", 264, 4), ("reserved", 268, 4),
          ("sum_u_q8", 272, 8), ("sum_v_q8", 280, 8), ("sum_mag_q8", 288, 8), ("max_key", 296, 8)]
BIN_PX = (0.25, 2.0, 3.7)
_cache = {}


def tensors(bin_px, dtype):
    """The planted flow (float32 or float16) and its occlusion map for one bin width, made once."""
    key = (bin_px, np.dtype(dtype).name)
    if key not in _cache:
        _cache[key] = fsr.planted(N, H, W, bin_px, dtype)
    return _cache[key]


def occ_as(occ, kind):
    if kind is None:
        return None
    return occ.astype(np.uint8) * np.uint8(3) if kind == "u8" else occ.astype(np.float32) * np.float32(0.5)  # (any non-zero value hides)


def test_layout_is_304_bytes_everywhere(ofdg):
    hdr = open(os.path.join(ROOT, "include", "ofdg.h")).read()
    m = re.search(r"typedef struct ofdg_flow_stats_row \{(.*?)\} ofdg_flow_stats_row;", hdr, re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    decls = [re.sub(r"\s+", " ", d).strip() for d in body.split(";") if d.strip()]
    assert decls == ["uint32_t hist[OFDG_FLOW_HIST_BINS]", "uint32_t n_counted, n_bad, n_occluded, reserved",
                     "int64_t sum_u_q8, sum_v_q8, sum_mag_q8", "uint64_t max_key"]
    assert re.search(r"#define\s+OFDG_FLOW_HIST_BINS\s+64\b", hdr) and ofdg.FLOW_HIST_BINS == 64 == fsr.BINS
    for name, value in (("ACCUMULATE", 1), ("VISIBLE_ONLY", 2), ("ONE_ROW", 4)):
        assert re.search(r"#define\s+OFDG_STATS_%s\s+%d\b" % (name, value), hdr)
        assert getattr(ofdg, "STATS_" + name) == value == getattr(fsr, name)
    assert C.sizeof(ofdg.FlowStatsRow) == 304 and ofdg.FLOW_STATS_DTYPE.itemsize == 304
    for name, offset, size in FIELDS:
        f = getattr(ofdg.FlowStatsRow, name)
        assert (f.offset, f.size) == (offset, size), name
        dt, off = ofdg.FLOW_STATS_DTYPE.fields[name][:2]
        assert (off, dt.itemsize) == (offset, size), name
    assert [n for n, _ in ofdg.FlowStatsRow._fields_] == list(ofdg.FLOW_STATS_DTYPE.names) == [n for n, _, _ in FIELDS] == list(fsr.FIELDS)
    for fn in ("ofdg_flow_stats", "ofdg_host_flow_stats"):
        assert re.search(r"\bint\s+%s\s*\(" % fn, hdr), fn
        assert fn in ofdg.EXPORTS and hasattr(ofdg.lib(), fn)


def test_planted_tensors_hold_what_they_should():
    """(the test's own inputs: every case of the definition occurs)"""
    f, occ = tensors(2.0, np.float32)
    rows = fsr.flow_stats(f, None, 2.0)
    assert all(r["n_bad"] == 5 for r in rows) and all(r["hist"][63] >= 2 for r in rows)
    for k in (1, 2, 7, 31, 63):
        assert all(r["hist"][k] >= 1 for r in rows)
    top = int(np.array([fsr.BELOW_LIMIT * fsr.BELOW_LIMIT + fsr.BELOW_LIMIT * fsr.BELOW_LIMIT], np.float32).view(np.uint32)[0])
    assert rows[0]["max_key"] >> 32 == top and 0xFFFFFFFF - (rows[0]["max_key"] & 0xFFFFFFFF) == 5 + 5
    m2 = int(np.array([1620000.0], np.float32).view(np.uint32)[0])
    assert rows[1]["max_key"] == (m2 << 32) | (0xFFFFFFFF - H * W // 3)          # the first of three equal maxima
    vis = fsr.flow_stats(f, occ, 2.0, fsr.VISIBLE_ONLY)
    assert vis[1]["max_key"] == (m2 << 32) | (0xFFFFFFFF - (H * W // 2 + 1))     # ... of the two visible ones
    assert vis[1]["n_bad"] == 4 and vis[1]["n_occluded"] > 100
    h = fsr.flow_stats(tensors(2.0, np.float16)[0], None, 2.0)
    assert [r["n_bad"] for r in h] == [6, 5, 6]  # (the limits and the value below them overflow a half)
    assert np.float32(1e-20) * np.float32(1e-20) > 0  # m2 of the subnormal pixel is not flushed here


@pytest.mark.parametrize("bin_px", BIN_PX)
@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("occ_kind", [None, "u8", "f32"])
def test_host_flow_stats_equals_the_restatement(ofdg, dtype, occ_kind, bin_px):
    f, occ = tensors(bin_px, dtype)
    o = occ_as(occ, occ_kind)
    for flags in (0, fsr.ONE_ROW) + ((fsr.VISIBLE_ONLY, fsr.VISIBLE_ONLY | fsr.ONE_ROW) if o is not None else ()):
        vis, one = bool(flags & fsr.VISIBLE_ONLY), bool(flags & fsr.ONE_ROW)
        got = ofdg.host_flow_stats(f, o, bin_px, visible_only=vis, one_row=one)
        want = fsr.flow_stats(f, o, bin_px, flags)
        assert got.shape == ((1,) if one else (N,)) and got.dtype == ofdg.FLOW_STATS_DTYPE
        fsr.expect_equal(got, want, "flags %d" % flags)
        fsr.expect_invariants(want, H, W, N if one else 1, vis)
        if o is None:
            assert not got["n_occluded"].any()
        assert not got["reserved"].any()


def merged(a, b):
    """What two plain calls add up to: sums of everything, the larger key."""
    out = []
    for x, y in zip(a, b):
        r = {f: x[f] + y[f] for f in fsr.FIELDS if f not in ("hist", "max_key")}
        r["hist"] = [p + q for p, q in zip(x["hist"], y["hist"])]
        r["max_key"] = max(x["max_key"], y["max_key"])
        out.append(r)
    return out


@pytest.mark.parametrize("one", [False, True], ids=["per_sample", "one_row"])
def test_accumulate_over_two_calls_is_the_sum_of_two_plain_calls(ofdg, one):
    a, occ = tensors(2.0, np.float32)
    b = fsr.planted(N, H, W, 2.0, np.float16, seed=8)[0]
    o = occ_as(occ, "u8")
    first = ofdg.host_flow_stats(a, o, 2.0, one_row=one)
    plain_a, plain_b = fsr.rows_of(first), fsr.rows_of(ofdg.host_flow_stats(b, None, 2.0, one_row=one))
    both = ofdg.host_flow_stats(b, None, 2.0, accumulate=True, one_row=one, rows=first)
    assert both is first
    fsr.expect_equal(both, merged(plain_a, plain_b))
    fsr.expect_equal(both, fsr.flow_stats(b, None, 2.0, fsr.ACCUMULATE | (fsr.ONE_ROW if one else 0),
                                          rows=fsr.flow_stats(a, o, 2.0, fsr.ONE_ROW if one else 0)))
    # an all-zero row is the identity
    zero = np.zeros((1 if one else N,), ofdg.FLOW_STATS_DTYPE)
    fsr.expect_equal(ofdg.host_flow_stats(a, o, 2.0, accumulate=True, one_row=one, rows=zero), plain_a)


def test_rows_are_fully_overwritten_without_accumulate(ofdg):
    f, occ = tensors(2.0, np.float32)
    rows = np.frombuffer(bytes([FILL]) * (N * 304), ofdg.FLOW_STATS_DTYPE).copy()
    fsr.expect_equal(ofdg.host_flow_stats(f, None, 2.0, rows=rows), fsr.flow_stats(f, None, 2.0))
    rows = np.frombuffer(bytes([FILL]) * (N * 304), ofdg.FLOW_STATS_DTYPE).copy()
    buf = rows.view(np.uint8)
    rc = ofdg.lib().ofdg_host_flow_stats(f.ctypes.data_as(C.c_void_p), ofdg.FMT_F32, None, 0, N, W, H, 2.0, ofdg.STATS_ONE_ROW,
                                         rows.ctypes.data_as(C.c_void_p))
    assert rc == ofdg.OK and (buf[304:] == FILL).all()  # one row: the others are not the call's
    fsr.expect_equal(rows[:1], fsr.flow_stats(f, None, 2.0, fsr.ONE_ROW))


def test_flow_stats_numpy_decodes_the_key(ofdg):
    f, occ = tensors(2.0, np.float32)
    per = ofdg.flow_stats_numpy(ofdg.host_flow_stats(f, None, 2.0).view(np.uint8).reshape(N, 304), width=W, height=H)
    assert per["rows"].dtype == ofdg.FLOW_STATS_DTYPE and per["max_mag2"].dtype == np.float32
    assert per["max_mag2"][1] == np.float32(1620000.0) and per["max_index"][1] == H * W // 3
    assert (per["max_x"][1], per["max_y"][1], per["max_sample"][1]) == (H * W // 3 % W, H * W // 3 // W, 1)
    assert list(per["max_sample"]) == [0, 1, 2] and per["max_index"][0] == 10
    one = ofdg.flow_stats_numpy(ofdg.host_flow_stats(f[1:], None, 2.0, one_row=True).view(np.uint8), width=W, height=H, one_row=True)
    # (sample 2 of f is sample 1 of this batch; its pixel just below the limit sits at 5 + 3 * 2 + 5)
    assert one["max_sample"][0] == 1 and one["max_index"][0] == H * W + 16 and (one["max_x"][0], one["max_y"][0]) == (16, 0)
    none = ofdg.flow_stats_numpy(np.zeros((2, 304), np.uint8), width=W, height=H)
    assert list(none["max_index"]) == [-1, -1] and list(none["max_sample"]) == [-1, -1] and not none["max_mag2"].any()


def test_refusals_leave_the_rows_untouched(ofdg):
    f, occ = tensors(2.0, np.float32)
    o = occ_as(occ, "u8")
    L, vp = ofdg.lib(), C.c_void_p
    buf = np.full(8 + N * 304, FILL, np.uint8)
    base = buf.ctypes.data
    off = (-base) % 8
    rows = base + off  # 8-byte aligned

    def refused(word, flow=f.ctypes.data, ffmt=ofdg.FMT_F32, occ_p=None, ofmt=0, n=N, w=W, h=H, bin_px=2.0, flags=0, r=rows):
        rc = L.ofdg_host_flow_stats(vp(flow), ffmt, vp(occ_p), ofmt, n, w, h, bin_px, flags, vp(r))
        assert rc == ofdg.EINVAL
        msg = L.ofdg_host_last_error().decode()
        assert msg.startswith("ofdg_host_flow_stats") and word in msg, msg
        assert (buf == FILL).all()

    refused("d_flow", flow=None)
    refused("d_rows", r=None)
    refused("flow_fmt", ffmt=ofdg.FMT_U8)
    refused("flow_fmt", ffmt=7)
    refused("occ_fmt", occ_p=o.ctypes.data, ofmt=ofdg.FMT_F16)
    refused("n_samples", n=0)
    refused("width", w=0)
    for bad in (float("nan"), 0.0, -2.0, 2.0 ** -11, 2.0 ** 14 * 1.001, float("inf")):
        refused("bin_px", bin_px=bad)
    refused("flags", flags=8)
    refused("VISIBLE_ONLY", flags=ofdg.STATS_VISIBLE_ONLY)
    refused("ONE_ROW", flags=ofdg.STATS_ONE_ROW, n=1 << 16, w=1 << 8, h=1 << 8)  # n*H*W = 2^32 (checked before any pixel is read)
    refused("8-byte", r=rows + 4)
    # ... and the limits themselves are valid
    for ok in (2.0 ** -10, 2.0 ** 14):
        assert L.ofdg_host_flow_stats(vp(f.ctypes.data), ofdg.FMT_F32, None, 0, N, W, H, ok, 0, vp(rows)) == ofdg.OK
    assert not (buf[off:off + N * 304] == FILL).all()


def test_python_argument_rules(ofdg):
    torch = pytest.importorskip("torch")
    n, h, w = 2, 16, 24
    rows = ofdg.alloc_flow_stats(n, device="cpu")
    assert tuple(rows.shape) == (n, 304) and rows.dtype == torch.uint8 and not rows.any()
    with pytest.raises(ValueError):
        ofdg.alloc_flow_stats(0, device="cpu")
    flow = torch.zeros((n, 2, h, w))
    occ = torch.zeros((n, 1, h, w), dtype=torch.uint8)
    assert ofdg.flow_stats_format(flow, None, rows, h, w) == (n, ofdg.FMT_F32, ofdg.FMT_F32)
    assert ofdg.flow_stats_format(flow.half(), occ, rows, h, w) == (n, ofdg.FMT_F16, ofdg.FMT_U8)
    assert ofdg.flow_stats_format(flow, occ.float(), rows[:1], h, w, one_row=True) == (n, ofdg.FMT_F32, ofdg.FMT_F32)
    bad = [dict(flow=flow.double()), dict(flow=flow[:, :1]), dict(flow=flow[0]), dict(flow=None), dict(rows=None),
           dict(flow=torch.zeros((n, 2, w, h))), dict(occ=occ.to(torch.int8)), dict(occ=occ[:1]), dict(occ=occ[:, 0]),
           dict(rows=rows[:1]), dict(rows=rows, one_row=True), dict(rows=rows[:, :300]), dict(rows=rows.to(torch.int8))]
    for change in bad:
        args = dict(flow=flow, occ=occ, rows=rows, one_row=False)
        args.update(change)
        with pytest.raises(ValueError):
            ofdg.flow_stats_format(args["flow"], args["occ"], args["rows"], h, w, args["one_row"])
    with pytest.raises(ValueError):
        ofdg.host_flow_stats(np.zeros((n, 2, h, w), np.float32), accumulate=True)  # nothing to add to
    with pytest.raises(ValueError):
        ofdg.host_flow_stats(np.zeros((2, h, w), np.float32))
    with pytest.raises(ofdg.OfdgError):
        ofdg.host_flow_stats(np.zeros((n, 2, h, w), np.float32), bin_px=0.0)
