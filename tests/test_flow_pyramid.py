"""CPU tests of the multi-scale flow pyramid (ofdg_host_flow_pyramid, include/ofdg.h): the host twin against the numpy
restatement of the definition (tests/flow_pyramid_reference.py) byte for byte over every option, the invariants of the
definition, what the planted tensors hold, and every refusal with the outputs left untouched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import flow_pyramid_reference as fpr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0xA5
SHAPES = [(8, 8, 3), (64, 64, 6), (72, 40, 3), (128, 96, 5), (192, 128, 6), (72, 40, 1)]  # W, H, levels
_cache = {}


def tensors(W, H, L, dtype, n=3):
    key = (W, H, L, np.dtype(dtype).name, n)
    if key not in _cache:
        _cache[key] = fpr.planted(n, H, W, dtype, levels=L)
    return _cache[key]


def occ_as(occ, kind):
    if kind is None:
        return None
    return occ.astype(np.uint8) * np.uint8(3) if kind == "u8" else occ.astype(np.float32) * np.float32(0.5)


def test_header_and_bindings(ofdg):
    hdr = open(os.path.join(ROOT, "include", "ofdg.h")).read()
    for name, value in (("OFDG_PYR_MAX_LEVELS", 6), ("OFDG_PYR_SCALE", 1)):
        m = re.search(r"#define\s+%s\s+(\d+)" % name, hdr)
        assert m and int(m.group(1)) == value, name
    assert (ofdg.PYR_MAX_LEVELS, ofdg.PYR_SCALE) == (6, 1) == (fpr.MAX_LEVELS, fpr.SCALE)
    for fn in ("ofdg_flow_pyramid", "ofdg_host_flow_pyramid"):
        assert re.search(r"\bint\s+%s\s*\(" % fn, hdr), fn
        assert fn in ofdg.EXPORTS and hasattr(ofdg.lib(), fn)
    m = re.search(r"struct ofdg_flow_pyramid \{(.*?)\};", hdr, re.S)
    fields = [re.sub(r"\s+", " ", f).strip() for f in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(";")]
    assert [f for f in fields if f] == ["void* flow[OFDG_PYR_MAX_LEVELS]", "void* weight[OFDG_PYR_MAX_LEVELS]", "int32_t levels", "int32_t out_fmt"]
    assert C.sizeof(ofdg.FlowPyramid) == 104
    assert [(n, getattr(ofdg.FlowPyramid, n).offset) for n, _ in ofdg.FlowPyramid._fields_] == [("flow", 0), ("weight", 48), ("levels", 96), ("out_fmt", 100)]


@pytest.mark.parametrize("W,H,L", SHAPES)
@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["f32", "f16"])
def test_planted_tensors_hold_what_they_should(W, H, L, dtype):
    """(the test's own inputs) planted() itself asserts that the order of summation shows in every level >= 2, with and
    without the map; here: unusable pixels and usable extremes meet every child position of every level, a level-L cell
    has no usable pixel and one has exactly one, float32 tensors hold denormals."""
    f, occ = tensors(W, H, L, dtype)
    w = f.astype(np.float32)
    bad = ~((np.abs(w[:, 0]) < fpr.LIMIT) & (np.abs(w[:, 1]) < fpr.LIMIT))
    with np.errstate(over="ignore", under="ignore"):
        kept = np.array(fpr.SPECIALS, np.float32).astype(dtype).astype(np.float32)
    kept = np.unique(np.abs(kept[np.isfinite(kept) & (np.abs(kept) < fpr.LIMIT) & (kept != 0)]))
    edge = np.isin(np.abs(w), kept).any(axis=1)  # the usable extremes: just below the limit, around 65504, the denormals
    ys, xs = np.mgrid[0:H, 0:W]
    if H * W >= 64 * 64:
        for k in range(1, L + 1):
            role = ((ys >> (k - 1)) & 1) * 2 + ((xs >> (k - 1)) & 1)
            assert set(role[bad[0]]) == {0, 1, 2, 3}, k
            assert set(role[edge[0]]) == {0, 1, 2, 3}, k
    _, wt = fpr.flow_pyramid(f, L, None)
    assert (wt[L - 1] == 0).any() and (wt[L - 1] == 1).any()
    assert np.signbit(w[0, 1, 2, 2]) and w[0, 1, 2, 2] == 0
    if dtype == np.float32:
        tiny = np.float32(2.0 ** -126)
        assert ((w != 0) & (np.abs(w) < tiny)).any()
        lv, _ = fpr.flow_pyramid(f, 1, None, fpr.SCALE)
        assert 0 < lv[0][0, 0, 1, 1] < tiny  # (the scaled mean of the denormal cell)
    assert occ.any() and not occ.all()


@pytest.mark.parametrize("W,H,L", SHAPES)
@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["in_f32", "in_f16"])
@pytest.mark.parametrize("out_dtype", [np.float32, np.float16], ids=["out_f32", "out_f16"])
@pytest.mark.parametrize("occ_kind", [None, "u8", "f32"])
def test_host_twin_equals_the_restatement(ofdg, W, H, L, dtype, out_dtype, occ_kind):
    f, occ = tensors(W, H, L, dtype)
    o = occ_as(occ, occ_kind)
    for flags in (0, fpr.SCALE):
        want, want_w = fpr.flow_pyramid(f, L, o, flags, out_dtype)
        what = "%dx%d L=%d flags %d" % (W, H, L, flags)
        got = ofdg.host_flow_pyramid(f, L, o, scale=bool(flags), out_dtype=out_dtype)
        fpr.expect_equal(got, want, what + " without weights")
        got, got_w = ofdg.host_flow_pyramid(f, L, o, scale=bool(flags), out_dtype=out_dtype, weights=True)
        fpr.expect_equal(got, want, what)
        fpr.expect_equal(got_w, want_w, what + " weights")


@pytest.mark.parametrize("occ_kind", [None, "u8"])
def test_weights_add_up(ofdg, occ_kind):
    W, H, L = 192, 128, 6
    f, occ = tensors(W, H, L, np.float32)
    o = occ_as(occ, occ_kind)
    _, wt = ofdg.host_flow_pyramid(f, L, o, weights=True)
    _, c0 = fpr.level0(f, o)
    assert int(wt[0].astype(np.int64).sum()) == int(c0.sum())
    for k in range(1, L):
        assert np.array_equal(wt[k][:, 0].astype(np.int64), sum(fpr.blocks(wt[k - 1][:, 0].astype(np.int64)))), k
    assert wt[L - 1].max() <= 4 ** L


@pytest.mark.parametrize("dtype,out_dtype", [(np.float32, np.float32), (np.float16, np.float16), (np.float32, np.float16)])
def test_constant_field_and_all_occluded(ofdg, dtype, out_dtype):
    W, H, L, n = 128, 64, 6, 2
    f = np.empty((n, 2, H, W), dtype)
    f[:, 0], f[:, 1] = 12.5, -3.0
    for scale in (False, True):
        lv, wt = ofdg.host_flow_pyramid(f, L, scale=scale, out_dtype=out_dtype, weights=True)
        for k in range(1, L + 1):
            s = 2.0 ** -k if scale else 1.0
            assert lv[k - 1].dtype == out_dtype and (lv[k - 1][:, 0] == out_dtype(12.5 * s)).all() and (lv[k - 1][:, 1] == out_dtype(-3.0 * s)).all()
            assert (wt[k - 1] == 4 ** k).all()
    hidden = np.ones((n, 1, H, W), np.uint8)
    hidden[1] = 0
    lv, wt = ofdg.host_flow_pyramid(f, L, hidden, out_dtype=out_dtype, weights=True)
    for k in range(1, L + 1):
        assert not lv[k - 1][0].view(np.uint8).any() and not wt[k - 1][0].any()  # +0.0 in every bit
        assert (wt[k - 1][1] == 4 ** k).all()


def test_refusals_leave_the_outputs_alone(ofdg):
    W, H, L, n = 64, 32, 3, 2
    lib, vp = ofdg.lib(), C.c_void_p
    F32, U8, F16 = ofdg.FMT_F32, ofdg.FMT_U8, ofdg.FMT_F16
    flow = np.zeros((n, 2, H, W), np.float32)
    occ = np.zeros((n, 1, H, W), np.uint8)
    lv = [np.full((n * 2 * (H >> k) * (W >> k) * 4 + 16,), FILL, np.uint8) for k in range(1, 7)]
    wt = [np.full((n * (H >> k) * (W >> k) * 2 + 16,), FILL, np.uint8) for k in range(1, 7)]

    def record(levels=L, out_fmt=F32, flows=None, weights=None):
        rec = ofdg.FlowPyramid()
        rec.levels, rec.out_fmt = levels, out_fmt
        for k in range(6):
            rec.flow[k] = (flows or [t.ctypes.data for t in lv])[k]
            rec.weight[k] = (weights or [None] * 6)[k]
        return rec

    def refused(word, d_flow=flow.ctypes.data, ffmt=F32, d_occ=None, ofmt=F32, n_=n, w=W, h=H, flags=0, rec=None, null_rec=False):
        rec = record() if rec is None else rec
        rc = lib.ofdg_host_flow_pyramid(vp(d_flow), ffmt, vp(d_occ), ofmt, n_, w, h, flags, None if null_rec else C.byref(rec))
        assert rc == ofdg.EINVAL, word
        msg = lib.ofdg_host_last_error().decode()
        assert msg.startswith("ofdg_host_flow_pyramid") and word in msg, msg
        assert all((t == FILL).all() for t in lv + wt), word

    all_w = [t.ctypes.data for t in wt]
    refused("d_flow", d_flow=None)
    refused("pyr", null_rec=True)
    refused("levels", rec=record(levels=0))
    refused("levels", rec=record(levels=7))
    refused("multiples", rec=record(levels=6))          # H = 32
    refused("multiples", w=W + 4)
    refused("multiples", h=H + 4)
    refused("pyr->flow", rec=record(flows=[lv[0].ctypes.data, None, lv[2].ctypes.data, None, None, None]))
    refused("pyr->weight", rec=record(weights=[all_w[0], None, all_w[2], None, None, None]))
    refused("pyr->weight", rec=record(weights=[None, all_w[1], all_w[2], None, None, None]))
    refused("flow_fmt", ffmt=U8)
    refused("flow_fmt", ffmt=3)
    refused("occ_fmt", d_occ=occ.ctypes.data, ofmt=F16)
    refused("out_fmt", rec=record(out_fmt=U8))
    refused("n_samples", n_=0)
    refused("flags", flags=2)
    refused("16-byte", rec=record(flows=[lv[0].ctypes.data + 8] + [t.ctypes.data for t in lv[1:]]))
    refused("4-byte", rec=record(weights=[all_w[0], all_w[1] + 2] + all_w[2:]))
    # entries past `levels` are never read: NULL or wild, set or not, the call is valid
    rec = record(flows=[t.ctypes.data for t in lv[:3]] + [None, 8, None], weights=all_w[:3] + [None, 2, None])
    assert lib.ofdg_host_flow_pyramid(vp(flow.ctypes.data), F32, None, F32, n, W, H, 0, C.byref(rec)) == ofdg.OK
    for k in range(1, 7):
        size = n * 2 * (H >> k) * (W >> k) * 4
        assert (lv[k - 1][size:] == FILL).all() and (not lv[k - 1][:size].any() if k <= 3 else (lv[k - 1] == FILL).all())
    with pytest.raises(ValueError):
        ofdg.host_flow_pyramid(flow, 6)
    with pytest.raises(ValueError):
        ofdg.host_flow_pyramid(flow.astype(np.float64), 3)
