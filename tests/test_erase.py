"""CPU tests of the occluder rectangles (ofdg_erase, include/ofdg.h): ofdg_host_erase and ofdg_erase_draw against the numpy
restatement (tests/erase_reference.py), byte for byte - every format, fill and size, given and drawn records with every edge
case of the sanitising -, the known answers of the integer mean, the occlusion rule at the rectangle edges, the draw's
recorded values and statistics, the refusals and the layout."""
import ctypes as C
import math

import numpy as np
import pytest

import erase_reference as er

FILL = 0xA5
COLOR = (3, 250, 128)


def run_both(ofdg, images, occ, flow, **kw):
    """the twin (in place on copies) and the restatement on the same inputs: ((images, occ, recs) of each)"""
    h_img = [None if t is None else np.array(t) for t in images]
    h_occ = None if occ is None else [None if t is None else np.array(t) for t in occ]
    h_flow = None if flow is None else [None if t is None else np.array(t) for t in flow]
    used = ofdg.host_erase(h_img, h_occ, h_flow, **kw)
    if h_flow is not None:
        er.expect_equal(h_flow, flow, "the flows are read only")
    return (h_img, h_occ or [None, None], used), er.erase(images, occ, flow, **kw)


def expect_same(got, want, what):
    er.expect_equal(got[0], want[0], what + ": images")
    er.expect_equal(got[1], want[1], what + ": maps")
    assert er.equal_bits(got[2], want[2]), "%s: records\n%s\n%s" % (what, got[2], want[2])


@pytest.mark.parametrize("W,H", er.SIZES)
@pytest.mark.parametrize("fill", [er.MEAN, er.CONST, er.NOISE])
@pytest.mark.parametrize("flow_dtype", ["float32", "float16"])
@pytest.mark.parametrize("occ_dtype", ["float32", "uint8"])
@pytest.mark.parametrize("image_dtype", ["float32", "uint8"])
def test_twin_equals_restatement(ofdg, image_dtype, occ_dtype, flow_dtype, fill, W, H):
    """n = 3: one sample without a rectangle, one with one, one with four (er.records); then the 1x1 / full-row / border /
    corner rectangles (er.records_edges); then drawn records across a 2^32 boundary of the global index."""
    images, occ, flow = er.frames(W, H, image_dtype), er.maps(W, H, occ_dtype), er.flows(W, H, flow_dtype)
    what = "%dx%d %s %s %s fill %d" % (W, H, image_dtype, occ_dtype, flow_dtype, fill)
    for frames in ((1,), (0, 1)):
        for recs in (er.records(W, H), er.records_edges(W, H)):
            kw = dict(recs=recs, seed=5, first_index=7, fill=fill, color=COLOR, frames=frames)
            got, want = run_both(ofdg, images, occ, flow, **kw)
            expect_same(got, want, what + " frames %s" % (frames,))
            assert (got[2]["reserved"] == 0).all() and (got[2]["count"] <= 4).all() and (got[2]["count"] >= 0).all()
        ranges = dict(prob=0.8, min_rects=0, max_rects=4, min_size=1, max_size=max(W // 2, 1))
        kw = dict(seed=11, first_index=2 ** 32 - 1, ranges=ranges, fill=fill, color=COLOR, frames=frames)
        got, want = run_both(ofdg, images, occ, flow, **kw)
        expect_same(got, want, what + " drawn, frames %s" % (frames,))
    given = er.sanitise(er.records(W, H), W, H, (1,))
    assert list(given["count"]) == [0, 1, 2]      # (of the four, one lies outside and one is of frame 0)
    assert list(er.sanitise(er.records(W, H), W, H, (0, 1))["count"]) == [0, 1, 3]


def test_frame0_only_and_missing_planes(ofdg):
    W, H = 24, 6
    images, occ, flow = er.frames(W, H), er.maps(W, H), er.flows(W, H)
    for kw in (dict(frames=(0,)), dict(frames=(0,), mark_occ=False), dict(frames=(1,), mark_occ=True)):
        got, want = run_both(ofdg, images, occ, flow, recs=er.records_edges(W, H), fill=er.CONST, color=COLOR, **kw)
        expect_same(got, want, str(kw))
    # frame 1 only: image0, occ1 and flow1 need not be there
    got, want = run_both(ofdg, (None, images[1]), (occ[0], None), (flow[0], None), recs=er.records(W, H))
    expect_same(got, want, "frame 1, occ0 alone")
    er.expect_equal([got[0][1]], [run_both(ofdg, images, None, None, recs=er.records(W, H))[0][0][1]], "the maps do not change the frames")


def q8_frame(qs, P=16):
    """a float32 channel of P elements whose Q8 values are qs (the rest 0), as [1,3,2,8] with the same channel three times"""
    ch = np.zeros(P, np.float32)
    ch[:len(qs)] = np.array(qs, np.float64) / 256.0
    return np.tile(ch.reshape(1, 1, 2, 8), (1, 3, 1, 1))


def fill_of(ofdg, frame):
    rec = np.zeros((1,), er.REC)
    rec[0]["count"] = 1
    rec[0]["rect"][0] = (0, 0, 1, 1, 1)
    used = ofdg.host_erase((None, np.array(frame)), recs=rec)
    return [int(v) for v in used[0]["fill"][1]]


def test_mean_known_answers(ofdg):
    """Worked out here, P = 16: mean_q8 = (2 S + 16) // 32 and m = (mean_q8 + 128) >> 8."""
    assert (2 * 8 + 16) // 32 == 1 and er.mean_byte(8, 16) == 0        # S = 8: 0.5 rounds half up to mean_q8 1
    assert (127 + 128) >> 8 == 0 and (128 + 128) >> 8 == 1              # m at mean_q8 127 and 128
    assert (2 * 2039 + 16) // 32 == 127 and (2 * 2040 + 16) // 32 == 128   # 127.44 -> 127, 127.5 -> 128 (half up)
    assert fill_of(ofdg, q8_frame([2039])) == [0, 0, 0]                 # mean_q8 127
    assert fill_of(ofdg, q8_frame([2040])) == [1, 1, 1]                 # mean_q8 127.5 -> 128
    assert fill_of(ofdg, q8_frame([2048])) == [1, 1, 1]                 # mean_q8 128
    # q of 1/512 is 0 (0.5 ties to even), of 3/512 is 2 (1.5 ties to even), of 1/256 is 1
    for value, q in ((1.0 / 512, 0), (3.0 / 512, 2), (1.0 / 256, 1)):
        assert int(er.q8(np.array([value], np.float32))[0]) == q
        frame = q8_frame([2039, 0])
        frame[0, :, 0, 1] = value
        assert fill_of(ofdg, frame) == [1 if 2039 + q >= 2040 else 0] * 3, value
    # NaN and negatives count as 0, everything above 255 as 255: S = 16 * 255 * 256 for a channel of 1e9, +inf, 255.5, 300
    frame = q8_frame([])
    frame[0, 0] = 1e9
    frame[0, 1] = np.array([np.nan, -3.0, -np.inf, 1e-45, -0.0, 0.0, np.nan, -1e9] * 2, np.float32).reshape(2, 8)
    frame[0, 2] = np.array([np.inf, 255.5, 300.0, 255.0] * 4, np.float32).reshape(2, 8)
    assert fill_of(ofdg, frame) == [255, 0, 255]
    # an all-255 frame at 264 x 200, in both formats
    for dtype in (np.uint8, np.float32):
        assert fill_of(ofdg, np.full((1, 3, 200, 264), 255, dtype)) == [255, 255, 255]


def test_same_fill_in_both_formats_and_mean_of_the_unerased_frame(ofdg):
    W, H = 264, 200
    _, image1 = er.frames(W, H, "uint8")
    recs = np.zeros((er.N,), er.REC)
    recs["count"] = 4
    recs["rect"] = [(0, 0, W, H // 2, 1), (0, H // 2, W // 2, H, 1), (W // 2, H // 2, W, H // 4, 1), (5, 5, W - 10, H - 10, 1)]
    u8, f32 = np.array(image1), image1.astype(np.float32)
    used_u8 = ofdg.host_erase((None, u8), recs=recs)
    used_f32 = ofdg.host_erase((None, f32), recs=recs)
    assert er.equal_bits(used_u8, used_f32)
    assert np.array_equal(u8.astype(np.float32), f32)
    # the mean is that of the frame as it was, worked out here in exact integers: round half up of the mean to Q8, then to a byte
    for i in range(er.N):
        for c in range(3):
            S, P = int(image1[i, c].astype(np.int64).sum()) * 256, W * H
            assert int(used_u8[i]["fill"][1][c]) == (((2 * S + P) // (2 * P)) + 128) >> 8
            assert (u8[i, c, 5:H - 5, 5:W - 5] == used_u8[i]["fill"][1][c]).all()


def test_occlusion_rule_at_the_edges(ofdg):
    """One rectangle of frame 1, x 10..13, y 2..3, in a 24 x 6 plane.  Targets exactly on each edge are inside, one pixel
    further outside; the + 0.5 ties go up; NaN and infinities are in no rectangle; non-zero elements keep their bits."""
    W, H = 24, 6
    rec = np.zeros((1,), er.REC)
    rec[0]["count"] = 1
    rec[0]["rect"][0] = (10, 2, 4, 2, 1)
    cases = [  # (x, y, u, v, marked)
        (0, 0, 10.0, 2.0, True), (0, 1, 9.0, 1.0, False), (1, 0, 12.0, 3.0, True), (1, 1, 13.0, 2.0, False), (2, 0, 8.0, 3.0, True),
        (2, 1, 8.0, 3.0, False),                                    # (y = 1: target row 4)
        (3, 0, 6.5, 2.0, True), (3, 1, 6.49, 1.0, False),            # 3 + 6.5 + 0.5 = 10 exactly; 9.99 floors to 9
        (4, 0, 9.5, 1.5, False),                                     # 4 + 9.5 + 0.5 = 14: one outside the right edge
        (5, 5, 5.0, -3.5, True),                                     # 5 - 3.5 + 0.5 = 2
        (6, 5, 4.0, -1.5, False),                                    # 5 - 1.5 + 0.5 = 4
        (7, 2, np.nan, 0.0, False), (8, 2, np.inf, 0.0, False), (9, 2, 1.0, -np.inf, False), (9, 3, 1.0, np.nan, False),
        (20, 2, -65504.0, 0.0, False), (20, 3, -7.0, -0.0, True), (21, 3, 65504.0, 0.0, False), (23, 5, -10.0, -2.0, True),
        (23, 4, -9.49, -2.0, False),                                 # 23 - 9.49 + 0.5 = 14.01
    ]
    for flow_dtype in ("float32", "float16"):
        for occ_dtype in ("float32", "uint8"):
            flow = np.full((1, 2, H, W), 100.0, flow_dtype)          # everything else points far away
            for x, y, u, v, _ in cases:
                flow[0, :, y, x] = (u, v)
            occ0 = np.zeros((1, 1, H, W), occ_dtype)
            occ0[0, 0, 0, 23] = 7                                    # (not marked: stays 7)
            occ0[0, 0, 0, 0] = 5                                     # (marked: becomes 1)
            before = np.array(occ0)
            image1 = np.zeros((1, 3, H, W), np.uint8)
            got, want = run_both(ofdg, (None, image1), (occ0, None), (flow, None), recs=rec)
            expect_same(got, want, "%s %s" % (flow_dtype, occ_dtype))
            out = got[1][0][0, 0]
            expected = np.array(before[0, 0])
            for x, y, u, v, marked in cases:
                if flow_dtype == "float16" and (u, v) in ((6.49, 1.0), (-9.49, -2.0)):
                    marked = bool(er.marks(er.sanitise(rec, W, H)[0], 0, True, flow[0].astype(np.float32), W, H)[y, x])
                if marked:
                    expected[y, x] = 1
            assert er.equal_bits(out, expected), (flow_dtype, occ_dtype, np.argwhere(out != expected))
            # the map of frame 1 itself: exactly the rectangle, and no flow is needed
            occ1 = np.zeros((1, 1, H, W), occ_dtype)
            ofdg.host_erase((None, np.array(image1)), (None, occ1), None, recs=rec)
            direct = np.zeros((H, W), occ_dtype)
            direct[2:4, 10:14] = 1
            assert er.equal_bits(occ1[0, 0], direct)


def test_without_the_flag_maps_and_flows_are_not_looked_at(ofdg):
    W, H, n = 24, 6, 2
    lib = ofdg.lib()
    image1 = np.zeros((n, 3, H, W), np.uint8)
    recs = np.zeros((n,), er.REC)
    recs["count"] = 1
    recs["rect"][:, 0] = (2, 1, 5, 3, 1)
    for garbage in (0, 0x10, 0xDEAD0001):
        j = ofdg.EraseJob()
        j.image[1], j.recs = image1.ctypes.data, recs.ctypes.data
        j.flags, j.fill, j.image_fmt = ofdg.ERASE_FRAME1, ofdg.ERASE_CONST, ofdg.FMT_U8
        j.occ_fmt, j.flow_fmt = 77, -5                               # (not looked at either)
        for f in range(2):
            j.occ[f], j.flow[f] = garbage or None, garbage or None
        j.color[0], j.color[1], j.color[2] = 1, 2, 3
        image1[:] = 0
        assert lib.ofdg_host_erase(C.byref(j), n, W, H) == ofdg.OK, lib.ofdg_host_last_error()
        assert (image1[:, 2, 1:4, 2:7] == 3).all() and int(image1.sum()) == n * 15 * 6


def test_draw_equals_restatement_and_recorded_values(ofdg):
    ranges = dict(er.RAFT, prob=1.0, max_rects=4)
    for frames in ((1,), (0,), (0, 1)):
        for index in (0, 1, 2, 2 ** 32 + 3, -1 & 0x7FFFFFFFFFFFFFFF):
            got = ofdg.erase_draw(2024, index, 512, 384, ranges, frames)
            want = er.draw(2024, index, 512, 384, ranges, frames)
            assert er.equal_bits(np.array(got), np.array(want)), (frames, index, got, want)
    for index, count, rects in RECORDED:
        got = ofdg.erase_draw(2024, index, 512, 384, ranges, (0, 1))
        assert int(got["count"]) == count and got["rect"][:count].tolist() == rects, (index, got)
        assert not got["rect"][count:].any() and not got["fill"].any() and not got["reserved"].any()
    # ERASE_RAFT itself
    assert ofdg.ERASE_RAFT == er.RAFT
    # prob 0: never; prob 1: always; the draw does not clip
    for index in range(200):
        assert int(ofdg.erase_draw(1, index, 64, 32, dict(er.RAFT, prob=0.0))["count"]) == 0
        r = ofdg.erase_draw(1, index, 64, 32, dict(er.RAFT, prob=1.0))
        assert 1 <= int(r["count"]) <= 2 and (r["rect"][:int(r["count"]), 2:4] >= 50).all() and (r["rect"][:, 4] == (np.arange(4) < r["count"])).all()


# recorded from the restatement: seed 2024, a 512 x 384 plane, ERASE_RAFT with prob 1 and 1..4 rectangles, both frames:
# (index, count, rectangles as x0, y0, w, h, frame)
RECORDED = [
    (0, 4, [[488, 236, 85, 51, 1], [150, 56, 74, 69, 1], [75, 149, 70, 50, 1], [182, 105, 52, 50, 1]]),
    (1, 2, [[452, 212, 76, 53, 0], [178, 269, 94, 83, 0]]),
    (2, 2, [[156, 241, 96, 65, 1], [345, 184, 67, 69, 1]]),
    (2 ** 32 + 3, 1, [[318, 380, 63, 51, 0]]),
]


def test_draw_statistics(ofdg):
    """20 000 indices at seed 12345 with ERASE_RAFT on 512 x 384: the share of erased samples (p = 1/2), the mean count (0.75:
    0 with 1/2, 1 and 2 with 1/4 each; variance 0.6875) and the mean size (uniform in 50..99: 74.5, variance (50^2 - 1) / 12),
    each within 6 standard errors.  The seed is fixed, so this either passes always or never."""
    n = 20000
    counts, sizes = [], []
    for index in range(n):
        r = ofdg.erase_draw(12345, index, 512, 384, er.RAFT)
        c = int(r["count"])
        counts.append(c)
        sizes.extend(r["rect"][:c, 2:4].reshape(-1).tolist())
        assert (r["rect"][:c, 0] < 512).all() and (r["rect"][:c, 1] < 384).all() and (r["rect"][:c, :2] >= 0).all()
    counts, sizes = np.array(counts), np.array(sizes)
    share = (counts > 0).mean()
    assert abs(share - 0.5) <= 6 * math.sqrt(0.25 / n), share
    assert abs(counts.mean() - 0.75) <= 6 * math.sqrt(0.6875 / n), counts.mean()
    assert set(np.unique(counts)) == {0, 1, 2} and sizes.min() == 50 and sizes.max() == 99
    assert abs(sizes.mean() - 74.5) <= 6 * math.sqrt((50 ** 2 - 1) / 12.0 / sizes.size), sizes.mean()


def test_noise_statistics(ofdg):
    """The noise fill on one rectangle of 264 x 200 x 3 bytes at a fixed seed: uniform bytes - mean 127.5, variance (256^2 - 1) /
    12, fourth central moment (n^2 - 1)(3 n^2 - 7) / 240 with n = 256 -, mean and variance each within 6 standard errors."""
    W, H = 264, 200
    rec = np.zeros((1,), er.REC)
    rec[0]["count"] = 1
    rec[0]["rect"][0] = (0, 0, W, H, 1)
    image1 = np.zeros((1, 3, H, W), np.uint8)
    ofdg.host_erase((None, image1), recs=rec, fill=er.NOISE, seed=99, first_index=5)
    x = image1.astype(np.float64).reshape(-1)
    var, m4 = (256.0 ** 2 - 1) / 12.0, (256.0 ** 2 - 1) * (3 * 256.0 ** 2 - 7) / 240.0
    assert abs(x.mean() - 127.5) <= 6 * math.sqrt(var / x.size), x.mean()
    assert abs(((x - 127.5) ** 2).mean() - var) <= 6 * math.sqrt((m4 - var * var) / x.size), x.var()
    assert len(np.unique(image1)) == 256
    as_float = np.zeros((1, 3, H, W), np.float32)
    ofdg.host_erase((None, as_float), recs=rec, fill=er.NOISE, seed=99, first_index=5)
    assert np.array_equal(as_float, image1.astype(np.float32))


def test_struct_layout(ofdg):
    J, R = ofdg.EraseJob, ofdg.EraseRec
    assert C.sizeof(R) == 96 and C.sizeof(ofdg.EraseRect) == 20 and C.sizeof(J) == 152 and er.REC.itemsize == 96
    assert {name: getattr(R, name).offset for name, _ in R._fields_} == dict(count=0, rect=4, fill=84, reserved=90)
    assert {name: er.REC.fields[name][1] for name in er.REC.names} == dict(count=0, rect=4, fill=84, reserved=90)
    assert {name: getattr(J, name).offset for name, _ in J._fields_} == dict(
        image=0, occ=16, flow=32, recs=48, recs_out=56, work=64, first_index=72, seed=80, width=84, height=88, image_fmt=92, occ_fmt=96,
        flow_fmt=100, flags=104, fill=108, min_rects=112, max_rects=116, min_size=120, max_size=124, prob=128, color=132, reserved=144)
    assert (ofdg.ERASE_MAX_RECTS, ofdg.ERASE_FRAME0, ofdg.ERASE_FRAME1, ofdg.ERASE_OCC, ofdg.ERASE_WORK_BYTES, ofdg.ERASE_REC_WORDS) == (4, 1, 2, 4, 64, 24)
    assert (ofdg.ERASE_MEAN, ofdg.ERASE_CONST, ofdg.ERASE_NOISE) == (0, 1, 2)
    for name in ("ofdg_erase", "ofdg_host_erase", "ofdg_erase_draw"):
        assert name in ofdg.EXPORTS
    a = np.arange(48, dtype=np.int32).reshape(2, 24)
    s = ofdg.erase_numpy(a)
    assert s.shape == (2,) and int(s[1]["count"]) == 24 and s[0]["rect"].tolist() == np.arange(1, 21).reshape(4, 5).tolist()


def test_refusals_write_nothing(ofdg):
    W, H, n = 24, 6, 2
    lib = ofdg.lib()
    flows = [np.zeros((n, 2, H, W), np.float32) for _ in range(2)]
    plane = n * H * W
    # one buffer for everything written (two uint8 frames, two uint8 maps, the records), so that overlaps are offsets
    raw = np.full(8 * plane + 96 * n + 64, FILL, np.uint8)
    base = raw.ctypes.data
    recs_in = np.zeros((n,), er.REC)
    recs_in["count"] = 1
    recs_in["rect"][:, 0] = (1, 1, 9, 3, 1)

    def job(**kw):
        j = ofdg.EraseJob()
        for f in range(2):
            j.image[f], j.occ[f], j.flow[f] = base + 3 * plane * f, base + 6 * plane + plane * f, flows[f].ctypes.data
        j.recs_out = base + 8 * plane
        j.image_fmt, j.occ_fmt, j.flow_fmt = ofdg.FMT_U8, ofdg.FMT_U8, ofdg.FMT_F32
        j.flags, j.fill = ofdg.ERASE_FRAME0 | ofdg.ERASE_FRAME1 | ofdg.ERASE_OCC, ofdg.ERASE_MEAN
        j.prob, j.min_rects, j.max_rects, j.min_size, j.max_size = 1.0, 1, 4, 1, 9
        for k, v in kw.items():
            if isinstance(v, dict):
                for idx, val in v.items():
                    getattr(j, k)[idx] = val
            else:
                setattr(j, k, v)
        return j

    def refused(word, j, n_samples=n, w=W, h=H):
        rc = lib.ofdg_host_erase(None if j is None else C.byref(j), n_samples, w, h)
        assert rc == ofdg.EINVAL, word
        msg = lib.ofdg_host_last_error().decode()
        assert msg.startswith("ofdg_host_erase: ") and word in msg, (word, msg)
        assert (raw == FILL).all(), word

    refused("job", None)
    refused("n_samples", job(), n_samples=0)
    refused("both be 0", job(width=W))
    refused("plane size given", job(width=W + 8, height=H))
    for bad_w, bad_h in ((20, 6), (24, 5), (4, 2), (8, 0)):
        refused("width", job(), w=bad_w, h=bad_h)
    refused("2^31", job(), n_samples=1, w=32768, h=32768)
    refused("image_fmt", job(image_fmt=ofdg.FMT_F16))
    refused("occ_fmt", job(occ_fmt=ofdg.FMT_F16))
    refused("flow_fmt", job(flow_fmt=ofdg.FMT_U8))
    refused("flags holds unknown bits", job(flags=8 | 2))
    refused("flags holds unknown bits", job(flags=-1))
    refused("reserved", job(reserved={0: 1}))
    refused("reserved", job(reserved={1: -1}))
    refused("OFDG_ERASE_FRAME0 or OFDG_ERASE_FRAME1", job(flags=ofdg.ERASE_OCC))
    refused("no frame is set", job(image={0: None, 1: None}))
    refused("flagged frame has no image", job(image={0: None}))
    refused("fill", job(fill=3))
    refused("fill", job(fill=-1))
    for c, bad in ((0, 256), (1, -1), (2, 1 << 20)):
        refused("color", job(fill=ofdg.ERASE_CONST, color={c: bad}))
    for bad in (float("nan"), -0.001, 1.0001, float("inf")):
        refused("prob", job(prob=bad))
    for lo, hi in ((-1, 2), (0, 5), (3, 2)):
        refused("min_rects", job(min_rects=lo, max_rects=hi))
    for lo, hi in ((0, 5), (1, 32768), (9, 8)):
        refused("min_size", job(min_size=lo, max_size=hi))
    refused("needs a map", job(occ={0: None, 1: None}))
    refused("needs its flow", job(flow={0: None}))
    refused("needs its flow", job(flow={1: None}))
    refused("overlaps", job(image={1: base + 3 * plane - 1}))                    # image1 starts on the last byte of image0
    refused("overlaps", job(occ={0: base + 6 * plane - 1}))                      # occ0 on the last byte of image1
    refused("overlaps", job(recs_out=base + 8 * plane - 1))                      # the records on the last byte of occ1
    refused("overlaps", job(occ={1: flows[1].ctypes.data + 4}))                  # a map inside a flow
    refused("overlaps", job(flow={0: base + 8}))                                 # a flow inside a written frame
    refused("overlaps", job(recs=base + 8 * plane + 96))                         # the given records inside the written ones
    refused("overlaps", job(image={0: base, 1: base}))
    # the draw
    out = np.full(96, FILL, np.uint8)
    for word, kw, w, h in (("prob", dict(prob=float("nan")), W, H), ("min_rects", dict(max_rects=5), W, H), ("min_size", dict(min_size=0), W, H),
                           ("FRAME", dict(flags=0), W, H), ("unknown", dict(flags=16 | 1), W, H), ("1..32768", {}, 0, H), ("1..32768", {}, W, 32769)):
        j = job(**kw)
        assert lib.ofdg_erase_draw(1, 0, w, h, C.byref(j), out.ctypes.data_as(C.POINTER(ofdg.EraseRec))) == ofdg.EINVAL, word
        msg = lib.ofdg_host_last_error().decode()
        assert msg.startswith("ofdg_erase_draw: ") and word in msg, (word, msg)
        assert (out == FILL).all()
    assert lib.ofdg_erase_draw(1, 0, W, H, None, out.ctypes.data_as(C.POINTER(ofdg.EraseRec))) == ofdg.EINVAL
    assert lib.ofdg_erase_draw(1, 0, W, H, C.byref(job()), None) == ofdg.EINVAL and (out == FILL).all()
    # the ranges are not read with given records; a flow is not needed for a map whose other frame is not flagged; the job's own size
    raw[:8 * plane] = 0
    ok = job(recs=recs_in.ctypes.data, prob=float("nan"), min_size=-4, flags=ofdg.ERASE_FRAME1 | ofdg.ERASE_OCC, flow={0: flows[0].ctypes.data, 1: None},
             image={0: None}, width=W, height=H, fill=ofdg.ERASE_CONST)
    ok.color[1] = 200
    assert lib.ofdg_host_erase(C.byref(ok), n, W, H) == ofdg.OK, lib.ofdg_host_last_error()
    frames = raw[:6 * plane].reshape(2, n, 3, H, W)
    maps = raw[6 * plane:8 * plane].reshape(2, n, 1, H, W)
    assert not frames[0].any() and (frames[1][:, 1, 1:4, 1:10] == 200).all() and int(frames[1].sum()) == 200 * 27 * n
    assert (maps[1][:, 0, 1:4, 1:10] == 1).all() and int(maps[1].sum()) == 27 * n and (maps[0][:, 0, 1:4, 1:10] == 1).all()
    used = raw[8 * plane:8 * plane + 96 * n].view(er.REC)
    assert used["count"].tolist() == [1, 1] and used["fill"][:, 1].tolist() == [[0, 200, 0]] * n
    assert (raw[8 * plane + 96 * n:] == FILL).all()


def test_erase_format_raises(ofdg):
    z = np.zeros
    img, occ, flow = z((2, 3, 6, 24), np.uint8), z((2, 1, 6, 24), np.float32), z((2, 2, 6, 24), np.float16)
    assert ofdg.erase_format((None, img), (occ, None), (flow, None)) == (2, 6, 24, ofdg.FMT_U8, ofdg.FMT_F32, ofdg.FMT_F16)
    assert ofdg.erase_format((img, img)) == (2, 6, 24, ofdg.FMT_U8, ofdg.FMT_F32, ofdg.FMT_F32)
    for bad in (dict(images=(None, None)), dict(images=(img,)), dict(images=(img, img.astype(np.float32))), dict(images=(img, img[:1])),
                dict(images=(img.astype(np.float16), None)), dict(images=(img[:, :2], None)), dict(occ=(occ, occ.astype(np.uint8))),
                dict(occ=(occ[:, :, :4], None)), dict(occ=(z((2, 6, 24), np.float32), None)), dict(flow=(flow.astype(np.float64), None)),
                dict(flow=(flow, flow.astype(np.float32))), dict(flow=(occ, None)), dict(height=8, width=24)):
        kw = dict(dict(images=(img, img), occ=(occ, occ), flow=(flow, flow)), **bad)
        with pytest.raises(ValueError):
            ofdg.erase_format(kw.pop("images"), **kw)
    with pytest.raises(ValueError):
        ofdg.host_erase((None, img), ranges=dict(size=3))
    with pytest.raises(ValueError):
        ofdg.host_erase((None, img), frames=(2,))
    with pytest.raises(ValueError):
        ofdg.host_erase((None, img), frames=(0,))                    # image0 is None
    with pytest.raises(ValueError):
        ofdg.host_erase((None, img), mark_occ=True)                  # no map
    with pytest.raises(ValueError):
        ofdg.host_erase((img, img), (None, occ), None, frames=(0, 1))   # occ1 needs flow1
    with pytest.raises(ValueError):
        ofdg.host_erase((None, img), fill=5)
    with pytest.raises(ValueError):
        ofdg.host_erase((None, img.transpose(0, 1, 3, 2)))
