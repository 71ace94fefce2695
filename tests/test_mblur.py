"""CPU tests of motion blur (ofdg_motion_blur_draw, ofdg_host_motion_blur; include/ofdg.h): the host twin against the numpy
restatement (tests/mblur_reference.py) byte for byte over formats, sizes, tap caps and subsets of frames, the known answers of
the definition, its rounding boundaries, given records, the draw against the restatement and recorded answers, its moments,
composition of batches and every refusal.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import mblur_reference as mr

GRID, KNOWN = mr.GRID, mr.KNOWN


@pytest.mark.parametrize("W,H,src_dtype,dst_dtype,flow_dtype,taps_side", GRID)
def test_host_equals_restatement(ofdg, W, H, src_dtype, dst_dtype, flow_dtype, taps_side):
    """Shutters 0, 0.5 and (2, 1.25); flows with sub-pixel parts, beyond the clamp and the cap, leaving every border and corner,
    with NaN, infinities, -0.0, denormals and +-65504 in samples 1 and 2; float32 frames with fractions, NaN, -3, 255.5, 1e9."""
    images, flows, recs, want, used = mr.case(W, H, src_dtype, flow_dtype, taps_side)
    what = "%dx%d %s to %s, flow %s, taps_side %d" % (W, H, src_dtype, dst_dtype, flow_dtype, taps_side)
    got, got_recs = ofdg.host_motion_blur(images, flows, recs=recs, taps_side=taps_side, dst_dtype=dst_dtype)
    mr.expect_equal(got, want[dst_dtype], what)
    assert mr.equal_bits(got_recs, used) and mr.equal_bits(used, recs)
    # sample 0 has shutter 0: the source bytes
    for f in range(2):
        assert np.array_equal(got[f][0].astype(np.int64), mr.pr.index_of(images[f][0]))
    # frame 0 alone and frame 1 alone give that frame's bytes
    only0, _ = ofdg.host_motion_blur((images[0], None), (flows[0], None), recs=recs, taps_side=taps_side, dst_dtype=dst_dtype)
    mr.expect_equal(only0, (want[dst_dtype][0], None), what + ", frame 0 alone")
    only1, _ = ofdg.host_motion_blur((None, images[1]), (None, flows[1]), recs=recs, taps_side=taps_side, dst_dtype=dst_dtype)
    mr.expect_equal(only1, (None, want[dst_dtype][1]), what + ", frame 1 alone")


def test_the_data_holds_what_it_should():
    images, flows, recs, want, _ = mr.case(264, 200, "float32", "float32", 16)
    flat = images[0].reshape(-1)
    assert np.isnan(flat).any() and all((flat == v).any() for v in (-3.0, 255.5, 1e9, 0.5))
    for f in range(2):
        fl = flows[f]
        assert not np.isnan(fl[0]).any() and np.isnan(fl[1]).any() and np.isinf(fl[2]).any() and (np.abs(fl[1]) == 65504).any()
        assert (np.signbit(fl[1]) & (fl[1] == 0)).any() and ((fl[2] != 0) & (np.abs(fl[2]) < 1e-38)).any()
        Dx, Dy = mr.half_displacement(fl[2], 2.0)
        m = mr.taps(Dx, Dy, 16)[0]
        assert np.abs(Dx).max() == 8192 and np.abs(Dy).max() == 8192 and m.max() == 16 and m.min() == 0
        assert (((np.maximum(np.abs(Dx), np.abs(Dy)) + 255) >> 8) > 16).any()  # beyond the cap
        for ys, xs in ((0, 0), (0, -1), (-1, 0), (-1, -1), (100, 0), (100, -1), (0, 132), (-1, 132)):  # corners and borders: streaks leave
            assert m[ys, xs] > 0, (ys, xs)
    assert not np.array_equal(want["float32"][0][1], want["float32"][0][0]) and len(np.unique(flows[0][0].reshape(2, -1), axis=1).T) > 10


def test_the_data_takes_every_path_of_the_kernel():
    """The kernel's 64 x 16 tiles (csrc/kernels.hip) copy where no pixel has a tap beside its centre, stage a window where every
    tap lies within 16 px of its pixel, and gather from global memory otherwise (mr.tile_paths restates the rule).  The three
    sets of flows: with the special values every tile of samples 1 and 2 holds a +-65504 and gathers, at every size; without
    them 264x200 has all three kinds side by side, but the one tile of 8x2 and of 24x6 still holds a streak beyond the halo; the
    gentle set is staged everywhere - at 8x2 and 24x6, where the window exceeds the plane on all four sides, the one tile is a
    copy in sample 0 and a window in samples 1 and 2, under every cap and in both frames."""
    recs = mr.sanitise(mr.records())
    kinds = lambda fl, i, f, t: set(mr.tile_paths(fl[f][i], recs[i][f], t))  # noqa: E731
    for W, H in mr.SIZES:
        with_special, plain, gentle = mr.flows(W, H, "float32"), mr.flows(W, H, "float32", special=False), mr.flows(W, H, "float16", gentle=True)
        for f in range(2):
            for t in (1, 4, 16):
                assert kinds(with_special, 0, f, t) == kinds(plain, 0, f, t) == kinds(gentle, 0, f, t) == {"copy"}, (W, H, f, t)
                for i in (1, 2):
                    assert kinds(with_special, i, f, t) == {"gather"}, (W, H, f, t, i)
                    assert kinds(gentle, i, f, t) - {"copy"} == {"window"}, (W, H, f, t, i)
                    if (W, H) in ((8, 2), (24, 6)):
                        assert kinds(plain, i, f, t) == {"gather"} and kinds(gentle, i, f, t) == {"window"}, (W, H, f, t, i)
        if (W, H) == (264, 200):
            assert kinds(plain, 1, 0, 16) == {"gather", "window"} and kinds(plain, 2, 0, 16) == {"gather", "window", "copy"}
            # the three planted streaks of the plain set, where the flows' docstring puts them
            for i in (1, 2):
                Dx, Dy = mr.half_displacement(plain[0][i], recs[i][0])
                m, sx, sy = mr.taps(Dx, Dy, 16)
                far = (m * np.abs(sx) > 4096) | (m * np.abs(sy) > 4096)
                assert m[15, 63] > 0 and m[16, 64] > 0 and not far[15, 63]         # across the corner of four tiles
                assert m[100, 100] * abs(sx[100, 100]) > 256 * 16 * (i - 1)         # 25 px at shutter 0.5 fits the halo, 50 px at 2 does not
                assert far[150, 200] == (i == 2) and abs(sx[150, 200]) >= 256       # 32 px: taps a whole pixel and more apart
    # the gentle set reaches the cap of 16 taps, the halo's edge and every border and corner
    Dx, Dy = mr.half_displacement(mr.flows(24, 6, "float32", gentle=True)[0][2], 2.0)
    m, sx, sy = mr.taps(Dx, Dy, 16)
    assert m.max() == 16 and 3900 < (m * np.abs(sx)).max() <= 4096 and all(m[y, x] > 0 for y in (0, -1) for x in (0, -1))


@pytest.mark.parametrize("W,H", mr.SIZES[:3])
@pytest.mark.parametrize("src_dtype,dst_dtype,flow_dtype", mr.FORMATS)
def test_host_equals_restatement_on_the_gentle_flows(ofdg, W, H, src_dtype, dst_dtype, flow_dtype):
    for taps_side in (16, 4):
        images, flows, recs, want, used = mr.case(W, H, src_dtype, flow_dtype, taps_side, gentle=True)
        got, got_recs = ofdg.host_motion_blur(images, flows, recs=recs, taps_side=taps_side, dst_dtype=dst_dtype)
        mr.expect_equal(got, want[dst_dtype], "gentle %dx%d %s to %s, flow %s, taps_side %d" % (W, H, src_dtype, dst_dtype, flow_dtype, taps_side))
        assert mr.equal_bits(got_recs, used) and not np.array_equal(got[0][1].astype(np.int64), mr.pr.index_of(images[0][1]))


@pytest.mark.parametrize("vec,shutter,taps_side,answer", KNOWN)
def test_known_answers(ofdg, vec, shutter, taps_side, answer):
    img, fl, rec = mr.impulse(vec[0], vec[1], shutter)
    want = np.zeros((6, 24), np.uint8)
    for (x, y), b in answer.items():
        want[y, x] = b
    for dst_dtype in ("uint8", "float32"):
        (got, _), _ = ofdg.host_motion_blur((img, None), (fl, None), recs=rec, taps_side=taps_side, dst_dtype=dst_dtype)
        assert got.dtype == np.dtype(dst_dtype) and all(np.array_equal(got[0, c], want) for c in range(3)), (vec, got[0, 0])
    (ref, _), _ = mr.motion_blur((img, None), (fl, None), rec, taps_side)
    assert np.array_equal(ref, got.astype(np.uint8))


def test_constant_frames_and_zero_shutter(ofdg):
    flows = mr.flows(72, 40, "float32")
    for value in (0, 37, 255):
        const = tuple(np.full((mr.N, 3, 40, 72), value, np.uint8) for _ in range(2))
        got, _ = ofdg.host_motion_blur(const, flows, recs=mr.records(), taps_side=16)
        mr.expect_equal(got, const, "a constant frame stays constant")
    images = mr.frames(72, 40, "uint8")
    zero = np.zeros((mr.N, 4), np.float32)
    got, used = ofdg.host_motion_blur(images, flows, recs=zero, taps_side=16)
    mr.expect_equal(got, images, "shutter 0")
    assert mr.equal_bits(used, zero)
    got, used = ofdg.host_motion_blur(images, flows, seed=5, ranges=dict(prob=0.0, shutter_min=1.0, shutter_max=2.0), taps_side=16)
    mr.expect_equal(got, images, "prob 0")
    assert mr.equal_bits(used, zero)
    still = tuple(np.zeros_like(t) for t in flows)
    got, _ = ofdg.host_motion_blur(images, still, recs=mr.records(), taps_side=16)
    mr.expect_equal(got, images, "zero flow")
    f32 = mr.frames(72, 40, "float32")
    got, _ = ofdg.host_motion_blur(f32, flows, recs=zero, taps_side=16)  # float32 to float32 at shutter 0: (float)byte
    assert all(np.array_equal(g, mr.pr.index_of(s).astype(np.float32)) for g, s in zip(got, f32))


def blur_row(ofdg, u, v, shutter, taps_side=16):
    img, fl, rec = mr.impulse(u, v, shutter, W=40, H=6, at=(20, 3))
    (got, _), _ = ofdg.host_motion_blur((img, None), (fl, None), recs=rec, taps_side=taps_side)
    (ref, _), _ = mr.motion_blur((img, None), (fl, None), rec, taps_side)
    assert np.array_equal(got, ref)
    return got[0, 0]


def test_rounding_boundaries(ofdg):
    """D: 0.0039 px is D = 0, 0.004 px is D = 1 (0.4992 and 0.512 of a 24.8 unit); ties of rintf go to even: u = 2.5 / 128 is
    D = 2, 3.5 / 128 is D = 4.  m: L = 256 is one tap a side, L = 257 two.  s: D = 3, m = 2 steps by rintf(1.5) = 2, D = 5,
    m = 2 by rintf(2.5) = 2 - seen through the restatement's own functions and through the twin's pixels."""
    f = lambda u: mr.half_displacement(np.array([[[u]], [[0.0]]], np.float32), 1.0)[0][0, 0]  # noqa: E731
    assert [f(0.0039), f(0.004), f(2.5 / 128), f(3.5 / 128), f(-2.5 / 128), f(0.5 / 128), f(1.5 / 128)] == [0, 1, 2, 4, -2, 0, 2]
    assert [f(64.0), f(64.01), f(-1e30), f(3e38)] == [8192, 8192, -8192, 8192]
    img, fl, rec = mr.impulse(0.0039, 0.0, 1.0)
    assert np.array_equal(ofdg.host_motion_blur((img, None), (fl, None), recs=rec, taps_side=16)[0][0], img)
    # D = 1: three taps 1/256 px apart, t = 65280, 65025, 65025 at the centre: S = 21846 * 65280 + 2 * 21845 * 65025 = 254.3 * 2^24;
    # a neighbour's one tap that reaches the pixel has t = 255: 21845 * 255 is below half of 2^24
    row = blur_row(ofdg, 0.004, 0.0, 1.0)
    assert row[3, 19:22].tolist() == [0, 254, 0] and (21846 * 65280 + 2 * 21845 * 65025 + (1 << 23)) >> 24 == 254 and row.sum() == 254
    m = lambda D: int(mr.taps(np.array([D]), np.array([0]), 16)[0][0])  # noqa: E731
    assert [m(0), m(1), m(256), m(257), m(512), m(513), m(8192)] == [0, 1, 1, 2, 2, 3, 16]
    # L = 256 (u = 2 px at shutter 1): N = 3 at -1, 0, +1 px; L = 257 (u = 2 + 1/128 px): N = 5, steps of rintf(128.5) = 128
    assert blur_row(ofdg, 2.0, 0.0, 1.0)[3, 18:23].tolist() == [0, 85, 85, 85, 0]
    assert np.count_nonzero(blur_row(ofdg, 2.0 + 1.0 / 128, 0.0, 1.0)[3]) == 3 and int(mr.taps(np.array([257]), np.array([0]), 16)[1][0]) == 128
    s = lambda D, mm: int(mr.taps(np.array([D]), np.array([256 * mm]), 16)[1][0])  # noqa: E731
    assert [s(3, 2), s(5, 2), s(7, 2), s(-3, 2), s(-5, 2), s(10, 4)] == [2, 2, 4, -2, -2, 2]
    # the same ties through the twin: v = 4 px (Dy = 512, m = 2), u chosen so that Dx = 3 and 5
    for Dx in (3, 5, 7):
        img, fl, rec = mr.impulse(Dx / 128.0, 4.0, 1.0, W=40, H=8, at=(20, 4))
        (got, _), _ = ofdg.host_motion_blur((img, None), (fl, None), recs=rec, taps_side=16)
        (ref, _), _ = mr.motion_blur((img, None), (fl, None), rec, 16)
        assert np.array_equal(got, ref), Dx


def test_given_records_are_sanitised(ofdg):
    images, flows = mr.frames(24, 6, "uint8"), mr.flows(24, 6, "float32")
    recs = np.array([[np.nan, -1.0, 0, 0], [2.5, np.inf, 0, 0], [-0.0, 1.0, 0, 0]], np.float32)
    recs.view(np.int32)[:, 2:] = [[7, -1], [0, 1 << 30], [5, 5]]  # non-zero reserved words in a given record are cleared
    got, used = ofdg.host_motion_blur(images, flows, recs=recs, taps_side=16)
    assert used.tolist() == [[0, 0, 0, 0], [2, 2, 0, 0], [0, 1, 0, 0]] and not np.signbit(used).any()
    assert mr.equal_bits(used, mr.sanitise(recs))
    want, _ = mr.motion_blur(images, flows, recs, 16)
    mr.expect_equal(got, want, "given records")
    assert np.array_equal(got[0][0], images[0][0]) and np.array_equal(got[0][2], images[0][2]) and not np.array_equal(got[1][2], images[1][2])


# seed 12345, MBLUR_DEFAULT with prob 1: index -> shutter[0], shutter[1] (recorded from the restatement)
KNOWN_DRAWS = {
    0: ("0x1.4d7b8p-4", "0x1.17c7b4p-4"),
    1: ("0x1.3ab7eep-2", "0x1.2de716p-2"),
    2: ("0x1.93a25cp-3", "0x1.bfaf52p-4"),
    (1 << 32) + 3: ("0x1.de468p-2", "0x1.b2683ep-2"),
}


@pytest.mark.parametrize("index", [0, 1, 2, (1 << 32) + 3])
def test_draw(ofdg, index):
    q = dict(ofdg.MBLUR_DEFAULT, prob=1.0)
    got = ofdg.motion_blur_draw(12345, index, q)
    assert got.dtype == np.float32 and got.shape == (4,) and mr.equal_bits(got, mr.draw(12345, index, q))
    assert [float(got[0]), float(got[1])] == [float.fromhex(v) for v in KNOWN_DRAWS[index]]
    assert got[2] == 0 and got[3] == 0 and 0 <= got[0] < 0.5 and abs(got[1] - got[0]) <= 0.1 * 1.0001
    assert mr.equal_bits(ofdg.motion_blur_draw(12345, index, dict(q, prob=0.0)), np.zeros(4, np.float32))
    assert mr.equal_bits(ofdg.motion_blur_draw(12345, index, {}), np.zeros(4, np.float32))
    half = ofdg.motion_blur_draw(12345, index, ofdg.MBLUR_DEFAULT)  # prob 0.5: this record or the zero record
    assert mr.equal_bits(half, mr.draw(12345, index, ofdg.MBLUR_DEFAULT)) and (mr.equal_bits(half, got) or not half.any())
    fixed = ofdg.motion_blur_draw(9, index, dict(prob=1.0, shutter_min=0.75, shutter_max=0.75))
    assert fixed.tolist() == [0.75, 0.75, 0, 0]
    assert set(ofdg.MBLUR_DEFAULT) == set(ofdg.MBLUR_RANGES) | {"taps_side"} and tuple(ofdg.MBLUR_RANGES) == mr.RANGES


def test_draw_moments(ofdg):
    """20 000 draws under prob 0.5, shutter uniform in [0.2, 1.0), pair_shutter 0: the on-rate is binomial, standard error
    sqrt(0.25 / n); the shutter of the samples that are on is uniform, mean 0.6, standard deviation 0.8 / sqrt(12), standard error
    that over sqrt(n_on).  Seed 2026: both within 6 standard errors (measured 0.3 and 0.5)."""
    n = 20000
    q = dict(prob=0.5, shutter_min=0.2, shutter_max=1.0, pair_shutter=0.0)
    recs = np.stack([ofdg.motion_blur_draw(2026, i, q) for i in range(n)])
    on = recs[:, 0] > 0
    assert abs(on.mean() - 0.5) <= 6 * math.sqrt(0.25 / n), on.mean()
    s = recs[on, 0].astype(np.float64)
    assert abs(s.mean() - 0.6) <= 6 * (0.8 / math.sqrt(12)) / math.sqrt(on.sum()), s.mean()
    assert s.min() >= 0.2 and s.max() < 1.0 and np.array_equal(recs[:, 0], recs[:, 1]) and not recs[~on].any()
    assert mr.equal_bits(recs[:50], mr.drawn_records(2026, 0, 50, q))
    paired = np.stack([ofdg.motion_blur_draw(2026, i, dict(q, prob=1.0, pair_shutter=0.25)) for i in range(2000)])
    d = (paired[:, 1] - paired[:, 0]).astype(np.float64)
    assert np.abs(d).max() <= 0.25 * 1.0001 and abs(d.mean()) <= 6 * (0.5 / math.sqrt(12)) / math.sqrt(2000) and d.std() > 0.1


def test_batches_compose(ofdg):
    """Five samples in one call are two and three with first_index advanced: the records follow the global index."""
    images, flows = mr.frames(24, 6, "uint8", n=5), mr.flows(24, 6, "float16", n=5)
    kw = dict(seed=21, ranges=dict(ofdg.MBLUR_DEFAULT, prob=1.0, shutter_max=2.0))
    first = (1 << 32) + 1
    whole, recs = ofdg.host_motion_blur(images, flows, first_index=first, **kw)
    a, ra = ofdg.host_motion_blur(tuple(t[:2] for t in images), tuple(t[:2] for t in flows), first_index=first, **kw)
    b, rb = ofdg.host_motion_blur(tuple(t[2:] for t in images), tuple(t[2:] for t in flows), first_index=first + 2, **kw)
    mr.expect_equal(tuple(np.concatenate(p) for p in zip(a, b)), whole)
    assert mr.equal_bits(np.concatenate([ra, rb]), recs)
    assert mr.equal_bits(recs, mr.sanitise(mr.drawn_records(21, first, 5, kw["ranges"])))
    mr.expect_equal(whole, mr.motion_blur(images, flows, recs, 8)[0], "against the restatement")
    assert len({r.tobytes() for r in recs}) == 5 and not np.array_equal(whole[0], images[0])


def test_draw_refusals(ofdg):
    lib = ofdg.lib()
    out = ofdg.MblurRec()
    C.memset(C.byref(out), 0xA5, 16)
    job = ofdg.MblurJob()
    assert lib.ofdg_motion_blur_draw(1, 0, None, C.byref(out)) == ofdg.EINVAL and "NULL" in lib.ofdg_host_last_error().decode()
    assert lib.ofdg_motion_blur_draw(1, 0, C.byref(job), None) == ofdg.EINVAL and "NULL" in lib.ofdg_host_last_error().decode()
    bad = [("prob", -0.1), ("prob", 1.5), ("prob", float("nan")), ("shutter_min", -0.5), ("shutter_min", float("nan")), ("shutter_min", float("inf")),
           ("shutter_min", 2.5), ("shutter_max", -0.5), ("shutter_max", float("nan")), ("shutter_max", float("inf")), ("shutter_max", 2.5),
           ("pair_shutter", -0.5), ("pair_shutter", float("nan")), ("pair_shutter", float("inf"))]
    for name, value in bad:
        q = dict(prob=0.5, shutter_min=0.0, shutter_max=1.0, pair_shutter=0.0)
        q[name] = value
        if name == "shutter_min" and value == 2.5:
            q["shutter_max"] = 2.0
        with pytest.raises(ofdg.OfdgError, match=name):
            ofdg.motion_blur_draw(1, 0, q)
        j = ofdg._mblur_ranges(ofdg.MblurJob(), q)
        assert lib.ofdg_motion_blur_draw(1, 0, C.byref(j), C.byref(out)) == ofdg.EINVAL
        assert lib.ofdg_host_last_error().decode().startswith("ofdg_motion_blur_draw: ")
    with pytest.raises(ofdg.OfdgError, match="shutter_min must not be above shutter_max"):
        ofdg.motion_blur_draw(1, 0, dict(prob=1.0, shutter_min=1.0, shutter_max=0.5))
    assert bytes(out) == b"\xa5" * 16
    with pytest.raises(ValueError, match="unknown range"):
        ofdg.motion_blur_draw(1, 0, {"shutter": 1.0})
    assert lib.ofdg_motion_blur_draw(1, 0, C.byref(ofdg._mblur_ranges(ofdg.MblurJob(), dict(prob=1.0, shutter_min=2.0, shutter_max=2.0))), C.byref(out)) == ofdg.OK
    assert list(out.shutter) == [2.0, 2.0] and list(out.reserved) == [0, 0]


GUARD, FILL = 64, 0xA5


def test_refusals_write_nothing(ofdg):
    W, H, n = 16, 4, 2
    lib = ofdg.lib()
    size = n * 3 * H * W
    raw = {k: np.full(GUARD + 4 * size + GUARD, FILL, np.uint8) for k in ("s0", "s1", "d0", "d1", "f0", "f1")}
    rraw = {k: np.full(GUARD + 16 * n + GUARD, FILL, np.uint8) for k in ("recs", "out")}
    at = {k: v.ctypes.data + GUARD for k, v in dict(raw, **rraw).items()}

    def job(**kw):
        j = ofdg.MblurJob()
        j.src[0], j.src[1], j.dst[0], j.dst[1], j.flow[0], j.flow[1] = at["s0"], at["s1"], at["d0"], at["d1"], at["f0"], at["f1"]
        j.recs, j.recs_out = at["recs"], at["out"]
        j.src_fmt = j.dst_fmt = j.flow_fmt = ofdg.FMT_F32
        j.taps_side, j.prob, j.shutter_max = 8, 1.0, 1.0
        for k, v in kw.items():
            if k in ("src", "dst", "flow"):
                for idx, val in v.items():
                    getattr(j, k)[idx] = val
            elif k == "reserved":
                j.reserved[v[0]] = v[1]
            else:
                setattr(j, k, v)
        return j

    def refused(word, j, n_samples=n, width=W, height=H):
        assert lib.ofdg_host_motion_blur(None if j is None else C.byref(j), n_samples, width, height) == ofdg.EINVAL, word
        msg = lib.ofdg_host_last_error().decode()
        assert msg.startswith("ofdg_host_motion_blur: ") and word in msg, (word, msg)
        assert all((v == FILL).all() for v in list(raw.values()) + list(rraw.values())), word

    refused("job", None)
    refused("n_samples", job(), n_samples=0)
    refused("no frame", job(src={0: None, 1: None}, dst={0: None, 1: None}, flow={0: None, 1: None}))
    refused("dst: a frame is incomplete", job(dst={1: None}))
    refused("src: a frame is incomplete", job(src={0: None}))
    refused("flow: a frame is incomplete", job(flow={1: None}))
    refused("incomplete", job(src={0: None}, dst={0: None}))  # frame 0 with its flow alone
    refused("src_fmt", job(src_fmt=ofdg.FMT_F16))
    refused("dst_fmt", job(dst_fmt=5))
    refused("flow_fmt", job(flow_fmt=ofdg.FMT_U8))
    refused("flags", job(flags=1))
    refused("reserved", job(reserved=(0, -1)))
    refused("reserved", job(reserved=(1, 3)))
    for bad in (0, 17, -1):
        refused("taps_side", job(taps_side=bad))
    for bad_w, bad_h in ((12, 4), (16, 3), (0, 4), (16, 0), (-8, 4)):
        refused("width", job(), width=bad_w, height=bad_h)
    refused("width", job(width=W))            # one of the job's two set
    refused("width", job(width=8, height=4))  # the job's own size is not the plane's
    refused("2^32", job(), n_samples=1, width=65536, height=21846)
    # the ranges count when the record is drawn ...
    for name, bad in (("prob", -0.5), ("prob", 1.5), ("prob", float("nan")), ("shutter_min", -1.0), ("shutter_min", float("nan")),
                      ("shutter_max", float("inf")), ("shutter_max", 2.5), ("shutter_max", float("nan")), ("pair_shutter", -1.0),
                      ("pair_shutter", float("nan")), ("pair_shutter", float("inf"))):
        refused(name, job(recs=None, **{name: bad}))
    refused("shutter_min must not be above", job(recs=None, shutter_min=1.5, shutter_max=1.0))
    # ... there is no in-place form: a destination meets no other range
    refused("overlaps", job(dst={0: at["s0"]}))
    refused("overlaps", job(dst={1: at["s1"] + 16}))
    refused("overlaps", job(dst={0: at["f1"]}))
    refused("overlaps", job(dst={1: at["d0"] + 4 * size - 4}))
    refused("overlaps", job(dst={0: at["s0"]}, dst_fmt=ofdg.FMT_U8))
    refused("overlaps", job(recs_out=at["recs"] + 8))
    refused("overlaps", job(recs_out=at["d1"]))
    refused("overlaps", job(recs_out=at["f0"] + 4 * n * 2 * H * W - 8))  # (the last bytes of the flow)
    # and a valid call with the same buffers works; with given records the ranges are not looked at
    for k in ("s0", "s1"):
        raw[k][GUARD:GUARD + 4 * size].view(np.float32)[:] = 100.0
    for k in ("f0", "f1"):
        raw[k][GUARD:GUARD + 4 * size].view(np.float32)[:] = 3.25
    rraw["recs"][GUARD:GUARD + 16 * n].view(np.float32)[:] = np.tile(np.array([1.0, 9.0, 0, 0], np.float32), n)
    assert lib.ofdg_host_motion_blur(C.byref(job(width=W, height=H, prob=-1.0, shutter_max=float("nan"))), n, W, H) == ofdg.OK
    assert (raw["d0"][GUARD:GUARD + 4 * size].view(np.float32) == np.float32(100.0)).all()
    assert (raw["d1"][GUARD:GUARD + 4 * size].view(np.float32) == np.float32(100.0)).all()
    assert all((v[:GUARD] == FILL).all() and (v[-GUARD:] == FILL).all() for v in list(raw.values()) + list(rraw.values()))
    assert rraw["out"][GUARD:GUARD + 16 * n].view(np.float32).tolist() == [1.0, 2.0, 0.0, 0.0] * n


def test_python_argument_checks(ofdg):
    a = np.zeros((2, 3, 4, 16), np.uint8)
    fl = np.zeros((2, 2, 4, 16), np.float32)
    assert ofdg.motion_blur_format((a, a), (a.astype(np.float32),) * 2, (fl, fl.astype(np.float16))[:1] * 2) == (2, 4, 16, ofdg.FMT_U8, ofdg.FMT_F32, ofdg.FMT_F32)
    assert ofdg.motion_blur_format((None, a), (None, a), (None, fl.astype(np.float16)), 4, 16) == (2, 4, 16, ofdg.FMT_U8, ofdg.FMT_U8, ofdg.FMT_F16)
    with pytest.raises(ValueError, match="at least one frame"):
        ofdg.host_motion_blur((None, None), (None, None))
    with pytest.raises(ValueError, match="frame 1 must be set in images, out and flow.*only frame 0"):
        ofdg.host_motion_blur((a, a), (fl, None))
    with pytest.raises(ValueError, match="frame 0 must be set"):
        ofdg.host_motion_blur((None, a), (fl, fl))
    with pytest.raises(ValueError, match="n,3"):
        ofdg.host_motion_blur((np.zeros((2, 2, 4, 16), np.uint8), None), (fl, None))
    with pytest.raises(ValueError, match="one dtype"):
        ofdg.host_motion_blur((a, a.astype(np.float32)), (fl, fl))
    with pytest.raises(ValueError, match="one dtype"):
        ofdg.host_motion_blur((a, a), (fl, fl.astype(np.float16)))
    with pytest.raises(ValueError, match=r"flow\[0\]"):
        ofdg.host_motion_blur((a, None), (fl.astype(np.float64), None))
    with pytest.raises(ValueError, match=r"flow\[0\]"):
        ofdg.host_motion_blur((a, None), (fl[:, :1], None))
    with pytest.raises(ValueError, match=r"images\[0\]"):
        ofdg.host_motion_blur((a.astype(np.float16), None), (fl, None))
    with pytest.raises(ValueError, match="n,3,8,16"):
        ofdg.motion_blur_format((a, None), (a, None), (fl, None), 8, 16)
    with pytest.raises(ValueError, match="recs must be float32"):
        ofdg.host_motion_blur((a, None), (fl, None), recs=np.zeros((2, 16), np.float32))
    with pytest.raises(ValueError, match="unknown range"):
        ofdg.host_motion_blur((a, None), (fl, None), ranges={"shutter": 1.0})
    with pytest.raises(ofdg.OfdgError, match="taps_side"):
        ofdg.host_motion_blur((a, None), (fl, None), taps_side=17)
    with pytest.raises(ofdg.OfdgError, match="width"):
        ofdg.host_motion_blur((np.zeros((1, 3, 4, 12), np.uint8), None), (np.zeros((1, 2, 4, 12), np.float32), None))
    assert C.sizeof(ofdg.MblurRec) == 16 and C.sizeof(ofdg.MblurJob) == 128 and ofdg.MblurJob.taps_side.offset == 100
    assert ofdg.MblurJob.flow.offset == 32 and ofdg.MblurJob.prob.offset == 104 and ofdg.MblurJob.pair_shutter.offset == 116 and ofdg.MblurJob.reserved.offset == 120
    assert ofdg.MblurRec.reserved.offset == 8 and ofdg.MBLUR_REC_FLOATS == 4 and ofdg.MBLUR_MAX_TAPS_SIDE == 16 and ofdg.MBLUR_MAX_SHUTTER == 2.0
    hdr = open(ofdg.__file__.replace("__init__.py", "../include/ofdg.h")).read()
    for fn in ("ofdg_motion_blur", "ofdg_host_motion_blur", "ofdg_motion_blur_draw"):
        assert "int %s(" % fn in hdr and fn in ofdg.EXPORTS and hasattr(ofdg.lib(), fn)
    assert "/* 128 bytes */" in hdr and "OFDG_MBLUR_MAX_TAPS_SIDE 16" in hdr and "OFDG_MBLUR_MAX_HALF_PX 32" in hdr
    assert ofdg.MBLUR_DEFAULT == dict(prob=0.5, shutter_min=0.0, shutter_max=0.5, pair_shutter=0.1, taps_side=8)
    # taps_side: the argument, else the dict's, else 8
    assert ofdg._mblur_ranges(ofdg.MblurJob(), None).taps_side == 8 and ofdg._mblur_ranges(ofdg.MblurJob(), dict(taps_side=3)).taps_side == 3
    assert ofdg._mblur_ranges(ofdg.MblurJob(), dict(taps_side=3), 5).taps_side == 5


def test_flowloader_options_need_no_gpu(ofdg):
    opts = ofdg.FlowLoader._motion_blur_options
    assert opts(None, None) is None
    assert opts(ofdg.MBLUR_DEFAULT, ("flow1", "occ0")) == (ofdg.MBLUR_DEFAULT, (0, 1))
    assert opts(ofdg.MBLUR_DEFAULT, None) == (ofdg.MBLUR_DEFAULT, (0,))
    assert opts(dict(prob=1.0, frames=[1]), ("flow1",)) == (dict(prob=1.0), (1,))
    with pytest.raises(ValueError, match="unknown motion_blur option"):
        opts(dict(shutter=1.0), None)
    with pytest.raises(ValueError, match=r"frames=\(0,\)"):
        opts(dict(frames=(0, 1)), ("occ0",))
    with pytest.raises(ValueError, match="frames of 0 and / or 1"):
        opts(dict(frames=(2,)), ("flow1",))
    with pytest.raises(ValueError, match="frames of 0 and / or 1"):
        opts(dict(frames=()), ("flow1",))
