"""CPU tests of the spatial augmentation (ofdg_spatial_draw, ofdg_host_spatial; include/ofdg.h): the host twin against the numpy
restatement byte for byte, the draw, the cross-pin to the crop, known answers on affine frames and flows, every refusal.
No GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest

import crop_reference as cr
import spatial_reference as sr

FORMATS = list(itertools.product(("float32", "uint8"), ("float32", "float16"), ("float32", "uint8")))


@pytest.mark.parametrize("W,H,ow,oh", sr.SHAPES)
@pytest.mark.parametrize("image,flow,occ", FORMATS)
def test_host_spatial_equals_restatement(ofdg, W, H, ow, oh, image, flow, occ):
    src = sr.planes(W, H, image, flow, occ)
    recs = sr.records(W, H, ow, oh)
    for window in (False, True):
        want, want_recs = sr.spatial(src, recs, ow, oh, window)
        got, got_recs = ofdg.host_spatial(src, oh, ow, recs=recs, occ_window=window)
        sr.expect_equal(got, want, "window %s" % window)
        assert got_recs.tobytes() == want_recs.tobytes()
    # what sanitising did: the broken frames became the centred integer window, the others and the bounds themselves stayed
    centred = [1.0, 0.0, (W - ow) // 2, 0.0, 1.0, (H - oh) // 2]
    assert want_recs[13, :6].tolist() == centred and want_recs[13, 6:12].tolist() == recs[13, 6:12].tolist()
    assert want_recs[14, 6:12].tolist() == centred and want_recs[14, :6].tolist() == recs[14, :6].tolist()
    assert want_recs[15, :12].tolist() == centred * 2 and want_recs[16, :12].tolist() == centred * 2
    assert want_recs[17].tolist() == recs[17].tolist() and not want_recs[:, 12:].any()
    assert recs[5, 12:].view(np.int32).tolist() == [77, -1, 5, 1 << 30]


@pytest.mark.parametrize("subset", sr.SUBSETS[1:])
def test_plane_subsets(ofdg, subset):
    W, H, ow, oh = sr.SHAPES[1]
    full = sr.planes(W, H, "uint8", "float16", "float32")
    recs = sr.records(W, H, ow, oh)
    window = not (("occ0" in subset and "flow" not in subset) or ("occ1" in subset and "flow1" not in subset))
    src = {k: full[k] for k in subset}
    got, _ = ofdg.host_spatial(src, oh, ow, recs=recs, occ_window=window)
    want, _ = sr.spatial(full, recs, ow, oh, window)
    sr.expect_equal(got, {k: want[k] for k in subset}, str(subset))


def test_drawn_records(ofdg):
    W, H, ow, oh = 160, 100, 136, 66
    ranges = dict(zoom_log=0.3, rot=0.4, squeeze_log=0.2, translate=0.75, pair_zoom_log=0.05, pair_rot=0.04, pair_translate=1.5)
    for index in (0, 1, (1 << 32) + 3):
        got = ofdg.spatial_draw(12345, index, W, H, ow, oh, ranges, hflip=True, vflip=True)
        want = sr.draw(12345, index, W, H, ow, oh, ranges, sr.RANDOM_HFLIP | sr.RANDOM_VFLIP)
        assert got.tobytes() == want.tobytes(), (index, got, want)
    # all ranges 0: the centred identity window, both frames, whatever the index
    for index in (0, 5, (1 << 40) + 1):
        assert ofdg.spatial_draw(3, index, W, H, ow, oh).tolist() == [1, 0, 12, 0, 1, 17] * 2 + [0, 0]
        assert ofdg.spatial_draw(3, index, W, H, ow, oh).tobytes() == sr.draw(3, index, W, H, ow, oh).tobytes()  # (+0, not -0)
    # flips are drawn only where allowed, and all four pairs occur
    plain = [ofdg.spatial_draw(1, i, W, H, ow, oh, dict(zoom_log=0.1)) for i in range(64)]
    assert all(r[0] > 0 and r[4] > 0 for r in plain)
    signs = {(r[0] > 0, r[4] > 0) for r in (ofdg.spatial_draw(1, i, W, H, ow, oh, dict(zoom_log=0.1), hflip=True, vflip=True) for i in range(64))}
    assert len(signs) == 4
    # the record of index g does not depend on the batch it is drawn in
    src = {k: sr.planes(W, H)[k][:4] for k in ("image0", "flow", "label1")}
    _, first = ofdg.host_spatial(src, oh, ow, first_index=8, seed=12345, ranges=ranges, hflip=True, vflip=True)
    _, later = ofdg.host_spatial(src, oh, ow, first_index=10, seed=12345, ranges=ranges, hflip=True, vflip=True)
    assert first[2:].tobytes() == later[:2].tobytes() and first[0].tobytes() != first[1].tobytes()
    for first_index in (0, (1 << 32) + 3):
        recs = sr.drawn_records(12345, first_index, 4, W, H, ow, oh, ranges, sr.RANDOM_HFLIP | sr.RANDOM_VFLIP)
        got, used = ofdg.host_spatial(src, oh, ow, first_index=first_index, seed=12345, ranges=ranges, hflip=True, vflip=True)
        want, want_used = sr.spatial(src, recs, ow, oh)
        assert used.tobytes() == want_used.tobytes()
        sr.expect_equal(got, want)


def test_drawn_windows_that_fit_stay_inside(ofdg):
    """translate = 1: the centre may sit anywhere in the slack.  Of 3000 drawn records, every frame-0 window with slack on both
    axes has its four corners inside the frame by the definition's own test (0 <= Q <= (side - 1) * 256)."""
    W, H = 512, 384
    ranges = dict(zoom_log=0.4, rot=0.3, squeeze_log=0.15, translate=1.0)
    fitting = 0
    for k, (ow, oh) in enumerate([(448, 320), (256, 256), (512, 384), (40, 24)]):
        for index in range(750 * k, 750 * (k + 1)):
            want, slack = sr.draw(99, index, W, H, ow, oh, ranges, sr.RANDOM_HFLIP, with_slack=True)
            rec = ofdg.spatial_draw(99, index, W, H, ow, oh, ranges, hflip=True)
            assert rec.tobytes() == want.tobytes()
            if not (slack[0] > 0 and slack[1] > 0):
                continue
            fitting += 1
            a, b, c, d, e, g = rec[:6]
            for X, Y in ((0, 0), (ow - 1, 0), (0, oh - 1), (ow - 1, oh - 1)):
                Qx, Qy = int(sr._fixed(np.float64((a * X + b * Y) + c))), int(sr._fixed(np.float64((d * X + e * Y) + g)))
                assert 0 <= Qx <= (W - 1) * 256 and 0 <= Qy <= (H - 1) * 256, (ow, oh, index, X, Y, Qx, Qy)
    assert fitting > 1500, fitting


@pytest.mark.parametrize("image,flow,occ", [FORMATS[0], FORMATS[7]])
def test_cross_pin_to_the_crop(ofdg, image, flow, occ):
    """Maps {+-1, 0, c, 0, +-1, g} with integer c, g are the crop's windows and flips: frames, labels and maps (0 / 1 sources,
    without the window flag) equal ofdg_host_crop byte for byte, the flows number for number."""
    W, H, cw, ch = 160, 100, 136, 66
    base = cr.planes(W, H, image, flow, occ)
    src = {k: np.array(v) for k, v in base.items()}
    for name in ("occ0", "occ1"):
        src[name] = (src[name] != 0).astype(src[name].dtype)
    for name in ("flow", "flow1"):  # finite components: 0 or of magnitude in [2^-20, 2^20] (denormals out); -0.0 becomes +0
        f = src[name].astype(np.float32)
        small = np.isfinite(f) & (np.abs(f) < 2.0 ** -20)
        src[name][small] = 0
    crop_recs = cr.records(W, H, cw, ch)
    got_crop, used = ofdg.host_crop(src, ch, cw, recs=crop_recs)
    recs = np.zeros((cr.N, 14), np.float64)
    for i, (x0, y0, fl, _) in enumerate(used):
        m = [-1.0 if fl & 1 else 1.0, 0.0, float(x0 + (cw - 1 if fl & 1 else 0)), 0.0, -1.0 if fl & 2 else 1.0, float(y0 + (ch - 1 if fl & 2 else 0))]
        recs[i, :12] = m + m
    got, _ = ofdg.host_spatial(src, ch, cw, recs=recs)
    for name in ("image0", "image1", "occ0", "occ1", "label0", "label1"):
        assert got[name].tobytes() == got_crop[name].tobytes(), name
    for name in ("flow", "flow1"):
        a, b = got[name].astype(np.float32), got_crop[name].astype(np.float32)
        whole = np.isfinite(b).all(axis=1, keepdims=True) & np.ones_like(b, bool)  # pixels whose two source components are finite
        assert whole.sum() > whole.size // 2 and np.array_equal(a[whole], b[whole]), name
        assert not np.isfinite(a[~whole].reshape(-1, 1)).all() and (~np.isfinite(a).all(axis=1) == ~np.isfinite(b).all(axis=1)).all(), name


def test_known_answers_on_affine_planes(ofdg):
    """A frame that is an affine function of position, sampled at quarter pixels, comes back as that function of the mapped
    position; a flow of a known affine motion comes back as the motion between the two warped frames.  The expected numbers are
    worked out here in fp64 from the maps alone (every step is exact in these dyadic numbers) and rounded to float32 once."""
    W, H, ow, oh, n = 72, 40, 40, 24, 1
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    image = np.stack([3.0 + 0.5 * x + 0.25 * y, 100.0 - 0.25 * x + 0.5 * y, 7.0 + x])[None].astype(np.float32)
    # source motion: frame-1 position = (1.5 x + 0.5, 1.25 y - 0.25)
    flow = np.stack([0.5 * x + 0.5, 0.25 * y - 0.25])[None].astype(np.float32)
    m0 = [0.75, 0.0, 2.25, 0.0, 0.5, 3.5]          # quarter-pixel taps, inside the frame: x in [2.25, 31.5], y in [3.5, 15]
    m0_int = [1.0, 0.0, 3.0, 0.0, 1.0, 2.0]        # integer taps: the nearest tap is the position itself
    m1 = [0.0, -2.0, 60.0, 2.0, 0.0, 5.0]          # (px, py) -> (60 - 2 py, 5 + 2 px)
    X, Y = np.meshgrid(np.arange(ow, dtype=np.float64), np.arange(oh, dtype=np.float64))
    got, _ = ofdg.host_spatial({"image0": image}, oh, ow, recs=np.array([m0 + m1 + [0, 0]], np.float64))
    qx, qy = 0.75 * X + 2.25, 0.5 * Y + 3.5
    want = np.stack([3.0 + 0.5 * qx + 0.25 * qy, 100.0 - 0.25 * qx + 0.5 * qy, 7.0 + qx]).astype(np.float32)
    assert np.array_equal(got["image0"][0], want)
    got, _ = ofdg.host_spatial({"flow": flow, "occ0": np.zeros((n, 1, H, W), np.uint8)}, oh, ow,
                               recs=np.array([m0_int + m1 + [0, 0]], np.float64), occ_window=True)
    sx, sy = X + 3.0, Y + 2.0                       # source position of the destination pixel
    tx, ty = 1.5 * sx + 0.5, 1.25 * sy - 0.25       # where it moves to in source frame 1
    px, py = (ty - 5.0) / 2.0, (60.0 - tx) / 2.0    # m1 solved for (px, py)
    assert np.array_equal(got["flow"][0], np.stack([px - X, py - Y]).astype(np.float32))
    outside = (np.floor(px + 0.5) < 0) | (np.floor(px + 0.5) > ow - 1) | (np.floor(py + 0.5) < 0) | (np.floor(py + 0.5) > oh - 1)
    assert 0 < outside.sum() < outside.size and np.array_equal(got["occ0"][0, 0] != 0, outside)


def test_refusals_write_nothing(ofdg):
    W, H, ow, oh, n = 72, 40, 40, 24, 2
    src = {k: np.array(v[:n]) for k, v in sr.planes(W, H).items()}
    dst = {k: np.full(int(np.prod(src[k].shape[:-2])) * oh * ow * src[k].itemsize, 0xA5, np.uint8) for k in src}
    recs = np.zeros((n, 14), np.float64)
    recs[:, [0, 4, 6, 10]] = 1.0
    recs_out = np.full((n, 14 * 8), 0xA5, np.uint8)
    lib = ofdg.lib()

    def job(planes=sr.PLANES, **kw):
        j = ofdg.SpatialJob()
        for k, name in enumerate(sr.PLANES):
            if name in planes:
                j.src[k], j.dst[k] = src[name].ctypes.data, dst[name].ctypes.data
        j.recs, j.recs_out = recs.ctypes.data, recs_out.ctypes.data
        j.out_w, j.out_h = ow, oh
        for k, v in kw.items():
            if k in ("src", "dst"):
                for idx, val in v.items():
                    getattr(j, k)[idx] = val
            elif k == "reserved":
                j.reserved[v[0]] = v[1]
            else:
                setattr(j, k, v)
        return j

    def refused(word, j, n_samples=n, width=W, height=H):
        rc = lib.ofdg_host_spatial(None if j is None else C.byref(j), n_samples, width, height)
        assert rc == ofdg.EINVAL, word
        msg = lib.ofdg_host_last_error().decode()
        assert msg.startswith("ofdg_host_spatial") and word in msg, (word, msg)
        assert all((d == 0xA5).all() for d in dst.values()) and (recs_out == 0xA5).all(), word

    refused("job", None)
    refused("n_samples", job(), n_samples=0)
    refused("width", job(), width=W + 4)
    refused("height", job(), height=H + 1)
    refused("width and height", job(width=W))                      # only one of the two set
    refused("width and height of the job", job(width=W + 8, height=H))
    refused("2^20", job(), width=(1 << 20) + 8, height=2)
    for bad in (0, 4, 44, (1 << 20) + 8):
        refused("out_w", job(out_w=bad))
    for bad in (0, 1, 23, (1 << 20) + 2):
        refused("out_h", job(out_h=bad))
    refused("width * height", job(), width=1 << 16, height=1 << 15)
    refused("out_w * out_h", job(out_w=1 << 16, out_h=1 << 15))
    refused("flags", job(flags=32))
    refused("flags", job(flags=1))
    refused("reserved", job(reserved=(0, 1)))
    refused("reserved", job(reserved=(1, -1)))
    refused("image_fmt", job(image_fmt=ofdg.FMT_F16))
    refused("flow_fmt", job(flow_fmt=ofdg.FMT_U8))
    refused("occ_fmt", job(occ_fmt=ofdg.FMT_F16))
    for name in sr.RANGES:
        for bad in (-0.5, float("nan"), float("inf")):
            refused(name, job(**{name: bad}))
    refused("translate", job(translate=1.5))
    refused("no plane", job(planes=()))
    refused("dst", job(dst={2: None}))
    refused("src", job(src={6: None}))
    refused("occ0", job(planes=("occ0", "flow1"), flags=sr.OCC_WINDOW))
    refused("occ1", job(planes=("occ1", "flow"), flags=sr.OCC_WINDOW))
    refused("overlaps", job(dst={0: src["image0"].ctypes.data}))                       # in place
    refused("overlaps", job(dst={1: dst["image0"].ctypes.data + 16}))                  # two destinations
    refused("overlaps", job(recs_out=recs.ctypes.data))                                # the records in place
    refused("overlaps", job(planes=("label0",), dst={6: src["label0"].ctypes.data + W * H * n - 1}))  # one byte
    # flow alone is fine, and so is a valid job with everything right after
    assert lib.ofdg_host_spatial(C.byref(job(planes=("flow",))), n, W, H) == ofdg.OK
    rc = lib.ofdg_host_spatial(C.byref(job(flags=sr.OCC_WINDOW, width=W, height=H)), n, W, H)
    assert rc == ofdg.OK, lib.ofdg_host_last_error().decode()
    want, used = sr.spatial(src, recs, ow, oh, True)
    for name in want:
        assert dst[name].tobytes() == want[name].tobytes(), name
    assert recs_out.tobytes() == used.tobytes()
    # the draw's own refusals
    r = np.zeros(14, np.float64)
    p = r.ctypes.data_as(C.c_void_p)
    for word, j in (("width and height must be set", job()), ("out_w", job(width=W, height=H, out_w=12)),
                    ("flags", job(width=W, height=H, flags=64)), ("rot", job(width=W, height=H, rot=-1.0)),
                    ("translate", job(width=W, height=H, translate=2.0)), ("width", job(width=W + 1, height=H))):
        assert lib.ofdg_spatial_draw(1, 0, C.byref(j), p) == ofdg.EINVAL, word
        assert word in lib.ofdg_host_last_error().decode(), (word, lib.ofdg_host_last_error().decode())
    assert lib.ofdg_spatial_draw(1, 0, None, p) == ofdg.EINVAL and lib.ofdg_spatial_draw(1, 0, C.byref(job(width=W, height=H)), None) == ofdg.EINVAL
    assert not r.any()


def test_spatial_format_and_alloc(ofdg):
    src = {k: np.array(v[:2]) for k, v in sr.planes(40, 24, "uint8", "float16", "uint8").items()}
    dst = ofdg.alloc_spatial(src, 40, 72)  # larger than the source
    assert ofdg.spatial_format(src, dst, 24, 40) == (2, 40, 72, ofdg.FMT_U8, ofdg.FMT_F16, ofdg.FMT_U8)
    assert dst["label0"].shape == (2, 40, 72) and dst["flow1"].shape == (2, 2, 40, 72) and dst["flow"].dtype == np.float16
    for bad_src, bad_dst in [({}, {}), (src, {k: v for k, v in dst.items() if k != "flow"}), (src, ofdg.alloc_spatial(src, 40, 44)),
                             (src, ofdg.alloc_spatial(src, 23, 40)), (src, dict(dst, flow=dst["flow"].astype(np.float32)))]:
        with pytest.raises(ValueError):
            ofdg.spatial_format(bad_src, bad_dst, 24, 40)
    assert set(ofdg.SPATIAL_FLOWNET) == set(ofdg.SPATIAL_RANGES) == set(sr.RANGES)
    with pytest.raises(ValueError):
        ofdg.spatial_draw(1, 0, 72, 40, 40, 24, dict(zoom=0.1))
    assert C.sizeof(ofdg.SpatialRec) == 112 and C.sizeof(ofdg.SpatialJob) == 224
