"""CPU tests of the training crop (ofdg_crop_draw, ofdg_host_crop; include/ofdg.h): Philox and the draw against known
answers, the coverage of the draw, the host twin against the numpy restatement byte for byte, the window rule of the
occlusion maps on hand-made flows, composition, every refusal, and the reductions on a cropped flow.  No GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest

import crop_reference as cr
import flow_pyramid_reference as fpr
import flow_stats_reference as fsr

FORMATS = list(itertools.product(("float32", "uint8"), ("float32", "float16"), ("float32", "uint8")))


def test_philox_known_answers(ofdg):
    """The three known answers published with the generator (Random123's kat_vectors, philox4x32 10 rounds), through the
    library's own function - the one the draw on the host and in the kernel is made of - and through the restatement."""
    ones = 0xFFFFFFFF
    for counter, key, want in [
        ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
        ((ones,) * 4, (ones, ones), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
        ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
    ]:
        assert ofdg.crop_philox(counter, key) == want
        assert cr.philox4x32(counter, key) == want
    # and the block of a draw: counter {0, 0, 0x0c70, 0} under the key of (seed 12345, index 2^32 + 5)
    block = ofdg.crop_philox((0, 0, 0x0C70, 0), (12345 ^ 0x9E3779B9, 5))
    assert block == cr.philox4x32((0, 0, 0x0C70, 0), (12345 ^ 0x9E3779B9, 5))
    assert ((block[0] * 65) >> 32, (block[1] * 65) >> 32) == ofdg.crop_draw(12345, (1 << 32) + 5, 512, 384, 448, 320)[:2]
    lib = ofdg.lib()
    assert lib.ofdg_crop_philox(None, None, None) == ofdg.EINVAL and "NULL" in lib.ofdg_host_last_error().decode()


KNOWN = [  # seed, W, H, crop_w, crop_h, index -> x0, y0, HFLIP, VFLIP (both random flips allowed)
    (12345, 512, 384, 448, 320, 0, (1, 5, 0, 1)), (12345, 512, 384, 448, 320, 1, (11, 16, 1, 1)),
    (12345, 512, 384, 448, 320, 2, (16, 2, 1, 0)), (12345, 512, 384, 448, 320, (1 << 32) + 5, (2, 47, 0, 1)),
    (7, 72, 40, 72, 40, 0, (0, 0, 1, 1)),
    (1, 72, 40, 40, 24, 0, (27, 6, None, None)), (1, 72, 40, 40, 24, 1, (6, 7, None, None)),
    (1, 72, 40, 40, 24, 2, (2, 4, None, None)), (1, 72, 40, 40, 24, 3, (21, 3, None, None)),
]


@pytest.mark.parametrize("seed,W,H,cw,ch,index,want", KNOWN)
def test_crop_draw_known_answers(ofdg, seed, W, H, cw, ch, index, want):
    if want[2] is None:  # (the last four are drawn with RANDOM_VFLIP alone and all carry VFLIP)
        got = ofdg.crop_draw(seed, index, W, H, cw, ch, vflip=True)
        assert got == (want[0], want[1], cr.VFLIP)
        assert got == cr.draw(seed, index, W, H, cw, ch, cr.RANDOM_VFLIP)
        return
    x0, y0, fl = ofdg.crop_draw(seed, index, W, H, cw, ch, hflip=True, vflip=True)
    assert (x0, y0, fl & 1, (fl >> 1) & 1) == want
    assert (x0, y0, fl) == cr.draw(seed, index, W, H, cw, ch, cr.RANDOM_HFLIP | cr.RANDOM_VFLIP)


def test_crop_draw_coverage(ofdg):
    """Seed 1, 72x40 to 40x24, indices 0..4095: every position and every flip pair occurs, in numbers that a wrong range or a
    stuck bit cannot reach (the definition itself gives 98..147, 209..264 and 988..1055)."""
    recs = [ofdg.crop_draw(1, i, 72, 40, 40, 24, hflip=True, vflip=True) for i in range(4096)]
    assert recs == [cr.draw(1, i, 72, 40, 40, 24, cr.RANDOM_HFLIP | cr.RANDOM_VFLIP) for i in range(4096)]
    xs = np.bincount([r[0] for r in recs], minlength=33)
    ys = np.bincount([r[1] for r in recs], minlength=17)
    fl = np.bincount([r[2] for r in recs], minlength=4)
    assert len(xs) == 33 and xs.min() >= 62 and xs.max() <= 186, xs
    assert len(ys) == 17 and ys.min() >= 120 and ys.max() <= 362, ys
    assert len(fl) == 4 and fl.min() >= 900 and fl.max() <= 1150, fl
    assert (xs.min(), xs.max(), ys.min(), ys.max(), fl.min(), fl.max()) == (98, 147, 209, 264, 988, 1055)
    plain = [ofdg.crop_draw(1, i, 72, 40, 40, 24) for i in range(4096)]
    assert all(r[2] == 0 for r in plain) and [r[:2] for r in plain] == [r[:2] for r in recs]
    assert all(ofdg.crop_draw(1, i, 72, 40, 40, 24, hflip=True)[2] in (0, cr.HFLIP) for i in range(64))


@pytest.mark.parametrize("W,H,cw,ch", cr.SHAPES)
@pytest.mark.parametrize("image,flow,occ", FORMATS)
def test_host_crop_equals_restatement(ofdg, W, H, cw, ch, image, flow, occ):
    src = cr.planes(W, H, image, flow, occ)
    recs = cr.records(W, H, cw, ch)
    for window in (False, True):
        want, want_recs = cr.crop(src, recs, cw, ch, window)
        got, got_recs = ofdg.host_crop(src, ch, cw, recs=recs, occ_window=window)
        cr.expect_equal(got, want, "window %s" % window)
        assert np.array_equal(got_recs, want_recs)
    assert want_recs[7].tolist() == [0, H - ch, 3, 0] and want_recs[8].tolist() == [W - cw, min(1, H - ch), 3, 0]


def test_sign_bit_rule_on_special_values(ofdg):
    """Every special pattern of the flow reaches the output with its sign bit inverted and every other bit kept - where the
    component is mirrored, and only there."""
    for flow, bits_t in (("float32", np.uint32), ("float16", np.uint16)):
        src = {"flow": cr.planes(72, 40, flow=flow)["flow"][:4]}
        sign = bits_t(1 << (8 * np.dtype(bits_t).itemsize - 1))
        recs = np.array([(0, 0, f, 0) for f in range(4)], np.int32)
        got, _ = ofdg.host_crop(src, 40, 72, recs=recs)
        for f in range(4):
            a = src["flow"][f].view(bits_t)
            a = a[:, :, ::-1] if f & 1 else a
            a = a[:, ::-1, :] if f & 2 else a
            b = got["flow"][f].view(bits_t)
            assert np.array_equal(b[0], a[0] ^ (sign if f & 1 else bits_t(0))) and np.array_equal(b[1], a[1] ^ (sign if f & 2 else bits_t(0)))
        special = cr._SPECIAL32 if flow == "float32" else cr._SPECIAL16
        assert all((src["flow"].view(bits_t) == s).any() for s in special)


def window_case(flow_dtype, occ_dtype):
    """One sample, 72x40, window 40x24 at (16, 8): pixels whose targets lie exactly on the window's first and last column / row,
    half a pixel to either side of them, at NaN and +-inf; the source map is non-zero in places."""
    W, H, cw, ch, x0, y0 = 72, 40, 40, 24, 16, 8
    u = np.zeros((H, W), np.float32)
    v = np.zeros((H, W), np.float32)
    xs = np.arange(W, dtype=np.float32)[None, :]
    ys = np.arange(H, dtype=np.float32)[:, None]
    # row y0 + k, every column: the target column is the k-th of these (a displacement exact in binary16: multiples of 0.25)
    targets_x = [x0, x0 - 0.5, x0 - 0.75, x0 + 0.5, x0 + cw - 1, x0 + cw - 1 + 0.25, x0 + cw - 0.5, x0 + cw - 0.75, x0 - 1, x0 + cw]
    for k, t in enumerate(targets_x):
        u[y0 + k, :] = (np.float32(t) - xs)[0]
    targets_y = [y0, y0 - 0.5, y0 - 0.75, y0 + 0.5, y0 + ch - 1, y0 + ch - 1 + 0.25, y0 + ch - 0.5, y0 + ch - 0.75, y0 - 1, y0 + ch]
    for k, t in enumerate(targets_y):
        v[y0 + 12:y0 + 24, x0 + 2 * k] = (np.float32(t) - ys)[y0 + 12:y0 + 24, 0]
    u[y0 + 10, x0:x0 + 6] = [np.nan, np.inf, -np.inf, 0, 0, 0]
    v[y0 + 10, x0 + 3:x0 + 6] = [np.nan, np.inf, -np.inf]
    flow = np.stack([u, v])[None].astype(flow_dtype)
    occ = np.zeros((1, 1, H, W), occ_dtype)
    occ[0, 0, ::3, ::5] = 1
    occ[0, 0, 1::7, 2::3] = 3 if occ_dtype == "uint8" else 0.25
    if occ_dtype == "float32":
        occ[0, 0, y0 + 11, x0 + 1] = -0.0  # (row 11: no displacement, the target is the pixel itself)
        occ[0, 0, y0 + 11, x0 + 3] = np.nan
    return dict(flow=flow, occ0=occ, flow1=flow[:, ::-1].copy(), occ1=occ.copy()), (W, H, cw, ch, x0, y0)


@pytest.mark.parametrize("flow_dtype", ["float32", "float16"])
@pytest.mark.parametrize("occ_dtype", ["float32", "uint8"])
def test_occ_window(ofdg, flow_dtype, occ_dtype):
    src, (W, H, cw, ch, x0, y0) = window_case(flow_dtype, occ_dtype)
    recs = np.array([(x0, y0, 0, 0)], np.int32)
    want, _ = cr.crop(src, recs, cw, ch, True)
    got, _ = ofdg.host_crop(src, ch, cw, recs=recs, occ_window=True)
    cr.expect_equal(got, want)
    o = got["occ0"][0, 0].astype(np.float32)
    base = src["occ0"][0, 0, y0:y0 + ch, x0:x0 + cw]
    free = (base[:10] == 0).all(axis=0)  # columns whose first ten rows the source map leaves at zero
    # rows 0..9: targets x0 (in), x0-0.5 (floor(x0) = in), x0-0.75 (out), x0+0.5 (in), last (in), last+0.25 (in), last+0.5 (out),
    # x0+cw-0.75 (a quarter pixel past the last column: in), x0-1 (out), x0+cw (out)
    marks = [bool(o[k, free].all()) for k in range(10)]
    assert marks == [False, False, True, False, False, False, True, False, True, True], marks
    assert not o[:10, free][[0, 1, 3, 4, 5, 7]].any()
    row = o[10]  # NaN, +inf, -inf in u; NaN, +inf, -inf in v
    assert row[:6].tolist() == [1, 1, 1, 1, 1, 1]
    keep = (base != 0) & (base == base)
    assert (o[keep] == 1).all()
    if occ_dtype == "float32":
        assert got["occ0"].view(np.uint32)[0, 0, 11, 1] == 0x80000000 and got["occ0"][0, 0, 11, 3] == 1.0
    # invariant under the flips: the flipped call equals the flipped result of the unflipped call
    for fl in (1, 2, 3):
        flipped, _ = ofdg.host_crop(src, ch, cw, recs=np.array([(x0, y0, fl, 0)], np.int32), occ_window=True)
        for name in ("occ0", "occ1"):
            a = got[name]
            a = a[..., ::-1] if fl & 1 else a
            a = a[..., ::-1, :] if fl & 2 else a
            assert np.array_equal(flipped[name].view(np.uint8), np.ascontiguousarray(a).view(np.uint8)), (name, fl)
    # without the flag the maps are moved as bits
    plain, _ = ofdg.host_crop(src, ch, cw, recs=recs)
    assert plain["occ0"].tobytes() == np.ascontiguousarray(src["occ0"][..., y0:y0 + ch, x0:x0 + cw]).tobytes()


def test_composition(ofdg):
    src = cr.planes(160, 100, "uint8", "float16", "uint8")
    a = np.array([(i, 2 * i, 0, 0) for i in range(cr.N)], np.int32)
    b = np.array([(7 - (i % 8), i % 5, 0, 0) for i in range(cr.N)], np.int32)
    first, _ = ofdg.host_crop(src, 80, 144, recs=a)
    second, _ = ofdg.host_crop(first, 66, 136, recs=b)
    summed = a + b
    once, _ = ofdg.host_crop(src, 66, 136, recs=summed)
    cr.expect_equal(second, once)
    flip = np.array([(0, 0, cr.HFLIP, 0)] * cr.N, np.int32)
    there, _ = ofdg.host_crop(src, 100, 160, recs=flip)
    back, _ = ofdg.host_crop(there, 100, 160, recs=flip)
    cr.expect_equal(back, {k: np.asarray(v) for k, v in src.items()})
    assert there["flow"].tobytes() != src["flow"].tobytes()


def test_drawn_records_on_the_host(ofdg):
    src = {k: cr.planes(72, 40)[k] for k in ("image0", "flow", "label1")}
    for first_index in (0, (1 << 32) + 3):
        recs = cr.drawn_records(12345, first_index, cr.N, 72, 40, 40, 24, cr.RANDOM_HFLIP | cr.RANDOM_VFLIP)
        got, used = ofdg.host_crop(src, 24, 40, first_index=first_index, seed=12345, hflip=True, vflip=True)
        assert np.array_equal(used, recs)
        cr.expect_equal(got, cr.crop(src, recs, 40, 24)[0])
    assert len({tuple(r) for r in recs.tolist()}) > 4


def test_refusals_write_nothing(ofdg):
    W, H, cw, ch, n = 72, 40, 40, 24, 2
    src = {k: np.array(v[:n]) for k, v in cr.planes(W, H).items()}
    dst = {k: np.full(int(np.prod(src[k].shape[:-2])) * ch * cw * src[k].itemsize, 0xA5, np.uint8) for k in src}
    recs = np.zeros((n, 4), np.int32)
    recs_out = np.full((n, 4), -1515870811, np.int32)  # 0xA5A5A5A5
    lib = ofdg.lib()

    def job(planes=cr.PLANES, **kw):
        j = ofdg.CropJob()
        for k, name in enumerate(cr.PLANES):
            if name in planes:
                j.src[k], j.dst[k] = src[name].ctypes.data, dst[name].ctypes.data
        j.recs, j.recs_out = recs.ctypes.data, recs_out.ctypes.data
        j.crop_w, j.crop_h = cw, ch
        for k, v in kw.items():
            if k in ("src", "dst"):
                for idx, val in v.items():
                    getattr(j, k)[idx] = val
            else:
                setattr(j, k, v)
        return j

    def refused(word, j, n_samples=n, width=W, height=H):
        rc = lib.ofdg_host_crop(None if j is None else C.byref(j), n_samples, width, height)
        assert rc == ofdg.EINVAL, word
        msg = lib.ofdg_host_last_error().decode()
        assert msg.startswith("ofdg_host_crop") and word in msg, (word, msg)
        assert all((d == 0xA5).all() for d in dst.values()) and (recs_out == -1515870811).all(), word

    refused("job", None)
    refused("n_samples", job(), n_samples=0)
    for bad in (0, 4, 44, W + 8):
        refused("crop_w", job(crop_w=bad))
    for bad in (0, 1, 23, H + 2):
        refused("crop_h", job(crop_h=bad))
    refused("flags", job(flags=32))
    refused("flags", job(flags=cr.HFLIP))  # (a record flag is no job flag)
    refused("reserved", job(reserved=1))
    refused("image_fmt", job(image_fmt=ofdg.FMT_F16))
    refused("flow_fmt", job(flow_fmt=ofdg.FMT_U8))
    refused("occ_fmt", job(occ_fmt=ofdg.FMT_F16))
    refused("occ_fmt", job(occ_fmt=3))
    refused("no plane", job(planes=()))
    refused("dst", job(dst={2: None}))
    refused("src", job(src={6: None}))
    refused("occ0", job(planes=("occ0", "flow1"), flags=cr.OCC_WINDOW))
    refused("occ1", job(planes=("occ1", "flow"), flags=cr.OCC_WINDOW))
    refused("overlaps", job(dst={0: src["image0"].ctypes.data}))                       # in place
    refused("overlaps", job(dst={1: dst["image0"].ctypes.data + 16}))                  # two destinations
    refused("overlaps", job(recs_out=recs.ctypes.data))                                # the records in place
    refused("overlaps", job(planes=("label0",), dst={6: src["label0"].ctypes.data + W * H * n - 1}))  # one byte
    # and a valid job right after
    rc = lib.ofdg_host_crop(C.byref(job(flags=cr.OCC_WINDOW)), n, W, H)
    assert rc == ofdg.OK, lib.ofdg_host_last_error().decode()
    want, _ = cr.crop(src, recs, cw, ch, True)
    for name in want:
        assert dst[name].tobytes() == want[name].tobytes(), name
    assert not recs_out.any()
    r = ofdg.CropRec()
    assert lib.ofdg_crop_draw(1, 0, W, H, W + 1, ch, 0, C.byref(r)) == ofdg.EINVAL and "crop_w" in lib.ofdg_host_last_error().decode()
    assert lib.ofdg_crop_draw(1, 0, W, H, cw, ch, 3, C.byref(r)) == ofdg.EINVAL and "flags" in lib.ofdg_host_last_error().decode()
    assert lib.ofdg_crop_draw(1, 0, W, H, cw, ch, 0, None) == ofdg.EINVAL


def test_crop_format_and_alloc(ofdg):
    src = {k: np.array(v[:2]) for k, v in cr.planes(72, 40, "uint8", "float16", "uint8").items()}
    dst = ofdg.alloc_crop(src, 24, 40)
    assert ofdg.crop_format(src, dst, 40, 72) == (2, 24, 40, ofdg.FMT_U8, ofdg.FMT_F16, ofdg.FMT_U8)
    assert dst["label0"].shape == (2, 24, 40) and dst["flow1"].shape == (2, 2, 24, 40) and dst["flow"].dtype == np.float16
    only = {"label1": src["label1"]}
    assert ofdg.crop_format(only, ofdg.alloc_crop(only, 40, 72), 40, 72) == (2, 40, 72, ofdg.FMT_F32, ofdg.FMT_F32, ofdg.FMT_F32)
    for bad_src, bad_dst in [
        ({}, {}),
        (src, {k: v for k, v in dst.items() if k != "flow"}),
        (dict(src, depth=src["occ0"]), dict(dst, depth=dst["occ0"])),
        (dict(src, flow=src["flow"].astype(np.float32)), dict(dst, flow=dst["flow"].astype(np.float32))),  # flow1 stays float16
        (dict(src, image0=src["image0"].astype(np.int8)), dict(dst, image0=dst["image0"].astype(np.int8))),
        (dict(src, occ0=src["occ0"][:1]), dict(dst, occ0=dst["occ0"][:1])),
        (dict(src, flow=src["flow"][:, :1]), dict(dst, flow=dst["flow"][:, :1])),
        (src, dict(dst, flow=dst["flow"][..., :32])),
        (src, dict(dst, flow=dst["flow"].astype(np.float32))),
        (src, ofdg.alloc_crop(src, 24, 44)),
        (src, ofdg.alloc_crop(src, 23, 40)),
        (src, ofdg.alloc_crop(src, 42, 40)),
    ]:
        with pytest.raises(ValueError):
            ofdg.crop_format(bad_src, bad_dst, 40, 72)


@pytest.mark.parametrize("flow_dtype,occ_dtype", [("float32", "float32"), ("float16", "uint8")])
def test_reductions_of_the_cropped_flow(ofdg, flow_dtype, occ_dtype):
    """host_flow_stats / host_flow_pyramid take their size from the arrays: on host_crop's flow and occ0 they equal the
    restatements on the cropped arrays."""
    all_planes = cr.planes(160, 100, "uint8", flow_dtype, occ_dtype)
    src = {k: all_planes[k] for k in ("flow", "occ0")}
    got, _ = ofdg.host_crop(src, 64, 136, first_index=5, seed=3, hflip=True, vflip=True, occ_window=True)
    flow, occ = got["flow"], got["occ0"]
    assert flow.shape == (cr.N, 2, 64, 136)
    levels = ofdg.host_flow_pyramid(flow, 3, occ, weights=True)
    want = fpr.flow_pyramid(flow, 3, occ, fpr.SCALE, np.dtype(flow_dtype).type)
    fpr.expect_equal(levels[0], want[0])
    fpr.expect_equal(levels[1], want[1])
    rows = ofdg.host_flow_stats(flow, occ, 2.0)
    fsr.expect_equal(rows, fsr.flow_stats(flow, occ, 2.0))
    fsr.expect_invariants(fsr.rows_of(rows), 64, 136)
