"""GPU tests of reprojection (ofdg_reproject, include/ofdg.h): the device planes and rows against ofdg_host_reproject and against
the numpy restatement (tests/reproject_reference.py), byte for byte and field for field - every format and size, between guard
bytes, twice, with and without accumulation, subsets of frames and outputs; behind forward_counter, the crop and the spatial
step without synchronisation, in mode 9, with three calls in flight, through the loader - and the refusals."""
import numpy as np
import pytest

import reproject_reference as rr

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 64  # bytes in front of and behind every written plane (keeps the 16-byte alignment)
KINDS = {"warped": 3, "err": 1, "mask": 1, "fb2": 1}


def make_gen(ofdg, W, H, mode=7, pool=False, **kw):
    g = ofdg.Generator(ofdg.default_params(width=W, height=H, mode=mode, **kw))
    if pool:
        g.pool_synthetic(3, 2 * W, 2 * H, 11)
    return g


def guarded(array):
    """(the whole uint8 buffer with 0xA5 guards; the tensor holding `array` in its middle)"""
    import torch
    src = torch.from_numpy(np.array(array))
    size = src.numel() * src.element_size()
    raw = torch.full((GUARD + size + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    t = raw[GUARD:GUARD + size].view(src.dtype).view(src.shape)
    t.copy_(src)
    return raw, t


def guards_intact(bufs):
    return all(bool((raw[:GUARD] == FILL).all()) and bool((raw[-GUARD:] == FILL).all()) for raw, _ in bufs)


def to_dev(planes):
    import torch
    return tuple(None if t is None else torch.from_numpy(np.array(t)).cuda() for t in planes)


def to_host(planes):
    return tuple(None if t is None else t.cpu().numpy() for t in planes)


def out_buffers(n, H, W, dst_dtype, frames=(0, 1), names=rr.PLANES):
    """guarded destinations by reproject_key name, filled with 7"""
    dts = {"warped": dst_dtype, "err": "uint8", "mask": "uint8", "fb2": "float32"}
    return {rr.key(name, f): guarded(np.full((n, KINDS[name], H, W), 7, dts[name])) for f in frames for name in names}


def rows_buffer(n, fill=0):
    return guarded(np.full((n, 256), fill, np.uint8))


def rows_of(ofdg, t):
    return ofdg.reproject_numpy(t)["rows"]


def same_rows(a, b):
    return all(np.array_equal(a[k], b[k]) for k in rr.FIELDS)


def expect_planes(got, want, what):
    for k, t in got.items():
        assert rr.equal_bits(t, want[k]), "%s: %s" % (what, k)


# A workgroup owns a 64 x 16 tile, a lane four pixels, a pair of lanes one 8-byte store of a uint8 row.  8x2 and 24x6: one
# partial tile.  72x40: 2 x 3 tiles, the second column 8 pixels wide.  264x200: 5 x 13 tiles, partial last ones both ways,
# uint8 rows 8 mod 16 wide.  Sample 0 keeps a tile's targets together, sample 1 spreads them over the whole plane.
@pytest.mark.parametrize("W,H", rr.SIZES)
@pytest.mark.parametrize("src_dtype,dst_dtype,flow_dtype", rr.FORMATS)
def test_device_equals_host_twin_and_restatement(ofdg, W, H, src_dtype, dst_dtype, flow_dtype):
    """Every written plane and the rows lie between 0xA5 guards; the inputs stay as they are.  Each call runs twice; the rows
    without accumulation (over rows full of 0xA5: the call clears them) and then with it on top."""
    import torch
    g = make_gen(ofdg, 64, 32)  # (the context's own frame is another: the job gives the size)
    occ_dtype = "uint8" if flow_dtype == "float16" else "float32"
    images, flows, occ, want, rows = rr.case(W, H, src_dtype, flow_dtype, occ_dtype)
    what = "%dx%d %s to %s, flow %s, occ %s" % (W, H, src_dtype, dst_dtype, flow_dtype, occ_dtype)
    host, host_rows = ofdg.host_reproject(images, flows, occ, outputs=ofdg.REPROJ_OUTPUTS, dst_dtype=dst_dtype)
    expect_planes(host, want[dst_dtype], what + ": twin against restatement")
    assert same_rows(host_rows, rows), what
    d_img, d_flow, d_occ = to_dev(images), to_dev(flows), to_dev(occ)
    for _ in range(2):
        bufs = out_buffers(rr.N, H, W, dst_dtype)
        rraw, rout = rows_buffer(rr.N, FILL)
        g.reproject(d_img, d_flow, d_occ, out={k: t for k, (_, t) in bufs.items()}, rows=rout, size=(H, W))
        torch.cuda.synchronize()
        assert guards_intact(list(bufs.values()) + [(rraw, rout)]), what
        got = {k: t.cpu().numpy() for k, (_, t) in bufs.items()}
        expect_planes(got, want[dst_dtype], what + ": device against restatement")
        expect_planes(got, host, what + ": device against twin")
        assert same_rows(rows_of(ofdg, rout), rows), what
        g.reproject(d_img, d_flow, d_occ, rows=rout, accumulate=True, size=(H, W))
        torch.cuda.synchronize()
        assert same_rows(rows_of(ofdg, rout), rr.add_rows(rows, rows)) and guards_intact([(rraw, rout)]), what + ": accumulated"
    for got, src, name in ((to_host(d_img), images, "images"), (to_host(d_flow), flows, "flows"), (to_host(d_occ), occ, "maps")):
        for f in range(2):
            assert rr.equal_bits(got[f], src[f]), what + ": the " + name


@pytest.mark.parametrize("src_dtype,dst_dtype,flow_dtype", [rr.FORMATS[0], rr.FORMATS[7], rr.FORMATS[5]])
def test_subsets_of_frames_and_outputs(ofdg, src_dtype, dst_dtype, flow_dtype):
    """A frame alone, an output alone, the rows alone, no maps, and the least inputs each output needs: what was not asked for
    is not touched, and fields whose inputs are absent stay 0."""
    import torch
    W, H = 72, 40
    g = make_gen(ofdg, W, H)
    images, flows, occ, want, rows = rr.case(W, H, src_dtype, flow_dtype)
    d_img, d_flow, d_occ = to_dev(images), to_dev(flows), to_dev(occ)
    for sel in ((0,), (1,)):
        for names in (("warped",), ("err", "mask"), ("fb2",), rr.PLANES):
            bufs = out_buffers(rr.N, H, W, dst_dtype)
            rraw, rout = rows_buffer(rr.N)
            g.reproject(d_img, d_flow, d_occ, out={rr.key(n_, sel[0]): bufs[rr.key(n_, sel[0])][1] for n_ in names}, rows=rout)
            torch.cuda.synchronize()
            assert guards_intact(list(bufs.values()) + [(rraw, rout)])
            for k, (_, t) in bufs.items():
                name, f = ofdg._REPROJ_KEYS[k]
                if f in sel and name in names:
                    assert rr.equal_bits(t.cpu().numpy(), want[dst_dtype][k]), (sel, names, k)
                else:
                    assert bool((t == 7).all()), (sel, names, k)
            got = rows_of(ofdg, rout)
            assert same_rows(got[:, sel[0]], rows[:, sel[0]]) and not np.ascontiguousarray(got[:, 1 - sel[0]]).view(np.uint8).any()
    # without maps every inside pixel is visible; frame 0 from image1 and flow alone: mask and warped, the err and fb fields stay 0
    _, lean = rr.reproject((None, images[1]), (flows[0], None), None, (0,))
    bufs = out_buffers(rr.N, H, W, dst_dtype, (0,), ("warped", "mask"))
    rraw, rout = rows_buffer(rr.N)
    g.reproject((None, d_img[1]), (d_flow[0], None), None, out={k: t for k, (_, t) in bufs.items()}, rows=rout)
    torch.cuda.synchronize()
    got = rows_of(ofdg, rout)
    assert same_rows(got, lean) and not got["n_hidden"].any() and not got["sum_err_visible"].any() and not got["max_fb2_visible"].any()
    assert got["n_visible"][:, 0].all() and guards_intact(list(bufs.values()) + [(rraw, rout)])
    expect_planes({k: t.cpu().numpy() for k, (_, t) in bufs.items()}, want[dst_dtype], "frame 0 from image1 and flow alone")


def test_known_answers_on_the_device(ofdg):
    """An impulse of 255 in image1 at (10, 3) of 24x6 seen from frame 0: under flow (2, 0) it lands at (8, 3) whole, under
    (2.5, 0) it is halved between (7, 3) and (8, 3) - 128 each, (127.5 * 256 + 128) >> 8 after the tap's own rounding.  A constant
    flow with its exact negative as flow1 leaves no residual inside; outside the mask is 0."""
    import torch
    g = make_gen(ofdg, 24, 6)
    for (u, v), answer in (((2.0, 0.0), {(8, 3): 255}), ((2.5, 0.0), {(7, 3): 128, (8, 3): 128}), ((0.0, -1.5), {(10, 4): 128, (10, 5): 128})):
        images, fl = rr.impulse(u, v)
        out, rows = ofdg.alloc_reproject(1, 6, 24, (0,), ofdg.REPROJ_OUTPUTS, torch.uint8)
        g.reproject(to_dev(images), to_dev((fl, -fl)), None, out=out, rows=rows)
        torch.cuda.synchronize()
        w = out["warped0"].cpu().numpy()[0]
        expect = np.zeros((6, 24), np.uint8)
        for (x, y), b in answer.items():
            expect[y, x] = b
        assert all(np.array_equal(w[c], expect) for c in range(3)), (u, v)
        mask = out["mask0"].cpu().numpy()[0, 0]
        y, x = np.mgrid[0:6, 0:24]
        inside = (np.floor(x + u + 0.5) >= 0) & (np.floor(x + u + 0.5) <= 23) & (np.floor(y + v + 0.5) >= 0) & (np.floor(y + v + 0.5) <= 5)
        assert np.array_equal(mask, inside.astype(np.uint8)) and np.array_equal(out["err0"].cpu().numpy()[0, 0], expect)
        fb2 = out["fb2_0"].cpu().numpy()[0, 0]
        assert not fb2.any() and fb2.dtype == np.float32
        r = rows_of(ofdg, rows)[0, 0]
        assert r["n_visible"] == inside.sum() and r["n_outside"] == 144 - inside.sum() and r["max_fb2_visible"] == 0 and r["sum_err_visible"] == expect.sum()


PLANE_NAMES = ("image0", "image1", "flow")
EXTRAS = ("flow1", "occ0", "occ1")


def rendered(ofdg, g, B, compact, then=None, extras=EXTRAS):
    """forward_counter on the internal stream and `then(planes, True, more)` behind it, nothing waited for in between"""
    import torch
    W, H = g.params.width, g.params.height
    kw = dict(image_dtype=torch.uint8, flow_dtype=torch.float16) if compact else {}
    xkw = dict(flow_dtype=torch.float16, occ_dtype=torch.uint8) if compact else {}
    outs = ofdg.alloc_outputs(B, H, W, **kw)
    ex = ofdg.alloc_extras(B, H, W, extras, **xkw) if extras else None
    src = dict(zip(PLANE_NAMES, outs), **(ex or {}))
    more = then(src, False) if then else None
    torch.cuda.synchronize()  # (the allocations were zeroed on torch's stream)
    g.forward_counter(0, B, *outs, ofdg.STREAM_OWN, extras=ex)
    if then:
        then(src, True, more)
    g.synchronize(ofdg.STREAM_OWN)
    torch.cuda.synchronize()
    return src, more


def twin_of(ofdg, p, frames=(0, 1), fb_thresh=1.0, outputs=None, dst_dtype=None):
    """ofdg_host_reproject on downloaded planes (a dict by name)"""
    h = {k: v.cpu().numpy() for k, v in p.items()}
    return ofdg.host_reproject((h["image0"], h["image1"]), (h["flow"], h.get("flow1")), (h.get("occ0"), h.get("occ1")),
                               outputs=outputs or ofdg.REPROJ_OUTPUTS, frames=frames, fb_thresh=fb_thresh, dst_dtype=dst_dtype)


def reproject_all(ofdg, g, p, out, rows, **kw):
    g.reproject((p["image0"], p["image1"]), (p["flow"], p.get("flow1")), (p.get("occ0"), p.get("occ1")), out=out, rows=rows, stream=ofdg.STREAM_OWN, **kw)


@pytest.mark.parametrize("compact", [False, True])
def test_behind_forward_counter_on_its_own_stream(ofdg, compact):
    """Mode 7, 128x64, B = 3: forward_counter, then reproject on STREAM_OWN with no synchronisation in between, against the twin
    on the downloaded planes."""
    import torch
    W, H, B = 128, 64, 3
    g = make_gen(ofdg, W, H, 7, pool=True, sampler=1, seed=5, batch_size=B)

    def then(src, enqueue, more=None):
        if not enqueue:
            return ofdg.alloc_reproject(B, H, W, (0, 1), ofdg.REPROJ_OUTPUTS, torch.uint8 if compact else None)
        reproject_all(ofdg, g, src, *more)

    src, (out, rows) = rendered(ofdg, g, B, compact, then)
    host, host_rows = twin_of(ofdg, src)
    expect_planes({k: t.cpu().numpy() for k, t in out.items()}, host, "behind forward_counter")
    got = rows_of(ofdg, rows)
    assert same_rows(got, host_rows) and got["n_visible"].all() and got["n_hidden"].any()


@pytest.mark.parametrize("window", ["crop", "spatial"])
def test_behind_the_window(ofdg, window):
    """forward_counter, the 96x48 window and the reprojection of the window's planes on one stream, no synchronisation."""
    W, H, B, wh, ww = 128, 64, 3, 48, 96
    g = make_gen(ofdg, W, H, 7, pool=True, sampler=1, seed=6, batch_size=B)

    def then(src, enqueue, more=None):
        if not enqueue:
            return ofdg.alloc_crop(src, wh, ww), ofdg.alloc_reproject(B, wh, ww, (0, 1), ofdg.REPROJ_OUTPUTS)
        dst, (out, rows) = more
        if window == "crop":
            g.crop(src, dst, first_index=8, occ_window=True, stream=ofdg.STREAM_OWN)
        else:
            g.spatial(src, dst, first_index=8, ranges=ofdg.SPATIAL_FLOWNET, occ_window=True, stream=ofdg.STREAM_OWN)
        reproject_all(ofdg, g, dst, out, rows, size=(wh, ww))

    _, (dst, (out, rows)) = rendered(ofdg, g, B, False, then)
    host, host_rows = twin_of(ofdg, dst)
    expect_planes({k: t.cpu().numpy() for k, t in out.items()}, host, "behind " + window)
    assert same_rows(rows_of(ofdg, rows), host_rows)


def test_mode_9_frame_0_only(ofdg):
    """Mode 9 has no flow1 and no maps: frame 0 without fb2 works; frame 1 and fb2 are refused by name."""
    W, H, B = 128, 64, 2
    g = make_gen(ofdg, W, H, 9, pool=True, sampler=1, seed=3, batch_size=B)
    g.warp_generate(1, 3)
    names = ("warped", "err", "mask", "rows")

    def then(src, enqueue, more=None):
        if not enqueue:
            return ofdg.alloc_reproject(B, H, W, (0,), names)
        reproject_all(ofdg, g, src, *more)

    src, (out, rows) = rendered(ofdg, g, B, False, then, extras=None)
    host, host_rows = twin_of(ofdg, src, frames=(0,), outputs=names)
    expect_planes({k: t.cpu().numpy() for k, t in out.items()}, host, "mode 9")
    assert same_rows(rows_of(ofdg, rows), host_rows) and rows_of(ofdg, rows)["n_visible"][:, 0].all()
    more, _ = ofdg.alloc_reproject(B, H, W, (0, 1), ("fb2", "mask"))
    pair = (src["image0"], src["image1"])
    with pytest.raises(RuntimeError, match=r"ofdg_reproject: flow\[1\]: fb2 of frame 0 needs both flows"):
        g.reproject(pair, (src["flow"], None), None, out={"fb2_0": more["fb2_0"]})
    with pytest.raises(RuntimeError, match=r"ofdg_reproject: flow\[1\]: a flagged frame needs its flow"):
        g.reproject(pair, (src["flow"], None), None, out={"mask1": more["mask1"]})


def test_the_ground_truth_is_self_consistent_on_device_planes(ofdg):
    """One batch of mode 7 at 128x96 over the smooth pool: the visible mean residual is below the hidden one in both frames of
    every sample, and the rows equal the twin's."""
    W, H, B = 128, 96, 4
    g = ofdg.Generator(ofdg.default_params(width=W, height=H, mode=7, sampler=1, seed=2, batch_size=B))
    pool = rr.smooth_pool(4, 2 * W, 2 * H)
    g.pool_alloc(len(pool), 2 * W, 2 * H)
    for k, img in enumerate(pool):
        g.pool_upload(k, img)

    def then(src, enqueue, more=None):
        if not enqueue:
            return ofdg.alloc_reproject(B, H, W, (0, 1), ("rows",))
        reproject_all(ofdg, g, src, *more)

    src, (_, rows) = rendered(ofdg, g, B, False, then)
    _, host_rows = twin_of(ofdg, src, outputs=("rows",))
    assert same_rows(rows_of(ofdg, rows), host_rows)
    r = ofdg.reproject_numpy(rows)
    print("visible", r["mean_err_visible"], "hidden", r["mean_err_hidden"])
    assert (r["rows"]["n_visible"] > 0).all() and (r["rows"]["n_hidden"] > 0).all()
    assert (r["mean_err_visible"] < r["mean_err_hidden"]).all()


def test_three_calls_in_flight(ofdg):
    """Two caller streams and STREAM_OWN, each with planes and rows of its own, synchronised once at the end."""
    import torch
    W, H = 72, 40
    g = make_gen(ofdg, W, H, 7, pool=True, sampler=1, batch_size=1)
    rendered(ofdg, g, 1, False, extras=None)  # (STREAM_OWN needs a former forward call)
    cases = [rr.case(W, H, *fmt) for fmt in (("uint8", "float32"), ("float32", "float16"), ("uint8", "float16"))]
    streams = [torch.cuda.Stream(), torch.cuda.Stream(), None]
    runs = []
    for (images, flows, occ, want, rows), s in zip(cases, streams):
        dev = (to_dev(images), to_dev(flows), to_dev(occ))
        runs.append((dev, ofdg.alloc_reproject(rr.N, H, W, (0, 1), ofdg.REPROJ_OUTPUTS), want, rows, s))
    torch.cuda.synchronize()
    for (d_img, d_flow, d_occ), (out, rows_t), _, _, s in runs:
        g.reproject(d_img, d_flow, d_occ, out=out, rows=rows_t, stream=ofdg.STREAM_OWN if s is None else s.cuda_stream)
    torch.cuda.synchronize()
    g.synchronize(ofdg.STREAM_OWN)
    torch.cuda.synchronize()
    for _, (out, rows_t), want, rows, _ in runs:
        expect_planes({k: t.cpu().numpy() for k, t in out.items()}, want["float32"], "in flight")
        assert same_rows(rows_of(ofdg, rows_t), rows)


LOADER = dict(extras=("flow1", "occ0", "occ1"), crop=(48, 96))


def loader_batches(ofdg, count, start=0, **kw):
    import torch
    p = ofdg.default_params(width=128, height=64, mode=7, batch_size=2, sampler=1, seed=21)
    out = []
    loader = ofdg.FlowLoader(p, pool=lambda g: g.pool_synthetic(3, 256, 128, 11), prefetch=3, start=start, **dict(LOADER, **kw))
    it = iter(loader)
    for _ in range(count):
        batch = next(it)
        torch.cuda.current_stream().synchronize()
        out.append(tuple({n_: v.cpu().numpy() for n_, v in t.items()} if isinstance(t, dict) else t.cpu().numpy() for t in batch))
    return out


def test_the_loader_reprojects_the_sharp_unerased_window(ofdg):
    """reproject= with and without motion_blur=, photo= and erase= behind it: rows and planes equal the twin's on the plain
    loader's cropped planes, so the stage reads sharp, un-erased frames and maps.  Resume at start=2 gives batch 2; without
    reproject= the batch has the names it had."""
    opts = dict(frames=(0, 1), fb_thresh=1.5, outputs=("rows", "err", "fb2"))
    plain = loader_batches(ofdg, 3)
    assert len(plain[0]) == 4 and "reproject" not in plain[0][3] and not any(k in plain[0][3] for k in ofdg._REPROJ_KEYS)
    expect = []
    for b in plain:
        x = b[3]
        expect.append(ofdg.host_reproject((b[0], b[1]), (b[2], x["flow1"]), (x["occ0"], x["occ1"]), outputs=opts["outputs"], fb_thresh=1.5))
    later = dict(motion_blur=dict(ofdg.MBLUR_DEFAULT, prob=1.0), photo=ofdg.PHOTO_FLOWNET, erase=dict(ofdg.ERASE_RAFT, prob=1.0))
    for kw, first, count in ((dict(reproject=opts), 0, 3), (dict(reproject=opts, **later), 0, 2), (dict(reproject=opts), 2, 1)):
        got = loader_batches(ofdg, count, start=first, **kw)
        for k, b in enumerate(got):
            planes, rows = expect[first + k]
            x = b[3]
            assert x["reproject"].dtype == np.uint8 and x["reproject"].shape == (2, 256)
            assert same_rows(rows_of(ofdg, x["reproject"]), rows), (sorted(kw), k)
            assert set(planes) == {"err0", "err1", "fb2_0", "fb2_1"} and all(rr.equal_bits(x[n_], planes[n_]) for n_ in planes), (sorted(kw), k)
            assert "warped0" not in x and "mask0" not in x
            if len(kw) == 1:  # the stage changes nothing of the batch itself
                assert all(rr.equal_bits(b[i], plain[first + k][i]) for i in range(3))
                assert all(rr.equal_bits(x[n_], plain[first + k][3][n_]) for n_ in plain[first + k][3])


def test_refusals_enqueue_nothing(ofdg):
    """Every refusal names its field, leaves planes and rows as they were, and a valid call on the same context still works."""
    import torch
    W, H = 24, 6
    g = make_gen(ofdg, W, H)
    images, flows, occ, want, rows = rr.case(W, H, "uint8", "float32")
    d_img, d_flow, d_occ = to_dev(images), to_dev(flows), to_dev(occ)
    bufs = out_buffers(rr.N, H, W, "uint8")
    out = {k: t for k, (_, t) in bufs.items()}
    rraw, rout = rows_buffer(rr.N, 7)
    with pytest.raises(RuntimeError, match="ofdg_reproject: stream: OFDG_STREAM_OWN before any render / forward call"):
        g.reproject(d_img, d_flow, d_occ, out=out, rows=rout, stream=ofdg.STREAM_OWN)
    L, h = ofdg.lib(), g.h
    import ctypes as C

    def job(**kw):
        j = ofdg._reproject_job(d_img, d_flow, d_occ, out, rout.data_ptr(), lambda t: t.data_ptr(), (ofdg.FMT_U8, ofdg.FMT_U8, ofdg.FMT_F32, ofdg.FMT_U8),
                                (0, 0), (0, 1), 1.0, False)
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(j, k)[v[0]] = v[1]
            else:
                setattr(j, k, v)
        return j

    refusals = [(dict(img_fmt=ofdg.FMT_F16), "img_fmt must be"), (dict(dst_fmt=7), "dst_fmt must be"), (dict(flow_fmt=ofdg.FMT_U8), "flow_fmt must be"),
                (dict(occ_fmt=ofdg.FMT_F16), "occ_fmt must be"), (dict(flags=11), "flags holds unknown bits"), (dict(flags=4), "flags: no frame is flagged"),
                (dict(flags=1), "flags: frame 1 has an output but is not flagged"), (dict(reserved=(1, 1)), "reserved must be 0"),
                (dict(fb_thresh_q8=-1), "fb_thresh_q8 must lie in"), (dict(fb_thresh_q8=(1 << 23) + 1), "fb_thresh_q8 must lie in"),
                (dict(width=W), "width and height must both be 0 or both be set"), (dict(width=12, height=6), "width must be a multiple of 8"),
                (dict(flow=(0, None)), r"flow\[0\]: a flagged frame needs its flow"), (dict(img=(1, None)), r"img\[1\]: warped, err and mask of frame 0 need the other frame"),
                (dict(warped=(0, out["mask0"].data_ptr())), "a destination range overlaps another range of the job"),
                (dict(err=(1, d_img[0].data_ptr())), "a destination range overlaps another range of the job"),
                (dict(rows=rout.data_ptr() + 8), "rows must be 16-byte aligned"), (dict(mask=(0, out["mask0"].data_ptr() + 4)), r"mask\[0\] must be 16-byte aligned"),
                (dict(flow=(1, d_flow[1].data_ptr() + 4)), r"flow\[1\] must be 16-byte aligned")]
    import re
    for kw, text in refusals:
        assert L.ofdg_reproject(h, C.byref(job(**kw)), rr.N, None) == ofdg.EINVAL, kw
        assert re.search("^ofdg_reproject: " + text, L.ofdg_last_error(h).decode()), (kw, L.ofdg_last_error(h))
    assert L.ofdg_reproject(h, None, rr.N, None) == ofdg.EINVAL and L.ofdg_reproject(h, C.byref(job()), 0, None) == ofdg.EINVAL
    none = job(rows=None)
    for name in rr.PLANES:
        getattr(none, name)[0] = getattr(none, name)[1] = None
    assert L.ofdg_reproject(h, C.byref(none), rr.N, None) == ofdg.EINVAL and b"rows: no output is given" in L.ofdg_last_error(h)
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in out.values()) and bool((rout == 7).all()) and guards_intact(list(bufs.values()) + [(rraw, rout)])
    g.reproject(d_img, d_flow, d_occ, out=out, rows=rout)
    torch.cuda.synchronize()
    expect_planes({k: t.cpu().numpy() for k, t in out.items()}, want["uint8"], "the valid call afterwards")
    assert same_rows(rows_of(ofdg, rout), rows)
