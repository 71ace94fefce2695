"""GPU tests of the spatial augmentation (ofdg_spatial, include/ofdg.h): the device planes against ofdg_host_spatial and against
the numpy restatement (tests/spatial_reference.py), byte for byte - every format, shrinking and enlarging, tiles partial on
both axes, subsets of planes, every record of the CPU tests, between guard bytes; drawn records; behind a render call without
synchronisation with the sized reductions behind it (rigid, compact formats, mode 9), with three calls in flight, through
the loader - and the refusals."""
import ctypes as C
import itertools

import numpy as np
import pytest

import flow_pyramid_reference as fpr
import flow_stats_reference as fsr
import spatial_reference as sr

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 64  # bytes in front of and behind every destination (keeps the 16-byte alignment)
FORMATS = list(itertools.product(("float32", "uint8"), ("float32", "float16"), ("float32", "uint8")))
SHAPES = sr.SHAPES + [sr.GPU_SHAPE]
SUBSETS = [(sr.PLANES, False), (sr.PLANES, True), (("flow",), False), (("label0", "label1"), False), (("occ0", "flow"), True),
           (("image1", "occ1"), False)]
RANGES = dict(zoom_log=0.3, rot=0.4, squeeze_log=0.2, translate=0.75, pair_zoom_log=0.05, pair_rot=0.04, pair_translate=1.5)


def make_gen(ofdg, W, H, mode=7, pool=False, **kw):
    g = ofdg.Generator(ofdg.default_params(width=W, height=H, mode=mode, **kw))
    if pool:
        g.pool_synthetic(3, 2 * W, 2 * H, 11)
    return g


def guarded(shape, dtype):
    """(the whole uint8 buffer, filled with 0xA5; the tensor of `shape` in its middle)"""
    import torch
    size = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    raw = torch.full((GUARD + size + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    return raw, raw[GUARD:GUARD + size].view(dtype).view(shape)


def guarded_like(src, out_h, out_w):
    return {k: guarded(tuple(t.shape[:-2]) + (out_h, out_w), t.dtype) for k, t in src.items()}


def guards_intact(bufs):
    return all(bool((raw[:GUARD] == FILL).all()) and bool((raw[-GUARD:] == FILL).all()) for raw, _ in bufs)


def to_host(planes):
    return {k: t.cpu().numpy() for k, t in planes.items()}


@pytest.mark.parametrize("W,H,ow,oh", SHAPES)
@pytest.mark.parametrize("image,flow,occ", FORMATS)
def test_device_equals_host_twin_and_restatement(ofdg, W, H, ow, oh, image, flow, occ):
    """The destinations start as 0xA5 bytes between 0xA5 guards: equality shows every element was written, the guards that
    nothing else was.  The context's frame is another size than the planes: the job carries its own."""
    import torch
    g = make_gen(ofdg, 64, 32)
    src = sr.planes(W, H, image, flow, occ)
    dev = {k: torch.from_numpy(np.array(v)).cuda() for k, v in src.items()}
    recs = sr.records(W, H, ow, oh)
    drecs = torch.from_numpy(recs).cuda()
    for names, window in SUBSETS:
        part = {k: src[k] for k in names}
        want, want_recs = sr.spatial(part, recs, ow, oh, window)
        host, host_recs = ofdg.host_spatial(part, oh, ow, recs=recs, occ_window=window)
        bufs = guarded_like({k: dev[k] for k in names}, oh, ow)
        rraw, rout = guarded((sr.N, 14), torch.float64)
        g.spatial({k: dev[k] for k in names}, {k: t for k, (_, t) in bufs.items()}, recs=drecs, occ_window=window, recs_out=rout, size=(H, W))
        torch.cuda.synchronize()
        what = "%dx%d to %dx%d %s window %s" % (W, H, ow, oh, names, window)
        got = to_host({k: t for k, (_, t) in bufs.items()})
        sr.expect_equal(got, want, what + " against the restatement")
        sr.expect_equal(got, host, what + " against ofdg_host_spatial")
        assert guards_intact(list(bufs.values()) + [(rraw, rout)]), what
        assert rout.cpu().numpy().tobytes() == want_recs.tobytes() and host_recs.tobytes() == want_recs.tobytes(), what
        assert drecs.cpu().numpy().tobytes() == recs.tobytes()
    for k, t in dev.items():
        assert t.cpu().numpy().tobytes() == src[k].tobytes(), k  # the inputs are as they were


@pytest.mark.parametrize("first_index", [0, (1 << 32) + 3])
def test_drawn_records(ofdg, first_index):
    import torch
    W, H, ow, oh, n = 160, 100, 136, 66, 9
    g = make_gen(ofdg, W, H)
    src = {k: v[:n] for k, v in sr.planes(W, H, "uint8", "float16", "float32").items()}
    dev = {k: torch.from_numpy(np.array(v)).cuda() for k, v in src.items()}
    out = ofdg.alloc_spatial(dev, oh, ow)
    rout = torch.full((n, 14), -1, dtype=torch.float64, device="cuda")
    g.spatial(dev, out, first_index=first_index, seed=12345, ranges=RANGES, hflip=True, vflip=True, occ_window=True, recs_out=rout)
    torch.cuda.synchronize()
    used = rout.cpu().numpy()
    drawn = sr.drawn_records(12345, first_index, n, W, H, ow, oh, RANGES, sr.RANDOM_HFLIP | sr.RANDOM_VFLIP)
    for i in range(n):
        assert ofdg.spatial_draw(12345, first_index + i, W, H, ow, oh, RANGES, hflip=True, vflip=True).tobytes() == drawn[i].tobytes()
    want, want_used = sr.spatial(src, drawn, ow, oh, True)
    assert used.tobytes() == want_used.tobytes()
    host, _ = ofdg.host_spatial(src, oh, ow, recs=used, occ_window=True)
    sr.expect_equal(to_host(out), host)
    sr.expect_equal(to_host(out), want)
    assert len({tuple(r) for r in used.tolist()}) == n and len({(r[0] > 0, r[4] > 0) for r in used.tolist()}) > 1


def rendered(ofdg, g, B, compact, batch, oh, ow, first_index):
    """render(..., all extras) on the internal stream, the warp of all eight planes behind it and both reductions of the warped
    flow and occ0 behind that, nothing waited for in between."""
    import torch
    W, H = g.params.width, g.params.height
    if compact:
        outs = ofdg.alloc_outputs(B, H, W, image_dtype=torch.uint8, flow_dtype=torch.float16)
        ex = ofdg.alloc_extras(B, H, W, flow_dtype=torch.float16, occ_dtype=torch.uint8)
    else:
        outs = ofdg.alloc_outputs(B, H, W)
        ex = ofdg.alloc_extras(B, H, W)
    src = dict(zip(("image0", "image1", "flow"), outs), **ex)
    dst = ofdg.alloc_spatial(src, oh, ow)
    recs = torch.zeros((B, 14), dtype=torch.float64, device="cuda")
    L = fpr.max_levels(oh, ow)
    pyr = ofdg.alloc_flow_pyramid(B, oh, ow, L, dst["flow"].dtype, weights=True)
    rows = ofdg.alloc_flow_stats(B)
    torch.cuda.synchronize()  # (the allocations were zeroed on torch's stream)
    tasks, bps, n = batch
    g.render(tasks, B, bps, n, *outs, ofdg.STREAM_OWN, extras=ex)
    g.spatial(src, dst, first_index=first_index, ranges=RANGES, hflip=True, vflip=True, occ_window=True, recs_out=recs, stream=ofdg.STREAM_OWN)
    g.flow_stats(dst["flow"], rows, occ=dst["occ0"], stream=ofdg.STREAM_OWN, size=(oh, ow))
    g.flow_pyramid(dst["flow"], L, occ=dst["occ0"], out=pyr, stream=ofdg.STREAM_OWN, size=(oh, ow))
    g.synchronize(ofdg.STREAM_OWN)
    torch.cuda.synchronize()
    return to_host(src), to_host(dst), recs.cpu().numpy(), pyr, rows, L


def test_end_to_end_rigid_and_compact(ofdg):
    """160x100 to 128x64, mode 7, all extras: float32, then the compact formats; the sized reductions on the warped flow and
    occ0 against their host twins on the host-warped arrays."""
    W, H, B, ow, oh = 160, 100, 3, 128, 64
    g = make_gen(ofdg, W, H, 7, pool=True, seed=5)
    batch = g.sample(B)
    for compact in (False, True):
        src, dst, recs, pyr, rows, L = rendered(ofdg, g, B, compact, batch, oh, ow, 40)
        what = "compact %s" % compact
        assert L == 6 and src["flow"].dtype == (np.float16 if compact else np.float32) and src["occ1"].dtype == (np.uint8 if compact else np.float32)
        want, used = ofdg.host_spatial(src, oh, ow, first_index=40, seed=5, ranges=RANGES, hflip=True, vflip=True, occ_window=True)
        drawn = sr.drawn_records(5, 40, B, W, H, ow, oh, RANGES, 12)
        assert recs.tobytes() == used.tobytes() and used.tobytes() == sr.sanitise_all(drawn, W, H, ow, oh).tobytes(), what
        sr.expect_equal(dst, want, what)
        sr.expect_equal(dst, sr.spatial(src, drawn, ow, oh, True)[0], what + " against the restatement")
        lv, wt = ofdg.host_flow_pyramid(want["flow"], L, want["occ0"], weights=True)
        fpr.expect_equal([t.cpu().numpy() for t in pyr[0]], lv, what + " pyramid")
        fpr.expect_equal([t.cpu().numpy() for t in pyr[1]], wt, what + " pyramid weights")
        fsr.expect_equal(ofdg.flow_stats_numpy(rows)["rows"], fsr.rows_of(ofdg.host_flow_stats(want["flow"], want["occ0"], 2.0)), what + " statistics")
        assert np.abs(want["flow"].astype(np.float32)).max() > 0 and want["occ0"].any() and want["label0"].any() and want["image1"].any()


def test_end_to_end_mode_9(ofdg):
    import torch
    W, H, B, ow, oh = 160, 100, 3, 128, 64
    g = make_gen(ofdg, W, H, 9, pool=True, sampler=1, seed=3, batch_size=B)
    g.warp_generate(1, 3)
    outs = ofdg.alloc_outputs(B, H, W)
    src = dict(zip(("image0", "image1", "flow"), outs))
    dst = ofdg.alloc_spatial(src, oh, ow)
    torch.cuda.synchronize()
    g.forward_counter(0, B, *outs, ofdg.STREAM_OWN)
    g.spatial(src, dst, first_index=0, ranges=RANGES, vflip=True, stream=ofdg.STREAM_OWN)
    g.synchronize(ofdg.STREAM_OWN)
    torch.cuda.synchronize()
    want, _ = ofdg.host_spatial(to_host(src), oh, ow, first_index=0, seed=3, ranges=RANGES, vflip=True)
    sr.expect_equal(to_host(dst), want)
    assert np.abs(want["flow"]).max() > 0


def test_three_calls_in_flight(ofdg):
    """Two calls on two caller streams and one on OFDG_STREAM_OWN, each into its own buffers, one wait at the end."""
    import torch
    W, H, B, ow, oh = 160, 100, 2, 128, 64
    g = make_gen(ofdg, W, H, 7, pool=True)
    users = [torch.cuda.Stream(), torch.cuda.Stream()]
    batches = [g.sample(B) for _ in range(3)]
    outs = [ofdg.alloc_outputs(B, H, W) for _ in range(3)]
    srcs = [dict(zip(("image0", "image1", "flow"), o)) for o in outs]
    dsts = [ofdg.alloc_spatial(s, oh, ow) for s in srcs]
    torch.cuda.synchronize()
    streams = [users[0].cuda_stream, users[1].cuda_stream, ofdg.STREAM_OWN]
    for k, ((tasks, bps, n), o, s, d, st) in enumerate(zip(batches, outs, srcs, dsts, streams)):
        g.render(tasks, B, bps, n, *o, st)
        g.spatial(s, d, first_index=100 * k, seed=9, ranges=RANGES, hflip=True, stream=st)
    for st in streams:
        g.synchronize(st)
    torch.cuda.synchronize()
    flows = [o[2].cpu().numpy() for o in outs]
    assert not np.array_equal(flows[0], flows[1]) and not np.array_equal(flows[1], flows[2])
    for k, (s, d) in enumerate(zip(srcs, dsts)):
        want, _ = ofdg.host_spatial(to_host(s), oh, ow, first_index=100 * k, seed=9, ranges=RANGES, hflip=True)
        sr.expect_equal(to_host(d), want, "call %d" % k)


def test_flowloader_spatial(ofdg):
    import torch
    W, H, B, ow, oh = 128, 96, 2, 96, 48
    kw = dict(width=W, height=H, mode=7, batch_size=B, sampler=1, seed=21)
    pool = lambda g: g.pool_synthetic(3, 2 * W, 2 * H, 11)  # noqa: E731
    make = lambda **more: ofdg.FlowLoader(ofdg.default_params(**kw), pool=pool, prefetch=3, extras=("occ0",), **more)  # noqa: E731
    photo = dict(gamma_log=0.3, contrast_log=0.2, brightness=0.05, colour_log=0.1, sigma_max=4.0, pair_gamma_log=0.02)
    warped = dict(spatial=RANGES, spatial_size=(oh, ow), spatial_hflip=True, photo=photo, pyramid=2, stats=True)
    it, pit = iter(make(**warped)), iter(make())
    third = None
    for step in range(3):
        i0, i1, fl, more = next(it)
        p = next(pit)
        torch.cuda.current_stream().synchronize()
        assert set(more) == {"occ0", "spatial", "photo", "flow_stats", "flow_pyramid"} and len(more["flow_pyramid"]) == 2
        first = ofdg.shard_first_index(step, B, 1, 0)
        recs = sr.sanitise_all(sr.drawn_records(21, first, B, W, H, ow, oh, RANGES, sr.RANDOM_HFLIP), W, H, ow, oh)
        assert more["spatial"].cpu().numpy().tobytes() == recs.tobytes() and more["spatial"].dtype == torch.float64
        # the manual sequence: the warp of the plain loader's batch, then the photometric step on the warped frames
        src = to_host(dict(image0=p[0], image1=p[1], flow=p[2], occ0=p[3]["occ0"]))
        want, _ = ofdg.host_spatial(src, oh, ow, recs=recs, occ_window=True)
        frames, prec = ofdg.host_photo((want["image0"], want["image1"]), first_index=first, seed=21, ranges=photo)
        want["image0"], want["image1"] = frames
        assert np.array_equal(more["photo"].cpu().numpy(), prec)
        got = to_host(dict(image0=i0, image1=i1, flow=fl, occ0=more["occ0"]))
        sr.expect_equal(got, want, "batch %d" % step)
        fpr.expect_equal([t.cpu().numpy() for t in more["flow_pyramid"]], ofdg.host_flow_pyramid(want["flow"], 2, want["occ0"]))
        fsr.expect_equal(ofdg.flow_stats_numpy(more["flow_stats"])["rows"], fsr.flow_stats(want["flow"], want["occ0"], 2.0))
        third = got
    assert third["occ0"].any()
    resumed = iter(make(start=2, **warped))
    i0, i1, fl, more = next(resumed)
    torch.cuda.current_stream().synchronize()
    sr.expect_equal(to_host(dict(image0=i0, image1=i1, flow=fl, occ0=more["occ0"])), third, "resumed at batch 2")
    assert more["spatial"].cpu().numpy().tobytes() == recs.tobytes()
    with pytest.raises(ValueError, match="objects"):
        ofdg.FlowLoader(ofdg.default_params(**kw), pool=pool, extras=("label0", "label1"), objects=True, spatial=RANGES, spatial_size=(oh, ow))
    with pytest.raises(ValueError, match="crop"):
        ofdg.FlowLoader(ofdg.default_params(**kw), pool=pool, crop=(oh, ow), spatial=RANGES, spatial_size=(oh, ow))
    with pytest.raises(ValueError, match="spatial_size"):
        ofdg.FlowLoader(ofdg.default_params(**kw), pool=pool, spatial=RANGES)
    with pytest.raises(ValueError, match="unknown range"):
        ofdg.FlowLoader(ofdg.default_params(**kw), pool=pool, spatial=dict(zoom=1.0), spatial_size=(oh, ow))


def test_refusals_enqueue_nothing(ofdg):
    import torch
    W, H, B, ow, oh = 128, 96, 2, 96, 48
    g = make_gen(ofdg, W, H, 7, pool=True, batch_size=B)
    outs = ofdg.alloc_outputs(B, H, W, image_dtype=torch.uint8, flow_dtype=torch.float16)
    ex = ofdg.alloc_extras(B, H, W, flow_dtype=torch.float16)
    src = dict(zip(("image0", "image1", "flow"), outs), **ex)
    bufs = guarded_like(src, oh, ow)
    recs = torch.zeros((B, 14), dtype=torch.float64, device="cuda")
    rraw, rout = guarded((B, 14), torch.float64)
    torch.cuda.synchronize()
    lib, vp = ofdg.lib(), C.c_void_p
    codes = dict(image_fmt=ofdg.FMT_U8, flow_fmt=ofdg.FMT_F16, occ_fmt=ofdg.FMT_F32)

    def job(planes=sr.PLANES, **kw):
        j = ofdg.SpatialJob()
        for k, name in enumerate(sr.PLANES):
            if name in planes:
                j.src[k], j.dst[k] = src[name].data_ptr(), bufs[name][1].data_ptr()
        j.recs, j.recs_out, j.out_w, j.out_h = recs.data_ptr(), rout.data_ptr(), ow, oh
        for k, v in dict(codes, **kw).items():
            if k in ("src", "dst"):
                for idx, val in v.items():
                    getattr(j, k)[idx] = val
            elif k == "reserved":
                j.reserved[v[0]] = v[1]
            else:
                setattr(j, k, v)
        return j

    def refused(word, j, n=B, stream=0):
        rc = lib.ofdg_spatial(g.h, None if j is None else C.byref(j), n, vp(stream))
        assert rc == ofdg.EINVAL, word
        msg = lib.ofdg_last_error(g.h).decode()
        assert msg.startswith("ofdg_spatial") and word in msg, (word, msg)
        g.synchronize()
        torch.cuda.synchronize()
        assert all(bool((raw == FILL).all()) for raw, _ in list(bufs.values()) + [(rraw, rout)]), word

    refused("OFDG_STREAM_OWN", job(), stream=ofdg.STREAM_OWN)  # a fresh context: no call has worked on an internal stream yet
    refused("job", None)
    refused("n_samples", job(), n=0)
    refused("width and height", job(height=H))
    refused("width", job(width=W + 4, height=H))
    for bad in (0, 4, 100):
        refused("out_w", job(out_w=bad))
    for bad in (0, 47):
        refused("out_h", job(out_h=bad))
    refused("flags", job(flags=32))
    refused("reserved", job(reserved=(1, -1)))
    refused("image_fmt", job(image_fmt=ofdg.FMT_F16))
    refused("flow_fmt", job(flow_fmt=ofdg.FMT_U8))
    refused("occ_fmt", job(occ_fmt=7))
    refused("zoom_log", job(zoom_log=-1.0))
    refused("pair_rot", job(pair_rot=float("nan")))
    refused("translate", job(translate=1.25))
    refused("no plane", job(planes=()))
    refused("dst", job(dst={3: None}))
    refused("src", job(src={7: None}))
    refused("occ0", job(planes=("occ0",), flags=sr.OCC_WINDOW))
    refused("occ1", job(planes=("occ1", "flow"), flags=sr.OCC_WINDOW))
    refused("4-byte", job(src={0: src["image0"].data_ptr() + 2}))
    refused("8-byte", job(src={2: src["flow"].data_ptr() + 4}))
    refused("16-byte", job(src={4: src["occ0"].data_ptr() + 8}))
    refused("16-byte", job(dst={6: bufs["label0"][1].data_ptr() + 8}))
    refused("recs must", job(recs=recs.data_ptr() + 8))
    refused("recs_out", job(recs_out=rout.data_ptr() + 8))
    refused("overlaps", job(dst={1: src["image1"].data_ptr()}))
    refused("overlaps", job(dst={5: bufs["occ0"][1].data_ptr() + 16}))
    refused("overlaps", job(recs_out=recs.data_ptr()))
    # a valid call on the same context still works, also on OFDG_STREAM_OWN once a call has been made
    g.forward(*outs, ofdg.STREAM_OWN, extras=ex)
    dst = {k: t for k, (_, t) in bufs.items()}
    g.spatial(src, dst, first_index=7, ranges=RANGES, hflip=True, vflip=True, occ_window=True, recs_out=rout, stream=ofdg.STREAM_OWN)
    g.synchronize(ofdg.STREAM_OWN)
    torch.cuda.synchronize()
    want, used = ofdg.host_spatial(to_host(src), oh, ow, first_index=7, seed=g.params.seed, ranges=RANGES, hflip=True, vflip=True, occ_window=True)
    sr.expect_equal(to_host(dst), want)
    assert rout.cpu().numpy().tobytes() == used.tobytes() and guards_intact(list(bufs.values()) + [(rraw, rout)])
