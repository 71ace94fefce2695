"""GPU tests of the training crop (ofdg_crop, include/ofdg.h): the device planes against ofdg_host_crop and against the numpy
restatement (tests/crop_reference.py), byte for byte - every format, windows at every alignment, flips, records outside the
frame, subsets of planes, between guard bytes; drawn records; behind a render call without synchronisation with the sized
reductions behind it (rigid, compact formats, mode 9), with three calls in flight, through the loader - and the refusals."""
import ctypes as C
import itertools

import numpy as np
import pytest

import crop_reference as cr
import flow_pyramid_reference as fpr
import flow_stats_reference as fsr

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 64  # bytes in front of and behind every destination (keeps the 16-byte alignment)
FORMATS = list(itertools.product(("float32", "uint8"), ("float32", "float16"), ("float32", "uint8")))
# the shapes of the CPU tests (a workgroup moves 1024 16-byte pieces of a channel: 160x100 to 136x66 is 2244 pieces of float32 -
# three workgroups, the last partial - and 1122 of binary16), and one whose uint8 channels take three workgroups too (2077
# pieces), 8 mod 16 wide, so that pieces straddle two rows
SHAPES = cr.SHAPES + [(264, 200, 248, 134)]
SUBSETS = [(cr.PLANES, False), (cr.PLANES, True), (("flow",), False), (("label0", "label1"), False), (("occ0", "flow"), True)]


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


def guarded_like(src, crop_h, crop_w):
    """name -> (raw, tensor) for the destination of every plane in src (torch tensors)"""
    return {k: guarded(tuple(t.shape[:-2]) + (crop_h, crop_w), t.dtype) for k, t in src.items()}


def guards_intact(bufs):
    return all(bool((raw[:GUARD] == FILL).all()) and bool((raw[-GUARD:] == FILL).all()) for raw, _ in bufs)


def to_host(planes):
    return {k: t.cpu().numpy() for k, t in planes.items()}


@pytest.mark.parametrize("W,H,cw,ch", SHAPES)
@pytest.mark.parametrize("image,flow,occ", FORMATS)
def test_device_equals_host_twin_and_restatement(ofdg, W, H, cw, ch, image, flow, occ):
    """The destinations start as 0xA5 bytes between 0xA5 guards: equality shows every element was written, the guards that
    nothing else was."""
    import torch
    g = make_gen(ofdg, W, H)
    src = cr.planes(W, H, image, flow, occ)
    dev = {k: torch.from_numpy(np.array(v)).cuda() for k, v in src.items()}
    recs = cr.records(W, H, cw, ch)
    drecs = torch.from_numpy(recs).cuda()
    for names, window in SUBSETS:
        part = {k: src[k] for k in names}
        want, want_recs = cr.crop(part, recs, cw, ch, window)
        host, host_recs = ofdg.host_crop(part, ch, cw, recs=recs, occ_window=window)
        bufs = guarded_like({k: dev[k] for k in names}, ch, cw)
        rraw, rout = guarded((cr.N, 4), torch.int32)
        g.crop({k: dev[k] for k in names}, {k: t for k, (_, t) in bufs.items()}, recs=drecs, occ_window=window, recs_out=rout)
        torch.cuda.synchronize()
        what = "%dx%d to %dx%d %s window %s" % (W, H, cw, ch, names, window)
        got = to_host({k: t for k, (_, t) in bufs.items()})
        cr.expect_equal(got, want, what + " against the restatement")
        cr.expect_equal(got, host, what + " against ofdg_host_crop")
        assert guards_intact(list(bufs.values()) + [(rraw, rout)]), what
        assert np.array_equal(rout.cpu().numpy(), want_recs) and np.array_equal(host_recs, want_recs), what
        assert torch.equal(drecs.cpu(), torch.from_numpy(recs))


@pytest.mark.parametrize("first_index", [0, (1 << 32) + 3])
def test_drawn_records(ofdg, first_index):
    import torch
    W, H, cw, ch = 160, 100, 136, 66
    g = make_gen(ofdg, W, H)
    src = cr.planes(W, H, "uint8", "float16", "float32")
    dev = {k: torch.from_numpy(np.array(v)).cuda() for k, v in src.items()}
    out = ofdg.alloc_crop(dev, ch, cw)
    rout = torch.full((cr.N, 4), -1, dtype=torch.int32, device="cuda")
    g.crop(dev, out, first_index=first_index, seed=12345, hflip=True, vflip=True, recs_out=rout)
    torch.cuda.synchronize()
    used = rout.cpu().numpy()
    for i in range(cr.N):
        assert tuple(used[i]) == ofdg.crop_draw(12345, first_index + i, W, H, cw, ch, hflip=True, vflip=True) + (0,)
    assert np.array_equal(used, cr.drawn_records(12345, first_index, cr.N, W, H, cw, ch, cr.RANDOM_HFLIP | cr.RANDOM_VFLIP))
    host, _ = ofdg.host_crop(src, ch, cw, recs=used)
    cr.expect_equal(to_host(out), host)
    assert len({tuple(r) for r in used.tolist()}) == cr.N and len(set(used[:, 2].tolist())) > 1


def rendered(ofdg, g, B, compact, batch, ch, cw, first_index):
    """render(..., all extras) on the internal stream, the crop of all eight planes behind it and both reductions of the cropped
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
    dst = ofdg.alloc_crop(src, ch, cw)
    recs = torch.zeros((B, 4), dtype=torch.int32, device="cuda")
    L = fpr.max_levels(ch, cw)
    pyr = ofdg.alloc_flow_pyramid(B, ch, cw, L, dst["flow"].dtype, weights=True)
    rows = ofdg.alloc_flow_stats(B)
    torch.cuda.synchronize()  # (the allocations were zeroed on torch's stream)
    tasks, bps, n = batch
    g.render(tasks, B, bps, n, *outs, ofdg.STREAM_OWN, extras=ex)
    g.crop(src, dst, first_index=first_index, hflip=True, vflip=True, occ_window=True, recs_out=recs, stream=ofdg.STREAM_OWN)
    g.flow_stats(dst["flow"], rows, occ=dst["occ0"], stream=ofdg.STREAM_OWN, size=(ch, cw))
    g.flow_pyramid(dst["flow"], L, occ=dst["occ0"], out=pyr, stream=ofdg.STREAM_OWN, size=(ch, cw))
    g.synchronize(ofdg.STREAM_OWN)
    torch.cuda.synchronize()
    return to_host(src), to_host(dst), recs.cpu().numpy(), pyr, rows, L


def test_end_to_end_rigid_and_compact(ofdg):
    """128x64 to 96x48, mode 7, all extras: float32, then the compact formats; the sized reductions on the cropped flow and
    occ0 against their host twins on the host-cropped arrays."""
    W, H, B, cw, ch = 128, 64, 3, 96, 48
    g = make_gen(ofdg, W, H, 7, pool=True, seed=5)
    batch = g.sample(B)
    for compact in (False, True):
        src, dst, recs, pyr, rows, L = rendered(ofdg, g, B, compact, batch, ch, cw, 40)
        what = "compact %s" % compact
        assert L == 4 and src["flow"].dtype == (np.float16 if compact else np.float32) and src["occ1"].dtype == (np.uint8 if compact else np.float32)
        assert src["label0"].shape == (B, H, W) and dst["label0"].shape == (B, ch, cw)
        want, used = ofdg.host_crop(src, ch, cw, first_index=40, seed=5, hflip=True, vflip=True, occ_window=True)
        assert np.array_equal(recs, used) and np.array_equal(used, cr.drawn_records(5, 40, B, W, H, cw, ch, 12)), what
        cr.expect_equal(dst, want, what)
        cr.expect_equal(dst, cr.crop(src, used, cw, ch, True)[0], what + " against the restatement")
        lv, wt = ofdg.host_flow_pyramid(want["flow"], L, want["occ0"], weights=True)
        fpr.expect_equal([t.cpu().numpy() for t in pyr[0]], lv, what + " pyramid")
        fpr.expect_equal([t.cpu().numpy() for t in pyr[1]], wt, what + " pyramid weights")
        fsr.expect_equal(ofdg.flow_stats_numpy(rows)["rows"], fsr.rows_of(ofdg.host_flow_stats(want["flow"], want["occ0"], 2.0)), what + " statistics")
        assert np.abs(want["flow"].astype(np.float32)).max() > 0 and want["occ0"].any() and want["label0"].any() and want["image1"].any()
        plain, _ = ofdg.host_crop({k: src[k] for k in ("occ0", "flow")}, ch, cw, recs=used)
        assert (want["occ0"] != 0).sum() >= (plain["occ0"] != 0).sum()


def test_end_to_end_mode_9(ofdg):
    import torch
    W, H, B, cw, ch = 128, 64, 3, 96, 48
    g = make_gen(ofdg, W, H, 9, pool=True, sampler=1, seed=3, batch_size=B)
    g.warp_generate(1, 3)
    outs = ofdg.alloc_outputs(B, H, W)
    src = dict(zip(("image0", "image1", "flow"), outs))
    dst = ofdg.alloc_crop(src, ch, cw)
    torch.cuda.synchronize()
    g.forward_counter(0, B, *outs, ofdg.STREAM_OWN)
    g.crop(src, dst, first_index=0, vflip=True, stream=ofdg.STREAM_OWN)
    g.synchronize(ofdg.STREAM_OWN)
    torch.cuda.synchronize()
    want, _ = ofdg.host_crop(to_host(src), ch, cw, first_index=0, seed=3, vflip=True)
    cr.expect_equal(to_host(dst), want)
    assert np.abs(want["flow"]).max() > 0


def test_three_calls_in_flight(ofdg):
    """Two calls on two caller streams and one on OFDG_STREAM_OWN, each into its own windows, one wait at the end."""
    import torch
    W, H, B, cw, ch = 128, 64, 2, 96, 48
    g = make_gen(ofdg, W, H, 7, pool=True)
    users = [torch.cuda.Stream(), torch.cuda.Stream()]
    batches = [g.sample(B) for _ in range(3)]
    outs = [ofdg.alloc_outputs(B, H, W) for _ in range(3)]
    srcs = [dict(zip(("image0", "image1", "flow"), o)) for o in outs]
    dsts = [ofdg.alloc_crop(s, ch, cw) for s in srcs]
    torch.cuda.synchronize()
    streams = [users[0].cuda_stream, users[1].cuda_stream, ofdg.STREAM_OWN]
    for k, ((tasks, bps, n), o, s, d, st) in enumerate(zip(batches, outs, srcs, dsts, streams)):
        g.render(tasks, B, bps, n, *o, st)
        g.crop(s, d, first_index=100 * k, seed=9, hflip=True, stream=st)
    for st in streams:
        g.synchronize(st)
    torch.cuda.synchronize()
    flows = [o[2].cpu().numpy() for o in outs]
    assert not np.array_equal(flows[0], flows[1]) and not np.array_equal(flows[1], flows[2])
    for k, (s, d) in enumerate(zip(srcs, dsts)):
        want, _ = ofdg.host_crop(to_host(s), ch, cw, first_index=100 * k, seed=9, hflip=True)
        cr.expect_equal(to_host(d), want, "call %d" % k)


def test_flowloader_crop(ofdg):
    import torch
    W, H, B, cw, ch = 128, 96, 2, 96, 48
    kw = dict(width=W, height=H, mode=7, batch_size=B, sampler=1, seed=21)
    pool = lambda g: g.pool_synthetic(3, 2 * W, 2 * H, 11)  # noqa: E731
    make = lambda **more: ofdg.FlowLoader(ofdg.default_params(**kw), pool=pool, prefetch=3, extras=("occ0",), **more)  # noqa: E731
    cropped = dict(crop=(ch, cw), crop_hflip=True, pyramid=3, stats=True)
    it, pit = iter(make(**cropped)), iter(make())
    third = None
    for step in range(3):
        i0, i1, fl, more = next(it)
        p = next(pit)
        torch.cuda.current_stream().synchronize()
        assert set(more) == {"occ0", "crop", "flow_stats", "flow_pyramid"} and len(more["flow_pyramid"]) == 3
        first = ofdg.shard_first_index(step, B, 1, 0)
        recs = np.array([ofdg.crop_draw(21, first + i, W, H, cw, ch, hflip=True) + (0,) for i in range(B)], np.int32)
        assert np.array_equal(more["crop"].cpu().numpy(), recs) and more["crop"].dtype == torch.int32
        src = to_host(dict(image0=p[0], image1=p[1], flow=p[2], occ0=p[3]["occ0"]))
        want, _ = ofdg.host_crop(src, ch, cw, recs=recs, occ_window=True)
        got = to_host(dict(image0=i0, image1=i1, flow=fl, occ0=more["occ0"]))
        cr.expect_equal(got, want, "batch %d" % step)
        fpr.expect_equal([t.cpu().numpy() for t in more["flow_pyramid"]], ofdg.host_flow_pyramid(want["flow"], 3, want["occ0"]))
        fsr.expect_equal(ofdg.flow_stats_numpy(more["flow_stats"])["rows"], fsr.flow_stats(want["flow"], want["occ0"], 2.0))
        third = got
    assert third["occ0"].any()
    resumed = iter(make(start=2, **cropped))
    i0, i1, fl, more = next(resumed)
    torch.cuda.current_stream().synchronize()
    cr.expect_equal(to_host(dict(image0=i0, image1=i1, flow=fl, occ0=more["occ0"])), third, "resumed at batch 2")
    assert np.array_equal(more["crop"].cpu().numpy(), recs)
    with pytest.raises(ValueError, match="objects"):
        ofdg.FlowLoader(ofdg.default_params(**kw), pool=pool, extras=("label0", "label1"), objects=True, crop=(ch, cw))


def test_refusals_enqueue_nothing(ofdg):
    import torch
    W, H, B, cw, ch = 128, 96, 2, 96, 48
    g = make_gen(ofdg, W, H, 7, pool=True, batch_size=B)
    outs = ofdg.alloc_outputs(B, H, W, image_dtype=torch.uint8, flow_dtype=torch.float16)
    ex = ofdg.alloc_extras(B, H, W, flow_dtype=torch.float16)
    src = dict(zip(("image0", "image1", "flow"), outs), **ex)
    bufs = guarded_like(src, ch, cw)
    recs = torch.zeros((B, 4), dtype=torch.int32, device="cuda")
    rraw, rout = guarded((B, 4), torch.int32)
    torch.cuda.synchronize()
    lib, vp = ofdg.lib(), C.c_void_p
    codes = dict(image_fmt=ofdg.FMT_U8, flow_fmt=ofdg.FMT_F16, occ_fmt=ofdg.FMT_F32)

    def job(planes=cr.PLANES, **kw):
        j = ofdg.CropJob()
        for k, name in enumerate(cr.PLANES):
            if name in planes:
                j.src[k], j.dst[k] = src[name].data_ptr(), bufs[name][1].data_ptr()
        j.recs, j.recs_out, j.crop_w, j.crop_h = recs.data_ptr(), rout.data_ptr(), cw, ch
        for k, v in dict(codes, **kw).items():
            if k in ("src", "dst"):
                for idx, val in v.items():
                    getattr(j, k)[idx] = val
            else:
                setattr(j, k, v)
        return j

    def refused(word, j, n=B, stream=0):
        rc = lib.ofdg_crop(g.h, None if j is None else C.byref(j), n, vp(stream))
        assert rc == ofdg.EINVAL, word
        msg = lib.ofdg_last_error(g.h).decode()
        assert msg.startswith("ofdg_crop") and word in msg, (word, msg)
        g.synchronize()
        torch.cuda.synchronize()
        assert all(bool((raw == FILL).all()) for raw, _ in list(bufs.values()) + [(rraw, rout)]), word

    refused("OFDG_STREAM_OWN", job(), stream=ofdg.STREAM_OWN)  # a fresh context: no call has worked on an internal stream yet
    refused("job", None)
    refused("n_samples", job(), n=0)
    for bad in (0, 4, 100, W + 8):
        refused("crop_w", job(crop_w=bad))
    for bad in (0, 47, H + 2):
        refused("crop_h", job(crop_h=bad))
    refused("flags", job(flags=32))
    refused("reserved", job(reserved=-1))
    refused("image_fmt", job(image_fmt=ofdg.FMT_F16))
    refused("flow_fmt", job(flow_fmt=ofdg.FMT_U8))
    refused("occ_fmt", job(occ_fmt=7))
    refused("no plane", job(planes=()))
    refused("dst", job(dst={3: None}))
    refused("src", job(src={7: None}))
    refused("occ0", job(planes=("occ0",), flags=cr.OCC_WINDOW))
    refused("occ1", job(planes=("occ1", "flow"), flags=cr.OCC_WINDOW))
    refused("4-byte", job(src={0: src["image0"].data_ptr() + 2}))
    refused("8-byte", job(src={2: src["flow"].data_ptr() + 4}))
    refused("16-byte", job(src={4: src["occ0"].data_ptr() + 8}))
    refused("16-byte", job(dst={6: bufs["label0"][1].data_ptr() + 8}))
    refused("recs must", job(recs=recs.data_ptr() + 8))
    refused("recs_out", job(recs_out=rout.data_ptr() + 4))
    refused("overlaps", job(dst={1: src["image1"].data_ptr()}))
    refused("overlaps", job(dst={5: bufs["occ0"][1].data_ptr() + 16}))
    refused("overlaps", job(recs_out=recs.data_ptr()))
    # the other entries' texts are what they were
    rows = ofdg.alloc_flow_stats(B)
    assert lib.ofdg_flow_stats(g.h, vp(src["flow"].data_ptr() + 4), ofdg.FMT_F16, None, 0, B, 2.0, 0, vp(rows.data_ptr()), None) == ofdg.EINVAL
    assert lib.ofdg_last_error(g.h).decode() == "ofdg_flow_stats: d_flow must be 8-byte aligned (binary16)"
    rec = ofdg.FlowPyramid()
    rec.levels, rec.out_fmt = 6, ofdg.FMT_F32
    for k in range(6):
        rec.flow[k] = src["occ0"].data_ptr()
    assert lib.ofdg_flow_pyramid(g.h, vp(src["flow"].data_ptr()), ofdg.FMT_F16, None, 0, B, 0, C.byref(rec), None) == ofdg.EINVAL
    assert lib.ofdg_last_error(g.h).decode() == "ofdg_flow_pyramid: pyr->levels: width and height must be multiples of 2^levels"
    # the sized entries name themselves and check the size they are given
    for bad_w, bad_h in ((100, 48), (96, 47), (0, 48)):
        assert lib.ofdg_flow_stats_sized(g.h, vp(src["flow"].data_ptr()), ofdg.FMT_F16, None, 0, B, bad_w, bad_h, 2.0, 0, vp(rows.data_ptr()), None) == ofdg.EINVAL
        assert lib.ofdg_last_error(g.h).decode().startswith("ofdg_flow_stats_sized: width")
        assert lib.ofdg_flow_pyramid_sized(g.h, vp(src["flow"].data_ptr()), ofdg.FMT_F16, None, 0, B, bad_w, bad_h, 0, C.byref(rec), None) == ofdg.EINVAL
        assert lib.ofdg_last_error(g.h).decode().startswith("ofdg_flow_pyramid_sized: width")
    assert lib.ofdg_flow_pyramid_sized(g.h, vp(src["flow"].data_ptr()), ofdg.FMT_F16, None, 0, B, cw, ch, 0, C.byref(rec), None) == ofdg.EINVAL
    assert lib.ofdg_last_error(g.h).decode() == "ofdg_flow_pyramid_sized: pyr->levels: width and height must be multiples of 2^levels"
    g.synchronize()
    torch.cuda.synchronize()
    assert all(bool((raw == FILL).all()) for raw, _ in list(bufs.values()) + [(rraw, rout)])
    # a valid call on the same context still works, also on OFDG_STREAM_OWN once a call has been made
    g.forward(*outs, ofdg.STREAM_OWN, extras=ex)
    dst = {k: t for k, (_, t) in bufs.items()}
    g.crop(src, dst, first_index=7, hflip=True, vflip=True, occ_window=True, recs_out=rout, stream=ofdg.STREAM_OWN)
    g.synchronize(ofdg.STREAM_OWN)
    torch.cuda.synchronize()
    want, used = ofdg.host_crop(to_host(src), ch, cw, first_index=7, seed=g.params.seed, hflip=True, vflip=True, occ_window=True)
    cr.expect_equal(to_host(dst), want)
    assert np.array_equal(rout.cpu().numpy(), used) and guards_intact(list(bufs.values()) + [(rraw, rout)])
