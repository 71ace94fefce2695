"""GPU tests of the motion boundaries (ofdg_boundaries, include/ofdg.h): the device planes against ofdg_host_boundaries and against
the numpy restatement (tests/boundaries_reference.py), byte for byte between guard bytes - the grid of the CPU tests, a plane
of 3 x 3 tiles with discs that cross tile corners, radii larger than the plane; behind forward_counter, the crop and the spatial
step without synchronisation; three calls in flight; through the loader - and the device's refusals."""
import ctypes as C

import numpy as np
import pytest

import boundaries_reference as br

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 64  # bytes in front of and behind every output (keeps the 16-byte alignment)
TILE_W, TILE_H = 128, 32  # kBndTileW, kBndTileH of csrc/kernels.hip


def make_gen(ofdg, W, H, mode=7, pool=False, **kw):
    g = ofdg.Generator(ofdg.default_params(width=W, height=H, mode=mode, **kw))
    if pool:
        g.pool_synthetic(3, 2 * W, 2 * H, 11)
    return g


def guarded(n, H, W):
    """(the whole uint8 buffer, filled with 0xA5; the [n,1,H,W] tensor in its middle)"""
    import torch
    raw = torch.full((GUARD + n * H * W + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    return raw, raw[GUARD:GUARD + n * H * W].view(n, 1, H, W)


def guards_intact(bufs):
    return all(bool((raw[:GUARD] == FILL).all()) and bool((raw[-GUARD:] == FILL).all()) for raw, _ in bufs.values())


def to_dev(planes):
    import torch
    return {k: torch.from_numpy(np.array(t)).cuda() for k, t in planes.items()}


def to_host(planes):
    return {k: t.cpu().numpy() for k, t in planes.items() if t is not None}


def run(g, dev, bufs, size, **kw):
    """Generator.boundaries of the device planes dev (flow, label, flow1, label1 as far as present) into bufs (edge0, dist0, edge1, dist1)"""
    t = {k: v[1] for k, v in bufs.items()}
    g.boundaries(dev.get("flow"), t.get("edge0"), t.get("dist0"), dev.get("label"), dev.get("flow1"), t.get("edge1"), t.get("dist1"),
                 dev.get("label1"), size=size, **kw)


def host_like(ofdg, host, names, **kw):
    """ofdg_host_boundaries of host planes for the outputs named (edge0, dist0, edge1, dist1)"""
    frames = [f for f in (0, 1) if "edge%d" % f in names or "dist%d" % f in names]
    out = ofdg.host_boundaries(host.get("flow") if 0 in frames else None, host.get("label") if 0 in frames else None,
                               host.get("flow1") if 1 in frames else None, host.get("label1") if 1 in frames else None, **kw)
    return {k: v for k, v in out.items() if k in names}


# A workgroup owns a 128 x 32 tile and reads a halo of `radius` around it.  8x2 and 24x6: one partial tile, the halo larger than
# the plane at radius 15.  72x40: one partial tile.  264x200: 3 x 7 tiles, the last partial on both axes.
@pytest.mark.parametrize("W,H", br.SIZES)
@pytest.mark.parametrize("labels", [True, False])
@pytest.mark.parametrize("fmt", [br.F32, br.F16])
def test_device_equals_host_twin_and_restatement(ofdg, fmt, labels, W, H):
    """The outputs start as 0xA5 bytes between 0xA5 guards: equality shows every byte was written, the guards that nothing
    else was.  The sources are unmodified afterwards."""
    import torch
    g = make_gen(ofdg, 64, 32)  # (the context's own frame is another: the job gives the size)
    src = br.inputs(W, H, fmt)
    dev = to_dev(src)
    for radius in br.RADII:
        for min_step in br.MIN_STEPS:
            bufs = {name: guarded(br.N, H, W) for name in ("edge0", "dist0", "edge1", "dist1")}
            run(g, dev, bufs, (H, W), radius=radius, min_step=min_step, labels=labels)
            torch.cuda.synchronize()
            what = "%dx%d fmt %d labels %d radius %d min_step %g" % (W, H, fmt, labels, radius, min_step)
            got = to_host({k: v[1] for k, v in bufs.items()})
            br.expect_equal(got, br.expected(W, H, fmt, labels, radius, min_step), what + " against the restatement")
            twin = ofdg.host_boundaries(src["flow"], src["label"], src["flow1"], src["label1"], radius=radius, min_step=min_step, labels=labels)
            br.expect_equal(got, twin, what + " against ofdg_host_boundaries")
            assert guards_intact(bufs), what
    assert all(dev[k].cpu().numpy().tobytes() == src[k].tobytes() for k in src), "the sources"


def test_discs_across_tile_corners(ofdg):
    """296 x 86 is 3 x 3 tiles of 128 x 32, the last partial on both axes; the tile in the middle is columns 128..255, rows
    32..63.  A spike at each of its four corner pixels, radius 15: each disc reaches the tile diagonally opposite, whose pixels
    are asserted here from the five edge pixels of the spike."""
    import torch
    W, H, R = 2 * TILE_W + 40, 2 * TILE_H + 22, 15
    corners = [(TILE_W, TILE_H), (2 * TILE_W - 1, TILE_H), (TILE_W, 2 * TILE_H - 1), (2 * TILE_W - 1, 2 * TILE_H - 1)]
    flow = np.zeros((1, 2, H, W), np.float32)
    for x, y in corners:
        flow[0, 1, y, x] = -4.0
    g = make_gen(ofdg, W, H)
    bufs = {name: guarded(1, H, W) for name in ("edge0", "dist0")}
    run(g, to_dev(dict(flow=flow)), bufs, None, radius=R)
    torch.cuda.synchronize()
    got = to_host({k: v[1] for k, v in bufs.items()})
    assert guards_intact(bufs)
    edge, dist = got["edge0"][0, 0], got["dist0"][0, 0]
    assert edge.sum() == 20
    for (x, y), (sx, sy) in zip(corners, ((-1, -1), (1, -1), (-1, 1), (1, 1))):
        plus = [(x, y), (x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1)]
        assert all(edge[py, px] == 1 for px, py in plus)
        seen = 0
        for a in range(1, R + 2):      # the pixel (x + sx * a, y + sy * b) lies in the diagonal neighbour tile
            for b in range(1, R + 2):
                px, py = x + sx * a, y + sy * b
                assert (px // TILE_W, py // TILE_H) == (1 + sx, 1 + sy)
                d2 = min((px - ex) ** 2 + (py - ey) ** 2 for ex, ey in plus)
                assert dist[py, px] == (d2 if d2 <= R * R else 255), (x, y, px, py)
                seen += d2 <= R * R
        assert seen > 60
    br.expect_equal(got, {"edge0": br.edge_of(flow, None, 0.0, False), "dist0": br.dist2_of(br.edge_of(flow, None, 0.0, False), R)}, "the whole plane")
    br.expect_equal(got, ofdg.host_boundaries(flow, radius=R), "the twin")


def test_subsets(ofdg):
    """edge only (no halo is read), dist2 only, frame 1 only"""
    import torch
    W, H = 264, 200
    g = make_gen(ofdg, W, H)
    src = br.inputs(W, H, br.F16)
    dev = to_dev(src)
    want = br.expected(W, H, br.F16, True, 15, 0.5)
    for names, planes in ((("edge0", "edge1"), dev), (("dist0", "dist1"), dev), (("edge1", "dist1"), {k: dev[k] for k in ("flow1", "label1")}),
                          (("dist0",), {k: dev[k] for k in ("flow", "label")})):
        bufs = {name: guarded(br.N, H, W) for name in names}
        run(g, planes, bufs, None, radius=15, min_step=0.5, labels=True)
        torch.cuda.synchronize()
        br.expect_equal(to_host({k: v[1] for k, v in bufs.items()}), {k: want[k] for k in names}, str(names))
        assert guards_intact(bufs)


def test_behind_forward_counter(ofdg):
    """forward_counter on the internal stream and the boundaries behind it, nothing waited for in between: mode 7 with all
    extras in float32 and in the compact formats, labels on; mode 9 (no labels), min_step alone."""
    import torch
    W, H, B = 128, 64, 3
    for mode, compact in ((7, False), (7, True), (9, False)):
        g = make_gen(ofdg, W, H, mode, pool=True, sampler=1, seed=5, batch_size=B)
        if mode == 9:
            g.warp_generate(1, 3)
        fmt = dict(image_dtype=torch.uint8, flow_dtype=torch.float16) if compact else {}
        outs = ofdg.alloc_outputs(B, H, W, **fmt)
        extras = None
        if mode == 7:
            extras = ofdg.alloc_extras(B, H, W, **(dict(flow_dtype=torch.float16, occ_dtype=torch.uint8) if compact else {}))
        bnd = ofdg.alloc_boundaries(B, H, W, frames=(0, 1) if mode == 7 else (0,))
        torch.cuda.synchronize()  # (the allocations were zeroed on torch's stream)
        g.forward_counter(40, B, *outs, ofdg.STREAM_OWN, extras=extras)
        if mode == 7:
            kw = dict(radius=10, min_step=0.0)
            g.boundaries(outs[2], bnd["edge0"], bnd["dist0"], extras["label0"], extras["flow1"], bnd["edge1"], bnd["dist1"], extras["label1"],
                         stream=ofdg.STREAM_OWN, **kw)
        else:
            kw = dict(radius=10, min_step=0.25, labels=False)
            g.boundaries(outs[2], bnd["edge0"], bnd["dist0"], stream=ofdg.STREAM_OWN, **kw)
        g.synchronize(ofdg.STREAM_OWN)
        torch.cuda.synchronize()
        host = to_host(dict(flow=outs[2]))
        if mode == 7:
            host = to_host(dict(flow=outs[2], label=extras["label0"], flow1=extras["flow1"], label1=extras["label1"]))
        got = to_host(bnd)
        assert got["edge0"].any() and not got["edge0"].all() and np.abs(host["flow"].astype(np.float32)).max() > 0
        br.expect_equal(got, host_like(ofdg, host, set(got), **kw), "mode %d compact %d" % (mode, compact))


@pytest.mark.parametrize("step", ["crop", "spatial"])
def test_behind_crop_and_spatial(ofdg, step):
    """128x64 -> 96x48 on OFDG_STREAM_OWN: forward_counter, the crop / the warp, the boundaries of the planes it wrote through
    the sized form - one wait at the end."""
    import torch
    W, H, B, cw, ch = 128, 64, 3, 96, 48
    g = make_gen(ofdg, W, H, 7, pool=True, sampler=1, seed=5, batch_size=B)
    outs = ofdg.alloc_outputs(B, H, W)
    extras = ofdg.alloc_extras(B, H, W)
    src = dict(zip(("image0", "image1", "flow"), outs), **extras)
    small = ofdg.alloc_crop(src, ch, cw) if step == "crop" else ofdg.alloc_spatial(src, ch, cw)
    bnd = ofdg.alloc_boundaries(B, ch, cw, frames=(0, 1))
    torch.cuda.synchronize()
    g.forward_counter(40, B, *outs, ofdg.STREAM_OWN, extras=extras)
    if step == "crop":
        g.crop(src, small, first_index=40, hflip=True, stream=ofdg.STREAM_OWN)
    else:
        g.spatial(src, small, first_index=40, ranges=ofdg.SPATIAL_FLOWNET, stream=ofdg.STREAM_OWN)
    kw = dict(radius=7, min_step=0.1)
    g.boundaries(small["flow"], bnd["edge0"], bnd["dist0"], small["label0"], small["flow1"], bnd["edge1"], bnd["dist1"], small["label1"],
                 stream=ofdg.STREAM_OWN, size=(ch, cw), **kw)
    g.synchronize(ofdg.STREAM_OWN)
    torch.cuda.synchronize()
    host = to_host(dict(flow=small["flow"], label=small["label0"], flow1=small["flow1"], label1=small["label1"]))
    got = to_host(bnd)
    assert got["edge0"].any() and got["edge1"].any()
    br.expect_equal(got, host_like(ofdg, host, set(got), **kw), "behind " + step)


def test_three_calls_in_flight(ofdg):
    """Two calls on two caller streams and one on OFDG_STREAM_OWN, each with its own radius, one wait at the end."""
    import torch
    W, H, B = 128, 64, 2
    g = make_gen(ofdg, W, H, 7, pool=True)
    users = [torch.cuda.Stream(), torch.cuda.Stream()]
    batches = [g.sample(B) for _ in range(3)]
    outs = [ofdg.alloc_outputs(B, H, W) for _ in range(3)]
    extras = [ofdg.alloc_extras(B, H, W, names=("label0",)) for _ in range(3)]
    bnds = [ofdg.alloc_boundaries(B, H, W) for _ in range(3)]
    kws = [dict(radius=3 + 6 * k, min_step=0.25 * k) for k in range(3)]
    torch.cuda.synchronize()
    streams = [users[0].cuda_stream, users[1].cuda_stream, ofdg.STREAM_OWN]
    for (tasks, bps, n), o, x, d, st, kw in zip(batches, outs, extras, bnds, streams, kws):
        g.render(tasks, B, bps, n, *o, st, extras=x)
        g.boundaries(o[2], d["edge0"], d["dist0"], x["label0"], stream=st, **kw)
    for st in streams:
        g.synchronize(st)
    torch.cuda.synchronize()
    for k, (o, x, d, kw) in enumerate(zip(outs, extras, bnds, kws)):
        host = to_host(dict(flow=o[2], label=x["label0"]))
        br.expect_equal(to_host(d), host_like(ofdg, host, set(d), **kw), "call %d" % k)
    assert not np.array_equal(outs[0][2].cpu().numpy(), outs[1][2].cpu().numpy())


def test_flowloader_boundaries(ofdg):
    import torch
    W, H, B, cw, ch = 128, 96, 2, 96, 48
    kw = dict(width=W, height=H, mode=7, batch_size=B, sampler=1, seed=21)
    names = ("flow1", "occ0", "label0", "label1")
    pool = lambda g: g.pool_synthetic(3, 2 * W, 2 * H, 11)  # noqa: E731
    make = lambda **more: ofdg.FlowLoader(ofdg.default_params(**kw), pool=pool, prefetch=3, extras=names, crop=(ch, cw), **more)  # noqa: E731
    opts = dict(radius=6, min_step=0.1, frames=(0, 1))
    it, pit = iter(make(boundaries=opts, stats=True, pyramid=2)), iter(make(stats=True, pyramid=2))
    last = None
    for step in range(3):
        a, p = next(it), next(pit)
        torch.cuda.current_stream().synchronize()
        assert set(a[3]) == set(p[3]) | {"edge0", "dist0", "edge1", "dist1"}
        assert all(tuple(a[3][k].shape) == (B, 1, ch, cw) and a[3][k].dtype == torch.uint8 for k in ("edge0", "dist0", "edge1", "dist1"))
        # what the loader yielded without boundaries= is what it yields with it ...
        assert all(torch.equal(x, y) for x, y in zip(a[:3], p[:3]))
        for k in p[3]:
            if k == "flow_pyramid":
                assert all(torch.equal(x, y) for x, y in zip(a[3][k], p[3][k]))
            else:
                assert torch.equal(a[3][k], p[3][k]), k
        # ... and the manual sequence on those planes gives the loader's boundary planes, as does the host twin
        manual = ofdg.alloc_boundaries(B, ch, cw, frames=(0, 1))
        torch.cuda.synchronize()
        it.gen.boundaries(p[2], manual["edge0"], manual["dist0"], p[3]["label0"], p[3]["flow1"], manual["edge1"], manual["dist1"], p[3]["label1"],
                          radius=6, min_step=0.1, size=(ch, cw))
        it.gen.synchronize()
        torch.cuda.synchronize()
        got = to_host({k: a[3][k] for k in manual})
        br.expect_equal(got, to_host(manual), "batch %d against the manual sequence" % step)
        host = to_host(dict(flow=p[2], label=p[3]["label0"], flow1=p[3]["flow1"], label1=p[3]["label1"]))
        br.expect_equal(got, host_like(ofdg, host, set(got), radius=6, min_step=0.1), "batch %d against host_boundaries" % step)
        assert got["edge0"].any()
        last = got
    resumed = next(iter(make(boundaries=opts, start=2)))
    torch.cuda.current_stream().synchronize()
    br.expect_equal(to_host({k: resumed[3][k] for k in last}), last, "resumed at batch 2")
    # without a crop, labels off, frame 0, the edge alone: the dict holds the extras and "edge0"
    plain = ofdg.FlowLoader(ofdg.default_params(**kw), pool=pool, boundaries=dict(labels=False, min_step=0.5, dist=False))
    a = next(iter(plain))
    torch.cuda.current_stream().synchronize()
    assert len(a) == 4 and set(a[3]) == {"edge0"}
    br.expect_equal(to_host(a[3]), host_like(ofdg, to_host(dict(flow=a[2])), {"edge0"}, min_step=0.5, labels=False), "uncropped")
    params = ofdg.default_params(**kw)
    with pytest.raises(ValueError, match="label"):
        ofdg.FlowLoader(params, pool=pool, extras=("flow1", "label0"), boundaries=dict(labels=True, frames=(0, 1)))
    with pytest.raises(ValueError, match="flow1"):
        ofdg.FlowLoader(params, pool=pool, extras=("label0", "label1"), boundaries=dict(frames=(0, 1)))
    with pytest.raises(ValueError, match="min_step"):
        ofdg.FlowLoader(params, pool=pool, extras=("label0",), boundaries=dict(labels=False))
    with pytest.raises(ValueError, match="min_step"):
        ofdg.FlowLoader(params, pool=pool, boundaries=dict(radius=4))  # no label plane among extras=: labels are off


def test_refusals_enqueue_nothing(ofdg):
    """What only the device entry refuses - misaligned planes of each kind, OFDG_STREAM_OWN before any call - and a sample of
    the shared rules through it: guards and outputs stay 0xA5, a valid call works afterwards."""
    import torch
    W, H, B = 128, 96, 2
    g = make_gen(ofdg, W, H, 7, pool=True, batch_size=B)
    outs = ofdg.alloc_outputs(B, H, W, flow_dtype=torch.float16)
    fouts = ofdg.alloc_outputs(B, H, W)
    extras = ofdg.alloc_extras(B, H, W, names=("label0",))
    bufs = {name: guarded(B, H, W) for name in ("edge0", "dist0")}
    torch.cuda.synchronize()
    lib, vp = ofdg.lib(), C.c_void_p

    def job(**kw):
        j = ofdg.BoundaryJob()
        j.flow[0], j.label[0] = outs[2].data_ptr(), extras["label0"].data_ptr()
        j.edge[0], j.dist2[0] = bufs["edge0"][1].data_ptr(), bufs["dist0"][1].data_ptr()
        j.flow_fmt, j.flags, j.radius, j.min_step = ofdg.FMT_F16, ofdg.BND_LABELS, 5, 0.0
        for k, v in kw.items():
            if isinstance(v, dict):
                for idx, val in v.items():
                    getattr(j, k)[idx] = val
            else:
                setattr(j, k, v)
        return j

    def refused(word, j, n=B, stream=0):
        rc = lib.ofdg_boundaries(g.h, None if j is None else C.byref(j), n, vp(stream))
        assert rc == ofdg.EINVAL, word
        msg = lib.ofdg_last_error(g.h).decode()
        assert msg.startswith("ofdg_boundaries: ") and word in msg, (word, msg)
        g.synchronize()
        torch.cuda.synchronize()
        assert all(bool((raw == FILL).all()) for raw, _ in bufs.values()), word

    refused("OFDG_STREAM_OWN", job(), stream=ofdg.STREAM_OWN)  # a fresh context: no call has worked on an internal stream yet
    refused("job", None)
    refused("n_samples", job(), n=0)
    refused("both be 0", job(height=H))
    for bad_w, bad_h in ((100, 48), (96, 47), (4, 2)):
        refused("width", job(width=bad_w, height=bad_h))
    refused("2^31", job(width=65536, height=32768), n=1)
    refused("flags", job(flags=3))
    refused("reserved", job(reserved={0: 7}))
    refused("flow_fmt", job(flow_fmt=ofdg.FMT_U8))
    refused("no frame", job(flow={0: None}, edge={0: None}, dist2={0: None}))
    refused("without its flow", job(edge={1: bufs["edge0"][1].data_ptr()}, dist2={0: None}))
    refused("no output", job(edge={0: None}, dist2={0: None}))
    refused("label", job(label={0: None}))
    refused("min_step", job(min_step=float("nan")))
    refused("min_step", job(min_step=-0.5))
    refused("radius", job(radius=16))
    refused("radius", job(radius=0))
    refused("flow[0] must be 8-byte aligned (binary16)", job(flow={0: outs[2].data_ptr() + 4}))
    refused("flow[0] must be 16-byte aligned (float32)", job(flow={0: fouts[2].data_ptr() + 8}, flow_fmt=ofdg.FMT_F32))
    refused("label[0] must be 4-byte", job(label={0: extras["label0"].data_ptr() + 2}))
    refused("edge[0] must be 16-byte", job(edge={0: bufs["edge0"][1].data_ptr() + 8}))
    refused("dist2[0] must be 16-byte", job(dist2={0: bufs["dist0"][1].data_ptr() + 8}))
    refused("overlaps", job(dist2={0: bufs["edge0"][1].data_ptr() + 16}))
    refused("overlaps", job(edge={0: outs[2].data_ptr()}))
    # a valid call on the same context still works, also on OFDG_STREAM_OWN once a call has been made
    g.forward(*outs, ofdg.STREAM_OWN, extras=extras)
    g.boundaries(outs[2], bufs["edge0"][1], bufs["dist0"][1], extras["label0"], radius=5, stream=ofdg.STREAM_OWN)
    g.synchronize(ofdg.STREAM_OWN)
    torch.cuda.synchronize()
    host = to_host(dict(flow=outs[2], label=extras["label0"]))
    br.expect_equal(to_host({k: v[1] for k, v in bufs.items()}), host_like(ofdg, host, {"edge0", "dist0"}, radius=5), "after the refusals")
    assert guards_intact(bufs)
