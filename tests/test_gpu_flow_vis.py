"""GPU tests of the flow visualisation (ofdg_flow_vis, include/ofdg.h): the device picture and rows against
ofdg_host_flow_vis and against the numpy restatement (tests/flow_vis_reference.py), byte for byte - both layouts and flow
formats, the three norms, with and without dimming, between guard bytes, twice, with a dirty workspace; the BATCH norm with
the maximum in the last sample; behind forward_counter and the crop without synchronisation, in mode 9, with three calls in
flight, through the loader - and the refusals."""
import ctypes as C

import numpy as np
import pytest

import flow_vis_reference as fv

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 64  # bytes in front of and behind every written plane (keeps the 16-byte alignment)
PLANES = ("image0", "image1", "flow")


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


def rows_of(ofdg, t):
    return ofdg.flow_vis_numpy(t)


# Both kernels take 4096 pixels of a plane per workgroup, a lane 4 pixels: 1024 a round of the 256 lanes.  8x2: 16 pixels, four
# lanes of one wave.  24x6 (144 pixels) and 72x40 (2880): one workgroup that ends inside a round of its lanes - the first, and
# the third.  264x200: 52800 pixels - thirteen workgroups, the last a partial one of 3648 pixels that again ends inside a
# round; the maximum then comes from thirteen atomics per sample.  So the sizes of the CPU tests are the ones the tiling asks
# for.
@pytest.mark.parametrize("W,H", fv.SIZES)
@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_device_equals_host_twin_and_restatement(ofdg, dtype, W, H):
    """The picture, the rows and the workspace lie between 0xA5 guards; the flow and the map stay as they are.  Each call runs
    twice on the same inputs, the second time with the workspace filled with 0xA5.  Four samples: every special value, all
    unusable (black), all zero (under SAMPLE no atomic is issued and the cleared slot gives the row {0, 1, 0}; white), and one
    large vector in a zero plane."""
    import torch
    g = make_gen(ofdg, 64, 32)  # (the context's own frame is another: the job gives the size)
    flow = fv.flows(W, H, dtype)
    fraw, dflow = guarded(flow)
    maps = {dim: (fv.occ_map(W, H, dim),) + guarded(fv.occ_map(W, H, dim)) for dim in ("uint8", "float32")}
    for norm, max_flow, layout, dim in fv.cases():
        occ, oraw, docc = maps[dim] if dim else (None, None, None)
        kw = dict(norm=norm, max_flow=max_flow, layout=layout, dim_occ=dim is not None)
        want = fv.flow_vis(flow, occ=occ, **kw)
        host = ofdg.host_flow_vis(flow, occ=occ, **kw)
        for dirty in (False, True):
            draw, dst = guarded(np.full(ofdg.flow_vis_shape(fv.N, H, W, layout), 0x5A, np.uint8))
            rraw, rout = guarded(np.full((fv.N, 4), -1, np.int32))
            wraw, work = guarded(np.full((fv.N, 8), FILL if dirty else 0, np.uint8))
            g.flow_vis(dflow, dst, occ=docc, rows_out=rout, work=None if norm == "fixed" else work, size=(H, W), **kw)
            torch.cuda.synchronize()
            tag = "%dx%d %s %s %s dim %s dirty %s" % (W, H, dtype, norm, layout, dim, dirty)
            assert guards_intact([(draw, dst), (rraw, rout), (wraw, work), (fraw, dflow)] + ([(oraw, docc)] if dim else [])), tag
            assert fv.equal_bits(dflow.cpu().numpy(), flow), tag + ": the flow"
            if dim:
                assert fv.equal_bits(docc.cpu().numpy(), occ), tag + ": the map"
            if norm == "fixed":
                assert bool((work == (FILL if dirty else 0)).all()), tag + ": FIXED looked at the workspace"
            got = dst.cpu().numpy()
            assert fv.equal_bits(got, want[0]), tag + ": picture against the restatement"
            assert fv.equal_bits(got, host[0]), tag + ": picture against ofdg_host_flow_vis"
            rows = rows_of(ofdg, rout)
            assert fv.equal_bits(rows, want[1]) and fv.equal_bits(rows, host[1]), "%s: rows\n%s\n%s" % (tag, rows, want[1])
            if norm == "sample":  # the all-zero sample: no atomic is issued, the cleared slot is read back, M = 1
                zero = rows[fv.ALL_ZERO]
                assert (int(zero["max_r2_q16"]), int(zero["scale_q8"]), int(zero["reserved"])) == (0, 1, 0), tag
            assert set(np.unique(got[fv.ALL_ZERO])) == ({255} if dim is None else {127, 255}), tag + ": the all-zero sample is white"
            assert not got[fv.ALL_UNUSABLE].any(), tag + ": the unusable sample is black"


@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_fixed_scale_at_both_ends(ofdg, dtype):
    """FIXED at max_flow = 2^-8 (M = 1: every non-zero vector is out of range, the radius' quotient far above its cap) and
    2^20 (M = 2^28: the quotient small, the largest usable value just inside): the device's float quotient and its correction
    step at both ends of M, on the flows that hold roots near 2^28.5, at a size with a partial lane round."""
    import torch
    W, H = 72, 40
    g = make_gen(ofdg, W, H)
    flow = fv.flows(W, H, dtype)
    dflow = torch.from_numpy(flow).cuda()
    for max_flow in fv.FIXED_ENDS:
        for layout in ("planar_bgr", "hwc_rgb"):
            want, wrows = fv.flow_vis(flow, norm="fixed", max_flow=max_flow, layout=layout)
            host, hrows = ofdg.host_flow_vis(flow, norm="fixed", max_flow=max_flow, layout=layout)
            dst, rout, _ = ofdg.alloc_flow_vis(fv.N, (H, W), layout, "fixed")
            g.flow_vis(dflow, dst, norm="fixed", max_flow=max_flow, layout=layout, rows_out=rout)
            torch.cuda.synchronize()
            tag = "%s %g %s" % (dtype, max_flow, layout)
            assert fv.equal_bits(dst.cpu().numpy(), want) and fv.equal_bits(host, want), tag
            assert fv.equal_bits(rows_of(ofdg, rout), wrows) and fv.equal_bits(hrows, wrows) and wrows["scale_q8"].tolist() == [int(max_flow * 256)] * fv.N, tag
            assert (want[fv.ALL_ZERO] == 255).all() and not want[fv.ALL_UNUSABLE].any() and len(np.unique(want[0])) > 2, tag


def test_batch_norm_with_the_maximum_in_the_last_sample(ofdg):
    """Five samples of small random flows, the call's largest vector in the last pixel of the last sample: every sample is
    scaled by it (slot 0 of the workspace serves all), and SAMPLE gives other pictures."""
    import torch
    W, H, n = 72, 40, 5
    g = make_gen(ofdg, W, H)
    rng = np.random.RandomState(5)
    flow = rng.uniform(-3.0, 3.0, (n, 2, H, W)).astype(np.float32)
    flow[n - 1, 0, -1, -1], flow[n - 1, 1, -1, -1] = 60.0, -80.0
    want, wrows = ofdg.host_flow_vis(flow, norm="batch")
    dst, rout, work = ofdg.alloc_flow_vis(n, (H, W), norm="batch")
    g.flow_vis(torch.from_numpy(flow).cuda(), dst, norm="batch", rows_out=rout, work=work)
    torch.cuda.synchronize()
    rows = rows_of(ofdg, rout)
    assert fv.equal_bits(dst.cpu().numpy(), want) and fv.equal_bits(rows, wrows) and fv.equal_bits(want, fv.flow_vis(flow, norm="batch")[0])
    assert rows["scale_q8"].tolist() == [25600] * n and rows["max_r2_q16"].tolist() == [25600 ** 2] * n
    own, orows = ofdg.host_flow_vis(flow, norm="sample")
    assert orows["scale_q8"][:n - 1].max() < 1100 and not fv.equal_bits(own[0], want[0]) and fv.equal_bits(own[n - 1], want[n - 1])


def rendered(ofdg, g, B, compact, first_index, then=None, extras=None):
    """forward_counter on the internal stream and `then(planes)` behind it, nothing waited for in between"""
    import torch
    W, H = g.params.width, g.params.height
    outs = ofdg.alloc_outputs(B, H, W, image_dtype=torch.uint8, flow_dtype=torch.float16) if compact else ofdg.alloc_outputs(B, H, W)
    src = dict(zip(PLANES, outs))
    more = then(src, False) if then else None
    torch.cuda.synchronize()  # (the allocations were made on torch's stream)
    g.forward_counter(first_index, B, *outs, ofdg.STREAM_OWN)
    if then:
        then(src, True, more)
    g.synchronize(ofdg.STREAM_OWN)
    torch.cuda.synchronize()
    return src, more


@pytest.mark.parametrize("compact", [False, True])
def test_behind_forward_counter_and_crop(ofdg, compact):
    """Mode 7 on OFDG_STREAM_OWN: forward_counter and the picture of its flow behind it; then forward_counter, the crop to 96x48
    and the picture of the cropped flow through size=."""
    W, H, B, cw, ch = 128, 64, 3, 96, 48
    g = make_gen(ofdg, W, H, 7, pool=True, sampler=1, seed=5, batch_size=B)

    def direct(src, enqueue, more=None):
        if not enqueue:
            return ofdg.alloc_flow_vis(B, (H, W), "hwc_rgb")
        g.flow_vis(src["flow"], more[0], layout="hwc_rgb", rows_out=more[1], work=more[2], stream=ofdg.STREAM_OWN)

    got, (dst, rout, _) = rendered(ofdg, g, B, compact, 40, direct)
    flow = got["flow"].cpu().numpy()
    want, rows = ofdg.host_flow_vis(flow, layout="hwc_rgb")
    assert fv.equal_bits(dst.cpu().numpy(), want) and fv.equal_bits(rows_of(ofdg, rout), rows)
    assert (rows["scale_q8"] > 1).all() and len(np.unique(want.reshape(-1, 3), axis=0)) > 10  # (a real picture: the samples move)

    def cropped(src, enqueue, more=None):
        if not enqueue:
            return ofdg.alloc_crop(src, ch, cw), ofdg.alloc_flow_vis(B, (ch, cw), norm="fixed")
        dst, (pic, rows, _) = more
        g.crop(src, dst, first_index=40, stream=ofdg.STREAM_OWN)
        g.flow_vis(dst["flow"], pic, norm="fixed", max_flow=12.0, rows_out=rows, stream=ofdg.STREAM_OWN, size=(ch, cw))

    _, (dst, (pic, rout, _)) = rendered(ofdg, g, B, compact, 40, cropped)
    want, rows = ofdg.host_flow_vis(dst["flow"].cpu().numpy(), norm="fixed", max_flow=12.0)
    assert fv.equal_bits(pic.cpu().numpy(), want) and fv.equal_bits(rows_of(ofdg, rout), rows) and rows["scale_q8"].tolist() == [3072] * B


def test_mode_9(ofdg):
    import torch
    W, H, B = 128, 64, 2
    g = make_gen(ofdg, W, H, 9, pool=True, sampler=1, seed=3, batch_size=B)
    g.warp_generate(1, 3)
    outs = ofdg.alloc_outputs(B, H, W)
    dst, rout, work = ofdg.alloc_flow_vis(B, (H, W))
    torch.cuda.synchronize()
    g.forward_counter(0, B, *outs, ofdg.STREAM_OWN)
    g.flow_vis(outs[2], dst, rows_out=rout, work=work, stream=ofdg.STREAM_OWN)
    g.synchronize(ofdg.STREAM_OWN)
    torch.cuda.synchronize()
    want, rows = ofdg.host_flow_vis(outs[2].cpu().numpy())
    assert fv.equal_bits(dst.cpu().numpy(), want) and fv.equal_bits(rows_of(ofdg, rout), rows) and (rows["scale_q8"] > 1).all()


def test_three_calls_in_flight(ofdg):
    """Two calls on two caller streams and one on OFDG_STREAM_OWN, each with its own picture, rows and workspace, one wait at
    the end."""
    import torch
    W, H, B = 128, 64, 2
    g = make_gen(ofdg, W, H, 7, pool=True)
    users = [torch.cuda.Stream(), torch.cuda.Stream()]
    batches = [g.sample(B) for _ in range(3)]
    sets = [(ofdg.alloc_outputs(B, H, W), ofdg.alloc_flow_vis(B, (H, W), norm="batch")) for _ in range(3)]
    torch.cuda.synchronize()
    streams = [users[0].cuda_stream, users[1].cuda_stream, ofdg.STREAM_OWN]
    for (tasks, bps, n), (o, (dst, rout, work)), st in zip(batches, sets, streams):
        g.render(tasks, B, bps, n, *o, st)
        g.flow_vis(o[2], dst, norm="batch", rows_out=rout, work=work, stream=st)
    for st in streams:
        g.synchronize(st)
    torch.cuda.synchronize()
    for k, (o, (dst, rout, work)) in enumerate(sets):
        want, rows = ofdg.host_flow_vis(o[2].cpu().numpy(), norm="batch")
        assert fv.equal_bits(dst.cpu().numpy(), want) and fv.equal_bits(rows_of(ofdg, rout), rows), "call %d" % k
    assert not fv.equal_bits(sets[0][1][0].cpu().numpy(), sets[1][1][0].cpu().numpy())


def test_flowloader_vis(ofdg):
    """FlowLoader(vis=...) against the host twin on the batch's own flow: behind the crop and the eraser (whose occ0 dims), in
    front of pack= (whose flow_scale the picture does not see); both flows; without vis= the loader yields what it yielded."""
    import torch
    import erase_reference as er
    W, H, B, cw, ch = 128, 96, 2, 96, 48
    kw = dict(width=W, height=H, mode=7, batch_size=B, sampler=1, seed=21)
    pool = lambda g: g.pool_synthetic(3, 2 * W, 2 * H, 11)  # noqa: E731
    extras = ("flow1", "occ0", "occ1")
    make = lambda **more: ofdg.FlowLoader(ofdg.default_params(**kw), pool=pool, prefetch=3, **more)  # noqa: E731
    erase = dict(er.RAFT, prob=1.0, min_size=8, max_size=30, frames=(0, 1))
    opts = dict(extras=extras, crop=(ch, cw), erase=erase)
    vis = dict(which=("flow", "flow1"), layout="hwc_rgb", dim_occ=True)
    full, plain = iter(make(vis=vis, pack=dict(flow_scale=0.05), **opts)), iter(make(**opts))
    for step in range(3):
        a, p = next(full), next(plain)
        torch.cuda.current_stream().synchronize()
        assert set(a[3]) == set(p[3]) | {"flow_vis", "flow_vis_rows", "flow1_vis", "flow1_vis_rows"}
        assert torch.equal(a[3]["occ0"], p[3]["occ0"]) and not torch.equal(a[2], p[2])  # (packed: rescaled)
        for name, occ in (("flow", "occ0"), ("flow1", "occ1")):
            flow = (p[2] if name == "flow" else p[3]["flow1"]).cpu().numpy()
            want, rows = ofdg.host_flow_vis(flow, occ=p[3][occ].cpu().numpy(), layout="hwc_rgb", dim_occ=True)
            assert a[3][name + "_vis"].dtype == torch.uint8 and tuple(a[3][name + "_vis"].shape) == (B, ch, cw, 3)
            assert fv.equal_bits(a[3][name + "_vis"].cpu().numpy(), want), "%s, batch %d" % (name, step)
            assert fv.equal_bits(rows_of(ofdg, a[3][name + "_vis_rows"]), rows)
            undimmed, _ = ofdg.host_flow_vis(flow, layout="hwc_rgb")
            assert not fv.equal_bits(undimmed, want)
    # compact formats, the frame's own size, a fixed scale, planar
    opts = dict(image_dtype=torch.uint8, flow_dtype=torch.float16)
    full, plain = iter(make(vis=dict(norm="fixed", max_flow=16.0), **opts)), iter(make(**opts))
    for step in range(2):
        a, p = next(full), next(plain)
        torch.cuda.current_stream().synchronize()
        assert len(p) == 3 and set(a[3]) == {"flow_vis", "flow_vis_rows"} and torch.equal(a[2], p[2]) and torch.equal(a[0], p[0])
        want, rows = ofdg.host_flow_vis(p[2].cpu().numpy(), norm="fixed", max_flow=16.0)
        assert fv.equal_bits(a[3]["flow_vis"].cpu().numpy(), want) and fv.equal_bits(rows_of(ofdg, a[3]["flow_vis_rows"]), rows)
    with pytest.raises(ValueError, match="extras= must contain \"flow1\""):
        make(vis=dict(which=("flow1",)))
    with pytest.raises(ValueError, match="unknown vis option"):
        make(vis=dict(arrows=True))


def test_refusals_enqueue_nothing(ofdg):
    import torch
    W, H, B = 128, 96, 2
    g = make_gen(ofdg, W, H, 7, pool=True, batch_size=B)
    fraw, flow = guarded(np.zeros((B, 2, H, W), np.float32))
    oraw, occ = guarded(np.zeros((B, 1, H, W), np.uint8))
    draw, dst = guarded(np.full((B, 3, H, W), FILL, np.uint8))
    wraw, work = guarded(np.full((B, 8), FILL, np.uint8))
    rraw, rout = guarded(np.full((B, 4), -1, np.int32))
    everything = [(fraw, flow), (oraw, occ), (draw, dst), (wraw, work), (rraw, rout)]
    before = [raw.clone() for raw, _ in everything]
    torch.cuda.synchronize()
    lib, vp = ofdg.lib(), C.c_void_p

    def job(**kw):
        j = ofdg.FlowVisJob()
        j.flow, j.occ, j.dst, j.rows_out, j.work = flow.data_ptr(), occ.data_ptr(), dst.data_ptr(), rout.data_ptr(), work.data_ptr()
        j.flow_fmt, j.occ_fmt, j.norm = ofdg.FMT_F32, ofdg.FMT_U8, ofdg.VIS_NORM_SAMPLE
        for k, v in kw.items():
            if isinstance(v, dict):
                for idx, val in v.items():
                    getattr(j, k)[idx] = val
            else:
                setattr(j, k, v)
        return j

    def refused(word, j, n=B, stream=0):
        rc = lib.ofdg_flow_vis(g.h, None if j is None else C.byref(j), n, vp(stream))
        assert rc == ofdg.EINVAL, word
        msg = lib.ofdg_last_error(g.h).decode()
        assert msg.startswith("ofdg_flow_vis: ") and word in msg, (word, msg)
        g.synchronize()
        torch.cuda.synchronize()
        assert all(torch.equal(raw, b) for (raw, _), b in zip(everything, before)), word

    refused("OFDG_STREAM_OWN", job(), stream=ofdg.STREAM_OWN)  # a fresh context: no call has worked on an internal stream yet
    refused("job", None)
    refused("flow is NULL", job(flow=None))
    refused("dst is NULL", job(dst=None))
    refused("n_samples", job(), n=0)
    for bad_w, bad_h in ((100, 48), (96, 47), (0, 48), (4, 2)):
        refused("width", job(width=bad_w, height=bad_h))
    refused("2^32", job(width=65536, height=32768), n=1)
    refused("flow_fmt", job(flow_fmt=ofdg.FMT_U8))
    refused("occ_fmt", job(occ_fmt=ofdg.FMT_F16))
    refused("layout", job(layout=2))
    refused("norm", job(norm=-1))
    refused("flags", job(flags=2))
    refused("reserved", job(reserved=1))
    refused("reserved2", job(reserved2={4: 1}))
    refused("OFDG_VIS_DIM_OCC needs occ", job(occ=None, flags=ofdg.VIS_DIM_OCC))
    refused("max_flow", job(norm=ofdg.VIS_NORM_FIXED, max_flow=float("nan")))
    refused("max_flow", job(norm=ofdg.VIS_NORM_FIXED, max_flow=0.001))
    refused("max_flow", job(norm=ofdg.VIS_NORM_FIXED, max_flow=2.0 ** 20 + 1))
    refused("work is NULL", job(work=None))
    refused("work is NULL", job(work=None, norm=ofdg.VIS_NORM_BATCH))
    refused("work must be 16-byte", job(work=work.data_ptr() + 8))
    refused("flow must be 16-byte aligned", job(flow=flow.data_ptr() + 8))
    refused("flow must be 8-byte aligned", job(flow=flow.data_ptr() + 4, flow_fmt=ofdg.FMT_F16))
    refused("occ must be 4-byte aligned", job(occ=occ.data_ptr() + 2))
    refused("occ must be 16-byte aligned", job(occ=flow.data_ptr() + 4, occ_fmt=ofdg.FMT_F32))  # (two read ranges may meet)
    refused("dst must be 16-byte aligned", job(dst=dst.data_ptr() + 4))
    refused("rows_out must be 16-byte", job(rows_out=rout.data_ptr() + 8))
    refused("overlaps", job(dst=flow.data_ptr() + 16))
    refused("overlaps", job(dst=occ.data_ptr()))
    refused("overlaps", job(work=rout.data_ptr()))
    refused("overlaps", job(rows_out=dst.data_ptr() + 64))
    refused("overlaps", job(work=flow.data_ptr() + 4 * 2 * B * H * W - 16))
    # a valid call on the same context still works, also on OFDG_STREAM_OWN once a call has been made
    outs = ofdg.alloc_outputs(B, H, W)
    torch.cuda.synchronize()
    g.forward(*outs, ofdg.STREAM_OWN)
    g.flow_vis(outs[2], dst, rows_out=rout, work=work, stream=ofdg.STREAM_OWN)
    g.synchronize(ofdg.STREAM_OWN)
    torch.cuda.synchronize()
    want, rows = ofdg.host_flow_vis(outs[2].cpu().numpy())
    assert fv.equal_bits(dst.cpu().numpy(), want) and fv.equal_bits(rows_of(ofdg, rout), rows) and guards_intact(everything)
