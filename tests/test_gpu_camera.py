"""GPU tests of the camera (ofdg_camera, include/ofdg.h): the device planes and records against ofdg_host_camera and against the
numpy restatement (tests/camera_reference.py), byte for byte - every format pair, one frame and both, between guard bytes,
twice; behind forward_counter and the crop without synchronisation, in mode 9, with three calls in flight, through the loader -
and the refusals."""
import ctypes as C

import numpy as np
import pytest

import camera_reference as cr

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


def to_host(planes):
    return tuple(None if t is None else t.cpu().numpy() for t in planes)


def dev_recs(recs):
    import torch
    return torch.from_numpy(np.ascontiguousarray(recs).view(np.int32).reshape(-1, 8)).cuda()


# The kernel's tile is 64 x 16 pixels, a workgroup of 256 lanes with four pixels of one row each; the blur stages the tile and a
# halo of R + 1 <= 13 rows and columns.  8x2: a plane smaller than the radius - one tile of two rows and two lanes a row, every
# tap beyond the first clamps, every mosaic neighbour of the first and last row and column reflects.  24x6: one partial tile.
# 72x40: 2 x 3 tiles, the second column of tiles 8 pixels wide (one pair of lanes a row), the last row of tiles 8 rows high; the
# halo of every tile reaches over an edge of the plane.  264x200: 5 x 13 tiles, inner ones whose halo lies in the plane on every
# side, a last column of 8 pixels and a last row of 8 rows.
@pytest.mark.parametrize("W,H", cr.SIZES)
@pytest.mark.parametrize("src_dtype,dst_dtype", [("float32", "float32"), ("uint8", "uint8"), ("float32", "uint8"), ("uint8", "float32")])
def test_device_equals_host_twin_and_restatement(ofdg, src_dtype, dst_dtype, W, H):
    """Every written plane lies between 0xA5 guards; the sources and the given records stay as they are.  The three sets of
    given records on both frames, the second on frame 0 and on frame 1 alone, then drawn ones.  Each call runs twice on the
    same buffers."""
    import torch
    g = make_gen(ofdg, 64, 32)  # (the context's own frame is another: the job gives the size)
    src = cr.frames(W, H, src_dtype)
    what = "%dx%d %s to %s" % (W, H, src_dtype, dst_dtype)
    sets = cr.record_sets()
    calls = [(dict(recs=sets[0]), (0, 1)), (dict(recs=sets[1]), (0, 1)), (dict(recs=sets[1]), (0,)), (dict(recs=sets[1]), (1,)), (dict(recs=sets[2]), (0, 1)),
             (dict(ranges=dict(cr.DEFAULT, sigma_max=4.0, sigma_delta=0.5), first_index=2 ** 32 - 1), (0, 1))]
    for kw, pick in calls:
        kw = dict(kw, seed=11)
        frames = tuple(t if f in pick else None for f, t in enumerate(src))
        want = cr.camera(frames, dst_dtype=np.dtype(dst_dtype), **kw)
        host = ofdg.host_camera(frames, dst_dtype=np.dtype(dst_dtype), **kw)
        sbufs = [None if t is None else guarded(t) for t in frames]
        dbufs = [None if t is None else guarded(np.full(t.shape, 77, dst_dtype)) for t in frames]
        rraw, rout = guarded(np.full((cr.N, 8), -1, np.int32))
        drecs = dev_recs(kw["recs"]) if "recs" in kw else None
        pair = lambda bufs: tuple(None if b is None else b[1] for b in bufs)  # noqa: E731
        for run in range(2):
            g.camera(pair(sbufs), pair(dbufs), recs_out=rout, size=(H, W), **dict(kw, recs=drecs))
            torch.cuda.synchronize()
            got = (to_host(pair(dbufs)), ofdg.camera_numpy(rout))
            tag = "%s frames %s run %d" % (what, pick, run)
            assert guards_intact([b for b in sbufs + dbufs if b is not None] + [(rraw, rout)]), tag
            if drecs is not None:
                assert cr.equal_bits(ofdg.camera_numpy(drecs), kw["recs"]), tag
            cr.expect_equal(to_host(pair(sbufs)), frames, tag + ": the sources")
            cr.expect_equal(got[0], want[0], tag + ": planes against the restatement")
            cr.expect_equal(got[0], host[0], tag + ": planes against ofdg_host_camera")
            assert cr.equal_bits(got[1], want[1]) and cr.equal_bits(got[1], host[1]), "%s: records\n%s\n%s" % (tag, got[1], want[1])


def rendered(ofdg, g, B, compact, first_index, then=None):
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


RANGES = dict(sigma_min=0.4, sigma_max=2.5, sigma_delta=0.3, blur_prob=0.8, bayer_prob=0.6, pattern=-1)


@pytest.mark.parametrize("compact", [False, True])
def test_behind_forward_counter_and_crop(ofdg, compact):
    """Mode 7 on OFDG_STREAM_OWN: forward_counter and the camera behind it into buffers of the other format; then
    forward_counter, the crop to 96x48 and the camera of the crop's planes through size=.  The flow is untouched."""
    import torch
    W, H, B, cw, ch = 128, 64, 3, 96, 48
    kw = dict(first_index=40, ranges=RANGES)
    g = make_gen(ofdg, W, H, 7, pool=True, sampler=1, seed=5, batch_size=B)
    plain, _ = rendered(ofdg, g, B, compact, 40)
    base = to_host((plain["image0"], plain["image1"]))
    other = torch.float32 if compact else torch.uint8
    other_np = np.uint8 if other == torch.uint8 else np.float32

    def behind(src, enqueue, more=None):
        if not enqueue:
            return ofdg.alloc_camera(B, H, W, other)
        g.camera((src["image0"], src["image1"]), more[0], recs_out=more[1], stream=ofdg.STREAM_OWN, **kw)

    got, (out, recs) = rendered(ofdg, g, B, compact, 40, behind)
    want, used = ofdg.host_camera(base, seed=5, dst_dtype=other_np, **kw)
    cr.expect_equal(to_host(out), want, "behind forward_counter")
    assert cr.equal_bits(ofdg.camera_numpy(recs), used) and used["sigma_q8"].any() and (used["bayer"] >= 0).any()
    cr.expect_equal(to_host((got["image0"], got["image1"])), base, "the sources")
    assert cr.equal_bits(got["flow"].cpu().numpy(), plain["flow"].cpu().numpy())

    def cropped(src, enqueue, more=None):
        if not enqueue:
            return ofdg.alloc_crop(src, ch, cw), ofdg.alloc_camera(B, ch, cw, other)
        dst, (out, recs) = more
        g.crop(src, dst, first_index=40, stream=ofdg.STREAM_OWN)
        g.camera((dst["image0"], dst["image1"]), out, recs_out=recs, stream=ofdg.STREAM_OWN, size=(ch, cw), **kw)

    _, (dst, (out, recs)) = rendered(ofdg, g, B, compact, 40, cropped)
    crop_host = to_host((dst["image0"], dst["image1"]))
    want, used = ofdg.host_camera(crop_host, seed=5, dst_dtype=other_np, **kw)
    cr.expect_equal(to_host(out), want, "behind the crop")
    assert cr.equal_bits(ofdg.camera_numpy(recs), used)


def test_mode_9(ofdg):
    import torch
    W, H, B = 128, 64, 2
    g = make_gen(ofdg, W, H, 9, pool=True, sampler=1, seed=3, batch_size=B)
    g.warp_generate(1, 3)
    kw = dict(first_index=0, ranges=dict(RANGES, blur_prob=1.0, bayer_prob=1.0))
    outs = ofdg.alloc_outputs(B, H, W)
    plain = ofdg.alloc_outputs(B, H, W)
    shot, recs = ofdg.alloc_camera(B, H, W)
    torch.cuda.synchronize()
    g.forward_counter(0, B, *plain, ofdg.STREAM_OWN)
    g.forward_counter(0, B, *outs, ofdg.STREAM_OWN)
    g.camera(outs[:2], shot, recs_out=recs, stream=ofdg.STREAM_OWN, **kw)
    g.synchronize(ofdg.STREAM_OWN)
    torch.cuda.synchronize()
    base = to_host(plain)
    want, used = ofdg.host_camera(base[:2], seed=3, **kw)
    cr.expect_equal(to_host(shot), want, "mode 9")
    cr.expect_equal(to_host(outs), base, "mode 9: the sources and the flow")
    assert cr.equal_bits(ofdg.camera_numpy(recs), used) and not cr.equal_bits(want[0], base[0])


def test_three_calls_in_flight(ofdg):
    """Two calls on two caller streams and one on OFDG_STREAM_OWN, each with its own frames and records, one wait at the end."""
    import torch
    W, H, B = 128, 64, 2
    g = make_gen(ofdg, W, H, 7, pool=True)
    users = [torch.cuda.Stream(), torch.cuda.Stream()]
    batches = [g.sample(B) for _ in range(3)]
    kw = lambda k: dict(first_index=100 * k, seed=9, ranges=dict(RANGES, blur_prob=1.0))  # noqa: E731
    plain = []
    for tasks, bps, n in batches:
        outs = ofdg.alloc_outputs(B, H, W)
        torch.cuda.synchronize()
        g.render(tasks, B, bps, n, *outs, 0)
        g.synchronize(0)
        torch.cuda.synchronize()
        plain.append(to_host(outs[:2]))
    sets = [(ofdg.alloc_outputs(B, H, W), ofdg.alloc_camera(B, H, W, torch.uint8)) for _ in range(3)]
    torch.cuda.synchronize()
    streams = [users[0].cuda_stream, users[1].cuda_stream, ofdg.STREAM_OWN]
    for k, ((tasks, bps, n), (o, (shot, recs)), st) in enumerate(zip(batches, sets, streams)):
        g.render(tasks, B, bps, n, *o, st)
        g.camera(o[:2], shot, recs_out=recs, stream=st, **kw(k))
    for st in streams:
        g.synchronize(st)
    torch.cuda.synchronize()
    for k, (o, (shot, recs)) in enumerate(sets):
        want, used = ofdg.host_camera(plain[k], dst_dtype=np.uint8, **kw(k))
        cr.expect_equal(to_host(shot), want, "call %d" % k)
        assert cr.equal_bits(ofdg.camera_numpy(recs), used)
    assert not cr.equal_bits(ofdg.camera_numpy(sets[0][1][1]), ofdg.camera_numpy(sets[1][1][1]))


def test_flowloader_camera(ofdg):
    """FlowLoader(camera=...) against the same chain made by hand from the loader without it: with motion_blur= in front (the
    blurred frames pass the camera), with photo=, jitter=, erase= and pack= behind (they work on the camera's frames), resumed
    with start=; bare; an unknown key."""
    import torch
    import erase_reference as er
    W, H, B, cw, ch = 128, 96, 2, 96, 48
    kw = dict(width=W, height=H, mode=7, batch_size=B, sampler=1, seed=21)
    pool = lambda g: g.pool_synthetic(3, 2 * W, 2 * H, 11)  # noqa: E731
    make = lambda **more: ofdg.FlowLoader(ofdg.default_params(**kw), pool=pool, prefetch=3, **more)  # noqa: E731
    camera = dict(RANGES, blur_prob=1.0)
    # 1. motion_blur= in front: the hand-made chain starts from the loader with motion_blur= alone
    opts = dict(extras=("flow1",), motion_blur=ofdg.MBLUR_DEFAULT, image_dtype=torch.uint8, flow_dtype=torch.float16, extras_compact=True)
    full, plain = iter(make(camera=camera, **opts)), iter(make(**opts))
    for step in range(3):
        a, p = next(full), next(plain)
        torch.cuda.current_stream().synchronize()
        assert set(a[3]) == set(p[3]) | {"camera"} and a[3]["camera"].dtype == torch.int32 and tuple(a[3]["camera"].shape) == (B, 8)
        index = ofdg.shard_first_index(step, B, 1, 0)
        want, used = ofdg.host_camera(to_host(p[:2]), first_index=index, seed=21, ranges=camera)
        cr.expect_equal(to_host(a[:2]), want, "behind motion_blur=, batch %d" % step)
        assert cr.equal_bits(ofdg.camera_numpy(a[3]["camera"]), used) and torch.equal(a[3]["motion_blur"], p[3]["motion_blur"]) and torch.equal(a[2], p[2])
        assert not cr.equal_bits(want[0], p[0].cpu().numpy())
    resumed = next(iter(make(camera=camera, start=2, **opts)))
    torch.cuda.current_stream().synchronize()
    assert torch.equal(resumed[3]["camera"], a[3]["camera"]) and torch.equal(resumed[0], a[0]) and torch.equal(resumed[1], a[1])
    # 2. crop in front; photo, jitter, erase and pack behind.  photo= draws noise per element from the frame it is given, so
    # the hand-made chain runs the host twins of all four on the camera's frames.
    extras = ("flow1", "occ0", "occ1")
    erase = dict(er.RAFT, prob=1.0, min_size=8, max_size=30, frames=(0, 1))
    ranges = {k: v for k, v in erase.items() if k in ofdg.ERASE_RANGES}
    pack = dict(image_dtype=torch.float16, concat=True)
    opts = dict(extras=extras, crop=(ch, cw))
    full, plain = iter(make(camera=camera, photo=ofdg.PHOTO_FLOWNET, jitter=ofdg.JITTER_RAFT, erase=erase, pack=pack, **opts)), iter(make(**opts))
    for step in range(2):
        a, p = next(full), next(plain)
        torch.cuda.current_stream().synchronize()
        assert set(a[3]) == set(p[3]) | {"camera", "photo", "jitter", "erase"}
        index = ofdg.shard_first_index(step, B, 1, 0)
        base = dict(zip(PLANES, to_host(p[:3])), **{k: p[3][k].cpu().numpy() for k in extras})
        shot, used = ofdg.host_camera((base["image0"], base["image1"]), first_index=index, seed=21, ranges=camera)
        assert cr.equal_bits(ofdg.camera_numpy(a[3]["camera"]), used)
        lit, ph_used = ofdg.host_photo(shot, first_index=index, seed=21, ranges=ofdg.PHOTO_FLOWNET)
        assert np.array_equal(a[3]["photo"].cpu().numpy(), ph_used)
        (j0, j1), j_used = ofdg.host_jitter(lit, first_index=index, seed=21, ranges=ofdg.JITTER_RAFT)
        assert cr.equal_bits(ofdg.jitter_numpy(a[3]["jitter"]), j_used)
        erased = [np.array(j0), np.array(j1)]
        occ = [np.array(base["occ0"]), np.array(base["occ1"])]
        e_used = ofdg.host_erase(erased, occ, (base["flow"], base["flow1"]), first_index=index, seed=21, ranges=ranges, frames=(0, 1))
        assert er.equal_bits(ofdg.erase_numpy(a[3]["erase"]), e_used)
        packed = ofdg.host_pack(dict(image0=erased[0], image1=erased[1], flow=base["flow"]), image_dtype=np.float16, concat=True)
        assert a[1] is None and cr.equal_bits(a[0].cpu().numpy(), packed["image0"]) and cr.equal_bits(a[2].cpu().numpy(), packed["flow"])
    # without camera= the loader yields what it yielded before; an unknown key raises
    bare = next(iter(make()))
    assert len(bare) == 3
    only = next(iter(make(camera=camera)))
    torch.cuda.current_stream().synchronize()
    assert set(only[3]) == {"camera"} and torch.equal(only[2], bare[2]) and not torch.equal(only[0], bare[0])
    want, _ = ofdg.host_camera(to_host(bare[:2]), first_index=0, seed=21, ranges=camera)
    cr.expect_equal(to_host(only[:2]), want, "camera= alone")
    with pytest.raises(ValueError, match="unknown range"):
        make(camera=dict(sigma=0.2))


def test_refusals_enqueue_nothing(ofdg):
    import torch
    W, H, B = 128, 96, 2
    g = make_gen(ofdg, W, H, 7, pool=True, batch_size=B)
    bufs = [guarded(np.zeros((B, 3, H, W), np.float32)) for _ in range(4)]   # src0, src1, dst0, dst1
    rraw, rout = guarded(np.full((B, 8), -1, np.int32))
    given = cr.record_sets()[1][1:3]
    recs = dev_recs(given)
    everything = bufs + [(rraw, rout)]
    before = [raw.clone() for raw, _ in everything]
    torch.cuda.synchronize()
    lib, vp = ofdg.lib(), C.c_void_p

    def job(**kw):
        j = ofdg.CameraJob()
        for f in range(2):
            j.src[f], j.dst[f] = bufs[f][1].data_ptr(), bufs[2 + f][1].data_ptr()
        j.recs, j.recs_out = recs.data_ptr(), rout.data_ptr()
        j.src_fmt, j.dst_fmt = ofdg.FMT_F32, ofdg.FMT_U8
        j.pattern = -1
        for k, v in kw.items():
            if isinstance(v, dict):
                for idx, val in v.items():
                    getattr(j, k)[idx] = val
            else:
                setattr(j, k, v)
        return j

    def refused(word, j, n=B, stream=0):
        rc = lib.ofdg_camera(g.h, None if j is None else C.byref(j), n, vp(stream))
        assert rc == ofdg.EINVAL, word
        msg = lib.ofdg_last_error(g.h).decode()
        assert msg.startswith("ofdg_camera: ") and word in msg, (word, msg)
        g.synchronize()
        torch.cuda.synchronize()
        assert all(torch.equal(raw, b) for (raw, _), b in zip(everything, before)), word

    refused("OFDG_STREAM_OWN", job(), stream=ofdg.STREAM_OWN)  # a fresh context: no call has worked on an internal stream yet
    refused("job", None)
    refused("n_samples", job(), n=0)
    for bad_w, bad_h in ((100, 48), (96, 47), (0, 48), (4, 2)):
        refused("width", job(width=bad_w, height=bad_h))
    refused("2^32", job(width=65536, height=32768), n=1)
    refused("src_fmt", job(src_fmt=ofdg.FMT_F16))
    refused("dst_fmt", job(dst_fmt=9))
    refused("flags", job(flags=1))
    refused("reserved", job(reserved=1))
    refused("sigma_max", job(recs=None, sigma_max=4.5))
    refused("sigma_delta", job(recs=None, sigma_delta=float("nan")))
    refused("sigma_min must not be above", job(sigma_min=1.0, sigma_max=0.5))
    refused("blur_prob", job(blur_prob=-0.5))
    refused("bayer_prob", job(bayer_prob=float("inf")))
    refused("pattern", job(pattern=4))
    refused("no frame is set", job(src={0: None, 1: None}, dst={0: None, 1: None}))
    refused("source and no destination", job(dst={0: None}))
    refused("destination and no source", job(src={1: None}))
    refused("src[image0] must be 16-byte aligned", job(src={0: bufs[0][1].data_ptr() + 4}))
    refused("src[image1] must be 4-byte aligned", job(src={1: bufs[1][1].data_ptr() + 2}, src_fmt=ofdg.FMT_U8))
    refused("dst[image1] must be 16-byte aligned", job(dst={1: bufs[3][1].data_ptr() + 4}))
    refused("recs must", job(recs=recs.data_ptr() + 8))
    refused("recs_out", job(recs_out=rout.data_ptr() + 4))
    refused("overlaps", job(dst={1: bufs[2][1].data_ptr() + 16}))
    refused("overlaps", job(dst={0: bufs[1][1].data_ptr()}))
    refused("overlaps", job(dst={0: bufs[0][1].data_ptr()}))                             # in place, in another format
    refused("overlaps", job(dst={0: bufs[0][1].data_ptr()}, dst_fmt=ofdg.FMT_F32))       # in place: there is no such form
    refused("overlaps", job(recs_out=recs.data_ptr()))
    refused("overlaps", job(recs_out=bufs[3][1].data_ptr() + 64))
    # a valid call on the same context still works, also on OFDG_STREAM_OWN once a call has been made
    outs = ofdg.alloc_outputs(B, H, W)
    shot, _ = ofdg.alloc_camera(B, H, W)
    torch.cuda.synchronize()
    g.forward(*outs, ofdg.STREAM_OWN)
    g.synchronize(ofdg.STREAM_OWN)
    torch.cuda.synchronize()
    base = to_host(outs[:2])
    g.camera(outs[:2], shot, recs=recs, recs_out=rout, stream=ofdg.STREAM_OWN)
    g.synchronize(ofdg.STREAM_OWN)
    torch.cuda.synchronize()
    want, used = ofdg.host_camera(base, recs=given)
    cr.expect_equal(to_host(shot), want, "after the refusals")
    assert cr.equal_bits(ofdg.camera_numpy(rout), used) and guards_intact(everything)
