"""GPU tests of the photometric augmentation (ofdg_photo, include/ofdg.h): the device frames against ofdg_host_photo and against
the numpy restatement (tests/photo_reference.py), byte for byte - every format pair, records at and beyond every clamp edge,
between guard bytes; in place; one frame; the device's table; drawn records; behind a forward call and behind the crop without
synchronisation, with three calls in flight, through the loader - and the refusals."""
import ctypes as C

import numpy as np
import pytest

import photo_reference as pr

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 64  # bytes in front of and behind every destination (keeps the 16-byte alignment)


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


def guards_intact(bufs):
    return all(bool((raw[:GUARD] == FILL).all()) and bool((raw[-GUARD:] == FILL).all()) for raw, _ in bufs)


def to_dev(frames):
    import torch
    return tuple(None if t is None else torch.from_numpy(np.array(t)).cuda() for t in frames)


def to_host(frames):
    return tuple(None if t is None else t.cpu().numpy() for t in frames)


# A workgroup serves 32768 elements of one channel.  8x2: one piece of uint8 output, four of float32, in the only workgroup.
# 160x100: 16000 elements, one workgroup that ends inside a round of its lanes.  264x200: 52800 elements - a channel's second
# workgroup, which is also a partial last one (20032 elements) -, and uint8 rows 8 mod 16 wide, so that 16-element pieces straddle
# two rows.
@pytest.mark.parametrize("W,H", pr.SIZES)
@pytest.mark.parametrize("src_dtype,dst_dtype", pr.PAIRS)
def test_device_equals_host_twin_and_restatement(ofdg, W, H, src_dtype, dst_dtype):
    """The destinations start as 0xA5 bytes between 0xA5 guards: equality shows every element was written, the guards that
    nothing else was.  The records carry sigma 0 for some samples and frames and sigma > 0 for others."""
    import torch
    g = make_gen(ofdg, 64, 32)  # (the context's own frame is another: the job gives the size)
    src = pr.frames(W, H, src_dtype)
    recs = pr.records()
    assert (recs[:, pr.SIGMA] > 0).any() and (recs[:, pr.SIGMA] == 0).any()
    want, want_recs = pr.photo(src, recs, seed=7, dst_dtype=dst_dtype)
    host, host_recs = ofdg.host_photo(src, recs=recs, seed=7, dst_dtype=dst_dtype)
    dev = to_dev(src)
    drecs = torch.from_numpy(recs).cuda()
    bufs = [guarded(t.shape, getattr(torch, dst_dtype)) for t in dev]
    rraw, rout = guarded((pr.N, 16), torch.float32)
    g.photo(dev, tuple(t for _, t in bufs), recs=drecs, seed=7, recs_out=rout, size=(H, W))
    torch.cuda.synchronize()
    what = "%dx%d %s to %s" % (W, H, src_dtype, dst_dtype)
    got = to_host(tuple(t for _, t in bufs))
    pr.expect_equal(got, want, what + " against the restatement")
    pr.expect_equal(got, host, what + " against ofdg_host_photo")
    assert guards_intact(bufs + [(rraw, rout)]), what
    assert pr.equal_bits(rout.cpu().numpy(), want_recs) and pr.equal_bits(host_recs, want_recs), what
    pr.expect_equal(to_host(dev), src, what + ": the sources")
    assert pr.equal_bits(drecs.cpu().numpy(), recs)


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_in_place_and_one_frame(ofdg, dtype):
    import torch
    W, H = 264, 200
    g = make_gen(ofdg, W, H)
    src = pr.frames(W, H, dtype)
    recs = pr.records()
    want, _ = ofdg.host_photo(src, recs=recs, seed=3)
    drecs = torch.from_numpy(recs).cuda()
    bufs = [guarded(t.shape, getattr(torch, dtype)) for t in src]
    for (_, t), s in zip(bufs, src):
        t.copy_(torch.from_numpy(np.array(s)))
    work = tuple(t for _, t in bufs)
    out = g.photo(work, recs=drecs, seed=3)
    assert out[0] is work[0] and out[1] is work[1]
    torch.cuda.synchronize()
    pr.expect_equal(to_host(work), want, "in place")
    assert guards_intact(bufs)
    # frame 1 alone, into another format; frame 0's buffer stays as it is
    other = torch.float32 if dtype == "uint8" else torch.uint8
    raw1, out1 = guarded(src[1].shape, other)
    dev = to_dev(src)
    g.photo((None, dev[1]), (None, out1), recs=drecs, seed=3)
    torch.cuda.synchronize()
    only1, _ = ofdg.host_photo((None, src[1]), recs=recs, seed=3, dst_dtype=str(other).replace("torch.", ""))
    pr.expect_equal((None, out1.cpu().numpy()), only1, "frame 1 alone")
    assert guards_intact([(raw1, out1)])
    # the identity record leaves the frames as they are
    ident = torch.from_numpy(np.tile(pr.IDENTITY, (pr.N, 1))).cuda()
    bytes_ = to_dev(pr.frames(W, H, "uint8"))
    same = tuple(t.clone().to(getattr(torch, dtype)) for t in bytes_)
    g.photo(same, recs=ident)
    torch.cuda.synchronize()
    assert all(torch.equal(a.to(torch.uint8), b) for a, b in zip(same, bytes_))


def test_debug_photo_table(ofdg):
    g = make_gen(ofdg, 64, 32)
    recs = [pr.IDENTITY] + list(pr.records())
    for gamma in (0.125, 0.1250001, 0.5, 0.99999994, 1.0000001, 2.2, 7.999999, 8.0):
        r = pr.IDENTITY.copy()
        r[pr.GAMMA:pr.GAMMA + 2] = gamma, 1.0 / gamma
        r[pr.GAIN:pr.GAIN + 6] = 0.3, 1.0, 1.7, 8.0, 0.9, 1.1
        recs.append(r)
    for r in recs:
        dev, host = g.debug_photo_table(r), ofdg.host_photo_table(r)
        assert pr.equal_bits(dev, host), r
        assert pr.equal_bits(dev, pr.table(r)), r
    t = g.debug_photo_table(pr.IDENTITY)
    assert all(np.array_equal(t[f, c], np.arange(256, dtype=np.float32)) for f in range(2) for c in range(3))
    assert ofdg.lib().ofdg_debug_photo_table(g.h, None, None) == ofdg.EINVAL and "NULL" in ofdg.lib().ofdg_last_error(g.h).decode()


@pytest.mark.parametrize("first_index", [0, (1 << 32) + 3])
def test_drawn_records(ofdg, first_index):
    import torch
    W, H, n = 160, 100, 5
    g = make_gen(ofdg, W, H)
    src = pr.frames(W, H, "uint8", n=n)
    dev = to_dev(src)
    out = tuple(torch.zeros(t.shape, dtype=torch.float32, device="cuda") for t in dev)
    rout = torch.full((n, 16), -1.0, dtype=torch.float32, device="cuda")
    g.photo(dev, out, first_index=first_index, seed=12345, ranges=ofdg.PHOTO_FLOWNET, recs_out=rout)
    torch.cuda.synchronize()
    used = rout.cpu().numpy()
    for i in range(n):
        assert pr.equal_bits(used[i], ofdg.photo_draw(12345, first_index + i, ofdg.PHOTO_FLOWNET))  # (FLOWNET's draws need no clamp)
    assert pr.equal_bits(used, pr.sanitise(pr.drawn_records(12345, first_index, n, ofdg.PHOTO_FLOWNET)))
    host, host_recs = ofdg.host_photo(src, first_index=first_index, seed=12345, ranges=ofdg.PHOTO_FLOWNET, dst_dtype=np.float32)
    pr.expect_equal(to_host(out), host)
    pr.expect_equal(to_host(out), pr.photo(src, used, seed=12345, first_index=first_index, dst_dtype=np.float32)[0], "restatement")
    assert pr.equal_bits(host_recs, used) and len({r.tobytes() for r in used}) == n and (used[:, pr.SIGMA] > 0).all()


def test_behind_forward_counter_and_crop(ofdg):
    """forward_counter on the internal stream, the augmentation of the frames into other buffers behind it, the crop behind that
    and the augmentation of the cropped frames in place behind that: nothing is waited for in between."""
    import torch
    W, H, B, cw, ch = 128, 64, 3, 96, 48
    for image_dtype in (torch.float32, torch.uint8):
        g = make_gen(ofdg, W, H, 7, pool=True, sampler=1, seed=5, batch_size=B)
        outs = ofdg.alloc_outputs(B, H, W, image_dtype=image_dtype)
        aug = tuple(torch.zeros_like(t) for t in outs[:2])
        src = dict(zip(("image0", "image1", "flow"), outs))
        dst = ofdg.alloc_crop(src, ch, cw)
        recs = torch.zeros((B, 16), dtype=torch.float32, device="cuda")
        crecs = torch.zeros((B, 4), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()  # (the allocations were zeroed on torch's stream)
        g.forward_counter(40, B, *outs, ofdg.STREAM_OWN)
        g.photo(outs[:2], aug, first_index=40, ranges=ofdg.PHOTO_FLOWNET, recs_out=recs, stream=ofdg.STREAM_OWN)
        g.crop(src, dst, first_index=40, hflip=True, recs_out=crecs, stream=ofdg.STREAM_OWN)
        g.photo((dst["image0"], dst["image1"]), first_index=40, ranges=ofdg.PHOTO_FLOWNET, stream=ofdg.STREAM_OWN, size=(ch, cw))
        g.synchronize(ofdg.STREAM_OWN)
        torch.cuda.synchronize()
        frames = to_host(outs[:2])
        assert frames[0].any() and frames[1].any()
        want, used = ofdg.host_photo(frames, first_index=40, seed=5, ranges=ofdg.PHOTO_FLOWNET)
        pr.expect_equal(to_host(aug), want, "behind forward_counter %s" % image_dtype)
        assert pr.equal_bits(recs.cpu().numpy(), used)
        cropped, _ = ofdg.host_crop({"image0": frames[0], "image1": frames[1]}, ch, cw, recs=crecs.cpu().numpy())
        want_c, _ = ofdg.host_photo((cropped["image0"], cropped["image1"]), first_index=40, seed=5, ranges=ofdg.PHOTO_FLOWNET)
        pr.expect_equal(to_host((dst["image0"], dst["image1"])), want_c, "behind the crop %s" % image_dtype)
        assert not np.array_equal(want_c[0], cropped["image0"])
        if image_dtype == torch.float32:  # the generator's float32 frames hold byte values: both element types name the same index
            assert np.array_equal(frames[0], np.rint(frames[0])) and frames[0].min() >= 0 and frames[0].max() <= 255


def test_three_calls_in_flight(ofdg):
    """Two calls on two caller streams and one on OFDG_STREAM_OWN, each with its own records, one wait at the end."""
    import torch
    W, H, B = 128, 64, 2
    g = make_gen(ofdg, W, H, 7, pool=True)
    users = [torch.cuda.Stream(), torch.cuda.Stream()]
    batches = [g.sample(B) for _ in range(3)]
    outs = [ofdg.alloc_outputs(B, H, W) for _ in range(3)]
    augs = [tuple(torch.zeros((B, 3, H, W), dtype=torch.uint8, device="cuda") for _ in range(2)) for _ in range(3)]
    torch.cuda.synchronize()
    streams = [users[0].cuda_stream, users[1].cuda_stream, ofdg.STREAM_OWN]
    for k, ((tasks, bps, n), o, a, st) in enumerate(zip(batches, outs, augs, streams)):
        g.render(tasks, B, bps, n, *o, st)
        g.photo(o[:2], a, first_index=100 * k, seed=9, ranges=ofdg.PHOTO_FLOWNET, stream=st)
    for st in streams:
        g.synchronize(st)
    torch.cuda.synchronize()
    for k, (o, a) in enumerate(zip(outs, augs)):
        want, _ = ofdg.host_photo(to_host(o[:2]), first_index=100 * k, seed=9, ranges=ofdg.PHOTO_FLOWNET, dst_dtype=np.uint8)
        pr.expect_equal(to_host(a), want, "call %d" % k)
    assert not np.array_equal(augs[0][0].cpu().numpy(), augs[1][0].cpu().numpy())


def test_flowloader_photo(ofdg):
    import torch
    W, H, B, cw, ch = 128, 96, 2, 96, 48
    kw = dict(width=W, height=H, mode=7, batch_size=B, sampler=1, seed=21)
    pool = lambda g: g.pool_synthetic(3, 2 * W, 2 * H, 11)  # noqa: E731
    make = lambda **more: ofdg.FlowLoader(ofdg.default_params(**kw), pool=pool, prefetch=3, **more)  # noqa: E731
    cropped = dict(crop=(ch, cw), crop_hflip=True)
    first, second, plain = iter(make(photo=ofdg.PHOTO_FLOWNET, **cropped)), iter(make(photo=ofdg.PHOTO_FLOWNET, **cropped)), iter(make(**cropped))
    last = None
    for step in range(3):
        a, b, p = next(first), next(second), next(plain)
        torch.cuda.current_stream().synchronize()
        assert set(a[3]) == {"crop", "photo"} and a[3]["photo"].dtype == torch.float32 and tuple(a[3]["photo"].shape) == (B, 16)
        for x, y in zip(a[:3] + (a[3]["crop"], a[3]["photo"]), b[:3] + (b[3]["crop"], b[3]["photo"])):
            assert torch.equal(x, y), step
        assert torch.equal(a[2], p[2]) and torch.equal(a[3]["crop"], p[3]["crop"])
        index = ofdg.shard_first_index(step, B, 1, 0)
        want, used = ofdg.host_photo(to_host(p[:2]), first_index=index, seed=21, ranges=ofdg.PHOTO_FLOWNET)
        pr.expect_equal(to_host(a[:2]), want, "batch %d" % step)
        assert pr.equal_bits(a[3]["photo"].cpu().numpy(), used) and not torch.equal(a[0], p[0])
        last = to_host(a[:2])
    resumed = next(iter(make(photo=ofdg.PHOTO_FLOWNET, start=2, **cropped)))
    torch.cuda.current_stream().synchronize()
    pr.expect_equal(to_host(resumed[:2]), last, "resumed at batch 2")
    # without a crop, on compact frames: the whole frame, in place in the ring
    it, pit = iter(make(photo=ofdg.PHOTO_FLOWNET, image_dtype=torch.uint8)), iter(make(image_dtype=torch.uint8))
    a, p = next(it), next(pit)
    torch.cuda.current_stream().synchronize()
    assert set(a[3]) == {"photo"} and a[0].dtype == torch.uint8
    pr.expect_equal(to_host(a[:2]), ofdg.host_photo(to_host(p[:2]), first_index=0, seed=21, ranges=ofdg.PHOTO_FLOWNET)[0], "uncropped uint8")
    with pytest.raises(ValueError, match="unknown range"):
        make(photo={"noise": 1.0})


def test_refusals_enqueue_nothing(ofdg):
    import torch
    W, H, B = 128, 96, 2
    g = make_gen(ofdg, W, H, 7, pool=True, batch_size=B)
    outs = ofdg.alloc_outputs(B, H, W, image_dtype=torch.uint8)
    bufs = [guarded((B, 3, H, W), torch.float32) for _ in range(2)]
    recs = torch.from_numpy(np.tile(pr.IDENTITY, (B, 1))).cuda()
    rraw, rout = guarded((B, 16), torch.float32)
    torch.cuda.synchronize()
    lib, vp = ofdg.lib(), C.c_void_p

    def job(**kw):
        j = ofdg.PhotoJob()
        for f in range(2):
            j.src[f], j.dst[f] = outs[f].data_ptr(), bufs[f][1].data_ptr()
        j.recs, j.recs_out, j.src_fmt, j.dst_fmt = recs.data_ptr(), rout.data_ptr(), ofdg.FMT_U8, ofdg.FMT_F32
        for k, v in kw.items():
            if k in ("src", "dst"):
                for idx, val in v.items():
                    getattr(j, k)[idx] = val
            else:
                setattr(j, k, v)
        return j

    def refused(word, j, n=B, stream=0):
        rc = lib.ofdg_photo(g.h, None if j is None else C.byref(j), n, vp(stream))
        assert rc == ofdg.EINVAL, word
        msg = lib.ofdg_last_error(g.h).decode()
        assert msg.startswith("ofdg_photo: ") and word in msg, (word, msg)
        g.synchronize()
        torch.cuda.synchronize()
        assert all(bool((raw == FILL).all()) for raw, _ in bufs + [(rraw, rout)]), word

    refused("OFDG_STREAM_OWN", job(), stream=ofdg.STREAM_OWN)  # a fresh context: no call has worked on an internal stream yet
    refused("job", None)
    refused("n_samples", job(), n=0)
    refused("no frame", job(src={0: None, 1: None}, dst={0: None, 1: None}))
    refused("dst", job(dst={1: None}))
    refused("src", job(src={0: None}))
    refused("src_fmt", job(src_fmt=ofdg.FMT_F16))
    refused("dst_fmt", job(dst_fmt=9))
    refused("flags", job(flags=4))
    refused("reserved", job(reserved=1))
    for name in ofdg.PHOTO_RANGES:
        for bad in (-1.0, float("nan"), float("inf")):
            refused(name, job(**{name: bad}))
    for bad_w, bad_h in ((100, 48), (96, 47), (0, 48), (96, 0), (4, 2)):
        refused("width", job(width=bad_w, height=bad_h))
    refused("2^32", job(width=65536, height=21846), n=1)
    refused("4-byte", job(src={0: outs[0].data_ptr() + 2}))
    refused("16-byte", job(src={0: None, 1: bufs[1][1].data_ptr() + 8}, dst={0: None, 1: outs[1].data_ptr()}, src_fmt=ofdg.FMT_F32, dst_fmt=ofdg.FMT_U8))
    refused("16-byte", job(dst={0: bufs[0][1].data_ptr() + 8}))
    refused("recs must", job(recs=recs.data_ptr() + 8))
    refused("recs_out", job(recs_out=rout.data_ptr() + 4))
    refused("overlaps", job(dst={1: bufs[0][1].data_ptr() + 16}))
    refused("overlaps", job(dst={0: outs[0].data_ptr()}))                   # the same address in another format
    refused("overlaps", job(dst={0: outs[1].data_ptr()}, dst_fmt=ofdg.FMT_U8))  # the other frame's source
    refused("overlaps", job(dst={0: outs[0].data_ptr() + 16}, dst_fmt=ofdg.FMT_U8))
    refused("overlaps", job(recs_out=recs.data_ptr()))
    # a valid call on the same context still works, also on OFDG_STREAM_OWN once a call has been made
    g.forward(*outs, ofdg.STREAM_OWN)
    g.photo(outs[:2], tuple(t for _, t in bufs), first_index=7, ranges=ofdg.PHOTO_FLOWNET, recs_out=rout, stream=ofdg.STREAM_OWN)
    g.synchronize(ofdg.STREAM_OWN)
    torch.cuda.synchronize()
    want, used = ofdg.host_photo(to_host(outs[:2]), first_index=7, seed=g.params.seed, ranges=ofdg.PHOTO_FLOWNET, dst_dtype=np.float32)
    pr.expect_equal(to_host(tuple(t for _, t in bufs)), want)
    assert pr.equal_bits(rout.cpu().numpy(), used) and guards_intact(bufs + [(rraw, rout)])
