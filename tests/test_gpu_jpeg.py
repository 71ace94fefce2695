"""GPU tests of the block compression (ofdg_jpeg, include/ofdg.h): the device planes and records against ofdg_host_jpeg and
against the numpy restatement (tests/jpeg_reference.py), byte for byte - every format pair, both subsamplings, the phases and
qualities of the CPU tests, between guard bytes; the in-place form; the drawn records; behind forward_counter without
synchronisation; through the loader - and the refusals."""
import ctypes as C

import numpy as np
import pytest

import jpeg_reference as jr

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 64  # bytes in front of and behind every written plane (keeps the 16-byte alignment)
PLANES = ("image0", "image1", "flow")
FORMATS = [("float32", "float32"), ("uint8", "uint8"), ("float32", "uint8"), ("uint8", "float32")]
RANGES = dict(prob=0.8, quality_min=5, quality_max=100, quality_delta=10, subsample=-1, sub_prob=0.5, phase=True)


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


def record_grid():
    """the (subsampling, phase, quality) grid of the CPU tests, three qualities a call - one per sample, rotated over the
    samples from phase to phase, so that every quality meets the structured samples and the one of plain noise"""
    for sub in (0, 1):
        for k, phase in enumerate(jr.PHASES):
            for qualities in ((1, 10, 50), (90, 100, (50, 0))):
                turn = (k + sub) % 3
                yield np.array([jr.rec_of(q, sub, phase) for q in qualities[turn:] + qualities[:turn]], jr.REC)


# The kernel's workgroup owns a 16x16 region of the block grid, a wave an 8x8 quadrant, and the grid of workgroups covers the
# largest phase.  8x2: a plane smaller than one block - every lane but 16 of a region clamps.  24x10: a partial bottom row of
# blocks.  40x26: two and a half regions across and one and five eighths down at phase 0, partial regions on every side at a
# phase.  72x34: several workgroups across and down.  136x18: 9 or 10 regions across, two rows of them.
@pytest.mark.parametrize("W,H", jr.GPU_SIZES)
@pytest.mark.parametrize("src_dtype,dst_dtype", FORMATS)
def test_device_equals_host_twin_and_restatement(ofdg, src_dtype, dst_dtype, W, H):
    """Every written plane lies between 0xA5 guards; the sources and the given records stay as they are.  The grid of given
    records on both frames, one set on frame 0 and on frame 1 alone, hostile records, then drawn ones."""
    import torch
    g = make_gen(ofdg, 64, 32)  # (the context's own frame is another: the job gives the size)
    src = jr.frames(W, H, src_dtype)
    what = "%dx%d %s to %s" % (W, H, src_dtype, dst_dtype)
    grid = list(record_grid())
    calls = [(dict(recs=r), (0, 1)) for r in grid] + [(dict(recs=grid[3]), (0,)), (dict(recs=grid[11]), (1,)), (dict(recs=jr.hostile_records()), (0, 1)),
                                                      (dict(ranges=RANGES, first_index=2 ** 32 - 1), (0, 1))]
    sbufs = [guarded(t) for t in src]
    dbufs = [guarded(np.full(t.shape, 77, dst_dtype)) for t in src]
    rraw, rout = guarded(np.full((jr.N, 8), -1, np.int32))
    for k, (kw, pick) in enumerate(calls):
        kw = dict(kw, seed=11)
        frames = tuple(t if f in pick else None for f, t in enumerate(src))
        want = jr.jpeg(frames, dst_dtype=np.dtype(dst_dtype), **kw)
        host = ofdg.host_jpeg(frames, dst_dtype=np.dtype(dst_dtype), **kw)
        drecs = dev_recs(kw["recs"]) if "recs" in kw else None
        pair = lambda bufs: tuple(b[1] if f in pick else None for f, b in enumerate(bufs))  # noqa: E731
        for _, t in dbufs:
            t.fill_(77)
        g.jpeg(pair(sbufs), pair(dbufs), recs_out=rout, size=(H, W), **dict(kw, recs=drecs))
        torch.cuda.synchronize()
        got = (to_host(pair(dbufs)), ofdg.jpeg_numpy(rout))
        tag = "%s call %d frames %s" % (what, k, pick)
        assert guards_intact(sbufs + dbufs + [(rraw, rout)]), tag
        if drecs is not None:
            assert jr.equal_bits(ofdg.jpeg_numpy(drecs), kw["recs"]), tag
        jr.expect_equal(to_host(pair(sbufs)), frames, tag + ": the sources")
        jr.expect_equal(got[0], want[0], tag + ": planes against the restatement")
        jr.expect_equal(got[0], host[0], tag + ": planes against ofdg_host_jpeg")
        assert jr.equal_bits(got[1], want[1]) and jr.equal_bits(got[1], host[1]), "%s: records\n%s\n%s" % (tag, got[1], want[1])
        for f in range(2):
            if f not in pick:
                assert bool((dbufs[f][1] == 77).all()), tag + ": a frame that is not set"


@pytest.mark.parametrize("W,H", jr.GPU_SIZES)
@pytest.mark.parametrize("dtype", ["float32", "uint8"])
def test_in_place_equals_copying(ofdg, dtype, W, H):
    """out=None: the frames themselves are written, between guards, and hold what the copying form gives; a frame of quality 0
    keeps its bits"""
    import torch
    g = make_gen(ofdg, 64, 32)
    src = jr.frames(W, H, dtype)
    for recs in list(record_grid()) + [None]:
        kw = dict(ranges=RANGES, seed=4, first_index=77) if recs is None else dict(recs=dev_recs(recs))
        sbufs = [guarded(t) for t in src]
        mine = [guarded(t) for t in src]
        out, rec_copy = ofdg.alloc_jpeg(jr.N, H, W, getattr(torch, dtype))
        _, rec_mine = ofdg.alloc_jpeg(jr.N)
        g.jpeg((sbufs[0][1], sbufs[1][1]), out, recs_out=rec_copy, size=(H, W), **kw)
        back = g.jpeg((mine[0][1], mine[1][1]), recs_out=rec_mine, size=(H, W), **kw)
        torch.cuda.synchronize()
        assert back[0] is mine[0][1] and back[1] is mine[1][1] and guards_intact(sbufs + mine)
        host = ofdg.host_jpeg(src, recs=recs) if recs is not None else ofdg.host_jpeg(src, **kw)
        jr.expect_equal(to_host(back), to_host(out), "%dx%d %s in place against copying" % (W, H, dtype))
        jr.expect_equal(to_host(back), host[0], "%dx%d %s in place against the twin" % (W, H, dtype))
        assert torch.equal(rec_copy, rec_mine) and jr.equal_bits(ofdg.jpeg_numpy(rec_mine), host[1])
        for i in range(jr.N):
            for f in range(2):
                if host[1][i]["quality"][f] == 0:
                    assert jr.equal_bits(back[f][i].cpu().numpy(), src[f][i])


def test_drawn_records(ofdg):
    """the records of a drawn call are jpeg_draw's, sanitised, at first_index (also beyond 2^32) under the seed given or the
    context's; the same records given reproduce the call"""
    import torch
    W, H, n = 24, 10, 64
    g = make_gen(ofdg, 64, 32, seed=9)
    rng = np.random.RandomState(2)
    src = (rng.randint(0, 256, (n, 3, H, W)).astype(np.uint8), rng.randint(0, 256, (n, 3, H, W)).astype(np.uint8))
    dev = tuple(torch.from_numpy(t).cuda() for t in src)
    seen = []
    for first, seed in ((0, None), (1000, 3), (2 ** 32 + 7, 3), (2 ** 40 - 5, 0xFFFFFFFF)):
        out, recs = ofdg.alloc_jpeg(n, H, W, torch.uint8)
        g.jpeg(dev, out, recs_out=recs, first_index=first, seed=seed, ranges=RANGES, size=(H, W))
        torch.cuda.synchronize()
        used = ofdg.jpeg_numpy(recs)
        s = 9 if seed is None else seed
        want = jr.sanitise(np.array([ofdg.jpeg_draw(s, first + i, RANGES) for i in range(n)]))
        assert jr.equal_bits(used, want) and jr.equal_bits(used, jr.sanitise(jr.drawn_records(s, first, n, RANGES))), (first, seed)
        assert used["quality"].any() and (used["quality"] == 0).any() and used["subsample"].any() and used["phase_x"].any()
        again, recs2 = ofdg.alloc_jpeg(n, H, W, torch.uint8)
        g.jpeg(dev, again, recs=recs, recs_out=recs2, size=(H, W))
        torch.cuda.synchronize()
        assert torch.equal(again[0], out[0]) and torch.equal(again[1], out[1]) and torch.equal(recs, recs2)
        host, _ = ofdg.host_jpeg(src, recs=used)
        jr.expect_equal(to_host(out), host, "drawn at %d" % first)
        seen.append(used.tobytes())
    assert len(set(seen)) == 4
    # without the flag the grid starts at (0, 0); prob 0 copies
    out, recs = ofdg.alloc_jpeg(n, H, W, torch.uint8)
    g.jpeg(dev, out, recs_out=recs, ranges=dict(RANGES, phase=False), size=(H, W))
    torch.cuda.synchronize()
    used = ofdg.jpeg_numpy(recs)
    assert not used["phase_x"].any() and not used["phase_y"].any() and used["quality"].any()
    g.jpeg(dev, out, recs_out=recs, ranges=dict(RANGES, prob=0.0), size=(H, W))
    torch.cuda.synchronize()
    assert not ofdg.jpeg_numpy(recs)["quality"].any() and torch.equal(out[0], dev[0]) and torch.equal(out[1], dev[1])


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


@pytest.mark.parametrize("compact", [False, True])
def test_behind_forward_counter(ofdg, compact):
    """a rendered 64x48 batch on OFDG_STREAM_OWN: forward_counter, the copying call into the other format and the in-place call
    behind it, no wait in between; the flow is untouched"""
    import torch
    W, H, B = 64, 48, 3
    kw = dict(first_index=40, ranges=dict(RANGES, prob=1.0))
    g = make_gen(ofdg, W, H, 7, pool=True, sampler=1, seed=5, batch_size=B)
    plain, _ = rendered(ofdg, g, B, compact, 40)
    base = to_host((plain["image0"], plain["image1"]))
    other = torch.float32 if compact else torch.uint8
    other_np = np.uint8 if other == torch.uint8 else np.float32

    def behind(src, enqueue, more=None):
        if not enqueue:
            return ofdg.alloc_jpeg(B, H, W, other)
        g.jpeg((src["image0"], src["image1"]), more[0], recs_out=more[1], stream=ofdg.STREAM_OWN, **kw)
        g.jpeg((src["image0"], src["image1"]), stream=ofdg.STREAM_OWN, **kw)

    got, (out, recs) = rendered(ofdg, g, B, compact, 40, behind)
    want, used = ofdg.host_jpeg(base, seed=5, dst_dtype=other_np, **kw)
    jr.expect_equal(to_host(out), want, "behind forward_counter")
    assert jr.equal_bits(ofdg.jpeg_numpy(recs), used) and used["quality"].all()
    same, _ = ofdg.host_jpeg(base, seed=5, **kw)
    jr.expect_equal(to_host((got["image0"], got["image1"])), same, "in place behind forward_counter")
    assert not jr.equal_bits(same[0], base[0]) and jr.equal_bits(got["flow"].cpu().numpy(), plain["flow"].cpu().numpy())


def test_flowloader_jpeg(ofdg):
    """FlowLoader(jpeg=...): alone; with photo=, jitter=, erase=, crop= and pack= against the host twins run in the documented
    order (photo, jitter, jpeg, erase, pack); jpeg=None is the loader without the option; prob 0 leaves the frames as they
    were; an unknown key raises."""
    import torch
    import erase_reference as er
    W, H, B, cw, ch = 128, 96, 2, 96, 48
    kw = dict(width=W, height=H, mode=7, batch_size=B, sampler=1, seed=21)
    pool = lambda g: g.pool_synthetic(3, 2 * W, 2 * H, 11)  # noqa: E731
    make = lambda **more: ofdg.FlowLoader(ofdg.default_params(**kw), pool=pool, prefetch=3, **more)  # noqa: E731
    jpeg = dict(RANGES, prob=1.0)
    # 1. alone, three batches, resumed with start=
    full, plain = iter(make(jpeg=jpeg)), iter(make())
    for step in range(3):
        a, p = next(full), next(plain)
        torch.cuda.current_stream().synchronize()
        assert len(p) == 3 and set(a[3]) == {"jpeg"} and a[3]["jpeg"].dtype == torch.int32 and tuple(a[3]["jpeg"].shape) == (B, 8)
        index = ofdg.shard_first_index(step, B, 1, 0)
        want, used = ofdg.host_jpeg(to_host(p[:2]), first_index=index, seed=21, ranges=jpeg)
        jr.expect_equal(to_host(a[:2]), want, "jpeg= alone, batch %d" % step)
        assert jr.equal_bits(ofdg.jpeg_numpy(a[3]["jpeg"]), used) and torch.equal(a[2], p[2]) and not jr.equal_bits(want[0], p[0].cpu().numpy())
    resumed = next(iter(make(jpeg=jpeg, start=2)))
    torch.cuda.current_stream().synchronize()
    assert torch.equal(resumed[3]["jpeg"], a[3]["jpeg"]) and torch.equal(resumed[0], a[0]) and torch.equal(resumed[1], a[1])
    # 2. crop in front; photo and jitter in front, erase and pack behind.  photo= draws noise per element from the frame it
    # is given, so the hand-made chain runs the host twins of all five on the plain loader's frames.
    extras = ("flow1", "occ0", "occ1")
    erase = dict(er.RAFT, prob=1.0, min_size=8, max_size=30, frames=(0, 1))
    ranges = {k: v for k, v in erase.items() if k in ofdg.ERASE_RANGES}
    pack = dict(image_dtype=torch.float16, concat=True)
    opts = dict(extras=extras, crop=(ch, cw))
    full, plain = iter(make(jpeg=jpeg, photo=ofdg.PHOTO_FLOWNET, jitter=ofdg.JITTER_RAFT, erase=erase, pack=pack, **opts)), iter(make(**opts))
    for step in range(2):
        a, p = next(full), next(plain)
        torch.cuda.current_stream().synchronize()
        assert set(a[3]) == set(p[3]) | {"jpeg", "photo", "jitter", "erase"}
        index = ofdg.shard_first_index(step, B, 1, 0)
        base = dict(zip(PLANES, to_host(p[:3])), **{k: p[3][k].cpu().numpy() for k in extras})
        lit, ph_used = ofdg.host_photo((base["image0"], base["image1"]), first_index=index, seed=21, ranges=ofdg.PHOTO_FLOWNET)
        assert np.array_equal(a[3]["photo"].cpu().numpy(), ph_used)
        jittered, j_used = ofdg.host_jitter(lit, first_index=index, seed=21, ranges=ofdg.JITTER_RAFT)
        assert jr.equal_bits(ofdg.jitter_numpy(a[3]["jitter"]), j_used)
        (c0, c1), used = ofdg.host_jpeg(jittered, first_index=index, seed=21, ranges=jpeg)
        assert jr.equal_bits(ofdg.jpeg_numpy(a[3]["jpeg"]), used) and not jr.equal_bits(c0, jittered[0])
        erased = [np.array(c0), np.array(c1)]
        occ = [np.array(base["occ0"]), np.array(base["occ1"])]
        e_used = ofdg.host_erase(erased, occ, (base["flow"], base["flow1"]), first_index=index, seed=21, ranges=ranges, frames=(0, 1))
        assert er.equal_bits(ofdg.erase_numpy(a[3]["erase"]), e_used)
        packed = ofdg.host_pack(dict(image0=erased[0], image1=erased[1], flow=base["flow"]), image_dtype=np.float16, concat=True)
        assert a[1] is None and jr.equal_bits(a[0].cpu().numpy(), packed["image0"]) and jr.equal_bits(a[2].cpu().numpy(), packed["flow"])
    # 3. jpeg=None is the loader as it is without the option; prob 0 hands out the uncompressed frames; an unknown key raises
    bare, none, off = next(iter(make())), next(iter(make(jpeg=None))), next(iter(make(jpeg=dict(jpeg, prob=0.0))))
    torch.cuda.current_stream().synchronize()
    assert len(bare) == 3 and len(none) == 3 and all(torch.equal(x, y) for x, y in zip(bare, none))
    assert set(off[3]) == {"jpeg"} and not ofdg.jpeg_numpy(off[3]["jpeg"])["quality"].any() and all(torch.equal(x, y) for x, y in zip(bare, off[:3]))
    with pytest.raises(ValueError, match="unknown range"):
        make(jpeg=dict(quality=50))


def test_refusals_enqueue_nothing(ofdg):
    import torch
    W, H, B = 128, 96, 2
    g = make_gen(ofdg, W, H, 7, pool=True, batch_size=B)
    bufs = [guarded(np.zeros((B, 3, H, W), np.float32)) for _ in range(4)]   # src0, src1, dst0, dst1
    rraw, rout = guarded(np.full((B, 8), -1, np.int32))
    given = np.array([jr.rec_of((40, 90), 1, (3, 5)), jr.rec_of((0, 15), 0, (15, 1))], jr.REC)
    recs = dev_recs(given)
    everything = bufs + [(rraw, rout)]
    before = [raw.clone() for raw, _ in everything]
    torch.cuda.synchronize()
    lib, vp = ofdg.lib(), C.c_void_p

    def job(**kw):
        j = ofdg.JpegJob()
        for f in range(2):
            j.src[f], j.dst[f] = bufs[f][1].data_ptr(), bufs[2 + f][1].data_ptr()
        j.recs, j.recs_out = recs.data_ptr(), rout.data_ptr()
        j.src_fmt, j.dst_fmt = ofdg.FMT_F32, ofdg.FMT_U8
        j.quality_min, j.quality_max, j.subsample = 30, 95, -1
        for k, v in kw.items():
            if isinstance(v, dict):
                for idx, val in v.items():
                    getattr(j, k)[idx] = val
            else:
                setattr(j, k, v)
        return j

    def refused(word, j, n=B, stream=0):
        rc = lib.ofdg_jpeg(g.h, None if j is None else C.byref(j), n, vp(stream))
        assert rc == ofdg.EINVAL, word
        msg = lib.ofdg_last_error(g.h).decode()
        assert msg.startswith("ofdg_jpeg: ") and word in msg, (word, msg)
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
    refused("flags", job(flags=2))
    refused("reserved", job(reserved={1: 1}))
    refused("quality_min", job(recs=None, quality_min=0))
    refused("quality_max", job(recs=None, quality_max=101))
    refused("quality_min must not be above", job(quality_min=96))
    refused("quality_delta", job(quality_delta=100))
    refused("prob", job(prob=-0.5))
    refused("sub_prob", job(sub_prob=float("nan")))
    refused("subsample", job(subsample=2))
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
    refused("overlaps", job(dst={0: bufs[0][1].data_ptr()}))                                          # in place, in another format
    refused("overlaps", job(dst={0: bufs[0][1].data_ptr() + 16}, dst_fmt=ofdg.FMT_F32))               # a partial overlap
    refused("overlaps", job(dst={0: bufs[0][1].data_ptr(), 1: bufs[0][1].data_ptr()}, dst_fmt=ofdg.FMT_F32))
    refused("overlaps", job(recs_out=recs.data_ptr()))
    refused("overlaps", job(recs_out=bufs[3][1].data_ptr() + 64))
    # a valid call on the same context still works, also on OFDG_STREAM_OWN once a call has been made: copying, then in place
    outs = ofdg.alloc_outputs(B, H, W)
    shot, _ = ofdg.alloc_jpeg(B, H, W)
    torch.cuda.synchronize()
    g.forward(*outs, ofdg.STREAM_OWN)
    g.synchronize(ofdg.STREAM_OWN)
    torch.cuda.synchronize()
    base = to_host(outs[:2])
    g.jpeg(outs[:2], shot, recs=recs, recs_out=rout, stream=ofdg.STREAM_OWN)
    g.jpeg(outs[:2], recs=recs, stream=ofdg.STREAM_OWN)
    g.synchronize(ofdg.STREAM_OWN)
    torch.cuda.synchronize()
    want, used = ofdg.host_jpeg(base, recs=given)
    jr.expect_equal(to_host(shot), want, "after the refusals")
    jr.expect_equal(to_host(outs[:2]), want, "after the refusals, in place")
    assert jr.equal_bits(ofdg.jpeg_numpy(rout), used) and guards_intact(everything)
