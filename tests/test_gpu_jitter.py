"""GPU tests of the colour jitter (ofdg_jitter, include/ofdg.h): the device planes and records against ofdg_host_jitter and
against the numpy restatement (tests/jitter_reference.py), byte for byte - every format pair, copying and in place, one frame
and both, between guard bytes, twice, with a dirty workspace; the whole colour cube; behind forward_counter and the crop
without synchronisation, in mode 9, with three calls in flight, through the loader - and the refusals."""
import ctypes as C

import numpy as np
import pytest

import jitter_reference as jr

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


def to_dev(planes):
    import torch
    return tuple(None if t is None else torch.from_numpy(np.array(t)).cuda() for t in planes)


def to_host(planes):
    return tuple(None if t is None else t.cpu().numpy() for t in planes)


def dev_recs(recs):
    import torch
    return torch.from_numpy(np.ascontiguousarray(recs).view(np.int32).reshape(-1, 16)).cuda()


# Both kernels take 8192 pixels of a frame per workgroup, a lane 16 pixels of a uint8 piece (4096 a round of the 256 lanes) or 4
# of a float32 one (1024 a round).  8x2: one piece.  24x6 (144 pixels), 72x40 (2880): one workgroup that ends inside a round of
# its lanes - the first, and the third of the float32 pieces.  264x200: 52800 pixels - seven workgroups, the last a partial one
# of 3648 pixels that again ends inside a round; the reduction then adds seven partial sums per frame.
@pytest.mark.parametrize("W,H", jr.SIZES)
@pytest.mark.parametrize("src_dtype,dst_dtype", [("float32", "float32"), ("uint8", "uint8"), ("float32", "uint8"), ("uint8", "float32")])
def test_device_equals_host_twin_and_restatement(ofdg, src_dtype, dst_dtype, W, H):
    """Every written plane lies between 0xA5 guards; the sources of a copying call and the given records stay as they are.  Given
    records on both frames, on frame 0 and on frame 1 alone, then drawn ones; copying and - where the formats agree - in place.
    Each call runs twice on the same inputs, the second time with the workspace filled with 0xA5."""
    import torch
    g = make_gen(ofdg, 64, 32)  # (the context's own frame is another: the job gives the size)
    src = jr.frames(W, H, src_dtype)
    what = "%dx%d %s to %s" % (W, H, src_dtype, dst_dtype)
    calls = [(dict(recs=jr.records()), (0, 1)), (dict(recs=jr.records()), (0,)), (dict(recs=jr.records()), (1,)),
             (dict(ranges=dict(jr.RAFT, asym_prob=0.5), first_index=2 ** 32 - 1), (0, 1))]
    for kw, pick in calls:
        kw = dict(kw, seed=11)
        frames = tuple(t if f in pick else None for f, t in enumerate(src))
        want = jr.jitter(frames, dst_dtype=np.dtype(dst_dtype), **kw)
        host = ofdg.host_jitter(frames, dst_dtype=np.dtype(dst_dtype), **kw)
        for in_place in ((False, True) if src_dtype == dst_dtype else (False,)):
            for dirty in (False, True):
                sbufs = [None if t is None else guarded(t) for t in frames]
                dbufs = sbufs if in_place else [None if t is None else guarded(np.full(t.shape, 0, dst_dtype)) for t in frames]
                wraw, work = guarded(np.full((jr.N, 16), FILL if dirty else 0, np.uint8))
                rraw, rout = guarded(np.full((jr.N, 16), -1, np.int32))
                drecs = dev_recs(kw["recs"]) if "recs" in kw else None
                pair = lambda bufs: tuple(None if b is None else b[1] for b in bufs)  # noqa: E731
                g.jitter(pair(sbufs), None if in_place else pair(dbufs), recs_out=rout, work=work, size=(H, W), **dict(kw, recs=drecs))
                torch.cuda.synchronize()
                got = (to_host(pair(dbufs)), ofdg.jitter_numpy(rout))
                tag = "%s frames %s in place %s dirty %s" % (what, pick, in_place, dirty)
                assert guards_intact([b for b in sbufs + dbufs if b is not None] + [(wraw, work), (rraw, rout)]), tag
                if drecs is not None:
                    assert jr.equal_bits(ofdg.jitter_numpy(drecs), kw["recs"]), tag
                if not in_place:
                    jr.expect_equal(to_host(pair(sbufs)), frames, tag + ": the sources")
                jr.expect_equal(got[0], want[0], tag + ": planes against the restatement")
                jr.expect_equal(got[0], host[0], tag + ": planes against ofdg_host_jitter")
                assert jr.equal_bits(got[1], want[1]) and jr.equal_bits(got[1], host[1]), "%s: records\n%s\n%s" % (tag, got[1], want[1])


def test_no_workspace_without_a_contrast(ofdg):
    """Drawn records under ranges without a contrast need no workspace (one launch); with a contrast, and with given records,
    the call without one is refused."""
    import torch
    W, H = 72, 40
    g = make_gen(ofdg, W, H)
    src = jr.frames(W, H, "uint8")
    ranges = dict(jr.RAFT, contrast=0.0)
    (h0, h1), used = ofdg.host_jitter(src, ranges=ranges, seed=4, first_index=77)
    d = to_dev(src)
    _, rout = ofdg.alloc_jitter(jr.N)
    g.jitter(d, recs_out=rout, ranges=ranges, seed=4, first_index=77)
    torch.cuda.synchronize()
    jr.expect_equal(to_host(d), (h0, h1), "no contrast")
    assert jr.equal_bits(ofdg.jitter_numpy(rout), used) and (used["contrast"] == jr.ONE).all() and (used["mean"] == -1).all()
    for kw in (dict(ranges=jr.RAFT), dict(recs=dev_recs(jr.records()))):
        with pytest.raises(ofdg.OfdgError, match="work is NULL"):
            g.jitter(d, **kw)


CUBE_CASES = {"hue -196608": dict(hue=-196608), "hue 21845": dict(hue=21845), "hue 131072": dict(hue=131072),
              "all four, order 5": dict(brightness=75000, contrast=110000, saturation=20000, hue=40000, order=5),
              "all four, order 18": dict(brightness=75000, contrast=110000, saturation=20000, hue=40000, order=18)}


@pytest.mark.parametrize("case", sorted(CUBE_CASES))
def test_colour_cube(ofdg, case):
    """All 2^24 colours, sixteen uint8 samples of 1024 x 1024: the device against the host twin."""
    import torch
    g = make_gen(ofdg, 64, 32)
    cube = jr.cube()
    recs = np.array([jr.rec_of(**CUBE_CASES[case])] * 16, jr.REC)
    (want, _), used = ofdg.host_jitter((cube, None), recs=recs)
    work, rout = ofdg.alloc_jitter(16)
    d = torch.from_numpy(cube).cuda()
    g.jitter((d, None), recs=dev_recs(recs), recs_out=rout, work=work, size=(1024, 1024))
    torch.cuda.synchronize()
    assert jr.equal_bits(d.cpu().numpy(), want), case
    assert jr.equal_bits(ofdg.jitter_numpy(rout), used) and not np.array_equal(want, cube)


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
def test_behind_forward_counter_and_crop(ofdg, compact):
    """Mode 7 on OFDG_STREAM_OWN: forward_counter and the jitter in place behind it; then forward_counter, the crop to 96x48 and
    the jitter of the crop's planes through size=, into buffers of the other format."""
    import torch
    W, H, B, cw, ch = 128, 64, 3, 96, 48
    kw = dict(first_index=40, ranges=dict(jr.RAFT, asym_prob=0.5))
    g = make_gen(ofdg, W, H, 7, pool=True, sampler=1, seed=5, batch_size=B)
    plain, _ = rendered(ofdg, g, B, compact, 40)
    base = to_host((plain["image0"], plain["image1"]))

    def in_place(src, enqueue, more=None):
        if not enqueue:
            return ofdg.alloc_jitter(B)
        g.jitter((src["image0"], src["image1"]), recs_out=more[1], work=more[0], stream=ofdg.STREAM_OWN, **kw)

    got, (_, recs) = rendered(ofdg, g, B, compact, 40, in_place)
    want, used = ofdg.host_jitter(base, seed=5, **kw)
    jr.expect_equal(to_host((got["image0"], got["image1"])), want, "behind forward_counter")
    assert jr.equal_bits(ofdg.jitter_numpy(recs), used) and not jr.equal_bits(want[0], base[0]) and (used["mean"] >= 0).all()
    assert jr.equal_bits(got["flow"].cpu().numpy(), plain["flow"].cpu().numpy())
    other = torch.float32 if compact else torch.uint8

    def cropped(src, enqueue, more=None):
        if not enqueue:
            dst = ofdg.alloc_crop(src, ch, cw)
            return dst, tuple(torch.zeros((B, 3, ch, cw), dtype=other, device="cuda") for _ in range(2)), ofdg.alloc_jitter(B)
        dst, out, (work, recs) = more
        g.crop(src, dst, first_index=40, stream=ofdg.STREAM_OWN)
        g.jitter((dst["image0"], dst["image1"]), out, recs_out=recs, work=work, stream=ofdg.STREAM_OWN, size=(ch, cw), **kw)

    _, (dst, out, (_, recs)) = rendered(ofdg, g, B, compact, 40, cropped)
    crop_host = to_host((dst["image0"], dst["image1"]))
    want, used = ofdg.host_jitter(crop_host, seed=5, dst_dtype=np.uint8 if other == torch.uint8 else np.float32, **kw)
    jr.expect_equal(to_host(out), want, "behind the crop")
    assert jr.equal_bits(ofdg.jitter_numpy(recs), used)


def test_mode_9(ofdg):
    import torch
    W, H, B = 128, 64, 2
    g = make_gen(ofdg, W, H, 9, pool=True, sampler=1, seed=3, batch_size=B)
    g.warp_generate(1, 3)
    kw = dict(first_index=0, ranges=jr.RAFT)
    both = []
    for jitter in (False, True):
        outs = ofdg.alloc_outputs(B, H, W)
        work, recs = ofdg.alloc_jitter(B)
        torch.cuda.synchronize()
        g.forward_counter(0, B, *outs, ofdg.STREAM_OWN)
        if jitter:
            g.jitter(outs[:2], recs_out=recs, work=work, stream=ofdg.STREAM_OWN, **kw)
        g.synchronize(ofdg.STREAM_OWN)
        torch.cuda.synchronize()
        both.append((to_host(outs), ofdg.jitter_numpy(recs)))
    want, used = ofdg.host_jitter(both[0][0][:2], seed=3, **kw)
    jr.expect_equal(both[1][0][:2], want, "mode 9")
    assert jr.equal_bits(both[1][1], used) and jr.equal_bits(both[1][0][2], both[0][0][2]) and not jr.equal_bits(want[0], both[0][0][0])


def test_three_calls_in_flight(ofdg):
    """Two calls on two caller streams and one on OFDG_STREAM_OWN, each with its own workspace and records, one wait at the end."""
    import torch
    W, H, B = 128, 64, 2
    g = make_gen(ofdg, W, H, 7, pool=True)
    users = [torch.cuda.Stream(), torch.cuda.Stream()]
    batches = [g.sample(B) for _ in range(3)]
    kw = lambda k: dict(first_index=100 * k, seed=9, ranges=dict(jr.RAFT, asym_prob=0.5))  # noqa: E731
    plain = []
    for tasks, bps, n in batches:
        outs = ofdg.alloc_outputs(B, H, W)
        torch.cuda.synchronize()
        g.render(tasks, B, bps, n, *outs, 0)
        g.synchronize(0)
        torch.cuda.synchronize()
        plain.append(to_host(outs[:2]))
    sets = [(ofdg.alloc_outputs(B, H, W), ofdg.alloc_jitter(B)) for _ in range(3)]
    torch.cuda.synchronize()
    streams = [users[0].cuda_stream, users[1].cuda_stream, ofdg.STREAM_OWN]
    for k, ((tasks, bps, n), (o, (work, recs)), st) in enumerate(zip(batches, sets, streams)):
        g.render(tasks, B, bps, n, *o, st)
        g.jitter(o[:2], recs_out=recs, work=work, stream=st, **kw(k))
    for st in streams:
        g.synchronize(st)
    torch.cuda.synchronize()
    for k, (o, (work, recs)) in enumerate(sets):
        want, used = ofdg.host_jitter(plain[k], **kw(k))
        jr.expect_equal(to_host(o[:2]), want, "call %d" % k)
        assert jr.equal_bits(ofdg.jitter_numpy(recs), used)
    assert not jr.equal_bits(ofdg.jitter_numpy(sets[0][1][1]), ofdg.jitter_numpy(sets[1][1][1]))


def test_flowloader_jitter(ofdg):
    """FlowLoader(jitter=JITTER_RAFT) against the same chain made by hand from the loader without it: with photo=, erase= and pack=
    around it (the eraser's mean fill is that of the jittered frame), and behind motion_blur= (the blurred frames are jittered)."""
    import torch
    import erase_reference as er
    W, H, B, cw, ch = 128, 96, 2, 96, 48
    kw = dict(width=W, height=H, mode=7, batch_size=B, sampler=1, seed=21)
    pool = lambda g: g.pool_synthetic(3, 2 * W, 2 * H, 11)  # noqa: E731
    extras = ("flow1", "occ0", "occ1")
    make = lambda **more: ofdg.FlowLoader(ofdg.default_params(**kw), pool=pool, prefetch=3, **more)  # noqa: E731
    erase = dict(er.RAFT, prob=1.0, min_size=8, max_size=30, frames=(0, 1))
    ranges = {k: v for k, v in erase.items() if k in ofdg.ERASE_RANGES}
    # 1. crop, photo, jitter, erase, pack: the hand-made chain starts from the loader with crop= and photo= alone
    opts = dict(extras=extras, crop=(ch, cw), photo=ofdg.PHOTO_FLOWNET)
    pack = dict(image_dtype=torch.float16, concat=True)
    full, plain = iter(make(jitter=ofdg.JITTER_RAFT, erase=erase, pack=pack, **opts)), iter(make(**opts))
    for step in range(3):
        a, p = next(full), next(plain)
        torch.cuda.current_stream().synchronize()
        assert set(a[3]) == set(p[3]) | {"jitter", "erase"} and a[3]["jitter"].dtype == torch.int32 and tuple(a[3]["jitter"].shape) == (B, 16)
        index = ofdg.shard_first_index(step, B, 1, 0)
        base = dict(zip(PLANES, to_host(p[:3])), **{k: p[3][k].cpu().numpy() for k in extras})
        (j0, j1), used = ofdg.host_jitter((base["image0"], base["image1"]), first_index=index, seed=21, ranges=ofdg.JITTER_RAFT)
        assert jr.equal_bits(ofdg.jitter_numpy(a[3]["jitter"]), used) and torch.equal(a[3]["photo"], p[3]["photo"])
        erased = [np.array(j0), np.array(j1)]
        occ = [np.array(base["occ0"]), np.array(base["occ1"])]
        e_used = ofdg.host_erase(erased, occ, (base["flow"], base["flow1"]), first_index=index, seed=21, ranges=ranges, frames=(0, 1))
        assert er.equal_bits(ofdg.erase_numpy(a[3]["erase"]), e_used) and jr.equal_bits(a[3]["occ0"].cpu().numpy(), occ[0])
        packed = ofdg.host_pack(dict(image0=erased[0], image1=erased[1], flow=base["flow"]), image_dtype=np.float16, concat=True)
        assert a[1] is None and jr.equal_bits(a[0].cpu().numpy(), packed["image0"]) and jr.equal_bits(a[2].cpu().numpy(), packed["flow"])
        assert not jr.equal_bits(j0, base["image0"])
    resumed = next(iter(make(jitter=ofdg.JITTER_RAFT, erase=erase, pack=pack, start=2, **opts)))
    torch.cuda.current_stream().synchronize()
    assert torch.equal(resumed[3]["jitter"], a[3]["jitter"]) and torch.equal(resumed[0], a[0])
    # 2. motion_blur=: the jitter works on the blurred frames
    opts = dict(extras=("flow1",), motion_blur=ofdg.MBLUR_DEFAULT, image_dtype=torch.uint8, flow_dtype=torch.float16, extras_compact=True)
    full, plain = iter(make(jitter=ofdg.JITTER_RAFT, **opts)), iter(make(**opts))
    for step in range(2):
        a, p = next(full), next(plain)
        torch.cuda.current_stream().synchronize()
        index = ofdg.shard_first_index(step, B, 1, 0)
        want, used = ofdg.host_jitter(to_host(p[:2]), first_index=index, seed=21, ranges=ofdg.JITTER_RAFT)
        jr.expect_equal(to_host(a[:2]), want, "behind motion_blur=, batch %d" % step)
        assert jr.equal_bits(ofdg.jitter_numpy(a[3]["jitter"]), used) and torch.equal(a[3]["motion_blur"], p[3]["motion_blur"]) and torch.equal(a[2], p[2])
    # without jitter= the loader yields what it yielded before; an unknown key raises
    bare = next(iter(make()))
    assert len(bare) == 3
    only = next(iter(make(jitter=ofdg.JITTER_RAFT)))
    torch.cuda.current_stream().synchronize()
    assert set(only[3]) == {"jitter"} and torch.equal(only[2], bare[2]) and not torch.equal(only[0], bare[0])
    with pytest.raises(ValueError, match="unknown range"):
        make(jitter=dict(gamma=0.2))


def test_refusals_enqueue_nothing(ofdg):
    import torch
    W, H, B = 128, 96, 2
    g = make_gen(ofdg, W, H, 7, pool=True, batch_size=B)
    bufs = [guarded(np.zeros((B, 3, H, W), np.float32)) for _ in range(4)]   # src0, src1, dst0, dst1
    wraw, work = guarded(np.full((B, 16), FILL, np.uint8))
    rraw, rout = guarded(np.full((B, 16), -1, np.int32))
    recs = dev_recs(jr.records()[1:3])
    everything = bufs + [(wraw, work), (rraw, rout)]
    before = [raw.clone() for raw, _ in everything]
    torch.cuda.synchronize()
    lib, vp = ofdg.lib(), C.c_void_p

    def job(**kw):
        j = ofdg.JitterJob()
        for f in range(2):
            j.src[f], j.dst[f] = bufs[f][1].data_ptr(), bufs[2 + f][1].data_ptr()
        j.recs, j.recs_out, j.work = recs.data_ptr(), rout.data_ptr(), work.data_ptr()
        j.src_fmt, j.dst_fmt = ofdg.FMT_F32, ofdg.FMT_U8
        for k, v in kw.items():
            if isinstance(v, dict):
                for idx, val in v.items():
                    getattr(j, k)[idx] = val
            else:
                setattr(j, k, v)
        return j

    def refused(word, j, n=B, stream=0):
        rc = lib.ofdg_jitter(g.h, None if j is None else C.byref(j), n, vp(stream))
        assert rc == ofdg.EINVAL, word
        msg = lib.ofdg_last_error(g.h).decode()
        assert msg.startswith("ofdg_jitter: ") and word in msg, (word, msg)
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
    refused("contrast", job(recs=None, contrast=3.5))
    refused("hue", job(recs=None, hue=float("nan")))
    refused("asym_prob", job(asym_prob=-0.5))
    refused("no frame is set", job(src={0: None, 1: None}, dst={0: None, 1: None}))
    refused("source and no destination", job(dst={0: None}))
    refused("destination and no source", job(src={1: None}))
    refused("work is NULL", job(work=None))
    refused("work is NULL", job(work=None, recs=None, contrast=0.4))
    refused("work must be 16-byte", job(work=work.data_ptr() + 8))
    refused("src[image0] must be 16-byte aligned", job(src={0: bufs[0][1].data_ptr() + 4}))
    refused("src[image1] must be 4-byte aligned", job(src={1: bufs[1][1].data_ptr() + 2}, src_fmt=ofdg.FMT_U8))
    refused("dst[image1] must be 16-byte aligned", job(dst={1: bufs[3][1].data_ptr() + 4}))
    refused("recs must", job(recs=recs.data_ptr() + 8))
    refused("recs_out", job(recs_out=rout.data_ptr() + 4))
    refused("overlaps", job(dst={1: bufs[2][1].data_ptr() + 16}))
    refused("overlaps", job(dst={0: bufs[1][1].data_ptr()}))
    refused("overlaps", job(dst={0: bufs[0][1].data_ptr()}))                    # in place, but in another format
    refused("overlaps", job(work=rout.data_ptr()))
    refused("overlaps", job(recs_out=recs.data_ptr()))
    refused("overlaps", job(work=bufs[3][1].data_ptr() + 64))
    # a valid call on the same context still works, also on OFDG_STREAM_OWN once a call has been made
    outs = ofdg.alloc_outputs(B, H, W)
    torch.cuda.synchronize()
    g.forward(*outs, ofdg.STREAM_OWN)
    g.synchronize(ofdg.STREAM_OWN)
    torch.cuda.synchronize()
    base = to_host(outs[:2])
    g.jitter(outs[:2], recs=recs, recs_out=rout, work=work, stream=ofdg.STREAM_OWN)
    g.synchronize(ofdg.STREAM_OWN)
    torch.cuda.synchronize()
    want, used = ofdg.host_jitter(base, recs=jr.records()[1:3])
    jr.expect_equal(to_host(outs[:2]), want, "after the refusals")
    assert jr.equal_bits(ofdg.jitter_numpy(rout), used) and guards_intact(everything)
