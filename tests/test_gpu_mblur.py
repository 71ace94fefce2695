"""GPU tests of motion blur (ofdg_motion_blur, include/ofdg.h): the device frames against ofdg_host_motion_blur and against the
numpy restatement (tests/mblur_reference.py), byte for byte - every format, size and tap cap, between guard bytes, twice,
subsets of frames; behind forward_counter, the crop and the spatial step without synchronisation, in mode 9, with three calls
in flight, through the loader - and the refusals."""
import ctypes as C

import numpy as np
import pytest

import mblur_reference as mr

pytestmark = pytest.mark.gpu

GRID, KNOWN = mr.GRID, mr.KNOWN

FILL = 0xA5
GUARD = 64  # bytes in front of and behind every written plane (keeps the 16-byte alignment)
PLANES = ("image0", "image1", "flow")
RANGES = dict(prob=1.0, shutter_min=0.5, shutter_max=2.0, pair_shutter=0.25)


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


def pick(pair, sel):
    return tuple(t if f in sel else None for f, t in enumerate(pair))


# A workgroup owns a 64 x 16 tile, a lane four pixels, a pair of lanes one 8-byte store of a uint8 row.  8x2 and 24x6: one
# partial tile (the window path on them: test_tiles_that_stage_a_window).  72x40: 2 x 3 tiles, the second column 8 pixels
# wide.  264x200: 5 x 13 tiles, partial last ones both ways, uint8 rows 8 mod 16 wide; its flows hold a streak across the tile
# corner at (64, 16), one 50 px long and one whose taps but the centre lie 20 px and more from the pixel, and streaks that
# leave every border.
@pytest.mark.parametrize("W,H,src_dtype,dst_dtype,flow_dtype,taps_side", GRID)
def test_device_equals_host_twin_and_restatement(ofdg, W, H, src_dtype, dst_dtype, flow_dtype, taps_side):
    """Every destination and recs_out lies between 0xA5 guards; sources, flows and given records stay as they are.  Both frames
    with given records, then with drawn ones; each call runs twice."""
    import torch
    g = make_gen(ofdg, 64, 32)  # (the context's own frame is another: the job gives the size)
    images, flows, recs, want, used = mr.case(W, H, src_dtype, flow_dtype, taps_side)
    what = "%dx%d %s to %s, flow %s, taps_side %d" % (W, H, src_dtype, dst_dtype, flow_dtype, taps_side)
    d_img, d_flow = to_dev(images), to_dev(flows)
    drawn = mr.drawn_records(11, 2 ** 32 - 1, mr.N, RANGES)
    calls = [(dict(recs=recs), want[dst_dtype], used)]
    if taps_side == 16:
        host, host_used = ofdg.host_motion_blur(images, flows, seed=11, first_index=2 ** 32 - 1, ranges=RANGES, taps_side=taps_side, dst_dtype=dst_dtype)
        assert mr.equal_bits(host_used, mr.sanitise(drawn))
        calls.append((dict(seed=11, first_index=2 ** 32 - 1, ranges=RANGES), host, host_used))
    for kw, expect, expect_recs in calls:
        for _ in range(2):
            bufs = [guarded(np.full(t.shape, 7, dst_dtype)) for t in images]
            rraw, rout = guarded(np.full((mr.N, 4), -1.0, np.float32))
            d_recs = to_dev((kw["recs"],))[0] if "recs" in kw else None
            g.motion_blur(d_img, (bufs[0][1], bufs[1][1]), flow=d_flow, taps_side=taps_side, recs_out=rout, size=(H, W), **dict(kw, recs=d_recs))
            torch.cuda.synchronize()
            assert guards_intact(bufs + [(rraw, rout)]), what
            mr.expect_equal(to_host((bufs[0][1], bufs[1][1])), expect, what)
            assert mr.equal_bits(rout.cpu().numpy(), expect_recs), what
            if d_recs is not None:
                assert mr.equal_bits(d_recs.cpu().numpy(), recs)
    if taps_side == 16:  # the twin against the restatement under the drawn records too
        mr.expect_equal(calls[1][1], mr.motion_blur(images, flows, drawn, taps_side, dst_dtype)[0], what + ": drawn, twin against restatement")
    mr.expect_equal(to_host(d_img), images, what + ": the sources")
    mr.expect_equal(to_host(d_flow), flows, what + ": the flows")


@pytest.mark.parametrize("W,H,taps_side,gentle", [(264, 200, 16, False), (264, 200, 4, False), (72, 40, 16, False), (8, 2, 16, True), (8, 2, 4, True),
                                                  (24, 6, 16, True), (24, 6, 4, True), (72, 40, 16, True)])
@pytest.mark.parametrize("src_dtype,dst_dtype,flow_dtype", mr.FORMATS)
def test_tiles_that_stage_a_window(ofdg, W, H, taps_side, gentle, src_dtype, dst_dtype, flow_dtype):
    """A +-65504 in every tile sends every tile of the grid above to the gather.  Without the special values 264x200 and 72x40
    have tiles that copy, tiles that stage their window - those at the borders and corners of the plane among them - and
    tiles that gather side by side.  The gentle flows keep every tap within 16 px: at 8x2 and 24x6 the one tile of samples 1
    and 2 stages a window that exceeds the plane on all four sides (its origin is negative both ways, every border is
    replicated at once), over random float32 and uint8 frames, float32 ones with NaN, -3, 255.5 and 1e9 through the byte rule of
    the staging loop; tests/test_mblur.py asserts which path each of these cases takes.  Twice."""
    import torch
    g = make_gen(ofdg, W, H)
    images, flows, recs, want, used = mr.case(W, H, src_dtype, flow_dtype, taps_side, special=False, gentle=gentle)
    host, host_used = ofdg.host_motion_blur(images, flows, recs=recs, taps_side=taps_side, dst_dtype=dst_dtype)
    d_img, d_flow, d_recs = to_dev(images), to_dev(flows), to_dev((recs,))[0]
    for _ in range(2):
        bufs = [guarded(np.full(t.shape, 7, dst_dtype)) for t in images]
        rraw, rout = guarded(np.full((mr.N, 4), -1.0, np.float32))
        g.motion_blur(d_img, (bufs[0][1], bufs[1][1]), flow=d_flow, recs=d_recs, taps_side=taps_side, recs_out=rout)
        torch.cuda.synchronize()
        got = to_host((bufs[0][1], bufs[1][1]))
        mr.expect_equal(got, want[dst_dtype], "against the restatement")
        mr.expect_equal(got, host, "against ofdg_host_motion_blur")
        assert guards_intact(bufs + [(rraw, rout)]) and mr.equal_bits(rout.cpu().numpy(), used) and mr.equal_bits(host_used, used)


@pytest.mark.parametrize("src_dtype,dst_dtype,flow_dtype", [mr.FORMATS[0], mr.FORMATS[7], mr.FORMATS[5]])
def test_subsets_of_frames(ofdg, src_dtype, dst_dtype, flow_dtype):
    """Frame 0 alone and frame 1 alone give that frame's bytes; the other destination is not touched."""
    import torch
    W, H = 264, 200
    g = make_gen(ofdg, W, H)
    images, flows, recs, want, used = mr.case(W, H, src_dtype, flow_dtype, 16)
    d_img, d_flow, d_recs = to_dev(images), to_dev(flows), to_dev((recs,))[0]
    for sel in ((0,), (1,)):
        bufs = [guarded(np.full(t.shape, 7, dst_dtype)) for t in images]
        rraw, rout = guarded(np.full((mr.N, 4), -1.0, np.float32))
        g.motion_blur(pick(d_img, sel), pick((bufs[0][1], bufs[1][1]), sel), flow=pick(d_flow, sel), recs=d_recs, taps_side=16, recs_out=rout)
        torch.cuda.synchronize()
        f = sel[0]
        assert mr.equal_bits(bufs[f][1].cpu().numpy().astype(np.float32), want[dst_dtype][f].astype(np.float32)), sel
        assert bool((bufs[1 - f][1] == 7).all()) and guards_intact(bufs + [(rraw, rout)]) and mr.equal_bits(rout.cpu().numpy(), used)


@pytest.mark.parametrize("vec,shutter,taps_side,answer", KNOWN)
def test_known_answers_on_the_device(ofdg, vec, shutter, taps_side, answer):
    import torch
    g = make_gen(ofdg, 24, 6)
    img, fl, rec = mr.impulse(vec[0], vec[1], shutter)
    want = np.zeros((6, 24), np.uint8)
    for (x, y), b in answer.items():
        want[y, x] = b
    (out, _), _ = ofdg.alloc_motion_blur(1, 6, 24, torch.uint8, frames=(0,))
    g.motion_blur((to_dev((img,))[0], None), (out, None), flow=(to_dev((fl,))[0], None), recs=to_dev((rec,))[0], taps_side=taps_side)
    torch.cuda.synchronize()
    assert all(np.array_equal(out[0, c].cpu().numpy(), want) for c in range(3)), out[0, 0]


def rendered(ofdg, g, B, compact, first_index, then=None, extras=True):
    """forward_counter with all extras on the internal stream and `then(planes)` behind it, nothing waited for in between"""
    import torch
    W, H = g.params.width, g.params.height
    kw = dict(image_dtype=torch.uint8, flow_dtype=torch.float16) if compact else {}
    xkw = dict(flow_dtype=torch.float16, occ_dtype=torch.uint8) if compact else {}
    outs = ofdg.alloc_outputs(B, H, W, **kw)
    ex = ofdg.alloc_extras(B, H, W, **xkw) if extras else None
    src = dict(zip(PLANES, outs), **(ex or {}))
    more = then(src, False) if then else None
    torch.cuda.synchronize()  # (the allocations were zeroed on torch's stream)
    g.forward_counter(first_index, B, *outs, ofdg.STREAM_OWN, extras=ex)
    if then:
        then(src, True, more)
    g.synchronize(ofdg.STREAM_OWN)
    torch.cuda.synchronize()
    return src, more


def host_planes(src):
    return {k: v.cpu().numpy() for k, v in src.items()}


def blur_host(ofdg, p, frames=(0, 1), **kw):
    """ofdg_host_motion_blur of the named host planes: ((out0, out1), records)"""
    return ofdg.host_motion_blur(pick((p["image0"], p["image1"]), frames), pick((p["flow"], p.get("flow1")), frames), **kw)


@pytest.mark.parametrize("compact", [False, True])
def test_behind_forward_counter(ofdg, compact):
    """Mode 7 with all extras, float32 and compact: both frames blurred behind forward_counter; nothing else is touched."""
    import torch
    W, H, B = 128, 64, 3
    kw = dict(first_index=40, ranges=RANGES, taps_side=8)
    g = make_gen(ofdg, W, H, 7, pool=True, sampler=1, seed=5, batch_size=B)
    plain, _ = rendered(ofdg, g, B, compact, 40)

    def then(src, enqueue, more=None):
        if not enqueue:
            return ofdg.alloc_motion_blur(B, H, W, src["image0"].dtype)
        out, recs = more
        g.motion_blur((src["image0"], src["image1"]), out, flow=(src["flow"], src["flow1"]), recs_out=recs, stream=ofdg.STREAM_OWN, **kw)

    src, (out, recs) = rendered(ofdg, g, B, compact, 40, then)
    base = host_planes(plain)
    want, used = blur_host(ofdg, base, seed=5, **kw)
    mr.expect_equal(to_host(out), want, "compact %s" % compact)
    assert mr.equal_bits(recs.cpu().numpy(), used) and (used[:, :2] > 0).all()
    got = host_planes(src)
    assert all(np.array_equal(got[k].view(np.uint8), base[k].view(np.uint8)) for k in base)  # sources, flows, maps and labels untouched
    assert not np.array_equal(want[0], base["image0"]) and not np.array_equal(want[1], base["image1"])


def test_mode_9_frame_0_only(ofdg):
    import torch
    W, H, B = 128, 64, 2
    g = make_gen(ofdg, W, H, 9, pool=True, sampler=1, seed=3, batch_size=B)
    g.warp_generate(1, 3)
    kw = dict(first_index=0, ranges=RANGES, taps_side=4)
    (out, _), recs = ofdg.alloc_motion_blur(B, H, W, frames=(0,))
    outs = ofdg.alloc_outputs(B, H, W)
    torch.cuda.synchronize()
    g.forward_counter(0, B, *outs, ofdg.STREAM_OWN)
    g.motion_blur((outs[0], None), (out, None), flow=(outs[2], None), recs_out=recs, stream=ofdg.STREAM_OWN, **kw)
    g.synchronize(ofdg.STREAM_OWN)
    torch.cuda.synchronize()
    base = to_host(outs)
    (want, _), used = ofdg.host_motion_blur((base[0], None), (base[2], None), seed=3, **kw)
    assert mr.equal_bits(out.cpu().numpy(), want) and mr.equal_bits(recs.cpu().numpy(), used) and not np.array_equal(want, base[0])
    with pytest.raises(ValueError, match="only frame 0"):
        g.motion_blur(outs[:2], (out, out), flow=(outs[2], None))


def test_behind_crop_and_spatial(ofdg):
    """128x64 to 96x48 on OFDG_STREAM_OWN: forward_counter, the crop (then the spatial step) and the blur of its planes."""
    import torch
    W, H, B, ow, oh = 128, 64, 3, 96, 48
    kw = dict(first_index=8, ranges=RANGES, taps_side=16)
    for step in ("crop", "spatial"):
        g = make_gen(ofdg, W, H, 7, pool=True, sampler=1, seed=6, batch_size=B)

        def window(src, dst):
            if step == "crop":
                g.crop(src, dst, first_index=8, occ_window=True, stream=ofdg.STREAM_OWN)
            else:
                g.spatial(src, dst, first_index=8, ranges=ofdg.SPATIAL_FLOWNET, occ_window=True, stream=ofdg.STREAM_OWN)

        def then(src, enqueue, more=None):
            if not enqueue:
                return (ofdg.alloc_crop(src, oh, ow) if step == "crop" else ofdg.alloc_spatial(src, oh, ow)), ofdg.alloc_motion_blur(B, oh, ow)
            dst, (out, recs) = more
            window(src, dst)
            g.motion_blur((dst["image0"], dst["image1"]), out, flow=(dst["flow"], dst["flow1"]), recs_out=recs, stream=ofdg.STREAM_OWN, size=(oh, ow), **kw)

        _, (dst, (out, recs)) = rendered(ofdg, g, B, False, 8, then)
        base = host_planes(dst)
        want, used = blur_host(ofdg, base, seed=6, **kw)
        mr.expect_equal(to_host(out), want, step)
        assert mr.equal_bits(recs.cpu().numpy(), used) and not np.array_equal(want[0], base["image0"])


def test_three_calls_in_flight(ofdg):
    """Two calls on two caller streams and one on OFDG_STREAM_OWN, each with its own frames and records, one wait at the end."""
    import torch
    W, H, B = 128, 64, 2
    g = make_gen(ofdg, W, H, 7, pool=True)
    users = [torch.cuda.Stream(), torch.cuda.Stream()]
    batches = [g.sample(B) for _ in range(3)]
    kw = lambda k: dict(first_index=100 * k, seed=9, ranges=RANGES, taps_side=(4, 8, 16)[k])  # noqa: E731
    plain = []
    for tasks, bps, n in batches:
        outs, ex = ofdg.alloc_outputs(B, H, W), ofdg.alloc_extras(B, H, W)
        torch.cuda.synchronize()
        g.render(tasks, B, bps, n, *outs, 0, extras=ex)
        g.synchronize(0)
        torch.cuda.synchronize()
        plain.append(host_planes(dict(zip(PLANES, outs), **ex)))
    sets = [(ofdg.alloc_outputs(B, H, W), ofdg.alloc_extras(B, H, W), ofdg.alloc_motion_blur(B, H, W)) for _ in range(3)]
    torch.cuda.synchronize()
    streams = [users[0].cuda_stream, users[1].cuda_stream, ofdg.STREAM_OWN]
    for k, ((tasks, bps, n), (o, ex, (out, recs)), st) in enumerate(zip(batches, sets, streams)):
        g.render(tasks, B, bps, n, *o, st, extras=ex)
        g.motion_blur(o[:2], out, flow=(o[2], ex["flow1"]), recs_out=recs, stream=st, **kw(k))
    for st in streams:
        g.synchronize(st)
    torch.cuda.synchronize()
    for k, (o, ex, (out, recs)) in enumerate(sets):
        want, used = blur_host(ofdg, plain[k], **kw(k))
        mr.expect_equal(to_host(out), want, "call %d" % k)
        assert mr.equal_bits(recs.cpu().numpy(), used)
    assert not mr.equal_bits(sets[0][2][1].cpu().numpy(), sets[1][2][1].cpu().numpy())


def test_flowloader_motion_blur(ofdg):
    """extras=, crop=, motion_blur=, photo=, erase= and pack= for three batches against the manual sequence on the host - the
    blur of the plain loader's cropped frames, then the photometric step and the eraser of the twins -, resumed at start=2, and
    without motion_blur=."""
    import torch
    W, H, B, cw, ch = 128, 96, 2, 96, 48
    kw = dict(width=W, height=H, mode=7, batch_size=B, sampler=1, seed=21)
    pool = lambda g: g.pool_synthetic(3, 2 * W, 2 * H, 11)  # noqa: E731
    extras = ("flow1", "occ0", "occ1")
    photo = dict(ofdg.PHOTO_FLOWNET, sigma_max=0.0)
    erase = dict(ofdg.ERASE_RAFT, prob=1.0, min_size=8, max_size=30, fill=ofdg.ERASE_CONST, color=(1, 2, 3), frames=(0, 1))
    blur = dict(RANGES, taps_side=8)
    make = lambda **more: ofdg.FlowLoader(ofdg.default_params(**kw), pool=pool, prefetch=3, extras=extras, crop=(ch, cw), **more)  # noqa: E731
    full, sharp = iter(make(motion_blur=blur, photo=photo, erase=erase, pack=dict())), iter(make())
    blurred_only = iter(make(motion_blur=blur))
    last = None
    for step in range(3):
        a, p, b = next(full), next(sharp), next(blurred_only)
        torch.cuda.current_stream().synchronize()
        assert set(a[3]) == set(p[3]) | {"motion_blur", "photo", "erase"} and set(b[3]) == set(p[3]) | {"motion_blur"}
        assert a[3]["motion_blur"].dtype == torch.float32 and tuple(a[3]["motion_blur"].shape) == (B, 4)
        index = ofdg.shard_first_index(step, B, 1, 0)
        base = dict(zip(PLANES, to_host(p[:3])), **{k: p[3][k].cpu().numpy() for k in extras})
        want, used = blur_host(ofdg, base, first_index=index, seed=21, ranges=RANGES, taps_side=8)
        mr.expect_equal(to_host(b[:2]), want, "batch %d: the blurred frames" % step)
        assert mr.equal_bits(b[3]["motion_blur"].cpu().numpy(), used) and mr.equal_bits(a[3]["motion_blur"].cpu().numpy(), used)
        assert (used[:, :2] > 0).all() and not np.array_equal(want[0], base["image0"])
        # flow, maps and the crop's records are those of the sharp frames
        assert all(torch.equal(b[3][k], p[3][k]) for k in p[3]) and torch.equal(b[2], p[2])
        # the later stages work on the blurred frames: photo, erase and pack of the twins on `want`
        lit, photo_used = ofdg.host_photo(want, first_index=index, seed=21, ranges=photo)
        assert mr.equal_bits(a[3]["photo"].cpu().numpy(), photo_used)
        planes = dict(base, image0=np.array(lit[0]), image1=np.array(lit[1]))
        erase_used = ofdg.host_erase((planes["image0"], planes["image1"]), (planes["occ0"], planes["occ1"]), (planes["flow"], planes["flow1"]),
                                     first_index=index, seed=21, ranges={k: v for k, v in erase.items() if k in ofdg.ERASE_RANGES},
                                     fill=ofdg.ERASE_CONST, color=(1, 2, 3), frames=(0, 1))
        assert ofdg.erase_numpy(a[3]["erase"]).tobytes() == erase_used.tobytes()
        mr.expect_equal(to_host(a[:2]), (planes["image0"], planes["image1"]), "batch %d: behind photo, erase and pack" % step)
        assert np.array_equal(a[2].cpu().numpy(), base["flow"])
        assert np.array_equal(a[3]["occ0"].cpu().numpy(), planes["occ0"])
        last = (to_host(b[:2]), used)
    resumed = next(iter(make(motion_blur=blur, start=2)))
    torch.cuda.current_stream().synchronize()
    assert mr.equal_bits(resumed[3]["motion_blur"].cpu().numpy(), last[1])
    mr.expect_equal(to_host(resumed[:2]), last[0], "resumed")
    # without motion_blur= the loader yields what it yielded: a plain tuple without extras, the same dict with them
    bare = next(iter(ofdg.FlowLoader(ofdg.default_params(**kw), pool=pool, prefetch=3)))
    assert len(bare) == 3
    x = next(iter(ofdg.FlowLoader(ofdg.default_params(**kw), pool=pool, prefetch=3, extras=("occ0",))))
    assert set(x[3]) == {"occ0"}
    # without extras= and a window: MBLUR_DEFAULT as it is, frame 0 alone into the further ring; image1 and flow are the ring's own
    it = iter(ofdg.FlowLoader(ofdg.default_params(**kw), pool=pool, prefetch=3, motion_blur=ofdg.MBLUR_DEFAULT))
    b0 = next(it)
    torch.cuda.current_stream().synchronize()
    assert set(b0[3]) == {"motion_blur"} and torch.equal(b0[1], bare[1]) and torch.equal(b0[2], bare[2])
    h = to_host(bare)
    (w0, _), u0 = ofdg.host_motion_blur((h[0], None), (h[2], None), first_index=0, seed=21, ranges=ofdg.MBLUR_DEFAULT)
    assert mr.equal_bits(b0[0].cpu().numpy(), w0) and mr.equal_bits(b0[3]["motion_blur"].cpu().numpy(), u0)
    for bad, word in ((dict(motion_blur=dict(shutter=3)), "unknown motion_blur"), (dict(motion_blur=dict(frames=(0, 1)), extras=("occ0",)), r"frames=\(0,\)"),
                      (dict(motion_blur=dict(frames=(1,))), r"frames=\(0,\)"), (dict(motion_blur=dict(frames=(3,)), extras=("flow1",)), "frames")):
        with pytest.raises(ValueError, match=word):
            ofdg.FlowLoader(ofdg.default_params(**kw), pool=pool, prefetch=3, **bad)


def test_refusals_enqueue_nothing(ofdg):
    import torch
    W, H, B = 128, 96, 2
    g = make_gen(ofdg, W, H, 7, pool=True, batch_size=B)
    dsts = [guarded(np.full((B, 3, H, W), 7, np.float32)) for _ in range(2)]
    srcs = [torch.full((B, 3, H, W), 100.0, dtype=torch.float32, device="cuda") for _ in range(2)]
    flows = [torch.full((B, 2, H, W), 3.25, dtype=torch.float32, device="cuda") for _ in range(2)]
    rraw, rout = guarded(np.full((B, 4), -1.0, np.float32))
    recs = to_dev((np.array([[1.0, 9.0, 0, 0]] * B, np.float32),))[0]
    everything = dsts + [(rraw, rout)]
    before = [raw.clone() for raw, _ in everything]
    torch.cuda.synchronize()
    lib, vp = ofdg.lib(), C.c_void_p

    def job(**kw):
        j = ofdg.MblurJob()
        for f in range(2):
            j.src[f], j.dst[f], j.flow[f] = srcs[f].data_ptr(), dsts[f][1].data_ptr(), flows[f].data_ptr()
        j.recs, j.recs_out = recs.data_ptr(), rout.data_ptr()
        j.src_fmt = j.dst_fmt = j.flow_fmt = ofdg.FMT_F32
        j.taps_side, j.prob, j.shutter_max = 8, 1.0, 1.0
        for k, v in kw.items():
            if isinstance(v, dict):
                for idx, val in v.items():
                    getattr(j, k)[idx] = val
            else:
                setattr(j, k, v)
        return j

    def refused(word, j, n=B, stream=0):
        rc = lib.ofdg_motion_blur(g.h, None if j is None else C.byref(j), n, vp(stream))
        assert rc == ofdg.EINVAL, word
        msg = lib.ofdg_last_error(g.h).decode()
        assert msg.startswith("ofdg_motion_blur: ") and word in msg, (word, msg)
        g.synchronize()
        torch.cuda.synchronize()
        assert all(torch.equal(raw, b) for (raw, _), b in zip(everything, before)), word

    refused("OFDG_STREAM_OWN", job(), stream=ofdg.STREAM_OWN)  # a fresh context: no call has worked on an internal stream yet
    refused("job", None)
    refused("n_samples", job(), n=0)
    for bad_w, bad_h in ((100, 48), (96, 47), (0, 48), (4, 2)):
        refused("width", job(width=bad_w, height=bad_h))
    refused("2^32", job(width=65536, height=21846), n=1)
    refused("src_fmt", job(src_fmt=ofdg.FMT_F16))
    refused("dst_fmt", job(dst_fmt=7))
    refused("flow_fmt", job(flow_fmt=ofdg.FMT_U8))
    refused("flags", job(flags=1))
    refused("reserved", job(reserved={1: 1}))
    for bad in (0, 17):
        refused("taps_side", job(taps_side=bad))
    refused("no frame is set", job(src={0: None, 1: None}, dst={0: None, 1: None}, flow={0: None, 1: None}))
    refused("flow: a frame is incomplete", job(flow={1: None}))
    refused("dst: a frame is incomplete", job(dst={0: None}))
    refused("src: a frame is incomplete", job(src={1: None}))
    refused("prob", job(recs=None, prob=2.0))
    refused("shutter_max", job(recs=None, shutter_max=2.5))
    refused("shutter_min must not be above", job(recs=None, shutter_min=1.5))
    refused("pair_shutter", job(recs=None, pair_shutter=float("nan")))
    refused("src[0] must be 16-byte aligned (float32)", job(src={0: srcs[0].data_ptr() + 4}))
    refused("src[1] must be 4-byte aligned (uint8)", job(src={1: srcs[1].data_ptr() + 2}, src_fmt=ofdg.FMT_U8))
    refused("flow[0] must be 16-byte aligned (float32)", job(flow={0: flows[0].data_ptr() + 8}))
    refused("flow[1] must be 8-byte aligned (binary16)", job(flow={1: flows[1].data_ptr() + 4}, flow_fmt=ofdg.FMT_F16))
    refused("dst[0] must be 16-byte", job(dst={0: dsts[0][1].data_ptr() + 8}))
    refused("dst[1] must be 16-byte", job(dst={1: dsts[1][1].data_ptr() + 4}, dst_fmt=ofdg.FMT_U8))
    refused("recs must", job(recs=recs.data_ptr() + 8))
    refused("recs_out", job(recs_out=rout.data_ptr() + 4))
    refused("overlaps", job(dst={0: srcs[0].data_ptr()}))
    refused("overlaps", job(dst={1: dsts[0][1].data_ptr() + 16}))
    refused("overlaps", job(dst={0: flows[1].data_ptr() + 16}))
    refused("overlaps", job(recs_out=recs.data_ptr()))
    refused("overlaps", job(recs_out=dsts[1][1].data_ptr() + 32))
    # a valid call on the same context still works, also on OFDG_STREAM_OWN once a call has been made
    outs, ex = ofdg.alloc_outputs(B, H, W), ofdg.alloc_extras(B, H, W)
    torch.cuda.synchronize()
    g.forward(*outs, ofdg.STREAM_OWN, extras=ex)
    g.motion_blur(outs[:2], (dsts[0][1], dsts[1][1]), flow=(outs[2], ex["flow1"]), recs=recs, recs_out=rout, taps_side=8, stream=ofdg.STREAM_OWN)
    g.synchronize(ofdg.STREAM_OWN)
    torch.cuda.synchronize()
    base = host_planes(dict(zip(PLANES, outs), **ex))
    want, used = blur_host(ofdg, base, recs=recs.cpu().numpy(), taps_side=8)
    mr.expect_equal(to_host((dsts[0][1], dsts[1][1])), want, "after the refusals")
    assert mr.equal_bits(rout.cpu().numpy(), used) and used.tolist() == [[1.0, 2.0, 0.0, 0.0]] * B and guards_intact(everything)
