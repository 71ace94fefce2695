"""GPU tests of the occluder rectangles (ofdg_erase, include/ofdg.h): the device planes against ofdg_host_erase and against the
numpy restatement (tests/erase_reference.py), byte for byte - every format, fill and size, between guard bytes, twice, with a
dirty workspace; behind forward_counter, the crop and the spatial step without synchronisation, in mode 9, with three calls in
flight, through the loader - and the refusals."""
import ctypes as C

import numpy as np
import pytest

import erase_reference as er

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 64  # bytes in front of and behind every written plane (keeps the 16-byte alignment)
COLOR = (3, 250, 128)
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
    return torch.from_numpy(np.ascontiguousarray(recs).view(np.int32).reshape(-1, 24)).cuda()


# The reduction takes 32768 elements of a channel per workgroup, the pass over the maps 4096.  8x2: one piece.  24x6, 72x40: one
# workgroup that ends inside a round of its lanes.  264x200: 52800 elements - a second, partial workgroup of the reduction and
# thirteen of the pass, rectangles across their borders - and uint8 rows 8 mod 16 wide, so that the rows of a rectangle start
# at every alignment and the head, body and tail of a row all occur.
@pytest.mark.parametrize("W,H", er.SIZES)
@pytest.mark.parametrize("fill", [er.MEAN, er.CONST, er.NOISE])
@pytest.mark.parametrize("image_dtype,occ_dtype,flow_dtype", [("float32", "float32", "float32"), ("uint8", "uint8", "float16"),
                                                              ("float32", "uint8", "float32"), ("uint8", "float32", "float16"),
                                                              ("float32", "float32", "float16"), ("uint8", "uint8", "float32"),
                                                              ("float32", "uint8", "float16"), ("uint8", "float32", "float32")])
def test_device_equals_host_twin_and_restatement(ofdg, image_dtype, occ_dtype, flow_dtype, fill, W, H):
    """Every written plane lies between 0xA5 guards; the flows and the given records stay as they are.  Frame 1 only, then both
    frames; given records (none / one / four rectangles, then the 1x1, border and corner ones), then drawn ones.  Each call runs
    twice on the same inputs, the second time with the workspace filled with 0xA5."""
    import torch
    g = make_gen(ofdg, 64, 32)  # (the context's own frame is another: the job gives the size)
    images, occ, flow = er.frames(W, H, image_dtype), er.maps(W, H, occ_dtype), er.flows(W, H, flow_dtype)
    ranges = dict(prob=0.8, min_rects=0, max_rects=4, min_size=1, max_size=max(W // 2, 1))
    what = "%dx%d %s %s %s fill %d" % (W, H, image_dtype, occ_dtype, flow_dtype, fill)
    dflow = to_dev(flow)
    calls = [dict(recs=er.records(W, H), frames=(1,)), dict(recs=er.records(W, H), frames=(0, 1)), dict(recs=er.records_edges(W, H), frames=(0, 1)),
             dict(ranges=ranges, first_index=2 ** 32 - 1, frames=(0, 1))]
    for kw in calls:
        kw = dict(kw, seed=11, fill=fill, color=COLOR)
        want = er.erase(images, occ, flow, **kw)
        h_img, h_occ = [np.array(t) for t in images], [np.array(t) for t in occ]
        host_recs = ofdg.host_erase(h_img, h_occ, [np.array(t) for t in flow], **kw)
        results = []
        for dirty in (False, True):
            bufs = [guarded(t) for t in images + occ]
            wraw, work = guarded(np.full((er.N, 64), FILL if dirty else 0, np.uint8))
            rraw, rout = guarded(np.full((er.N, 24), -1, np.int32))
            drecs = dev_recs(kw["recs"]) if "recs" in kw else None
            dkw = dict(kw, recs=drecs)
            g.erase((bufs[0][1], bufs[1][1]), (bufs[2][1], bufs[3][1]), dflow, recs_out=rout, work=work, size=(H, W), **dkw)
            torch.cuda.synchronize()
            got = (to_host((bufs[0][1], bufs[1][1])), to_host((bufs[2][1], bufs[3][1])), ofdg.erase_numpy(rout))
            assert guards_intact(bufs + [(wraw, work), (rraw, rout)]), what
            if drecs is not None:
                assert er.equal_bits(ofdg.erase_numpy(drecs), kw["recs"]), what
            results.append(got)
        for got in results:
            er.expect_equal(got[0], want[0], what + ": images against the restatement")
            er.expect_equal(got[1], want[1], what + ": maps against the restatement")
            er.expect_equal(got[0], h_img, what + ": images against ofdg_host_erase")
            er.expect_equal(got[1], h_occ, what + ": maps against ofdg_host_erase")
            assert er.equal_bits(got[2], want[2]) and er.equal_bits(got[2], host_recs), "%s: records\n%s\n%s" % (what, got[2], want[2])
    er.expect_equal(to_host(dflow), flow, what + ": the flows")


@pytest.mark.parametrize("image_dtype", ["float32", "uint8"])
def test_subsets_of_planes(ofdg, image_dtype):
    """Frame 0 only with both maps; frame 1 only with occ0 alone and image0 absent; no marking: the maps are not touched."""
    import torch
    W, H = 264, 200
    g = make_gen(ofdg, W, H)
    images, occ, flow = er.frames(W, H, image_dtype), er.maps(W, H, "uint8"), er.flows(W, H, "float16")
    work, rout = ofdg.alloc_erase(er.N)
    recs = er.records_edges(W, H)
    for sel_img, sel_occ, sel_flow, kw in (((0, 1), (0, 1), (0, 1), dict(frames=(0,))), ((1,), (0,), (0,), dict(frames=(1,))),
                                           ((0, 1), (0, 1), (), dict(frames=(0, 1), mark_occ=False))):
        pick = lambda planes, sel: tuple(planes[f] if f in sel else None for f in range(2))  # noqa: E731
        h_img, h_occ = [None if t is None else np.array(t) for t in pick(images, sel_img)], [None if t is None else np.array(t) for t in pick(occ, sel_occ)]
        used = ofdg.host_erase(h_img, h_occ, pick(flow, sel_flow), recs=recs, fill=er.MEAN, **kw)
        d_img, d_occ = to_dev(pick(images, sel_img)), to_dev(pick(occ, sel_occ))
        g.erase(d_img, d_occ, to_dev(pick(flow, sel_flow)), recs=dev_recs(recs), recs_out=rout, work=work, **kw)
        torch.cuda.synchronize()
        er.expect_equal(to_host(d_img), h_img, str(kw))
        er.expect_equal(to_host(d_occ), h_occ, str(kw) + " maps")
        assert er.equal_bits(ofdg.erase_numpy(rout), used)
        if kw.get("mark_occ") is False:
            er.expect_equal(h_occ, occ, "not marked")


def rendered(ofdg, g, B, compact, first_index, then=None):
    """forward_counter with all extras on the internal stream and `then(planes)` behind it, nothing waited for in between"""
    import torch
    W, H = g.params.width, g.params.height
    if compact:
        outs = ofdg.alloc_outputs(B, H, W, image_dtype=torch.uint8, flow_dtype=torch.float16)
        ex = ofdg.alloc_extras(B, H, W, flow_dtype=torch.float16, occ_dtype=torch.uint8)
    else:
        outs = ofdg.alloc_outputs(B, H, W)
        ex = ofdg.alloc_extras(B, H, W)
    src = dict(zip(PLANES, outs), **ex)
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


def erase_host(ofdg, planes, **kw):
    """ofdg_host_erase on copies of the named planes: (planes as erased, records)"""
    p = {k: np.array(v) for k, v in planes.items()}
    used = ofdg.host_erase((p["image0"], p["image1"]), (p.get("occ0"), p.get("occ1")) if "occ0" in p else None, (p["flow"], p.get("flow1")), **kw)
    return p, used


def expect_planes(got, want, what):
    for k in want:
        assert er.equal_bits(got[k], want[k]), "%s: %s differs" % (what, k)


@pytest.mark.parametrize("compact", [False, True])
def test_behind_forward_counter_with_reductions(ofdg, compact):
    """Mode 7 with all extras: the rectangles into both frames and both maps behind forward_counter, the statistics of the
    visible pixels and the pyramid weights behind that - they see the extended occ0."""
    import torch
    W, H, B = 128, 64, 3
    kw = dict(first_index=40, ranges=dict(er.RAFT, prob=1.0, min_size=10, max_size=40), frames=(0, 1), fill=er.MEAN)
    g = make_gen(ofdg, W, H, 7, pool=True, sampler=1, seed=5, batch_size=B)
    plain, _ = rendered(ofdg, g, B, compact, 40)

    def then(src, enqueue, more=None):
        if not enqueue:
            return ofdg.alloc_erase(B) + (ofdg.alloc_flow_stats(B), ofdg.alloc_flow_pyramid(B, H, W, 2, src["flow"].dtype, weights=True))
        work, recs, rows, pyr = more
        g.erase((src["image0"], src["image1"]), (src["occ0"], src["occ1"]), (src["flow"], src["flow1"]), recs_out=recs, work=work, stream=ofdg.STREAM_OWN, **kw)
        g.flow_stats(src["flow"], rows, occ=src["occ0"], visible_only=True, stream=ofdg.STREAM_OWN)
        g.flow_pyramid(src["flow"], 2, occ=src["occ0"], out=pyr, stream=ofdg.STREAM_OWN)

    erased, (work, recs, rows, pyr) = rendered(ofdg, g, B, compact, 40, then)
    base = host_planes(plain)
    want, used = erase_host(ofdg, base, seed=5, **kw)
    expect_planes(host_planes(erased), want, "compact %s" % compact)
    assert er.equal_bits(ofdg.erase_numpy(recs), used) and (used["count"] >= 1).all()
    assert (want["occ0"] != base["occ0"]).any() and (want["occ1"] != base["occ1"]).any() and (want["image1"] != base["image1"]).any()
    assert er.equal_bits(want["flow"], base["flow"]) and er.equal_bits(want["label0"], base["label0"])
    import flow_stats_reference as fsr
    import flow_pyramid_reference as fpr
    fsr.expect_equal(ofdg.flow_stats_numpy(rows)["rows"], fsr.rows_of(ofdg.host_flow_stats(want["flow"], want["occ0"], 2.0, visible_only=True)), "statistics")
    lv, wt = ofdg.host_flow_pyramid(want["flow"], 2, want["occ0"], weights=True)
    fpr.expect_equal([t.cpu().numpy() for t in pyr[1]], wt, "pyramid weights")
    assert not all(np.array_equal(a, b) for a, b in zip(wt, ofdg.host_flow_pyramid(base["flow"], 2, base["occ0"], weights=True)[1]))


def test_behind_crop_and_spatial(ofdg):
    """128x64 to 96x48 on OFDG_STREAM_OWN: forward_counter, the crop (then the spatial step) and the rectangles on its planes."""
    import torch
    W, H, B, ow, oh = 128, 64, 3, 96, 48
    kw = dict(first_index=8, ranges=dict(er.RAFT, prob=1.0, min_size=8, max_size=30), frames=(1,), fill=er.NOISE)
    for step in ("crop", "spatial"):
        g = make_gen(ofdg, W, H, 7, pool=True, sampler=1, seed=6, batch_size=B)

        def then(src, enqueue, more=None):
            if not enqueue:
                dst = ofdg.alloc_crop(src, oh, ow) if step == "crop" else ofdg.alloc_spatial(src, oh, ow)
                return dst, ofdg.alloc_erase(B)
            dst, (work, recs) = more
            if step == "crop":
                g.crop(src, dst, first_index=8, occ_window=True, stream=ofdg.STREAM_OWN)
            else:
                g.spatial(src, dst, first_index=8, ranges=ofdg.SPATIAL_FLOWNET, occ_window=True, stream=ofdg.STREAM_OWN)
            g.erase((dst["image0"], dst["image1"]), (dst["occ0"], dst["occ1"]), (dst["flow"], dst["flow1"]), recs_out=recs, work=work,
                    stream=ofdg.STREAM_OWN, size=(oh, ow), **kw)

        # the un-erased planes of the same step: once without the rectangles
        def only(src, enqueue, more=None):
            if not enqueue:
                return ofdg.alloc_crop(src, oh, ow) if step == "crop" else ofdg.alloc_spatial(src, oh, ow)
            if step == "crop":
                g.crop(src, more, first_index=8, occ_window=True, stream=ofdg.STREAM_OWN)
            else:
                g.spatial(src, more, first_index=8, ranges=ofdg.SPATIAL_FLOWNET, occ_window=True, stream=ofdg.STREAM_OWN)

        _, plain = rendered(ofdg, g, B, False, 8, only)
        _, (dst, (work, recs)) = rendered(ofdg, g, B, False, 8, then)
        base = host_planes(plain)
        want, used = erase_host(ofdg, base, seed=6, **kw)
        expect_planes(host_planes(dst), want, step)
        assert er.equal_bits(ofdg.erase_numpy(recs), used) and (want["occ0"] != base["occ0"]).any() and (want["image1"] != base["image1"]).any()
        assert er.equal_bits(want["image0"], base["image0"])


def test_mode_9_without_maps(ofdg):
    import torch
    W, H, B = 128, 64, 2
    g = make_gen(ofdg, W, H, 9, pool=True, sampler=1, seed=3, batch_size=B)
    g.warp_generate(1, 3)
    kw = dict(first_index=0, ranges=dict(er.RAFT, prob=1.0, min_size=8, max_size=30), frames=(0, 1), fill=er.CONST, color=COLOR)
    both = []
    for erase in (False, True):
        outs = ofdg.alloc_outputs(B, H, W)
        recs = torch.zeros((B, 24), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        g.forward_counter(0, B, *outs, ofdg.STREAM_OWN)
        if erase:
            g.erase(outs[:2], recs_out=recs, stream=ofdg.STREAM_OWN, **kw)
        g.synchronize(ofdg.STREAM_OWN)
        torch.cuda.synchronize()
        both.append((to_host(outs), ofdg.erase_numpy(recs)))
    base = [np.array(t) for t in both[0][0][:2]]
    used = ofdg.host_erase(base, seed=3, **kw)
    er.expect_equal(both[1][0][:2], base, "mode 9")
    assert er.equal_bits(both[1][1], used) and er.equal_bits(both[1][0][2], both[0][0][2]) and not er.equal_bits(base[0], both[0][0][0])


def test_three_calls_in_flight(ofdg):
    """Two calls on two caller streams and one on OFDG_STREAM_OWN, each with its own workspace and records, one wait at the end."""
    import torch
    W, H, B = 128, 64, 2
    g = make_gen(ofdg, W, H, 7, pool=True)
    users = [torch.cuda.Stream(), torch.cuda.Stream()]
    batches = [g.sample(B) for _ in range(3)]
    kw = lambda k: dict(first_index=100 * k, seed=9, ranges=dict(er.RAFT, prob=1.0, min_size=8, max_size=30), frames=(0, 1))  # noqa: E731
    plain = []
    for tasks, bps, n in batches:
        outs, ex = ofdg.alloc_outputs(B, H, W), ofdg.alloc_extras(B, H, W)
        torch.cuda.synchronize()
        g.render(tasks, B, bps, n, *outs, 0, extras=ex)
        g.synchronize(0)
        torch.cuda.synchronize()
        plain.append(host_planes(dict(zip(PLANES, outs), **ex)))
    sets = [(ofdg.alloc_outputs(B, H, W), ofdg.alloc_extras(B, H, W), ofdg.alloc_erase(B)) for _ in range(3)]
    torch.cuda.synchronize()
    streams = [users[0].cuda_stream, users[1].cuda_stream, ofdg.STREAM_OWN]
    for k, ((tasks, bps, n), (o, ex, (work, recs)), st) in enumerate(zip(batches, sets, streams)):
        g.render(tasks, B, bps, n, *o, st, extras=ex)
        g.erase(o[:2], (ex["occ0"], ex["occ1"]), (o[2], ex["flow1"]), recs_out=recs, work=work, stream=st, **kw(k))
    for st in streams:
        g.synchronize(st)
    torch.cuda.synchronize()
    for k, (o, ex, (work, recs)) in enumerate(sets):
        want, used = erase_host(ofdg, plain[k], **kw(k))
        expect_planes(host_planes(dict(zip(PLANES, o), **ex)), want, "call %d" % k)
        assert er.equal_bits(ofdg.erase_numpy(recs), used)
    assert not er.equal_bits(ofdg.erase_numpy(sets[0][2][1]), ofdg.erase_numpy(sets[1][2][1]))


def test_flowloader_erase(ofdg):
    import torch
    import flow_stats_reference as fsr
    import flow_pyramid_reference as fpr
    W, H, B, cw, ch = 128, 96, 2, 96, 48
    kw = dict(width=W, height=H, mode=7, batch_size=B, sampler=1, seed=21)
    pool = lambda g: g.pool_synthetic(3, 2 * W, 2 * H, 11)  # noqa: E731
    extras = ("flow1", "occ0", "occ1", "label0", "label1")
    opts = dict(extras=extras, crop=(ch, cw), photo=ofdg.PHOTO_FLOWNET, stats=True, pyramid=2, pyramid_weights=True)
    make = lambda **more: ofdg.FlowLoader(ofdg.default_params(**kw), pool=pool, prefetch=3, **dict(opts, **more))  # noqa: E731
    erase = dict(er.RAFT, prob=1.0, min_size=8, max_size=30, frames=(0, 1))
    ranges = {k: v for k, v in erase.items() if k in ofdg.ERASE_RANGES}
    first, plain = iter(make(erase=erase)), iter(make())
    last = None
    for step in range(3):
        a, p = next(first), next(plain)
        torch.cuda.current_stream().synchronize()
        assert set(a[3]) == set(p[3]) | {"erase"} and a[3]["erase"].dtype == torch.int32 and tuple(a[3]["erase"].shape) == (B, 24)
        index = ofdg.shard_first_index(step, B, 1, 0)
        base = dict(zip(PLANES, to_host(p[:3])), **{k: p[3][k].cpu().numpy() for k in extras})
        want, used = erase_host(ofdg, base, first_index=index, seed=21, ranges=ranges, frames=(0, 1))
        got = dict(zip(PLANES, to_host(a[:3])), **{k: a[3][k].cpu().numpy() for k in extras})
        expect_planes(got, want, "batch %d" % step)
        assert er.equal_bits(ofdg.erase_numpy(a[3]["erase"]), used) and (used["count"] >= 1).all()
        assert torch.equal(a[3]["crop"], p[3]["crop"]) and torch.equal(a[3]["photo"], p[3]["photo"]) and (want["occ0"] != base["occ0"]).any()
        # the reductions ran behind the rectangles: they are those of the extended occ0
        fsr.expect_equal(ofdg.flow_stats_numpy(a[3]["flow_stats"])["rows"], fsr.rows_of(ofdg.host_flow_stats(want["flow"], want["occ0"], 2.0)), "statistics")
        _, wt = ofdg.host_flow_pyramid(want["flow"], 2, want["occ0"], weights=True)
        fpr.expect_equal([t.cpu().numpy() for t in a[3]["flow_pyramid_weights"]], wt, "pyramid weights")
        rows_a, rows_p = ofdg.flow_stats_numpy(a[3]["flow_stats"])["rows"], ofdg.flow_stats_numpy(p[3]["flow_stats"])["rows"]
        assert (rows_a["n_occluded"] > rows_p["n_occluded"]).all()
        last = (got, used)
    resumed = next(iter(make(erase=erase, start=2)))
    torch.cuda.current_stream().synchronize()
    assert er.equal_bits(ofdg.erase_numpy(resumed[3]["erase"]), last[1])
    expect_planes(dict(zip(PLANES, to_host(resumed[:3])), occ0=resumed[3]["occ0"].cpu().numpy()), {k: last[0][k] for k in PLANES + ("occ0",)}, "resumed")
    # without erase= the loader yields what it yielded before: a plain tuple without extras, the same dict with them
    bare = next(iter(ofdg.FlowLoader(ofdg.default_params(**kw), pool=pool, prefetch=3)))
    assert len(bare) == 3
    x = next(iter(ofdg.FlowLoader(ofdg.default_params(**kw), pool=pool, prefetch=3, extras=("occ0",))))
    assert set(x[3]) == {"occ0"}
    # without a crop, ERASE_RAFT as it is, frame 1 into the ring's own frames
    it = iter(ofdg.FlowLoader(ofdg.default_params(**kw), pool=pool, prefetch=3, erase=ofdg.ERASE_RAFT))
    b0 = next(it)
    torch.cuda.current_stream().synchronize()
    assert set(b0[3]) == {"erase"} and torch.equal(b0[0], bare[0]) and torch.equal(b0[2], bare[2])
    for bad, word in ((dict(erase=dict(size=3)), "unknown erase"), (dict(erase=dict(ofdg.ERASE_RAFT, mark_occ=True), extras=("flow1",)), "occlusion map"),
                      (dict(erase=dict(ofdg.ERASE_RAFT, frames=(0, 1)), extras=("occ0", "occ1")), "flow1"), (dict(erase=dict(frames=(3,))), "frames")):
        with pytest.raises(ValueError, match=word):
            ofdg.FlowLoader(ofdg.default_params(**kw), pool=pool, prefetch=3, **bad)


def test_refusals_enqueue_nothing(ofdg):
    import torch
    W, H, B = 128, 96, 2
    g = make_gen(ofdg, W, H, 7, pool=True, batch_size=B)
    # (maps and flows in buffers of the float32 size, so that the jobs below that call them float32 stay inside them)
    bufs = [guarded(np.zeros((B, 3, H, W), np.float32)) for _ in range(2)] + [guarded(np.zeros((B, 1, H, W), np.float32)) for _ in range(2)]
    flows = [torch.zeros((B, 2, H, W), dtype=torch.float32, device="cuda") for _ in range(2)]
    wraw, work = guarded(np.full((B, 64), FILL, np.uint8))
    rraw, rout = guarded(np.full((B, 24), -1, np.int32))
    recs = dev_recs(er.records(W, H)[1:])
    everything = bufs + [(wraw, work), (rraw, rout)]
    before = [raw.clone() for raw, _ in everything]
    torch.cuda.synchronize()
    lib, vp = ofdg.lib(), C.c_void_p

    def job(**kw):
        j = ofdg.EraseJob()
        for f in range(2):
            j.image[f], j.occ[f], j.flow[f] = bufs[f][1].data_ptr(), bufs[2 + f][1].data_ptr(), flows[f].data_ptr()
        j.recs, j.recs_out, j.work = recs.data_ptr(), rout.data_ptr(), work.data_ptr()
        j.image_fmt, j.occ_fmt, j.flow_fmt = ofdg.FMT_F32, ofdg.FMT_U8, ofdg.FMT_F16
        j.flags, j.fill = ofdg.ERASE_FRAME0 | ofdg.ERASE_FRAME1 | ofdg.ERASE_OCC, ofdg.ERASE_MEAN
        for k, v in kw.items():
            if isinstance(v, dict):
                for idx, val in v.items():
                    getattr(j, k)[idx] = val
            else:
                setattr(j, k, v)
        return j

    def refused(word, j, n=B, stream=0):
        rc = lib.ofdg_erase(g.h, None if j is None else C.byref(j), n, vp(stream))
        assert rc == ofdg.EINVAL, word
        msg = lib.ofdg_last_error(g.h).decode()
        assert msg.startswith("ofdg_erase: ") and word in msg, (word, msg)
        g.synchronize()
        torch.cuda.synchronize()
        assert all(torch.equal(raw, b) for (raw, _), b in zip(everything, before)), word

    refused("OFDG_STREAM_OWN", job(), stream=ofdg.STREAM_OWN)  # a fresh context: no call has worked on an internal stream yet
    refused("job", None)
    refused("n_samples", job(), n=0)
    for bad_w, bad_h in ((100, 48), (96, 47), (0, 48), (4, 2)):
        refused("width", job(width=bad_w, height=bad_h))
    refused("2^31", job(width=32768, height=32768), n=1)
    refused("image_fmt", job(image_fmt=ofdg.FMT_F16))
    refused("flags holds unknown bits", job(flags=15))
    refused("reserved", job(reserved={1: 1}))
    refused("FRAME0", job(flags=ofdg.ERASE_OCC))
    refused("no frame is set", job(image={0: None, 1: None}))
    refused("fill", job(fill=7))
    refused("prob", job(recs=None, prob=2.0, max_rects=1, min_size=1, max_size=1))
    refused("needs its flow", job(flow={1: None}))
    refused("work is NULL", job(work=None))
    refused("work must be 16-byte", job(work=work.data_ptr() + 8))
    refused("image[0] must be 16-byte aligned (float32)", job(image={0: bufs[0][1].data_ptr() + 4}))
    refused("image[1] must be 4-byte aligned (uint8)", job(image={1: bufs[1][1].data_ptr() + 2}, image_fmt=ofdg.FMT_U8))
    refused("occ[0] must be 4-byte", job(occ={0: bufs[2][1].data_ptr() + 1}))
    refused("occ[1] must be 16-byte", job(occ={1: bufs[3][1].data_ptr() + 4}, occ_fmt=ofdg.FMT_F32))
    refused("flow[0] must be 8-byte", job(flow={0: flows[0].data_ptr() + 4}))
    refused("flow[1] must be 16-byte", job(flow={1: flows[1].data_ptr() + 8}, flow_fmt=ofdg.FMT_F32))
    refused("recs must", job(recs=recs.data_ptr() + 8))
    refused("recs_out", job(recs_out=rout.data_ptr() + 4))
    refused("overlaps", job(image={1: bufs[0][1].data_ptr() + 16}))
    refused("overlaps", job(occ={0: bufs[1][1].data_ptr() + 64}))
    refused("overlaps", job(occ={1: flows[1].data_ptr() + 16}))
    refused("overlaps", job(work=rout.data_ptr()))
    refused("overlaps", job(recs_out=recs.data_ptr()))
    refused("overlaps", job(flow={0: bufs[0][1].data_ptr()}))
    # a valid call on the same context still works, also on OFDG_STREAM_OWN once a call has been made
    outs, ex = ofdg.alloc_outputs(B, H, W), ofdg.alloc_extras(B, H, W)
    torch.cuda.synchronize()
    g.forward(*outs, ofdg.STREAM_OWN, extras=ex)
    g.synchronize(ofdg.STREAM_OWN)
    torch.cuda.synchronize()
    base = host_planes(dict(zip(PLANES, outs), **ex))
    g.erase(outs[:2], (ex["occ0"], ex["occ1"]), (outs[2], ex["flow1"]), recs=recs, recs_out=rout, work=work, frames=(0, 1), stream=ofdg.STREAM_OWN)
    g.synchronize(ofdg.STREAM_OWN)
    torch.cuda.synchronize()
    want, used = erase_host(ofdg, base, recs=er.records(W, H)[1:], frames=(0, 1))
    expect_planes(host_planes(dict(zip(PLANES, outs), **ex)), want, "after the refusals")
    assert er.equal_bits(ofdg.erase_numpy(rout), used) and guards_intact(everything)
