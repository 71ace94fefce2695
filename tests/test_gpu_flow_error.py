"""GPU tests of the flow error (ofdg_flow_error, include/ofdg.h): the device rows, epe plane and picture against
ofdg_host_flow_error and against the numpy restatement (tests/flow_error_reference.py), byte for byte - both ground-truth and
all three estimate formats, the maps, dist2, both layouts, between guard bytes; each output on its own; accumulation and the
one-row form; behind forward_counter, the crop and the boundaries without synchronisation, in mode 9, with three calls in
flight, through the loader - and the refusals."""
import ctypes as C

import numpy as np
import pytest

import flow_error_reference as fe

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 64  # bytes in front of and behind every written plane (keeps the 16-byte alignment)
PLANES = ("image0", "image1", "flow")
ALL = ("rows", "epe", "picture")


def make_gen(ofdg, W, H, mode=7, pool=False, **kw):
    g = ofdg.Generator(ofdg.default_params(width=W, height=H, mode=mode, **kw))
    if pool:
        g.pool_synthetic(3, 2 * W, 2 * H, 11)
    return g


def guarded(array, bf16=False):
    """(the whole uint8 buffer with 0xA5 guards; the tensor holding `array` in its middle); bf16: uint16 bit patterns as a
    bfloat16 tensor"""
    import torch
    array = np.ascontiguousarray(array)
    src = torch.from_numpy(array.view(np.int16) if bf16 else array.copy())
    size = src.numel() * src.element_size()
    raw = torch.full((GUARD + size + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    t = raw[GUARD:GUARD + size].view(src.dtype).view(src.shape)
    t.copy_(src)
    return raw, (t.view(torch.bfloat16) if bf16 else t)


def guards_intact(bufs):
    return all(bool((raw[:GUARD] == FILL).all()) and bool((raw[-GUARD:] == FILL).all()) for raw, _ in bufs)


def outputs(ofdg, n, H, W, layout="planar_bgr", epe_dtype=np.float32, one_row=False):
    """guarded rows, epe and picture, filled with bytes the call must overwrite"""
    rows = guarded(np.full((1 if one_row else n, 672), 0x5A, np.uint8))
    epe = guarded(np.full((n, 1, H, W), 7.0, epe_dtype))
    picture = guarded(np.full(ofdg.flow_vis_shape(n, H, W, layout), 0x5A, np.uint8))
    return rows, epe, picture


def device_bits(t):
    import torch
    return t.view(torch.int16).cpu().numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.cpu().numpy()


# The kernel takes 4096 pixels of a plane per workgroup, a lane 4 pixels: 1024 a round of the 256 lanes.  8x2: 16 pixels, four
# lanes of one wave.  24x6 (144 pixels) and 72x40 (2880): one workgroup that ends inside a round of its lanes - the first, and
# the third.  264x200: 52800 pixels - thirteen workgroups per sample, the last a partial one of 3648 pixels; a row then comes
# from thirteen workgroups' atomics.
@pytest.mark.parametrize("W,H", fe.SIZES)
@pytest.mark.parametrize("est_dtype", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("gt_dtype", ["float32", "float16"])
def test_device_equals_host_twin_and_restatement(ofdg, gt_dtype, est_dtype, W, H):
    """Rows, epe and the picture lie between 0xA5 guards and are filled with other bytes before the call; the inputs stay as
    they are.  Four samples: every special value, all ground truth unusable, the estimate equal to the ground truth, and one
    with its largest error in the last pixel."""
    import torch
    g = make_gen(ofdg, 64, 32)  # (the context's own frame is another: the job gives the size)
    gt, est = fe.inputs(W, H, gt_dtype, est_dtype)
    px = fe.pixels(gt, est)
    graw, dgt = guarded(gt)
    eraw, dest = guarded(est, bf16=est_dtype == "bfloat16")
    maps = {dim: (fe.occ_map(W, H, dim),) + guarded(fe.occ_map(W, H, dim)) for dim in ("uint8", "float32")}
    dist2 = fe.dist2_map(W, H)
    draw, ddist = guarded(dist2)
    for gd, ed, occ_dtype, dist, layout in fe.cases():
        if (gd, ed) != (gt_dtype, est_dtype):
            continue
        occ, oraw, docc = maps[occ_dtype] if occ_dtype else (None, None, None)
        epe_dtype = np.float16 if layout == "hwc_rgb" else np.float32
        kw = dict(layout=layout, dim_occ=occ is not None)
        want = fe.flow_error(gt, est, occ=occ, dist2=dist2 if dist else None, outputs=ALL, epe_dtype=epe_dtype, px=px, **kw)
        host = ofdg.host_flow_error(gt, est, occ=occ, dist2=dist2 if dist else None, outputs=ALL, epe_dtype=epe_dtype, **kw)
        (rraw, rows), (praw, epe), (iraw, picture) = outputs(ofdg, fe.N, H, W, layout, epe_dtype)
        got = g.flow_error(dgt, dest, occ=docc, dist2=ddist if dist else None, rows=rows, epe=epe, picture=picture, size=(H, W), **kw)
        torch.cuda.synchronize()
        tag = "%dx%d gt %s est %s occ %s dist2 %s %s" % (W, H, gt_dtype, est_dtype, occ_dtype, dist, layout)
        assert set(got) == set(ALL) and got["rows"] is rows
        assert guards_intact([(rraw, rows), (praw, epe), (iraw, picture), (graw, dgt), (eraw, dest), (draw, ddist)] + ([(oraw, docc)] if occ_dtype else [])), tag
        assert fe.equal_bits(dgt.cpu().numpy(), gt) and fe.equal_bits(device_bits(dest), est), tag + ": the inputs"
        dev = {"rows": ofdg.flow_error_numpy(rows), "epe": epe.cpu().numpy(), "picture": picture.cpu().numpy()}
        for name in ALL:
            assert fe.equal_bits(dev[name], want[name]), "%s: %s against the restatement" % (tag, name)
            assert fe.equal_bits(dev[name], host[name]), "%s: %s against ofdg_host_flow_error" % (tag, name)
        assert int(dev["rows"]["n_bad_gt"][fe.ALL_BAD_GT]) == W * H and int(dev["rows"]["hist"][fe.EST_IS_GT][0]) == W * H, tag


@pytest.mark.parametrize("only", ALL)
def test_each_output_on_its_own(ofdg, only):
    """Rows only (the kernel without the planes' code), epe only and the picture only (no row is touched): the same bytes as
    in the call that makes all three, at the size of thirteen workgroups a sample."""
    import torch
    W, H = fe.SIZES[3]
    g = make_gen(ofdg, W, H)
    gt, est = fe.inputs(W, H, "float32", "bfloat16")
    occ, dist2 = fe.occ_map(W, H, "uint8"), fe.dist2_map(W, H)
    want = ofdg.host_flow_error(gt, est, occ=occ, dist2=dist2, outputs=ALL, dim_occ=True)
    dgt, dest = torch.from_numpy(gt).cuda(), torch.from_numpy(est.view(np.int16)).cuda().view(torch.bfloat16)
    bufs = dict(zip(ALL, outputs(ofdg, fe.N, H, W)))
    before = {k: raw.clone() for k, (raw, _) in bufs.items()}
    got = g.flow_error(dgt, dest, occ=torch.from_numpy(occ).cuda(), dist2=torch.from_numpy(dist2).cuda(), dim_occ=only == "picture",
                       **{only: bufs[only][1]})
    torch.cuda.synchronize()
    assert list(got) == [only] and guards_intact(bufs.values())
    for k, (raw, t) in bufs.items():
        if k != only:
            assert torch.equal(raw, before[k]), k
    dev = ofdg.flow_error_numpy(bufs["rows"][1]) if only == "rows" else bufs[only][1].cpu().numpy()
    assert fe.equal_bits(dev, want[only])


def test_accumulate_and_one_row(ofdg):
    import torch
    W, H = fe.SIZES[3]
    g = make_gen(ofdg, W, H)
    gt, est = fe.inputs(W, H, "float16", "float16")
    occ, dist2 = fe.occ_map(W, H, "float32"), fe.dist2_map(W, H)
    d = dict(occ=torch.from_numpy(occ).cuda(), dist2=torch.from_numpy(dist2).cuda())
    dgt, dest = torch.from_numpy(gt).cuda(), torch.from_numpy(est).cuda()
    once = ofdg.host_flow_error(gt, est, occ=occ, dist2=dist2)["rows"]
    rows = ofdg.alloc_flow_error(fe.N, H, W)["rows"]
    assert rows.dtype == torch.uint8 and tuple(rows.shape) == (fe.N, 672) and not bool(rows.any())
    g.flow_error(dgt, dest, rows=rows, accumulate=True, **d)   # an all-zero row is the identity
    torch.cuda.synchronize()
    assert fe.equal_bits(ofdg.flow_error_numpy(rows), once)
    g.flow_error(dgt, dest, rows=rows, accumulate=True, **d)
    torch.cuda.synchronize()
    twice = ofdg.flow_error_numpy(rows)
    assert fe.equal_bits(twice, ofdg.host_flow_error(gt, est, occ=occ, dist2=dist2, rows=once.copy(), accumulate=True)["rows"])
    assert np.array_equal(twice["cell"]["n"], 2 * once["cell"]["n"]) and np.array_equal(twice["max_key"], once["max_key"])
    g.flow_error(dgt, dest, rows=rows, **d)   # without the flag the rows are overwritten
    torch.cuda.synchronize()
    assert fe.equal_bits(ofdg.flow_error_numpy(rows), once)
    # all samples into one row, three times: an epoch on the device
    one = ofdg.alloc_flow_error(fe.N, H, W, one_row=True)["rows"]
    assert tuple(one.shape) == (1, 672)
    for _ in range(3):
        g.flow_error(dgt, dest, rows=one, accumulate=True, one_row=True, **d)
    torch.cuda.synchronize()
    want = fe.add_rows(once, plane=W * H)
    epoch = ofdg.flow_error_numpy(one)
    assert int(epoch["max_key"][0]) == int(want["max_key"][0]) and np.array_equal(epoch["cell"]["sum_epe_q8"], 3 * want["cell"]["sum_epe_q8"])
    assert np.array_equal(epoch["hist"], 3 * want["hist"]) and int(epoch["n_bad_gt"][0]) == 3 * int(want["n_bad_gt"][0])
    g.flow_error(dgt, dest, rows=one, one_row=True, **d)
    torch.cuda.synchronize()
    assert fe.equal_bits(ofdg.flow_error_numpy(one), want) and fe.equal_bits(want, ofdg.host_flow_error(gt, est, occ=occ, dist2=dist2, one_row=True)["rows"])
    s = ofdg.flow_error_summary(one)
    assert s["n"] == int(want["cell"]["n"].sum()) and s["hidden"]["n"] + s["visible"]["n"] == s["n"] and s["worst_row"] == 0


def rendered(ofdg, g, B, first_index, then, mode9=False):
    """forward_counter with uint8 frames, a binary16 flow and the uint8 occ0 on the internal stream and `then(planes, True,
    more)` behind it, nothing waited for in between"""
    import torch
    W, H = g.params.width, g.params.height
    outs = ofdg.alloc_outputs(B, H, W, image_dtype=torch.uint8, flow_dtype=torch.float16)
    extras = None if mode9 else ofdg.alloc_extras(B, H, W, ("occ0",), flow_dtype=torch.float16, occ_dtype=torch.uint8)
    src = dict(zip(PLANES, outs), **(extras or {}))
    more = then(src, False, None)
    torch.cuda.synchronize()  # (the allocations were made on torch's stream)
    g.forward_counter(first_index, B, *outs, ofdg.STREAM_OWN, extras=extras)
    then(src, True, more)
    g.synchronize(ofdg.STREAM_OWN)
    torch.cuda.synchronize()
    return src, more


def test_behind_forward_counter_crop_and_boundaries(ofdg):
    """Mode 7 on OFDG_STREAM_OWN at 72x40 behind the crop of a 128x64 frame: the cropped binary16 flow as ground truth, the
    cropped uint8 occ0 and the dist2 plane of the boundaries of that flow.  est = gt: every sum is 0, every counted pixel in
    hist[0], the picture all bin 0.  est = gt + (3, -4): every error exactly 5 px, where gt + the offset is exact."""
    import torch
    W, H, B, cw, ch = 128, 64, 3, 72, 40
    g = make_gen(ofdg, W, H, 7, pool=True, sampler=1, seed=5, batch_size=B)

    def chain(src, enqueue, more):
        if not enqueue:
            return (ofdg.alloc_crop(src, ch, cw), ofdg.alloc_boundaries(B, ch, cw, edge=False),
                    ofdg.alloc_flow_error(B, ch, cw, ALL, layout="hwc_rgb"), ofdg.alloc_flow_error(B, ch, cw, ("rows",)))
        dst, edges, same, _ = more
        g.crop(src, dst, first_index=40, stream=ofdg.STREAM_OWN)
        g.boundaries(dst["flow"], dist2=edges["dist0"], min_step=1.0, stream=ofdg.STREAM_OWN, size=(ch, cw))
        g.flow_error(dst["flow"], dst["flow"], occ=dst["occ0"], dist2=edges["dist0"], layout="hwc_rgb",
                     stream=ofdg.STREAM_OWN, size=(ch, cw), **same)

    _, (dst, edges, same, shifted) = rendered(ofdg, g, B, 40, chain)
    gt, occ, dist2 = dst["flow"].cpu().numpy(), dst["occ0"].cpu().numpy(), edges["dist0"].cpu().numpy()
    assert gt.dtype == np.float16 and occ.dtype == np.uint8 and occ.any() and (dist2 < 26).any() and (dist2 >= 26).any()
    rows = ofdg.flow_error_numpy(same["rows"])
    assert not rows["cell"]["sum_epe_q8"].any() and rows["hist"][:, 0].tolist() == [cw * ch] * B and not rows["hist"][:, 1:].any()
    assert (same["picture"].cpu().numpy() == np.array([49, 54, 149], np.uint8)).all() and not same["epe"].cpu().numpy().any()
    assert (rows["cell"]["n"][:, 1].sum(axis=(1, 2)) == (occ != 0).sum(axis=(1, 2, 3))).all()
    assert (rows["cell"]["n"][:, :, :, 1:].sum(axis=(1, 2, 3)) == (dist2 >= 26).sum(axis=(1, 2, 3))).all()
    assert fe.equal_bits(rows, ofdg.host_flow_error(gt, gt, occ=occ, dist2=dist2)["rows"])
    # the estimate of a second call: a fixed offset, as float32
    est = gt.astype(np.float32) + np.array([3.0, -4.0], np.float32).reshape(1, 2, 1, 1)
    g.flow_error(dst["flow"], torch.from_numpy(est).cuda(), occ=dst["occ0"], dist2=edges["dist0"], size=(ch, cw), **shifted)
    torch.cuda.synchronize()
    rows = ofdg.flow_error_numpy(shifted["rows"])
    assert fe.equal_bits(rows, ofdg.host_flow_error(gt, est, occ=occ, dist2=dist2)["rows"]) and fe.equal_bits(rows, fe.flow_error(gt, est, occ=occ, dist2=dist2)["rows"])
    assert rows["cell"]["n_3px"].sum() == B * cw * ch and not rows["cell"]["n_5px"].any() and rows["hist"][:, 7].tolist() == [cw * ch] * B
    assert rows["cell"]["sum_epe_q8"].sum() == 1280 * B * cw * ch


def test_mode_9(ofdg):
    import torch
    W, H, B = 128, 64, 2
    g = make_gen(ofdg, W, H, 9, pool=True, sampler=1, seed=3, batch_size=B)
    g.warp_generate(1, 3)
    outs = ofdg.alloc_outputs(B, H, W)
    out = ofdg.alloc_flow_error(B, H, W, ALL, epe_dtype=torch.float16)
    est = torch.zeros((B, 2, H, W), dtype=torch.bfloat16, device="cuda")
    torch.cuda.synchronize()
    g.forward_counter(0, B, *outs, ofdg.STREAM_OWN)
    g.flow_error(outs[2], est, stream=ofdg.STREAM_OWN, **out)   # the zero estimate: the error is the flow's length
    g.synchronize(ofdg.STREAM_OWN)
    torch.cuda.synchronize()
    gt = outs[2].cpu().numpy()
    want = ofdg.host_flow_error(gt, np.zeros(gt.shape, np.uint16), outputs=ALL, epe_dtype=np.float16)
    assert fe.equal_bits(ofdg.flow_error_numpy(out["rows"]), want["rows"]) and fe.equal_bits(out["epe"].cpu().numpy(), want["epe"])
    assert fe.equal_bits(out["picture"].cpu().numpy(), want["picture"]) and want["rows"]["cell"]["sum_epe_q8"].sum() > 0


def test_three_calls_in_flight(ofdg):
    """Two calls on two caller streams and one on OFDG_STREAM_OWN, each with its own outputs, one wait at the end."""
    import torch
    W, H, B = 128, 64, 2
    g = make_gen(ofdg, W, H, 7, pool=True)
    users = [torch.cuda.Stream(), torch.cuda.Stream()]
    batches = [g.sample(B) for _ in range(3)]
    est = torch.from_numpy(np.random.RandomState(2).uniform(-4, 4, (B, 2, H, W)).astype(np.float16)).cuda()
    sets = [(ofdg.alloc_outputs(B, H, W), ofdg.alloc_flow_error(B, H, W, ALL)) for _ in range(3)]
    torch.cuda.synchronize()
    streams = [users[0].cuda_stream, users[1].cuda_stream, ofdg.STREAM_OWN]
    for (tasks, bps, n), (o, out), st in zip(batches, sets, streams):
        g.render(tasks, B, bps, n, *o, st)
        g.flow_error(o[2], est, stream=st, **out)
    for st in streams:
        g.synchronize(st)
    torch.cuda.synchronize()
    for k, (o, out) in enumerate(sets):
        want = ofdg.host_flow_error(o[2].cpu().numpy(), est.cpu().numpy(), outputs=ALL)
        assert fe.equal_bits(ofdg.flow_error_numpy(out["rows"]), want["rows"]), "call %d" % k
        assert fe.equal_bits(out["epe"].cpu().numpy(), want["epe"]) and fe.equal_bits(out["picture"].cpu().numpy(), want["picture"]), "call %d" % k
    assert not fe.equal_bits(sets[0][1]["epe"].cpu().numpy(), sets[1][1]["epe"].cpu().numpy())


@pytest.mark.parametrize("flow_scale", [None, 0.05])
def test_flowloader_flow_error(ofdg, flow_scale):
    """FlowLoader.flow_error against host_flow_error of the same batch: the ground truth is the unpacked flow behind the crop,
    with occ0 and the dist0 plane of boundaries=; the estimate is what a network trained on the packed flow would give (the
    packed flow plus noise), scored in pixels through est_scale = 1 / flow_scale; three batches accumulate into one row."""
    import torch
    W, H, B, cw, ch = 128, 96, 2, 96, 48
    kw = dict(width=W, height=H, mode=7, batch_size=B, sampler=1, seed=21)
    pool = lambda g: g.pool_synthetic(3, 2 * W, 2 * H, 11)  # noqa: E731
    more = {} if flow_scale is None else dict(pack=dict(flow_scale=flow_scale))
    loader = ofdg.FlowLoader(ofdg.default_params(**kw), pool=pool, prefetch=3, extras=("occ0",), crop=(ch, cw), boundaries=dict(edge=False, min_step=1.0), **more)
    with pytest.raises(RuntimeError, match="call next"):
        loader.flow_error(torch.zeros((B, 2, ch, cw), device="cuda"))
    it = iter(loader)
    noise = torch.from_numpy(np.random.RandomState(4).uniform(-6, 6, (B, 2, ch, cw)).astype(np.float32)).cuda()
    epoch, want_epoch = None, None
    scale = 1.0 if flow_scale is None else 1.0 / flow_scale
    for step in range(3):
        batch = next(it)
        est = (batch[2] + noise * (flow_scale or 1.0)).to(torch.bfloat16 if step == 1 else torch.float32)
        out = loader.flow_error(est, outputs=ALL, layout="hwc_rgb", dim_occ=True)
        epoch = loader.flow_error(est, rows=epoch, accumulate=epoch is not None, one_row=True)["rows"]
        torch.cuda.current_stream().synchronize()
        t = loader.slots[(loader.k - 1) % loader.prefetch]
        gt, occ, dist2 = t.planes["flow"].cpu().numpy(), batch[3]["occ0"].cpu().numpy(), batch[3]["dist0"].cpu().numpy()
        if flow_scale is not None:
            assert not torch.equal(batch[2], t.planes["flow"])   # (the batch hands out the packed flow; the unpacked one is scored)
        est_host = device_bits(est)
        want = ofdg.host_flow_error(gt, est_host, occ=occ, dist2=dist2, outputs=ALL, layout="hwc_rgb", dim_occ=True, est_scale=scale)
        assert set(out) == set(ALL) and tuple(out["picture"].shape) == (B, ch, cw, 3) and tuple(out["rows"].shape) == (B, 672)
        assert fe.equal_bits(ofdg.flow_error_numpy(out["rows"]), want["rows"]), "batch %d" % step
        assert fe.equal_bits(out["epe"].cpu().numpy(), want["epe"]) and fe.equal_bits(out["picture"].cpu().numpy(), want["picture"]), "batch %d" % step
        one = ofdg.host_flow_error(gt, est_host, occ=occ, dist2=dist2, one_row=True, est_scale=scale, rows=want_epoch, accumulate=want_epoch is not None)
        want_epoch = one["rows"]
        s = ofdg.flow_error_summary(out["rows"])
        assert s["n"] == B * cw * ch and 1.0 < s["epe"] < 8.0 and s["distance"][0] is not None and s["hidden"] is not None
    assert tuple(epoch.shape) == (1, 672) and fe.equal_bits(ofdg.flow_error_numpy(epoch), want_epoch)
    assert int(ofdg.flow_error_numpy(epoch)["cell"]["n"].sum()) == 3 * B * cw * ch
    for bad, word in ((torch.zeros((B, 2, ch, cw + 8), device="cuda"), "est must be"), (torch.zeros((B, 2, ch, cw), dtype=torch.float64, device="cuda"), "est must be"),
                      (torch.zeros((B, 2, ch, cw)), "est must be a tensor on")):
        with pytest.raises(ValueError, match=word):
            loader.flow_error(bad)
    with pytest.raises(ValueError, match="unknown flow_error option"):
        loader.flow_error(est, percentile=99)
    with pytest.raises(ValueError, match="accumulate=True needs rows"):
        loader.flow_error(est, accumulate=True)
    assert loader.flow_error(est, est_scale=scale)["rows"].shape == (B, 672)
    torch.cuda.synchronize()


def test_refusals_enqueue_nothing(ofdg):
    import torch
    W, H, B = 128, 96, 2
    g = make_gen(ofdg, W, H, 7, pool=True, batch_size=B)
    graw, gt = guarded(np.zeros((B, 2, H, W), np.float32))
    eraw, est = guarded(np.zeros((B, 2, H, W), np.float32))
    oraw, occ = guarded(np.zeros((B, 1, H, W), np.uint8))
    draw, dist2 = guarded(np.full((B, 1, H, W), 255, np.uint8))
    (rraw, rows), (praw, epe), (iraw, picture) = outputs(ofdg, B, H, W)
    everything = [(graw, gt), (eraw, est), (oraw, occ), (draw, dist2), (rraw, rows), (praw, epe), (iraw, picture)]
    before = [raw.clone() for raw, _ in everything]
    torch.cuda.synchronize()
    lib, vp = ofdg.lib(), C.c_void_p

    def job(**kw):
        j = ofdg.FlowErrorJob()
        j.gt, j.est, j.occ, j.dist2 = gt.data_ptr(), est.data_ptr(), occ.data_ptr(), dist2.data_ptr()
        j.rows, j.epe, j.picture = rows.data_ptr(), epe.data_ptr(), picture.data_ptr()
        j.gt_fmt, j.est_fmt, j.occ_fmt, j.epe_fmt, j.est_scale = ofdg.FMT_F32, ofdg.FMT_F32, ofdg.FMT_U8, ofdg.FMT_F32, 1.0
        j.speed_px[0], j.speed_px[1], j.dist2_edge[0], j.dist2_edge[1] = 10.0, 40.0, 26, 101
        for k, v in kw.items():
            if isinstance(v, dict):
                for idx, val in v.items():
                    getattr(j, k)[idx] = val
            else:
                setattr(j, k, v)
        return j

    def refused(word, j, n=B, stream=0):
        rc = lib.ofdg_flow_error(g.h, None if j is None else C.byref(j), n, vp(stream))
        assert rc == ofdg.EINVAL, word
        msg = lib.ofdg_last_error(g.h).decode()
        assert msg.startswith("ofdg_flow_error: ") and word in msg, (word, msg)
        g.synchronize()
        torch.cuda.synchronize()
        assert all(torch.equal(raw, b) for (raw, _), b in zip(everything, before)), word

    refused("OFDG_STREAM_OWN", job(), stream=ofdg.STREAM_OWN)  # a fresh context: no call has worked on an internal stream yet
    refused("job", None)
    refused("gt is NULL", job(gt=None))
    refused("est is NULL", job(est=None))
    refused("no output", job(rows=None, epe=None, picture=None))
    refused("n_samples", job(), n=0)
    for bad_w, bad_h in ((100, 48), (96, 47), (0, 48), (4, 2)):
        refused("width", job(width=bad_w, height=bad_h))
    refused("3 * width * height", job(width=65536, height=32768), n=1)
    refused("OFDG_ERR_ONE_ROW needs", job(width=65536, height=21844, flags=ofdg.ERR_ONE_ROW), n=4)
    refused("gt_fmt", job(gt_fmt=ofdg.FMT_BF16))
    refused("est_fmt", job(est_fmt=ofdg.FMT_U8))
    refused("occ_fmt", job(occ_fmt=ofdg.FMT_F16))
    refused("epe_fmt", job(epe_fmt=ofdg.FMT_U8))
    refused("layout", job(layout=2))
    refused("flags", job(flags=8))
    refused("reserved", job(reserved={4: 1}))
    refused("OFDG_ERR_DIM_OCC needs occ", job(occ=None, flags=ofdg.ERR_DIM_OCC))
    refused("OFDG_ERR_DIM_OCC needs picture", job(picture=None, flags=ofdg.ERR_DIM_OCC))
    for bad in (float("nan"), 0.0, 2.0 ** -11, -(2.0 ** 11)):
        refused("est_scale", job(est_scale=bad))
    refused("speed_px", job(speed_px={0: 0.0}))
    refused("speed_px", job(speed_px={1: float("nan")}))
    refused("speed_px", job(speed_px={0: 50.0}))
    refused("dist2_edge", job(dist2_edge={0: 0}))
    refused("dist2_edge", job(dist2_edge={1: 256}))
    refused("gt must be 16-byte aligned", job(gt=gt.data_ptr() + 8))
    refused("gt must be 8-byte aligned", job(gt=gt.data_ptr() + 4, gt_fmt=ofdg.FMT_F16))
    refused("est must be 16-byte aligned", job(est=est.data_ptr() + 8))
    refused("est must be 8-byte aligned", job(est=est.data_ptr() + 4, est_fmt=ofdg.FMT_BF16))
    refused("occ must be 4-byte aligned", job(occ=occ.data_ptr() + 2))
    refused("occ must be 16-byte aligned", job(occ=gt.data_ptr() + 4, occ_fmt=ofdg.FMT_F32))  # (two read ranges may meet)
    refused("dist2 must be 4-byte aligned", job(dist2=dist2.data_ptr() + 1))
    refused("rows must be 8-byte aligned", job(rows=rows.data_ptr() + 4))
    refused("epe must be 16-byte aligned", job(epe=epe.data_ptr() + 8))
    refused("picture must be 16-byte aligned", job(picture=picture.data_ptr() + 4))
    refused("overlaps", job(epe=gt.data_ptr() + 16))
    refused("overlaps", job(picture=occ.data_ptr()))
    refused("overlaps", job(rows=dist2.data_ptr() + 8))
    refused("overlaps", job(rows=picture.data_ptr() + 64))
    refused("overlaps", job(picture=est.data_ptr() + 4 * 2 * B * H * W - 16))
    with pytest.raises(ValueError, match="est must be"):
        g.flow_error(gt, est[:, :1], rows=rows)
    with pytest.raises(ValueError, match="rows must be"):
        g.flow_error(gt, est, rows=rows, one_row=True)
    with pytest.raises(ofdg.OfdgError, match="no output"):
        g.flow_error(gt, est)
    # a valid call on the same context still works, also on OFDG_STREAM_OWN once a call has been made
    outs = ofdg.alloc_outputs(B, H, W)
    torch.cuda.synchronize()
    g.forward(*outs, ofdg.STREAM_OWN)
    g.flow_error(outs[2], est, occ=occ, dist2=dist2, rows=rows, epe=epe, picture=picture, stream=ofdg.STREAM_OWN)
    g.synchronize(ofdg.STREAM_OWN)
    torch.cuda.synchronize()
    want = ofdg.host_flow_error(outs[2].cpu().numpy(), np.zeros((B, 2, H, W), np.float32), occ=occ.cpu().numpy(), dist2=dist2.cpu().numpy(), outputs=ALL)
    assert fe.equal_bits(ofdg.flow_error_numpy(rows), want["rows"]) and fe.equal_bits(epe.cpu().numpy(), want["epe"])
    assert fe.equal_bits(picture.cpu().numpy(), want["picture"]) and guards_intact(everything)
