"""GPU tests of the network-ready packing (ofdg_pack, include/ofdg.h): the device planes against ofdg_host_pack and against
the numpy restatement (tests/pack_reference.py), byte for byte - every format pair, layout, flag and constant set, between
guard bytes; the channels-last property and the eager torch restatement; behind a forward call, the crop and the photometric
step without synchronisation; three calls in flight; through the loader - and the device's refusals."""
import ctypes as C

import numpy as np
import pytest

import pack_reference as pk

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 64  # bytes in front of and behind every destination (keeps the 16-byte alignment)
TORCH = {"float32": "float32", "float16": "float16", "bfloat16": "bfloat16", "uint8": "uint8"}


def make_gen(ofdg, W, H, mode=7, pool=False, **kw):
    g = ofdg.Generator(ofdg.default_params(width=W, height=H, mode=mode, **kw))
    if pool:
        g.pool_synthetic(3, 2 * W, 2 * H, 11)
    return g


def guarded(n, c, H, W, dtype, layout):
    """(the whole uint8 buffer, filled with 0xA5; the logical [n,c,H,W] tensor of `dtype` in its middle, in the layout's memory)"""
    import torch
    dtype = getattr(torch, dtype)
    size = n * c * H * W * torch.empty((), dtype=dtype).element_size()
    raw = torch.full((GUARD + size + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    flat = raw[GUARD:GUARD + size].view(dtype)
    return raw, flat.view(n, H, W, c).permute(0, 3, 1, 2) if layout == pk.NHWC else flat.view(n, c, H, W)


def guards_intact(bufs):
    return all(bool((raw[:GUARD] == FILL).all()) and bool((raw[-GUARD:] == FILL).all()) for raw, _ in bufs)


def to_dev(planes):
    import torch
    return {k: torch.from_numpy(np.array(t)).cuda() for k, t in planes.items()}


def to_host(planes):
    """numpy arrays with the tensors' logical shapes and memory orders; bfloat16 as uint16 bit patterns"""
    import torch
    out = {}
    for k, t in planes.items():
        t = t.view(torch.int16) if t.dtype == torch.bfloat16 else t
        nhwc = t.dim() == 4 and not t.is_contiguous()
        a = (t.permute(0, 2, 3, 1) if nhwc else t).cpu().numpy()
        a = a.view(np.uint16) if planes[k].dtype == torch.bfloat16 else a
        out[k] = a.transpose(0, 3, 1, 2) if nhwc else a
    return out


def host_like(ofdg, src, dst, **kw):
    """ofdg_host_pack of host copies of src into the formats of the device tensors dst"""
    name = lambda t: "bfloat16" if "bfloat16" in str(t.dtype) else str(t.dtype).replace("torch.", "")  # noqa: E731
    image = next((name(t) for k, t in dst.items() if k != "flow"), None)
    return ofdg.host_pack(src, image_dtype=image, flow_dtype=name(dst["flow"]) if "flow" in dst else None, **kw)


# A workgroup is 256 lanes, a lane owns 8 pixels of all channels of its plane group.  8x2: two units.  24x6: three units per row.
# 72x40: 360 units - a second, partial workgroup.  264x200: 33 units per row, 26 workgroups per plane group, the last partial.
@pytest.mark.parametrize("W,H", pk.SIZES)
@pytest.mark.parametrize("layout,concat,rgb", pk.LAYOUTS)
def test_device_equals_host_twin_and_restatement(ofdg, W, H, layout, concat, rgb):
    """The destinations start as 0xA5 bytes between 0xA5 guards: equality shows every element was written, the guards that
    nothing else was.  The sources are unmodified afterwards."""
    import torch
    g = make_gen(ofdg, 64, 32)  # (the context's own frame is another: the job gives the size)
    dev_src = {}
    for k in range(len(pk.CONSTANTS)):
        scale, bias, flow_scale = pk.CONSTANTS[k]
        for image_pair, flow_pair in pk.cases(k):
            src, want = pk.expected(W, H, image_pair, flow_pair, k, layout, concat, rgb)
            kw = dict(scale=scale, bias=bias, flow_scale=flow_scale, layout=layout, concat=concat, rgb=rgb)
            twin = ofdg.host_pack(src, image_dtype=image_pair[1], flow_dtype=flow_pair[1], **kw)
            key = (image_pair[0], flow_pair[0])
            if key not in dev_src:
                dev_src[key] = to_dev(src)
            bufs = {name: guarded(pk.N, t.shape[1], H, W, TORCH[flow_pair[1] if name == "flow" else image_pair[1]], layout) for name, t in want.items()}
            g.pack(dev_src[key], {name: t for name, (_, t) in bufs.items()}, size=(H, W), **kw)
            torch.cuda.synchronize()
            what = "%dx%d %s %s constants %d layout %d concat %d rgb %d" % (W, H, image_pair, flow_pair, k, layout, concat, rgb)
            got = to_host({name: t for name, (_, t) in bufs.items()})
            pk.expect_equal(got, want, layout, what + " against the restatement")
            pk.expect_equal(got, twin, layout, what + " against ofdg_host_pack")
            assert guards_intact(list(bufs.values())), what
    for (image_dtype, flow_dtype), dev in dev_src.items():
        src = pk.sources(W, H, image_dtype, flow_dtype)
        assert all(dev[name].cpu().numpy().tobytes() == src[name].tobytes() for name in src), "the sources"


@pytest.mark.parametrize("layout", [pk.NCHW, pk.NHWC])
@pytest.mark.parametrize("concat", [False, True])
def test_channels_last_and_eager_torch(ofdg, layout, concat):
    """alloc_pack's tensors are logical [n,C,H,W]; with PACK_NHWC they are channels_last memory.  For finite inputs the result
    equals the eager torch restatement (x.float() * s + b).to(dtype) - two kernels, two roundings -, channels flipped and
    concatenated accordingly."""
    import torch
    W, H, n = 72, 40, 3
    g = make_gen(ofdg, W, H)
    scale, bias = ofdg.pack_norm((0.406, 0.456, 0.485), (0.225, 0.224, 0.229))
    rng = np.random.default_rng(3)
    for src_dtype in ("uint8", "float32"):
        for dtype in (torch.float32, torch.float16, torch.bfloat16):
            frames = [torch.from_numpy(rng.integers(0, 256, (n, 3, H, W), dtype=np.uint8) if src_dtype == "uint8"
                                       else rng.uniform(0.0, 255.0, (n, 3, H, W)).astype(np.float32)).cuda() for _ in range(2)]
            flow = torch.from_numpy(rng.normal(0.0, 30.0, (n, 2, H, W)).astype(np.float32)).cuda()
            dst = ofdg.alloc_pack(n, H, W, image_dtype=dtype, flow_dtype=dtype, layout=layout, concat=concat)
            assert set(dst) == ({"image0", "flow"} if concat else {"image0", "image1", "flow"})
            for key, t in dst.items():
                assert tuple(t.shape) == (n, 2 if key == "flow" else 6 if concat else 3, H, W) and t.dtype == dtype
                assert t.is_contiguous(memory_format=torch.channels_last if layout == pk.NHWC else torch.contiguous_format)
            torch.cuda.synchronize()
            g.pack(dict(image0=frames[0], image1=frames[1], flow=flow), dst, scale=scale, bias=bias, flow_scale=0.05, layout=layout, concat=concat,
                   rgb=True)
            torch.cuda.synchronize()
            s = torch.from_numpy(scale).cuda().view(1, 3, 1, 1)
            b = torch.from_numpy(bias).cuda().view(1, 3, 1, 1)
            eager = [((x.float() * s) + b).flip(1).to(dtype) for x in frames]
            if concat:
                assert torch.equal(dst["image0"], torch.cat(eager, 1))
            else:
                assert torch.equal(dst["image0"], eager[0]) and torch.equal(dst["image1"], eager[1])
            assert torch.equal(dst["flow"], (flow * 0.05).to(dtype))


def test_behind_forward_counter(ofdg):
    """forward_counter on the internal stream and the pack behind it, nothing waited for in between: mode 7 with float32 and
    with uint8 / float16 outputs, and mode 9."""
    import torch
    W, H, B = 128, 64, 3
    scale, bias = ofdg.pack_norm((0.406, 0.456, 0.485), (0.225, 0.224, 0.229))
    for mode, image_dtype, flow_dtype in ((7, None, None), (7, torch.uint8, torch.float16), (9, None, None)):
        g = make_gen(ofdg, W, H, mode, pool=True, sampler=1, seed=5, batch_size=B)
        if mode == 9:
            g.warp_generate(1, 3)
        outs = ofdg.alloc_outputs(B, H, W, image_dtype=image_dtype, flow_dtype=flow_dtype)
        src = dict(zip(ofdg.PACK_PLANES, outs))
        kw = dict(scale=scale, bias=bias, flow_scale=0.05, layout=ofdg.PACK_NHWC, concat=True, rgb=True)
        dst = ofdg.alloc_pack(B, H, W, image_dtype=torch.bfloat16, flow_dtype=torch.float16, layout=ofdg.PACK_NHWC, concat=True)
        torch.cuda.synchronize()  # (the allocations were zeroed on torch's stream)
        g.forward_counter(40, B, *outs, ofdg.STREAM_OWN)
        g.pack(src, dst, stream=ofdg.STREAM_OWN, **kw)
        g.synchronize(ofdg.STREAM_OWN)
        torch.cuda.synchronize()
        host = to_host(src)
        assert host["image0"].any() and host["image1"].any() and np.abs(host["flow"].astype(np.float32)).max() > 0
        pk.expect_equal(to_host(dst), host_like(ofdg, host, dst, **kw), ofdg.PACK_NHWC, "mode %d %s" % (mode, image_dtype))


def test_behind_crop_and_photo(ofdg):
    """128x64 -> 96x48 on OFDG_STREAM_OWN: forward_counter, the crop, the photometric step in place on the cropped frames, the
    pack of the cropped planes - one wait at the end."""
    import torch
    W, H, B, cw, ch = 128, 64, 3, 96, 48
    g = make_gen(ofdg, W, H, 7, pool=True, sampler=1, seed=5, batch_size=B)
    outs = ofdg.alloc_outputs(B, H, W, image_dtype=torch.uint8)
    src = dict(zip(ofdg.PACK_PLANES, outs))
    cropped = ofdg.alloc_crop(src, ch, cw)
    crecs = torch.zeros((B, 4), dtype=torch.int32, device="cuda")
    kw = dict(scale=(2.0 / 255.0,) * 3, bias=(-1.0,) * 3, flow_scale=0.05, layout=ofdg.PACK_NCHW, rgb=True)
    dst = ofdg.alloc_pack(B, ch, cw, image_dtype=torch.float16, flow_dtype=torch.bfloat16)
    torch.cuda.synchronize()
    g.forward_counter(40, B, *outs, ofdg.STREAM_OWN)
    g.crop(src, cropped, first_index=40, hflip=True, recs_out=crecs, stream=ofdg.STREAM_OWN)
    g.photo((cropped["image0"], cropped["image1"]), first_index=40, ranges=ofdg.PHOTO_FLOWNET, stream=ofdg.STREAM_OWN, size=(ch, cw))
    g.pack(cropped, dst, stream=ofdg.STREAM_OWN, size=(ch, cw), **kw)
    g.synchronize(ofdg.STREAM_OWN)
    torch.cuda.synchronize()
    want, _ = ofdg.host_crop(to_host(src), ch, cw, recs=crecs.cpu().numpy())
    frames, _ = ofdg.host_photo((want["image0"], want["image1"]), first_index=40, seed=5, ranges=ofdg.PHOTO_FLOWNET)
    want["image0"], want["image1"] = frames
    pk.expect_equal(to_host(cropped), want, ofdg.PACK_NCHW, "the planes the pack read")
    pk.expect_equal(to_host(dst), host_like(ofdg, want, dst, **kw), ofdg.PACK_NCHW, "behind crop and photo")
    assert want["image0"].any() and np.abs(want["flow"]).max() > 0


def test_three_calls_in_flight(ofdg):
    """Two calls on two caller streams and one on OFDG_STREAM_OWN, each with its own constants, one wait at the end."""
    import torch
    W, H, B = 128, 64, 2
    g = make_gen(ofdg, W, H, 7, pool=True)
    users = [torch.cuda.Stream(), torch.cuda.Stream()]
    batches = [g.sample(B) for _ in range(3)]
    outs = [ofdg.alloc_outputs(B, H, W) for _ in range(3)]
    kws = [dict(scale=(1.0 / 255.0,) * 3, flow_scale=1.0 + k, layout=ofdg.PACK_NHWC if k != 1 else ofdg.PACK_NCHW, concat=k == 2) for k in range(3)]
    dsts = [ofdg.alloc_pack(B, H, W, image_dtype=torch.bfloat16, flow_dtype=torch.float32, layout=kw["layout"], concat=kw["concat"]) for kw in kws]
    torch.cuda.synchronize()
    streams = [users[0].cuda_stream, users[1].cuda_stream, ofdg.STREAM_OWN]
    for (tasks, bps, n), o, d, st, kw in zip(batches, outs, dsts, streams, kws):
        g.render(tasks, B, bps, n, *o, st)
        g.pack(dict(zip(ofdg.PACK_PLANES, o)), d, stream=st, **kw)
    for st in streams:
        g.synchronize(st)
    torch.cuda.synchronize()
    for k, (o, d, kw) in enumerate(zip(outs, dsts, kws)):
        host = to_host(dict(zip(ofdg.PACK_PLANES, o)))
        pk.expect_equal(to_host(d), host_like(ofdg, host, d, **kw), kw["layout"], "call %d" % k)
    assert not np.array_equal(outs[0][0].cpu().numpy(), outs[1][0].cpu().numpy())


def test_flowloader_pack(ofdg):
    import torch
    W, H, B, cw, ch = 128, 96, 2, 96, 48
    kw = dict(width=W, height=H, mode=7, batch_size=B, sampler=1, seed=21)
    pool = lambda g: g.pool_synthetic(3, 2 * W, 2 * H, 11)  # noqa: E731
    make = lambda **more: ofdg.FlowLoader(ofdg.default_params(**kw), pool=pool, prefetch=3, crop=(ch, cw), photo=ofdg.PHOTO_FLOWNET, **more)  # noqa: E731
    scale, bias = ofdg.pack_norm((0.406, 0.456, 0.485), (0.225, 0.224, 0.229))
    opts = dict(image_dtype=torch.bfloat16, flow_dtype=torch.float16, layout=ofdg.PACK_NHWC, concat=True, rgb=True, scale=scale, bias=bias, flow_scale=0.05)
    call = {k: v for k, v in opts.items() if k not in ("image_dtype", "flow_dtype")}
    it, pit = iter(make(pack=opts, stats=True, pyramid=2)), iter(make(stats=True, pyramid=2))
    last = None
    for step in range(3):
        a, p = next(it), next(pit)
        torch.cuda.current_stream().synchronize()
        assert a[1] is None and tuple(a[0].shape) == (B, 6, ch, cw) and a[0].dtype == torch.bfloat16 and a[2].dtype == torch.float16
        assert a[0].is_contiguous(memory_format=torch.channels_last) and a[2].is_contiguous(memory_format=torch.channels_last)
        assert set(a[3]) == set(p[3]) == {"crop", "photo", "flow_stats", "flow_pyramid"}
        # the manual sequence: the pack of what the loader without pack= yields
        got = to_host({"image0": a[0], "flow": a[2]})
        want = host_like(ofdg, to_host(dict(zip(ofdg.PACK_PLANES, p[:3]))), {"image0": a[0], "flow": a[2]}, **call)
        pk.expect_equal(got, want, ofdg.PACK_NHWC, "batch %d" % step)
        # extras, statistics and pyramid are those of the unpacked, unscaled flow
        assert torch.equal(a[3]["crop"], p[3]["crop"]) and torch.equal(a[3]["photo"], p[3]["photo"]) and torch.equal(a[3]["flow_stats"], p[3]["flow_stats"])
        assert all(torch.equal(x, y) for x, y in zip(a[3]["flow_pyramid"], p[3]["flow_pyramid"]))
        last = got
    resumed = next(iter(make(pack=opts, start=2)))
    torch.cuda.current_stream().synchronize()
    pk.expect_equal(to_host({"image0": resumed[0], "flow": resumed[2]}), last, ofdg.PACK_NHWC, "resumed at batch 2")
    # without crop and photo, planar and not concatenated: three tensors in their places
    plain = ofdg.FlowLoader(ofdg.default_params(**kw), pool=pool, pack=dict(image_dtype=torch.float16, scale=(1.0 / 255.0,) * 3))
    ref = ofdg.FlowLoader(ofdg.default_params(**kw), pool=pool)
    a, p = next(iter(plain)), next(iter(ref))
    torch.cuda.current_stream().synchronize()
    assert len(a) == 3 and len(p) == 3 and a[0].dtype == torch.float16 and a[2].dtype == torch.float32 and a[0].is_contiguous()
    got = to_host(dict(zip(ofdg.PACK_PLANES, a)))
    pk.expect_equal(got, host_like(ofdg, to_host(dict(zip(ofdg.PACK_PLANES, p))), dict(zip(ofdg.PACK_PLANES, a)), scale=(1.0 / 255.0,) * 3), ofdg.PACK_NCHW)
    with pytest.raises(ValueError, match="unknown pack option"):
        ofdg.FlowLoader(ofdg.default_params(**kw), pool=pool, pack=dict(dtype=torch.float16))


def test_refusals_enqueue_nothing(ofdg):
    """What only the device entry refuses - misaligned pointers, OFDG_STREAM_OWN before any call - and a sample of the shared
    rules through it: guards and destinations stay 0xA5, a valid call works afterwards."""
    import torch
    W, H, B = 128, 96, 2
    g = make_gen(ofdg, W, H, 7, pool=True, batch_size=B)
    outs = ofdg.alloc_outputs(B, H, W, image_dtype=torch.uint8, flow_dtype=torch.float16)
    fouts = ofdg.alloc_outputs(B, H, W)
    bufs = [guarded(B, 3, H, W, "bfloat16", pk.NCHW), guarded(B, 3, H, W, "bfloat16", pk.NCHW), guarded(B, 2, H, W, "float32", pk.NCHW)]
    torch.cuda.synchronize()
    lib, vp = ofdg.lib(), C.c_void_p

    def job(**kw):
        j = ofdg.PackJob()
        for k in range(3):
            j.src[k], j.dst[k] = outs[k].data_ptr(), bufs[k][1].data_ptr()
        j.image_src_fmt, j.flow_src_fmt, j.image_dst_fmt, j.flow_dst_fmt = ofdg.FMT_U8, ofdg.FMT_F16, ofdg.FMT_BF16, ofdg.FMT_F32
        j.scale[:], j.bias[:], j.flow_scale = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), 1.0
        for k, v in kw.items():
            if k in ("src", "dst", "scale", "bias"):
                for idx, val in v.items():
                    getattr(j, k)[idx] = val
            else:
                setattr(j, k, v)
        return j

    def refused(word, j, n=B, stream=0):
        rc = lib.ofdg_pack(g.h, None if j is None else C.byref(j), n, vp(stream))
        assert rc == ofdg.EINVAL, word
        msg = lib.ofdg_last_error(g.h).decode()
        assert msg.startswith("ofdg_pack: ") and word in msg, (word, msg)
        g.synchronize()
        torch.cuda.synchronize()
        assert all(bool((raw == FILL).all()) for raw, _ in bufs), word

    refused("OFDG_STREAM_OWN", job(), stream=ofdg.STREAM_OWN)  # a fresh context: no call has worked on an internal stream yet
    refused("job", None)
    refused("n_samples", job(), n=0)
    refused("both be 0", job(width=W))
    for bad_w, bad_h in ((100, 48), (96, 47), (4, 2)):
        refused("width", job(width=bad_w, height=bad_h))
    refused("2^31", job(width=32768, height=10924), n=1)
    refused("image_dst_fmt", job(image_dst_fmt=ofdg.FMT_U8))
    refused("flow_src_fmt", job(flow_src_fmt=ofdg.FMT_BF16))
    refused("layout", job(layout=2))
    refused("flags", job(flags=8))
    refused("reserved", job(reserved=-1))
    refused("scale", job(scale={0: float("nan")}))
    refused("bias", job(bias={1: float("inf")}))
    refused("flow_scale", job(flow_scale=float("-inf")))
    refused("no plane", job(src={0: None, 1: None, 2: None}, dst={0: None, 1: None, 2: None}))
    refused("dst", job(dst={0: None}))
    refused("src", job(src={2: None}))
    refused("CONCAT needs both", job(flags=ofdg.PACK_CONCAT, src={1: None}, dst={1: None}))
    refused("dst[image1]", job(flags=ofdg.PACK_CONCAT))
    refused("src[image0] must be 4-byte", job(src={0: outs[0].data_ptr() + 2}))
    refused("src[flow] must be 8-byte", job(src={2: outs[2].data_ptr() + 4}))
    refused("src[image1] must be 16-byte", job(src={1: fouts[1].data_ptr() + 8, 0: fouts[0].data_ptr()}, image_src_fmt=ofdg.FMT_F32))
    refused("dst[image0] must be 16-byte", job(dst={0: bufs[0][1].data_ptr() + 8}))
    refused("dst[flow] must be 16-byte", job(dst={2: bufs[2][1].data_ptr() + 4}))
    refused("overlaps", job(dst={1: bufs[0][1].data_ptr() + 16}))
    refused("overlaps", job(dst={0: outs[0].data_ptr()}))
    # a valid call on the same context still works, also on OFDG_STREAM_OWN once a call has been made
    g.forward(*outs, ofdg.STREAM_OWN)
    dst = {name: t for name, (_, t) in zip(ofdg.PACK_PLANES, bufs)}
    g.pack(dict(zip(ofdg.PACK_PLANES, outs)), dst, scale=(1.0 / 255.0,) * 3, stream=ofdg.STREAM_OWN)
    g.synchronize(ofdg.STREAM_OWN)
    torch.cuda.synchronize()
    pk.expect_equal(to_host(dst), host_like(ofdg, to_host(dict(zip(ofdg.PACK_PLANES, outs))), dst, scale=(1.0 / 255.0,) * 3), pk.NCHW)
    assert guards_intact(bufs)
