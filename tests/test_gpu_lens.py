"""GPU tests of the lens (ofdg_lens, include/ofdg.h): the device planes against ofdg_host_lens and against the numpy restatement
(tests/lens_reference.py), byte for byte - every size and format, every plane alone and all eight together, between guard
bytes; drawn records, first_index and seed; behind a render call without synchronisation (rigid, mode 9); through the loader
with the later stages on the bent planes - and the refusals.  Hostile records are sanitised by definition: the test of that
compares bytes with the host twin."""
import ctypes as C
import itertools

import numpy as np
import pytest

import flow_stats_reference as fsr
import lens_reference as lr

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 64  # bytes in front of and behind every destination (keeps the 16-byte alignment)
FORMATS = list(itertools.product(("float32", "uint8"), ("float32", "float16"), ("float32", "uint8")))
RANGES = dict(prob=1.0, k1_range=0.125, ca_range=1.0 / 64, vig_max=0.5, centre=0.25)


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


def guarded_like(src):
    return {k: guarded(tuple(t.shape), t.dtype) for k, t in src.items()}


def guards_intact(bufs):
    return all(bool((raw[:GUARD] == FILL).all()) and bool((raw[-GUARD:] == FILL).all()) for raw, _ in bufs)


def to_host(planes):
    return {k: t.cpu().numpy() for k, t in planes.items()}


def to_dev(planes):
    import torch
    return {k: torch.from_numpy(np.array(v)).cuda() for k, v in planes.items()}


@pytest.mark.parametrize("W,H", lr.GPU_SIZES)
@pytest.mark.parametrize("image,flow,occ", FORMATS)
def test_device_equals_host_twin_and_restatement(ofdg, W, H, image, flow, occ):
    """n = 3, all eight planes, every record of the CPU tests with and without the window flag.  The destinations start as 0xA5
    bytes between 0xA5 guards: equality shows every element was written, the guards that nothing else was.  The context's
    frame is another size than the planes: the job carries its own."""
    import torch
    g = make_gen(ofdg, 64, 32)
    src = lr.planes(W, H, image, flow, occ)
    dev = to_dev(src)
    for fill, window in ((False, True), (True, False)):
        recs = lr.records(W, H, fill)
        for k in range(0, len(recs), lr.N):
            part = recs[k:k + lr.N]
            host, host_recs = ofdg.host_lens(src, recs=part, occ_window=window)
            bufs = guarded_like(dev)
            rraw, rout = guarded((lr.N, 8), torch.float64)
            g.lens(dev, {name: t for name, (_, t) in bufs.items()}, recs=torch.from_numpy(part).cuda(), occ_window=window, recs_out=rout,
                   size=(H, W))
            torch.cuda.synchronize()
            what = "%dx%d fill %s records %d.. window %s" % (W, H, fill, k, window)
            got = to_host({name: t for name, (_, t) in bufs.items()})
            lr.expect_equal(got, host, what + " against ofdg_host_lens")
            if k == 12:
                lr.expect_equal(got, lr.lens(src, part, window)[0], what + " against the restatement")
            assert guards_intact(list(bufs.values()) + [(rraw, rout)]), what
            assert rout.cpu().numpy().tobytes() == host_recs.tobytes() == part.tobytes(), what
    for name, t in dev.items():
        assert t.cpu().numpy().tobytes() == src[name].tobytes(), name  # the inputs are as they were


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("subset", lr.SUBSETS)
def test_every_plane_alone_and_all_together(ofdg, subset, n):
    import torch
    W, H = lr.GPU_SIZES[4]
    g = make_gen(ofdg, W, H)
    full = {k: v[:n] for k, v in lr.planes(W, H, "uint8", "float16", "float32").items()}
    src = {k: full[k] for k in subset}
    recs = lr.records(W, H, False)[[14, 2, 9][:n]]
    dev = to_dev(src)
    bufs = guarded_like(dev)
    g.lens(dev, {k: t for k, (_, t) in bufs.items()}, recs=torch.from_numpy(recs).cuda())
    torch.cuda.synchronize()
    host, _ = ofdg.host_lens(src, recs=recs)
    lr.expect_equal(to_host({k: t for k, (_, t) in bufs.items()}), host, str(subset))
    if not subset[0].startswith("occ"):     # (a map alone lacks the marks its flow's unsolvable pixels would set)
        lr.expect_equal(host, {k: v for k, v in ofdg.host_lens(full, recs=recs)[0].items() if k in subset}, "a plane does not depend on the others")
    assert guards_intact(bufs.values())


def test_hostile_records_are_sanitised(ofdg):
    """NaN, infinities and values beyond every limit become the identity on the device as on the host: bytes compared with the
    twin, guards intact."""
    import torch
    W, H = 40, 26
    g = make_gen(ofdg, W, H)
    src = {k: v[:1] for k, v in lr.planes(W, H, "float32", "float32", "uint8").items()}
    dev = to_dev(src)
    good = np.array([0.05, 0.9, 0.001, -0.002, 0.2, 20.0, 12.0, 0.0], np.float64)
    rows = []
    for field in range(7):
        for value in (np.nan, np.inf, -np.inf, 1e300, -1e300, 2.5, -2.5):
            rec = good.copy()
            rec[field] = value
            rows.append(rec)
    for rec in rows + [good]:
        bufs = guarded_like(dev)
        rraw, rout = guarded((1, 8), torch.float64)
        g.lens(dev, {k: t for k, (_, t) in bufs.items()}, recs=torch.from_numpy(rec[None]).cuda(), occ_window=True, recs_out=rout)
        torch.cuda.synchronize()
        host, used = ofdg.host_lens(src, recs=rec[None], occ_window=True)
        lr.expect_equal(to_host({k: t for k, (_, t) in bufs.items()}), host, str(rec))
        assert rout.cpu().numpy().tobytes() == used.tobytes() and guards_intact(list(bufs.values()) + [(rraw, rout)])
        assert (used.tobytes() == lr.identity(W, H)[None].tobytes()) == (rec is not good)


@pytest.mark.parametrize("first_index,seed", [(0, 12345), ((1 << 32) + 3, 12345), (5, 99)])
def test_drawn_records(ofdg, first_index, seed):
    """recs given against recs drawn: recs_out equals lens_draw, first_index and seed honoured."""
    import torch
    W, H, n = 136, 18, 5
    g = make_gen(ofdg, W, H)
    src = lr.planes(W, H, "uint8", "float16", "float32", n=n)
    dev = to_dev(src)
    out, again = ofdg.alloc_lens(dev), ofdg.alloc_lens(dev)
    rout = torch.full((n, 8), -1, dtype=torch.float64, device="cuda")
    g.lens(dev, out, first_index=first_index, seed=seed, ranges=RANGES, fill=True, occ_window=True, recs_out=rout)
    torch.cuda.synchronize()
    used = rout.cpu().numpy()
    for i in range(n):
        assert ofdg.lens_draw(seed, first_index + i, W, H, RANGES, fill=True).tobytes() == used[i].tobytes()
    assert used.tobytes() == lr.drawn_records(seed, first_index, n, W, H, RANGES, lr.FILL).tobytes()
    host, _ = ofdg.host_lens(src, recs=used, occ_window=True)
    lr.expect_equal(to_host(out), host)
    g.lens(dev, again, recs=rout, occ_window=True)      # the same records, given
    torch.cuda.synchronize()
    lr.expect_equal(to_host(again), host)
    assert len({tuple(r) for r in used.tolist()}) == n
    # the context's seed is the default
    g2 = make_gen(ofdg, W, H, seed=seed)
    g2.lens(dev, again, first_index=first_index, ranges=RANGES, fill=True, occ_window=True, recs_out=rout)
    torch.cuda.synchronize()
    assert rout.cpu().numpy().tobytes() == used.tobytes()


@pytest.mark.parametrize("mode", [7, 9])
def test_rendered_batch(ofdg, mode):
    """A rendered 64x48 batch of a rigid mode and of mode 9 through Generator.lens on OFDG_STREAM_OWN, nothing waited for in
    between, against the host twin."""
    import torch
    W, H, B = 64, 48, 3
    g = make_gen(ofdg, W, H, mode, pool=True, sampler=1, seed=3, batch_size=B)
    if mode == 9:
        g.warp_generate(1, 3)
    outs = ofdg.alloc_outputs(B, H, W)
    ex = ofdg.alloc_extras(B, H, W) if mode == 7 else {}
    src = dict(zip(("image0", "image1", "flow"), outs), **ex)
    dst = ofdg.alloc_lens(src)
    recs = torch.zeros((B, 8), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    g.forward_counter(0, B, *outs, ofdg.STREAM_OWN, **(dict(extras=ex) if ex else {}))
    g.lens(src, dst, first_index=40, ranges=RANGES, fill=True, occ_window=bool(ex), recs_out=recs, stream=ofdg.STREAM_OWN)
    g.synchronize(ofdg.STREAM_OWN)
    torch.cuda.synchronize()
    want, used = ofdg.host_lens(to_host(src), first_index=40, seed=3, ranges=RANGES, fill=True, occ_window=bool(ex))
    lr.expect_equal(to_host(dst), want)
    assert recs.cpu().numpy().tobytes() == used.tobytes()
    assert np.nanmax(np.abs(want["flow"])) > 0 and want["image1"].any() and not np.array_equal(want["image0"], to_host(src)["image0"])


def test_flowloader_lens(ofdg):
    """FlowLoader(lens=LENS_DEFAULT), alone and with crop=, motion_blur=, stats= and pack=: the batch's planes equal host_lens of
    the window's planes under the records the dict returns, the later stages' outputs their host twins run on the bent planes;
    lens=None is the loader without the option, and a lens that never fires moves bytes only."""
    import torch
    W, H, B, cw, ch = 128, 96, 2, 96, 48
    kw = dict(width=W, height=H, mode=7, batch_size=B, sampler=1, seed=21)
    pool = lambda g: g.pool_synthetic(3, 2 * W, 2 * H, 11)  # noqa: E731
    extras = ("flow1", "occ0", "occ1", "label0")
    lens = dict(ofdg.LENS_DEFAULT, prob=1.0)
    blur = dict(ofdg.MBLUR_DEFAULT, taps_side=8)
    make = lambda **more: ofdg.FlowLoader(ofdg.default_params(**kw), pool=pool, prefetch=3, extras=extras, **more)  # noqa: E731
    names = ("image0", "image1", "flow") + extras

    def planes_of(batch):
        return dict(zip(names[:3], (t.cpu().numpy() for t in batch[:3])), **{k: batch[3][k].cpu().numpy() for k in extras})

    alone, plain = iter(make(lens=lens)), iter(make())
    full = iter(make(lens=lens, crop=(ch, cw), motion_blur=blur, stats=True, pack=dict(flow_scale=0.05)))
    cropped, none = iter(make(crop=(ch, cw))), iter(make(lens=None, crop=(ch, cw)))
    never = iter(make(lens=dict(lens, prob=0.0), crop=(ch, cw)))
    for step in range(2):
        a, p, f, c, o, z = next(alone), next(plain), next(full), next(cropped), next(none), next(never)
        torch.cuda.current_stream().synchronize()
        first = ofdg.shard_first_index(step, B, 1, 0)
        # alone: the frame's planes bent
        assert set(a[3]) == set(p[3]) | {"lens"} and a[3]["lens"].dtype == torch.float64 and tuple(a[3]["lens"].shape) == (B, 8)
        recs = a[3]["lens"].cpu().numpy()
        assert recs.tobytes() == lr.drawn_records(21, first, B, W, H, lens, lr.FILL).tobytes()
        assert all(ofdg.lens_draw(21, first + i, W, H, ofdg.LENS_DEFAULT | dict(prob=1.0)).tobytes() == recs[i].tobytes() for i in range(B))
        want, _ = ofdg.host_lens(planes_of(p), recs=recs, occ_window=True)
        lr.expect_equal(planes_of(a), want, "batch %d: lens alone" % step)
        assert not np.array_equal(want["flow"], planes_of(p)["flow"])
        # behind the crop, on the window's size; then blur, statistics and pack on the bent planes
        recs = f[3]["lens"].cpu().numpy()
        assert recs.tobytes() == lr.drawn_records(21, first, B, cw, ch, lens, lr.FILL).tobytes()
        assert torch.equal(f[3]["crop"], c[3]["crop"])
        bent, _ = ofdg.host_lens(planes_of(c), recs=recs, occ_window=True)
        for k in ("flow1", "occ0", "occ1", "label0"):
            assert f[3][k].cpu().numpy().tobytes() == bent[k].tobytes(), k
        blurred, used = ofdg.host_motion_blur((bent["image0"], bent["image1"]), (bent["flow"], bent["flow1"]), first_index=first, seed=21,
                                              ranges={k: v for k, v in blur.items() if k != "taps_side"}, taps_side=8)
        assert f[3]["motion_blur"].cpu().numpy().tobytes() == used.tobytes()
        packed = ofdg.host_pack(dict(image0=blurred[0], image1=blurred[1], flow=bent["flow"]), flow_scale=0.05)
        for k, t in zip(names[:3], f[:3]):
            assert t.cpu().numpy().tobytes() == np.ascontiguousarray(packed[k]).tobytes(), k
        fsr.expect_equal(ofdg.flow_stats_numpy(f[3]["flow_stats"])["rows"], fsr.rows_of(ofdg.host_flow_stats(bent["flow"], bent["occ0"], 2.0)))
        # lens=None is the loader without the option; a lens that never fires copies the window's planes
        assert set(o[3]) == set(c[3]) and all(torch.equal(o[3][k], c[3][k]) for k in c[3]) and all(torch.equal(x, y) for x, y in zip(o[:3], c[:3]))
        assert z[3]["lens"].cpu().numpy().tobytes() == np.stack([lr.identity(cw, ch)] * B).tobytes()
        lr.expect_equal(planes_of(z), planes_of(c), "batch %d: the identity lens" % step)
    with pytest.raises(ValueError, match="objects"):
        ofdg.FlowLoader(ofdg.default_params(**kw), pool=pool, extras=("label0", "label1"), objects=True, lens=lens)
    with pytest.raises(ValueError, match="unknown range"):
        ofdg.FlowLoader(ofdg.default_params(**kw), pool=pool, lens=dict(zoom=1.0))


def test_refusals_enqueue_nothing(ofdg):
    import torch
    W, H, B = 128, 96, 2
    g = make_gen(ofdg, W, H, 7, pool=True, batch_size=B)
    outs = ofdg.alloc_outputs(B, H, W, image_dtype=torch.uint8, flow_dtype=torch.float16)
    ex = ofdg.alloc_extras(B, H, W, flow_dtype=torch.float16)
    src = dict(zip(("image0", "image1", "flow"), outs), **ex)
    bufs = guarded_like(src)
    recs = torch.from_numpy(np.stack([lr.identity(W, H)] * B)).cuda()
    rraw, rout = guarded((B, 8), torch.float64)
    torch.cuda.synchronize()
    lib, vp = ofdg.lib(), C.c_void_p
    codes = dict(image_fmt=ofdg.FMT_U8, flow_fmt=ofdg.FMT_F16, occ_fmt=ofdg.FMT_F32)

    def job(planes=lr.PLANES, **kw):
        j = ofdg.LensJob()
        for k, name in enumerate(lr.PLANES):
            if name in planes:
                j.src[k], j.dst[k] = src[name].data_ptr(), bufs[name][1].data_ptr()
        j.recs, j.recs_out = recs.data_ptr(), rout.data_ptr()
        for k, v in dict(codes, **kw).items():
            if k in ("src", "dst"):
                for idx, val in v.items():
                    getattr(j, k)[idx] = val
            else:
                setattr(j, k, v)
        return j

    def refused(word, j, n=B, stream=0):
        rc = lib.ofdg_lens(g.h, None if j is None else C.byref(j), n, vp(stream))
        assert rc == ofdg.EINVAL, word
        msg = lib.ofdg_last_error(g.h).decode()
        assert msg.startswith("ofdg_lens") and word in msg, (word, msg)
        g.synchronize()
        torch.cuda.synchronize()
        assert all(bool((raw == FILL).all()) for raw, _ in list(bufs.values()) + [(rraw, rout)]), word

    refused("OFDG_STREAM_OWN", job(), stream=ofdg.STREAM_OWN)  # a fresh context: no call has worked on an internal stream yet
    refused("job", None)
    refused("n_samples", job(), n=0)
    refused("width and height", job(height=H))
    refused("width", job(width=W + 4, height=H))
    refused("height", job(width=W, height=H + 1))
    refused("flags", job(flags=2))
    refused("flags", job(flags=32))
    refused("reserved", job(reserved=-1))
    refused("image_fmt", job(image_fmt=ofdg.FMT_F16))
    refused("flow_fmt", job(flow_fmt=ofdg.FMT_U8))
    refused("occ_fmt", job(occ_fmt=7))
    refused("prob", job(prob=1.5))
    refused("k1_range", job(k1_range=0.2))
    refused("ca_range", job(ca_range=float("nan")))
    refused("vig_max", job(vig_max=0.6))
    refused("centre", job(centre=-0.1))
    refused("no plane", job(planes=()))
    refused("dst", job(dst={3: None}))
    refused("src", job(src={7: None}))
    refused("occ0", job(planes=("occ0",), flags=lr.OCC_WINDOW))
    refused("occ1", job(planes=("occ1", "flow"), flags=lr.OCC_WINDOW))
    refused("4-byte", job(src={0: src["image0"].data_ptr() + 2}))
    refused("8-byte", job(src={2: src["flow"].data_ptr() + 4}))
    refused("16-byte", job(src={4: src["occ0"].data_ptr() + 8}))
    refused("16-byte", job(dst={6: bufs["label0"][1].data_ptr() + 8}))
    refused("recs must", job(recs=recs.data_ptr() + 8))
    refused("recs_out", job(recs_out=rout.data_ptr() + 8))
    refused("overlaps", job(dst={1: src["image1"].data_ptr()}))
    refused("overlaps", job(dst={5: bufs["occ0"][1].data_ptr() + 16}))
    refused("overlaps", job(recs_out=recs.data_ptr()))
    # a valid call on the same context still works, also on OFDG_STREAM_OWN once a call has been made
    g.forward(*outs, ofdg.STREAM_OWN, extras=ex)
    dst = {k: t for k, (_, t) in bufs.items()}
    g.lens(src, dst, first_index=7, ranges=RANGES, fill=True, occ_window=True, recs_out=rout, stream=ofdg.STREAM_OWN)
    g.synchronize(ofdg.STREAM_OWN)
    torch.cuda.synchronize()
    want, used = ofdg.host_lens(to_host(src), first_index=7, seed=g.params.seed, ranges=RANGES, fill=True, occ_window=True)
    lr.expect_equal(to_host(dst), want)
    assert rout.cpu().numpy().tobytes() == used.tobytes() and guards_intact(list(bufs.values()) + [(rraw, rout)])
