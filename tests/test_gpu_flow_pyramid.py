"""GPU tests of the multi-scale flow pyramid (ofdg_flow_pyramid, include/ofdg.h): the device levels against
ofdg_host_flow_pyramid and against the numpy restatement of the definition (tests/flow_pyramid_reference.py), byte for byte -
on tensors with every special pixel planted and the order of summation visible, between guard bytes, on the flow a render
call has just written (rigid, flow1, compact formats, mode 9), with three calls in flight, through the loader - and the
refusals."""
import ctypes as C

import numpy as np
import pytest

import flow_pyramid_reference as fpr

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 64  # bytes in front of and behind every level (keeps the 16-byte alignment)
# W, H, levels: one tile and one top cell; 3x2 whole tiles; partial tiles, idle lanes and a 9-element pitch; half a tile in y
# that still owns level-5 cells; one level on partial tiles
SHAPES = [(64, 64, 6), (192, 128, 6), (72, 40, 3), (128, 96, 5), (72, 40, 1)]
_cache = {}


def tensors(W, H, L, dtype, n=3):
    key = (W, H, L, np.dtype(dtype).name, n)
    if key not in _cache:
        _cache[key] = fpr.planted(n, H, W, dtype, levels=L)
    return _cache[key]


def occ_as(occ, kind):
    if kind is None:
        return None
    return occ.astype(np.uint8) * np.uint8(3) if kind == "u8" else occ.astype(np.float32) * np.float32(0.5)


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


def guarded_pyramid(n, H, W, L, dtype, weights):
    import torch
    lv = [guarded((n, 2, H >> k, W >> k), dtype) for k in range(1, L + 1)]
    wt = [guarded((n, 1, H >> k, W >> k), torch.uint16) for k in range(1, L + 1)] if weights else None
    return lv, wt


def guards_intact(bufs):
    return all(bool((raw[:GUARD] == FILL).all()) and bool((raw[-GUARD:] == FILL).all()) for raw, _ in bufs)


def host_arrays(ts):
    return [t.cpu().numpy() for t in ts]


@pytest.mark.parametrize("W,H,L", SHAPES)
@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["in_f32", "in_f16"])
@pytest.mark.parametrize("out_dtype", [np.float32, np.float16], ids=["out_f32", "out_f16"])
@pytest.mark.parametrize("occ_kind", [None, "u8", "f32"])
def test_planted_tensors_every_option(ofdg, W, H, L, dtype, out_dtype, occ_kind):
    """The levels start as 0xA5 bytes between 0xA5 guards: equality shows every cell was written, the guards that nothing else
    was."""
    import torch
    g = make_gen(ofdg, W, H)
    f, occ = tensors(W, H, L, dtype)
    o = occ_as(occ, occ_kind)
    ft = torch.from_numpy(f).cuda()
    ot = None if o is None else torch.from_numpy(o).cuda()
    tdt = torch.float16 if out_dtype == np.float16 else torch.float32
    for flags in (0, fpr.SCALE):
        want, want_w = fpr.flow_pyramid(f, L, o, flags, out_dtype)
        host, host_w = ofdg.host_flow_pyramid(f, L, o, scale=bool(flags), out_dtype=out_dtype, weights=True)
        for weights in (False, True):
            lv, wt = guarded_pyramid(3, H, W, L, tdt, weights)
            out = [t for _, t in lv]
            out = (out, [t for _, t in wt]) if weights else out
            g.flow_pyramid(ft, L, occ=ot, scale=bool(flags), out=out)
            torch.cuda.synchronize()
            what = "%dx%d L=%d flags %d weights %s" % (W, H, L, flags, weights)
            got = host_arrays(t for _, t in lv)
            fpr.expect_equal(got, want, what + " against the restatement")
            fpr.expect_equal(got, host, what + " against ofdg_host_flow_pyramid")
            assert guards_intact(lv), what
            if weights:
                got_w = host_arrays(t for _, t in wt)
                fpr.expect_equal(got_w, want_w, what + " weights against the restatement")
                fpr.expect_equal(got_w, host_w, what + " weights against ofdg_host_flow_pyramid")
                assert guards_intact(wt), what


def test_entries_past_levels_are_never_read(ofdg):
    """levels = 3 with entries 4..6 set to buffers of 0xA5 (flow) and to wild, misaligned addresses (weight): the call is
    valid, those buffers keep every byte."""
    import torch
    W, H, L, n = 128, 64, 3, 3
    g = make_gen(ofdg, W, H)
    f, _ = tensors(W, H, 6, np.float32)
    ft = torch.from_numpy(f).cuda()
    lv, wt = guarded_pyramid(n, H, W, 6, torch.float32, True)
    rec = ofdg.FlowPyramid()
    rec.levels, rec.out_fmt = L, ofdg.FMT_F32
    for k in range(6):
        rec.flow[k] = lv[k][1].data_ptr()
        rec.weight[k] = wt[k][1].data_ptr() if k < L else 2 + k
    torch.cuda.synchronize()
    rc = ofdg.lib().ofdg_flow_pyramid(g.h, C.c_void_p(ft.data_ptr()), ofdg.FMT_F32, None, ofdg.FMT_F32, n, ofdg.PYR_SCALE, C.byref(rec), None)
    assert rc == ofdg.OK, ofdg.lib().ofdg_last_error(g.h).decode()
    torch.cuda.synchronize()
    want, want_w = fpr.flow_pyramid(f, L, None, fpr.SCALE)
    fpr.expect_equal(host_arrays(t for _, t in lv[:L]), want)
    fpr.expect_equal(host_arrays(t for _, t in wt[:L]), want_w)
    assert guards_intact(lv) and guards_intact(wt)
    assert all(bool((raw == FILL).all()) for raw, _ in lv[L:] + wt[L:])


def rendered(ofdg, g, B, compact, batch):
    """render(..., extras=(flow1, occ0, occ1)) on the internal stream and the pyramids of both flows behind it on the same
    stream, nothing waited for in between."""
    import torch
    W, H = g.params.width, g.params.height
    names = ("flow1", "occ0", "occ1")
    if compact:
        outs = ofdg.alloc_outputs(B, H, W, image_dtype=torch.uint8, flow_dtype=torch.float16)
        ex = ofdg.alloc_extras(B, H, W, names, flow_dtype=torch.float16, occ_dtype=torch.uint8)
    else:
        outs = ofdg.alloc_outputs(B, H, W)
        ex = ofdg.alloc_extras(B, H, W, names)
    L = fpr.max_levels(H, W)
    p0 = ofdg.alloc_flow_pyramid(B, H, W, L, outs[2].dtype, weights=True)
    p1 = ofdg.alloc_flow_pyramid(B, H, W, L, torch.float32, weights=True)
    torch.cuda.synchronize()  # (the allocations were zeroed on torch's stream)
    tasks, bps, n = batch
    g.render(tasks, B, bps, n, *outs, ofdg.STREAM_OWN, extras=ex)
    g.flow_pyramid(outs[2], L, out=p0, stream=ofdg.STREAM_OWN)
    g.flow_pyramid(ex["flow1"], L, occ=ex["occ1"], scale=False, out=p1, stream=ofdg.STREAM_OWN)
    g.synchronize(ofdg.STREAM_OWN)
    torch.cuda.synchronize()
    planes = dict(flow=outs[2].cpu().numpy(), flow1=ex["flow1"].cpu().numpy(), occ1=ex["occ1"].cpu().numpy())
    return p0, p1, planes, L


def test_end_to_end_rigid_and_compact(ofdg):
    """128x64, mode 7: the forward flow without a map, flow1 with occ1 (float32 out, unscaled); then the same in the compact
    formats (fp16 flow, uint8 map)."""
    W, H, B = 128, 64, 3
    g = make_gen(ofdg, W, H, 7, pool=True)
    batch = g.sample(B)
    for compact in (False, True):
        p0, p1, p, L = rendered(ofdg, g, B, compact, batch)
        assert L == 6 and p["flow"].dtype == (np.float16 if compact else np.float32) and p["occ1"].dtype == (np.uint8 if compact else np.float32)
        want0, want0_w = ofdg.host_flow_pyramid(p["flow"], L, weights=True)
        want1, want1_w = ofdg.host_flow_pyramid(p["flow1"], L, p["occ1"], scale=False, out_dtype=np.float32, weights=True)
        what = "compact %s" % compact
        fpr.expect_equal(host_arrays(p0[0]), want0, what + " forward flow")
        fpr.expect_equal(host_arrays(p0[1]), want0_w, what + " forward flow weights")
        fpr.expect_equal(host_arrays(p1[0]), want1, what + " flow1")
        fpr.expect_equal(host_arrays(p1[1]), want1_w, what + " flow1 weights")
        assert (want0_w[0] == 4).all() and 0 < int(want1_w[0].astype(np.int64).sum()) < B * H * W  # (a real flow, a real map)
        assert any(np.abs(a.astype(np.float32)).max() > 0 for a in want0)


def test_end_to_end_mode_9(ofdg):
    import torch
    W, H, B, L = 128, 64, 3, 6
    g = make_gen(ofdg, W, H, 9, pool=True, sampler=1, seed=3, batch_size=B)
    g.warp_generate(1, 3)
    outs = ofdg.alloc_outputs(B, H, W)
    pyr = ofdg.alloc_flow_pyramid(B, H, W, L, weights=True)
    torch.cuda.synchronize()
    g.forward_counter(0, B, *outs, ofdg.STREAM_OWN)
    g.flow_pyramid(outs[2], L, out=pyr, stream=ofdg.STREAM_OWN)
    g.synchronize(ofdg.STREAM_OWN)
    torch.cuda.synchronize()
    want, want_w = ofdg.host_flow_pyramid(outs[2].cpu().numpy(), L, weights=True)
    fpr.expect_equal(host_arrays(pyr[0]), want)
    fpr.expect_equal(host_arrays(pyr[1]), want_w)
    assert int(want_w[L - 1].astype(np.int64).sum()) > 0


def test_three_calls_in_flight(ofdg):
    """Two calls on two caller streams and one on OFDG_STREAM_OWN, each into its own pyramid, one wait at the end."""
    import torch
    W, H, B, L = 128, 64, 2, 6
    g = make_gen(ofdg, W, H, 7, pool=True)
    users = [torch.cuda.Stream(), torch.cuda.Stream()]
    batches = [g.sample(B) for _ in range(3)]
    outs = [ofdg.alloc_outputs(B, H, W) for _ in range(3)]
    pyrs = [ofdg.alloc_flow_pyramid(B, H, W, L, weights=True) for _ in range(3)]
    torch.cuda.synchronize()
    streams = [users[0].cuda_stream, users[1].cuda_stream, ofdg.STREAM_OWN]
    for (tasks, bps, n), o, p, st in zip(batches, outs, pyrs, streams):
        g.render(tasks, B, bps, n, *o, st)
        g.flow_pyramid(o[2], L, out=p, stream=st)
    for st in streams:
        g.synchronize(st)
    torch.cuda.synchronize()
    flows = [o[2].cpu().numpy() for o in outs]
    assert not np.array_equal(flows[0], flows[1]) and not np.array_equal(flows[1], flows[2])
    for i, (fl, p) in enumerate(zip(flows, pyrs)):
        want, want_w = ofdg.host_flow_pyramid(fl, L, weights=True)
        fpr.expect_equal(host_arrays(p[0]), want, "call %d" % i)
        fpr.expect_equal(host_arrays(p[1]), want_w, "call %d weights" % i)


def test_flowloader_pyramid(ofdg):
    import torch
    W, H, B = 128, 96, 2
    kw = dict(width=W, height=H, mode=7, batch_size=B, sampler=1, seed=21)
    pool = lambda g: g.pool_synthetic(3, 2 * W, 2 * H, 11)  # noqa: E731
    loader = ofdg.FlowLoader(ofdg.default_params(**kw), pool=pool, prefetch=3, extras=("occ0",), pyramid=3)
    plain = ofdg.FlowLoader(ofdg.default_params(**kw), pool=pool, prefetch=3, extras=("occ0",))
    it, pit = iter(loader), iter(plain)
    for _ in range(2):
        i0, i1, fl, more = next(it)
        p = next(pit)
        torch.cuda.current_stream().synchronize()
        assert set(more) == {"occ0", "flow_pyramid"} and len(more["flow_pyramid"]) == 3
        assert torch.equal(i0, p[0]) and torch.equal(i1, p[1]) and torch.equal(fl, p[2])  # the loader yields what it yielded
        occ = more["occ0"].cpu().numpy()
        fpr.expect_equal(host_arrays(more["flow_pyramid"]), ofdg.host_flow_pyramid(fl.cpu().numpy(), 3, occ))
        assert occ.any()


def test_flowloader_statistics_and_pyramid_of_the_uncropped_batch(ofdg):
    """stats=True with pyramid=3 and no crop=: both reductions of a set are enqueued by one method of the loader (the cropped
    form is tests/test_gpu_crop.py::test_flowloader_crop); each against its host twin, the batch what a plain loader yields."""
    import torch
    import flow_stats_reference as fsr
    W, H, B = 128, 96, 2
    kw = dict(width=W, height=H, mode=7, batch_size=B, sampler=1, seed=21)
    pool = lambda g: g.pool_synthetic(3, 2 * W, 2 * H, 11)  # noqa: E731
    it = iter(ofdg.FlowLoader(ofdg.default_params(**kw), pool=pool, prefetch=3, extras=("occ0",), stats=True, pyramid=3))
    pit = iter(ofdg.FlowLoader(ofdg.default_params(**kw), pool=pool, prefetch=3, extras=("occ0",)))
    for _ in range(2):
        i0, i1, fl, more = next(it)
        p = next(pit)
        torch.cuda.current_stream().synchronize()
        assert set(more) == {"occ0", "flow_stats", "flow_pyramid"} and len(more["flow_pyramid"]) == 3
        assert torch.equal(i0, p[0]) and torch.equal(i1, p[1]) and torch.equal(fl, p[2]) and torch.equal(more["occ0"], p[3]["occ0"])
        flow, occ = fl.cpu().numpy(), more["occ0"].cpu().numpy()
        fpr.expect_equal(host_arrays(more["flow_pyramid"]), ofdg.host_flow_pyramid(flow, 3, occ))
        assert ofdg.flow_stats_numpy(more["flow_stats"])["rows"].tobytes() == ofdg.host_flow_stats(flow, occ, 2.0).tobytes()
        fsr.expect_equal(ofdg.flow_stats_numpy(more["flow_stats"])["rows"], fsr.flow_stats(flow, occ, 2.0))


def test_refusals_enqueue_nothing(ofdg):
    import torch
    W, H, B, L = 128, 96, 2, 3
    flow = torch.zeros((B, 2, H, W), device="cuda")
    half = torch.zeros((B, 2, H, W), dtype=torch.float16, device="cuda")
    occ8 = torch.zeros((B, 1, H, W), dtype=torch.uint8, device="cuda")
    occf = torch.zeros((B, 1, H, W), device="cuda")
    lv, wt = guarded_pyramid(B, H, W, 6, torch.float32, True)
    torch.cuda.synchronize()
    g = make_gen(ofdg, W, H, 7, pool=True, batch_size=B)
    lib, vp = ofdg.lib(), C.c_void_p
    F32, U8, F16 = ofdg.FMT_F32, ofdg.FMT_U8, ofdg.FMT_F16
    all_f, all_w = [t.data_ptr() for _, t in lv], [t.data_ptr() for _, t in wt]

    def record(levels=L, out_fmt=F32, flows=all_f, weights=(None,) * 6):
        rec = ofdg.FlowPyramid()
        rec.levels, rec.out_fmt = levels, out_fmt
        for k in range(6):
            rec.flow[k], rec.weight[k] = flows[k], weights[k]
        return rec

    def refused(word, d_flow=flow.data_ptr(), ffmt=F32, d_occ=None, ofmt=F32, n=B, flags=0, rec=None, null_rec=False, stream=0):
        rec = record() if rec is None else rec
        rc = lib.ofdg_flow_pyramid(g.h, vp(d_flow), ffmt, vp(d_occ), ofmt, n, flags, None if null_rec else C.byref(rec), vp(stream))
        assert rc == ofdg.EINVAL, word
        msg = lib.ofdg_last_error(g.h).decode()
        assert msg.startswith("ofdg_flow_pyramid") and word in msg, msg
        g.synchronize()
        torch.cuda.synchronize()
        assert all(bool((raw == FILL).all()) for raw, _ in lv + wt), word

    refused("OFDG_STREAM_OWN", stream=ofdg.STREAM_OWN)  # a fresh context: no call has worked on an internal stream yet
    refused("d_flow", d_flow=None)
    refused("pyr", null_rec=True)
    refused("levels", rec=record(levels=0))
    refused("levels", rec=record(levels=7))
    refused("multiples", rec=record(levels=6))  # H = 96
    refused("pyr->flow", rec=record(flows=[all_f[0], None] + all_f[2:]))
    refused("pyr->weight", rec=record(weights=[all_w[0], None, all_w[2], None, None, None]))
    refused("flow_fmt", ffmt=U8)
    refused("flow_fmt", ffmt=3)
    refused("occ_fmt", d_occ=occ8.data_ptr(), ofmt=F16)
    refused("out_fmt", rec=record(out_fmt=U8))
    refused("n_samples", n=0)
    refused("flags", flags=2)
    refused("16-byte", d_flow=flow.data_ptr() + 8)
    refused("8-byte", d_flow=half.data_ptr() + 4, ffmt=F16)
    refused("4-byte", d_occ=occ8.data_ptr() + 2, ofmt=U8)
    refused("16-byte", d_occ=occf.data_ptr() + 4, ofmt=F32)
    refused("16-byte", rec=record(flows=[all_f[0] + 8] + all_f[1:]))
    refused("4-byte", rec=record(weights=[all_w[0], all_w[1] + 2] + all_w[2:]))
    # a valid call on the same context still works, also on OFDG_STREAM_OWN once a call has been made
    outs = ofdg.alloc_outputs(B, H, W)
    torch.cuda.synchronize()
    g.forward(*outs, ofdg.STREAM_OWN)
    got = g.flow_pyramid(outs[2], L, stream=ofdg.STREAM_OWN)
    g.synchronize(ofdg.STREAM_OWN)
    torch.cuda.synchronize()
    fpr.expect_equal(host_arrays(got), ofdg.host_flow_pyramid(outs[2].cpu().numpy(), L))
