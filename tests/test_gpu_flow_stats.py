"""GPU tests of the per-sample flow statistics (ofdg_flow_stats, include/ofdg.h): the device rows against ofdg_host_flow_stats
and against the numpy restatement of the definition (tests/flow_stats_reference.py), field for field and bit for bit - on
tensors with every special pixel planted, on the flow a render call has just written (rigid, compact formats, mode 9), across
streams with two calls in flight, through the loader - and the refusals."""
import ctypes as C

import numpy as np
import pytest

import flow_stats_reference as fsr

pytestmark = pytest.mark.gpu

FILL = 0xA5
BIN_PX = (0.25, 2.0, 3.7)
_cache = {}


def tensors(W, H, bin_px, dtype, n=3):
    key = (W, H, bin_px, np.dtype(dtype).name, n)
    if key not in _cache:
        _cache[key] = fsr.planted(n, H, W, bin_px, dtype)
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


def filled_rows(m):
    import torch
    return torch.full((m, 304), FILL, dtype=torch.uint8, device="cuda")


def flags_of(o):
    return (0, fsr.ONE_ROW) + ((fsr.VISIBLE_ONLY, fsr.VISIBLE_ONLY | fsr.ONE_ROW) if o is not None else ())


def device_rows(ofdg, g, flow_t, occ_t, bin_px, flags, rows=None, stream=0, n=None):
    """One call into rows pre-filled with 0xA5 (or into `rows` as they are); returns the tensor, nothing waited for."""
    one = bool(flags & fsr.ONE_ROW)
    if rows is None:
        rows = filled_rows(1 if one else flow_t.shape[0])
    g.flow_stats(flow_t, rows, occ=occ_t, bin_px=bin_px, accumulate=bool(flags & fsr.ACCUMULATE),
                 visible_only=bool(flags & fsr.VISIBLE_ONLY), one_row=one, stream=stream)
    return rows


def structured(ofdg, rows):
    return ofdg.flow_stats_numpy(rows)["rows"]


def check_all_options(ofdg, W, H, dtype, occ_kind, bins):
    import torch
    g = make_gen(ofdg, W, H)
    for bin_px in bins:
        f, occ = tensors(W, H, bin_px, dtype)
        o = occ_as(occ, occ_kind)
        ft = torch.from_numpy(f).cuda()
        ot = None if o is None else torch.from_numpy(o).cuda()
        for flags in flags_of(o):
            got = structured(ofdg, device_rows(ofdg, g, ft, ot, bin_px, flags))  # (.cpu() waits for the null stream)
            want = fsr.flow_stats(f, o, bin_px, flags)
            what = "%dx%d bin %s flags %d" % (W, H, bin_px, flags)
            fsr.expect_equal(got, want, what + " against the restatement")
            host = ofdg.host_flow_stats(f, o, bin_px, visible_only=bool(flags & fsr.VISIBLE_ONLY), one_row=bool(flags & fsr.ONE_ROW))
            assert got.tobytes() == host.tobytes(), what + " against ofdg_host_flow_stats"
            fsr.expect_invariants(want, H, W, 3 if flags & fsr.ONE_ROW else 1, bool(flags & fsr.VISIBLE_ONLY))


@pytest.mark.parametrize("W,H", [(72, 40), (128, 96)])
@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("occ_kind", [None, "u8", "f32"])
def test_planted_tensors_every_option(ofdg, W, H, dtype, occ_kind):
    """72x40: one workgroup per sample with idle lanes in its last pass; 128x96: three whole workgroups per sample.  The rows
    start as 0xA5 bytes: equality shows they were overwritten in full."""
    check_all_options(ofdg, W, H, dtype, occ_kind, BIN_PX)


@pytest.mark.parametrize("dtype,occ_kind", [(np.float32, "u8"), (np.float16, "f32"), (np.float32, None)], ids=["f32_u8", "f16_f32", "f32_none"])
def test_several_workgroups_per_sample(ofdg, dtype, occ_kind):
    """160x100 = 4000 quads: four workgroups per sample, four passes each, the last one partial - what reaches a row comes
    through the global atomics of all of them."""
    check_all_options(ofdg, 160, 100, dtype, occ_kind, (2.0,))


def test_accumulate_adds_to_the_rows(ofdg):
    import torch
    W, H = 128, 96
    g = make_gen(ofdg, W, H)
    a, occ = tensors(W, H, 2.0, np.float32)
    b = fsr.planted(3, H, W, 2.0, np.float16, seed=8)[0]
    o = occ_as(occ, "u8")
    at, bt, ot = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), torch.from_numpy(o).cuda()
    for one in (0, fsr.ONE_ROW):
        rows = ofdg.alloc_flow_stats(1 if one else 3)  # zeroed once: the identity
        device_rows(ofdg, g, at, ot, 2.0, one | fsr.ACCUMULATE, rows)
        device_rows(ofdg, g, bt, None, 2.0, one | fsr.ACCUMULATE, rows)
        want = fsr.flow_stats(b, None, 2.0, one | fsr.ACCUMULATE, rows=fsr.flow_stats(a, o, 2.0, one))
        fsr.expect_equal(structured(ofdg, rows), want)


def rendered_batch(ofdg, g, B, compact, batch=None):
    """render(..., extras=(flow1, occ0, occ1)) on the internal stream, then the statistics of both flows behind it on the same
    stream, nothing waited for in between.  Returns (rows of the forward flow, rows of flow1, the planes on the host)."""
    import torch
    W, H = g.params.width, g.params.height
    names = ("flow1", "occ0", "occ1")
    if compact:
        outs = ofdg.alloc_outputs(B, H, W, image_dtype=torch.uint8, flow_dtype=torch.float16)
        ex = ofdg.alloc_extras(B, H, W, names, flow_dtype=torch.float16, occ_dtype=torch.uint8)
    else:
        outs = ofdg.alloc_outputs(B, H, W)
        ex = ofdg.alloc_extras(B, H, W, names)
    r0, r1 = filled_rows(B), filled_rows(B)
    torch.cuda.synchronize()  # (the fills ran on torch's stream)
    tasks, bps, n = batch
    g.render(tasks, B, bps, n, *outs, ofdg.STREAM_OWN, extras=ex)
    g.flow_stats(outs[2], r0, occ=ex["occ0"], bin_px=2.0, visible_only=True, stream=ofdg.STREAM_OWN)
    g.flow_stats(ex["flow1"], r1, occ=ex["occ1"], bin_px=2.0, stream=ofdg.STREAM_OWN)
    g.synchronize(ofdg.STREAM_OWN)
    torch.cuda.synchronize()
    planes = dict(flow=outs[2].cpu().numpy(), flow1=ex["flow1"].cpu().numpy(), occ0=ex["occ0"].cpu().numpy(), occ1=ex["occ1"].cpu().numpy())
    return r0, r1, planes


def test_end_to_end_rigid_and_compact(ofdg):
    W, H, B = 128, 96, 3
    g = make_gen(ofdg, W, H, 7, pool=True)
    batch = g.sample(B)
    for compact in (False, True):
        r0, r1, p = rendered_batch(ofdg, g, B, compact, batch)
        assert p["flow"].dtype == (np.float16 if compact else np.float32) and p["occ0"].dtype == (np.uint8 if compact else np.float32)
        want0 = fsr.flow_stats(p["flow"], p["occ0"], 2.0, fsr.VISIBLE_ONLY)
        want1 = fsr.flow_stats(p["flow1"], p["occ1"], 2.0)
        fsr.expect_equal(structured(ofdg, r0), want0, "forward flow, compact %s" % compact)
        fsr.expect_equal(structured(ofdg, r1), want1, "flow1, compact %s" % compact)
        fsr.expect_invariants(want0, H, W, visible_only=True)
        assert all(r["n_counted"] > 0 and r["n_occluded"] > 0 and r["sum_mag_q8"] > 0 for r in want0 + want1)  # (a real flow)


def test_end_to_end_mode_9(ofdg):
    import torch
    W, H, B = 128, 96, 3
    g = make_gen(ofdg, W, H, 9, pool=True, sampler=1, seed=3, batch_size=B)
    g.warp_generate(1, 3)
    outs = ofdg.alloc_outputs(B, H, W)
    rows = filled_rows(B)
    torch.cuda.synchronize()
    g.forward_counter(0, B, *outs, ofdg.STREAM_OWN)
    g.flow_stats(outs[2], rows, bin_px=2.0, stream=ofdg.STREAM_OWN)
    g.synchronize(ofdg.STREAM_OWN)
    torch.cuda.synchronize()
    flow = outs[2].cpu().numpy()
    got = structured(ofdg, rows)
    fsr.expect_equal(got, fsr.flow_stats(flow, None, 2.0))
    bad = ~((np.abs(flow[:, 0]) < 1048576.0) & (np.abs(flow[:, 1]) < 1048576.0))
    assert list(got["n_bad"]) == [int(bad[i].sum()) for i in range(B)]  # (whatever it is: mode 9 may hold non-finite flow)
    assert all(got["n_counted"] > 0)


@pytest.mark.parametrize("own", [False, True], ids=["callers_stream", "stream_own"])
def test_streams_two_calls_in_flight(ofdg, own):
    """Two render + flow_stats pairs back to back on one stream - a caller's, or the internal ones (every chain's slot is taken
    again by the pairs that follow) - one synchronisation at the end: per-batch rows are their own batch's, and the rows both
    calls ACCUMULATE into hold the restatement over both."""
    import torch
    W, H, B = 128, 96, 2
    g = make_gen(ofdg, W, H, 7, pool=True)
    K = g.num_chains() + 2
    user = torch.cuda.Stream()
    st = ofdg.STREAM_OWN if own else user.cuda_stream
    batches = [g.sample(B) for _ in range(K)]
    outs = [ofdg.alloc_outputs(B, H, W) for _ in range(K)]
    each = [filled_rows(B) for _ in range(K)]
    running = ofdg.alloc_flow_stats(1)
    torch.cuda.synchronize()
    for (tasks, bps, n), o, r in zip(batches, outs, each):
        g.render(tasks, B, bps, n, *o, st)
        g.flow_stats(o[2], r, bin_px=3.7, stream=st)
        # (on the internal streams consecutive calls run on different chains: only a caller's stream orders the adds of one call
        # behind the other's - integer atomics make the result the same either way, but the zeroing above must have finished)
        g.flow_stats(o[2], running, bin_px=3.7, accumulate=True, one_row=True, stream=st)
    g.synchronize(st)
    torch.cuda.synchronize()
    want = fsr.zero_rows(1)
    for o, r in zip(outs, each):
        flow = o[2].cpu().numpy()
        fsr.expect_equal(structured(ofdg, r), fsr.flow_stats(flow, None, 3.7))
        one = fsr.flow_stats(flow, None, 3.7, fsr.ONE_ROW)[0]
        want[0] = {f: ([p + q for p, q in zip(want[0][f], one[f])] if f == "hist" else max(want[0][f], one[f]) if f == "max_key"
                       else want[0][f] + one[f]) for f in fsr.FIELDS}
    fsr.expect_equal(structured(ofdg, running), want)
    assert want[0]["n_counted"] == K * B * H * W


def test_refusals_enqueue_nothing(ofdg):
    import torch
    W, H, B = 128, 96, 2
    rows = filled_rows(B + 1)
    flow = torch.zeros((B, 2, H, W), device="cuda")
    half = torch.zeros((B, 2, H, W), dtype=torch.float16, device="cuda")
    occ8 = torch.zeros((B + 1, 1, H, W), dtype=torch.uint8, device="cuda")
    occf = torch.zeros((B + 1, 1, H, W), device="cuda")
    torch.cuda.synchronize()
    g = make_gen(ofdg, W, H, 7, pool=True, batch_size=B)
    L, vp = ofdg.lib(), C.c_void_p
    F32, U8, F16 = ofdg.FMT_F32, ofdg.FMT_U8, ofdg.FMT_F16

    def refused(word, d_flow=flow.data_ptr(), ffmt=F32, d_occ=None, ofmt=F32, n=B, bin_px=2.0, flags=0, d_rows=rows.data_ptr(), stream=0):
        rc = L.ofdg_flow_stats(g.h, vp(d_flow), ffmt, vp(d_occ), ofmt, n, bin_px, flags, vp(d_rows), vp(stream))
        assert rc == ofdg.EINVAL
        msg = L.ofdg_last_error(g.h).decode()
        assert msg.startswith("ofdg_flow_stats") and word in msg, msg
        g.synchronize()
        torch.cuda.synchronize()
        assert bool((rows == FILL).all())

    refused("OFDG_STREAM_OWN", stream=ofdg.STREAM_OWN)  # a fresh context: no call has worked on an internal stream yet
    refused("d_flow", d_flow=None)
    refused("d_rows", d_rows=None)
    refused("flow_fmt", ffmt=U8)
    refused("flow_fmt", ffmt=3)
    refused("occ_fmt", d_occ=occ8.data_ptr(), ofmt=F16)
    refused("n_samples", n=0)
    for bad in (float("nan"), 0.0, -2.0, 2.0 ** -11, 2.0 ** 14 * 1.001, float("inf")):
        refused("bin_px", bin_px=bad)
    refused("flags", flags=8)
    refused("VISIBLE_ONLY", flags=ofdg.STATS_VISIBLE_ONLY)
    refused("ONE_ROW", flags=ofdg.STATS_ONE_ROW, n=(1 << 32) // (W * H) + 1)  # n*H*W >= 2^32 (refused before anything is read)
    refused("8-byte", d_rows=rows.data_ptr() + 4)
    refused("16-byte", d_flow=flow.data_ptr() + 8)
    refused("8-byte", d_flow=half.data_ptr() + 4, ffmt=F16)
    refused("4-byte", d_occ=occ8.data_ptr() + 2, ofmt=U8)
    refused("16-byte", d_occ=occf.data_ptr() + 4, ofmt=F32)
    # the valid call still works, also on OFDG_STREAM_OWN once a call has been made
    outs = ofdg.alloc_outputs(B, H, W)
    torch.cuda.synchronize()
    g.forward(*outs, ofdg.STREAM_OWN)
    g.flow_stats(outs[2], rows[:B], stream=ofdg.STREAM_OWN)
    g.synchronize(ofdg.STREAM_OWN)
    torch.cuda.synchronize()
    fsr.expect_equal(structured(ofdg, rows[:B]), fsr.flow_stats(outs[2].cpu().numpy(), None, 2.0))
    assert bool((rows[B:] == FILL).all())  # (the row behind the call's rows is not the call's)


@pytest.mark.parametrize("extras", [None, ("occ0",)], ids=["flow_only", "with_occ0"])
def test_flowloader_stats(ofdg, extras):
    import torch
    W, H, B = 128, 96, 2
    kw = dict(width=W, height=H, mode=7, batch_size=B, sampler=1, seed=21)
    pool = lambda g: g.pool_synthetic(3, 2 * W, 2 * H, 11)  # noqa: E731
    loader = ofdg.FlowLoader(ofdg.default_params(**kw), pool=pool, prefetch=3, extras=extras, stats=True, stats_bin_px=3.7)
    plain = ofdg.FlowLoader(ofdg.default_params(**kw), pool=pool, prefetch=3, extras=extras)
    it, pit = iter(loader), iter(plain)
    for _ in range(2):
        i0, i1, fl, more = next(it)
        p = next(pit)
        torch.cuda.current_stream().synchronize()
        assert set(more) == set(extras or ()) | {"flow_stats"}
        assert torch.equal(i0, p[0]) and torch.equal(i1, p[1]) and torch.equal(fl, p[2])  # the loader yields what it yielded
        occ = more["occ0"].cpu().numpy() if extras else None
        fsr.expect_equal(structured(ofdg, more["flow_stats"]), fsr.flow_stats(fl.cpu().numpy(), occ, 3.7))
        if extras:
            assert structured(ofdg, more["flow_stats"])["n_occluded"].all()
