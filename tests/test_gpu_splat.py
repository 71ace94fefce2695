"""GPU tests of the splat (ofdg_splat, include/ofdg.h): the device planes, keys and rows against ofdg_host_splat and against the
numpy restatement (tests/splat_reference.py), byte for byte, float bit for float bit and field for field - every format and
size, between guard bytes, twice over keys and rows full of 0xA5, with and without accumulation, subsets of frames, inputs and
outputs; behind forward_counter, the crop and the spatial step without synchronisation, in mode 9, with three calls in flight,
ten runs of one call, through the loader - and the refusals."""
import ctypes as C
import re

import numpy as np
import pytest

import splat_reference as sr

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 64  # bytes in front of and behind every written plane (keeps the 16-byte alignment)
KINDS = {"image": 3, "to_own": 2, "to_other": 2, "mask": 1, "fate": 1}


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
    return None if planes is None else tuple(None if t is None else torch.from_numpy(np.array(t)).cuda() for t in planes)


def to_host(planes):
    return tuple(None if t is None else t.cpu().numpy() for t in planes)


def out_buffers(n, H, W, dst_dtype, oflow_dtype, frames=(0, 1), names=sr.PLANES):
    """guarded destinations by splat_key name, filled with 7"""
    dts = {"image": dst_dtype, "to_own": oflow_dtype, "to_other": oflow_dtype, "mask": "uint8", "fate": "uint8"}
    return {sr.key(name, f): guarded(np.full((n, KINDS[name], H, W), 7, dts[name])) for f in frames for name in names}


def key_buffers(n, H, W, frames=(0, 1)):
    """guarded key planes, every byte 0xA5: the call has to clear them"""
    return [guarded(np.full((n, H, W), -0x5A5A5A5B, np.int32)) if f in frames else None for f in range(2)]


def rows_buffer(n, fill=0):
    return guarded(np.full((n, 128), fill, np.uint8))


def recs_buffer(recs):
    return guarded(np.array(recs, np.int32))


def keys_of(pair):
    return tuple(None if k is None else k[1] for k in pair)


def rows_of(ofdg, t):
    return ofdg.splat_numpy(t)["rows"]


def same_rows(a, b):
    return all(np.array_equal(a[k], b[k]) for k in sr.FIELDS)


def same_keys(got, want):
    return all((g is None) == (w is None) and (g is None or np.array_equal(g.cpu().numpy().view(np.uint32), w)) for g, w in zip(got, want))


def expect_planes(got, want, what):
    for k, t in got.items():
        assert sr.equal_bits(t, want[k]), "%s: %s" % (what, k)


# A workgroup owns a 64 x 16 tile, a lane four pixels, a pair of lanes one 8-byte store of a uint8 row.  8x2 and 24x6: one
# partial tile.  72x40: 2 x 3 tiles, the second column 8 pixels wide (narrower than a lane pair's 16-byte float32 stores side by
# side).  264x200: 5 x 13 tiles, partial last ones both ways, uint8 rows 8 mod 16 wide.  Sample 0 keeps a tile's targets
# together, sample 1 sprays them over the whole plane.
@pytest.mark.parametrize("W,H", sr.SIZES)
@pytest.mark.parametrize("src_dtype,dst_dtype,flow_dtype", sr.FORMATS)
def test_device_equals_host_twin_and_restatement(ofdg, W, H, src_dtype, dst_dtype, flow_dtype):
    """Every written plane, the keys, the rows and the records lie between 0xA5 guards; the inputs stay as they are.  Each call
    runs twice over keys and rows full of 0xA5 (the call clears them), then with accumulation on top."""
    import torch
    g = make_gen(ofdg, 64, 32)  # (the context's own frame is another: the job gives the size)
    occ_dtype = "uint8" if flow_dtype == "float16" else "float32"
    T = 256 if src_dtype == "uint8" else 128
    images, flows, labels, occ, recs, forms, keys, rows = sr.case(W, H, src_dtype, flow_dtype, occ_dtype, T)
    want = forms[dst_dtype, flow_dtype]
    what = "%dx%d T %d %s to %s, flow %s, occ %s" % (W, H, T, src_dtype, dst_dtype, flow_dtype, occ_dtype)
    host, host_keys, host_rows, _ = ofdg.host_splat(images, flows, labels, occ, recs=recs, dst_dtype=dst_dtype, oflow_dtype=flow_dtype)
    expect_planes(host, want, what + ": twin against restatement")
    assert same_rows(host_rows, rows) and all(np.array_equal(host_keys[f], keys[f]) for f in range(2)), what
    d_img, d_flow, d_lab, d_occ, d_recs = to_dev(images), to_dev(flows), to_dev(labels), to_dev(occ), to_dev((recs,))[0]
    for _ in range(2):
        bufs = out_buffers(sr.N, H, W, dst_dtype, flow_dtype)
        kbufs = key_buffers(sr.N, H, W)
        rraw, rout = rows_buffer(sr.N, FILL)
        uraw, used = recs_buffer(np.full((sr.N, 4), 7))
        every = list(bufs.values()) + kbufs + [(rraw, rout), (uraw, used)]
        g.splat(d_img, d_flow, d_lab, d_occ, recs=d_recs, out={k: t for k, (_, t) in bufs.items()}, keys=keys_of(kbufs), rows=rout, recs_out=used, size=(H, W))
        torch.cuda.synchronize()
        assert guards_intact(every), what
        got = {k: t.cpu().numpy() for k, (_, t) in bufs.items()}
        expect_planes(got, want, what + ": device against restatement")
        expect_planes(got, host, what + ": device against twin")
        assert same_keys(keys_of(kbufs), keys) and same_rows(rows_of(ofdg, rout), rows) and np.array_equal(used.cpu().numpy(), recs), what
        g.splat(d_img, d_flow, d_lab, d_occ, recs=d_recs, keys=keys_of(kbufs), rows=rout, accumulate=True, size=(H, W))
        torch.cuda.synchronize()
        assert same_rows(rows_of(ofdg, rout), sr.add_rows(rows, rows)) and same_keys(keys_of(kbufs), keys) and guards_intact(every), what + ": accumulated"
    for got, src, name in ((to_host(d_img), images, "images"), (to_host(d_flow), flows, "flows"), (to_host(d_lab), labels, "labels"), (to_host(d_occ), occ, "maps")):
        for f in range(2):
            assert sr.equal_bits(got[f], src[f]), what + ": the " + name
    assert np.array_equal(d_recs.cpu().numpy(), recs)


@pytest.mark.parametrize("T", [0, 1, 77, 255])
def test_the_other_fractions(ofdg, T):
    import torch
    W, H = 72, 40
    g = make_gen(ofdg, W, H)
    images, flows, labels, occ, recs, forms, keys, rows = sr.case(W, H, "uint8", "float32", "uint8", T)
    out, dkeys, drows, used = ofdg.alloc_splat(sr.N, H, W, (0, 1), image_dtype=torch.uint8)
    g.splat(to_dev(images), to_dev(flows), to_dev(labels), to_dev(occ), recs=to_dev((recs,))[0], out=out, keys=dkeys, rows=drows, recs_out=used)
    torch.cuda.synchronize()
    expect_planes({k: t.cpu().numpy() for k, t in out.items()}, forms["uint8", "float32"], "T %d" % T)
    assert same_keys(dkeys, keys) and same_rows(rows_of(ofdg, drows), rows) and np.array_equal(used.cpu().numpy(), recs)


@pytest.mark.parametrize("src_dtype,dst_dtype,flow_dtype", [sr.FORMATS[0], sr.FORMATS[7], sr.FORMATS[5]])
def test_subsets_of_frames_and_outputs(ofdg, src_dtype, dst_dtype, flow_dtype):
    """A frame alone, an output alone, the rows alone, the keys alone, no labels and no maps: what was not asked for is not
    touched, and fields whose inputs are absent stay 0."""
    import torch
    W, H = 72, 40
    g = make_gen(ofdg, W, H)
    images, flows, labels, occ, recs, forms, keys, rows = sr.case(W, H, src_dtype, flow_dtype, "uint8", 128)
    want = forms[dst_dtype, flow_dtype]
    d_img, d_flow, d_lab, d_occ, d_recs = to_dev(images), to_dev(flows), to_dev(labels), to_dev(occ), to_dev((recs,))[0]
    for sel in (0, 1):
        for names, with_rows in ((("image",), False), (("to_own",), False), (("to_other",), False), (("mask",), False), (("fate",), False), ((), True), ((), False),
                                 (sr.PLANES, True)):
            bufs = out_buffers(sr.N, H, W, dst_dtype, flow_dtype)
            kbufs = key_buffers(sr.N, H, W)
            rraw, rout = rows_buffer(sr.N, 7)
            dk = tuple(kbufs[f][1] if f == sel else None for f in range(2))
            g.splat(d_img, d_flow, d_lab, d_occ, recs=d_recs, out={sr.key(n_, sel): bufs[sr.key(n_, sel)][1] for n_ in names}, keys=dk,
                    rows=rout if with_rows else None, frames=(sel,))
            torch.cuda.synchronize()
            assert guards_intact(list(bufs.values()) + kbufs + [(rraw, rout)])
            for k, (_, t) in bufs.items():
                name, f = ofdg._SPLAT_KEYS[k]
                if f == sel and name in names:
                    assert sr.equal_bits(t.cpu().numpy(), want[k]), (sel, names, k)
                else:
                    assert bool((t == 7).all()), (sel, names, k)
            assert np.array_equal(kbufs[sel][1].cpu().numpy().view(np.uint32), keys[sel]) and bool((kbufs[1 - sel][0] == FILL).all()), (sel, names)
            if with_rows:
                got = rows_of(ofdg, rout)
                assert same_rows(got[:, sel], rows[:, sel]) and not np.ascontiguousarray(got[:, 1 - sel]).view(np.uint8).any()
            else:
                assert bool((rout == 7).all())
    # flows alone: no labels (the lowest index wins), no maps (the split counts stay 0), no frames
    lean, lean_keys, lean_rows = sr.splat(None, flows, None, None, recs, (0, 1), oflow_dtype=flow_dtype)
    bufs = out_buffers(sr.N, H, W, dst_dtype, flow_dtype, names=("to_own", "to_other", "mask", "fate"))
    kbufs = key_buffers(sr.N, H, W)
    rraw, rout = rows_buffer(sr.N, FILL)
    g.splat(None, d_flow, None, None, recs=d_recs, out={k: t for k, (_, t) in bufs.items()}, keys=keys_of(kbufs), rows=rout)
    torch.cuda.synchronize()
    got = rows_of(ofdg, rout)
    assert same_rows(got, lean_rows) and same_keys(keys_of(kbufs), lean_keys) and not any(got[k].any() for k in sr.FIELDS if "visible" in k or "hidden" in k)
    expect_planes({k: t.cpu().numpy() for k, (_, t) in bufs.items()}, lean, "flows alone")
    assert guards_intact(list(bufs.values()) + kbufs + [(rraw, rout)])


PLANE_NAMES = ("image0", "image1", "flow")
EXTRAS = ("flow1", "occ0", "occ1", "label0", "label1")


def rendered(ofdg, g, B, compact, then=None, extras=EXTRAS, explicit=False):
    """forward_counter on the internal stream - named as STREAM_OWN, or, explicit, by its handle - and `then(planes, True, more,
    stream)` behind it, nothing waited for in between"""
    import torch
    W, H = g.params.width, g.params.height
    kw = dict(image_dtype=torch.uint8, flow_dtype=torch.float16) if compact else {}
    xkw = dict(flow_dtype=torch.float16, occ_dtype=torch.uint8) if compact else {}
    outs = ofdg.alloc_outputs(B, H, W, **kw)
    ex = ofdg.alloc_extras(B, H, W, extras, **xkw) if extras else None
    src = dict(zip(PLANE_NAMES, outs), **(ex or {}))
    more = then(src, False) if then else None
    torch.cuda.synchronize()  # (the allocations were zeroed on torch's stream)
    s = g.next_stream() if explicit else ofdg.STREAM_OWN
    g.forward_counter(0, B, *outs, s, extras=ex)
    if then:
        then(src, True, more, s)
    g.synchronize(s)
    torch.cuda.synchronize()
    return src, more


def pairs_of(p):
    return ((p["image0"], p["image1"]), (p["flow"], p.get("flow1")), (p.get("label0"), p.get("label1")), (p.get("occ0"), p.get("occ1")))


def twin_of(ofdg, p, frames=(0, 1), **kw):
    """ofdg_host_splat on downloaded planes (a dict by name)"""
    h = {k: v.cpu().numpy() for k, v in p.items()}
    return ofdg.host_splat(*pairs_of(h), frames=frames, oflow_dtype=h["flow"].dtype, **kw)


def splat_all(ofdg, g, p, more, stream=None, **kw):
    out, keys, rows, recs = more
    g.splat(*pairs_of(p), out=out, keys=keys, rows=rows, recs_out=recs, stream=ofdg.STREAM_OWN if stream is None else stream, **kw)


def expect_twin(ofdg, more, host, what):
    out, keys, rows, recs = more
    h_out, h_keys, h_rows, h_recs = host
    assert set(out) == set(h_out)
    expect_planes({k: t.cpu().numpy() for k, t in out.items()}, h_out, what)
    assert same_keys(keys, h_keys) and same_rows(rows_of(ofdg, rows), h_rows) and np.array_equal(recs.cpu().numpy(), h_recs), what


@pytest.mark.parametrize("compact,own", [(False, True), (True, True), (False, False)])
def test_behind_forward_counter(ofdg, compact, own):
    """Mode 7, 128x64, B = 3: forward_counter with extras, then the splat with drawn fractions - on STREAM_OWN, or on the
    internal stream named by its handle - with no synchronisation in between, against the twin on the downloaded planes."""
    import torch
    W, H, B = 128, 64, 3
    g = make_gen(ofdg, W, H, 7, pool=True, sampler=1, seed=5, batch_size=B)
    draw = dict(t=(0.25, 1.0), first_index=(1 << 32) + 6)

    def then(src, enqueue, more=None, s=None):
        if not enqueue:
            return ofdg.alloc_splat(B, H, W, (0, 1), image_dtype=torch.uint8 if compact else None, flow_dtype=torch.float16 if compact else None)
        splat_all(ofdg, g, src, more, s, **draw)

    src, more = rendered(ofdg, g, B, compact, then, explicit=not own)
    host = twin_of(ofdg, src, seed=5, **draw)
    expect_twin(ofdg, more, host, "behind forward_counter")
    r = host[2]
    assert r["n_filled"].all() and r["n_holes"].any() and r["n_covered"].any() and r["n_covered_hidden"].any() and r["n_hole_other_hidden"].any()
    assert host[3].tolist() == [ofdg.splat_draw(5, (1 << 32) + 6 + i, (0.25, 1.0)).tolist() for i in range(B)] and (host[1][0] >> 24).max() > 0


@pytest.mark.parametrize("window", ["crop", "spatial"])
def test_behind_the_window(ofdg, window):
    """forward_counter, the 96x48 window and the splat of the window's planes on one stream, no synchronisation."""
    W, H, B, wh, ww = 128, 64, 3, 48, 96
    g = make_gen(ofdg, W, H, 7, pool=True, sampler=1, seed=6, batch_size=B)

    def then(src, enqueue, more=None, s=None):
        if not enqueue:
            return ofdg.alloc_crop(src, wh, ww), ofdg.alloc_splat(B, wh, ww, (0, 1))
        dst, sp = more
        if window == "crop":
            g.crop(src, dst, first_index=8, occ_window=True, stream=ofdg.STREAM_OWN)
        else:
            g.spatial(src, dst, first_index=8, ranges=ofdg.SPATIAL_FLOWNET, occ_window=True, stream=ofdg.STREAM_OWN)
        splat_all(ofdg, g, dst, sp, t=0.5, size=(wh, ww))

    _, (dst, sp) = rendered(ofdg, g, B, False, then)
    expect_twin(ofdg, sp, twin_of(ofdg, dst, t=0.5), "behind " + window)


def test_mode_9_frame_0_only(ofdg):
    """Mode 9 has no flow1, no labels and no maps: frame 0 works, every priority 0; frame 1 is refused by name."""
    W, H, B = 128, 64, 2
    g = make_gen(ofdg, W, H, 9, pool=True, sampler=1, seed=3, batch_size=B)
    g.warp_generate(1, 3)

    def then(src, enqueue, more=None, s=None):
        if not enqueue:
            return ofdg.alloc_splat(B, H, W, (0,))
        splat_all(ofdg, g, src, more, t=1.0)

    src, more = rendered(ofdg, g, B, False, then, extras=None)
    host = twin_of(ofdg, src, frames=(0,), t=1.0)
    expect_twin(ofdg, more, host, "mode 9")
    assert host[2]["n_filled"][:, 0].all() and not (host[1][0] >> 24).any() and more[1][1] is None
    _, keys, _, _ = ofdg.alloc_splat(B, H, W, (0, 1), outputs=("keys",))
    with pytest.raises(RuntimeError, match=r"ofdg_splat: flow\[1\]: a flagged frame needs its flow"):
        g.splat((src["image0"], src["image1"]), (src["flow"], None), keys=keys, frames=(0, 1), t=1.0)


def test_three_calls_in_flight(ofdg):
    """Two caller streams and STREAM_OWN, each with planes, keys and rows of its own, synchronised once at the end."""
    import torch
    W, H = 72, 40
    g = make_gen(ofdg, W, H, 7, pool=True, sampler=1, batch_size=1)
    rendered(ofdg, g, 1, False, extras=None)  # (STREAM_OWN needs a former forward call)
    cases = [sr.case(W, H, s, f, "uint8", T) for s, f, T in (("uint8", "float32", 256), ("float32", "float16", 128), ("uint8", "float16", 77))]
    streams = [torch.cuda.Stream(), torch.cuda.Stream(), None]
    runs = []
    for c, s in zip(cases, streams):
        dev = tuple(to_dev(t) for t in c[:4]) + (to_dev((c[4],))[0],)
        runs.append((dev, ofdg.alloc_splat(sr.N, H, W, (0, 1)), c, s))
    torch.cuda.synchronize()
    for (d_img, d_flow, d_lab, d_occ, d_recs), (out, keys, rows, used), _, s in runs:
        g.splat(d_img, d_flow, d_lab, d_occ, recs=d_recs, out=out, keys=keys, rows=rows, recs_out=used, stream=ofdg.STREAM_OWN if s is None else s.cuda_stream)
    torch.cuda.synchronize()
    g.synchronize(ofdg.STREAM_OWN)
    torch.cuda.synchronize()
    for _, (out, keys, rows, used), c, _ in runs:
        expect_planes({k: t.cpu().numpy() for k, t in out.items()}, c[5]["float32", "float32"], "in flight")
        assert same_keys(keys, c[6]) and same_rows(rows_of(ofdg, rows), c[7]) and np.array_equal(used.cpu().numpy(), c[4])


def test_ten_runs_give_the_same_bytes(ofdg):
    """The point of the integer maximum: the sprayed sample, where hundreds of sources race for a target, ten times into fresh
    buffers."""
    import torch
    W, H = 72, 40
    g = make_gen(ofdg, W, H)
    images, flows, labels, occ, recs, forms, keys, rows = sr.case(W, H, "float32", "float32", "float32", 256)
    dev = (to_dev(images), to_dev(flows), to_dev(labels), to_dev(occ))
    d_recs = to_dev((recs,))[0]
    first = None
    for k in range(10):
        out, dkeys, drows, used = ofdg.alloc_splat(sr.N, H, W, (0, 1))
        g.splat(*dev, recs=d_recs, out=out, keys=dkeys, rows=drows, recs_out=used)
        torch.cuda.synchronize()
        got = [out[n_].cpu().numpy().tobytes() for n_ in sorted(out)] + [t.cpu().numpy().tobytes() for t in dkeys] + [drows.cpu().numpy().tobytes()]
        first = first or got
        assert got == first, k
    assert same_keys(dkeys, keys) and same_rows(rows_of(ofdg, drows), rows)


LOADER = dict(extras=EXTRAS, crop=(48, 96))
SEED, BATCH = 21, 2


def loader_batches(ofdg, count, start=0, batch=BATCH, rank=0, world=1, **kw):
    import torch
    p = ofdg.default_params(width=128, height=64, mode=7, batch_size=batch, sampler=1, seed=SEED, rank=rank, world_size=world)
    out = []
    loader = ofdg.FlowLoader(p, pool=lambda g: g.pool_synthetic(3, 256, 128, 11), prefetch=3, start=start, **dict(LOADER, **kw))
    it = iter(loader)
    for _ in range(count):
        batch_ = next(it)
        torch.cuda.current_stream().synchronize()
        host = lambda t: {n_: host(v) for n_, v in t.items()} if isinstance(t, dict) else t.cpu().numpy()  # noqa: E731
        out.append(tuple(host(t) for t in batch_))
    return out


def expect_loader_batch(ofdg, b, plain, first_index, t, what):
    """batch b's "splat" against the by-hand chain: the twin on the plain loader's cropped planes with the drawn records"""
    x, s = plain[3], b[3]["splat"]
    want_recs = np.array([ofdg.splat_draw(SEED, first_index + i, t) for i in range(len(b[0]))], np.int32)
    out, keys, rows, used = ofdg.host_splat((plain[0], plain[1]), (plain[2], x["flow1"]), (x["label0"], x["label1"]), (x["occ0"], x["occ1"]), recs=want_recs)
    assert np.array_equal(s["recs"], want_recs) and np.array_equal(used, want_recs), what
    assert set(s) == set(out) | {"keys0", "keys1", "rows", "recs"}, what
    expect_planes({k: s[k] for k in out}, out, what)
    assert all(np.array_equal(s["keys%d" % f].view(np.uint32), keys[f]) for f in range(2)) and same_rows(rows_of(ofdg, s["rows"]), rows), what


def test_the_loader_splats_the_sharp_unerased_window(ofdg):
    """splat= with and without reproject=, motion_blur=, photo= and erase= around it: planes, keys and rows equal the twin's on
    the plain loader's cropped planes with the records splat_draw gives for (seed, global index) - two consecutive batches and
    a third across the prefetch=3 ring.  Resume at start=2 gives batch 2; two ranks give the halves of a batch of twice the
    size; without splat= the batch has the names it had."""
    t = (0.25, 0.75)
    opts = dict(t=t)
    plain = loader_batches(ofdg, 4)
    assert len(plain[0]) == 4 and "splat" not in plain[0][3]
    around = dict(reproject=dict(outputs=("rows",)), motion_blur=dict(ofdg.MBLUR_DEFAULT, prob=1.0), photo=ofdg.PHOTO_FLOWNET, erase=dict(ofdg.ERASE_RAFT, prob=1.0))
    for kw, first, count in ((dict(splat=opts), 0, 4), (dict(splat=opts, **around), 0, 2), (dict(splat=opts), 2, 1)):
        got = loader_batches(ofdg, count, start=first, **kw)
        for k, b in enumerate(got):
            expect_loader_batch(ofdg, b, plain[first + k], BATCH * (first + k), t, (sorted(kw), k))
            if len(kw) == 1:  # the stage changes nothing of the batch itself
                assert all(sr.equal_bits(b[i], plain[first + k][i]) for i in range(3))
                assert all(sr.equal_bits(b[3][n_], plain[first + k][3][n_]) for n_ in plain[first + k][3])
    assert len({tuple(r) for b in loader_batches(ofdg, 3, splat=opts) for r in b[3]["splat"]["recs"]}) > 1
    # two ranks: rank r's batch k holds samples 2 B k + r B ... of the stream, with their records
    whole = loader_batches(ofdg, 2, batch=2 * BATCH, splat=opts)
    for rank in range(2):
        part = loader_batches(ofdg, 2, rank=rank, world=2, splat=opts)
        for k in range(2):
            lo = rank * BATCH
            assert ofdg.shard_first_index(k, BATCH, 2, rank) == 2 * BATCH * k + lo
            for name, v in part[k][3]["splat"].items():
                assert sr.equal_bits(v, whole[k][3]["splat"][name][lo:lo + BATCH]), (rank, k, name)
    # a fixed fraction, one frame, chosen outputs
    got = loader_batches(ofdg, 1, splat=dict(t=1.0, frames=(0,), outputs=("image", "mask", "rows")))
    s = got[0][3]["splat"]
    assert set(s) == {"image0", "mask0", "keys0", "rows", "recs"} and s["recs"].tolist() == [[256, 0, 0, 0]] * BATCH
    with pytest.raises(ValueError, match="splat= of frame 1 reads flow1"):
        ofdg.FlowLoader(ofdg.default_params(width=128, height=64, mode=7, batch_size=2, sampler=1), extras=("occ0",), splat=dict(frames=(0, 1)))


def test_refusals_enqueue_nothing(ofdg):
    """Every refusal names its field, leaves planes, keys, rows and records as they were, and a valid call on the same context
    still works."""
    import torch
    W, H = 24, 6
    g = make_gen(ofdg, W, H)
    images, flows, labels, occ, recs, forms, keys, rows = sr.case(W, H, "uint8", "float32", "uint8", 256)
    want = forms["uint8", "float32"]
    d_img, d_flow, d_lab, d_occ, d_recs = to_dev(images), to_dev(flows), to_dev(labels), to_dev(occ), to_dev((recs,))[0]
    bufs = out_buffers(sr.N, H, W, "uint8", "float32")
    out = {k: t for k, (_, t) in bufs.items()}
    kbufs = key_buffers(sr.N, H, W)
    dkeys = keys_of(kbufs)
    rraw, rout = rows_buffer(sr.N, 7)
    uraw, used = recs_buffer(np.full((sr.N, 4), 7))
    with pytest.raises(RuntimeError, match="ofdg_splat: stream: OFDG_STREAM_OWN before any render / forward call"):
        g.splat(d_img, d_flow, d_lab, d_occ, recs=d_recs, out=out, keys=dkeys, rows=rout, recs_out=used, stream=ofdg.STREAM_OWN)
    L, h = ofdg.lib(), g.h
    codes = (ofdg.FMT_U8, ofdg.FMT_U8, ofdg.FMT_F32, ofdg.FMT_F32, ofdg.FMT_U8)

    def job(**kw):
        j = ofdg._splat_job(d_img, d_flow, d_lab, d_occ, out, dkeys, rout.data_ptr(), lambda t: t.data_ptr(), codes, (0, 0), (0, 1), (0, 256), d_recs.data_ptr(),
                            used.data_ptr(), 0, 0, False)
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(j, k)[v[0]] = v[1]
            else:
                setattr(j, k, v)
        return j

    refusals = [(dict(img_fmt=ofdg.FMT_F16), "img_fmt must be"), (dict(dst_fmt=7), "dst_fmt must be"), (dict(flow_fmt=ofdg.FMT_U8), "flow_fmt must be"),
                (dict(oflow_fmt=ofdg.FMT_U8), "oflow_fmt must be"), (dict(occ_fmt=ofdg.FMT_F16), "occ_fmt must be"), (dict(flags=11), "flags holds unknown bits"),
                (dict(flags=4), "flags: no frame is flagged"), (dict(flags=1), "flags: frame 1 has a pointer but is not flagged"),
                (dict(reserved=(1, 1)), "reserved must be 0"), (dict(width=W), "width and height must both be 0 or both be set"),
                (dict(width=12, height=6), "width must be a multiple of 8"), (dict(width=4096, height=4096), r"width \* height must be at most 2\^24 - 1"),
                (dict(flow=(0, None)), r"flow\[0\]: a flagged frame needs its flow"), (dict(keys=(1, None)), r"keys\[1\]: a flagged frame needs its key plane"),
                (dict(img=(1, None)), r"img\[1\]: image of frame 1 needs its frame"),
                (dict(recs=None, t_min_q8=-1), "t_min_q8 must lie in 0..256"), (dict(recs=None, t_max_q8=257), "t_max_q8 must lie in 0..256"),
                (dict(recs=None, t_min_q8=9, t_max_q8=8), "t_min_q8 must not be above t_max_q8"),
                (dict(image=(0, out["mask0"].data_ptr())), "a written range overlaps another range of the job"),
                (dict(keys=(1, d_flow[0].data_ptr())), "a written range overlaps another range of the job"),
                (dict(recs_out=d_recs.data_ptr()), "a written range overlaps another range of the job"),
                (dict(rows=rout.data_ptr() + 8), "rows must be 16-byte aligned"), (dict(mask=(0, out["mask0"].data_ptr() + 4)), r"mask\[0\] must be 16-byte aligned"),
                (dict(keys=(0, dkeys[0].data_ptr() + 8)), r"keys\[0\] must be 16-byte aligned"), (dict(to_own=(1, out["to_own1"].data_ptr() + 4)), r"to_own\[1\] must be 16-byte aligned"),
                (dict(recs=d_recs.data_ptr() + 4), "recs must be 16-byte aligned"), (dict(recs_out=used.data_ptr() + 8), "recs_out must be 16-byte aligned"),
                (dict(flow=(1, d_flow[1].data_ptr() + 4)), r"flow\[1\] must be 16-byte aligned"), (dict(label=(0, d_lab[0].data_ptr() + 2)), r"label\[0\] must be 4-byte aligned"),
                (dict(img=(0, d_img[0].data_ptr() + 1)), r"img\[0\] must be 4-byte aligned")]
    for kw, text in refusals:
        assert L.ofdg_splat(h, C.byref(job(**kw)), sr.N, None) == ofdg.EINVAL, kw
        assert re.search("^ofdg_splat: " + text, L.ofdg_last_error(h).decode()), (kw, L.ofdg_last_error(h))
    assert L.ofdg_splat(h, None, sr.N, None) == ofdg.EINVAL and L.ofdg_splat(h, C.byref(job()), 0, None) == ofdg.EINVAL
    torch.cuda.synchronize()
    every = list(bufs.values()) + kbufs + [(rraw, rout), (uraw, used)]
    assert all(bool((t == 7).all()) for t in out.values()) and bool((rout == 7).all()) and bool((used == 7).all()) and guards_intact(every)
    assert all(bool((raw == FILL).all()) for raw, _ in kbufs)
    g.splat(d_img, d_flow, d_lab, d_occ, recs=d_recs, out=out, keys=dkeys, rows=rout, recs_out=used)
    torch.cuda.synchronize()
    expect_planes({k: t.cpu().numpy() for k, t in out.items()}, want, "the valid call afterwards")
    assert same_keys(dkeys, keys) and same_rows(rows_of(ofdg, rout), rows) and guards_intact(every)
