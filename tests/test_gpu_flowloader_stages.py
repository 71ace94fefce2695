"""GPU tests of FlowLoader's stage order, through the public API only: with every post-processing option on at once - on the
frame, behind a crop and behind the spatial step - (a) every tensor of every batch is, byte for byte, what the public
Generator methods give when they are called by hand in the documented order (forward; spatial or crop; photo; erase;
object_table; flow_stats; flow_pyramid; boundaries; pack), and (b) the loader makes exactly those calls, once each and in
that order, all of a batch on the one stream next_stream() gave for it.  The order shows in the content: the eraser fills with
the mean of the photo-augmented frame, the statistics and the pyramid's weights see the occ0 it extended, the pack sees the
erased frames.  Five batches from three ring sets: sets 0 and 1 are rendered a second time, through the release path."""
import inspect

import pytest

pytestmark = pytest.mark.gpu

W, H, B = 128, 96, 2
WINDOW = (48, 96)
STEPS = 5
EXTRAS = ("flow1", "occ0", "occ1", "label0", "label1")
CONFIGS = ("frame", "crop", "spatial")
WRAPPED = ("forward", "crop", "spatial", "photo", "erase", "object_table", "flow_stats", "flow_pyramid", "boundaries", "pack")


def params(ofdg):
    return ofdg.default_params(width=W, height=H, mode=7, batch_size=B, sampler=1, seed=21)


def fill_pool(g):
    g.pool_synthetic(3, 2 * W, 2 * H, 11)


def erase_options(ofdg):
    return dict(ofdg.ERASE_RAFT, prob=1.0, min_size=8, max_size=30, frames=(0, 1))


def pack_options(ofdg):
    import torch
    return dict(image_dtype=torch.float16, layout=ofdg.PACK_NHWC, concat=True, rgb=True, flow_scale=0.05)


def loader_options(ofdg, config):
    import torch
    o = dict(extras=EXTRAS, photo=ofdg.PHOTO_FLOWNET, erase=erase_options(ofdg), stats=True, stats_bin_px=3.7, pyramid=2,
             pyramid_weights=True, boundaries=dict(frames=(0, 1), radius=4), pack=pack_options(ofdg))
    if config == "frame":
        o.update(objects=True)
    elif config == "crop":
        o.update(crop=WINDOW, crop_hflip=True, image_dtype=torch.uint8, flow_dtype=torch.float16, extras_compact=True)
    else:
        o.update(spatial=ofdg.SPATIAL_FLOWNET, spatial_size=WINDOW, spatial_hflip=True)
    return o


def make_loader(ofdg, config):
    return ofdg.FlowLoader(params(ofdg), pool=fill_pool, prefetch=3, **loader_options(ofdg, config))


def expected_calls(config):
    window = () if config == "frame" else (config,)
    table = ("object_table",) if config == "frame" else ()
    return ("forward",) + window + ("photo", "erase") + table + ("flow_stats", "flow_pyramid", "boundaries", "pack")


def expected_keys(config):
    keys = set(EXTRAS) | {"photo", "erase", "flow_stats", "flow_pyramid", "flow_pyramid_weights", "edge0", "dist0", "edge1", "dist1"}
    return keys | ({"objects", "object_counts"} if config == "frame" else {config})


def raw(t):
    """(dtype, shape, the bytes) of a tensor, of None, or of a list of tensors: bytes, so that a NaN cannot hide"""
    if t is None:
        return None
    if isinstance(t, (list, tuple)):
        return [raw(x) for x in t]
    return (str(t.dtype), tuple(t.shape), t.cpu().numpy().tobytes())


def raw_batch(batch):
    return [raw(t) for t in batch[:3]], {k: raw(v) for k, v in batch[3].items()}


def hand_step(ofdg, g, config, step):
    """Batch `step` by the public methods, in the documented order, on one stream of next_stream(): what the loader hands out"""
    import torch
    compact = config == "crop"
    fdt = torch.float16 if compact else None
    outs = ofdg.alloc_outputs(B, H, W, image_dtype=torch.uint8 if compact else None, flow_dtype=fdt)
    ex = ofdg.alloc_extras(B, H, W, EXTRAS, flow_dtype=fdt, occ_dtype=torch.uint8 if compact else None)
    planes, size, more = dict(zip(("image0", "image1", "flow"), outs), **ex), None, {}
    if config != "frame":
        size = WINDOW
        src, planes = planes, ofdg.alloc_crop(planes, *WINDOW)
        wrecs = torch.zeros((B, 4), dtype=torch.int32, device="cuda") if config == "crop" else \
            torch.zeros((B, ofdg.SPATIAL_REC_DOUBLES), dtype=torch.float64, device="cuda")
    ph, pw = size or (H, W)
    precs = torch.zeros((B, ofdg.PHOTO_REC_FLOATS), dtype=torch.float32, device="cuda")
    work, erecs = ofdg.alloc_erase(B)
    table = ofdg.alloc_object_table(B)
    rows = ofdg.alloc_flow_stats(B)
    pyr = ofdg.alloc_flow_pyramid(B, ph, pw, 2, fdt, True)
    bnd = ofdg.alloc_boundaries(B, ph, pw, frames=(0, 1))
    po = pack_options(ofdg)
    packed = ofdg.alloc_pack(B, ph, pw, image_dtype=po["image_dtype"], layout=po["layout"], concat=True)
    torch.cuda.synchronize()  # (the allocations were zeroed on torch's stream)

    s = g.next_stream()
    first = ofdg.shard_first_index(step, B, 1, 0)
    g.forward(*outs, s, extras=ex)
    if config == "crop":
        g.crop(src, planes, first_index=first, hflip=True, occ_window=True, recs_out=wrecs, stream=s)
    elif config == "spatial":
        g.spatial(src, planes, first_index=first, ranges=ofdg.SPATIAL_FLOWNET, hflip=True, occ_window=True, recs_out=wrecs, stream=s)
    g.photo((planes["image0"], planes["image1"]), first_index=first, ranges=ofdg.PHOTO_FLOWNET, recs_out=precs, stream=s, size=size)
    eo = erase_options(ofdg)
    g.erase((planes["image0"], planes["image1"]), occ=(planes["occ0"], planes["occ1"]), flow=(planes["flow"], planes["flow1"]),
            first_index=first, ranges={k: v for k, v in eo.items() if k in ofdg.ERASE_RANGES}, frames=eo["frames"], mark_occ=True,
            recs_out=erecs, work=work, stream=s, size=size)
    if config == "frame":
        g.object_table(ex["label0"], ex["label1"], *table, stream=s)
    g.flow_stats(planes["flow"], rows, occ=planes["occ0"], bin_px=3.7, stream=s, size=size)
    g.flow_pyramid(planes["flow"], 2, occ=planes["occ0"], out=pyr, stream=s, size=size)
    g.boundaries(planes["flow"], bnd["edge0"], bnd["dist0"], planes["label0"], planes["flow1"], bnd["edge1"], bnd["dist1"], planes["label1"],
                 radius=4, labels=True, stream=s, size=size)
    g.pack({k: planes[k] for k in ("image0", "image1", "flow")}, packed, flow_scale=po["flow_scale"], layout=po["layout"], concat=True,
           rgb=True, stream=s, size=size)
    g.synchronize(s)
    torch.cuda.synchronize()

    more.update({k: planes[k] for k in EXTRAS})
    if config != "frame":
        more[config] = wrecs
    else:
        more.update(objects=table[0], object_counts=table[1])
    more.update(photo=precs, erase=erecs, flow_stats=rows, flow_pyramid=pyr[0], flow_pyramid_weights=pyr[1], **bnd)
    return raw_batch((packed["image0"], None, packed["flow"], more))


@pytest.mark.parametrize("config", CONFIGS)
def test_loader_equals_the_hand_chain(ofdg, config):
    import torch
    g = ofdg.Generator(params(ofdg))
    fill_pool(g)
    want = [hand_step(ofdg, g, config, step) for step in range(STEPS)]
    del g
    it = iter(make_loader(ofdg, config))
    for step in range(STEPS):
        batch = next(it)
        torch.cuda.current_stream().synchronize()
        assert len(batch) == 4 and batch[1] is None and set(batch[3]) == expected_keys(config), (config, step, sorted(batch[3]))
        places, more = raw_batch(batch)
        for k, (a, b) in enumerate(zip(places, want[step][0])):
            assert a == b, "%s batch %d: place %d differs" % (config, step, k)
        for key in sorted(more):
            assert more[key] == want[step][1][key], "%s batch %d: %r differs" % (config, step, key)
    # (the batches differ from one another and the stages did something: what is compared is not five times the same bytes)
    assert want[0][0][0] != want[1][0][0] and want[0][1]["erase"] != want[3][1]["erase"] and want[1][1]["photo"] != want[4][1]["photo"]


@pytest.mark.parametrize("config", CONFIGS)
def test_loader_makes_each_call_once_in_order_on_one_stream(ofdg, config, monkeypatch):
    import torch
    log = []

    def recorded(name):
        inner = getattr(ofdg.Generator, name)
        sig = inspect.signature(inner)

        def call(self, *args, **kw):
            bound = sig.bind(self, *args, **kw)
            bound.apply_defaults()
            log.append((name, bound.arguments["stream"]))
            return inner(self, *args, **kw)
        return call

    for name in WRAPPED:
        monkeypatch.setattr(ofdg.Generator, name, recorded(name))
    inner_next = ofdg.Generator.next_stream

    def next_stream(self):
        s = inner_next(self)
        log.append(("next_stream", s))
        return s
    monkeypatch.setattr(ofdg.Generator, "next_stream", next_stream)

    it = iter(make_loader(ofdg, config))  # (the constructor enqueues the first two batches: they are in the log)
    for _ in range(STEPS):
        next(it)
    torch.cuda.current_stream().synchronize()
    batches = []
    for name, s in log:
        if name == "next_stream":
            batches.append((s, []))
        else:
            assert batches, "%s before the first next_stream()" % name
            batches[-1][1].append((name, s))
    assert len(batches) == 2 + STEPS  # prefetch - 1 in the constructor, one more with every next()
    for k, (s, calls) in enumerate(batches):
        assert tuple(name for name, _ in calls) == expected_calls(config), (config, k, calls)
        assert all(cs == s for _, cs in calls), (config, k, s, calls)
