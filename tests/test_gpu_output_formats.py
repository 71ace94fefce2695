"""GPU tests of the compact output formats (ofdg_render_fmt / ofdg_forward_fmt / ofdg_forward_counter_fmt): uint8 frames
and an fp16 flow.  The definition (include/ofdg.h) makes the plain call the reference and every comparison exact: a uint8
frame byte widened to float32 is what the plain call stores, an fp16 flow value is the plain call's float32 value
converted once, round to nearest even (numpy's astype(float16)); NaNs compare equal whatever their payload."""
import ctypes as C
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FORMS = (("u8", "f32"), ("u8", "f16"), ("f32", "f16"))
SENTINEL = 0xA5


def dtypes(form):
    import torch
    return {"u8": torch.uint8, "f32": torch.float32}[form[0]], {"f16": torch.float16, "f32": torch.float32}[form[1]]


def alloc(ofdg, n, H, W, form=("f32", "f32")):
    """Outputs in `form`, every byte set to the sentinel."""
    import torch
    idt, fdt = dtypes(form)
    outs = ofdg.alloc_outputs(n, H, W, image_dtype=idt, flow_dtype=fdt)
    for t in outs:
        t.view(torch.uint8).fill_(SENTINEL)
    return outs


def host(outs):
    return [t.cpu().numpy() for t in outs]


def bits(a):
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def same_bytes(xs, ys):
    return all(a.dtype == b.dtype and np.array_equal(bits(a), bits(b)) for a, b in zip(xs, ys))


def check_form(plain, got, form, what=""):
    """plain, got: [image0, image1, flow] numpy arrays of the plain call and of the call in `form`."""
    for k in (0, 1):
        if form[0] == "u8":
            assert got[k].dtype == np.uint8
            wide = got[k].astype(np.float32)
        else:
            assert got[k].dtype == np.float32
            wide = got[k]
        bad = bits(wide) != bits(plain[k])
        assert not bad.any(), "%s image%d (%s): %d values differ" % (what, k, form[0], bad.sum())
    if form[1] == "f16":
        assert got[2].dtype == np.float16
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)  # |flow| > 65504 -> inf is part of the definition
            want = plain[2].astype(np.float16)
        bad = ~((got[2] == want) | (np.isnan(got[2]) & np.isnan(want)))
        assert not bad.any(), "%s flow (f16): %d values are not the float32 flow rounded to nearest even" % (what, bad.sum())
    else:
        assert got[2].dtype == np.float32
        bad = bits(got[2]) != bits(plain[2])
        assert not bad.any(), "%s flow (f32): %d values differ" % (what, bad.sum())


def make_gen(ofdg, W, H, mode, pool=(3, None, None, 11), **kw):
    g = ofdg.Generator(ofdg.default_params(width=W, height=H, mode=mode, **kw))
    n, pw, ph, seed = pool
    g.pool_synthetic(n, pw or 2 * W, ph or 2 * H, seed)
    return g


def render(ofdg, g, tasks, n, bps, n_bps, form=("f32", "f32"), stream=0):
    import torch
    outs = alloc(ofdg, n, g.params.height, g.params.width, form)
    g.render(tasks, n, bps, n_bps, *outs, stream)
    g.synchronize(0 if stream == ofdg.STREAM_OWN else stream)
    torch.cuda.synchronize()
    return host(outs)


# ---- 1. host sampler, every compact form against the plain call on the same tasks ----
@pytest.mark.parametrize("W,H,mode,aa", [(W, H, m, 1) for (W, H) in ((128, 96), (160, 100)) for m in (1, 2, 3, 5, 7, 13)]
                         + [(512, 384, 7, 1), (512, 384, 7, 0), (136, 100, 7, 1)])
def test_compact_forms_match_the_plain_call_host_sampler(ofdg, W, H, mode, aa):
    B = 1 if W == 512 else 2
    g = make_gen(ofdg, W, H, mode, use_antialiasing=aa)
    tasks, bps, n = g.sample(B)
    plain = render(ofdg, g, tasks, B, bps, n)
    assert np.abs(plain[2]).max() > 0 and plain[0].max() > 0
    for form in FORMS:
        check_form(plain, render(ofdg, g, tasks, B, bps, n, form), form, "mode %d %dx%d" % (mode, W, H))


@pytest.mark.parametrize("W,H", [(128, 96), (160, 100)])
def test_compact_forms_match_the_plain_call_mode9(ofdg, W, H):
    """Mode 9: the crop serving order is part of a context's state, so every form renders on a context of its own, built
    like the plain one (same warp fields, same tasks)."""
    B = 4

    def make():
        g = make_gen(ofdg, W, H, 9)
        g.warp_generate(1, seed=4)
        return g

    g = make()
    tasks, bps, n = g.sample(B)
    deforming = 0
    for i in range(B):
        idx = [tasks[i].background] + list(range(tasks[i].first_object, tasks[i].first_object + tasks[i].n_objects))
        deforming += any(bps[j].do_warpfield_deformation for j in idx)
    assert deforming >= 1, "no sample of the batch deforms: the test would pass on the rigid paths alone"
    plain = render(ofdg, g, tasks, B, bps, n)
    for form in FORMS:
        check_form(plain, render(ofdg, make(), tasks, B, bps, n, form), form, "mode 9 %dx%d" % (W, H))


# ---- 2. counter sampler with the background preparation ----
@pytest.mark.parametrize("W,H,B,mode,nobj,first", [(512, 384, 32, 5, 16, 640), (128, 96, 128, 7, 0, 1000)])
def test_forward_counter_compact_against_plain(ofdg, W, H, B, mode, nobj, first):
    import torch
    g = make_gen(ofdg, W, H, mode, pool=(8, 1024, 768, 2024) if W == 512 else (3, None, None, 11), sampler=1, seed=20261003,
                 batch_size=B, num_objects=nobj, background_prep=1)
    outs = alloc(ofdg, B, H, W)
    g.forward_counter(first, B, *outs)
    g.synchronize()
    plain = host(outs)
    del outs
    for form in FORMS:
        outs = alloc(ofdg, B, H, W, form)
        g.forward_counter(first, B, *outs)
        g.synchronize()
        torch.cuda.synchronize()
        got = host(outs)
        del outs
        for s in range(B):  # every sample
            check_form([a[s] for a in plain], [a[s] for a in got], form, "sample %d" % s)


# ---- 3. forward(): the context's own step counter ----
@pytest.mark.parametrize("sampler", [0, 1])
def test_forward_compact_steps_like_plain(ofdg, sampler):
    W, H, B = 128, 96, 2
    form = ("u8", "f16")
    gp = make_gen(ofdg, W, H, 7, sampler=sampler, seed=5, batch_size=B)
    gc = make_gen(ofdg, W, H, 7, sampler=sampler, seed=5, batch_size=B)
    for k in range(3):
        a, b = alloc(ofdg, B, H, W), alloc(ofdg, B, H, W, form)
        gp.forward(*a)
        gc.forward(*b)
        gp.synchronize()
        gc.synchronize()
        check_form(host(a), host(b), form, "step %d" % k)
        assert gp.step == gc.step == k + 1


# ---- 4. nothing else is written ----
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("W,H,mode", [(128, 96, 7), (136, 100, 7), (128, 96, 9)])
def test_compact_call_writes_its_own_slots_only(ofdg, form, W, H, mode):
    import torch
    B = 2
    g = make_gen(ofdg, W, H, mode)
    if mode == 9:
        g.warp_generate(1, seed=4)
    tasks, bps, n = g.sample(B)
    big = alloc(ofdg, B + 2, H, W, form)  # one guard sample slot in front, one behind
    g.render(tasks, B, bps, n, *[t[1:B + 1] for t in big])
    g.synchronize()
    torch.cuda.synchronize()
    for name, t in zip(("image0", "image1", "flow"), big):
        raw = t.cpu().numpy().view(np.uint8)
        assert (raw[0] == SENTINEL).all(), "%s: the slot in front was written" % name
        assert (raw[B + 1] == SENTINEL).all(), "%s: the slot behind was written" % name
        assert not (raw[1:B + 1] == SENTINEL).all()
    if mode != 9:  # (mode 9: a second render on this context would take other crops)
        check_form(render(ofdg, g, tasks, B, bps, n), [t[1:B + 1].cpu().numpy() for t in big], form)


# ---- 5. fmt = NULL and {F32, F32} are the plain call ----
def test_fmt_entry_points_with_float32_are_the_plain_calls(ofdg):
    import torch
    W, H, B = 128, 96, 2
    L = ofdg.lib()
    vp = C.c_void_p
    g = make_gen(ofdg, W, H, 7)
    tasks, bps, n = g.sample(B)
    plain = render(ofdg, g, tasks, B, bps, n)
    for fmt in (None, C.byref(ofdg.OutFormat(ofdg.FMT_F32, ofdg.FMT_F32))):
        outs = alloc(ofdg, B, H, W)
        g._check(L.ofdg_render_fmt(g.h, C.cast(tasks, vp), B, C.cast(bps, vp), n, *[vp(t.data_ptr()) for t in outs], fmt, vp(0)))
        g.synchronize()
        check_form(plain, host(outs), ("f32", "f32"))
    # forward_counter and forward
    gc = make_gen(ofdg, W, H, 7, sampler=1, seed=5, batch_size=B, background_prep=1)
    ref = alloc(ofdg, B, H, W)
    gc.forward_counter(40, B, *ref)
    gc.synchronize()
    for fmt in (None, C.byref(ofdg.OutFormat(ofdg.FMT_F32, ofdg.FMT_F32))):
        outs = alloc(ofdg, B, H, W)
        gc._check(L.ofdg_forward_counter_fmt(gc.h, 40, B, *[vp(t.data_ptr()) for t in outs], fmt, vp(0)))
        gc.synchronize()
        check_form(host(ref), host(outs), ("f32", "f32"))
    ga = make_gen(ofdg, W, H, 7, sampler=1, seed=5, batch_size=B)
    gb = make_gen(ofdg, W, H, 7, sampler=1, seed=5, batch_size=B)
    for fmt in (None, C.byref(ofdg.OutFormat(ofdg.FMT_F32, ofdg.FMT_F32))):
        a, b = alloc(ofdg, B, H, W), alloc(ofdg, B, H, W)
        ga.forward(*a)
        gb._check(L.ofdg_forward_fmt(gb.h, *[vp(t.data_ptr()) for t in b], fmt, vp(0)))
        ga.synchronize()
        gb.synchronize()
        check_form(host(a), host(b), ("f32", "f32"))
    assert ga.step == gb.step == 2
    torch.cuda.synchronize()


# ---- 6. argument errors ----
BAD = [("image", (7, 0, 0, 0)), ("flow", (0, 9, 0, 0)), ("flow", (0, 1, 0, 0)), ("image", (2, 0, 0, 0)), ("image", (-1, 0, 0, 0)),
       ("reserved", (1, 2, 1, 0)), ("reserved", (1, 2, 0, 5))]


@pytest.mark.parametrize("field,codes", BAD)
def test_invalid_formats_fail_and_enqueue_nothing(ofdg, field, codes):
    import torch
    W, H, B = 128, 96, 2
    L = ofdg.lib()
    vp = C.c_void_p
    fmt = ofdg.OutFormat(codes[0], codes[1])
    fmt.reserved[0], fmt.reserved[1] = codes[2], codes[3]

    g = make_gen(ofdg, W, H, 7)
    tasks, bps, n = g.sample(B)
    outs = alloc(ofdg, B, H, W)  # (float32-sized: large enough for whatever a wrong call might write)
    ticket = g.last_ticket()
    rc = L.ofdg_render_fmt(g.h, C.cast(tasks, vp), B, C.cast(bps, vp), n, *[vp(t.data_ptr()) for t in outs], C.byref(fmt), vp(0))
    assert rc == ofdg.EINVAL
    assert field in L.ofdg_last_error(g.h).decode()
    g.synchronize()
    torch.cuda.synchronize()
    assert all((t.cpu().numpy().view(np.uint8) == SENTINEL).all() for t in outs)
    assert g.last_ticket() == ticket
    fresh = make_gen(ofdg, W, H, 7)
    check_form(render(ofdg, fresh, tasks, B, bps, n), render(ofdg, g, tasks, B, bps, n), ("f32", "f32"))

    # the counter sampler's path (preparation kernels ahead of compose) and forward's step counter
    gc = make_gen(ofdg, W, H, 7, sampler=1, seed=5, batch_size=B, background_prep=1)
    assert L.ofdg_forward_counter_fmt(gc.h, 40, B, *[vp(t.data_ptr()) for t in outs], C.byref(fmt), vp(0)) == ofdg.EINVAL
    assert field in L.ofdg_last_error(gc.h).decode()
    assert L.ofdg_forward_fmt(gc.h, *[vp(t.data_ptr()) for t in outs], C.byref(fmt), vp(0)) == ofdg.EINVAL
    assert gc.step == 0
    gc.synchronize()
    torch.cuda.synchronize()
    assert all((t.cpu().numpy().view(np.uint8) == SENTINEL).all() for t in outs)
    fresh = make_gen(ofdg, W, H, 7, sampler=1, seed=5, batch_size=B, background_prep=1)
    a, b = alloc(ofdg, B, H, W), alloc(ofdg, B, H, W)
    gc.forward_counter(40, B, *a)
    fresh.forward_counter(40, B, *b)
    gc.synchronize()
    fresh.synchronize()
    check_form(host(b), host(a), ("f32", "f32"))


def test_python_rejects_compact_formats_with_extras_and_wrong_dtypes(ofdg):
    import torch
    W, H, B = 128, 96, 2
    g = make_gen(ofdg, W, H, 7)
    tasks, bps, n = g.sample(B)
    outs = alloc(ofdg, B, H, W, ("u8", "f16"))
    with pytest.raises(ValueError):
        g.render(tasks, B, bps, n, *outs, extras=ofdg.alloc_extras(B, H, W, ("flow1",)))
    with pytest.raises(ValueError):  # int8 frames: refused before the library is called
        g.render(tasks, B, bps, n, outs[0].view(torch.int8), outs[1].view(torch.int8), outs[2])
    with pytest.raises(ValueError):  # one sample short
        g.render(tasks, B, bps, n, outs[0][:1], outs[1], outs[2])
    g.synchronize()
    assert all((t.cpu().numpy().view(np.uint8) == SENTINEL).all() for t in outs)


# ---- 7. streams and tickets ----
def test_compact_call_on_a_callers_stream_and_on_its_own(ofdg):
    import torch
    W, H, B = 128, 96, 2
    form = ("u8", "f16")
    g = make_gen(ofdg, W, H, 7)
    tasks, bps, n = g.sample(B)
    ref = render(ofdg, g, tasks, B, bps, n, form)
    check_form(render(ofdg, g, tasks, B, bps, n), ref, form)
    s = torch.cuda.Stream()
    for stream in (s.cuda_stream, ofdg.STREAM_OWN):
        ticket = g.last_ticket()
        got = render(ofdg, g, tasks, B, bps, n, form, stream)
        assert g.last_ticket() == ticket + 1
        g.poll_errors_of(g.last_ticket())  # (raises unless OK)
        assert same_bytes(ref, got)
    # raw pointers: the format is named
    outs = alloc(ofdg, B, H, W, form)
    g.render(tasks, B, bps, n, *ofdg.device_pointers(outs), ofdg.STREAM_OWN, fmt=form)
    g.synchronize()
    assert same_bytes(ref, host(outs))


# ---- 8. the prefetch ring ----
@pytest.mark.parametrize("sampler", [0, 1])
def test_flow_loader_in_the_compact_formats(ofdg, sampler):
    import torch
    W, H, B = 128, 96, 3
    kw = dict(width=W, height=H, mode=7, sampler=sampler, seed=9, batch_size=B, background_prep=sampler)

    def pool(g):
        g.pool_synthetic(3, 2 * W, 2 * H, 11)

    plain = ofdg.FlowLoader(pool=pool, prefetch=3, **kw)
    compact = ofdg.FlowLoader(pool=pool, prefetch=3, image_dtype=torch.uint8, flow_dtype=torch.float16, **kw)
    for k in range(5):
        a, b = next(plain), next(compact)
        assert len(b) == 3
        assert b[0].dtype == b[1].dtype == torch.uint8 and b[2].dtype == torch.float16
        assert tuple(b[0].shape) == tuple(b[1].shape) == (B, 3, H, W) and tuple(b[2].shape) == (B, 2, H, W)
        torch.cuda.current_stream().synchronize()
        check_form(host(a), host(b), ("u8", "f16"), "batch %d" % k)
    with pytest.raises(ValueError):
        ofdg.FlowLoader(pool=pool, prefetch=3, image_dtype=torch.uint8, extras=("flow1",), **kw)
