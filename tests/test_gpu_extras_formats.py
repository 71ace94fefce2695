"""GPU tests of the optional outputs in the compact formats (ofdg_render_ex_fmt / ofdg_forward_ex_fmt /
ofdg_forward_counter_ex_fmt).  The definition (include/ofdg.h) makes the float32 ofdg_*_ex call the reference - itself pinned
to tests/extras_reference.py and through it to the oracle by tests/test_gpu_extras.py - and every comparison exact: a uint8
frame byte widened to float32 is what the float call stores, an fp16 flow / flow1 value is the float call's value converted
once (numpy's astype(float16): round to nearest even), labels are the same bytes, a uint8 occlusion map is 1 where the
float32 map is 1.0f and 0 elsewhere - rounded from the float32 flow, whatever the flow is stored as."""
import ctypes as C
import itertools

import numpy as np
import pytest

import extras_reference as xr
from test_extras_formats import occlusion_from_fp16_flows
from test_gpu_extras import ALL, make_gen

pytestmark = pytest.mark.gpu

FORMS = tuple(itertools.product(("f32", "u8"), ("f32", "f16"), ("f32", "u8")))  # (frames, flow and flow1, occlusion maps)
COMPACT = ("u8", "f16", "u8")
SENTINEL = 0xA5
CASES = [(W, H, m, 1) for (W, H) in ((128, 96), (160, 100)) for m in (1, 2, 3, 5, 7, 13)] + [(512, 384, 7, 1), (512, 384, 7, 0)]


def dtypes(form):
    import torch
    return ({"u8": torch.uint8, "f32": torch.float32}[form[0]], {"f16": torch.float16, "f32": torch.float32}[form[1]],
            {"u8": torch.uint8, "f32": torch.float32}[form[2]])


def alloc(ofdg, n, H, W, form, names=ALL):
    """Outputs and extras in `form`, every byte set to the sentinel."""
    import torch
    idt, fdt, odt = dtypes(form)
    outs = ofdg.alloc_outputs(n, H, W, image_dtype=idt, flow_dtype=fdt)
    ex = ofdg.alloc_extras(n, H, W, names, flow_dtype=fdt, occ_dtype=odt) if names is not None else None
    for t in list(outs) + list((ex or {}).values()):
        t.view(torch.uint8).fill_(SENTINEL)
    return outs, ex


def host(outs, ex):
    return [t.cpu().numpy() for t in outs], {k: t.cpu().numpy() for k, t in (ex or {}).items()}


def bits(a):
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def render(ofdg, g, tasks, n, bps, n_bps, form, names=ALL, stream=0):
    import torch
    outs, ex = alloc(ofdg, n, g.params.height, g.params.width, form, names)
    g.render(tasks, n, bps, n_bps, *outs, stream, extras=ex)
    g.synchronize(0 if stream == ofdg.STREAM_OWN else stream)
    torch.cuda.synchronize()
    return host(outs, ex)


def check_form(ref, got, form, what=""):
    """ref, got: ([image0, image1, flow], {extras}) of the float32 call and of the call in `form`; every check bit for bit."""
    (r_outs, r_ex), (g_outs, g_ex) = ref, got
    assert set(g_ex) <= set(r_ex)
    for k in (0, 1):
        assert g_outs[k].dtype == (np.uint8 if form[0] == "u8" else np.float32)
        bad = bits(g_outs[k].astype(np.float32)) != bits(r_outs[k])
        assert not bad.any(), "%s image%d (%s): %d values differ" % (what, k, form[0], bad.sum())
    flows = [("flow", r_outs[2], g_outs[2])] + ([("flow1", r_ex["flow1"], g_ex["flow1"])] if "flow1" in g_ex else [])
    for name, r, g_ in flows:
        assert np.isfinite(r).all()
        assert g_.dtype == (np.float16 if form[1] == "f16" else np.float32)
        bad = bits(g_) != bits(r.astype(g_.dtype))
        assert not bad.any(), "%s %s (%s): %d values are not the float32 values (rounded once to nearest even)" % (what, name, form[1], bad.sum())
    for name in ("label0", "label1"):
        if name in g_ex:
            bad = g_ex[name] != r_ex[name]
            assert g_ex[name].dtype == np.uint8 and not bad.any(), "%s %s: %d labels differ" % (what, name, bad.sum())
    for name in ("occ0", "occ1"):
        if name in g_ex:
            o = g_ex[name]
            assert o.shape == r_ex[name].shape
            if form[2] == "u8":
                assert o.dtype == np.uint8 and (o <= 1).all(), "%s %s: a byte that is neither 0 nor 1" % (what, name)
                bad = o != (r_ex[name] != 0)
            else:
                assert o.dtype == np.float32
                bad = bits(o) != bits(r_ex[name])
            assert not bad.any(), "%s %s (%s): %d flags differ" % (what, name, form[2], bad.sum())


# ---- 1. host sampler: every form against the float32 _ex call, on contexts made alike ----
@pytest.mark.parametrize("W,H,mode,aa", CASES)
def test_every_form_matches_the_float_call_host_sampler(ofdg, W, H, mode, aa):
    B = 1 if W == 512 else 2
    g_ref, g = make_gen(ofdg, W, H, mode, use_antialiasing=aa), make_gen(ofdg, W, H, mode, use_antialiasing=aa)
    tasks, bps, n = g_ref.sample(B)
    ref = render(ofdg, g_ref, tasks, B, bps, n, ("f32", "f32", "f32"))
    assert np.abs(ref[0][2]).max() > 0 and ref[1]["occ0"].max() == 1 and ref[1]["label0"].max() >= 1
    for form in FORMS:
        check_form(ref, render(ofdg, g, tasks, B, bps, n, form), form, "mode %d %dx%d %s" % (mode, W, H, "/".join(form)))


# ---- 2. against the definitions themselves, and: the occlusion is rounded from the float32 flow ----
def test_compact_occlusion_is_the_definition_not_the_fp16_flows_rounding(ofdg, oracle):
    """Mode 7 at 512x384, uint8 frames, fp16 flows, uint8 maps: labels and occlusion against extras_reference directly.  The
    maps an occlusion pass would get from the STORED fp16 flows are different ones (asserted: at least one pixel per frame),
    so the equality tells the two apart."""
    W, H = 512, 384
    g = make_gen(ofdg, W, H, 7)
    tasks, bps, n = g.sample(1)
    ref = xr.reference_extras(ofdg, oracle, oracle.default_params(W, H, 7), tasks, 1, bps, n, g.pool_download_all())
    (_, _, fl), ex = render(ofdg, g, tasks, 1, bps, n, COMPACT)
    for k in ("label0", "label1"):
        assert np.array_equal(ex[k], ref[k]), "%s differs at %d px" % (k, (ex[k] != ref[k]).sum())
    assert np.array_equal(bits(fl), bits(ref["flow"].astype(np.float16)))
    assert np.array_equal(bits(ex["flow1"]), bits(ref["flow1"].astype(np.float16)))
    wrong = occlusion_from_fp16_flows(ref)
    for k, w in zip(("occ0", "occ1"), wrong):
        n_wrong = int((w != ref[k][0]).sum())
        print("%s: rounding the fp16 flows instead changes %d px" % (k, n_wrong))
        assert n_wrong >= 1
        assert ex[k].dtype == np.uint8 and (ex[k] <= 1).all()
        assert np.array_equal(ex[k], ref[k] != 0), "%s differs from the definition at %d px" % (k, (ex[k] != (ref[k] != 0)).sum())
        assert not np.array_equal(ex[k][0], w != 0)
        # ... and from the device's own stored flows the rule does not follow either
    own = xr.occlusion(fl[0].astype(np.float32), ex["label0"][0], ex["label1"][0])
    assert not np.array_equal(own != 0, ex["occ0"][0])


# ---- 3. counter sampler at config 2's shape, every sample ----
def test_forward_counter_compact_extras_against_float_config2(ofdg):
    import torch
    W, H, B, first = 512, 384, 32, 640
    g = ofdg.Generator(ofdg.default_params(width=W, height=H, mode=5, sampler=1, seed=20261003, batch_size=B, num_objects=16,
                                           background_prep=1))
    g.pool_synthetic(8, 1024, 768, 2024)
    outs, ex = alloc(ofdg, B, H, W, ("f32", "f32", "f32"))
    g.forward_counter(first, B, *outs, extras=ex)
    g.synchronize()
    ref = host(outs, ex)
    del outs, ex
    assert 0.0 < ref[1]["occ0"].mean() < 0.5
    for form in (COMPACT, ("u8", "f32", "u8"), ("f32", "f16", "f32")):
        outs, ex = alloc(ofdg, B, H, W, form)
        g.forward_counter(first, B, *outs, extras=ex)
        g.synchronize()
        torch.cuda.synchronize()
        got = host(outs, ex)
        del outs, ex
        for s in range(B):  # every sample
            check_form(([a[s] for a in ref[0]], {k: v[s] for k, v in ref[1].items()}),
                       ([a[s] for a in got[0]], {k: v[s] for k, v in got[1].items()}), form, "sample %d %s" % (s, "/".join(form)))


# ---- 4. every subset of the five pointers; nothing else is written ----
@pytest.mark.parametrize("W,H,form", [(128, 96, COMPACT), (160, 100, ("u8", "f16", "f32")), (128, 96, ("f32", "f32", "u8"))])
def test_every_subset_of_the_extras_and_the_guard_slots(ofdg, W, H, form):
    import torch
    B = 2
    g_ref, g = make_gen(ofdg, W, H, 5), make_gen(ofdg, W, H, 5)
    tasks, bps, n = g_ref.sample(B)
    ref = render(ofdg, g_ref, tasks, B, bps, n, ("f32", "f32", "f32"))
    full = render(ofdg, g, tasks, B, bps, n, form)
    check_form(ref, full, form)
    for r in range(0, 6):
        for names in itertools.combinations(ALL, r):  # (occ0 / occ1 without labels: the chain's workspace)
            outs, ex = alloc(ofdg, B + 2, H, W, form, names)  # one guard sample slot in front, one behind
            g.render(tasks, B, bps, n, *[t[1:B + 1] for t in outs], extras={k: t[1:B + 1] for k, t in ex.items()})
            g.synchronize()
            torch.cuda.synchronize()
            for name, t in list(zip(("image0", "image1", "flow"), outs)) + list(ex.items()):
                raw = t.cpu().numpy()
                assert (bits(raw[0]).view(np.uint8) == SENTINEL).all(), "%s of %s: the slot in front was written" % (name, names)
                assert (bits(raw[B + 1]).view(np.uint8) == SENTINEL).all(), "%s of %s: the slot behind was written" % (name, names)
            got = host([t[1:B + 1] for t in outs], {k: t[1:B + 1] for k, t in ex.items()})
            assert set(got[1]) == set(names)
            for a, b in zip(full[0], got[0]):
                assert a.dtype == b.dtype and np.array_equal(bits(a), bits(b)), names
            for k in names:
                assert got[1][k].dtype == full[1][k].dtype and np.array_equal(bits(got[1][k]), bits(full[1][k])), (k, names)


# ---- 5. streams and tickets ----
def test_compact_extras_on_a_callers_stream_and_on_its_own(ofdg):
    import torch
    W, H, B = 128, 96, 2
    g = make_gen(ofdg, W, H, 7)
    tasks, bps, n = g.sample(B)
    ref = render(ofdg, g, tasks, B, bps, n, ("f32", "f32", "f32"))
    first = render(ofdg, g, tasks, B, bps, n, COMPACT)
    check_form(ref, first, COMPACT)
    s = torch.cuda.Stream()
    for stream in (s.cuda_stream, ofdg.STREAM_OWN, s.cuda_stream, ofdg.STREAM_OWN):
        for names in (ALL, ("occ1",)):
            ticket = g.last_ticket()
            got = render(ofdg, g, tasks, B, bps, n, COMPACT, names, stream)
            assert g.last_ticket() == ticket + 1
            g.poll_errors_of(g.last_ticket())  # (raises unless OK)
            for a, b in zip(first[0], got[0]):
                assert np.array_equal(bits(a), bits(b))
            for k in names:
                assert np.array_equal(bits(first[1][k]), bits(got[1][k])), k
    # raw pointers for the outputs: the format is named
    outs, ex = alloc(ofdg, B, H, W, COMPACT)
    g.render(tasks, B, bps, n, *ofdg.device_pointers(outs), ofdg.STREAM_OWN, extras=ex, fmt=("u8", "f16"))
    g.synchronize()
    got = host(outs, ex)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(first[0], got[0]))
    assert all(np.array_equal(bits(first[1][k]), bits(got[1][k])) for k in ALL)


# ---- 6. the degenerate forms are the calls they stand for ----
def test_degenerate_forms_write_the_bytes_of_ex_and_of_fmt(ofdg):
    import torch
    W, H, B = 128, 96, 2
    L, vp = ofdg.lib(), C.c_void_p
    g = make_gen(ofdg, W, H, 7)
    tasks, bps, n = g.sample(B)
    t_, b_ = C.cast(tasks, vp), C.cast(bps, vp)

    def xfmt(ex, occ=ofdg.FMT_F32):
        x = ofdg.ExtrasFmt(occ=occ)
        for k, t in ex.items():
            setattr(x, k, t.data_ptr())
        return x

    # {F32, F32} / NULL with occ F32: ofdg_render_ex
    ref = render(ofdg, g, tasks, B, bps, n, ("f32", "f32", "f32"))
    for fmt in (None, C.byref(ofdg.OutFormat(ofdg.FMT_F32, ofdg.FMT_F32))):
        outs, ex = alloc(ofdg, B, H, W, ("f32", "f32", "f32"))
        g._check(L.ofdg_render_ex_fmt(g.h, t_, B, b_, n, *[vp(t.data_ptr()) for t in outs], C.byref(xfmt(ex)), fmt, vp(0)))
        g.synchronize()
        got = host(outs, ex)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(ref[0], got[0]))
        assert all(np.array_equal(bits(ref[1][k]), bits(got[1][k])) for k in ALL)
    # ex == NULL / all pointers NULL: ofdg_render_fmt
    outs, _ = alloc(ofdg, B, H, W, COMPACT, None)
    g.render(tasks, B, bps, n, *outs)
    g.synchronize()
    want, _ = host(outs, None)
    for ex in (None, C.byref(ofdg.ExtrasFmt()), C.byref(ofdg.ExtrasFmt(occ=ofdg.FMT_U8))):
        outs, _ = alloc(ofdg, B, H, W, COMPACT, None)
        g._check(L.ofdg_render_ex_fmt(g.h, t_, B, b_, n, *[vp(t.data_ptr()) for t in outs], ex,
                                      C.byref(ofdg.OutFormat(ofdg.FMT_U8, ofdg.FMT_F16)), vp(0)))
        g.synchronize()
        got, _ = host(outs, None)
        assert all(a.dtype == b.dtype and np.array_equal(bits(a), bits(b)) for a, b in zip(want, got))
    # forward_counter and forward (the step counter moves as with the float call)
    kw = dict(sampler=1, seed=5, batch_size=B, background_prep=1)
    ga, gb = make_gen(ofdg, W, H, 7, **kw), make_gen(ofdg, W, H, 7, **kw)
    for k in range(2):
        a, ax = alloc(ofdg, B, H, W, ("f32", "f32", "f32"))
        b, bx = alloc(ofdg, B, H, W, ("f32", "f32", "f32"))
        if k == 0:
            ga.forward_counter(40, B, *a, extras=ax)
            gb._check(L.ofdg_forward_counter_ex_fmt(gb.h, 40, B, *[vp(t.data_ptr()) for t in b], C.byref(xfmt(bx)), None, vp(0)))
        else:
            ga.forward(*a, extras=ax)
            gb._check(L.ofdg_forward_ex_fmt(gb.h, *[vp(t.data_ptr()) for t in b], C.byref(xfmt(bx)), None, vp(0)))
        ga.synchronize()
        gb.synchronize()
        ra, rb = host(a, ax), host(b, bx)
        assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(ra[0], rb[0]))
        assert all(np.array_equal(bits(ra[1][k_]), bits(rb[1][k_])) for k_ in ALL)
    assert ga.step == gb.step == 1
    # forward / forward_counter in the compact form against the float call
    a, ax = alloc(ofdg, B, H, W, ("f32", "f32", "f32"))
    b, bx = alloc(ofdg, B, H, W, COMPACT)
    ga.forward(*a, extras=ax)
    gb.forward(*b, extras=bx)
    ga.synchronize()
    gb.synchronize()
    torch.cuda.synchronize()
    check_form(host(a, ax), host(b, bx), COMPACT, "forward")
    assert ga.step == gb.step == 2


# ---- 7. refusals: nothing is enqueued, the field is named ----
@pytest.mark.parametrize("field,occ,reserved,fmt", [("occ", 2, (0, 0, 0), (1, 2)), ("occ", -1, (0, 0, 0), (1, 2)), ("occ", 7, (0, 0, 0), (0, 0)),
                                                    ("reserved", 1, (1, 0, 0), (1, 2)), ("reserved", 0, (0, 0, 9), (0, 0)),
                                                    ("image", 1, (0, 0, 0), (5, 2)), ("flow", 1, (0, 0, 0), (1, 1))])
def test_invalid_arguments_fail_and_enqueue_nothing(ofdg, field, occ, reserved, fmt):
    import torch
    W, H, B = 128, 96, 2
    L, vp = ofdg.lib(), C.c_void_p
    g = make_gen(ofdg, W, H, 7)
    tasks, bps, n = g.sample(B)
    outs, ex = alloc(ofdg, B, H, W, ("f32", "f32", "f32"))  # (float32-sized: large enough for whatever a wrong call might write)
    x = ofdg.ExtrasFmt(occ=occ)
    for k, t in ex.items():
        setattr(x, k, t.data_ptr())
    for k in range(3):
        x.reserved[k] = reserved[k]
    of = ofdg.OutFormat(*fmt)
    ticket = g.last_ticket()
    ptrs = [vp(t.data_ptr()) for t in outs]
    assert L.ofdg_render_ex_fmt(g.h, C.cast(tasks, vp), B, C.cast(bps, vp), n, *ptrs, C.byref(x), C.byref(of), vp(0)) == ofdg.EINVAL
    assert field in L.ofdg_last_error(g.h).decode()
    gc = make_gen(ofdg, W, H, 7, sampler=1, seed=5, batch_size=B, background_prep=1)
    assert L.ofdg_forward_counter_ex_fmt(gc.h, 40, B, *ptrs, C.byref(x), C.byref(of), vp(0)) == ofdg.EINVAL
    assert field in L.ofdg_last_error(gc.h).decode()
    assert L.ofdg_forward_ex_fmt(gc.h, *ptrs, C.byref(x), C.byref(of), vp(0)) == ofdg.EINVAL
    assert field in L.ofdg_last_error(gc.h).decode()
    assert gc.step == 0
    g.synchronize()
    gc.synchronize()
    torch.cuda.synchronize()
    assert all((bits(t.cpu().numpy()).view(np.uint8) == SENTINEL).all() for t in list(outs) + list(ex.values()))
    assert g.last_ticket() == ticket
    # a following plain call renders what a fresh context renders
    fresh = make_gen(ofdg, W, H, 7)
    a, b = render(ofdg, fresh, tasks, B, bps, n, ("f32", "f32", "f32"), None), render(ofdg, g, tasks, B, bps, n, ("f32", "f32", "f32"), None)
    assert all(np.array_equal(bits(p), bits(q)) for p, q in zip(a[0], b[0]))
    fresh = make_gen(ofdg, W, H, 7, sampler=1, seed=5, batch_size=B, background_prep=1)
    pa, pb = ofdg.alloc_outputs(B, H, W), ofdg.alloc_outputs(B, H, W)
    gc.forward_counter(40, B, *pa)
    fresh.forward_counter(40, B, *pb)
    gc.synchronize()
    fresh.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(pa, pb))


def test_mode9_compact_extras_are_refused_and_nothing_is_enqueued(ofdg):
    import torch
    W, H, B = 128, 96, 2
    g = make_gen(ofdg, W, H, 9, sampler=1, seed=3, batch_size=B)
    g.warp_generate(1, 3)
    outs, ex = alloc(ofdg, B, H, W, COMPACT, ("label0",))
    before = g.last_ticket()
    for call in (lambda: g.forward_counter(0, B, *outs, extras=ex), lambda: g.forward(*outs, extras=ex)):
        with pytest.raises(ofdg.OfdgError) as e:
            call()
        assert e.value.code == ofdg.EINVAL and "rigid" in str(e.value)
    tasks, bps, n = g.sample_counter(0, B)
    with pytest.raises(ofdg.OfdgError) as e:
        g.render(tasks, B, bps, n, *outs, extras=ex)
    assert e.value.code == ofdg.EINVAL and "rigid" in str(e.value)
    g.synchronize()
    torch.cuda.synchronize()
    assert g.last_ticket() == before and g.step == 0
    assert all((bits(t.cpu().numpy()).view(np.uint8) == SENTINEL).all() for t in list(outs) + list(ex.values()))
    # no pointer set: the compact mode-9 call, as ofdg_forward_counter_fmt renders it
    g.forward_counter(0, B, *outs, extras={})
    want, _ = alloc(ofdg, B, H, W, COMPACT, None)
    g2 = make_gen(ofdg, W, H, 9, sampler=1, seed=3, batch_size=B)
    g2.warp_generate(1, 3)
    g2.forward_counter(0, B, *want)
    g.synchronize()
    g2.synchronize()
    assert g.last_ticket() != before
    assert all(torch.equal(a, b) for a, b in zip(outs, want))


# ---- 8. the prefetch ring ----
def test_flowloader_with_compact_extras_hands_out_the_direct_batches(ofdg):
    import torch
    W, H, B = 128, 96, 2
    names = ("flow1", "occ0", "occ1", "label1")
    kw = dict(width=W, height=H, mode=7, batch_size=B, sampler=1, seed=21)
    loader = ofdg.FlowLoader(ofdg.default_params(**kw), pool=lambda g: g.pool_synthetic(3, 2 * W, 2 * H, 11), prefetch=3,
                             extras=names, extras_compact=True, image_dtype=torch.uint8, flow_dtype=torch.float16)
    g = make_gen(ofdg, W, H, 7, batch_size=B, sampler=1, seed=21)
    gf = make_gen(ofdg, W, H, 7, batch_size=B, sampler=1, seed=21)
    it = iter(loader)
    for k in range(4):
        i0, i1, fl, ex = next(it)
        torch.cuda.current_stream().synchronize()
        assert i0.dtype == i1.dtype == torch.uint8 and fl.dtype == ex["flow1"].dtype == torch.float16
        assert ex["occ0"].dtype == ex["occ1"].dtype == ex["label1"].dtype == torch.uint8 and set(ex) == set(names)
        got = [i0.clone(), i1.clone(), fl.clone()] + [ex[n_].clone() for n_ in names]
        outs, dx = alloc(ofdg, B, H, W, COMPACT, names)
        g.forward(*outs, extras=dx)
        g.synchronize()
        for a, b in zip(got, list(outs) + [dx[n_] for n_ in names]):
            assert a.dtype == b.dtype and torch.equal(a, b)
        fo, fx = alloc(ofdg, B, H, W, ("f32", "f32", "f32"), names)  # ... and those are the float32 batches
        gf.forward(*fo, extras=fx)
        gf.synchronize()
        check_form(host(fo, fx), host(outs, dx), COMPACT, "batch %d" % k)
    # without the switch the extras stay float32
    plain = ofdg.FlowLoader(ofdg.default_params(**kw), pool=lambda g: g.pool_synthetic(3, 2 * W, 2 * H, 11), prefetch=2, extras=("occ0",))
    assert next(iter(plain))[3]["occ0"].dtype == torch.float32
