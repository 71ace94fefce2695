"""GPU tests of the paths that replace, grow, alias and tear down what a context holds (device buffers, pinned staging, events,
streams): the parity tests take a context through each of them once at the most.  Every case works on a 64 x 32 frame with
batches of at most 8 samples and compares bytes with what a FRESH context gives for the same call - no case asserts a memory
figure: the only one a process can read is the device-wide free memory, which other processes move."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 64, 32
ALL = ("flow1", "occ0", "occ1", "label0", "label1")
MIXED = ((160, 120), (40, 24), (200, 96))   # (w, h); the second is smaller than the frame: resized copies, two-kernel preparation


def image(w, h, seed):
    return np.random.RandomState(seed).randint(0, 256, (3, h, w)).astype(np.uint8)


def gen(ofdg, mode=7, **kw):
    return ofdg.Generator(ofdg.default_params(width=W, height=H, mode=mode, **kw))


def host(tensors):
    return [t.cpu().numpy().copy() for t in tensors]


def same(a, b, what):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.dtype == y.dtype and x.shape == y.shape, what
        bad = x.view(np.uint8) != y.view(np.uint8)
        assert not bad.any(), "%s: output %d differs in %d bytes" % (what, k, bad.sum())


def render(ofdg, g, batch, stream=0):
    import torch
    tasks, bps, n_bps = batch
    outs = ofdg.alloc_outputs(len(tasks), H, W)
    g.render(tasks, len(tasks), bps, n_bps, *outs, stream)
    g.synchronize(stream)
    torch.cuda.synchronize()
    return host(outs)


def counter(ofdg, g, first, n):
    import torch
    outs = ofdg.alloc_outputs(n, H, W)
    g.forward_counter(first, n, *outs, ofdg.STREAM_OWN)
    g.synchronize(ofdg.STREAM_OWN)
    torch.cuda.synchronize()
    return host(outs)


def batches(ofdg, mode, sizes):
    s = ofdg.HostSampler(mode, W, H)
    return [s.next(n) for n in sizes]


# ---- the pools of the replacement test: name -> how a context gets it ----
def pool_uniform(g):   # images smaller than the frame: both derived pools are resized copies
    g.pool_alloc(2, 48, 24)
    for i in range(2):
        g.pool_upload(i, image(48, 24, 20 + i))


def pool_synth(g):     # large enough for the foreground, too small for the backgrounds: one resized copy
    g.pool_synthetic(3, 100, 50, 11)


def pool_mixed(g):
    g.pool_alloc_mixed(len(MIXED))
    for i, (w, h) in enumerate(MIXED):
        g.pool_upload_mixed(i, image(w, h, 30 + i))


# ---- 1. the whole surface on four contexts, one after another ----
def whole_surface(ofdg):
    import torch
    B = 4
    g = gen(ofdg, 7, sampler=1, seed=5, batch_size=B, background_prep=1)
    pool_mixed(g)
    g.debug_bgprep_paths()   # (switches the counting on)
    outs = ofdg.alloc_outputs(B, H, W, image_dtype=torch.uint8, flow_dtype=torch.float16)
    ex = ofdg.alloc_extras(B, H, W, ALL, flow_dtype=torch.float16, occ_dtype=torch.uint8)
    g.forward_counter(8, B, *outs, ofdg.STREAM_OWN, extras=ex)
    rows, counts = ofdg.alloc_object_table(B)
    g.object_table(ex["label0"], ex["label1"], rows, counts, ofdg.STREAM_OWN)
    stats = ofdg.alloc_flow_stats(B)
    g.flow_stats(outs[2], stats, occ=ex["occ0"], stream=ofdg.STREAM_OWN)
    ticket = g.last_ticket()
    g.synchronize(ofdg.STREAM_OWN)
    torch.cuda.synchronize()
    g.poll_errors_of(ticket)
    got = host(list(outs) + [ex[k] for k in ALL] + [rows, counts, stats])
    g.set_profiling(2)
    again = ofdg.alloc_outputs(B, H, W, image_dtype=torch.uint8, flow_dtype=torch.float16)
    g.forward_counter(8, B, *again, ofdg.STREAM_OWN)
    g.synchronize(ofdg.STREAM_OWN)
    torch.cuda.synchronize()
    assert g.kernel_ms("compose") > 0
    got += host(again) + [np.asarray(g.debug_bgprep_paths(), np.int64)]
    g.close()
    return got


def test_whole_surface_four_contexts_in_a_row(ofdg):
    first = whole_surface(ofdg)
    assert first[0].any() and first[2].any() and first[6].max() >= 1   # frames, flow, label0: the call rendered something
    same(first[:3], first[11:14], "the profiled call against the first")
    for k in range(1, 4):
        same(first, whole_surface(ofdg), "context %d against context 0" % k)


# ---- 2. replacement on one context ----
def test_pools_replaced_on_one_context(ofdg):
    batch = batches(ofdg, 7, [3])[0]
    fresh = {}
    for fill in (pool_uniform, pool_synth, pool_mixed):
        f = gen(ofdg)
        fill(f)
        fresh[fill] = render(ofdg, f, batch)
        f.close()
    assert any(not np.array_equal(fresh[pool_uniform][0], fresh[p][0]) for p in (pool_synth, pool_mixed))
    g = gen(ofdg)
    for fill in (pool_uniform, pool_synth, pool_mixed, pool_synth):
        fill(g)
        same(render(ofdg, g, batch), fresh[fill], "after %s" % fill.__name__)
    g.close()


def test_warp_crops_replaced_on_one_context(ofdg):
    """Mode 9: forward_counter reads the static crop table of the context, render the crop table of its batch.  A big field
    of side 3 * 64 holds no displacer (they sit on a 200 px grid), so every generated crop of this frame is the identity
    field: a fourth set, uploaded, bends the pixels, and its output must differ from the generated sets'."""
    seed = 3
    batch = batches(ofdg, 9, [8])[0]
    yy, xx = np.mgrid[0:H + 1, 0:W + 1].astype(np.float32)
    bent = np.stack([np.stack([a * np.sin(yy / 5 + k), a * np.cos(xx / 7 + k), -a * np.sin(yy / 5 + k), -a * np.cos(xx / 7 + k)])
                     for k, a in enumerate(np.float32([1.5, 1.0, 0.75, 1.25, 0.5]))])

    def both(g):
        return counter(ofdg, g, 4, 8) + render(ofdg, g, batch)

    def context():
        g = gen(ofdg, 9, sampler=1, seed=5)
        g.pool_synthetic(2, 2 * W, 2 * H, 11)
        return g

    g = context()
    g.warp_generate(1, seed)
    got_a = both(g)
    crops_a = np.stack([g.warp_download(i) for i in range(g.warp_count())])
    g.warp_generate(1, seed + 1)
    got_b = both(g)
    g.warp_upload(crops_a)
    got_c = both(g)
    g.warp_upload(bent)
    got_d = both(g)
    g.warp_generate(1, seed)
    got_e = both(g)
    g.close()
    for call in (slice(0, 3), slice(3, 6)):   # both calls read the crops: what they write changes with the set
        assert any(not np.array_equal(x, y) for x, y in zip(got_a[call], got_d[call])), "the uploaded crops must bend something"
    same(got_e, got_a, "the first set again, after the bent one")
    for got, install in ((got_a, lambda f: f.warp_generate(1, seed)), (got_b, lambda f: f.warp_generate(1, seed + 1)),
                         (got_c, lambda f: f.warp_upload(crops_a)), (got_d, lambda f: f.warp_upload(bent))):
        f = context()
        install(f)
        same(got, both(f), "against a fresh context")
        f.close()


# ---- 3. grow, shrink, alias ----
def test_grow_shrink_alias_on_one_context(ofdg):
    """chains = 1: every call works on the same chain, so its private slot sees batch after batch."""
    sizes = (1, 8, 1)
    bs = batches(ofdg, 7, sizes)

    def context(**kw):
        g = gen(ofdg, **kw)
        g.pool_synthetic(3, 2 * W, 2 * H, 11)
        return g

    want_render, want_counter = [], {}
    for b in bs:
        f = context()
        want_render.append(render(ofdg, f, b))
        f.close()
    for n in set(sizes):
        f = context()
        want_counter[n] = counter(ofdg, f, 16, n)
        f.close()
    g = context(chains=1)
    assert g.num_chains() == 1
    for b, want in zip(bs, want_render):        # one arena, looked into (alias)
        same(render(ofdg, g, b), want, "render of %d" % len(b[0]))
    for n in sizes:                             # the same slot's buffers, now owned (reserve on what was a view)
        same(counter(ofdg, g, 16, n), want_counter[n], "forward_counter of %d" % n)
    same(render(ofdg, g, bs[1]), want_render[1], "render of 8 after forward_counter")   # ... and views again
    import torch
    for slot in (0, 3):                         # a caller's slots, each uploaded again with a larger batch
        for b, want in ((bs[0], want_render[0]), (bs[1], want_render[1])):
            tasks, bps, n_bps = b
            outs = ofdg.alloc_outputs(len(tasks), H, W)
            g.upload_slot(slot, tasks, len(tasks), bps, n_bps)
            g.render_slot(slot, *outs)
            g.synchronize()
            torch.cuda.synchronize()
            same(host(outs), want, "slot %d, batch of %d" % (slot, len(tasks)))
    g.close()


# ---- 4. two contexts alive at once ----
@pytest.mark.parametrize("reverse", (False, True), ids=("closed in creation order", "closed in reverse order"))
def test_two_contexts_alive_at_once(ofdg, reverse):
    b7, b5 = batches(ofdg, 7, [2, 3]), batches(ofdg, 5, [3, 2])

    def ctx7():
        g = gen(ofdg, 7)
        g.pool_synthetic(3, 2 * W, 2 * H, 11)
        return g

    def ctx5():
        g = gen(ofdg, 5, background_prep=1)
        g.pool_synthetic(2, 3 * W, 3 * H, 12)
        return g

    solo = []
    for make, bs in ((ctx7, b7), (ctx5, b5)):
        f = make()
        solo.append([render(ofdg, f, b) for b in bs] + [counter(ofdg, f, 0, 2)])
        f.close()
    a, b = ctx7(), ctx5()
    got = ([], [])
    for k in range(2):
        got[0].append(render(ofdg, a, b7[k]))
        got[1].append(render(ofdg, b, b5[k]))
    got[1].append(counter(ofdg, b, 0, 2))
    got[0].append(counter(ofdg, a, 0, 2))
    for g in ((b, a) if reverse else (a, b)):
        g.close()
    for k in range(2):
        for j in range(3):
            same(got[k][j], solo[k][j], "context %d, call %d" % (k, j))
    third = ctx7()
    same(render(ofdg, third, b7[0]), solo[0][0], "a third context afterwards")
    third.close()


# ---- 5. refused creation ----
# (what is wrong, the parameters, the code and the text the build of the parent commit gives for them)
def _refusals(ofdg, ndev):
    return [("mode 14", dict(mode=14), ofdg.EBADMODE, "BAD MODE"),
            ("width 12", dict(width=12), ofdg.EINVAL, "width must be a multiple of 8 and height even"),
            ("num_objects 99", dict(num_objects=99), ofdg.EINVAL, "num_objects must be 0 (reference: 16..23) or 1..64 for this sampler"),
            ("device = the device count", dict(device=ndev), ofdg.EHIP, "hipSetDevice: invalid device ordinal")]


def test_refused_creation_leaves_the_next_context_working(ofdg):
    import torch
    L = ofdg.lib()
    batch = batches(ofdg, 7, [2])[0]
    want = None
    for what, kw, code, text in _refusals(ofdg, torch.cuda.device_count()):
        p = ofdg.default_params(**dict(dict(width=W, height=H, mode=7), **kw))
        h = C.c_void_p()
        rc = L.ofdg_create(C.byref(p), C.byref(h))
        print("%s: %d %r" % (what, rc, L.ofdg_last_error(None).decode()))
        assert rc == code and not h.value, what
        assert L.ofdg_last_error(None).decode() == text, what
        # (a refused hipSetDevice stays the HIP runtime's "last error" of this thread until somebody reads it - the next
        #  hipGetLastError() after a launch would report it as its own: read it, as a caller that handles the refusal does)
        L.hipGetLastError()
        g = gen(ofdg)
        g.pool_synthetic(3, 2 * W, 2 * H, 11)
        got = render(ofdg, g, batch)
        g.close()
        assert got[0].any()
        if want is None:
            want = got
        same(got, want, "the context created after '%s'" % what)
