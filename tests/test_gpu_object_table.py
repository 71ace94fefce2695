"""GPU tests of the per-object annotation table (ofdg_object_table, include/ofdg.h): ids, types, counts and motions
against the blueprints and ofdg.host_realize, areas and boxes against plain numpy on the label planes of the numpy
restatement (extras_reference.labels_of, pinned to the oracle by tests/test_extras_reference.py), and the guarantees
around the call: truncation, optional planes, streams and slot reuse, refusals, the loader."""
import ctypes as C

import numpy as np
import pytest

import extras_reference as xr
import object_table_reference as otr

pytestmark = pytest.mark.gpu

LABELS = ("label0", "label1")
FILL = 0xA5


def make_gen(ofdg, W, H, mode, **kw):
    g = ofdg.Generator(ofdg.default_params(width=W, height=H, mode=mode, **kw))
    g.pool_synthetic(3, 2 * W, 2 * H, 11)
    return g


def host_pool(W, H):
    """(the definitions read no texel: any pool of the generator's shape does)"""
    return np.random.default_rng(0).integers(0, 256, (3, 3, 2 * H, 2 * W), dtype=np.uint8)


def expected(ofdg, oracle, W, H, mode, tasks, B, bps, n_bps):
    """Per sample: the reference label planes, and ids / types / motions in table order (background, then painter's order)."""
    pool = host_pool(W, H)
    q = oracle.default_params(W, H, mode)
    prm = ofdg.default_params(width=W, height=H, mode=mode)
    _, om = ofdg.host_realize(prm, 3, 2 * W, 2 * H, tasks, B, bps, n_bps, cap=max(4096, B * 200))
    out, base = [], 0
    for t in range(B):
        l0, l1, order = xr.labels_of(oracle, q, tasks[t], bps, pool)
        assert len(order) == tasks[t].n_objects
        out.append(dict(l0=l0, l1=l1, ids=[bps[tasks[t].background].obj_id] + [bps[bi].obj_id for bi in order],
                        types=[0] + [bps[bi].obj_type for bi in order], motions=om[base:base + 1 + len(order), 0].copy()))
        base += 1 + len(order)
    assert base == len(om)
    return out


def check_sample(ofdg, rows, count, e, H, W, frames=(True, True), motion_bits=True):
    """One sample's rows (cut to what the table reports) against its expectation `e`."""
    n = len(e["ids"])
    assert count == n, (count, n)
    k = len(rows)
    assert list(rows["obj_id"]) == e["ids"][:k] and rows["obj_id"][0] == ofdg.BACKGROUND_ID
    assert list(rows["obj_type"]) == e["types"][:k]
    if motion_bits:
        assert np.array_equal(rows["motion"].view(np.int64), np.ascontiguousarray(e["motions"][:k]).view(np.int64))
    otr.expect_geometry(rows, e["l0"] if frames[0] else None, e["l1"] if frames[1] else None, (H, W))


def render_and_tabulate(ofdg, g, tasks, B, bps, n_bps, per=None, frames=(True, True), compact=False):
    """render(..., extras=labels) then object_table on the same stream; returns (raw rows uint8 [B, per, 96], counts, labels)."""
    import torch
    W, H = g.params.width, g.params.height
    per = ofdg.MAX_OBJECT_ROWS if per is None else per
    if compact:
        outs = ofdg.alloc_outputs(B, H, W, image_dtype=torch.uint8, flow_dtype=torch.float16)
        ex = ofdg.alloc_extras(B, H, W, flow_dtype=torch.float16, occ_dtype=torch.uint8)
    else:
        outs = ofdg.alloc_outputs(B, H, W)
        ex = ofdg.alloc_extras(B, H, W, LABELS)
    rows, counts = ofdg.alloc_object_table(B, per)
    rows.fill_(FILL)
    counts.fill_(-7)
    g.render(tasks, B, bps, n_bps, *outs, extras=ex)
    g.object_table(ex["label0"] if frames[0] else None, ex["label1"] if frames[1] else None, rows, counts)
    g.synchronize()
    torch.cuda.synchronize()
    return rows.cpu().numpy(), counts.cpu().numpy(), {k: ex[k].cpu().numpy() for k in LABELS}


def check_batch(ofdg, raw, counts, exp, H, W, **kw):
    tabs = ofdg.object_table_numpy(raw, counts)
    for s, e in enumerate(exp):
        check_sample(ofdg, tabs[s], int(counts[s]), e, H, W, **kw)
        assert not raw[s, min(int(counts[s]), raw.shape[1]):].any(), "rows beyond the count must be zero bytes"


@pytest.mark.parametrize("W,H,mode", [(W, H, m) for (W, H) in ((128, 96), (160, 100)) for m in (1, 2, 3, 5, 7, 13)])
def test_table_matches_the_definition_host_sampler(ofdg, oracle, W, H, mode):
    B = 3
    g = make_gen(ofdg, W, H, mode)
    tasks, bps, n = g.sample(B)
    raw, counts, labels = render_and_tabulate(ofdg, g, tasks, B, bps, n)
    exp = expected(ofdg, oracle, W, H, mode, tasks, B, bps, n)
    assert list(counts) == [1 + tasks[t].n_objects for t in range(B)]
    check_batch(ofdg, raw, counts, exp, H, W)
    for s in range(B):  # (the planes the table was reduced from are the reference's)
        assert np.array_equal(labels["label0"][s], exp[s]["l0"]) and np.array_equal(labels["label1"][s], exp[s]["l1"])


def test_table_matches_the_definition_full_size(ofdg, oracle):
    W, H, B = 512, 384, 2
    g = make_gen(ofdg, W, H, 7)
    tasks, bps, n = g.sample(B)
    raw, counts, _ = render_and_tabulate(ofdg, g, tasks, B, bps, n)
    check_batch(ofdg, raw, counts, expected(ofdg, oracle, W, H, 7, tasks, B, bps, n), H, W)


def detmath_motions(oracle, W, H, bg, objs):
    """m_motion of a background and its foreground blueprints as the device counter-sampler path builds them (sampler_counter.hip:
    setMotion / addBackgroundMotion, DG:312-335, in fp64 without contraction, sin / cos from include/ofdg_detmath.h)."""
    def rot(a):
        s, c = oracle.det_sincos(np.array([float(a)], np.float64))
        return (float(c[0]), float(s[0]), -float(s[0]), float(c[0]), 0.0, 0.0)

    def scale(s):
        return (float(s), 0.0, 0.0, float(s), 0.0, 0.0)

    def trans(x, y):
        return (1.0, 0.0, 0.0, 1.0, float(x), float(y))

    bgm = xr.mat_mul(xr.mat_mul(rot(bg.rot), scale(bg.scale)), trans(bg.trans_x, bg.trans_y))
    around = xr.mat_mul(xr.mat_mul(trans(-W / 2., -H / 2.), bgm), trans(W / 2., H / 2.))
    out = [bgm]
    for o in objs:
        out.append(xr.mat_mul(xr.mat_mul(xr.mat_mul(rot(o.rot), scale(o.scale)), trans(o.trans_x, o.trans_y)), around))
    return np.array(out, np.float64)


def test_table_counter_sampler(ofdg, oracle):
    """Areas and boxes: numpy on the GPU's own label planes.  Ids, types, counts: the blueprints of sample_counter.  Motions:
    bit for bit the composition the device path is defined with (detmath sin / cos; ofdg.host_realize uses libm's, which is
    why the counter-sampler extras test allows the flow 1 ULP - here the comparison is made with detmath itself, so no
    tolerance is needed)."""
    import torch
    W, H, B = 128, 96, 3
    g = make_gen(ofdg, W, H, 7, sampler=1, seed=5, background_prep=1)
    outs = ofdg.alloc_outputs(B, H, W)
    ex = ofdg.alloc_extras(B, H, W, LABELS)
    rows, counts = ofdg.alloc_object_table(B)
    rows.fill_(FILL)
    g.forward_counter(1000, B, *outs, extras=ex)
    g.object_table(ex["label0"], ex["label1"], rows, counts)
    g.synchronize()
    torch.cuda.synchronize()
    tasks, bps, _ = g.sample_counter(1000, B)
    raw, cnt = rows.cpu().numpy(), counts.cpu().numpy()
    tabs = ofdg.object_table_numpy(raw, cnt)
    l0, l1 = ex["label0"].cpu().numpy(), ex["label1"].cpu().numpy()
    for s in range(B):
        objs = [bps[tasks[s].first_object + k] for k in range(tasks[s].n_objects)]
        assert [o.obj_id for o in objs] == sorted(o.obj_id for o in objs)
        bg = bps[tasks[s].background]
        e = dict(l0=l0[s], l1=l1[s], ids=[bg.obj_id] + [o.obj_id for o in objs], types=[0] + [o.obj_type for o in objs],
                 motions=detmath_motions(oracle, W, H, bg, objs))
        check_sample(ofdg, tabs[s], int(cnt[s]), e, H, W)
        assert not raw[s, cnt[s]:].any()
        assert l0[s].max() < cnt[s] and l1[s].max() < cnt[s]


def hidden_and_off_frame_batch(ofdg, W, H):
    """Hand-made blueprints on the background and an ellipse of a mode-3 sample (ellipses, translations only): four circles
    in ascending obj_id - one that leaves the frame entirely in frame 1, a small one, a larger one on the same centre with
    the same motion (painted later: it hides the small one in both frames), and an ordinary one."""
    tasks, bps, _ = ofdg.HostSampler(3, W, H).next(1)
    t = tasks[0]
    out = (ofdg.Blueprint * 5)()
    C.memmove(C.byref(out[0]), C.byref(bps[t.background]), C.sizeof(ofdg.Blueprint))
    circles = [(10., 30., 30., 6. * W, 0.), (8., 90., 50., 3., 2.), (20., 90., 50., 3., 2.), (12., 40., 70., 5., -4.)]
    for k, (r, cx, cy, tx, ty) in enumerate(circles, 1):
        b = out[k]
        C.memmove(C.byref(b), C.byref(bps[t.first_object]), C.sizeof(ofdg.Blueprint))
        assert b.obj_type == ofdg.OBJ_ELLIPSE
        b.obj_id = 9 + k
        b.init_rot, b.init_trans_x, b.init_trans_y = 0., cx, cy
        b.rot, b.scale, b.trans_x, b.trans_y = 0., 1., tx, ty
        b.ellipse_scale_x = b.ellipse_scale_y = r
    task = (ofdg.Task * 1)()
    task[0].background, task[0].first_object, task[0].n_objects = 0, 1, 4
    return task, out, 5


def test_hidden_and_off_frame_objects(ofdg, oracle):
    W, H = 128, 96
    tasks, bps, n = hidden_and_off_frame_batch(ofdg, W, H)
    exp = expected(ofdg, oracle, W, H, 3, tasks, 1, bps, n)
    areas = [[otr.area_and_box(exp[0][l], k)[0] for k in range(len(exp[0]["ids"]))] for l in ("l0", "l1")]
    assert areas[1][1] == 0 and areas[0][1] > 0, "the first object must be visible in frame 0 and gone in frame 1"
    assert areas[0][2] == 0 and areas[1][2] == 0, "the second object must be hidden in both frames"
    assert min(areas[0][3], areas[1][3], areas[0][4], areas[1][4]) > 0
    g = make_gen(ofdg, W, H, 3)
    raw, counts, _ = render_and_tabulate(ofdg, g, tasks, 1, bps, n)
    check_batch(ofdg, raw, counts, exp, H, W)


@pytest.mark.parametrize("per", [5, 65])
def test_truncation_and_guard_rows(ofdg, oracle, per):
    import torch
    W, H, B, G = 160, 100, 2, 3
    g = make_gen(ofdg, W, H, 7)
    tasks, bps, n = g.sample(B)
    assert all(tasks[t].n_objects >= 16 for t in range(B))
    full, full_counts, _ = render_and_tabulate(ofdg, g, tasks, B, bps, n)
    outs = ofdg.alloc_outputs(B, H, W)
    ex = ofdg.alloc_extras(B, H, W, LABELS)
    rbuf = torch.full((G + B * per + G, 96), FILL, dtype=torch.uint8, device="cuda")
    cbuf = torch.full((G + B + G,), -7, dtype=torch.int32, device="cuda")
    rows, counts = rbuf[G:G + B * per].view(B, per, 96), cbuf[G:G + B]
    g.render(tasks, B, bps, n, *outs, extras=ex)
    g.object_table(ex["label0"], ex["label1"], rows, counts)
    g.synchronize()
    torch.cuda.synchronize()
    rb, cb = rbuf.cpu().numpy(), cbuf.cpu().numpy()
    assert (rb[:G] == FILL).all() and (rb[G + B * per:] == FILL).all(), "guard rows around the table"
    assert (cb[:G] == -7).all() and (cb[G + B:] == -7).all(), "guard words around the counts"
    assert np.array_equal(cb[G:G + B], full_counts) and list(full_counts) == [1 + tasks[t].n_objects for t in range(B)]
    assert np.array_equal(rb[G:G + B * per].reshape(B, per, 96), full[:, :per]), "rows inside equal the full table's"
    if per == 65:
        check_batch(ofdg, full, full_counts, expected(ofdg, oracle, W, H, 7, tasks, B, bps, n), H, W)


def test_optional_label_planes(ofdg):
    W, H, B = 160, 100, 2
    g = make_gen(ofdg, W, H, 5)
    tasks, bps, n = g.sample(B)
    full, counts, _ = render_and_tabulate(ofdg, g, tasks, B, bps, n)
    ft = full.view(ofdg.OBJECT_ROW_DTYPE).reshape(B, -1)
    assert ft["area0"].any() and ft["area1"].any()
    for frames in ((True, False), (False, True), (False, False)):
        raw, cnt, _ = render_and_tabulate(ofdg, g, tasks, B, bps, n, frames=frames)
        t = raw.view(ofdg.OBJECT_ROW_DTYPE).reshape(B, -1)
        assert np.array_equal(cnt, counts)
        for name in ("obj_id", "obj_type", "motion"):
            assert np.ascontiguousarray(t[name]).tobytes() == np.ascontiguousarray(ft[name]).tobytes(), name
        for f in (0, 1):
            if frames[f]:
                assert np.array_equal(t["area%d" % f], ft["area%d" % f]) and np.array_equal(t["box%d" % f], ft["box%d" % f])
            else:
                for s in range(B):
                    c = int(cnt[s])
                    assert not t["area%d" % f][s].any()
                    assert (t["box%d" % f][s, :c] == np.array([W, H, -1, -1])).all() and not t["box%d" % f][s, c:].any()


def test_labels_of_the_compact_path_give_the_same_table(ofdg):
    W, H, B = 160, 100, 2
    tables = []
    for compact in (False, True):
        g = make_gen(ofdg, W, H, 7)  # (contexts made alike draw the same samples)
        tasks, bps, n = g.sample(B)
        tables.append(render_and_tabulate(ofdg, g, tasks, B, bps, n, compact=compact))
    assert np.array_equal(tables[0][0], tables[1][0]) and np.array_equal(tables[0][1], tables[1][1])
    assert tables[0][0].view(ofdg.OBJECT_ROW_DTYPE)["area1"].any()


@pytest.mark.parametrize("own", [False, True], ids=["callers_stream", "stream_own"])
def test_streams_and_slot_reuse(ofdg, oracle, own):
    """2 * chains + 1 render + object_table pairs back to back, every chain's slot reused twice, nothing waited for in
    between: every table is its own batch's."""
    import torch
    W, H, B = 128, 96, 1
    g = make_gen(ofdg, W, H, 7)
    K = 2 * g.num_chains() + 1
    user = torch.cuda.Stream()
    st = ofdg.STREAM_OWN if own else user.cuda_stream
    batches = [g.sample(B) for _ in range(K)]
    bufs = []
    for _ in range(K):
        rows, counts = ofdg.alloc_object_table(B)
        rows.fill_(FILL)
        bufs.append((ofdg.alloc_outputs(B, H, W), ofdg.alloc_extras(B, H, W, LABELS), rows, counts))
    torch.cuda.synchronize()  # (the fills ran on torch's stream)
    for (tasks, bps, n), (outs, ex, rows, counts) in zip(batches, bufs):
        g.render(tasks, B, bps, n, *outs, st, extras=ex)
        g.object_table(ex["label0"], ex["label1"], rows, counts, stream=st)
    g.synchronize(st)
    torch.cuda.synchronize()
    for (tasks, bps, n), (outs, ex, rows, counts) in zip(batches, bufs):
        check_batch(ofdg, rows.cpu().numpy(), counts.cpu().numpy(), expected(ofdg, oracle, W, H, 7, tasks, B, bps, n), H, W)
    # the chain bookkeeping lets the context go on: a plain forward behind a table call on a caller's stream
    outs, ex, rows, counts = bufs[0]
    tasks, bps, n = batches[0]
    plain = [ofdg.alloc_outputs(B, H, W) for _ in range(g.num_chains() + 1)]
    torch.cuda.synchronize()
    g.render(tasks, B, bps, n, *outs, user.cuda_stream, extras=ex)
    g.object_table(ex["label0"], ex["label1"], rows, counts, stream=user.cuda_stream)
    for p in plain:  # (one more than there are chains: the chain of the pair above is taken again)
        g.forward(*p)
    g.synchronize(user.cuda_stream)
    torch.cuda.synchronize()
    assert all(float(p[0].abs().sum()) > 0 for p in plain)
    check_batch(ofdg, rows.cpu().numpy(), counts.cpu().numpy(), expected(ofdg, oracle, W, H, 7, tasks, B, bps, n), H, W)


def test_refusals_enqueue_nothing(ofdg):
    import torch
    W, H, B = 128, 96, 2
    rows, counts = ofdg.alloc_object_table(B)
    lab = torch.zeros((B, H, W), dtype=torch.uint8, device="cuda")
    rows.fill_(FILL)
    counts.fill_(-7)
    torch.cuda.synchronize()

    def refused(g, call, word):
        with pytest.raises(ofdg.OfdgError) as e:
            call()
        assert e.value.code == ofdg.EINVAL and word in str(e.value), str(e.value)
        g.synchronize()
        torch.cuda.synchronize()
        assert bool((rows == FILL).all()) and bool((counts == -7).all())

    # a fresh context: there is no batch to annotate
    g = make_gen(ofdg, W, H, 7, batch_size=B)
    refused(g, lambda: g.object_table(lab, lab, rows, counts), "no render")
    # argument errors after a call (the C entry point itself: the Python checks would catch these first)
    outs = ofdg.alloc_outputs(B, H, W)
    ex = ofdg.alloc_extras(B, H, W, LABELS)
    g.forward(*outs, extras=ex)
    g.synchronize()
    L, vp = ofdg.lib(), C.c_void_p

    def raw_call(r, per, c):
        g._check(L.ofdg_object_table(g.h, vp(ex["label0"].data_ptr()), vp(ex["label1"].data_ptr()), r, per, c, vp(0)))

    refused(g, lambda: raw_call(vp(rows.data_ptr()), 0, vp(counts.data_ptr())), "rows_per_sample")
    refused(g, lambda: raw_call(None, 65, vp(counts.data_ptr())), "d_rows")
    refused(g, lambda: raw_call(vp(rows.data_ptr()), 65, None), "d_counts")
    g.object_table(ex["label0"], ex["label1"], rows, counts)  # (and the valid call still works)
    g.synchronize()
    assert int(counts.min()) >= 2
    rows.fill_(FILL)
    counts.fill_(-7)
    torch.cuda.synchronize()
    # mode 9: refused, also after a plain mode-9 call
    g9 = make_gen(ofdg, W, H, 9, sampler=1, seed=3, batch_size=B)
    g9.warp_generate(1, 3)
    g9.forward_counter(0, B, *outs)
    g9.synchronize()
    refused(g9, lambda: g9.object_table(None, None, rows, counts), "mode 9")


def test_flowloader_objects(ofdg):
    import torch
    W, H, B = 128, 96, 2
    kw = dict(width=W, height=H, mode=7, batch_size=B, sampler=1, seed=21)
    pool = lambda g: g.pool_synthetic(3, 2 * W, 2 * H, 11)  # noqa: E731
    loader = ofdg.FlowLoader(ofdg.default_params(**kw), pool=pool, prefetch=3, extras=LABELS, objects=True)
    plain = ofdg.FlowLoader(ofdg.default_params(**kw), pool=pool, prefetch=3, extras=LABELS)
    it, pit = iter(loader), iter(plain)
    for _ in range(3):
        i0, i1, fl, ex = next(it)
        p0, p1, pf, pex = next(pit)
        torch.cuda.current_stream().synchronize()
        assert set(ex) == set(LABELS) | {"objects", "object_counts"} and set(pex) == set(LABELS)
        for a, b in ((i0, p0), (i1, p1), (fl, pf), (ex["label0"], pex["label0"]), (ex["label1"], pex["label1"])):
            assert torch.equal(a, b)  # without objects=True the loader yields what it yields today - and with it, too
        cnt = ex["object_counts"].cpu().numpy()
        tabs = ofdg.object_table_numpy(ex["objects"], cnt)
        l0, l1 = ex["label0"].cpu().numpy(), ex["label1"].cpu().numpy()
        for s in range(B):
            assert len(tabs[s]) == cnt[s] >= 2 and tabs[s]["obj_id"][0] == ofdg.BACKGROUND_ID
            assert int(tabs[s]["area0"].sum()) == int(tabs[s]["area1"].sum()) == W * H
            otr.expect_geometry(tabs[s], l0[s], l1[s], (H, W))
