"""GPU tests of the device counter-based sampler (OFDG_SAMPLER_COUNTER): determinism and
index purity, statistical equivalence with the reference stream (it is not bitwise equal
by design), and end-to-end rendering of device-sampled blueprints against the oracle."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def fields(bps, tasks):
    """Per top-level object: dict of arrays."""
    out = {k: [] for k in ("type", "init_rot", "init_tx", "init_ty", "rot", "scale", "tx", "ty", "ncomp", "ex", "nseg", "curves", "px", "deform")}
    nobj = []
    bg = {k: [] for k in ("rot", "scale", "tx", "ty")}
    for t in tasks:
        nobj.append(t.n_objects)
        b = bps[t.background]
        bg["rot"].append(b.rot); bg["scale"].append(b.scale); bg["tx"].append(b.trans_x); bg["ty"].append(b.trans_y)
        for i in range(t.n_objects):
            o = bps[t.first_object + i]
            out["type"].append(o.obj_type); out["init_rot"].append(o.init_rot)
            out["init_tx"].append(o.init_trans_x); out["init_ty"].append(o.init_trans_y)
            out["rot"].append(o.rot); out["scale"].append(o.scale); out["tx"].append(o.trans_x); out["ty"].append(o.trans_y)
            out["ncomp"].append(o.n_components); out["ex"].append(o.ellipse_scale_x); out["nseg"].append(o.n_segments)
            out["curves"].append(sum(1 for j in range(o.n_segments) if o.segment_type[j] == 3))
            out["px"].append(o.segment_x[0]); out["deform"].append(o.do_warpfield_deformation)
    return {k: np.array(v) for k, v in out.items()}, np.array(nobj), {k: np.array(v) for k, v in bg.items()}


def ks(a, b):
    from scipy.stats import ks_2samp
    return ks_2samp(a, b).pvalue


@pytest.mark.parametrize("mode", list(range(1, 14)))
def test_counter_sampler_statistics_match_reference_stream(ofdg, mode):
    """Every one of the 13 mode tables (DataGenerator.cpp:1363-2001) as the device sampler holds it, against the
    reference-stream sampler of the same mode: trigger thresholds (point masses at rot = 0 / scale = 1), magnitudes
    (two-sample KS on the continuous parts), object-type sets, composite / thin / deform frequencies."""
    W, H, N = 512, 384, 600
    g = ofdg.Generator(ofdg.default_params(width=W, height=H, mode=mode, sampler=1, seed=1234))
    tasks, bps, n = g.sample_counter(0, N)
    rt, rb, rn = ofdg.HostSampler(mode, W, H).next(N, cap=N * 300)
    a, na, bga = fields(bps, tasks)
    b, nb, bgb = fields(rb, rt)
    # number of objects: uniform on 16..23
    assert set(np.unique(na)) <= set(range(16, 24)) and abs(na.mean() - nb.mean()) < 0.4
    # type frequencies (and the same set of types)
    for t in (1, 2, 3):
        assert abs((a["type"] == t).mean() - (b["type"] == t).mean()) < 0.03
        assert ((a["type"] == t).any()) == ((b["type"] == t).any()), t
    # continuous fields: two-sample KS
    for k in ("init_rot", "init_tx", "init_ty", "tx", "ty"):
        assert ks(a[k], b[k]) > 1e-3, k
        assert abs(a[k].std() - b[k].std()) <= 0.05 * max(b[k].std(), 1e-6), k    # magnitudes (mode tables)
    for k in ("rot", "scale"):  # point mass at 0 / 1 (trigger) + shaped Gaussian
        rest = 0 if k == "rot" else 1
        assert abs((a[k] == rest).mean() - (b[k] == rest).mean()) < 0.03, k
        fa, fb = a[k][a[k] != rest], b[k][b[k] != rest]
        assert (len(fa) > 50) == (len(fb) > 50), k
        if len(fa) > 50:
            assert ks(fa, fb) > 1e-3, k
            assert abs(fa.std() - fb.std()) <= 0.08 * fb.std(), k
    for k in ("rot", "scale", "tx", "ty"):
        rest = 1 if k == "scale" else 0
        assert abs((bga[k] == rest).mean() - (bgb[k] == rest).mean()) < 0.08, "bg " + k
        fa, fb = bga[k][bga[k] != rest], bgb[k][bgb[k] != rest]
        assert (len(fa) > 30) == (len(fb) > 30), "bg " + k
        if len(fa) > 30:
            assert ks(fa, fb) > 1e-4, "bg " + k
            assert abs(fa.std() - fb.std()) <= 0.25 * fb.std(), "bg " + k
    el = a["type"] == 1
    if el.any():
        assert ks(a["ex"][el], b["ex"][b["type"] == 1]) > 1e-3      # incl. the 0.05x "needle" mass in modes 7, 9-13
    po = a["type"] == 2
    if po.any():
        assert abs(a["nseg"][po].mean() - b["nseg"][b["type"] == 2].mean()) < 0.5
        assert abs(a["curves"][po].mean() - b["curves"][b["type"] == 2].mean()) < 0.15   # curve3 trigger (modes >= 4)
        assert ks(a["px"][po], b["px"][b["type"] == 2]) > 1e-3     # first vertex: radius x scale (thin polygons included)
    co = a["type"] == 3
    if co.any():
        assert abs(a["ncomp"][co].mean() - b["ncomp"][b["type"] == 3].mean()) < 0.3
    assert abs((a["deform"] != 0).mean() - (b["deform"] != 0).mean()) < 0.02       # mode 9: trigger 0.2, else never


def test_counter_sampler_is_a_pure_function_of_the_index(ofdg):
    W, H = 512, 384
    g = ofdg.Generator(ofdg.default_params(width=W, height=H, mode=7, sampler=1, seed=9))
    t1, b1, _ = g.sample_counter(100, 8)
    t2, b2, _ = g.sample_counter(104, 8)   # overlaps indices 104..107
    sz = C.sizeof(ofdg.Blueprint)
    fc = ofdg.Blueprint.first_component.offset // 4

    def live(bps, s, n_obj):
        """bytes of the live blueprints of sample s (unused slots hold stale data)."""
        a = np.frombuffer(C.string_at(C.addressof(bps) + s * 257 * sz, 257 * sz), np.int32).reshape(257, -1).copy()
        a[:, fc] = 0  # component indices are positions in the batch array
        rows = [0] + [1 + o for o in range(n_obj)]
        for o in range(n_obj):
            b = bps[s * 257 + 1 + o]
            if b.obj_type == 3:
                rows += [1 + 32 + o * 7 + k for k in range(b.n_components)]
        return a[rows]

    for k in range(4):
        assert t1[4 + k].n_objects == t2[k].n_objects
        assert np.array_equal(live(b1, 4 + k, t1[4 + k].n_objects), live(b2, k, t2[k].n_objects))
    g2 = ofdg.Generator(ofdg.default_params(width=W, height=H, mode=7, sampler=1, seed=10))
    t3, b3, _ = g2.sample_counter(100, 1)
    assert not np.array_equal(live(b3, 0, t3[0].n_objects)[:17], live(b1, 0, t1[0].n_objects)[:17])   # the seed matters


def test_detmath_on_the_device_equals_the_host_bit_for_bit(ofdg, oracle):
    """include/ofdg_detmath.h is fp64 +, -, * only: gfx950 and the host produce the same bits."""
    rng = np.random.default_rng(5)
    a = np.concatenate([rng.uniform(-8, 8, 300000), rng.uniform(-8, 8, 300000).astype(np.float32).astype(np.float64),
                        rng.uniform(-1e5, 1e5, 100000), [0.0, -0.0, np.pi, 1e-300, 1e9, np.inf]])
    x = np.concatenate([rng.uniform(-120, 90, 400000), [0.0, -0.0, -1e4, 1e4]]).astype(np.float32)
    g = ofdg.Generator(ofdg.default_params(width=64, height=48, mode=1))
    s, c, e = g.debug_detmath(a, x)
    hs, hc = oracle.det_sincos(a)
    he = oracle.det_expf(x)
    assert np.array_equal(s.view(np.int64), hs.view(np.int64)) and np.array_equal(c.view(np.int64), hc.view(np.int64))
    assert np.array_equal(e.view(np.int32), he.view(np.int32))


def ulp_diff(got, exp):
    a = got.view(np.int32).astype(np.int64); b = exp.view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7FFFFFFF), a); b = np.where(b < 0, -(b & 0x7FFFFFFF), b)
    return np.abs(a - b)


def counter_vs_oracle(ofdg, oracle, mode, W, H, B, first, seed=77, pool=(4, 256, 192), threads=1, num_objects=0, background_prep=0, pool_seed=5):
    """ofdg_forward_counter (device sampling + device realize + render: the path bench.py times) against the oracle
    fed with the blueprints ofdg_sample_counter downloads.  The device builds its affines with include/ofdg_detmath.h;
    so does the oracle here (oracle.detmath()): every byte must agree."""
    g = ofdg.Generator(ofdg.default_params(width=W, height=H, mode=mode, sampler=1, seed=seed, num_objects=num_objects, background_prep=background_prep))
    g.pool_synthetic(pool[0], pool[1], pool[2], pool_seed)
    crops = None
    if mode == 9:
        crops = oracle.warp_crops(W, H, seed=5)[::5][:6] * 4.0
        g.warp_upload(crops)
    pl = g.pool_download_all()
    i0, i1, fl = ofdg.alloc_outputs(B, H, W)
    g.forward_counter(first, B, i0, i1, fl)
    g.synchronize()
    tasks, bps, n = g.sample_counter(first, B)
    q = oracle.default_params(W, H, mode)
    q.background_prep = background_prep
    with oracle.detmath():
        e0, e1, ef = oracle.render(q, tasks, B, bps, n, pl, warp_crops=crops, reuse=-1, n_threads=threads)
    g0, g1, gf = i0.cpu().numpy(), i1.cpu().numpy(), fl.cpu().numpy()
    assert np.array_equal(g0, e0), (np.abs(g0 - e0) > 0).sum()
    assert np.array_equal(g1, e1), (np.abs(g1 - e1) > 0).sum()
    assert np.array_equal(np.isnan(gf), np.isnan(ef))
    ok = ~np.isnan(ef)
    assert ulp_diff(gf[ok], ef[ok]).max() <= 1     # north-star tolerance; in practice 0
    assert (ulp_diff(gf[ok], ef[ok]) > 0).mean() < 1e-6
    return tasks, bps, crops, (e0, e1, ef)


@pytest.mark.parametrize("mode", list(range(1, 14)))
def test_counter_forward_matches_oracle_on_its_own_blueprints(ofdg, oracle, mode):
    """All 13 modes at 128 x 96: frames bit-exact, flow <= 1 ULP on every value (NaN pattern included in mode 9)."""
    tasks, bps, crops, _ = counter_vs_oracle(ofdg, oracle, mode, 128, 96, 6, first=40)
    if mode == 9:
        flags = [bps[t.background].do_warpfield_deformation for t in tasks] + \
                [bps[t.first_object + i].do_warpfield_deformation for t in tasks for i in range(t.n_objects)]
        assert sum(1 for f in flags if f) >= 5 and max(flags) <= len(crops)


def test_counter_forward_matches_oracle_at_benchmark_size(ofdg, oracle):
    """BASELINE config 2 as bench.py runs it (mode 5, 512 x 384, batch 32, 16 objects, counter sampler), one whole
    batch against the oracle: frames bit-exact, flow <= 1 ULP."""
    counter_vs_oracle(ofdg, oracle, 5, 512, 384, 32, first=64, seed=0, pool=(6, 1024, 768), threads=8, num_objects=16)


def test_forward_with_counter_sampler_shards_by_index(ofdg):
    import torch
    W, H, B = 128, 96, 4
    outs = []
    for rank in range(2):
        g = ofdg.Generator(ofdg.default_params(width=W, height=H, mode=5, sampler=1, seed=3, batch_size=B, rank=rank, world_size=2))
        g.pool_synthetic(3, 256, 192, 1)
        i0, i1, fl = ofdg.alloc_outputs(B, H, W)
        g.forward(i0, i1, fl); g.synchronize()      # step 0
        a = i0.clone()
        g.forward(i0, i1, fl); g.synchronize()      # step 1
        outs.append((a, i0.clone()))
    ref = ofdg.Generator(ofdg.default_params(width=W, height=H, mode=5, sampler=1, seed=3))
    ref.pool_synthetic(3, 256, 192, 1)
    i0, i1, fl = ofdg.alloc_outputs(B, H, W)
    for step in range(2):
        for rank in range(2):
            ref.forward_counter(step * B * 2 + rank * B, B, i0, i1, fl); ref.synchronize()
            assert torch.equal(i0, outs[rank][step])


@pytest.mark.parametrize("nobj", [16, 24, 32])
def test_counter_forward_is_repeatable_across_its_slot_ring(ofdg, nobj):
    """The same global indices rendered five times in a row (every call lands in another slot of
    the private ring, first use included, and the sampler runs ahead on its own stream) give
    identical bytes: no read of a buffer before its initialisation has finished."""
    import torch
    W, H, B = 128, 96, 4
    g = ofdg.Generator(ofdg.default_params(width=W, height=H, mode=5, sampler=1, seed=77, num_objects=nobj))
    g.pool_synthetic(4, 256, 192, 5)
    i0, i1, fl = ofdg.alloc_outputs(B, H, W)
    ref = None
    for _ in range(5):
        g.forward_counter(40, B, i0, i1, fl)
        g.synchronize()
        cur = (i0.cpu().numpy().copy(), i1.cpu().numpy().copy(), fl.cpu().numpy().copy())
        if ref is None:
            ref = cur
        for a, b in zip(cur, ref):
            assert np.array_equal(a, b)


def test_counter_sampler_mode9_matches_oracle_with_named_crops(ofdg, oracle):
    """Mode 9 on the device sampler: the crop of a deforming object is a function of (seed, sample, object);
    ofdg_sample_counter returns it as do_warpfield_deformation = 1 + crop, and the oracle renders with exactly
    those crops (reuse = -1): bit-exact like the rigid modes, and the deformations are not a no-op."""
    W, H, B = 128, 96, 8
    tasks, bps, crops, (e0, e1, ef) = counter_vs_oracle(ofdg, oracle, 9, W, H, B, first=300, seed=12)
    n = B * 257
    flags = [bps[t.background].do_warpfield_deformation for t in tasks] + \
            [bps[t.first_object + i].do_warpfield_deformation for t in tasks for i in range(t.n_objects)]
    assert sum(1 for f in flags if f) >= 10 and max(flags) <= len(crops) and len({f for f in flags if f}) >= 3
    # rigid rendering of the same samples differs (frame 1 and flow)
    for i in range(n):
        bps[i].do_warpfield_deformation = 0
    pool = ofdg.Generator(ofdg.default_params(width=W, height=H, mode=9, sampler=1, seed=12))
    pool.pool_synthetic(4, 256, 192, 5)
    with oracle.detmath():
        r0, r1, rf = oracle.render(oracle.default_params(W, H, 9), tasks, B, bps, n, pool.pool_download_all(), warp_crops=crops, reuse=-1)
    assert (r1 != e1).mean() > 0.01


def test_counter_sampler_mode9_prepared_backgrounds_match_oracle(ofdg, oracle):
    """Mode 9 on the device sampler with prepared backgrounds (background_prep = 1): a background that deforms reads its
    own 2W x 2H texture at displaced positions, so the device realize grows the prepared region by the crop's largest
    displacement (bg_prep_region with grow > 0); a rigid one gets the plain region (grow = 0).  A batch with both kinds
    against the oracle, which prepares whole textures: frames bit-exact, flow <= 1 ULP."""
    W, H, B = 128, 96, 16
    tasks, bps, crops, _ = counter_vs_oracle(ofdg, oracle, 9, W, H, B, first=300, seed=12, pool=(4, 2 * W + 64, 2 * H + 56),
                                             background_prep=1, pool_seed=7)
    flags = [bps[t.background].do_warpfield_deformation for t in tasks]
    assert any(f != 0 for f in flags) and any(f == 0 for f in flags), flags
    assert max(flags) <= len(crops)


def test_flow_loader_ring_yields_the_index_stream_in_order(ofdg):
    """FlowLoader (prefetch ring over ofdg_forward): batch k of the iterator is the samples with global
    indices k*B .. k*B+B-1, although up to prefetch-1 later batches are already in flight."""
    import torch
    W, H, B = 128, 96, 3
    prm = ofdg.default_params(width=W, height=H, mode=5, sampler=1, seed=8, batch_size=B)
    loader = ofdg.FlowLoader(prm, pool=lambda g: g.pool_synthetic(3, 256, 192, 2), prefetch=3)
    got = []
    for k, (a, b, f) in zip(range(5), loader):
        torch.cuda.synchronize()
        got.append((a.clone(), b.clone(), f.clone()))
    g = ofdg.Generator(ofdg.default_params(width=W, height=H, mode=5, sampler=1, seed=8, batch_size=B))
    g.pool_synthetic(3, 256, 192, 2)
    i0, i1, fl = ofdg.alloc_outputs(B, H, W)
    for k in range(5):
        g.forward_counter(k * B, B, i0, i1, fl)
        g.synchronize()
        assert torch.equal(got[k][0], i0) and torch.equal(got[k][1], i1) and torch.equal(got[k][2], fl)


def test_flow_loader_resumes_at_a_batch_index(ofdg):
    """FlowLoader(start=k): the iterator continues with batch k of the stream (`consumed` is what a checkpoint stores)."""
    import torch
    W, H, B = 128, 96, 2
    prm = ofdg.default_params(width=W, height=H, mode=5, sampler=1, seed=8, batch_size=B)
    fill = lambda g: g.pool_synthetic(3, 256, 192, 2)
    a = ofdg.FlowLoader(prm, pool=fill, prefetch=3)
    ref = []
    for k, o in zip(range(6), a):
        torch.cuda.synchronize()
        ref.append([t.clone() for t in o])
    assert a.consumed == 6
    b = ofdg.FlowLoader(prm, pool=fill, prefetch=4, start=4)
    for k, o in zip((4, 5), b):
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(o, ref[k]))
    assert b.consumed == 6


def test_flow_loader_hands_batches_to_a_consumer_stream(ofdg):
    """FlowLoader with a consumer stream of the caller's: the consumer's kernels (here: a running sum on that
    stream, enqueued without any host synchronisation) see complete batches, and a buffer set is not re-rendered
    before the consumer work that reads it has run - the sums equal those of isolated renders."""
    import torch
    W, H, B = 128, 96, 2
    prm = ofdg.default_params(width=W, height=H, mode=5, sampler=1, seed=9, batch_size=B)
    side = torch.cuda.Stream()
    loader = ofdg.FlowLoader(prm, pool=lambda g: g.pool_synthetic(3, 256, 192, 2), prefetch=3, stream=side.cuda_stream)
    sums = []
    with torch.cuda.stream(side):
        for k, (a, b, f) in zip(range(12), loader):
            big = a.double().sum() + b.double().sum() * 3 + torch.nan_to_num(f.double()).sum() * 7   # (enqueued on `side`)
            for _ in range(20):                      # keep the consumer busy while the ring renders ahead
                big = big + (a.double() * 0).sum()
            sums.append(big)
    torch.cuda.synchronize()
    g = ofdg.Generator(ofdg.default_params(width=W, height=H, mode=5, sampler=1, seed=9, batch_size=B))
    g.pool_synthetic(3, 256, 192, 2)
    o = ofdg.alloc_outputs(B, H, W)
    for k in range(12):
        g.forward_counter(k * B, B, *o)
        g.synchronize()
        want = o[0].double().sum() + o[1].double().sum() * 3 + torch.nan_to_num(o[2].double()).sum() * 7
        assert float(sums[k]) == float(want), k


def test_counter_sampler_has_room_for_the_worst_case_sample(ofdg):
    """32 objects per sample in mode 7 (BASELINE config 4): up to 7 outlines per object - the device sampler's
    per-sample outline slots must cover the worst case (no capacity error), at 1024x768."""
    W, H, B = 1024, 768, 4
    g = ofdg.Generator(ofdg.default_params(width=W, height=H, mode=7, sampler=1, seed=2, num_objects=32, batch_size=B))
    g.pool_synthetic(3, 2048, 1536, 1)
    # find a sample with more outlines than the old fixed capacity of 96 (about 1 in 250)
    hit = None
    for first in range(0, 8192, 256):
        tasks, bps, n = g.sample_counter(first, 256)
        for k, t in enumerate(tasks):
            if sum(max(1, bps[t.first_object + i].n_components) for i in range(t.n_objects)) > 96:
                hit = first + k
                break
        if hit is not None:
            break
    assert hit is not None, "no sample with more than 96 outlines among 8192"
    i0, i1, fl = ofdg.alloc_outputs(B, H, W)
    g.forward_counter(hit - hit % B, B, i0, i1, fl)
    g.synchronize()   # raises on a device capacity flag
    import torch
    assert torch.isfinite(fl).all()


@pytest.mark.parametrize("own_stream", [False, True])
def test_interleaved_entry_points_give_the_same_bytes_as_isolated_calls(ofdg, own_stream):
    """Stream/event plumbing: ofdg_render, ofdg_render_slot on several resident slots and ofdg_forward_counter
    interleaved at random on one context (in-order chains taking turns, one coverage workspace and one private
    slot each, user slots shared between them) produce exactly what each call produces on a fresh context -
    both when the caller passes its own stream (cross-stream hand-over) and when it passes ofdg_stream(),
    where consecutive calls overlap on the device."""
    import torch
    W, H, B = 128, 96, 3
    rng = np.random.default_rng(0)

    def fresh():
        g = ofdg.Generator(ofdg.default_params(width=W, height=H, mode=7, sampler=1, seed=4, batch_size=B))
        g.pool_synthetic(3, 256, 192, 2)
        return g

    hs = ofdg.HostSampler(7, W, H)
    batches = [hs.next(B, cap=B * 64) for _ in range(4)]

    def isolated(kind, arg):
        g = fresh()
        o = ofdg.alloc_outputs(B, H, W)
        if kind == "counter":
            g.forward_counter(arg, B, *o)
        else:
            t, b, n = batches[arg]
            g.render(t, B, b, n, *o)
        g.synchronize()
        return [x.clone() for x in o]

    want = {("counter", i): isolated("counter", i) for i in (0, 3, 6, 9, 50)}
    want.update({("host", k): isolated("host", k) for k in range(4)})
    g = fresh()
    for k in range(4):
        t, b, n = batches[k]
        g.upload_slot(k, t, B, b, n)
    outs = [ofdg.alloc_outputs(B, H, W) for _ in range(3)]
    log = []
    seen = set()
    for step in range(40):
        o = outs[step % 3]
        r = rng.integers(0, 3)
        st = g.next_stream() if own_stream else 0
        seen.add(st)
        if r == 0:
            i = int(rng.choice([0, 3, 6, 9, 50]))
            g.forward_counter(i, B, *o, st)
            key = ("counter", i)
        elif r == 1:
            k = int(rng.integers(0, 4))
            g.render_slot(k, *o, st)
            key = ("host", k)
        else:
            k = int(rng.integers(0, 4))
            t, b, n = batches[k]
            g.render(t, B, b, n, *o, st)   # (records travel into the chain's private slot)
            g.upload_slot(0, *batches[0][:1], B, batches[0][1], batches[0][2])   # (slot 0 replaced while in use)
            key = ("host", k)
        log.append((step % 3, key))
        if step % 3 == 2 or step == 39:   # check the buffers written since the last check
            g.synchronize()
            for bi, kk in log:
                for a, w in zip(outs[bi], want[kk]):
                    assert torch.equal(a, w), (step, kk)
            log = []
    assert len(seen) == (3 if own_stream else 1) and (0 not in seen or not own_stream)   # the chains take turns


def test_render_resident_repeats_the_last_call(ofdg):
    """ofdg_render_resident re-renders the records of the last render / forward call (whichever chain they live
    on) into other buffers: identical bytes."""
    import torch
    W, H, B = 128, 96, 2
    g = ofdg.Generator(ofdg.default_params(width=W, height=H, mode=7, sampler=1, seed=3, batch_size=B))
    g.pool_synthetic(3, 256, 192, 2)
    a = ofdg.alloc_outputs(B, H, W)
    b = ofdg.alloc_outputs(B, H, W)
    t, bp, n = ofdg.HostSampler(7, W, H).next(B, cap=B * 64)
    for first in (lambda: g.render(t, B, bp, n, *a, g.next_stream()), lambda: g.forward_counter(11, B, *a)):
        first()
        for _ in range(4):   # (every repeat runs on the next chain)
            for x in b:
                x.zero_()
            torch.cuda.synchronize()
            g.render_resident(*b, g.next_stream())
            g.synchronize()
            for x, y in zip(a, b):
                assert torch.equal(x, y)


def test_pipeline_shape_does_not_change_the_bytes(ofdg, tmp_path):
    """ofdg_params.chains (number of in-order chains), .serial (everything on the caller's stream) and .lookahead
    (batches prepared ahead of the call that composes them) are scheduling choices: the same calls produce the same
    bytes as the default."""
    import subprocess, sys, os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "run.py"
    script.write_text('''
import importlib, sys, numpy as np, torch
sys.path.insert(0, %r)
ofdg = importlib.import_module("optical-flow-2d-data-generation_amd")
W, H, B = 128, 96, 3
g = ofdg.Generator(ofdg.default_params(width=W, height=H, mode=7, sampler=1, seed=6, batch_size=B, **eval(sys.argv[2])))
g.pool_synthetic(3, 256, 192, 2)
outs = [ofdg.alloc_outputs(B, H, W) for _ in range(5)]
for k in range(5):
    g.forward_counter(7 * k, B, *outs[k], g.next_stream() if k %% 2 else 0)
g.synchronize()
np.savez(sys.argv[1], *[t.cpu().numpy() for o in outs for t in o])
''' % root)
    results = []
    for kw in ({}, {"chains": 1}, {"chains": 2}, {"serial": 1}, {"lookahead": 2}, {"chains": 2, "lookahead": 1}):
        out = tmp_path / ("out_%d.npz" % len(results))
        subprocess.run([sys.executable, str(script), str(out), repr(kw)], check=True, env=dict(os.environ), timeout=300)
        results.append(np.load(out))
    for other in results[1:]:
        for k in results[0].files:
            assert np.array_equal(results[0][k], other[k]), k


@pytest.mark.parametrize("sampler,mode", [(0, 7), (1, 7), (0, 9), (1, 9)])
def test_forward_resumes_from_a_step_counter(ofdg, sampler, mode):
    """Checkpoint / resume: a fresh context with step = k continues exactly where another one was after k
    batches - reference streams (replayed on the host) and counter sampler alike, also per rank."""
    import torch
    W, H, B = 128, 96, 2
    def make(rank=0, world=1):
        g = ofdg.Generator(ofdg.default_params(width=W, height=H, mode=mode, sampler=sampler, seed=5, batch_size=B, rank=rank, world_size=world))
        g.pool_synthetic(3, 256, 192, 2)
        if mode == 9:
            g.warp_generate(1, seed=4)   # (mode 9, reference streams: the crop serving order is part of the state)
        return g
    for rank, world in ((0, 1), (1, 2)):
        g = make(rank, world)
        outs = []
        for k in range(5):
            o = ofdg.alloc_outputs(B, H, W)
            g.forward(*o)
            outs.append(o)
        g.synchronize()
        assert g.step == 5
        r = make(rank, world)
        r.step = 3
        for k in (3, 4):
            o = ofdg.alloc_outputs(B, H, W)
            r.forward(*o)
            r.synchronize()
            assert all(torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)) for a, b in zip(o, outs[k])), (rank, k)
    if mode == 9:   # the batches do use different crops: the state matters
        assert not torch.equal(torch.nan_to_num(outs[3][1]), torch.nan_to_num(outs[4][1]))
