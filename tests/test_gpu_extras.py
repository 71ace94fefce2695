"""GPU tests of the optional outputs (ofdg_render_ex / ofdg_forward_ex / ofdg_forward_counter_ex): backward flow,
labels and occlusion maps against the numpy restatement of their definitions (extras_reference.py, pinned to the
oracle by tests/test_extras_reference.py), and the guarantees around them."""
import ctypes as C

import numpy as np
import pytest

import extras_reference as xr

pytestmark = pytest.mark.gpu

ALL = ("flow1", "occ0", "occ1", "label0", "label1")


def make_gen(ofdg, W, H, mode, **kw):
    g = ofdg.Generator(ofdg.default_params(width=W, height=H, mode=mode, **kw))
    g.pool_synthetic(3, 2 * W, 2 * H, 11)
    return g


def run(ofdg, g, tasks, n, bps, n_bps, names=ALL):
    import torch
    W, H = g.params.width, g.params.height
    outs = ofdg.alloc_outputs(n, H, W)
    ex = ofdg.alloc_extras(n, H, W, names) if names is not None else None
    for t in outs:
        t.fill_(-12345)
    for k, t in (ex or {}).items():
        t.fill_(77)
    g.render(tasks, n, bps, n_bps, *outs, extras=ex)
    g.synchronize()
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in outs], {k: t.cpu().numpy() for k, t in (ex or {}).items()}


def check_against_helper(got, ref, flow1_ulp=0):
    for k in ("label0", "label1"):
        assert np.array_equal(got[k], ref[k]), "%s differs at %d px" % (k, (got[k] != ref[k]).sum())
    d = xr.ulp_diff(got["flow1"], ref["flow1"])
    assert d.max() <= flow1_ulp, "flow1 differs by up to %d ULP at %d px" % (d.max(), (d > flow1_ulp).sum())


@pytest.mark.parametrize("W,H,mode,aa", [(W, H, m, 1) for (W, H) in ((128, 96), (160, 100)) for m in (1, 2, 3, 5, 7, 13)]
                         + [(512, 384, 7, 1), (512, 384, 7, 0)])
def test_extras_match_definitions_host_sampler(ofdg, oracle, W, H, mode, aa):
    B = 1 if W == 512 else 2
    g = make_gen(ofdg, W, H, mode, use_antialiasing=aa)
    tasks, bps, n = g.sample(B)
    (i0, i1, fl), ex = run(ofdg, g, tasks, B, bps, n)
    ref = xr.reference_extras(ofdg, oracle, oracle.default_params(W, H, mode, aa), tasks, B, bps, n, g.pool_download_all())
    assert np.array_equal(fl.view(np.int32), ref["flow"].view(np.int32))
    check_against_helper(ex, ref)
    for k in ("occ0", "occ1"):
        assert np.array_equal(ex[k], ref[k]), "%s differs at %d px" % (k, (ex[k] != ref[k]).sum())


def test_extras_counter_sampler_with_background_prep(ofdg, oracle):
    import torch
    W, H, B = 128, 96, 3
    g = make_gen(ofdg, W, H, 7, sampler=1, seed=5, background_prep=1)
    outs = ofdg.alloc_outputs(B, H, W)
    ex = ofdg.alloc_extras(B, H, W)
    g.forward_counter(1000, B, *outs, extras=ex)
    plain = ofdg.alloc_outputs(B, H, W)
    g.forward_counter(1000, B, *plain)
    g.synchronize()
    for a, b in zip(outs, plain):
        assert torch.equal(a, b)
    tasks, bps, n = g.sample_counter(1000, B)
    pool = np.random.default_rng(0).integers(0, 256, (3, 3, 2 * H, 2 * W), dtype=np.uint8)
    sub = (ofdg.Blueprint * n)()
    C.memmove(sub, bps, C.sizeof(sub))
    for i in range(n):
        sub[i].tex_id = sub[i].tex_id % 3
    with oracle.detmath():
        ref = xr.reference_extras(ofdg, oracle, oracle.default_params(W, H, 7), tasks, B, sub, n, pool)
    got = {k: t.cpu().numpy() for k, t in ex.items()}
    check_against_helper(got, ref, flow1_ulp=1)
    fl = outs[2].cpu().numpy()
    assert xr.ulp_diff(fl, ref["flow"]).max() <= 1
    for s in range(B):  # the occlusion rule on the device's own flows and the (exact) labels
        assert np.array_equal(got["occ0"][s], xr.occlusion(fl[s], ref["label0"][s], ref["label1"][s]))
        assert np.array_equal(got["occ1"][s], xr.occlusion(got["flow1"][s], ref["label1"][s], ref["label0"][s]))


@pytest.mark.parametrize("W,H", [(128, 96), (160, 100)])
def test_extras_leave_the_outputs_alone_and_are_independent(ofdg, W, H):
    B = 3
    g = make_gen(ofdg, W, H, 5)
    tasks, bps, n = g.sample(B)
    plain, _ = run(ofdg, g, tasks, B, bps, n, names=None)
    full, ex_all = run(ofdg, g, tasks, B, bps, n)
    for a, b in zip(plain, full):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    for name in ALL:
        outs, ex = run(ofdg, g, tasks, B, bps, n, names=(name,))
        assert set(ex) == {name}
        assert np.array_equal(ex[name].view(np.uint8), ex_all[name].view(np.uint8)), name
        for a, b in zip(plain, outs):
            assert np.array_equal(a.view(np.int32), b.view(np.int32))
    # all-NULL extras: the plain call
    outs, ex = run(ofdg, g, tasks, B, bps, n, names=())
    assert ex == {}
    for a, b in zip(plain, outs):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


def test_occlusion_follows_from_the_gpus_own_labels_and_flows(ofdg):
    W, H, B = 512, 384, 4
    g = make_gen(ofdg, W, H, 7, sampler=1, seed=9)
    import torch
    outs = ofdg.alloc_outputs(B, H, W)
    ex = ofdg.alloc_extras(B, H, W)
    g.forward_counter(0, B, *outs, extras=ex)
    g.synchronize()
    torch.cuda.synchronize()
    fl = outs[2].cpu().numpy()
    got = {k: t.cpu().numpy() for k, t in ex.items()}
    for s in range(B):
        assert np.array_equal(got["occ0"][s], xr.occlusion(fl[s], got["label0"][s], got["label1"][s]))
        assert np.array_equal(got["occ1"][s], xr.occlusion(got["flow1"][s], got["label1"][s], got["label0"][s]))


def test_backward_flow_is_physically_consistent_full_size(ofdg):
    """Where occ0 == 0, |flow0(p) + flow1(round(p + flow0(p)))| <= (1 + |M^-1|) sqrt(2)/2: the target's rounding to a
    pixel, mapped back through the owner's inverse motion.  Occlusion is present and far from everywhere."""
    W, H, B = 512, 384, 2
    g = make_gen(ofdg, W, H, 7)
    tasks, bps, n = g.sample(B)
    (_, _, fl), ex = run(ofdg, g, tasks, B, bps, n)
    _, om = ofdg.host_realize(g.params, 3, 2 * W, 2 * H, tasks, B, bps, n)
    inv_norm = max(np.linalg.norm(np.linalg.inv(np.array([[m[0], m[2]], [m[1], m[3]]])), 2) for m in om[:, 0])
    bound = (1 + inv_norm) * np.sqrt(2) / 2 + 1e-3
    ys, xs = np.mgrid[0:H, 0:W]
    for s in range(B):
        f0, f1, occ = fl[s], ex["flow1"][s], ex["occ0"][s, 0]
        xr_ = np.floor(xs.astype(np.float32) + f0[0] + np.float32(0.5)).astype(np.int64)
        yr_ = np.floor(ys.astype(np.float32) + f0[1] + np.float32(0.5)).astype(np.int64)
        vis = occ == 0
        e = np.hypot(f0[0][vis] + f1[0][yr_[vis], xr_[vis]], f0[1][vis] + f1[1][yr_[vis], xr_[vis]])
        assert e.max() <= bound, (e.max(), bound)
        for k in ("occ0", "occ1"):
            assert 0.0 < ex[k][s].mean() < 0.5


def test_extras_edge_cases(ofdg):
    import torch
    W, H = 128, 96
    g = make_gen(ofdg, W, H, 7)
    # ragged batches: 1 and 5 samples through the same context, each equal to its own definition of "alone"
    for B in (1, 5, 1):
        tasks, bps, n = g.sample(B)
        (_, _, fl), ex = run(ofdg, g, tasks, B, bps, n)
        for s in range(B):
            assert np.array_equal(ex["occ0"][s], xr.occlusion(fl[s], ex["label0"][s], ex["label1"][s]))
    # an empty batch is an argument error
    tasks, bps, n = g.sample(1)
    outs = ofdg.alloc_outputs(1, H, W)
    with pytest.raises(ofdg.OfdgError) as e:
        g.render(tasks, 0, bps, n, *outs, extras=ofdg.alloc_extras(0, H, W))
    assert e.value.code == ofdg.EINVAL
    # wrong shapes / dtypes are refused before the call
    with pytest.raises(ValueError):
        g.render(tasks, 1, bps, n, *outs, extras={"label0": torch.zeros((1, H, W), dtype=torch.float32, device="cuda")})
    with pytest.raises(ValueError):
        g.render(tasks, 1, bps, n, *outs, extras={"flow1": torch.zeros((2, 2, H, W), device="cuda")})


def test_mode9_extras_are_refused_and_nothing_is_enqueued(ofdg):
    import torch
    W, H, B = 128, 96, 2
    g = make_gen(ofdg, W, H, 9, sampler=1, seed=3, batch_size=B)
    g.warp_generate(1, 3)
    outs = ofdg.alloc_outputs(B, H, W)
    for t in outs:
        t.fill_(-1)
    ex = ofdg.alloc_extras(B, H, W, ("label0",))
    ex["label0"].fill_(200)
    torch.cuda.synchronize()
    before = g.last_ticket()
    for call in (lambda: g.forward_counter(0, B, *outs, extras=ex), lambda: g.forward(*outs, extras=ex)):
        with pytest.raises(ofdg.OfdgError) as e:
            call()
        assert e.value.code == ofdg.EINVAL and "rigid" in str(e.value)
    g.synchronize()
    torch.cuda.synchronize()
    assert g.last_ticket() == before
    assert all(bool((t == -1).all()) for t in outs) and bool((ex["label0"] == 200).all())
    g.forward_counter(0, B, *outs, extras={})  # (all-NULL extras: the plain mode-9 call)
    g.synchronize()
    assert g.last_ticket() != before


def test_flowloader_with_extras_hands_out_the_direct_batches(ofdg):
    import torch
    W, H, B = 128, 96, 2
    kw = dict(width=W, height=H, mode=7, batch_size=B, sampler=1, seed=21)
    loader = ofdg.FlowLoader(ofdg.default_params(**kw), pool=lambda g: g.pool_synthetic(3, 2 * W, 2 * H, 11), prefetch=3,
                             extras=("flow1", "occ0", "label1"))
    g = make_gen(ofdg, W, H, 7, batch_size=B, sampler=1, seed=21)
    it = iter(loader)
    for _ in range(4):
        i0, i1, fl, ex = next(it)
        torch.cuda.current_stream().synchronize()
        got = [i0.clone(), i1.clone(), fl.clone()] + [ex[k].clone() for k in ("flow1", "occ0", "label1")]
        outs = ofdg.alloc_outputs(B, H, W)
        dx = ofdg.alloc_extras(B, H, W, ("flow1", "occ0", "label1"))
        g.forward(*outs, extras=dx)
        g.synchronize()
        want = list(outs) + [dx[k] for k in ("flow1", "occ0", "label1")]
        for a, b in zip(got, want):
            assert torch.equal(a, b)
    plain = ofdg.FlowLoader(ofdg.default_params(**kw), pool=lambda g: g.pool_synthetic(3, 2 * W, 2 * H, 11), prefetch=2)
    assert len(next(iter(plain))) == 3
