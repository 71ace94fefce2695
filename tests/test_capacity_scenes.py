"""The inputs of tests/test_gpu_capacity.py, checked on the oracle alone (no GPU): each scene of capacity_scenes.py and each
sampler-drawn batch reaches what it is there to reach - painter's positions above 32 that own pixels, tiles that show all 65
positions, deforming objects in the upper half, an eighth component that changes the picture."""
import numpy as np
import pytest

import capacity_scenes as cs
import extras_reference as xr


def pool(W, H):
    """(labels read no texel: any pool of the right shape does)"""
    return np.random.default_rng(0).integers(0, 256, (3, 3, 2 * H, 2 * W), dtype=np.uint8)


def labels(oracle, W, H, mode, task, bps):
    return xr.labels_of(oracle, oracle.default_params(W, H, mode), task, bps, pool(W, H))[:2]


@pytest.mark.parametrize("W,H,mode,aa,B", cs.DRAWN, ids=["%dx%d-mode%d-aa%d" % c[:4] for c in cs.DRAWN])
def test_drawn_batches_reach_the_upper_half(oracle, W, H, mode, aa, B):
    tasks, bps, n = oracle.Sampler(mode, W, H, 64).next(B, cap=B * 1024)
    high = [set(), set()]
    for s in range(B):
        if s == B - 1 and B > 1:
            assert min(len(h) for h in high) < 8  # (a smaller batch would not do)
        for f, l in enumerate(labels(oracle, W, H, mode, tasks[s], bps)):
            high[f] |= cs.high_positions(l)
    assert min(len(h) for h in high) >= 8, [len(h) for h in high]
    assert max(bps[i].n_components for i in range(n)) == (7 if mode == 7 else 0)


@pytest.mark.parametrize("W,H,name", cs.STACKS, ids=["%dx%d-%s" % c for c in cs.STACKS])
def test_stacks_show_every_position_and_fill_a_tile(oracle, W, H, name):
    tasks, bps, n = getattr(cs, name)(oracle.Sampler, W, H)
    l0, l1 = labels(oracle, W, H, 5, tasks[0], bps)
    assert cs.positions(l0) == cs.positions(l1) == set(range(65))
    if (W, H, name) == (160, 100, "stack"):
        assert not cs.full_tiles(l0) and cs.richest_tile(l0, l1) >= 55
    else:
        assert len(cs.full_tiles(l0)) == 4 and cs.richest_tile(l0, l1) == 65


@pytest.mark.parametrize("W,H", cs.SIZES)
def test_grids_show_the_positions_they_are_named_for(oracle, W, H):
    want = {"grid": set(range(65)), "grid_upper_half": set(range(33)), "grid_low_offscreen": {0} | set(range(33, 65))}
    for name in cs.GRIDS:
        tasks, bps, n = getattr(cs, name)(oracle.Sampler, W, H)
        l0, l1 = labels(oracle, W, H, 5, tasks[0], bps)
        assert cs.positions(l0) == cs.positions(l1) == want[name], name
        assert cs.richest_tile(l0, l1) <= 17, name  # (sparse masks: 4 x 2 objects of the grid and their neighbours' rims)
    tasks, bps, n = cs.many_ellipses(oracle.Sampler, W, H, 64)
    assert all(cs.positions(l) == set(range(65)) for l in labels(oracle, W, H, 5, tasks[0], bps))


def test_mode9_batches_deform_objects_of_the_upper_half(oracle):
    for W, H in cs.SIZES:
        tasks, bps, n = oracle.Sampler(9, W, H, 64).next(cs.MODE9_B, cap=cs.MODE9_B * 1024)
        assert cs.deforming_high(tasks, bps) >= 6


def test_the_oracle_sorts_by_id(oracle):
    W, H = 128, 96
    tasks, bps, n = cs.stack(oracle.Sampler, W, H)
    pt, pb, pn = cs.permuted(tasks, bps, n)
    a = oracle.render(oracle.default_params(W, H, 5), tasks, 1, bps, n, pool(W, H))
    b = oracle.render(oracle.default_params(W, H, 5), pt, 1, pb, pn, pool(W, H))
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


@pytest.mark.parametrize("W,H", cs.SIZES)
def test_the_eighth_component_matters(ofdg, oracle, W, H):
    """The eighth component is a copy of component 3 (a subtracted satellite), moved and made additive: bit 7 of the composite's
    additive word is 1 where bit 3 is 0, and the composite's own pixels change in both frames."""
    tasks, bps, n, oi = cs.seven_component_composite(oracle.Sampler, W, H)
    pos = tasks[0].n_objects
    assert pos == 54
    l0, l1 = labels(oracle, W, H, 7, tasks[0], bps)
    assert (l0 == pos).sum() > 1000 and (l1 == pos).sum() > 1000
    t8, b8, n8 = cs.with_component_added(tasks, 1, bps, n, oi, source=3)
    run = b8[oi]
    assert run.n_components == 8 and [b8[run.first_component + k].is_additive_component for k in (3, 7)] == [0, 1]
    m0, m1 = labels(oracle, W, H, 7, t8[0], b8)
    print("pixels of the composite that the eighth component changes: %d / %d" % ((l0 != m0).sum(), (l1 != m1).sum()))
    assert (l0 != m0).sum() >= 8 and (l1 != m1).sum() >= 8
    # every other blueprint the task reaches is the one it reached before
    sm7, om7 = ofdg.host_realize(ofdg.default_params(width=W, height=H, mode=7), 3, 2 * W, 2 * H, tasks, 1, bps, n)
    sm8, om8 = ofdg.host_realize(ofdg.default_params(width=W, height=H, mode=7), 3, 2 * W, 2 * H, t8, 1, b8, n8)
    assert np.array_equal(om7, om8) and len(sm8) == len(sm7) + 1 and np.array_equal(sm7, sm8[:-1])
