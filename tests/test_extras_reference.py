"""CPU tests of the optional outputs' definitions (include/ofdg.h, ofdg_extras): the numpy restatement in
extras_reference.py is pinned to the oracle - its forward flow, rebuilt from its own frame-0 labels and the motions of
host_realize, is the oracle's flow bit for bit - and the C-ABI declares and exports the entry points."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import extras_reference as xr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def batch(oracle, mode, W, H, B, seed=3):
    tasks, bps, n = oracle.Sampler(mode, W, H).next(B)
    pool = np.random.default_rng(seed).integers(0, 256, (3, 3, 2 * H, 2 * W), dtype=np.uint8)
    return tasks, bps, n, pool


@pytest.mark.parametrize("W,H", [(128, 96), (160, 100)])
@pytest.mark.parametrize("mode", [1, 2, 3, 5, 7, 13])
def test_helper_forward_flow_is_the_oracles(ofdg, oracle, mode, W, H):
    B = 2
    tasks, bps, n, pool = batch(oracle, mode, W, H, B)
    q = oracle.default_params(W, H, mode)
    ref = xr.reference_extras(ofdg, oracle, q, tasks, B, bps, n, pool)
    _, _, ef = oracle.render(q, tasks, B, bps, n, pool)
    assert np.array_equal(ref["flow"].view(np.int32), ef.view(np.int32)), "%d px differ" % (ref["flow"] != ef).sum()
    # the definitions hold together: objects are present in both frames, occlusion is neither empty nor everything
    assert ref["label0"].max() >= 1 and ref["label1"].max() >= 1
    for k in ("occ0", "occ1"):
        assert set(np.unique(ref[k])) <= {0.0, 1.0}
        assert 0.0 < ref[k].mean() < 0.9
    assert np.isfinite(ref["flow1"]).all()


def test_helper_forward_flow_is_the_oracles_full_size(ofdg, oracle):
    tasks, bps, n, pool = batch(oracle, 7, 512, 384, 1)
    q = oracle.default_params(512, 384, 7)
    ref = xr.reference_extras(ofdg, oracle, q, tasks, 1, bps, n, pool)
    _, _, ef = oracle.render(q, tasks, 1, bps, n, pool)
    assert np.array_equal(ref["flow"].view(np.int32), ef.view(np.int32))


def test_backward_flow_inverts_the_motion(ofdg, oracle):
    """Where a pixel keeps its owner, flow1 at the forward-mapped point undoes the forward flow up to the rounding of the
    target to a pixel: |flow0(p) + flow1(round(p + flow0(p)))| <= (1 + |M^-1|) sqrt(2)/2 with |M^-1| <= the largest
    inverse scale of the sampled motions (< 4 for these modes)."""
    tasks, bps, n, pool = batch(oracle, 5, 160, 100, 2)
    ref = xr.reference_extras(ofdg, oracle, oracle.default_params(160, 100, 5), tasks, 2, bps, n, pool)
    H, W = 100, 160
    ys, xs = np.mgrid[0:H, 0:W]
    for s in range(2):
        f0, f1, occ = ref["flow"][s], ref["flow1"][s], ref["occ0"][s, 0]
        xr_ = np.floor(xs.astype(np.float32) + f0[0] + np.float32(0.5)).astype(np.int64)
        yr_ = np.floor(ys.astype(np.float32) + f0[1] + np.float32(0.5)).astype(np.int64)
        vis = occ == 0
        e = np.hypot(f0[0][vis] + f1[0][yr_[vis], xr_[vis]], f0[1][vis] + f1[1][yr_[vis], xr_[vis]])
        assert e.max() <= (1 + 4) * np.sqrt(2) / 2


def test_header_declares_the_extras_entry_points(ofdg):
    hdr = open(os.path.join(ROOT, "include", "ofdg.h")).read()
    for name in ("ofdg_render_ex", "ofdg_forward_ex", "ofdg_forward_counter_ex"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in ofdg.EXPORTS
        assert hasattr(ofdg.lib(), name)
    m = re.search(r"typedef struct ofdg_extras \{(.*?)\} ofdg_extras;", hdr, re.S)
    assert [f for f in re.findall(r"\*\s*(\w+);", m.group(1))] == [n for n, _ in ofdg.Extras._fields_]
    assert C.sizeof(ofdg.Extras) == 5 * 8


def test_alloc_extras_shapes_and_names(ofdg):
    torch = pytest.importorskip("torch")
    ex = ofdg.alloc_extras(3, 96, 128, device="cpu")
    assert ex["flow1"].shape == (3, 2, 96, 128) and ex["flow1"].dtype == torch.float32
    assert ex["occ0"].shape == ex["occ1"].shape == (3, 1, 96, 128)
    assert ex["label0"].shape == ex["label1"].shape == (3, 96, 128) and ex["label0"].dtype == torch.uint8
    assert set(ofdg.alloc_extras(1, 8, 8, names=("occ1",), device="cpu")) == {"occ1"}
    with pytest.raises(ValueError):
        ofdg.alloc_extras(1, 8, 8, names=("flow2",), device="cpu")
