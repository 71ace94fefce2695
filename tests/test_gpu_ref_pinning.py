"""GPU tests against the REFERENCE's own compiled code (fixtures tests/golden/ref_*, see tests/test_ref_pinning.py):
the device's warp-field generation, the motions of the object table and the flow of every pixel are compared with what
the reference's WarpFields.cpp / DataGenerator.cpp computed - not with the oracle, which only restates them.

Bars: warp crops bit-equal (NaNs canonical: the reference writes signalling NaNs); motions equal as fp64 bit patterns;
forward and backward flow 0 ULP, the bar of every host-affine comparison of tests/test_gpu_parity.py and of the backward
flow in tests/test_gpu_extras.py.
"""
import os

import numpy as np
import pytest

import extras_reference as xr
import ref_stream as rs

pytestmark = pytest.mark.gpu


def make_gen(ofdg, W, H, mode):
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    g = ofdg.Generator(ofdg.default_params(width=W, height=H, mode=mode))
    g.pool_synthetic(3, 2 * W, 2 * H, 11)
    return g


# ---- warp fields ------------------------------------------------------------------------------------------------------
def where_crop_differs(crop, origin, strided):
    """Text for an assertion: the texels of a crop that lie on the fixture's every-8th-texel copy of the big field and
    differ from it."""
    x0, y0 = origin
    _, h, w = crop.shape
    ys = np.array([y for y in range(h) if (y0 + y) % rs.STRIDE == 0])
    xs = np.array([x for x in range(w) if (x0 + x) % rs.STRIDE == 0])
    got = rs.canon_bits(crop[:, ys][:, :, xs])
    ref = rs.canon_bits(strided[:, (y0 + ys) // rs.STRIDE][:, :, (x0 + xs) // rs.STRIDE])
    d = np.argwhere(got != ref)
    if not len(d):
        return "the every-%dth-texel copy agrees: the difference lies between its texels" % rs.STRIDE
    p, j, i = d[0]
    return "%d of %d sampled texels differ; first: plane %d, field texel (%d, %d): got %r, reference %r" % (
        len(d), got.size, p, x0 + xs[i], y0 + ys[j], crop[p, ys[j], xs[i]], strided[p, (y0 + ys[j]) // rs.STRIDE, (x0 + xs[i]) // rs.STRIDE])


@pytest.mark.parametrize("name", sorted(rs.WARP_SETS))
def test_device_warp_fields_equal_the_compiled_reference(ofdg, name):
    """warp_generate(1, seed): displacer placement, elementary fields, 17 composition passes, NaN flags, clamp and crop
    loop of the DEVICE against the crops of the field the reference's WarpFields.cpp made of the same displacers (built
    with expf = ofdg_det_expf).  128 x 96 and 256 x 192 are the smallest frames whose 3 * max(W, H) field holds
    displacers at all; the second holds all three displacer types."""
    m = rs.load_json("ref_warpfields.json")[name]
    W, H, seed = rs.WARP_SETS[name]
    assert (m["width"], m["height"], m["seed"]) == (W, H, seed)
    strided = np.load(os.path.join(rs.GOLD, "ref_warpfields.npz"))[name + "_strided"]
    g = make_gen(ofdg, W, H, 9)
    g.warp_generate(1, seed)
    assert g.warp_count() == len(m["crop_digests"]) == len(m["crop_origins"])
    strongest = 0.0
    for k, want in enumerate(m["crop_digests"]):
        crop = g.warp_download(k)
        assert crop.shape == (4, H + 1, W + 1)
        strongest = max(strongest, float(np.nanmax(np.abs(crop))))
        assert rs.field_digest(crop) == want, "crop %d at %s: %s" % (k, m["crop_origins"][k], where_crop_differs(crop, m["crop_origins"][k], strided))
    assert strongest > 1.0   # (the flagged texels of these fields lie on their rim, outside every crop; the crops do move)


# ---- motions and flow -------------------------------------------------------------------------------------------------
class Scene:
    """Two samples of a mode at the reference's frame (DGEN_WIDTH x DGEN_HEIGHT = 512 x 384 enters addBackgroundMotion),
    blueprints from the host reference-stream sampler, rendered once with labels, backward flow and the object table."""

    def __init__(self, ofdg, mode):
        import torch
        self.fx = rs.load_json("ref_motion_mode%d.json" % mode)
        W, H, B = self.fx["width"], self.fx["height"], len(self.fx["tasks"])
        assert (W, H, B) == (512, 384, 2)
        g = make_gen(ofdg, W, H, mode)
        tasks, bps, n = g.sample(B)
        # the tasks rendered ARE the fixture's: their digests are the first of the reference's stream
        want = rs.load_json("ref_sampler_streams.json")["modes"][str(mode)]["task_digests"][:B]
        assert [rs.task_digest(rs.task_bytes(tasks, bps, t)) for t in range(B)] == want
        outs = ofdg.alloc_outputs(B, H, W)
        ex = ofdg.alloc_extras(B, H, W, ("flow1", "label0", "label1"))
        rows, counts = ofdg.alloc_object_table(B)
        outs[2].fill_(-12345)
        ex["flow1"].fill_(-12345)
        g.render(tasks, B, bps, n, *outs, extras=ex)
        g.object_table(ex["label0"], ex["label1"], rows, counts)
        g.synchronize()
        torch.cuda.synchronize()
        self.W, self.H, self.B = W, H, B
        self.flow = outs[2].cpu().numpy()
        self.extras = {k: t.cpu().numpy() for k, t in ex.items()}
        self.table = ofdg.object_table_numpy(rows, counts)
        self.counts = counts.cpu().numpy()


@pytest.fixture(scope="module", params=[5, 7])
def scene(request, ofdg):
    return Scene(ofdg, request.param)


def test_object_table_motions_equal_the_compiled_reference(scene):
    """Every row's motion[6] is the m_motion the reference's setMotion (+ addBackgroundMotion for foreground objects)
    computed for that object, as fp64 bits; ids and types are the reference's too."""
    types = set()
    for s, objs in enumerate(scene.fx["tasks"]):
        rows = scene.table[s]
        assert int(scene.counts[s]) == len(rows) == len(objs)
        assert list(rows["obj_id"]) == [o["obj_id"] for o in objs]
        assert list(rows["obj_type"]) == [o["obj_type"] for o in objs]
        ref = np.stack([rs.hex_f64(o["m_motion"]) for o in objs])
        bad = np.argwhere(rs.bits64(rows["motion"]) != rs.bits64(ref))
        assert not len(bad), "sample %d: row %d member %d: got %r, reference %r" % (
            s, bad[0][0], bad[0][1], rows["motion"][bad[0][0]][bad[0][1]], ref[bad[0][0]][bad[0][1]])
        types.update(o["obj_type"] for o in objs)
    assert {1, 2} <= types


@pytest.mark.parametrize("frame", ["forward", "backward"])
def test_flow_of_every_pixel_equals_the_reference_point_flow(scene, frame):
    """For every pixel: the owner from the GPU's own label plane (ownership is pinned through the AGG goldens), the flow
    from getPointFlow's formula (extras_reference.point_flow_*; tests/test_ref_pinning.py proves it reproduces the
    reference's recorded samples) on the FIXTURE's matrix of that owner - m_motion on label0 for the forward flow,
    m_motion_inv on label1 for the backward flow.  0 ULP."""
    got_all, labels, key = ((scene.flow, scene.extras["label0"], "m_motion") if frame == "forward"
                            else (scene.extras["flow1"], scene.extras["label1"], "m_motion_inv"))
    ys, xs = np.mgrid[0:scene.H, 0:scene.W]
    for s, objs in enumerate(scene.fx["tasks"]):
        lab = labels[s]
        owners = np.unique(lab)
        assert owners.max() < len(objs)
        # not an empty scene: the background and at least three distinct foreground objects own pixels
        assert owners[0] == 0 and len(owners) >= 4, owners
        want = np.full((2, scene.H, scene.W), np.nan, np.float32)
        for k in owners:
            sel = lab == k
            m = tuple(rs.hex_f64(objs[k][key]))
            u, v = xr.point_flow_bg(m, scene.W, scene.H, xs[sel], ys[sel]) if k == 0 else xr.point_flow_fg(m, xs[sel], ys[sel])
            want[0][sel], want[1][sel] = u, v
        assert not np.isnan(want).any()
        print("%s flow, sample %d: %d owners, max ULP distance %d" % (frame, s, len(owners), xr.ulp_diff(got_all[s], want).max()))
        d = xr.ulp_diff(got_all[s], want)
        assert d.max() == 0, "sample %d: %d px differ, by up to %d ULP; owners of those: %s" % (
            s, (d.max(0) > 0).sum(), d.max(), np.unique(lab[d.max(0) > 0]))
