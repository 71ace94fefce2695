"""GPU tests at the capacity limits the render front end is built around: 64 foreground objects per sample (kMaxFgObjects: the
64-bit tile masks of geom / raster / compose, DevSample::shape_of[64], labels 0..64, the 65 rows of the object table) and 8
components per composite (kMaxComponents: DevObject::additive).  The bars are those of test_gpu_parity.py and
test_gpu_extras.py: frames byte-equal to the oracle, flow and flow1 at 0 ULP, labels and occlusion equal, the NaN pattern
equal in mode 9.  Sampler-drawn samples of 64 objects show few of them (later objects hide earlier ones), so besides them
the scenes of capacity_scenes.py are rendered, in which every painter's position owns pixels; the conditions the inputs must
meet are asserted on the reference (and, without a GPU, by tests/test_capacity_scenes.py)."""
import ctypes as C

import numpy as np
import pytest

import capacity_scenes as cs
import extras_reference as xr
import test_gpu_extras_formats as xf
import test_gpu_object_table as tot
from test_gpu_extras import check_against_helper, make_gen, run
from test_gpu_parity import nan_equal_ulp, params_for_oracle, render_gpu

pytestmark = pytest.mark.gpu

SIZES = cs.SIZES
_pools, _refs = {}, {}


def pool_of(g):
    """The generator's texture pool on the host (make_gen: pool_synthetic(3, 2W, 2H, 11), the same for every context of a size)."""
    key = (g.params.width, g.params.height)
    if key not in _pools:
        _pools[key] = g.pool_download_all()
    return _pools[key]


def reference(ofdg, oracle, key, g, mode, tasks, B, bps, n, aa=1):
    """The oracle's frames and flow and the restated optional outputs of a batch, computed once per `key` and left unchanged."""
    W, H = g.params.width, g.params.height
    key = (key, W, H, mode, aa)
    if key not in _refs:
        q = oracle.default_params(W, H, mode, aa)
        ref = xr.reference_extras(ofdg, oracle, q, tasks, B, bps, n, pool_of(g))
        ref["image0"], ref["image1"], ref["oracle_flow"] = oracle.render(q, tasks, B, bps, n, pool_of(g))
        for v in ref.values():
            v.setflags(write=False)
        _refs[key] = ref
    return _refs[key]


def check_render(got, ref):
    """(outs, extras) of run() against reference(): every bar of the module's docstring."""
    (i0, i1, fl), ex = got
    assert np.array_equal(i0, ref["image0"]), "image0 differs: %d values" % (i0 != ref["image0"]).sum()
    assert np.array_equal(i1, ref["image1"]), "image1 differs: %d values" % (i1 != ref["image1"]).sum()
    d = xr.ulp_diff(fl, ref["oracle_flow"])
    assert d.max() == 0, "flow differs by up to %d ULP at %d px" % (d.max(), (d > 0).sum())
    assert np.array_equal(ref["flow"].view(np.int32), ref["oracle_flow"].view(np.int32))  # (the restatement is the oracle's)
    check_against_helper(ex, ref, flow1_ulp=0)
    for k in ("occ0", "occ1"):
        assert np.array_equal(ex[k], ref[k]), "%s differs at %d px" % (k, (ex[k] != ref[k]).sum())


def high_positions_of_batch(ref):
    """Per frame: the painter's positions above 32 that own pixels in some sample of the batch."""
    return [set().union(*(cs.high_positions(l) for l in ref[k])) for k in ("label0", "label1")]


# ---- a. sampler-drawn samples of 64 objects ------------------------------------------------------------------------------
# (the cases and why their batch sizes are what they are: capacity_scenes.DRAWN)
@pytest.mark.parametrize("W,H,mode,aa,B", cs.DRAWN, ids=["%dx%d-mode%d-aa%d" % c[:4] for c in cs.DRAWN])
def test_sampler_drawn_samples_of_64_objects(ofdg, oracle, W, H, mode, aa, B):
    g = make_gen(ofdg, W, H, mode, use_antialiasing=aa, num_objects=64)
    tasks, bps, n = oracle.Sampler(mode, W, H, 64).next(B, cap=B * 1024)
    assert all(t.n_objects == 64 for t in tasks)
    ref = reference(ofdg, oracle, "drawn%d" % B, g, mode, tasks, B, bps, n, aa)
    high = high_positions_of_batch(ref)
    print("positions above 32 that own pixels, frame 0 / 1: %d / %d" % (len(high[0]), len(high[1])))
    assert min(len(h) for h in high) >= 8, "the batch does not reach the upper half of the masks often enough"
    check_render(run(ofdg, g, tasks, B, bps, n), ref)


# ---- b. the full mask ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,name", cs.STACKS, ids=["%dx%d-%s" % c for c in cs.STACKS])
def test_full_tile_masks_every_form(ofdg, oracle, W, H, name):
    g = make_gen(ofdg, W, H, 5, num_objects=64)
    tasks, bps, n = getattr(cs, name)(oracle.Sampler, W, H)
    ref = reference(ofdg, oracle, name, g, 5, tasks, 1, bps, n)
    for k in ("label0", "label1"):
        assert cs.positions(ref[k][0]) == set(range(65)), "%s: not every painter's position owns pixels" % k
    if (W, H, name) != (160, 100, "stack"):
        assert len(cs.full_tiles(ref["label0"][0])) >= 1, "no tile holds all 65 positions"
    else:
        assert cs.richest_tile(ref["label0"][0], ref["label1"][0]) >= 55
    got = run(ofdg, g, tasks, 1, bps, n)
    check_render(got, ref)
    # every compact form against the float call (test_gpu_extras_formats.py)
    for form in xf.FORMS:
        xf.check_form(got, xf.render(ofdg, g, tasks, 1, bps, n, form), form, "%s %dx%d %s" % (name, W, H, "/".join(form)))


# ---- c. sparse high bits ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cs.GRIDS)
@pytest.mark.parametrize("W,H", SIZES)
def test_sparse_high_bits(ofdg, oracle, W, H, name):
    g = make_gen(ofdg, W, H, 5, num_objects=64)
    tasks, bps, n = getattr(cs, name)(oracle.Sampler, W, H)
    ref = reference(ofdg, oracle, name, g, 5, tasks, 1, bps, n)
    want = {"grid": set(range(65)), "grid_upper_half": set(range(33)), "grid_low_offscreen": {0} | set(range(33, 65))}[name]
    for k in ("label0", "label1"):
        assert cs.positions(ref[k][0]) == want, k
    check_render(run(ofdg, g, tasks, 1, bps, n), ref)


# ---- d. per-shape coverage with well over a hundred outlines -------------------------------------------------------------
def test_shape_coverage_of_a_64_object_sample(ofdg, oracle):
    W, H = 128, 96
    g = make_gen(ofdg, W, H, 7, num_objects=64)
    tasks, bps, n = oracle.Sampler(7, W, H, 64).next(1, cap=1024)
    render_gpu(ofdg, g, tasks, 1, bps, n)
    _, _, aa = oracle.tables()
    masks = oracle.shape_masks(params_for_oracle(oracle, g.params), tasks[0], bps, pool_of(g), max_shapes=512)
    assert len(masks) > 128 and g.debug_num_shapes(0) == len(masks)
    for k in range(len(masks)):
        for fr in range(2):
            cov = g.debug_coverage(0, k, fr)
            assert np.array_equal(aa[cov], masks[k][fr]), (k, fr)
            assert np.array_equal(np.where(cov >= 128, 255, 0).astype(np.uint8), masks[k][2 + fr]), (k, fr)


# ---- e. the object table with all 65 rows --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("stack", "grid"))
@pytest.mark.parametrize("W,H", SIZES)
def test_object_table_with_65_rows(ofdg, oracle, W, H, name):
    g = make_gen(ofdg, W, H, 5, num_objects=64)
    tasks, bps, n = getattr(cs, name)(oracle.Sampler, W, H)
    ref = reference(ofdg, oracle, name, g, 5, tasks, 1, bps, n)
    raw, counts, labels = tot.render_and_tabulate(ofdg, g, tasks, 1, bps, n)
    assert list(counts) == [65] and ofdg.MAX_OBJECT_ROWS == 65
    for k in ("label0", "label1"):
        assert np.array_equal(labels[k], ref[k]), k
    tot.check_batch(ofdg, raw, counts, tot.expected(ofdg, oracle, W, H, 5, tasks, 1, bps, n), H, W)
    rows = ofdg.object_table_numpy(raw, counts)[0]
    assert len(rows) == 65 and list(rows["obj_id"][1:]) == list(range(10, 74))
    assert (rows["area0"][33:] > 0).all() and (rows["area1"][33:] > 0).all()


# ---- f. mode 9 at 64 objects -----------------------------------------------------------------------------------------------
# B = 2: of the first two samples of Sampler(9, W, H, 64), 5 + 4 foreground objects with a local index of 32 or more deform
# (10 + 10 in all), at both sizes (the blueprints' flags do not depend on the frame size).
@pytest.mark.parametrize("W,H", SIZES)
def test_mode9_with_64_objects(ofdg, oracle, W, H):
    B = cs.MODE9_B
    crops = oracle.warp_crops(W, H, seed=5)[::5][:6] * 4.0
    g = make_gen(ofdg, W, H, 9, num_objects=64)
    g.warp_upload(crops)
    tasks, bps, n = oracle.Sampler(9, W, H, 64).next(B, cap=B * 1024)
    high = cs.deforming_high(tasks, bps)
    print("deforming foreground objects with a local index >= 32: %d" % high)
    assert all(t.n_objects == 64 for t in tasks) and high >= 6
    got = render_gpu(ofdg, g, tasks, B, bps, n)
    e0, e1, ef = oracle.render(oracle.default_params(W, H, 9), tasks, B, bps, n, pool_of(g), warp_crops=crops, reuse=2)
    assert np.array_equal(got[0], e0), "image0 differs at %d values" % (got[0] != e0).sum()
    assert np.array_equal(got[1], e1), "image1 differs at %d values" % (got[1] != e1).sum()
    assert nan_equal_ulp(got[2], ef) == 0


# ---- g. eight components -----------------------------------------------------------------------------------------------------
def guarded_refusal(ofdg, g, tasks, B, bps, n, code, text):
    """A render call that must be refused: the error, nothing enqueued, the outputs keep their fill, the context stays usable."""
    import torch
    W, H = g.params.width, g.params.height
    outs, ex = xf.alloc(ofdg, B, H, W, ("f32", "f32", "f32"))
    ticket = g.last_ticket()
    with pytest.raises(ofdg.OfdgError) as e:
        g.render(tasks, B, bps, n, *outs, extras=ex)
    assert e.value.code == code and text in str(e.value), str(e.value)
    assert g.last_ticket() == ticket
    g.synchronize()
    torch.cuda.synchronize()
    for t in list(outs) + list(ex.values()):
        assert bool((t.view(torch.uint8) == xf.SENTINEL).all()), "an output of a refused call was written"


@pytest.mark.parametrize("W,H", SIZES)
def test_eight_components_and_a_ninth(ofdg, oracle, W, H):
    """A composite of 7 components at painter's position 54, cut free of what the sampler drew on top of it, with an eighth
    appended: a copy of its component 3 (a subtracted satellite), moved and made additive - bit 7 of DevObject::additive is 1
    where bit 3 is 0.  A ninth is refused."""
    g = make_gen(ofdg, W, H, 7, num_objects=64)
    tasks, bps, n, oi = cs.seven_component_composite(oracle.Sampler, W, H)
    ref7 = reference(ofdg, oracle, "seven", g, 7, tasks, 1, bps, n)
    pos = tasks[0].n_objects
    assert pos == 54 and (ref7["label0"][0] == pos).sum() > 1000 and (ref7["label1"][0] == pos).sum() > 1000
    t8, b8, n8 = cs.with_component_added(tasks, 1, bps, n, oi, source=3)
    assert b8[oi].n_components == 8 and [b8[b8[oi].first_component + k].is_additive_component for k in (3, 7)] == [0, 1]
    ref8 = reference(ofdg, oracle, "eight", g, 7, t8, 1, b8, n8)
    for k in ("image0", "image1", "label0", "label1"):
        assert not np.array_equal(ref7[k], ref8[k]), "%s: the eighth component changes nothing" % k
    check_render(run(ofdg, g, tasks, 1, bps, n), ref7)
    check_render(run(ofdg, g, t8, 1, b8, n8), ref8)
    t9, b9, n9 = cs.with_component_added(t8, 1, b8, n8, oi, source=0)
    assert b9[oi].n_components == 9
    guarded_refusal(ofdg, g, t9, 1, b9, n9, ofdg.ECAPACITY, "component range outside [1, 8]")
    check_render(run(ofdg, g, t8, 1, b8, n8), ref8)


# ---- h. 64 and 65 ------------------------------------------------------------------------------------------------------------
def test_65_objects_are_refused_and_64_rendered(ofdg, oracle):
    W, H = 128, 96
    g = make_gen(ofdg, W, H, 5, num_objects=64)
    tasks, bps, n = cs.many_ellipses(oracle.Sampler, W, H, 65)
    assert tasks[0].n_objects == 65 and tasks[0].first_object + 65 == n
    guarded_refusal(ofdg, g, tasks, 1, bps, n, ofdg.ECAPACITY, "more than 64")
    tasks[0].n_objects = 64
    ref = reference(ofdg, oracle, "many64", g, 5, tasks, 1, bps, n)
    assert cs.positions(ref["label0"][0]) == set(range(65))
    check_render(run(ofdg, g, tasks, 1, bps, n), ref)


# ---- i. order and identity of ids ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", SIZES)
def test_blueprint_order_is_free(ofdg, oracle, W, H):
    g = make_gen(ofdg, W, H, 5, num_objects=64)
    tasks, bps, n = cs.stack(oracle.Sampler, W, H)
    ref = reference(ofdg, oracle, "stack", g, 5, tasks, 1, bps, n)
    pt, pb, pn = cs.permuted(tasks, bps, n)
    ids = [pb[pt[0].first_object + k].obj_id for k in range(64)]
    assert sorted(ids) == list(range(10, 74)) and ids != sorted(ids)
    e = oracle.render(oracle.default_params(W, H, 5), pt, 1, pb, pn, pool_of(g))  # (the oracle's std::map sorts by id)
    assert all(np.array_equal(a, ref[k]) for a, k in zip(e, ("image0", "image1", "oracle_flow")))
    sorted_run = run(ofdg, g, tasks, 1, bps, n)
    permuted_run = run(ofdg, g, pt, 1, pb, pn)
    check_render(permuted_run, ref)
    for a, b in zip(sorted_run[0], permuted_run[0]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for k in sorted_run[1]:
        assert np.array_equal(sorted_run[1][k].view(np.uint8), permuted_run[1][k].view(np.uint8)), k
    raw_s, counts_s, _ = tot.render_and_tabulate(ofdg, g, tasks, 1, bps, n)
    raw_p, counts_p, _ = tot.render_and_tabulate(ofdg, g, pt, 1, pb, pn)
    assert np.array_equal(raw_s, raw_p) and list(counts_p) == [65]
    assert list(ofdg.object_table_numpy(raw_p, counts_p)[0]["obj_id"][1:]) == list(range(10, 74))


def test_duplicate_ids_are_refused(ofdg, oracle):
    """Two foreground blueprints of a task with one obj_id: the reference keeps the last (objects_map[ID] = ..., DG:1210), which
    would shift every later label and table row by one; the library refuses the task and names the id."""
    W, H = 128, 96
    g = make_gen(ofdg, W, H, 5, num_objects=64)
    tasks, bps, n = cs.grid(oracle.Sampler, W, H)
    ref = reference(ofdg, oracle, "grid", g, 5, tasks, 1, bps, n)
    dup = cs.clone(bps, n)
    dup[tasks[0].first_object + 5].obj_id = dup[tasks[0].first_object + 40].obj_id
    guarded_refusal(ofdg, g, tasks, 1, dup, n, ofdg.EINVAL, "object id 50 appears more than once in task 0")
    check_render(run(ofdg, g, tasks, 1, bps, n), ref)
