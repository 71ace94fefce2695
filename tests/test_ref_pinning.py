"""CPU tests that pin the oracle AND the product's host code to the REFERENCE's own compiled code (no GPU needed).

Every other parity test compares the HIP path with oracle/, our restatement of the reference written by reading it: a
wrong draw order, a swapped operand in the warp composition or a wrong multiplication order in addBackgroundMotion
would be copied into oracle, host code and kernels alike and nothing would notice.  The fixtures tests/golden/ref_*
were written by the reference's WarpFields.cpp and DataGenerator.cpp themselves, compiled against container shells of
AGG / CImg (oracle/ref_shell, oracle/ref_*_harness.cpp; generator: tests/golden/gen_ref_goldens.py):

  sampler     ObjectParametersGenerator driven like load_batch: 13 modes x 200 tasks, every blueprint member
  warp field  supports, displacers, DisplacementComposer, 17 composition passes, NaN flags, clamp_near_zeros -
              built with expf defined as ofdg_det_expf, i.e. in the arithmetic of oracle.detmath() and of the device
  motion      setIntrinsicTransform / setMotion / addBackgroundMotion / getPointFlow of modes 5 and 7

The fixture tests never skip.  One test runs the reference binaries live (libm build against the oracle's default
arithmetic) and skips where oracle/_ref/ does not exist.
"""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import extras_reference as xr
import ref_stream as rs


@pytest.fixture(scope="module")
def streams():
    return rs.load_json("ref_sampler_streams.json")


@pytest.fixture(scope="module")
def full_tasks():
    return np.load(os.path.join(rs.GOLD, "ref_sampler_tasks.npz"))


@pytest.fixture(scope="module")
def warp_meta():
    return rs.load_json("ref_warpfields.json")


@pytest.fixture(scope="module")
def warp_arrays():
    return np.load(os.path.join(rs.GOLD, "ref_warpfields.npz"))


# ---- sampler ---------------------------------------------------------------------------------------------------------
def check_stream(got, mode, streams, full_tasks, who):
    want = streams["modes"][str(mode)]
    for k in range(rs.N_FULL):  # the first tasks are stored in full: a failure names the member
        ref = full_tasks["m%d_t%d" % (mode, k)].tobytes()
        assert got[k] == ref, "%s, mode %d, task %d: %s" % (who, mode, k, rs.first_difference(got[k], ref))
    digests = [rs.task_digest(b) for b in got]
    bad = [t for t, (a, b) in enumerate(zip(digests, want["task_digests"])) if a != b]
    assert not bad, "%s, mode %d: task %d is the first of %d that differ from the reference's stream" % (who, mode, bad[0], len(bad))
    whole = b"".join(got)
    assert len(got) == streams["n_tasks"] == len(want["task_digests"])
    assert (len(whole), hashlib.sha256(whole).hexdigest()) == (want["n_bytes"], want["sha256"]), (who, mode)


@pytest.mark.parametrize("mode", rs.MODES)
def test_sampler_streams_equal_the_compiled_reference(ofdg, oracle, streams, full_tasks, mode):
    """The oracle's sampler and the product's HostSampler, serialised like the reference harness serialises its
    ObjectBlueprints, give the reference's stream: 200 tasks, every member as int32 / float32 bits, digest for digest."""
    check_stream(rs.sampler_task_bytes(oracle.Sampler(mode, 512, 384), rs.N_TASKS), mode, streams, full_tasks, "oracle.Sampler")
    check_stream(rs.sampler_task_bytes(ofdg.HostSampler(mode, 512, 384), rs.N_TASKS), mode, streams, full_tasks, "ofdg.HostSampler")


def test_sampler_fixture_covers_every_branch_kind(full_tasks, streams):
    """The stream the digests are of is not a trivial one: all object types, curved segments, composites with additive
    and subtractive components occur in the tasks stored in full."""
    types, seg_types, additive = set(), set(), set()
    for mode in rs.MODES:
        for k in range(rs.N_FULL):
            for b in rs.parse_task(full_tasks["m%d_t%d" % (mode, k)].tobytes())[1:]:
                types.add(b["obj_type"])
                seg_types.update(s[0] for s in b["segments"])
                for c in b["components"]:
                    additive.add(c["is_additive_component"])
                    seg_types.update(s[0] for s in c["segments"])
    assert types == {1, 2, 3} and seg_types == {0, 1, 3} and additive == {0, 1}
    assert len({m["sha256"] for m in streams["modes"].values()}) >= 11   # (modes 4 / 5 / 8 differ in motion only ...)


# ---- warp fields ------------------------------------------------------------------------------------------------------
def where_fields_differ(got, ref, step=1):
    """Text for an assertion: planes, count and first texel in which two [4, n, n] fields differ (NaNs canonical)."""
    a, b = rs.canon_bits(got), rs.canon_bits(ref)
    d = np.argwhere(a != b)
    if not len(d):
        return "no difference on the compared texels"
    p, y, x = d[0]
    return "%d texels differ (planes %s); first: plane %d at (%d, %d): got %r, reference %r" % (
        len(d), sorted(set(d[:, 0].tolist())), p, x * step, y * step, got[p, y, x], ref[p, y, x])


@pytest.mark.parametrize("name", ["w128_s11", "w256_s3", "hand96"])
def test_oracle_flowfield_equals_the_compiled_reference(oracle, warp_meta, warp_arrays, name):
    """oracle.flowfield under oracle.detmath() on the fixture's displacers against the field the reference's own
    WarpFields.cpp computed with the same exponential: every plane, NaN pattern included; for the seeded sets also
    every (W+1) x (H+1) crop of oracle.warp_crops (the oracle's crop loop against the generator's)."""
    m = warp_meta[name]
    assert m["expf_calls"] > 0   # the fixture IS of the build whose expf is ofdg_det_expf
    disp = warp_arrays[name + "_displacers"]
    assert len(disp) == m["n_displacers"]
    with oracle.detmath():
        flow, iflow = oracle.flowfield(m["size"], disp)
    field = np.concatenate([flow, iflow])
    if name == "hand96":
        ref = warp_arrays["hand96_field"]
        assert np.isnan(ref[:2]).mean() > 0.2 and np.isnan(ref[2:]).mean() > 0.05   # the flagging paths are exercised
        assert np.array_equal(rs.canon_bits(field), rs.canon_bits(ref)), where_fields_differ(field, ref)
    else:
        strided = field[:, ::rs.STRIDE, ::rs.STRIDE]
        assert np.array_equal(rs.canon_bits(strided), rs.canon_bits(warp_arrays[name + "_strided"])), \
            where_fields_differ(strided, warp_arrays[name + "_strided"], rs.STRIDE)
    got = [rs.field_digest(field[k]) for k in range(4)]
    assert got == m["plane_digests"], "planes %s differ from the reference's" % [k for k in range(4) if got[k] != m["plane_digests"][k]]
    if name != "hand96":
        W, H, seed = m["width"], m["height"], m["seed"]
        assert [list(o) for o in rs.crop_origins(W, H)] == m["crop_origins"]
        with oracle.detmath():
            crops = oracle.warp_crops(W, H, seed)
        assert [rs.field_digest(c) for c in crops] == m["crop_digests"]
        assert np.isnan(field).any() and np.abs(np.nan_to_num(field)).max() > 1.0


def test_displacer_lists_of_product_and_oracle_are_the_fixture_s(ofdg, oracle, warp_meta, warp_arrays):
    """The lists the reference's code was run on are what both samplers place for these seeds (a third party to
    test_displacer_placement_equals_oracle), and they hold all three displacer types."""
    kinds = set()
    for name, (W, H, seed) in rs.WARP_SETS.items():
        ref = warp_arrays[name + "_displacers"]
        for got in (oracle.displacers(W, H, seed), ofdg.host_displacers(W, H, seed)):
            assert got.shape == ref.shape and np.array_equal(rs.bits64(got), rs.bits64(ref)), name
        kinds.update(int(t) for t in ref[:, 0])
    assert kinds == {0, 1, 2}
    assert np.array_equal(warp_arrays["hand96_displacers"], rs.HAND_DISPLACERS)


def test_live_libm_reference_field_equals_oracle_default_arithmetic(oracle, warp_arrays, tmp_path):
    """Where oracle/_ref/ exists: the reference's WarpFields.cpp built as is (libm expf) against the oracle in its
    default arithmetic, on the same three sets, bit for bit."""
    binary = os.path.join(rs.REF_BIN, "ref_warpfields")
    if not os.path.exists(binary):
        pytest.skip("oracle/_ref/ref_warpfields is not built (needs the reference checkout)")
    for name, size in (("w128_s11", 384), ("w256_s3", 768), ("hand96", 96)):
        disp = warp_arrays[name + "_displacers"]
        src, dst = str(tmp_path / "d.f64"), str(tmp_path / "f.f32")
        np.ascontiguousarray(disp, "<f8").tofile(src)
        rep = json.loads(subprocess.check_output([binary, str(size), src, dst]))
        assert rep == {"displacers": len(disp), "expf": "libm"}
        ref = np.fromfile(dst, "<f4").reshape(4, size, size)
        flow, iflow = oracle.flowfield(size, disp)
        got = np.concatenate([flow, iflow])
        assert np.array_equal(rs.canon_bits(got), rs.canon_bits(ref)), "%s: %s" % (name, where_fields_differ(got, ref))


# ---- motions ----------------------------------------------------------------------------------------------------------
def motion_fixture(mode):
    return rs.load_json("ref_motion_mode%d.json" % mode)


@pytest.mark.parametrize("mode", [5, 7])
def test_realize_matrices_equal_the_compiled_reference(ofdg, mode):
    """ofdg.host_realize on the HostSampler's first tasks (by the stream test above: the fixture's tasks) against the
    m_motion / m_motion_inv the reference's setMotion + addBackgroundMotion left in its objects, as fp64 bit patterns.
    (ofdg_host_object_table fills areas and boxes only; the table's motions are the device's, tests/test_gpu_ref_pinning.py.)"""
    fx = motion_fixture(mode)
    W, H, n_tasks = fx["width"], fx["height"], len(fx["tasks"])
    assert (W, H) == (512, 384)
    tasks, bps, n = ofdg.HostSampler(mode, W, H).next(n_tasks)
    _, om = ofdg.host_realize(ofdg.default_params(width=W, height=H, mode=mode), 3, 2 * W, 2 * H, tasks, n_tasks, bps, n)
    base, kinds = 0, set()
    for t, objs in enumerate(fx["tasks"]):
        assert len(objs) == 1 + tasks[t].n_objects
        ids = [bps[tasks[t].background].obj_id] + [bps[tasks[t].first_object + k].obj_id for k in range(tasks[t].n_objects)]
        assert [o["obj_id"] for o in objs] == ids == sorted(ids)
        for k, o in enumerate(objs):
            kinds.add(o["obj_type"])
            assert np.array_equal(rs.bits64(om[base + k, 0]), rs.bits64(rs.hex_f64(o["m_motion"]))), (t, k)
            if k:  # (the background's second matrix is its texture warp, not m_motion_inv)
                assert np.array_equal(rs.bits64(om[base + k, 1]), rs.bits64(rs.hex_f64(o["m_motion_inv"]))), (t, k)
            # the suite's numpy statement of trans_affine::invert against the reference's m_motion_inv
            assert np.array_equal(rs.bits64(xr.mat_invert(rs.hex_f64(o["m_motion"]))), rs.bits64(rs.hex_f64(o["m_motion_inv"])))
        base += len(objs)
    assert base == len(om)
    assert kinds == ({0, 1, 2} if mode == 5 else {0, 1, 2, 3})


@pytest.mark.parametrize("mode", [5, 7])
def test_numpy_point_flow_reproduces_every_recorded_getPointFlow(mode):
    """extras_reference.point_flow_fg / point_flow_bg - the per-pixel formula of the GPU flow tests - on the fixture's
    OWN matrices reproduce every getPointFlow sample the reference recorded, forward and inverse, bit for bit."""
    fx = motion_fixture(mode)
    W, H = fx["width"], fx["height"]
    ys, xs = [a.reshape(-1) for a in np.meshgrid(fx["ys"], fx["xs"], indexing="ij")]
    assert len(xs) >= 48 and xs.max() == W - 1 and ys.max() == H - 1
    n = 0
    for objs in fx["tasks"]:
        for k, o in enumerate(objs):
            for key, mat in (("flow", "m_motion"), ("iflow", "m_motion_inv")):
                m = tuple(rs.hex_f64(o[mat]))
                u, v = xr.point_flow_bg(m, W, H, xs, ys) if k == 0 else xr.point_flow_fg(m, xs, ys)
                ref = rs.hex_f32_pairs(o[key])
                assert np.array_equal(np.stack([u, v], 1).view(np.uint32), ref.view(np.uint32)), (k, key)
                n += len(ref)
    assert n >= 2 * 2 * 48 * 15
