"""CPU tests of the motion boundaries (ofdg_boundaries, include/ofdg.h): the host twin ofdg_host_boundaries against the numpy
restatement (tests/boundaries_reference.py) byte for byte, known answers worked out here, subsets of the outputs, the refusals
(nothing written), the struct layout and the ValueErrors of boundaries_format."""
import ctypes as C

import numpy as np
import pytest

import boundaries_reference as br

FILL = 0xA5


def twin(ofdg, src, frames=(0, 1), **kw):
    return ofdg.host_boundaries(src["flow"] if 0 in frames else None, src["label"] if 0 in frames else None,
                                src["flow1"] if 1 in frames else None, src["label1"] if 1 in frames else None, **kw)


@pytest.mark.parametrize("W,H", br.SIZES)
@pytest.mark.parametrize("radius", br.RADII)
@pytest.mark.parametrize("labels", [True, False])
@pytest.mark.parametrize("fmt", [br.F32, br.F16])
def test_twin_equals_restatement(ofdg, fmt, labels, radius, W, H):
    """Both frames in one job, n = 3: blocks, spikes in the corners and on the borders, NaN, +-inf, -0.0, denormals and
    +-65504 every 7th element of two of the samples."""
    src = br.inputs(W, H, fmt)
    before = {k: v.tobytes() for k, v in src.items()}
    for min_step in br.MIN_STEPS:
        got = twin(ofdg, src, radius=radius, min_step=min_step, labels=labels)
        want = br.expected(W, H, fmt, labels, radius, min_step)
        assert set(got) == set(want)
        br.expect_equal(got, want, "%dx%d fmt %d labels %d radius %d min_step %g" % (W, H, fmt, labels, radius, min_step))
    assert all(src[k].tobytes() == before[k] for k in src), "the sources"
    if W >= 24:  # the inputs exercise both outcomes
        e = br.expected(W, H, fmt, labels, radius, 0.0)["edge0"]
        assert e.any() and not e.all()


def test_labels_decide():
    """The inputs hold two labels that move identically and flow steps inside one label: the first is an edge with neither
    setting, the second only with labels off."""
    flow = np.zeros((1, 2, 4, 16), np.float32)
    label = np.zeros((1, 4, 16), np.uint8)
    label[:, :, 8:] = 1          # two labels, one motion
    flow[:, 0, :, 12:] = 2.0     # a step inside label 1
    on, off = br.edge_of(flow, label, 0.0, True), br.edge_of(flow, label, 0.0, False)
    assert not on.any()
    assert off[0, 0, :, 11:13].all() and off.sum() == 8


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_labels_decide_twin(ofdg, dtype):
    flow = np.zeros((1, 2, 4, 16), dtype)
    label = np.zeros((1, 4, 16), np.uint8)
    label[:, :, 8:] = 1
    flow[:, 0, :, 12:] = 2.0
    on = ofdg.host_boundaries(flow, label, radius=3, labels=True)
    off = ofdg.host_boundaries(flow, label, radius=3, labels=False)
    assert not on["edge0"].any() and (on["dist0"] == ofdg.BND_FAR).all()
    want = np.zeros((4, 16), np.uint8)
    want[:, 11:13] = 1
    assert np.array_equal(off["edge0"][0, 0], want)
    # labels=None: used, because a label plane is given
    assert not ofdg.host_boundaries(flow, label, radius=3)["edge0"].any()
    assert np.array_equal(ofdg.host_boundaries(flow, radius=3)["edge0"][0, 0], want)


@pytest.mark.parametrize("radius", [1, 4, 10, 15])
def test_vertical_step(ofdg, radius):
    """A step between columns k - 1 and k: edge on exactly those two columns, dist2 = d^2 for d = 1..radius, then 255."""
    W, H, k = 48, 6, 20
    flow = np.zeros((2, 2, H, W), np.float32)
    flow[:, 1, :, k:] = 1.0
    out = ofdg.host_boundaries(flow, radius=radius, min_step=0.5)
    cols = np.arange(W)
    d = np.where(cols < k, k - 1 - cols, cols - k)
    assert np.array_equal(out["edge0"], np.broadcast_to((d == 0).astype(np.uint8), (2, 1, H, W)))
    assert np.array_equal(out["dist0"], np.broadcast_to(np.where(d <= radius, d * d, 255).astype(np.uint8), (2, 1, H, W)))
    # a step of exactly min_step is none: the comparison is strict
    assert not ofdg.host_boundaries(flow, radius=radius, min_step=1.0)["edge0"].any()


@pytest.mark.parametrize("radius", [2, 7, 15])
def test_single_spike(ofdg, radius):
    """edge on the plus-shaped five pixels, dist2 the union of five discs"""
    W, H, sx, sy = 40, 36, 17, 18
    flow = np.zeros((1, 2, H, W), np.float16)
    flow[0, 0, sy, sx] = 3.0
    out = ofdg.host_boundaries(flow, radius=radius)
    plus = [(sx, sy), (sx - 1, sy), (sx + 1, sy), (sx, sy - 1), (sx, sy + 1)]
    edge = np.zeros((H, W), np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    d2 = np.full((H, W), 10 ** 6)
    for x, y in plus:
        edge[y, x] = 1
        d2 = np.minimum(d2, (xx - x) ** 2 + (yy - y) ** 2)
    assert np.array_equal(out["edge0"][0, 0], edge)
    assert np.array_equal(out["dist0"][0, 0], np.where(d2 <= radius * radius, d2, 255).astype(np.uint8))


def test_constant_flow_and_special_values(ofdg):
    flow = np.full((2, 2, 6, 16), 1.25, np.float32)
    out = ofdg.host_boundaries(flow, radius=15)
    assert not out["edge0"].any() and (out["dist0"] == 255).all()
    # inf beside inf: inf - inf is a NaN, no step; inf beside 0: d2 is inf, a step; a NaN beside anything: no step
    flow = np.zeros((1, 2, 2, 16), np.float32)
    flow[0, 0, :, 4:8] = np.inf
    flow[0, 1, :, 12] = np.nan
    edge = ofdg.host_boundaries(flow, dist=False)["edge0"][0, 0]
    want = np.zeros((2, 16), np.uint8)
    want[:, [3, 4, 7, 8]] = 1
    assert np.array_equal(edge, want)
    # min_step 0 and a denormal difference whose square underflows: no step; a difference whose square is a denormal: a step
    flow = np.zeros((1, 2, 2, 16), np.float32)
    flow[0, 0, :, 8:] = 1e-40
    assert not ofdg.host_boundaries(flow, dist=False)["edge0"].any()
    flow[0, 0, :, 8:] = 1e-20
    assert ofdg.host_boundaries(flow, dist=False)["edge0"].sum() == 4
    # -0.0 beside +0.0 is no step
    flow[0, 0, :, 8:] = -0.0
    assert not ofdg.host_boundaries(flow, dist=False)["edge0"].any()


def test_subsets(ofdg):
    W, H = 72, 40
    src = br.inputs(W, H, br.F32)
    want = br.expected(W, H, br.F32, True, 4, 0.5)
    kw = dict(radius=4, min_step=0.5, labels=True)
    only_edge = twin(ofdg, src, edge=True, dist=False, **kw)
    assert set(only_edge) == {"edge0", "edge1"}
    br.expect_equal(only_edge, want, "edge only")
    only_dist = twin(ofdg, src, edge=False, dist=True, **kw)
    assert set(only_dist) == {"dist0", "dist1"}
    br.expect_equal(only_dist, want, "dist2 only")
    frame1 = twin(ofdg, src, frames=(1,), **kw)
    assert set(frame1) == {"edge1", "dist1"}
    br.expect_equal(frame1, want, "frame 1 only")
    frame0 = twin(ofdg, src, frames=(0,), **kw)
    assert set(frame0) == {"edge0", "dist0"}
    br.expect_equal(frame0, want, "frame 0 only")


def test_struct_layout(ofdg):
    J = ofdg.BoundaryJob
    assert C.sizeof(J) == 96
    offs = {name: getattr(J, name).offset for name, _ in J._fields_}
    assert offs == dict(flow=0, label=16, edge=32, dist2=48, width=64, height=68, flow_fmt=72, flags=76, radius=80, min_step=84, reserved=88)
    assert (ofdg.BND_LABELS, ofdg.BND_MAX_RADIUS, ofdg.BND_FAR) == (1, 15, 255)
    assert "ofdg_boundaries" in ofdg.EXPORTS and "ofdg_host_boundaries" in ofdg.EXPORTS


def test_refusals_write_nothing(ofdg):
    W, H, n = 24, 6, 2
    lib = ofdg.lib()
    flows = [np.zeros((n, 2, H, W), np.float32) for _ in range(2)]
    for f in flows:
        f[:, 0, :, 10:] = 2.0
    labs = [np.zeros((n, H, W), np.uint8) for _ in range(2)]
    # one buffer for the four outputs, so that "just apart" and "overlapping" are a matter of offsets
    plane = n * H * W
    raw = np.full(4 * plane + 64, FILL, np.uint8)
    base = raw.ctypes.data

    def job(**kw):
        j = ofdg.BoundaryJob()
        for f in range(2):
            j.flow[f], j.label[f] = flows[f].ctypes.data, labs[f].ctypes.data
            j.edge[f], j.dist2[f] = base + (2 * f) * plane, base + (2 * f + 1) * plane
        j.flow_fmt, j.flags, j.radius, j.min_step = ofdg.FMT_F32, ofdg.BND_LABELS, 3, 0.5
        for k, v in kw.items():
            if isinstance(v, dict):
                for idx, val in v.items():
                    getattr(j, k)[idx] = val
            else:
                setattr(j, k, v)
        return j

    def refused(word, j, n_samples=n, w=W, h=H):
        rc = lib.ofdg_host_boundaries(None if j is None else C.byref(j), n_samples, w, h)
        assert rc == ofdg.EINVAL, word
        msg = lib.ofdg_host_last_error().decode()
        assert msg.startswith("ofdg_host_boundaries: ") and word in msg, (word, msg)
        assert (raw == FILL).all(), word

    refused("job", None)
    refused("n_samples", job(), n_samples=0)
    refused("both be 0", job(width=W))
    refused("plane size given", job(width=W + 8, height=H))
    for bad_w, bad_h in ((20, 6), (24, 5), (4, 2), (8, 0)):
        refused("width", job(), w=bad_w, h=bad_h)
    refused("2^31", job(), n_samples=1, w=65536, h=32768)
    refused("flags", job(flags=2))
    refused("flags", job(flags=-1))
    refused("reserved", job(reserved={1: 1}))
    refused("flow_fmt", job(flow_fmt=ofdg.FMT_U8))
    refused("flow_fmt", job(flow_fmt=3))
    refused("no frame", job(flow={0: None, 1: None}, edge={0: None, 1: None}, dist2={0: None, 1: None}))
    refused("edge: an output of a frame without its flow", job(flow={1: None}, dist2={1: None}))
    refused("dist2: an output of a frame without its flow", job(flow={0: None}, edge={0: None}))
    refused("no output", job(edge={1: None}, dist2={1: None}))
    refused("label", job(label={1: None}))
    for bad in (float("nan"), -1.0, float("inf"), -0.0 - 1e-30):
        refused("min_step", job(min_step=bad))
    for bad in (0, 16, -3):
        refused("radius", job(radius=bad))
    refused("overlaps", job(dist2={0: base + plane - 1}))             # dist2[0] starts on the last byte of edge[0]
    refused("overlaps", job(edge={1: flows[0].ctypes.data + 8}))      # an output inside a flow
    refused("overlaps", job(edge={0: labs[1].ctypes.data}))           # an output on a label plane
    refused("overlaps", job(edge={0: base, 1: base}))
    # radius is not read without a dist2 plane; a label plane is not needed without OFDG_BND_LABELS; ranges just apart are fine
    ok = job(radius=99, dist2={0: None, 1: None}, flags=0, label={0: None, 1: None})
    assert lib.ofdg_host_boundaries(C.byref(ok), n, W, H) == ofdg.OK
    ok = job(width=W, height=H)
    assert lib.ofdg_host_boundaries(C.byref(ok), n, W, H) == ofdg.OK
    out = raw[:4 * plane].reshape(4, n, 1, H, W)
    want = ofdg.host_boundaries(flows[0], labs[0], flows[1], labs[1], radius=3, min_step=0.5)
    for k, name in enumerate(("edge0", "dist0", "edge1", "dist1")):
        assert np.array_equal(out[k], want[name]), name
    assert (raw[4 * plane:] == FILL).all()


def test_boundaries_format_raises(ofdg):
    z = np.zeros
    flow, out, lab = z((2, 2, 6, 24), np.float32), z((2, 1, 6, 24), np.uint8), z((2, 6, 24), np.uint8)
    assert ofdg.boundaries_format(flow, out, out, lab) == (2, 6, 24, ofdg.FMT_F32)
    assert ofdg.boundaries_format(None, flow1=flow.astype(np.float16), dist2_1=out) == (2, 6, 24, ofdg.FMT_F16)
    bad = [
        dict(flow=None),
        dict(flow=flow),                                            # a frame without an output
        dict(flow=flow, edge=out, edge1=out),                       # an output without its flow
        dict(flow=flow, edge=out, dist2_1=out),
        dict(flow=flow.astype(np.float64), edge=out),
        dict(flow=z((2, 3, 6, 24), np.float32), edge=out),
        dict(flow=z((2, 2, 6, 20), np.float32), edge=z((2, 1, 6, 20), np.uint8)),
        dict(flow=z((2, 2, 5, 24), np.float32), edge=z((2, 1, 5, 24), np.uint8)),
        dict(flow=flow, edge=z((2, 6, 24), np.uint8)),
        dict(flow=flow, edge=out.astype(np.int8)),
        dict(flow=flow, dist2=z((1, 1, 6, 24), np.uint8)),
        dict(flow=flow, edge=out, label=z((2, 1, 6, 24), np.uint8)),
        dict(flow=flow, edge=out, label=lab.astype(np.int32)),
        dict(flow=flow, edge=out, flow1=flow.astype(np.float16), edge1=out),  # two dtypes
        dict(flow=flow, edge=out, flow1=z((3, 2, 6, 24), np.float32), edge1=z((3, 1, 6, 24), np.uint8)),
        dict(flow=flow, edge=out, height=8, width=24),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            ofdg.boundaries_format(**kw)
    with pytest.raises(ValueError, match="labels=True"):
        ofdg.host_boundaries(flow, None, labels=True)
