"""CPU tests of the network-ready packing (ofdg_host_pack, include/ofdg.h): the host twin against the numpy restatement
(tests/pack_reference.py) byte for byte over formats, layouts, sizes and constants; the roundings pinned to torch and numpy;
known answers worked out here; subsets of planes; every refusal; pack_norm, the ctypes layout and pack_format.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import pack_reference as pk

FILL = 0xA5


def host(ofdg, src, image_pair, flow_pair, k, layout, concat, rgb):
    scale, bias, flow_scale = pk.CONSTANTS[k]
    return ofdg.host_pack(src, image_dtype=image_pair[1], flow_dtype=flow_pair[1], scale=scale, bias=bias, flow_scale=flow_scale,
                          layout=layout, concat=concat, rgb=rgb)


@pytest.mark.parametrize("W,H", pk.SIZES)
@pytest.mark.parametrize("layout,concat,rgb", pk.LAYOUTS)
def test_host_pack_equals_restatement(ofdg, W, H, layout, concat, rgb):
    """Every image pair and every flow pair under every set of constants (pack_reference.cases), n = 3; float32 frames hold
    NaN, infinities, -0.0, denormals and values that overflow binary16 and bfloat16, flows the same every 7th element."""
    for k in range(len(pk.CONSTANTS)):
        for image_pair, flow_pair in pk.cases(k):
            src, want = pk.expected(W, H, image_pair, flow_pair, k, layout, concat, rgb)
            got = host(ofdg, src, image_pair, flow_pair, k, layout, concat, rgb)
            pk.expect_equal(got, want, layout, "%dx%d %s %s constants %d layout %d concat %d rgb %d" % (W, H, image_pair, flow_pair, k, layout, concat, rgb))
    f = pk.frames(W, H, "float32")["image0"].reshape(-1)
    if f.size >= 5 * pk.SPECIAL_F32.size:
        assert np.isnan(f).any() and np.isinf(f).any() and (f == np.float32(1e-40)).any() and (f == np.float32(3.4e38)).any()
        assert (np.signbit(f) & (f == 0)).any()


def test_restatement_roundings_match_torch_and_numpy():
    """The restatement's bfloat16 against torch's conversion and its binary16 against numpy's, on every finite value the tests
    store - all sources under all constants - and on 2^18 random finite bit patterns."""
    import torch
    rng = np.random.default_rng(11)
    bits = rng.integers(0, 1 << 32, 1 << 18, dtype=np.uint64).astype(np.uint32)
    values = [bits.view(np.float32), np.float32([0.0, -0.0, 1e-45, -1e-45, 65504.0, 65519.996, 65520.0, 3.3961775e38, 3.4028235e38, np.inf, -np.inf])]
    with np.errstate(all="ignore"):
        for W, H in pk.SIZES[:3]:
            for scale, bias, flow_scale in pk.CONSTANTS:
                for dtype in ("float32", "uint8"):
                    for t in pk.frames(W, H, dtype).values():
                        values.append(((t.astype(np.float32) * scale.reshape(1, 3, 1, 1)).astype(np.float32) + bias.reshape(1, 3, 1, 1)).reshape(-1))
                for dtype in ("float32", "float16"):
                    values.append((pk.flow(W, H, dtype).astype(np.float32) * flow_scale).reshape(-1))
        y = np.concatenate(values).astype(np.float32)
        y = y[~np.isnan(y)]
        want_bf16 = torch.from_numpy(y).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
        assert np.array_equal(pk.bf16_bits(y), want_bf16)
        assert np.array_equal(pk.f16_bits(y), y.astype(np.float16).view(np.uint16))
    assert np.isinf(y).any() and (np.abs(y) > 3.3961775e38).any() and ((np.abs(y) > 65520) & np.isfinite(y)).any() and ((y != 0) & (np.abs(y) < 1e-38)).any()
    nan = np.uint32([0x7FC00000, 0xFFC00001, 0x7F800001, 0xFFFFFFFF]).view(np.float32)
    assert pk.bf16_bits(nan).tolist() == [0x7FC0] * 4 and pk.f16_bits(nan).tolist() == [0x7E00] * 4
    assert pk.stored(nan, "float32").view(np.uint32).tolist() == [0x7FC00000] * 4


def test_known_answers(ofdg):
    """Bytes 0, 51 and 255 under scale = fl32(1/255) = 0x3B808081 = 0.003921568859...: 51 * scale = 0.20000001183 lies above the
    tie 0.20000001043 between 0.2f = 0x3E4CCCCD and its successor, so the float32 result is 0x3E4CCCCE - one ulp above 0.2f, as
    the definition's two roundings give it (a single rounding of 51 / 255 would give 0.2f); 255 * scale = 1.0000000591 is below
    the tie 1 + 2^-24 = 1.0000000596, so 1.0f.  Of 0x3E4CCCCE: binary16 0x3266 (the 13 bits cut off, 0xCCE, are below the tie
    0x1000), bfloat16 0x3E4D (the lower half 0xCCCE is above 0x8000)."""
    t = np.zeros((1, 3, 2, 8), np.uint8)
    t[0, :, 0, :3] = [0, 51, 255]
    s = np.float32(1.0) / np.float32(255.0)
    assert s.view(np.uint32) == 0x3B808081
    answers = {"float32": (np.uint32, [0x00000000, 0x3E4CCCCE, 0x3F800000]), "float16": (np.uint16, [0x0000, 0x3266, 0x3C00]),
               "bfloat16": (np.uint16, [0x0000, 0x3E4D, 0x3F80])}
    for dtype, (bits, want) in answers.items():
        got = ofdg.host_pack({"image0": t}, image_dtype=dtype, scale=(s, s, s))["image0"]
        for c in range(3):
            assert np.ascontiguousarray(got[0, c, 0, :3]).view(bits).tolist() == want, (dtype, c)
    # a flow of 20 px under FlowNet's 1/20: fl32(20 * fl32(0.05)) = 1.0 (0.05f = 0x3D4CCCCD, the product 1.00000001490 rounds down)
    u = np.full((1, 2, 2, 8), 20.0, np.float16)
    got = ofdg.host_pack({"flow": u}, flow_dtype="bfloat16", flow_scale=0.05)["flow"]
    assert (got == 0x3F80).all()


@pytest.mark.parametrize("layout", [pk.NCHW, pk.NHWC])
@pytest.mark.parametrize("concat", [False, True])
def test_placement_by_encoded_coordinates(ofdg, layout, concat):
    """A float32 frame whose element (i, c, y, x) of frame f holds the number ((((f * n + i) * 3 + c) * H + y) * W + x) (exact
    below 2^24), identity constants, float32 destination: the destination's memory, read at the header's element index, must hold
    the number of the source element the header names - all four (layout, concat) pairs, with and without OFDG_PACK_RGB."""
    n, H, W = 2, 4, 16
    code = np.arange(2 * n * 3 * H * W, dtype=np.float32).reshape(2, n, 3, H, W)
    src = {"image0": code[0], "image1": code[1]}
    for rgb in (False, True):
        got = ofdg.host_pack(src, layout=layout, concat=concat, rgb=rgb)
        Cd = 6 if concat else 3
        for f in range(2):
            t = got["image0" if concat else "image%d" % f]
            mem = (np.ascontiguousarray(t.transpose(0, 2, 3, 1)) if layout == pk.NHWC else np.ascontiguousarray(t)).reshape(-1)
            assert mem.size == n * Cd * H * W
            for i in range(n):
                for c in range(3):
                    cd = (3 * f if concat else 0) + (2 - c if rgb else c)
                    for y in range(H):
                        for x in (0, 7, 8, W - 1):
                            at = ((i * H + y) * W + x) * Cd + cd if layout == pk.NHWC else ((i * Cd + cd) * H + y) * W + x
                            assert mem[at] == code[f, i, c, y, x], (rgb, f, i, c, y, x)
    # the flow's channels keep their order, whatever the flags
    flow = np.arange(n * 2 * H * W, dtype=np.float32).reshape(n, 2, H, W)
    t = ofdg.host_pack({"flow": flow}, layout=layout, rgb=True)["flow"]
    mem = (np.ascontiguousarray(t.transpose(0, 2, 3, 1)) if layout == pk.NHWC else np.ascontiguousarray(t)).reshape(-1)
    for i, c, y, x in ((0, 0, 0, 0), (1, 1, 3, 15), (1, 0, 2, 9), (0, 1, 1, 8)):
        at = ((i * H + y) * W + x) * 2 + c if layout == pk.NHWC else ((i * 2 + c) * H + y) * W + x
        assert mem[at] == flow[i, c, y, x]


@pytest.mark.parametrize("layout", [pk.NCHW, pk.NHWC])
def test_subsets_of_planes(ofdg, layout):
    W, H = 72, 40
    src = pk.sources(W, H, "uint8", "float16")
    scale, bias, flow_scale = pk.CONSTANTS[1]
    kw = dict(image_dtype="bfloat16", flow_dtype="float16", scale=scale, bias=bias, flow_scale=flow_scale, layout=layout, rgb=True)
    whole = pk.pack(src, **kw)
    for keys in (("flow",), ("image1",), ("image0",), ("image0", "image1"), ("image1", "flow")):
        part = {k: src[k] for k in keys}
        got = ofdg.host_pack(part, **kw)
        pk.expect_equal(got, {k: whole[k] for k in keys}, layout, "planes %s" % (keys,))
    both = ofdg.host_pack({k: src[k] for k in ("image0", "image1")}, concat=True, **kw)
    pk.expect_equal(both, pk.pack({k: src[k] for k in ("image0", "image1")}, concat=True, **kw), layout, "frames without flow, concatenated")
    assert set(both) == {"image0"} and both["image0"].shape == (pk.N, 6, H, W)


def test_pack_norm_and_layouts(ofdg):
    scale, bias = ofdg.pack_norm((0.406, 0.456, 0.485), (0.225, 0.224, 0.229))
    assert scale.dtype == np.float32 and bias.dtype == np.float32 and scale.shape == (3,) and bias.shape == (3,)
    for c, (m, s) in enumerate(zip((0.406, 0.456, 0.485), (0.225, 0.224, 0.229))):
        assert scale[c] == np.float32(1.0 / (255.0 * s)) and bias[c] == np.float32(-m / s)
    want_scale, want_bias = pk.norm((0.406, 0.456, 0.485), (0.225, 0.224, 0.229))
    assert np.array_equal(scale, want_scale) and np.array_equal(bias, want_bias)
    s1, b1 = ofdg.pack_norm((0.5, 0.5, 0.5), (0.5, 0.5, 0.5), unit=1.0)
    assert s1.tolist() == [2.0] * 3 and b1.tolist() == [-1.0] * 3
    J = ofdg.PackJob
    assert C.sizeof(J) == 112
    offsets = dict(src=0, dst=24, width=48, height=52, image_src_fmt=56, flow_src_fmt=60, image_dst_fmt=64, flow_dst_fmt=68, layout=72, flags=76,
                   scale=80, bias=92, flow_scale=104, reserved=108)
    assert {k: getattr(J, k).offset for k in offsets} == offsets
    assert (ofdg.FMT_BF16, ofdg.PACK_NCHW, ofdg.PACK_NHWC, ofdg.PACK_CONCAT, ofdg.PACK_RGB) == (3, 0, 1, 1, 2)
    assert ofdg.PACK_PLANES == ("image0", "image1", "flow")
    assert "ofdg_pack" in ofdg.EXPORTS and "ofdg_host_pack" in ofdg.EXPORTS


def test_pack_format(ofdg):
    n, H, W = 2, 6, 24
    img = lambda dt="uint8", c=3: np.zeros((n, c, H, W), dt)  # noqa: E731
    flw = lambda dt="float16": np.zeros((n, 2, H, W), dt)     # noqa: E731
    src = {"image0": img(), "image1": img(), "flow": flw()}
    dst = {"image0": img("uint16"), "image1": img("uint16"), "flow": flw("float32")}
    assert ofdg.pack_format(src, dst, ofdg.PACK_NCHW, False) == (n, H, W, ofdg.FMT_U8, ofdg.FMT_F16, ofdg.FMT_BF16, ofdg.FMT_F32)
    cat = {"image0": img("float16", 6), "flow": flw("float16")}
    assert ofdg.pack_format(src, cat, ofdg.PACK_NHWC, True, H, W) == (n, H, W, ofdg.FMT_U8, ofdg.FMT_F16, ofdg.FMT_F16, ofdg.FMT_F16)
    assert ofdg.pack_format({"flow": flw("float32")}, {"flow": flw("float32")}, 0, False) == (n, H, W, 0, 0, 0, 0)
    bad = [
        (src, dst, 2, False, {}, "layout"),
        ({}, {}, 0, False, {}, "at least one"),
        ({"depth": img()}, {"depth": img()}, 0, False, {}, "unknown plane"),
        ({"image0": img()}, {"image0": img("uint16", 6)}, 0, True, {}, "concat needs"),
        (src, dst, 0, True, {}, "dst must hold"),
        ({"image0": img()}, {"flow": flw()}, 0, False, {}, "dst must hold"),
        (src, dst, 0, False, dict(height=H, width=W + 8), "source plane"),
        ({"image0": np.zeros((n, 3, H, 20), np.uint8)}, {"image0": np.zeros((n, 3, H, 20), np.float32)}, 0, False, {}, "multiple of 8"),
        ({"image0": np.zeros((n, 3, 5, W), np.uint8)}, {"image0": np.zeros((n, 3, 5, W), np.float32)}, 0, False, {}, "multiple of 8"),
        ({"image0": img("float16")}, {"image0": img("float32")}, 0, False, {}, r"src\[image0\] must be"),
        ({"flow": flw("uint8")}, {"flow": flw("float32")}, 0, False, {}, r"src\[flow\] must be"),
        ({"image0": img()}, {"image0": img("uint8")}, 0, False, {}, r"dst\[image0\] must be float32, float16 or bfloat16"),
        ({"image0": img()}, {"image0": img("float32", 6)}, 0, False, {}, r"dst\[image0\] must be"),
        (src, dict(dst, image1=img("float32")), 0, False, {}, "one dtype"),
        (dict(src, image1=img("float32")), dst, 0, False, {}, "one dtype"),
        ({"image0": img(), "flow": np.zeros((n, 2, H, W + 8), np.float32)}, {"image0": img("float32"), "flow": np.zeros((n, 2, H, W + 8), np.float32)}, 0,
         False, {}, r"src\[flow\] must be"),
    ]
    for s, d, layout, concat, kw, word in bad:
        with pytest.raises(ValueError, match=word):
            ofdg.pack_format(s, d, layout, concat, **kw)


def test_refusals_write_nothing(ofdg):
    """Every rule of the header the host twin can break, each with outputs that stay 0xA5 and the field named; then a valid
    call with the same buffers."""
    lib = ofdg.lib()
    n, W, H = 2, 24, 6
    src = pk.sources(W, H, "uint8", "float16", n)
    outs = [np.full((n, 6, H, W), FILL, np.uint8).view(np.uint8) for _ in range(2)] + [np.full((n, 2, H, W, 4), FILL, np.uint8)]
    big = np.full((n * 6 * H * W * 4 + 64,), FILL, np.uint8)  # room for any format, for the overlap cases

    def job(**kw):
        j = ofdg.PackJob()
        for k, key in enumerate(ofdg.PACK_PLANES):
            j.src[k], j.dst[k] = src[key].ctypes.data, outs[k].ctypes.data
        j.image_src_fmt, j.flow_src_fmt, j.image_dst_fmt, j.flow_dst_fmt = ofdg.FMT_U8, ofdg.FMT_F16, ofdg.FMT_BF16, ofdg.FMT_F32
        j.scale[:], j.bias[:], j.flow_scale = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), 1.0
        for k, v in kw.items():
            if k in ("src", "dst", "scale", "bias"):
                for idx, val in v.items():
                    getattr(j, k)[idx] = val
            else:
                setattr(j, k, v)
        return j

    def refused(word, j, n_samples=n, width=W, height=H):
        rc = lib.ofdg_host_pack(None if j is None else C.byref(j), n_samples, width, height)
        assert rc == ofdg.EINVAL, word
        msg = lib.ofdg_host_last_error().decode()
        assert msg.startswith("ofdg_host_pack: ") and word in msg, (word, msg)
        assert all((o == FILL).all() for o in outs) and (big == FILL).all(), word

    refused("job", None)
    refused("n_samples", job(), n_samples=0)
    refused("both be 0", job(width=W))
    refused("both be 0", job(height=H))
    refused("0, 0 or the plane size", job(width=W + 8, height=H))
    for bad_w, bad_h in ((20, 6), (24, 5), (4, 2), (0, 6), (24, 0)):
        refused("width", job(), width=bad_w, height=bad_h)
    refused("2^31", job(), n_samples=1, width=32768, height=10924)
    refused("image_src_fmt", job(image_src_fmt=ofdg.FMT_F16))
    refused("image_src_fmt", job(image_src_fmt=ofdg.FMT_BF16))
    refused("flow_src_fmt", job(flow_src_fmt=ofdg.FMT_U8))
    refused("flow_src_fmt", job(flow_src_fmt=ofdg.FMT_BF16))
    refused("image_dst_fmt", job(image_dst_fmt=ofdg.FMT_U8))
    refused("flow_dst_fmt", job(flow_dst_fmt=4))
    refused("layout", job(layout=2))
    refused("layout", job(layout=-1))
    refused("flags", job(flags=4))
    refused("reserved", job(reserved=1))
    for bad in (float("nan"), float("inf"), float("-inf")):
        refused("scale", job(scale={1: bad}))
        refused("bias", job(bias={2: bad}))
        refused("flow_scale", job(flow_scale=bad))
    refused("no plane", job(src={0: None, 1: None, 2: None}, dst={0: None, 1: None, 2: None}))
    refused("dst", job(dst={2: None}))
    refused("src", job(src={1: None}))
    refused("CONCAT needs both", job(flags=ofdg.PACK_CONCAT, src={1: None}, dst={1: None}))
    refused("dst[image1]", job(flags=ofdg.PACK_CONCAT))
    refused("overlaps", job(dst={1: outs[0].ctypes.data + 16}))
    refused("overlaps", job(dst={0: src["image0"].ctypes.data}))            # in place
    refused("overlaps", job(src={0: None}, dst={0: None, 2: src["image1"].ctypes.data + n * 3 * H * W - 1}))  # the last byte of another source
    refused("overlaps", job(flags=ofdg.PACK_CONCAT, dst={0: big.ctypes.data, 1: None, 2: big.ctypes.data + n * 6 * H * W * 2 - 2}))  # C = 6 counts
    # the ranges just apart are accepted: the flow right behind the 6-channel frames
    j = job(flags=ofdg.PACK_CONCAT, dst={0: big.ctypes.data, 1: None, 2: big.ctypes.data + n * 6 * H * W * 2})
    assert lib.ofdg_host_pack(C.byref(j), n, W, H) == ofdg.OK and (big[n * 6 * H * W * 2 + n * 2 * H * W * 4:] == FILL).all()
    assert all((o == FILL).all() for o in outs)
    # a valid call into the same buffers
    assert lib.ofdg_host_pack(C.byref(job(width=W, height=H)), n, W, H) == ofdg.OK
    want = pk.pack(src, "bfloat16", "float32")
    for k, key in enumerate(ofdg.PACK_PLANES):
        m = pk.memory(want[key], pk.NCHW)
        assert np.array_equal(outs[k].reshape(-1)[:m.size], m) and (outs[k].reshape(-1)[m.size:] == FILL).all(), key
