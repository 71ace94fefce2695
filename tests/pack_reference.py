"""numpy restatement of ofdg_pack (include/ofdg.h): what the CPU and GPU tests compare ofdg_host_pack and the device with, byte
for byte.  Reads nothing from the library: the value, the three roundings and the placement are written out here from the
header's text."""
import functools

import numpy as np

N = 3
NCHW, NHWC = 0, 1
# 8x2: one unit of 8 pixels per row, two in all.  24x6: three units per row.  72x40: 360 units - a second workgroup of 256 lanes
# that is partial.  264x200: 33 units per row (odd), 6600 units: 26 workgroups, the last one partial.
SIZES = [(8, 2), (24, 6), (72, 40), (264, 200)]
IMAGE_PAIRS = [(s, d) for s in ("float32", "uint8") for d in ("float32", "float16", "bfloat16")]
FLOW_PAIRS = [(s, d) for s in ("float32", "float16") for d in ("float32", "float16", "bfloat16")]
LAYOUTS = [(layout, concat, rgb) for layout in (NCHW, NHWC) for concat in (False, True) for rgb in (False, True)]


def norm(mean, std, unit=255.0):
    mean, std = np.asarray(mean, np.float64), np.asarray(std, np.float64)
    return (1.0 / (unit * std)).astype(np.float32), (-mean / std).astype(np.float32)


# (scale, bias, flow_scale): identity; the ImageNet statistics in B, G, R order; a negative scale; [-1, 1]
CONSTANTS = [
    (np.ones(3, np.float32), np.zeros(3, np.float32), np.float32(1.0)),
    norm((0.406, 0.456, 0.485), (0.225, 0.224, 0.229)) + (np.float32(0.05),),
    (np.float32([-1.0 / 255.0, -0.5, -2.0]), np.float32([1.0, 0.25, -0.0]), np.float32(-0.05)),
    (np.full(3, np.float32(2.0 / 255.0)), np.full(3, np.float32(-1.0)), np.float32(1.0 / 20.0)),
]
# 70000 overflows binary16 as it is, 2e7 under 1/255; 3.4e38 is above 0x7F7F8000: bfloat16 makes it infinite; 1e-40 is a denormal
SPECIAL_F32 = np.float32([np.nan, np.inf, -np.inf, -0.0, 1e-40, 1e9, 70000.0, 2e7, 3.4e38, -3.4e38, 65519.9, 65520.0, 0.0, 255.0, 127.5,
                          0.2 * 255.0, 1.0039063, 1.0117188, -1e-40, 5.9e-8, 2.9802322e-8, 8.9406967e-8])
SPECIAL_FLOW = np.float32([np.nan, np.inf, -np.inf, -0.0, 65504.0, -65504.0, 5.9604645e-8, -5.9604645e-8, 6.0975552e-5, 0.0])


@functools.lru_cache(maxsize=None)
def frames(W, H, dtype, n=N):
    """{image0, image1}: uint8 noise, or float32 values with fractions around the byte range and SPECIAL_F32 planted every 5th
    element"""
    rng = np.random.default_rng(W * 1000 + H)
    out = {}
    for f in range(2):
        if dtype == "uint8":
            t = rng.integers(0, 256, (n, 3, H, W), dtype=np.uint8)
            m = min(256, t.size)
            t.reshape(-1)[:m] = np.arange(256 - m, 256, dtype=np.uint8)
        else:
            t = rng.uniform(-20.0, 280.0, (n, 3, H, W)).astype(np.float32)
            flat = t.reshape(-1)
            at = np.arange(f, flat.size, 5)
            flat[at] = SPECIAL_F32[np.arange(at.size) % SPECIAL_F32.size]
        t.setflags(write=False)
        out["image%d" % f] = t
    return out


@functools.lru_cache(maxsize=None)
def flow(W, H, dtype, n=N):
    """float32 or float16 [n,2,H,W] with SPECIAL_FLOW planted every 7th element (float32 also holds its own denormal and values
    binary16 cannot hold)"""
    rng = np.random.default_rng(W * 1000 + H + 1)
    t = rng.normal(0.0, 30.0, (n, 2, H, W)).astype(np.float32)
    flat = t.reshape(-1)
    at = np.arange(3, flat.size, 7)
    special = SPECIAL_FLOW if dtype == "float16" else np.concatenate([SPECIAL_FLOW, np.float32([1e-40, -1e-40, 1e6, 3.4e38, 1.3e6, -70000.0])])
    flat[at] = special[np.arange(at.size) % special.size]
    t = t.astype(dtype)
    t.setflags(write=False)
    return t


def sources(W, H, image_dtype, flow_dtype, n=N):
    return dict(frames(W, H, image_dtype, n), flow=flow(W, H, flow_dtype, n))


def bf16_bits(y):
    """(uint16)((b + 0x7FFF + ((b >> 16) & 1)) >> 16) of the bits b of float32 y; a NaN: 0x7FC0"""
    b = np.ascontiguousarray(y, np.float32).view(np.uint32).astype(np.uint64)
    out = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    out[np.isnan(y)] = 0x7FC0
    return out


def f16_bits(y):
    """float32 -> binary16 bits to nearest even, in integers: an overflow becomes +-inf, subnormals are kept, a NaN is 0x7E00"""
    y = np.ascontiguousarray(y, np.float32)
    b = y.view(np.uint32)
    sign = ((b >> 16) & 0x8000).astype(np.uint32)
    a = b & 0x7FFFFFFF
    x = a.astype(np.int64) - 0x38000000
    normal = ((x + 0xFFF + ((x >> 13) & 1)) >> 13).astype(np.int64)
    tiny = np.where(a < 0x38800000, np.abs(y), np.float32(0.0)).astype(np.float64)
    small = np.rint(tiny * 2.0 ** 24).astype(np.int64)  # (exact product, to nearest even: 0 .. 1024)
    h = np.where(a >= 0x477FF000, 0x7C00, np.where(a >= 0x38800000, normal, small)).astype(np.uint32)
    out = (sign | h).astype(np.uint16)
    out[a > 0x7F800000] = 0x7E00
    return out


def stored(y, dtype):
    """the array that holds y in a destination of dtype: float32 (NaNs canonical), float16, or uint16 bit patterns of bfloat16"""
    if dtype == "bfloat16":
        return bf16_bits(y)
    if dtype == "float16":
        return f16_bits(y).view(np.float16)
    out = np.array(y, np.float32)
    out.view(np.uint32)[np.isnan(out)] = 0x7FC00000
    return out


def pack(src, image_dtype="float32", flow_dtype="float32", scale=(1, 1, 1), bias=(0, 0, 0), flow_scale=1.0, layout=NCHW, concat=False,
         rgb=False):
    """The packed planes of a dict of source arrays, each in the logical shape [n,C,H,W] - with NHWC a transposed view of an
    [n,H,W,C] array, so its memory is the header's element order."""
    scale, bias, flow_scale = np.float32(scale), np.float32(bias), np.float32(flow_scale)
    out = {}
    with np.errstate(all="ignore"):
        for key, t in src.items():
            if key == "flow":
                y = t.astype(np.float32) * flow_scale
                out[key] = stored(y, flow_dtype)
                continue
            f = int(key[-1])
            x = t.astype(np.float32)
            y = (x * scale.reshape(1, 3, 1, 1)).astype(np.float32) + bias.reshape(1, 3, 1, 1)
            if rgb:
                y = y[:, ::-1]
            y = stored(y, image_dtype)
            if not concat:
                out[key] = y
            else:
                if "image0" not in out:
                    out["image0"] = np.zeros((y.shape[0], 6) + y.shape[2:], y.dtype)
                out["image0"][:, 3 * f:3 * f + 3] = y
    if layout == NHWC:
        out = {k: np.ascontiguousarray(v.transpose(0, 2, 3, 1)).transpose(0, 3, 1, 2) for k, v in out.items()}
    return out


def memory(t, layout):
    """the bytes of a packed plane in memory order (a logical [n,C,H,W] array or torch-free view of one)"""
    t = np.asarray(t)
    m = np.ascontiguousarray(t.transpose(0, 2, 3, 1)) if layout == NHWC else np.ascontiguousarray(t)
    return m.view(np.uint8).reshape(-1)


def expect_equal(got, want, layout, what=""):
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for key in want:
        g, w = got[key], want[key]
        assert g.shape == w.shape and g.dtype.itemsize == w.dtype.itemsize, (what, key, g.shape, g.dtype, w.shape, w.dtype)
        if layout == NHWC:
            assert np.asarray(g).transpose(0, 2, 3, 1).flags["C_CONTIGUOUS"], (what, key, "not channels-last memory")
        a, b = memory(g, layout), memory(w, layout)
        if not np.array_equal(a, b):
            bad = np.flatnonzero(a != b)
            raise AssertionError("%s %s: %d bytes differ, first at byte %d (got %d, want %d)" % (what, key, bad.size, bad[0], a[bad[0]], b[bad[0]]))


def cases(k):
    """the six (image pair, flow pair) combinations met with constants k: image pair a with flow pair (a + k) % 6, so the four
    constants cross every image pair with four flow pairs"""
    return [(IMAGE_PAIRS[a], FLOW_PAIRS[(a + k) % 6]) for a in range(6)]


@functools.lru_cache(maxsize=8)
def expected(W, H, image_pair, flow_pair, k, layout, concat, rgb):
    """(sources, restatement) of one cell of the grid, computed once for the tests that need it"""
    scale, bias, flow_scale = CONSTANTS[k]
    src = sources(W, H, image_pair[0], flow_pair[0])
    return src, pack(src, image_pair[1], flow_pair[1], scale, bias, flow_scale, layout, concat, rgb)
