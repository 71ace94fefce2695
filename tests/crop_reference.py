"""The training crop (ofdg_crop, include/ofdg.h) restated in numpy and plain integers, independent of the library: Philox4x32-10,
the draw of a record, its sanitising, the move with its sign-bit rule and the window rule of the occlusion maps - plus the
planes and records the CPU and the GPU tests share."""
import numpy as np

HFLIP, VFLIP, RANDOM_HFLIP, RANDOM_VFLIP, OCC_WINDOW = 1, 2, 4, 8, 16
PLANES = ("image0", "image1", "flow", "flow1", "occ0", "occ1", "label0", "label1")
M32 = 0xFFFFFFFF
# W, H, crop_w, crop_h: a window inside the frame, the whole frame, a window that is no multiple of 16 wide or 4 high and
# spans several workgroups with a partial last one in float32 and binary16
SHAPES = [(72, 40, 40, 24), (72, 40, 72, 40), (160, 100, 136, 66)]
N = 9


def philox4x32(ctr, key, rounds=10):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw: Parallel random numbers - as easy as 1, 2, 3; SC'11) on Python integers."""
    c, k = list(ctr), list(key)
    for _ in range(rounds):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & M32, (p0 >> 32) ^ c[3] ^ k[1], p0 & M32]
        k = [(k[0] + 0x9E3779B9) & M32, (k[1] + 0xBB67AE85) & M32]
    return tuple(c)


def draw(seed, index, W, H, crop_w, crop_h, flags):
    """(x0, y0, record flags) of global sample `index`."""
    g = index & 0xFFFFFFFFFFFFFFFF
    key = ((seed ^ (((g >> 32) * 0x9E3779B9) & M32)) & M32, g & M32)
    w = philox4x32((0, 0, 0x0C70, 0), key)
    x0 = (w[0] * (W - crop_w + 1)) >> 32
    y0 = (w[1] * (H - crop_h + 1)) >> 32
    fl = ((w[2] & 1) if flags & RANDOM_HFLIP else 0) | ((((w[2] >> 1) & 1) << 1) if flags & RANDOM_VFLIP else 0)
    return x0, y0, fl


def sanitise(rec, W, H, crop_w, crop_h):
    x0, y0, fl = int(rec[0]), int(rec[1]), int(rec[2])
    return min(max(x0, 0), W - crop_w), min(max(y0, 0), H - crop_h), fl & 3, 0


def drawn_records(seed, first_index, n, W, H, crop_w, crop_h, flags):
    return np.array([draw(seed, first_index + i, W, H, crop_w, crop_h, flags) + (0,) for i in range(n)], np.int32)


def _inside(at, d, lo, length):
    """the window test of one axis in float32: floorf(fl32(fl32(at + d) + 0.5f)) in [lo, lo + length - 1]; a NaN is outside"""
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.floor((at.astype(np.float32) + d.astype(np.float32)).astype(np.float32) + np.float32(0.5))
        return (t >= np.float32(lo)) & (t <= np.float32(lo + length - 1))


def crop(src, recs, crop_w, crop_h, occ_window=False):
    """(dst, sanitised records) of the planes in `src` (name -> array [n,C,H,W], labels [n,H,W]) under recs (int [n,4])."""
    first = next(iter(src.values()))
    n, (H, W) = first.shape[0], first.shape[-2:]
    used = np.array([sanitise(r, W, H, crop_w, crop_h) for r in recs], np.int32)
    dst = {}
    for name, a in src.items():
        out = np.zeros(a.shape[:-2] + (crop_h, crop_w), a.dtype)
        for i, (x0, y0, fl, _) in enumerate(used):
            win = a[i, ..., y0:y0 + crop_h, x0:x0 + crop_w].copy()
            if name.startswith("occ") and occ_window:
                flow = src["flow" if name == "occ0" else "flow1"][i, :, y0:y0 + crop_h, x0:x0 + crop_w]
                xs = np.broadcast_to(np.arange(x0, x0 + crop_w)[None, :], (crop_h, crop_w))
                ys = np.broadcast_to(np.arange(y0, y0 + crop_h)[:, None], (crop_h, crop_w))
                inside = _inside(xs, flow[0], x0, crop_w) & _inside(ys, flow[1], y0, crop_h)
                win[0] = np.where((win[0] != 0) | ~inside, np.ones((), a.dtype), win[0])
            if fl & HFLIP:
                win = win[..., ::-1]
            if fl & VFLIP:
                win = win[..., ::-1, :]
            win = np.ascontiguousarray(win)
            if name.startswith("flow"):
                bits = win.view(np.uint32 if a.dtype == np.float32 else np.uint16)
                sign = bits.dtype.type(1 << (8 * bits.dtype.itemsize - 1))
                if fl & HFLIP:
                    bits[0] ^= sign
                if fl & VFLIP:
                    bits[1] ^= sign
            out[i] = win
        dst[name] = out
    return dst, used


def records(W, H, crop_w, crop_h):
    """Nine records: x0 in {0, 1, 2, 3, 5, 7, W - crop_w}, y0 in {0, 1, H - crop_h}, the four flip pairs, and two that lie
    outside the frame and carry unknown flag bits and a non-zero reserved word."""
    return np.array([(0, 0, 0, 0), (1, 1, HFLIP, 0), (2, H - crop_h, VFLIP, 0), (3, 0, HFLIP | VFLIP, 0), (5, 1, 0, 0),
                     (7, H - crop_h, HFLIP, 0), (W - crop_w, 0, VFLIP, 0), (-5, 1 << 30, HFLIP | VFLIP, 77), (W, 1, -1, -1)], np.int32)


_SPECIAL32 = np.array([0x7FC12345, 0xFFC00001, 0x7F800000, 0xFF800000, 0x80000000, 0x477FE000, 0xC77FE000, 0x00000001, 0x80000123],
                      np.uint32)  # NaNs with payloads, +-inf, -0.0, +-65504, float32 denormals
_SPECIAL16 = np.array([0x7E55, 0xFE01, 0x7C00, 0xFC00, 0x8000, 0x7BFF, 0xFBFF, 0x0001, 0x8123], np.uint16)
_planes = {}


def planes(W, H, image="float32", flow="float32", occ="float32", n=N):
    """The eight planes of n samples: frames and labels whose value encodes (sample, channel, y, x) - exactly in float32, by a
    mix of the four modulo 251 in uint8 -, flows with a smooth field and the special bit patterns planted all over (also in
    columns and rows every window covers), occlusion maps that are non-zero in places (values other than 1 among them)."""
    key = (W, H, image, flow, occ, n)
    if key in _planes:
        return _planes[key]
    i, c, y, x = np.meshgrid(np.arange(n), np.arange(3), np.arange(H), np.arange(W), indexing="ij", sparse=True)
    src = {}
    for k, name in enumerate(("image0", "image1")):
        if image == "float32":
            src[name] = ((((i * 3 + c) * H + y) * W + x) * 2 + k).astype(np.float32)
        else:
            src[name] = ((x * 7 + y * 13 + c * 101 + i * 29 + k * 53) % 251).astype(np.uint8)
    for k, name in enumerate(("flow", "flow1")):
        f = (((x * 3 - y * 5 + i * 7) % 41 - 20) * 0.25 + c * 0.125 + k).astype(np.float32)[:, :2]
        f = np.ascontiguousarray(f.astype(flow))
        bits = f.view(np.uint32 if flow == "float32" else np.uint16).reshape(-1)
        special = _SPECIAL32 if flow == "float32" else _SPECIAL16
        at = np.arange(k + 3, bits.size, 7)
        bits[at] = special[np.arange(at.size) % special.size]
        src[name] = f
    for k, name in enumerate(("occ0", "occ1")):
        o = (((x[:, :1] * 5 + y[:, :1] * 3 + i * 11 + k) % 7) == 0)
        src[name] = (o * np.where((x[:, :1] + y[:, :1]) % 2 == 0, 1, 3)).astype(occ) * (np.float32(0.5) if occ == "float32" else 1)
        src[name] = np.ascontiguousarray(src[name].astype(occ))
    for k, name in enumerate(("label0", "label1")):
        src[name] = ((x[:, 0] * 11 + y[:, 0] * 17 + i[:, 0] * 31 + k * 5) % 251).astype(np.uint8)
    for name in src:
        src[name].setflags(write=False)
    _planes[key] = src
    return src


def expect_equal(got, want, what=""):
    """byte for byte, plane by plane (NaNs compare as their bits)"""
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for name in want:
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, b.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            bad = np.argwhere(a.view(np.uint8).reshape(a.shape + (-1,)) != b.view(np.uint8).reshape(b.shape + (-1,)))
            raise AssertionError("%s: %s differs in %d bytes, first at %s" % (what, name, len(bad), bad[0].tolist()))
