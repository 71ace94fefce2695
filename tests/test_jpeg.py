"""CPU tests of the block compression (ofdg_jpeg, include/ofdg.h): ofdg_host_jpeg against the numpy restatement
(tests/jpeg_reference.py) byte for byte and record for record, the in-place form, the tables, what a grey plane keeps, the
independence of the MCUs, the block against the float64 codec, the whole against Pillow's encoder and decoder, the draw, the
sanitising, the refusals, the structs, the loader's option and the sanitizer program."""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest

import jpeg_reference as jr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "optical-flow-2d-data-generation_amd")
FILL = 0xA5
QUALITIES = (1, 10, 50, 90, 100, (50, 0))


def expect_same(got, want, what):
    jr.expect_equal(got[0], want[0], what + ": planes")
    assert jr.equal_bits(got[1], want[1]), "%s: records\n%s\n%s" % (what, got[1], want[1])


# ---- twin against restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", jr.SIZES)
@pytest.mark.parametrize("dst_dtype", ["float32", "uint8"])
@pytest.mark.parametrize("src_dtype", ["float32", "uint8"])
def test_twin_equals_restatement(ofdg, src_dtype, dst_dtype, W, H):
    """Both subsamplings, the phases (0,0), (3,5), (8,8), (15,1), the qualities 1, 10, 50, 90, 100 and {50, 0}; then hostile and
    drawn records.  The float32 sources hold NaN, negatives, values above 255 and halves."""
    src = jr.frames(W, H, src_dtype)
    dt = np.dtype(dst_dtype)
    what = "%dx%d %s to %s" % (W, H, src_dtype, dst_dtype)
    calls = [dict(recs=jr.recs_of(q, sub, phase)) for sub in (0, 1) for phase in jr.PHASES for q in QUALITIES]
    calls += [dict(recs=jr.hostile_records()), dict(ranges=dict(jr.DEFAULT, prob=0.8), seed=11, first_index=2 ** 32 - 1)]
    for k, kw in enumerate(calls):
        for pick in ((0, 1), (0,), (1,)) if k in (3, 30) else ((0, 1),):
            frames = tuple(t if f in pick else None for f, t in enumerate(src))
            got = ofdg.host_jpeg(frames, dst_dtype=dt, **kw)
            expect_same(got, jr.jpeg(frames, dst_dtype=dt, **kw), "%s call %d frames %s" % (what, k, pick))


@pytest.mark.parametrize("W,H", jr.SIZES)
@pytest.mark.parametrize("dtype", ["float32", "uint8"])
def test_in_place_equals_copying(ofdg, dtype, W, H):
    """a frame of quality 0 is left untouched in place: its odd float32 values stay as they are"""
    src = jr.frames(W, H, dtype)
    for sub in (0, 1):
        for phase in jr.PHASES:
            recs = np.array([jr.rec_of(35, sub, phase), jr.rec_of((90, 0), sub, phase), jr.rec_of((0, 5), sub, phase)], jr.REC)
            copied, used = ofdg.host_jpeg(src, recs=recs)
            mine = tuple(np.array(t) for t in src)
            out, used2 = ofdg.host_jpeg(mine, recs=recs, in_place=True)
            assert out[0] is mine[0] and out[1] is mine[1] and jr.equal_bits(used, used2)
            jr.expect_equal(mine, copied, "%dx%d %s sub %d phase %s" % (W, H, dtype, sub, phase))
            assert jr.equal_bits(mine[1][1], src[1][1]) and jr.equal_bits(mine[0][2], src[0][2])
            assert not jr.equal_bits(mine[0][0], src[0][0])


def test_identity_keeps_bits_and_other_format_goes_through_bytes(ofdg):
    odd = jr.frames(24, 10, "float32")
    recs = jr.recs_of(0, 1, (3, 5))
    (o0, o1), _ = ofdg.host_jpeg(odd, recs=recs)
    assert jr.equal_bits(o0, odd[0]) and jr.equal_bits(o1, odd[1]) and np.isnan(o0).any()
    (o0, _), _ = ofdg.host_jpeg(odd, recs=recs, dst_dtype=np.uint8)
    assert np.array_equal(o0, jr.to_bytes(odd[0]).astype(np.uint8))
    # quality 100 is not the identity
    plain = jr.frames(24, 10, "uint8")
    (o0, _), _ = ofdg.host_jpeg(plain, recs=jr.recs_of(100))
    assert not np.array_equal(o0, plain[0]) and np.abs(o0.astype(int) - plain[0]).max() <= 3


# ---- the tables ------------------------------------------------------------------------------------------------------------
def test_tables_known_answers(ofdg):
    luma, chroma = ofdg.host_jpeg_tables(50)
    assert np.array_equal(luma, jr.K1) and np.array_equal(chroma, jr.K2)
    assert luma[0].tolist() == [16, 11, 10, 16, 24, 40, 51, 61] and luma[7].tolist() == [72, 92, 95, 98, 112, 100, 103, 99] and int(luma.sum()) == 3688
    assert chroma[0].tolist() == [17, 18, 24, 47, 99, 99, 99, 99] and chroma[3].tolist() == [47, 66, 99, 99, 99, 99, 99, 99] and int(chroma.sum()) == 5505
    assert all((t == 1).all() for t in ofdg.host_jpeg_tables(100))
    assert ofdg.host_jpeg_tables(10)[0][0, 0] == 80 and ofdg.host_jpeg_tables(1)[0][0, 0] == 255
    for q in range(1, 101):
        for got, want in zip(ofdg.host_jpeg_tables(q), jr.tables(q)):
            assert np.array_equal(got, want) and got.min() >= 1 and got.max() <= 255, q
    lib = ofdg.lib()
    out = np.full(128, 0xA5A5, np.uint16)
    for bad in (0, -1, 101):
        assert lib.ofdg_jpeg_tables(bad, out.ctypes.data, out.ctypes.data + 128) == ofdg.EINVAL
        assert lib.ofdg_host_last_error().decode().startswith("ofdg_jpeg_tables: ") and (out == 0xA5A5).all()
    assert lib.ofdg_jpeg_tables(50, None, out.ctypes.data) == ofdg.EINVAL and lib.ofdg_jpeg_tables(50, out.ctypes.data, None) == ofdg.EINVAL


def pillow_round_trip(bgr, quality):
    """(decoded [3,H,W] B, G, R; the tables Pillow reports) of a 4:4:4 baseline JPEG made in memory"""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[::-1].transpose(1, 2, 0)), "RGB").save(buf, "JPEG", quality=quality, subsampling=0)
    im = Image.open(io.BytesIO(buf.getvalue()))
    q = im.quantization
    return np.asarray(im.convert("RGB")).transpose(2, 0, 1)[::-1], q


def test_tables_equal_pillows(ofdg):
    pytest.importorskip("PIL")
    zigzag = sorted(range(64), key=lambda k: (k // 8 + k % 8, (k // 8 if (k // 8 + k % 8) % 2 else k % 8)))
    for quality in (10, 50, 90):
        _, q = pillow_round_trip(jr.synthetic(), quality)
        for t, mine in zip((0, 1), ofdg.host_jpeg_tables(quality)):
            theirs = list(q[t])
            natural = mine.reshape(-1).tolist()
            # (Pillow reports the tables in natural order since 8.3, in zigzag order before)
            assert theirs == natural or theirs == [natural[k] for k in zigzag], (quality, t)


def test_against_pillow(ofdg):
    """4:4:4, phase 0: the mean absolute difference to the bytes Pillow's encoder and decoder leave is at most 1.0 (measured:
    the printed figures), while the source's own distance to them is several bytes."""
    pytest.importorskip("PIL")
    src = jr.synthetic()
    for quality in (10, 25, 50, 75, 90):
        theirs, _ = pillow_round_trip(src, quality)
        (mine, _), _ = ofdg.host_jpeg((src[None], None), recs=jr.recs_of(quality, n=1))
        (rest, _), _ = jr.jpeg((src[None], None), recs=jr.recs_of(quality, n=1))
        mad = np.abs(mine[0].astype(int) - theirs).mean()
        own = np.abs(src.astype(int) - theirs).mean()
        print("quality %d: mean |twin - Pillow| %.3f, restatement %.3f, mean |source - Pillow| %.3f" % (quality, mad, np.abs(rest[0].astype(int) - theirs).mean(), own))
        assert mad <= 1.0 and np.abs(rest[0].astype(int) - theirs).mean() <= 1.0 and own > 2.0, quality


# ---- what the definition keeps ---------------------------------------------------------------------------------------------
def test_grey_planes_come_back_exactly_at_quality_100(ofdg):
    """B = G = R = c: Y = c and Cb = Cr = 128 by the constants, and a constant block is exact at Q = 1 - every c (one sample
    each), every phase, both subsamplings"""
    frame = np.ascontiguousarray(np.broadcast_to(np.arange(256, dtype=np.uint8)[:, None, None, None], (256, 3, 18, 24)))
    for sub in (0, 1):
        for px in range(16):
            for py in (range(16) if px in (0, 7, 15) else (px,)):
                (out, _), _ = ofdg.host_jpeg((frame, None), recs=jr.recs_of(100, sub, (px, py), 256))
                assert np.array_equal(out, frame), (sub, px, py)


@pytest.mark.parametrize("sub", [0, 1])
def test_blocks_are_independent(ofdg, sub):
    """one changed pixel changes bytes inside its MCU only, at every phase of a row of the grid"""
    W, H, M = 40, 26, 16 if sub else 8
    base = jr.frames(W, H, "uint8", n=1)[0]
    for py in (0, 5):
        for px in range(16):
            recs = jr.recs_of(60, sub, (px, py), 1)
            (want, _), _ = ofdg.host_jpeg((base, None), recs=recs)
            for x, y in ((0, 0), (17, 9), (W - 1, H - 1), (23, 16)):
                other = np.array(base)
                other[0, :, y, x] ^= 0x80
                (got, _), _ = ofdg.host_jpeg((other, None), recs=recs)
                ex, ey = (px if sub else px & 7), (py if sub else py & 7)
                x0, y0 = (x + ex) // M * M - ex, (y + ey) // M * M - ey
                changed = np.argwhere((got != want).any(axis=(0, 1)))
                assert len(changed) and (changed[:, 0] >= y0).all() and (changed[:, 0] < y0 + M).all(), (px, py, x, y)
                assert (changed[:, 1] >= x0).all() and (changed[:, 1] < x0 + M).all(), (px, py, x, y)


def float_blocks():
    rng = np.random.RandomState(17)
    k = 40
    y, x = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    kinds = dict(random=rng.randint(0, 256, (k, 8, 8)), low_contrast=rng.randint(0, 256, (k, 1, 1)) // 2 + 60 + rng.randint(-4, 5, (k, 8, 8)),
                 two_level=np.where(rng.randint(0, 2, (k, 8, 8)) > 0, rng.randint(128, 256, (k, 1, 1)), rng.randint(0, 128, (k, 1, 1))),
                 ramp=np.clip(rng.randint(0, 256, (k, 1, 1)) + rng.randint(-16, 17, (k, 1, 1)) * x + rng.randint(-16, 17, (k, 1, 1)) * y, 0, 255))
    extreme = np.stack([np.zeros((8, 8), int), np.full((8, 8), 255), ((x + y) & 1) * 255, (x & 1) * 255, (y >= 4) * 255, 255 - ((x + y) & 1) * 255])
    return dict(kinds, extreme=extreme)


def test_block_against_float64(ofdg):
    """ofdg_host_jpeg_block = the restatement's integer codec, and against the orthonormal float64 DCT with round-half-away
    quantisation: every level within 1; in a block whose levels all agree every byte within 1; at most 3 % of levels differ
    (a prototype of this arithmetic measured at most 1.9 %, at quality 100)."""
    blocks = float_blocks()
    worst = 0.0
    for quality in (1, 10, 25, 50, 75, 90, 95, 100):
        levels = differ = 0
        for t, table in enumerate(ofdg.host_jpeg_tables(quality)):
            Q = table.astype(np.int64)
            for kind, stack in blocks.items():
                want_l, want_o = jr.codec(stack, Q)
                flo_l, flo_o = jr.codec_float(stack, Q)
                for k, block in enumerate(stack):
                    got_l, got_o = ofdg.host_jpeg_block(block, table)
                    what = (quality, t, kind, k)
                    assert np.array_equal(got_l, want_l[k]) and np.array_equal(got_o, want_o[k]), what
                    assert np.abs(got_l - flo_l[k]).max() <= 1, what
                    off = int((got_l != flo_l[k]).sum())
                    if not off:
                        assert np.abs(got_o.astype(int) - flo_o[k]).max() <= 1, what
                    levels, differ = levels + 64, differ + off
        print("quality %3d: %.2f %% of %d levels differ from the float64 codec" % (quality, 100.0 * differ / levels, levels))
        worst = max(worst, differ / levels)
        assert differ <= 0.03 * levels, quality
    lib = ofdg.lib()
    block, out, q = np.zeros(64, np.uint8), np.full(64, FILL, np.uint8), np.ones(64, np.uint16)
    for bad in (0, 256):
        q[63] = bad
        assert lib.ofdg_host_jpeg_block(block.ctypes.data, q.ctypes.data, None, out.ctypes.data) == ofdg.EINVAL and (out == FILL).all()
    q[63] = 255
    assert lib.ofdg_host_jpeg_block(block.ctypes.data, q.ctypes.data, None, out.ctypes.data) == ofdg.OK and (out == 0).all()
    assert lib.ofdg_host_jpeg_block(None, q.ctypes.data, None, out.ctypes.data) == ofdg.EINVAL
    assert lib.ofdg_host_jpeg_block(block.ctypes.data, None, None, out.ctypes.data) == ofdg.EINVAL
    assert lib.ofdg_host_jpeg_block(block.ctypes.data, q.ctypes.data, None, None) == ofdg.EINVAL


def test_intermediates_fit_32_bits(ofdg):
    """the largest magnitude of any sum over the extreme blocks is below 2^28 in the restatement, which computes in int64, and
    the library's 32-bit passes give the restatement's levels and bytes on those blocks at every uniform Q of 1, 2, 16, 255 (the
    sanitizer program runs the same blocks under UBSan, where a signed overflow is a report)"""
    stack = float_blocks()["extreme"]
    p = stack.astype(np.int64) - 128
    for Q in (1, 2, 16, 255):
        A = p @ jr.T.T
        A1 = (A + 256) >> 9
        F = jr.T @ A1
        level = np.sign(F) * ((np.abs(F) + Q * 65536) // (Q * 131072))
        B = jr.T.T @ (level * Q)
        P = ((B + 256) >> 9) @ jr.T
        assert max(int(np.abs(v).max()) for v in (A, F, np.abs(F) + Q * 65536, B, P)) < 2 ** 28
        want_l, want_o = jr.codec(stack, np.full((8, 8), Q, np.int64))
        for k, block in enumerate(stack):
            got_l, got_o = ofdg.host_jpeg_block(block, np.full((8, 8), Q, np.uint16))
            assert np.array_equal(got_l, want_l[k]) and np.array_equal(got_o, want_o[k]), (Q, k)


# ---- the draw --------------------------------------------------------------------------------------------------------------
def test_draw(ofdg):
    n = 3000
    recs = np.array([ofdg.jpeg_draw(7, 1000 + i, jr.DEFAULT) for i in range(n)])
    again = np.array([ofdg.jpeg_draw(7, 1000 + i, jr.DEFAULT) for i in range(0, n, 97)])
    assert jr.equal_bits(recs[::97], again), "not a pure function of (seed, index)"
    assert jr.equal_bits(recs[:50], jr.drawn_records(7, 1000, 50, jr.DEFAULT))
    # three known answers
    always = dict(jr.DEFAULT, prob=1.0)
    for (seed, index), want in (((7, 0), ((38, 36), 1, 0, 6)), ((7, 1), ((40, 45), 0, 14, 1)), ((11, 2 ** 32 + 5), ((85, 83), 1, 1, 8))):
        r = ofdg.jpeg_draw(seed, index, always)
        assert (tuple(r["quality"].tolist()), int(r["subsample"]), int(r["phase_x"]), int(r["phase_y"])) == want and not r["reserved"].any(), (seed, index, r)
        assert jr.equal_bits(r, jr.draw(seed, index, always))
    assert not jr.equal_bits(ofdg.jpeg_draw(8, 1000, jr.DEFAULT), recs[0]) and not jr.equal_bits(recs[0], recs[1])
    on = recs["quality"][:, 0] > 0
    q0, q1 = recs["quality"][on, 0], recs["quality"][on, 1]
    assert q0.min() == 30 and q0.max() == 95 and (np.abs(q1 - q0) <= 5).all() and (q1 != q0).any() and (recs["quality"][~on] == 0).all()
    assert abs(on.mean() - 0.5) <= 5 * np.sqrt(0.25 / n) and abs(recs["subsample"].mean() - 0.5) <= 5 * np.sqrt(0.25 / n)
    assert set(recs["phase_x"].tolist()) == set(range(16)) and set(recs["phase_y"].tolist()) == set(range(16)) and not recs["reserved"].any()
    # prob 0: never; q1 never leaves 1..100; no phase without the flag; a fixed subsampling is kept
    recs = np.array([ofdg.jpeg_draw(5, i, dict(jr.DEFAULT, prob=0.0)) for i in range(500)])
    assert not recs["quality"].any()
    for lo, hi in ((1, 3), (98, 100)):
        recs = np.array([ofdg.jpeg_draw(5, i, dict(prob=1.0, quality_min=lo, quality_max=hi, quality_delta=99, subsample=1)) for i in range(2000)])
        assert recs["quality"].min() == 1 and recs["quality"].max() == 100 and set(recs["quality"][:, 0].tolist()) == set(range(lo, hi + 1))
        assert (recs["subsample"] == 1).all() and not recs["phase_x"].any() and not recs["phase_y"].any()
    recs = np.array([ofdg.jpeg_draw(5, i, dict(prob=1.0, subsample=0, sub_prob=1.0)) for i in range(100)])
    assert (recs["subsample"] == 0).all() and (recs["quality"] == 75).all()
    for ranges in (None, {}):
        r = ofdg.jpeg_draw(3, 12345, ranges)
        assert r["quality"].tolist() == [0, 0] and r["subsample"] == 0 and r["phase_x"] == 0
    frame = jr.frames(24, 10, "uint8")
    (o0, o1), _ = ofdg.host_jpeg(frame, ranges={}, seed=3, first_index=9)
    assert np.array_equal(o0, frame[0]) and np.array_equal(o1, frame[1])
    with pytest.raises(ValueError, match="unknown range"):
        ofdg.jpeg_draw(1, 1, dict(quality=50))


def test_given_records_are_sanitised_as_stated(ofdg):
    src = jr.frames(24, 10, "uint8")
    _, used = ofdg.host_jpeg(src, recs=jr.hostile_records())
    assert used["quality"].tolist() == [[0, 100], [100, 0], [60, 100]] and used["subsample"].tolist() == [0, 0, 0]
    assert used["phase_x"].tolist() == [0, 0, 15] and used["phase_y"].tolist() == [0, 0, 15] and not used["reserved"].any()
    # each limit at the bound and beyond
    for field, cases in (("quality", ((0, 0), (100, 100), (-1, 0), (101, 100))), ("subsample", ((0, 0), (1, 1), (-1, 0), (2, 0))),
                         ("phase_x", ((0, 0), (15, 15), (-1, 0), (16, 0))), ("phase_y", ((0, 0), (15, 15), (-1, 0), (16, 0)))):
        for given, want in cases:
            recs = jr.recs_of(50, 1, (4, 4))
            recs[field] = given
            _, used = ofdg.host_jpeg(src, recs=recs)
            assert (used[field] == want).all() and jr.equal_bits(used, jr.sanitise(recs)), (field, given)


# ---- refusals, structs, the loader's option, the sanitizer program ---------------------------------------------------------
def test_refusals_write_nothing(ofdg):
    W, H, n = 24, 10, 2
    lib = ofdg.lib()
    plane = n * H * W
    src = [np.zeros((n, 3, H, W), np.uint8) for _ in range(2)]
    raw = np.full(6 * plane + 32 * n + 64, FILL, np.uint8)   # everything written: two uint8 frames, then the records
    base = raw.ctypes.data
    recs_in = np.array([jr.rec_of(100, 1, (3, 5))] * n, jr.REC)   # (a grey plane is exact at quality 100)

    def job(**kw):
        j = ofdg.JpegJob()
        for f in range(2):
            j.src[f], j.dst[f] = src[f].ctypes.data, base + 3 * plane * f
        j.recs_out = base + 6 * plane
        j.src_fmt, j.dst_fmt = ofdg.FMT_U8, ofdg.FMT_U8
        j.quality_min, j.quality_max, j.quality_delta, j.prob, j.sub_prob, j.subsample, j.flags = 30, 95, 5, 0.5, 0.5, -1, ofdg.JPEG_PHASE
        for k, v in kw.items():
            if isinstance(v, dict):
                for idx, val in v.items():
                    getattr(j, k)[idx] = val
            else:
                setattr(j, k, v)
        return j

    def refused(word, j, n_samples=n, w=W, h=H):
        rc = lib.ofdg_host_jpeg(None if j is None else C.byref(j), n_samples, w, h)
        assert rc == ofdg.EINVAL, word
        msg = lib.ofdg_host_last_error().decode()
        assert msg.startswith("ofdg_host_jpeg: ") and word in msg, (word, msg)
        assert (raw == FILL).all(), word

    refused("job", None)
    refused("n_samples", job(), n_samples=0)
    refused("plane size given", job(width=W))
    refused("plane size given", job(width=W + 8, height=H))
    for bad_w, bad_h in ((20, 10), (24, 9), (4, 2), (8, 0)):
        refused("width", job(), w=bad_w, h=bad_h)
    refused("2^32", job(), n_samples=1, w=65536, h=32768)
    refused("src_fmt", job(src_fmt=ofdg.FMT_F16))
    refused("dst_fmt", job(dst_fmt=7))
    for bad in (2, 3, -1):
        refused("flags", job(flags=bad))
    refused("reserved", job(reserved={0: 1}))
    refused("reserved", job(reserved={1: -1}))
    for name in ("quality_min", "quality_max"):
        for bad in (0, 101, -2 ** 31, 2 ** 31 - 1):
            refused(name, job(**{name: bad}))
    refused("quality_min must not be above quality_max", job(quality_min=96))
    for bad in (-1, 100):
        refused("quality_delta", job(quality_delta=bad))
    for name in ("prob", "sub_prob"):
        for bad in (float("nan"), -0.001, float("inf"), np.nextafter(np.float32(1), np.float32(9))):
            refused(name, job(**{name: bad}))
    for bad in (-2, 2):
        refused("subsample", job(subsample=bad))
    refused("no frame is set", job(src={0: None, 1: None}, dst={0: None, 1: None}))
    refused("source and no destination", job(dst={1: None}))
    refused("destination and no source", job(src={0: None}))
    refused("overlaps", job(dst={1: base + 3 * plane - 1}))
    refused("overlaps", job(recs_out=base + 6 * plane - 1))
    refused("overlaps", job(dst={0: src[1].ctypes.data + 16}))
    refused("overlaps", job(recs=base + 6 * plane + 32))
    refused("overlaps", job(dst={0: base, 1: base}))
    refused("overlaps", job(src={0: base}, dst={0: base}, dst_fmt=ofdg.FMT_F32))   # in place, in another format
    refused("overlaps", job(src={0: base + 1}, dst={0: base}))                      # a partial overlap
    refused("overlaps", job(src={0: base, 1: base}, dst={0: base, 1: base}))        # both frames in place on one buffer
    # the bounds themselves pass: the limits of each range, then the in-place form
    for kw in (dict(quality_min=1, quality_max=100, quality_delta=99, prob=1.0, sub_prob=1.0, subsample=1, flags=0),
               dict(quality_min=100, quality_max=100, quality_delta=0, prob=0.0, sub_prob=0.0, subsample=-1)):
        scratch = np.zeros(6 * plane + 32 * n, np.uint8)
        ok = job(dst={0: scratch.ctypes.data, 1: scratch.ctypes.data + 3 * plane}, recs_out=scratch.ctypes.data + 6 * plane, **kw)
        assert lib.ofdg_host_jpeg(C.byref(ok), n, W, H) == ofdg.OK, lib.ofdg_host_last_error()
    out = np.full(32, FILL, np.uint8)
    for name, bad in (("quality_min", 0), ("quality_max", 101), ("quality_delta", 100), ("prob", 1.5), ("sub_prob", -1.0), ("subsample", 2), ("flags", 2)):
        assert lib.ofdg_jpeg_draw(1, 0, C.byref(job(**{name: bad})), out.ctypes.data_as(C.POINTER(ofdg.JpegRec))) == ofdg.EINVAL
        msg = lib.ofdg_host_last_error().decode()
        assert msg.startswith("ofdg_jpeg_draw: ") and name in msg and (out == FILL).all()
    assert lib.ofdg_jpeg_draw(1, 0, None, out.ctypes.data_as(C.POINTER(ofdg.JpegRec))) == ofdg.EINVAL
    assert lib.ofdg_jpeg_draw(1, 0, C.byref(job()), None) == ofdg.EINVAL and (out == FILL).all()
    # the host twin asks no alignment; the job's own size; one frame, records given, at an odd address; then in place
    src[1][:] = 200
    ok = job(src={0: None}, dst={0: None, 1: base + 1}, recs=recs_in.ctypes.data, width=W, height=H)
    assert lib.ofdg_host_jpeg(C.byref(ok), n, W, H) == ofdg.OK, lib.ofdg_host_last_error()
    assert (raw[1:1 + 3 * plane] == 200).all() and raw[0] == FILL and (raw[1 + 3 * plane:6 * plane] == FILL).all() and (raw[6 * plane + 32 * n:] == FILL).all()
    used = raw[6 * plane:6 * plane + 32 * n].view(jr.REC)
    assert used["quality"].tolist() == [[100, 100]] * n and used["subsample"].tolist() == [1] * n and used["phase_y"].tolist() == [5] * n
    ok = job(src={0: None, 1: base + 1}, dst={0: None, 1: base + 1}, recs=recs_in.ctypes.data)
    assert lib.ofdg_host_jpeg(C.byref(ok), n, W, H) == ofdg.OK, lib.ofdg_host_last_error()
    assert (raw[1:1 + 3 * plane] == 200).all() and raw[0] == FILL


def test_struct_layout_and_contract(ofdg):
    J, R = ofdg.JpegJob, ofdg.JpegRec
    assert C.sizeof(R) == 32 and C.sizeof(J) == 112 and jr.REC.itemsize == 32 and ofdg._jpeg_rec_dtype() == jr.REC
    offsets = dict(quality=0, subsample=8, phase_x=12, phase_y=16, reserved=20)
    assert {name: getattr(R, name).offset for name, _ in R._fields_} == offsets and {k: jr.REC.fields[k][1] for k in jr.REC.names} == offsets
    assert {name: getattr(J, name).offset for name, _ in J._fields_} == dict(
        src=0, dst=16, recs=32, recs_out=40, first_index=48, seed=56, width=60, height=64, src_fmt=68, dst_fmt=72, flags=76, subsample=80,
        quality_min=84, quality_max=88, quality_delta=92, prob=96, sub_prob=100, reserved=104)
    assert (ofdg.JPEG_REC_WORDS, ofdg.JPEG_PHASE) == (8, 1)
    assert ofdg.JPEG_RANGES == ("quality_min", "quality_max", "quality_delta", "prob", "sub_prob", "subsample", "phase") and ofdg.JPEG_DEFAULT == jr.DEFAULT
    hdr = open(os.path.join(ROOT, "include", "ofdg.h")).read()
    for fn in ("ofdg_jpeg", "ofdg_host_jpeg", "ofdg_jpeg_draw", "ofdg_jpeg_tables", "ofdg_host_jpeg_block"):
        assert "int %s(" % fn in hdr and fn in ofdg.EXPORTS and hasattr(ofdg.lib(), fn)
    assert "#define OFDG_JPEG_PHASE 1" in hdr and "0x0c7b" in hdr and "Quality 100 is NOT the identity" in hdr
    dev = open(os.path.join(PKG, "csrc", "ofdg_device.h")).read()
    assert "sizeof(DevJpegRec) == 32" in dev and "sizeof(DevJpegJob) == 112" in dev and "0x0c7bu" in dev
    # the literal transform table of the shared header is the one of the formula
    literal = dev[dev.index("constexpr int32_t kJpegT[64] = {"):]
    literal = literal[literal.index("{") + 1:literal.index("}")]
    assert [int(v) for v in literal.split(",")] == jr.T.reshape(-1).tolist()
    a = np.arange(16, dtype=np.int32).reshape(2, 8)
    s = ofdg.jpeg_numpy(a)
    assert s.shape == (2,) and s[1]["quality"].tolist() == [8, 9] and int(s[0]["subsample"]) == 2 and int(s[0]["phase_y"]) == 4
    with pytest.raises(ValueError, match="32 bytes"):
        ofdg.jpeg_numpy(np.zeros(5, np.int32))


def test_flowloader_option_needs_no_gpu(ofdg):
    opts = ofdg.FlowLoader._jpeg_options
    assert opts(None) is None and opts(ofdg.JPEG_DEFAULT) == ofdg.JPEG_DEFAULT and opts({}) == {}
    with pytest.raises(ValueError, match="unknown range"):
        opts(dict(quality=50))
    slots = list(ofdg._RingSlot.__slots__)
    assert "jpeg" in slots
    doc = ofdg.FlowLoader.__doc__
    assert "jpeg=" in doc and doc.index("9. jitter=          in place") < doc.index("10. jpeg=           in place") < doc.index("11. erase=           in place")
    assert "16. pack=" in doc


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="the sanitizer build belongs on the CPU machine")
def test_sanitizer_program_passes_the_jpeg_mode():
    """make san builds tools/host_input_check.cpp with ASan + UBSan; its jpeg mode runs ofdg_host_jpeg, ofdg_jpeg_draw,
    ofdg_jpeg_tables and ofdg_host_jpeg_block on exactly sized heap buffers: hostile records, the five sizes, every format pair,
    both subsamplings, the in-place form and every refusal."""
    subprocess.run(["make", "-s", "-C", PKG, "san"], check=True, timeout=600)
    run = subprocess.run([os.path.join(PKG, "build", "san", "host_input_check"), "jpeg"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "jpeg calls=" in run.stdout
