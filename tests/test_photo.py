"""CPU tests of the photometric augmentation (ofdg_photo_draw, ofdg_host_photo, ofdg_host_photo_table, ofdg_det_log;
include/ofdg.h, include/ofdg_detmath.h): the host twin against the numpy restatement (tests/photo_reference.py) byte for byte,
the identity record, the logarithm against libm, tables, the draw against the restatement and recorded answers, composition
of batches, the noise's moments and every refusal.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import photo_reference as pr


@pytest.mark.parametrize("W,H", pr.SIZES)
@pytest.mark.parametrize("src_dtype,dst_dtype", pr.PAIRS)
def test_host_photo_equals_restatement(ofdg, W, H, src_dtype, dst_dtype):
    """Records at every clamp edge, beyond it, NaN and infinite; float32 inputs with NaN, -3, 255.5, 1e9, ties and infinities."""
    src = pr.frames(W, H, src_dtype)
    recs = pr.records()
    want, want_recs = pr.photo(src, recs, seed=7, dst_dtype=dst_dtype)
    got, got_recs = ofdg.host_photo(src, recs=recs, seed=7, dst_dtype=dst_dtype)
    pr.expect_equal(got, want, "%dx%d %s to %s" % (W, H, src_dtype, dst_dtype))
    assert pr.equal_bits(got_recs, want_recs)
    if src_dtype == "float32":
        flat = src[0].reshape(-1)
        assert np.isnan(flat).any() and all((flat == v).any() for v in (-3.0, 255.5, 1e9, np.inf))
    # what the sanitising made of the records: edges kept, beyond them clamped, NaN to the identity, reserved cleared
    assert pr.equal_bits(got_recs[2], recs[2]) and pr.equal_bits(got_recs[3], recs[3]) and pr.equal_bits(got_recs[5], pr.IDENTITY)
    assert got_recs[4].tolist() == [0.125, 8.0, 0.0, 4.0, -1.0, 1.0, 0.0, 8.0, 1.0, 1.0, 1.0, 1.0, 0.0, 64.0, 0.0, 0.0]
    assert got_recs[6].tolist() == [8.0, 0.125, 4.0, 0.0, 1.0, -1.0, 8.0, 0.0, 8.0, 1.0, 0.0, 1.0, 64.0, 0.0, 0.0, 0.0]
    assert got_recs[7].view(np.int32)[14:].tolist() == [0, 0] and np.signbit(got_recs[7][2]) and np.signbit(got_recs[7][12])
    # one frame alone gives that frame's bytes
    only1, _ = ofdg.host_photo((None, src[1]), recs=recs, seed=7, dst_dtype=dst_dtype)
    pr.expect_equal(only1, (None, want[1]), "frame 1 alone")


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_identity_record_changes_nothing(ofdg, dtype):
    src = pr.frames(160, 100, "uint8")
    src = tuple(t.astype(dtype) for t in src)  # (float32: the byte values, what the generator stores)
    recs = np.tile(pr.IDENTITY, (pr.N, 1))
    got, used = ofdg.host_photo(src, recs=recs)
    pr.expect_equal(got, src, "identity %s" % dtype)
    assert pr.equal_bits(used, recs)
    drawn, used = ofdg.host_photo(src, seed=99, first_index=1 << 40, ranges={})  # all ranges 0: the identity record drawn
    pr.expect_equal(drawn, src, "identity drawn")
    assert pr.equal_bits(used, recs)
    work = tuple(np.array(t) for t in src)
    same, _ = ofdg.host_photo(work, recs=recs, in_place=True)
    assert same[0] is work[0] and same[1] is work[1]
    pr.expect_equal(work, src, "identity in place")
    other = ofdg.host_photo(src, recs=recs, dst_dtype=np.uint8 if dtype == "float32" else np.float32)[0]
    assert all(np.array_equal(a.astype(np.float32), b.astype(np.float32)) for a, b in zip(other, src))


def test_in_place_equals_copy(ofdg):
    for dtype in ("uint8", "float32"):
        src = pr.frames(160, 100, dtype)
        want, _ = ofdg.host_photo(src, recs=pr.records(), seed=3)
        work = tuple(np.array(t) for t in src)
        ofdg.host_photo(work, recs=pr.records(), seed=3, in_place=True)
        pr.expect_equal(work, want, "in place %s" % dtype)


def test_det_log_against_libm(ofdg):
    """The stated bound of ofdg_det_log (include/ofdg_detmath.h): relative error below 2^-50, against libm's log (itself
    within 1 ulp, 2^-53 relative)."""
    rng = np.random.default_rng(5)
    x = np.concatenate([np.arange(1, 256) / 255.0, rng.uniform(2.0 ** -20, 2.0, 200000), np.exp(rng.uniform(-700.0, 700.0, 200000)),
                        np.linspace(0.7, 1.42, 20001), 1.0 + np.ldexp(1.0, -np.arange(1, 53)), 1.0 - np.ldexp(1.0, -np.arange(1, 54)),
                        [1.0 / 255.0, 1.0, 2.2250738585072014e-308, 1.7976931348623157e308, math.sqrt(0.5), math.sqrt(2.0), 0.5, 2.0]])
    got = ofdg.host_det_log(x)
    want = np.array([math.log(v) for v in x])
    assert got[-7] == 0.0 and np.array_equal(got == 0.0, want == 0.0)
    err = np.abs(got - want)
    bound = np.abs(want) * 2.0 ** -50
    assert (err <= bound).all(), (x[(err > bound)][:5], (err / np.abs(want)).max())
    assert np.array_equal(pr.det_log(x), got)  # the restatement, bit for bit
    special = ofdg.host_det_log([0.0, -0.0, -1.0, np.inf, np.nan, 5e-324])
    assert special[0] == -np.inf and special[1] == -np.inf and np.isnan(special[2]) and special[3] == np.inf and np.isnan(special[4])
    assert abs(special[5] - math.log(5e-324)) <= abs(math.log(5e-324)) * 2.0 ** -50


def record_with(**kw):
    r = pr.IDENTITY.copy()
    for key, v in kw.items():
        at = dict(gamma=pr.GAMMA, contrast=pr.CONTRAST, brightness=pr.BRIGHTNESS, sigma=pr.SIGMA)[key]
        r[at:at + 2] = v
    return r


def test_host_photo_table(ofdg):
    t = ofdg.host_photo_table(pr.IDENTITY)
    assert t.shape == (2, 3, 256) and all(np.array_equal(t[f, c], np.arange(256, dtype=np.float32)) for f in range(2) for c in range(3))
    assert pr.equal_bits(pr.table(pr.IDENTITY), t)
    for gamma in (0.125, 1.0, 8.0):
        rec = record_with(gamma=(gamma, 1.0 / gamma if gamma != 1.0 else 1.0))
        got = ofdg.host_photo_table(rec)
        assert pr.equal_bits(got, pr.table(rec)), gamma
        want = 255.0 * (np.arange(256) / 255.0) ** gamma
        assert np.abs(got[0, 1] - want).max() < 1e-4 and got[0, 0, 0] == 0.0 and got[0, 2, 255] == 255.0
        assert (np.diff(got[0, 0]) >= 0).all()
    for rec in pr.records():
        assert pr.equal_bits(ofdg.host_photo_table(rec), pr.table(rec))
    assert ofdg.lib().ofdg_host_photo_table(None, None) == ofdg.EINVAL and "NULL" in ofdg.lib().ofdg_host_last_error().decode()


# seed 12345, PHOTO_FLOWNET: index -> gamma[0], gamma[1], contrast[0], brightness[0], gain[0][0], gain[1][2], sigma[0] (recorded)
KNOWN = {
    0: ("0x1.9b41dcp-1", "0x1.8a248ap-1", "0x1.3aca68p-1", "0x1.697bcp-4", "0x1.ecd804p-1", "0x1.133f74p+0", "0x1.c3442ep+1"),
    1: ("0x1.977384p-1", "0x1.9de322p-1", "0x1.39c5dcp-1", "0x1.3b3166p-5", "0x1.bb12f8p-1", "0x1.5f2114p+0", "0x1.e17fd4p+2"),
    2: ("0x1.7081e2p+0", "0x1.7bb90ep+0", "0x1.c19ef4p+0", "-0x1.2f391p-4", "0x1.26e3a2p+0", "0x1.687464p-1", "0x1.c49be4p+2"),
    (1 << 32) + 3: ("0x1.ddd76p-1", "0x1.d3b278p-1", "0x1.b994d6p+0", "-0x1.7adf8ep-4", "0x1.98ec68p-1", "0x1.d3bd1ep-1", "0x1.dc2bfp+2"),
}


@pytest.mark.parametrize("index", [0, (1 << 32) + 3, 1, 2])
def test_photo_draw(ofdg, index):
    got = ofdg.photo_draw(12345, index, ofdg.PHOTO_FLOWNET)
    assert pr.equal_bits(got, pr.draw(12345, index, ofdg.PHOTO_FLOWNET))
    assert [float(got[k]) for k in (0, 1, 2, 4, 6, 11, 12)] == [float.fromhex(v) for v in KNOWN[index]]
    assert got[12] == got[13] and got[14] == 0 and got[15] == 0
    q = ofdg.PHOTO_FLOWNET
    assert math.exp(-q["gamma_log"]) <= got[0] <= math.exp(q["gamma_log"]) and 0 <= got[12] < q["sigma_max"]
    assert abs(math.log(got[1] / got[0])) <= q["pair_gamma_log"] * 1.0001 and abs(got[5] - got[4]) <= q["pair_brightness"] * 1.0001
    ratios = [math.log(got[9 + c] / got[6 + c]) for c in range(3)]  # one delta of the colour gain for the three channels
    assert max(ratios) - min(ratios) < 1e-6 and abs(ratios[0]) <= q["pair_colour_log"] * 1.0001
    assert pr.equal_bits(ofdg.photo_draw(12345, index, {}), pr.IDENTITY)
    assert set(ofdg.PHOTO_FLOWNET) == set(ofdg.PHOTO_RANGES) == set(pr.RANGES)


def test_photo_draw_refusals(ofdg):
    lib = ofdg.lib()
    out = np.zeros(16, np.float32)
    assert lib.ofdg_photo_draw(1, 0, None, out.ctypes.data) == ofdg.EINVAL and "NULL" in lib.ofdg_host_last_error().decode()
    for name in ofdg.PHOTO_RANGES:
        for bad in (-0.5, float("nan"), float("inf")):
            with pytest.raises(ofdg.OfdgError, match=name):
                ofdg.photo_draw(1, 0, {name: bad})
    with pytest.raises(ValueError, match="unknown range"):
        ofdg.photo_draw(1, 0, {"gama": 1.0})


def test_batches_compose(ofdg):
    """Six samples in one call are two and four with first_index advanced: records and noise follow the global index."""
    src = pr.frames(160, 100, "uint8", n=6)
    kw = dict(seed=21, ranges=ofdg.PHOTO_FLOWNET)
    whole, recs = ofdg.host_photo(src, first_index=(1 << 32) + 1, **kw)
    a, ra = ofdg.host_photo(tuple(t[:2] for t in src), first_index=(1 << 32) + 1, **kw)
    b, rb = ofdg.host_photo(tuple(t[2:] for t in src), first_index=(1 << 32) + 3, **kw)
    pr.expect_equal(tuple(np.concatenate(p) for p in zip(a, b)), whole)
    assert pr.equal_bits(np.concatenate([ra, rb]), recs)
    assert pr.equal_bits(recs, pr.sanitise(pr.drawn_records(21, (1 << 32) + 1, 6, ofdg.PHOTO_FLOWNET)))
    pr.expect_equal(whole, pr.photo(src, recs, seed=21, first_index=(1 << 32) + 1)[0], "against the restatement")
    assert len({r.tobytes() for r in recs}) == 6 and not np.array_equal(whole[0], src[0]) and not np.array_equal(whole[0][0], whole[1][0])


def test_noise_moments(ofdg):
    """One 160x100 frame of mid-grey with sigma 8, identity otherwise, float32 out: 48000 elements a frame.  The byte sum is an
    Irwin-Hall variable of four uniform bytes: mean 0, variance sigma^2 = 64, excess kurtosis -1.2 / 4 (up to the discreteness
    of a byte: 1e-5), so the standard error of the mean is 8 / sqrt(n) and that of the variance 64 sqrt((2 - 0.3) / n); nothing
    reaches the clamps (the sum ends at 8 * 510 / 147.8 = 27.6 from the mean).  Seed 2024: 0.6 and 0.3 standard errors in frame
    0, 0.6 and 1.3 in frame 1."""
    grey = np.full((1, 3, 100, 160), 128, np.uint8)
    (f0, f1), _ = ofdg.host_photo((grey, grey), recs=record_with(sigma=8.0)[None], seed=2024, dst_dtype=np.float32)
    n = f0.size
    for f in (f0, f1):
        d = f.astype(np.float64) - 128.0
        assert abs(d.mean()) <= 6 * 8.0 / math.sqrt(n), d.mean()
        assert abs(d.var() - 64.0) <= 6 * 64.0 * math.sqrt(1.7 / n), d.var()
        assert np.abs(d).max() < 27.7 and len(np.unique(d)) > 500
    assert not np.array_equal(f0, f1)
    as_bytes = ofdg.host_photo((grey, None), recs=record_with(sigma=8.0)[None], seed=2024)[0][0]
    assert np.array_equal(as_bytes, np.rint(f0).astype(np.uint8))
    quiet = ofdg.host_photo((grey, None), recs=record_with(sigma=0.0)[None], seed=2024)[0][0]
    assert np.array_equal(quiet, grey)


GUARD, FILL = 64, 0xA5


def test_refusals_write_nothing(ofdg):
    W, H, n = 16, 4, 2
    lib = ofdg.lib()
    size = n * 3 * H * W
    raw = {k: np.full(GUARD + 4 * size + GUARD, FILL, np.uint8) for k in ("s0", "s1", "d0", "d1")}
    rraw = {k: np.full(GUARD + 64 * n + GUARD, FILL, np.uint8) for k in ("recs", "out")}
    at = {k: v.ctypes.data + GUARD for k, v in dict(raw, **rraw).items()}

    def job(**kw):
        j = ofdg.PhotoJob()
        j.src[0], j.src[1], j.dst[0], j.dst[1], j.recs, j.recs_out = at["s0"], at["s1"], at["d0"], at["d1"], at["recs"], at["out"]
        j.src_fmt = j.dst_fmt = ofdg.FMT_F32
        for k, v in kw.items():
            if k in ("src", "dst"):
                for idx, val in v.items():
                    getattr(j, k)[idx] = val
            else:
                setattr(j, k, v)
        return j

    def refused(word, j, n_samples=n, width=W, height=H):
        assert lib.ofdg_host_photo(None if j is None else C.byref(j), n_samples, width, height) == ofdg.EINVAL, word
        msg = lib.ofdg_host_last_error().decode()
        assert msg.startswith("ofdg_host_photo: ") and word in msg, (word, msg)
        assert all((v == FILL).all() for v in list(raw.values()) + list(rraw.values())), word

    refused("job", None)
    refused("n_samples", job(), n_samples=0)
    refused("no frame", job(src={0: None, 1: None}, dst={0: None, 1: None}))
    refused("dst", job(dst={1: None}))
    refused("src", job(src={0: None}))
    refused("src_fmt", job(src_fmt=ofdg.FMT_F16))
    refused("dst_fmt", job(dst_fmt=5))
    refused("flags", job(flags=1))
    refused("reserved", job(reserved=-1))
    for name in ofdg.PHOTO_RANGES:
        for bad in (-1.0, float("nan"), float("inf")):
            refused(name, job(**{name: bad}))
    for bad_w, bad_h in ((12, 4), (16, 3), (0, 4), (16, 0), (-8, 4)):
        refused("width", job(), width=bad_w, height=bad_h)
    refused("width", job(width=W))          # one of the job's two set
    refused("width", job(width=8, height=4))  # the job's own size is not the plane's
    refused("2^32", job(), n_samples=1, width=65536, height=21846)
    refused("overlaps", job(dst={1: at["s1"] + 16}))
    refused("overlaps", job(dst={0: at["s1"]}))
    refused("overlaps", job(dst={0: at["s0"]}, dst_fmt=ofdg.FMT_U8))  # the same address in another format is no in-place form
    refused("overlaps", job(dst={1: at["d0"] + 4 * size - 4}))
    refused("overlaps", job(recs_out=at["recs"] + 32))
    refused("overlaps", job(recs_out=at["d1"]))
    # and a valid call with the same buffers works, in place in frame 0
    for k in ("s0", "s1"):
        raw[k][GUARD:GUARD + 4 * size].view(np.float32)[:] = 100.0
    rraw["recs"][GUARD:GUARD + 64 * n].view(np.float32)[:] = np.tile(record_with(brightness=(0.1, -0.1)), n)
    assert lib.ofdg_host_photo(C.byref(job(dst={0: at["s0"]}, width=W, height=H)), n, W, H) == ofdg.OK
    assert (raw["s0"][GUARD:GUARD + 4 * size].view(np.float32) == np.float32(125.5)).all()
    assert (raw["d1"][GUARD:GUARD + 4 * size].view(np.float32) == np.float32(74.5)).all() and (raw["d0"] == FILL).all()
    assert all((v[:GUARD] == FILL).all() and (v[-GUARD:] == FILL).all() for v in list(raw.values()) + list(rraw.values()))
    assert pr.equal_bits(rraw["out"][GUARD:GUARD + 64 * n].view(np.float32), np.tile(record_with(brightness=(0.1, -0.1)), n))


def test_python_argument_checks(ofdg):
    a = np.zeros((2, 3, 4, 16), np.uint8)
    with pytest.raises(ValueError, match="at least one frame"):
        ofdg.host_photo((None, None))
    with pytest.raises(ValueError, match="n,3"):
        ofdg.host_photo((np.zeros((2, 2, 4, 16), np.uint8), None))
    with pytest.raises(ValueError, match="one dtype"):
        ofdg.host_photo((a, a.astype(np.float32)))
    with pytest.raises(ValueError, match="one dtype"):
        ofdg.host_photo((a.astype(np.float16), None))
    with pytest.raises(ValueError, match="recs must be float32"):
        ofdg.host_photo((a, None), recs=np.zeros((2, 4), np.float32))
    with pytest.raises(ValueError, match="unknown range"):
        ofdg.host_photo((a, None), ranges={"sigma": 1.0})
    with pytest.raises(ofdg.OfdgError, match="width"):
        ofdg.host_photo((np.zeros((1, 3, 4, 12), np.uint8), None))
    assert C.sizeof(ofdg.PhotoRec) == 64 and C.sizeof(ofdg.PhotoJob) == 120 and ofdg.PhotoJob.gamma_log.offset == 84
    hdr = open(ofdg.__file__.replace("__init__.py", "../include/ofdg.h")).read()
    for fn in ("ofdg_photo", "ofdg_host_photo", "ofdg_photo_draw", "ofdg_debug_photo_table", "ofdg_host_photo_table", "ofdg_host_det_log"):
        assert "int %s(" % fn in hdr and fn in ofdg.EXPORTS and hasattr(ofdg.lib(), fn)
