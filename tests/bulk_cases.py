"""Periodic bulk batches for the post-processing operations: what tests/test_bulk_cases.py (CPU) and
tests/test_gpu_many_samples.py (GPU) share.

Every post-processing kernel walks its samples with `for (i = blockIdx.y; i < n; i += gridDim.y)` under a grid of at most
65535 rows, so a workgroup meets a second sample only from n = 65536 on.  A bulk batch here is P = 16 distinct pattern samples
repeated along the sample axis - sample s holds pattern s mod 16, its record, labels and maps alike.  Every operation is a
function of one sample's planes and record, so

  * sample s must equal sample s - 16 byte for byte (one comparison on the device per output tensor), and
  * the first 16 samples (and, past 4 GiB, the last 16) must equal the host twin and the numpy restatement on 16 tiny samples.

65535 mod 16 = 15: workgroup row y works on pattern y mod 16 first and on pattern (y + 15) mod 16 - the pattern in front of
it - on its second trip.  The patterns are ordered so that cyclic neighbours take different paths through the kernel (each
case states the path of every pattern in `paths`, derived from the restatement's own intermediate values; the CPU test asserts
that neighbours differ), and n = 65535 + 16 lets each of the 16 neighbour pairs occur on some workgroup.

A case is an object with
  name, H, W        the operation and the frame
  inputs            dict: name -> numpy array [16, ...], read only
  recs              None or the 16 given records as the plain 2-D array the device entry reads
  paths             16 hashable labels: the path each pattern takes
  excluded          16 booleans: the pattern lies in a range the restatement does not cover (the CPU test wants none)
  restate(inputs, recs) / twin(ofdg, inputs, recs=None, first_index=None)
                    dict: output name -> numpy array, of the restatement / the host twin
  outputs(n)        dict: output name -> (shape, numpy dtype) of the device destinations of n samples
  in_place          dict: output name -> input name it overwrites (the in-place form), usually empty
  run(ofdg, g, tin, trecs, touts, first_index=None)
                    the device call on torch tensors
"""
import numpy as np

P = 16                    # patterns
GRID = 65535              # rows of a launch at most
N_BULK = GRID + P         # 65551: every cyclic neighbour pair on some workgroup
SEED = 11
FIRST_INDEX = 2 ** 40 - 9  # drawn records: the 64-bit sample index crosses 2^40 inside the batch's first 16
DRAWN_AT = (0, 15, 65534, 65535, 65536, 65550)
FILL, GUARD = 0xA5, 64    # the guard convention of the per-operation GPU tests
SMALL, WIDE_IMAGE, WIDE_FLOW = (16, 16), (64, 96), (64, 128)  # (H, W): part A; parts B: 3*W*H*4*65550 >= 2^32, 2*W*H*4*65550 >= 2^32


def plain(recs, dtype, width):
    """records (structured or not) as the plain [n, width] array of the device entry"""
    a = np.ascontiguousarray(recs)
    return a.view(np.uint8).reshape(a.shape[0], -1).view(np.dtype(dtype)).reshape(a.shape[0], width).copy()


def neighbours_differ(paths):
    """the cyclic neighbour pairs (k, k + 1 mod 16) whose paths are the same: the CPU test wants none"""
    return [(k, (k + 1) % P) for k in range(P) if paths[k] == paths[(k + 1) % P]]


def bytes_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def expect_same(got, want, what):
    """two dicts of arrays, byte for byte, with the first sample that differs in the message"""
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for k in sorted(want):
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.dtype, b.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            rows = a.view(np.uint8).reshape(a.shape[0], -1) != b.view(np.uint8).reshape(b.shape[0], -1)
            bad = np.flatnonzero(rows.any(axis=1))
            raise AssertionError("%s: %s differs in %d of %d samples, first %d (%d bytes)" % (what, k, len(bad), a.shape[0], bad[0], rows[bad[0]].sum()))


class Case:
    in_place = {}
    recs = None
    ranges = None
    channels = 3  # of the widest plane
    can_in_place = False

    def outputs(self, n):
        return {}

    def twin_and_restatement(self, ofdg):
        """(twin's outputs, restatement's outputs, what) of the 16 patterns, for every mode the GPU tests run"""
        yield self.twin(ofdg, self.inputs, self.recs), self.restate(self.inputs, self.recs), "the 16 patterns"

    def take(self, idx):
        """(inputs, recs) of the samples whose patterns are idx"""
        idx = np.asarray(idx)
        return {k: v[idx] for k, v in self.inputs.items()}, None if self.recs is None else self.recs[idx]


# ---- the operations on a pair of frames with a record per sample: photo, jitter, camera, jpeg, motion_blur --------------------
class FramePair(Case):
    """image0 / image1 (wide: frame 1 alone, float32 at 96x64) -> the same names; recs_out beside them"""
    flow = False
    def __init__(self, wide=False, in_place=False):
        import importlib
        self.ref = importlib.import_module(self.module)
        self.wide = wide
        self.H, self.W = WIDE_IMAGE if wide else SMALL
        self.dtype = "float32" if wide else "uint8"
        self.frames = (1,) if wide else (0, 1)
        img = self.ref.frames(self.W, self.H, self.dtype, n=P, seed=3)
        self.inputs = {"image%d" % f: img[f] for f in self.frames}
        if self.flow:
            fl = self.flows()
            self.inputs.update({"flow%s" % ("1" if f else ""): fl[f] for f in self.frames})
        self.recs = self.records()
        assert self.recs.shape[0] == P
        self.in_place = {"image%d" % f: "image%d" % f for f in self.frames} if in_place and self.can_in_place else {}
        used = self.restate(self.inputs, self.recs)["recs_out"]
        self.paths, self.excluded = self.classify(used)

    def pair(self, d, stem="image"):
        return tuple(d.get(stem + str(f)) for f in range(2))

    def outputs(self, n):
        out = {"image%d" % f: ((n, 3, self.H, self.W), np.dtype(self.dtype)) for f in self.frames if "image%d" % f not in self.in_place}
        out["recs_out"] = ((n, self.rec_width), np.dtype(self.rec_dtype))
        return out

    def pack(self, pair, used):
        out = {"image%d" % f: pair[f] for f in self.frames}
        out["recs_out"] = plain(used, self.rec_dtype, self.rec_width)
        return out

    def restate(self, inputs, recs, first_index=None):
        fn = getattr(self.ref, self.ref_name)
        if first_index is None:
            return self.pack(*fn(self.pair(inputs), self.typed(recs)))
        return self.pack(*fn(self.pair(inputs), None, seed=SEED, first_index=first_index, ranges=self.ranges))

    def typed(self, recs):
        """plain records as the restatement's own array"""
        return recs if not hasattr(self.ref, "REC") else np.ascontiguousarray(recs).view(self.ref.REC).reshape(-1)

    def twin(self, ofdg, inputs, recs=None, first_index=None):
        fn = getattr(ofdg, "host_" + self.name)
        kw = dict(recs=recs) if first_index is None else dict(seed=SEED, first_index=first_index, ranges=self.ranges)
        return self.pack(*fn(self.pair(inputs), **kw))

    def run(self, ofdg, g, tin, trecs, touts, first_index=None):
        kw = dict(recs=trecs) if first_index is None else dict(seed=SEED, first_index=first_index, ranges=self.ranges)
        dst = None if self.in_place else self.pair(touts)
        getattr(g, self.name)(self.pair(tin), dst, recs_out=touts["recs_out"], size=(self.H, self.W), **kw, **self.more(touts))

    def more(self, touts):
        return {}


class Photo(FramePair):
    """A table per (sample, frame, channel) in LDS behind a barrier, rewritten on every trip.  Given records hold no noise: the
    noise of a sample is keyed by first_index + i, so it is no function of the pattern - the drawn call covers it."""
    name, module, ref_name, rec_dtype, rec_width, can_in_place = "photo", "photo_reference", "photo", "float32", 16, True
    ranges = dict(gamma_log=0.3, contrast_log=0.3, brightness=0.2, colour_log=0.2, sigma_max=8.0, pair_gamma_log=0.05, pair_contrast_log=0.05,
                  pair_brightness=0.02, pair_colour_log=0.02)

    def records(self):
        r = self.ref.records()
        r = np.concatenate([r, r[[1, 8, 9, 11]]])
        r[:, self.ref.SIGMA:self.ref.SIGMA + 2] = 0.0
        # identity records (0, 7, 9 -> 5 after NaN sanitising) apart from each other, the clamp edges between them
        return np.ascontiguousarray(r[[0, 2, 7, 3, 5, 4, 9, 6, 13, 1, 14, 8, 10, 11, 12, 15]])

    def classify(self, used):
        # the path is the table a workgroup leaves in LDS: a neighbour's must be another
        return [u.tobytes() for u in used], [False] * P

    def restate(self, inputs, recs, first_index=None):
        if first_index is None:
            return self.pack(*self.ref.photo(self.pair(inputs), recs))
        n = len(next(iter(inputs.values())))
        return self.pack(*self.ref.photo(self.pair(inputs), self.ref.drawn_records(SEED, first_index, n, self.ranges), seed=SEED, first_index=first_index))


class Jitter(FramePair):
    """jitter_mean_kernel: s_part per sample, `continue` for frames without a contrast; jitter_apply_kernel: identity frames
    copied.  Patterns: identity, contrast only, no contrast, shared = 1, every order (the 24 orders over the two frames of the
    patterns that apply all four operations)."""
    name, module, ref_name, rec_dtype, rec_width, can_in_place = "jitter", "jitter_reference", "jitter", "int32", 16, True
    ranges = dict(brightness=0.4, contrast=0.4, saturation=0.4, hue=0.5 / 3.14, asym_prob=0.2)

    def records(self):
        ref, one = self.ref, self.ref.ONE
        full = lambda a, b, shared=0: ref.rec_of(brightness=(75000, 52000), contrast=(110000, 40000), saturation=(20000, 100000),  # noqa: E731
                                                 hue=(40000, -50000), order=(a, b), shared=shared)
        nocon = lambda k: ref.rec_of(brightness=80000, saturation=30000, hue=-50000, order=k, shared=1)  # noqa: E731
        both = lambda k: ref.rec_of(brightness=75000, contrast=110000, saturation=20000, hue=40000, order=k, shared=1)  # noqa: E731
        rows = [ref.rec_of(order=(10, 23)),                       # identity: copied, no mean
                full(0, 12),
                nocon(17),                                        # no contrast: `continue` in the mean kernel
                full(1, 13),
                ref.rec_of(contrast=90000, order=(8, 21)),        # contrast only
                nocon(5),
                both(2),                                          # shared: one mean for both frames
                ref.rec_of(order=(11, 0)),
                full(3, 14), nocon(15), full(4, 16),
                ref.rec_of(brightness=(70000, one), contrast=(one, 30000), order=(9, 22)),  # frame 0 without, frame 1 with a contrast
                full(6, 18), nocon(19), both(7), nocon(20)]
        r = np.array(rows, ref.REC)
        return plain(r, "int32", 16)

    def classify(self, used):
        u = self.typed(used)
        one = self.ref.ONE
        paths = []
        for r in u:
            per = []
            for f in self.frames:
                ident = all(int(r[k][f]) == one for k in ("brightness", "contrast", "saturation")) and int(r["hue"][f]) == 0
                per.append("copy" if ident else "mean" if int(r["contrast"][f]) != one else "continue")
            paths.append((tuple(per), int(r["shared"]), tuple(int(r["order"][f]) for f in self.frames)))
        return paths, [False] * P

    def more(self, touts):
        return dict(work=touts["work"])

    def outputs(self, n):
        return dict(super().outputs(n), work=((n, 16), np.dtype("uint8")))


class Camera(FramePair):
    """Identity (copy), Bayer alone, blur alone at radii 1, 3 and 12, both, one frame blurred and the other not, every pattern."""
    name, module, ref_name, rec_dtype, rec_width = "camera", "camera_reference", "camera", "int32", 8
    ranges = dict(sigma_min=0.3, sigma_max=1.5, sigma_delta=0.1, blur_prob=0.8, bayer_prob=0.5, pattern=-1)

    def records(self):
        rec = self.ref.rec_of
        rows = [rec(), rec(1024), rec(bayer=2), rec(85), rec(0, bayer=0), rec((300, 0), bayer=1), rec(), rec((0, 700), bayer=3),
                rec(256), rec(bayer=1), rec((40, 1000)), rec(), rec(1024, bayer=3), rec(1), rec(bayer=0), rec(600, bayer=2)]
        return plain(np.array(rows, self.ref.REC), "int32", 8)

    def classify(self, used):
        u = self.typed(used)
        return [(tuple(int(r["radius"][f]) for f in self.frames), int(r["bayer"])) for r in u], [False] * P


class Jpeg(FramePair):
    """Quality 0 (copy), 4:4:4 and 4:2:0, phases on and off the block grid, the extreme qualities, frames at different
    qualities.  16x16 at phase (0, 0): one 4:2:0 MCU."""
    name, module, ref_name, rec_dtype, rec_width, can_in_place = "jpeg", "jpeg_reference", "jpeg", "int32", 8, True
    ranges = dict(prob=0.7, quality_min=30, quality_max=95, quality_delta=5, subsample=-1, sub_prob=0.5, phase=True)

    def records(self):
        rec = self.ref.rec_of
        rows = [rec(0), rec(75, 1, (0, 0)), rec(90, 0, (3, 5)), rec(1, 1, (15, 1)), rec(0, 1, (8, 8)), rec(100, 0, (0, 0)), rec((30, 0), 1, (3, 5)),
                rec(50, 0, (8, 8)), rec(0), rec(100, 1, (8, 8)), rec(1, 0, (15, 1)), rec((0, 60), 1, (0, 0)), rec(95, 0, (7, 7)), rec(20, 1, (1, 15)),
                rec(75, 0, (0, 0)), rec(49, 1, (9, 6))]
        return plain(np.array(rows, self.ref.REC), "int32", 8)

    def classify(self, used):
        u = self.typed(used)
        return [(tuple(int(r["quality"][f]) for f in self.frames), int(r["subsample"]), int(r["phase_x"]), int(r["phase_y"])) for r in u], [False] * P


class MotionBlur(FramePair):
    """mblur_kernel: paths[2][..] by `turn`, the staged window, the uniform `continue` of the copy path.  One 64 x 16 tile per
    sample; the path of a pattern is mblur_reference.tile_paths of its frames under the sanitised shutter: shutter 0 on both
    (copy), a short streak (window), a streak beyond the 16 px halo (gather), non-finite flow, one frame blurred only."""
    name, module, ref_name, rec_dtype, rec_width, flow = "motion_blur", "mblur_reference", "motion_blur", "float32", 4, True
    ranges = dict(prob=0.8, shutter_min=0.5, shutter_max=2.0, pair_shutter=0.25)
    TAPS = 16

    def flows(self):
        H, W = self.H, self.W
        dtype = "float32" if self.wide else "float16"
        rng = np.random.RandomState(5)
        out = [np.zeros((P, 2, H, W), np.float32) for _ in range(2)]
        kinds = self.kinds()
        for f in range(2):
            for k, kind in enumerate(kinds):
                a = out[f][k]
                if kind in ("window", "one", "copy"):      # gentle: every tap within the halo under shutters up to 2
                    a[:] = rng.uniform(-7.5, 7.5, (2, H, W))
                    a[:, ::3, ::2] = np.array([2.5 + k, -1.25], np.float32)[:, None, None]
                elif kind == "gather":                     # a streak beyond the 16 px halo
                    a[:] = rng.uniform(-4, 4, (2, H, W))
                    a[:, 5:9, 3:11] = np.array([40.5 + k, -33.0], np.float32)[:, None, None]
                else:                                      # non-finite flow among gentle vectors
                    a[:] = rng.uniform(-6, 6, (2, H, W))
                    flat = a.reshape(-1)
                    flat[3::7] = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-40, 65504.0], np.float32)[np.arange(len(flat[3::7])) % 6]
        with np.errstate(over="ignore"):
            return tuple(t.astype(dtype) for t in out)

    @staticmethod
    def kinds():
        return ["copy", "window", "gather", "one", "nonfinite", "window", "copy", "gather", "window", "nonfinite", "one", "gather", "copy", "window",
                "gather", "window"]

    def records(self):
        shutter = dict(copy=(0.0, 0.0), window=(1.0, 0.75), gather=(2.0, 1.25), nonfinite=(1.5, 1.5))
        rows, ones = [], 0
        for kind in self.kinds():
            if kind == "one":
                rows.append(((0.0, 1.0), (1.0, 0.0))[ones % 2])
                ones += 1
            else:
                rows.append(shutter[kind])
        r = np.zeros((P, 4), np.float32)
        r[:, :2] = rows
        r[7, :2] = (np.nan, 9.0)   # sanitised: 0 and 2
        return r

    def classify(self, used):
        paths = []
        for k in range(P):
            per = []
            for f in self.frames:
                fl = self.inputs["flow%s" % ("1" if f else "")][k]
                per.append(tuple(self.ref.tile_paths(fl, used[k][f], self.TAPS)))
            paths.append(tuple(per))
        return paths, [False] * P

    def restate(self, inputs, recs, first_index=None):
        if first_index is not None:
            n = len(next(iter(inputs.values())))
            recs = self.ref.drawn_records(SEED, first_index, n, self.ranges)
        return self.pack(*self.ref.motion_blur(self.pair(inputs), self.pair_flow(inputs), recs, self.TAPS))

    def pair_flow(self, d):
        return (d.get("flow"), d.get("flow1"))

    def twin(self, ofdg, inputs, recs=None, first_index=None):
        kw = dict(recs=recs) if first_index is None else dict(seed=SEED, first_index=first_index, ranges=self.ranges)
        return self.pack(*ofdg.host_motion_blur(self.pair(inputs), self.pair_flow(inputs), taps_side=self.TAPS, **kw))

    def run(self, ofdg, g, tin, trecs, touts, first_index=None):
        kw = dict(recs=trecs) if first_index is None else dict(seed=SEED, first_index=first_index, ranges=self.ranges)
        g.motion_blur(self.pair(tin), self.pair(touts), flow=self.pair_flow(tin), taps_side=self.TAPS, recs_out=touts["recs_out"],
                      size=(self.H, self.W), **kw)


# ---- the operations on a dict of planes with a record per sample: crop, spatial, lens -------------------------------------------
class Planes(Case):
    """All eight planes in the compact formats (wide: the four planes of frame 1 in float32) -> the same names; recs_out"""
    shrink = True   # the output is a smaller window

    def __init__(self, wide=False):
        import importlib
        self.ref = importlib.import_module(self.module)
        self.wide = wide
        self.oh, self.ow = WIDE_IMAGE if wide else ((8, 8) if self.shrink else SMALL)
        self.H, self.W = ((self.oh, self.ow + 16) if wide else SMALL) if self.shrink else (self.oh, self.ow)
        fmt = dict(image="float32", flow="float32", occ="float32") if wide else dict(image="uint8", flow="float16", occ="uint8")
        src = self.ref.planes(self.W, self.H, n=P, **fmt)
        self.inputs = {k: np.array(v) for k, v in src.items() if not wide or k.endswith("1")}
        self.recs = np.ascontiguousarray(self.records())
        assert self.recs.shape == (P, self.rec_width) and self.recs.dtype == np.dtype(self.rec_dtype)
        self.paths, self.excluded = self.classify(self.restate(self.inputs, self.recs)["recs_out"])

    def outputs(self, n):
        out = {k: ((n,) + v.shape[1:-2] + (self.oh, self.ow), v.dtype) for k, v in self.inputs.items()}
        out["recs_out"] = ((n, self.rec_width), np.dtype(self.rec_dtype))
        return out

    def pack(self, dst, used):
        return dict(dst, recs_out=np.ascontiguousarray(used).astype(self.rec_dtype).reshape(-1, self.rec_width))

    def drawn(self, first_index):
        return dict(seed=SEED, first_index=first_index, **self.draw_kw)

    def run(self, ofdg, g, tin, trecs, touts, first_index=None):
        kw = dict(recs=trecs) if first_index is None else self.drawn(first_index)
        dst = {k: v for k, v in touts.items() if k != "recs_out"}
        getattr(g, self.name)(tin, dst, recs_out=touts["recs_out"], occ_window=True, **self.size_kw(), **kw)

    def size_kw(self):
        return dict(size=(self.H, self.W))


class Crop(Planes):
    """crop_kernel: the window at every alignment of x0 mod 4, both flips, records that need clamping"""
    name, module, rec_dtype, rec_width = "crop", "crop_reference", "int32", 4
    draw_kw = dict(hflip=True, vflip=True)

    def records(self):
        W, H, cw, ch = self.W, self.H, self.ow, self.oh
        xs = [0, W - cw, 3, 1, 4, 7, W - cw, -5, 2, W, 5, 6, 0, W - cw - 1, 1, 3]
        ys = [0, H - ch, 5, 7, 4, 1, 0, 1 << 30, 2, 1, H - ch, 0, H - ch, 3, -9, 6]
        fl = [0, 1, 2, 3] * 4
        r = np.array([(x, y, f, 0) for x, y, f in zip(xs, ys, fl)], np.int32)
        r[7, 2:], r[9, 2:] = (3 | 0x70, 77), (-3, -1)   # unknown flag bits and reserved words: -3 & 3 = 1
        return r

    def classify(self, used):
        return [(int(u[2]), int(u[0]) & 3) for u in used], [bool(u[3]) for u in used]

    def restate(self, inputs, recs, first_index=None):
        if first_index is not None:
            n = len(next(iter(inputs.values())))
            recs = self.ref.drawn_records(SEED, first_index, n, self.W, self.H, self.ow, self.oh, self.ref.RANDOM_HFLIP | self.ref.RANDOM_VFLIP)
        return self.pack(*self.ref.crop(inputs, recs, self.ow, self.oh, occ_window=True))

    def twin(self, ofdg, inputs, recs=None, first_index=None):
        kw = dict(recs=recs) if first_index is None else self.drawn(first_index)
        return self.pack(*ofdg.host_crop(inputs, self.oh, self.ow, occ_window=True, **kw))

    def size_kw(self):
        return {}  # (the crop takes the context's frame)


class Spatial(Planes):
    """spatial_kernel: the identity, integer and fractional shifts, flips, rotations, zooms, windows outside the frame, records
    that sanitising replaces"""
    name, module, rec_dtype, rec_width = "spatial", "spatial_reference", "float64", 14
    ORDER = [0, 3, 6, 11, 8, 4, 13, 2, 5, 7, 1, 9, 12, 10, 15, 17]
    ranges = dict(zoom_log=0.3, rot=0.3, squeeze_log=0.2, translate=1.0, pair_zoom_log=0.03, pair_rot=0.03, pair_translate=1.0)

    @property
    def draw_kw(self):
        return dict(ranges=self.ranges, hflip=True, vflip=True)

    def records(self):
        return self.ref.records(self.W, self.H, self.ow, self.oh)[self.ORDER]

    def classify(self, used):
        paths = []
        for u, r in zip(used, self.recs):
            per = []
            for f in range(2):
                a, b, tx, d, e, ty = (float(v) for v in u[6 * f:6 * f + 6])
                replaced = not bytes_equal(u[6 * f:6 * f + 6], r[6 * f:6 * f + 6])
                whole = tx == int(tx) and ty == int(ty)
                kind = ("shift" if whole else "fraction") if (a, b, d, e) == (1.0, 0.0, 0.0, 1.0) else "flip" if b == 0 and d == 0 and abs(a) == 1 and abs(e) == 1 else "affine"
                per.append((kind, replaced))
            paths.append(tuple(per))
        return paths, [False] * P

    def restate(self, inputs, recs, first_index=None):
        if first_index is not None:
            n = len(next(iter(inputs.values())))
            recs = self.ref.drawn_records(SEED, first_index, n, self.W, self.H, self.ow, self.oh, self.ranges, self.ref.RANDOM_HFLIP | self.ref.RANDOM_VFLIP)
        return self.pack(*self.ref.spatial(inputs, recs, self.ow, self.oh, occ_window=True))

    def twin(self, ofdg, inputs, recs=None, first_index=None):
        kw = dict(recs=recs) if first_index is None else self.drawn(first_index)
        return self.pack(*ofdg.host_spatial(inputs, self.oh, self.ow, occ_window=True, **kw))


class Lens(Planes):
    """lens_kernel: every k1 of the restatement's grid - barrel, pincushion, none - centred and off centre, with and without
    fringes and vignette, and a record sanitising replaces by the identity"""
    name, module, rec_dtype, rec_width, shrink = "lens", "lens_reference", "float64", 8, False
    ranges = dict(prob=0.8, k1_range=0.1, ca_range=0.01, vig_max=0.4, centre=0.2)

    @property
    def draw_kw(self):
        return dict(ranges=self.ranges, fill=True)

    def records(self):
        r = self.ref.records(self.W, self.H, True)
        bad = self.ref.identity(self.W, self.H)
        bad[0] = np.nan
        return np.concatenate([r, bad[None]])

    def classify(self, used):
        hw, hh = self.ref.half(self.W, self.H)
        return [(float(u[0]), float(u[1]) != 1.0, float(u[2]) != 0.0, float(u[4]) != 0.0, (float(u[5]), float(u[6])) != (hw, hh)) for u in used], [False] * P

    def restate(self, inputs, recs, first_index=None):
        if first_index is not None:
            n = len(next(iter(inputs.values())))
            recs = self.ref.drawn_records(SEED, first_index, n, self.W, self.H, self.ranges, self.ref.FILL)
        return self.pack(*self.ref.lens(inputs, recs, occ_window=True))

    def twin(self, ofdg, inputs, recs=None, first_index=None):
        kw = dict(recs=recs) if first_index is None else self.drawn(first_index)
        return self.pack(*ofdg.host_lens(inputs, occ_window=True, **kw))


# ---- reductions of a flow tensor ---------------------------------------------------------------------------------------------
def flow_patterns(H, W, dtype, seed=7):
    """(flow [17,2,H,W], occ uint8 [17,1,H,W], kinds): the 16 patterns of the flow reductions, cyclic neighbours of different
    kinds - "empty": every pixel unusable (empty tables, key 0); "const": one vector (one bin, all lanes vote together); "noisy":
    64 bins' worth of lengths side by side (the peel loop falls through to the per-lane atomics); "hidden": a usable flow fully
    occluded - and a 17th sample whose one pixel is longer than every pixel of the 16 (the extreme only the last sample holds)."""
    rng = np.random.RandomState(seed)
    kinds = ["empty", "const", "noisy", "hidden"] * 4
    f = np.zeros((P + 1, 2, H, W), np.float32)
    occ = np.zeros((P + 1, 1, H, W), np.uint8)
    for k, kind in enumerate(kinds):
        if kind == "empty":
            f[k] = np.array([np.nan, np.inf, -np.inf, 2.0 ** 20], np.float32)[rng.randint(0, 4, (2, H, W))]
            occ[k, 0, ::2, 1::2] = 3 * (k % 2)
        elif kind == "const":
            f[k, 0], f[k, 1] = 1.5 + 6 * (k // 4), -2.25 * (k // 4)
            occ[k, 0, 1::4] = 1
        elif kind == "noisy":
            f[k] = rng.uniform(-90.0, 90.0, (2, H, W)).astype(np.float32)
            f[k, :, 3, 5] = (np.nan, 1.0)
            occ[k, 0] = rng.randint(0, 5, (H, W)) == 0
        else:
            f[k] = rng.uniform(-20.0, 20.0, (2, H, W)).astype(np.float32)
            occ[k, 0] = 1 + k
    f[P] = rng.uniform(-5.0, 5.0, (2, H, W)).astype(np.float32)
    f[P, :, H - 3, W - 6] = (-300.0, 400.0)   # |flow| = 500: beyond every pixel of the patterns (<= 128), a float16 too
    occ[P, 0, 0, :4] = 1
    with np.errstate(over="ignore"):
        return f.astype(dtype), occ, kinds


class FlowStats(Case):
    """flow_stats_kernel: s_hist, s_cnt, s_sum and s_key cleared per sample."""
    name, channels = "flow_stats", 2
    BIN_PX = 2.0

    def __init__(self, wide=False):
        import flow_stats_reference as fsr
        self.ref, self.wide = fsr, wide
        self.H, self.W = WIDE_FLOW if wide else SMALL
        flow, occ, kinds = flow_patterns(self.H, self.W, "float32" if wide else "float16")
        self.inputs = dict(flow=flow[:P], occ=occ[:P])
        self.last = dict(flow=flow[P:], occ=occ[P:])
        self.kinds = kinds
        rows = fsr.flow_stats(flow[:P], occ[:P], self.BIN_PX, fsr.VISIBLE_ONLY)
        self.paths = []
        for r, kind in zip(rows, kinds):
            bins = sum(1 for h in r["hist"] if h)
            got = "empty" if r["n_counted"] == 0 and r["n_occluded"] < self.H * self.W else "hidden" if r["n_counted"] == 0 else \
                "const" if bins == 1 else "noisy" if bins >= 32 else "other"
            self.paths.append(got)
        self.excluded = [got != kind for got, kind in zip(self.paths, kinds)]

    def structured(self, ofdg, rows):
        return ofdg.flow_stats_numpy(rows)["rows"]

    def restate_rows(self, inputs, flags=0):
        return self.ref.flow_stats(inputs["flow"], inputs["occ"], self.BIN_PX, flags)

    def twin_rows(self, ofdg, inputs, flags=0, rows=None):
        return ofdg.host_flow_stats(inputs["flow"], inputs["occ"], self.BIN_PX, accumulate=bool(flags & self.ref.ACCUMULATE),
                                    visible_only=bool(flags & self.ref.VISIBLE_ONLY), one_row=bool(flags & self.ref.ONE_ROW), rows=rows)

    def rows_array(self, rows):
        """rows (structured, or the restatement's dicts) as uint64 [n, 72], two's complement"""
        rows = rows if isinstance(rows, list) else self.ref.rows_of(rows)
        return np.array([[v & (2 ** 64 - 1) for f in self.ref.FIELDS for v in (r[f] if f == "hist" else [r[f]])] for r in rows], np.uint64)

    def twin_and_restatement(self, ofdg):
        for flags in (0, self.ref.VISIBLE_ONLY):
            for inputs, what in ((self.inputs, "the 16 patterns"), (self.last, "the extreme sample")):
                yield (dict(rows=self.rows_array(self.twin_rows(ofdg, inputs, flags))), dict(rows=self.rows_array(self.restate_rows(inputs, flags))),
                       "%s, flags %d" % (what, flags))

    def expected_one_row(self, per_pattern, last_row, n):
        """The single row of n - 1 periodic samples and the extreme sample behind them, in Python integers: every count and sum
        floor((n - 1) / 16) times plus the remainder patterns once, plus the last sample's; the key is the last sample's own
        with its pixel index moved to sample n - 1 (the low word holds 2^32 - 1 - index)."""
        times, rest = divmod(n - 1, P)
        rows = self.ref.rows_of(per_pattern)
        last = self.ref.rows_of(last_row)[0]
        out = self.ref.zero_rows(1)[0]
        for f in self.ref.FIELDS:
            if f == "hist":
                out[f] = [sum(r[f][b] for r in rows) * times + sum(r[f][b] for r in rows[:rest]) + last[f][b] for b in range(self.ref.BINS)]
            elif f == "max_key":
                assert last[f] >> 32 > max(r[f] >> 32 for r in rows), "the extreme must be the last sample's alone"
                out[f] = last[f] - (n - 1) * self.H * self.W
            else:
                out[f] = sum(r[f] for r in rows) * times + sum(r[f] for r in rows[:rest]) + last[f]
        return out


class FlowPyramid(Case):
    """flow_pyramid_kernel walks its samples along gridDim.z; levels 1..4 of a 16x16 flow with weights."""
    name, channels = "flow_pyramid", 2

    def __init__(self, wide=False):
        import flow_pyramid_reference as fpr
        self.ref, self.wide = fpr, wide
        self.H, self.W = WIDE_FLOW if wide else SMALL
        self.levels = 6 if wide else 4
        self.np_dtype = np.dtype("float32" if wide else "float16")
        flow, occ, kinds = flow_patterns(self.H, self.W, self.np_dtype)
        self.inputs = dict(flow=flow[:P], occ=occ[:P])
        self.kinds = kinds
        w1 = self.restate(self.inputs)["weight1"].reshape(P, -1).astype(np.int64).sum(axis=1)
        self.paths = ["none" if w == 0 else "all" if w == self.H * self.W else "some" for w in w1]
        want = dict(empty="none", hidden="none", const="some", noisy="some")
        self.excluded = [want[k] != p for k, p in zip(kinds, self.paths)]
        # cyclic neighbours: empty -> const -> noisy -> hidden -> empty: hidden and empty both store zeros, told apart by the map
        self.paths = ["%s/%s" % (p, k) for p, k in zip(self.paths, kinds)]

    def outputs(self, n):
        out = {"level%d" % k: ((n, 2, self.H >> k, self.W >> k), self.np_dtype) for k in range(1, self.levels + 1)}
        out.update({"weight%d" % k: ((n, 1, self.H >> k, self.W >> k), np.dtype("uint16")) for k in range(1, self.levels + 1)})
        return out

    def restate(self, inputs, recs=None):
        lv, wt = self.ref.flow_pyramid(inputs["flow"], self.levels, inputs["occ"])
        out = {"level%d" % (k + 1): np.ascontiguousarray(t) for k, t in enumerate(lv)}
        out.update({"weight%d" % (k + 1): np.ascontiguousarray(t) for k, t in enumerate(wt)})
        return out

    def twin(self, ofdg, inputs, recs=None, first_index=None):
        lv, wt = ofdg.host_flow_pyramid(inputs["flow"], self.levels, inputs["occ"], weights=True)
        out = {"level%d" % (k + 1): t for k, t in enumerate(lv)}
        out.update({"weight%d" % (k + 1): t for k, t in enumerate(wt)})
        return out

    def run(self, ofdg, g, tin, trecs, touts, first_index=None):
        out = ([touts["level%d" % k] for k in range(1, self.levels + 1)], [touts["weight%d" % k] for k in range(1, self.levels + 1)])
        g.flow_pyramid(tin["flow"], self.levels, occ=tin["occ"], out=out, size=(self.H, self.W))


class Reproject(Case):
    """reproject_kernel: s_words[2] and s_sums[2] by `turn`.  Patterns, cyclic neighbours of different kinds: "still" - zero
    flow, every target its own pixel -, "outside" - every target leaves the frame -, "collide" - every pixel aims at one and
    the same target pixel -, "hidden" - a smooth flow under a map that
    hides every pixel -, "visible" - the same kind of flow with nothing hidden."""
    name = "reproject"
    KINDS = ["still", "outside", "collide", "hidden", "visible", "outside", "still", "collide"] * 2

    def __init__(self, wide=False):
        import reproject_reference as rr
        self.ref, self.wide = rr, wide
        self.H, self.W = WIDE_IMAGE if wide else SMALL
        self.frames = (1,) if wide else (0, 1)
        self.dtype, fdt, odt = ("float32", "float32", "float32") if wide else ("uint8", "float16", "uint8")
        H, W = self.H, self.W
        rng = np.random.RandomState(9)
        img = rr.frames(W, H, self.dtype, n=P, seed=4)
        fl = [np.zeros((P, 2, H, W), np.float32) for _ in range(2)]
        occ = [np.zeros((P, 1, H, W), np.float32) for _ in range(2)]
        for f in range(2):
            for k, kind in enumerate(self.KINDS):
                if kind == "outside":
                    fl[f][k, 0], fl[f][k, 1] = (W + 3.5 + k) * (1 if f else -1), rng.uniform(-2, 2, (H, W))
                    occ[f][k, 0, ::2] = 1
                elif kind == "collide":
                    yy, xx = np.mgrid[0:H, 0:W]
                    fl[f][k, 0], fl[f][k, 1] = (W // 2 + k % 3) - xx, (H // 3 + f) - yy
                elif kind in ("hidden", "visible"):
                    fl[f][k] = rng.uniform(-3.0, 3.0, (2, H, W))
                    fl[f][k, :, 2, 3] = (np.nan, 1.0)
                    occ[f][k] = 2 if kind == "hidden" else 0
        # (a frame's residual needs both frames, its forward-backward residual both flows)
        self.inputs = dict(image0=img[0], image1=img[1], flow=fl[0].astype(fdt), flow1=fl[1].astype(fdt))
        for f in self.frames:
            self.inputs["occ%d" % f] = occ[f].astype(odt)
        want = self.restate(self.inputs)
        rows, warped = want["rows"].view(np.uint8).reshape(P, 2, -1).view(rr.ROW_DTYPE).reshape(P, 2), want["warped1"]
        self.paths = []
        for k in range(P):
            r = rows[k, self.frames[-1]]
            px = H * W
            one_target = len(np.unique(warped[k].reshape(3, -1), axis=1).T) == 1   # every pixel sampled the same place
            self.paths.append("outside" if r["n_outside"] + r["n_bad"] == px else "hidden" if r["n_hidden"] > 0 and r["n_visible"] == 0 else
                              "still" if not self.inputs["flow1"][k].any() else "collide" if one_target else "visible")
        self.excluded = [p != k for p, k in zip(self.paths, self.KINDS)]

    def pairs(self, d):
        return ((d.get("image0"), d.get("image1")), (d.get("flow"), d.get("flow1")), (d.get("occ0"), d.get("occ1")))

    def outputs(self, n):
        kinds = {"warped": (3, self.dtype), "err": (1, "uint8"), "mask": (1, "uint8"), "fb2": (1, "float32")}
        out = {self.ref.key(name, f): ((n, c, self.H, self.W), np.dtype(dt)) for f in self.frames for name, (c, dt) in kinds.items()}
        out["rows"] = ((n, 256), np.dtype("uint8"))
        return out

    def pack(self, out, rows):
        rows = np.ascontiguousarray(rows)
        return dict(out, rows=rows.view(np.uint8).reshape(rows.shape[0], 256))

    def restate(self, inputs, recs=None):
        images, flows, occ = self.pairs(inputs)
        out, rows = self.ref.reproject(images, flows, occ, frames=self.frames, dst_dtype=self.dtype)
        assert self.ref.ROW_DTYPE.itemsize == 128  # (the restatement's own statement of a frame's row: two make a sample's 256 bytes)
        return self.pack(out, rows)

    def twin(self, ofdg, inputs, recs=None, first_index=None):
        images, flows, occ = self.pairs(inputs)
        return self.pack(*ofdg.host_reproject(images, flows, occ, outputs=ofdg.REPROJ_OUTPUTS, frames=self.frames, dst_dtype=np.dtype(self.dtype)))

    def run(self, ofdg, g, tin, trecs, touts, first_index=None, accumulate=False):
        images, flows, occ = self.pairs(tin)
        g.reproject(images, flows, occ, out={k: v for k, v in touts.items() if k != "rows"}, rows=touts["rows"], frames=self.frames, size=(self.H, self.W),
                    accumulate=accumulate)


def int_rows(rows):
    """a structured array of rows as a list (one per element of the flattened array) of {field path: Python int}"""
    out = []
    for r in np.ascontiguousarray(rows).reshape(-1):
        d = {}

        def walk(v, path):
            if v.dtype.names:
                for name in v.dtype.names:
                    walk(v[name], path + (name,))
            elif v.ndim:
                for i in range(v.shape[0]):
                    walk(v[i], path + (i,))
            else:
                d[path] = int(v)
        walk(r, ())
        out.append(d)
    return out


def summed(per_pattern, n, last=None, maxima=(), keep=()):
    """What n periodic samples (the last replaced by `last` when given) reduce to, in Python integers: every field of the 16
    per-pattern rows floor(m / 16) times plus the remainder patterns once (m the periodic samples), plus the last sample's;
    fields whose last path element is among `maxima` take the maximum, those among `keep` the value of the final sample."""
    m = n if last is None else n - 1
    times, rest = divmod(m, P)
    out = {}
    for path in per_pattern[0]:
        vals = [r[path] for r in per_pattern]
        tail = [] if last is None else [last[path]]
        if path[-1] in maxima or (len(path) > 1 and path[-2] in maxima):
            out[path] = max(vals[:P if times else rest] + tail)
        elif path[-1] in keep:
            out[path] = tail[0] if tail else vals[(m - 1) % P]
        else:
            out[path] = sum(vals) * times + sum(vals[:rest]) + sum(tail)
    return out


class Splat(Case):
    """splat_scatter_kernel and splat_resolve_kernel (double-buffered by `turn`), the clearing of the key planes.  Patterns:
    "still" - zero flow, every source its own target -, "outside" - every source leaves the frame -, "collide" - every source of a
    frame aims at one pixel, labels decide -, "hidden" / "visible" - a smooth flow under a map that hides all / nothing."""
    name, can_in_place = "splat", False
    KINDS = ["still", "outside", "collide", "hidden", "visible", "outside", "still", "collide"] * 2
    TS = [256, 128, 128, 255, 1, 179, 0, 128, 256, 77, 128, 1, 255, 128, 0, 128]   # (collisions: both frames half way)
    t_range = (0.25, 0.75)

    def __init__(self, wide=False):
        import splat_reference as sr
        self.ref, self.wide = sr, wide
        self.H, self.W = WIDE_IMAGE if wide else SMALL
        self.frames = (1,) if wide else (0, 1)
        self.dtype, self.fdt, odt = ("float32", "float32", "float32") if wide else ("uint8", "float16", "uint8")
        H, W = self.H, self.W
        rng = np.random.RandomState(13)
        img = sr.frames(W, H, self.dtype, n=P, seed=6)
        y, x = np.mgrid[0:H, 0:W]
        self.inputs = {}
        for f in self.frames:
            fl, occ = np.zeros((P, 2, H, W), np.float32), np.zeros((P, 1, H, W), np.float32)
            label = rng.randint(0, 4, (P, H, W)).astype(np.uint8) * 85
            for k, kind in enumerate(self.KINDS):
                if kind == "outside":
                    fl[k, 0], fl[k, 1] = 4.0 * W + k, -3.0 * H
                elif kind == "collide":
                    fl[k, 0], fl[k, 1] = (W // 2 + k % 3) - x, (H // 2) - y
                    fl[k, :, 1, 2] = (np.nan, 0.0)
                elif kind in ("hidden", "visible"):
                    fl[k] = rng.uniform(-3.0, 3.0, (2, H, W))
                    occ[k] = 2 if kind == "hidden" else 0
            s = "" if f == 0 else "1"
            self.inputs.update({"image%d" % f: img[f], "flow" + s: fl.astype(self.fdt), "label%d" % f: label, "occ%d" % f: occ.astype(odt)})
        self.recs = np.array([[t, 256 - t, 0, 0] for t in self.TS], np.int32)
        self.recs[3] = (-7, 999, 5, 5)   # sanitised: 0 and 256
        rows = self.restate(self.inputs, self.recs)["rows"].view(sr.ROW_DTYPE).reshape(P, 2)
        self.paths = []
        for k in range(P):
            r, px = rows[k, self.frames[-1]], H * W
            fl = self.inputs["flow1"][k].astype(np.float32)
            kind = "hidden" if self.inputs["occ1"][k].all() else "outside" if r["n_outside"] == px else "still" if not fl.any() else \
                "collide" if r["n_covered"] > px // 2 else "visible"
            self.paths.append((kind, int(r["t_q8"])))
        self.excluded = [p[0] != k for p, k in zip(self.paths, self.KINDS)]

    def pairs(self, d):
        g = lambda a, b: (d.get(a), d.get(b))  # noqa: E731
        return g("image0", "image1"), g("flow", "flow1"), g("label0", "label1"), g("occ0", "occ1")

    def outputs(self, n):
        kinds = {"image": (3, self.dtype), "to_own": (2, self.fdt), "to_other": (2, self.fdt), "mask": (1, "uint8"), "fate": (1, "uint8")}
        out = {self.ref.key(name, f): ((n, c, self.H, self.W), np.dtype(dt)) for f in self.frames for name, (c, dt) in kinds.items()}
        out.update({"keys%d" % f: ((n, self.H, self.W), np.dtype("int32")) for f in self.frames})
        out["rows"], out["recs_out"] = ((n, 128), np.dtype("uint8")), ((n, 4), np.dtype("int32"))
        return out

    def pack(self, out, keys, rows, used):
        out = dict(out)
        out.update({"keys%d" % f: np.ascontiguousarray(keys[f]).view(np.int32) for f in self.frames})
        rows = np.ascontiguousarray(rows)
        out["rows"] = rows.view(np.uint8).reshape(rows.shape[0], 128)
        out["recs_out"] = np.ascontiguousarray(used).astype(np.int32).reshape(-1, 4)
        return out

    def restate(self, inputs, recs, first_index=None):
        images, flows, labels, occ = self.pairs(inputs)
        out, keys, rows = self.ref.splat(images, flows, labels, occ, recs, frames=self.frames, dst_dtype=self.dtype, oflow_dtype=self.fdt)
        used = np.array([tuple(self.ref.sanitise(r))[:2] + (0, 0) for r in recs], np.int32)
        return self.pack(out, keys, rows, used)

    def twin(self, ofdg, inputs, recs=None, first_index=None):
        images, flows, labels, occ = self.pairs(inputs)
        kw = dict(recs=recs) if first_index is None else dict(t=self.t_range, seed=SEED, first_index=first_index)
        return self.pack(*ofdg.host_splat(images, flows, labels, occ, frames=self.frames, dst_dtype=np.dtype(self.dtype), oflow_dtype=np.dtype(self.fdt), **kw))

    def run(self, ofdg, g, tin, trecs, touts, first_index=None, accumulate=False):
        images, flows, labels, occ = self.pairs(tin)
        kw = dict(recs=trecs) if first_index is None else dict(t=self.t_range, seed=SEED, first_index=first_index)
        out = {k: v for k, v in touts.items() if k not in ("rows", "recs_out", "keys0", "keys1")}
        g.splat(images, flows, labels, occ, out=out, keys=(touts.get("keys0"), touts.get("keys1")), rows=touts["rows"], recs_out=touts["recs_out"],
                frames=self.frames, size=(self.H, self.W), accumulate=accumulate, **kw)


class FlowVis(Case):
    """flow_vis_max_kernel and flow_vis_colour_kernel, the clearing of the work words; norm is per call"""
    name, channels = "flow_vis", 2

    def __init__(self, wide=False, norm="sample", layout="planar_bgr"):
        import flow_vis_reference as fv
        self.ref, self.wide, self.norm, self.layout = fv, wide, norm, layout
        self.H, self.W = WIDE_FLOW if wide else SMALL
        flow, occ, kinds = flow_patterns(self.H, self.W, "float32" if wide else "float16")
        self.inputs = dict(flow=flow[:P], occ=occ[:P])
        self.last = dict(flow=flow[P:], occ=occ[P:])
        rows = fv.flow_vis(flow[:P], occ[:P], "sample")[1]
        self.paths = ["empty" if r["max_r2_q16"] == 0 else k for r, k in zip(rows, kinds)]
        self.excluded = [(p == "empty") != (k == "empty") for p, k in zip(self.paths, kinds)]

    def kw(self):
        return dict(norm=self.norm, max_flow=37.5 if self.norm == "fixed" else None, layout=self.layout, dim_occ=True)

    def outputs(self, n):
        shape = (n, 3, self.H, self.W) if self.layout == "planar_bgr" else (n, self.H, self.W, 3)
        return dict(picture=(shape, np.dtype("uint8")), rows=((n, 4), np.dtype("int32")), work=((n, 8), np.dtype("uint8")))

    def pack(self, picture, rows):
        return dict(picture=picture, rows=np.ascontiguousarray(rows).view(np.int32).reshape(-1, 4))

    def restate(self, inputs, recs=None):
        return self.pack(*self.ref.flow_vis(inputs["flow"], inputs["occ"], **self.kw()))

    def twin(self, ofdg, inputs, recs=None, first_index=None):
        return self.pack(*ofdg.host_flow_vis(inputs["flow"], inputs["occ"], **self.kw()))

    def run(self, ofdg, g, tin, trecs, touts, first_index=None):
        g.flow_vis(tin["flow"], touts["picture"], occ=tin["occ"], rows_out=touts["rows"], work=touts["work"], size=(self.H, self.W), **self.kw())


class FlowError(Case):
    """flow_error_kernel: the LDS reduction per sample, the rows, ONE_ROW and ACCUMULATE"""
    name, channels = "flow_error", 2

    def __init__(self, wide=False):
        import flow_error_reference as fe
        self.ref, self.wide = fe, wide
        self.H, self.W = WIDE_FLOW if wide else SMALL
        dt = "float32" if wide else "float16"
        flow, occ, kinds = flow_patterns(self.H, self.W, "float32")
        rng = np.random.RandomState(17)
        est = flow + rng.uniform(-4.0, 4.0, flow.shape).astype(np.float32) * (np.arange(P + 1) % 4 != 1)[:, None, None, None]
        est[2::4, :, 1, 1] = np.inf
        est[P, :, 2, 2] = (3000.0, -4000.0)   # the largest error of all, in the extreme sample alone
        dist2 = rng.randint(0, 256, occ.shape).astype(np.uint8)
        with np.errstate(over="ignore"):
            full = dict(gt=flow.astype(dt), est=est.astype(dt), occ=occ, dist2=dist2)
        self.inputs = {k: v[:P] for k, v in full.items()}
        self.last = {k: v[P:] for k, v in full.items()}
        rows = self.restate(self.inputs)["rows"].view(fe.ROW).reshape(P)
        self.paths = []
        for r, k in zip(rows, kinds):
            n = int(r["cell"]["n"].sum())
            self.paths.append("empty" if n == 0 else "exact" if r["hist"][1:].sum() == 0 else "hidden" if r["cell"]["n"][0].sum() == 0 else "mixed")
        self.kinds = kinds
        self.excluded = [(p == "empty") != (k == "empty") for p, k in zip(self.paths, kinds)]

    def outputs(self, n):
        return dict(rows=((n, 672), np.dtype("uint8")), epe=((n, 1, self.H, self.W), np.dtype("float32" if self.wide else "float16")),
                    picture=((n, 3, self.H, self.W), np.dtype("uint8")))

    def pack(self, out):
        rows = np.ascontiguousarray(out["rows"])
        return dict(out, rows=rows.view(np.uint8).reshape(-1, 672))

    def restate(self, inputs, recs=None, one_row=False):
        return self.pack(self.ref.flow_error(inputs["gt"], inputs["est"], inputs["occ"], inputs["dist2"], outputs=("rows", "epe", "picture"),
                                             epe_dtype=np.float32 if self.wide else np.float16, dim_occ=True, one_row=one_row))

    def twin(self, ofdg, inputs, recs=None, first_index=None, one_row=False):
        return self.pack(ofdg.host_flow_error(inputs["gt"], inputs["est"], inputs["occ"], inputs["dist2"], outputs=("rows", "epe", "picture"),
                                              epe_dtype=None if self.wide else np.float16, dim_occ=True, one_row=one_row))

    def run(self, ofdg, g, tin, trecs, touts, first_index=None, **kw):
        g.flow_error(tin["gt"], tin["est"], occ=tin["occ"], dist2=tin["dist2"], rows=touts["rows"], epe=touts.get("epe"), picture=touts.get("picture"),
                     dim_occ="picture" in touts, size=(self.H, self.W), **kw)   # (the flag needs a picture)


class Erase(Case):
    """erase_mean_kernel and erase_apply_kernel, work[i]: no rectangle, the most (4), one, in either frame; fill is per call"""
    name, can_in_place = "erase", True
    COUNTS = [0, 4, 0, 1, 0, 3, 0, 2, 0, 7, 0, 4, 0, 1, 0, 2]   # (7: sanitised to the most)
    ranges = dict(prob=0.7, min_rects=1, max_rects=4, min_size=2, max_size=9)

    def __init__(self, wide=False, fill=0):
        import erase_reference as er
        self.ref, self.wide, self.fill = er, wide, fill
        self.H, self.W = WIDE_IMAGE if wide else SMALL
        self.frames = (1,) if wide else (0, 1)
        H, W = self.H, self.W
        idt, fdt, odt = ("float32", "float32", "float32") if wide else ("uint8", "float16", "uint8")
        img, fl, occ = er.frames(W, H, idt, n=P, seed=8), er.flows(W, H, fdt, n=P, seed=2), er.maps(W, H, odt, n=P, seed=3)
        if wide:   # frame 1 alone: its rectangles, its map (marked where a rectangle lies)
            self.inputs = dict(image1=np.array(img[1]), occ1=np.array(occ[1]))
        else:
            self.inputs = dict(image0=np.array(img[0]), image1=np.array(img[1]), occ0=np.array(occ[0]), occ1=np.array(occ[1]), flow=np.array(fl[0]),
                               flow1=np.array(fl[1]))
        r = np.zeros((P,), er.REC)
        rng = np.random.RandomState(21)
        for k, c in enumerate(self.COUNTS):
            r[k]["count"] = c
            for j in range(4):
                r[k]["rect"][j] = (rng.randint(-3 if j else 0, W - 1), rng.randint(-2 if j else 0, H - 1), rng.randint(1, W // 2 + 2), rng.randint(1, H // 2 + 2),
                                   1 if wide else (k + j) % 2)
        r[11]["rect"][0] = (0, 0, W, H, 1)       # the whole frame
        self.recs = plain(r, "int32", 24)
        self.in_place = {k: k for k in self.inputs if not k.startswith("flow")}
        used = self.restate(self.inputs, self.recs)["recs_out"].view(er.REC).reshape(P)
        self.paths = [int(u["count"]) for u in used]
        self.excluded = [False] * P

    def trio(self, d, copy=False):
        c = (lambda a: None if a is None else np.array(a)) if copy else (lambda a: a)
        images, occ = (c(d.get("image0")), c(d.get("image1"))), (c(d.get("occ0")), c(d.get("occ1")))
        flow = (d.get("flow"), d.get("flow1"))
        return images, occ, None if all(t is None for t in flow) else flow

    def kw(self):
        return dict(fill=self.fill, color=(10, 200, 33), frames=self.frames)

    def outputs(self, n):
        return dict(recs_out=((n, 24), np.dtype("int32")), work=((n, 64), np.dtype("uint8")))

    def pack(self, images, occ, used):
        out = {"image%d" % f: images[f] for f in range(2) if images[f] is not None}
        out.update({"occ%d" % f: occ[f] for f in range(2) if occ[f] is not None})
        out["recs_out"] = plain(used, "int32", 24)
        return out

    def restate(self, inputs, recs, first_index=None):
        images, occ, flow = self.trio(inputs)
        typed = None if recs is None else np.ascontiguousarray(recs).view(self.ref.REC).reshape(-1)
        more = {} if first_index is None else dict(seed=SEED, first_index=first_index, ranges=self.ranges)
        return self.pack(*self.ref.erase(images, occ, flow, typed, **self.kw(), **more))

    def twin(self, ofdg, inputs, recs=None, first_index=None):
        images, occ, flow = self.trio(inputs, copy=True)
        more = dict(recs=recs) if first_index is None else dict(seed=SEED, first_index=first_index, ranges=self.ranges)
        used = ofdg.host_erase(images, occ, flow, **self.kw(), **more)
        return self.pack(images, occ, used)

    def run(self, ofdg, g, tin, trecs, touts, first_index=None):
        images, occ, flow = self.trio(tin)
        more = dict(recs=trecs) if first_index is None else dict(seed=SEED, first_index=first_index, ranges=self.ranges)
        g.erase(images, occ, flow, recs_out=touts["recs_out"], work=touts["work"], size=(self.H, self.W), **self.kw(), **more)


class Pack(Case):
    """pack_kernel: layout, concat and rgb are per call"""
    name = "pack"

    def __init__(self, wide=False, layout=0, concat=False, rgb=False):
        import pack_reference as pk
        self.ref, self.wide, self.mode = pk, wide, (layout, concat, rgb)
        self.H, self.W = WIDE_IMAGE if wide else SMALL
        self.out_dtype = "float32" if wide else "float16"
        idt, fdt = ("float32", "float32") if wide else ("uint8", "float16")
        src = pk.sources(self.W, self.H, idt, fdt, n=P)
        img, fl = (src["image0"], src["image1"]), np.array(src["flow"])
        fl[0::2] = np.where(np.isfinite(fl[0::2].astype(np.float32)), fl[0::2], fl.dtype.type(1.5))   # even patterns: finite flows only
        fl[1::2, :, 0, :4] = fl.dtype.type(np.inf)
        self.inputs = dict(image1=np.array(img[1]), flow=fl) if wide else dict(image0=np.array(img[0]), image1=np.array(img[1]), flow=fl)
        self.paths = ["finite" if np.isfinite(fl[k].astype(np.float32)).all() else "special" for k in range(P)]
        self.excluded = [False] * P

    def kw(self):
        layout, concat, rgb = self.mode
        return dict(scale=(0.5, 1.25, 2.0), bias=(-3.0, 0.25, 7.5), flow_scale=0.05, layout=layout, concat=concat, rgb=rgb)

    def outputs(self, n):
        layout, concat, _ = self.mode
        out = {}
        for k in self.inputs:
            if concat and k == "image1":
                continue
            c = 2 if k == "flow" else 6 if concat else 3
            out[k] = ((n, self.H, self.W, c) if layout == self.ref.NHWC else (n, c, self.H, self.W), np.dtype(self.out_dtype))
        return out

    def memory(self, out):
        """the planes as their memory holds them (NHWC: [n,H,W,C])"""
        nhwc = self.mode[0] == self.ref.NHWC
        return {k: np.ascontiguousarray(np.asarray(v).transpose(0, 2, 3, 1)) if nhwc else np.ascontiguousarray(v) for k, v in out.items()}

    def restate(self, inputs, recs=None):
        return self.memory(self.ref.pack(inputs, self.out_dtype, self.out_dtype, **self.kw()))

    def twin(self, ofdg, inputs, recs=None, first_index=None):
        return self.memory(ofdg.host_pack(inputs, np.dtype(self.out_dtype), np.dtype(self.out_dtype), **self.kw()))

    def run(self, ofdg, g, tin, trecs, touts, first_index=None):
        nhwc = self.mode[0] == self.ref.NHWC
        g.pack(tin, {k: v.permute(0, 3, 1, 2) if nhwc else v for k, v in touts.items()}, size=(self.H, self.W), **self.kw())


class Boundaries(Case):
    """boundary_kernel: the label mode, the radius and min_step are per call"""
    name, channels = "boundaries", 2

    def __init__(self, wide=False, labels=True, radius=4, min_step=0.0):
        import boundaries_reference as br
        self.ref, self.wide, self.mode = br, wide, (labels, radius, min_step)
        self.H, self.W = WIDE_FLOW if wide else SMALL
        self.frames = (1,) if wide else (0, 1)
        H, W = self.H, self.W
        rng = np.random.RandomState(23)
        self.inputs = {}
        for f in self.frames:
            fl, label = np.zeros((P, 2, H, W), np.float32), np.zeros((P, H, W), np.uint8)
            for k in range(P):
                if k % 2 == 0:    # flat: one motion, one label, no step anywhere
                    fl[k, 0], fl[k, 1], label[k] = 1.5 * k, -0.75, k
                else:             # blocks with their own labels and motions, a step inside a label, special values in every fourth
                    label[k] = rng.randint(1, 5, (H // 4, W // 4)).repeat(4, axis=0).repeat(4, axis=1)
                    fl[k] = np.moveaxis(rng.randint(-3, 4, (5, 2)).astype(np.float32)[label[k]] * 0.75, -1, 0)
                    fl[k, 0, :, W // 2:] += 1.5
                    if k % 4 == 3:
                        fl[k].reshape(-1)[5::37] = np.array([np.nan, np.inf, -np.inf, 65504.0], np.float32)[np.arange(len(fl[k].reshape(-1)[5::37])) % 4]
            s = "" if f == 0 else "1"
            self.inputs.update({"flow" + s: fl.astype("float32" if wide else "float16"), "label" + s: label})
        out = self.restate(self.inputs)
        e = out["edge%d" % self.frames[-1]].reshape(P, -1)
        self.paths = ["edges" if row.any() else "flat" for row in e]
        self.excluded = [(p == "flat") != (k % 2 == 0) for k, p in enumerate(self.paths)]

    def outputs(self, n):
        return {"%s%d" % (name, f): ((n, 1, self.H, self.W), np.dtype("uint8")) for f in self.frames for name in ("edge", "dist")}

    def restate(self, inputs, recs=None):
        labels, radius, min_step = self.mode
        out = {}
        for f in self.frames:
            s = "" if f == 0 else "1"
            out["edge%d" % f] = np.ascontiguousarray(self.ref.edge_of(inputs["flow" + s], inputs["label" + s], min_step, labels))
            out["dist%d" % f] = np.ascontiguousarray(self.ref.dist2_of(out["edge%d" % f], radius))
        return out

    def twin(self, ofdg, inputs, recs=None, first_index=None):
        labels, radius, min_step = self.mode
        return ofdg.host_boundaries(inputs.get("flow"), inputs.get("label"), inputs.get("flow1"), inputs.get("label1"), radius=radius, min_step=min_step,
                                    labels=labels)

    def run(self, ofdg, g, tin, trecs, touts, first_index=None):
        labels, radius, min_step = self.mode
        g.boundaries(tin.get("flow"), touts.get("edge0"), touts.get("dist0"), tin.get("label"), tin.get("flow1"), touts.get("edge1"), touts.get("dist1"),
                     tin.get("label1"), radius=radius, min_step=min_step, labels=labels, size=(self.H, self.W))


RECORD_CASES = dict(photo=Photo, jitter=Jitter, camera=Camera, jpeg=Jpeg, motion_blur=MotionBlur, crop=Crop, spatial=Spatial, lens=Lens)
CASES = dict(RECORD_CASES, flow_stats=FlowStats, flow_pyramid=FlowPyramid, reproject=Reproject, splat=Splat, flow_vis=FlowVis, flow_error=FlowError,
             erase=Erase, pack=Pack, boundaries=Boundaries)
_cache = {}


def case(name, wide=False, **kw):
    """the case of an operation, built once; read only"""
    key = (name, wide, tuple(sorted(kw.items())))
    if key not in _cache:
        cls = CASES[name]
        c = cls(wide=wide, **kw)
        for v in c.inputs.values():
            v.setflags(write=False)
        _cache[key] = c
    return _cache[key]
