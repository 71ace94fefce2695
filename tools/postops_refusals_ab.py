"""What the post-processing entries answer to bad arguments, at a
parent revision and in the working tree, side by side:

    tools/build_rev.sh <rev> parent                      # the parent's library and a checkout with its __init__.py
    python tools/postops_refusals_ab.py [--gpu] [--parent-root DIR] [--parent-lib LIB]

Every case breaks one rule, or two neighbouring rules of an entry's order of checks at once - those twice, the two breakages
applied in either order -, so a changed order of checks or a changed text shows as a row whose columns differ.  Without --gpu:
the rules of flow_stats_arg_error, flow_pyramid_arg_error and crop_arg_error through the ofdg_host_* entries, and every
ValueError of the six *_format functions of the package (CPU tensors).  With --gpu, also, on a 64x32 context in mode 7: the
rules only the device entries have (misaligned pointers, OFDG_STREAM_OWN before any call, plane_size_error of the sized
entries, everything ofdg_object_table refuses), then one valid call of each entry behind a render call with a hash of what it
wrote.  Then every job-struct entry (crop, photo, spatial, lens, pack, boundaries, erase, jitter, flow_vis, flow_error, camera,
jpeg, motion blur, reproject, splat) from the ctypes _fields_ of its job (job_cases): without --gpu the ofdg_host_* twin and the
ofdg_X_draw entry on a host arena, and the ValueError of every range dict; with --gpu the device entry on a device arena -
every pointer field misaligned, OFDG_STREAM_OWN before any call, `work` missing, the base job as the valid call, a hash of the
arena.  Equal rows of these entries are printed as one line an entry.  These are argument refusals: nothing is enqueued by them.  Each side runs in a process of its own (OFDG_LIB names the
parent's library there).  Exit 0: every row equal."""
import argparse
import ctypes as C
import hashlib
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "optical-flow-2d-data-generation_amd"


def cases_of(rules):
    """[(label, [mutations in the order to apply])]: every rule alone, neighbours together in both orders of application"""
    out = [(name, [fn]) for name, fn in rules]
    for (a, fa), (b, fb) in zip(rules, rules[1:]):
        out += [("%s + %s" % (a, b), [fa, fb]), ("%s + %s" % (b, a), [fb, fa])]
    return out


def put(**kw):
    return lambda a: a.update(kw)


def mutated(base, muts):
    """a copy of the arguments (its lists and dicts copied too) with the mutations applied in their order"""
    a = {k: (dict(v) if isinstance(v, dict) else list(v) if isinstance(v, list) else v) for k, v in base.items()}
    for f in muts:
        f(a)
    return a


# ---- the C entries on host buffers -------------------------------------------------------------------------------------------
def host_cases(m, np):
    L = m.lib()
    rows = []
    n, W, H = 2, 16, 8
    flow = np.zeros((n, 2, H, W), np.float32)
    occ = np.zeros((n, 1, H, W), np.float32)
    stats = np.zeros((n, 304 + 8), np.uint8)
    levels = [np.zeros((n, 2, H >> k, W >> k), np.float32) for k in (1, 2)]
    weights = [np.zeros((n, 1, H >> k, W >> k), np.uint16) for k in (1, 2)]
    adr = lambda a: a.ctypes.data  # noqa: E731

    def answer(entry, label, rc):
        rows.append(("%s: %s" % (entry, label), int(rc), L.ofdg_host_last_error().decode() if rc else ""))

    huge = put(n=65536, width=65536, height=1)
    base = dict(flow=adr(flow), flow_fmt=m.FMT_F32, occ=adr(occ), occ_fmt=m.FMT_F32, n=n, width=W, height=H, bin_px=2.0, flags=0, rows=adr(stats))
    rules = [("flow NULL", put(flow=None)), ("rows NULL", put(rows=None)), ("flow_fmt u8", put(flow_fmt=m.FMT_U8)), ("occ_fmt f16", put(occ_fmt=m.FMT_F16)),
             ("n 0", put(n=0)), ("width 0", put(width=0)), ("height -1", put(height=-1)), ("bin_px 0", put(bin_px=0.0)), ("bin_px nan", put(bin_px=float("nan"))),
             ("flags 8", put(flags=8)), ("visible_only without occ", put(flags=2, occ=None)),
             ("one_row 2^32", lambda a: (huge(a), a.update(flags=4))), ("rows + 4", put(rows=adr(stats) + 4))]
    for label, muts in cases_of(rules):
        a = mutated(base, muts)
        answer("ofdg_host_flow_stats", label, L.ofdg_host_flow_stats(a["flow"], a["flow_fmt"], a["occ"], a["occ_fmt"], a["n"], a["width"], a["height"],
                                                                    a["bin_px"], a["flags"], a["rows"]))

    base = dict(flow=adr(flow), flow_fmt=m.FMT_F32, occ=adr(occ), occ_fmt=m.FMT_F32, n=n, width=W, height=H, flags=0, pyr=True, levels=2, out_fmt=m.FMT_F32,
                lv=[adr(t) for t in levels], wt=[adr(t) for t in weights])
    rules = [("flow NULL", put(flow=None)), ("pyr NULL", put(pyr=False)), ("flow_fmt u8", put(flow_fmt=m.FMT_U8)), ("occ_fmt f16", put(occ_fmt=m.FMT_F16)),
             ("out_fmt u8", put(out_fmt=m.FMT_U8)), ("n 0", put(n=0)), ("height 0", put(height=0)), ("flags 2", put(flags=2)), ("levels 0", put(levels=0)),
             ("levels 7", put(levels=7)), ("width 18", put(width=18)), ("level 2 NULL", lambda a: a.update(lv=[a["lv"][0], None])),
             ("one weight", lambda a: a.update(wt=[a["wt"][0], None])), ("level 1 + 4", lambda a: a.update(lv=[a["lv"][0] + 4, a["lv"][1]])),
             ("weight 2 + 2", lambda a: a.update(wt=[a["wt"][0], a["wt"][1] + 2]))]
    for label, muts in cases_of(rules):
        a = mutated(base, muts)
        rec = m.FlowPyramid()
        rec.levels, rec.out_fmt = a["levels"], a["out_fmt"]
        for k in range(2):
            rec.flow[k], rec.weight[k] = a["lv"][k], a["wt"][k]
        answer("ofdg_host_flow_pyramid", label, L.ofdg_host_flow_pyramid(a["flow"], a["flow_fmt"], a["occ"], a["occ_fmt"], a["n"], a["width"], a["height"],
                                                                        a["flags"], C.byref(rec) if a["pyr"] else None))

    cw, ch = 8, 4
    src = {k: np.zeros((n, c, H, W), np.float32) for k, c in zip(m.CROP_PLANES, (3, 3, 2, 2, 1, 1))}
    dst = {k: np.zeros((n, t.shape[1], ch, cw), np.float32) for k, t in src.items()}
    recs = np.zeros((n, 4), np.int32)
    base = dict(job=True, n=n, width=W, height=H, crop_w=cw, crop_h=ch, flags=0, reserved=0, image_fmt=0, flow_fmt=0, occ_fmt=0, recs=None, recs_out=None,
                src=[adr(src[k]) for k in m.CROP_PLANES[:6]] + [None, None], dst=[adr(dst[k]) for k in m.CROP_PLANES[:6]] + [None, None])

    def plane(which, k, v):
        def f(a):
            a[which] = a[which][:k] + [v] + a[which][k + 1:]
        return f

    def only(*ks):
        def f(a):
            a["src"] = [p if k in ks else None for k, p in enumerate(a["src"])]
            a["dst"] = [p if k in ks else None for k, p in enumerate(a["dst"])]
        return f

    rules = [("height 0", put(height=0)), ("job NULL", put(job=False)), ("n 0", put(n=0)), ("crop_w 4", put(crop_w=4)), ("crop_w 24", put(crop_w=24)),
             ("crop_w 12", put(crop_w=12)), ("crop_h 0", put(crop_h=0)), ("crop_h 10", put(crop_h=10)), ("crop_h 3", put(crop_h=3)),
             ("frame 2^31", put(width=65536, height=32768)), ("flags 32", put(flags=32)), ("reserved 1", put(reserved=1)), ("image_fmt f16", put(image_fmt=m.FMT_F16)),
             ("flow_fmt u8", put(flow_fmt=m.FMT_U8)), ("occ_fmt f16", put(occ_fmt=m.FMT_F16)), ("src without dst", plane("dst", 1, None)),
             ("dst without src", plane("src", 2, None)), ("no plane", only()), ("occ_window: occ0 without flow", lambda a: (only(4, 5, 3)(a), a.update(flags=16))),
             ("occ_window: occ1 without flow1", lambda a: (only(4, 5, 2)(a), a.update(flags=16))), ("dst = src", plane("dst", 0, adr(src["image1"]))),
             ("recs_out in a source", put(recs_out=adr(src["flow"]) + 16))]
    for label, muts in cases_of(rules):
        a = mutated(base, muts)
        job = m.CropJob()
        for k in range(8):
            job.src[k], job.dst[k] = a["src"][k], a["dst"][k]
        job.recs, job.recs_out, job.crop_w, job.crop_h, job.flags, job.reserved = a["recs"], a["recs_out"], a["crop_w"], a["crop_h"], a["flags"], a["reserved"]
        job.image_fmt, job.flow_fmt, job.occ_fmt = a["image_fmt"], a["flow_fmt"], a["occ_fmt"]
        answer("ofdg_host_crop", label, L.ofdg_host_crop(C.byref(job) if a["job"] else None, a["n"], a["width"], a["height"]))
    return rows


# ---- every job-struct entry, from the ctypes _fields_ of its job -------------------------------------------------------------
# A valid base job at 8 x 2, n = 1, every pointer in a slot of its own inside ONE arena; then every field alone against a short
# list of hostile values and every pair of fields that are neighbours in the entry's order of checks, in both orders.  Pointers
# take NULL or addresses inside the arena only (the other buffers, +-1 byte, a one-byte overlap from either side); n_samples and
# the plane size take values the parent must refuse (main() asserts that on the parent's answers: rows marked `sized`).
JW, JH = 8, 2
PX = JW * JH
INTS = [-1, 0, 1, 2, 3, 7, 255, 65537, 2 ** 31 - 1, -2 ** 31]
FLOATS = [-1.0, float("nan"), float("inf"), 0.0, 0.5, 1.0, 4.0, 1e9, float("-inf")]
SIZED = dict(n_samples=[0, -1, -2 ** 31], width=[0, -1, 4, 12, 7, 2 ** 31 - 1], height=[0, -1, 1, 3, 2 ** 31 - 1])
F3, F2, F1, B1 = 12 * PX, 8 * PX, 4 * PX, PX  # bytes of a float32 frame, flow, map and of a uint8 plane


def job_ops(m):
    """name -> (job class, base scalars, {pointer field: bytes at the base formats}, order of checks or None, draw entry or None,
    record bytes)"""
    eight = lambda: {"%s[%d]" % (w, k): b for w in ("src", "dst") for k, b in enumerate((F3, F3, F2, F2, F1, F1, B1, B1))}  # noqa: E731
    pair = lambda rec: dict({"%s[%d]" % (w, f): F3 for w in ("src", "dst") for f in (0, 1)}, recs=rec, recs_out=rec)  # noqa: E731
    two = lambda **kw: {"%s[%d]" % (k, f): b for k, b in kw.items() for f in (0, 1)}  # noqa: E731
    head = ["n_samples", "job.width", "job.height", "width", "height", "src_fmt", "dst_fmt"]
    tail = ["src[0]", "dst[0]", "src[1]", "dst[1]", "recs", "recs_out"]
    return {
        "crop": (m.CropJob, dict(crop_w=JW, crop_h=JH), dict(eight(), recs=16, recs_out=16), None, None, 16),
        "photo": (m.PhotoJob, {}, pair(64), head + ["flags", "reserved"] + list(m.PHOTO_RANGES) + tail, "ofdg_photo_draw", 64),
        "spatial": (m.SpatialJob, dict(out_w=JW, out_h=JH), dict(eight(), recs=112, recs_out=112), None, None, 112),
        "lens": (m.LensJob, {}, dict(eight(), recs=64, recs_out=64), None, None, 64),
        "pack": (m.PackJob, {"scale[0]": 1.0, "scale[1]": 1.0, "scale[2]": 1.0, "flow_scale": 1.0},
                 {"src[0]": F3, "src[1]": F3, "src[2]": F2, "dst[0]": F3, "dst[1]": F3, "dst[2]": F2}, None, None, 0),
        "boundaries": (m.BoundaryJob, dict(radius=1, min_step=1.0), two(flow=F2, label=B1, edge=B1, dist2=B1), None, None, 0),
        "erase": (m.EraseJob, dict(flags=7, max_rects=4, min_size=1, max_size=8, prob=1.0),
                  dict(two(image=F3, occ=F1, flow=F2), recs=96, recs_out=96, work=64), None, "ofdg_erase_draw", 96),
        "jitter": (m.JitterJob, {}, dict(pair(64), work=64),
                   head + ["flags", "reserved"] + list(m.JITTER_RANGES) + tail + ["work"], "ofdg_jitter_draw", 64),
        "flow_vis": (m.FlowVisJob, dict(max_flow=10.0), dict(flow=F2, occ=F1, dst=3 * PX, rows_out=16, work=8), None, None, 0),
        "flow_error": (m.FlowErrorJob, {"est_scale": 1.0, "speed_px[0]": 1.0, "speed_px[1]": 10.0, "dist2_edge[0]": 1, "dist2_edge[1]": 2},
                       dict(gt=F2, est=F2, occ=F1, dist2=B1, rows=672, epe=F1, picture=3 * PX), None, None, 0),
        "camera": (m.CameraJob, dict(pattern=-1), pair(32),
                   head + ["flags", "reserved", "sigma_min", "sigma_max", "sigma_delta", "blur_prob", "bayer_prob", "pattern"] + tail, "ofdg_camera_draw", 32),
        "jpeg": (m.JpegJob, dict(quality_min=75, quality_max=75), pair(32),
                 head + ["reserved[0]", "reserved[1]", "flags", "quality_min", "quality_max", "quality_delta", "prob", "sub_prob", "subsample"] + tail,
                 "ofdg_jpeg_draw", 32),
        "motion_blur": (m.MblurJob, dict(taps_side=4), dict(two(src=F3, dst=F3, flow=F2), recs=16, recs_out=16),
                        head + ["flow_fmt", "flags", "reserved[0]", "reserved[1]", "taps_side", "src[0]", "dst[0]", "flow[0]", "src[1]", "dst[1]", "flow[1]"] +
                        list(m.MBLUR_RANGES) + ["recs", "recs_out"], "ofdg_motion_blur_draw", 16),
        "reproject": (m.ReprojectJob, dict(flags=3), dict(two(img=F3, flow=F2, occ=F1, warped=F3, err=B1, mask=B1, fb2=F1), rows=256), None, None, 0),
        "splat": (m.SplatJob, dict(flags=3, t_min_q8=128, t_max_q8=128),
                  dict(two(img=F3, flow=F2, label=B1, occ=F1, keys=F1, image=F3, to_own=F2, to_other=F2, mask=B1, fate=B1), rows=128, recs=16, recs_out=16),
                  None, "ofdg_splat_draw", 16),
    }


def job_fields(cls):
    """[(name, "p" | "i" | "f")] of a job class, an array's elements one by one"""
    out = []
    for name, t in cls._fields_:
        n = getattr(t, "_length_", None)
        e = t._type_ if n else t
        kind = "p" if e is C.c_void_p else "f" if e is C.c_float else "i"
        out += [("%s[%d]" % (name, k), kind) for k in range(n)] if n else [(name, kind)]
    return out


def job_set(job, name, v):
    if name.endswith("]"):
        getattr(job, name[:name.index("[")])[int(name[name.index("[") + 1:-1])] = v
    else:
        setattr(job, name, v)


def job_cases(m, L, base_adr, slot, device=None):
    """rows of every job-struct entry; device: None for the ofdg_host_* twins (and the draws), else (ctx handle, stream cases)"""
    rows = []
    for op, (cls, scalars, ptrs, order, draw, rec_bytes) in job_ops(m).items():
        fields = job_fields(cls)
        kinds = dict(fields)
        adr = {name: base_adr + slot * k for k, name in enumerate(ptrs)}  # (a slot each: `slot` bytes, far more than any buffer)
        assert set(ptrs) == {f for f, k in fields if k == "p"}, op
        base = dict({f: 0 for f, k in fields if k != "p"}, **scalars)
        base.update(adr)
        if "recs" in ptrs:
            base["recs"] = None  # (the draw; a given record array is one of the pointer cases)
        if device and op == "crop":
            continue  # (the context's own 64 x 32 frame: gpu_cases above)
        has_size = "width" in kinds
        call = dict(n_samples=1, width=JW, height=JH)
        if device and has_size:
            base["width"], base["height"] = JW, JH  # (a device entry takes the job's own size; the context's is 64 x 32)

        def hostile(f):
            if f in call:  # (ofdg_host_crop takes any frame its window fits in: only what it refuses)
                return [0, -1, 2 ** 31 - 1] if op == "crop" and f != "n_samples" else SIZED[f]
            name = f[4:] if f.startswith("job.") else f
            if kinds[name] == "f":
                return FLOATS
            if kinds[name] == "i":
                return [v for v in INTS if v != base[name]][:9] if name not in ("width", "height") else [-1, 1, 2, 3, 7, 255, 65537, 2 ** 31 - 1, -2 ** 31]
            vals = [None, adr[name] + 1, adr[name] - 1]
            if device:
                return vals + [adr[name] + 2, adr[name] + 4, adr[name] + 8]
            for other in ptrs:
                if other != name:
                    vals += [adr[other], adr[other] + ptrs[other] - 1, adr[other] - ptrs[name] + 1]
            return vals

        def answer(label, muts, sized):
            job, c = cls(), dict(call)
            vals = dict(base)
            for f, v in muts:
                if f in c:
                    c[f] = v
                else:
                    vals[f[4:] if f.startswith("job.") else f] = v
            stream = vals.pop("stream", None)
            for f, v in vals.items():
                job_set(job, f, v)
            if device:
                rc = getattr(L, "ofdg_" + op)(device, C.byref(job), c["n_samples"], stream)
                why = L.ofdg_last_error(device).decode() if rc else ""
            else:
                rc = getattr(L, "ofdg_host_" + op)(C.byref(job), c["n_samples"], c["width"], c["height"])
                why = L.ofdg_host_last_error().decode() if rc else ""
            rows.append(("%s %s: %s" % ("ofdg_" + op if device else "ofdg_host_" + op, "sized" if sized else "", label), int(rc), why))
            if draw and not device and not sized and all(kinds.get(f, "p") != "p" for f, _ in muts):
                out = C.cast((C.c_uint8 * rec_bytes)(), getattr(L, draw).argtypes[-1])
                args = (7, 3, JW, JH, C.byref(job), out) if op == "erase" else (7, 3, C.byref(job), out)
                rc = getattr(L, draw)(*args)
                rows.append(("%s: %s" % (draw, label), int(rc), L.ofdg_host_last_error().decode() if rc else ""))

        names = list(call) * (not device) + [("job." + f if f in ("width", "height") else f) for f, _ in fields]
        if device:
            names = [f for f in names if kinds.get(f) == "p"] + ["stream"]
            kinds["stream"], base["stream"] = "s", None
        show = lambda v: "NULL" if v is None else ("arena%+d" % (v - base_adr) if isinstance(v, int) and v > 2 ** 32 else repr(v))  # noqa: E731
        values = lambda f: [C.c_void_p(m.STREAM_OWN)] if f == "stream" else hostile(f)  # noqa: E731
        label = lambda f, v: "%s = %s" % (f, "own" if f == "stream" else show(v))  # noqa: E731
        is_sized = lambda f: f in call or f in ("job.width", "job.height")  # noqa: E731
        answer("the base job", [], False)
        for f in names:
            for v in values(f):
                answer(label(f, v), [(f, v)], is_sized(f))
        seq = [f for f in (order or names) if f in names] if not device else names
        for a, b in zip(seq, seq[1:]):
            for va in values(a)[:3]:
                for vb in values(b)[:3]:
                    answer("%s, %s" % (label(a, va), label(b, vb)), [(a, va), (b, vb)], is_sized(a) or is_sized(b))
                    answer("%s, %s" % (label(b, vb), label(a, va)), [(b, vb), (a, va)], is_sized(a) or is_sized(b))
        if draw and not device:
            out = C.cast((C.c_uint8 * rec_bytes)(), getattr(L, draw).argtypes[-1])
            job = cls()
            for who, a in (("ranges NULL", (None, out)), ("out NULL", (C.byref(job), None))):
                rc = getattr(L, draw)(7, 3, *(((JW, JH) if op == "erase" else ()) + a))
                rows.append(("%s: %s" % (draw, who), int(rc), L.ofdg_host_last_error().decode() if rc else ""))
    return rows


def host_job_cases(m, np):
    slot = 4096
    arena = np.zeros(slot * 48, np.uint8)
    return job_cases(m, m.lib(), arena.ctypes.data + slot, slot)


def range_dict_cases(m):
    """the ValueError of every range dict for a name it does not know, alone and beside a name it knows; through X_draw where the
    operation has one that takes the dict (splat has no dict: t=).  Anything but a ValueError ends the run: a mistake of this tool."""
    rows = []
    calls = dict(photo=lambda d: m.photo_draw(7, 3, d), spatial=lambda d: m.spatial_draw(7, 3, JW, JH, JW, JH, d), lens=lambda d: m.lens_draw(7, 3, JW, JH, d),
                 erase=lambda d: m.erase_draw(7, 3, JW, JH, d), jitter=lambda d: m.jitter_draw(7, 3, d), camera=lambda d: m.camera_draw(7, 3, d),
                 jpeg=lambda d: m.jpeg_draw(7, 3, d), motion_blur=lambda d: m.motion_blur_draw(7, 3, d))
    known = dict(photo="brightness", spatial="rot", lens="prob", erase="prob", jitter="hue", camera="blur_prob", jpeg="prob", motion_blur="prob")
    for name, fn in calls.items():
        for label, d in (("unknown range", dict(bogus=1)), ("a known range, then an unknown one", {known[name]: 0.5, "bogus": 1}),
                         ("a known range alone", {known[name]: 0.5}), ("no dict", None)):
            try:
                fn(d)
                rows.append(("%s_draw: %s" % (name, label), 0, ""))
            except ValueError as e:
                rows.append(("%s_draw: %s" % (name, label), 1, str(e)))
    return rows


def gpu_job_cases(m, torch):
    """the rules only the device entries have - the alignment of every pointer field, OFDG_STREAM_OWN before any call, `work`
    missing (a NULL among the pointer values) - and the base job of every entry as its one valid call, with a hash of the arena"""
    slot = 4096
    arena = torch.zeros(slot * 48, dtype=torch.uint8, device="cuda")
    g = m.Generator(m.default_params(width=64, height=32, mode=7, sampler=1, seed=5))  # (no call made on it: OFDG_STREAM_OWN is refused)
    rows = job_cases(m, m.lib(), arena.data_ptr() + slot, slot, device=g.h)
    torch.cuda.synchronize()
    rows.append(("bytes in the arena after every accepted job (sha256)", 0, hashlib.sha256(arena.cpu().numpy().tobytes()).hexdigest()))
    return rows


# ---- the *_format functions of the package -----------------------------------------------------------------------------------
def format_cases(m, torch):
    rows = []
    n, H, W = 2, 16, 16
    z = lambda dtype, *shape: torch.zeros(shape, dtype=dtype)  # noqa: E731
    f32, f16, u8, f64, i32, u16 = torch.float32, torch.float16, torch.uint8, torch.float64, torch.int32, torch.uint16

    def run(fn, base, rules, call):
        for label, muts in cases_of(rules):
            a = mutated(base, muts)
            try:
                call(a)
                rows.append(("%s: %s" % (fn, label), 0, ""))
            except ValueError as e:
                rows.append(("%s: %s" % (fn, label), 1, str(e)))

    def item(key, k, v):
        def f(a):
            a[key][k] = v
        return f

    def drop(key, k):
        return lambda a: a[key] is not None and a[key].pop(k)

    run("output_format", dict(image0=z(u8, n, 3, H, W), image1=z(u8, n, 3, H, W), flow=z(f16, n, 2, H, W)),
        [("image1 float32", put(image1=z(f32, n, 3, H, W))), ("images float64", put(image0=z(f64, n, 3, H, W), image1=z(f64, n, 3, H, W))),
         ("flow float64", put(flow=z(f64, n, 2, H, W))), ("image0 short", put(image0=z(u8, 1, 3, H, W))), ("image1 short", put(image1=z(u8, 1, 3, H, W))),
         ("flow short", put(flow=z(f16, n, 1, H, W)))],
        lambda a: m.output_format(a["image0"], a["image1"], a["flow"], n, H, W))

    extras = dict(flow1=z(f16, n, 2, H, W), occ0=z(u8, n, 1, H, W), occ1=z(u8, n, 1, H, W), label0=z(u8, n, H, W), label1=z(u8, n, H, W))
    run("extras_format", dict(x=extras),
        [("flow1 float32", item("x", "flow1", z(f32, n, 2, H, W))), ("flow1 shape", item("x", "flow1", z(f16, n, 1, H, W))),
         ("occ0 float16", item("x", "occ0", z(f16, n, 1, H, W))), ("occ1 float32", item("x", "occ1", z(f32, n, 1, H, W))),
         ("occ1 shape", item("x", "occ1", z(u8, n, H, W))), ("label0 float32", item("x", "label0", z(f32, n, H, W))),
         ("label1 shape", item("x", "label1", z(u8, n, 1, H, W))), ("unknown key", item("x", "depth", None))],
        lambda a: m.extras_format(a["x"], m.FMT_F16, n, H, W))
    run("extras_format", dict(x=dict(depth=None, **extras)), [("unknown key first", put()), ("flow1 float32 behind it", item("x", "flow1", z(f32, n, 2, H, W)))],
        lambda a: m.extras_format(a["x"], m.FMT_F16, n, H, W))

    run("object_table_format", dict(label0=z(u8, n, H, W), label1=z(u8, n, H, W), rows=z(u8, n, 65, 96), counts=z(i32, n), n=n),
        [("rows None", put(rows=None)), ("counts None", put(counts=None)), ("rows int32", put(rows=z(i32, n, 65, 96))), ("rows 2-d", put(rows=z(u8, n, 96))),
         ("rows 95 bytes", put(rows=z(u8, n, 65, 95))), ("rows 0 per sample", put(rows=z(u8, n, 0, 96))), ("rows 0 samples", put(rows=z(u8, 0, 65, 96))),
         ("n 3", put(n=3)), ("counts uint8", put(counts=z(u8, n))), ("counts shape", put(counts=z(i32, n, 1))), ("label0 float32", put(label0=z(f32, n, H, W))),
         ("label0 shape", put(label0=z(u8, n, 1, H, W))), ("label1 shape", put(label1=z(u8, 1, H, W)))],
        lambda a: m.object_table_format(a["label0"], a["label1"], a["rows"], a["counts"], H, W, a["n"]))

    flow_rules = [("flow float64", put(flow=z(f64, n, 2, H, W))), ("flow 3-d", put(flow=z(f32, 2, H, W))), ("flow 0 samples", put(flow=z(f32, 0, 2, H, W))),
                  ("flow 3 channels", put(flow=z(f32, n, 3, H, W))), ("occ float16", put(occ=z(f16, n, 1, H, W))), ("occ shape", put(occ=z(u8, n, H, W)))]
    run("flow_stats_format", dict(flow=z(f32, n, 2, H, W), occ=z(u8, n, 1, H, W), rows=z(u8, n, 304), one_row=False),
        [("flow None", put(flow=None)), ("rows None", put(rows=None))] + flow_rules +
        [("rows int32", put(rows=z(i32, n, 304))), ("rows shape", put(rows=z(u8, n, 300))), ("one_row with n rows", put(one_row=True))],
        lambda a: m.flow_stats_format(a["flow"], a["occ"], a["rows"], H, W, a["one_row"]))

    run("flow_pyramid_format", dict(flow=z(f32, n, 2, H, W), occ=z(u8, n, 1, H, W), levels=2, out=[z(f16, n, 2, H >> k, W >> k) for k in (1, 2)],
                                    wt=[z(u16, n, 1, H >> k, W >> k) for k in (1, 2)]),
        [("flow None", put(flow=None))] + flow_rules +
        [("levels 0", put(levels=0)), ("levels 7", put(levels=7)), ("levels 5", put(levels=5)), ("out None", put(out=None)), ("out 1 level", drop("out", 1)),
         ("out float64", item("out", 0, z(f64, n, 2, H >> 1, W >> 1))), ("level 2 float32", item("out", 1, z(f32, n, 2, H >> 2, W >> 2))),
         ("level 2 shape", item("out", 1, z(f16, n, 2, H >> 1, W >> 1))), ("weights 1 level", drop("wt", 0)),
         ("weight 1 uint8", item("wt", 0, z(u8, n, 1, H >> 1, W >> 1))), ("weight 2 shape", item("wt", 1, z(u16, n, 2, H >> 2, W >> 2)))],
        lambda a: m.flow_pyramid_format(a["flow"], a["occ"], a["levels"], a["out"], a["wt"], H, W))

    ch, cw = 8, 8
    src = dict(image0=z(u8, n, 3, H, W), image1=z(u8, n, 3, H, W), flow=z(f16, n, 2, H, W), flow1=z(f16, n, 2, H, W), occ0=z(f32, n, 1, H, W),
               occ1=z(f32, n, 1, H, W), label0=z(u8, n, H, W), label1=z(u8, n, 1, H, W))
    dst = {k: z(t.dtype, *(tuple(t.shape[:-2]) + (ch, cw))) for k, t in src.items()}

    def both(k, a, b):
        def f(args):
            args["src"][k], args["dst"][k] = a, b
        return f

    run("crop_format", dict(src=src, dst=dst),
        [("src empty", put(src={})), ("dst a list", put(dst=[])), ("unknown key in src", item("src", "depth", None)), ("unknown key in dst", item("dst", "depth", None)),
         ("dst lacks a plane", drop("dst", "occ1")), ("image0 float16", item("src", "image0", z(f16, n, 3, H, W))), ("image1 float32", item("src", "image1", z(f32, n, 3, H, W))),
         ("flow1 float32", item("src", "flow1", z(f32, n, 2, H, W))), ("flow 2-d", item("src", "flow", z(f16, H, W))), ("flow frame", item("src", "flow", z(f16, n, 2, H, W + 8))),
         ("flow 3 channels", item("src", "flow", z(f16, n, 3, H, W))), ("occ0 3-d", item("src", "occ0", z(f32, n, H, W))),
         ("flow1 0 samples", item("src", "flow1", z(f16, 0, 2, H, W))), ("occ1 3 samples", item("src", "occ1", z(f32, 3, 1, H, W))),
         ("dst occ0 uint8", item("dst", "occ0", z(u8, n, 1, ch, cw))), ("dst label0 4-d", item("dst", "label0", z(u8, n, 1, ch, cw))),
         ("dst label1 window", item("dst", "label1", z(u8, n, 1, ch, cw + 8)))],
        lambda a: m.crop_format(a["src"], a["dst"], H, W))
    one = lambda h, w: both("flow", z(f16, n, 2, H, W), z(f16, n, 2, h, w))  # noqa: E731
    run("crop_format", dict(src=dict(flow=src["flow"]), dst=dict(flow=dst["flow"])),
        [("window 4 wide", one(8, 4)), ("window 24 wide", one(8, 24)), ("window 12 wide", one(8, 12)), ("window 0 high", one(0, 8)), ("window 18 high", one(18, 8)),
         ("window 3 high", one(3, 8))],
        lambda a: m.crop_format(a["src"], a["dst"], H, W))
    return rows


# ---- the device entries ------------------------------------------------------------------------------------------------------
def gpu_cases(m, torch):
    L = m.lib()
    rows = []
    W, H, n, cw, ch = 64, 32, 2, 40, 24
    vp = C.c_void_p
    OWN = vp(m.STREAM_OWN)
    z = lambda dtype, *shape: torch.zeros(shape, dtype=dtype, device="cuda")  # noqa: E731
    adr = lambda t: t.data_ptr()  # noqa: E731
    g9 = m.Generator(m.default_params(width=W, height=H, mode=9))
    g = m.Generator(m.default_params(width=W, height=H, mode=7, sampler=1, seed=5))
    g.pool_synthetic(3, 2 * W, 2 * H, 11)
    i0, i1, fl = m.alloc_outputs(n, H, W, flow_dtype=torch.float16)
    ex = m.alloc_extras(n, H, W, flow_dtype=torch.float16, occ_dtype=torch.uint8)
    flow32, occ32 = z(torch.float32, n, 2, H, W), z(torch.float32, n, 1, H, W)
    stats = m.alloc_flow_stats(n)
    levels = [z(torch.float32, n, 2, H >> k, W >> k) for k in (1, 2)]
    table, counts = m.alloc_object_table(n)
    planes = dict(image0=i0, image1=i1, flow=fl, flow1=ex["flow1"], occ0=ex["occ0"], occ1=ex["occ1"], label0=ex["label0"], label1=ex["label1"])
    out = m.alloc_crop(planes, ch, cw)
    recs, recs_out = z(torch.int32, n, 4), z(torch.int32, n, 4)

    def answer(ctx, entry, label, rc):
        rows.append(("%s: %s" % (entry, label), int(rc), L.ofdg_last_error(ctx.h).decode() if rc else ""))

    apply = mutated
    def pyramid_record(lv):
        rec = m.FlowPyramid()
        rec.levels, rec.out_fmt = 2, m.FMT_F32
        for k in range(2):
            rec.flow[k] = lv[k]
        return rec

    def stats_call(a, entry):
        size = (a["width"], a["height"]) if entry.endswith("_sized") else ()
        return getattr(L, entry)(g.h, a["flow"], a["flow_fmt"], a["occ"], a["occ_fmt"], n, *size, 2.0, 0, adr(stats), a["stream"])

    def pyramid_call(a, entry):
        size = (a["width"], a["height"]) if entry.endswith("_sized") else ()
        rec = pyramid_record([adr(t) for t in levels])
        return getattr(L, entry)(g.h, a["flow"], a["flow_fmt"], a["occ"], a["occ_fmt"], n, *size, 0, C.byref(rec), a["stream"])

    def crop_call(a):
        job = m.CropJob()
        for k, key in enumerate(m.CROP_PLANES):
            job.src[k], job.dst[k] = a["src"][k], a["dst"][k]
        job.recs, job.recs_out, job.crop_w, job.crop_h = a["recs"], a["recs_out"], cw, ch
        job.image_fmt, job.flow_fmt, job.occ_fmt = m.FMT_F32, m.FMT_F16, m.FMT_U8
        return L.ofdg_crop(g.h, C.byref(job), n, a["stream"])

    def table_call(ctx, a):
        return L.ofdg_object_table(ctx.h, a["label0"], a["label1"], a["rows"], a["per"], a["counts"], a["stream"])

    def plane(which, k, v):
        def f(a):
            a[which][k] = v
        return f

    reduction = dict(flow=adr(flow32), flow_fmt=m.FMT_F32, occ=adr(occ32), occ_fmt=m.FMT_F32, width=W, height=H, stream=None)
    reduction_rules = [("flow NULL", put(flow=None)), ("float32 flow + 8", put(flow=adr(flow32) + 8)), ("binary16 flow + 4", put(flow=adr(fl) + 4, flow_fmt=m.FMT_F16)),
                       ("float32 occ + 4", put(occ=adr(occ32) + 4)), ("uint8 occ + 2", put(occ=adr(ex["occ0"]) + 2, occ_fmt=m.FMT_U8)), ("stream own", put(stream=OWN))]
    size_rules = [("width 4", put(width=4)), ("width 68", put(width=68)), ("height 0", put(height=0)), ("height 31", put(height=31))]
    crop_base = dict(src=[adr(planes[k]) for k in m.CROP_PLANES], dst=[adr(out[k]) for k in m.CROP_PLANES], recs=adr(recs), recs_out=adr(recs_out), stream=None)
    crop_rules = [("float32 image0 + 8", plane("src", 0, adr(i0) + 8)), ("dst image0 + 8", plane("dst", 0, adr(out["image0"]) + 8)),
                  ("binary16 flow + 4", plane("src", 2, adr(fl) + 4)), ("uint8 occ0 + 2", plane("src", 4, adr(ex["occ0"]) + 2)), ("label1 + 1", plane("src", 7, adr(ex["label1"]) + 1)),
                  ("dst label1 + 4", plane("dst", 7, adr(out["label1"]) + 4)), ("recs + 8", put(recs=adr(recs) + 8)), ("recs_out + 4", put(recs_out=adr(recs_out) + 4)),
                  ("stream own", put(stream=OWN))]
    table_base = dict(label0=adr(ex["label0"]), label1=adr(ex["label1"]), rows=adr(table), per=65, counts=adr(counts), stream=None)
    table_rules = [("rows NULL", put(rows=None)), ("counts NULL", put(counts=None)), ("rows_per_sample 0", put(per=0)), ("rows + 4", put(rows=adr(table) + 4)),
                   ("counts + 2", put(counts=adr(counts) + 2)), ("label0 + 1", put(label0=adr(ex["label0"]) + 1)), ("label1 + 2", put(label1=adr(ex["label1"]) + 2)),
                   ("stream own", put(stream=OWN))]

    def refusals(when):
        for label, muts in cases_of(reduction_rules):
            answer(g, "ofdg_flow_stats", label + when, stats_call(apply(reduction, muts), "ofdg_flow_stats"))
            answer(g, "ofdg_flow_pyramid", label + when, pyramid_call(apply(reduction, muts), "ofdg_flow_pyramid"))
        for label, muts in cases_of(size_rules + reduction_rules[:2] + reduction_rules[-1:]):
            answer(g, "ofdg_flow_stats_sized", label + when, stats_call(apply(reduction, muts), "ofdg_flow_stats_sized"))
            answer(g, "ofdg_flow_pyramid_sized", label + when, pyramid_call(apply(reduction, muts), "ofdg_flow_pyramid_sized"))
        for label, muts in cases_of(crop_rules):
            answer(g, "ofdg_crop", label + when, crop_call(apply(crop_base, muts)))
        for label, muts in cases_of(table_rules):
            answer(g, "ofdg_object_table", label + when, table_call(g, apply(table_base, muts)))

    refusals(" (before any call)")
    answer(g, "ofdg_object_table", "nothing rendered yet", table_call(g, table_base))
    answer(g9, "ofdg_object_table", "mode 9", table_call(g9, table_base))
    answer(g9, "ofdg_object_table", "mode 9 + rows NULL", table_call(g9, apply(table_base, [put(rows=None)])))
    # one valid call of each behind a render call, on the internal stream that call worked on
    s = g.next_stream()
    g.forward_counter(0, n, i0, i1, fl, s, extras=ex)
    answer(g, "ofdg_object_table", "valid, stream own", table_call(g, apply(table_base, [put(stream=OWN)])))
    answer(g, "ofdg_flow_stats", "valid, stream own", stats_call(dict(reduction, flow=adr(fl), flow_fmt=m.FMT_F16, occ=adr(ex["occ0"]), occ_fmt=m.FMT_U8, stream=OWN), "ofdg_flow_stats"))
    answer(g, "ofdg_flow_pyramid", "valid, stream own", pyramid_call(dict(reduction, flow=adr(fl), flow_fmt=m.FMT_F16, occ=adr(ex["occ0"]), occ_fmt=m.FMT_U8, stream=OWN), "ofdg_flow_pyramid"))
    job = dict(crop_base, stream=OWN, recs=None)
    answer(g, "ofdg_crop", "valid, stream own", crop_call(job))
    answer(g, "ofdg_flow_stats_sized", "valid, of the cropped flow", stats_call(dict(reduction, flow=adr(out["flow"]), flow_fmt=m.FMT_F16, occ=adr(out["occ0"]), occ_fmt=m.FMT_U8,
                                                                                width=cw, height=ch, stream=OWN), "ofdg_flow_stats_sized"))
    g.synchronize(s)
    torch.cuda.synchronize()
    written = [i0, i1, fl, table, counts, stats] + levels + [out[k] for k in m.CROP_PLANES] + [recs_out]
    h = hashlib.sha256()
    for t in written:
        h.update(t.cpu().numpy().tobytes())
    rows.append(("bytes written by the valid calls (sha256)", 0, h.hexdigest()))
    refusals(" (after a call)")
    g.synchronize()
    return rows


def emit(gpu):
    import numpy as np
    import torch
    m = importlib.import_module(PKG)
    rows = host_cases(m, np) + format_cases(m, torch) + host_job_cases(m, np) + range_dict_cases(m)
    if gpu:
        rows += gpu_cases(m, torch) + gpu_job_cases(m, torch)
    print("ROWS " + json.dumps(rows))


def side(root, lib, gpu):
    env = dict(os.environ, PYTHONPATH=root)
    if lib:
        env["OFDG_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--emit"] + (["--gpu"] if gpu else []), env=env, cwd=root, capture_output=True, text=True,
                       timeout=300)
    if r.returncode != 0:
        sys.exit("the side of %s ended with %d:\n%s\n%s" % (root, r.returncode, r.stdout[-2000:], r.stderr[-4000:]))
    return json.loads([ln for ln in r.stdout.split("\n") if ln.startswith("ROWS ")][-1][5:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--emit", action="store_true", help="(internal) print this side's answers")
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--parent-root", default=os.path.join(os.environ.get("TMPDIR", "/tmp"), "ofdg_rev_parent"))
    ap.add_argument("--parent-lib", default=os.path.join(ROOT, PKG, "lib", "libofdg_parent.so"))
    a = ap.parse_args()
    if a.emit:
        return emit(a.gpu)
    parent = side(os.path.abspath(a.parent_root), os.path.abspath(a.parent_lib), a.gpu)
    branch = side(ROOT, None, a.gpu)  # (one side after the other; a side that failed has ended the run above)
    differ = 0
    print("%d cases at the parent, %d in the working tree%s" % (len(parent), len(branch), " (with the device entries)" if a.gpu else ""))
    print("case | return code (*_format: 1 = ValueError) | error text: `same` - both sides answer this; DIFF - each side's answer below")
    inside = [r for r in parent if " sized: " in r[0] and r[1] == 0]
    if inside:
        sys.exit("the parent ACCEPTS a job whose n_samples or plane size is not the base's - it may leave the arena: %s" % inside[:5])
    entry = lambda r: r[0].split(": ")[0]  # noqa: E731
    count = {}
    for r in parent:
        count[entry(r)] = count.get(entry(r), 0) + 1
    folded = {}  # an entry of the generic generator: its equal rows as one line
    for k in range(max(len(parent), len(branch))):
        p, b = (parent[k] if k < len(parent) else None), (branch[k] if k < len(branch) else None)
        same = p == b
        differ += not same
        if same and count[entry(p)] > 60:
            f = folded.setdefault(entry(p), [0, 0, set()])
            f[0] += 1
            f[1] += p[1] != 0
            f[2].add(p[2])
        elif same:
            print("same  %-72s | %d | %s" % (p[0], p[1], p[2]))
        else:
            print("DIFF  %s\n      parent | %s\n      branch | %s" % ((p or b)[0], p and p[1:], b and b[1:]))
    for name, (cases, refused, texts) in folded.items():
        print("same  %-40s | %5d cases equal on both sides: %d accepted, %d refused with %d distinct texts" % (name, cases, cases - refused, refused, len(texts - {""})))
    print("rows that differ: %d of %d" % (differ, max(len(parent), len(branch))))
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
