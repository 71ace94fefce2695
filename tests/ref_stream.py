"""Helpers of the reference-pinning tests (tests/test_ref_pinning.py, tests/test_gpu_ref_pinning.py) and of their
fixture generator (tests/golden/gen_ref_goldens.py).  TEST INFRASTRUCTURE.

The fixtures under tests/golden/ref_* were written by the REFERENCE's own compiled code (oracle/ref_*_harness.cpp,
built into oracle/_ref/ where the reference checkout exists); this module holds what both sides share: the canonical
byte stream of a task (layout: oracle/ref_tasks.h), digests, NaN canonicalisation and the warp-field sets.
"""
import hashlib
import json
import os
import struct

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_BIN = os.path.join(ROOT, "oracle", "_ref")

N_TASKS = 200          # tasks per mode of the sampler fixture
N_FULL = 2             # of which the first N_FULL are stored in full
MODES = tuple(range(1, 14))

# seeded warp-field sets (frame W, H, seed): the smallest frames whose 3 * max(W, H) field holds displacers at all
# (spacing 200), and one that holds all three displacer types
WARP_SETS = {"w128_s11": (128, 96, 11), "w256_s3": (256, 192, 3)}
# a hand-made set of four strong displacers on a 96 x 96 field: 27 % of the forward and 7 % of the backward texels
# leave the field and are flagged (NaN)
HAND_SIZE = 96
HAND_DISPLACERS = np.array([
    # type, p0, p1, p2, support cx, cy, sigma_x, sigma_y, angle
    [0, 4.0e-4, -2.0e-4, 0, 30, 30, 25, 30, 0.5],
    [1, 60, 40, 1.2e-5, 58, 44, 30, 20, -0.7],
    [2, 50, 60, 1 + 8.0e-6, 52, 57, 22, 28, 1.1],
    [0, -3.0e-4, 5.0e-4, 0, 72, 70, 20, 15, -1.0],
], np.float64)
STRIDE = 8             # the fixture keeps every STRIDE-th texel of the seeded fields for diagnosis


# ---- the task stream ---------------------------------------------------------------------------------------------
_SCALARS = (("obj_id", "i"), ("obj_type", "i"), ("init_rot", "f"), ("init_scale", "f"), ("init_trans_x", "f"),
            ("init_trans_y", "f"), ("rot", "f"), ("scale", "f"), ("trans_x", "f"), ("trans_y", "f"), ("tex_id", "i"),
            ("tex_rot", "f"), ("tex_scale", "f"), ("tex_shift_x", "i"), ("tex_shift_y", "i"), ("ellipse_scale_x", "f"),
            ("ellipse_scale_y", "f"))
FIELD_NAMES = [n for n, _ in _SCALARS]


def blueprint_bytes(bps, i):
    """Blueprint i of the flat array of the oracle / the product (include/ofdg.h, ofdg_blueprint) in the layout of
    oracle/ref_tasks.h: members in the reference's declaration order, components recursed in place."""
    b = bps[i]
    out = [struct.pack("<" + "".join(k for _, k in _SCALARS), *(getattr(b, n) for n, _ in _SCALARS))]
    out.append(struct.pack("<i", b.n_segments))
    for k in range(b.n_segments):
        out.append(struct.pack("<iff", b.segment_type[k], b.segment_x[k], b.segment_y[k]))
    out.append(struct.pack("<i", b.n_components))
    for k in range(b.n_components):
        out.append(blueprint_bytes(bps, b.first_component + k))
    out.append(struct.pack("<ii", b.is_additive_component, b.do_warpfield_deformation))
    return b"".join(out)


def task_bytes(tasks, bps, t):
    task = tasks[t]
    out = [blueprint_bytes(bps, task.background), struct.pack("<i", task.n_objects)]
    out += [blueprint_bytes(bps, task.first_object + k) for k in range(task.n_objects)]
    return b"".join(out)


def sampler_task_bytes(sampler, n_tasks):
    """[bytes] of the next n_tasks tasks of an oracle.Sampler / ofdg.HostSampler."""
    tasks, bps, _ = sampler.next(n_tasks, cap=n_tasks * 400)
    return [task_bytes(tasks, bps, t) for t in range(n_tasks)]


def task_digest(b):
    return hashlib.sha256(b).hexdigest()[:12]


def parse_blueprint(buf, off=0):
    """Inverse of blueprint_bytes for diagnosis: (dict, next offset)."""
    d = {}
    for n, k in _SCALARS:
        d[n] = struct.unpack_from("<" + k, buf, off)[0]
        off += 4
    ns = struct.unpack_from("<i", buf, off)[0]
    off += 4
    d["segments"] = [struct.unpack_from("<iff", buf, off + 12 * k) for k in range(ns)]
    off += 12 * ns
    nc = struct.unpack_from("<i", buf, off)[0]
    off += 4
    d["components"] = []
    for _ in range(nc):
        c, off = parse_blueprint(buf, off)
        d["components"].append(c)
    d["is_additive_component"], d["do_warpfield_deformation"] = struct.unpack_from("<ii", buf, off)
    return d, off + 8


def parse_task(buf):
    bg, off = parse_blueprint(buf, 0)
    n = struct.unpack_from("<i", buf, off)[0]
    off += 4
    objs = []
    for _ in range(n):
        o, off = parse_blueprint(buf, off)
        objs.append(o)
    assert off == len(buf), (off, len(buf))
    return [bg] + objs


def first_difference(got, want):
    """Names the first blueprint and member in which two task byte strings differ (for assertion messages)."""
    try:
        a, b = parse_task(got), parse_task(want)
    except Exception as e:  # a stream that does not even parse
        return "unparsable (%s); first differing byte %d" % (e, next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), -1))

    def walk(x, y, path):
        for k in list(FIELD_NAMES) + ["segments", "is_additive_component", "do_warpfield_deformation"]:
            if struct.pack("<f", x[k]) != struct.pack("<f", y[k]) if isinstance(x[k], float) else x[k] != y[k]:
                return "%s.%s: got %r, reference %r" % (path, k, x[k], y[k])
        if len(x["components"]) != len(y["components"]):
            return "%s: %d components, reference %d" % (path, len(x["components"]), len(y["components"]))
        for i, (cx, cy) in enumerate(zip(x["components"], y["components"])):
            r = walk(cx, cy, "%s.component[%d]" % (path, i))
            if r:
                return r
        return None

    if len(a) != len(b):
        return "%d blueprints, reference %d" % (len(a), len(b))
    for i, (x, y) in enumerate(zip(a, b)):
        r = walk(x, y, "background" if i == 0 else "object[%d]" % (i - 1))
        if r:
            return r
    return "no difference found"


# ---- float fields --------------------------------------------------------------------------------------------------
def canon_bits(a):
    """float32 array -> uint32 bit patterns with every NaN replaced by the one quiet NaN 0x7FC00000 (the reference
    writes signalling NaNs into flagged texels, the oracle and the device quiet ones)."""
    a = np.ascontiguousarray(a, np.float32)
    bits = a.view(np.uint32).copy()
    bits[np.isnan(a)] = 0x7FC00000
    return bits


def field_digest(a):
    return hashlib.sha256(canon_bits(a).astype("<u4").tobytes()).hexdigest()


def crop_origins(W, H):
    """(x, y) of the crops of one big field in serving order.  This is the generator's and the tests' OWN statement of
    the reference's crop loop (WarpFields.cpp:617-633) - a third one, independent of the oracle's crop_origins and
    of the product's: the fixture's crops are sliced with it, in Python, from the field the reference's code made."""
    big = 3 * max(W, H)
    return [(x, y) for y in range(H // 4, big - 5 * H // 4, H // 3) for x in range(W // 4, big - 5 * W // 4, W // 3)]


def crops_of(field, W, H):
    """field float32 [4, big, big] (flow x, y, iflow x, y) -> [n, 4, H+1, W+1], the (W+1) x (H+1) crops
    get_crop(x, y, x+W, y+H) (both ends inclusive)."""
    return np.stack([field[:, y:y + H + 1, x:x + W + 1] for (x, y) in crop_origins(W, H)])


def load_json(name):
    with open(os.path.join(GOLD, name)) as f:
        return json.load(f)


# ---- motions ------------------------------------------------------------------------------------------------------
def hex_f64(words):
    return np.array([int(w, 16) for w in words], np.uint64).view(np.float64)


def hex_f32_pairs(s):
    """The harness's flow string -> float32 [n, 2] (u, v)."""
    return np.array([int(s[i:i + 8], 16) for i in range(0, len(s), 8)], np.uint32).view(np.float32).reshape(-1, 2)


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)
