"""Engineered samples at the render path's capacity limits (64 foreground objects, 8 components): TEST INFRASTRUCTURE shared
by tests/test_gpu_capacity.py (the device against the oracle) and tests/test_capacity_scenes.py (the conditions these inputs
must meet, on the oracle alone).  Sampler-drawn samples of 64 objects hide most of their early objects under later ones, so
the tile masks' upper bits are set in few tiles; the scenes here are built so that every painter's position owns pixels.

`S` below is a sampler class (oracle_lib.Sampler or the package's HostSampler: same streams, same records)."""
import ctypes as C

import numpy as np

N_OBJ = 64  # kMaxFgObjects
TILE_W, TILE_H = 64, 16  # compose's tile (kTileW x kTileH)
CAP = 4096

SIZES = [(128, 96), (160, 100)]  # compose_rigid_pow2_kernel / compose_rigid_kernel (any width)
# Sampler-drawn cases (W, H, mode, use_antialiasing, B).  B is the smallest batch in which, in the oracle's labels, at least 8
# painter's positions above 32 own pixels in each frame.  Counted on the reference (frame 0 / frame 1, the first samples of
# Sampler(mode, W, H, 64)): mode 5 shows 4 / 8 in its first sample at 128x96 and 6 / 9 at 160x100 (the second: 13 / 12 and
# 13 / 14), so B = 2; mode 7 shows 13 / 13 and 13 / 12 in its first, and 11 / 12 at 256x192 (more than one tile row and column
# per band), so B = 1.
DRAWN = [(128, 96, 5, 1, 2), (160, 100, 5, 1, 2), (128, 96, 7, 1, 1), (160, 100, 7, 1, 1), (128, 96, 7, 0, 1), (256, 192, 7, 1, 1)]
# The concentric stack around the frame's centre; at 160x100 also around (64, 48), a tile corner as at 128x96 (around (80, 50)
# the richest tile of the 160x100 frame shows 55 of the 65 positions)
STACKS = [(128, 96, "stack"), (160, 100, "stack"), (160, 100, "stack_at_tile_corner")]
GRIDS = ("grid", "grid_upper_half", "grid_low_offscreen")
MODE9_B = 2  # of the first two samples of Sampler(9, W, H, 64), 5 + 4 foreground objects with a local index >= 32 deform


def clone(bps, n_bps, cap=None):
    """A writable copy of the first n_bps blueprints, in an array of `cap` records."""
    out = (type(bps[0]) * max(cap or n_bps, n_bps))()
    C.memmove(out, bps, n_bps * C.sizeof(type(bps[0])))
    return out


def clone_tasks(tasks, n):
    out = (type(tasks[0]) * n)()
    C.memmove(out, tasks, n * C.sizeof(type(tasks[0])))
    return out


def _ellipses(S, W, H, place):
    """The 64 blueprints of a mode-5 sample, each rewritten as an unrotated ellipse with centre and radii place(k) and a small
    motion of its own (so that neighbouring objects' flows differ)."""
    tasks, bps, n = S(5, W, H, N_OBJ).next(1, cap=CAP)
    t = tasks[0]
    assert t.n_objects == N_OBJ
    for k in range(N_OBJ):
        b = bps[t.first_object + k]
        cx, cy, rx, ry = place(k)
        b.obj_type = 1
        b.init_rot = 0.0
        b.init_trans_x, b.init_trans_y = cx, cy
        b.ellipse_scale_x, b.ellipse_scale_y = rx, ry
        b.rot = 0.002 * (k % 5 - 2)
        b.scale = 1 + 0.001 * (k % 3 - 1)
        b.trans_x = 0.3 * (k % 7 - 3)
        b.trans_y = 0.2 * (k % 4 - 1)
    return tasks, bps, n


def stack(S, W, H, centre=None):
    """Concentric ellipses around `centre` (default: the frame's), each smaller than the one below it: every object shows as a
    ring.  Around a corner of compose's tile grid - (64, 48), the centre of a 128x96 frame - the four tiles that meet there hold
    all 65 painter's positions: full 64-bit tile masks, 64 visits of a wave."""
    cx, cy = centre or (W / 2.0, H / 2.0)
    return _ellipses(S, W, H, lambda k: (cx, cy, 66.0 - k, 50.0 - 0.75 * k))


def grid_centre(k):
    return 8.0 + 16.0 * (k % 8), 6.0 + 12.0 * (k // 8)


def grid(S, W, H):
    """8 x 8 small ellipses side by side: every object shows, each tile's mask holds a few bits, most of them high."""
    return _ellipses(S, W, H, lambda k: grid_centre(k) + (7.0, 5.0))


def grid_upper_half(S, W, H):
    """The grid with objects 33..64 only (the task's range moved): they take painter's positions 1..32."""
    tasks, bps, n = grid(S, W, H)
    tasks[0].first_object += 32
    tasks[0].n_objects = 32
    return tasks, bps, n


def grid_low_offscreen(S, W, H):
    """The grid with objects 1..32 moved out of the frame: every tile mask has a zero low word, the first object a wave visits
    (and prefetches) has an index above 32."""
    tasks, bps, n = grid(S, W, H)
    for k in range(32):
        bps[tasks[0].first_object + k].init_trans_x = -500.0
    return tasks, bps, n


def permuted(tasks, bps, n, seed=2):
    """The same sample with its foreground blueprints in another order inside the task's range (mode-5 scenes: no composites,
    no index to fix up)."""
    t = tasks[0]
    out = clone(bps, n)
    perm = np.random.RandomState(seed).permutation(t.n_objects)
    assert list(perm) != sorted(perm)
    for dst, src in enumerate(perm):
        out[t.first_object + dst] = bps[t.first_object + int(src)]
    return clone_tasks(tasks, 1), out, n


def positions(label):
    """Painter's positions that own at least one pixel of a label plane."""
    return set(int(v) for v in np.unique(label))


def high_positions(label):
    return set(p for p in positions(label) if p > 32)


def full_tiles(label, n_positions=N_OBJ + 1):
    """Tiles of compose's grid in which all n_positions labels appear."""
    H, W = label.shape
    return [(ty, tx) for ty in range(0, H, TILE_H) for tx in range(0, W, TILE_W)
            if len(np.unique(label[ty:ty + TILE_H, tx:tx + TILE_W])) == n_positions]


def with_component_added(tasks, n_tasks, bps, n_bps, obj_index, source=0, shift=(3.0, -2.0)):
    """A copy of the batch in which the composite blueprint at obj_index has one more component, inserted at the end of its run:
    a copy of its component `source`, moved by `shift` and with is_additive_component flipped.  Every first_component /
    first_object / background index behind the insertion point moves up by one."""
    comp = bps[obj_index]
    assert comp.obj_type == 3
    at = comp.first_component + comp.n_components
    out = (type(bps[0]) * (n_bps + 1))()
    for i in range(n_bps):
        out[i + (i >= at)] = bps[i]
    extra = clone(bps, n_bps)[comp.first_component + source]
    extra.init_trans_x += shift[0]
    extra.init_trans_y += shift[1]
    extra.is_additive_component = 0 if extra.is_additive_component else 1
    out[at] = extra
    assert obj_index < at  # (a task's components lie behind its top-level blueprints)
    for i in range(n_bps + 1):
        if out[i].obj_type == 3 and out[i].first_component >= at:
            out[i].first_component += 1
    out[obj_index].n_components += 1
    new_tasks = clone_tasks(tasks, n_tasks)
    for t in new_tasks:
        if t.background >= at:
            t.background += 1
        if t.first_object >= at:
            t.first_object += 1
    return new_tasks, out, n_bps + 1


COMPOSITE_AT = (2, 53)  # (sample, local index) of the composite below in the stream of Sampler(7, W, H, 64)


def seven_component_composite(S, W, H):
    """(tasks, bps, n_bps, blueprint index): the third sample of Sampler(7, W, H, 64), cut behind its 54th object - a composite of
    7 components, additive [1, 1, 1, 0, 0, 0, 0], that lies inside the frame.  Nothing is drawn on top of it, so it owns the
    pixels of its mask, at painter's position 54."""
    ti, local = COMPOSITE_AT
    tasks, bps, n = S(7, W, H, N_OBJ).next(ti + 1, cap=CAP)
    one = (type(tasks[0]) * 1)()
    C.memmove(one, C.byref(tasks[ti]), C.sizeof(tasks[ti]))
    one[0].n_objects = local + 1
    oi = one[0].first_object + local
    b = bps[oi]
    assert b.obj_type == 3 and b.n_components == 7
    assert [bps[b.first_component + k].is_additive_component for k in range(7)] == [1, 1, 1, 0, 0, 0, 0]
    return one, bps, n, oi


def richest_tile(label0, label1):
    """The largest number of positions that one tile of compose's grid shows in either frame (a lower bound of the bits set in
    its mask, the background counted)."""
    H, W = label0.shape
    return max(len(set(np.unique(label0[ty:ty + TILE_H, tx:tx + TILE_W])) | set(np.unique(label1[ty:ty + TILE_H, tx:tx + TILE_W])))
               for ty in range(0, H, TILE_H) for tx in range(0, W, TILE_W))


def many_ellipses(S, W, H, n):
    """One task whose range runs over n top-level blueprints: copies of one small ellipse with distinct ids, spread over the frame."""
    tasks, bps, n_bps = grid(S, W, H)
    t = tasks[0]
    out = (type(bps[0]) * (t.first_object + n))()
    for i in range(t.first_object):
        out[i] = bps[i]
    for k in range(n):
        out[t.first_object + k] = bps[t.first_object + 9]
        b = out[t.first_object + k]
        b.obj_id = 10 + k
        b.init_trans_x, b.init_trans_y = grid_centre(k % 64)
        if k >= 64:
            b.init_trans_x += 8.0
    new_tasks = clone_tasks(tasks, 1)
    new_tasks[0].n_objects = n
    return new_tasks, out, t.first_object + n


def stack_at_tile_corner(S, W, H):
    return stack(S, W, H, centre=(64.0, 48.0))


def deforming_high(tasks, bps):
    """Foreground objects of the batch with a local index of 32 or more whose blueprint asks for a warp-field deformation."""
    return sum(1 for t in tasks for i in range(32, t.n_objects) if bps[t.first_object + i].do_warpfield_deformation)
