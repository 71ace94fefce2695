"""CPU tests of the product's host side (no GPU needed): the C-ABI library loads and
exports every declared symbol, the hand-written reference-stream sampler equals the
oracle's libstdc++-based one, realize's affines, the prototxt parser, error codes and
the multi-rank sharding rule (gloo, world_size 2)."""
import ctypes as C
import math
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol(ofdg):
    hdr = open(os.path.join(ROOT, "include", "ofdg.h")).read()
    declared = set(re.findall(r"\b(ofdg_[a-z0-9_]+)\s*\(", hdr))
    declared -= {"ofdg_ctx", "ofdg_layer", "ofdg_host_sampler"}
    assert len(declared) >= 25
    L = ofdg.lib()
    missing = [s for s in sorted(declared) if not hasattr(L, s)]
    assert not missing, missing
    assert set(ofdg.EXPORTS) <= declared | {"ofdg_debug_item_count"}


def test_struct_layouts_match_header(ofdg, oracle):
    # ofdg_blueprint: 17 scalars + 3 x 20 arrays + 4 trailing ints, all 4-byte fields
    assert C.sizeof(ofdg.Blueprint) == 4 * (17 + 1 + 60 + 4) == C.sizeof(oracle.Blueprint)
    assert C.sizeof(ofdg.Task) == 16 == C.sizeof(oracle.Task)
    assert C.sizeof(ofdg.Params) == 4 * 24 == C.sizeof(oracle.Params)


@pytest.mark.parametrize("mode", list(range(1, 14)))
def test_host_sampler_equals_oracle_sampler(ofdg, oracle, mode):
    """45 hand-written mt19937 streams + restated libstdc++ distributions vs <random>."""
    a = oracle.Sampler(mode)
    b = ofdg.HostSampler(mode)
    for _ in range(2):  # two calls: the stream state carries over
        ta, ba, na = a.next(25, cap=25 * 300)
        tb, bb, nb = b.next(25, cap=25 * 300)
        assert na == nb
        assert C.string_at(C.addressof(ta), C.sizeof(ta)) == C.string_at(C.addressof(tb), C.sizeof(tb))
        assert C.string_at(C.addressof(ba), na * C.sizeof(oracle.Blueprint)) == \
            C.string_at(C.addressof(bb), nb * C.sizeof(ofdg.Blueprint))


def test_host_sampler_other_sizes_and_object_override(ofdg, oracle):
    for (W, H, n) in ((1024, 768, 32), (128, 96, 1), (64, 48, 3)):
        ta, ba, na = oracle.Sampler(7, W, H, n).next(5, cap=5000)
        tb, bb, nb = ofdg.HostSampler(7, W, H, n).next(5, cap=5000)
        assert na == nb and all(t.n_objects == n for t in tb)
        assert C.string_at(C.addressof(ba), na * C.sizeof(oracle.Blueprint)) == \
            C.string_at(C.addressof(bb), nb * C.sizeof(ofdg.Blueprint))


def test_bad_mode_and_capacity(ofdg):
    for mode in (0, 14, -3):
        with pytest.raises(ofdg.OfdgError) as e:
            ofdg.HostSampler(mode)
        assert e.value.code == ofdg.EBADMODE
    with pytest.raises(ofdg.OfdgError) as e:
        ofdg.HostSampler(7).next(4, cap=8)
    assert e.value.code == ofdg.ECAPACITY


# ---- realize: fp64 affines in AGG's operation order -------------------------------
def mul(a, m):
    sx, shy, shx, sy, tx, ty = a
    return (sx * m[0] + shy * m[2], sx * m[1] + shy * m[3], shx * m[0] + sy * m[2], shx * m[1] + sy * m[3],
            tx * m[0] + ty * m[2] + m[4], tx * m[1] + ty * m[3] + m[5])


def rot(a):
    return (math.cos(a), math.sin(a), -math.sin(a), math.cos(a), 0.0, 0.0)


def inv(a):
    sx, shy, shx, sy, tx, ty = a
    d = 1.0 / (sx * sy - shy * shx)
    t0 = sy * d
    nsy = sx * d
    nshy = -shy * d
    nshx = -shx * d
    t4 = -tx * t0 - ty * nshx
    nty = -tx * nshy - ty * nsy
    return (t0, nshy, nshx, nsy, t4, nty)


def test_realize_matrices(ofdg):
    W, H = 512, 384
    ident = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)
    hs = ofdg.HostSampler(5, W, H)
    tasks, bps, n = hs.next(3)
    prm = ofdg.default_params(width=W, height=H, mode=5)
    sm, om = ofdg.host_realize(prm, 7, 1024, 768, tasks, 3, bps, n)
    si = oi = 0
    for t in tasks:
        bg = bps[t.background]
        bgm = mul(mul(mul(ident, rot(bg.rot)), (bg.scale, 0, 0, bg.scale, 0, 0)), (1, 0, 0, 1, bg.trans_x, bg.trans_y))
        intr = mul(mul(ident, rot(0.0)), (1, 0, 0, 1, float(W), float(H)))
        warp = mul(mul(inv(intr), bgm), intr)
        assert tuple(om[oi][0]) == bgm and tuple(om[oi][1]) == inv(warp)
        oi += 1
        for k in range(t.n_objects):
            b = bps[t.first_object + k]
            intrinsic = mul(mul(ident, rot(b.init_rot)), (1, 0, 0, 1, b.init_trans_x, b.init_trans_y))
            motion = mul(mul(mul(ident, rot(b.rot)), (b.scale, 0, 0, b.scale, 0, 0)), (1, 0, 0, 1, b.trans_x, b.trans_y))
            bg_n = mul(mul((1, 0, 0, 1, -W / 2., -H / 2.), bgm), (1, 0, 0, 1, W / 2., H / 2.))
            motion = mul(motion, bg_n)
            assert tuple(sm[si][0]) == intrinsic and tuple(sm[si][1]) == mul(intrinsic, motion)
            assert tuple(om[oi][0]) == motion and tuple(om[oi][1]) == inv(motion)
            si += 1
            oi += 1
    assert si == len(sm) and oi == len(om)


def _motions(b, bgm, W, H):
    """(intrinsic, motion) of a blueprint as object_motion composes them (realize.cpp: setIntrinsicTransform, setMotion,
    addBackgroundMotion)."""
    ident = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)
    intrinsic = mul(mul(ident, rot(b.init_rot)), (1, 0, 0, 1, b.init_trans_x, b.init_trans_y))
    motion = mul(mul(mul(ident, rot(b.rot)), (b.scale, 0, 0, b.scale, 0, 0)), (1, 0, 0, 1, b.trans_x, b.trans_y))
    bg_n = mul(mul((1, 0, 0, 1, -W / 2., -H / 2.), bgm), (1, 0, 0, 1, W / 2., H / 2.))
    return intrinsic, mul(motion, bg_n)


def test_realize_matrices_of_composites(ofdg):
    """Mode 7: an object's matrices come from its own (the composite's) blueprint; a composite's shape rows are its components',
    each from the component's own init_* / rot / scale / trans composed with the background motion (push_shape); a simple
    object has one shape row, its own."""
    W, H, B = 512, 384, 3
    ident = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)
    tasks, bps, n = ofdg.HostSampler(7, W, H).next(B)
    sm, om = ofdg.host_realize(ofdg.default_params(width=W, height=H, mode=7), 7, 1024, 768, tasks, B, bps, n)
    si = oi = composites = 0
    for t in tasks:
        bg = bps[t.background]
        bgm = mul(mul(mul(ident, rot(bg.rot)), (bg.scale, 0, 0, bg.scale, 0, 0)), (1, 0, 0, 1, bg.trans_x, bg.trans_y))
        assert tuple(om[oi][0]) == bgm
        oi += 1
        for k in range(t.n_objects):
            b = bps[t.first_object + k]
            _, motion = _motions(b, bgm, W, H)
            assert tuple(om[oi][0]) == motion and tuple(om[oi][1]) == inv(motion)
            oi += 1
            parts = [bps[b.first_component + j] for j in range(b.n_components)] if b.obj_type == 3 else [b]
            composites += b.obj_type == 3
            for c in parts:
                c_intrinsic, c_motion = _motions(c, bgm, W, H)
                assert tuple(sm[si][0]) == c_intrinsic and tuple(sm[si][1]) == mul(c_intrinsic, c_motion)
                si += 1
    assert composites >= 10
    assert oi == len(om) and si == len(sm)
    assert len(sm) == sum(max(1, bps[t.first_object + k].n_components) for t in tasks for k in range(t.n_objects))


def _realize(ofdg, W, H, mode, tasks, n_tasks, bps, n):
    return ofdg.host_realize(ofdg.default_params(width=W, height=H, mode=mode), 3, 2 * W, 2 * H, tasks, n_tasks, bps, n)


def test_realize_counts_at_the_capacity_limits(ofdg):
    """64 foreground objects (kMaxFgObjects) and 8 components (kMaxComponents) are taken, 65 and 9 are not."""
    import capacity_scenes as cs
    W, H, B = 128, 96, 2
    tasks, bps, n = ofdg.HostSampler(7, W, H, 64).next(B, cap=B * 1024)
    assert all(t.n_objects == 64 for t in tasks)
    sm, om = _realize(ofdg, W, H, 7, tasks, B, bps, n)
    assert len(om) == B * 65
    assert len(sm) == sum(max(1, bps[t.first_object + k].n_components) for t in tasks for k in range(t.n_objects)) > 2 * 64
    # 65: the range runs one blueprint into the task's components, still inside the array
    more = cs.clone_tasks(tasks, B)
    more[0].n_objects = 65
    assert more[0].first_object + 65 <= n
    with pytest.raises(ofdg.OfdgError) as e:
        _realize(ofdg, W, H, 7, more, B, bps, n)
    assert e.value.code == ofdg.ECAPACITY and "more than 64" in str(e.value)
    # 8 components are realised (one more shape row, the last one's own matrices), 9 and 0 are not
    one, bps1, n1, ci = cs.seven_component_composite(ofdg.HostSampler, W, H)
    sm7, om7 = _realize(ofdg, W, H, 7, one, 1, bps1, n1)
    t8, b8, n8 = cs.with_component_added(one, 1, bps1, n1, ci, source=3)
    sm8, om8 = _realize(ofdg, W, H, 7, t8, 1, b8, n8)
    assert np.array_equal(om7, om8) and len(sm8) == len(sm7) + 1 and np.array_equal(sm7, sm8[:-1])
    bg = b8[t8[0].background]
    bgm = mul(mul(mul((1.0, 0.0, 0.0, 1.0, 0.0, 0.0), rot(bg.rot)), (bg.scale, 0, 0, bg.scale, 0, 0)), (1, 0, 0, 1, bg.trans_x, bg.trans_y))
    c_intrinsic, c_motion = _motions(b8[b8[ci].first_component + 7], bgm, W, H)
    assert tuple(sm8[-1][0]) == c_intrinsic and tuple(sm8[-1][1]) == mul(c_intrinsic, c_motion)
    t9, b9, n9 = cs.with_component_added(t8, 1, b8, n8, ci, source=3)
    for bad_bps, bad_n, count in ((b9, n9, 9), (cs.clone(bps1, n1), n1, 0)):
        bad_bps[ci].n_components = count
        with pytest.raises(ofdg.OfdgError) as e:
            _realize(ofdg, W, H, 7, one if count == 0 else t9, 1, bad_bps, bad_n)
        assert e.value.code == ofdg.ECAPACITY and "component range outside [1, 8]" in str(e.value), count
    # a component run that leaves the array
    past = cs.clone(bps1, n1)
    past[ci].first_component = n1 - past[ci].n_components + 1
    with pytest.raises(ofdg.OfdgError) as e:
        _realize(ofdg, W, H, 7, one, 1, past, n1)
    assert e.value.code == ofdg.ECAPACITY and "the array" in str(e.value)
    past[ci].first_component = n1 - past[ci].n_components  # (the last run that fits is taken)
    _realize(ofdg, W, H, 7, one, 1, past, n1)


def test_realize_sorts_by_id_and_refuses_duplicates(ofdg):
    """Foreground blueprints may come in any order: objects and shapes are realised in ascending obj_id.  Two blueprints of a
    task with one id are refused (the reference would keep the last, DG:1210, and every later label / table row would shift)."""
    import capacity_scenes as cs
    W, H = 128, 96
    tasks, bps, n = ofdg.HostSampler(7, W, H, 64).next(1, cap=1024)
    sm, om = _realize(ofdg, W, H, 7, tasks, 1, bps, n)
    pt, pb, pn = cs.permuted(tasks, bps, n)  # (a composite's first_component is an index into the array: nothing to fix up)
    ids = [pb[pt[0].first_object + k].obj_id for k in range(64)]
    assert ids != sorted(ids) and sorted(ids) == [bps[tasks[0].first_object + k].obj_id for k in range(64)]
    sm_p, om_p = _realize(ofdg, W, H, 7, pt, 1, pb, pn)
    assert np.array_equal(om, om_p) and np.array_equal(sm, sm_p)
    assert len({tuple(m[0]) for m in om}) == 65  # (every object has a motion of its own: the order is visible in the rows)
    two, bps2, n2 = ofdg.HostSampler(7, W, H, 64).next(2, cap=2048)
    bps2[two[1].first_object + 63].obj_id = bps2[two[1].first_object + 7].obj_id
    with pytest.raises(ofdg.OfdgError) as e:
        _realize(ofdg, W, H, 7, two, 2, bps2, n2)
    assert e.value.code == ofdg.EINVAL and "object id 17 " in str(e.value) and "task 1" in str(e.value)
    bps2[two[1].first_object + 63].obj_id = 9  # (below the sampler's ids, distinct: accepted, and realised first)
    sm2, om2 = _realize(ofdg, W, H, 7, two, 2, bps2, n2)
    _, motion = _motions(bps2[two[1].first_object + 63], tuple(om2[65][0]), W, H)
    assert tuple(om2[66][0]) == motion


def test_realize_rejects_bad_blueprints(ofdg):
    hs = ofdg.HostSampler(5, 128, 96)
    tasks, bps, n = hs.next(1)
    prm = ofdg.default_params(width=128, height=96, mode=5)
    bps[tasks[0].first_object].obj_type = 0
    with pytest.raises(ofdg.OfdgError) as e:
        ofdg.host_realize(prm, 2, 256, 192, tasks, 1, bps, n)
    assert e.value.code == ofdg.EOBJTYPE and "Bad object type" in str(e.value)
    tasks[0].n_objects = 10 ** 6
    with pytest.raises(ofdg.OfdgError) as e:
        ofdg.host_realize(prm, 2, 256, 192, tasks, 1, bps, n)
    assert e.value.code == ofdg.EINVAL


# ---- prototxt ---------------------------------------------------------------------------
PROTOTXT = '''
layer {
  name: "gen"            # a DataGeneration layer, same fields as the reference's example
  type: "DataGeneration"
  top: "img0"
  top: "img1"
  top: "flow"
  data_param {
    batch_size: 8
    prefetch: 40
  }
  data_generation_param {
    mode: 7
    texture_dbases: "/data/textures/database.txt"
    first_level_threads: 8
    second_level_threads: 3
  }
}
'''


def test_prototxt_parser(ofdg):
    p, db, ntop = ofdg.parse_prototxt(PROTOTXT)
    assert (p.mode, p.batch_size, p.prefetch, p.first_level_threads, p.second_level_threads) == (7, 8, 40, 8, 3)
    assert p.use_antialiasing == 1 and (p.width, p.height) == (512, 384)  # proto defaults / DGEN_WIDTH x DGEN_HEIGHT
    assert db == "/data/textures/database.txt" and ntop == 3
    assert p.background_prep == 1   # the layer prepares backgrounds like the reference unless told otherwise (extension key)
    p2, _, _ = ofdg.parse_prototxt('layer { type: "DataGeneration" data_generation_param { mode: 7 background_prep: false } }')
    p3, _, _ = ofdg.parse_prototxt('layer { type: "DataGeneration" data_generation_param { mode: 7 background_prep: fast } }')
    assert (p2.background_prep, p3.background_prep) == (0, 2)
    ext = PROTOTXT.replace("mode: 7", "mode: 5 use_antialiasing: false width: 1024 height: 768 num_objects: 32")
    p, _, _ = ofdg.parse_prototxt(ext)
    assert (p.mode, p.use_antialiasing, p.width, p.height, p.num_objects) == (5, 0, 1024, 768, 32)
    with pytest.raises(ofdg.OfdgError):
        ofdg.parse_prototxt(PROTOTXT.replace("mode: 7", "moode: 7"))
    with pytest.raises(ofdg.OfdgError):
        ofdg.parse_prototxt(PROTOTXT[:-4])  # missing closing brace


def test_create_rejects_object_counts_the_sampler_cannot_hold(ofdg):
    """num_objects beyond what a sample record holds is an error, not a silent clamp: 32 for the device counter
    sampler, 64 for the reference-stream sampler (checked before any device is touched)."""
    for sampler, bad in ((1, 33), (0, 65), (0, -1)):
        with pytest.raises(ofdg.OfdgError) as e:
            ofdg.Generator(ofdg.default_params(mode=7, sampler=sampler, num_objects=bad))
        assert e.value.code == ofdg.EINVAL and "num_objects" in str(e.value)


def test_no_gpu_means_loud_failure(ofdg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(ofdg.OfdgError) as e:
        ofdg.Generator(ofdg.default_params(mode=7))
    assert e.value.code == ofdg.EHIP
    with pytest.raises(ofdg.OfdgError) as e:
        ofdg.DataGenerationLayer(PROTOTXT.replace("/data/textures/database.txt", "synthetic:2:1024:768"))
    assert "HIP" in str(e.value)


# ---- multi-rank sharding (gloo, world_size 2) -----------------------------------------------
WORKER = r'''
import ctypes as C, importlib, os, sys
sys.path.insert(0, os.environ["OFDG_ROOT"])
import torch, torch.distributed as dist
ofdg = importlib.import_module("optical-flow-2d-data-generation_amd")
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
# the one collective of the path: rank 0's stream description
hdr = torch.tensor([7, 512, 384, 0] if rank == 0 else [0, 0, 0, 0], dtype=torch.int64)
dist.broadcast(hdr, src=0)
mode, W, H, nobj = [int(v) for v in hdr]
B, steps = 4, 3
def fingerprint(bps, t):
    # position-independent fingerprint of a task (component indices depend on the array layout)
    bg, o = bps[t.background], bps[t.first_object]
    key = (t.n_objects, bg.rot, bg.scale, bg.trans_x, bg.trans_y, bg.tex_id, o.obj_type, o.init_rot, o.init_trans_x,
           o.init_trans_y, o.trans_x, o.tex_id, o.n_components)
    return hash(key) & 0x7FFFFFFFFFFF
hs = ofdg.HostSampler(mode, W, H, nobj)
mine = []
for step in range(steps):
    tasks, bps, n = hs.next(B * world, cap=B * world * 300)
    for i in range(B):
        t = tasks[rank * B + i]
        mine.append(fingerprint(bps, t))
out = [torch.zeros(len(mine), dtype=torch.int64) for _ in range(world)]
dist.all_gather(out, torch.tensor(mine, dtype=torch.int64))
if rank == 0:
    # reference: the sequential stream
    ref = []
    hs2 = ofdg.HostSampler(mode, W, H, nobj)
    tasks, bps, n = hs2.next(B * world * steps, cap=B * world * steps * 300)
    for t in tasks:
        ref.append(fingerprint(bps, t))
    got = {}
    for r in range(world):
        for k, v in enumerate(out[r].tolist()):
            step, i = divmod(k, B)
            got[step * B * world + r * B + i] = v
    assert sorted(got) == list(range(len(ref))), "shards do not cover the stream"
    assert [got[g] for g in range(len(ref))] == ref, "sharded samples differ from the sequential stream"
    assert len(set(ref)) == len(ref)
    print("SHARDING_OK")
dist.destroy_process_group()
'''


def test_sharding_two_ranks_gloo(tmp_path, ofdg):
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, OFDG_ROOT=ROOT, PYTHONHASHSEED="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), str(script)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "SHARDING_OK" in r.stdout


def test_displacer_placement_equals_oracle(ofdg, oracle):
    """Mode-9 displacer draws: hand-written mt19937 + distributions vs the oracle's <random>."""
    for (W, H, seed) in ((512, 384, 0), (512, 384, 12345), (128, 96, 7), (1024, 768, 3)):
        a = oracle.displacers(W, H, seed)
        b = ofdg.host_displacers(W, H, seed)
        assert a.shape == b.shape and np.array_equal(a, b)
    assert len(oracle.displacers(512, 384, 1)) == 63  # 9 rows x 7 columns


def test_background_prep_record_equals_oracle(ofdg, oracle):
    """The coordinate-map record of getRandomizedCrop(2W, 2H, rot, zoom, shift) (host logic of
    background_prep = 1) is the oracle's, bit for bit, over the sampler's parameter ranges."""
    import ctypes as C
    sig = [C.c_int] * 4 + [C.c_float, C.c_float, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int)]
    fp, fo = ofdg.lib().ofdg_host_bg_prep, oracle.lib().ofdg_oracle_bg_prep
    fp.argtypes = fo.argtypes = sig
    rng = np.random.default_rng(5)
    for _ in range(300):
        W, H = int(rng.choice([64, 128, 160, 512])), int(rng.choice([48, 96, 100, 384]))
        pw, ph = 2 * W + 4 * int(rng.integers(0, 40)), 2 * H + int(rng.integers(0, 90))
        angle, zoom = float(rng.uniform(-np.pi, np.pi)), float(rng.uniform(0.8, 1.2))
        sx, sy = int(rng.integers(0, 2)) * W, int(rng.integers(0, 2)) * H
        a, b = ((C.c_float * 8)(), (C.c_int * 6)()), ((C.c_float * 8)(), (C.c_int * 6)())
        assert fp(pw, ph, W, H, angle, zoom, sx, sy, *a) == 0
        fo(pw, ph, W, H, angle, zoom, sx, sy, *b)
        assert bytes(a[0]) == bytes(b[0]) and list(a[1]) == list(b[1])
    # identity parameters: the centre crop, unit steps
    assert fp(300, 200, 64, 48, 0.0, 1.0, 0, 0, *a) == 0
    assert list(a[0])[:2] == [1.0, 0.0] and list(a[0])[6:] == [1.0, 1.0] and list(a[1]) == [86, 52, 128, 96, 0, 0]


# ---- include/ofdg_detmath.h: the functions the device counter-sampler path is defined with ----
def test_detmath_is_within_one_ulp_of_libm(oracle):
    rng = np.random.default_rng(3)
    a = np.concatenate([rng.uniform(-8, 8, 400000), rng.uniform(-8, 8, 400000).astype(np.float32).astype(np.float64),
                        rng.uniform(-2000, 2000, 100000), [0.0, -0.0, math.pi, -math.pi, math.pi / 2, math.pi / 4, 1e-30, 1e-300]])
    s, c = oracle.det_sincos(a)
    def ulps(x, y):
        xi, yi = x.view(np.int64), y.view(np.int64)
        xi = np.where(xi < 0, np.int64(-2**63) - xi, xi); yi = np.where(yi < 0, np.int64(-2**63) - yi, yi)
        return np.abs(xi - yi)
    assert ulps(s, np.sin(a)).max() <= 1 and ulps(c, np.cos(a)).max() <= 1
    assert (ulps(s, np.sin(a)) > 0).mean() < 0.05
    assert s[-8] == 0.0 and c[-8] == 1.0 and np.isnan(oracle.det_sincos([1e9, np.inf, np.nan])[0]).all()
    x = np.concatenate([rng.uniform(-104, 12, 500000), [0.0, -0.0, -200.0, 100.0]]).astype(np.float32)
    e = oracle.det_expf(x)
    want = np.exp(x.astype(np.float64)).astype(np.float32)           # fp64 exp rounded once
    assert (np.abs(e.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)) > 1).sum() == 0
    assert (e != want).mean() < 1e-6 and e[-4] == 1.0 and e[-3] == 1.0 and e[-2] == 0.0 and np.isinf(e[-1])


def test_oracle_detmath_switch_only_touches_the_last_bit(oracle):
    """oracle.detmath(): same scene, affines from include/ofdg_detmath.h instead of libm - a handful of pixels may
    flip (that is why the device path is DEFINED with these functions), nothing else changes."""
    W, H = 128, 96
    tasks, bps, n = oracle.Sampler(7, W, H).next(2, cap=600)
    pool = np.random.default_rng(0).integers(0, 256, (2, 3, 2 * H, 2 * W), np.uint8)
    a = oracle.render(oracle.default_params(W, H, 7), tasks, 2, bps, n, pool)
    with oracle.detmath():
        b = oracle.render(oracle.default_params(W, H, 7), tasks, 2, bps, n, pool)
    c = oracle.render(oracle.default_params(W, H, 7), tasks, 2, bps, n, pool)
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x, z)                                   # the switch is restored
        assert (x != y).mean() < 1e-2


def test_division_free_byte_quotient_is_the_correctly_rounded_one():
    """kernels.hip byte_over_255 replaces (float)u / 255.f by a product and one Newton step: exact for all 256 bytes
    (the bare product is not), so the composite masks' strict-fp32 chain is unchanged (DG:606, 626)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("check_q255", os.path.join(os.path.dirname(__file__), "..", "tools", "check_q255.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mul, newton = mod.newton_wrong()
    assert newton == [] and len(mul) > 0


def test_integer_forms_of_the_resize_passes_equal_the_reference_arithmetic():
    """kernels.hip fix_weight / enlarge_texel_fix and the moving-average branch of cimg_resize_texel_pre replace CImg's
    double interpolation (enlarging) and float moving average (shrinking) by integer arithmetic: equal for every byte pair
    and every weight with at most 45 fractional bits (all table entries at source positions >= 128; the others are told
    apart and keep the double form), and at every sum next to a multiple of the divisor (DG:87-109, CImg get_resize)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("check_resize_fix", os.path.join(os.path.dirname(__file__), "..", "tools", "check_resize_fix.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.check_enlarging(np.random.default_rng(1)) > 4000
    assert mod.check_shrinking() < 2 ** 24


# ---- the sampler's statistics against what the REFERENCE's own sampler produced ----
# Measured during the survey with the reference's ObjectParametersGenerator (DataGenerator.cpp:1358-2835, compiled
# unmodified), 20 000 samples per mode: top-level objects, rasterised shapes, polygon vertices and curve3 segments per
# sample (mode 9: deforming objects per sample).  The reference ships no fixtures and cannot be run here, so these
# reference-measured means are what pins the thirteen-table sampler logic beyond the two mode-7 known-answer tasks.
REFERENCE_SAMPLER_STATS = {
    1: dict(objects=19.5, shapes=19.5, vertices=78.0),
    2: dict(objects=19.5, shapes=19.5, vertices=224.0),
    3: dict(objects=19.5, shapes=19.5, vertices=0.0),
    5: dict(objects=19.5, shapes=19.5, vertices=112.0, curve3=23.6),
    7: dict(objects=19.5, shapes=36.45, vertices=210.0, curve3=44.0),
    9: dict(objects=19.5, shapes=36.45, vertices=210.0, deforming=3.9),
    13: dict(objects=19.5, shapes=36.45, vertices=210.0),
}


def _sampler_stats(tasks, bps, n_tasks, n_bps):
    t = np.frombuffer(tasks, dtype=np.dtype(type(tasks[0])), count=n_tasks)
    b = np.frombuffer(bps, dtype=np.dtype(type(bps[0])), count=n_bps)
    top = np.zeros(n_bps, bool)
    for first, n in zip(t["first_object"], t["n_objects"]):   # (20 000 slices: cheap)
        top[first:first + n] = True
    composite = b["obj_type"] == 3
    comp_part = np.zeros(n_bps, bool)
    for first, n in zip(b["first_component"][top & composite], b["n_components"][top & composite]):
        comp_part[first:first + n] = True
    shape = (top & ~composite) | comp_part                   # what is rasterised
    polygon = shape & (b["obj_type"] == 2)
    seg_types = b["segment_type"][polygon]
    n_seg = b["n_segments"][polygon]
    valid = np.arange(seg_types.shape[1])[None, :] < n_seg[:, None]
    return dict(objects=top.sum() / n_tasks, shapes=shape.sum() / n_tasks, vertices=n_seg.sum() / n_tasks,
                curve3=((seg_types == 3) & valid).sum() / n_tasks,
                deforming=(top & (b["do_warpfield_deformation"] != 0)).sum() / n_tasks)


@pytest.mark.parametrize("mode", sorted(REFERENCE_SAMPLER_STATS))
def test_sampler_statistics_match_the_reference_sampler(ofdg, oracle, mode):
    """20 000 samples per mode from the oracle's sampler and from the product's host sampler: the per-sample means of
    objects / rasterised shapes / polygon vertices / curve3 segments (/ deforming objects) equal the reference-measured
    table within the sampling error (and each other exactly: same streams)."""
    N = 20000
    ref = REFERENCE_SAMPLER_STATS[mode]
    got = {}
    for name, S in (("oracle", oracle.Sampler(mode, 512, 384)), ("product", ofdg.HostSampler(mode, 512, 384))):
        tasks, bps, n = S.next(N, cap=N * 48)
        got[name] = _sampler_stats(tasks, bps, N, n)
    assert got["oracle"] == got["product"]
    for key, want in ref.items():
        have = got["product"][key]
        # tolerances: a few standard errors of the mean over 20 000 samples, plus the table's rounding
        tol = {"objects": 0.06, "shapes": 0.25, "vertices": max(1.5, 0.012 * want), "curve3": 0.03 * want + 0.2, "deforming": 0.1}[key]
        assert abs(have - want) <= tol, (mode, key, have, want)


@pytest.mark.parametrize("world,batch", [(8, 32), (8, 8), (2, 32), (1, 32), (4, 5)])
def test_shards_tile_the_sample_stream(ofdg, world, batch):
    """g = step * B * world + rank * B + i (what ofdg_forward renders on rank `rank` at step `step`): over all
    ranks the index ranges of consecutive steps cover the stream exactly once - no gap, no overlap - for the 8-GPU
    configurations of BASELINE.json (configs 4 and 5: 8 and 32 samples per GPU)."""
    steps = 5
    seen = np.zeros(steps * batch * world, np.int32)
    for step in range(steps):
        for rank in range(world):
            first = ofdg.shard_first_index(step, batch, world, rank)
            assert first == step * batch * world + rank * batch
            seen[first:first + batch] += 1
    assert (seen == 1).all()
    assert ofdg.shard_first_index(0, batch, world, world) == -1 and ofdg.shard_first_index(-1, batch, world, 0) == -1


def test_tile_index_division_by_reciprocal_is_exact():
    """bgprep_fused_kernel splits a tile's texel-pair index k into (row, pair) with k // pairs computed as
    (k * (2^20 // pairs + 1)) >> 20 (both factors below 2^24: one 24-bit multiply).  Exact over the whole range the kernel
    can reach: pairs <= 45 (a 90-texel LDS row), k < pairs * 48 rows."""
    for pairs in range(1, 46):
        inv = (1 << 20) // pairs + 1
        assert inv < (1 << 24)
        for k in range(pairs * 48 + 1):
            assert k * inv < (1 << 32)
            assert (k * inv) >> 20 == k // pairs



def test_native_image_decode_png_and_ppm(ofdg, tmp_path):
    """The layer's texture loader decodes binary PPM itself and PNG through the system's libpng (bound at run time): same
    texels as Pillow's decode, as planes in B, G, R order (TextureCollection swaps R and B, DataGenerator.cpp:129-131);
    RGB, RGBA (alpha dropped), palette and grey PNGs; anything else is refused with the loader's message."""
    from PIL import Image
    rng = np.random.RandomState(4)
    rgb = rng.randint(0, 256, (37, 53, 3)).astype(np.uint8)
    want = np.stack([rgb[:, :, 2], rgb[:, :, 1], rgb[:, :, 0]])
    p = tmp_path / "a.png"
    Image.fromarray(rgb).save(p)
    assert np.array_equal(ofdg.decode_image(p), want)
    rgba = np.dstack([rgb, rng.randint(0, 256, (37, 53)).astype(np.uint8)])
    p = tmp_path / "b.png"
    Image.fromarray(rgba, "RGBA").save(p)
    assert np.array_equal(ofdg.decode_image(p), want)                      # the stored colours, whatever the alpha
    grey = rng.randint(0, 256, (20, 31)).astype(np.uint8)
    p = tmp_path / "c.png"
    Image.fromarray(grey, "L").save(p)
    assert np.array_equal(ofdg.decode_image(p), np.stack([grey, grey, grey]))
    pal = Image.fromarray(rgb).quantize(16)
    p = tmp_path / "d.png"
    pal.save(p)
    q = np.asarray(pal.convert("RGB"))
    assert np.array_equal(ofdg.decode_image(p), np.stack([q[:, :, 2], q[:, :, 1], q[:, :, 0]]))
    p = tmp_path / "e.ppm"
    with open(p, "wb") as f:
        f.write(b"P6\n# a comment\n53 37\n255\n" + rgb.tobytes())
    assert np.array_equal(ofdg.decode_image(p), want)
    p = tmp_path / "f.bmp"
    Image.fromarray(rgb).save(p)
    with pytest.raises(ofdg.OfdgError) as e:
        ofdg.decode_image(p)
    assert e.value.code == ofdg.ETEXTURES and "neither a binary PPM" in str(e.value)
    p = tmp_path / "g.png"
    p.write_bytes(b"\x89PNG\r\n\x1a\n" + b"garbage" * 8)                     # a PNG signature and nothing behind it
    with pytest.raises(ofdg.OfdgError) as e:
        ofdg.decode_image(p)
    assert e.value.code == ofdg.ETEXTURES
    # A PNG's colour-management chunks (gAMA, cHRM, sRGB, iCCP) would make libpng's 8-bit sRGB output re-encode the samples; the
    # reference's CImg::load keeps raw values (DataGenerator.cpp:128): the loader decodes from memory without those chunks, so
    # the stored bytes come out whatever gamma the file claims.  16 bits per sample are refused, with the way out in the message.
    import struct
    from PIL import PngImagePlugin

    def with_chunks(gamma=None, srgb=False):
        info = PngImagePlugin.PngInfo()
        if srgb:
            info.add(b"sRGB", b"\x00")
        if gamma is not None:
            info.add(b"gAMA", struct.pack(">I", int(round(gamma * 100000))))
        return info
    for name, info in (("h", with_chunks(1.0)), ("i", with_chunks(0.45455)), ("i2", with_chunks(0.0)), ("i3", with_chunks(0.3, srgb=True)), ("i4", with_chunks(srgb=True))):
        p = tmp_path / (name + ".png")
        Image.fromarray(rgb).save(p, pnginfo=info)
        assert np.array_equal(ofdg.decode_image(p), want), name
    p = tmp_path / "j.png"
    Image.fromarray((grey.astype(np.uint16) * 257)).save(p)                # mode I;16
    with pytest.raises(ofdg.OfdgError) as e:
        ofdg.decode_image(p)
    assert e.value.code == ofdg.ETEXTURES and "16-bit" in str(e.value)
