"""numpy restatement of the optional outputs (include/ofdg.h, ofdg_extras): backward flow, the index images of both
frames as painter's positions, occlusion maps.  TEST INFRASTRUCTURE, built from the oracle's non-AA masks
(oracle.shape_masks, composites composed through oracle.tables()) and the motions of ofdg.host_realize:

  labels   RenderCore::blitObject (DG:762-775): in ascending obj_id, an object owns the pixels where its non-AA mask of
           that frame is 255; 0 = background, k = the k-th top-level foreground object
  flow     RenderCore::computeFlowImage(objects_map, inverse) (DG:801-818) with getPointFlow (DG:388-407 foreground,
           DG:692-718 background): fp64 affines, fp32 save / result casts; inverse uses m_motion_inv = invert(m_motion)
           (agg::trans_affine::invert, DG:320-321, 333-334)
  occ      1 where (int)floorf((float)x + u + 0.5f) (likewise y, fp32 as written) leaves the frame or lands on a pixel of the
           other frame with another label
"""
import numpy as np

F32, F64 = np.float32, np.float64


# ---- agg::trans_affine, members (sx, shy, shx, sy, tx, ty) ----
def mat_mul(a, m):  # a *= m
    sx, shy, shx, sy, tx, ty = a
    return (sx * m[0] + shy * m[2], sx * m[1] + shy * m[3], shx * m[0] + sy * m[2], shx * m[1] + sy * m[3],
            tx * m[0] + ty * m[2] + m[4], tx * m[1] + ty * m[3] + m[5])


def mat_invert(a):  # trans_affine::invert (AGG 2.4)
    sx, shy, shx, sy, tx, ty = (float(v) for v in a)
    d = 1.0 / (sx * sy - shy * shx)
    t0 = sy * d
    r_sy = sx * d
    r_shy = -shy * d
    r_shx = -shx * d
    t4 = -tx * t0 - ty * r_shx
    r_ty = -tx * r_shy - ty * r_sy
    return (t0, r_shy, r_shx, r_sy, t4, r_ty)


def transform(m, x, y):  # trans_affine::transform on float64 arrays
    sx, shy, shx, sy, tx, ty = (F64(v) for v in m)
    return x * sx + y * shx + tx, x * shy + y * sy + ty


def point_flow_fg(m, xs, ys):
    """MovingObjectBase::getPointFlow (DG:388-407) of pixels (xs, ys) under m (motion, or its inverse)."""
    ix, iy = xs.astype(F64), ys.astype(F64)
    sx, sy = xs.astype(F32), ys.astype(F32)
    ix, iy = transform(m, ix, iy)
    return (ix - sx.astype(F64)).astype(F32), (iy - sy.astype(F64)).astype(F32)


def point_flow_bg(m, W, H, xs, ys):
    """MovingObjectBackground::getPointFlow (DG:692-718): the detour through the 2W x 2H texture's coordinates."""
    ix = (xs.astype(F32) + F32(W // 2)).astype(F64)
    iy = (ys.astype(F32) + F32(H // 2)).astype(F64)
    save_x, save_y = ix.astype(F32), iy.astype(F32)
    intrinsic = mat_mul(mat_mul((1.0, 0.0, 0.0, 1.0, 0.0, 0.0), (np.cos(0.0), np.sin(0.0), -np.sin(0.0), np.cos(0.0), 0.0, 0.0)),
                        (1.0, 0.0, 0.0, 1.0, float(W), float(H)))  # setIntrinsicTransform(0.f, W, H)
    ix, iy = transform(mat_invert(intrinsic), ix, iy)
    ix, iy = transform(m, ix, iy)
    ix, iy = transform(intrinsic, ix, iy)
    return (ix - save_x.astype(F64)).astype(F32), (iy - save_y.astype(F64)).astype(F32)


def occlusion(flow, own, other):
    """flow [2,H,W] of one frame, its labels `own` [H,W], the other frame's labels: float32 [1,H,W]."""
    _, H, W = flow.shape
    ys, xs = np.mgrid[0:H, 0:W]
    fx = np.floor((xs.astype(F32) + flow[0]) + F32(0.5))
    fy = np.floor((ys.astype(F32) + flow[1]) + F32(0.5))
    inside = (fx >= 0) & (fx < W) & (fy >= 0) & (fy < H)
    xr = np.where(inside, fx, 0).astype(np.int64)
    yr = np.where(inside, fy, 0).astype(np.int64)
    same = inside & (other[yr, xr] == own)
    return np.where(same, F32(0), F32(1))[None].astype(F32)


def labels_of(oracle, oparams, task, bps, pool):
    """(label0, label1) uint8 [H,W] of one task and its painter's order (blueprint indices by ascending obj_id)."""
    add, sub, _ = oracle.tables()
    masks = oracle.shape_masks(oparams, task, bps, pool, max_shapes=512)
    H, W = oparams.height, oparams.width
    # rasterised shapes in realisation order: top-level objects in task order, a composite's components in order
    owner_shapes, k = {}, 0
    objs = [task.first_object + i for i in range(task.n_objects)]
    for bi in objs:
        b = bps[bi]
        if b.obj_type == 3:
            owner_shapes[bi] = [(k + j, bool(bps[b.first_component + j].is_additive_component)) for j in range(b.n_components)]
            k += b.n_components
        else:
            owner_shapes[bi] = [(k, True)]
            k += 1
    assert k == len(masks), (k, len(masks))
    order = sorted(objs, key=lambda bi: bps[bi].obj_id)
    labels = []
    for f in (0, 1):
        lab = np.zeros((H, W), np.uint8)
        for pos, bi in enumerate(order, 1):
            if bps[bi].obj_type == 3:  # MovingObjectComposite::renderMasks (DG:591-646), non-AA
                u = np.zeros((H, W), np.uint8)
                for sh, additive in owner_shapes[bi]:
                    v = masks[sh, 2 + f]
                    u = (add if additive else sub)[u, v]
            else:
                u = masks[owner_shapes[bi][0][0], 2 + f]
            lab[u == 255] = pos
        labels.append(lab)
    return labels[0], labels[1], order


def reference_extras(ofdg, oracle, oparams, tasks, n_tasks, bps, n_bps, pool):
    """All optional outputs of a batch plus the forward flow rebuilt from label0 (what pins the helper to the oracle):
    dict of numpy arrays label0, label1 [n,H,W] uint8, flow, flow1 [n,2,H,W] float32, occ0, occ1 [n,1,H,W] float32."""
    pool = np.ascontiguousarray(pool, np.uint8)
    pn, _, ph, pw = pool.shape
    W, H = oparams.width, oparams.height
    prm = ofdg.default_params(width=W, height=H, mode=oparams.mode)
    _, om = ofdg.host_realize(prm, pn, pw, ph, tasks, n_tasks, bps, n_bps, cap=max(4096, n_tasks * 200))
    out = {k: [] for k in ("label0", "label1", "flow", "flow1", "occ0", "occ1")}
    ys, xs = np.mgrid[0:H, 0:W]
    base = 0
    for t in range(n_tasks):
        task = tasks[t]
        l0, l1, order = labels_of(oracle, oparams, task, bps, pool)
        motions = [om[base + k, 0] for k in range(1 + len(order))]  # background, then the objects in painter's order
        base += 1 + len(order)
        flows = []
        for lab, inverse in ((l0, False), (l1, True)):
            fl = np.zeros((2, H, W), F32)
            for pos, m in enumerate(motions):
                sel = lab == pos
                if not sel.any():
                    continue
                mm = mat_invert(m) if inverse else tuple(m)
                if pos == 0:
                    u, v = point_flow_bg(mm, W, H, xs[sel], ys[sel])
                else:
                    u, v = point_flow_fg(mm, xs[sel], ys[sel])
                fl[0][sel], fl[1][sel] = u, v
            flows.append(fl)
        out["label0"].append(l0); out["label1"].append(l1)
        out["flow"].append(flows[0]); out["flow1"].append(flows[1])
        out["occ0"].append(occlusion(flows[0], l0, l1)); out["occ1"].append(occlusion(flows[1], l1, l0))
    return {k: np.stack(v) for k, v in out.items()}


def ulp_diff(a, b):
    a = np.ascontiguousarray(a, F32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, F32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7FFFFFFF), a)
    b = np.where(b < 0, -(b & 0x7FFFFFFF), b)
    return np.abs(a - b)
