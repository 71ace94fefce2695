"""What the spatial augmentation costs.  On one batch rendered at the bench's config 2 (mode 5, 512x384, batch 32, 16 objects,
counter sampler, background_prep 1, synthetic pool) with all extras, float32 and in the compact formats, on an otherwise idle
device - "kernel" lines, the median time between two events:

    spatial                ofdg_spatial 512x384 to 448x320 with records drawn from SPATIAL_FLOWNET, and with the identity record
                           (all ranges 0: the same taps as the crop's), frames only and all eight planes
    crop                   ofdg_crop writing the same destination bytes (the centred 448x320 window): the floor - the same
                           stores with no gather and no arithmetic
    grid_sample            the same warp restated with torch.nn.functional.affine_grid / grid_sample (bilinear frames, nearest
                           flow, maps and labels, the flow's transform in float32) - float32 only, for scale, not for bits

then "loader" lines: FlowLoader's samples/s with and without spatial= (extras occ0, the same config), interleaved --reps times.
With --out FILE the lines are appended to FILE too; with --tag NAME every line carries "variant": NAME (default "as built") -
for runs with OFDG_LIB set to another build.

    python tools/spatial_cost.py [--steps K] [--warmup W] [--reps R] [--pool N] [--out FILE] [--tag NAME] [--kernel-only]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def grid_sample_restatement(src, m, OW, OH):
    """The warp of the planes in src (torch tensors, float32 but for the labels) by the maps m [n, frame, row, (a b c)] with
    torch's own resampling: bilinear frames, nearest flow, maps and labels, the flow's target taken through the inverse of the
    other frame's map, all in float32.  For scale, not for bits (the maps are not even binarised)."""
    import torch
    import torch.nn.functional as F
    first = next(iter(src.values()))
    n, (H, W), dev = first.shape[0], first.shape[-2:], first.device
    # pixel coordinates to the normalised ones of grid_sample (align_corners=True): x_n = x / ((W - 1) / 2) - 1
    sx, sy, dx, dy = (W - 1) / 2.0, (H - 1) / 2.0, (OW - 1) / 2.0, (OH - 1) / 2.0
    ys, xs = torch.meshgrid(torch.arange(OH, device=dev, dtype=torch.float32), torch.arange(OW, device=dev, dtype=torch.float32), indexing="ij")
    X = torch.stack([xs, ys], 0)[None]  # [1, 2, OH, OW]
    res = {}
    for f in range(2):
        a, b, c, d, e, g = (m[:, f, r, k] for r in range(2) for k in range(3))
        theta = torch.stack([torch.stack([a * dx / sx, b * dy / sx, (a * dx + b * dy + c) / sx - 1], 1),
                             torch.stack([d * dx / sy, e * dy / sy, (d * dx + e * dy + g) / sy - 1], 1)], 1)
        grid = F.affine_grid(theta, (n, 1, OH, OW), align_corners=True)
        for name, mode in (("image%d" % f, "bilinear"), ("flow1" if f else "flow", "nearest"), ("occ%d" % f, "nearest"), ("label%d" % f, "nearest")):
            if name in src:
                t = src[name]
                t = t.float().unsqueeze(1) if t.dim() == 3 else t.float()
                res[name] = F.grid_sample(t, grid, mode=mode, padding_mode="border", align_corners=True)
        name = "flow1" if f else "flow"
        if name in res:
            q = torch.stack([(grid[..., 0] + 1) * sx, (grid[..., 1] + 1) * sy], 1)  # [n, 2, OH, OW]: the source position
            o = m[:, 1 - f]
            t = q + res[name] - o[:, :, 2, None, None]
            res[name] = torch.einsum("nij,njyx->niyx", torch.linalg.inv(o[:, :, :2]), t) - X
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pool", type=int, default=1000, help="textures of the synthetic pool")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    ap.add_argument("--tag", default="as built", help="the \"variant\" every line carries")
    ap.add_argument("--kernel-only", action="store_true", help="skip the loader: the kernels alone")
    args = ap.parse_args()
    import torch
    ofdg = importlib.import_module("optical-flow-2d-data-generation_amd")
    W, H, B, OW, OH = 512, 384, 32, 448, 320
    seed = 20261019
    params = dict(width=W, height=H, mode=5, num_objects=16, batch_size=B, sampler=1, seed=seed, background_prep=1)
    g = ofdg.Generator(ofdg.default_params(**params))
    g.pool_synthetic(args.pool, 1024, 768, 2024)

    def emit(d):
        line = json.dumps(dict(d, variant=args.tag))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    def timed(fn, reps=30):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b) * 1e3)
        return statistics.median(out), min(out)

    s = torch.cuda.current_stream().cuda_stream
    for compact in (False, True):
        if compact:
            outs = ofdg.alloc_outputs(B, H, W, image_dtype=torch.uint8, flow_dtype=torch.float16)
            ex = ofdg.alloc_extras(B, H, W, flow_dtype=torch.float16, occ_dtype=torch.uint8)
        else:
            outs = ofdg.alloc_outputs(B, H, W)
            ex = ofdg.alloc_extras(B, H, W)
        g.forward_counter(0, B, *outs, s, extras=ex)
        torch.cuda.synchronize()
        every = dict(zip(("image0", "image1", "flow"), outs), **ex)
        for what, names in (("frames only", ("image0", "image1")), ("all eight planes", tuple(every))):
            src = {k: every[k] for k in names}
            dst = ofdg.alloc_spatial(src, OH, OW)
            torch.cuda.synchronize()
            written = sum(t.numel() * t.element_size() for t in dst.values())
            window = len(names) > 2
            common = {"planes": what, "formats": "compact" if compact else "float32", "written_MB": round(written / 1e6, 1),
                      "us_store_floor_at_6_TB_per_s": round(written / 6e6, 1)}
            for records, ranges in (("drawn, SPATIAL_FLOWNET", ofdg.SPATIAL_FLOWNET), ("identity", None)):
                med, best = timed(lambda: g.spatial(src, dst, first_index=0, ranges=ranges, hflip=ranges is not None, occ_window=window, stream=s))
                emit(dict(common, kernel="spatial", records=records, us_median=round(med, 1), us_min=round(best, 1)))
            recs = torch.tensor([[(W - OW) // 2, (H - OH) // 2, 0, 0]] * B, dtype=torch.int32, device="cuda")
            med, best = timed(lambda: g.crop(src, dst, recs=recs, occ_window=window, stream=s))
            emit(dict(common, kernel="crop", us_median=round(med, 1), us_min=round(best, 1)))
            if not compact:
                import numpy as np
                maps = np.stack([ofdg.spatial_draw(seed, i, W, H, OW, OH, ofdg.SPATIAL_FLOWNET, True) for i in range(B)])
                m = torch.from_numpy(maps[:, :12].reshape(B, 2, 2, 3)).float().cuda()  # [sample, frame, row, (a b c)]
                restated = lambda: grid_sample_restatement(src, m, OW, OH)  # noqa: E731
                med, best = timed(restated, reps=10)
                emit(dict(common, kernel="grid_sample", us_median=round(med, 1), us_min=round(best, 1)))
    if args.kernel_only:
        return
    del g
    pool = lambda gen: gen.pool_synthetic(args.pool, 1024, 768, 2024)  # noqa: E731
    forms = {"loader": {}, "loader_crop": dict(crop=(OH, OW)), "loader_spatial": dict(spatial=ofdg.SPATIAL_FLOWNET, spatial_size=(OH, OW), spatial_hflip=True)}
    rate = {f: [] for f in forms}
    for rep in range(args.reps):
        for f, kw in forms.items():
            it = iter(ofdg.FlowLoader(ofdg.default_params(**params), pool=pool, prefetch=4, extras=("occ0",), **kw))
            for _ in range(args.warmup):
                next(it)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                next(it)
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
            rate[f].append(args.steps * B / el)
            emit({"form": f, "rep": rep, "samples_per_s": round(rate[f][-1], 1), "us_per_step": round(el / args.steps * 1e6, 1), "steps": args.steps, "batch": B})
            del it
    for f in forms:
        emit({"loader": f, "samples_per_s_min_max": [round(min(rate[f]), 1), round(max(rate[f]), 1)]})


if __name__ == "__main__":
    main()
