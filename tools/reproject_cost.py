"""What reprojection costs: ofdg_reproject alone on one batch of the bench's config 2 (mode 5, 512x384, batch 32, 16 objects,
counter sampler, background_prep 1, synthetic pool) rendered with flow1, occ0 and occ1, float32 and in the compact formats, on
an otherwise idle device - the median of 30 calls between two events ("us_median": it holds what issuing the call from Python
costs, some 20 us) and the device time of one call among ten queued behind a long matrix product ("us_device"), --rounds
interleaved rounds of all rows, one JSON line per row and round:

    reproject    outputs rows only / warped + err + mask / everything (warped, err, mask, fb2, rows) x float32 / uint8 frames
                 x float32 / binary16 flow x frame 0 / both frames.  "moved_MB": the bytes of the planes read once and the
                 planes written (the gathered reads counted once).  "x_spatial" / "x_mblur": us_device over the comparisons' of
                 the same round, formats and frames.
    spatial      a comparison: ofdg_spatial, frames only, under the identity record at the same size and formats - one
                 bilinear tap per pixel, the frames' bytes read and written.
    motion_blur  a comparison: ofdg_motion_blur at taps_side 1 and shutter 1 - up to three taps per pixel of the own frame.
    grid_sample  an eager torch restatement for scale, float32 only, frame 0: grid_sample of image1 at the flow's targets, the
                 residual against image0, grid_sample of flow1 and the squared forward-backward residual - not for bits.

Then "loader" lines: FlowLoader at config 2 with extras flow1, occ0, occ1, with and without reproject= (rows, both frames),
--reps interleaved repetitions of --steps steps.  With --out FILE the lines are appended to FILE too; with --tag NAME every
line carries "variant": NAME (default "as built") - for runs with OFDG_LIB set to another build (tools/build_variant.sh).

    python tools/reproject_cost.py [--rounds R] [--steps K] [--warmup W] [--reps R] [--pool N] [--out FILE] [--tag NAME] [--kernel-only]
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

FORMS = (("rows", ("rows",)), ("warped+err+mask", ("warped", "err", "mask")), ("everything", ("warped", "err", "mask", "fb2", "rows")))


def grid_sample_restatement(image0, image1, flow, flow1):
    """frame 0 the framework way: the warped frame, the photometric residual and the squared forward-backward residual"""
    import torch
    import torch.nn.functional as F
    n, _, H, W = image0.shape
    ys, xs = torch.meshgrid(torch.arange(H, device=flow.device, dtype=torch.float32), torch.arange(W, device=flow.device, dtype=torch.float32), indexing="ij")
    fl = flow.float()
    grid = torch.stack([(xs + fl[:, 0]) / ((W - 1) / 2.0) - 1.0, (ys + fl[:, 1]) / ((H - 1) / 2.0) - 1.0], -1)
    warped = F.grid_sample(image1.float(), grid, mode="bilinear", padding_mode="border", align_corners=True)
    err = (warped - image0.float()).abs().amax(dim=1, keepdim=True)
    back = F.grid_sample(flow1.float(), grid, mode="bilinear", padding_mode="border", align_corners=True)
    fb2 = ((fl + back) ** 2).sum(dim=1, keepdim=True)
    mask = (grid.abs() <= 1.0).all(dim=-1)
    return warped, err, fb2, mask


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pool", type=int, default=1000, help="textures of the synthetic pool")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    ap.add_argument("--tag", default="as built", help="the \"variant\" every line carries")
    ap.add_argument("--kernel-only", action="store_true", help="skip the loader lines")
    args = ap.parse_args()
    import torch
    ofdg = importlib.import_module("optical-flow-2d-data-generation_amd")
    W, H, B = 512, 384, 32
    seed = 20261020
    params = dict(width=W, height=H, mode=5, num_objects=16, batch_size=B, sampler=1, seed=seed, background_prep=1)
    pool = lambda gen: gen.pool_synthetic(args.pool, 1024, 768, 2024)  # noqa: E731
    extras = ("flow1", "occ0", "occ1")

    def emit(d):
        line = json.dumps(dict(d, variant=args.tag))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    g = ofdg.Generator(ofdg.default_params(**params))
    pool(g)
    s = torch.cuda.current_stream().cuda_stream
    sets = {}
    for image_u8 in (False, True):
        for flow_f16 in (False, True):
            kw = dict(image_dtype=torch.uint8 if image_u8 else None, flow_dtype=torch.float16 if flow_f16 else None)
            xkw = dict(flow_dtype=kw["flow_dtype"], occ_dtype=torch.uint8 if flow_f16 else None)
            outs, ex = ofdg.alloc_outputs(B, H, W, **kw), ofdg.alloc_extras(B, H, W, extras, **xkw)
            torch.cuda.synchronize()
            g.forward_counter(0, B, *outs, s, extras=ex)
            torch.cuda.synchronize()
            planes, rows = ofdg.alloc_reproject(B, H, W, (0, 1), ofdg.REPROJ_OUTPUTS, outs[0].dtype)
            blurred, recs_out = ofdg.alloc_motion_blur(B, H, W, outs[0].dtype)
            warped = ofdg.alloc_spatial(dict(image0=outs[0], image1=outs[1]), H, W)
            sets[(image_u8, flow_f16)] = (outs, ex, planes, rows, blurred, recs_out, warped)
    torch.cuda.synchronize()

    big = torch.ones((8192, 8192), dtype=torch.float32, device="cuda")
    big_out = torch.empty_like(big)

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
        # ... and the device time alone: ten calls queued behind a long matrix product, so that issuing them costs nothing
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.mm(big, big, out=big_out)
        a.record()
        for _ in range(10):
            fn()
        b.record()
        b.synchronize()
        return round(statistics.median(out), 1), round(a.elapsed_time(b) * 100.0, 1)

    size = lambda t: t.numel() * t.element_size()  # noqa: E731
    for rnd in range(args.rounds):
        for (image_u8, flow_f16), (outs, ex, planes, rows, blurred, recs_out, warped) in sets.items():
            fmt = dict(frames_fmt="u8" if image_u8 else "f32", flow_fmt="f16" if flow_f16 else "f32")
            flows, occ = (outs[2], ex["flow1"]), (ex["occ0"], ex["occ1"])
            recs = torch.tensor([[1.0, 1.0, 0.0, 0.0]] * B, dtype=torch.float32, device="cuda")
            for frames in ((0,), (0, 1)):
                sel = lambda pair: tuple(t if f in frames else None for f, t in enumerate(pair))  # noqa: E731
                src = {"image%d" % f: outs[f] for f in frames}
                dst = {k: warped[k] for k in src}
                med, yard = timed(lambda: g.spatial(src, dst, first_index=0, ranges=None, stream=s))
                emit(dict(fmt, kernel="spatial, identity record, frames only", round=rnd, frames=list(frames), us_median=med, us_device=yard,
                          moved_MB=round(sum(size(t) for t in src.values()) * 2 / 1e6, 1)))
                med, blur = timed(lambda: g.motion_blur(sel(outs[:2]), sel(blurred), flow=sel(flows), recs=recs, taps_side=1, recs_out=recs_out, stream=s))
                emit(dict(fmt, kernel="motion_blur, taps_side 1, shutter 1", round=rnd, frames=list(frames), us_median=med, us_device=blur,
                          moved_MB=round(sum(size(outs[f]) * 2 + size(flows[f]) for f in frames) / 1e6, 1)))
                for name, outputs in FORMS:
                    out = {ofdg.reproject_key(n_, f): planes[ofdg.reproject_key(n_, f)] for f in frames for n_ in outputs if n_ != "rows"}
                    r = rows if "rows" in outputs else None
                    med, dev = timed(lambda: g.reproject(outs[:2], flows, occ, out=out, rows=r, frames=frames, stream=s))
                    # (a frame reads both frames and both flows: its own whole, the other's gathered)
                    read = size(outs[0]) + size(outs[1]) + size(flows[0]) + size(flows[1]) + sum(size(occ[f]) for f in frames)
                    moved = read + sum(size(t) for t in out.values())
                    emit(dict(fmt, kernel="reproject", outputs=name, round=rnd, frames=list(frames), us_median=med, us_device=dev, moved_MB=round(moved / 1e6, 1),
                              GBps=round(moved / dev / 1e3, 1), x_spatial=round(dev / yard, 2), x_mblur=round(dev / blur, 2)))
            if not image_u8 and not flow_f16:
                med, dev = timed(lambda: grid_sample_restatement(outs[0], outs[1], outs[2], ex["flow1"]), reps=10)
                emit(dict(fmt, kernel="torch eager: grid_sample of image1 and flow1, residuals, frame 0", round=rnd, frames=[0], us_median=med, us_device=dev))
    del g
    if args.kernel_only:
        return
    for rep in range(args.reps):
        for name, more in (("plain", {}), ("reproject", dict(reproject=dict(frames=(0, 1), outputs=("rows",))))):
            it = iter(ofdg.FlowLoader(ofdg.default_params(**params), pool=pool, prefetch=3, extras=extras, **more))
            for _ in range(args.warmup):
                next(it)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                next(it)
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
            emit({"loader": name, "rep": rep, "samples_per_s": round(args.steps * B / el, 1), "us_per_step": round(el / args.steps * 1e6, 1),
                  "steps": args.steps, "batch": B, "W": W, "H": H, "pool": args.pool})
            del it


if __name__ == "__main__":
    main()
