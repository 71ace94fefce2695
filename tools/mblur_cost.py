"""What motion blur costs: ofdg_motion_blur alone on one batch of the bench's config 2 (mode 5, 512x384, batch 32, 16 objects,
counter sampler, background_prep 1, synthetic pool) rendered with all extras, float32 and in the compact formats, on an
otherwise idle device - the median of 30 calls between two events ("us_median": it holds what issuing the call from Python
costs, some 20 us) and the device time of one call among ten queued behind a long matrix product ("us_device"), --rounds
interleaved rounds of all rows, one JSON line per row and round:

    motion_blur  given records - every sample at shutter 0 / 0.25 / 0.5 / 1 in both frames - x taps_side 4 / 8 / 16 (8 only at
                 shutter 0) x float32 / uint8 frames x float32 / binary16 flow x frame 0 / both frames; "mean_taps" is the mean
                 N = 2 m + 1 per pixel of the form, computed from the flow outside the kernel (torch, by the definition's
                 roundings): cost follows it.  "x_spatial": us_device over the yardstick's of the same round and formats,
                 per frame.
    spatial      the yardstick: ofdg_spatial, frames only, under the identity record at the same size and formats - one
                 bilinear tap per pixel, the same bytes read and written.
    grid_sample  an eager torch restatement for scale, float32 only: 2 * 8 + 1 calls of grid_sample per frame at shutter 0.5,
                 averaged - not for bits (float32 blends, taps not capped per pixel).

Then "loader" lines: FlowLoader at config 2 with extras flow1, with and without motion_blur=MBLUR_DEFAULT, --reps interleaved
repetitions of --steps steps.  With --out FILE the lines are appended to FILE too; with --tag NAME every line carries
"variant": NAME (default "as built") - for runs with OFDG_LIB set to another build (the all-global-gather variant:
tools/build_variant.sh mblur_gather -DOFDG_MBLUR_WINDOW=0).

    python tools/mblur_cost.py [--rounds R] [--steps K] [--warmup W] [--reps R] [--pool N] [--out FILE] [--tag NAME] [--kernel-only]
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


def mean_taps(flow, shutter, taps_side):
    """the mean of N = 2 m + 1 over the pixels of a flow tensor [n,2,H,W] (include/ofdg.h, step 3a and 3b)"""
    import torch
    uv = flow.float()
    finite = torch.isfinite(uv).all(dim=1, keepdim=True)
    d = torch.round(torch.clamp(uv * shutter * 128.0, -8192.0, 8192.0)).to(torch.int32)
    d = torch.where(finite, d, torch.zeros_like(d))
    m = torch.clamp((d.abs().amax(dim=1) + 255) >> 8, max=taps_side)
    return float((2 * m + 1).float().mean().item())


def grid_sample_restatement(frame, flow, shutter, taps_side):
    """2 * taps_side + 1 bilinear samples of the frame along +- shutter / 2 of the flow, averaged: torch's own resampling"""
    import torch
    import torch.nn.functional as F
    n, _, H, W = frame.shape
    ys, xs = torch.meshgrid(torch.arange(H, device=frame.device, dtype=torch.float32), torch.arange(W, device=frame.device, dtype=torch.float32), indexing="ij")
    acc = torch.zeros_like(frame)
    half = flow.float() * (shutter * 0.5)
    for k in range(-taps_side, taps_side + 1):
        t = k / float(taps_side)
        gx = (xs + t * half[:, 0]) / ((W - 1) / 2.0) - 1.0
        gy = (ys + t * half[:, 1]) / ((H - 1) / 2.0) - 1.0
        acc += F.grid_sample(frame, torch.stack([gx, gy], -1), mode="bilinear", padding_mode="border", align_corners=True)
    return acc / (2 * taps_side + 1)


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
            outs, ex = ofdg.alloc_outputs(B, H, W, **kw), ofdg.alloc_extras(B, H, W, ("flow1",), flow_dtype=kw["flow_dtype"])
            torch.cuda.synchronize()
            g.forward_counter(0, B, *outs, s, extras=ex)
            torch.cuda.synchronize()
            blurred, recs_out = ofdg.alloc_motion_blur(B, H, W, outs[0].dtype)
            warped = ofdg.alloc_spatial(dict(image0=outs[0], image1=outs[1]), H, W)
            sets[(image_u8, flow_f16)] = (outs, ex["flow1"], blurred, recs_out, warped)
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

    taps_of = {}
    for rnd in range(args.rounds):
        for (image_u8, flow_f16), (outs, flow1, blurred, recs_out, warped) in sets.items():
            fmt = dict(frames_fmt="u8" if image_u8 else "f32", flow_fmt="f16" if flow_f16 else "f32")
            yard = {}
            for frames in ((0,), (0, 1)):
                sel = lambda pair: tuple(t if f in frames else None for f, t in enumerate(pair))  # noqa: E731
                src = {"image%d" % f: outs[f] for f in frames}
                dst = {k: warped[k] for k in src}
                med, dev = timed(lambda: g.spatial(src, dst, first_index=0, ranges=None, stream=s))
                yard[frames] = dev
                moved = sum(t.numel() * t.element_size() for t in src.values()) * 2
                emit(dict(fmt, kernel="spatial, identity record, frames only", round=rnd, frames=list(frames), us_median=med, us_device=dev,
                          moved_MB=round(moved / 1e6, 1)))
                for shutter in (0.0, 0.25, 0.5, 1.0):
                    recs = torch.tensor([[shutter, shutter, 0.0, 0.0]] * B, dtype=torch.float32, device="cuda")
                    for taps_side in ((8,) if shutter == 0.0 else (4, 8, 16)):
                        key = (flow_f16, frames, shutter, taps_side)
                        if key not in taps_of:
                            taps_of[key] = round(statistics.mean(mean_taps((outs[2], flow1)[f], shutter, taps_side) for f in frames), 2)
                        med, dev = timed(lambda: g.motion_blur(sel(outs[:2]), sel(blurred), flow=sel((outs[2], flow1)), recs=recs, taps_side=taps_side,
                                                               recs_out=recs_out, stream=s))
                        emit(dict(fmt, kernel="motion_blur", round=rnd, frames=list(frames), shutter=shutter, taps_side=taps_side, mean_taps=taps_of[key],
                                  us_median=med, us_device=dev, x_spatial=round(dev / yard[frames], 2)))
            if not image_u8 and not flow_f16:
                med, dev = timed(lambda: grid_sample_restatement(outs[0], outs[2], 0.5, 8), reps=5)
                emit(dict(fmt, kernel="torch eager: 17 grid_sample calls, frame 0, shutter 0.5", round=rnd, us_median=med, us_device=dev))
    del g
    if args.kernel_only:
        return
    for rep in range(args.reps):
        for name, more in (("plain", {}), ("motion_blur", dict(motion_blur=ofdg.MBLUR_DEFAULT))):
            it = iter(ofdg.FlowLoader(ofdg.default_params(**params), pool=pool, prefetch=3, extras=("flow1",), **more))
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
