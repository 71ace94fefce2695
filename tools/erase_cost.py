"""What the occluder rectangles cost: ofdg_erase alone on one batch of the bench's config 2 (mode 5, 512x384, batch 32, 16
objects, counter sampler, background_prep 1, synthetic pool) rendered with all extras, on an otherwise idle device - the median
of 30 calls between two events ("us_median": it holds what issuing the call from Python costs, some 20 us) and the device time
of one call among ten queued behind a long matrix product ("us_device"), --rounds interleaved rounds of all rows, one JSON line
per row and round:

    erase       fill mean / const / noise x float32 / uint8 frames x with / without occlusion marking x frame 1 / both frames,
                ERASE_RAFT with prob 1 (every sample works: one or two rectangles of 50..99 pixels)
    photo       the yardstick of the fill: ofdg_photo noise-free, in place, on frame 1 only - it reads and writes that frame once
    flow_stats  the yardstick of the occlusion pass: ofdg_flow_stats with occ0 - it reads the same flow and map once
    torch       an eager restatement for scale: per-sample mean and slice assignment of the same rectangles into frame 1

Then "loader" lines: FlowLoader at config 2 with and without erase=ERASE_RAFT, --reps interleaved repetitions of --steps steps.
With --out FILE the lines are appended to FILE too.

    python tools/erase_cost.py [--rounds R] [--steps K] [--warmup W] [--reps R] [--pool N] [--out FILE] [--kernel-only]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pool", type=int, default=1000, help="textures of the synthetic pool")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    ap.add_argument("--kernel-only", action="store_true", help="skip the loader lines")
    args = ap.parse_args()
    import torch
    ofdg = importlib.import_module("optical-flow-2d-data-generation_amd")
    W, H, B = 512, 384, 32
    seed = 20261020
    params = dict(width=W, height=H, mode=5, num_objects=16, batch_size=B, sampler=1, seed=seed, background_prep=1)
    pool = lambda gen: gen.pool_synthetic(args.pool, 1024, 768, 2024)  # noqa: E731

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    g = ofdg.Generator(ofdg.default_params(**params))
    pool(g)
    s = torch.cuda.current_stream().cuda_stream
    ranges = dict(ofdg.ERASE_RAFT, prob=1.0)
    sets = {}
    for u8 in (False, True):
        kw = dict(image_dtype=torch.uint8, flow_dtype=torch.float16) if u8 else {}
        xkw = dict(flow_dtype=torch.float16, occ_dtype=torch.uint8) if u8 else {}
        outs, ex = ofdg.alloc_outputs(B, H, W, **kw), ofdg.alloc_extras(B, H, W, **xkw)
        torch.cuda.synchronize()
        g.forward_counter(0, B, *outs, s, extras=ex)
        torch.cuda.synchronize()
        sets[u8] = (outs, ex)
    work, recs = ofdg.alloc_erase(B)
    rows = ofdg.alloc_flow_stats(B)
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

    def torch_eager(frame, used):
        for i in range(B):
            mean = frame[i].float().mean(dim=(1, 2)).round().to(frame.dtype)
            for x0, y0, w, h, _ in used[i]["rect"][:int(used[i]["count"])].tolist():
                frame[i, :, y0:y0 + h, x0:x0 + w] = mean[:, None, None]

    for rnd in range(args.rounds):
        for u8 in (False, True):
            outs, ex = sets[u8]
            fmt = "u8" if u8 else "f32"
            for fill, name in ((ofdg.ERASE_MEAN, "mean"), (ofdg.ERASE_CONST, "const"), (ofdg.ERASE_NOISE, "noise")):
                for frames in ((1,), (0, 1)):
                    for mark in (False, True):
                        occ = (ex["occ0"], ex["occ1"]) if mark else None
                        med, best = timed(lambda: g.erase(outs[:2], occ, (outs[2], ex["flow1"]), first_index=0, ranges=ranges, fill=fill, color=(10, 20, 30),
                                                          frames=frames, mark_occ=mark, recs_out=recs, work=work, stream=s))
                        emit({"kernel": "erase", "round": rnd, "frames_fmt": fmt, "fill": name, "frames": list(frames), "mark_occ": mark,
                              "us_median": med, "us_device": best})
            one = outs[1].clone()
            med, best = timed(lambda: g.photo((None, one), first_index=0, ranges=dict(ofdg.PHOTO_FLOWNET, sigma_max=0.0), stream=s))
            emit({"kernel": "photo, noise-free, in place, frame 1 only", "round": rnd, "frames_fmt": fmt, "us_median": med, "us_device": best,
                  "moved_MB": round(2 * one.numel() * one.element_size() / 1e6, 1)})
            med, best = timed(lambda: g.flow_stats(outs[2], rows, occ=ex["occ0"], stream=s))
            emit({"kernel": "flow_stats with occ0", "round": rnd, "flow_fmt": "f16" if u8 else "f32", "us_median": med, "us_device": best,
                  "read_MB": round((outs[2].numel() * outs[2].element_size() + ex["occ0"].numel() * ex["occ0"].element_size()) / 1e6, 1)})
            used = ofdg.erase_numpy(recs)  # (the records of the last erase call above: both frames; frame-0 ones painted into frame 1 all the same)
            med, best = timed(lambda: torch_eager(one, used), reps=5)
            emit({"kernel": "torch eager: per-sample mean and slice assignment, frame 1", "round": rnd, "frames_fmt": fmt, "us_median": med, "us_device": best})
    del g
    if args.kernel_only:
        return
    for rep in range(args.reps):
        for name, more in (("plain", {}), ("erase", dict(erase=ofdg.ERASE_RAFT))):
            it = iter(ofdg.FlowLoader(ofdg.default_params(**params), pool=pool, prefetch=3, extras=("flow1", "occ0", "occ1"), **more))
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
