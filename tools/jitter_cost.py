"""What the colour jitter costs: ofdg_jitter alone on one batch of the bench's config 2 (mode 5, 512x384, batch 32, 16 objects,
counter sampler, background_prep 1, synthetic pool), on an otherwise idle device - the median of 30 calls between two events
("us_median": it holds what issuing the call from Python costs, some 20 us) and the device time of one call among ten queued
behind a long matrix product ("us_device"), --rounds interleaved rounds of all rows, one JSON line per row and round.  Every
row uses given records, the same for all samples, so that every sample works:

    jitter      identity / hue only / saturation + brightness / all four without a contrast (one pass over the frames) / all four
                with one (two passes: the mean's reduction reads the frames once more), float32 / uint8 frames, in place / copying,
                one frame / both; "moved_MB" is what the form has to read and write
    photo       the yardstick: ofdg_photo noise-free on the same planes and formats, in place and copying - one pass
    torch       an eager restatement of the four operations in float32 (HSV round trip for the hue), for scale

Then "loader" lines: FlowLoader at config 2 with and without jitter=JITTER_RAFT, --reps interleaved repetitions of --steps
steps.  With --out FILE the lines are appended to FILE too; "lib" names the library when OFDG_LIB selects another build.

    python tools/jitter_cost.py [--rounds R] [--steps K] [--warmup W] [--reps R] [--pool N] [--out FILE] [--kernel-only]
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
    import numpy as np
    import torch
    ofdg = importlib.import_module("optical-flow-2d-data-generation_amd")
    W, H, B = 512, 384, 32
    seed = 20261020
    params = dict(width=W, height=H, mode=5, num_objects=16, batch_size=B, sampler=1, seed=seed, background_prep=1)
    pool = lambda gen: gen.pool_synthetic(args.pool, 1024, 768, 2024)  # noqa: E731
    lib_name = os.path.basename(ofdg.LIB_PATH)

    def emit(d):
        line = json.dumps(dict(d, lib=lib_name))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    g = ofdg.Generator(ofdg.default_params(**params))
    pool(g)
    s = torch.cuda.current_stream().cuda_stream
    sets = {}
    for u8 in (False, True):
        kw = dict(image_dtype=torch.uint8, flow_dtype=torch.float16) if u8 else {}
        outs = ofdg.alloc_outputs(B, H, W, **kw)
        torch.cuda.synchronize()
        g.forward_counter(0, B, *outs, s)
        torch.cuda.synchronize()
        sets[u8] = (outs[:2], tuple(torch.empty_like(t) for t in outs[:2]))
    work, rout = ofdg.alloc_jitter(B)

    def records(**fields):
        r = np.zeros((B,), ofdg._jitter_rec_dtype())
        for k in ("brightness", "contrast", "saturation"):
            r[k] = fields.get(k, ofdg.JITTER_ONE)
        r["hue"], r["shared"] = fields.get("hue", 0), 1
        return torch.from_numpy(r.view(np.int32).reshape(B, 16)).cuda()

    forms = [("identity", records(), 0), ("hue only", records(hue=40000), 1), ("saturation + brightness", records(saturation=50000, brightness=75000), 1),
             ("all four without a contrast", records(brightness=75000, saturation=50000, hue=40000), 1),
             ("all four", records(brightness=75000, contrast=90000, saturation=50000, hue=40000), 2)]
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

    def torch_eager(frame):
        """brightness, saturation, hue, contrast in float32 on a [n,3,H,W] B, G, R frame; returns a frame of its dtype"""
        x = frame.float()
        x = (x * 1.14).clamp(0, 255)
        lum = (0.114 * x[:, 0] + 0.587 * x[:, 1] + 0.299 * x[:, 2]).unsqueeze(1)
        x = (0.76 * x + 0.24 * lum).clamp(0, 255)
        b, gr, r = x[:, 0], x[:, 1], x[:, 2]
        mx, mn = x.max(dim=1).values, x.min(dim=1).values
        d = mx - mn
        dd = torch.where(d == 0, torch.ones_like(d), d)
        h = torch.where(mx == r, ((gr - b) / dd) % 6, torch.where(mx == gr, (b - r) / dd + 2, (r - gr) / dd + 4))
        h = (h + 6 * 40000 / 393216.0) % 6
        k = lambda n: (n + h) % 6  # noqa: E731
        ch = lambda n: mx - d * torch.minimum(torch.minimum(k(n), 4 - k(n)), torch.ones_like(h)).clamp(min=0)  # noqa: E731
        x = torch.stack([ch(1), ch(3), ch(5)], dim=1)
        mean = (0.114 * x[:, 0] + 0.587 * x[:, 1] + 0.299 * x[:, 2]).mean(dim=(1, 2)).round()[:, None, None, None]
        x = (1.37 * x - 0.37 * mean).clamp(0, 255)
        return x.round().to(frame.dtype)

    for rnd in range(args.rounds):
        for u8 in (False, True):
            src, dst = sets[u8]
            fmt = "u8" if u8 else "f32"
            frame_mb = src[0].numel() * src[0].element_size() / 1e6
            for name, recs, passes in forms:
                for frames in ((0, 1), (1,)):
                    for in_place in (True, False):
                        if name in ("hue only", "saturation + brightness") and (frames != (0, 1) or not in_place):
                            continue
                        pick = lambda pair: tuple(t if f in frames else None for f, t in enumerate(pair))  # noqa: E731
                        a, b = pick(src), None if in_place else pick(dst)
                        med, best = timed(lambda: g.jitter(a, b, recs=recs, recs_out=rout, work=work, stream=s))
                        moved = 0.0 if passes == 0 and in_place else (2 + (passes == 2)) * frame_mb * len(frames)  # read and written, and read once more for the mean
                        emit({"kernel": "jitter", "form": name, "round": rnd, "frames_fmt": fmt, "frames": list(frames), "in_place": in_place,
                              "passes": passes, "us_median": med, "us_device": best, "moved_MB": round(moved, 1)})
            quiet = dict(ofdg.PHOTO_FLOWNET, sigma_max=0.0)
            for in_place in (True, False):
                med, best = timed(lambda: g.photo(src, None if in_place else dst, first_index=0, ranges=quiet, stream=s))
                emit({"kernel": "photo, noise-free, both frames", "round": rnd, "frames_fmt": fmt, "in_place": in_place, "us_median": med, "us_device": best,
                      "moved_MB": round(4 * frame_mb, 1)})
            med, best = timed(lambda: (torch_eager(src[0]), torch_eager(src[1])), reps=5)
            emit({"kernel": "torch eager: the four operations in float32, both frames", "round": rnd, "frames_fmt": fmt, "us_median": med, "us_device": best})
            g.forward_counter(0, B, *(src + (torch.empty((B, 2, H, W), dtype=torch.float16 if u8 else torch.float32, device="cuda"),)), s)  # (fresh frames: the in-place rows wore them down)
            torch.cuda.synchronize()
    del g
    if args.kernel_only:
        return
    for rep in range(args.reps):
        for name, more in (("plain", {}), ("jitter", dict(jitter=ofdg.JITTER_RAFT))):
            it = iter(ofdg.FlowLoader(ofdg.default_params(**params), pool=pool, prefetch=3, **more))
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
