"""What the photometric augmentation costs: forward_counter at the bench's config 2 (mode 5, 512x384, batch 32, 16 objects,
counter sampler, background_prep 1, synthetic 1000 x 1024x768 pool) with and without ofdg_photo (PHOTO_FLOWNET ranges, drawn
records) behind every batch on the same internal stream - one JSON line per form and repetition with samples/s:

    f32 / u8                    the yardsticks: float32 frames and flow; uint8 frames with fp16 flow
    f32_photo0 / u8_photo0      both frames in place, sigma_max 0 (a table lookup per element)
    f32_photo / u8_photo        both frames in place, sigma_max 10 (and a Philox block per four elements)
    f32_photo_copy / u8_photo_copy   sigma_max 10, into other buffers of the same format
    f32_photo_to_u8             float32 frames into uint8 buffers, sigma_max 10

The forms are interleaved (--reps rounds of all) so that drift of the box hits them alike.  "in_pipeline" lines: the mean time
per step a form adds to its yardstick.  Then, on the last batch rendered and an otherwise idle device, "kernel" lines: the
median time of ofdg_photo alone between two events for the four format pairs, sigma_max 0 and 10, in place and copying, with
the bytes it moves and the rate that makes - and of ofdg_crop moving the same frames whole (512x384 to 512x384, image0 and
image1 only): the same bytes read and written with nothing done to them.  With --out FILE the lines are appended to FILE too;
with --tag NAME every line carries "variant": NAME (default "as built") - for runs with OFDG_LIB set to another build.

    python tools/photo_cost.py [--steps K] [--warmup W] [--reps R] [--pool N] [--out FILE] [--tag NAME] [--kernel-only]
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

FORMS = ("f32", "f32_photo0", "f32_photo", "f32_photo_copy", "f32_photo_to_u8", "u8", "u8_photo0", "u8_photo", "u8_photo_copy")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--pool", type=int, default=1000, help="textures of the synthetic pool")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    ap.add_argument("--tag", default="as built", help="the \"variant\" every line carries")
    ap.add_argument("--kernel-only", action="store_true", help="skip the pipeline forms: the kernels alone")
    args = ap.parse_args()
    import torch
    ofdg = importlib.import_module("optical-flow-2d-data-generation_amd")
    W, H, B = 512, 384, 32
    seed = 20261019
    g = ofdg.Generator(ofdg.default_params(width=W, height=H, mode=5, num_objects=16, batch_size=B, sampler=1, seed=seed, background_prep=1))
    g.pool_synthetic(args.pool, 1024, 768, 2024)
    nbuf = 2 * g.num_chains()
    noisy = ofdg.PHOTO_FLOWNET
    quiet = dict(noisy, sigma_max=0.0)
    sets = {}
    for u8 in (False, True):
        kw = dict(image_dtype=torch.uint8, flow_dtype=torch.float16) if u8 else {}
        sets[u8] = []
        for _ in range(nbuf):
            outs = ofdg.alloc_outputs(B, H, W, **kw)
            same = tuple(torch.zeros_like(t) for t in outs[:2])
            other = tuple(torch.zeros(t.shape, dtype=torch.float32 if u8 else torch.uint8, device="cuda") for t in outs[:2])
            sets[u8].append((outs, same, other))
    torch.cuda.synchronize()

    def emit(d):
        line = json.dumps(dict(d, variant=args.tag))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    elements = 2 * B * 3 * H * W
    us = {f: [] for f in FORMS}
    for rep in range(0 if args.kernel_only else args.reps):
        for f in FORMS:
            u8 = f.startswith("u8")
            bufs = sets[u8]
            ranges = None if "_photo" not in f else quiet if "photo0" in f else noisy

            def step(i):
                outs, same, other = bufs[i % nbuf]
                g.forward_counter(i * B, B, *outs, ofdg.STREAM_OWN)
                if ranges is not None:
                    dst = same if f.endswith("_copy") else other if f.endswith("_to_u8") else None
                    g.photo(outs[:2], dst, first_index=i * B, ranges=ranges, stream=ofdg.STREAM_OWN)

            for i in range(args.warmup):
                step(i)
            g.synchronize()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.warmup, args.warmup + args.steps):
                step(i)
            g.synchronize()
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
            us[f].append(el / args.steps * 1e6)
            emit({"form": f, "rep": rep, "samples_per_s": round(args.steps * B / el, 1), "us_per_step": round(us[f][-1], 1),
                  "steps": args.steps, "batch": B, "W": W, "H": H})
    for f in FORMS:
        if "_photo" in f and us[f]:
            base = f.split("_photo")[0]
            emit({"in_pipeline": f, "added_us_per_step_mean": round(statistics.mean(us[f]) - statistics.mean(us[base]), 1),
                  "yardstick_us_per_step_min_max": [round(min(us[base]), 1), round(max(us[base]), 1)],
                  "with_photo_us_per_step_min_max": [round(min(us[f]), 1), round(max(us[f]), 1)]})

    # the kernels alone on an idle device
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
    for u8 in (False, True):
        outs, same, other = sets[u8][0]
        g.forward_counter(0, B, *outs, s)
        torch.cuda.synchronize()
        es = outs[0].element_size()
        for dst, what in ((None, "in place"), (same, "copy"), (other, "copy to the other format")):
            for ranges in (quiet, noisy):
                src = tuple(t.clone() for t in outs[:2]) if dst is None else outs[:2]  # (in place: on a copy, so the other rows see the rendered frames)
                med, best = timed(lambda: g.photo(src, dst, first_index=0, ranges=ranges, stream=s))
                moved = elements * (es + (es if dst is not other else other[0].element_size()))
                emit({"kernel": "photo", "src": "u8" if u8 else "f32", "dst": what, "sigma_max": ranges["sigma_max"], "us_median": round(med, 1),
                      "us_min": round(best, 1), "moved_MB": round(moved / 1e6, 1), "GB_per_s_at_median": round(moved / med / 1e3, 1),
                      "us_floor_at_6_TB_per_s": round(moved / 6e6, 1)})
        src = dict(image0=outs[0], image1=outs[1])
        dst = ofdg.alloc_crop(src, H, W)
        torch.cuda.synchronize()
        med, best = timed(lambda: g.crop(src, dst, first_index=0, stream=s))
        moved = elements * 2 * es
        emit({"kernel": "crop, the frames whole", "src": "u8" if u8 else "f32", "us_median": round(med, 1), "us_min": round(best, 1),
              "moved_MB": round(moved / 1e6, 1), "GB_per_s_at_median": round(moved / med / 1e3, 1), "us_floor_at_6_TB_per_s": round(moved / 6e6, 1)})


if __name__ == "__main__":
    main()
