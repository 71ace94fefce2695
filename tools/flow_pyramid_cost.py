"""What the multi-scale flow pyramid costs: forward_counter at the bench's config 2 (mode 5, 512x384, batch 32, 16 objects,
counter sampler, background_prep 1, synthetic 1000 x 1024x768 pool) in six forms - one JSON line per form and repetition with
samples/s:

    f32        float32 outputs (ofdg_forward_counter): the yardstick
    f32_pyr    the same call followed by ofdg_flow_pyramid (6 levels, scaled, float32) on the same internal stream
    f32_pyr_w  ... with the weight planes
    f16        uint8 frames, fp16 flow (ofdg_forward_counter_fmt): the compact yardstick
    f16_pyr    the same call followed by ofdg_flow_pyramid (6 levels, scaled, fp16)
    f16_pyr_w  ... with the weight planes

The forms are interleaved (--reps rounds of all six) so that drift of the box hits them alike.  Then, on the last batch
rendered and an otherwise idle device, "kernel" lines: the median time of ofdg_flow_pyramid alone between two events
(float32 and fp16, with and without weights) with the bytes it moves - 8 or 4 B/px read, 4/3 of 2 or 1 B/px (+ 1/3 of 2 B/px of
weights) written - and the rate that makes; and "pool_chain" lines: the same six levels made by a chain of six
torch.nn.functional.avg_pool2d(x, 2) calls on the same tensor, for scale only - its bits differ by design (no validity rule,
the framework's order of summation, no level-k pixel units).  "in_pipeline" lines: the mean time per step a form with the
pyramid adds to its yardstick over the repetitions.  With --out FILE the lines are appended to FILE too.

    python tools/flow_pyramid_cost.py [--steps K] [--warmup W] [--reps R] [--pool N] [--out FILE]
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

FORMS = ("f32", "f32_pyr", "f32_pyr_w", "f16", "f16_pyr", "f16_pyr_w")
LEVELS = 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--pool", type=int, default=1000, help="textures of the synthetic pool")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    import torch
    ofdg = importlib.import_module("optical-flow-2d-data-generation_amd")
    W, H, B = 512, 384, 32
    g = ofdg.Generator(ofdg.default_params(width=W, height=H, mode=5, num_objects=16, batch_size=B, sampler=1, seed=20261003,
                                           background_prep=1))
    g.pool_synthetic(args.pool, 1024, 768, 2024)
    nbuf = 2 * g.num_chains()
    sets = {}
    for half in (False, True):
        kw = dict(image_dtype=torch.uint8, flow_dtype=torch.float16) if half else {}
        dt = torch.float16 if half else torch.float32
        sets[half] = [(ofdg.alloc_outputs(B, H, W, **kw), ofdg.alloc_flow_pyramid(B, H, W, LEVELS, dt),
                       ofdg.alloc_flow_pyramid(B, H, W, LEVELS, dt, weights=True)) for _ in range(nbuf)]
    torch.cuda.synchronize()
    px = B * W * H

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    def moved(half, weights):
        """bytes per pixel the pyramid call reads and writes"""
        tail = sum(0.25 ** k for k in range(1, LEVELS + 1))
        return (4 if half else 8), 2 * (2 if half else 4) * tail + (2 * tail if weights else 0)

    us = {f: [] for f in FORMS}
    for rep in range(args.reps):
        for f in FORMS:
            half, pyr, weights = f.startswith("f16"), "_pyr" in f, f.endswith("_w")
            bufs = sets[half]

            def step(i):
                outs, lv, lvw = bufs[i % nbuf]
                g.forward_counter(i * B, B, *outs, ofdg.STREAM_OWN)
                if pyr:
                    g.flow_pyramid(outs[2], LEVELS, out=lvw if weights else lv, stream=ofdg.STREAM_OWN)

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
            rd, wr = moved(half, weights)
            emit({"form": f, "rep": rep, "samples_per_s": round(args.steps * B / el, 1), "us_per_step": round(us[f][-1], 1),
                  "pyramid_bytes_per_px": round(rd + wr, 3) if pyr else 0, "steps": args.steps, "batch": B, "W": W, "H": H})
    for f in FORMS:
        if "_pyr" in f:
            base = f.split("_")[0]
            emit({"in_pipeline": f, "added_us_per_step_mean": round(statistics.mean(us[f]) - statistics.mean(us[base]), 1),
                  "yardstick_us_per_step_min_max": [round(min(us[base]), 1), round(max(us[base]), 1)]})

    # the kernel alone, and the framework's pooling chain, on an idle device
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
    for half in (False, True):
        outs, lv, lvw = sets[half][0]
        for weights in (False, True):
            med, best = timed(lambda: g.flow_pyramid(outs[2], LEVELS, out=lvw if weights else lv, stream=s))
            rd, wr = moved(half, weights)
            emit({"kernel": "flow_pyramid", "flow": "f16" if half else "f32", "weights": weights, "us_median": round(med, 1),
                  "us_min": round(best, 1), "read_bytes_per_px": rd, "written_bytes_per_px": round(wr, 3),
                  "GB_per_s_at_median": round((rd + wr) * px / med / 1e3, 1), "us_floor_at_6_TB_per_s": round((rd + wr) * px / 6e6, 1)})

        def chain():
            x = outs[2]
            for _ in range(LEVELS):
                x = torch.nn.functional.avg_pool2d(x, 2)
            return x

        med, best = timed(chain)
        emit({"pool_chain": "6 x avg_pool2d(2)", "flow": "f16" if half else "f32", "us_median": round(med, 1), "us_min": round(best, 1),
              "launches": LEVELS})


if __name__ == "__main__":
    main()
