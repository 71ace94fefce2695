"""What the per-sample flow statistics cost: forward_counter at the bench's config 2 (mode 5, 512x384, batch 32, 16 objects,
counter sampler, background_prep 1, synthetic 1000 x 1024x768 pool) in four forms - one JSON line per form and repetition with
samples/s:

    f32        float32 outputs (ofdg_forward_counter): the yardstick
    f32_stats  the same call followed by ofdg_flow_stats on the same internal stream (reads 8 B/px)
    f16        uint8 frames, fp16 flow (ofdg_forward_counter_fmt): the compact yardstick
    f16_stats  the same call followed by ofdg_flow_stats (reads 4 B/px)

With --occ the calls also render occ0 (float32 / uint8 with the compact formats) and the statistics take the map (+4 / +1
B/px), in all four forms.  The forms are interleaved (--reps rounds of all four) so that drift of the box hits them alike; the
expectation to confirm or refute is that each *_stats form stays within the min .. max spread of its yardstick over the
repetitions (the pass reads 8 or 4 B/px beside compose's >= 34 or 14, and its launch rides on the chains).  With --out FILE
the lines are appended to FILE too (profiles/flow_stats_cost.jsonl).  Per-kernel times: run it under
    rocprofv3 --kernel-trace --stats -d DIR -o flowstats -- python tools/flow_stats_cost.py --reps 1
(flow_stats_kernel beside compose_rigid_*).

    python tools/flow_stats_cost.py [--steps K] [--warmup W] [--reps R] [--pool N] [--occ] [--out FILE]
"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORMS = ("f32", "f32_stats", "f16", "f16_stats")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--pool", type=int, default=1000, help="textures of the synthetic pool")
    ap.add_argument("--occ", action="store_true", help="render occ0 too and pass it to the statistics")
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
        xkw = dict(flow_dtype=torch.float16, occ_dtype=torch.uint8) if half else {}
        sets[half] = [(ofdg.alloc_outputs(B, H, W, **kw), ofdg.alloc_extras(B, H, W, ("occ0",), **xkw) if args.occ else None,
                       ofdg.alloc_flow_stats(B)) for _ in range(nbuf)]
    torch.cuda.synchronize()
    px = B * W * H
    for rep in range(args.reps):
        for f in FORMS:
            half, stats = f.startswith("f16"), f.endswith("_stats")
            bufs = sets[half]

            def step(i):
                outs, ex, rows = bufs[i % nbuf]
                g.forward_counter(i * B, B, *outs, ofdg.STREAM_OWN, extras=ex)
                if stats:
                    g.flow_stats(outs[2], rows, occ=ex["occ0"] if ex else None, stream=ofdg.STREAM_OWN)

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
            read = (4 if half else 8) + ((1 if half else 4) if args.occ else 0)
            line = json.dumps({"form": f, "rep": rep, "occ": bool(args.occ), "samples_per_s": round(args.steps * B / el, 1),
                               "us_per_step": round(el / args.steps * 1e6, 1), "stats_bytes_per_px": read if stats else 0,
                               "stats_bytes_per_step": read * px if stats else 0, "steps": args.steps, "batch": B, "W": W, "H": H})
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as fh:
                    fh.write(line + "\n")


if __name__ == "__main__":
    main()
