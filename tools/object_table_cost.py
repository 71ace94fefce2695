"""What the per-object annotation table costs: forward_counter at the bench's config 2 (mode 5, 512x384, batch 32, 16 objects,
counter sampler, background_prep 1, synthetic 1000 x 1024x768 pool) in two forms - one JSON line per form and repetition with
samples/s:

    labels        both label planes (ofdg_forward_counter_ex): the yardstick
    labels_table  the same call followed by ofdg_object_table on the same internal stream

The forms are interleaved (--reps rounds of both) so that drift of the box hits them alike; the expectation to confirm or
refute is that labels_table stays within the min .. max spread of labels over the repetitions (the table pass reads 2 B/px
beside compose's >= 34 B/px, and its two launches ride on the chains).  With --out FILE the lines are appended to FILE too
(profiles/object_table_cost.jsonl).  Per-kernel times: run it under
    rocprofv3 --kernel-trace --stats -d DIR -o objtab -- python tools/object_table_cost.py --reps 1
(object_table_header_kernel / object_table_reduce_kernel beside compose_rigid_ext_pow2_kernel).

    python tools/object_table_cost.py [--steps K] [--warmup W] [--reps R] [--pool N] [--out FILE]
"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORMS = ("labels", "labels_table")


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
    bufs = [ofdg.alloc_outputs(B, H, W) for _ in range(nbuf)]
    exs = [ofdg.alloc_extras(B, H, W, ("label0", "label1")) for _ in range(nbuf)]
    tabs = [ofdg.alloc_object_table(B) for _ in range(nbuf)]
    ptrs = [ofdg.device_pointers(o) for o in bufs]
    torch.cuda.synchronize()
    for rep in range(args.reps):
        for f in FORMS:
            def step(i):
                j = i % nbuf
                g.forward_counter(i * B, B, *ptrs[j], ofdg.STREAM_OWN, extras=exs[j])
                if f == "labels_table":
                    g.object_table(exs[j]["label0"], exs[j]["label1"], *tabs[j], stream=ofdg.STREAM_OWN)

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
            line = json.dumps({"form": f, "rep": rep, "samples_per_s": round(args.steps * B / el, 1),
                               "us_per_step": round(el / args.steps * 1e6, 1), "steps": args.steps, "batch": B, "W": W, "H": H})
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as fh:
                    fh.write(line + "\n")


if __name__ == "__main__":
    main()
