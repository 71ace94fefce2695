"""What the compact output formats buy: forward_counter at the bench's config 2 (mode 5, 512x384, batch 32, 16 objects,
counter sampler, background_prep 1, synthetic 1000 x 1024x768 pool) in three forms - float32 frames and flow, uint8 frames
with the float32 flow, uint8 frames with an fp16 flow - one JSON line per form and repetition with samples/s and the output
bytes of a step.  The forms are interleaved (--reps rounds of all forms) so that drift of the box hits them alike.
Per-kernel times: run it under
    rocprofv3 --kernel-trace --stats -d DIR -o formats -- python tools/output_format_cost.py --reps 1
(the plain and the compact compose kernels have names of their own).

    python tools/output_format_cost.py [--mode 5|9] [--steps K] [--warmup W] [--reps R] [--forms f32/f32,u8/f32,u8/f16] [--pool N]
"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", type=int, default=5, help="9: the non-rigid kernels")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--forms", default="f32/f32,u8/f32,u8/f16")
    ap.add_argument("--pool", type=int, default=1000, help="textures of the synthetic pool")
    args = ap.parse_args()
    import torch
    ofdg = importlib.import_module("optical-flow-2d-data-generation_amd")
    W, H, B = 512, 384, 32
    g = ofdg.Generator(ofdg.default_params(width=W, height=H, mode=args.mode, num_objects=16, batch_size=B, sampler=1, seed=20261003,
                                           background_prep=1))
    g.pool_synthetic(args.pool, 1024, 768, 2024)
    if args.mode == 9:
        g.warp_generate(2, 20261003)
    nbuf = 2 * g.num_chains()
    dt = {"f32": torch.float32, "u8": torch.uint8, "f16": torch.float16}
    forms = [tuple(f.split("/")) for f in args.forms.split(",")]
    bufs = {f: [ofdg.alloc_outputs(B, H, W, image_dtype=dt[f[0]], flow_dtype=dt[f[1]]) for _ in range(nbuf)] for f in forms}
    for rep in range(args.reps):
        for form in forms:
            ptrs = [ofdg.device_pointers(o) for o in bufs[form]]

            def step(i):
                g.forward_counter(i * B, B, *ptrs[i % nbuf], ofdg.STREAM_OWN, fmt=form)

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
            print(json.dumps({"form": "/".join(form), "rep": rep, "mode": args.mode, "samples_per_s": round(args.steps * B / el, 1),
                              "us_per_step": round(el / args.steps * 1e6, 1),
                              "output_bytes_per_step": sum(t.numel() * t.element_size() for t in bufs[form][0]),
                              "steps": args.steps, "batch": B, "W": W, "H": H}), flush=True)


if __name__ == "__main__":
    main()
