"""What the optional outputs cost: forward_counter at the bench's config 2 (mode 5, 512x384, batch 32, 16 objects,
counter sampler, background_prep 1, synthetic 1000 x 1024x768 pool) in three forms - no extras, flow1 + both labels,
all five - one JSON line per form with samples/s.  Per-kernel times: run it under
    rocprofv3 --kernel-trace --stats -d DIR -o extras -- python tools/extras_cost.py --forms all
(one form per run keeps the kernels of the forms apart in the statistics).

    python tools/extras_cost.py [--steps K] [--warmup W] [--forms none,flow1_labels,all]
"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORMS = {"none": None, "flow1_labels": ("flow1", "label0", "label1"), "all": ("flow1", "occ0", "occ1", "label0", "label1")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--forms", default="none,flow1_labels,all")
    args = ap.parse_args()
    import torch
    ofdg = importlib.import_module("optical-flow-2d-data-generation_amd")
    W, H, B = 512, 384, 32
    g = ofdg.Generator(ofdg.default_params(width=W, height=H, mode=5, num_objects=16, batch_size=B, sampler=1, seed=20261003,
                                           background_prep=1))
    g.pool_synthetic(1000, 1024, 768, 2024)
    nbuf = 2 * g.num_chains()
    outs = [ofdg.alloc_outputs(B, H, W) for _ in range(nbuf)]
    for form in args.forms.split(","):
        names = FORMS[form]
        ex = [ofdg.alloc_extras(B, H, W, names) if names else None for _ in range(nbuf)]
        ptrs = [ofdg.device_pointers(o) for o in outs]

        def step(i):
            g.forward_counter(i * B, B, *ptrs[i % nbuf], ofdg.STREAM_OWN, extras=ex[i % nbuf])

        for i in range(args.warmup):
            step(i)
        g.synchronize()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.warmup, args.warmup + args.steps):
            step(i)
        g.synchronize()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(json.dumps({"form": form, "extras": list(names or ()), "samples_per_s": round(args.steps * B / dt, 1),
                          "steps": args.steps, "batch": B, "W": W, "H": H}), flush=True)
        del ex


if __name__ == "__main__":
    main()
