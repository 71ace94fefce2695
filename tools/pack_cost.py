"""What the network-ready packing costs: batch 32 of 512x384 frames and flow of the bench's config 2 (mode 5, 16 objects, counter
sampler, background_prep 1, synthetic 1000 x 1024x768 pool) - one JSON line per measurement:

    "kernel" lines   ofdg_pack alone on an idle device, the median of 30 between two events, with the bytes it moves, the rate
                     that makes and the time those bytes take at 6 TB/s: uint8 -> bfloat16 channels-last concatenated (what the
                     entry exists for), uint8 -> bfloat16 channels-last (C = 3), uint8 -> float32 planar, float32 -> float32
                     planar, float32 -> bfloat16 channels-last, each with and without the flow (binary16 beside uint8 frames,
                     float32 beside float32 ones, into the frames' destination type)
    "yardstick"      ofdg_photo, uint8 -> float32 under the identity record (no noise): the same bytes read and written as the
                     uint8 -> float32 planar pack at identity constants, which is measured right beside it
    "eager"          the torch restatement of the uint8 -> bfloat16 channels-last concatenated result, frames and flow
    "loader" lines   FlowLoader of uint8 / binary16 batches with and without pack= (bfloat16, channels-last, concatenated),
                     --reps rounds interleaved; "in_pipeline": the mean time per batch the pack adds

The kernel forms are measured in --rounds interleaved rounds, so that drift of the device hits them alike; a line carries the
median and the minimum of every round.  With --out FILE the lines are appended to FILE too; with --tag NAME every line carries
"variant": NAME (default "as built") - for runs with OFDG_LIB set to another build.

    python tools/pack_cost.py [--steps K] [--warmup W] [--reps R] [--rounds N] [--pool N] [--out FILE] [--tag NAME] [--kernel-only]
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
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pool", type=int, default=1000, help="textures of the synthetic pool")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    ap.add_argument("--tag", default="as built", help="the \"variant\" every line carries")
    ap.add_argument("--kernel-only", action="store_true", help="skip the loader: the kernels alone")
    args = ap.parse_args()
    import torch
    ofdg = importlib.import_module("optical-flow-2d-data-generation_amd")
    W, H, B = 512, 384, 32
    seed = 20261019
    params = dict(width=W, height=H, mode=5, num_objects=16, batch_size=B, sampler=1, seed=seed, background_prep=1)
    pool = lambda gen: gen.pool_synthetic(args.pool, 1024, 768, 2024)  # noqa: E731
    g = ofdg.Generator(ofdg.default_params(**params))
    pool(g)

    def emit(d):
        line = json.dumps(dict(d, variant=args.tag))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

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
    rendered = {}
    for u8 in (False, True):
        outs = ofdg.alloc_outputs(B, H, W, **(dict(image_dtype=torch.uint8, flow_dtype=torch.float16) if u8 else {}))
        g.forward_counter(0, B, *outs, s)
        rendered[u8] = dict(zip(ofdg.PACK_PLANES, outs))
    torch.cuda.synchronize()
    scale, bias = ofdg.pack_norm((0.406, 0.456, 0.485), (0.225, 0.224, 0.229))
    norm = dict(scale=scale, bias=bias, flow_scale=0.05, rgb=True)
    ident = dict()
    # name: (uint8 sources, destination dtype, layout, concat, constants)
    forms = {
        "u8_bf16_nhwc_concat": (True, torch.bfloat16, ofdg.PACK_NHWC, True, norm),
        "u8_bf16_nhwc": (True, torch.bfloat16, ofdg.PACK_NHWC, False, norm),
        "u8_f32_nchw": (True, torch.float32, ofdg.PACK_NCHW, False, ident),
        "f32_f32_nchw": (False, torch.float32, ofdg.PACK_NCHW, False, norm),
        "f32_bf16_nhwc": (False, torch.bfloat16, ofdg.PACK_NHWC, False, norm),
    }
    calls = {}
    for name, (u8, dtype, layout, concat, consts) in forms.items():
        for with_flow in (False, True):
            planes = ofdg.PACK_PLANES if with_flow else ofdg.PACK_PLANES[:2]
            src = {k: rendered[u8][k] for k in planes}
            dst = ofdg.alloc_pack(B, H, W, image_dtype=dtype, flow_dtype=dtype, layout=layout, concat=concat, planes=planes)
            moved = sum(t.numel() * t.element_size() for t in src.values()) + sum(t.numel() * t.element_size() for t in dst.values())
            fn = (lambda src=src, dst=dst, layout=layout, concat=concat, consts=consts: g.pack(src, dst, layout=layout, concat=concat, stream=s, **consts))
            calls[(name, with_flow)] = (fn, moved)
    # the yardstick: ofdg_photo, uint8 -> float32 under the identity record - the bytes of u8_f32_nchw without the flow
    ident_recs = torch.zeros((B, ofdg.PHOTO_REC_FLOATS), dtype=torch.float32, device="cuda")
    ident_recs[:, :4] = 1.0      # gamma, contrast
    ident_recs[:, 6:12] = 1.0    # gain
    frames = (rendered[True]["image0"], rendered[True]["image1"])
    photo_dst = tuple(torch.zeros((B, 3, H, W), dtype=torch.float32, device="cuda") for _ in range(2))
    moved = sum(t.numel() for t in frames) * 5
    calls[("photo_u8_f32_identity", False)] = (lambda: g.photo(frames, photo_dst, recs=ident_recs, stream=s), moved)
    # the eager torch restatement of u8_bf16_nhwc_concat with the flow
    sc, bi = torch.from_numpy(scale).cuda().view(1, 3, 1, 1), torch.from_numpy(bias).cuda().view(1, 3, 1, 1)

    def eager():
        x = torch.cat([((t.float() * sc) + bi).flip(1) for t in frames], 1).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        f = (rendered[True]["flow"].float() * 0.05).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        return x, f
    calls[("eager_torch_u8_bf16_nhwc_concat", True)] = (eager, calls[("u8_bf16_nhwc_concat", True)][1])
    torch.cuda.synchronize()
    # the pack's identity result is the photo pass's: the same values
    g.pack({k: rendered[True][k] for k in ofdg.PACK_PLANES[:2]}, dict(zip(ofdg.PACK_PLANES[:2], photo_dst)), stream=s)
    torch.cuda.synchronize()
    check = tuple(t.clone() for t in photo_dst)
    g.photo(frames, photo_dst, recs=ident_recs, stream=s)
    torch.cuda.synchronize()
    emit({"check": "pack at identity constants equals photo under the identity record", "equal": all(torch.equal(a, b) for a, b in zip(check, photo_dst))})
    x, f = eager()
    dst = ofdg.alloc_pack(B, H, W, image_dtype=torch.bfloat16, flow_dtype=torch.bfloat16, layout=ofdg.PACK_NHWC, concat=True)
    g.pack(rendered[True], dst, layout=ofdg.PACK_NHWC, concat=True, stream=s, **norm)
    torch.cuda.synchronize()
    emit({"check": "pack equals the eager torch restatement", "equal": torch.equal(dst["image0"], x) and torch.equal(dst["flow"], f)})

    results = {key: [] for key in calls}
    for _ in range(args.rounds):
        for key, (fn, _) in calls.items():
            results[key].append(timed(fn))
    for (name, with_flow), (fn, moved) in calls.items():
        meds, mins = [r[0] for r in results[(name, with_flow)]], [r[1] for r in results[(name, with_flow)]]
        kind = "yardstick" if name.startswith("photo") else "eager" if name.startswith("eager") else "kernel"
        med = statistics.median(meds)
        emit({kind: name, "flow": with_flow, "us_median": round(med, 1), "us_median_of_rounds": [round(v, 1) for v in meds],
              "us_min_of_rounds": [round(v, 1) for v in mins], "moved_MB": round(moved / 1e6, 1), "GB_per_s_at_median": round(moved / med / 1e3, 1),
              "us_floor_at_6_TB_per_s": round(moved / 6e6, 1)})

    if args.kernel_only:
        return
    # the loader at config 2, compact batches, with and without pack=
    opts = dict(image_dtype=torch.bfloat16, flow_dtype=torch.bfloat16, layout=ofdg.PACK_NHWC, concat=True, **norm)
    us = {"u8": [], "u8_pack": []}
    for rep in range(args.reps):
        for form in us:
            loader = ofdg.FlowLoader(ofdg.default_params(**params), pool=pool, prefetch=2 * g.num_chains(), image_dtype=torch.uint8,
                                     flow_dtype=torch.float16, pack=opts if form == "u8_pack" else None)
            it = iter(loader)
            for _ in range(args.warmup):
                next(it)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                next(it)
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
            us[form].append(el / args.steps * 1e6)
            emit({"loader": form, "rep": rep, "samples_per_s": round(args.steps * B / el, 1), "us_per_step": round(us[form][-1], 1),
                  "steps": args.steps, "batch": B, "W": W, "H": H})
            del it, loader
            torch.cuda.synchronize()
    emit({"in_pipeline": "u8_pack", "added_us_per_step_mean": round(statistics.mean(us["u8_pack"]) - statistics.mean(us["u8"]), 1),
          "yardstick_us_per_step_min_max": [round(min(us["u8"]), 1), round(max(us["u8"]), 1)],
          "with_pack_us_per_step_min_max": [round(min(us["u8_pack"]), 1), round(max(us["u8_pack"]), 1)]})


if __name__ == "__main__":
    main()
