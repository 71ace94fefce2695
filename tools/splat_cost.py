"""What the splat costs: ofdg_splat alone on one batch of the bench's config 2 (mode 5, 512x384, batch 32, 16 objects, counter
sampler, background_prep 1, synthetic pool) rendered with flow1, occ0, occ1, label0 and label1, float32 and in the compact
formats, on an otherwise idle device - the median of 30 calls between two events ("us_median": it holds what issuing the call
from Python costs, some 20 us) and the device time of one call among ten queued behind a long matrix product ("us_device"),
--rounds interleaved rounds of all rows, one JSON line per row and round:

    splat        t = 0 / 128 / 256 (in 1/256) x outputs keys only / image + mask / everything (image, to_own, to_other, mask,
                 fate, rows) x float32 / uint8 frames x float32 / binary16 flow x frame 0 / both frames x with / without
                 labels.  "moved_MB": the key planes cleared, raised once per source and read once, the planes read once and
                 the planes written (the gathered reads counted once).  "x_reproject": us_device over the comparison's of the
                 same round, formats and frames.
    reproject    a comparison: ofdg_reproject writing comparable bytes - warped + mask for "image + mask", everything for
                 "everything".
    torch        an eager torch restatement for scale, float32 only, frame 0, t = 256, with labels: scatter_reduce_(amax) of
                 int64 keys, then the gathers of the image and of the two flows - not for bits.

Then "loader" lines: FlowLoader at config 2 with extras flow1, occ0, occ1, label0, label1, with and without splat= (every output,
both frames, t drawn from 0..1), --reps interleaved repetitions of --steps steps.  With --out FILE the lines are appended to FILE
too; with --tag NAME every line carries "variant": NAME (default "as built") - for runs with OFDG_LIB set to another build
(tools/build_variant.sh).

    python tools/splat_cost.py [--rounds R] [--steps K] [--warmup W] [--reps R] [--pool N] [--out FILE] [--tag NAME] [--kernel-only]
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

FORMS = (("keys", ()), ("image+mask", ("image", "mask")), ("everything", ("image", "to_own", "to_other", "mask", "fate", "rows")))
REPROJECT = {"image+mask": ("warped", "mask"), "everything": ("warped", "err", "mask", "fb2", "rows")}


def torch_restatement(image0, flow, label0, t_q8):
    """frame 0 the framework way: the winner per target by scatter_reduce_(amax) on int64 keys, then the gathers"""
    import torch
    n, _, H, W = image0.shape
    fl = flow.float()
    D = torch.round(fl * 256.0).to(torch.int64)
    S = (D * t_q8 + 128) >> 8
    ys, xs = torch.meshgrid(torch.arange(H, device=flow.device), torch.arange(W, device=flow.device), indexing="ij")
    rx, ry = (256 * xs + S[:, 0] + 128) >> 8, (256 * ys + S[:, 1] + 128) >> 8
    inside = (rx >= 0) & (rx < W) & (ry >= 0) & (ry < H)
    idx = (ys * W + xs).expand(n, H, W)
    key = torch.where(inside, (label0.to(torch.int64) << 24) | ((1 << 24) - 1 - idx), torch.zeros((), dtype=torch.int64, device=flow.device))
    tgt = torch.where(inside, ry * W + rx, idx)
    keys = torch.zeros((n, H * W), dtype=torch.int64, device=flow.device)
    keys.scatter_reduce_(1, tgt.reshape(n, -1), key.reshape(n, -1), "amax", include_self=True)
    filled = keys != 0
    s = torch.where(filled, (1 << 24) - 1 - (keys & ((1 << 24) - 1)), torch.zeros((), dtype=torch.int64, device=flow.device))
    image = torch.gather(image0.reshape(n, 3, -1), 2, s[:, None].expand(n, 3, -1)) * filled[:, None]
    sx, sy = s % W, s // W
    to_own = torch.stack([(sx - xs.reshape(1, -1)).float(), (sy - ys.reshape(1, -1)).float()], 1) * filled[:, None]
    to_other = (to_own + torch.gather(fl.reshape(n, 2, -1), 2, s[:, None].expand(n, 2, -1))) * filled[:, None]
    return keys, image, to_own, to_other, filled


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
    extras = ("flow1", "occ0", "occ1", "label0", "label1")

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
            xkw = dict(flow_dtype=kw["flow_dtype"], occ_dtype=torch.uint8 if flow_f16 else None)
            outs, ex = ofdg.alloc_outputs(B, H, W, **kw), ofdg.alloc_extras(B, H, W, extras, **xkw)
            torch.cuda.synchronize()
            g.forward_counter(0, B, *outs, s, extras=ex)
            torch.cuda.synchronize()
            splat = ofdg.alloc_splat(B, H, W, (0, 1), image_dtype=outs[0].dtype, flow_dtype=outs[2].dtype)
            repro = ofdg.alloc_reproject(B, H, W, (0, 1), ofdg.REPROJ_OUTPUTS, outs[0].dtype)
            sets[(image_u8, flow_f16)] = (outs, ex, splat, repro)
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

    size = lambda t: t.numel() * t.element_size()  # noqa: E731
    for rnd in range(args.rounds):
        for (image_u8, flow_f16), (outs, ex, (planes, keys, rows, recs_out), (rplanes, rrows)) in sets.items():
            fmt = dict(frames_fmt="u8" if image_u8 else "f32", flow_fmt="f16" if flow_f16 else "f32")
            flows, occ, labels = (outs[2], ex["flow1"]), (ex["occ0"], ex["occ1"]), (ex["label0"], ex["label1"])
            for frames in ((0,), (0, 1)):
                yard = {}
                for name, outputs in REPROJECT.items():
                    out = {ofdg.reproject_key(n_, f): rplanes[ofdg.reproject_key(n_, f)] for f in frames for n_ in outputs if n_ != "rows"}
                    r = rrows if "rows" in outputs else None
                    med, yard[name] = timed(lambda: g.reproject(outs[:2], flows, occ, out=out, rows=r, frames=frames, stream=s))
                    emit(dict(fmt, kernel="reproject", outputs=name, round=rnd, frames=list(frames), us_median=med, us_device=yard[name]))
                for with_labels in (True, False):
                    for name, outputs in FORMS:
                        out = {ofdg.splat_key(n_, f): planes[ofdg.splat_key(n_, f)] for f in frames for n_ in outputs if n_ != "rows"}
                        r = rows if "rows" in outputs else None
                        for t_q8 in (0, 128, 256):
                            recs = torch.tensor([[t_q8, t_q8, 0, 0]] * B, dtype=torch.int32, device="cuda")
                            med, dev = timed(lambda: g.splat(outs[:2], flows, labels if with_labels else None, occ, recs=recs, out=out, keys=keys, rows=r,
                                                             frames=frames, recs_out=recs_out, stream=s))
                            # (per frame: the key plane cleared, raised and read; the flow read by both kernels unless keys alone)
                            passes = 2 if outputs else 1
                            read = sum(size(keys[f]) * (2 + passes) + size(flows[f]) * passes + (size(labels[f]) * passes if with_labels else 0) for f in frames)
                            read += sum(size(outs[f]) for f in frames if "image" in outputs) + sum(size(occ[f]) * 2 for f in frames if r is not None)
                            moved = read + sum(size(t) for t in out.values())
                            line = dict(fmt, kernel="splat", outputs=name, labels=with_labels, t_q8=t_q8, round=rnd, frames=list(frames), us_median=med, us_device=dev,
                                        moved_MB=round(moved / 1e6, 1), GBps=round(moved / dev / 1e3, 1))
                            if name in yard:
                                line["x_reproject"] = round(dev / yard[name], 2)
                            emit(line)
            if not image_u8 and not flow_f16:
                med, dev = timed(lambda: torch_restatement(outs[0], outs[2], ex["label0"], 256), reps=10)
                emit(dict(fmt, kernel="torch eager: scatter_reduce_(amax) of the keys, gathers of image and flows, frame 0", t_q8=256, round=rnd, frames=[0],
                          us_median=med, us_device=dev))
    del g
    if args.kernel_only:
        return
    for rep in range(args.reps):
        for name, more in (("plain", {}), ("splat", dict(splat=dict(t=(0.0, 1.0), frames=(0, 1))))):
            it = iter(ofdg.FlowLoader(ofdg.default_params(**params), pool=pool, prefetch=3, extras=extras, **more))
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
