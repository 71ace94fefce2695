"""What the camera costs: ofdg_camera alone on one batch of the bench's config 2 (mode 5, 512x384, batch 32, 16 objects, counter
sampler, background_prep 1, synthetic pool), on an otherwise idle device - the median of 30 calls between two events
("us_median": it holds what issuing the call from Python costs, some 20 us) and the device time of one call among ten queued
behind a long matrix product ("us_device"), --rounds interleaved rounds of all rows, one JSON line per row and round.  Every
row uses given records, the same for all samples, so that every sample works:

    camera       identity / Bayer only / sigma 0.5, 1, 2, 4 px without and with Bayer, float32 / uint8 on either side, one frame /
                 both; "moved_MB" is what the form has to read and write
    motion_blur  the yardstick of the identity: ofdg_motion_blur at shutter 0 - a copy through the same accessors - on the same
                 planes and formats
    jitter       the other yardstick: ofdg_jitter under the identity record, copying
    torch        an eager restatement in float32 (two conv2d with a 25-tap Gaussian, then the mosaic and the bilinear
                 demosaic as masked convolutions), for scale

Then "loader" lines: FlowLoader at config 2 with and without camera=CAMERA_DEFAULT, --reps interleaved repetitions of --steps
steps.  With --out FILE the lines are appended to FILE too; "lib" names the library when OFDG_LIB selects another build.

    python tools/camera_cost.py [--rounds R] [--steps K] [--warmup W] [--reps R] [--pool N] [--out FILE] [--kernel-only]
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


def torch_eager(frame, sigma_px, bayer):
    """the blur as two conv2d in float32 and the demosaic as masked 3x3 convolutions, on a [n,3,H,W] B, G, R frame"""
    import numpy as np
    import torch
    F = torch.nn.functional
    x = frame.float()
    n, _, h, w = x.shape
    if sigma_px > 0:
        R = min(12, int(np.ceil(3 * sigma_px)))
        k = torch.exp(-torch.arange(-R, R + 1, device=x.device, dtype=torch.float32) ** 2 / (2 * sigma_px * sigma_px))
        k = k / k.sum()
        x = x.reshape(n * 3, 1, h, w)
        x = F.conv2d(F.pad(x, (R, R, 0, 0), mode="replicate"), k.view(1, 1, 1, -1))
        x = F.conv2d(F.pad(x, (0, 0, R, R), mode="replicate"), k.view(1, 1, -1, 1)).reshape(n, 3, h, w)
    if bayer:
        yy, xx = torch.meshgrid(torch.arange(h, device=x.device), torch.arange(w, device=x.device), indexing="ij")
        a, b = xx & 1, yy & 1
        masks = torch.stack([(a == 1) & (b == 1), a != b, (a == 0) & (b == 0)]).float()   # B, G, R sites of RGGB
        m = (x * masks).reshape(n * 3, 1, h, w)
        rb = torch.tensor([[0.25, 0.5, 0.25], [0.5, 1.0, 0.5], [0.25, 0.5, 0.25]], device=x.device)
        gk = torch.tensor([[0.0, 0.25, 0.0], [0.25, 1.0, 0.25], [0.0, 0.25, 0.0]], device=x.device)
        m = F.pad(m, (1, 1, 1, 1), mode="reflect").reshape(n, 3, h + 2, w + 2)
        x = torch.cat([F.conv2d(m[:, 0:1], rb.view(1, 1, 3, 3)), F.conv2d(m[:, 1:2], gk.view(1, 1, 3, 3)), F.conv2d(m[:, 2:3], rb.view(1, 1, 3, 3))], dim=1)
    return x.round().clamp(0, 255).to(frame.dtype)


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
    seed = 20261021
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
        sets[u8] = (outs[:2], (outs[2], torch.empty_like(outs[2])))
    dsts = {u8: ofdg.alloc_camera(B, H, W, torch.uint8 if u8 else torch.float32)[0] for u8 in (False, True)}
    rout = ofdg.alloc_camera(B, 8, 8)[1]
    work, jout = ofdg.alloc_jitter(B)
    mout = ofdg.alloc_motion_blur(B, 8, 8)[1]

    def records(sigma_q8=0, bayer=-1):
        r = np.zeros((B,), ofdg._camera_rec_dtype())
        r["sigma_q8"], r["bayer"] = sigma_q8, bayer
        return torch.from_numpy(r.view(np.int32).reshape(B, ofdg.CAMERA_REC_WORDS)).cuda()

    forms = [("identity", 0, -1), ("Bayer only", 0, 0)]
    for px in (0.5, 1.0, 2.0, 4.0):
        forms += [("sigma %g" % px, int(px * 256), -1), ("sigma %g + Bayer" % px, int(px * 256), 0)]
    forms = [(name, records(sq, p), sq, p) for name, sq, p in forms]
    jitter_identity = np.zeros((B,), ofdg._jitter_rec_dtype())
    for k in ("brightness", "contrast", "saturation"):
        jitter_identity[k] = ofdg.JITTER_ONE
    jitter_identity = torch.from_numpy(jitter_identity.view(np.int32).reshape(B, ofdg.JITTER_REC_WORDS)).cuda()
    still = torch.zeros((B, ofdg.MBLUR_REC_FLOATS), dtype=torch.float32, device="cuda")
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

    for rnd in range(args.rounds):
        for src_u8 in (False, True):
            src, flows = sets[src_u8]
            for dst_u8 in (False, True):
                dst = dsts[dst_u8]
                fmt = ("u8" if src_u8 else "f32") + " to " + ("u8" if dst_u8 else "f32")
                frame_mb = (src[0].numel() * src[0].element_size() + dst[0].numel() * dst[0].element_size()) / 1e6
                for name, recs, sq, p in forms:
                    for frames in ((0, 1), (0,)):
                        if frames == (0,) and name not in ("identity", "sigma 1 + Bayer"):
                            continue
                        if src_u8 != dst_u8 and name not in ("identity", "Bayer only", "sigma 1", "sigma 1 + Bayer"):
                            continue
                        pick = lambda pair: tuple(t if f in frames else None for f, t in enumerate(pair))  # noqa: E731
                        a, b = pick(src), pick(dst)
                        med, best = timed(lambda: g.camera(a, b, recs=recs, recs_out=rout, stream=s))
                        emit({"kernel": "camera", "form": name, "round": rnd, "fmt": fmt, "frames": list(frames), "sigma_q8": sq, "bayer": p,
                              "us_median": med, "us_device": best, "moved_MB": round(frame_mb * len(frames), 1)})
                med, best = timed(lambda: g.motion_blur(src, dst, flow=(flows[0], flows[0]), recs=still, recs_out=mout, stream=s))
                emit({"kernel": "motion_blur at shutter 0, both frames", "round": rnd, "fmt": fmt, "us_median": med, "us_device": best, "moved_MB": round(2 * frame_mb, 1)})
                med, best = timed(lambda: g.jitter(src, dst, recs=jitter_identity, recs_out=jout, work=work, stream=s))
                emit({"kernel": "jitter, identity record, copying, both frames", "round": rnd, "fmt": fmt, "us_median": med, "us_device": best,
                      "moved_MB": round(2 * frame_mb, 1)})
            for px, bayer in ((1.0, False), (1.0, True), (4.0, False), (0.0, True)):
                med, best = timed(lambda: (torch_eager(src[0], px, bayer), torch_eager(src[1], px, bayer)), reps=5)
                emit({"kernel": "torch eager, both frames", "form": "sigma %g%s" % (px, " + Bayer" if bayer else ""), "round": rnd,
                      "fmt": "u8" if src_u8 else "f32", "us_median": med, "us_device": best})
    del g
    if args.kernel_only:
        return
    for rep in range(args.reps):
        for name, more in (("plain", {}), ("camera", dict(camera=ofdg.CAMERA_DEFAULT))):
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
