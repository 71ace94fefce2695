"""What the block compression costs: ofdg_jpeg alone on one batch of the bench's config 2 (mode 5, 512x384, batch 32, 16 objects,
counter sampler, background_prep 1, synthetic pool), on an otherwise idle device - the median of 30 calls between two events
("us_median": it holds what issuing the call from Python costs, some 20 us) and the device time of one call among ten queued
behind a long matrix product ("us_device"), --rounds interleaved rounds of all rows, one JSON line per row and round.  Every
row uses given records, the same for all samples, so that every sample works:

    jpeg         identity / 4:4:4 / 4:2:0 at quality 75, phase off (0, 0) / on (5, 11); float32 / uint8 on either side; in place /
                 copying; one frame / both; "moved_MB" is what the form has to read and write
    camera       a yardstick: ofdg_camera under sigma 1 on the same planes and formats
    jitter       the other yardstick: ofdg_jitter under the identity record, copying
    torch        an eager restatement in float32 (unfold into 8x8 blocks, two matmuls each way, the quantiser between them; the
                 colour transforms as 3x3 matmuls; 4:4:4, phase 0), for scale

Then "loader" lines: FlowLoader at config 2 with and without jpeg=JPEG_DEFAULT, --reps interleaved repetitions of --steps
steps.  With --out FILE the lines are appended to FILE too; "lib" names the library when OFDG_LIB selects another build.

    python tools/jpeg_cost.py [--rounds R] [--steps K] [--warmup W] [--reps R] [--pool N] [--out FILE] [--kernel-only]
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


def torch_eager(frame, luma, chroma):
    """4:4:4 at phase 0 in float32 on a [n,3,H,W] B, G, R frame (H, W multiples of 8): luma, chroma the tables as [8,8] tensors"""
    import math
    import torch
    x = frame.float()
    n, _, h, w = x.shape
    dev = x.device
    k = torch.arange(8, device=dev, dtype=torch.float32)
    Cm = torch.cos((2 * k[None, :] + 1) * k[:, None] * math.pi / 16) / 2
    Cm[0] *= math.sqrt(0.5)
    fwd = torch.tensor([[0.114, 0.587, 0.299], [0.5, -0.331264, -0.168736], [-0.081312, -0.418688, 0.5]], device=dev)   # Y, Cb, Cr of B, G, R
    ycc = torch.einsum("kc,nchw->nkhw", fwd, x) + torch.tensor([0.0, 128.0, 128.0], device=dev).view(1, 3, 1, 1)
    blocks = ycc.round().reshape(n, 3, h // 8, 8, w // 8, 8).permute(0, 1, 2, 4, 3, 5) - 128.0
    q = torch.stack([luma, chroma, chroma]).float().view(1, 3, 1, 1, 8, 8)
    coef = Cm @ blocks @ Cm.T
    coef = torch.round(coef / q) * q
    out = (Cm.T @ coef @ Cm + 128.0).round().clamp(0, 255).permute(0, 1, 2, 4, 3, 5).reshape(n, 3, h, w)
    back = torch.linalg.inv(fwd)
    bgr = torch.einsum("kc,nchw->nkhw", back, out - torch.tensor([0.0, 128.0, 128.0], device=dev).view(1, 3, 1, 1))
    return bgr.round().clamp(0, 255).to(frame.dtype)


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
        sets[u8] = outs[:2]
    dsts = {u8: ofdg.alloc_jpeg(B, H, W, torch.uint8 if u8 else torch.float32)[0] for u8 in (False, True)}
    # the in-place rows work on copies of their own: what they read changes from call to call, what they cost does not
    own = {u8: tuple(t.clone() for t in sets[u8]) for u8 in (False, True)}
    rout = ofdg.alloc_jpeg(B)[1]
    cout = ofdg.alloc_camera(B, 8, 8)[1]
    work, jout = ofdg.alloc_jitter(B)

    def records(quality=0, sub=0, phase=(0, 0)):
        r = np.zeros((B,), ofdg._jpeg_rec_dtype())
        r["quality"], r["subsample"], r["phase_x"], r["phase_y"] = quality, sub, phase[0], phase[1]
        return torch.from_numpy(r.view(np.int32).reshape(B, ofdg.JPEG_REC_WORDS)).cuda()

    forms = [("identity", 0, 0, (0, 0))]
    for sub in (0, 1):
        for phase in ((0, 0), (5, 11)):
            forms.append(("%s phase %s" % ("4:2:0" if sub else "4:4:4", "on" if phase[0] else "off"), 75, sub, phase))
    forms = [(name, records(q, sub, phase), q, sub, phase) for name, q, sub, phase in forms]
    camera_sigma1 = np.zeros((B,), ofdg._camera_rec_dtype())
    camera_sigma1["sigma_q8"], camera_sigma1["bayer"] = 256, -1
    camera_sigma1 = torch.from_numpy(camera_sigma1.view(np.int32).reshape(B, ofdg.CAMERA_REC_WORDS)).cuda()
    jitter_identity = np.zeros((B,), ofdg._jitter_rec_dtype())
    for k in ("brightness", "contrast", "saturation"):
        jitter_identity[k] = ofdg.JITTER_ONE
    jitter_identity = torch.from_numpy(jitter_identity.view(np.int32).reshape(B, ofdg.JITTER_REC_WORDS)).cuda()
    tables = tuple(torch.from_numpy(t.astype(np.float32)).cuda() for t in ofdg.host_jpeg_tables(75))
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
            src = sets[src_u8]
            for dst_u8 in (False, True):
                dst = dsts[dst_u8]
                fmt = ("u8" if src_u8 else "f32") + " to " + ("u8" if dst_u8 else "f32")
                frame_mb = (src[0].numel() * src[0].element_size() + dst[0].numel() * dst[0].element_size()) / 1e6
                for name, recs, q, sub, phase in forms:
                    for frames in ((0, 1), (0,)):
                        for in_place in (False, True):
                            if in_place and (src_u8 != dst_u8 or frames == (0,)):
                                continue
                            if frames == (0,) and name not in ("identity", "4:2:0 phase on"):
                                continue
                            pick = lambda pair: tuple(t if f in frames else None for f, t in enumerate(pair))  # noqa: E731
                            a, b = (pick(own[src_u8]), None) if in_place else (pick(src), pick(dst))
                            med, best = timed(lambda: g.jpeg(a, b, recs=recs, recs_out=rout, stream=s))
                            emit({"kernel": "jpeg", "form": name, "round": rnd, "fmt": fmt, "frames": list(frames), "in_place": in_place, "quality": q,
                                  "subsample": sub, "phase": list(phase), "us_median": med, "us_device": best,
                                  "moved_MB": round(frame_mb * len(frames) * (0.0 if in_place and q == 0 else 1.0), 1)})
                med, best = timed(lambda: g.camera(src, dst, recs=camera_sigma1, recs_out=cout, stream=s))
                emit({"kernel": "camera, sigma 1, both frames", "round": rnd, "fmt": fmt, "us_median": med, "us_device": best, "moved_MB": round(2 * frame_mb, 1)})
                med, best = timed(lambda: g.jitter(src, dst, recs=jitter_identity, recs_out=jout, work=work, stream=s))
                emit({"kernel": "jitter, identity record, copying, both frames", "round": rnd, "fmt": fmt, "us_median": med, "us_device": best,
                      "moved_MB": round(2 * frame_mb, 1)})
            med, best = timed(lambda: (torch_eager(src[0], *tables), torch_eager(src[1], *tables)), reps=5)
            emit({"kernel": "torch eager, both frames", "form": "4:4:4 phase off", "round": rnd, "fmt": "u8" if src_u8 else "f32", "us_median": med, "us_device": best})
    del g
    if args.kernel_only:
        return
    for rep in range(args.reps):
        for name, more in (("plain", {}), ("jpeg", dict(jpeg=ofdg.JPEG_DEFAULT))):
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
