#!/usr/bin/env python3
"""Regenerates the tests/golden/ref_* fixtures from the REFERENCE's own compiled code: the harnesses of oracle/
(ref_sampler, ref_warpfields_det, ref_motion), which `make -C oracle ref` builds into oracle/_ref/ where the reference
checkout exists (only possible in the build container).  Data only: task streams, displacer lists, float fields and
affines the reference's programs wrote, and digests of them.

    python tests/golden/gen_ref_goldens.py            # rewrites the fixtures (byte-identical on a re-run)
    python tests/golden/gen_ref_goldens.py --check    # compares instead of writing; exit status 1 on a difference

  ref_sampler_streams.json   per mode 1..13, 200 tasks: sha256 of the stream, 12-hex digest per task
  ref_sampler_tasks.npz      the first 2 tasks of every mode in full (uint8 "m<mode>_t<k>")
  ref_warpfields.json        per set: frame, seed, interposed expf calls, digest per plane of the big field and per crop
  ref_warpfields.npz         per set: the displacer list, every 8th texel of the field; the hand-made set in full
  ref_motion_mode5.json, ref_motion_mode7.json   ref_motion's output for 2 tasks, verbatim
"""
import hashlib
import io
import json
import os
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracle_lib as oracle  # noqa: E402  (only for the seeded displacer LISTS, the harness's input)
import ref_stream as rs      # noqa: E402


def run_field(binary, size, displacers):
    """(field float32 [4, size, size], the harness's report) of one run of a ref_warpfields build."""
    with tempfile.TemporaryDirectory() as tmp:
        src, dst = os.path.join(tmp, "d.f64"), os.path.join(tmp, "f.f32")
        np.ascontiguousarray(displacers, "<f8").tofile(src)
        rep = json.loads(subprocess.check_output([os.path.join(rs.REF_BIN, binary), str(size), src, dst]))
        return np.fromfile(dst, "<f4").reshape(4, size, size), rep


def npz_bytes(arrays):
    """A deterministic .npz: what np.savez_compressed writes, but with sorted keys and a fixed time stamp."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            one = io.BytesIO()
            np.lib.format.write_array(one, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, one.getvalue())
    return buf.getvalue()


def json_bytes(obj):
    return (json.dumps(obj, indent=1, sort_keys=True) + "\n").encode()


def sampler_fixtures():
    streams, full = {}, {}
    for mode in rs.MODES:
        raw = subprocess.check_output([os.path.join(rs.REF_BIN, "ref_sampler"), str(mode), str(rs.N_TASKS)])
        # cut the stream into tasks with the layout's own parser
        tasks, off = [], 0
        for _ in range(rs.N_TASKS):
            end = off
            _, end = rs.parse_blueprint(raw, end)
            n = int.from_bytes(raw[end:end + 4], "little", signed=True)
            end += 4
            for _ in range(n):
                _, end = rs.parse_blueprint(raw, end)
            tasks.append(raw[off:end])
            off = end
        assert off == len(raw), (mode, off, len(raw))
        streams[str(mode)] = {"sha256": hashlib.sha256(raw).hexdigest(), "n_bytes": len(raw),
                              "task_digests": [rs.task_digest(t) for t in tasks]}
        for k in range(rs.N_FULL):
            full["m%d_t%d" % (mode, k)] = np.frombuffer(tasks[k], np.uint8)
    return {"ref_sampler_streams.json": json_bytes({"n_tasks": rs.N_TASKS, "modes": streams}),
            "ref_sampler_tasks.npz": npz_bytes(full)}


def warp_fixtures():
    meta, arrays = {}, {}
    sets = [(name, 3 * max(W, H), oracle.displacers(W, H, seed), (W, H, seed)) for name, (W, H, seed) in sorted(rs.WARP_SETS.items())]
    sets.append(("hand96", rs.HAND_SIZE, rs.HAND_DISPLACERS, None))
    for name, size, disp, frame in sets:
        field, rep = run_field("ref_warpfields_det", size, disp)
        if not rep.get("expf_calls"):
            raise SystemExit("%s: the reference's code did not call the interposed expf - this is not the det-expf build" % name)
        m = {"size": size, "n_displacers": len(disp), "expf_calls": rep["expf_calls"], "nan_share": float(np.isnan(field).mean()),
             "plane_digests": [rs.field_digest(field[k]) for k in range(4)]}
        arrays[name + "_displacers"] = np.ascontiguousarray(disp, "<f8")
        if frame is None:
            arrays[name + "_field"] = rs.canon_bits(field).view(np.float32)
        else:
            W, H, seed = frame
            m.update(width=W, height=H, seed=seed, stride=rs.STRIDE)
            # the crops are sliced HERE, in Python, from the reference's field: rs.crop_origins is a third statement of the
            # reference's crop loop (WarpFields.cpp:617-633), independent of the oracle's and the product's
            m["crop_origins"] = [list(o) for o in rs.crop_origins(W, H)]
            m["crop_digests"] = [rs.field_digest(c) for c in rs.crops_of(field, W, H)]
            arrays[name + "_strided"] = rs.canon_bits(field[:, ::rs.STRIDE, ::rs.STRIDE]).view(np.float32)
        meta[name] = m
    return {"ref_warpfields.json": json_bytes(meta), "ref_warpfields.npz": npz_bytes(arrays)}


def motion_fixtures():
    return {"ref_motion_mode%d.json" % mode: subprocess.check_output([os.path.join(rs.REF_BIN, "ref_motion"), str(mode), "2"])
            for mode in (5, 7)}


def main():
    check = "--check" in sys.argv[1:]
    subprocess.check_call(["make", "-s", "-C", os.path.join(rs.ROOT, "oracle"), "ref"])
    if not os.path.exists(os.path.join(rs.REF_BIN, "ref_sampler")):
        raise SystemExit("oracle/_ref/ was not built: the reference checkout is absent")
    files = {}
    files.update(sampler_fixtures())
    files.update(warp_fixtures())
    files.update(motion_fixtures())
    limit = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if not f.startswith("ref_"))
    bad = 0
    for name, data in sorted(files.items()):
        path = os.path.join(HERE, name)
        if len(data) > limit:
            raise SystemExit("%s: %d bytes, more than the largest fixture so far (%d)" % (name, len(data), limit))
        if check:
            same = os.path.exists(path) and open(path, "rb").read() == data
            print("%-28s %7d bytes  %s" % (name, len(data), "identical" if same else "DIFFERS"))
            bad += not same
        else:
            with open(path, "wb") as f:
                f.write(data)
            print("%-28s %7d bytes" % (name, len(data)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
