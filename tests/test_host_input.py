"""CPU tests of the code that reads untrusted input (csrc/host_input.cpp, csrc/host_api.cpp: the prototxt parser, the image
readers, the texture list's plan).  Inputs that once ended the process run in a child; tools/host_input_check.cpp is the
same code as a stand-alone ASan + UBSan program (make san), run here on a seed set and compared with libofdg.so's answers."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from test_host_logic import PROTOTXT

# CPU machines only: a sanitizer build has no business on a GPU machine, and the rest of the file needs none
pytestmark = pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="runs on CPU machines only")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "optical-flow-2d-data-generation_amd")
NOT_AN_IMAGE = "neither a binary PPM (P6, maxval 255) nor a PNG"

# The call in a fresh interpreter: prints the error code and text, then the growth of the peak resident set in KiB.
CHILD = '''
import importlib, resource, sys
sys.path.insert(0, %r)
ofdg = importlib.import_module("optical-flow-2d-data-generation_amd")
ofdg.lib()
before = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
try:
    r = %%s
    print("OK", r)
except ofdg.OfdgError as e:
    print("ERR", e.code, e)
print("KIB", resource.getrusage(resource.RUSAGE_SELF).ru_maxrss - before)
''' % ROOT


def in_child(expr):
    """(first line, KiB the peak resident set grew by) of `expr` evaluated in a fresh python; a process that dies fails here."""
    r = subprocess.run([sys.executable, "-c", CHILD % expr], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    lines = r.stdout.strip().split("\n")
    return lines[0], int(lines[-1].split()[1])


# Headers that claim what the file does not hold, and headers the old list scan let through.  (name, bytes)
BAD_PPMS = [
    ("claims_30gb", b"P6\n100000 100000\n255\nabc"),                 # 28 bytes: once allocated and zeroed 30 GB
    ("claims_12e18", b"P6\n2000000000 2000000000\n255\n"),          # 30 bytes: once std::length_error -> std::terminate
    ("maxval_65535", b"P6\n4 2\n65535\n" + bytes(48)),
    ("negative_width", b"P6\n-4 2\n255\n" + bytes(24)),
    ("width_99999999999", b"P6\n99999999999 2\n255\n" + bytes(24)),
    ("header_only", b"P6\n4 2\n255\n"),
]


@pytest.mark.parametrize("name,data", BAD_PPMS, ids=[n for n, _ in BAD_PPMS])
def test_decode_image_refuses_ppm_headers_the_file_does_not_bear_out(ofdg, tmp_path, name, data):
    """ETEXTURES with the reader's text, without allocating what the header claims: the file has a few dozen bytes, so the
    peak resident set may grow by the pages a refusal touches - 16 MiB is far above that and far below the 30 GB once zeroed."""
    p = tmp_path / (name + ".ppm")
    p.write_bytes(data)
    line, kib = in_child("ofdg.decode_image(%r).shape" % str(p))
    assert line.startswith("ERR %d " % ofdg.ETEXTURES) and line.endswith(": cannot read %s: %s" % (p, NOT_AN_IMAGE)), line
    assert kib < 16 * 1024, kib


def test_prototxt_nesting_is_not_recursion(ofdg):
    """100 000 open messages: "missing '}'", not a stack overflow; closed again and followed by the ordinary layer block, the
    ordinary values (fields under unknown messages are ignored)."""
    line, _ = in_child('ofdg.parse_prototxt("a{" * 100000)')
    assert line.startswith("ERR %d " % ofdg.EINVAL) and "missing '}'" in line, line
    line, _ = in_child('(lambda p, db, n: (p.mode, p.batch_size, p.prefetch, p.first_level_threads, p.second_level_threads, p.background_prep, db, n))'
                       '(*ofdg.parse_prototxt("a{" * 100000 + "}" * 100000 + %r))' % PROTOTXT)
    assert line == "OK (7, 8, 40, 8, 3, 1, '/data/textures/database.txt', 3)", line


# ---- the stand-alone sanitizer program ----------------------------------------------------------------------------------
def fnv1a(data):
    h = 14695981039346656037
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def write_seeds(d):
    """Small good files of every kind the readers take: the longest header (a.ppm, 25 bytes) lies inside the program's window."""
    from PIL import Image, PngImagePlugin
    rng = np.random.RandomState(11)
    rgb = rng.randint(0, 256, (12, 16, 3)).astype(np.uint8)
    (d / "a.ppm").write_bytes(b"P6\n# one\n# two\n16 12\n255\n" + rgb.tobytes())
    (d / "b.ppm").write_bytes(b"P6 5 3 255\n" + rgb.tobytes()[:45])
    Image.fromarray(rgb).save(d / "rgb.png")
    Image.fromarray(rgb).quantize(8).save(d / "palette.png")
    Image.fromarray(np.dstack([rgb, rgb[:, :, :1]]), "RGBA").save(d / "rgba.png")
    info = PngImagePlugin.PngInfo()
    info.add(b"gAMA", struct.pack(">I", 100000))
    Image.fromarray(rgb[:, :, 0], "L").save(d / "grey_gamma.png", pnginfo=info)
    (d / "layer.prototxt").write_text(PROTOTXT)
    (d / "nested.prototxt").write_text('layer { type: "DataGeneration" include { phase: TRAIN x { y: 1 } } data_generation_param { mode: 5 sampler: counter } }')


@pytest.fixture(scope="module")
def san_program():
    subprocess.run(["make", "-s", "-C", PKG, "san"], check=True)
    return os.path.join(PKG, "build", "san", "host_input_check")


def run_san(program, mode, d):
    # Measured where this was written: `mutate` 0.67 s on the seed set (8 793 cases), `check` 0.02 s; three times the longer
    # one, rounded up to whole seconds.
    r = subprocess.run([program, mode, str(d)], capture_output=True, text=True, timeout=3)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout.split("\n")[:-1]


def test_host_twins_read_planes_at_an_odd_address_under_the_sanitizers(san_program, tmp_path):
    """ofdg_host_flow_stats, ofdg_host_flow_pyramid and ofdg_host_crop ask no alignment of their inputs: a binary16 flow and a
    float32 map one byte off give the bytes of the aligned planes, with no ASan / UBSan report (exit 0)."""
    assert run_san(san_program, "planes", tmp_path)[-1].endswith("odd=same")


def test_range_overlap_checker_gives_its_known_answers_under_the_sanitizers(san_program, tmp_path):
    """RangeSet and frame_pair_ranges (csrc/ofdg_device.h), the rule every post-processing operation decides with whether a kernel
    may write to a caller's pointer: touching ranges, a one-byte overlap from either side in either order, read-read, the
    in-place pair (same pointer and same format only), a written range against another frame's pair, the set at full capacity -
    17 checks of which 11 are refusals, none wrong, no ASan / UBSan report (exit 0)."""
    assert run_san(san_program, "overlap", tmp_path)[-1] == "overlap checks=17 refused=11 wrong=0"


def test_sanitizer_build_agrees_with_the_library_and_survives_the_mutations(ofdg, san_program, tmp_path):
    """Two builds of one source agree: every line of `check` equals what libofdg.so answers through ctypes; `mutate` ends with
    exit 0 (no ASan / UBSan report, no escaped exception) and refuses most, not all, of what it made."""
    from PIL import Image
    write_seeds(tmp_path)
    counts = run_san(san_program, "mutate", tmp_path)[-1]
    cases, probe, decode, parser = (int(x.split("=")[-1]) for x in counts.replace("refused: ", "").split())
    assert cases > 5000 and 0 < decode < cases and probe <= decode and 0 < parser < cases, counts
    # the refusals join the seeds for `check`
    for name, data in BAD_PPMS:
        (tmp_path / (name + ".ppm")).write_bytes(data)
    Image.fromarray(np.zeros((4, 4), np.uint16)).save(tmp_path / "deep.png")
    (tmp_path / "cut.png").write_bytes((tmp_path / "rgb.png").read_bytes()[:60])
    Image.fromarray(np.zeros((4, 4, 3), np.uint8)).save(tmp_path / "c.bmp")
    (tmp_path / "typo.prototxt").write_text(PROTOTXT.replace("mode: 7", "moode: 7"))
    (tmp_path / "open.prototxt").write_text(PROTOTXT[:-4])
    L = ofdg.lib()
    L.ofdg_host_decode_image.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.ofdg_host_last_error.restype = C.c_char_p
    want = []
    for name in sorted(os.listdir(tmp_path)):
        path = str(tmp_path / name).encode()
        if name.endswith(".prototxt"):
            p, db, ntop = ofdg.Params(), C.create_string_buffer(4096), C.c_int(0)
            rc = L.ofdg_parse_prototxt(open(path).read().encode(), C.byref(p), db, 4096, C.byref(ntop))
            want.append("prototxt %s rc=%d mode=%d batch=%d prefetch=%d threads=%d,%d aa=%d size=%dx%d objects=%d seed=%d chains=%d lookahead=%d "
                        "prep=%d sampler=%d db=%s tops=%d msg=%s" % (
                            name, rc, p.mode, p.batch_size, p.prefetch, p.first_level_threads, p.second_level_threads, p.use_antialiasing,
                            p.width, p.height, p.num_objects, p.seed, p.chains, p.lookahead, p.background_prep, p.sampler, db.value.decode(),
                            ntop.value, L.ofdg_host_last_error().decode() if rc else ""))
            continue
        w, h = C.c_int(0), C.c_int(0)
        rc = L.ofdg_host_decode_image(path, None, 0, C.byref(w), C.byref(h))
        want.append("image %s size rc=%d %dx%d msg=%s" % (name, rc, w.value, h.value, L.ofdg_host_last_error().decode() if rc else ""))
        planes = np.zeros(1 if rc else 3 * w.value * h.value, np.uint8)
        w, h = C.c_int(0), C.c_int(0)
        rc = L.ofdg_host_decode_image(path, planes.ctypes.data_as(C.c_void_p), planes.size, C.byref(w), C.byref(h))
        want.append("image %s decode rc=%d %dx%d fnv=%016x msg=%s" % (name, rc, w.value, h.value, 0 if rc else fnv1a(planes.tobytes()),
                                                                      L.ofdg_host_last_error().decode() if rc else ""))
    got = run_san(san_program, "check", tmp_path)
    assert got == want
    assert sum(" rc=0 " in g for g in got) == 2 * 6 + 2 and sum(NOT_AN_IMAGE in g for g in got) == 2 * 7


def test_texture_list_plan(san_program, tmp_path):
    """plan_texture_collection through `check`: uniform and mixed sizes, the dropped last line without a newline (DG:124-126), the
    reference's message for an empty and a missing list (DG:121), and every unusable member named in ONE error."""
    from PIL import Image
    img = tmp_path / "img"
    img.mkdir()
    write_seeds(img)
    for name, data in BAD_PPMS[2:4]:
        (img / (name + ".ppm")).write_bytes(data)
    Image.fromarray(np.zeros((4, 4), np.uint16)).save(img / "deep.png")
    (img / "junk.ppm").write_bytes(b"not an image")
    lists = tmp_path / "lists"
    lists.mkdir()

    def listing(names, end="\n"):
        return "\n".join(str(img / n) for n in names) + end
    (lists / "uniform.txt").write_text(listing(["a.ppm", "rgb.png", "palette.png"]))
    (lists / "mixed.txt").write_text(listing(["a.ppm", "b.ppm", "rgb.png"]))
    (lists / "no_newline.txt").write_text(listing(["a.ppm", "rgb.png", "b.ppm"], end=""))
    (lists / "empty.txt").write_text("")
    bad = ["maxval_65535.ppm", "negative_width.ppm", "deep.png", "junk.ppm"]   # three kinds: PPM header, 16-bit PNG, no image
    (lists / "unusable.txt").write_text(listing(["a.ppm", bad[0], bad[1], "rgb.png", bad[2], bad[3]]))
    (lists / "missing_member.txt").write_text(listing(["a.ppm", "nowhere.ppm"]))
    out = run_san(san_program, "check", lists)
    head = {l.split()[1]: l for l in out if l.startswith("list ")}
    assert head["uniform.txt"] == "list uniform.txt files=3 mixed=false error="
    assert head["mixed.txt"] == "list mixed.txt files=3 mixed=true error="
    assert head["no_newline.txt"] == "list no_newline.txt files=2 mixed=false error="
    assert out[out.index(head["mixed.txt"]) + 1:][:3] == ["  %s %s" % (img / n, s) for n, s in (("a.ppm", "16x12"), ("b.ppm", "5x3"), ("rgb.png", "16x12"))]
    assert head["empty.txt"] == "list empty.txt files=0 mixed=false error=Could not open texture collection (no images listed)"
    msg = head["unusable.txt"].split("error=")[1]
    assert msg.startswith("Could not open texture collection (cannot read 4 files: ") and msg.count(NOT_AN_IMAGE) == 3 and "16-bit" in msg
    assert all(str(img / n) + ": " in msg for n in bad) and str(img / "a.ppm") not in msg and str(img / "rgb.png") not in msg
    assert head["missing_member.txt"].endswith("error=Could not open texture collection (cannot read %s: %s)" % (img / "nowhere.ppm", NOT_AN_IMAGE))
    gone = run_san(san_program, "check", lists / "missing.txt")   # (a path that is no directory is checked as the one file)
    assert gone == ["list missing.txt files=0 mixed=false error=Could not open texture collection"]
