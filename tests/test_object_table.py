"""Host-side tests of the per-object annotation table (ofdg_object_row, ofdg_object_table, ofdg_host_object_table in
include/ofdg.h): the layout in header / ctypes / numpy, the host restatement of the reduction against plain numpy on the
oracle's label planes and on hand-made planes, and the argument rules of the Python plumbing.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import extras_reference as xr
import object_table_reference as otr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = [("obj_id", 0, 4), ("obj_type", 4, 4), ("area0", 8, 4), ("area1", 12, 4), ("box0", 16, 16), ("box1", 32, 16), ("motion", 48, 48)]


def test_layout_is_96_bytes_everywhere(ofdg):
    hdr = open(os.path.join(ROOT, "include", "ofdg.h")).read()
    m = re.search(r"typedef struct ofdg_object_row \{(.*?)\} ofdg_object_row;", hdr, re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    decls = [re.sub(r"\s+", " ", d).strip() for d in body.split(";") if d.strip()]
    assert decls == ["int32_t obj_id", "int32_t obj_type", "int32_t area0, area1", "int32_t box0[4]", "int32_t box1[4]", "double motion[6]"]
    assert re.search(r"#define\s+OFDG_MAX_OBJECT_ROWS\s+65\b", hdr) and ofdg.MAX_OBJECT_ROWS == 65
    assert C.sizeof(ofdg.ObjectRow) == 96 and ofdg.OBJECT_ROW_DTYPE.itemsize == 96
    for name, offset, size in FIELDS:
        f = getattr(ofdg.ObjectRow, name)
        assert (f.offset, f.size) == (offset, size), name
        dt, off = ofdg.OBJECT_ROW_DTYPE.fields[name][:2]
        assert (off, dt.itemsize) == (offset, size), name
    assert [n for n, _ in ofdg.ObjectRow._fields_] == list(ofdg.OBJECT_ROW_DTYPE.names) == [n for n, _, _ in FIELDS]
    for fn in ("ofdg_object_table", "ofdg_host_object_table"):
        assert re.search(r"\bint\s+%s\s*\(" % fn, hdr), fn
        assert fn in ofdg.EXPORTS and hasattr(ofdg.lib(), fn)


@pytest.mark.parametrize("W,H", [(128, 96), (160, 100)])
@pytest.mark.parametrize("mode", [1, 5, 7, 13])
def test_host_object_table_against_numpy_on_oracle_labels(ofdg, oracle, mode, W, H):
    B = 2
    tasks, bps, n = ofdg.HostSampler(mode, W, H).next(B)
    pool = np.random.default_rng(3).integers(0, 256, (3, 3, 2 * H, 2 * W), dtype=np.uint8)
    q = oracle.default_params(W, H, mode)
    planes = [xr.labels_of(oracle, q, tasks[t], bps, pool)[:2] for t in range(B)]
    l0, l1 = np.stack([p[0] for p in planes]), np.stack([p[1] for p in planes])
    counts = np.array([1 + tasks[t].n_objects for t in range(B)], np.int32)
    assert l0.max() >= 1 and l1.max() >= 1
    tab = ofdg.host_object_table(l0, l1, counts)
    assert tab.shape == (B, ofdg.MAX_OBJECT_ROWS)
    for s in range(B):
        otr.expect_geometry(tab[s, :counts[s]], l0[s], l1[s], (H, W))
        assert int(tab["area0"][s].sum()) == int(tab["area1"][s].sum()) == W * H  # every pixel has exactly one owner
        rest = tab[s, counts[s]:]
        assert not rest.view(np.uint8).any()  # rows past the count are left alone
        assert not tab["obj_id"][s].any() and not tab["motion"][s].any()  # ... and so is every other field


def hand_made(W=24, H=10):
    """Labels 0..4 of a count of 5: 1 never occurs in frame 0, 2 is the single pixel (W-1, H-1), 4 covers all of frame 1."""
    l0 = np.zeros((1, H, W), np.uint8)
    l0[0, 2:5, 3:9] = 3
    l0[0, H - 1, W - 1] = 2
    l0[0, 0, 0] = 4
    l1 = np.full((1, H, W), 4, np.uint8)
    return l0, l1


def test_hand_made_planes(ofdg):
    l0, l1 = hand_made()
    H, W = l0.shape[1:]
    tab = ofdg.host_object_table(l0, l1, [5], rows_per_sample=7)[0]
    assert (tab["area0"][1], list(tab["box0"][1])) == (0, [W, H, -1, -1])               # a label that never occurs
    assert (tab["area0"][2], list(tab["box0"][2])) == (1, [W - 1, H - 1, W - 1, H - 1])  # one pixel in the last corner
    assert (tab["area0"][3], list(tab["box0"][3])) == (18, [3, 2, 8, 4])
    assert (tab["area0"][4], list(tab["box0"][4])) == (1, [0, 0, 0, 0])
    assert (tab["area1"][4], list(tab["box1"][4])) == (W * H, [0, 0, W - 1, H - 1])     # a label that covers the frame
    for k in range(4):
        assert (tab["area1"][k], list(tab["box1"][k])) == (0, [W, H, -1, -1])
    otr.expect_geometry(tab[:5], l0[0], l1[0], (H, W))
    assert not tab[5:].view(np.uint8).any()
    # one plane only: the other frame is empty
    only1 = ofdg.host_object_table(None, l1, [5], rows_per_sample=5)[0]
    otr.expect_geometry(only1, None, l1[0], (H, W))
    neither = ofdg.host_object_table(None, None, [5], rows_per_sample=5, width=W, height=H)[0]
    otr.expect_geometry(neither, None, None, (H, W))


def test_fewer_rows_than_objects_leaves_the_memory_behind_alone(ofdg):
    l0, l1 = hand_made()
    H, W = l0.shape[1:]
    full = ofdg.host_object_table(l0, l1, [5], rows_per_sample=5)[0]
    per = 3
    buf = np.full((1 + per + 2) * 96, 0xA5, np.uint8)  # one guard row in front, two behind
    rows = buf[96:96 + per * 96]
    counts = np.array([5], np.int32)
    rc = ofdg.lib().ofdg_host_object_table(l0.ctypes.data_as(C.c_void_p), l1.ctypes.data_as(C.c_void_p), 1, W, H,
                                           counts.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p), per)
    assert rc == ofdg.OK
    got = rows.view(ofdg.OBJECT_ROW_DTYPE)
    for name in ("area0", "area1", "box0", "box1"):
        assert np.array_equal(got[name], full[name][:per]), name
    assert (buf[:96] == 0xA5).all() and (buf[96 + per * 96:] == 0xA5).all()
    for name in ("obj_id", "obj_type"):  # the fields the host function leaves alone keep the fill
        assert (np.ascontiguousarray(got[name]).view(np.uint8) == 0xA5).all()
    assert counts[0] == 5
    # argument errors
    assert ofdg.lib().ofdg_host_object_table(None, None, 1, W, H, None, rows.ctypes.data_as(C.c_void_p), per) == ofdg.EINVAL
    assert ofdg.lib().ofdg_host_object_table(None, None, 1, W, H, counts.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p), 0) == ofdg.EINVAL


def test_object_table_numpy_cuts_to_the_count(ofdg):
    rows = np.zeros((2, 4, 96), np.uint8)
    t = rows.view(ofdg.OBJECT_ROW_DTYPE).reshape(2, 4)
    t["obj_id"] = np.arange(8).reshape(2, 4)
    out = ofdg.object_table_numpy(rows, np.array([3, 9], np.int32))
    assert [len(o) for o in out] == [3, 4]  # (a count beyond the table: the rows the table holds)
    assert list(out[0]["obj_id"]) == [0, 1, 2] and list(out[1]["obj_id"]) == [4, 5, 6, 7]
    assert out[0].dtype == ofdg.OBJECT_ROW_DTYPE


def test_object_table_argument_rules(ofdg):
    torch = pytest.importorskip("torch")
    N, H, W = 2, 16, 24
    rows, counts = ofdg.alloc_object_table(N, device="cpu")
    assert tuple(rows.shape) == (N, 65, 96) and rows.dtype == torch.uint8 and tuple(counts.shape) == (N,) and counts.dtype == torch.int32
    assert tuple(ofdg.alloc_object_table(3, rows=5, device="cpu")[0].shape) == (3, 5, 96)
    with pytest.raises(ValueError):
        ofdg.alloc_object_table(0, device="cpu")
    with pytest.raises(ValueError):
        ofdg.alloc_object_table(1, rows=0, device="cpu")
    lab = torch.zeros((N, H, W), dtype=torch.uint8)
    assert ofdg.object_table_format(lab, lab, rows, counts, H, W) == (N, 65)
    assert ofdg.object_table_format(None, lab, rows, counts, H, W, n=N) == (N, 65)
    assert ofdg.object_table_format(None, None, rows[:, :5].contiguous(), counts, H, W) == (N, 5)
    bad = [
        dict(label0=lab.to(torch.int8)),                          # labels are uint8
        dict(label1=lab[:1]),                                     # a sample short
        dict(label0=lab[:, None]),                                # [n,1,H,W] instead of [n,H,W]
        dict(label1=torch.zeros((N, W, H), dtype=torch.uint8)),   # transposed
        dict(rows=rows.to(torch.int8)),
        dict(rows=rows[:, :, :95]),                               # not rows of 96 bytes
        dict(rows=rows[0]),
        dict(rows=rows[:, :0]),                                   # rows_per_sample < 1
        dict(rows=None),
        dict(counts=None),
        dict(counts=counts.to(torch.int64)),
        dict(counts=counts[:1]),
        dict(n=N + 1),                                            # the table is of a batch of another size
    ]
    for change in bad:
        args = dict(label0=lab, label1=lab, rows=rows, counts=counts, n=None)
        args.update(change)
        with pytest.raises(ValueError):
            ofdg.object_table_format(args["label0"], args["label1"], args["rows"], args["counts"], H, W, n=args["n"])
    with pytest.raises(ValueError):
        ofdg.host_object_table(None, None, [3])  # no plane and no size
    with pytest.raises(ValueError):
        ofdg.host_object_table(np.zeros((2, H, W), np.uint8), None, [3])  # planes of two samples, one count


def test_flow_loader_objects_need_both_label_planes(ofdg):
    """(argument check only: it comes before the generator is created)"""
    for extras in (None, ("flow1",), ("label0",), ("label1", "occ0")):
        with pytest.raises(ValueError):
            ofdg.FlowLoader(extras=extras, objects=True)
