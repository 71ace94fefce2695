"""Plain-numpy statement of the per-object annotation table's areas and boxes (include/ofdg.h, ofdg_object_row): of the
pixels of a label plane whose value is k, their number and the inclusive box x0, y0, x1, y1; no such pixel: area 0 and the
empty box {W, H, -1, -1}.  TEST INFRASTRUCTURE shared by tests/test_object_table.py and tests/test_gpu_object_table.py."""
import numpy as np


def area_and_box(plane, k):
    """(area, [x0, y0, x1, y1]) of label k in one uint8 plane [H, W]."""
    H, W = plane.shape
    sel = plane == k
    area = int(np.count_nonzero(sel))
    if area == 0:
        return 0, [W, H, -1, -1]
    ys, xs = np.nonzero(sel)
    return area, [int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())]


def expect_geometry(rows, label0, label1, shape):
    """Assert areas and boxes of one sample's rows (structured array, already cut to the rows that are reported) against the
    planes label0 / label1 [H, W]; None: that frame was not given (area 0, empty box).  shape = (H, W)."""
    H, W = shape
    for k in range(len(rows)):
        for f, plane in ((0, label0), (1, label1)):
            area, box = (0, [W, H, -1, -1]) if plane is None else area_and_box(plane, k)
            assert int(rows["area%d" % f][k]) == area, "row %d area%d: %d, numpy says %d" % (k, f, rows["area%d" % f][k], area)
            assert list(rows["box%d" % f][k]) == box, "row %d box%d: %s, numpy says %s" % (k, f, list(rows["box%d" % f][k]), box)
