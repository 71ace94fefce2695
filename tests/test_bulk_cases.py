"""The 16 patterns of tests/bulk_cases.py, without a GPU: for every operation the host twin equals the numpy restatement on
them, cyclic neighbours take different paths through the kernel - read from the restatement's own intermediate values - and no
pattern lies in a range the restatement leaves out.  What tests/test_gpu_many_samples.py concludes from a periodic batch rests
on this."""
import numpy as np
import pytest

import bulk_cases as bc

OPS = sorted(bc.CASES)


@pytest.mark.parametrize("wide", [False, True], ids=["small", "wide"])
@pytest.mark.parametrize("name", OPS)
def test_twin_equals_restatement_and_neighbours_differ(ofdg, name, wide):
    c = bc.case(name, wide=wide)
    assert len(c.paths) == bc.P and all(v.shape[0] == bc.P for v in c.inputs.values())
    assert bc.neighbours_differ(c.paths) == [], (name, c.paths)
    assert not any(c.excluded), (name, c.excluded, c.paths)
    for got, want, what in c.twin_and_restatement(ofdg):
        bc.expect_same(got, want, "%s (%s): %s" % (name, "wide" if wide else "small", what))
    # the sizes the GPU tests rely on
    last = (bc.N_BULK - 1) * 4 * c.W * c.H
    if wide:
        assert min(3, c.channels) * last >= 2 ** 32 and c.W % 16 == 0 and c.H % 2 == 0
    else:
        assert (c.H, c.W) == bc.SMALL


VARIANTS = [("pack", dict(layout=layout, concat=concat, rgb=rgb)) for layout in (0, 1) for concat in (False, True) for rgb in (False, True)] + \
    [("erase", dict(fill=1)), ("boundaries", dict(labels=False, radius=15, min_step=0.5)), ("boundaries", dict(labels=True, radius=1, min_step=3.0)),
     ("flow_vis", dict(norm="fixed", layout="hwc_rgb")), ("flow_vis", dict(norm="sample", layout="hwc_rgb")), ("flow_vis", dict(norm="batch"))]


@pytest.mark.parametrize("name,kw", VARIANTS, ids=lambda v: v if isinstance(v, str) else "-".join("%s" % x for x in v.values()))
def test_per_call_modes_twin_equals_restatement(ofdg, name, kw):
    """the modes that are per call: the same 16 patterns under each mode the GPU tests run"""
    c = bc.case(name, **kw)
    for got, want, what in c.twin_and_restatement(ofdg):
        bc.expect_same(got, want, "%s %s: %s" % (name, kw, what))


def test_flow_vis_batch_extreme(ofdg):
    """norm "batch" with the 17th pattern behind the 16: its vector is the longest, and twin and restatement agree on all 17"""
    c = bc.case("flow_vis", norm="batch")
    inputs = {k: np.concatenate([c.inputs[k], c.last[k]]) for k in c.inputs}
    bc.expect_same(c.twin(ofdg, inputs), c.restate(inputs), "flow_vis batch, 17 samples")
    assert c.restate(c.last)["rows"].view(c.ref.ROW)["max_r2_q16"][0] > c.ref.flow_vis(c.inputs["flow"], None, "sample")[1]["max_r2_q16"].max()


def test_flow_error_sums(ofdg):
    """bulk_cases.summed against the twin itself on a batch small enough to run whole: 16 * 3 + 5 periodic samples and the extreme"""
    c = bc.case("flow_error")
    n = 16 * 3 + 5 + 1
    idx = np.arange(n - 1) % bc.P
    inputs = {k: np.concatenate([c.inputs[k][idx], c.last[k]]) for k in c.inputs}
    got = bc.int_rows(c.twin(ofdg, inputs, one_row=True)["rows"].view(c.ref.ROW))[0]
    per = bc.int_rows(c.twin(ofdg, c.inputs)["rows"].view(c.ref.ROW))
    last = bc.int_rows(c.twin(ofdg, c.last)["rows"].view(c.ref.ROW))[0]
    want = bc.summed(per, n, last, maxima=("max_key",))
    want[("max_key",)] = last[("max_key",)] - (n - 1) * c.H * c.W
    assert got == want
    assert bc.int_rows(c.restate(inputs, one_row=True)["rows"].view(c.ref.ROW))[0] == want


@pytest.mark.parametrize("name", sorted(bc.RECORD_CASES) + ["erase"])
def test_drawn_records_twin_equals_restatement(ofdg, name):
    """the six samples the drawn GPU test looks at, each alone at first_index + s: the records (sanitised) and the frames"""
    c = bc.case(name, **(dict(fill=1) if name == "erase" else {}))
    seen = set()
    for s in bc.DRAWN_AT:
        one = {k: v[s % bc.P:s % bc.P + 1] for k, v in c.inputs.items()}
        twin = c.twin(ofdg, one, first_index=bc.FIRST_INDEX + s)
        bc.expect_same(twin, c.restate(one, None, first_index=bc.FIRST_INDEX + s), "%s drawn at first_index + %d" % (name, s))
        seen.add(twin["recs_out"].tobytes())
    assert len(seen) > 1
    assert bc.FIRST_INDEX < 2 ** 40 <= bc.FIRST_INDEX + bc.P and 65535 % bc.P == 15 and bc.N_BULK == 65535 + bc.P


def test_motion_blur_paths():
    """copy, window and gather all occur, non-finite flow is among the patterns, and one pattern blurs one frame only"""
    c = bc.case("motion_blur")
    flat = {p for pattern in c.paths for frame in pattern for p in frame}
    assert flat == {"copy", "window", "gather"}
    assert any(p[0] != p[1] and ("copy",) in p for p in c.paths)
    assert any(not np.isfinite(c.inputs["flow"][k].astype(np.float32)).all() for k in range(bc.P))
    for k, kind in enumerate(c.kinds()):
        if kind in ("copy", "window", "gather"):
            want = ((kind,), (kind,)) if k != 7 else (("copy",), ("gather",))
            assert c.paths[k] == want, (k, kind, c.paths[k])


def test_jitter_patterns():
    c = bc.case("jitter")
    kinds = {k for p in c.paths for k in p[0]}
    assert kinds == {"copy", "mean", "continue"} and {p[1] for p in c.paths} == {0, 1}
    assert {o for p in c.paths for o in p[2]} == set(range(24))
    assert any(p[0] == ("continue", "mean") for p in c.paths)


def test_flow_patterns():
    c = bc.case("flow_stats")
    assert set(c.paths) == {"empty", "const", "noisy", "hidden"}
    rows = c.restate_rows(c.inputs)
    top = max(r["max_key"] >> 32 for r in rows)
    assert c.restate_rows(c.last)[0]["max_key"] >> 32 > top
    assert [r["max_key"] == 0 for r in rows] == [k == "empty" for k in c.kinds]
