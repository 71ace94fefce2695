"""GPU tests of the post-processing operations beyond 65535 samples (part A) and with sample offsets past 2^32 bytes (part B):
periodic batches of the 16 patterns of tests/bulk_cases.py, n = 65551.  Every workgroup row goes round its sample loop twice,
on a pattern that takes another path than the one it has just served; sample s must equal sample s - 16 byte for byte, the
first 16 (part B: and the last 16) the host twin and the numpy restatement.  tests/test_bulk_cases.py checks the patterns
themselves without a GPU."""
import numpy as np
import pytest

import bulk_cases as bc

pytestmark = pytest.mark.gpu

P, N = bc.P, bc.N_BULK
FILL, GUARD = bc.FILL, bc.GUARD
CHUNK = 4096  # samples per comparison on the device


def make_gen(ofdg, case):
    return ofdg.Generator(ofdg.default_params(width=case.W, height=case.H, mode=7))


def tdtype(dt):
    import torch
    return getattr(torch, np.dtype(dt).name)


class Bufs:
    """device tensors between 0xA5 guards, all checked at once"""

    def __init__(self):
        self.raws = []

    def empty(self, shape, dtype, fill=FILL):
        import torch
        dt = tdtype(dtype)
        size = int(np.prod(shape)) * np.dtype(dtype).itemsize
        raw = torch.full((GUARD + size + GUARD,), fill, dtype=torch.uint8, device="cuda")
        if fill != FILL:
            raw[:GUARD] = FILL
            raw[-GUARD:] = FILL
        self.raws.append(raw)
        return raw[GUARD:GUARD + size].view(dt).view(tuple(shape))

    def repeated(self, patterns, n, last=None):
        """[n, ...]: sample s holds patterns[s mod 16], filled on the device; `last` (one sample) replaces sample n - 1"""
        import torch
        small = torch.from_numpy(np.array(patterns)).cuda()
        t = self.empty((n,) + tuple(small.shape[1:]), patterns.dtype)
        for lo in range(0, n, CHUNK * 4):
            hi = min(n, lo + CHUNK * 4)
            idx = torch.arange(lo, hi, device="cuda") % P
            t[lo:hi] = small[idx]
        if last is not None:
            t[n - 1] = torch.from_numpy(np.array(last)).cuda()[0]
        return t

    def intact(self):
        return all(bool((raw[:GUARD] == FILL).all()) and bool((raw[-GUARD:] == FILL).all()) for raw in self.raws)

    def bytes(self):
        return sum(raw.numel() for raw in self.raws)

    def free(self):
        import torch
        self.raws = []
        torch.cuda.empty_cache()


def as_words(t):
    """[n, bytes or words of a sample]"""
    import torch
    flat = t.reshape(t.shape[0], -1)
    per = flat.shape[1] * flat.element_size()
    return flat.view(torch.int32) if per % 4 == 0 and flat.data_ptr() % 4 == 0 else flat.view(torch.uint8)


def first_aperiodic(t, n=None):
    """the first sample s >= 16 (below n) that differs from sample s - 16 in any byte, or None"""
    w = as_words(t)
    n = w.shape[0] if n is None else n
    for lo in range(P, n, CHUNK):
        hi = min(n, lo + CHUNK)
        bad = (w[lo:hi] != w[lo - P:hi - P]).any(dim=1)
        if bool(bad.any()):
            return lo + int(bad.nonzero()[0])
    return None


def expect_periodic(touts, names, what, n=None):
    for k in names:
        s = first_aperiodic(touts[k], n)
        assert s is None, "%s: %s of sample %d differs from sample %d (the same pattern %d)" % (what, k, s, s - P, s % P)


def host(touts, names, sl):
    return {k: touts[k][sl].cpu().numpy() for k in names}


def need_memory(nbytes):
    """Part B: skips only when the device has less than twice the test's own tensors free"""
    import torch
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < 2 * nbytes:
        pytest.skip("needs 2 x %d bytes of device memory, %d are free" % (nbytes, free))


def planned_bytes(case, n):
    total = sum(int(np.prod(v.shape[1:])) * v.dtype.itemsize * n for v in case.inputs.values())
    total += sum(int(np.prod(shape)) * np.dtype(dt).itemsize for shape, dt in case.outputs(n).values())
    return total


def run_given(ofdg, case, n=N, ends=False, after=None):
    """One call with the repeating given records (where the operation has records) into guarded destinations: guards, the
    periodic comparison, the first 16 (ends: and the last 16) against twin and restatement, the inputs as they were."""
    import torch
    what = "%s %dx%d n %d" % (case.name, case.W, case.H, n)
    bufs = Bufs()
    try:
        g = make_gen(ofdg, case)
        tin = {k: bufs.repeated(v, n) for k, v in case.inputs.items()}
        trecs = None if case.recs is None else bufs.repeated(case.recs, n)
        touts = {k: bufs.empty(shape, dt) for k, (shape, dt) in case.outputs(n).items()}
        for k, src in case.in_place.items():
            touts[k] = tin[src]
        names = [k for k in touts if k != "work"]
        tail = np.arange(n - P, n)
        tail_in = {k: tin[k][n - P:].cpu().numpy() for k in tin} if ends else None
        if ends:  # (the fill itself, at the far end)
            bc.expect_same(tail_in, case.take(tail % P)[0], what + ": the last 16 sources")
        torch.cuda.synchronize()
        case.run(ofdg, g, tin, trecs, touts)
        g.synchronize()
        torch.cuda.synchronize()
        assert bufs.intact(), what + ": guard bytes"
        expect_periodic(touts, names, what)
        for k in tin:
            if k not in case.in_place.values():
                assert first_aperiodic(tin[k]) is None, what + ": source %s was written" % k
        if trecs is not None:
            assert first_aperiodic(trecs) is None and bc.bytes_equal(trecs[:P].cpu().numpy(), case.recs), what + ": given records were written"
        got = host(touts, names, slice(0, P))
        bc.expect_same(got, case.twin(ofdg, case.inputs, case.recs), what + ": first 16 against the host twin")
        bc.expect_same(got, case.restate(case.inputs, case.recs), what + ": first 16 against the restatement")
        if ends:
            inputs, recs = case.take(tail % P)
            bc.expect_same(host(touts, names, slice(n - P, n)), case.twin(ofdg, tail_in, recs), what + ": last 16 against the host twin")
        if after is not None:
            after(g, tin, trecs, touts, what)
        return bufs.bytes()
    finally:
        bufs.free()


def run_drawn(ofdg, case, n=N):
    """One call with drawn records (seed, first_index near 2^40), recs_out requested: recs_out and the frames of six samples
    against the twin run on that sample alone with first_index + s, n = 1."""
    import torch
    what = "%s drawn, %dx%d n %d" % (case.name, case.W, case.H, n)
    bufs = Bufs()
    try:
        g = make_gen(ofdg, case)
        tin = {k: bufs.repeated(v, n) for k, v in case.inputs.items()}
        touts = {k: bufs.empty(shape, dt) for k, (shape, dt) in case.outputs(n).items()}
        for k, src in case.in_place.items():
            touts[k] = tin[src]
        names = [k for k in touts if k != "work"]
        torch.cuda.synchronize()
        case.run(ofdg, g, tin, None, touts, first_index=bc.FIRST_INDEX)
        g.synchronize()
        torch.cuda.synchronize()
        assert bufs.intact(), what + ": guard bytes"
        for k in tin:
            if k not in case.in_place.values():
                assert first_aperiodic(tin[k]) is None, what + ": source %s was written" % k
        seen = set()
        for s in bc.DRAWN_AT:
            one = {k: v[s % P:s % P + 1] for k, v in case.inputs.items()}
            want = case.twin(ofdg, one, first_index=bc.FIRST_INDEX + s)
            bc.expect_same(host(touts, names, slice(s, s + 1)), want, what + ": sample %d against the twin at first_index + %d" % (s, s))
            seen.add(want["recs_out"].tobytes())
        assert len(seen) > 1, what + ": the six drawn records are all the same"
    finally:
        bufs.free()


RECORD_OPS = sorted(bc.RECORD_CASES)
PACK_MODES = [(layout, concat, rgb) for layout in (0, 1) for concat in (False, True) for rgb in (False, True)]  # PACK_NCHW, PACK_NHWC


def rows_doubled(case, names, add):
    """after=: a second call with accumulate=True into the same per-sample rows - every row read, added to and written back on
    the workgroup's second trip too: still periodic, the first 16 what `add` makes of the twin's rows reduced twice"""
    def after(g, tin, trecs, touts, what):
        import torch
        import importlib
        ofdg = importlib.import_module("optical-flow-2d-data-generation_amd")
        case.run(ofdg, g, tin, trecs, touts, accumulate=True)
        g.synchronize()
        torch.cuda.synchronize()
        s = first_aperiodic(touts["rows"])
        assert s is None, "%s, accumulated: the row of sample %d differs from that of sample %d" % (what, s, s - P)
        twin = case.twin(ofdg, case.inputs, case.recs)
        rows = twin["rows"].view(case.ref.ROW_DTYPE).reshape(P, 2)
        want = add(rows, rows)
        assert touts["rows"][:P].cpu().numpy().tobytes() == want.tobytes(), what + ", accumulated: first 16 rows"
        bc.expect_same(host(touts, [k for k in names if k != "rows"], slice(0, P)), {k: twin[k] for k in names if k != "rows"}, what + ", accumulated: planes")
    return after


# ---- part A: the second trip of every sample loop ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", RECORD_OPS)
def test_second_trip_given_records(ofdg, name):
    """photo_kernel, jitter_mean_kernel + jitter_apply_kernel, camera_kernel, jpeg_kernel, mblur_kernel: 16x16 uint8 frames
    (binary16 flow), both frames, recs_out requested, everything between guards."""
    run_given(ofdg, bc.case(name))


@pytest.mark.parametrize("name", RECORD_OPS)
def test_second_trip_drawn_records(ofdg, name):
    run_drawn(ofdg, bc.case(name))


@pytest.mark.parametrize("name", [n for n in RECORD_OPS if bc.RECORD_CASES[n].can_in_place])
def test_second_trip_in_place(ofdg, name):
    run_given(ofdg, bc.case(name, in_place=True))


def test_second_trip_flow_pyramid(ofdg):
    """flow_pyramid_kernel (gridDim.z): levels 1..4 of 16x16 binary16 flows with their weights"""
    run_given(ofdg, bc.case("flow_pyramid"))


def test_second_trip_reproject(ofdg):
    """reproject_kernel: both frames of 16x16 uint8 images through binary16 flows, every plane and the per-sample rows; then
    OFDG_REPROJ_ACCUMULATE on top (the operation has no single-row mode: the sums are per sample, and every one of the 65551
    rows must be twice its pattern's - the periodic comparison and the first 16 against reproject_reference.add_rows)"""
    case = bc.case("reproject")
    run_given(ofdg, case, after=rows_doubled(case, list(case.outputs(1)), case.ref.add_rows))


def test_second_trip_splat(ofdg):
    """splat_scatter_kernel, splat_resolve_kernel and the clearing of the key planes: given records, every plane, keys, rows
    and recs_out; then OFDG_SPLAT_ACCUMULATE on top"""
    case = bc.case("splat")
    run_given(ofdg, case, after=rows_doubled(case, list(case.outputs(1)), case.ref.add_rows))


def test_second_trip_splat_drawn(ofdg):
    run_drawn(ofdg, bc.case("splat"))


@pytest.mark.parametrize("fill", [0, 1], ids=["mean", "colour"])  # ERASE_MEAN, ERASE_CONST
def test_second_trip_erase(ofdg, fill):
    """erase_mean_kernel (fill = mean only) and erase_apply_kernel, in place on both frames and both maps, work[i]"""
    run_given(ofdg, bc.case("erase", fill=fill))


def test_second_trip_erase_drawn(ofdg):
    run_drawn(ofdg, bc.case("erase", fill=1))


@pytest.mark.parametrize("layout,concat,rgb", PACK_MODES)
def test_second_trip_pack(ofdg, layout, concat, rgb):
    """pack_kernel: every layout mode of the operation's own grid, uint8 frames and binary16 flow to binary16"""
    run_given(ofdg, bc.case("pack", layout=layout, concat=concat, rgb=rgb))


@pytest.mark.parametrize("labels,radius,min_step", [(True, 4, 0.0), (False, 15, 0.5), (True, 1, 3.0)])
def test_second_trip_boundaries(ofdg, labels, radius, min_step):
    """boundary_kernel: both frames, with and without labels, the radii and steps of the operation's own grid"""
    run_given(ofdg, bc.case("boundaries", labels=labels, radius=radius, min_step=min_step))


@pytest.mark.parametrize("norm,layout", [("sample", "planar_bgr"), ("fixed", "hwc_rgb"), ("sample", "hwc_rgb")])
def test_second_trip_flow_vis(ofdg, norm, layout):
    """flow_vis_max_kernel (not under "fixed") and flow_vis_colour_kernel, the clearing of the work words"""
    run_given(ofdg, bc.case("flow_vis", norm=norm, layout=layout))


def test_second_trip_flow_vis_batch(ofdg):
    """norm "batch": the longest vector of the call stands in the last sample alone (the 17th pattern), so every sample's scale
    comes from a maximum that only sample 65550 extends"""
    import torch
    case = bc.case("flow_vis", norm="batch")
    n, what = N, "flow_vis batch n %d" % N
    bufs = Bufs()
    try:
        g = make_gen(ofdg, case)
        tin = {k: bufs.repeated(v, n, case.last[k]) for k, v in case.inputs.items()}
        touts = {k: bufs.empty(shape, dt) for k, (shape, dt) in case.outputs(n).items()}
        torch.cuda.synchronize()
        case.run(ofdg, g, tin, None, touts)
        g.synchronize()
        torch.cuda.synchronize()
        assert bufs.intact(), what + ": guard bytes"
        expect_periodic(touts, ["picture", "rows"], what, n - 1)
        inputs = {k: np.concatenate([case.inputs[k], case.last[k]]) for k in case.inputs}
        got = {k: torch.cat([touts[k][:P], touts[k][n - 1:]]).cpu().numpy() for k in ("picture", "rows")}
        bc.expect_same(got, case.twin(ofdg, inputs), what + ": first 16 and the last against the twin")
        bc.expect_same(got, case.restate(inputs), what + ": first 16 and the last against the restatement")
        top = case.ref.flow_vis(case.last["flow"], None, "sample")[1]["max_r2_q16"][0]
        assert top > case.ref.flow_vis(case.inputs["flow"], None, "sample")[1]["max_r2_q16"].max()
        assert got["rows"].view(case.ref.ROW)["max_r2_q16"].tolist() == [[top]] * (P + 1)
    finally:
        bufs.free()


def check_flow_error(ofdg, case, n=N, ends=False):
    """Per-sample rows, epe and picture: run_given.  Then OFDG_ERR_ONE_ROW: every count and sum of the 16 patterns
    floor((n - 1) / 16) times, the remainder patterns once, the extreme sample once, in Python integers; the key is the extreme
    sample's with its pixel index moved to sample n - 1; then ACCUMULATE | ONE_ROW on top: the sums twice, the key the same."""
    import torch
    fe = case.ref
    used = run_given(ofdg, case, n, ends)
    what = "flow_error %dx%d n %d ONE_ROW" % (case.W, case.H, n)
    bufs = Bufs()
    try:
        g = make_gen(ofdg, case)
        tin = {k: bufs.repeated(v, n, case.last[k]) for k, v in case.inputs.items()}
        one = bufs.empty((1, 672), np.uint8)
        per = bc.int_rows(case.twin(ofdg, case.inputs)["rows"].view(fe.ROW))
        last = bc.int_rows(case.twin(ofdg, case.last)["rows"].view(fe.ROW))[0]
        assert last[("max_key",)] >> 32 > max(r[("max_key",)] >> 32 for r in per), "the extreme must be the last sample's alone"
        want = bc.summed(per, n, last, maxima=("max_key",))
        want[("max_key",)] = last[("max_key",)] - (n - 1) * case.H * case.W
        for accumulate in (False, True):
            torch.cuda.synchronize()
            case.run(ofdg, g, tin, None, dict(rows=one), one_row=True, accumulate=accumulate)
            g.synchronize()
            torch.cuda.synchronize()
            got = bc.int_rows(one.cpu().numpy().view(fe.ROW))[0]
            expect = {k: v if k == ("max_key",) else (2 * v if accumulate else v) for k, v in want.items()}
            bad = [k for k in expect if got[k] != expect[k]]
            assert not bad, "%s accumulate %s: %s: got %s, expected %s" % (what, accumulate, bad[0], got[bad[0]], expect[bad[0]])
        assert bufs.intact(), what + ": guard bytes"
        return max(used, bufs.bytes())
    finally:
        bufs.free()


def test_second_trip_flow_error(ofdg):
    """flow_error_kernel: 16x16 binary16 ground truth and estimate, uint8 map and dist2 plane"""
    check_flow_error(ofdg, bc.case("flow_error"))


def stats_call(ofdg, g, case, tin, rows, flags):
    fsr = case.ref
    g.flow_stats(tin["flow"], rows, occ=tin["occ"], bin_px=case.BIN_PX, accumulate=bool(flags & fsr.ACCUMULATE),
                 visible_only=bool(flags & fsr.VISIBLE_ONLY), one_row=bool(flags & fsr.ONE_ROW), size=(case.H, case.W))
    g.synchronize()


def check_flow_stats(ofdg, case, n=N, ends=False):
    """Per-sample rows (plain and VISIBLE_ONLY): periodic, the first 16 (ends: and the last 16) the twin's and the
    restatement's.  ONE_ROW: the sums of the 16 patterns floor((n - 1) / 16) times, the remainder patterns once and the last
    sample - the 17th pattern, which alone holds the longest vector - once; then ACCUMULATE | ONE_ROW on top of it."""
    import torch
    fsr = case.ref
    what = "flow_stats %dx%d n %d" % (case.W, case.H, n)
    bufs = Bufs()
    try:
        g = make_gen(ofdg, case)
        tin = {k: bufs.repeated(v, n, case.last[k]) for k, v in case.inputs.items()}
        torch.cuda.synchronize()
        per = {}
        for flags in (0, fsr.VISIBLE_ONLY):
            rows = bufs.empty((n, 304), np.uint8)
            stats_call(ofdg, g, case, tin, rows, flags)
            torch.cuda.synchronize()
            s = first_aperiodic(rows, n - 1)
            assert s is None, "%s flags %d: the row of sample %d differs from that of sample %d (pattern %d)" % (what, flags, s, s - P, s % P)
            got = case.structured(ofdg, rows[:P])
            twin = case.twin_rows(ofdg, case.inputs, flags)
            assert got.tobytes() == twin.tobytes(), what + " flags %d: first 16 against ofdg_host_flow_stats" % flags
            fsr.expect_equal(got, case.restate_rows(case.inputs, flags), what + " flags %d: first 16 against the restatement" % flags)
            last = case.structured(ofdg, rows[n - 1:])
            assert last.tobytes() == case.twin_rows(ofdg, case.last, flags).tobytes(), what + " flags %d: the last sample" % flags
            if ends:
                tail = np.arange(n - 1 - P, n - 1)
                inputs = {k: tin[k][n - 1 - P:n - 1].cpu().numpy() for k in tin}
                bc.expect_same(inputs, case.take(tail % P)[0], what + ": the last 16 periodic sources")
                assert case.structured(ofdg, rows[n - 1 - P:n - 1]).tobytes() == case.twin_rows(ofdg, inputs, flags).tobytes(), \
                    what + " flags %d: the last 16 periodic rows against the twin" % flags
            stats_call(ofdg, g, case, tin, rows, flags | fsr.ACCUMULATE)   # each row read, added to and written back, on both trips
            torch.cuda.synchronize()
            s = first_aperiodic(rows, n - 1)
            assert s is None, "%s flags %d, accumulated: the row of sample %d differs from that of sample %d" % (what, flags, s, s - P)
            twice = case.twin_rows(ofdg, case.inputs, flags | fsr.ACCUMULATE, rows=twin.copy())
            assert case.structured(ofdg, rows[:P]).tobytes() == twice.tobytes(), what + " flags %d: per-sample ACCUMULATE, first 16" % flags
            assert [r["n_counted"] for r in fsr.rows_of(twice)] == [2 * r["n_counted"] for r in fsr.rows_of(twin)]
            per[flags] = (twin, case.twin_rows(ofdg, case.last, flags))
            one = bufs.empty((1, 304), np.uint8)
            stats_call(ofdg, g, case, tin, one, flags | fsr.ONE_ROW)
            torch.cuda.synchronize()
            want = case.expected_one_row(*per[flags], n)
            fsr.expect_equal(case.structured(ofdg, one), [want], what + " flags %d: ONE_ROW" % (flags | fsr.ONE_ROW))
            assert 0xFFFFFFFF - (want["max_key"] & 0xFFFFFFFF) >= (n - 1) * case.H * case.W  # (the extreme is the last sample's)
            stats_call(ofdg, g, case, tin, one, flags | fsr.ONE_ROW | fsr.ACCUMULATE)
            torch.cuda.synchronize()
            twice = {f: ([2 * h for h in want[f]] if f == "hist" else want[f] if f == "max_key" else 2 * want[f]) for f in fsr.FIELDS}
            fsr.expect_equal(case.structured(ofdg, one), [twice], what + " flags %d: ACCUMULATE | ONE_ROW" % flags)
        assert bufs.intact(), what + ": guard bytes"
        return bufs.bytes()
    finally:
        bufs.free()


def test_second_trip_flow_stats(ofdg):
    """flow_stats_kernel: 16x16 binary16 flows with uint8 maps"""
    check_flow_stats(ofdg, bc.case("flow_stats"))


# ---- part B: sample offsets past 2^32 bytes -----------------------------------------------------------------------------------
def wide_case(name):
    cls = bc.RECORD_CASES.get(name)
    return bc.case(name, wide=True, in_place=True) if cls is not None and cls.can_in_place else bc.case(name, wide=True)


@pytest.mark.parametrize("name", RECORD_OPS)
def test_past_4gib_frames(ofdg, name):
    """float32 frames of 96x64 (float32 flow), frame 1 alone, in place where the operation has that form: the last sample starts
    beyond byte 2^32 of every frame tensor."""
    case = wide_case(name)
    assert 3 * case.W * case.H * 4 * (N - 1) >= 2 ** 32
    need_memory(planned_bytes(case, N))
    used = run_given(ofdg, case, ends=True)
    print("peak bytes of the test's tensors: %d" % used)


def test_past_4gib_flow_pyramid(ofdg):
    case = bc.case("flow_pyramid", wide=True)
    assert 2 * case.W * case.H * 4 * (N - 1) >= 2 ** 32
    need_memory(planned_bytes(case, N))
    print("peak bytes of the test's tensors: %d" % run_given(ofdg, case, ends=True))


def test_past_4gib_reproject(ofdg):
    """frame 1 alone (it reads both frames and both flows), float32 at 96x64"""
    case = bc.case("reproject", wide=True)
    assert 3 * case.W * case.H * 4 * (N - 1) >= 2 ** 32
    need_memory(planned_bytes(case, N))
    print("peak bytes of the test's tensors: %d" % run_given(ofdg, case, ends=True))


@pytest.mark.parametrize("name", ["splat", "erase", "pack", "boundaries", "flow_vis"])
def test_past_4gib_more(ofdg, name):
    """float32 planes, frame 1 alone where the operation has frames; erase in place"""
    case = bc.case(name, wide=True)
    assert case.channels * case.W * case.H * 4 * (N - 1) >= 2 ** 32
    need_memory(planned_bytes(case, N))
    print("peak bytes of the test's tensors: %d" % run_given(ofdg, case, ends=True))


def test_past_4gib_flow_error(ofdg):
    case = bc.case("flow_error", wide=True)
    assert 2 * case.W * case.H * 4 * (N - 1) >= 2 ** 32
    need_memory(planned_bytes(case, N))
    print("peak bytes of the test's tensors: %d" % check_flow_error(ofdg, case, ends=True))


def test_past_4gib_flow_stats(ofdg):
    case = bc.case("flow_stats", wide=True)
    assert 2 * case.W * case.H * 4 * (N - 1) >= 2 ** 32
    need_memory(planned_bytes(case, N) + 2 * N * 304)
    print("peak bytes of the test's tensors: %d" % check_flow_stats(ofdg, case, ends=True))
