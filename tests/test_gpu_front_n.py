"""Groups of three and four batches per front end on the counter-sampler path (ofdg_set_front_batches, include/ofdg.h): a
chain's sampler -> geom -> raster launches serve the call's batch (part 0) AND the N - 1 batches that chain is asked for next;
those calls launch only their background preparation and compose.  It is a scheduling choice, so every test here compares
BYTES with a context on the same inputs that launches a front end per call (set_front_batches(1)): consecutive calls over every
part of a whole N-group and the first call of the group behind it, the optional outputs and the compact formats, the events
that make a chain forget the rest of a group (a jump of the first index, another batch size, set_step, a new pool,
set_front_batches), a sharded sequence and a caller's stream.  The batch served from the LAST part of a group is also held
against the oracle at the suite's 0 LSB / <= 1 ULP.

The first group a chain launches after a start may be shorter than N (kFrontFirstGroup, csrc/ofdg_device.h), so the tests do
not count calls to know where a group begins: they read Generator.front_pending(), the number of batches the chains hold ready
for calls that have not come yet.

Shapes as in test_gpu_paired_front.py: 128 x 96 (`_pow2` kernels) and 192 x 128 (general kernels) on a pool of 8 synthetic
512 x 384 images, 3 samples (2 where the batch size changes), 4 objects.  The front = 1 reference of a (size, mode,
preparation) is computed once and shared by N = 3 and N = 4.

Error words: as in test_gpu_paired_front.py no legitimate input raises a capacity flag at these sizes; what is checked is that
every batch of a grouped sequence has a ticket of its own and that each ticket's word reads clean."""
import numpy as np
import pytest

from test_gpu_bench_parity import check_samples

pytestmark = pytest.mark.gpu

POOL = (8, 512, 384)
B, NOBJ, SEED = 3, 4, 5
SIZES = [(128, 96), (192, 128)]
FRONTS = [3, 4]
ALL = ("flow1", "occ0", "occ1", "label0", "label1")
MAX_GROUPS = 2   # a short first group and a whole one: the most calls a test makes is (MAX_GROUPS x 4) x chains + 1


def make(ofdg, W, H, mode, prep, front, **kw):
    prm = ofdg.default_params(width=W, height=H, mode=mode, num_objects=NOBJ, batch_size=B, sampler=1, seed=SEED,
                              background_prep=prep, **kw)
    g = ofdg.Generator(prm)
    g.pool_synthetic(*POOL, 3)
    if mode == 9:
        g.warp_generate(1, 7)
    g.set_front_batches(front)
    assert g.info().endswith(" front=%d" % front)
    return g, prm


def outputs(ofdg, n, H, W, fmt=None, extras=None):
    import torch
    if fmt:
        outs = ofdg.alloc_outputs(n, H, W, image_dtype=torch.uint8, flow_dtype=torch.float16)
        ex = ofdg.alloc_extras(n, H, W, extras, flow_dtype=torch.float16, occ_dtype=torch.uint8) if extras else None
    else:
        outs = ofdg.alloc_outputs(n, H, W)
        ex = ofdg.alloc_extras(n, H, W, extras) if extras else None
    torch.cuda.synchronize()   # (the buffers are zeroed on torch's stream, the calls write them on others)
    return outs, ex


def forward_one(ofdg, g, H, W, stream=None, fmt=None, extras=None):
    outs, ex = outputs(ofdg, B, H, W, fmt, extras)
    g.forward(*outs, ofdg.STREAM_OWN if stream is None else stream, extras=ex)
    return outs, ex


def forwards(ofdg, g, n_calls, H, W, stream=None, fmt=None, extras=None):
    """n_calls x forward(), every call into buffers of its own; [(outputs, extras)] after everything has finished"""
    res = [forward_one(ofdg, g, H, W, stream, fmt, extras) for _ in range(n_calls)]
    g.synchronize(0 if stream is None else stream)
    return res


def whole_group(ofdg, g, front, H, W, **kw):
    """forward() from a fresh context until every part of a whole `front`-group of every chain and the first call of the group
    behind it have been served; (results, index of the first call that was served from the LAST part of a whole group)"""
    nc = g.num_chains()
    res = [forward_one(ofdg, g, H, W, **kw)]
    first = g.front_pending() + 1          # the size of the first group
    assert 1 <= first <= front
    lead = 0 if first == front else first * nc   # calls the shorter first groups serve
    assert lead + front * nc + 1 <= MAX_GROUPS * 4 * nc + 1
    pending = [g.front_pending()]
    while len(res) < lead + front * nc + 1:
        res.append(forward_one(ofdg, g, H, W, **kw))
        pending.append(g.front_pending())
    g.synchronize(0 if kw.get("stream") is None else kw["stream"])
    # the whole groups really were whole: after their part 0 calls every chain holds front - 1 parts, after the last parts none
    assert pending[lead + nc - 1] == (front - 1) * nc
    assert pending[lead + front * nc - 1] == 0
    assert pending[lead + front * nc] == front - 1
    return res, lead + (front - 1) * nc


def to_host(res):
    return [(tuple(t.cpu() for t in o), {k: v.cpu() for k, v in e.items()} if e else None) for o, e in res]


_reference = {}


def reference(ofdg, W, H, mode, prep, n_calls, fmt=None, extras=None, **kw):
    """the first n_calls outputs of a front = 1 context, on the host; computed once per configuration and left unchanged"""
    key = (W, H, mode, prep, fmt, extras, tuple(sorted(kw.items())))
    if key not in _reference:
        g1, _ = make(ofdg, W, H, mode, prep, 1, **kw)
        nc = g1.num_chains()
        _reference[key] = to_host(forwards(ofdg, g1, MAX_GROUPS * 4 * nc + 1, H, W, fmt=fmt, extras=extras))
        assert g1.front_pending() == 0
        g1.close()
    assert n_calls <= len(_reference[key])
    return _reference[key][:n_calls]


def assert_same(got, want):
    import torch
    assert len(got) == len(want)
    for k, ((o2, e2), (o1, e1)) in enumerate(zip(got, want)):
        for name, a, b in zip(("image0", "image1", "flow"), o2, o1):
            assert a.dtype == b.dtype and torch.equal(a.cpu().view(torch.uint8), b.cpu().view(torch.uint8)), "call %d: %s" % (k, name)
        for name in (e1 or {}):
            assert torch.equal(e2[name].cpu().view(torch.uint8), e1[name].cpu().view(torch.uint8)), "call %d: %s" % (k, name)


@pytest.mark.parametrize("front", FRONTS)
@pytest.mark.parametrize("prep", [0, 1])
@pytest.mark.parametrize("mode", [5, 7, 9])
@pytest.mark.parametrize("W,H", SIZES)
def test_consecutive_calls(ofdg, oracle, W, H, mode, prep, front):
    """Every part of a whole N-group of every chain and the first call of the next group (at least N x chains + 1 calls; a
    shorter first group comes on top): every output of every call is the ungrouped context's, and the first batch that was
    served from the last part of a group is the oracle's."""
    g, prm = make(ofdg, W, H, mode, prep, front)
    got, last = whole_group(ofdg, g, front, H, W)
    assert len(got) >= front * g.num_chains() + 1
    assert_same(got, reference(ofdg, W, H, mode, prep, len(got)))
    tasks, bps, n = g.sample_counter(last * B, B)
    crops = np.stack([g.warp_download(i) for i in range(g.warp_count())]) if mode == 9 else None
    check_samples(ofdg, oracle, g, prm, tasks, bps, n, got[last][0], range(B), POOL[0], crops)
    g.close()


@pytest.mark.parametrize("front", FRONTS)
@pytest.mark.parametrize("compact", [False, True])
def test_optional_outputs_and_compact_formats(ofdg, front, compact):
    """The same sequence with backward flow, labels and occlusion maps (rigid mode 7), float32 and in the compact formats (uint8
    frames, binary16 flows, uint8 maps): the occlusion pass behind compose works on every part of the slot."""
    W, H = SIZES[1]
    g, _ = make(ofdg, W, H, 7, 1, front)
    got, _ = whole_group(ofdg, g, front, H, W, fmt=compact, extras=ALL)
    assert_same(got, reference(ofdg, W, H, 7, 1, len(got), fmt=compact, extras=ALL))
    g.close()


def until_after_part_1(ofdg, g, H, W):
    """forward() until every chain has served part 1 of a 4-group and holds parts 2 and 3; the results"""
    nc = g.num_chains()
    res = []
    for _ in range(MAX_GROUPS * 4 * nc):
        res.append(forward_one(ofdg, g, H, W))
        if len(res) % nc == 0 and g.front_pending() == 2 * nc:
            return res
    raise AssertionError("no chain ever held parts 2 and 3 of a group of four: front_pending() = %d" % g.front_pending())


def event_jump(ofdg, g, H, W, n_before):
    res = []
    for first in (1000, 1003, (n_before + 2) * B, (n_before + 3) * B, 1006, 1009):   # (a jump, its sequence, back and away again)
        outs, _ = outputs(ofdg, B, H, W)
        g.forward_counter(first, B, *outs, ofdg.STREAM_OWN)
        res.append((outs, None))
    return res


def event_batch_size(ofdg, g, H, W, n_before):
    res, first = [], n_before * B
    for n in (2, 2, 2, 2, 3, 3, 2, 3):
        outs, _ = outputs(ofdg, n, H, W)
        g.forward_counter(first, n, *outs, ofdg.STREAM_OWN)
        res.append((outs, None))
        first += n
    return res


def event_set_step(ofdg, g, H, W, n_before):
    waiting = g.front_pending()
    g.step = g.step          # (the same step: nothing changes, nothing is forgotten)
    assert g.front_pending() == waiting
    g.step = 50
    return [forward_one(ofdg, g, H, W) for _ in range(g.num_chains() + 1)]


def event_pool(ofdg, g, H, W, n_before):
    g.pool_synthetic(*POOL, 9)   # (the remaining parts were sampled for the old pool's textures)
    return [forward_one(ofdg, g, H, W) for _ in range(g.num_chains() + 1)]


def event_set_front_batches(ofdg, g, H, W, n_before):
    if g.info().endswith(" front=4"):
        g.set_front_batches(3)
    return [forward_one(ofdg, g, H, W) for _ in range(3 * g.num_chains() + 1)]


@pytest.mark.parametrize("event", [event_jump, event_batch_size, event_set_step, event_pool, event_set_front_batches],
                         ids=lambda f: f.__name__)
@pytest.mark.parametrize("W,H", SIZES)
def test_events_that_forget_the_rest_of_a_group(ofdg, W, H, event):
    """After part 1 of a group of four on every chain (parts 2 and 3 wait): the event forgets them - at once where the event is
    a setter, at the chain's next call where it is a call for something else -, the outputs are the ungrouped context's, and
    synchronize finds no error left behind by the parts nobody came for."""
    g4, _ = make(ofdg, W, H, 5, 1, 4)
    g1, _ = make(ofdg, W, H, 5, 1, 1)
    nc = g4.num_chains()
    got = until_after_part_1(ofdg, g4, H, W)
    want = [forward_one(ofdg, g1, H, W) for _ in range(len(got))]
    assert g4.front_pending() == 2 * nc
    got += event(ofdg, g4, H, W, len(want))
    want += event(ofdg, g1, H, W, len(want))
    assert g1.front_pending() == 0
    g4.synchronize()   # (raises on a flag left in any word)
    g1.synchronize()
    assert_same(got, want)
    g4.close()
    g1.close()


@pytest.mark.parametrize("event", ["set_step", "pool", "set_front_batches"])
def test_setters_forget_at_once(ofdg, event):
    """ofdg_set_step to another step, a pool change and ofdg_set_front_batches leave no part waiting on any chain."""
    W, H = SIZES[0]
    g, _ = make(ofdg, W, H, 5, 1, 4)
    until_after_part_1(ofdg, g, H, W)
    assert g.front_pending() == 2 * g.num_chains()
    if event == "set_step":
        g.step = 50
    elif event == "pool":
        g.pool_synthetic(*POOL, 9)
    else:
        g.set_front_batches(4)
    assert g.front_pending() == 0
    g.synchronize()
    g.close()


@pytest.mark.parametrize("front", FRONTS)
def test_sharded_sequence(ofdg, front):
    """rank 1 of 2 (one process, no communicator): the sequence's stride is 2 x batch, which is what the later parts are sampled
    for."""
    W, H = SIZES[0]
    g, _ = make(ofdg, W, H, 7, 1, front, rank=1, world_size=2)
    got, _ = whole_group(ofdg, g, front, H, W)
    assert_same(got, reference(ofdg, W, H, 7, 1, len(got), rank=1, world_size=2))
    assert g.step == len(got)
    g.close()


@pytest.mark.parametrize("front", FRONTS)
@pytest.mark.parametrize("prep", [0, 1])
def test_callers_stream_and_tickets(ofdg, prep, front):
    """The calls on a stream that is not the context's own: compose runs there behind the hand-over event, which every part
    records behind ITS preparation.  Every batch has a ticket of its own, and each ticket's error word reads clean."""
    import torch
    W, H = SIZES[1]
    g, _ = make(ofdg, W, H, 5, prep, front)
    nc = g.num_chains()
    s = torch.cuda.Stream()
    got, tickets = [], []
    for _ in range(2 * front * nc + 1):   # (a shorter first group and a whole one at the least)
        got.append(forward_one(ofdg, g, H, W, stream=s.cuda_stream))
        tickets.append(g.last_ticket())
    g.synchronize(s.cuda_stream)
    assert_same(got, reference(ofdg, W, H, 5, prep, len(got)))
    assert len(set(tickets)) == len(tickets)
    for t in tickets:
        g.poll_errors_of(t)   # (raises unless clean)
    g.synchronize()
    g.close()
