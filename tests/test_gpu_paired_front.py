"""The paired front end of the counter-sampler path (ofdg_set_front_batches, include/ofdg.h): a chain's sampler -> geom ->
raster launches serve the call's batch AND the batch that chain is asked for next; that call launches only its background
preparation and compose.  It is a scheduling choice, so every test here compares BYTES with a second context on the same
inputs that launches a front end per call (set_front_batches(1)): consecutive calls (first halves, second halves and a second
round of pairs), the optional outputs and the compact formats, calls the prediction does not cover (a jump of the first index,
another batch size, set_step, a new pool), a sharded sequence and a caller's stream.  One batch served from a second half is
also held against the oracle at the suite's 0 LSB / <= 1 ULP.

Shapes: the smallest at which both compose kernels run - 128 x 96 (`_pow2`) and 192 x 128 (general) - on a pool of 8 synthetic
512 x 384 images (at least 2W x 2H: the one-launch form of the preparation with its tile loop), 3 samples, 4 objects.

Error words: no legitimate input of the counter sampler raises a capacity flag at these sizes (the outline slots are sized for
the worst case, a curve never needs more than its 96 points at these scales, the zoom is drawn from 0.8 .. 1.2 and the
preparation refuses below 0.75), so a flag of a second half alone cannot be built without forged records; what is checked is
that every batch of a paired sequence has a ticket of its own and that each ticket's word reads clean."""
import numpy as np
import pytest

from test_gpu_bench_parity import check_samples

pytestmark = pytest.mark.gpu

POOL = (8, 512, 384)
B, NOBJ, SEED = 3, 4, 5
SIZES = [(128, 96), (192, 128)]
ALL = ("flow1", "occ0", "occ1", "label0", "label1")


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


def both(ofdg, W, H, mode, prep, **kw):
    (g2, prm), (g1, _) = make(ofdg, W, H, mode, prep, 2, **kw), make(ofdg, W, H, mode, prep, 1, **kw)
    return g2, g1, prm


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


def forwards(ofdg, g, n_calls, H, W, stream=None, fmt=None, extras=None):
    """n_calls x forward(), every call into buffers of its own; [(outputs, extras)] after everything has finished"""
    stream = ofdg.STREAM_OWN if stream is None else stream
    res = []
    for _ in range(n_calls):
        outs, ex = outputs(ofdg, B, H, W, fmt, extras)
        g.forward(*outs, stream, extras=ex)
        res.append((outs, ex))
    g.synchronize(0 if stream == ofdg.STREAM_OWN else stream)
    return res


def assert_same(got, want):
    import torch
    assert len(got) == len(want)
    for k, ((o2, e2), (o1, e1)) in enumerate(zip(got, want)):
        for name, a, b in zip(("image0", "image1", "flow"), o2, o1):
            assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "call %d: %s" % (k, name)
        for name in (e1 or {}):
            assert torch.equal(e2[name].view(torch.uint8), e1[name].view(torch.uint8)), "call %d: %s" % (k, name)


@pytest.mark.parametrize("prep", [0, 1])
@pytest.mark.parametrize("mode", [5, 7, 9])
@pytest.mark.parametrize("W,H", SIZES)
def test_consecutive_calls(ofdg, oracle, W, H, mode, prep):
    """2 x chains + 1 forward calls on the context's own streams: every chain's first half, its second half and the first half
    of its next pair.  Every output of every call is the unpaired context's; the first batch that was served from a second half
    (call number `chains`) is the oracle's."""
    g2, g1, prm = both(ofdg, W, H, mode, prep)
    nc = g2.num_chains()
    assert g1.num_chains() == nc
    got = forwards(ofdg, g2, 2 * nc + 1, H, W)
    want = forwards(ofdg, g1, 2 * nc + 1, H, W)
    assert_same(got, want)
    first = nc * B
    tasks, bps, n = g2.sample_counter(first, B)
    crops = np.stack([g2.warp_download(i) for i in range(g2.warp_count())]) if mode == 9 else None
    check_samples(ofdg, oracle, g2, prm, tasks, bps, n, got[nc][0], range(B), POOL[0], crops)
    g2.close()
    g1.close()


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("W,H", SIZES)
def test_optional_outputs_and_compact_formats(ofdg, W, H, compact):
    """The same sequence with backward flow, labels and occlusion maps (rigid mode 7), float32 and in the compact formats (uint8
    frames, binary16 flows, uint8 maps): the occlusion pass behind compose works on the half slot too."""
    g2, g1, _ = both(ofdg, W, H, 7, 1)
    nc = g2.num_chains()
    got = forwards(ofdg, g2, 2 * nc + 1, H, W, fmt=compact, extras=ALL)
    want = forwards(ofdg, g1, 2 * nc + 1, H, W, fmt=compact, extras=ALL)
    assert_same(got, want)
    g2.close()
    g1.close()


def script_jump(ofdg, g, H, W):
    res = []
    for first in (0, 3, 1000, 9, 12, 1003, 18, 21):   # (hits and misses of the prediction on three and on four chains)
        outs, _ = outputs(ofdg, B, H, W)
        g.forward_counter(first, B, *outs, ofdg.STREAM_OWN)
        res.append((outs, None))
    return res


def script_batch_size(ofdg, g, H, W):
    res, first = [], 0
    for n in (3, 3, 3, 2, 3, 3, 2, 2, 2, 3):
        outs, _ = outputs(ofdg, n, H, W)
        g.forward_counter(first, n, *outs, ofdg.STREAM_OWN)
        res.append((outs, None))
        first += n
    return res


def script_set_step(ofdg, g, H, W):
    nc = g.num_chains()
    res = forwards(ofdg, g, nc + 1, H, W)
    g.step = 50
    res += forwards(ofdg, g, nc + 1, H, W)
    g.step = g.step          # (the same step: nothing changes)
    res += forwards(ofdg, g, 2, H, W)
    g.step = 1
    res += forwards(ofdg, g, 2, H, W)
    return res


def script_pool(ofdg, g, H, W):
    nc = g.num_chains()
    res = forwards(ofdg, g, nc + 1, H, W)
    g.pool_synthetic(*POOL, 9)   # (second halves were sampled for the old pool's textures)
    res += forwards(ofdg, g, nc + 2, H, W)
    return res


@pytest.mark.parametrize("script", [script_jump, script_batch_size, script_set_step, script_pool], ids=lambda f: f.__name__)
@pytest.mark.parametrize("W,H", SIZES)
def test_calls_the_prediction_does_not_cover(ofdg, W, H, script):
    """A second half is used only by the call it was made for: after a jump of the first index, another batch size, ofdg_set_step
    or a new pool the outputs are the unpaired context's, and no error is left behind."""
    g2, g1, _ = both(ofdg, W, H, 5, 1)
    got, want = script(ofdg, g2, H, W), script(ofdg, g1, H, W)
    g2.synchronize()
    g1.synchronize()
    assert_same(got, want)
    g2.close()
    g1.close()


def test_sharded_sequence(ofdg):
    """rank 1 of 2 (one process, no communicator): the sequence's stride is 2 x batch, which is what the second halves are
    sampled for."""
    W, H = SIZES[0]
    g2, g1, _ = both(ofdg, W, H, 7, 1, rank=1, world_size=2)
    nc = g2.num_chains()
    assert_same(forwards(ofdg, g2, 2 * nc, H, W), forwards(ofdg, g1, 2 * nc, H, W))
    assert g2.step == 2 * nc
    g2.close()
    g1.close()


@pytest.mark.parametrize("prep", [0, 1])
def test_callers_stream_and_tickets(ofdg, prep):
    """The calls on a stream that is not the context's own: compose runs there behind the hand-over event, which a second half
    records behind ITS preparation.  Every batch has a ticket of its own, and each ticket's error word reads clean."""
    import torch
    W, H = SIZES[1]
    g2, g1, _ = both(ofdg, W, H, 5, prep)
    nc = g2.num_chains()
    s = torch.cuda.Stream()
    got, tickets = [], []
    for _ in range(2 * nc + 1):
        outs, _ = outputs(ofdg, B, H, W)
        g2.forward(*outs, s.cuda_stream)
        tickets.append(g2.last_ticket())
        got.append((outs, None))
    g2.synchronize(s.cuda_stream)
    want = forwards(ofdg, g1, 2 * nc + 1, H, W, stream=s.cuda_stream)
    assert_same(got, want)
    assert len(set(tickets)) == len(tickets)
    for t in tickets:
        g2.poll_errors_of(t)   # (raises unless clean)
    g2.synchronize()
    g2.close()
    g1.close()
