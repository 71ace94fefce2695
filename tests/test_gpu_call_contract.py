"""GPU tests of what the twelve render / forward entry points (ofdg_render, ofdg_forward, ofdg_forward_counter; plain, _ex,
_fmt, _ex_fmt) and ofdg_render_slot / ofdg_render_resident promise about a call, through ctypes on the library itself:

  * a refused call returns OFDG_EINVAL, leaves its own text in ofdg_last_error and enqueues nothing (ofdg_last_ticket and the
    step counter stay, guard-filled outputs keep their fill);
  * every form of every family writes what the plain float32 call of its family writes, after the conversion include/ofdg.h
    documents - at a power-of-two width and at one that is none, so both kernels of every family are reached.

The expected texts are the library's as of the commit before the entry points were given one shared check (recorded from
that build); the ones marked NEW were EINVAL without a text of their own before it."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_extras_formats as xf
import test_gpu_output_formats as of
from test_gpu_extras import ALL

pytestmark = pytest.mark.gpu

H, B = 32, 2
FAMILIES = ("render", "forward", "forward_counter")
SUFFIXES = ("", "_ex", "_fmt", "_ex_fmt")
TWELVE = tuple("ofdg_" + f + s for f in FAMILIES for s in SUFFIXES)
RESIDENT = ("ofdg_render_slot", "ofdg_render_resident")
STALE = "pool_download: bad index"
MODE9 = (": backward flow, labels and occlusion are defined for the rigid modes only (mode 9: the reference's inverse branch adds "
         "the forward warp field, DG:403-406, 715-716)")


def family(entry):
    return "forward_counter" if "forward_counter" in entry else "forward" if "forward" in entry else "render"


class Ctx:
    """A generator, one sampled batch and what a raw call needs of them."""

    def __init__(self, ofdg, W, mode, sampler=0):
        self.ofdg, self.W = ofdg, W
        self.g = ofdg.Generator(ofdg.default_params(width=W, height=H, mode=mode, sampler=sampler, batch_size=B, seed=5))
        self.g.pool_synthetic(2, 2 * W, 2 * H, 11)
        self.tasks, self.bps, self.n_bps = (None, None, 0) if sampler else self.g.sample(B)
        if not sampler:
            self.g.step = 0   # (forward draws the batch that sample() just drew)

    def call(self, entry, outs, ex=None, fmt=None, n_tasks=B, slot=0):
        """entry(ctx, <its leading arguments>, outs..., [ex], [fmt], stream 0) -> return code.  outs: three pointers or None;
        ex: an Extras / ExtrasFmt or None; fmt: an OutFormat or None."""
        lead = {"render": (C.cast(self.tasks, C.c_void_p), n_tasks, C.cast(self.bps, C.c_void_p), self.n_bps) if self.tasks else (),
                "forward": (), "forward_counter": (0, B)}[family(entry)]
        if entry == "ofdg_render_slot":
            lead = (slot,)
        elif entry == "ofdg_render_resident":
            lead = ()
        tail = ()
        if entry.endswith("_ex") or entry.endswith("_ex_fmt"):
            tail += (C.byref(ex) if ex is not None else None,)
        if entry.endswith("_fmt"):
            tail += (C.byref(fmt) if fmt is not None else None,)
        return getattr(self.ofdg.lib(), entry)(self.g.h, *lead, *outs, *tail, None)

    def error(self):
        return self.ofdg.lib().ofdg_last_error(self.g.h).decode()

    def make_stale(self):
        """Leave another call's text in ofdg_last_error (host only: the index is refused before anything else happens)."""
        buf = (C.c_uint8 * 4)()
        assert self.ofdg.lib().ofdg_pool_download(self.g.h, -1, C.cast(buf, C.c_void_p)) == self.ofdg.ETEXTURES
        assert self.error() == STALE


def ptrs(tensors):
    return tuple(t.data_ptr() for t in tensors)


def extras_struct(ofdg, entry, ex_tensors, occ=None):
    """The Extras (ofdg_*_ex) or ExtrasFmt (ofdg_*_ex_fmt) of a dict of tensors."""
    ex = ofdg.ExtrasFmt(occ=ofdg.FMT_F32 if occ is None else occ) if entry.endswith("_ex_fmt") else ofdg.Extras()
    for name, t in ex_tensors.items():
        setattr(ex, name, t.data_ptr())
    return ex


# ---- 1. refused calls -------------------------------------------------------------------------------------------------
# (context, entry point, what is wrong with the call, the text it leaves) - the texts as the build of the parent commit gave them
# for these very calls; "NEW": that build returned OFDG_EINVAL and left the text of an earlier call in place
REFUSALS = [
    ("rigid", "ofdg_render", "null output", "ofdg_render: invalid argument"),
    ("rigid", "ofdg_render_ex", "null output", "ofdg_render: invalid argument"),
    ("rigid", "ofdg_render_fmt", "null output", "ofdg_render_fmt: invalid argument"),
    ("rigid", "ofdg_render_ex_fmt", "null output", "ofdg_render_ex_fmt: invalid argument"),
    ("rigid", "ofdg_forward", "null output", "ofdg_render: invalid argument"),
    ("rigid", "ofdg_forward_ex", "null output", "ofdg_render: invalid argument"),
    ("rigid", "ofdg_forward_fmt", "null output", "ofdg_render: invalid argument"),
    ("rigid", "ofdg_forward_ex_fmt", "null output", "ofdg_render: invalid argument"),
    ("rigid", "ofdg_forward_counter", "null output", "ofdg_forward_counter: invalid argument"),   # NEW
    ("rigid", "ofdg_forward_counter_ex", "null output", "ofdg_forward_counter_ex: invalid argument"),   # NEW
    ("rigid", "ofdg_forward_counter_fmt", "null output", "ofdg_forward_counter_fmt: invalid argument"),   # NEW
    ("rigid", "ofdg_forward_counter_ex_fmt", "null output", "ofdg_forward_counter_ex_fmt: invalid argument"),   # NEW
    ("rigid", "ofdg_render_slot", "null output", "ofdg_render_slot: invalid argument"),   # NEW
    ("rigid", "ofdg_render_resident", "null output", "ofdg_render_resident: invalid argument"),   # NEW
    ("counter", "ofdg_forward", "null output", "ofdg_forward: invalid argument"),   # NEW
    ("counter", "ofdg_forward_ex", "null output", "ofdg_forward_ex: invalid argument"),   # NEW
    ("counter", "ofdg_forward_fmt", "null output", "ofdg_forward_fmt: invalid argument"),   # NEW
    ("counter", "ofdg_forward_ex_fmt", "null output", "ofdg_forward_ex_fmt: invalid argument"),   # NEW
    ("rigid", "ofdg_render", "n_tasks = 0", "ofdg_render: invalid argument"),
    ("rigid", "ofdg_render_ex", "n_tasks = 0", "ofdg_render: invalid argument"),
    ("rigid", "ofdg_render_fmt", "n_tasks = 0", "ofdg_render_fmt: invalid argument"),
    ("rigid", "ofdg_render_ex_fmt", "n_tasks = 0", "ofdg_render_ex_fmt: invalid argument"),
    ("rigid", "ofdg_render_fmt", "image code", "ofdg_render_fmt: ofdg_out_format.image = 7 (valid: OFDG_FMT_F32, OFDG_FMT_U8)"),
    ("rigid", "ofdg_render_fmt", "reserved", "ofdg_render_fmt: ofdg_out_format.reserved[1] = 3 (valid: 0)"),
    ("rigid", "ofdg_render_ex_fmt", "image code", "ofdg_render_ex_fmt: ofdg_out_format.image = 7 (valid: OFDG_FMT_F32, OFDG_FMT_U8)"),
    ("rigid", "ofdg_render_ex_fmt", "reserved", "ofdg_render_ex_fmt: ofdg_out_format.reserved[1] = 3 (valid: 0)"),
    ("rigid", "ofdg_forward_fmt", "image code", "ofdg_forward_fmt: ofdg_out_format.image = 7 (valid: OFDG_FMT_F32, OFDG_FMT_U8)"),
    ("rigid", "ofdg_forward_fmt", "reserved", "ofdg_forward_fmt: ofdg_out_format.reserved[1] = 3 (valid: 0)"),
    ("rigid", "ofdg_forward_ex_fmt", "image code", "ofdg_forward_ex_fmt: ofdg_out_format.image = 7 (valid: OFDG_FMT_F32, OFDG_FMT_U8)"),
    ("rigid", "ofdg_forward_ex_fmt", "reserved", "ofdg_forward_ex_fmt: ofdg_out_format.reserved[1] = 3 (valid: 0)"),
    ("rigid", "ofdg_forward_counter_fmt", "image code", "ofdg_forward_counter_fmt: ofdg_out_format.image = 7 (valid: OFDG_FMT_F32, OFDG_FMT_U8)"),
    ("rigid", "ofdg_forward_counter_fmt", "reserved", "ofdg_forward_counter_fmt: ofdg_out_format.reserved[1] = 3 (valid: 0)"),
    ("rigid", "ofdg_forward_counter_ex_fmt", "image code", "ofdg_forward_counter_ex_fmt: ofdg_out_format.image = 7 (valid: OFDG_FMT_F32, OFDG_FMT_U8)"),
    ("rigid", "ofdg_forward_counter_ex_fmt", "reserved", "ofdg_forward_counter_ex_fmt: ofdg_out_format.reserved[1] = 3 (valid: 0)"),
    ("rigid", "ofdg_render_ex_fmt", "occ code", "ofdg_render_ex_fmt: ofdg_extras_fmt.occ = 2 (valid: OFDG_FMT_F32, OFDG_FMT_U8)"),
    ("rigid", "ofdg_forward_ex_fmt", "occ code", "ofdg_forward_ex_fmt: ofdg_extras_fmt.occ = 2 (valid: OFDG_FMT_F32, OFDG_FMT_U8)"),
    ("rigid", "ofdg_forward_counter_ex_fmt", "occ code", "ofdg_forward_counter_ex_fmt: ofdg_extras_fmt.occ = 2 (valid: OFDG_FMT_F32, OFDG_FMT_U8)"),
    ("deform", "ofdg_render_ex", "extras in mode 9", "ofdg_render_ex" + MODE9),
    ("deform", "ofdg_render_ex_fmt", "extras in mode 9", "ofdg_render_ex_fmt" + MODE9),
    ("deform", "ofdg_forward_ex", "extras in mode 9", "ofdg_forward_ex" + MODE9),
    ("deform", "ofdg_forward_ex_fmt", "extras in mode 9", "ofdg_forward_ex_fmt" + MODE9),
    ("deform", "ofdg_forward_counter_ex", "extras in mode 9", "ofdg_forward_counter_ex" + MODE9),
    ("deform", "ofdg_forward_counter_ex_fmt", "extras in mode 9", "ofdg_forward_counter_ex_fmt" + MODE9),
]


def what_is_wrong(ofdg, what, key):
    """The keyword arguments of run_refusal that make the call wrong in this way."""
    F = ofdg.OutFormat
    return {"null output": dict(null=2 if key == "counter" else 1),
            "n_tasks = 0": dict(n_tasks=0),
            "image code": dict(fmt=F(7, ofdg.FMT_F32)),
            "reserved": dict(fmt=F(ofdg.FMT_U8, ofdg.FMT_F16, (0, 3))),
            "occ code": dict(occ=ofdg.FMT_F16, fmt=F(ofdg.FMT_U8, ofdg.FMT_F16)),
            "extras in mode 9": dict(extras=True)}[what]


def run_refusal(ofdg, ctx, entry, null=None, n_tasks=B, fmt=None, occ=None, extras=False):
    """One refused call on `ctx` with guard-filled float32 buffers -> (return code, text); asserts that nothing was enqueued."""
    import torch
    outs, ex_t = xf.alloc(ofdg, B, H, ctx.W, ("f32", "f32", "f32"), ALL if (extras or occ is not None) else None)
    ex = extras_struct(ofdg, entry, ex_t or {}, occ) if "_ex" in entry else None
    p = list(ptrs(outs))
    if null is not None:
        p[null] = None
    ticket, step = ctx.g.last_ticket(), ctx.g.step
    ctx.make_stale()
    rc = ctx.call(entry, p, ex=ex, fmt=fmt, n_tasks=n_tasks)
    text = ctx.error()
    assert ctx.g.last_ticket() == ticket and ctx.g.step == step
    ctx.g.synchronize()
    torch.cuda.synchronize()
    for t in list(outs) + list((ex_t or {}).values()):
        assert bool((t.view(torch.uint8) == xf.SENTINEL).all()), "%s: an output of a refused call was written" % entry
    return rc, text


@pytest.fixture(scope="module")
def contexts(ofdg):
    """rigid: mode 7, host sampler, one batch rendered (a ticket to keep, a resident batch for ofdg_render_resident, slot 0
    uploaded); counter: the same with the device sampler; deform: mode 9, where the optional outputs are refused."""
    rigid = Ctx(ofdg, 64, 7)
    outs = of.alloc(ofdg, B, H, 64)
    rigid.g.render(rigid.tasks, B, rigid.bps, rigid.n_bps, *outs)
    rigid.g.upload_slot(0, rigid.tasks, B, rigid.bps, rigid.n_bps)
    rigid.g.synchronize()
    return {"rigid": rigid, "counter": Ctx(ofdg, 64, 7, sampler=1), "deform": Ctx(ofdg, 64, 9)}


def test_the_refusals_are_the_cases_asked_for():
    assert len(REFUSALS) == 14 + 4 + 4 + 12 + 3 + 6 and len(set(r[:3] for r in REFUSALS)) == len(REFUSALS)


@pytest.mark.parametrize("key,entry,what,text", REFUSALS, ids=["%s-%s-%s" % r[:3] for r in REFUSALS])
def test_refused_call_says_why_and_enqueues_nothing(ofdg, contexts, key, entry, what, text):
    rc, got = run_refusal(ofdg, contexts[key], entry, **what_is_wrong(ofdg, what, key))
    assert (rc, got) == (ofdg.EINVAL, text)


# ---- 2. every family in every form against its plain call ----------------------------------------------------------------
def run_form(ofdg, ctx, entry):
    """One call of `entry` in the most compact form it takes -> ((outs, extras) on the host, form)."""
    import torch
    compact = entry.endswith("_fmt")
    with_ex = "_ex" in entry
    form = xf.COMPACT if entry.endswith("_ex_fmt") else ("u8", "f16", "f32") if compact else ("f32", "f32", "f32")
    outs, ex_t = xf.alloc(ofdg, B, H, ctx.W, form, ALL if with_ex else None)
    ex = extras_struct(ofdg, entry, ex_t, ofdg.FMT_U8) if with_ex else None
    fmt = ofdg.OutFormat(ofdg.FMT_U8, ofdg.FMT_F16) if compact else None
    if family(entry) == "forward":
        ctx.g.step = 0
    assert ctx.call(entry, ptrs(outs), ex=ex, fmt=fmt) == ofdg.OK, ctx.error()
    ctx.g.synchronize()
    torch.cuda.synchronize()
    return xf.host(outs, ex_t), form


@pytest.mark.parametrize("W", [64, 72])
def test_every_family_and_form_writes_what_its_plain_call_writes(ofdg, W):
    host, counter = Ctx(ofdg, W, 7), Ctx(ofdg, W, 7, sampler=1)
    plains = {}
    for fam in FAMILIES:
        ctx = counter if fam == "forward_counter" else host
        (plain, _), _ = run_form(ofdg, ctx, "ofdg_" + fam)
        assert np.abs(plain[2]).max() > 0 and plain[0].max() > 0
        plains[fam] = plain
        ref, _ = run_form(ofdg, ctx, "ofdg_" + fam + "_ex")   # the float32 optional outputs: what _ex_fmt is defined by
        assert of.same_bytes(plain, ref[0]), fam + "_ex"
        assert ref[1]["occ0"].max() == 1 and ref[1]["label0"].max() >= 1
        got, form = run_form(ofdg, ctx, "ofdg_" + fam + "_fmt")
        of.check_form(plain, got[0], form[:2], fam + "_fmt")
        got, form = run_form(ofdg, ctx, "ofdg_" + fam + "_ex_fmt")
        xf.check_form(ref, got, form, fam + "_ex_fmt")
    # the host sampler's first batch, rendered from sample() and drawn by forward(): one batch
    assert of.same_bytes(plains["render"], plains["forward"])
