"""Host-side logic of the optional outputs in the compact formats (ofdg_extras_fmt, ofdg_*_ex_fmt in include/ofdg.h): the
dtype rules of the extras, their allocation, the header / ctypes agreement, and the case the GPU test of the occlusion
rounding relies on.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import extras_reference as xr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, H, W = 2, 16, 24


def header():
    return open(os.path.join(ROOT, "include", "ofdg.h")).read()


def test_alloc_extras_dtypes(ofdg):
    import torch
    ex = ofdg.alloc_extras(N, H, W, device="cpu")  # the default stays float32
    assert ex["flow1"].dtype == ex["occ0"].dtype == ex["occ1"].dtype == torch.float32
    assert ex["label0"].dtype == ex["label1"].dtype == torch.uint8
    ex = ofdg.alloc_extras(N, H, W, device="cpu", flow_dtype=torch.float16, occ_dtype=torch.uint8)
    assert ex["flow1"].dtype == torch.float16 and tuple(ex["flow1"].shape) == (N, 2, H, W)
    assert ex["occ0"].dtype == ex["occ1"].dtype == torch.uint8 and tuple(ex["occ0"].shape) == tuple(ex["occ1"].shape) == (N, 1, H, W)
    assert ex["label0"].dtype == ex["label1"].dtype == torch.uint8 and tuple(ex["label0"].shape) == (N, H, W)
    ex = ofdg.alloc_extras(N, H, W, ("occ1", "flow1"), device="cpu", occ_dtype=torch.uint8)
    assert set(ex) == {"occ1", "flow1"} and ex["occ1"].dtype == torch.uint8 and ex["flow1"].dtype == torch.float32
    with pytest.raises(ValueError):
        ofdg.alloc_extras(N, H, W, device="cpu", flow_dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        ofdg.alloc_extras(N, H, W, device="cpu", occ_dtype=torch.float16)
    with pytest.raises(ValueError):
        ofdg.alloc_extras(N, H, W, device="cpu", occ_dtype=torch.int8)


def test_extras_format_accepts_the_valid_combinations(ofdg):
    import torch
    for fdt, fcode in ((torch.float32, ofdg.FMT_F32), (torch.float16, ofdg.FMT_F16)):
        for odt, ocode in ((torch.float32, ofdg.FMT_F32), (torch.uint8, ofdg.FMT_U8)):
            ex = ofdg.alloc_extras(N, H, W, device="cpu", flow_dtype=fdt, occ_dtype=odt)
            assert ofdg.extras_format(ex, fcode, N, H, W) == ocode
            for name in ex:  # every output alone, and a None entry is "not requested"
                assert ofdg.extras_format({name: ex[name]}, fcode, N, H, W) == (ocode if name.startswith("occ") else ofdg.FMT_F32)
                assert ofdg.extras_format(dict(ex, **{name: None}), fcode, N, H, W) == ocode
    assert ofdg.extras_format({}, ofdg.FMT_F16, N, H, W) == ofdg.FMT_F32


def test_extras_format_rejects_everything_else(ofdg):
    import torch
    f32 = ofdg.alloc_extras(N, H, W, device="cpu")
    cmp_ = ofdg.alloc_extras(N, H, W, device="cpu", flow_dtype=torch.float16, occ_dtype=torch.uint8)
    bad = [
        (dict(f32), ofdg.FMT_F16),                                  # float32 flow1 beside an fp16 flow
        (dict(cmp_), ofdg.FMT_F32),                                 # fp16 flow1 beside a float32 flow
        ({"flow1": f32["flow1"].to(torch.bfloat16)}, ofdg.FMT_F16),
        ({"occ0": f32["occ0"], "occ1": cmp_["occ1"]}, ofdg.FMT_F32),  # occlusion maps of two dtypes
        ({"occ0": cmp_["occ0"], "occ1": f32["occ1"]}, ofdg.FMT_F16),
        ({"occ0": f32["occ0"].to(torch.float16)}, ofdg.FMT_F16),
        ({"occ1": f32["occ1"].to(torch.int8)}, ofdg.FMT_F32),
        ({"label0": f32["label0"].to(torch.float32)}, ofdg.FMT_F32),  # labels are uint8
        ({"label1": f32["label1"].to(torch.int8)}, ofdg.FMT_F16),
        ({"flow1": f32["flow1"][:1]}, ofdg.FMT_F32),                # a sample short
        ({"occ0": cmp_["occ0"][:, 0]}, ofdg.FMT_F32),               # [n,H,W] instead of [n,1,H,W]
        ({"label0": cmp_["occ0"]}, ofdg.FMT_F32),                   # [n,1,H,W] instead of [n,H,W]
        ({"flow2": f32["flow1"]}, ofdg.FMT_F32),                    # unknown name
    ]
    for ex, code in bad:
        with pytest.raises(ValueError):
            ofdg.extras_format(ex, code, N, H, W)


def test_header_declares_the_extras_format_interface(ofdg):
    hdr = header()
    for fn in ("ofdg_render_ex_fmt", "ofdg_forward_ex_fmt", "ofdg_forward_counter_ex_fmt"):
        assert re.search(r"\bint\s+%s\s*\(" % fn, hdr), fn
        assert fn in ofdg.EXPORTS
        assert hasattr(ofdg.lib(), fn)
    m = re.search(r"typedef struct ofdg_extras_fmt \{(.*?)\} ofdg_extras_fmt;", hdr, re.S)
    assert m
    fields = [re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", f, flags=re.S)).strip() for f in m.group(1).split(";")]
    assert [f for f in fields if f] == ["void* flow1", "void* occ0", "void* occ1", "uint8_t* label0", "uint8_t* label1", "int32_t occ",
                                        "int32_t reserved[3]"]
    assert C.sizeof(ofdg.ExtrasFmt) == 5 * 8 + 4 * 4
    assert [n for n, _ in ofdg.ExtrasFmt._fields_] == ["flow1", "occ0", "occ1", "label0", "label1", "occ", "reserved"]
    assert ofdg.ExtrasFmt.occ.offset == 40 and ofdg.ExtrasFmt.reserved.offset == 44
    # the float32 struct and the format struct keep their layouts
    assert C.sizeof(ofdg.Extras) == 40 and C.sizeof(ofdg.OutFormat) == 16
    assert "Not offered: a compact format together with the optional outputs" not in hdr


def test_flow_loader_refuses_compact_extras_without_the_switch(ofdg):
    """(argument check only: it comes before the generator is created)"""
    import torch
    with pytest.raises(ValueError):
        ofdg.FlowLoader(image_dtype=torch.uint8, extras=("flow1",))
    with pytest.raises(ValueError):
        ofdg.FlowLoader(flow_dtype=torch.float16, extras=("occ0",), extras_compact=False)


def occlusion_rounding_case(ofdg, oracle):
    """The 512x384 mode-7 sample of a fresh reference-stream sampler (what Generator.sample(1) of a fresh context draws) and
    its definitions; the pool only feeds textures, which none of these outputs depends on."""
    Wf, Hf = 512, 384
    tasks, bps, n = ofdg.HostSampler(7, Wf, Hf).next(1)
    pool = np.random.default_rng(0).integers(0, 256, (3, 3, 2 * Hf, 2 * Wf), dtype=np.uint8)
    return xr.reference_extras(ofdg, oracle, oracle.default_params(Wf, Hf, 7), tasks, 1, bps, n, pool)


def occlusion_from_fp16_flows(ref):
    """What an occlusion pass that read the STORED binary16 flows back would compute."""
    f0 = ref["flow"][0].astype(np.float16).astype(np.float32)
    f1 = ref["flow1"][0].astype(np.float16).astype(np.float32)
    return xr.occlusion(f0, ref["label0"][0], ref["label1"][0]), xr.occlusion(f1, ref["label1"][0], ref["label0"][0])


def test_occlusion_from_fp16_flows_differs_on_the_full_size_case(ofdg, oracle):
    """tests/test_gpu_extras_formats.py shows on this sample that the occlusion maps are rounded from the float32 flow: that
    needs the maps rounded from the fp16 flows to be different ones."""
    ref = occlusion_rounding_case(ofdg, oracle)
    w0, w1 = occlusion_from_fp16_flows(ref)
    assert (w0 != ref["occ0"][0]).sum() >= 1 and (w1 != ref["occ1"][0]).sum() >= 1
