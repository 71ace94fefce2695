"""Host-side logic of the compact output formats (uint8 frames, fp16 flow; ofdg_out_format in include/ofdg.h): buffer
allocation, the dtype -> format helper and the header / ctypes agreement.  No GPU needed."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    return open(os.path.join(ROOT, "include", "ofdg.h")).read()


def test_alloc_outputs_in_the_compact_formats(ofdg):
    import torch
    i0, i1, fl = ofdg.alloc_outputs(3, 24, 40, device="cpu", image_dtype=torch.uint8, flow_dtype=torch.float16)
    assert i0.dtype == i1.dtype == torch.uint8 and fl.dtype == torch.float16
    assert tuple(i0.shape) == tuple(i1.shape) == (3, 3, 24, 40) and tuple(fl.shape) == (3, 2, 24, 40)
    # the default stays float32
    assert all(t.dtype == torch.float32 for t in ofdg.alloc_outputs(1, 8, 8, device="cpu"))
    with pytest.raises(ValueError):
        ofdg.alloc_outputs(1, 8, 8, device="cpu", image_dtype=torch.int8)
    with pytest.raises(ValueError):
        ofdg.alloc_outputs(1, 8, 8, device="cpu", flow_dtype=torch.bfloat16)


def test_output_format_codes_of_the_valid_combinations(ofdg):
    import torch
    n, H, W = 2, 16, 24
    for idt, icode in ((torch.float32, ofdg.FMT_F32), (torch.uint8, ofdg.FMT_U8)):
        for fdt, fcode in ((torch.float32, ofdg.FMT_F32), (torch.float16, ofdg.FMT_F16)):
            outs = ofdg.alloc_outputs(n, H, W, device="cpu", image_dtype=idt, flow_dtype=fdt)
            assert ofdg.output_format(*outs, n, H, W) == (icode, fcode)
    assert (ofdg.FMT_F32, ofdg.FMT_U8, ofdg.FMT_F16) == (0, 1, 2)


def test_output_format_rejects_what_the_library_cannot_write(ofdg):
    import torch
    n, H, W = 2, 16, 24
    f32 = ofdg.alloc_outputs(n, H, W, device="cpu")
    u8 = ofdg.alloc_outputs(n, H, W, device="cpu", image_dtype=torch.uint8, flow_dtype=torch.float16)
    with pytest.raises(ValueError):  # frames of two dtypes
        ofdg.output_format(u8[0], f32[1], f32[2], n, H, W)
    with pytest.raises(ValueError):  # int8 frames
        ofdg.output_format(u8[0].to(torch.int8), u8[1].to(torch.int8), f32[2], n, H, W)
    with pytest.raises(ValueError):  # bfloat16 flow
        ofdg.output_format(f32[0], f32[1], f32[2].to(torch.bfloat16), n, H, W)
    with pytest.raises(ValueError):  # uint8 as flow, float16 as frames
        ofdg.output_format(f32[0], f32[1], u8[0], n, H, W)
    with pytest.raises(ValueError):
        ofdg.output_format(u8[2], u8[2], f32[2], n, H, W)
    # one element short, each of the three
    for k, ch in ((0, 3), (1, 3), (2, 2)):
        for outs in (f32, u8):
            short = list(outs)
            short[k] = outs[k].flatten()[: n * ch * H * W - 1]
            with pytest.raises(ValueError):
                ofdg.output_format(*short, n, H, W)
    # a larger buffer is fine (a ring slot cut out of a bigger allocation)
    assert ofdg.output_format(*u8, n - 1, H, W) == (ofdg.FMT_U8, ofdg.FMT_F16)


def test_header_declares_the_format_interface(ofdg):
    hdr = header()
    for name, value in (("OFDG_FMT_F32", 0), ("OFDG_FMT_U8", 1), ("OFDG_FMT_F16", 2)):
        m = re.search(r"#define\s+%s\s+(\d+)" % name, hdr)
        assert m and int(m.group(1)) == value, name
    for fn in ("ofdg_render_fmt", "ofdg_forward_fmt", "ofdg_forward_counter_fmt"):
        assert re.search(r"\bint\s+%s\s*\(" % fn, hdr), fn
        assert fn in ofdg.EXPORTS
        assert hasattr(ofdg.lib(), fn)
    m = re.search(r"typedef struct ofdg_out_format \{([^}]*)\} ofdg_out_format;", hdr)
    assert m
    fields = [f.strip() for f in m.group(1).split(";") if f.strip()]
    assert fields == ["int32_t image", "int32_t flow", "int32_t reserved[2]"]
    assert C.sizeof(ofdg.OutFormat) == 16
    assert [(n, C.sizeof(t)) for n, t in ofdg.OutFormat._fields_] == [("image", 4), ("flow", 4), ("reserved", 8)]
    assert ofdg.OutFormat.image.offset == 0 and ofdg.OutFormat.flow.offset == 4 and ofdg.OutFormat.reserved.offset == 8
    # the format belongs to the call: ofdg_params keeps its size
    assert C.sizeof(ofdg.Params) == 4 * 24
