"""The op shims' one argument check (ops/_common.gpu_tensor), the checks built on it (gpu_rows, require_gpu) and the
modules' local wrappers with texts of their own, branch by branch: the messages a caller receives, the order of the
checks, and a non-contiguous tensor coming back contiguous (or, with contiguous=False, as it came).  nchw_pitch on the
three kinds of [B, C, H, W] view.  No kernel of the library is launched: every call stops in the shim."""
import math

import pytest
import torch

from paddle3d_amd.ops import _common, caddn, dd3d, iassd, ms_deform_attn, pvrcnn, smoke

pytestmark = pytest.mark.gpu
two_gpus = pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs a second GPU")


def dev(i=0):
    return torch.device("cuda", i)


def f32(*shape, i=0, dtype=torch.float32):
    return torch.arange(math.prod(shape), device=dev(i)).reshape(shape).to(dtype)


def refused(text, fn, *args, **kw):
    with pytest.raises(RuntimeError) as e:
        fn(*args, **kw)
    assert str(e.value) == text


def test_gpu_tensor_dtype_shape_and_order():
    g = _common.gpu_tensor
    refused("Unsupported device type for op operator.", g, "op", "x", torch.zeros(2, 3))
    refused("Unsupported device type for op operator.", g, "op", "x", [[0.0]])
    refused("op: x must be torch.float32, got torch.float16", g, "op", "x", f32(2, 3, dtype=torch.float16))
    refused("op: x must be torch.int32, got torch.float32", g, "op", "x", f32(2, 3), torch.int32)
    refused("op: x must be (3, 2), got (2, 3)", g, "op", "x", f32(2, 3), shape=(3, 2))
    refused("op: x must be (3, 2), got (2, 3)", g, "op", "x", f32(2, 3), shape=[3, 2])
    # the dtype is checked before the shape; dtype=None takes any
    refused("op: x must be torch.float32, got torch.int64", g, "op", "x", f32(2, 3, dtype=torch.int64), shape=(3, 2))
    t = f32(2, 3, dtype=torch.int64)
    assert g("op", "x", t, dtype=None, dev=dev(), shape=(2, 3)) is t


def test_gpu_tensor_contiguity():
    g = _common.gpu_tensor
    t = f32(3, 2).t()
    assert not t.is_contiguous()
    out = g("op", "x", t, shape=(2, 3))
    assert out.is_contiguous() and out.data_ptr() != t.data_ptr() and torch.equal(out, t)
    assert g("op", "x", t, contiguous=False) is t
    c = f32(2, 3)
    assert g("op", "x", c) is c


@two_gpus
def test_gpu_tensor_device_index():
    g = _common.gpu_tensor
    refused("op: x is on cuda:1, expected cuda:0", g, "op", "x", f32(2, 3, i=1), dev=dev(0))
    # after the dtype, before the shape
    refused("op: x must be torch.float32, got torch.float16", g, "op", "x", f32(2, 3, i=1, dtype=torch.float16),
            dev=dev(0))
    refused("op: x is on cuda:1, expected cuda:0", g, "op", "x", f32(2, 3, i=1), dev=dev(0), shape=(3, 2))
    refused("smoke: reg_feat is on cuda:1, expected cuda:0", smoke._strided, "reg_feat", f32(2, 3, 4, 5, i=1), dev(0))
    refused("dd3d: box2d_feat[0] must be float32 (2, 3, 4, 5) on cuda:0, got torch.float32 (2, 3, 4, 5) on cuda:1",
            dd3d._strided, "box2d_feat[0]", f32(2, 3, 4, 5, i=1), dev(0), (2, 3, 4, 5))


def test_gpu_rows_and_require_gpu():
    r = _common.gpu_rows
    refused("Unsupported device type for op operator.", r, "op", "x", torch.zeros(2, 3), 3)
    refused("op: x must be torch.int32, got torch.float32", r, "op", "x", f32(2, 4), 4, torch.int32)
    refused("op: x must be [rows, 3], got (2, 4)", r, "op", "x", f32(2, 4), 3)
    refused("op: x must be [rows, C], got (2, 4, 1)", r, "op", "x", f32(2, 4, 1), None)
    t = f32(4, 2).t()
    out = r("op", "x", t, None)
    assert out.is_contiguous() and torch.equal(out, t)
    q = _common.require_gpu
    refused("Unsupported device type for op operator.", q, torch.zeros(2, 3), "op")
    refused("op: expected torch.float32, got torch.float16", q, f32(2, 3, dtype=torch.float16), "op")
    refused("op: expected torch.int32, got torch.float32", q, f32(2, 3), "op", torch.int32)
    out = q(t, "op")
    assert out.is_contiguous() and torch.equal(out, t)
    refused("op: x must be [4], got (3,)", pvrcnn._vec, f32(3), "op", "x", 4)
    refused("op: x must be torch.float32, got torch.int32", pvrcnn._vec, f32(4, dtype=torch.int32), "op", "x", 4)


@pytest.mark.parametrize("shaped,dtype_text", [(caddn._shaped, "float32"), (iassd._shaped, "torch.float32")],
                         ids=["caddn", "iassd"])
def test_wildcard_shapes(shaped, dtype_text):
    refused("Unsupported device type for op operator.", shaped, torch.zeros(2, 4, 4), "op", "x", (None, 4, 4))
    refused(f"op: x must be {dtype_text}, got torch.float16", shaped, f32(2, 4, 4, dtype=torch.float16), "op", "x",
            (None, 4, 4))
    refused("op: x must be [None, 4, 4], got (2, 3, 4)", shaped, f32(2, 3, 4), "op", "x", (None, 4, 4))
    refused("op: x must be [None, 4, 4], got (4, 4)", shaped, f32(4, 4), "op", "x", (None, 4, 4))
    refused("op: x must be [2, 3], got (3, 3)", shaped, f32(3, 3), "op", "x", (2, 3))
    t = f32(2, 4, 4).transpose(1, 2)
    out = shaped(t, "op", "x", (None, 4, 4))
    assert not t.is_contiguous() and out.is_contiguous() and torch.equal(out, t)


def test_strided_wrappers():
    refused("Unsupported device type for smoke operator.", smoke._strided, "cls_feat", torch.zeros(2, 3, 4, 5), None)
    refused("smoke: cls_feat must be float32 [B, C, H, W], got torch.float16 (2, 3, 4, 5)", smoke._strided, "cls_feat",
            f32(2, 3, 4, 5, dtype=torch.float16), None)
    refused("smoke: cls_feat must be float32 [B, C, H, W], got torch.float32 (3, 4, 5)", smoke._strided, "cls_feat",
            f32(3, 4, 5), None)
    refused("Unsupported device type for dd3d operator.", dd3d._strided, "box2d_feat[0]", torch.zeros(2, 3, 4, 5),
            dev(), (2, 3, 4, 5))
    refused("dd3d: box2d_feat[0] must be float32 (2, 3, 4, 5) on cuda:0, got torch.float16 (2, 3, 4, 5) on cuda:0",
            dd3d._strided, "box2d_feat[0]", f32(2, 3, 4, 5, dtype=torch.float16), dev(), (2, 3, 4, 5))
    refused("dd3d: box2d_feat[0] must be float32 (2, 3, 4, 5) on cuda:0, got torch.float32 (2, 3, 5, 4) on cuda:0",
            dd3d._strided, "box2d_feat[0]", f32(2, 3, 5, 4), dev(), (2, 3, 4, 5))
    x = f32(2, 3, 4, 5).contiguous(memory_format=torch.channels_last)
    for out, sb, pitch in (smoke._strided("cls_feat", x, dev()),
                           dd3d._strided("box2d_feat[0]", x, dev(), (2, 3, 4, 5))):
        assert out.is_contiguous() and torch.equal(out, x) and (sb, pitch) == (60, 5)


def test_ms_deform_attn_int64_texts():
    value, loc, w = f32(1, 6, 2, 4), f32(1, 3, 2, 1, 2, 2), f32(1, 3, 2, 1, 2)
    shapes, start = torch.tensor([[2, 3]], device=dev()), torch.zeros(1, dtype=torch.int64, device=dev())
    refused("ms_deform_attn: spatial_shapes must be int64, got torch.int32", ms_deform_attn.ms_deform_attn, value, loc,
            w, shapes.int(), start, 1)
    refused("ms_deform_attn: level_start_index must be int64, got torch.int32", ms_deform_attn.ms_deform_attn, value,
            loc, w, shapes, start.int(), 1)
    refused("ms_deform_attn: attention_weights must have value's dtype torch.float32, got torch.float64",
            ms_deform_attn.ms_deform_attn, value, loc, w.double(), shapes, start, 1)
    refused("ms_deform_attn: spatial_shapes must be [1, 2] and level_start_index [1], got (1, 2) and (2,)",
            ms_deform_attn.ms_deform_attn, value, loc, w, shapes, torch.zeros(2, dtype=torch.int64, device=dev()), 1)


def test_nchw_pitch():
    x = f32(2, 3, 4, 5)
    out, sb, pitch = _common.nchw_pitch(x)
    assert out is x and (sb, pitch) == (60, 5)
    padded = f32(2, 3, 4, 8)[..., :5]                   # rows of pitch 8: read in place
    out, sb, pitch = _common.nchw_pitch(padded)
    assert out is padded and (sb, pitch) == (96, 8) == (padded.stride(0), padded.stride(2))
    last = x.contiguous(memory_format=torch.channels_last)  # anything else: copied
    assert last.stride() == (60, 1, 15, 3)
    out, sb, pitch = _common.nchw_pitch(last)
    assert out.is_contiguous() and out.data_ptr() != last.data_ptr() and torch.equal(out, x) and (sb, pitch) == (60, 5)
