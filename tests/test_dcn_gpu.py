"""pd3_deform_conv2d_forward on the GPU: bit-equal to its NumPy restatement (tests/golden/dcn_numpy.py: the gather form,
one fmaf chain over ascending j, glibc's expf) on the golden cases and on seeded sweeps at the smallest shapes that reach
each border -- outputs from 1 x 1, Wo of 15 / 16 / 17 and 63 / 64 / 65, the workgroup's 64-pixel tile and one past it
(inside an image and across two), Cin of 16 and 48, Cout of 16, 48, 256, 272 and 512, strides 1 and 2, dilation 2,
paddings 0 and 2, the mask absent, given and given as logits, scale / shift / relu each on and off, offset and mask as
views of one 27-channel map and as separate tensors with a padded pitch, and hostile data (samples at exactly -1, -0.5,
H - 1, H - 0.5 and H, offsets of 1e30, +-Inf and NaN, a NaN and an Inf pixel, an Inf weight under an out-of-range
sample, saturated mask logits).  The three launch forms (4, 2 and 1 channel tiles per wave, chosen from the pixel and
channel counts) are reached with 64 x 64 frames and held to each other with torch.equal and to the restatement on a
channel subset.  A frame gives the same bits alone, elsewhere in the batch and on a side stream.  The modules of
paddle3d_amd.mm_resnet in their three forms, the bottleneck and a two-block stage are held to the reference's golden
results within the stored bounds; a fused DCN layer is one launch, a forward makes no host synchronisation, a refused
shape falls back to the torch composition."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
from guarded import launch_ledger  # noqa: E402

import dcn_numpy as dn  # noqa: E402
import make_dcn_golden as mk  # noqa: E402
import test_dcn_cpu as cpu  # noqa: E402
from test_dcn_cpu import expf, golden  # noqa: E402,F401

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32
SYMBOL = "pd3_deform_conv2d_forward"


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(got, want):
    """Bit equality of two float32 arrays, a NaN matching any NaN (the sign and payload of a NaN are not part of the
    arithmetic the header fixes)."""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and
                np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))


def random_case(seed, N, ci, co, H, W, stride=1, padding=1, dilation=1, spread=2.0):
    """Seeded x, offset (normal * spread), mask logits, weight, scale, shift as float32 arrays."""
    rng = np.random.default_rng(seed)
    Ho, Wo = dn.output_size(H, stride, padding, dilation), dn.output_size(W, stride, padding, dilation)
    return dict(x=rng.standard_normal((N, ci, H, W)).astype(F32),
                offset=(rng.standard_normal((N, 18, Ho, Wo)) * spread).astype(F32),
                mask=rng.standard_normal((N, 9, Ho, Wo)).astype(F32),
                w=(rng.standard_normal((co, ci, 3, 3)) / np.sqrt(9 * ci)).astype(F32),
                scale=rng.uniform(0.5, 1.5, co).astype(F32), shift=rng.uniform(-0.5, 0.5, co).astype(F32),
                stride=stride, padding=padding, dilation=dilation)


def kernel(c, mask="logit", scale=True, shift=True, relu=True, w=None):
    """The entry point on case `c`; mask: None, "given" (the logits taken as the mask itself) or "logit"."""
    from paddle3d_amd.ops import deform_conv as ops

    y = ops.deform_conv2d_packed(_t(c["x"]), _t(c["offset"]), _t(c["mask"]) if mask else None,
                                 ops.pack_deform_conv_weight(_t(c["w"] if w is None else w)),
                                 _t(c["scale"]) if scale else None, _t(c["shift"]) if shift else None, relu,
                                 mask == "logit", c["stride"], c["padding"], c["dilation"])
    assert y is not None
    return y


def restated(c, expf, mask="logit", scale=True, shift=True, relu=True, w=None):  # noqa: F811
    return dn.deform_conv2d(c["x"], c["offset"], c["mask"] if mask else None, c["w"] if w is None else w,
                            c["scale"] if scale else None, c["shift"] if shift else None, relu, mask == "logit",
                            c["stride"], c["padding"], c["dilation"], expf)


@pytest.mark.parametrize("tag", list(mk.CASES))
def test_golden_cases_equal_the_restatement(golden, expf, tag):  # noqa: F811
    from paddle3d_amd.ops import deform_conv as ops

    c = mk.CASES[tag]
    x, om, w, b = cpu.case_arrays(golden, tag)
    want = cpu.restated(golden, tag, expf)
    om_d = _t(om)
    y = ops.deform_conv2d_packed(_t(x), om_d[:, :18], om_d[:, 18:], ops.pack_deform_conv_weight(_t(w)), None, _t(b),
                                 False, True, c["stride"], c["dilation"], c["dilation"])
    assert same_bits(y.cpu().numpy(), want)
    assert cpu.err(y.cpu().numpy(), golden[f"{tag}_y"]) <= float(golden[f"{tag}_y_bound"])
    if tag == "a":  # the reference op's signature: the mask as given, the bias, the weight unpacked
        mask = torch.sigmoid(om_d[:, 18:])
        y2 = ops.deform_conv2d(_t(x), om_d[:, :18], _t(w), _t(b), 1, 1, 1, 1, 1, mask)
        want2 = dn.deform_conv2d(x, om[:, :18], mask.cpu().numpy(), w, None, b, False, False, 1, 1, 1)
        assert same_bits(y2.cpu().numpy(), want2)


# (N, H, W) with padding 1, stride 1: Ho = H, Wo = W.  One pixel; Wo around 16 and around 64 (one row: 63 / 64 / 65 pixels
# are also the tile's end and one past it); 65 pixels in rows of 13; tiles that end inside the second and fourth image
SIZES = ((1, 1, 1), (1, 1, 15), (1, 1, 16), (1, 1, 17), (1, 1, 63), (1, 1, 64), (1, 1, 65), (1, 5, 13), (2, 2, 17),
         (4, 3, 7), (3, 4, 16))


@pytest.mark.parametrize("N,H,W", SIZES)
def test_output_sizes(expf, N, H, W):  # noqa: F811
    c = random_case(100 + 7 * H + W, N, 16, 16, H, W)
    assert same_bits(kernel(c).cpu().numpy(), restated(c, expf))


@pytest.mark.parametrize("ci,co", [(16, 48), (48, 16), (48, 256), (16, 272), (16, 512)])
def test_channel_counts(expf, ci, co):  # noqa: F811
    c = random_case(ci + co, 2, ci, co, 3, 11)  # 66 pixels: two tiles, the second of two pixels
    assert same_bits(kernel(c).cpu().numpy(), restated(c, expf))


@pytest.mark.parametrize("stride,padding,dilation", [(1, 0, 1), (2, 0, 1), (2, 1, 1), (2, 2, 2), (1, 2, 2), (1, 0, 2),
                                                     (2, 2, 1)])
def test_strides_paddings_dilations(expf, stride, padding, dilation):  # noqa: F811
    c = random_case(10 * stride + 3 * padding + dilation, 2, 16, 32, 9, 12, stride, padding, dilation)
    y = kernel(c)
    assert tuple(y.shape[2:]) == (dn.output_size(9, stride, padding, dilation), dn.output_size(12, stride, padding, dilation))
    assert same_bits(y.cpu().numpy(), restated(c, expf))


@pytest.mark.parametrize("mask", [None, "given", "logit"])
def test_mask_forms_and_epilogues(expf, mask):  # noqa: F811
    c = random_case(5, 2, 16, 32, 5, 9)
    for scale, shift, relu in ((False, False, False), (True, False, False), (False, True, False), (False, False, True),
                               (True, True, True)):
        got = kernel(c, mask, scale, shift, relu).cpu().numpy()
        assert same_bits(got, restated(c, expf, mask, scale, shift, relu)), (mask, scale, shift, relu)
        assert relu == bool((got >= 0).all())


def test_views_of_one_map_and_padded_pitches():
    """offset and mask as the two parts of one 27-channel map (no copy) and as separate tensors whose rows are 3 and 5
    floats longer than Wo: the same bits as from contiguous tensors."""
    from paddle3d_amd.ops import _common
    from paddle3d_amd.ops import deform_conv as ops

    c = random_case(9, 2, 16, 32, 6, 10)
    want = kernel(c)
    packed = ops.pack_deform_conv_weight(_t(c["w"]))
    args = (_t(c["scale"]), _t(c["shift"]), True, True, 1, 1, 1)
    om = torch.cat([_t(c["offset"]), _t(c["mask"])], 1)
    offset, mask = om[:, :18], om[:, 18:]
    for view in (offset, mask):
        t, sb, pitch = _common.nchw_pitch(view)
        assert t.data_ptr() == view.data_ptr() and (sb, pitch) == (27 * 60, 10) and not view.is_contiguous()
    assert torch.equal(ops.deform_conv2d_packed(_t(c["x"]), offset, mask, packed, *args), want)
    wide_o, wide_m = torch.full((2, 18, 6, 13), float("nan"), device=DEV), torch.full((3, 9, 6, 15), float("nan"), device=DEV)
    wide_o[..., :10], wide_m[1:, ..., :10] = _t(c["offset"]), _t(c["mask"])
    offset, mask = wide_o[..., :10], wide_m[1:, ..., :10]
    assert _common.nchw_pitch(offset)[0].data_ptr() == offset.data_ptr() and _common.nchw_pitch(mask)[2] == 15
    assert torch.equal(ops.deform_conv2d_packed(_t(c["x"]), offset, mask, packed, *args), want)
    # a view nchw_pitch does not take (columns strided) is copied and gives the same bits
    turned = _t(c["offset"]).permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    assert turned.stride(3) != 1 and _common.nchw_pitch(turned)[0].data_ptr() != turned.data_ptr()
    assert torch.equal(ops.deform_conv2d_packed(_t(c["x"]), turned, _t(c["mask"]), packed, *args), want)


def test_hostile_data(expf):  # noqa: F811
    """Offsets drawn from {0, +-0.5, +-1, 2.5, 1e30, +-Inf, NaN} on integer base positions: samples at exactly -1, -0.5,
    H - 1, H - 0.5 and H; a NaN and an Inf pixel; an Inf weight on a tap that is out of range for some pixels; mask
    logits at which expf overflows, underflows and is special."""
    H, W = 6, 9
    c = random_case(77, 2, 16, 32, H, W)
    rng = np.random.default_rng(78)
    values = np.array([0, 0.5, -0.5, 1, -1, 2.5, 1e30, -1e30, np.inf, -np.inf, np.nan], F32)
    c["offset"] = values[rng.integers(0, values.size, c["offset"].shape)]
    h = np.stack([np.arange(H)[None, :, None] - 1 + k // 3 + c["offset"][:, 2 * k] for k in range(9)], 1)
    for at in (-1.0, -0.5, H - 1.0, H - 0.5, float(H)):
        assert (h == at).sum() > 0, at
    c["x"][0, 3, 2, 4], c["x"][1, 5, 0, 0], c["x"][1, 7, H - 1, W - 1] = np.nan, np.inf, -np.inf
    c["w"][5, 2, 0, 0], c["w"][17, 9, 2, 2] = np.inf, -np.inf  # taps 0 and 8 are out of range at the image's corners
    logits = np.array([200, -200, 88.5, -88.5, 104, -104, 89, -150, np.inf, -np.inf, np.nan, 0, 1, -1], F32)
    c["mask"] = logits[rng.integers(0, logits.size, c["mask"].shape)]
    for mask in (None, "given", "logit"):
        got, want = kernel(c, mask).cpu().numpy(), restated(c, expf, mask)
        assert same_bits(got, want), mask
        assert np.isnan(want).any() and np.isfinite(want).any()
    # an Inf weight under a sample that is out of range everywhere: fmaf(+0, Inf, .) is a NaN for every pixel of channel 5
    c2 = random_case(79, 1, 16, 16, 4, 4)
    c2["offset"][:, 0] = 1e30
    c2["w"][5, 0, 0, 0] = np.inf
    got = kernel(c2, None, False, False, False).cpu().numpy()
    assert same_bits(got, restated(c2, expf, None, False, False, False))
    assert np.isnan(got[:, 5]).all() and np.isfinite(np.delete(got, 5, 1)).all()


def test_three_launch_forms_agree(expf):  # noqa: F811
    """64 x 64 frames, Cout = 512 and 272: four, two (three for 272) and one frame launch the forms with 4, 2 and 1 channel
    tiles per wave (ops.tiles_per_wave restates the choice).  Every frame's output is the same bits in each, and equal
    to the restatement on 16 channels from both ends of the channel range and from both sides of 256."""
    from paddle3d_amd.ops import deform_conv as ops

    for co, frames in ((512, (4, 2, 1)), (272, (4, 3, 1))):
        c = random_case(co, 4, 16, co, 64, 64)
        assert [ops.tiles_per_wave(n * 4096, co) for n in frames] == [4, 2, 1]
        packed = ops.pack_deform_conv_weight(_t(c["w"]))
        x, offset, mask, scale, shift = (_t(c[k]) for k in ("x", "offset", "mask", "scale", "shift"))
        run = lambda lo, hi: ops.deform_conv2d_packed(x[lo:hi], offset[lo:hi], mask[lo:hi], packed, scale, shift, True,  # noqa: E731
                                                      True, 1, 1, 1)
        full = run(0, 4)
        assert torch.equal(run(4 - frames[1], 4), full[4 - frames[1]:])
        for i in range(4):
            assert torch.equal(run(i, i + 1), full[i:i + 1])
        sel = np.array([0, 1, 15, 16, 127, 128, 254, 255, 256, 257, 263, 264, 270, 271] +
                       ([510, 511] if co == 512 else [200, 201]))
        one = {k: (v[3:4] if k in ("x", "offset", "mask") else v) for k, v in c.items()}
        one.update(w=c["w"][sel], scale=c["scale"][sel], shift=c["shift"][sel])
        assert same_bits(full[3:4, sel].cpu().numpy(), restated(one, expf))


def test_frame_alone_in_a_batch_and_on_a_side_stream():
    c = random_case(31, 3, 48, 48, 5, 9)  # 45 pixels a frame: the tiles end inside the second and third frame
    full = kernel(c)
    for i in range(3):
        one = {k: (v[i:i + 1] if k in ("x", "offset", "mask") else v) for k, v in c.items()}
        assert torch.equal(kernel(one), full[i:i + 1])
    moved = {k: (v[[2, 0, 1]] if k in ("x", "offset", "mask") else v) for k, v in c.items()}
    assert torch.equal(kernel(moved), full[[2, 0, 1]])
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        again = kernel(c)
    side.synchronize()
    assert torch.equal(again, full)


@pytest.mark.parametrize("tag", [*mk.CASES, *mk.BLOCKS, *mk.STAGE])
def test_modules_in_three_forms_against_the_reference(golden, tag):  # noqa: F811
    """fused="force", the default and the torch composition within the stored bounds; the forced form launches the
    kernel once per DCN layer, the unfused form never."""
    from paddle3d_amd import _lib

    x = _t(mk.inputs(tag))
    layers = 1 if tag in mk.CASES or tag in mk.BLOCKS else 2
    for fused, launches in (("force", layers), (True, None), (False, 0)):
        m = cpu.build(golden, tag, fused).to(DEV)
        with torch.no_grad(), launch_ledger(_lib.lib(), (SYMBOL,)) as n:
            y = m(x)
        assert launches is None or n[SYMBOL] == launches, (fused, dict(n))
        assert tuple(y.shape) == golden[f"{tag}_y"].shape
        assert cpu.err(y.cpu().numpy(), golden[f"{tag}_y"]) <= float(golden[f"{tag}_y_bound"]), fused


def test_default_takes_the_kernel_from_its_measured_border(golden):  # noqa: F811
    from paddle3d_amd import _lib
    from paddle3d_amd.ops import deform_conv as ops

    m = cpu.build(golden, "a", True).to(DEV)
    x = _t(mk.inputs("a"))
    with torch.no_grad(), launch_ledger(_lib.lib(), (SYMBOL,)) as n:
        m(x)
    assert n[SYMBOL] == int(ops.fused_by_default(16, 16, 2 * 5 * 7)) == int(m.takes_kernel(x))
    assert not m.takes_kernel(x.cpu()) and not m.takes_kernel(x.double())


def test_no_host_synchronisation_and_one_launch_per_layer(golden):  # noqa: F811
    from paddle3d_amd import _lib

    stage = cpu.build(golden, "s", "force").to(DEV)
    x = _t(mk.inputs("s"))
    with torch.no_grad():
        stage(x)  # folds and packs once
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.no_grad(), launch_ledger(_lib.lib(), (SYMBOL,)) as n:
            y = stage(x)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert n[SYMBOL] == 2
    assert cpu.err(y.cpu().numpy(), golden["s_y"]) <= float(golden["s_y_bound"])


def test_refused_shapes_fall_back(golden):  # noqa: F811
    """24 channels: the op returns None, the reference-signature op raises, the forced module runs the composition."""
    from paddle3d_amd import _lib, mm_resnet as mr
    from paddle3d_amd.ops import deform_conv as ops

    rng = np.random.default_rng(3)
    x = _t(rng.standard_normal((1, 24, 5, 6)).astype(F32))
    m = mr.DeformableConvV2(24, 24, 3, padding=1, fused="force").to(DEV).eval()
    with torch.no_grad():
        m.conv_offset.weight.copy_(_t((rng.standard_normal((27, 24, 3, 3)) * 0.2).astype(F32)))
        with launch_ledger(_lib.lib(), (SYMBOL,)) as n:
            y = m(x)
        assert n[SYMBOL] == 0 and not m.takes_kernel(x)
        om = m.conv_offset(x)
        want = mr.deform_conv2d_composition(x, om[:, :18], torch.sigmoid(om[:, 18:]), m.conv_dcn.weight, m.conv_dcn.bias,
                                            1, 1, 1)
    assert torch.equal(y, want) and bool(om[:, :18].any())  # the same operators on the same inputs
    assert ops.deform_conv2d_packed(_t(np.zeros((1, 16, 2, 2), F32)), _t(np.zeros((1, 18, 1, 1), F32)), None,
                                    ops.pack_deform_conv_weight(_t(np.zeros((16, 16, 3, 3), F32))), stride=3) is None
    with pytest.raises(RuntimeError, match="unsupported configuration"):
        ops.deform_conv2d(x, om[:, :18], m.conv_dcn.weight, padding=1)
    with pytest.raises(RuntimeError):  # an offset map of the wrong size
        ops.deform_conv2d_packed(_t(np.zeros((1, 16, 4, 4), F32)), _t(np.zeros((1, 18, 4, 5), F32)), None,
                                 ops.pack_deform_conv_weight(_t(np.zeros((16, 16, 3, 3), F32))), padding=1)
